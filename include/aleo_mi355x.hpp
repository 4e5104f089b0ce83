// aleo_mi355x.hpp — C++ host-side mirror of the snarkVM operator interfaces, over the C ABI in aleo_mi355x.h.
//
// The reference's host code is Rust (snarkVM 0.14.5 behind /root/reference/rust/src/program/execute.rs:74); there is no
// Rust toolchain in the build image, so the host side above the C ABI is this header.  Names, argument meaning and
// error behaviour follow the reference interfaces [UPSTREAM-RECALL]:
//   snarkvm_algorithms::msm::VariableBase::msm(bases, scalars) -> Projective        (zips to the shorter slice)
//   snarkvm_algorithms::fft::EvaluationDomain::{new, fft_in_place, ifft_in_place, coset_fft_in_place, coset_ifft_in_place}
//   snarkvm_algorithms::polycommit::kzg10::KZG10::commit(powers, polynomial) -> Commitment (G1Affine); the commitments of one
//       prover round (SonicKZG10::commit over several labelled polynomials) as ONE call; CanonicalSerialize (compressed) of it
//   snarkvm_algorithms_cuda::{msm, NTT}: Result<_, Error> — an Err means "recompute on the CPU"
//   snarkvm_synthesizer_snark::ProvingKey::prove_batch / snarkvm_algorithms::snark::varuna::{CircuitProvingKey, Proof}: a proving key bound
//       to one circuit, `prove_batch(&[assignment])` -> Proof, Proof Display as bech32m `proof1…`; `prove_batch(keys -> assignments)` over several
//       keys and `Trace::prove_execution / prove_fee` above it (rows a6 / a7 of SURVEY.md §8)
//   snarkvm_console_program::Record<N, Ciphertext<N>>::{from_str, is_owner, decrypt} and the record search around it (RecordCiphertext, RecordPlaintext,
//   find_owned, find_owned_many, decrypt_owned; RecordBatch: the same three straight from "record1…" strings; decrypt_strings, balance: one call down to plain fields;
//   decrypt_strings_many, balances: the same for several accounts in one call)
// Layouts are snarkVM's: Fr = 4 x u64 Montgomery, scalar = 4 x u64 canonical, G1Affine = 104 bytes, Projective = 144 bytes.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <future>
#include <mutex>
#include <optional>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "aleo_mi355x.h"

namespace aleo_mi355x {

struct Fr { uint64_t l[4]; };                                   // Montgomery form
struct BigInteger256 { uint64_t l[4]; };                        // canonical scalar
struct G1Affine { uint64_t x[6], y[6]; uint8_t infinity; uint8_t pad[7]; };
static_assert(sizeof(G1Affine) == 104, "snarkVM Affine layout");
struct G1Projective { uint64_t x[6], y[6], z[6]; bool is_zero() const { uint64_t o = 0; for (auto v : z) o |= v; return o == 0; } };
static_assert(sizeof(G1Projective) == 144, "snarkVM Projective layout");

struct Error {
  int32_t code;
  std::string message() const { return std::string(aleo_mi355x_strerror(code)) + " [" + aleo_mi355x_last_error() + "]"; }
  bool unsatisfied() const { return code == ALEO_MI355X_ERR_UNSATISFIED; }      // a prover refused an assignment that violates its circuit
  bool not_owner() const { return code == ALEO_MI355X_ERR_NOT_OWNER; }          // a record's owner is not the given address (upstream: "view key did not match record")
};
template <class T> struct Result {       // Ok(value) or Err(Error), like the Rust side sees it
  std::optional<T> value; Error error{0};
  bool is_ok() const { return value.has_value(); }
};

// A base set resident in HBM (Arc<Vec<G1Affine>> on the Rust side).
class PinnedBases {
 public:
  PinnedBases() = default;
  static Result<PinnedBases> pin(const G1Affine* bases, size_t n) {
    PinnedBases p; int32_t rc = aleo_mi355x_bases_pin(bases, sizeof(G1Affine), n, &p.handle_);
    if (rc) return {std::nullopt, Error{rc}};
    p.n_ = n; return {std::move(p), Error{0}};
  }
  static Result<PinnedBases> generate_multiples(const G1Affine& base, uint64_t first, size_t n) {
    PinnedBases p; int32_t rc = aleo_mi355x_bases_generate(&base, first, n, &p.handle_);
    if (rc) return {std::nullopt, Error{rc}};
    p.n_ = n; return {std::move(p), Error{0}};
  }
  PinnedBases(PinnedBases&& o) noexcept : handle_(o.handle_), n_(o.n_) { o.handle_ = 0; }
  PinnedBases& operator=(PinnedBases&& o) noexcept { release(); handle_ = o.handle_; n_ = o.n_; o.handle_ = 0; return *this; }
  PinnedBases(const PinnedBases&) = delete; PinnedBases& operator=(const PinnedBases&) = delete;
  ~PinnedBases() { release(); }
  int32_t precompute() { return aleo_mi355x_bases_precompute(handle_); }
  uint64_t handle() const { return handle_; }
  size_t len() const { return n_; }
  static PinnedBases adopt(uint64_t handle, size_t n) { PinnedBases p; p.handle_ = handle; p.n_ = n; return p; }      // takes ownership of a handle the C ABI returned
 private:
  void release() { if (handle_) { aleo_mi355x_bases_unpin(handle_); handle_ = 0; } }
  uint64_t handle_ = 0; size_t n_ = 0;
};

// One base set over several devices of this process: contiguous point shards, shard g on devices[g] (aleo_mi355x_bases_pin_sharded).
class ShardedBases {
 public:
  ShardedBases() = default;
  static Result<ShardedBases> pin(const G1Affine* bases, size_t n, const std::vector<int32_t>& devices, bool precompute = true) {
    ShardedBases p; int32_t rc = aleo_mi355x_bases_pin_sharded(bases, sizeof(G1Affine), n, devices.data(), devices.size(), precompute ? 1 : 0, &p.handle_);
    if (rc) return {std::nullopt, Error{rc}};
    p.n_ = n; p.shards_ = devices.size(); return {std::move(p), Error{0}};
  }
  static Result<ShardedBases> generate_multiples(const G1Affine& base, uint64_t first, size_t n, const std::vector<int32_t>& devices, bool precompute = true) {
    ShardedBases p; int32_t rc = aleo_mi355x_bases_generate_sharded(&base, first, n, devices.data(), devices.size(), precompute ? 1 : 0, &p.handle_);
    if (rc) return {std::nullopt, Error{rc}};
    p.n_ = n; p.shards_ = devices.size(); return {std::move(p), Error{0}};
  }
  ShardedBases(ShardedBases&& o) noexcept : handle_(o.handle_), n_(o.n_), shards_(o.shards_) { o.handle_ = 0; }
  ShardedBases& operator=(ShardedBases&& o) noexcept { release(); handle_ = o.handle_; n_ = o.n_; shards_ = o.shards_; o.handle_ = 0; return *this; }
  ShardedBases(const ShardedBases&) = delete; ShardedBases& operator=(const ShardedBases&) = delete;
  ~ShardedBases() { release(); }
  uint64_t handle() const { return handle_; }
  size_t len() const { return n_; }
  size_t shards() const { return shards_; }
 private:
  void release() { if (handle_) { aleo_mi355x_bases_unpin_sharded(handle_); handle_ = 0; } }
  uint64_t handle_ = 0; size_t n_ = 0, shards_ = 0;
};

struct VariableBase {
  // ONE msm over the devices of a sharded set: per-device Pippenger, partial sums added on the host in shard order
  static Result<G1Projective> msm(const ShardedBases& bases, const BigInteger256* scalars, size_t n_scalars) {
    G1Projective out{}; size_t n = bases.len() < n_scalars ? bases.len() : n_scalars;
    int32_t rc = aleo_mi355x_msm_g1_sharded(&out, bases.handle(), scalars, n, nullptr);
    if (rc) return {std::nullopt, Error{rc}};
    return {out, Error{0}};
  }
  // VariableBase::msm(bases, scalars): sum_i scalars[i] * bases[i] over the shorter of the two slices.
  static Result<G1Projective> msm(const G1Affine* bases, size_t n_bases, const BigInteger256* scalars, size_t n_scalars) {
    G1Projective out{}; size_t n = n_bases < n_scalars ? n_bases : n_scalars;
    int32_t rc = aleo_mi355x_msm_g1(&out, bases, sizeof(G1Affine), scalars, n);
    if (rc) return {std::nullopt, Error{rc}};
    return {out, Error{0}};
  }
  static Result<G1Projective> msm(const PinnedBases& bases, const BigInteger256* scalars, size_t n_scalars) {
    G1Projective out{}; size_t n = bases.len() < n_scalars ? bases.len() : n_scalars;
    int32_t rc = aleo_mi355x_msm_g1_pinned(&out, bases.handle(), scalars, n);
    if (rc) return {std::nullopt, Error{rc}};
    return {out, Error{0}};
  }
};

// KZG10::commit over a pinned SRS.  Polynomials are coefficient vectors in Montgomery form (DensePolynomial::coeffs); trailing zero
// coefficients are skipped like the reference's `skip_leading_zeros_and_convert_to_bigints`.
struct KZG10 {
  static size_t degree_plus_one(const std::vector<Fr>& p) { size_t n = p.size(); while (n && !(p[n - 1].l[0] | p[n - 1].l[1] | p[n - 1].l[2] | p[n - 1].l[3])) --n; return n; }
  static Result<G1Affine> commit(const PinnedBases& powers, const std::vector<Fr>& poly) {
    G1Affine out{}; int32_t rc = aleo_mi355x_kzg_commit(&out, powers.handle(), poly.data(), degree_plus_one(poly));
    if (rc) return {std::nullopt, Error{rc}};
    return {out, Error{0}};
  }
  // the commitments of one prover round: k polynomials, one call (shared launches on the device), results in the order given
  static Result<std::vector<G1Affine>> commit_batch(const PinnedBases& powers, const std::vector<const std::vector<Fr>*>& polys) {
    std::vector<const void*> ptrs; std::vector<size_t> lens;
    for (auto* p : polys) { ptrs.push_back(p->data()); lens.push_back(degree_plus_one(*p)); }
    std::vector<G1Affine> out(polys.size());
    int32_t rc = aleo_mi355x_kzg_commit_batch(out.data(), powers.handle(), ptrs.data(), lens.data(), polys.size());
    if (rc) return {std::nullopt, Error{rc}};
    return {std::move(out), Error{0}};
  }
};

// CanonicalSerialize / CanonicalDeserialize (compressed) of G1Affine: 48 bytes
struct CompressedG1 { uint8_t b[48]; };
inline Result<CompressedG1> serialize_compressed(const G1Affine& p) {
  CompressedG1 c{}; int32_t rc = aleo_mi355x_g1_compress(c.b, &p, 1);
  if (rc) return {std::nullopt, Error{rc}};
  return {c, Error{0}};
}
inline Result<G1Affine> deserialize_compressed(const CompressedG1& c, bool validate_subgroup = true) {
  G1Affine p{}; int32_t rc = aleo_mi355x_g1_decompress(&p, c.b, 1, validate_subgroup ? 1 : 0);
  if (rc) return {std::nullopt, Error{rc}};
  return {p, Error{0}};
}

enum class NTTInputOutputOrder : int32_t { NN = 0, NR = 1, RN = 2, RR = 3 };
enum class NTTDirection : int32_t { Forward = 0, Inverse = 1 };
enum class NTTType : int32_t { Standard = 0, Coset = 1 };

// snarkvm_algorithms_cuda::NTT(domain_size, data, order, direction, type)
inline Result<bool> NTT(size_t domain_size, Fr* inout, NTTInputOutputOrder order, NTTDirection dir, NTTType type) {
  uint32_t lg = 0; while (((size_t)1 << lg) < domain_size) ++lg;
  if (((size_t)1 << lg) != domain_size) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  int32_t rc = aleo_mi355x_ntt_fr(inout, lg, (int32_t)order, (int32_t)dir, (int32_t)type);
  if (rc) return {std::nullopt, Error{rc}};
  return {true, Error{0}};
}

class EvaluationDomain {
 public:
  size_t size; uint32_t log_size_of_group;
  // EvaluationDomain::new(num_coeffs): None when the power of two exceeds the two-adicity of Fr (47)
  static std::optional<EvaluationDomain> new_(size_t num_coeffs) {
    size_t s = 1; uint32_t lg = 0; while (s < num_coeffs) { s <<= 1; ++lg; }
    if (lg > 47) return std::nullopt;
    return EvaluationDomain{s, lg};
  }
  // *_in_place resize the vector to the domain size with zeros first, as the reference does
  Result<bool> fft_in_place(std::vector<Fr>& x) const { return run(x, NTTDirection::Forward, NTTType::Standard); }
  Result<bool> ifft_in_place(std::vector<Fr>& x) const { return run(x, NTTDirection::Inverse, NTTType::Standard); }
  Result<bool> coset_fft_in_place(std::vector<Fr>& x) const { return run(x, NTTDirection::Forward, NTTType::Coset); }
  Result<bool> coset_ifft_in_place(std::vector<Fr>& x) const { return run(x, NTTDirection::Inverse, NTTType::Coset); }
  // the same transforms split over several devices of this process (4-step, one peer exchange): devices.size() a power of two
  // device-resident data (2^log_size_of_group elements at d_inout on the current device): the transform over several devices, no host buffer
  Result<bool> in_place_sharded_device(void* d_inout, NTTDirection d, NTTType t, const std::vector<int32_t>& devices, void* stream = nullptr) const {
    int32_t rc = aleo_mi355x_ntt_fr_sharded_device(d_inout, log_size_of_group, (int32_t)d, (int32_t)t, devices.data(), devices.size(), stream);
    if (rc) return {std::nullopt, Error{rc}};
    return {true, Error{0}};
  }
  Result<bool> in_place_sharded(std::vector<Fr>& x, NTTDirection d, NTTType t, const std::vector<int32_t>& devices) const {
    if (x.size() > size) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    x.resize(size, Fr{{0, 0, 0, 0}});
    int32_t rc = aleo_mi355x_ntt_fr_sharded(x.data(), log_size_of_group, (int32_t)d, (int32_t)t, devices.data(), devices.size());
    if (rc) return {std::nullopt, Error{rc}};
    return {true, Error{0}};
  }
 private:
  Result<bool> run(std::vector<Fr>& x, NTTDirection d, NTTType t) const {
    if (x.size() > size) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    x.resize(size, Fr{{0, 0, 0, 0}});
    return NTT(size, x.data(), NTTInputOutputOrder::NN, d, t);
  }
};


// ---- the prove call of one proving key ------------------------------------------------------------------------
// Mirrors what sits under `trace.prove_execution::<A, _>(…)` (/root/reference/rust/src/program/execute.rs:74) and `vm.execute(…)` (:177,
// transfer.rs:99): Trace::prove_execution -> ProvingKey::prove_batch(&[(pk, assignments)]) -> Varuna::prove_batch [UPSTREAM-RECALL], for ONE
// circuit with 1..32 instances.  CommitterKey = the universal SRS trimmed for the circuit (powers ‖ hiding powers, pinned in HBM);
// ProvingKey = the circuit's index in HBM (AHPForR1CS::index); prove_batch = one call of the C ABI.
struct R1CSMatrix { std::vector<uint32_t> row_ptr, col; std::vector<BigInteger256> val; };      // CSR over the variables, public ones first
struct R1CS { R1CSMatrix a, b, c; size_t num_constraints = 0, num_public = 0, num_private = 0; };
enum class DomainPolicy : uint32_t { Auto = 0, PerMatrix = 1, Shared = 2 };

class CommitterKey {
 public:
  // powers_of_beta_g[0..=max_degree] followed by powers_of_beta_times_gamma_g (>= 3): one resident set, fixed-base tables built once
  static Result<CommitterKey> pin(const G1Affine* powers_then_gamma_powers, size_t max_degree, size_t n_gamma) {
    auto b = PinnedBases::pin(powers_then_gamma_powers, max_degree + 1 + n_gamma);
    if (!b.is_ok()) return {std::nullopt, b.error};
    return finish(std::move(*b.value), max_degree, n_gamma);
  }
  // synthetic setup: P_i = s_i * base for canonical scalars s = (tau^i)_{i <= max_degree} ‖ (gamma tau^i)_{i < n_gamma}
  static Result<CommitterKey> from_scalars(const G1Affine& base, const BigInteger256* scalars, size_t max_degree, size_t n_gamma) {
    uint64_t h = 0; int32_t rc = aleo_mi355x_bases_from_scalars(&base, scalars, max_degree + 1 + n_gamma, &h);
    if (rc) return {std::nullopt, Error{rc}};
    return finish(PinnedBases::adopt(h, max_degree + 1 + n_gamma), max_degree, n_gamma);
  }
  uint64_t handle() const { return bases_.handle(); }
  size_t max_degree() const { return max_degree_; }
  size_t gamma_offset() const { return max_degree_ + 1; }
  size_t lagrange_offset() const { return lagrange_offset_; }      // 0: no Lagrange-basis powers pinned (commitments from coefficients)
  void set_lagrange_offset(size_t off) { lagrange_offset_ = off; }  // the set pinned holds L_i(tau) G of the circuit's domain H, then v_H(tau) G, from `off`
  // Large proofs over several devices (`north_star`: "large proofs shard MSM bases ... across the 8 GPUs"): a second copy of the key's
  // points cut into contiguous shards over `devices` (each device holds 1/G of the powers and of their window tables), owned by this key.  From then
  // on every commitment a prover makes against this key with at least min_points scalars in all is computed shard by shard — each device pulls its
  // slices of the coefficient vectors, 144 bytes per shard and result come back — and the proof bytes do not change (aleo_mi355x_bases_attach_shards).
  // transforms_from: the prover's transforms of at least that many elements take the same devices (0 = the library's default, 2^24)
  Error shard_over(const std::vector<int32_t>& devices, size_t min_points = (size_t)1 << 16, size_t transforms_from = 0) {
    unshard();
    std::vector<G1Affine> host(bases_.len());
    int32_t rc = aleo_mi355x_bases_download(bases_.handle(), 0, host.size(), host.data());
    if (rc) return Error{rc};
    auto sh = ShardedBases::pin(host.data(), host.size(), devices, true);
    if (!sh.is_ok()) return sh.error;
    rc = aleo_mi355x_bases_attach_shards(bases_.handle(), sh.value->handle(), min_points);
    if (rc) return Error{rc};
    if (transforms_from) { rc = aleo_mi355x_bases_shard_transforms(bases_.handle(), transforms_from); if (rc) return Error{rc}; }
    shards_ = std::move(*sh.value);
    return Error{0};
  }
  void unshard() { if (shards_.handle()) { aleo_mi355x_bases_attach_shards(bases_.handle(), 0, 0); shards_ = ShardedBases(); } }
  size_t shards() const { return shards_.shards(); }
  CommitterKey() = default;
  CommitterKey(CommitterKey&&) noexcept = default;
  CommitterKey& operator=(CommitterKey&& o) noexcept { if (this != &o) { unshard(); bases_ = std::move(o.bases_); shards_ = std::move(o.shards_); max_degree_ = o.max_degree_; lagrange_offset_ = o.lagrange_offset_; } return *this; }
  ~CommitterKey() { unshard(); }                                    // detach before the shards (and then the points) go
 private:
  static Result<CommitterKey> finish(PinnedBases b, size_t max_degree, size_t n_gamma) {
    if (n_gamma < 3) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    int32_t rc = b.precompute(); if (rc) return {std::nullopt, Error{rc}};
    CommitterKey k; k.bases_ = std::move(b); k.max_degree_ = max_degree; return {std::move(k), Error{0}};
  }
  PinnedBases bases_; ShardedBases shards_; size_t max_degree_ = 0, lagrange_offset_ = 0;
};

// The caller's randomness for one proof: 32 bytes, the key of the prover's ChaCha20 stream.  The reference's call sites pass a CSPRNG
// (`rand::thread_rng()`, /root/reference/rust/src/program/execute.rs:74); from_entropy() is that.  A repeated seed repeats the blinding of a
// proof: from_u64 exists for reproducible tests only.
struct Seed {
  uint8_t bytes[32];
  static Seed from_entropy() { Seed s; std::random_device rd; for (int i = 0; i < 32; i += 4) { const uint32_t v = rd(); std::memcpy(s.bytes + i, &v, 4); } return s; }
  static Seed from_u64(uint64_t v) { Seed s; std::memset(s.bytes, 0, 32); for (int i = 0; i < 8; ++i) s.bytes[i] = (uint8_t)(v >> (8 * i)); return s; }
};

struct Proof {
  std::vector<uint8_t> bytes;                                   // Proof::write_le layout
  Result<std::string> to_string() const {                       // Display: bech32m, hrp "proof"
    std::string s(2 * bytes.size() + 16, '\0');
    int32_t rc = aleo_mi355x_bech32m_encode(s.data(), s.size(), "proof", bytes.data(), bytes.size());
    if (rc) return {std::nullopt, Error{rc}};
    s.resize(std::char_traits<char>::length(s.c_str())); return {std::move(s), Error{0}};
  }
};

class ProvingKey {
 public:
  // AHPForR1CS::index + the circuit's commitments (Process::synthesize_key, /root/reference/wasm/src/programs/manager/mod.rs:164-177)
  static Result<ProvingKey> index(const CommitterKey& ck, const R1CS& cs, DomainPolicy policy = DomainPolicy::Auto) {
    aleo_mi355x_r1cs_matrix m[3] = {{cs.a.row_ptr.data(), cs.a.col.data(), cs.a.val.data()}, {cs.b.row_ptr.data(), cs.b.col.data(), cs.b.val.data()},
                                    {cs.c.row_ptr.data(), cs.c.col.data(), cs.c.val.data()}};
    for (auto* q : {&cs.a, &cs.b, &cs.c}) if (q->row_ptr.size() != cs.num_constraints + 1 || q->col.size() != q->val.size()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    ProvingKey pk;
    int32_t rc = aleo_mi355x_varuna_index_build(&pk.handle_, ck.handle(), ck.max_degree(), ck.gamma_offset(), ck.lagrange_offset(), m, cs.num_constraints, cs.num_public, cs.num_private, (uint32_t)policy);
    if (rc) return {std::nullopt, Error{rc}};
    pk.num_variables_ = cs.num_public + cs.num_private;
    return {std::move(pk), Error{0}};
  }
  // ProvingKey::prove_batch: one assignment (public variables first, z_0 = 1, canonical) per instance; `seed` stands for the caller's RNG
  Result<Proof> prove_batch(const std::vector<const std::vector<BigInteger256>*>& assignments, const Seed& seed = Seed::from_entropy()) const {
    std::vector<const void*> p;
    for (auto* a : assignments) { if (!a || a->size() != num_variables_) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}}; p.push_back(a->data()); }
    Proof out; out.bytes.resize(1024 + 192 * assignments.size()); size_t len = out.bytes.size();
    int32_t rc = aleo_mi355x_varuna_prove_indexed(handle_, p.data(), p.size(), seed.bytes, out.bytes.data(), &len);
    if (rc) return {std::nullopt, Error{rc}};
    out.bytes.resize(len); return {std::move(out), Error{0}};
  }
  // what the verifier's transcript starts from: 12 compressed index commitments + the domain sizes
  Result<std::vector<uint8_t>> verifying_key_bytes() const {
    std::vector<uint8_t> v(1024); size_t len = v.size();
    int32_t rc = aleo_mi355x_varuna_index_vk(handle_, v.data(), &len);
    if (rc) return {std::nullopt, Error{rc}};
    v.resize(len); return {std::move(v), Error{0}};
  }
  ProvingKey() = default;
  ProvingKey(ProvingKey&& o) noexcept : handle_(o.handle_), num_variables_(o.num_variables_) { o.handle_ = 0; }
  ProvingKey& operator=(ProvingKey&& o) noexcept { release(); handle_ = o.handle_; num_variables_ = o.num_variables_; o.handle_ = 0; return *this; }
  ProvingKey(const ProvingKey&) = delete; ProvingKey& operator=(const ProvingKey&) = delete;
  ~ProvingKey() { release(); }
  uint64_t handle() const { return handle_; }
  size_t num_variables() const { return num_variables_; }
 private:
  void release() { if (handle_) { aleo_mi355x_varuna_index_free(handle_); handle_ = 0; } }
  uint64_t handle_ = 0; size_t num_variables_ = 0;
};

// Varuna::prove_batch(keys_to_constraints: &BTreeMap<&ProvingKey, &[Assignment]>): ONE proof for several proving keys, each with its instances, in
// the order given (upstream: the map's key order).  All keys must have been indexed against the same CommitterKey.
using KeyedAssignments = std::vector<std::pair<const ProvingKey*, std::vector<const std::vector<BigInteger256>*>>>;
inline Result<Proof> prove_batch(const KeyedAssignments& keyed, const Seed& seed = Seed::from_entropy()) {
  std::vector<uint64_t> handles; std::vector<size_t> counts; std::vector<const void*> p;
  for (auto& [pk, zs] : keyed) {
    if (!pk || zs.empty()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    handles.push_back(pk->handle()); counts.push_back(zs.size());
    for (auto* a : zs) { if (!a || a->size() != pk->num_variables()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}}; p.push_back(a->data()); }
  }
  Proof out; out.bytes.resize(1024 + 400 * handles.size() + 192 * p.size()); size_t len = out.bytes.size();
  int32_t rc = aleo_mi355x_varuna_prove_batch_indexed(handles.data(), handles.size(), p.data(), counts.data(), seed.bytes, out.bytes.data(), &len);
  if (rc) return {std::nullopt, Error{rc}};
  out.bytes.resize(len); return {std::move(out), Error{0}};
}

// Independent proofs in lockstep (aleo_mi355x_varuna_prove_many): request i is what prove_batch(keyed[i], seeds[i]) would prove, byte for byte; the
// proofs share every round's commitment launch chain.  One Result per request: a request that fails carries its own error, the others complete.
inline std::vector<Result<Proof>> prove_many(const std::vector<KeyedAssignments>& requests, const std::vector<Seed>& seeds) {
  const size_t n = requests.size();
  std::vector<Result<Proof>> out; out.reserve(n);
  if (seeds.size() != n || n == 0) { for (size_t i = 0; i < n; ++i) out.push_back({std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}}); return out; }
  std::vector<std::vector<uint64_t>> handles(n); std::vector<std::vector<size_t>> counts(n); std::vector<std::vector<const void*>> ptrs(n);
  std::vector<Proof> proofs(n); std::vector<aleo_mi355x_prove_request> rq(n); std::vector<int32_t> pre(n, 0);
  for (size_t i = 0; i < n; ++i) {
    for (auto& [pk, zs] : requests[i]) {
      if (!pk || zs.empty()) { pre[i] = ALEO_MI355X_ERR_BAD_ARG; break; }
      handles[i].push_back(pk->handle()); counts[i].push_back(zs.size());
      for (auto* a : zs) { if (!a || a->size() != pk->num_variables()) { pre[i] = ALEO_MI355X_ERR_BAD_ARG; break; } ptrs[i].push_back(a->data()); }
    }
    if (requests[i].empty()) pre[i] = ALEO_MI355X_ERR_BAD_ARG;
    proofs[i].bytes.resize(1024 + 400 * handles[i].size() + 192 * ptrs[i].size());
    rq[i] = aleo_mi355x_prove_request{handles[i].data(), pre[i] ? 0 : handles[i].size(), ptrs[i].data(), counts[i].data(), seeds[i].bytes, proofs[i].bytes.data(), proofs[i].bytes.size(), 0};
  }
  const int32_t rc = aleo_mi355x_varuna_prove_many(rq.data(), n);
  for (size_t i = 0; i < n; ++i) {
    const int32_t st = pre[i] ? pre[i] : (rq[i].status ? rq[i].status : rc);
    if (st) { out.push_back({std::nullopt, Error{st}}); continue; }
    proofs[i].bytes.resize(rq[i].len); out.push_back({std::move(proofs[i]), Error{0}});
  }
  return out;
}

// The front end that turns concurrent provers into lockstep calls: every proving thread of the host — the dev server proves each request on a
// tokio::task::spawn_blocking thread, /root/reference/rust/develop/src/routes.rs:119,149,229 — submits its request and waits on a future; ONE drainer
// thread takes whatever is queued (up to max_batch requests, waiting at most max_wait for company once the first one is there) and proves it with a
// single prove_many call.  A proof is byte for byte what prove_batch(keyed, seed) returns; only WHO calls the library changes.  The keyed assignments
// (proving keys and assignment vectors) must stay alive until the future is ready.  `drainers` such threads share the queue (default 2): two lockstep
// calls in flight fill each other's gaps — the small kernels between one call's commitments run beside the other's accumulations (2^15 constraints,
// 8 proofs per call: 222 proofs/s from one caller, 254 from two; profiles/r04_lockstep_pipeline_ab.jsonl).
class ProvingQueue {
 public:
  explicit ProvingQueue(size_t max_batch = 8, std::chrono::microseconds max_wait = std::chrono::microseconds(200), int32_t device = -1, size_t drainers = 2)      // device: the one the proving keys live on (-1: the drainer threads' default)
      : max_batch_(max_batch < 1 ? 1 : (max_batch > 64 ? 64 : max_batch)), max_wait_(max_wait), device_(device) {
    const size_t nd = drainers < 1 ? 1 : (drainers > 4 ? 4 : drainers);
    for (size_t i = 0; i < nd; ++i) drainers_.emplace_back([this] { run(); });
  }
  ~ProvingQueue() { { std::lock_guard<std::mutex> lk(mu_); stop_ = true; } cv_.notify_all(); for (auto& t : drainers_) t.join(); }
  ProvingQueue(const ProvingQueue&) = delete; ProvingQueue& operator=(const ProvingQueue&) = delete;
  std::future<Result<Proof>> submit(KeyedAssignments keyed, const Seed& seed = Seed::from_entropy()) {
    Item it; it.keyed = std::move(keyed); it.seed = seed; auto f = it.done.get_future();
    { std::lock_guard<std::mutex> lk(mu_); q_.push_back(std::move(it)); }
    cv_.notify_all(); return f;
  }
  size_t calls() const { std::lock_guard<std::mutex> lk(mu_); return calls_; }          // prove_many calls made so far (tests: fewer than requests)
 private:
  struct Item { KeyedAssignments keyed; Seed seed; std::promise<Result<Proof>> done; };
  void run() {
    (void)aleo_mi355x_init_device(device_);                 // selects the device for this thread; if it fails the requests below come back with the library's error
    for (;;) {
      std::vector<Item> batch;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;                                                          // stop requested and nothing left
        if (q_.size() < max_batch_ && !stop_) cv_.wait_for(lk, max_wait_, [&] { return stop_ || q_.size() >= max_batch_; });
        while (!q_.empty() && batch.size() < max_batch_) { batch.push_back(std::move(q_.front())); q_.pop_front(); }
        ++calls_;
      }
      std::vector<KeyedAssignments> reqs; std::vector<Seed> seeds;
      for (auto& it : batch) { reqs.push_back(it.keyed); seeds.push_back(it.seed); }
      auto out = prove_many(reqs, seeds);
      for (size_t i = 0; i < batch.size(); ++i) batch[i].done.set_value(std::move(out[i]));
    }
  }
  const size_t max_batch_; const std::chrono::microseconds max_wait_; const int32_t device_;
  mutable std::mutex mu_; std::condition_variable cv_; std::deque<Item> q_; bool stop_ = false; size_t calls_ = 0;
  std::vector<std::thread> drainers_;
};

// snarkvm_synthesizer_process::Trace as the prover sees it: the transitions of one transaction, each the proving key of its
// function and the assignment its execution produced.  prove_execution / prove_fee group the assignments per proving key (order of first
// appearance; upstream: BTreeMap order of the keys) and make ONE proof for all of them — the call under
// `trace.prove_execution::<A, _>(locator, rng)` at /root/reference/rust/src/program/execute.rs:74.  Inclusion proofs (state paths from the
// ledger) are further assignments of one more circuit and enter the same way; fetching them is the SDK's business.
class Trace {
 public:
  void insert_transition(const ProvingKey& pk, const std::vector<BigInteger256>& assignment) {
    for (auto& e : keyed_) if (e.first == &pk) { e.second.push_back(&assignment); return; }
    keyed_.push_back({&pk, {&assignment}});
  }
  size_t transitions() const { size_t n = 0; for (auto& e : keyed_) n += e.second.size(); return n; }
  Result<Proof> prove_execution(const Seed& seed = Seed::from_entropy()) const { return keyed_.empty() ? Result<Proof>{std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}} : prove_batch(keyed_, seed); }
  Result<Proof> prove_fee(const Seed& seed = Seed::from_entropy()) const {              // a fee is exactly one transition
    return transitions() != 1 ? Result<Proof>{std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}} : prove_batch(keyed_, seed);
  }
 private:
  KeyedAssignments keyed_;
};

// ---- record ownership (the SDK's record search) ------------------------------------------------------------------------------------
// snarkvm_console_account::{ViewKey, Address} as the scan takes them: the scalar of "AViewKey1…" (base58) and the x-coordinate of "aleo1…" (bech32m),
// 32 little-endian bytes each.  The address of a view key is not derived here (upstream's generator is a hash to the curve): callers hold both.
struct ViewKey {
  uint8_t scalar[32];
  static Result<ViewKey> from_string(const std::string& s) {
    static const char* B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
    static const uint8_t prefix[7] = {14, 138, 223, 204, 247, 224, 122};
    uint8_t raw[39] = {};                                         // big-endian base-256 digits of the base-58 number
    for (char ch : s) {
      const char* q = ch ? std::strchr(B58, ch) : nullptr;
      if (!q) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
      uint32_t carry = (uint32_t)(q - B58);
      for (int i = 38; i >= 0; --i) { carry += 58u * raw[i]; raw[i] = (uint8_t)carry; carry >>= 8; }
      if (carry) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    }
    if (std::memcmp(raw, prefix, 7)) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    ViewKey v; std::memcpy(v.scalar, raw + 7, 32); return {v, Error{0}};
  }
};
struct Address {
  uint8_t x[32];
  static Result<Address> from_string(const std::string& s) {
    uint8_t raw[64]; size_t len = sizeof raw; char hrp[16];
    int32_t rc = aleo_mi355x_bech32m_decode(raw, &len, hrp, sizeof hrp, s.c_str());
    if (rc) return {std::nullopt, Error{rc}};
    if (std::strcmp(hrp, "aleo") || len != 32) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    Address a; std::memcpy(a.x, raw, 32); return {a, Error{0}};
  }
};

// Record<N, Plaintext<N>> as its string, the way the reference prints it ("{\n  owner: aleo1….private,\n  microcredits: 1500000000000000u64.private,\n  _nonce: …group.public\n}").
class RecordPlaintext {
 public:
  explicit RecordPlaintext(std::string s) : string_(std::move(s)) {}
  const std::string& to_string() const { return string_; }
  // RecordPlaintext.microcredits of the reference's wasm: the value of a u64 entry of that name at the record's top level, else 0
  uint64_t microcredits() const {
    const std::string key = "\n  microcredits: ";
    const size_t at = string_.find(key); if (at == std::string::npos) return 0;
    size_t p = at + key.size(); uint64_t v = 0; bool digits = false;
    while (p < string_.size() && string_[p] >= '0' && string_[p] <= '9') { v = v * 10 + (uint64_t)(string_[p++] - '0'); digits = true; }
    return digits && string_.compare(p, 4, "u64.") == 0 ? v : 0;
  }
 private:
  std::string string_;
};
// a string through the (out, in/out length) convention of the C ABI: a first try with room for most records, a second with the length the first returned
template <class Call> inline Result<RecordPlaintext> record_string_out(Call&& call) {
  std::string buf(4096, '\0'); size_t len = buf.size();
  int32_t rc = call(&buf[0], &len);
  if (rc == ALEO_MI355X_ERR_BAD_ARG && len >= buf.size()) { buf.assign(len + 1, '\0'); len = buf.size(); rc = call(&buf[0], &len); }
  if (rc) return {std::nullopt, Error{rc}};
  buf.resize(len); return {RecordPlaintext(std::move(buf)), Error{0}};
}

// Record<N, Ciphertext<N>>: FromStr, is_owner and decrypt (RecordCiphertext.isOwner / .decrypt of the reference's wasm), and the batch forms below.
class RecordCiphertext {
 public:
  static Result<RecordCiphertext> from_string(const std::string& s) {
    RecordCiphertext r; int32_t kind = -1;
    int32_t rc = aleo_mi355x_record_parse(s.c_str(), &kind, r.owner_, r.nonce_);
    if (rc) return {std::nullopt, Error{rc}};
    r.private_owner_ = kind == 1; r.string_ = s; return {std::move(r), Error{0}};
  }
  const std::string& to_string() const { return string_; }
  bool owner_is_private() const { return private_owner_; }
  const uint8_t* owner_field() const { return owner_; }           // the address x (public owner) or the one field of the owner ciphertext
  const uint8_t* nonce_x() const { return nonce_; }
  Result<bool> is_owner(const ViewKey& vk, const Address& address) const {
    if (!private_owner_) return {std::memcmp(owner_, address.x, 32) == 0, Error{0}};
    uint8_t flag = 0; int32_t rc = aleo_mi355x_records_scan(&flag, nullptr, owner_, nonce_, 1, vk.scalar, address.x);
    if (rc) return {std::nullopt, Error{rc}};
    return {flag == 1, Error{0}};
  }
  // RecordCiphertext.decrypt(viewKey), on the host; ALEO_MI355X_ERR_NOT_OWNER when the view key does not decrypt the owner to the address
  Result<RecordPlaintext> decrypt(const ViewKey& vk, const Address& address) const {
    return record_string_out([&](char* out, size_t* len) { return aleo_mi355x_record_decrypt(string_.c_str(), vk.scalar, address.x, out, len); });
  }
  // the private fields in randomizer order, 32 bytes each: the owner's if it is private, then every private entry's
  Result<std::vector<uint8_t>> fields() const {
    size_t n = 0; int32_t rc = aleo_mi355x_record_fields(string_.c_str(), nullptr, 0, &n);
    if (rc) return {std::nullopt, Error{rc}};
    std::vector<uint8_t> f(32 * n);
    if (n && (rc = aleo_mi355x_record_fields(string_.c_str(), f.data(), n, &n))) return {std::nullopt, Error{rc}};
    return {std::move(f), Error{0}};
  }
  // the plaintext from this record's decrypted fields (records_decrypt_fields); the owner must be `address`
  Result<RecordPlaintext> plaintext(const uint8_t* plain_fields, size_t n_fields, const Address& address) const {
    return record_string_out([&](char* out, size_t* len) { return aleo_mi355x_record_plaintext(string_.c_str(), plain_fields, n_fields, address.x, out, len); });
  }
 private:
  std::string string_; bool private_owner_ = false; uint8_t owner_[32] = {}, nonce_[32] = {};
};

struct OwnedRecord { size_t index; bool has_view_key; uint8_t record_view_key_x[32]; };      // has_view_key: false for a public owner (nothing is encrypted)
// The records of `batch` the account owns, in order, with the x of view_key * nonce of each (what decrypts it): one scan for the whole batch.  An Err means
// "test them on the CPU one by one", as for every other operator.
inline Result<std::vector<OwnedRecord>> find_owned(const std::vector<RecordCiphertext>& batch, const ViewKey& vk, const Address& address) {
  std::vector<uint8_t> c0, nx; std::vector<size_t> at;
  for (size_t i = 0; i < batch.size(); ++i)
    if (batch[i].owner_is_private()) { c0.insert(c0.end(), batch[i].owner_field(), batch[i].owner_field() + 32); nx.insert(nx.end(), batch[i].nonce_x(), batch[i].nonce_x() + 32); at.push_back(i); }
  std::vector<uint8_t> flags(at.size()), rvk(32 * at.size());
  if (!at.empty()) { int32_t rc = aleo_mi355x_records_scan(flags.data(), rvk.data(), c0.data(), nx.data(), at.size(), vk.scalar, address.x); if (rc) return {std::nullopt, Error{rc}}; }
  std::vector<OwnedRecord> out; size_t j = 0;
  for (size_t i = 0; i < batch.size(); ++i) {
    if (!batch[i].owner_is_private()) { if (!std::memcmp(batch[i].owner_field(), address.x, 32)) out.push_back(OwnedRecord{i, false, {}}); continue; }
    if (flags[j] == 1) { OwnedRecord o{i, true, {}}; std::memcpy(o.record_view_key_x, rvk.data() + 32 * j, 32); out.push_back(o); }
    ++j;
  }
  return {std::move(out), Error{0}};
}

// The records of `batch` the account owns, decrypted: the batch form of the reference's `if record.is_owner(..) { record.decrypt(..) }` loop
// (rust/src/api/blocking.rs:274-283).  One scan for the private owners (and for the record view keys of matching public owners that hold private entries), one
// aleo_mi355x_records_decrypt_fields call for the fields of all owned records, the strings on the host.  An owned record whose entries do not parse fails the call.
struct DecryptedRecord { size_t index; RecordPlaintext plaintext; };
inline Result<std::vector<DecryptedRecord>> decrypt_owned(const std::vector<RecordCiphertext>& batch, const ViewKey& vk, const Address& address) {
  using Out = Result<std::vector<DecryptedRecord>>;
  std::vector<std::vector<uint8_t>> fields(batch.size());
  std::vector<uint8_t> c0, nx; std::vector<size_t> at;                // what goes through the scan
  for (size_t i = 0; i < batch.size(); ++i) {
    bool scan = batch[i].owner_is_private();
    if (!scan && !std::memcmp(batch[i].owner_field(), address.x, 32)) { auto f = batch[i].fields(); if (!f.is_ok()) return Out{std::nullopt, f.error}; fields[i] = std::move(*f.value); scan = !fields[i].empty(); }
    if (scan) { c0.insert(c0.end(), batch[i].owner_field(), batch[i].owner_field() + 32); nx.insert(nx.end(), batch[i].nonce_x(), batch[i].nonce_x() + 32); at.push_back(i); }
  }
  std::vector<uint8_t> flags(at.size()), rvk(32 * at.size());
  if (!at.empty()) { int32_t rc = aleo_mi355x_records_scan(flags.data(), rvk.data(), c0.data(), nx.data(), at.size(), vk.scalar, address.x); if (rc) return Out{std::nullopt, Error{rc}}; }
  std::vector<size_t> owned; std::vector<uint8_t> keys, flat; std::vector<uint32_t> offsets{0};
  size_t j = 0;
  for (size_t i = 0; i < batch.size(); ++i) {
    const bool scanned = j < at.size() && at[j] == i;
    const bool is_public = !batch[i].owner_is_private();
    bool mine = is_public && !std::memcmp(batch[i].owner_field(), address.x, 32);
    uint8_t key[32] = {};
    if (scanned) {
      if (is_public && flags[j] == 2) return Out{std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
      if (is_public || flags[j] == 1) { std::memcpy(key, rvk.data() + 32 * j, 32); mine = true; }
      if (!is_public && flags[j] == 1) { auto f = batch[i].fields(); if (!f.is_ok()) return Out{std::nullopt, f.error}; fields[i] = std::move(*f.value); }
      ++j;
    }
    if (!mine) continue;
    owned.push_back(i); keys.insert(keys.end(), key, key + 32); flat.insert(flat.end(), fields[i].begin(), fields[i].end());
    offsets.push_back((uint32_t)(flat.size() / 32));
  }
  std::vector<uint8_t> plain(flat.size()), dflags(owned.size());
  if (!owned.empty()) { int32_t rc = aleo_mi355x_records_decrypt_fields(plain.data(), dflags.data(), keys.data(), offsets.data(), flat.data(), owned.size()); if (rc) return Out{std::nullopt, Error{rc}}; }
  std::vector<DecryptedRecord> out;
  for (size_t k = 0; k < owned.size(); ++k) {
    if (dflags[k]) return Out{std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    auto p = batch[owned[k]].plaintext(plain.data() + 32 * (size_t)offsets[k], offsets[k + 1] - offsets[k], address);
    if (!p.is_ok()) return Out{std::nullopt, p.error};
    out.push_back(DecryptedRecord{owned[k], std::move(*p.value)});
  }
  return Out{std::move(out), Error{0}};
}

// find_owned for several accounts over the same batch: one aleo_mi355x_records_scan_many call (at most 64 accounts) instead of one scan per account.
// (*result)[a] is what find_owned returns for accounts[a].
struct Account { ViewKey view_key; Address address; };
inline Result<std::vector<std::vector<OwnedRecord>>> find_owned_many(const std::vector<RecordCiphertext>& batch, const std::vector<Account>& accounts) {
  std::vector<uint8_t> c0, nx, vks, axs; std::vector<size_t> at;
  for (size_t i = 0; i < batch.size(); ++i)
    if (batch[i].owner_is_private()) { c0.insert(c0.end(), batch[i].owner_field(), batch[i].owner_field() + 32); nx.insert(nx.end(), batch[i].nonce_x(), batch[i].nonce_x() + 32); at.push_back(i); }
  for (const auto& a : accounts) { vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  const size_t n = at.size(), k = accounts.size();
  std::vector<uint8_t> flags(k * n), rvk(32 * k * n);
  if (n && k) { int32_t rc = aleo_mi355x_records_scan_many(flags.data(), rvk.data(), c0.data(), nx.data(), n, vks.data(), axs.data(), k); if (rc) return {std::nullopt, Error{rc}}; }
  std::vector<std::vector<OwnedRecord>> out(k);
  for (size_t a = 0; a < k; ++a) {
    size_t j = 0;
    for (size_t i = 0; i < batch.size(); ++i) {
      if (!batch[i].owner_is_private()) { if (!std::memcmp(batch[i].owner_field(), accounts[a].address.x, 32)) out[a].push_back(OwnedRecord{i, false, {}}); continue; }
      if (flags[a * n + j] == 1) { OwnedRecord o{i, true, {}}; std::memcpy(o.record_view_key_x, rvk.data() + 32 * (a * n + j), 32); out[a].push_back(o); }
      ++j;
    }
  }
  return {std::move(out), Error{0}};
}

// n "record1…" strings as the C ABI takes them — the text of all of them one after another and n + 1 offsets — for callers that hold what the chain hands out:
// the overloads below send the strings to the device as they are (aleo_mi355x_records_scan_strings) and parse on the host only the records they decrypt.
class RecordBatch {
 public:
  // (no default constructor: `{}` where a batch is expected goes on meaning an empty vector of RecordCiphertext)
  explicit RecordBatch(const std::vector<std::string>& strings) : offsets_{0} { for (const auto& s : strings) push_back(s); }
  // the strings of a text that holds one per line (or between any other separator character): the separators are dropped, a trailing one is ignored
  static RecordBatch from_text(const std::string& text, char sep = '\n') {
    RecordBatch b(std::vector<std::string>{});
    for (size_t at = 0; at < text.size();) {
      size_t end = text.find(sep, at); if (end == std::string::npos) end = text.size();
      b.text_.append(text, at, end - at); b.offsets_.push_back(b.text_.size());
      at = end + 1;
    }
    return b;
  }
  void push_back(const std::string& s) { text_ += s; offsets_.push_back(text_.size()); }
  size_t size() const { return offsets_.size() - 1; }
  std::string string(size_t i) const { return text_.substr((size_t)offsets_[i], (size_t)(offsets_[i + 1] - offsets_[i])); }
  const char* text() const { return text_.data(); }
  const uint64_t* offsets() const { return offsets_.data(); }
 private:
  std::string text_; std::vector<uint64_t> offsets_;
};

// find_owned_many from strings: one aleo_mi355x_records_scan_strings call.  A string that does not parse fails the call with what RecordCiphertext::from_string
// returns for the first of them (the batch of objects could not have been built).
inline Result<std::vector<std::vector<OwnedRecord>>> find_owned_many(const RecordBatch& batch, const std::vector<Account>& accounts) {
  const size_t n = batch.size(), k = accounts.size();
  std::vector<uint8_t> vks, axs;
  for (const auto& a : accounts) { vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  std::vector<uint8_t> flags(k * n), rvk(32 * k * n), rows; std::vector<int8_t> kinds(n);
  if (k) { int32_t rc = aleo_mi355x_records_scan_strings(flags.data(), kinds.data(), rvk.data(), batch.text(), batch.offsets(), n, vks.data(), axs.data(), k); if (rc) return {std::nullopt, Error{rc}}; }
  else { rows.resize(64 * n); int32_t rc = aleo_mi355x_records_parse_many(kinds.data(), rows.data(), rows.data() + 32 * n, batch.text(), batch.offsets(), n); if (rc) return {std::nullopt, Error{rc}}; }
  for (size_t i = 0; i < n; ++i)
    if (kinds[i] < 0) { auto r = RecordCiphertext::from_string(batch.string(i)); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  std::vector<std::vector<OwnedRecord>> out(k);
  for (size_t a = 0; a < k; ++a)
    for (size_t i = 0; i < n; ++i)
      if (flags[a * n + i] == 1) { OwnedRecord o{i, kinds[i] == 1, {}}; if (o.has_view_key) std::memcpy(o.record_view_key_x, rvk.data() + 32 * (a * n + i), 32); out[a].push_back(o); }
  return {std::move(out), Error{0}};
}
inline Result<std::vector<OwnedRecord>> find_owned(const RecordBatch& batch, const ViewKey& vk, const Address& address) {
  auto r = find_owned_many(batch, std::vector<Account>{Account{vk, address}});
  if (!r.is_ok()) return {std::nullopt, r.error};
  return {std::move((*r.value)[0]), Error{0}};
}
// decrypt_owned from strings: the scan over the strings says which records are the account's; those alone become RecordCiphertext objects and go through the
// batch above (which scans these few once more for their record view keys and keeps every error it has).
inline Result<std::vector<DecryptedRecord>> decrypt_owned(const RecordBatch& batch, const ViewKey& vk, const Address& address) {
  using Out = Result<std::vector<DecryptedRecord>>;
  auto found = find_owned(batch, vk, address);
  if (!found.is_ok()) return Out{std::nullopt, found.error};
  std::vector<RecordCiphertext> mine;
  for (const auto& o : *found.value) { auto r = RecordCiphertext::from_string(batch.string(o.index)); if (!r.is_ok()) return Out{std::nullopt, r.error}; mine.push_back(std::move(*r.value)); }
  auto dec = decrypt_owned(mine, vk, address);
  if (!dec.is_ok()) return dec;
  if (dec.value->size() != mine.size()) return Out{std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  for (size_t j = 0; j < mine.size(); ++j) (*dec.value)[j].index = (*found.value)[j].index;
  return dec;
}

// What decrypt_strings returns: the records one account owns among a batch of strings, decrypted (aleo_mi355x_records_decrypt_strings).  Owns the library's
// result; the pointers are valid while it lives.  Record k of the size() owned ones, in ascending index: index()[k], kind()[k] (0 public owner, 1 private),
// rvk(k), its n_fields(k) plain fields from fields(k) on in randomizer order, status()[k] (0 decrypted, 2 malformed: zero rows, 4 the structure is refused: no
// fields) and microcredits()[k].  unparsed() strings do not parse, first_unparsed() is the first of them (the batch's size if none).
class FoundRecords {
 public:
  explicit FoundRecords(aleo_mi355x_found* f) : f_(f) {}
  FoundRecords(FoundRecords&& o) noexcept : f_(o.f_) { o.f_ = nullptr; }
  FoundRecords& operator=(FoundRecords&& o) noexcept { if (this != &o) { aleo_mi355x_found_free(f_); f_ = o.f_; o.f_ = nullptr; } return *this; }
  FoundRecords(const FoundRecords&) = delete; FoundRecords& operator=(const FoundRecords&) = delete;
  ~FoundRecords() { aleo_mi355x_found_free(f_); }
  size_t size() const { return aleo_mi355x_found_count(f_); }
  const uint32_t* index() const { return aleo_mi355x_found_index(f_); }
  const int8_t* kind() const { return aleo_mi355x_found_kind(f_); }
  const uint8_t* rvk(size_t k) const { return aleo_mi355x_found_rvk(f_) + 32 * k; }
  const uint32_t* offsets() const { return aleo_mi355x_found_offsets(f_); }
  size_t total_fields() const { return aleo_mi355x_found_fields(f_); }
  size_t n_fields(size_t k) const { return offsets()[k + 1] - offsets()[k]; }
  const uint8_t* fields(size_t k) const { return aleo_mi355x_found_plain(f_) + 32 * (size_t)offsets()[k]; }
  const uint8_t* status() const { return aleo_mi355x_found_status(f_); }
  const uint64_t* microcredits() const { return aleo_mi355x_found_microcredits(f_); }
  size_t unparsed() const { return aleo_mi355x_found_unparsed(f_); }
  size_t first_unparsed() const { return aleo_mi355x_found_first_unparsed(f_); }
  // of unspent_strings[_many]: the kept records' serial numbers (32 bytes each; a null pointer from any other call) and how many records the account owned
  const uint8_t* serials() const { return aleo_mi355x_found_serials(f_); }
  const uint8_t* serial(size_t k) const { return aleo_mi355x_found_serials(f_) + 32 * k; }
  size_t owned() const { return aleo_mi355x_found_owned(f_); }
  // of unspent_named[_many]: the kept records' commitments as well (32 bytes each; a null pointer from any other call)
  const uint8_t* commitments() const { return aleo_mi355x_found_commitments(f_); }
  const uint8_t* commitment(size_t k) const { return aleo_mi355x_found_commitments(f_) + 32 * k; }
  const aleo_mi355x_found* handle() const { return f_; }
 private:
  aleo_mi355x_found* f_;
};
// One call: scan, gather, decrypt and microcredits on the device; only the owned records come back.  A string that does not parse is counted, not an error.
inline Result<FoundRecords> decrypt_strings(const RecordBatch& batch, const ViewKey& vk, const Address& address) {
  aleo_mi355x_found* f = nullptr;
  int32_t rc = aleo_mi355x_records_decrypt_strings(&f, batch.text(), batch.offsets(), batch.size(), vk.scalar, address.x);
  if (rc) return {std::nullopt, Error{rc}};
  return {FoundRecords(f), Error{0}};
}
// The sum of the microcredits of the records the account owns (those with status 0) and the indices of all it owns: the reference's get_unspent_records sum
// (rust/src/api/blocking.rs:274-283) without the spent check (serial_numbers / found_serial_numbers below are what it takes).  A string that does not parse fails the call with what RecordCiphertext::from_string returns for it.
struct Balance { unsigned __int128 microcredits; std::vector<size_t> indices; };
inline Result<Balance> balance(const RecordBatch& batch, const ViewKey& vk, const Address& address) {
  auto found = decrypt_strings(batch, vk, address);
  if (!found.is_ok()) return {std::nullopt, found.error};
  const FoundRecords& f = *found.value;
  if (f.unparsed()) { auto r = RecordCiphertext::from_string(batch.string(f.first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  Balance b{0, {}};
  for (size_t k = 0; k < f.size(); ++k) { b.indices.push_back(f.index()[k]); if (f.status()[k] == 0) b.microcredits += f.microcredits()[k]; }
  return {std::move(b), Error{0}};
}
// decrypt_strings and balance for several accounts (at most 64) over the same batch in one aleo_mi355x_records_decrypt_strings_many call: the text goes up and is
// parsed once, one grouped scan answers every account, and all owned (account, record) pairs are gathered and decrypted in one pass.  (*result)[a] is what
// decrypt_strings / balance returns for accounts[a]; no account gives an empty list.
inline Result<std::vector<FoundRecords>> decrypt_strings_many(const RecordBatch& batch, const std::vector<Account>& accounts) {
  std::vector<FoundRecords> out;
  if (accounts.empty()) return {std::move(out), Error{0}};
  std::vector<uint8_t> vks, axs;
  for (const auto& a : accounts) { vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  std::vector<aleo_mi355x_found*> f(accounts.size(), nullptr);
  int32_t rc = aleo_mi355x_records_decrypt_strings_many(f.data(), batch.text(), batch.offsets(), batch.size(), vks.data(), axs.data(), accounts.size());
  if (rc) return {std::nullopt, Error{rc}};
  out.reserve(f.size());
  for (aleo_mi355x_found* p : f) out.emplace_back(p);
  return {std::move(out), Error{0}};
}
inline Result<std::vector<Balance>> balances(const RecordBatch& batch, const std::vector<Account>& accounts) {
  auto found = decrypt_strings_many(batch, accounts);
  if (!found.is_ok()) return {std::nullopt, found.error};
  std::vector<Balance> out;
  for (const FoundRecords& f : *found.value) {
    if (f.unparsed()) { auto r = RecordCiphertext::from_string(batch.string(f.first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
    Balance b{0, {}};
    for (size_t k = 0; k < f.size(); ++k) { b.indices.push_back(f.index()[k]); if (f.status()[k] == 0) b.microcredits += f.microcredits()[k]; }
    out.push_back(std::move(b));
  }
  return {std::move(out), Error{0}};
}

// ---- serial numbers: which of the found records are unspent (rust/src/api/blocking.rs:277-278; aleo_mi355x_records_serial_numbers) ------------------------------
// What get_unspent_records is handed is a private key: sk_sig for the serial numbers, the view key and the address for the search.
// ---- account signatures (aleo_mi355x_signature_*, aleo_mi355x_signatures_verify: the reference's Signature::sign / verify, wasm/src/account/signature.rs:37-48) ----
// 128 bytes: challenge | response | pk_sig.x | pr_sig.x; as a string "sign1…"
struct Signature {
  uint8_t bytes[128];
  static Result<Signature> from_string(const std::string& s) {
    Signature g; int32_t rc = aleo_mi355x_signature_from_string(g.bytes, s.c_str());
    if (rc) return {std::nullopt, Error{rc}};
    return {g, Error{0}};
  }
  std::string to_string() const { char out[256]; return aleo_mi355x_signature_to_string(out, sizeof out, bytes) ? std::string() : std::string(out); }
};
// The signature of a message under the account of an "APrivateKey1…" string.  The nonce comes from seed32 alone: never use a seed for two messages.
inline Result<Signature> sign(const std::string& private_key, const void* message, size_t len, const uint8_t* seed32) {
  Signature g; int32_t rc = aleo_mi355x_signature_sign(g.bytes, private_key.c_str(), message, len, seed32);
  if (rc) return {std::nullopt, Error{rc}};
  return {g, Error{0}};
}
// Many signatures in one call (aleo_mi355x_signatures_sign): signatures[i] is sign(key i, message i, seed i) and flags[i] 0 — or zeros and 3 where the message is
// over the cap.  private_keys: one "APrivateKey1…" string for all messages, or one per message; seeds32: one row of 32 bytes per message, no two equal (the
// call refuses them: never use a seed for two messages).  Batches of aleo_mi355x_min_sign() and more run on the GPU, one signature per lane.
struct SignedBatch { std::vector<Signature> signatures; std::vector<uint8_t> flags; };
inline Result<SignedBatch> sign_many(const std::vector<std::string>& private_keys, const std::vector<std::string>& messages, const uint8_t* seeds32, bool host = false) {
  const size_t n = messages.size();
  if (private_keys.size() != n && private_keys.size() != 1) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  std::vector<uint8_t> keys(32 * private_keys.size()); std::vector<uint64_t> off(n + 1, 0); std::string text;
  for (size_t i = 0; i < private_keys.size(); ++i) if (int32_t rc = aleo_mi355x_private_key_seed(keys.data() + 32 * i, private_keys[i].c_str())) return {std::nullopt, Error{rc}};
  for (size_t i = 0; i < n; ++i) { text += messages[i]; off[i + 1] = text.size(); }
  SignedBatch out; out.signatures.resize(n); out.flags.assign(n, 0);
  static_assert(sizeof(Signature) == 128, "rows of 128 bytes");
  const size_t stride = private_keys.size() == n && n != 1 ? 32 : 0;
  int32_t rc = (host ? aleo_mi355x_signatures_sign_host : aleo_mi355x_signatures_sign)(out.signatures.data(), out.flags.data(), keys.data(), stride, text.data(), off.data(), seeds32, n);
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
// flags[i]: 0 signature i verifies under its address over message i, 1 it does not, 3 it is no signature.  addresses: one for all, or one per signature.
// Batches of aleo_mi355x_min_signatures() and more run on the GPU, one signature per lane.
inline Result<std::vector<uint8_t>> verify_many(const std::vector<Signature>& signatures, const std::vector<Address>& addresses, const std::vector<std::string>& messages, bool host = false) {
  const size_t n = signatures.size();
  if (messages.size() != n || (addresses.size() != n && addresses.size() != 1)) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  std::vector<uint8_t> flags(n), sg(128 * n), ax(32 * addresses.size()); std::vector<uint64_t> off(n + 1, 0); std::string text;
  for (size_t i = 0; i < n; ++i) { std::memcpy(sg.data() + 128 * i, signatures[i].bytes, 128); text += messages[i]; off[i + 1] = text.size(); }
  for (size_t i = 0; i < addresses.size(); ++i) std::memcpy(ax.data() + 32 * i, addresses[i].x, 32);
  const size_t stride = addresses.size() == n && n != 1 ? 32 : 0;
  int32_t rc = (host ? aleo_mi355x_signatures_verify_host : aleo_mi355x_signatures_verify)(flags.data(), sg.data(), ax.data(), stride, text.data(), off.data(), n);
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(flags), Error{0}};
}
// Signature::verify(address, message): one signature, on the calling thread
inline bool verify(const Signature& signature, const Address& address, const void* message, size_t len) {
  uint8_t flag = 1; const uint64_t off[2] = {0, len};
  return aleo_mi355x_signatures_verify_host(&flag, signature.bytes, address.x, 0, message, off, 1) == 0 && flag == 0;
}

// private_key: the string the account was made from (empty when it was put together from its parts: such an account verifies and cannot sign)
struct PrivateAccount {
  uint8_t sk_sig[32]; ViewKey view_key; Address address; std::string private_key;
  Result<Signature> sign(const void* message, size_t len, const uint8_t* seed32) const {
    if (private_key.empty()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    return aleo_mi355x::sign(private_key, message, len, seed32);
  }
  Result<SignedBatch> sign_many(const std::vector<std::string>& messages, const uint8_t* seeds32, bool host = false) const {
    if (private_key.empty()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    return aleo_mi355x::sign_many({private_key}, messages, seeds32, host);
  }
  bool verify(const void* message, size_t len, const Signature& signature) const { return aleo_mi355x::verify(signature, address, message, len); }
  // PrivateKey.fromPrivateKeyCiphertext / toCiphertext: account_from_ciphertext and account_to_ciphertext below (private key ciphertexts)
  static inline Result<PrivateAccount> from_ciphertext(const std::string& ciphertext, const std::string& secret);
  inline Result<std::string> to_ciphertext(const std::string& secret, const uint8_t* nonce32) const;
};
inline Result<PrivateAccount> account_from_private_key(const std::string& private_key) {
  PrivateAccount a; a.private_key = private_key;
  int32_t rc = aleo_mi355x_account_from_private_key(private_key.c_str(), a.sk_sig, a.view_key.scalar, a.address.x);
  if (rc) return {std::nullopt, Error{rc}};
  return {a, Error{0}};
}

// ---- accounts in batches (aleo_mi355x_accounts_derive, _accounts_search): wasm/src/account/private_key.rs:38-86, sdk/src/account.ts:82 ------------------------------
// A seed is the 32 bytes an "APrivateKey1…" string holds: a canonical little-endian field element.
using KeySeed = std::array<uint8_t, 32>;
inline Result<std::string> private_key_from_seed(const KeySeed& seed) {
  char out[64];
  int32_t rc = aleo_mi355x_private_key_from_seed(out, sizeof out, seed.data());
  if (rc) return {std::nullopt, Error{rc}};
  return {std::string(out), Error{0}};
}
inline Result<KeySeed> private_key_seed(const std::string& private_key) {
  KeySeed s;
  int32_t rc = aleo_mi355x_private_key_seed(s.data(), private_key.c_str());
  if (rc) return {std::nullopt, Error{rc}};
  return {s, Error{0}};
}
// from_seed_unchecked's reduction of 32 arbitrary bytes mod r (UNPINNED for a value not below r)
inline KeySeed seed_from_bytes(const uint8_t* bytes32) { KeySeed s; (void)aleo_mi355x_seed_from_bytes(s.data(), bytes32); return s; }
inline std::string view_key_to_string(const ViewKey& v) { char out[64] = {0}; (void)aleo_mi355x_view_key_to_string(out, sizeof out, v.scalar); return out; }
// The accounts of n seeds in one call (host: on the calling thread), with their private key strings; a seed that is not a canonical field element fails the call.
// addresses (optional): the n "aleo1…" strings, made where the accounts are.
inline Result<std::vector<PrivateAccount>> derive_accounts(const std::vector<KeySeed>& seeds, bool host = false, std::vector<std::string>* addresses = nullptr) {
  const size_t n = seeds.size();
  std::vector<uint8_t> in(32 * n), sk(32 * n), vk(32 * n), ax(32 * n), flags(n); std::vector<char> text(addresses ? 63 * n : 0);
  for (size_t i = 0; i < n; ++i) std::memcpy(in.data() + 32 * i, seeds[i].data(), 32);
  int32_t rc = (host ? aleo_mi355x_accounts_derive_host : aleo_mi355x_accounts_derive)(in.data(), n, sk.data(), vk.data(), ax.data(), addresses ? text.data() : nullptr, flags.data());
  if (rc) return {std::nullopt, Error{rc}};
  std::vector<PrivateAccount> out(n);
  if (addresses) addresses->clear();
  for (size_t i = 0; i < n; ++i) {
    if (flags[i]) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
    std::memcpy(out[i].sk_sig, sk.data() + 32 * i, 32); std::memcpy(out[i].view_key.scalar, vk.data() + 32 * i, 32); std::memcpy(out[i].address.x, ax.data() + 32 * i, 32);
    auto key = private_key_from_seed(seeds[i]);
    if (!key.is_ok()) return {std::nullopt, key.error};
    out[i].private_key = *key.value;
    if (addresses) addresses->emplace_back(text.data() + 63 * i, 63);
  }
  return {std::move(out), Error{0}};
}
// ... of n "APrivateKey1…" strings: decoded on the host, derived in one call
inline Result<std::vector<PrivateAccount>> accounts_from_private_keys(const std::vector<std::string>& keys, bool host = false) {
  std::vector<KeySeed> seeds;
  for (const auto& k : keys) { auto s = private_key_seed(k); if (!s.is_ok()) return {std::nullopt, s.error}; seeds.push_back(*s.value); }
  return derive_accounts(seeds, host);
}
// `new Account({seed})` of the reference's SDK: the 32 bytes reduced mod r, then the account, on the calling thread
inline Result<PrivateAccount> account_from_seed(const uint8_t* bytes32) {
  auto r = derive_accounts({seed_from_bytes(bytes32)}, true);
  if (!r.is_ok()) return {std::nullopt, r.error};
  return {(*r.value)[0], Error{0}};
}
// ---- private key ciphertexts (aleo_mi355x_private_key_encrypt, _decrypt, _private_keys_open): wasm/src/account/private_key_ciphertext.rs:39-73 -------------------------
// PrivateKeyCiphertext.encryptPrivateKey: the "ciphertext1…" string of an "APrivateKey1…" string under a secret (any bytes).  nonce32: a canonical field element the
// caller draws uniformly (aleo_mi355x_fr_random under 32 fresh bytes): a repeated nonce repeats the string.
inline Result<std::string> encrypt_private_key(const std::string& private_key, const std::string& secret, const uint8_t* nonce32) {
  char out[176];
  int32_t rc = aleo_mi355x_private_key_encrypt(out, sizeof out, private_key.c_str(), secret.data(), secret.size(), nonce32);
  if (rc) return {std::nullopt, Error{rc}};
  return {std::string(out), Error{0}};
}
// PrivateKeyCiphertext.decryptToPrivateKey: ALEO_MI355X_ERR_NOT_OWNER where the ciphertext does not decrypt under this secret, ERR_BAD_ARG for what is no ciphertext
inline Result<std::string> decrypt_private_key(const std::string& ciphertext, const std::string& secret) {
  char out[64];
  int32_t rc = aleo_mi355x_private_key_decrypt(out, sizeof out, ciphertext.c_str(), secret.data(), secret.size());
  if (rc) return {std::nullopt, Error{rc}};
  return {std::string(out), Error{0}};
}
// n (ciphertext, secret) pairs opened in one call (host: on the calling thread): accounts[i] with its private key string where flags[i] is 0; flags[i] 1 where the
// ciphertext does not decrypt under its secret, 3 where it is no ciphertext string — accounts[i] is then empty (no private key, zero rows).
struct OpenedKeys { std::vector<PrivateAccount> accounts; std::vector<uint8_t> flags; };
inline Result<OpenedKeys> open_private_keys(const std::vector<std::string>& ciphertexts, const std::vector<std::string>& secrets, bool host = false) {
  if (ciphertexts.size() != secrets.size()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  const size_t n = ciphertexts.size();
  std::string text, sec; std::vector<uint64_t> off(n + 1, 0), soff(n + 1, 0);
  for (size_t i = 0; i < n; ++i) { text += ciphertexts[i]; sec += secrets[i]; off[i + 1] = text.size(); soff[i + 1] = sec.size(); }
  std::vector<uint8_t> seeds(32 * n), sk(32 * n), vk(32 * n), ax(32 * n);
  OpenedKeys out; out.accounts.resize(n); out.flags.assign(n, 0);
  int32_t rc = (host ? aleo_mi355x_private_keys_open_host : aleo_mi355x_private_keys_open)(text.data(), off.data(), sec.data(), soff.data(), n, seeds.data(), sk.data(), vk.data(), ax.data(),
                                                                                          nullptr, out.flags.data());
  if (rc) return {std::nullopt, Error{rc}};
  for (size_t i = 0; i < n; ++i) {
    PrivateAccount& a = out.accounts[i];
    std::memcpy(a.sk_sig, sk.data() + 32 * i, 32); std::memcpy(a.view_key.scalar, vk.data() + 32 * i, 32); std::memcpy(a.address.x, ax.data() + 32 * i, 32);
    if (out.flags[i]) continue;
    KeySeed seed; std::memcpy(seed.data(), seeds.data() + 32 * i, 32);
    auto key = private_key_from_seed(seed);
    if (!key.is_ok()) return {std::nullopt, key.error};
    a.private_key = *key.value;
  }
  return {std::move(out), Error{0}};
}
// PrivateKey.fromPrivateKeyCiphertext and PrivateKey.toCiphertext (wasm/src/account/private_key.rs:113-130) for a PrivateAccount
inline Result<PrivateAccount> account_from_ciphertext(const std::string& ciphertext, const std::string& secret) {
  auto key = decrypt_private_key(ciphertext, secret);
  if (!key.is_ok()) return {std::nullopt, key.error};
  return account_from_private_key(*key.value);
}
inline Result<std::string> account_to_ciphertext(const PrivateAccount& account, const std::string& secret, const uint8_t* nonce32) {
  if (account.private_key.empty()) return {std::nullopt, Error{ALEO_MI355X_ERR_BAD_ARG}};
  return encrypt_private_key(account.private_key, secret, nonce32);
}
inline Result<PrivateAccount> PrivateAccount::from_ciphertext(const std::string& ciphertext, const std::string& secret) { return account_from_ciphertext(ciphertext, secret); }
inline Result<std::string> PrivateAccount::to_ciphertext(const std::string& secret, const uint8_t* nonce32) const { return account_to_ciphertext(*this, secret, nonce32); }

// The first max_hits candidates of [first, first + count) under a 32-byte master seed whose address begins with "aleo1" + prefix (0 to 12 characters of the
// bech32 alphabet), as accounts with their private key strings; index: their positions; next: where to resume.  Candidate i's private-key seed is element i of the
// ChaCha20 stream under the master seed, which regenerates every key found: keep it secret.
struct AccountSearch { std::vector<PrivateAccount> accounts; std::vector<uint64_t> index; uint64_t next = 0; };
inline Result<AccountSearch> search_accounts(const uint8_t* master32, const std::string& prefix, uint64_t first, uint64_t count, size_t max_hits = 1, bool host = false) {
  AccountSearch out; out.index.resize(max_hits ? max_hits : 1);
  std::vector<uint8_t> seeds(32 * out.index.size()); size_t n = 0;
  int32_t rc = (host ? aleo_mi355x_accounts_search_host : aleo_mi355x_accounts_search)(master32, first, count, prefix.c_str(), max_hits, out.index.data(), seeds.data(), &n, &out.next);
  if (rc) return {std::nullopt, Error{rc}};
  out.index.resize(n);
  std::vector<KeySeed> found(n);
  for (size_t i = 0; i < n; ++i) std::memcpy(found[i].data(), seeds.data() + 32 * i, 32);
  auto accts = derive_accounts(found, true);
  if (!accts.is_ok()) return {std::nullopt, accts.error};
  out.accounts = std::move(*accts.value);
  return {std::move(out), Error{0}};
}
// n serial numbers (32 canonical little-endian bytes each) and flags (0 computed, 2 refused: a zero row, the record is dropped as upstream's `.ok()?` drops it) of n
// commitments under one sk_sig
struct SerialNumbers { std::vector<uint8_t> rows, flags; const uint8_t* row(size_t i) const { return rows.data() + 32 * i; } size_t size() const { return flags.size(); } };
inline Result<SerialNumbers> serial_numbers(const uint8_t* commitments32, size_t n, const uint8_t* sk_sig32) {
  SerialNumbers out{std::vector<uint8_t>(32 * n), std::vector<uint8_t>(n)};
  int32_t rc = aleo_mi355x_records_serial_numbers(out.rows.data(), out.flags.data(), commitments32, n, sk_sig32);
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
// ... of the records a decrypt_strings result holds; commitments32: those of ALL n strings the result was made from
inline Result<SerialNumbers> found_serial_numbers(const FoundRecords& found, const uint8_t* commitments32, size_t n, const uint8_t* sk_sig32) {
  SerialNumbers out{std::vector<uint8_t>(32 * found.size()), std::vector<uint8_t>(found.size())};
  int32_t rc = aleo_mi355x_found_serial_numbers(found.handle(), commitments32, n, sk_sig32, out.rows.data(), out.flags.data());
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
// to_commitment(program_id, record_name) of a record's plaintext, from its "record1…" string and its decrypted fields in randomizer order; the checksum of the ciphertext
inline Result<std::array<uint8_t, 32>> record_commitment(const std::string& record1, const uint8_t* plain_fields, size_t n_fields, const std::string& program_id, const std::string& record_name) {
  std::array<uint8_t, 32> out;
  int32_t rc = aleo_mi355x_record_commitment(out.data(), record1.c_str(), plain_fields, n_fields, program_id.c_str(), record_name.c_str());
  if (rc) return {std::nullopt, Error{rc}};
  return {out, Error{0}};
}
inline Result<std::array<uint8_t, 32>> record_checksum(const std::string& record1) {
  std::array<uint8_t, 32> out;
  int32_t rc = aleo_mi355x_record_checksum(out.data(), record1.c_str());
  if (rc) return {std::nullopt, Error{rc}};
  return {out, Error{0}};
}

// The unspent records of several accounts (at most 64) over the same batch in ONE aleo_mi355x_records_unspent_strings_many call: the reference's
// get_unspent_records behind the fetch of the blocks.  commitments32: those of all strings of the batch (batch.size() x 32 bytes); spent32: n_spent spent serial
// numbers in any order (null with n_spent = 0: every owned record that decrypts is kept).  (*result)[a] holds accounts[a]'s records with status 0 whose serial
// number computes and is not spent, their serials() and what it owned().  A string that does not parse fails the call as balance fails.
inline Result<std::vector<FoundRecords>> unspent_strings_many(const RecordBatch& batch, const uint8_t* commitments32, const std::vector<PrivateAccount>& accounts,
                                                              const uint8_t* spent32 = nullptr, size_t n_spent = 0) {
  std::vector<FoundRecords> out;
  if (accounts.empty()) return {std::move(out), Error{0}};
  std::vector<uint8_t> sks, vks, axs;
  for (const auto& a : accounts) { sks.insert(sks.end(), a.sk_sig, a.sk_sig + 32); vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  std::vector<aleo_mi355x_found*> f(accounts.size(), nullptr);
  int32_t rc = aleo_mi355x_records_unspent_strings_many(f.data(), batch.text(), batch.offsets(), batch.size(), commitments32, sks.data(), vks.data(), axs.data(), accounts.size(), spent32, n_spent);
  if (rc) return {std::nullopt, Error{rc}};
  out.reserve(f.size());
  for (aleo_mi355x_found* p : f) out.emplace_back(p);
  if (out[0].unparsed()) { auto r = RecordCiphertext::from_string(batch.string(out[0].first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  return {std::move(out), Error{0}};
}
inline Result<FoundRecords> unspent_strings(const RecordBatch& batch, const uint8_t* commitments32, const PrivateAccount& account, const uint8_t* spent32 = nullptr, size_t n_spent = 0) {
  aleo_mi355x_found* f = nullptr;
  int32_t rc = aleo_mi355x_records_unspent_strings(&f, batch.text(), batch.offsets(), batch.size(), commitments32, account.sk_sig, account.view_key.scalar, account.address.x, spent32, n_spent);
  if (rc) return {std::nullopt, Error{rc}};
  FoundRecords found(f);
  if (found.unparsed()) { auto r = RecordCiphertext::from_string(batch.string(found.first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  return {std::move(found), Error{0}};
}

// ---- unspent records from the strings alone (sdk/src/aleo_network_client.ts:365-373; aleo_mi355x_records_unspent_named) ------------------------------------------
// The commitments (32 canonical little-endian bytes each) and flags of the records a result holds, under (program_id, record_name), from the batch it was made from:
// 0 computed; 4 refused where record_commitment refuses the record; a status that is not 0 is the flag.  A refused row is zeros.
struct Commitments { std::vector<uint8_t> rows, flags; const uint8_t* row(size_t i) const { return rows.data() + 32 * i; } size_t size() const { return flags.size(); } };
inline Result<Commitments> found_commitments(const RecordBatch& batch, const FoundRecords& found, const std::string& program_id, const std::string& record_name) {
  Commitments out{std::vector<uint8_t>(32 * found.size()), std::vector<uint8_t>(found.size())};
  int32_t rc = aleo_mi355x_records_commitments_found(out.rows.data(), out.flags.data(), found.handle(), batch.text(), batch.offsets(), batch.size(), program_id.c_str(), record_name.c_str());
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
// unspent_strings_many for a caller that has no commitments: every owned record's is computed from its plaintext under (program_id, record_name) inside the call.
// (*result)[a] holds accounts[a]'s unspent records with their serials(), commitments() and what it owned().
inline Result<std::vector<FoundRecords>> unspent_named_many(const RecordBatch& batch, const std::string& program_id, const std::string& record_name, const std::vector<PrivateAccount>& accounts,
                                                            const uint8_t* spent32 = nullptr, size_t n_spent = 0) {
  std::vector<FoundRecords> out;
  if (accounts.empty()) return {std::move(out), Error{0}};
  std::vector<uint8_t> sks, vks, axs;
  for (const auto& a : accounts) { sks.insert(sks.end(), a.sk_sig, a.sk_sig + 32); vks.insert(vks.end(), a.view_key.scalar, a.view_key.scalar + 32); axs.insert(axs.end(), a.address.x, a.address.x + 32); }
  std::vector<aleo_mi355x_found*> f(accounts.size(), nullptr);
  int32_t rc = aleo_mi355x_records_unspent_named_many(f.data(), batch.text(), batch.offsets(), batch.size(), program_id.c_str(), record_name.c_str(), sks.data(), vks.data(), axs.data(), accounts.size(), spent32, n_spent);
  if (rc) return {std::nullopt, Error{rc}};
  out.reserve(f.size());
  for (aleo_mi355x_found* p : f) out.emplace_back(p);
  if (out[0].unparsed()) { auto r = RecordCiphertext::from_string(batch.string(out[0].first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  return {std::move(out), Error{0}};
}
inline Result<FoundRecords> unspent_named(const RecordBatch& batch, const std::string& program_id, const std::string& record_name, const PrivateAccount& account, const uint8_t* spent32 = nullptr,
                                          size_t n_spent = 0) {
  aleo_mi355x_found* f = nullptr;
  int32_t rc = aleo_mi355x_records_unspent_named(&f, batch.text(), batch.offsets(), batch.size(), program_id.c_str(), record_name.c_str(), account.sk_sig, account.view_key.scalar, account.address.x, spent32, n_spent);
  if (rc) return {std::nullopt, Error{rc}};
  FoundRecords found(f);
  if (found.unparsed()) { auto r = RecordCiphertext::from_string(batch.string(found.first_unparsed())); return {std::nullopt, r.is_ok() ? Error{ALEO_MI355X_ERR_BAD_ARG} : r.error}; }
  return {std::move(found), Error{0}};
}

// ---- record plaintext strings (wasm/src/record/record_plaintext.rs:45-82; aleo_mi355x_plaintexts_serial_numbers) ---------------------------------------------------
// A batch of RecordPlaintext strings (RecordBatch::from_strings takes any strings): per string the commitment under (program_id, record_name), the microcredits
// and, from plaintext_serial_numbers, the serial number under the account's sk_sig.  flags: 0 computed (and not in the spent set); 1 computed and spent; 2 the
// serial number is refused; 3 not a record plaintext.  A row that is not computed is zeros.
struct PlaintextRows {
  std::vector<uint8_t> serials, commitments, flags; std::vector<uint64_t> microcredits;
  const uint8_t* serial(size_t i) const { return serials.data() + 32 * i; }
  const uint8_t* commitment(size_t i) const { return commitments.data() + 32 * i; }
  size_t size() const { return flags.size(); }
};
inline Result<PlaintextRows> plaintext_commitments(const RecordBatch& batch, const std::string& program_id, const std::string& record_name) {
  const size_t n = batch.size();
  PlaintextRows out{{}, std::vector<uint8_t>(32 * n), std::vector<uint8_t>(n), std::vector<uint64_t>(n)};
  int32_t rc = aleo_mi355x_plaintexts_commitments(out.commitments.data(), out.microcredits.data(), out.flags.data(), batch.text(), batch.offsets(), n, program_id.c_str(), record_name.c_str());
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
inline Result<PlaintextRows> plaintext_serial_numbers(const RecordBatch& batch, const std::string& program_id, const std::string& record_name, const uint8_t* sk_sig32,
                                                      const uint8_t* spent32 = nullptr, size_t n_spent = 0) {
  const size_t n = batch.size();
  PlaintextRows out{std::vector<uint8_t>(32 * n), std::vector<uint8_t>(32 * n), std::vector<uint8_t>(n), std::vector<uint64_t>(n)};
  int32_t rc = aleo_mi355x_plaintexts_serial_numbers(out.serials.data(), out.commitments.data(), out.microcredits.data(), out.flags.data(), batch.text(), batch.offsets(), n, program_id.c_str(),
                                                     record_name.c_str(), sk_sig32, spent32, n_spent);
  if (rc) return {std::nullopt, Error{rc}};
  return {std::move(out), Error{0}};
}
// the indices of the strings whose serial number computes and is not spent: "which of the plaintexts I hold are still unspent?"
inline Result<std::vector<size_t>> plaintexts_unspent(const RecordBatch& batch, const std::string& program_id, const std::string& record_name, const PrivateAccount& account,
                                                      const uint8_t* spent32 = nullptr, size_t n_spent = 0) {
  auto rows = plaintext_serial_numbers(batch, program_id, record_name, account.sk_sig, spent32, n_spent);
  if (!rows.is_ok()) return {std::nullopt, rows.error};
  std::vector<size_t> keep;
  for (size_t i = 0; i < rows.value->size(); ++i) if (!rows.value->flags[i]) keep.push_back(i);
  return {std::move(keep), Error{0}};
}
// RecordPlaintext.fromString(..).microcredits(): refused unless the string is a record plaintext whose owner, nonce and group values are points of the subgroup
inline Result<uint64_t> plaintext_microcredits(const std::string& plaintext) {
  uint64_t mc = 0;
  int32_t rc = aleo_mi355x_record_plaintext_parse(plaintext.c_str(), nullptr, nullptr, nullptr, &mc);
  if (rc) return {std::nullopt, Error{rc}};
  return {mc, Error{0}};
}

// ---- encryption: record plaintexts to record1… strings (rust/src/program/execute.rs:74,177, transfer.rs:99-106; aleo_mi355x_records_encrypt) --------------------------
// Record::encrypt(randomizer) of one plaintext on the host: randomizer32 a scalar below the subgroup order, 32 little-endian bytes.  x(randomizer G) must be the
// string's _nonce — or, with set_nonce, replaces it.
inline Result<RecordCiphertext> encrypt_record(const RecordPlaintext& plaintext, const uint8_t* randomizer32, bool set_nonce = false) {
  std::string buf(4096, '\0'); size_t len = buf.size();
  const int32_t mode = set_nonce ? ALEO_MI355X_ENCRYPT_SET_NONCE : 0;
  int32_t rc = aleo_mi355x_record_encrypt(plaintext.to_string().c_str(), randomizer32, mode, &buf[0], &len);
  if (rc == ALEO_MI355X_ERR_BAD_ARG && len + 1 > buf.size()) { buf.assign(len + 1, '\0'); len = buf.size(); rc = aleo_mi355x_record_encrypt(plaintext.to_string().c_str(), randomizer32, mode, &buf[0], &len); }      // too short, not refused: a refusal leaves len as it was
  if (rc) return {std::nullopt, Error{rc}};
  buf.resize(len); return RecordCiphertext::from_string(buf);
}
// n plaintext strings under n randomizers (n x 32 bytes) in one call: the record1… strings as a RecordBatch that find_owned, decrypt_strings and the rest take as it
// stands, flags (0 encrypted; 1 x(r G) is not the string's nonce; 2 the randomizer is not below the subgroup order or the owner is no point of the subgroup; 3 not
// a record plaintext — the row's string is empty and its key zeros) and the record view keys' x, 32 bytes each.  Equal randomizers are not looked for.
struct EncryptedRecords { RecordBatch batch; std::vector<uint8_t> flags, rvk; const uint8_t* record_view_key_x(size_t i) const { return rvk.data() + 32 * i; } };
inline Result<EncryptedRecords> encrypt_records(const RecordBatch& plaintexts, const uint8_t* randomizers32, bool set_nonce = false, bool host = false) {
  const size_t n = plaintexts.size();
  aleo_mi355x_encrypted* e = nullptr;
  int32_t rc = (host ? aleo_mi355x_records_encrypt_host : aleo_mi355x_records_encrypt)(&e, plaintexts.text(), plaintexts.offsets(), n, randomizers32, set_nonce ? ALEO_MI355X_ENCRYPT_SET_NONCE : 0);
  if (rc) return {std::nullopt, Error{rc}};
  EncryptedRecords out{RecordBatch(std::vector<std::string>{}), {}, {}};
  const char* text = aleo_mi355x_encrypted_text(e); const uint64_t* off = aleo_mi355x_encrypted_offsets(e);
  for (size_t i = 0; i < n; ++i) out.batch.push_back(std::string(text + off[i], (size_t)(off[i + 1] - off[i])));
  out.flags.assign(aleo_mi355x_encrypted_flags(e), aleo_mi355x_encrypted_flags(e) + n);
  out.rvk.assign(aleo_mi355x_encrypted_rvk(e), aleo_mi355x_encrypted_rvk(e) + 32 * n);
  aleo_mi355x_encrypted_free(e);
  return {std::move(out), Error{0}};
}

}  // namespace aleo_mi355x
