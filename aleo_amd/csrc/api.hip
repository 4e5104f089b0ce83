// api.hip — the C ABI of libaleo_mi355x.so (include/aleo_mi355x.h): argument checking, host<->HBM staging and the host-side tails of the MSM, KZG,
// field, transform, prover and self-test entry points.  Devices and slots: device.hip; base sets: bases.hip; several devices: sharded.hip.  Kernels live in msm_sort.hip / msm.hip / g1_setup.hip / ntt.hip / frops.hip / fr_spmv.hip / fr_divide.hip / ahp_kernels.hip.
#include "entry.h"
#include "frops.h"
#include "g2.h"
#include "host_field.hpp"
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <thread>

namespace aleo_mi355x {

thread_local MsmTiming g_last_msm;

static void jacobian_to_affine104(void* out104, const uint64_t* jac18) {
  uint8_t* o = (uint8_t*)out104; std::memset(o, 0, 104);
  bool inf = true; for (int i = 12; i < 18; ++i) if (jac18[i]) inf = false;
  if (inf) { o[96] = 1; host::HFq one = host::HFq::one(); std::memcpy(o + 48, one.l, 48); return; }  // Affine::zero() = (0, 1, true)
  std::memcpy(o, jac18, 96);   // results are normalised: z == 1
}

void jacobian_rows_to_affine104(void* out104, const uint64_t* jac18, size_t k) {
  for (size_t q = 0; q < k; ++q) jacobian_to_affine104((uint8_t*)out104 + 104 * q, jac18 + 18 * q);
}

// *_device entry points that only enqueue work.  On the caller's stream they return without synchronising (the caller orders
// its own work there).  With stream == NULL they run on the serving slot's stream, which the caller cannot order anything
// against — a following call may be served by another slot — so the work is complete when they return.
template <class F> static int32_t enqueue_on_slot(void* stream, F&& f) {
  Slot sl; if (sl.rc) return sl.rc;
  hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
  if (int32_t rc = f(sl.c, s)) return rc;
  if (!stream) HIPCHK(hipStreamSynchronize(s));
  return ALEO_MI355X_OK;
}
// the whole of such an entry point whose arguments need one check (refused before a slot is taken; `why`: the error text, when it has one)
template <class F> static int32_t device_entry(bool bad_args, const char* why, void* stream, F&& f) {
  return guarded([&] {
    if (bad_args) return why ? bad_arg(why) : ALEO_MI355X_ERR_BAD_ARG;
    return enqueue_on_slot(stream, f);
  });
}

namespace {      // aleo_mi355x_selftest_host_inverse
template <int N> void inverse_selftest(uint32_t count, uint64_t seed, uint32_t* failures, double* ns) {
  using F = host::HFp<N>; using Pm = host::HParams<N>;
  std::vector<F> v;
  auto from_canon = [](const uint64_t* c) { F x; std::memcpy(x.l, c, sizeof x.l); return x; };
  { uint64_t e[N]; std::memset(e, 0, sizeof e); v.push_back(from_canon(e)); e[0] = 1; v.push_back(from_canon(e)); e[0] = 2; v.push_back(from_canon(e));
    std::memcpy(e, Pm::P, sizeof e); e[0] -= 1; v.push_back(from_canon(e)); e[0] -= 1; v.push_back(from_canon(e)); }
  uint64_t st = seed * 0x9e3779b97f4a7c15ull + N;
  auto next = [&]() { st += 0x9e3779b97f4a7c15ull; uint64_t z = st; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); };
  for (uint32_t i = 0; i < count; ++i) {
    F x; for (int k = 0; k < N; ++k) x.l[k] = next();
    x.l[N - 1] &= (1ull << (N == 4 ? 60 : 56)) - 1;        // below the modulus' top limb: a valid residue
    if (i % 7 == 3) { for (int k = 1; k < N; ++k) x.l[k] = 0; }      // short values too
    v.push_back(x);
  }
  std::vector<F> a(v.size()), b(v.size());
  auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < v.size(); ++i) a[i] = F::inv(v[i]);
  auto t1 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < v.size(); ++i) b[i] = F::inv_fermat(v[i]);
  auto t2 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < v.size(); ++i) {
    bool ok = a[i] == b[i];
    if (ok && !v[i].is_zero()) ok = F::mul(a[i], v[i]) == F::one();      // and it IS the inverse
    ok = ok && F::sqr(v[i]) == F::mul(v[i], v[i]) && F::sqr(a[i]) == F::mul(a[i], a[i]);      // the dedicated squaring against the product
    { host::Wide<N> w; w.set_sqr(v[i].l); host::Wide<N> u; u.set_mul(v[i].l, v[i].l); ok = ok && w.redc() == u.redc(); }
    if (!ok) ++*failures;
  }
  if (ns) { ns[0] = std::chrono::duration<double, std::nano>(t1 - t0).count() / v.size(); ns[1] = std::chrono::duration<double, std::nano>(t2 - t1).count() / v.size(); }
}
}  // namespace

int32_t strings_args_ok(const char* who, const char* text, const uint64_t* offsets, size_t n) {
  if (!n) return ALEO_MI355X_OK;
  if (!offsets) { g_last_error = std::string(who) + ": null buffer"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (offsets[0] != 0) { g_last_error = std::string(who) + ": offsets[0] is not 0"; return ALEO_MI355X_ERR_BAD_ARG; }
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) { g_last_error = std::string(who) + ": offsets decrease"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (offsets[n] && !text) { g_last_error = std::string(who) + ": null buffer"; return ALEO_MI355X_ERR_BAD_ARG; }
  return ALEO_MI355X_OK;
}

// ---- one prover round's commitments in one call -------------------------------------------------------------------
int32_t batch_args_ok(const void* out, const void* const* ptrs, const size_t* lens, size_t k) {
  if (k == 0) return ALEO_MI355X_OK;
  if (!out || !ptrs || !lens) return bad_arg("batch: null argument");
  for (size_t q = 0; q < k; ++q) if (!ptrs[q] && lens[q]) return bad_arg("batch: null vector with a non-zero length");
  return ALEO_MI355X_OK;
}
// the k results of a batch: result q is the MSM of vector q against the first lens[q] bases
static std::vector<MsmSeg> batch_segs(const void* const* d_ptrs, const size_t* lens, size_t k) {
  std::vector<MsmSeg> sg(k); for (size_t q = 0; q < k; ++q) { sg[q].d_ptr = d_ptrs[q]; sg[q].len = lens[q]; sg[q].out = (uint32_t)q; }
  return sg;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_msm_g1(void* out, const void* bases, size_t base_stride, const void* scalars, size_t n) {
  return guarded([&] {
    if (!out || ((!bases || !scalars) && n) || (base_stride != 104 && base_stride != 96)) return bad_arg("msm_g1: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<PinnedOwner> keep; PinnedBases pb;
    if (int32_t rc = one_shot_bases(sl.c, bases, base_stride, n, &keep, &pb)) return rc;
    return msm_host_scalars(sl.c, out, pb, scalars, n, false);
  });
}

int32_t aleo_mi355x_msm_g1_pinned(void* out, uint64_t handle, const void* scalars, size_t n) {
  return guarded([&] {
    if (!out || (!scalars && n)) return bad_arg("msm_g1_pinned: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    return msm_host_scalars(sl.c, out, fb.pb, scalars, n, false);
  });
}

int32_t aleo_mi355x_msm_g1_device(void* out, uint64_t handle, const void* d_scalars, size_t n, void* stream) {
  return guarded([&] {
    if (!out || (!d_scalars && n)) return bad_arg("msm_g1_device: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    return msm_run1_split(sl.c, (uint64_t*)out, fb.pb, d_scalars, n, false, s, false, nullptr);
  });
}

int32_t aleo_mi355x_msm_g1_device_sparse(void* out, uint64_t handle, const void* d_scalars, size_t n, void* stream) {
  return guarded([&] {
    if (!out || (!d_scalars && n)) return bad_arg("msm_g1_device_sparse: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    return msm_run1(sl.c, (uint64_t*)out, fb.pb, d_scalars, n, false, s, true);
  });
}

// VariableBase::msm::<G2Affine>: one-shot, host pointers (G2 appears in SRS setup and verifying keys, never in the prover's loop:
// no residency handle).  bases: snarkVM G2Affine rows, stride 200 (flag byte at 192) or 192.
int32_t aleo_mi355x_msm_g2(void* out_jac288, const void* bases, size_t base_stride, const void* scalars, size_t n) {
  return guarded([&] {
    if (!out_jac288 || ((!bases || !scalars) && n) || (base_stride != 200 && base_stride != 192)) return bad_arg("msm_g2: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    int32_t rc; const void* xy = nullptr; const uint8_t* d_inf = nullptr;
    if ((rc = one_shot_bases_g2(sl.c, bases, base_stride, n, &xy, &d_inf))) return rc;
    if ((rc = sl.c->scalars_stage.reserve((n ? n : 1) * 32))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(sl.c->scalars_stage.p, scalars, n * 32, hipMemcpyHostToDevice, sl.c->stream));
    return msm_g2_run(sl.c, (uint64_t*)out_jac288, xy, d_inf, sl.c->scalars_stage.p, n, sl.c->stream);
  });
}

int32_t aleo_mi355x_msm_g2_pinned(void* out_jac288, uint64_t handle, const void* scalars, size_t n) {
  return guarded([&] {
    if (!out_jac288 || (!scalars && n)) return bad_arg("msm_g2_pinned: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<PinnedG2> keep;
    { std::lock_guard<std::mutex> lk2(sl.d->mu); if (int32_t rch = handle_get(sl.d->g2_bases, handle, "unknown G2 bases handle", &keep)) return rch; }
    if (n > keep->n) return bad_arg("msm_g2_pinned: more scalars than pinned bases");
    int32_t rc;
    if ((rc = sl.c->scalars_stage.reserve((n ? n : 1) * 32))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(sl.c->scalars_stage.p, scalars, n * 32, hipMemcpyHostToDevice, sl.c->stream));
    return msm_g2_run(sl.c, (uint64_t*)out_jac288, keep->d_xy, keep->d_inf, sl.c->scalars_stage.p, n, sl.c->stream, keep->d_rows28);
  });
}

int32_t aleo_mi355x_g2_sum(void* out, const void* pts, size_t count) {
  return guarded([&] {
    if (!out || (!pts && count)) return ALEO_MI355X_ERR_BAD_ARG;
    return g2_sum_host((uint64_t*)out, (const uint64_t*)pts, count);
  });
}

int32_t aleo_mi355x_g1_sum(void* out, const void* pts, size_t count) {
  return guarded([&] {
    if (!out || (!pts && count)) return ALEO_MI355X_ERR_BAD_ARG;
    host::HXYZZ t = host::HXYZZ::infinity();
    for (size_t i = 0; i < count; ++i) t = host::hadd(t, host::hfrom_jacobian((const uint64_t*)pts + 18 * i));
    host::hstore_jacobian_normalized((uint64_t*)out, t);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_kzg_commit(void* out104, uint64_t handle, const void* coeffs, size_t n) {
  return guarded([&] {
    if (!out104 || (!coeffs && n)) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    uint64_t jac[18];
    int32_t rc = msm_host_scalars(sl.c, jac, fb.pb, coeffs, n, true);
    if (rc) return rc;
    jacobian_to_affine104(out104, jac);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_kzg_commit_device(void* out104, uint64_t handle, const void* d_coeffs, size_t n, void* stream) {
  return guarded([&] {
    if (!out104 || (!d_coeffs && n)) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    uint64_t jac[18];
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    int32_t rc = msm_run1(sl.c, jac, fb.pb, d_coeffs, n, true, s);
    if (rc) return rc;
    jacobian_to_affine104(out104, jac);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_msm_g1_batch_device(void* out_jac, uint64_t handle, const void* const* d_scalars, const size_t* lens, size_t k, void* stream) {
  return guarded([&] {
    int32_t rc = batch_args_ok(out_jac, d_scalars, lens, k); if (rc || !k) return rc;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    const std::vector<MsmSeg> sg = batch_segs(d_scalars, lens, k);
    MsmJob j; j.segs = sg.data(); j.nseg = (uint32_t)k; j.k = (uint32_t)k; j.mont = false;
    if (k >= (1u << 20)) return bad_arg("batch: too many vectors");
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    return msm_batch(sl.c, (uint64_t*)out_jac, fb.pb, j, s);
  });
}

int32_t aleo_mi355x_kzg_commit_batch_device(void* out104, uint64_t handle, const void* const* d_coeffs, const size_t* lens, size_t k, void* stream) {
  return guarded([&] {
    int32_t rc = batch_args_ok(out104, d_coeffs, lens, k); if (rc || !k) return rc;
    if (k >= (1u << 20)) return bad_arg("batch: too many vectors");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    std::vector<uint64_t> jac(18 * k);
    const std::vector<MsmSeg> sg = batch_segs(d_coeffs, lens, k);
    MsmJob j; j.segs = sg.data(); j.nseg = (uint32_t)k; j.k = (uint32_t)k; j.mont = true;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    if ((rc = msm_batch(sl.c, jac.data(), fb.pb, j, s))) return rc;
    jacobian_rows_to_affine104(out104, jac.data(), k);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_kzg_commit_batch(void* out104, uint64_t handle, const void* const* coeffs, const size_t* lens, size_t k) {
  return guarded([&] {
    int32_t rc = batch_args_ok(out104, coeffs, lens, k); if (rc || !k) return rc;
    if (k >= (1u << 20)) return bad_arg("batch: too many vectors");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    size_t total = 0; for (size_t q = 0; q < k; ++q) total += lens[q];
    if ((rc = sl.c->scalars_stage.reserve((total ? total : 1) * 32))) return rc;
    std::vector<const void*> dptr(k); size_t off = 0;
    for (size_t q = 0; q < k; ++q) {          // one staging buffer, k uploads queued back to back on the slot's stream
      dptr[q] = (const char*)sl.c->scalars_stage.p + off * 32;
      if (lens[q]) HIPCHK(hipMemcpyAsync((char*)sl.c->scalars_stage.p + off * 32, coeffs[q], lens[q] * 32, hipMemcpyHostToDevice, sl.c->stream));
      off += lens[q];
    }
    std::vector<uint64_t> jac(18 * k);
    const std::vector<MsmSeg> sg = batch_segs(dptr.data(), lens, k);
    MsmJob j; j.segs = sg.data(); j.nseg = (uint32_t)k; j.k = (uint32_t)k; j.mont = true;
    if ((rc = msm_batch(sl.c, jac.data(), fb.pb, j, sl.c->stream))) return rc;
    jacobian_rows_to_affine104(out104, jac.data(), k);
    return ALEO_MI355X_OK;
  });
}

// SonicKZG10::commit shape: every commitment is a sum of segments (coefficient vector x base offset) over ONE pinned set.
// `stream`: the caller's, for scalars on the device; host scalars are staged on the slot's own (NULL).
static int32_t commit_segments(void* out104, size_t n_out, uint64_t handle, const aleo_mi355x_commit_segment* segs, size_t n_segs, bool host_scalars, void* stream, bool sparse = false) {
  Slot sl; if (sl.rc) return sl.rc;
  Ctx* c = sl.c; hipStream_t s = nullptr; if (int32_t rcs = pick_stream(c, stream, &s)) return rcs;
  if (!n_out) return ALEO_MI355X_OK;
  if (!out104 || (!segs && n_segs) || n_out >= (1u << 20) || n_segs >= (1u << 22)) return bad_arg("commit_segments: bad argument");
  FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
  std::vector<MsmSeg> sg(n_segs); size_t total = 0; int32_t rc;
  for (size_t q = 0; q < n_segs; ++q) {
    if ((!segs[q].scalars && segs[q].len) || segs[q].output >= n_out || segs[q].base_offset + segs[q].len > fb.pb.n) return bad_arg("commit_segments: segment out of range");
    sg[q].d_ptr = segs[q].scalars; sg[q].len = segs[q].len; sg[q].off = segs[q].base_offset; sg[q].out = segs[q].output; total += segs[q].len;
  }
  if (host_scalars) {          // one staging buffer, the uploads queued back to back on the slot's stream
    if ((rc = c->scalars_stage.reserve((total ? total : 1) * 32))) return rc;
    size_t off = 0;
    for (size_t q = 0; q < n_segs; ++q) {
      if (sg[q].len) HIPCHK(hipMemcpyAsync((char*)c->scalars_stage.p + off * 32, segs[q].scalars, sg[q].len * 32, hipMemcpyHostToDevice, s));
      sg[q].d_ptr = (const char*)c->scalars_stage.p + off * 32; off += sg[q].len;
    }
  }
  std::vector<uint64_t> jac(18 * n_out);
  MsmJob j; j.segs = sg.data(); j.nseg = (uint32_t)n_segs; j.k = (uint32_t)n_out; j.mont = true; j.sparse = sparse;
  if ((rc = msm_batch(c, jac.data(), fb.pb, j, s))) return rc;
  jacobian_rows_to_affine104(out104, jac.data(), n_out);
  return ALEO_MI355X_OK;
}

int32_t aleo_mi355x_kzg_commit_segments(void* out104, size_t n_out, uint64_t handle, const aleo_mi355x_commit_segment* segs, size_t n_segs) {
  return guarded([&] { return commit_segments(out104, n_out, handle, segs, n_segs, true, nullptr); });
}
int32_t aleo_mi355x_kzg_commit_segments_device(void* out104, size_t n_out, uint64_t handle, const aleo_mi355x_commit_segment* segs, size_t n_segs, void* stream) {
  return guarded([&] { return commit_segments(out104, n_out, handle, segs, n_segs, false, stream); });
}

int32_t aleo_mi355x_kzg_commit_segments_sparse_device(void* out104, size_t n_out, uint64_t handle, const aleo_mi355x_commit_segment* segs, size_t n_segs, void* stream) {
  return guarded([&] { return commit_segments(out104, n_out, handle, segs, n_segs, false, stream, true); });
}

int32_t aleo_mi355x_kzg_commit_hiding(void* out104, uint64_t h_powers, const void* coeffs, size_t n, uint64_t h_gamma, const void* blind, size_t m) {
  return guarded([&] {
    if (!out104 || (!coeffs && n) || (!blind && m)) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<PinnedOwner> kp, kg; PinnedBases pp, pg; int32_t rc;
    if ((rc = find_bases(sl.d, h_powers, &kp, &pp)) || (rc = find_bases(sl.d, h_gamma, &kg, &pg))) return rc;
    uint64_t parts[36];
    if ((rc = msm_host_scalars(sl.c, parts, pp, coeffs, n, true))) return rc;
    if ((rc = msm_host_scalars(sl.c, parts + 18, pg, blind, m, true))) return rc;
    host::HXYZZ t = host::hadd(host::hfrom_jacobian(parts), host::hfrom_jacobian(parts + 18));
    uint64_t jac[18]; host::hstore_jacobian_normalized(jac, t);
    jacobian_to_affine104(out104, jac);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_fr_vec_op_device(void* d_dst, const void* d_a, const void* d_b, size_t n, int32_t op, void* stream) {
  return device_entry((!d_dst || !d_a || !d_b) && n, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_vec_op(c, d_dst, d_a, d_b, n, op, s); });
}

int32_t aleo_mi355x_fr_lin_device(void* d_dst, size_t n, const void* c0_mont, const void* c1_mont, const void* d_a, const void* c2_mont, const void* d_b, void* stream) {
  return device_entry(!d_dst && n, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_lin(c, d_dst, n, c0_mont, c1_mont, d_a, c2_mont, d_b, s); });
}

int32_t aleo_mi355x_fr_powers_device(void* d_dst, size_t n, const void* first_mont, const void* ratio_mont, void* stream) {
  return device_entry((!d_dst && n) || !first_mont || !ratio_mont, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_powers(c, d_dst, n, first_mont, ratio_mont, s); });
}

int32_t aleo_mi355x_fr_gather_mul_device(void* d_dst, size_t n, const void* d_scale, const void* d_table1, const void* d_idx1, const void* d_table2, const void* d_idx2, void* stream) {
  return device_entry(n && (!d_dst || !d_table1 || !d_idx1 || (d_table2 && !d_idx2)), nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_gather_mul(c, d_dst, n, d_scale, d_table1, d_idx1, d_table2, d_idx2, s); });
}

int32_t aleo_mi355x_fr_eval_batch_device(void* d_out, const void* const* d_polys, const size_t* lens, const void* z_mont, size_t k, void* stream) {
  return device_entry(k && (!d_out || !d_polys || !lens || !z_mont), nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_eval_batch(c, d_out, d_polys, lens, z_mont, k, s); });
}

int32_t aleo_mi355x_varuna_prove(const aleo_mi355x_varuna_index* index, const void* const* assignments, size_t n_instances, const uint8_t* seed, void* out_proof, size_t* len) {
  return guarded([&] {
    if (!index || !assignments || !out_proof || !len || !seed || !index->positions || !index->vk_bytes) return bad_arg("varuna_prove: null argument");
    for (size_t i = 0; i < n_instances && i < 32; ++i) if (!assignments[i]) return bad_arg("varuna_prove: null assignment");
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, index->committer_key); if (fb.rc) return fb.rc;
    return varuna_prove_batch(sl.c, fb.pb, &index, 1, assignments, &n_instances, seed, (uint8_t*)out_proof, len);
  });
}

static int32_t find_varuna(Device* d, uint64_t handle, std::shared_ptr<VarunaIndexOwner>* keep, bool take = false) {
  std::lock_guard<std::mutex> lk(d->mu);
  return handle_get(d->varuna, handle, "unknown index handle", keep, take);
}

int32_t aleo_mi355x_varuna_index_build(uint64_t* index_handle, uint64_t committer_key, uint64_t max_degree, uint64_t gamma_offset, uint64_t lagrange_offset,
                                       const aleo_mi355x_r1cs_matrix abc[3], size_t n_constraints, size_t n_public, size_t n_private, uint32_t domain_flags) {
  return guarded([&] {
    if (!index_handle || !abc || domain_flags > 2) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, committer_key); if (fb.rc) return fb.rc;
    VarunaIndexOwner* raw = nullptr;
    int32_t rc = varuna_index_build(sl.c, fb.pb, fb.keep, committer_key, max_degree, gamma_offset, lagrange_offset, abc, n_constraints, n_public, n_private, domain_flags, &raw);
    if (rc) return rc;
    std::shared_ptr<VarunaIndexOwner> o(raw, varuna_index_delete);
    std::lock_guard<std::mutex> g(sl.d->mu);
    *index_handle = sl.d->next_varuna++; sl.d->varuna[*index_handle] = std::move(o);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_varuna_index_export(uint64_t index_handle, aleo_mi355x_varuna_index* out) {
  return guarded([&] {
    if (!out) return ALEO_MI355X_ERR_BAD_ARG;
    Device* d = nullptr; int32_t rc = get_device(&d); if (rc) return rc;
    std::shared_ptr<VarunaIndexOwner> keep; if ((rc = find_varuna(d, index_handle, &keep))) return rc;
    *out = *varuna_index_view(keep.get());
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_varuna_index_vk(uint64_t index_handle, void* out, size_t* len) {
  return guarded([&] {
    if (!out || !len) return ALEO_MI355X_ERR_BAD_ARG;
    Device* d = nullptr; int32_t rc = get_device(&d); if (rc) return rc;
    std::shared_ptr<VarunaIndexOwner> keep; if ((rc = find_varuna(d, index_handle, &keep))) return rc;
    const std::vector<uint8_t>& vk = varuna_index_vk(keep.get());
    if (*len < vk.size()) { *len = vk.size(); g_last_error = "index_vk: output buffer too small"; return ALEO_MI355X_ERR_BAD_ARG; }
    std::memcpy(out, vk.data(), vk.size()); *len = vk.size();
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_varuna_index_free(uint64_t index_handle) {
  return guarded([&] {
    Device* d = nullptr; int32_t rc = get_device(&d); if (rc) return rc;
    std::shared_ptr<VarunaIndexOwner> dead;              // freed after the lock is dropped, once no proof uses it
    return find_varuna(d, index_handle, &dead, true);
  });
}

int32_t aleo_mi355x_varuna_prove_indexed(uint64_t index_handle, const void* const* assignments, size_t n_instances, const uint8_t* seed, void* out_proof, size_t* len) {
  return guarded([&] {
    if (!assignments || !out_proof || !len || !seed) return ALEO_MI355X_ERR_BAD_ARG;
    for (size_t i = 0; i < n_instances && i < 32; ++i) if (!assignments[i]) return bad_arg("varuna_prove: null assignment");
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<VarunaIndexOwner> ixk; { int32_t rci = find_varuna(sl.d, index_handle, &ixk); if (rci) return rci; }
    const aleo_mi355x_varuna_index* ix = varuna_index_view(ixk.get());
    FoundBases fb(sl.d, ix->committer_key); if (fb.rc) return fb.rc;
    return varuna_prove_batch(sl.c, fb.pb, &ix, 1, assignments, &n_instances, seed, (uint8_t*)out_proof, len);
  });
}

int32_t aleo_mi355x_varuna_prove_batch_indexed(const uint64_t* index_handles, size_t n_circuits, const void* const* assignments, const size_t* n_instances, const uint8_t* seed,
                                               void* out_proof, size_t* len) {
  return guarded([&] {
    if (!seed || !index_handles || !assignments || !n_instances || !out_proof || !len || n_circuits < 1 || n_circuits > 32) return bad_arg("varuna_prove_batch: null argument or circuit count outside 1..32");
    size_t total = 0;
    for (size_t j = 0; j < n_circuits; ++j) { if (n_instances[j] < 1 || n_instances[j] > 32) return bad_arg("varuna_prove_batch: 1..32 instances per circuit"); total += n_instances[j]; }
    for (size_t i = 0; i < total; ++i) if (!assignments[i]) return bad_arg("varuna_prove_batch: null assignment");
    Slot sl; if (sl.rc) return sl.rc;
    std::vector<std::shared_ptr<VarunaIndexOwner>> ixk(n_circuits); std::vector<const aleo_mi355x_varuna_index*> views(n_circuits);
    for (size_t j = 0; j < n_circuits; ++j) { int32_t rci = find_varuna(sl.d, index_handles[j], &ixk[j]); if (rci) return rci; views[j] = varuna_index_view(ixk[j].get()); }
    FoundBases fb(sl.d, views[0]->committer_key); if (fb.rc) return fb.rc;
    return varuna_prove_batch(sl.c, fb.pb, views.data(), n_circuits, assignments, n_instances, seed, (uint8_t*)out_proof, len);
  });
}

int32_t aleo_mi355x_varuna_prove_many(aleo_mi355x_prove_request* requests, size_t n_requests) {
  return guarded([&] {
    if (!requests || n_requests < 1 || n_requests > 64) return bad_arg("varuna_prove_many: 1..64 requests");
    Slot sl; if (sl.rc) return sl.rc;
    std::vector<ProveRequest> rq(n_requests); std::vector<std::vector<std::shared_ptr<VarunaIndexOwner>>> keep_ix(n_requests);
    uint64_t key = 0; bool have_key = false;
    for (size_t p = 0; p < n_requests; ++p) {
      aleo_mi355x_prove_request& r = requests[p]; r.status = ALEO_MI355X_OK;
      auto bad = [&](const char* why) { r.status = ALEO_MI355X_ERR_BAD_ARG; rq[p].status = r.status; rq[p].error = why; };
      if (!r.index_handles || !r.assignments || !r.n_instances || !r.seed || !r.out_proof || r.n_circuits < 1 || r.n_circuits > 32) { bad("varuna_prove_many: null argument or circuit count outside 1..32"); continue; }
      size_t total = 0; bool ok = true;
      for (size_t j = 0; j < r.n_circuits; ++j) { if (r.n_instances[j] < 1 || r.n_instances[j] > 32) ok = false; total += r.n_instances[j]; }
      for (size_t i = 0; ok && i < total; ++i) if (!r.assignments[i]) ok = false;
      if (!ok) { bad("varuna_prove_many: 1..32 instances per circuit, no null assignment"); continue; }
      keep_ix[p].resize(r.n_circuits);
      for (size_t j = 0; j < r.n_circuits && !rq[p].status; ++j) {
        const int32_t rci = find_varuna(sl.d, r.index_handles[j], &keep_ix[p][j]);
        if (rci) { r.status = rci; rq[p].status = rci; rq[p].error = g_last_error; break; }
        rq[p].ixs.push_back(varuna_index_view(keep_ix[p][j].get()));
      }
      if (rq[p].status) continue;
      if (!have_key) { key = rq[p].ixs[0]->committer_key; have_key = true; }
      if (rq[p].ixs[0]->committer_key != key) { bad("varuna_prove_many: every request must use indexes of ONE committer key"); continue; }
      rq[p].assignments = r.assignments; rq[p].ks = r.n_instances; rq[p].seed32 = r.seed; rq[p].out = (uint8_t*)r.out_proof; rq[p].out_len = &r.len;
    }
    if (!have_key) { g_last_error = rq[0].error; return rq[0].status ? rq[0].status : ALEO_MI355X_ERR_BAD_ARG; }
    FoundBases fb(sl.d, key); if (fb.rc) return fb.rc;
    std::vector<ProveRequest> live; std::vector<size_t> where;
    for (size_t p = 0; p < n_requests; ++p) if (!rq[p].status) { live.push_back(rq[p]); where.push_back(p); }
    // The call runs as up to FOUR lockstep groups (ALEO_MI355X_LOCKSTEP_GROUPS, default 4) on as many threads (the caller's and one per further group, each on a context of
    // its own, whose main stream has a hardware queue of its own: "streams" above): while one group's commitments hold the card, the other groups' field kernels, sorts,
    // reductions and transcripts — a third of a lockstep round — run in their shadow.  Up to four proofs that is one proof per group; from five on the groups hold two or more
    // and batch their commitments.  Measured (2^15 constraints, same box; profiles/r05_lockstep_groups_ab.txt, r05_lockstep_retune*.txt, r05_group_min_ab.txt, r05_group_from_ab.txt):
    // 8 proofs 32.7 ms as one group, 27.3 as four; 2 proofs 10.4 ms in lockstep, 8.55 as two groups of one; 3: 13.5 -> 11.6; 4: 15.1 -> 14.5; 8 groups of one: 29.6.
    // Every call of two or more proofs is split, down to one proof per group.  ALEO_MI355X_LOCKSTEP_GROUPS=1: one group.  Proof bytes do not depend on any of it.
    static const int groups_env = [] { const char* e = std::getenv("ALEO_MI355X_LOCKSTEP_GROUPS"); const int k = e ? std::atoi(e) : 4; return k >= 1 && k <= 4 ? k : 4; }();
    int32_t rc = ALEO_MI355X_OK; bool split_done = false;
    const size_t want_groups = live.size() >= 2 ? std::min<size_t>((size_t)groups_env, live.size()) : 1;
    if (want_groups >= 2) {
      // contexts for groups 1..: never waited for (whatever is free now); fewer groups if fewer are free
      std::vector<Ctx*> gc{sl.c}; std::vector<std::unique_lock<std::mutex>> glk;
      for (size_t g = 1; g < want_groups; ++g) {
        Ctx* c2 = nullptr; std::unique_lock<std::mutex> lk2;
        if (acquire_other(sl.d, sl.c, &c2, lk2, false) != ALEO_MI355X_OK || !c2) break;
        gc.push_back(c2); glk.push_back(std::move(lk2));
      }
      const size_t G = gc.size();
      if (G >= 2) {
        std::vector<std::vector<ProveRequest>> grp(G); std::vector<std::vector<size_t>> at(G);
        for (size_t i = 0; i < live.size(); ++i) { const size_t g = i * G / live.size(); grp[g].push_back(live[i]); at[g].push_back(i); }      // contiguous, balanced
        std::vector<int32_t> rcs(G, ALEO_MI355X_OK); std::vector<std::string> errs(G); std::vector<std::thread> th; bool started = true;
        // inside a group ONE thread runs the group's proofs: the groups are the call's parallelism, and four busy streams beat eight (profiles/r05_lockstep_retune.txt: 29.4 / 28.5 / 27.5 ms per 8 proofs with 4 / 2 / 1 workers per group, 54.0 / 53.9 / 52.8 per 16)
        constexpr int group_workers = 1;
        auto run_group = [&](size_t g, Ctx* on) {              // group g's status and error text; never lets an exception out (nothing may unwind past the joinable threads)
          try {
            if (hipSetDevice(sl.d->device) != hipSuccess) { rcs[g] = ALEO_MI355X_ERR_HIP; errs[g] = "hipSetDevice failed"; return; }
            rcs[g] = varuna_prove_many(on, fb.pb, grp[g], group_workers); if (rcs[g]) errs[g] = g_last_error;
          } catch (...) { rcs[g] = ALEO_MI355X_ERR_HIP; errs[g] = g ? "varuna_prove_many: exception in a lockstep group" : "varuna_prove_many: exception in the first group"; }
        };
        for (size_t g = 1; g < G && started; ++g) { try { th.emplace_back(run_group, g, gc[g]); } catch (...) { started = false; } }
        // (a thread that could not be started: its group and the ones behind it run here, after group 0)
        run_group(0, sl.c);
        for (auto& t : th) t.join();
        for (size_t g = th.size() + 1; g < G; ++g) run_group(g, sl.c);
        for (size_t g = 0; g < G; ++g) { for (size_t i = 0; i < grp[g].size(); ++i) live[at[g][i]] = grp[g][i]; if (rcs[g] && !rc) { rc = rcs[g]; g_last_error = errs[g]; } }
        split_done = true;
      }
    }
    if (!split_done) rc = live.empty() ? ALEO_MI355X_OK : varuna_prove_many(sl.c, fb.pb, live);
    std::string first_error;
    for (size_t i = 0; i < live.size(); ++i) { requests[where[i]].status = live[i].status; if (live[i].status && first_error.empty()) first_error = live[i].error; }
    for (size_t p = 0; p < n_requests; ++p) if (rq[p].status && first_error.empty()) first_error = rq[p].error;
    if (!first_error.empty()) g_last_error = first_error;
    return rc;
  });
}

int32_t aleo_mi355x_varuna_last_timing(double* out_ms, int32_t cap) {
  int32_t n = cap < 8 ? cap : 8;
  for (int32_t i = 0; i < n; ++i) out_ms[i] = g_varuna_timing[i];
  return n;
}

int32_t aleo_mi355x_fr_random_device(void* d_dst, size_t n, const uint8_t* seed, uint64_t first_index, int32_t montgomery, void* stream) {
  return device_entry((!d_dst && n) || !seed, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_random(c, d_dst, n, seed, first_index, montgomery, s); });
}

int32_t aleo_mi355x_fr_lincomb_device(void* d_dst, size_t n, const void* c0_mont, const void* const* d_terms, const size_t* lens, const void* coeffs_mont, size_t k, void* stream) {
  return device_entry((!d_dst && n) || (k && (!d_terms || !lens || !coeffs_mont)), nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_lincomb(c, d_dst, n, c0_mont, d_terms, lens, coeffs_mont, k, s); });
}

int32_t aleo_mi355x_ahp_first_sumcheck_device(void* d_dst, size_t n, const void* d_r, const void* d_za, const void* d_zb, const void* d_t, const void* d_z,
                                              const void* eta_b_mont, const void* eta_c_mont, void* stream) {
  return device_entry(n && (!d_dst || !d_r || !d_za || !d_zb || !d_t || !d_z || !eta_b_mont || !eta_c_mont), nullptr, stream, [&](Ctx* c, hipStream_t s) { return ahp_first_sumcheck(c, d_dst, n, d_r, d_za, d_zb, d_t, d_z, eta_b_mont, eta_c_mont, s); });
}

int32_t aleo_mi355x_ahp_matrix_sumcheck_device(void* d_dst, size_t n, const void* const* d_index, size_t index_stride, const void* const* d_f, const void* consts_mont, void* stream) {
  return device_entry(n && (!d_dst || !d_index || !d_f || !consts_mont || (d_index[0] && !d_f[0]) || (d_index[1] && !d_f[1]) || (d_index[2] && !d_f[2])), nullptr, stream, [&](Ctx* c, hipStream_t s) { return ahp_matrix_sumcheck(c, d_dst, n, d_index, index_stride, d_f, consts_mont, s); });
}

int32_t aleo_mi355x_fr_blind_rows_device(void* d_dst, const void* d_src, size_t n, size_t rows, const void* rho_mont, void* stream) {
  return device_entry(rows && n && (!d_dst || !d_src || !rho_mont), nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_blind_rows(c, d_dst, d_src, n, rows, rho_mont, s); });
}

int32_t aleo_mi355x_ahp_sumcheck_operands_device(void* d_dst, const void* d_witness_polys, const void* d_x_polys, size_t n, size_t n_x, size_t instances, void* stream) {
  return device_entry(instances && n && (!d_dst || !d_witness_polys || (!d_x_polys && n_x)), nullptr, stream, [&](Ctx* c, hipStream_t s) { return ahp_sumcheck_operands(c, d_dst, d_witness_polys, d_x_polys, n, n_x, instances, s); });
}

int32_t aleo_mi355x_fr_batch_inverse_device(void* d_inout, size_t n, void* stream) {
  return device_entry(!d_inout && n, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_batch_inverse(c, d_inout, n, s); });
}

int32_t aleo_mi355x_fr_divide_by_linear_device(void* d_quotient, void* d_eval, const void* d_poly, size_t n, const void* z_mont, void* stream) {
  return guarded([&] {
    if ((!d_poly && n) || (!d_quotient && !d_eval)) return ALEO_MI355X_ERR_BAD_ARG;
    if (!z_mont || (d_quotient && d_quotient == d_poly)) return bad_arg("fr_divide_by_linear_device: null point, or quotient aliases the polynomial");
    return enqueue_on_slot(stream, [&](Ctx* c, hipStream_t s) { return fr_divide_by_linear(c, d_quotient, d_eval, d_poly, n, z_mont, s); });
  });
}

// KZG10::open for one polynomial at one point: witness polynomial on the device (slot scratch), then its commitment.
int32_t aleo_mi355x_kzg_open_device(void* out_affine104, void* out_eval_mont, uint64_t handle, const void* d_poly_mont, size_t n, const void* z_mont, void* stream) {
  return guarded([&] {
    if (!out_affine104 || !z_mont || (!d_poly_mont && n)) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    int32_t rc; if ((rc = sl.c->ntt_stage.reserve((n ? n : 1) * 32 + 32))) return rc;
    char* q = sl.c->ntt_stage.as<char>(); char* ev = q + (n ? n : 1) * 32;
    if ((rc = fr_divide_by_linear(sl.c, q, ev, d_poly_mont, n, z_mont, s))) return rc;
    if (out_eval_mont) HIPCHK(hipMemcpyAsync(out_eval_mont, ev, 32, hipMemcpyDeviceToHost, s));
    uint64_t jac[18];
    if ((rc = msm_run1(sl.c, jac, fb.pb, q, n ? n - 1 : 0, true, s))) return rc;      // synchronises: the evaluation has landed too
    if (n <= 1) HIPCHK(hipStreamSynchronize(s));
    jacobian_to_affine104(out_affine104, jac);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_fr_spmv_device(void* d_y, const void* d_row_ptr, const void* d_col_idx, const void* d_vals, const void* d_x, size_t rows, void* stream) {
  return device_entry((!d_y || !d_row_ptr) && rows, nullptr, stream, [&](Ctx* c, hipStream_t s) { return fr_spmv(c, d_y, d_row_ptr, d_col_idx, d_vals, d_x, rows, s); });
}

int32_t aleo_mi355x_ntt_fr(void* inout, uint32_t lg_n, int32_t order, int32_t direction, int32_t type) {
  return guarded([&] {
    if (!inout || lg_n > 30 || order < 0 || order > 3 || direction < 0 || direction > 1 || type < 0 || type > 1) return bad_arg("ntt_fr: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    size_t bytes = ((size_t)1 << lg_n) * 32;
    int32_t rc; if ((rc = sl.c->ntt_stage.reserve(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(sl.c->ntt_stage.p, inout, bytes, hipMemcpyHostToDevice, sl.c->stream));
    if ((rc = ntt_run(sl.c, sl.c->ntt_stage.p, lg_n, 1, order, direction, type, sl.c->stream))) return rc;
    HIPCHK(hipMemcpyAsync(inout, sl.c->ntt_stage.p, bytes, hipMemcpyDeviceToHost, sl.c->stream));
    HIPCHK(hipStreamSynchronize(sl.c->stream));
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_ntt_fr_device(void* d_inout, uint32_t lg_n, int32_t order, int32_t direction, int32_t type, void* stream) {
  return device_entry(!d_inout || lg_n > 30 || order < 0 || order > 3 || direction < 0 || direction > 1 || type < 0 || type > 1, "ntt_fr_device: bad argument", stream, [&](Ctx* c, hipStream_t s) { return ntt_run(c, d_inout, lg_n, 1, order, direction, type, s); });
}

int32_t aleo_mi355x_ntt_fr_batch_device(void* d_inout, uint32_t lg_n, size_t batch, int32_t order, int32_t direction, int32_t type, void* stream) {
  return device_entry((!d_inout && batch) || lg_n > 30 || order < 0 || order > 3 || direction < 0 || direction > 1 || type < 0 || type > 1, "ntt_fr_batch_device: bad argument", stream, [&](Ctx* c, hipStream_t s) { return ntt_run(c, d_inout, lg_n, batch, order, direction, type, s); });
}

int32_t aleo_mi355x_ntt_fr_from_device(void* d_out, const void* d_src, size_t src_stride, size_t src_len, uint32_t lg_n, size_t batch, int32_t direction, int32_t type, void* stream) {
  return guarded([&] {
    if (((!d_out || !d_src) && batch) || lg_n > 30 || direction < 0 || direction > 1 || type < 0 || type > 1 || src_len > ((size_t)1 << lg_n) || src_stride >= (1ull << 32)) {
      g_last_error = "ntt_fr_from_device: bad argument"; return ALEO_MI355X_ERR_BAD_ARG;
    }
    if (batch) {                                             // the output must not overlap the source (the first pass reads while later blocks of the same launch already write)
      const char* o0 = (const char*)d_out; const char* o1 = o0 + ((batch << lg_n) * 32);
      const char* s0 = (const char*)d_src; const char* s1 = s0 + ((batch - 1) * src_stride + src_len) * 32;
      if (src_len && o0 < s1 && s0 < o1) return bad_arg("ntt_fr_from_device: d_out overlaps d_src");
    }
    return enqueue_on_slot(stream, [&](Ctx* c, hipStream_t s) { return ntt_run_from(c, d_out, d_src, src_stride, src_len, lg_n, batch, direction, type, s); });
  });
}

int32_t aleo_mi355x_fr_grid_scale_device(void* d_data, uint32_t lg_n, uint64_t rows, uint64_t cols, uint64_t row0, uint64_t col0, uint64_t ld,
                                         int32_t mode, int32_t direction, void* stream) {
  return device_entry((!d_data && rows && cols) || lg_n == 0 || lg_n > 32 || mode < 0 || mode > 1 || direction < 0 || direction > 1, "fr_grid_scale_device: bad argument", stream, [&](Ctx* c, hipStream_t s) { return fr_grid_scale(c, d_data, lg_n, rows, cols, row0, col0, ld, mode, direction, s); });
}

int32_t aleo_mi355x_fr_transpose_device(void* d_dst, const void* d_src, uint64_t rows, uint64_t cols, void* stream) {
  return guarded([&] {
    if ((!d_dst || !d_src) && rows && cols) return bad_arg("fr_transpose_device: bad argument");
    if (d_dst == d_src && rows > 1 && cols > 1) return bad_arg("fr_transpose_device: in place is not supported");
    return enqueue_on_slot(stream, [&](Ctx* c, hipStream_t s) { return fr_transpose(c, d_dst, d_src, rows, cols, s); });
  });
}

int32_t aleo_mi355x_fq_mul(void* r, const void* a, const void* b, size_t n) {
  return guarded([&] { if ((!r || !a || !b) && n) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return launch_fq_mul(sl.c, r, a, b, n); });
}
int32_t aleo_mi355x_fr_mul(void* r, const void* a, const void* b, size_t n) {
  return guarded([&] { if ((!r || !a || !b) && n) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return launch_fr_mul(sl.c, r, a, b, n); });
}

int32_t aleo_mi355x_selftest_madd28(uint32_t lanes, uint32_t steps, uint64_t seed, uint32_t* failures) {
  return guarded([&] { if (!failures) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return selftest_madd28(sl.c, lanes, steps, seed, failures); });
}
int32_t aleo_mi355x_selftest_addquad(uint32_t ops, uint64_t seed, uint32_t* failures) {
  return guarded([&] { if (!failures || !ops || ops > (1u << 22)) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return selftest_addquad(sl.c, ops, seed, failures); });
}
int32_t aleo_mi355x_selftest_f28_rows(const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224,
                                      const void* acc224, const void* pt112, uint32_t n_madd, void* out_acc224, uint8_t* ok_u8) {
  return guarded([&] {
    if (n_add > (1u << 20) || n_madd > (1u << 20)) return bad_arg("selftest_f28_rows: at most 2^20 rows of either kind");
    if ((n_add && (!a224 || !b224 || !out_pair224 || !out_quad224)) || (n_madd && (!acc224 || !pt112 || !out_acc224 || !ok_u8))) return bad_arg("selftest_f28_rows: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    return selftest_f28_rows(sl.c, a224, b224, n_add, out_pair224, out_quad224, acc224, pt112, n_madd, out_acc224, ok_u8);
  });
}
int32_t aleo_mi355x_selftest_te28_rows(const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224, uint32_t* z_add_u32,
                                       const void* acc224, const void* row168, const uint8_t* how_u8, uint32_t n_madd, void* out_acc224, uint8_t* z_madd_u8) {
  return guarded([&] {
    if (n_add > (1u << 20) || n_madd > (1u << 20)) return bad_arg("selftest_te28_rows: at most 2^20 rows of either kind");
    if ((n_add && (!a224 || !b224 || !out_pair224 || !out_quad224 || !z_add_u32)) || (n_madd && (!acc224 || !row168 || !how_u8 || !out_acc224 || !z_madd_u8))) return bad_arg("selftest_te28_rows: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    return selftest_te28_rows(sl.c, a224, b224, n_add, out_pair224, out_quad224, z_add_u32, acc224, row168, how_u8, n_madd, out_acc224, z_madd_u8);
  });
}

int32_t aleo_mi355x_selftest_g2p_rows(const void* a448, const void* b448, uint32_t n_add, void* out_add448, const void* d448, uint32_t n_dbl, void* out_dbl448,
                                      const void* acc448, const void* ent224, const uint8_t* neg_u8, uint32_t n_madd, void* out_acc448, uint8_t* ok2_u8) {
  return guarded([&] {
    if (n_add > (1u << 20) || n_dbl > (1u << 20) || n_madd > (1u << 20)) return bad_arg("selftest_g2p_rows: at most 2^20 rows of each kind");
    if ((n_add && (!a448 || !b448 || !out_add448)) || (n_dbl && (!d448 || !out_dbl448)) || (n_madd && (!acc448 || !ent224 || !neg_u8 || !out_acc448 || !ok2_u8))) return bad_arg("selftest_g2p_rows: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    return selftest_g2p_rows(sl.c, a448, b448, n_add, out_add448, d448, n_dbl, out_dbl448, acc448, ent224, neg_u8, n_madd, out_acc448, ok2_u8);
  });
}

int32_t aleo_mi355x_selftest_ed29_rows(const void* mul_a36, const void* mul_b36, uint32_t n_mul, void* out_mul36, const void* tidy36, uint32_t n_tidy, void* out_tidy36,
                                       const void* canon36, uint32_t n_canon, void* out_canon36, const void* p144, const void* q144, const uint8_t* neg_u8, const void* d2_36,
                                       uint32_t n_add, void* out_add144, const void* dbl144, const uint8_t* want_t_u8, uint32_t n_dbl, void* out_dbl144) {
  return guarded([&] {
    if (n_mul > (1u << 20) || n_tidy > (1u << 20) || n_canon > (1u << 20) || n_add > (1u << 20) || n_dbl > (1u << 20)) return bad_arg("selftest_ed29_rows: at most 2^20 rows of each kind");
    if ((n_mul && (!mul_a36 || !mul_b36 || !out_mul36)) || (n_tidy && (!tidy36 || !out_tidy36)) || (n_canon && (!canon36 || !out_canon36)) ||
        (n_add && (!p144 || !q144 || !neg_u8 || !d2_36 || !out_add144)) || (n_dbl && (!dbl144 || !want_t_u8 || !out_dbl144))) return bad_arg("selftest_ed29_rows: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    return selftest_ed29_rows(sl.c, mul_a36, mul_b36, n_mul, out_mul36, tidy36, n_tidy, out_tidy36, canon36, n_canon, out_canon36, p144, q144, neg_u8, d2_36, n_add, out_add144,
                              dbl144, want_t_u8, n_dbl, out_dbl144);
  });
}

int32_t aleo_mi355x_selftest_slice_order(const uint32_t* hist, uint32_t n_buckets, uint32_t total_pairs, int32_t fused, uint32_t* violations) {
  return guarded([&] { if (!hist || !violations) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return selftest_slice_order(sl.c, hist, n_buckets, total_pairs, fused != 0, violations); });
}
int32_t aleo_mi355x_selftest_sort_pairs(const void* scalars, const uint32_t* seg_n, const uint32_t* seg_off, const uint8_t* seg_set, uint32_t nseg, int32_t c, int32_t pre, int32_t mont,
                                        uint32_t k_sets, uint32_t row_stride, const uint8_t* inf_u8, uint32_t tile, uint32_t* hist_out, uint32_t* sorted_out, size_t sorted_cap, uint32_t* pairs_out) {
  return guarded([&] {
    if (!scalars || !seg_n || !seg_off || !seg_set || !hist_out || !sorted_out || !pairs_out || (pre != 0 && pre != 1) || (mont != 0 && mont != 1)) return bad_arg("selftest_sort_pairs: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    return selftest_sort_pairs(sl.c, scalars, seg_n, seg_off, seg_set, nseg, c, pre != 0, mont != 0, k_sets, row_stride, inf_u8, tile, hist_out, sorted_out, sorted_cap, pairs_out);
  });
}
int32_t aleo_mi355x_selftest_g2pair(const void* affine192, uint32_t n_points, uint32_t n_pairs, uint32_t* failures2) {
  return guarded([&] { if (!affine192 || !failures2 || n_points < 3 || !n_pairs || n_pairs > (1u << 20)) return ALEO_MI355X_ERR_BAD_ARG; Slot sl; if (sl.rc) return sl.rc; return selftest_g2pair(sl.c, affine192, n_points, n_pairs, failures2); });
}

// One host function of frops.h that has no entry point of its own, as the prover calls it (test hook: the header lists what each step takes).
int32_t aleo_mi355x_selftest_fr_step(uint32_t step, const void* const* ptrs, const size_t* sizes, const void* consts_mont) {
  return guarded([&] {
    if (!ptrs || !sizes || step > 6) return bad_arg("selftest_fr_step: null array or unknown step");
    // the pointers a launch of the step dereferences: the first `need` (step 3: dst and up to 8 sources; step 4: both tables, then four per range that is not empty)
    const size_t count = sizes[0];
    const size_t need = step == 0 ? 2 : step == 1 ? 4 : step == 2 ? 2 : step == 3 ? 1 + (count < 8 ? count : 8) : step == 4 ? 2 : 3;
    for (size_t i = 0; i < need; ++i) if (!ptrs[i]) return bad_arg("selftest_fr_step: null pointer");
    if (step == 4) for (size_t m = 0; m < count && m < 3; ++m) for (size_t i = 0; i < 4; ++i) if (sizes[1 + m] && !ptrs[2 + 4 * m + i]) return bad_arg("selftest_fr_step: null pointer in a range");
    if (step == 2 && !consts_mont) return bad_arg("selftest_fr_step: scale_rows without constants");
    Slot sl; if (sl.rc) return sl.rc;
    Ctx* c = sl.c; hipStream_t s = c->stream; int32_t rc = ALEO_MI355X_OK;
    switch (step) {
      case 0: rc = fr_add_tiled(c, (void*)ptrs[0], sizes[0], ptrs[1], sizes[1], s); break;
      case 1: rc = fr_sub_mul(c, (void*)ptrs[0], ptrs[1], ptrs[2], ptrs[3], sizes[0], s); break;
      case 2: rc = fr_scale_rows(c, (void*)ptrs[0], ptrs[1], sizes[0], sizes[1], consts_mont, s); break;
      case 3: rc = fr_pick(c, (void*)ptrs[0], ptrs + 1, count, s); break;
      case 4: {
        void* dst[3] = {}; const void* scale[3] = {}; const void* idx1[3] = {}; const void* idx2[3] = {}; size_t n[3] = {};
        for (size_t m = 0; m < count && m < 3; ++m) { dst[m] = (void*)ptrs[2 + 4 * m]; scale[m] = ptrs[3 + 4 * m]; idx1[m] = ptrs[4 + 4 * m]; idx2[m] = ptrs[5 + 4 * m]; n[m] = sizes[1 + m]; }
        rc = fr_gather_mul3(c, dst, n, scale, ptrs[0], idx1, ptrs[1], idx2, count > 3 ? 4u : (uint32_t)count, s); break;
      }
      case 5: rc = fr_scatter_to_mont(c, (void*)ptrs[0], ptrs[1], ptrs[2], sizes[0], (void*)ptrs[3], s); break;
      default: rc = fr_split_quotient(c, (void*)ptrs[0], (void*)ptrs[1], ptrs[2], ptrs[3], sizes[0], (void*)ptrs[4], s); break;
    }
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_last_msm_timing(double* out_ms, int32_t cap) {
  return guarded([&] {
    if (!out_ms || cap <= 0) return 0;
    const MsmTiming& t = g_last_msm;          // of the calling thread's most recent MSM
    double v[7] = {t.total, t.sort, t.accum, t.reduce, t.host, t.accum_kernel, (double)t.accum_launches};
    int32_t k = cap < 7 ? cap : 7;
    for (int32_t i = 0; i < k; ++i) out_ms[i] = v[i];
    return k;
  }, 0);
}

const char* aleo_mi355x_strerror(int32_t status) {
  switch (status) {
    case ALEO_MI355X_OK: return "ok";
    case ALEO_MI355X_ERR_NO_DEVICE: return "no gfx950 device available";
    case ALEO_MI355X_ERR_BAD_ARG: return "bad argument";
    case ALEO_MI355X_ERR_HIP: return "HIP runtime error";
    case ALEO_MI355X_ERR_BAD_HANDLE: return "unknown handle";
    case ALEO_MI355X_ERR_OOM: return "out of device memory";
    case ALEO_MI355X_ERR_UNSATISFIED: return "assignment does not satisfy the circuit";
    case ALEO_MI355X_ERR_NOT_OWNER: return "the record's owner is not the given address";
    case ALEO_MI355X_ERR_INTERNAL: return "the device and the host path disagree";
    default: return "unknown status";
  }
}
// The sizes from which the drop-in's two arms should take the GPU: measured crossovers of the COLD one-shot calls against the CPU
// path on the same box (bench.py cpu_baseline.crossover, profiles/r04_crossover.json), overridable per deployment.
size_t aleo_mi355x_min_msm(void) { return env_size("ALEO_MI355X_MIN_MSM", (size_t)1 << 10); }
size_t aleo_mi355x_min_ntt(void) { return env_size("ALEO_MI355X_MIN_NTT", (size_t)1 << 12); }
int32_t aleo_mi355x_selftest_host_inverse(uint32_t count, uint64_t seed, uint32_t* failures, double* ns_per_inverse) {
  return guarded([&] {
    if (!failures) return bad_arg("selftest_host_inverse: bad argument");
    *failures = 0;
    inverse_selftest<6>(count, seed, failures, ns_per_inverse);
    inverse_selftest<4>(count, seed, failures, ns_per_inverse ? ns_per_inverse + 2 : nullptr);
    return ALEO_MI355X_OK;
  });
}
const char* aleo_mi355x_last_error(void) { return g_last_error.c_str(); }
const char* aleo_mi355x_version(void) { return "aleo_mi355x 0.4.0 (gfx950)"; }

}  // the entry points
