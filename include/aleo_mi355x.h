/*
 * aleo_mi355x.h — C ABI of libaleo_mi355x.so: the MI355X (gfx950) backend for the two operators that dominate
 * the Aleo SDK's execute/prove path:
 *
 *   a1  snarkvm_algorithms::msm::VariableBase::msm::<G1Affine>      (BLS12-377 G1 Pippenger MSM)
 *   a2  snarkvm_algorithms::fft::EvaluationDomain::<Fr>::{fft,ifft,coset_fft,coset_ifft}_in_place
 *
 * Reference interfaces this ABI replaces.  The prover is crates.io snarkVM =0.14.5 (pins:
 * /root/reference/Cargo.toml:28-53, /root/reference/Cargo.lock:2200 snarkvm-algorithms), entered from
 *   /root/reference/rust/src/program/execute.rs:74   trace.prove_execution::<A,_>(…)
 *   /root/reference/rust/src/program/execute.rs:177  vm.execute(…)
 *   /root/reference/rust/src/program/transfer.rs:99  vm.execute(… "credits.aleo","transfer_public" …)
 * and the seam is the one upstream's optional `cuda` feature uses [UPSTREAM-RECALL]:
 *   algorithms/src/msm/variable_base/mod.rs   VariableBase::msm  -> snarkvm_algorithms_cuda::msm(bases, scalars)
 *   algorithms/src/fft/domain.rs              in_order_{fft,ifft}_in_place -> snarkvm_algorithms_cuda::NTT(size, data,
 *                                             NTTInputOutputOrder, NTTDirection, NTTType)
 * with the same contract: a non-zero return means "not computed" and the Rust caller falls back to its CPU path.
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer adds on the snarkVM side.
 *
 * Data layouts are snarkVM's in-memory layouts (no conversion at the boundary):
 *   Fr      4 x u64 little-endian limbs, Montgomery form (R = 2^256)                         32 bytes
 *   scalar  BigInteger256: 4 x u64 little-endian limbs, CANONICAL (non-Montgomery), < r      32 bytes
 *   G1Affine {x: Fq, y: Fq, infinity: bool}: 6+6 x u64 Montgomery (R = 2^384) + flag byte    stride 104
 *            (stride 96 = x,y only, no flag, is also accepted)
 *   G1Projective (Jacobian) {x, y, z: Fq}                                                    144 bytes
 * MSM results are returned affine-normalised as Jacobian (x, y, 1), or (1, 1, 0) for the identity; compare
 * group elements after to_affine(), never raw Jacobian limbs.
 *
 * Threading: every entry point may be called concurrently from many host threads (snarkVM commits the
 * polynomials of one round from a rayon pool).  Each call runs on one of the device's slots (own stream and
 * workspaces; ALEO_MI355X_SLOTS = 1..8, default 4), so concurrent calls overlap on the GPU; a pinned set
 * stays alive until the calls using it return, even if another thread unpins it meanwhile.
 * Streams: the *_device entry points that return a result to HOST memory (msm, kzg_commit) complete before they return.
 * Those that only transform device data (ntt_fr*_device, fr_*_device) enqueue on the caller's `stream` and return at once:
 * the caller orders its own work on that stream, and the library orders its internal scratch between calls by events.
 * With stream == NULL they run on the serving slot's stream — which the caller cannot order against — and therefore
 * complete before returning.  hipStreamLegacy names the null stream; hipStreamPerThread is refused (BAD_ARG).
 * Ownership: the caller owns every buffer; nothing is retained after return except through bases_pin (and, when the
 * caller opts in with ALEO_MI355X_SRS_CACHE=1, the one-shot msm_g1's base-array cache described there).
 * No exceptions cross the boundary.
 */
#ifndef ALEO_MI355X_H
#define ALEO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (0 = OK; anything else: caller recomputes on CPU) */
#define ALEO_MI355X_OK 0
#define ALEO_MI355X_ERR_NO_DEVICE 1      /* no gfx950 device / HIP runtime failure at init */
#define ALEO_MI355X_ERR_BAD_ARG 2        /* null pointer, bad stride, lg_n out of range, … */
#define ALEO_MI355X_ERR_HIP 3            /* a HIP call failed; see aleo_mi355x_last_error() */
#define ALEO_MI355X_ERR_BAD_HANDLE 4
#define ALEO_MI355X_ERR_OOM 5
#define ALEO_MI355X_ERR_UNSATISFIED 6  /* varuna_prove*: an assignment does not satisfy its circuit (upstream: the synthesiser's is_satisfied check) */
#define ALEO_MI355X_ERR_NOT_OWNER 7    /* record_plaintext, record_decrypt: the decrypted (or public) owner is not the given address (upstream: "Decryption failed - view key did not match record") */
#define ALEO_MI355X_ERR_INTERNAL 8     /* accounts_search: the host path does not confirm what the kernel found; nothing is handed out */

/* NTT enums: mirror snarkvm_algorithms_cuda::{NTTInputOutputOrder, NTTDirection, NTTType} */
#define ALEO_NTT_ORDER_NN 0   /* natural in, natural out (what fft_in_place exposes) */
#define ALEO_NTT_ORDER_NR 1   /* natural in, bit-reversed out */
#define ALEO_NTT_ORDER_RN 2   /* bit-reversed in, natural out */
#define ALEO_NTT_ORDER_RR 3
#define ALEO_NTT_FORWARD 0
#define ALEO_NTT_INVERSE 1    /* multiplies by size_inv, as EvaluationDomain::ifft_in_place */
#define ALEO_NTT_STANDARD 0
#define ALEO_NTT_COSET 1      /* coset shift g = Fr::multiplicative_generator() = 22 */

/* ENVIRONMENT (set by the HOST before its first HIP call; the library never edits the process environment): GPU_MAX_HW_QUEUES=8 is recommended.  The HIP
 * runtime maps a process's streams onto that many hardware queues (4 by default) and reads the variable once, when it initialises; the library runs a
 * caller's stream, a side stream, high-priority streams and the lockstep prover's worker streams at once (lockstep proofs -5 % with 8 queues, everything
 * else within noise; results never depend on it; 12 or more oversubscribe the device's queues and cost 1.5-2x on lockstep calls).  The library creates
 * the main streams of its slots and of as many helper contexts FIRST, at the device's first use, so that each gets a hardware queue of its own (a
 * lockstep call of 8 proofs: 31.8 -> 27.5 ms): initialise the device (aleo_mi355x_init_device) before the host creates many streams of its own.
 * aleo_amd/__init__.py and bench.py set the variable as their own default; INTEGRATION.md 4 shows the Rust side. */

/* initialises the first n_devices visible devices (0 = all of them).  Idempotent, thread-safe; the calling thread's current
 * HIP device is left as it was.  Every single-device entry point below works on the CALLING THREAD's current HIP device (hipSetDevice is per
 * thread) and initialises it lazily if neither init call was made.  init_device selects and initialises one device (-1 = the current one).
 * device_count: visible devices / devices initialised so far (either pointer may be NULL). */
int32_t aleo_mi355x_init(int32_t n_devices);
int32_t aleo_mi355x_init_device(int32_t device);
int32_t aleo_mi355x_device_count(int32_t* visible, int32_t* initialised);
/* aleo_mi355x_init also turns on direct peer access (xGMI) between every ordered pair of the devices initialised so far, so that the exchange of a
 * sharded transform and the slice pulls of a sharded commitment are link-to-link copies; a pair the platform refuses is left to the runtime's staged
 * copies (never an error).  peer_info: ordered pairs with direct access / refused so far (either pointer may be NULL).
 * ABI note: since 0.2.0 `init` takes a device COUNT; 0.1.x callers that meant "select device d" call init_device(d). */
int32_t aleo_mi355x_peer_info(int32_t* enabled_pairs, int32_t* refused_pairs);

/* a1 — VariableBase::msm(bases: &[G1Affine], scalars: &[BigInteger256]) -> G1Projective.
 * Host pointers.  n = min(len(bases), len(scalars)) is the caller's job (the reference zips the slices).
 * By default every call uploads and converts its base array and keeps nothing.  ALEO_MI355X_SRS_CACHE=1 (read once)
 * opts in to a cache for callers that cannot hold a bases_pin handle: arrays of >= 1024 points stay in HBM keyed by host
 * pointer + stride and are re-validated on each call by hashing 256 sampled points (32 at the front, the rest spread);
 * the third use builds the fixed-base table (~0.15 s, inside that call).  Contract when opted in: a base array must not
 * be rewritten in place (nor its address reused for different points) between calls — unsampled changes are not seen.
 * Without the cache the call's copy of the bases lives in the serving slot's grow-only buffers, kept like its other workspaces;
 * ALEO_MI355X_COLD_POOL=0 (read once) allocates and frees them in every call instead. */
int32_t aleo_mi355x_msm_g1(void* out_jacobian, const void* bases, size_t base_stride, const void* scalars, size_t n);

/* SRS residency: upload + convert a base set once per proving key (SURVEY.md §5 "device-resident SRS").
 * The handle stays valid until unpin.  bases: host pointer. */
int32_t aleo_mi355x_bases_pin(const void* bases, size_t base_stride, size_t n, uint64_t* handle);
int32_t aleo_mi355x_bases_unpin(uint64_t handle);
/* Synthetic SRS-shaped base set generated in HBM: P_i = (first_multiple + i) * base for i in [0, n)
 * ("P_i = (i+1)*G generated on device" — 2^26 points never cross PCIe).  base_affine: one
 * snarkVM Affine (104 bytes, host).  first_multiple >= 1 and first_multiple + n must stay below r. */
int32_t aleo_mi355x_bases_generate(const void* base_affine104, uint64_t first_multiple, size_t n, uint64_t* handle);
/* Synthetic SRS-shaped set: P_i = s_i * base for n canonical 32-byte scalars in host memory (P_i = beta^i * G, the
 * shape of a universal setup's powers_of_beta_g, for which a commitment to p is p(beta) * G).  A zero scalar gives the identity. */
int32_t aleo_mi355x_bases_from_scalars(const void* base_affine104, const void* scalars, size_t n, uint64_t* handle);
/* Optional fixed-base acceleration for a pinned set (an SRS never changes): builds tables of window multiples
 * 2^(c w) * P_i in HBM, stored in the 28-bit-limb form the accumulation kernel computes in (112 bytes per entry), in up to
 * three tiers so that a prefix of ANY length >= 2^10 gets a window width that suits it (KZG10::commit multiplies polynomials
 * of every degree against one SRS): the whole set at c = 20 (>= 2^19 points; 13 rows) or c = 17, its first 2^17 + 64 points at
 * c = 16, its first 2^15 + 64 points at c = 13 (the 64: a committer key is a power of two of powers followed by a few hiding powers).  MSMs over this handle then add one table entry per window into ONE shared bucket
 * set (13 instead of 16 additions per point at 2^20) and skip the Horner tail.  Same results, bit for bit after
 * normalisation.  The whole-set tier is kept in twisted Edwards form (rows y - x | y + x | 2d x y of the point's Edwards image, 168 bytes at a
 * 192-byte stride: 7 field products per bucket addition instead of 10); the two prefix tiers keep x | y rows at a 128-byte stride.  Bytes per power
 * of a 2^20-point set: 13 x 192 + the prefix tiers' share = 2832 (3.0 GB, about 0.20 s) against 2000 (2.1 GB, 0.15 s) with x | y rows throughout.
 * Calls that use the tables REQUIRE bases in the prime-order subgroup, which is all a snarkVM G1Affine can hold: the Edwards tier's addition law has
 * exceptions only between points that differ by one of even order.  A set that breaks this still never yields a wrong result: an exception is noticed
 * on the device and the call computes the request again without tables; and a set with a base of even order whose multiples reach the identity inside a
 * table (such as (-1, 0)) gets no tables at all — the call succeeds and its products run on the plain path. */
int32_t aleo_mi355x_bases_precompute(uint64_t handle);
/* What a pinned set holds in HBM: out[0] points, [1] bytes of the base rows (96-byte snarkVM rows + their 112-byte
 * 28-bit-limb copies), [2] bytes of the fixed-base tables, [3..5] window width c of each table tier (0 = none), [6] tiers.
 * Returns the number of values written (<= cap), 0 for an unknown handle. */
/* A second, narrow-window table (window_bits 13 or 16) over ONE sub-range [offset, offset + n) of a pinned set, for MSMs whose scalars are mostly
 * 0 / 1 — a witness committed in evaluation form against Lagrange-basis powers (KZG10::commit_lagrange): such vectors put hardly a point per bucket into
 * the 2^19 buckets of the wide window, and a proof commits three of them per instance.  Used by aleo_mi355x_kzg_commit_segments_sparse_device (and by
 * the prover's first round) when every segment of the call lies inside the range; up to 32 results share one launch chain.  One range per set. */
int32_t aleo_mi355x_bases_precompute_range(uint64_t handle, size_t offset, size_t n, int32_t window_bits);
int32_t aleo_mi355x_bases_info(uint64_t handle, uint64_t* out, int32_t cap);
/* Copies pinned bases [offset, offset+n) back to the host as snarkVM Affine (stride 104). */
int32_t aleo_mi355x_bases_download(uint64_t handle, size_t offset, size_t n, void* out_affine104);
/* MSM over the first n pinned bases; scalars: host pointer (pageable memory is fine: the upload runs at the link's rate either way).  Against a set with
 * window tables, from 2^19 points on, the scalars go up and through in 2 chunks of 37 / 63 % (3 of 18 / 30 / 52 % from 2^21
 * points) on contexts of their own: a later chunk's upload and sort run under the previous chunk's accumulation, each
 * accumulation is SEEDED with the bucket sums of the chunk before it (no merge kernel), and ONE bucket reduction follows the last chunk; the result
 * does not depend on it. */
int32_t aleo_mi355x_msm_g1_pinned(void* out_jacobian, uint64_t handle, const void* scalars, size_t n);
/* Same, scalars already resident in device memory (hipMalloc'ed or a torch CUDA tensor's data_ptr).
 * The result (144 bytes) is written to HOST memory.  `stream` (here and in every *_device entry point) is a hipStream_t;
 * NULL = the stream of the library slot serving the call, which is NOT ordered with the caller's other streams — a caller
 * whose data was produced on the legacy default stream passes hipStreamLegacy. */
int32_t aleo_mi355x_msm_g1_device(void* out_jacobian, uint64_t handle, const void* d_scalars, size_t n, void* stream);
/* The same with the hint that the scalars are witness-like (mostly 0 / 1 / short): served from the set's range table (bases_precompute_range) when the call
 * lies inside it, otherwise exactly like msm_g1_device.  The host-scalar call msm_g1_pinned looks at 257 of its scalars and takes the hint by itself
 * when the range table starts at point 0. */
int32_t aleo_mi355x_msm_g1_device_sparse(void* out_jacobian, uint64_t handle, const void* d_scalars, size_t n, void* stream);
/* Sum of `count` Jacobian points (144 bytes each, host memory): the local group-add that follows the
 * all-gather of per-GPU partial MSM results.  Result affine-normalised as above. */
int32_t aleo_mi355x_g1_sum(void* out_jacobian, const void* jacobian_points, size_t count);
/* e — ONE MSM over several devices of this process (BASELINE configs[4]: 2^26 points over 8 GPUs).  The base set is cut into
 * n_devices contiguous shards [n g / G, n (g+1) / G); shard g is pinned on devices[g] (devices == NULL: device g mod visible; a device may be
 * listed more than once), with its fixed-base table when precompute != 0.  msm_g1_sharded multiplies scalars[0..n) (n <= the pinned count:
 * shards past n contribute the identity) — every shard runs the whole Pippenger on its device from its own host thread, the G partial sums
 * (144 bytes each; copied to partials_out in shard order when it is not NULL) are added on the host in shard order by aleo_mi355x_g1_sum, so the
 * result is the affine-normalised sum, bit for bit what a single device gives.  No collective: within one process the exchange is G stores
 * into host memory (ranks in separate processes exchange the same partials over RCCL: aleo_amd/dist.py).  generate_sharded: the synthetic set
 * P_i = (first_multiple + i) * base built shard by shard in each device's HBM.  sharded_info: [G, then per shard device, first point, count]. */
int32_t aleo_mi355x_bases_pin_sharded(const void* bases, size_t base_stride, size_t n, const int32_t* devices, size_t n_devices, int32_t precompute, uint64_t* handle);
int32_t aleo_mi355x_bases_generate_sharded(const void* base_affine104, uint64_t first_multiple, size_t n, const int32_t* devices, size_t n_devices, int32_t precompute, uint64_t* handle);
int32_t aleo_mi355x_bases_unpin_sharded(uint64_t handle);
int32_t aleo_mi355x_bases_sharded_info(uint64_t handle, uint64_t* out, int32_t cap);
int32_t aleo_mi355x_msm_g1_sharded(void* out_jacobian, uint64_t handle, const void* scalars, size_t n, void* partials_out);

/* VariableBase::msm::<G2Affine> (SRS / setup paths; the prover itself never runs one).  BLS12-377 G2 over
 * Fq2 = Fq[u]/(u^2 + 5).  bases: snarkVM G2Affine {x: Fq2 (c0, c1), y: Fq2, infinity: bool}, Montgomery limbs, stride 200 (flag byte
 * at 192) or 192; scalars as for G1; result G2Projective (Jacobian x, y, z: Fq2 = 288 bytes), affine-normalised like the G1 result:
 * (x, y, 1), or (1, 1, 0) for the identity.  Host pointers; nothing is retained.  g2_sum: the group add after an all-gather. */
int32_t aleo_mi355x_msm_g2(void* out_jacobian288, const void* bases, size_t base_stride, const void* scalars, size_t n);
int32_t aleo_mi355x_g2_sum(void* out_jacobian288, const void* jacobian_points288, size_t count);
/* A G2 base set resident in HBM (what aleo_mi355x_bases_pin is for G1; SRS powers in G2, a verifying key's elements): rows, infinity flags and the
 * accumulation's 28-bit rows stay on the device, a call uploads its scalars only and multiplies any PREFIX of the set (n <= pinned count).  Same
 * argument formats and result as aleo_mi355x_msm_g2, byte for byte; no window tables (the prover never runs a G2 MSM).  unpin frees the set once the
 * calls that hold it have returned. */
int32_t aleo_mi355x_bases_g2_pin(const void* bases, size_t base_stride, size_t n, uint64_t* handle);
int32_t aleo_mi355x_bases_g2_unpin(uint64_t handle);
int32_t aleo_mi355x_msm_g2_pinned(void* out_jacobian288, uint64_t handle, const void* scalars, size_t n);

/* a2 — EvaluationDomain NTT over Fr, in place, n = 2^lg_n elements (lg_n <= 30), host pointer. */
int32_t aleo_mi355x_ntt_fr(void* inout, uint32_t lg_n, int32_t order, int32_t direction, int32_t type);
/* Same on device-resident data (in place). */
int32_t aleo_mi355x_ntt_fr_device(void* d_inout, uint32_t lg_n, int32_t order, int32_t direction, int32_t type, void* stream);
/* `batch` independent transforms of 2^lg_n elements each, contiguous in d_inout (the local row / column transforms of a
 * transform sharded over several GPUs, SURVEY.md §8e "4-step"; also one call for the polynomials of a prover round). */
int32_t aleo_mi355x_ntt_fr_batch_device(void* d_inout, uint32_t lg_n, size_t batch, int32_t order, int32_t direction, int32_t type, void* stream);
/* The same OUT OF PLACE with a zero-padded input (natural order in and out): transform b reads element i from d_src + (b * src_stride + i) * 32 for
 * i < src_len <= 2^lg_n and takes 0 beyond, and writes its 2^lg_n values to d_out + b * 2^lg_n * 32.  EvaluationDomain::fft of a polynomial of fewer
 * coefficients than the domain (snarkVM resizes the coefficient vector with zeros first: `coeffs.resize(self.size(), F::zero())` in fft / coset_fft); the
 * padding costs no launch and no HBM traffic here — the first pass simply does not read past src_len.  d_out must not overlap the source. */
int32_t aleo_mi355x_ntt_fr_from_device(void* d_out, const void* d_src, size_t src_stride, size_t src_len, uint32_t lg_n, size_t batch, int32_t direction, int32_t type, void* stream);
/* Factors over a rows x cols block (row-major, in place) of the index space of the size-2^lg_n domain:
 *   mode 0: x[r][c] *= w^((row0 + r) * (col0 + c))   — the twiddle between the two axes of a 4-step transform
 *   mode 1: x[r][c] *= g^((row0 + r) * ld + col0 + c) — the coset shift (g = 22) of a block of the coefficient matrix
 *           (every index must stay below 2^lg_n)
 * direction 1 uses w^-1 / g^-1 (no n^-1: the inverse sub-transforms carry their own scale).  lg_n <= 32 here: the domain
 * may be larger than one GPU's share (exponents are carried in 32 bits). */
int32_t aleo_mi355x_fr_grid_scale_device(void* d_data, uint32_t lg_n, uint64_t rows, uint64_t cols, uint64_t row0, uint64_t col0, uint64_t ld,
                                         int32_t mode, int32_t direction, void* stream);
/* dst[c][r] = src[r][c] for 32-byte elements (rows x cols -> cols x rows; dst != src): the layout changes of a 4-step transform. */
int32_t aleo_mi355x_fr_transpose_device(void* d_dst, const void* d_src, uint64_t rows, uint64_t cols, void* stream);
/* e — ONE transform over several devices of this process (SURVEY.md 8(e) "NTT (if sharded): 4-step"): EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place
 * on a host buffer of 2^lg_n Montgomery elements, natural order in and out, split over n_devices (a power of two, <= 2^floor(lg_n / 2); devices == NULL:
 * device g mod visible; a device may be listed more than once).  n = R C: device g uploads the coefficient columns [g C / G, (g + 1) C / G) — its 1/G of the
 * PCIe traffic —, runs its column transforms and the twiddle, the devices exchange one block per pair (peer copies: one per xGMI link), every device
 * runs its row transforms and stores its k_r range of X[k_c R + k_r] straight into the host buffer.  Same values as aleo_mi355x_ntt_fr. */
int32_t aleo_mi355x_ntt_fr_sharded(void* inout, uint32_t lg_n, int32_t direction, int32_t type, const int32_t* devices, size_t n_devices);
/* e2 — the same transform on data RESIDENT in HBM: 2^lg_n Montgomery elements in natural order at d_inout on the calling thread's current device ("home"),
 * transformed in place over the listed devices with no host buffer: home transposes the coefficient matrix once so that every device's columns are one
 * contiguous slab, device g pulls its slab (hipMemcpyPeerAsync over xGMI; the home device itself: a plain copy), column transforms + twiddle, the all-to-all
 * as one peer copy per ordered pair, row transforms, every device pushes its rows back and home restores the natural order.  Same values as
 * aleo_mi355x_ntt_fr_device.  Blocking (the result is complete on return); `stream`: the stream the data was produced on (NULL = the slot's own).  The prover
 * routes its transforms of >= 2^24 elements (aleo_mi355x_bases_shard_transforms sets the size) through this entry when its committer key has shards attached (aleo_mi355x_bases_attach_shards): the
 * "NTT coefficients" half of "large proofs shard MSM bases and NTT coefficients across the GPUs". */
int32_t aleo_mi355x_ntt_fr_sharded_device(void* d_inout, uint32_t lg_n, int32_t direction, int32_t type, const int32_t* devices, size_t n_devices, void* stream);

/* a5 — KZG10::commit shape (commit_lagrange is the same call over the pinned Lagrange-basis powers with evaluations as
 * the scalars): coefficients in Montgomery form (as polynomials are stored), converted to canonical
 * bigints on the device, MSM over the first n pinned bases; affine result as snarkVM Affine (104 bytes, host). */
int32_t aleo_mi355x_kzg_commit(void* out_affine104, uint64_t handle, const void* coeffs_mont, size_t n);
/* Device-resident coefficients (e.g. straight out of aleo_mi355x_ntt_fr_device: no host round trip). */
int32_t aleo_mi355x_kzg_commit_device(void* out_affine104, uint64_t handle, const void* d_coeffs_mont, size_t n, void* stream);

/* The commitments of ONE prover round in one call.  Varuna commits 3*instances+1, then 2, 3 and 1 polynomials per round
 * (snarkvm-algorithms 0.14.5 snark/varuna/ahp/prover/round_functions [UPSTREAM-RECALL], reached from
 * /root/reference/rust/src/program/execute.rs:74), each by its own KZG10::commit -> VariableBase::msm from a rayon worker; at real
 * circuit sizes (2^14..2^17 coefficients) one such MSM is latency-bound on a GPU.  Here k coefficient vectors (k DEVICE
 * pointers and k lengths, both arrays in host memory) go against prefixes of ONE pinned SRS and share every launch: one sort
 * over k bucket sets, one accumulation, one reduction (pinned sets with a precomputed table; otherwise the call degrades to
 * k MSMs).  Results: k rows, in the order given — 144-byte Jacobian for msm_g1_batch_device (canonical scalars), snarkVM Affine
 * (104 bytes) for the kzg_commit_batch forms (Montgomery coefficients).  Each result is bit-identical to the single-vector call. */
int32_t aleo_mi355x_msm_g1_batch_device(void* out_jacobian, uint64_t handle, const void* const* d_scalars, const size_t* lens, size_t k, void* stream);
int32_t aleo_mi355x_kzg_commit_batch_device(void* out_affine104, uint64_t handle, const void* const* d_coeffs_mont, const size_t* lens, size_t k, void* stream);
/* Same with the k coefficient vectors in host memory (k host pointers). */
int32_t aleo_mi355x_kzg_commit_batch(void* out_affine104, uint64_t handle, const void* const* coeffs_mont, const size_t* lens, size_t k);

/* SonicKZG10::commit for the labelled polynomials of one round [UPSTREAM-RECALL: algorithms/src/polycommit/sonic_pc/mod.rs commit() ->
 * kzg10::KZG10::commit per polynomial with `powers` or, for a degree bound d, `shifted_powers` = powers_of_beta_g[max_degree - d ..], plus
 * a random polynomial against powers_of_beta_times_gamma_g when a hiding bound is set].  Every commitment is a SUM OF SEGMENTS over one
 * pinned set: a segment multiplies `len` Montgomery coefficients with the bases [base_offset, base_offset + len) and adds into commitment
 * `output`.  Plain polynomial: one segment at offset 0.  Degree bound d: one segment at offset max_degree - d.  Hiding: a second segment
 * for the blinding polynomial at the offset where the caller pinned the gamma powers behind the powers (one pinned array: powers |
 * gamma powers).  All segments of all commitments share one launch chain, like kzg_commit_batch.  out: n_outputs snarkVM Affine rows. */
typedef struct { const void* scalars; size_t len; size_t base_offset; uint32_t output; } aleo_mi355x_commit_segment;
int32_t aleo_mi355x_kzg_commit_segments(void* out_affine104, size_t n_outputs, uint64_t handle, const aleo_mi355x_commit_segment* segments, size_t n_segments);
int32_t aleo_mi355x_kzg_commit_segments_device(void* out_affine104, size_t n_outputs, uint64_t handle, const aleo_mi355x_commit_segment* segments, size_t n_segments, void* stream);
/* the same with the hint that the scalars are sparse (mostly 0 / 1): served from the set's range table (bases_precompute_range) when all segments lie inside it */
int32_t aleo_mi355x_kzg_commit_segments_sparse_device(void* out_affine104, size_t n_outputs, uint64_t handle, const aleo_mi355x_commit_segment* segments, size_t n_segments, void* stream);
/* e2 — commitments, and whole proofs, over several devices of this process (BASELINE north_star: "large proofs shard MSM bases ... across the 8 GPUs";
 * the reference's host is one process proving under spawn_blocking: /root/reference/rust/develop/src/routes.rs:119,149,229 -> rust/src/program/execute.rs:74).
 * The committer key is pinned twice: whole on the prover's device (bases_pin / bases_from_scalars — without tables it costs 224 bytes per power) and as
 * a sharded copy (bases_pin_sharded with precompute: each device holds 1/G of the powers and of the window tables, the part that needs the memory).
 *   kzg_commit_segments_sharded_device / kzg_commit_batch_sharded_device: the segment / batch commitment of kzg_commit_segments_device against the SHARDED
 *     set.  The coefficient vectors are device memory of the calling thread's current device; a segment [offset, offset + len) is cut at the shard
 *     boundaries, device g pulls its pieces (hipMemcpyPeerAsync over xGMI; no copy on the vectors' own device) and runs the ordinary batched Pippenger
 *     against its shard; n_outputs x 144 bytes per shard come back and are added on the host in shard order.  Same bytes as the single-device call.
 *   bases_attach_shards(handle, sharded_handle, min_points): from then on every commitment the PROVER makes against `handle` (varuna_index_build,
 *     varuna_prove*, the lockstep call) with at least min_points scalars in all goes through the sharded copy instead; the rounds' field work and the
 *     transcript stay on the prover's device, its transforms from a size of their own on take the shards' devices too (bases_shard_transforms below).  Same proof bytes.  sharded_handle 0 detaches. */
int32_t aleo_mi355x_kzg_commit_segments_sharded_device(void* out_affine104, size_t n_outputs, uint64_t sharded_handle, const aleo_mi355x_commit_segment* segments, size_t n_segments, void* stream);
int32_t aleo_mi355x_kzg_commit_batch_sharded_device(void* out_affine104, uint64_t sharded_handle, const void* const* d_coeffs_mont, const size_t* lens, size_t k, void* stream);
int32_t aleo_mi355x_bases_attach_shards(uint64_t handle, uint64_t sharded_handle, size_t min_points);
/* With shards attached the prover also runs its TRANSFORMS of at least min_elements elements over the shards' devices (aleo_mi355x_ntt_fr_sharded_device above;
 * the device list must be a power of two, else they stay on the prover's device).  Default (also restored by every attach, and by min_elements = 0): 2^24 —
 * below that a single-device transform takes 0.1-2 ms and the three barriers and 2 (G - 1) peer copies per device of the split cost more than they save; a
 * deployment whose vectors do not fit one card sets it lower.  Same proof bytes for every value. */
int32_t aleo_mi355x_bases_shard_transforms(uint64_t handle, size_t min_elements);

/* KZG10::commit with a hiding bound: msm(powers, coeffs) + msm(gamma_powers, blinding_coeffs), affine result.
 * Both coefficient vectors are Montgomery Fr on the host; both base sets are pinned handles. */
int32_t aleo_mi355x_kzg_commit_hiding(void* out_affine104, uint64_t h_powers, const void* coeffs_mont, size_t n,
                                      uint64_t h_gamma_powers, const void* blinding_mont, size_t m);

/* Field-only vector kernels on device-resident Montgomery Fr data (the pointwise work between
 * NTTs in Varuna's rounds — Evaluations::{mul,add,sub}_assign, snarkvm_fields::batch_inversion).
 * op: 0 = a*b, 1 = a+b, 2 = a-b; dst may alias a or b; outputs canonical.  batch_inverse leaves zeros in place. */
#define ALEO_FR_OP_MUL 0
#define ALEO_FR_OP_ADD 1
#define ALEO_FR_OP_SUB 2
int32_t aleo_mi355x_fr_vec_op_device(void* d_dst, const void* d_a, const void* d_b, size_t n, int32_t op, void* stream);
int32_t aleo_mi355x_fr_batch_inverse_device(void* d_inout, size_t n, void* stream);
/* dst[i] = c0 + c1 * a[i] + c2 * b[i]: c0, c1, c2 are 32-byte Montgomery Fr in HOST memory (c0 NULL = 0); d_a / d_b may be NULL
 * (the term drops out; its constant is then ignored); dst may alias a or b.  The scalar-times-vector and blended forms of the AHP
 * rounds: alpha - h_i ahead of a batch inversion, eta-weighted sums, the linear combinations opened at beta and gamma
 * [UPSTREAM-RECALL: snark/varuna/ahp/prover/round_functions/{second,third,fourth}.rs]. */
int32_t aleo_mi355x_fr_lin_device(void* d_dst, size_t n, const void* c0_mont, const void* c1_mont, const void* d_a, const void* c2_mont, const void* d_b, void* stream);
/* dst[k] = first * ratio^k (first, ratio: 32-byte Montgomery Fr in HOST memory).  With first = a^(n-1), ratio = 1/a this is the
 * coefficient vector of u_H(a, X) = (v_H(a) - v_H(X)) / (a - X) for |H| = n, whose NTT over H is v_H(a) / (a - h): the values the second
 * and third AHP rounds need, without a field inversion on the device. */
int32_t aleo_mi355x_fr_powers_device(void* d_dst, size_t n, const void* first_mont, const void* ratio_mont, void* stream);
/* dst[i] = scale[i] * table1[idx1[i]] * table2[idx2[i]] (uint32 indices; d_scale and the second table may be NULL): the third round's
 * val(k) / ((alpha - row(k)) (beta - col(k))) from the two tables above, by the row / column index of every non-zero entry. */
int32_t aleo_mi355x_fr_gather_mul_device(void* d_dst, size_t n, const void* d_scale, const void* d_table1, const void* d_idx1, const void* d_table2, const void* d_idx2, void* stream);
/* out[q] = p_q(z_q) for k <= 12 polynomials in two launches (d_polys, lens, z_mont: host arrays of k device pointers / lengths /
 * 32-byte Montgomery points; d_out: k x 32 bytes, device): the evaluations a proof carries (z_b, g_1 at beta; g_a, g_b, g_c at gamma). */
int32_t aleo_mi355x_fr_eval_batch_device(void* d_out, const void* const* d_polys, const size_t* lens, const void* z_mont, size_t k, void* stream);
/* Prover randomness.  `seed` is 32 bytes of caller entropy per proof (what `rand::thread_rng()` is to the reference's call sites,
 * /root/reference/rust/src/program/execute.rs:74): the key of a ChaCha20 stream (20 rounds, 64-bit block counter, 64-bit nonce).  Element i =
 * the first candidate below r among the two 32-byte halves (little-endian, low 253 bits) of block(counter = i, nonce = attempt), attempt = 0, 1, ...
 * (rejection sampling: uniform over Fr).  _device writes elements first_index .. first_index + n - 1 in HBM, canonical or (montgomery != 0)
 * Montgomery; aleo_mi355x_fr_random is the same stream on the host (out: n x 32 bytes canonical) — counter-based, so the host draws the handful
 * of blinding scalars of a proof while the device draws the 3|H| mask coefficients, and nothing is uploaded.  Never reuse a seed. */
int32_t aleo_mi355x_fr_random_device(void* d_dst, size_t n, const uint8_t seed[32], uint64_t first_index, int32_t montgomery, void* stream);
int32_t aleo_mi355x_fr_random(void* out, size_t n, const uint8_t seed[32], uint64_t first_index);
/* dst[i] = c0 [i == 0] + sum_j coeffs[j] * terms[j][i], term j contributing for i < lens[j] (k <= 28 terms; d_terms / lens / coeffs_mont
 * host arrays; c0_mont may be NULL): the linear combinations opened at beta and gamma, in one pass.  dst may be one of the terms (same offset). */
int32_t aleo_mi355x_fr_lincomb_device(void* d_dst, size_t n, const void* c0_mont, const void* const* d_terms, const size_t* lens, const void* coeffs_mont, size_t k, void* stream);
/* The numerators of the two sumchecks from evaluations already in HBM [UPSTREAM-RECALL: varuna/ahp/prover/round_functions/{second,fourth}.rs]:
 *   first:  dst = r (z_a + eta_b z_b + eta_c z_a z_b) - t z                  (n = 4|H| values each)
 *   matrix: dst = sum_M delta_M (vv val_M - (alpha beta - beta row_M - alpha col_M + row_col_M) f_M)   (n = 2|K| values; d_index[M] points at
 *           row_M, with col_M, val_M, row_col_M following at index_stride elements each; consts_mont = delta_a, delta_b, delta_c,
 *           alpha beta, -alpha, -beta, v_H(alpha) v_H(beta): 7 x 32 bytes on the host; a NULL d_index[M] leaves matrix M out — matrices whose
 *           non-zero domains differ in size are done one call each).  dst may alias an operand. */
/* Two layout steps of the first two rounds, one launch for all instances [UPSTREAM-RECALL: round_functions/{first,second}.rs]:
 *   blind_rows:         dst row q (n + 1 coefficients) = src row q (n coefficients) + rho_q (X^n - 1); rows <= 24, rho_mont: rows x 32 bytes on the host
 *   sumcheck_operands:  per instance i the rows  z_i = w_i (X^n_x - 1) + x_i,  z_a,i,  z_b,i  on 4n coefficients, zero padded (dst: 3 rows of 4n per
 *                       instance; d_witness_polys: 3 rows of n + 1 per instance in the order w, z_a, z_b; d_x_polys: n_x coefficients per instance) */
int32_t aleo_mi355x_fr_blind_rows_device(void* d_dst, const void* d_src, size_t n, size_t rows, const void* rho_mont, void* stream);
int32_t aleo_mi355x_ahp_sumcheck_operands_device(void* d_dst, const void* d_witness_polys, const void* d_x_polys, size_t n, size_t n_x, size_t instances, void* stream);
int32_t aleo_mi355x_ahp_first_sumcheck_device(void* d_dst, size_t n, const void* d_r, const void* d_za, const void* d_zb, const void* d_t, const void* d_z,
                                              const void* eta_b_mont, const void* eta_c_mont, void* stream);
int32_t aleo_mi355x_ahp_matrix_sumcheck_device(void* d_dst, size_t n, const void* const* d_index, size_t index_stride, const void* const* d_f, const void* consts_mont, void* stream);
/* Division by (X - z): quotient[j-1] = s_j with s_j = p_j + z s_(j+1) (n - 1 coefficients, canonical Montgomery form) and, when
 * d_eval != NULL, p(z) = s_0 (32 bytes, device) — KZG10's witness polynomial (p(X) - p(z)) / (X - z)
 * [UPSTREAM-RECALL: polycommit/kzg10 compute_witness_polynomial].  z_mont: 32 bytes Montgomery Fr in HOST memory.
 * d_quotient must not alias d_poly; it may be NULL when only the evaluation is wanted (d_eval then non-NULL). */
int32_t aleo_mi355x_fr_divide_by_linear_device(void* d_quotient, void* d_eval, const void* d_poly, size_t n, const void* z_mont, void* stream);
/* KZG10::open of one polynomial at one point (without hiding): the witness polynomial is built on the device and committed against
 * the first n - 1 pinned powers.  out_affine104: the opening proof's `w` (host); out_eval_mont (host, may be NULL): p(z). */
int32_t aleo_mi355x_kzg_open_device(void* out_affine104, void* out_eval_mont, uint64_t handle, const void* d_poly_mont, size_t n, const void* z_mont, void* stream);
/* y = M * x over Fr for a CSR matrix in device memory (row_ptr: uint32[rows + 1], col_idx: uint32[nnz], vals: Montgomery
 * Fr[nnz]); x and y Montgomery Fr vectors.  The z_a = A z, z_b = B z products of the R1CS matrices before round 1
 * [UPSTREAM-RECALL: snark/varuna/ahp/prover/round_functions/first.rs].  Empty rows give 0. */
int32_t aleo_mi355x_fr_spmv_device(void* d_y, const void* d_row_ptr, const void* d_col_idx, const void* d_vals, const void* d_x, size_t rows, void* stream);

/* ---- wire formats of the results (host code, no GPU needed) -------------------------------------------
 * What snarkVM does when a commitment / proof leaves the prover [UPSTREAM-RECALL: utilities/src/serialize, curves/.../affine.rs
 * CanonicalSerialize, synthesizer/snark Proof::to_bytes_le + bech32m Display]; pinned byte for byte by the `proof1...` string the
 * reference's own test holds (/root/reference/wasm/src/programs/transaction.rs:100, round-tripped at :104-120).
 * Compressed G1: 48 bytes little-endian canonical x; last byte bit 7 = y is the lexicographically larger root, bit 6 = infinity.
 * decompress rejects non-canonical x, x off the curve and (check_subgroup != 0) points outside the prime-order subgroup. */
int32_t aleo_mi355x_g1_compress(void* out48, const void* affine104, size_t n);
int32_t aleo_mi355x_g1_decompress(void* out_affine104, const void* in48, size_t n, int32_t check_subgroup);
/* Fr <-> 32 canonical little-endian bytes (Fr::to_bytes_le / from_bytes_le); from_bytes rejects values >= r. */
int32_t aleo_mi355x_fr_to_bytes(void* out32, const void* fr_mont, size_t n);
int32_t aleo_mi355x_fr_from_bytes(void* out_fr_mont, const void* in32, size_t n);
/* bech32m (BIP-350) strings: "proof1...", and every other Aleo object id.  encode writes a NUL-terminated string;
 * decode: *len in = capacity of out, out = payload bytes; hrp_out may be NULL. */
int32_t aleo_mi355x_bech32m_encode(char* out, size_t cap, const char* hrp, const void* data, size_t len);
int32_t aleo_mi355x_bech32m_decode(void* out, size_t* len, char* hrp_out, size_t hrp_cap, const char* s);
/* The byte layout of a Varuna proof (Proof::to_bytes_le) from its parts; points as snarkVM Affine (104 bytes), field elements
 * Montgomery Fr.  Field order read off the reference's own proof (one circuit, one instance).  The parts list g_a, g_b, g_c
 * and their evaluations circuit by circuit; the BYTES carry every g_a, then every g_b, then every g_c (one vector per matrix, as upstream's
 * Commitments / Evaluations structs hold them [UPSTREAM-RECALL] — unverified for more than one circuit: no such reference vector exists; with one
 * circuit both orders coincide).  n_evaluations must be instances + 1 + 3 n_circuits.  *len: in = capacity of out, out = bytes written. */
typedef struct {
  const uint64_t* batch_sizes; size_t n_circuits;      /* instances per circuit */
  const void* witness_commitments;                      /* 3 per instance: w, z_a, z_b */
  const void* mask_poly;                                /* NULL = None (non-hiding) */
  const void* g_1; const void* h_1;
  const void* g_abc;                                    /* 3 per circuit: g_a, g_b, g_c */
  const void* h_2;
  const void* evaluations; size_t n_evaluations;        /* z_b per instance, g_1, then g_a, g_b, g_c per circuit */
  const void* sums;                                     /* 3 per circuit (third-round sums) */
  const void* opening_points; const void* opening_random_v; const uint8_t* opening_has_v; size_t n_openings;   /* KZG10 proofs: w, Option<random_v> */
} aleo_mi355x_proof_parts;
int32_t aleo_mi355x_proof_to_bytes(void* out, size_t* len, const aleo_mi355x_proof_parts* parts);

/* ---- one proof in one call: the host side of Varuna::prove_batch, native (aleo_amd/csrc/varuna*.hip) ------------------------------
 * Replaces the CPU work snarkVM 0.14.5 does in algorithms/src/snark/varuna/{varuna.rs, ahp/prover/round_functions} [UPSTREAM-RECALL]
 * under /root/reference/rust/src/program/execute.rs:74 and transfer.rs:99 — for one circuit with 1..32 instances, upstream's Fiat-Shamir construction (the Poseidon
 * sponge over Fq, rate 2: aleo_mi355x_fs_* below) and the committer key the caller pinned (DESIGN.md 4d lists what differs from upstream).  The index is the prover-key material of the
 * circuit, built once (aleo_amd/varuna.py CircuitIndex does it through the entry points above) and described by device pointers:
 *   positions     host, uint32[n_vars]: index on H of every variable (public inputs on the subgroup X); positions_device: a copy in HBM (optional)
 *   a_*, b_*      device CSR of A, B with columns moved to positions on H and rows padded to n_h (uint32 row_ptr[n_h+1], col[], Montgomery val[])
 *   t_*           device CSR of the stacked transpose [A^T | B^T | C^T] (rows = positions on H, columns = matrix * n_h + row)
 *   vx_inv        device Fr[n_h]: 1 / v_X on H \ X, 0 on X
 *   k_evals       device Fr, matrix after matrix: row, col, val, row_col of M on K_M (|K_M| values each; matrix M starts at element 4 * (sum of the
 *                 earlier |K|));  k_idx  device uint32, matrix after matrix: row positions, column positions (|K_M| each; M starts at 2 * sum)
 *   k_polys       the same four polynomials per matrix as coefficients (layout of k_evals);  k2_evals  their values on the domain of size 2|K_M|
 *                 (2|K_M| each; M starts at element 8 * sum)
 *   vk_bytes      host: the circuit's verifying key as bytes (12 compressed index commitments, 5 domain sizes); vk_affine: the commitments as the
 *                 transcript absorbs them (12 x 104-byte G1Affine; NULL = decompress vk_bytes per proof)
 * committer_key: a pinned set holding powers[0..max_degree] and, from gamma_offset, at least 3 hiding powers; when lagrange_offset != 0 also, from
 * lagrange_offset, the n_h Lagrange-basis powers L_i(tau) G of the domain H followed by v_H(tau) G: w, z_a, z_b are then committed from their
 * EVALUATIONS (KZG10::commit_lagrange: the same group elements; a witness of bits stays a vector of small scalars for the MSM).
 * assignments: n_instances host pointers to n_vars x 32 bytes canonical (public variables first, z_0 = 1).  seed: 32 bytes of fresh
 * entropy per proof, the key of the proof's random stream (aleo_mi355x_fr_random_device; a repeated seed repeats the blinding).  out_proof / len: Proof::to_bytes_le layout, 901 + 176 (n_instances - 1) bytes; *len in = capacity.
 * Blocking; concurrent calls from several threads run on separate slots.  aleo_mi355x_varuna_last_timing: wall ms of the calling thread's
 * last proof: rounds 1..4, openings, total, time inside the five commitment calls, their host tails. */
typedef struct {
  uint64_t n_h, n_k_a, n_k_b, n_k_c, n_x, n_public, n_vars;      /* |H|, the non-zero domains |K_A|, |K_B|, |K_C|, |X| */
  uint64_t committer_key, max_degree, gamma_offset, lagrange_offset;
  const uint32_t* positions;
  const void* positions_device;      /* the same array in HBM (may be NULL: the assignment is then laid out on H by the host) */
  const void *a_row_ptr, *a_col, *a_val, *b_row_ptr, *b_col, *b_val, *t_row_ptr, *t_col, *t_val;
  const void *vx_inv, *k_evals, *k_idx, *k_polys, *k2_evals;
  const void* vk_bytes; size_t vk_len;
  const void* vk_affine;             /* the twelve index commitments as 104-byte G1Affine (what the transcript absorbs); may be NULL: decompressed from vk_bytes per proof */
  uint64_t max_row[3];               /* hints (0 = unknown): an upper bound of the longest row of a_*, b_*, t_* — the prover skips the launches for long (> 64) / huge (> 8192) rows of a
                                      * sparse product that cannot have any (index_build fills them; a caller-built struct may leave them 0) */
} aleo_mi355x_varuna_index;
/* The index built by the library itself from the R1CS (AHPForR1CS::index shape: the arithmetisation above + the twelve index commitments)
 * and kept in HBM under a handle.  Matrices: CSR over the variables (uint32 row_ptr[n_constraints + 1], uint32 col[nnz] = variable index
 * with the n_public public variables first, val[nnz] canonical 32-byte Fr), host memory.  Domains: |X| = 2^ceil(lg n_public), |H| = the power
 * of two >= max(n_constraints, |X| + n_private, 2|X|), |K_M| = the power of two >= the non-zero count of M (>= 2), one per matrix
 * (domain_flags 1), all three the largest of them (2), or (0) shared below 2^18 — latency-bound rounds, one batched transform beats three short
 * ones — and per matrix from there on.  The
 * committer key (powers[0..max_degree], >= 3 hiding powers from gamma_offset) must hold max(3|H|, max |K_M|) powers and stays pinned while the index lives.
 * index_export fills the struct view (pointers owned by the library, valid until index_free; the transposed matrices t_* list the entries of a column in no
 * fixed order — they are written through an atomic cursor — which the exact field sums over them do not see, but two builds of one circuit may differ there);
 * index_vk copies the bytes the transcript absorbs
 * first: 12 compressed index commitments (row, col, val, row_col of A, B, C) then |H|, |K_A|, |K_B|, |K_C|, |X| as u64 LE.  prove_indexed = varuna_prove. */
typedef struct { const uint32_t* row_ptr; const uint32_t* col; const void* val; } aleo_mi355x_r1cs_matrix;
int32_t aleo_mi355x_varuna_index_build(uint64_t* index_handle, uint64_t committer_key, uint64_t max_degree, uint64_t gamma_offset, uint64_t lagrange_offset,
                                       const aleo_mi355x_r1cs_matrix abc[3], size_t n_constraints, size_t n_public, size_t n_private, uint32_t domain_flags);
int32_t aleo_mi355x_varuna_index_export(uint64_t index_handle, aleo_mi355x_varuna_index* out);
int32_t aleo_mi355x_varuna_index_vk(uint64_t index_handle, void* out, size_t* len);
int32_t aleo_mi355x_varuna_index_free(uint64_t index_handle);
int32_t aleo_mi355x_varuna_prove_indexed(uint64_t index_handle, const void* const* assignments, size_t n_instances, const uint8_t seed[32], void* out_proof, size_t* len);
int32_t aleo_mi355x_varuna_prove(const aleo_mi355x_varuna_index* index, const void* const* assignments, size_t n_instances, const uint8_t seed[32], void* out_proof, size_t* len);
/* One proof over SEVERAL circuits — upstream's `Varuna::prove_batch(keys_to_constraints: BTreeMap<&ProvingKey, &[Assignment]>)`, what
 * `Trace::prove_execution` / `prove_fee` build from the transitions of a transaction (/root/reference/rust/src/program/execute.rs:74).
 * index_handles: 1..32 indexes built against ONE committer key (same max_degree / gamma_offset), in the order the proof lists them;
 * n_instances[j]: the assignments of circuit j — at most 32 over all circuits, in any split (one proof covers one transaction: snarkVM allows 32 transitions); assignments: the pointers of circuit 0's instances, then circuit 1's, ...
 * The cap of 32 instances is this library's (the protocol has none; snarkVM's transactions carry at most 32 transitions): a request beyond it is
 * refused with ALEO_MI355X_ERR_BAD_ARG before any launch and the caller falls back (CPU prover).  One proof is one object: the library never splits
 * a request into several proofs on its own.
 * The circuits share the transcript and every challenge, one mask / g_1 / h_1 over the largest constraint domain, one h_2 over the largest non-zero
 * domain and the two openings; a smaller circuit enters behind the selector v_{H*} / v_{H_j}.  out_proof: Proof::to_bytes_le layout —
 * batch sizes, 3 witness commitments per instance, mask, g_1, h_1, every g_a, every g_b, every g_c (one vector per matrix over the circuits,
 * [UPSTREAM-RECALL]; unverifiable offline for more than one circuit — the reference's proof string has one), h_2, evaluations (z_b's, g_1,
 * then g_a / g_b / g_c likewise), sums per circuit, openings.  With one circuit
 * the bytes are those of aleo_mi355x_varuna_prove_indexed.  ALEO_MI355X_ERR_UNSATISFIED if any assignment violates its circuit. */
int32_t aleo_mi355x_varuna_prove_batch_indexed(const uint64_t* index_handles, size_t n_circuits, const void* const* assignments, const size_t* n_instances, const uint8_t seed[32],
                                               void* out_proof, size_t* len);
/* Several INDEPENDENT proofs in one call, proved in lockstep (a serving path: the reference's dev server proves concurrent requests from
 * tokio::task::spawn_blocking threads, /root/reference/rust/develop/src/routes.rs:119,149,229 — a front end that collects them calls this instead of
 * n separate proves).  Every request is one prove_batch_indexed call's worth — its own circuits, assignments, 32-byte seed, transcript and output —
 * and comes out byte for byte as that call would give it; what the requests share is every commitment launch chain: round r of all of them is ONE
 * batched MSM, so its sort, slice tree, reduction, host tail and stream synchronisation are paid once per round instead of once per proof
 * (eight 2^15-constraint proofs: see DESIGN.md 4d).  All indexes must belong to one committer key.  len: in = capacity of out_proof, out = bytes
 * written.  status (out): per request — a request that fails (unsatisfied assignment: ALEO_MI355X_ERR_UNSATISFIED; bad argument) drops out, the
 * others complete; the call itself returns non-zero only when nothing could be started or a device call failed.  1..64 requests.
 * Between the commitments the proofs run on up to ALEO_MI355X_LOCKSTEP_WORKERS (default 4, 1..9) threads of the library's own, each with a
 * borrowed stream of the device: the calling thread blocks until all proofs are written. */
typedef struct {
  const uint64_t* index_handles; size_t n_circuits; const void* const* assignments; const size_t* n_instances; const uint8_t* seed;
  void* out_proof; size_t len; int32_t status;
} aleo_mi355x_prove_request;
int32_t aleo_mi355x_varuna_prove_many(aleo_mi355x_prove_request* requests, size_t n_requests);
int32_t aleo_mi355x_varuna_last_timing(double* out_ms, int32_t cap);

/* snarkVM's Poseidon on the host (no GPU needed).  Parameters: Grain LFSR, alpha = 17, 8 full + 31 partial rounds, capacity 1 [UPSTREAM-RECALL:
 * snarkvm-fields poseidon_default; pinned over Fr by the reference's private-key ciphertext and account vectors, tests/test_poseidon.py].
 *   poseidon_hash_fr: `Network::hash_many_psd{2,4,8}` — rate = 2, 4 or 8; inputs / outputs canonical 32-byte Fr; preimage = [domain
 *   "AleoPoseidon{rate}", n_inputs, 0.., inputs] (what /root/reference/rust/src/account/encryptor.rs:37-67 calls through hash_psd2).
 *   fs_*: the prover's Fiat-Shamir sponge — PoseidonSponge<Fq, 2, 1> behind upstream's AlgebraicSponge interface: bytes (bits of every byte most
 *   significant first, 376-bit chunks), G1Affine points (x, y Montgomery, stride 104 or 96; infinity as (0, 1)), Fr elements as non-native limbs
 *   (canonical input, 5 x 51 bits packed two per Fq element), challenges (canonical output): `short_` = 0: 252 bits each from ONE squeeze of
 *   ceil(252 n / 376) elements (squeeze_nonnative_field_elements(n)); 1: 168 bits (squeeze_short_nonnative_field_elements(n)).
 *   aleo_mi355x_varuna_prove* run this sponge inside the library; the entry points exist for a host side that drives the rounds itself
 *   (aleo_amd/varuna.py) and for verifiers. */
int32_t aleo_mi355x_poseidon_hash_fr(uint32_t rate, const void* inputs, size_t n_inputs, void* out, size_t n_out);
/* the round constants ark[39][rate + 1] and the matrix mds[rate + 1][rate + 1] (row-major, canonical 32-byte Fr) of that hash: what a circuit constraining it needs */
int32_t aleo_mi355x_poseidon_parameters_fr(uint32_t rate, void* ark_out, void* mds_out);
int32_t aleo_mi355x_fs_new(uint64_t* sponge);
int32_t aleo_mi355x_fs_free(uint64_t sponge);
int32_t aleo_mi355x_fs_absorb_bytes(uint64_t sponge, const void* data, size_t len);
int32_t aleo_mi355x_fs_absorb_g1(uint64_t sponge, const void* affine, size_t stride, size_t count);
int32_t aleo_mi355x_fs_absorb_fr(uint64_t sponge, const void* fr_canonical, size_t count);
int32_t aleo_mi355x_fs_squeeze_fr(uint64_t sponge, void* out_canonical, size_t count, int32_t short_);

/* Element-wise field products on the device (host pointers): r[i] = a[i]*b[i], Montgomery form, canonical
 * output.  Used by the parity tests to pin the device arithmetic against the oracle limb for limb; when a and b
 * are the same buffer the dedicated squaring block runs instead of the general product. */
int32_t aleo_mi355x_fq_mul(void* r, const void* a, const void* b, size_t n);
int32_t aleo_mi355x_fr_mul(void* r, const void* a, const void* b, size_t n);

/* Test hook: `lanes` device lanes each run `steps` mixed additions of pseudo-random field elements through the 28-bit-limb
 * formulas of the accumulation kernel and through the 32-bit ones, comparing every intermediate as canonical residues
 * (and that both refuse P == acc).  *failures = number of lanes that disagreed. */
int32_t aleo_mi355x_selftest_madd28(uint32_t lanes, uint32_t steps, uint64_t seed, uint32_t* failures);
/* The lane-quad XYZZ addition of the reduction chains against the lane-pair one on `ops` random operand pairs and the special cases
 * (identity operands, equal points, opposite points): *failures = number of disagreements (mod q, all four coordinates). */
int32_t aleo_mi355x_selftest_addquad(uint32_t ops, uint64_t seed, uint32_t* failures);
/* The same formulas on rows the caller built, raw 28-bit limbs in and out (host memory; the device converts nothing), so that a test can place
 * representatives at the edges of the stored invariant (X exact digits < 12q; Y limbs < 3 * 2^28, < 6q; ZZ, ZZZ exact digits < 2q; identity <=> ZZ all zero)
 * and compare with the group law in integers.  Additions: a224[i] + b224[i] (224-byte rows X | Y | ZZ | ZZZ of 14 limbs each) by one lane quad per row, into
 * out_quad224[i]; lanes 0 and 1 of the quad run the lane-pair form into out_pair224[i].  Mixed additions: acc224[i] (X exact < 12q, Y exact < 2q or the
 * limb-wise 2q - y, ZZ / ZZZ exact < 2q) + pt112[i] (x | y canonical, or y the limb-wise 2q - y) by one lane per row; out_acc224[i] = acc afterwards,
 * ok_u8[i] = what the formula returned (0: the point is +-acc and acc is untouched).  Either count may be 0 (its pointers are then ignored); at most 2^20. */
int32_t aleo_mi355x_selftest_f28_rows(const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224,
                                      const void* acc224, const void* pt112, uint32_t n_madd, void* out_acc224, uint8_t* ok_u8);
/* The Edwards-form formulas of the whole-set table tier (te28.h) on rows the caller built, the same way.  A point is a 224-byte row X | Y | Z | T of 14 limbs each,
 * every coordinate exact digits < 2q; the identity is the ordinary point (0 : Z : Z : 0).  Additions: a224[i] + b224[i] by one lane quad per row into
 * out_quad224[i], lanes 0 and 1 of the quad run the lane-pair form into out_pair224[i]; z_add_u32[i] bit 0 / bit 1: the pair / quad form reported Z3 == 0
 * (operands that differ by a point of even order: outside what the unified law covers).  Mixed additions: acc224[i] + the entry row168[i] (y - x | y + x | 2d x y of
 * the Edwards image, canonical digits) by one lane per row; how_u8[i] bit 0: the entry is negated on the device first, bit 1: the entry starts a slice (acc224[i] is
 * ignored); out_acc224[i] = the sum, z_madd_u8[i] = 1 if Z3 == 0 was reported.  Either count may be 0 (its pointers are then ignored); at most 2^20. */
int32_t aleo_mi355x_selftest_te28_rows(const void* a224, const void* b224, uint32_t n_add, void* out_pair224, void* out_quad224, uint32_t* z_add_u32,
                                       const void* acc224, const void* row168, const uint8_t* how_u8, uint32_t n_madd, void* out_acc224, uint8_t* z_madd_u8);

/* The 29-bit-limb form of Fr (csrc/fr29.h: 9 limbs, Montgomery with R = 2^261) and the Edwards helpers on it (csrc/edwards29.h) on rows the caller built, raw
 * limbs in and out (host memory; the device converts nothing), one lane per row, so that a test can place every limb at the edge of an operand class and compare
 * with integers.  An element is 9 u32, a point 36 u32 (X | Y | Z | T; each coordinate exact digits below 3 r).  out_mul36[i] = f29_mul(mul_a36[i], mul_b36[i])
 * (a: limbs below 2^31.4, value below 2^261; b: limbs 0..7 digits); out_tidy36[i] = f29_tidy(tidy36[i]) (any limbs whose carries fit, value below 445 r);
 * out_canon36[i] = f29_canonical(canon36[i]) (a multiplicand); out_add144[i] = p144[i] + q144[i], or p144[i] - q144[i] where neg_u8[i] != 0, by ed29_add onto
 * ed29_cache(q144[i], d2_36) with d2_36 the limbs of 2 d in Montgomery form; out_dbl144[i] = 2 dbl144[i] by ed29_dbl, which computes T only where want_t_u8[i] != 0
 * (the T that came in is stored otherwise).  Outputs are filled with 0xA5 before the kernels run.  A count may be 0 (its pointers are then ignored); at most 2^20 each. */
int32_t aleo_mi355x_selftest_ed29_rows(const void* mul_a36, const void* mul_b36, uint32_t n_mul, void* out_mul36, const void* tidy36, uint32_t n_tidy, void* out_tidy36,
                                       const void* canon36, uint32_t n_canon, void* out_canon36, const void* p144, const void* q144, const uint8_t* neg_u8, const void* d2_36,
                                       uint32_t n_add, void* out_add144, const void* dbl144, const uint8_t* want_t_u8, uint32_t n_dbl, void* out_dbl144);

/* The slice stage of the MSM sort alone (bucket scan, top scan, slice ordering) on a histogram from the host: hist[g] = points of bucket g, n_buckets <= 2^20,
 * total_pairs = the pair count the slice rule is picked from (the sum of hist or more: less is refused); fused != 0 runs the top scan inside the ordering kernel, as the
 * chains of a proof do.  *violations = how often what the device left behind breaks one of: `order` is a permutation of the slice ids; slice lengths never increase along
 * it; task_g[sid] is the bucket whose slice range holds sid; the length counts, the slice metadata (device and host copy) and both multi-slice bucket lists (as
 * sets) equal a host recount. */
int32_t aleo_mi355x_selftest_slice_order(const uint32_t* hist, uint32_t n_buckets, uint32_t total_pairs, int32_t fused, uint32_t* violations);

/* The scalar sort of the MSMs alone (signed balanced digits, both levels of the counting sort, as every G1 and G2 call runs them), on host memory, and what it left
 * behind copied back.  scalars: the segments' scalars one after another, 32 bytes each (canonical, or Montgomery form where mont != 0); segment q has seg_n[q] >= 1
 * scalars for the bases seg_off[q] .. of the set and adds into result seg_set[q]; nseg <= 64.  c = window width, pre != 0 the table path (every window of a set shares
 * its 2^(c-1) buckets; the index of digit w of scalar i is w * row_stride + off + i), pre == 0 the plain path (bucket sets per window; the index is off + i; k_sets == 1,
 * every seg_set 0).  inf_u8: NULL, or row_stride bytes: scalar i of segment q is skipped where inf_u8[off + i] != 0.  tile: 0 for the level-1 tile the sort picks itself,
 * or 2048, 4096, 8192.  With W = ceil(254 / c):  hist_out[M], M = (pre ? k_sets : W) * 2^(c-1): hist_out[g] = indices in bucket g;  sorted_out[sorted_cap], sorted_cap >=
 * (sum of seg_n) * W: uploaded as it comes (fill it with a value no index takes), sorted, and the first (sum of seg_n) * W words copied back: bucket g's indices (bit 31:
 * negative digit) at [prefix(g), prefix(g) + hist_out[g]) in any order, the rest untouched;  *pairs_out = the pair count of the level-1 scan.
 * ALEO_MI355X_ERR_BAD_ARG, and nothing launched: a (c, pre) without a sort instance (plain 2..16; table 13, 16, 17, 20), more sets than a chain of that width holds
 * (32, 32, 16, 2), a set >= k_sets, an empty segment, off + n > row_stride, W * row_stride >= 2^31, more than 2^20 scalars, a short sorted_out. */
int32_t aleo_mi355x_selftest_sort_pairs(const void* scalars, const uint32_t* seg_n, const uint32_t* seg_off, const uint8_t* seg_set, uint32_t nseg, int32_t c, int32_t pre, int32_t mont,
                                        uint32_t k_sets, uint32_t row_stride, const uint8_t* inf_u8, uint32_t tile, uint32_t* hist_out, uint32_t* sorted_out, size_t sorted_cap, uint32_t* pairs_out);

/* The lane-pair Fq2 arithmetic of the G2 path (g2.hip: components of an Fq2 value across two lanes, 28-bit limbs) against the one-lane 32-bit code on
 * chains over n_points affine G2 points (192-byte rows, host memory, >= 3 of them, all on the curve): sums, a sum with a shared operand, a doubling, the
 * same-point case of the addition.  failures2[0] = pairs that disagreed, failures2[1] = OR of the failing steps (1 a, 2 s, 4 u, 8 2u, 16 u + u). */
int32_t aleo_mi355x_selftest_g2pair(const void* affine192, uint32_t n_points, uint32_t n_pairs, uint32_t* failures2);
/* The lane-pair formulas themselves (csrc/g2p28.h) on rows the caller built, raw 28-bit limbs in and out (host memory; the device converts nothing), so that a
 * test can place every component of every coordinate where the stored invariant allows it and compare with the group law in integers.  A point is a 448-byte row
 * X.a | X.b | Y.a | Y.b | ZZ.a | ZZ.b | ZZZ.a | ZZZ.b of 14 limbs each (an Fq2 value a + b u): X exact digits < 12q, Y exact < 6q, ZZ / ZZZ exact < 2q per
 * component; the identity is the all-zero row.  One lane pair per row.  Additions: out_add448[i] = a448[i] + b448[i] (g2p_add_any: any operand may be the
 * identity, they may be equal or opposite).  Doublings: out_dbl448[i] = 2 d448[i] (g2p_double_any).  Mixed additions: acc448[i] + the entry ent224[i]
 * (x.a | y.a | x.b | y.b, exact digits < 2q; canonical where neg_u8[i] != 0, which has the device negate it first as the accumulation kernel does) through
 * g2p_madd_fast; out_acc448[i] = acc afterwards, ok2_u8[2 i] and ok2_u8[2 i + 1] = what the formula returned to the even and to the odd lane (0: the point is
 * +-acc and acc is untouched).  Outputs are filled with 0xA5 before the kernels run.  A count may be 0 (its pointers are then ignored); at most 2^20 each. */
int32_t aleo_mi355x_selftest_g2p_rows(const void* a448, const void* b448, uint32_t n_add, void* out_add448, const void* d448, uint32_t n_dbl, void* out_dbl448,
                                      const void* acc448, const void* ent224, const uint8_t* neg_u8, uint32_t n_madd, void* out_acc448, uint8_t* ok2_u8);

/* Host arithmetic (no device needed): the inversion the host tails use — Bernstein-Yang divsteps on 62-bit limbs (csrc/host_modinv.hpp) — against the Fermat
 * chain a^(p-2) on `count` pseudo-random elements of Fq and of Fr plus the edge values 0, 1, 2, p - 1, p - 2: *failures = results that differ; ns_per_inverse
 * (optional, 4 doubles): divsteps / Fermat for Fq, divsteps / Fermat for Fr. */
int32_t aleo_mi355x_selftest_host_inverse(uint32_t count, uint64_t seed, uint32_t* failures, double* ns_per_inverse);

/* Test hook: the Fr vector kernels that only the native prover launches (csrc/frops.h), one host function per call, on the serving slot's stream, complete on
 * return.  ptrs: device pointers (a pointer named "or NULL" may be absent); sizes: element counts; consts_mont: 32-byte Montgomery constants on the host.
 *   step 0  fr_add_tiled        ptrs = dst, src                        sizes = n, n_src                      dst[i] += src[i mod n_src]
 *   step 1  fr_sub_mul          ptrs = dst, a, b, m                    sizes = n                             dst = (a - b) m
 *   step 2  fr_scale_rows       ptrs = dst, src                        sizes = n, rows      consts = rows    dst[r][i] = k_r src[i]
 *   step 3  fr_pick             ptrs = dst, src_0 .. src_{count-1}     sizes = count                         dst[j] = *src_j
 *   step 4  fr_gather_mul3      ptrs = table1, table2, then (dst, scale, idx1, idx2) per range      sizes = count, n_0 .. n_{count-1}
 *   step 5  fr_scatter_to_mont  ptrs = dst, src, pos, flag or NULL     sizes = n                             dst[pos[v]] = to_mont(src[v]); *flag |= 1 if a src[v] >= r
 *   step 6  fr_split_quotient   ptrs = hq, rq, q, mask or NULL, host_sum or NULL    sizes = n                hq = [p1 + p2 | p2], rq = p0 + p1 + p2 (host_sum = rq[0])
 * What a host function refuses (a block size that does not divide n, 5 rows, 9 picks, 0 or 4 ranges) comes back as its status.  ALEO_MI355X_ERR_BAD_ARG for an
 * unknown step, a null array, or a null pointer the step needs. */
int32_t aleo_mi355x_selftest_fr_step(uint32_t step, const void* const* ptrs, const size_t* sizes, const void* consts_mont);

/* Per-call instrumentation of the calling thread's most recent MSM: milliseconds per phase
 * [0] total, [1] digit/sort, [2] bucket accumulation incl. slice tree, [3] bucket reduction, [4] host tail,
 * [5] the bucket-accumulation kernel alone (the dominant kernel bench.py prices against the roofline): mean duration of its launches,
 * [6] how many launches of it the call made (2 or 3 when host scalars went up in chunks whose accumulations are seeded from one another and share one reduction, else 1).
 * Returns the number of doubles written (<= cap). */
int32_t aleo_mi355x_last_msm_timing(double* out_ms, int32_t cap);

/* Routing thresholds for the drop-in: below these sizes the Rust arms keep the CPU path — a 2^6..2^12 host-buffer call costs two PCIe
 * copies and 20-50 us of launches against microseconds on a core.  Defaults = the crossovers measured for the cold one-shot calls against the CPU path on
 * the GPU box's host cores (bench.py cpu_baseline.crossover; profiles/r04_crossover.json); ALEO_MI355X_MIN_MSM / ALEO_MI355X_MIN_NTT override them. */
size_t aleo_mi355x_min_msm(void);
size_t aleo_mi355x_min_ntt(void);

/* The ownership scan of record ciphertexts: for every record of a batch, does the account own it?  What the reference asks record by record with
 * `record.is_owner_with_address_x_coordinate(&view_key, &address_x_coordinate)` (rust/src/api/blocking.rs:213-218, :274-276; RecordCiphertext.isOwner).
 *   record_parse   host: a "record1..." string -> owner variant (0 public, 1 private), the owner field (address x, or the one field c0 of the owner
 *                  ciphertext) and the nonce x, 32 canonical little-endian bytes each.  Refuses a wrong prefix or checksum, a private owner whose field count
 *                  is not 1, an entry that overruns the payload, trailing bytes and non-canonical fields.  Public owners are compared by the caller.
 *   records_scan   n private-owner records, all buffers on the host: owner_c0 and nonce_x n x 32 B canonical, view_key32 a canonical scalar below the
 *                  subgroup order, address_x32 the address's x.  flags[i] = 1 owner, 0 not owner, 2 malformed (c0 or the nonce not below r, or the nonce x not
 *                  on the curve); a malformed record never fails the batch.  rvk_out (optional, n x 32 B): the x of view_key * nonce — the record view key the
 *                  host decrypts an owned record with — zeros where the flag is 2.  Defined for EVERY on-curve x: where upstream would have refused the record
 *                  on parsing (no prime-order point with that x) the scan answers by the same formula; full validation stays with decryption.  Batches
 *                  below min_records run on the host inside the call.  Thread-safe (one slot per call); n = 0 is fine; large n goes through in chunks.
 *                  On the device it is records_scan_many with one key: ALEO_MI355X_SCAN_KEYS_PER_LANE (there) reaches it too, and the bytes do not depend on it.
 *   records_scan_host   the same bytes out, computed on the CPU by the calling thread; touches no device.
 *   min_records    the batch size from which records_scan takes the GPU: 64, the measured crossover against the host path on one thread (profiles/records_scan.txt: 0.88x at 2^5, 2.0x at 2^6); ALEO_MI355X_MIN_RECORDS overrides it, read per call. */
int32_t aleo_mi355x_record_parse(const char* record1, int32_t* owner_kind, void* owner32, void* nonce32);
int32_t aleo_mi355x_records_scan(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_key32, const void* address_x32);
int32_t aleo_mi355x_records_scan_host(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_key32, const void* address_x32);
size_t aleo_mi355x_min_records(void);

/* The same scan for SEVERAL accounts over one set of records in one call: what a front end asks that runs the record search for several callers over the same
 * blocks (the reference's dev server: rust/develop/src/routes.rs:112, :143, :194-220 -> rust/src/api/blocking.rs:229-292).
 *   records_scan_many   owner_c0, nonce_x: n x 32 B as for records_scan; view_keys32, address_xs32: n_keys x 32 B, key j's scalar and address x; 1 <= n_keys <= 64,
 *                  repeated keys allowed, n = 0 is fine.  flags (n_keys x n bytes, [key][record]) and rvk_out (optional, n_keys x n x 32 B): row j is byte for
 *                  byte what records_scan_host returns for key j alone.  A view key not below the subgroup order or an address x not canonical refuses the
 *                  call before any launch; last_error names the key's index.  The records go to the device once per chunk (a launch covers at most 2^22
 *                  pairs and 2^20 records); from 65 536 lanes per launch on, one lane answers a group of 2, 4 or 8 keys and shares among them what depends on
 *                  the record alone (csrc/records_many_lane.h; the widest group W that leaves the launch 65 536 lanes, with W / 2 < n_keys), below that one key per lane.
 *                  ALEO_MI355X_SCAN_KEYS_PER_LANE (1, 2, 4, 8; unset, 0 or anything else = that rule), read per call, forces the group's width; the bytes do not
 *                  depend on it.  A call with n * n_keys below min_records runs on the host.  Thread-safe (one slot per call).
 *   records_scan_many_host   the same bytes out from n_keys passes of the host path; touches no device. */
int32_t aleo_mi355x_records_scan_many(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys);
int32_t aleo_mi355x_records_scan_many_host(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys);
/* The record search straight from "record1..." strings: what a caller holds who reads records out of block JSON, as the reference does
 * (rust/src/api/blocking.rs:209-218, :264-276; RecordCiphertext.fromString).  The strings come in one blob and are decoded on the device: bech32m, checksum and
 * the layout walk of record_parse, one string per lane (csrc/records_strings_lane.h), writing the scan's inputs where the scan kernels read them.
 *   text, offsets  the strings one after another, no separators; offsets: n + 1 entries, offsets[0] = 0, nondecreasing; string i is text[offsets[i] .. offsets[i + 1]).
 *   records_parse_many   kinds[i] = 0 public owner, 1 private owner, -1 for a string record_parse refuses (a NUL inside a span, the empty span and a span of more
 *                  than 2^20 characters are refused); owner32 / nonce32 (n x 32 B): what record_parse writes, zeros where kinds[i] = -1.  A refused string is a
 *                  per-record answer, not a failed call.  Below min_records strings the call runs on the calling thread.
 *   records_parse_many_host   the same bytes out, computed on the CPU by the calling thread, with no allocation per string; touches no device.
 *   records_scan_strings   the scan of records_scan_many over the strings, 1 <= n_keys <= 64 (n_keys = 1 is the single scan; the width rule of records_scan_many
 *                  applies unchanged).  flags (n_keys x n bytes, [key][record]): 0 not owner, 1 owner, 2 malformed (as records_scan), 3 the string does not
 *                  parse.  A public owner is compared with the key's address x (flag 0 or 1; the nonce plays no part); a private owner goes through the scan.
 *                  rvk_out (optional, n_keys x n x 32 B): the x of view key * nonce for every string that parses, public owners included, zeros where the nonce
 *                  is malformed or the string does not parse.  kinds (optional, n): as records_parse_many.  The call fails only for null buffers, offsets that
 *                  decrease or do not start at 0, a key records_scan_many refuses, or a HIP error.  Chunks hold whole records, within the record and pair caps
 *                  of records_scan_many and 256 MiB of characters (ALEO_MI355X_SCAN_CHUNK_CHARS, read per call, lowers that cap: for tests; the bytes out do not
 *                  depend on it); an over-long string is not uploaded.  A call with n * n_keys below min_records runs on the host.  Thread-safe (one slot per call).
 *   records_scan_strings_host   the same bytes out, computed on the CPU by the calling thread; touches no device. */
int32_t aleo_mi355x_records_parse_many(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n);
int32_t aleo_mi355x_records_parse_many_host(int8_t* kinds, void* owner32, void* nonce32, const char* text, const uint64_t* offsets, size_t n);
int32_t aleo_mi355x_records_scan_strings(uint8_t* flags, int8_t* kinds, void* rvk_out, const char* text, const uint64_t* offsets, size_t n,
                                         const void* view_keys32, const void* address_xs32, size_t n_keys);
int32_t aleo_mi355x_records_scan_strings_host(uint8_t* flags, int8_t* kinds, void* rvk_out, const char* text, const uint64_t* offsets, size_t n,
                                              const void* view_keys32, const void* address_xs32, size_t n_keys);
/* Decrypting the records an account owns: what the reference does next with every record the search finds — `record.decrypt(&view_key)` and the sum of
 * `microcredits()` (rust/src/api/blocking.rs:274-283), RecordCiphertext.decrypt(viewKey) -> RecordPlaintext (wasm/src/record/record_ciphertext.rs:48-57).
 * snarkVM 0.14.5 console/program/src/data/record/decrypt.rs, ciphertext/decrypt.rs [UPSTREAM-RECALL], pinned by the reference's own ciphertext and plaintext
 * strings (tests/golden/reference_records.json) as far as they reach: a private owner, a private u64 entry, a public group nonce.
 *   The private fields of a record, in randomizer order: the owner's one field if the owner is private, then the fields of every private entry in entry order
 *   (m in all); randomizers = hash_many_psd8([domain "AleoSymmetricEncryption0", rvk], m), plain_i = c_i - randomizers_i, rvk the record view key's x that
 *   records_scan returns.  The owner's plain field is the address x; an entry's plain fields are one Plaintext in bits (252 per field).
 *   records_decrypt_fields   n records, all buffers on the host: rvk n x 32 B canonical; offsets n + 1 entries, offsets[0] = 0, nondecreasing (record i has the
 *                  fields offsets[i] .. offsets[i + 1], at most 65 535 of them); fields offsets[n] x 32 B canonical.  plain_out (offsets[n] x 32 B, not the
 *                  `fields` buffer): the plain fields, canonical; flags[i] = 0 decrypted, 2 malformed (rvk or one of the record's fields not below r: its rows
 *                  are zeros, its neighbours are not affected).  Offsets that decrease or do not start at 0, or a record of more than 65 535 fields, refuse
 *                  the call before any launch.  Returns byte for byte what records_decrypt_fields_host returns.  One record per lane; a launch covers at most
 *                  2^20 records and 2^22 fields, cut at record boundaries (ALEO_MI355X_DECRYPT_CHUNK_FIELDS, read per call, lowers the field cap: for tests;
 *                  the bytes do not depend on it).  Thread-safe (one slot per call); n = 0 and records without fields are fine.
 *   records_decrypt_fields_host   the same bytes, computed on the CPU by the calling thread; touches no device.
 *   min_decrypt    the size, counted in permutations (the sum of ceil(m / 8) over the records), from which records_decrypt_fields takes the GPU; a call
 *                  below it runs on the calling thread.  The default, 64, is the measured crossover against the host path on one thread (profiles/records_decrypt.txt:
 *                  records of two fields, 0.99x at 2^5, 2.68x at 2^6, and the GPU ahead at every larger size); ALEO_MI355X_MIN_DECRYPT overrides it, read per call.
 *   record_fields  host: the private fields of a "record1..." string in randomizer order, 32 B each, into fields_out (room for `cap` fields); *n_fields_out = their
 *                  number.  fields_out = NULL only counts.  Refuses whatever record_parse refuses, an entry without a known visibility, a private entry
 *                  whose length is not that of its field count or whose fields are not canonical.
 *   record_plaintext   host: puts n_fields decrypted fields (the record's own count) back into the record's structure and writes the RecordPlaintext string
 *                  "{\n  owner: aleo1....private,\n  <name>: <value>.<visibility>,\n  ...  _nonce: <decimal>group.public\n}".  address_x32 (may be NULL): the
 *                  owner, decrypted or public, must be it, else ERR_NOT_OWNER.  *out_len: in = the capacity of out, out = the string's length (without the
 *                  terminating 0, which is written as well): a buffer that is too short returns BAD_ARG with the length in place.  An entry that does not
 *                  parse is BAD_ARG, and last_error names it.  Literals by type number: 0 address (253 bits, bech32m), 1 boolean, 2 field, 3 group (253 bits,
 *                  decimal x), 4-8 i8..i128 (two's complement), 9-13 u8..u128, 14 scalar (251 bits), 15 string (quoted), each followed by its type's suffix
 *                  and the entry's visibility; a size that does not fit the type, a value not below the modulus and an unknown type are refused.  Types 0, 2
 *                  and 12 are pinned by reference-held vectors, the others are [UPSTREAM-RECALL].  Struct entries (one member per line, two spaces deeper per
 *                  level, the closing brace at the entry's own indentation) and the byte layout of public and constant entries (u8 variant; literal: u16 type,
 *                  little-endian value bytes, a string with a u16 length; struct: u8 member count, per member u8 name length, name, u16 length, plaintext)
 *                  are [UPSTREAM-RECALL] too, and UNPINNED: nothing the reference holds shows one.
 *   record_decrypt   the one-record mirror of RecordCiphertext.decrypt, entirely on the host: rvk from the host scan, the fields from the host path above, then
 *                  record_plaintext.  The address is passed in, not derived from the view key; a public owner is compared with it; ERR_NOT_OWNER when the view
 *                  key does not decrypt the owner to it.  A record with no private field needs no hash (and view_key32 may be NULL). */
int32_t aleo_mi355x_records_decrypt_fields(void* plain_out, uint8_t* flags, const void* rvk, const uint32_t* offsets, const void* fields, size_t n);
int32_t aleo_mi355x_records_decrypt_fields_host(void* plain_out, uint8_t* flags, const void* rvk, const uint32_t* offsets, const void* fields, size_t n);
size_t aleo_mi355x_min_decrypt(void);
int32_t aleo_mi355x_record_fields(const char* record1, void* fields_out, size_t cap, size_t* n_fields_out);
int32_t aleo_mi355x_record_plaintext(const char* record1, const void* plain_fields, size_t n_fields, const void* address_x32, char* out, size_t* out_len);
int32_t aleo_mi355x_record_decrypt(const char* record1, const void* view_key32, const void* address_x32, char* out, size_t* out_len);
/* The records ONE account owns among n strings, decrypted, in one call (csrc/records_found.hip): the scan of records_scan_strings, and then — on the device, from
 * the symbols the scan has left there — the private fields of every record with flag 1, their decryption, and the `microcredits` entry.  Only the owned records
 * come back.  text / offsets: the contract of records_scan_strings; the same arguments are refused with the same messages; n = 0 gives an empty result.
 *   *out          a result the library owns (its size is known only after the scan): read it through the accessors, whose pointers are valid until found_free.
 *                 The c records whose scan flag is 1 (a public owner equal to the address included), in ascending record index:
 *     found_count         c
 *     found_index         uint32_t[c]       the record indices, ascending
 *     found_kind          int8_t[c]         0 public owner, 1 private owner
 *     found_rvk           uint8_t[c][32]    the scan's row: the record view key's x, zeros where a public owner's nonce is not on the curve
 *     found_offsets       uint32_t[c + 1]   record k has the plain fields offsets[k] .. offsets[k + 1];  found_fields = offsets[c]
 *     found_plain         uint8_t[fields][32]   the decrypted private fields in randomizer order; a private owner's first one is the address x
 *     found_status        uint8_t[c]        0 decrypted; 2 malformed, as records_decrypt_fields flags it, and a public owner with private fields whose nonce
 *                                           is not on the curve: the rows are zeros; 4 record_fields refuses the string's structure (an entry without a valid
 *                                           name or a known visibility, a private entry whose length is not that of its field count or that holds a field not
 *                                           below r): no fields
 *     found_microcredits  uint64_t[c]       the value of the record's last entry named microcredits if it is a u64 literal — private: read from its plain
 *                                           fields' bits; constant or public: from its plaintext bytes — else 0, and 0 where the status is not 0.  What
 *                                           RecordPlaintext.microcredits() reads from the string of record_plaintext, with ONE difference: only that entry is
 *                                           examined, so a record in which ANOTHER entry cannot be rendered still reports its microcredits here.
 *     found_unparsed, found_first_unparsed   how many strings do not parse (flag 3 of the scan), and the first of them (n if none)
 *   records_decrypt_strings   n below min_records runs on the calling thread; else per chunk of whole records (the caps of records_scan_strings): parse, scan and
 *                 resolve as records_scan_strings, a count walk and a two-level prefix sum, one 16-byte read, a gather walk into compacted arrays,
 *                 k_records_decrypt over them in place (several launches above 2^22 fields; ALEO_MI355X_DECRYPT_CHUNK_FIELDS applies), the microcredits, and the
 *                 download of the compacted arrays.  Returns byte for byte what records_decrypt_strings_host returns.  Thread-safe (one slot per call).
 *   records_decrypt_strings_host   the existing host calls put together: the host scan, record_fields' structure, records_decrypt_fields_host; touches no device. */
typedef struct aleo_mi355x_found aleo_mi355x_found;
int32_t aleo_mi355x_records_decrypt_strings(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32);
int32_t aleo_mi355x_records_decrypt_strings_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_key32, const void* address_x32);
void aleo_mi355x_found_free(aleo_mi355x_found* found);
size_t aleo_mi355x_found_count(const aleo_mi355x_found* found);
const uint32_t* aleo_mi355x_found_index(const aleo_mi355x_found* found);
const int8_t* aleo_mi355x_found_kind(const aleo_mi355x_found* found);
const uint8_t* aleo_mi355x_found_rvk(const aleo_mi355x_found* found);
const uint32_t* aleo_mi355x_found_offsets(const aleo_mi355x_found* found);
size_t aleo_mi355x_found_fields(const aleo_mi355x_found* found);
const uint8_t* aleo_mi355x_found_plain(const aleo_mi355x_found* found);
const uint8_t* aleo_mi355x_found_status(const aleo_mi355x_found* found);
const uint64_t* aleo_mi355x_found_microcredits(const aleo_mi355x_found* found);
size_t aleo_mi355x_found_unparsed(const aleo_mi355x_found* found);
size_t aleo_mi355x_found_first_unparsed(const aleo_mi355x_found* found);
/* records_decrypt_strings for SEVERAL accounts in one call (csrc/records_found.hip): what a front end asks that serves K accounts over the same blocks and
 * needs each one's decrypted records and balance, not flags.  view_keys32 / address_xs32: n_keys x 32 bytes, 1 <= n_keys <= 64; keys, text and offsets are refused as
 * records_scan_strings refuses them (same status, same message, "key j" included).
 *   out           room for n_keys results: out[j] is byte for byte — every array, unparsed and first_unparsed — what records_decrypt_strings_host returns for key j
 *                 alone over the same strings; read it through the found_* accessors above and release each with found_free.  A key that appears twice gets two equal
 *                 results; a record that two keys own appears in both.  n = 0 gives n_keys empty results.  On any failure every out[j] is null (all n_keys of them, also
 *                 where n_keys itself is what is refused: out has room for as many entries as the caller says).
 *   records_decrypt_strings_many   n * n_keys below min_records (pairs, as records_scan_strings counts), or n = 0, runs on the calling thread; else per chunk of whole
 *                 records (the caps of records_scan_strings for n_keys keys; ALEO_MI355X_SCAN_CHUNK_CHARS and ALEO_MI355X_SCAN_KEYS_PER_LANE apply): ONE upload and
 *                 parse of the text, the grouped scan of records_scan_many, the resolve, then the count walk, prefix sums, gather walk, decryption and microcredits of
 *                 records_decrypt_strings over every (key, record) pair that is owned — compacted by key, then by record, and sized from the pairs there are — one
 *                 download, and the split into the n_keys results on the host.  Thread-safe (one slot per call).
 *   records_decrypt_strings_many_host   n_keys passes of records_decrypt_strings_host's path; touches no device. */
int32_t aleo_mi355x_records_decrypt_strings_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys);
int32_t aleo_mi355x_records_decrypt_strings_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* view_keys32, const void* address_xs32, size_t n_keys);
/* The serial numbers of the records an account has found: the step the reference takes with every owned record before it can use it,
 * `Record::<N, Ciphertext<N>>::serial_number(*private_key, commitment)` followed by the spent check (rust/src/api/blocking.rs:277-278), and what RecordPlaintext's
 * serialNumberString computes (wasm/src/record/record_plaintext.rs:64-82).  snarkVM 0.14.5 console/program/src/data/record/{serial_number,to_commitment,to_bits}.rs,
 * console/algorithms/src/{bhp,blake2xs,elligator2,poseidon/hash_to_group} [UPSTREAM-RECALL], pinned by data the reference holds (tests/golden/reference_serial.json,
 * reference_account.json): the account generator by three accounts, BHP1024 and the record's bits by a transaction output's checksum and id, the serial number by the
 * vector of wasm/src/record/record_plaintext.rs:131-140.  With D the domain separator "AleoSerialNumber0":
 *     H = 4 (Elligator2(h0) + Elligator2(h1)), (h0, h1) = Poseidon2 hash_many([D, cm], 2);   gamma = sk_sig H;
 *     nonce = the low 250 bits of Poseidon2 hash([D, x(4 gamma)]);   sn = x(BHP512 hash of (D, cm)'s bits + sum_i bit_i(nonce) R_i).
 *   records_serial_numbers   n commitments under one key, all buffers on the host: commitments32 n x 32 B canonical little-endian, sk_sig32 the account's sk_sig, a
 *                  canonical scalar below the subgroup order (else the call is refused).  sn_out (n x 32 B): the serial numbers, canonical; flags[i] = 0 computed,
 *                  2 refused: the commitment is not below r, or Elligator2 refuses an input (a zero among its input, v, x or y, or the degenerate r) — where
 *                  upstream's serial_number returns Err and the reference's `.ok()?` drops the record; the row is zeros.  A refused row never fails the batch.
 *                  One commitment per lane (csrc/records_serial_lane.h); a launch covers at most 2^20 commitments (ALEO_MI355X_SERIAL_CHUNK, read per call,
 *                  lowers that cap: for tests; the bytes do not depend on it).  The lane's tables (181 KB) are built at first use and stay resident per device.
 *                  Batches below min_serials run on the host inside the call.  Thread-safe (one slot per call); n = 0 is fine.
 *   records_serial_numbers_host   the same bytes out, computed on the CPU by the calling thread; touches no device.
 *   min_serials    the batch size from which records_serial_numbers takes the GPU: 64, the smallest power of two at which the GPU call beats the host path on one
 *                  thread in both timings (profiles/records_serial.txt: a call costs 3.7-4.5 ms; the host path 4.4 ms at 2^5, 0.98x, and 8.8 ms at 2^6, 2.35x);
 *                  ALEO_MI355X_MIN_SERIALS overrides it, read per call.
 *   found_serial_numbers   the serial numbers of the records a records_decrypt_strings result holds: commitments32 the commitments of ALL n strings the result was
 *                  made from (n x 32 B); the rows at found_index are gathered and go through records_serial_numbers; sn_out (found_count x 32 B) and flags
 *                  (found_count) as there.  An index not below n refuses the call.
 *   record_commitment   host: the commitment of a record — to_commitment(program_id, record_name) of its plaintext, the `commitment` the reference passes on — from
 *                  the "record1..." string and its n_fields decrypted fields in randomizer order (what record_decrypt and records_decrypt_strings hand out; the
 *                  record's own count).  A program id that is not "<identifier>.aleo" is refused with the last_error text "Invalid ProgramID specified", a record
 *                  name that is not an identifier (a letter, then letters, digits and underscores, at most 31) with "Invalid Identifier specified for record":
 *                  the strings the reference's tests expect (wasm/src/record/record_plaintext.rs:153-171).  The bits of constant and public entries are
 *                  [UPSTREAM-RECALL] and UNPINNED (csrc/records_bits.hpp).
 *   record_checksum   host: hash_bhp1024 of the bits of the record ciphertext as it stands: the "checksum" a transaction's record output carries.
 *   account_from_private_key   host: an "APrivateKey1..." string -> sk_sig, the view key's scalar and the address's x, 32 canonical little-endian bytes each; any
 *                  output may be NULL.  The account generator is hash_to_curve("AleoAccountEncryptionAndSignatureScheme0"). */
int32_t aleo_mi355x_records_serial_numbers(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const void* sk_sig32);
int32_t aleo_mi355x_records_serial_numbers_host(void* sn_out, uint8_t* flags, const void* commitments32, size_t n, const void* sk_sig32);
size_t aleo_mi355x_min_serials(void);
int32_t aleo_mi355x_found_serial_numbers(const aleo_mi355x_found* found, const void* commitments32, size_t n, const void* sk_sig32, void* sn_out, uint8_t* flags);
int32_t aleo_mi355x_record_commitment(void* out32, const char* record1, const void* plain_fields, size_t n_fields, const char* program_id, const char* record_name);
int32_t aleo_mi355x_record_checksum(void* out32, const char* record1);
int32_t aleo_mi355x_account_from_private_key(const char* private_key, void* sk_sig32, void* view_key32, void* address_x32);
/* The unspent records of one or several accounts in one call: the reference's get_unspent_records (rust/src/api/blocking.rs:229-325) behind the fetch of the
 * blocks — is_owner, decrypt, serial_number and the spent check — where records_decrypt_strings[_many] + found_serial_numbers + a host filter bring every owned
 * record down, run the serial-number kernel once per account and ask a callback per record.
 *   records_unspent_strings_many   n strings as records_decrypt_strings_many takes them; commitments32: their n commitments (the chain's record ids), n x 32 B —
 *                  the buffer has no length of its own: it must hold a row for every string; n_keys accounts, 1..64, account j = (sk_sigs32, view_keys32,
 *                  address_xs32) row j, 32 B each; spent32: a set S of n_spent spent serial numbers, n_spent x 32 B, in any order, duplicates allowed (a caller
 *                  that walks blocks reads them from the inputs of the transitions).  n_spent = 0 with spent32 NULL is legal: the result is then every owned record
 *                  that decrypts, with its serial number — for a caller who, like the reference, asks the chain per record.
 *                  For account j let F be what records_decrypt_strings_host returns for its view key and address, and for record k of F let (sn, flag) be what
 *                  records_serial_numbers_host returns for commitments32[F.index[k]] under sk_sig j.  Record k is KEPT iff F.status[k] == 0 && flag == 0 && sn
 *                  is not a row of S (a comparison of 32 bytes: a row of S that is no canonical field element matches nothing) — what the reference's `.ok()?`
 *                  and `if let Ok` keep.  out[j] is an aleo_mi355x_found of the kept records in record order: index, kind, rvk, offsets (rebased), plain, status
 *                  (all 0) and microcredits are byte for byte the kept rows of F, unparsed and first_unparsed are F's; found_serials is their serial numbers,
 *                  found_owned is F's count.
 *                  Refused: what records_decrypt_strings_many refuses; a null commitments32, sk_sigs32, view_keys32 or address_xs32; an sk_sig that is not
 *                  below the subgroup order (last_error names the key); spent32 NULL with n_spent > 0; n_spent > 2^30.  A malformed commitment row (not below
 *                  r, or an input Elligator2 refuses) never fails the call: its flag is 2 and its record is dropped.
 *                  n * n_keys below min_records, or n = 0, runs on the calling thread.  Else the flow of records_decrypt_strings_many, and per chunk behind it:
 *                  one serial-number launch over the owned pairs of ALL accounts (a wave holds one account's pairs; below min_serials owned pairs the calling
 *                  thread computes them instead, the same bytes), the spent check, and the compaction of the kept records on the device, so only they come
 *                  down.  Launches of at most ALEO_MI355X_SERIAL_CHUNK pairs.  Thread-safe (one slot per call).
 *                  The spent set on the device (csrc/records_spent_lane.h) — the slot rule, so that a test can build chains on purpose: a table of cap uint32
 *                  slots, cap the smallest power of two >= 2 n_spent and at least 64, zero = empty, else a row's number + 1; a row's (and a serial number's)
 *                  first slot is its first little-endian 32-bit word & (cap - 1), the next slot (slot + 1) & (cap - 1); an insert takes the first empty slot
 *                  (duplicates take one each), a probe walks to the first empty slot and hits where all 32 bytes are equal.  Rows that share their first word
 *                  lengthen chains and change no answer.
 *   records_unspent_strings_many_host   the same bytes: records_decrypt_strings_host's path per account, records_serial_numbers_host's per owned record, a sorted
 *                  copy of S; touches no device and shares no code with the device's spent set.
 *   records_unspent_strings[_host]   one account: the call above with n_keys = 1.
 *   found_serials  count x 32 B: the kept records' serial numbers; NULL for the result of any other call.
 *   found_owned    how many records the account owned before the filter; for the result of any other call, its count. */
int32_t aleo_mi355x_records_unspent_strings(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sig32, const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_strings_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sig32, const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_strings_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_strings_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const void* commitments32, const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent);
const uint8_t* aleo_mi355x_found_serials(const aleo_mi355x_found* found);
size_t aleo_mi355x_found_owned(const aleo_mi355x_found* found);
/* Unspent records from the strings alone: the commitments the calls above take from the chain, computed from each owned record's plaintext — what the JS/wasm SDK's
 * findUnspentRecords does, which has only the strings and the private key (sdk/src/aleo_network_client.ts:365-373: serialNumberString(privateKey, "credits.aleo",
 * "credits"), that is to_commitment(program_id, record_name) followed by serial_number: wasm/src/record/record_plaintext.rs:64-82).  A caller in that position
 * brought every owned record down with records_decrypt_strings, called record_commitment once per record on the host, and went back up for records_unspent_strings.
 * program_id / record_name: the same for every record of a call, refused as record_commitment refuses them, with its two last_error texts.
 *   records_commitments_found   the commitments of the records an aleo_mi355x_found holds (the result of any of the calls above), given the n strings it was made
 *                  from: cm_out (found_count x 32 B, canonical little-endian) and flags (found_count).  flags[k] = 0 computed: the row is byte for byte what
 *                  record_commitment returns for string found_index[k] and the record's plain fields; 4 refused where record_commitment refuses the record (a
 *                  private entry without a terminus bit or of no fields, a constant or public entry that does not parse); a record whose found_status is not 0
 *                  gets that status (2 or 4) as its flag and computes nothing.  A refused row is zeros and never fails the call.  Refused: a null result, a null
 *                  buffer with a count above 0, what records_scan_strings refuses of text and offsets, a found_index not below n.
 *                  One owned record per lane (csrc/records_commit_lane.h): the owned strings' text and the plain fields go up, one launch chain runs (launches of
 *                  at most 2^20 records; ALEO_MI355X_COMMIT_CHUNK, read per call, lowers that cap: for tests; the bytes do not depend on it), rows and flags come
 *                  down.  The lane's table (432 x 4 points of BHP1024, 217 KB with the scan's constants) is built at first use and stays resident per device.  A
 *                  record with a constant or public entry is not walked on the device (the conversion of such an entry is recursive and UNPINNED,
 *                  csrc/records_bits.hpp): the calling thread computes its row inside the call.  Fewer than min_commitments records run on the host.
 *                  Thread-safe (one slot per call).
 *   records_commitments_found_host   the same bytes, record_commitment's code per record on the calling thread; touches no device.
 *   min_commitments   the number of owned records from which the commitments take the GPU: 32, the smallest power of two at which the stand-alone GPU call beats the
 *                  host path on one thread in both of two timings (profiles/records_commit.txt: a call costs 1.2-1.5 ms; the host path 0.84 / 0.82 ms at 2^4, 0.57x
 *                  and 0.56x, and 1.63 / 1.63 ms at 2^5, 1.15x and 1.12x); ALEO_MI355X_MIN_COMMITMENTS overrides it, read per call.
 *   records_unspent_named_many   records_unspent_strings_many without commitments32.  For account j let F be what records_decrypt_strings_host returns, (cm, cf)
 *                  row k of records_commitments_found_host over F, and (sn, sf) what records_serial_numbers_host returns for cm under sk_sig j.  Record k is KEPT
 *                  iff F.status[k] == 0 && cf == 0 && sf == 0 && sn is not a row of S.  (A record dropped for cf is one the reference drops too: its plaintext does
 *                  not parse, so record.decrypt fails.)  out[j] has the layout of records_unspent_strings_many's result; found_commitments is the kept records'
 *                  commitments.  Refused: the program id and record name as above, and everything records_unspent_strings_many refuses (commitments32 aside).
 *                  n * n_keys below min_records, or n = 0, runs on the calling thread.  Else the flow of records_unspent_strings_many with one more kernel per
 *                  chunk, behind the decryption: the commitments of ALL accounts' owned records (below min_commitments of them, and for routed records, on the
 *                  calling thread), which the serial numbers, the spent check and the compaction then run on; the index download and the commitment upload of
 *                  records_unspent_strings_many fall away.
 *   records_unspent_named_many_host   the same bytes from the host paths named in the definition; touches no device.
 *   records_unspent_named[_host]   one account: the call above with n_keys = 1.
 *   found_commitments   count x 32 B: the kept records' commitments; NULL for the result of any other call. */
int32_t aleo_mi355x_records_commitments_found(void* cm_out, uint8_t* flags, const aleo_mi355x_found* found, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name);
int32_t aleo_mi355x_records_commitments_found_host(void* cm_out, uint8_t* flags, const aleo_mi355x_found* found, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name);
size_t aleo_mi355x_min_commitments(void);
int32_t aleo_mi355x_records_unspent_named(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32, const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_named_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32, const void* view_key32, const void* address_x32, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_named_many(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_records_unspent_named_many_host(aleo_mi355x_found** out, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sigs32, const void* view_keys32, const void* address_xs32, size_t n_keys, const void* spent32, size_t n_spent);
const uint8_t* aleo_mi355x_found_commitments(const aleo_mi355x_found* found);
/* Record PLAINTEXT strings — "{ owner: aleo1….private, microcredits: 5u64.private, _nonce: …group.public }" — read, committed and serial-numbered: what every
 * write call of the reference takes its records as (fee_record / amount_record: wasm/src/programs/manager/transfer.rs:66-68), what findUnspentRecords hands back
 * and a wallet stores, and what RecordPlaintext.fromString(..).serialNumberString(..) starts from (wasm/src/record/record_plaintext.rs:45-82, :131-140).  The calls
 * above start from a record1… ciphertext and its decrypted fields; these start from the text.  The grammar, the bits a string comes to and every choice the
 * reference cannot pin (UNPINNED: underscores in digits, leading zeros, signs, comments, the entry cap, reserved names) are csrc/plaintext_parse.hpp's header.
 *   record_plaintext_parse   host: RecordPlaintext.fromString and microcredits().  owner_kind 0 public / 1 private, the owner's address x, the nonce's x, and the
 *                  value of a top-level u64 entry named microcredits (else 0); every out pointer may be NULL.  This call alone also asks that the owner, the nonce
 *                  and every `group` value are x-coordinates of points of the prime-order subgroup; the batch calls check canonical encoding (below the modulus)
 *                  only, as record_plaintext's rendering does.  Refused with last_error beginning "The record plaintext string provided was invalid".
 *   plaintext_commitment   host: to_commitment(program_id, record_name) of the record the string says, 32 B canonical little-endian.  last_error is exactly
 *                  "Invalid ProgramID specified", "Invalid Identifier specified for record" or "The record plaintext string provided was invalid".
 *   plaintexts_commitments   n strings (text / offsets as records_parse_many takes them): cm_out (n x 32 B), microcredits (n, may be NULL) and flags (n): 0 computed;
 *                  3 not a record plaintext, the row zeros.  A bad string never fails the call.  One string per lane (csrc/plaintexts_lane.h) over the commitment
 *                  lane's resident table; launches of at most 2^20 strings (ALEO_MI355X_PLAINTEXTS_CHUNK, read per call, lowers the cap: for tests).  The lane
 *                  computes records whose entries are all numeric, boolean or address literals in the spelling record_plaintext prints, of at most 1024
 *                  characters and 8 entries; structs, quoted strings, other spellings, longer strings and everything that looks malformed are computed or
 *                  refused by the calling thread with the host code, inside the call.  Fewer than min_plaintexts strings run on the host.  Thread-safe.
 *   plaintexts_serial_numbers   the same, then the serial number of every computed commitment under sk_sig32 (one key per call) into sn_out (n x 32 B), and the
 *                  look-up of each in the n_spent rows of spent32 (may be NULL with n_spent 0).  cm_out may be NULL.  flags: 0 computed and not in the set; 1
 *                  computed and in the set; 2 the serial number is refused (records_serial_numbers' flag; the row zeros); 3 not a record plaintext (both rows
 *                  zeros).  One slot, one stream: k_plaintexts_commit, the routed rows patched, k_records_serial, k_spent_insert, the look-up, one download.
 *   plaintexts_commitments_host, plaintexts_serial_numbers_host   the same bytes on the calling thread; touch no device.
 *   min_plaintexts   the number of strings from which the two calls take the GPU: 32, the measured crossover against the host twin on one thread of a call that
 *                  brings no spent set (profiles/records_plaintexts.txt: at 2^4 the GPU road takes 5.86 ms against 3.04 for serial numbers and 1.37 against 0.80 for
 *                  commitments, at 2^5 5.89 against 6.09 and 1.38 against 1.58; with 2^16 spent rows, which the host twin sorts in every call, it wins from 2^3
 *                  on); ALEO_MI355X_MIN_PLAINTEXTS overrides it, read per call.
 *   plaintexts_last_routed   how many strings of the calling thread's last batch call the host code computed or refused: all n below the threshold, else the
 *                  rows the lane routed. */
int32_t aleo_mi355x_record_plaintext_parse(const char* plaintext, int32_t* owner_kind, void* owner_x32, void* nonce_x32, uint64_t* microcredits);
int32_t aleo_mi355x_plaintext_commitment(void* out32, const char* plaintext, const char* program_id, const char* record_name);
int32_t aleo_mi355x_plaintexts_commitments(void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name);
int32_t aleo_mi355x_plaintexts_commitments_host(void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name);
int32_t aleo_mi355x_plaintexts_serial_numbers(void* sn_out, void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32, const void* spent32, size_t n_spent);
int32_t aleo_mi355x_plaintexts_serial_numbers_host(void* sn_out, void* cm_out, uint64_t* microcredits, uint8_t* flags, const char* text, const uint64_t* offsets, size_t n, const char* program_id, const char* record_name, const void* sk_sig32, const void* spent32, size_t n_spent);
size_t aleo_mi355x_min_plaintexts(void);
size_t aleo_mi355x_plaintexts_last_routed(void);
/* Record plaintexts ENCRYPTED to the record1… strings a transition publishes (csrc/records_encrypt.hip, csrc/record_encrypt_host.hpp): the other direction of everything
 * above.  snarkVM 0.14.5 console/program/src/data/record/encrypt.rs, Record<N, Plaintext<N>>::encrypt(randomizer) / encrypt_symmetric_unchecked(record_view_key)
 * [UPSTREAM-RECALL], which every execute, transfer, split and join of the reference runs for each output record (rust/src/program/execute.rs:74,177,
 * rust/src/program/transfer.rs:99-106).  With r the randomizer, a scalar below the subgroup order l, G the account generator and Owner the point of the prime-order
 * subgroup with the owner's x:  nonce = x(r G);  rvk = x(r Owner);  the private fields in randomizer order — the owner's x if the owner is private, then for every
 * private entry its plaintext bits, a terminus 1 and zero padding, 252 bits to a field —;  c_i = plain_i + hash_many_psd8([domain "AleoSymmetricEncryption0", rvk], m)_i;
 * the bytes exactly as record_parse, record_fields and record_plaintext read them; bech32m under "record".
 * Pinned: the symmetric half.  The reference's own plaintext (tests/golden/reference_records.json, plaintexts.owner and .sdk) under x(view key . nonce) gives the
 * reference's record1… string character for character.  [UPSTREAM-RECALL] and UNPINNED: the byte layout of public and constant entries (as under record_plaintext);
 * and everything about `encrypt` that the randomizer-free known answer cannot reach — that the nonce is x(r G) with the account generator, that rvk is x(r Owner),
 * that r = 0 is computed and not refused, that upstream refuses what flag 2 refuses.  The two rest on r A = view key . (r G) and are tested by the round trip through
 * records_scan_strings and records_decrypt_strings.  Neither path is hardened against side channels, as elsewhere.  Equal randomizers are NOT looked for: two records
 * encrypted under one randomizer share their nonce, and if they share the owner their record view key; giving every record its own is the caller's to see to.
 *   record_encrypt   host, one record.  mode 0 is upstream's encrypt: the string's _nonce must be x(r G) (BAD_ARG otherwise).  mode ALEO_MI355X_ENCRYPT_SET_NONCE
 *                  ignores the value of the string's nonce and writes x(r G): for a producer that has a template and a randomizer.  out / out_len: the contract
 *                  of record_plaintext.  BAD_ARG with last_error beginning "The record plaintext string provided was invalid" for a string
 *                  record_plaintext_parse's grammar refuses (or an entry whose body passes the 65535 bytes its length holds); BAD_ARG for a randomizer not below l
 *                  and an owner whose x has no point in the prime-order subgroup.
 *   record_encrypt_symmetric   host: the string under a record view key given as it is (32 B canonical, below r): no randomizer, no owner point, the nonce kept.
 *                  This is the pinned half.
 *   record_nonce   host: x(r G), 32 B canonical little-endian; BAD_ARG for r not below l.
 *   records_encrypt   n plaintext strings (text / offsets as records_parse_many takes them) under n randomizers (n x 32 B), one mode for all.  *out is a result the
 *                  library owns (the sizes are known only afterwards), read through the accessors, whose pointers are valid until encrypted_free:
 *     encrypted_text      the record1… strings one after another, no separator
 *     encrypted_offsets   uint64_t[n + 1]   string i is text[offsets[i] .. offsets[i + 1])
 *     encrypted_flags     uint8_t[n]        first match wins: 3 not a record plaintext; 2 the randomizer is not below l, or the owner's x has no prime-order point;
 *                                           1 mode 0 and x(r G) is not the string's nonce; 0 encrypted.  A row whose flag is not 0 has an empty string and a zero rvk
 *     encrypted_rvk       uint8_t[n][32]    the record view key's x: what records_scan_strings returns for the owner
 *                  A bad row never fails the call; it fails only for null buffers, an unknown mode, offsets that records_parse_many refuses, and a launch of more
 *                  than 2^32 - 1 characters.  n = 0 gives an empty result.  On failure *out is null.  Below min_encrypt strings the call runs on the calling thread.
 *                  Else per launch of at most 2^20 strings (ALEO_MI355X_ENCRYPT_CHUNK, read per call, lowers the cap: for tests; the bytes do not depend on it) two
 *                  kernels, one string per lane each (csrc/records_encrypt_lane.h): the keys (the measure walk, r G from the resident table of G, the owner's point,
 *                  r Owner), the project's two-level exclusive sum over the rows' lengths, one 32-byte read, the text (the second walk, the squeeze, a bech32m symbol
 *                  writer).  The lanes compute the records plaintexts_commitments' lane computes (numeric, boolean and address literals in record_plaintext's
 *                  spelling, any visibility, at most 1024 characters and 8 entries); every other row is encrypted or refused by the calling thread with the host
 *                  code inside the call and spliced in.  Thread-safe (one slot per call).  Returns byte for byte what records_encrypt_host returns.
 *   records_encrypt_host   the same bytes on the calling thread; touches no device.
 *   min_encrypt    the number of strings from which records_encrypt takes the GPU: 32, the measured crossover against the host twin on one thread
 *                  (profiles/records_encrypt.txt: at 2^4 the GPU road takes 4.15 ms against 2.41, 0.58x; at 2^5 4.13 against 4.80, 1.16x; the parent commit has no road
 *                  from a plaintext to a ciphertext); ALEO_MI355X_MIN_ENCRYPT overrides it, read per call.
 *   records_encrypt_last_routed   how many strings of the calling thread's last batch call the host code encrypted or refused: all n below the threshold, else the
 *                  rows the lanes routed. */
#define ALEO_MI355X_ENCRYPT_SET_NONCE 1
typedef struct aleo_mi355x_encrypted aleo_mi355x_encrypted;
int32_t aleo_mi355x_record_encrypt(const char* plaintext, const void* randomizer32, int32_t mode, char* out, size_t* out_len);
int32_t aleo_mi355x_record_encrypt_symmetric(const char* plaintext, const void* rvk32, char* out, size_t* out_len);
int32_t aleo_mi355x_record_nonce(void* out32, const void* randomizer32);
int32_t aleo_mi355x_records_encrypt(aleo_mi355x_encrypted** out, const char* text, const uint64_t* offsets, size_t n, const void* randomizers32, int32_t mode);
int32_t aleo_mi355x_records_encrypt_host(aleo_mi355x_encrypted** out, const char* text, const uint64_t* offsets, size_t n, const void* randomizers32, int32_t mode);
void aleo_mi355x_encrypted_free(aleo_mi355x_encrypted* encrypted);
const char* aleo_mi355x_encrypted_text(const aleo_mi355x_encrypted* encrypted);
const uint64_t* aleo_mi355x_encrypted_offsets(const aleo_mi355x_encrypted* encrypted);
const uint8_t* aleo_mi355x_encrypted_flags(const aleo_mi355x_encrypted* encrypted);
const uint8_t* aleo_mi355x_encrypted_rvk(const aleo_mi355x_encrypted* encrypted);
size_t aleo_mi355x_min_encrypt(void);
size_t aleo_mi355x_records_encrypt_last_routed(void);

/* ---- account signatures: sign, the sign1… string, and many verifications in one call ---------------------------------------------------------------------------
 * The two account calls of the reference besides derivation, ownership and decryption (wasm/src/account/signature.rs:37-48 Signature::sign / verify,
 * wasm/src/account/address.rs:69-71, wasm/src/account/private_key.rs:244-248, sdk/src/account.ts:195,211-213) — snarkVM 0.14.5 console/account/src/signature
 * [UPSTREAM-RECALL].  A signature is 128 bytes: challenge | response | pk_sig.x | pr_sig.x, 32 bytes each, canonical little-endian; as a string it is bech32m
 * under the prefix "sign".  With G the account generator and m the message's fields: sign takes a nonce k, g_r = k G,
 * challenge = hash_to_scalar_psd8([g_r.x, pk_sig.x, pr_sig.x, address.x, m ...]), response = k - challenge sk_sig; verify takes g_r = response G + challenge pk_sig,
 * the challenge again, sk_prf = hash_to_scalar_psd4([pk_sig.x, pr_sig.x]), and accepts iff the challenges are equal and x(pk_sig + pr_sig + sk_prf G) is the
 * address.  A message's bytes become bits, little-endian within a byte, in fields of 252 bits, the last one short; no bytes, no fields.  Of the two points with
 * a given x the one in the prime-order subgroup is taken.
 * Pinned by the reference's data (three accounts): the generator, hash_to_scalar's 250 bits, rate 4 for sk_prf, the sum that makes the address, Poseidon at
 * rates 2, 4 and 8.  The reference holds no signature; its own tests are round trips (signature.rs:98-115).  So:
 *   UNPINNED  the order of the challenge's preimage
 *   UNPINNED  the packing of bytes into fields
 *   UNPINNED  the 128-byte layout and the "sign" prefix
 *   UNPINNED  the cap: a message of more than MAX_DATA_SIZE_IN_FIELDS = 4161 fields (131071 bytes) is refused
 *   signature_sign   host code.  out128: the signature of message[0 .. len) under the account of private_key ("APrivateKey1…").  The nonce is the first number below
 *                  the group order in the ChaCha20 stream under seed32 (32-byte blocks, the low 251 bits of each; rejection, so it is uniform) and signing is
 *                  a function of its arguments.  NEVER REUSE A SEED for two messages: two signatures under one nonce give the private key away.  Refused
 *                  (ALEO_MI355X_ERR_BAD_ARG): a key account_from_private_key refuses, a message over the cap.
 *   signature_to_string / signature_from_string   128 bytes <-> "sign1…" (cap: 219 bytes hold it).  from_string refuses a bad checksum, another prefix and a payload that is
 *                  not 128 bytes.
 *   signatures_verify   n signatures (sigs128: n x 128 B) under addresses_x32 — rows of 32 bytes address_stride apart: 0, one address for all; 32, one per signature —
 *                  over messages: concatenated bytes with n + 1 offsets, as records_scan_strings takes its strings.  flags[i]: 0 signature i verifies; 1 it does
 *                  not (a challenge or an address differs); 3 it is no signature (a scalar not below the group order, an x not below r or with no point in the
 *                  subgroup, a message over the cap) — the value the record calls give to what does not parse.  Refused: null buffers, another stride,
 *                  offsets that do not start at 0 or decrease.  n = 0 is fine.  Batches below min_signatures run the host code inside the call; else one kernel
 *                  launch per 2^20 signatures (one signature per lane), the copies inside the call.  Thread-safe (one slot per call).
 *   signatures_verify_host   the same flags, computed by the calling thread; touches no device.  It is the definition of the result.
 *   min_signatures   the batch size from which signatures_verify takes the GPU: 32, the smallest power of two at which the GPU call beats the host path on one thread in
 *                  both of two timings (profiles/signatures_verify.txt: a call costs 5.6-6.2 ms for any batch up to 2^10; the host path 3.75 / 3.75 ms at 2^4, 0.60x
 *                  and 0.61x, and 7.75 / 7.75 ms at 2^5, 1.25x and 1.26x); ALEO_MI355X_MIN_SIGNATURES overrides it, read per call (a bad value: the default). */
int32_t aleo_mi355x_signature_sign(void* out128, const char* private_key, const void* message, size_t len, const void* seed32);
int32_t aleo_mi355x_signature_to_string(char* out, size_t cap, const void* sig128);
int32_t aleo_mi355x_signature_from_string(void* out128, const char* s);
int32_t aleo_mi355x_signatures_verify(uint8_t* flags, const void* sigs128, const void* addresses_x32, size_t address_stride, const void* messages, const uint64_t* offsets, size_t n);
int32_t aleo_mi355x_signatures_verify_host(uint8_t* flags, const void* sigs128, const void* addresses_x32, size_t address_stride, const void* messages, const uint64_t* offsets, size_t n);
size_t aleo_mi355x_min_signatures(void);

/* ---- account signatures in batches: one key signing many messages, or many keys signing one message each ----------------------------------------------------------
 * Signature::sign (wasm/src/account/signature.rs:37-44, wasm/src/account/private_key.rs:92-96, sdk/src/account.ts:195) for n messages in one call.  Row i of the
 * result is byte for byte what signature_sign returns for (key i, message i, nonce seed i): nonce = the first number below the group order in the ChaCha20 stream
 * under the seed, g_r = nonce G, challenge = hash_to_scalar_psd8([g_r.x, pk_sig.x, pr_sig.x, address.x, m ...]), response = nonce - challenge sk_sig mod l, the
 * row challenge | response | pk_sig.x | pr_sig.x.  [UPSTREAM-RECALL], and UNPINNED exactly where the block above says so: the order of the preimage, the packing,
 * the layout and the cap are inherited from it unchanged.
 * Neither path is hardened against side channels: the table lookups are indexed by secret digits (of the nonce; of the key in the derivation), as accounts_derive's are.
 *   signatures_sign   sigs128: n rows of 128 bytes.  key_seeds32: rows of the 32 bytes an "APrivateKey1…" string holds (private_key_seed), as accounts_derive takes
 *                  them, key_stride apart: 0, one key for all (derived once, on the host); 32, one key per signature (derived on the device by a launch of its
 *                  own on the same stream; equal keys in such a batch are derived again, each).  messages / offsets: concatenated bytes with n + 1 offsets, as
 *                  signatures_verify takes them.  nonce_seeds32: n rows of 32 bytes, always one per signature.  flags[i]: 0 signed; 3 the key seed is no canonical
 *                  field element or the message is over the cap of 131071 bytes — row i is then zeros (the value accounts_derive and signatures_verify give
 *                  to such inputs).  Refused (ALEO_MI355X_ERR_BAD_ARG): null buffers with n > 0, another stride, offsets that do not start at 0 or decrease, and
 *                  TWO EQUAL ROWS IN nonce_seeds32 — NEVER REUSE A SEED: inside one call the library enforces it, on the host, before anything is uploaded,
 *                  also where the two rows sign under different keys; last_error names the two indices.  n = 0 is fine.  Batches below min_sign run the host
 *                  code inside the call and need no device; else launches of at most 2^20 signatures and 2^30 message bytes (ALEO_MI355X_SIGN_CHUNK caps the
 *                  signatures lower), one signature per lane, the copies inside the call.  Thread-safe (one slot per call).
 *   signatures_sign_host   the same bytes, computed by the calling thread; touches no device.  It is the definition of the result.
 *   min_sign       the batch size from which signatures_sign takes the GPU: 64, the smallest power of two at which the GPU call beats the host path on one thread in both
 *                  of two timings, in the mode that crosses later (profiles/signatures_sign.txt.  One key: a call costs 2.4-2.7 ms for any batch up to 2^12; the
 *                  host path 1.61 / 1.61 ms at 2^5, 0.65x and 0.65x, and 2.93 / 2.93 ms at 2^6, 1.23x and 1.22x.  A key each, whose host path derives a key per
 *                  row: a call costs 4.3-4.8 ms; the host path 5.61 / 5.61 ms at 2^4, 1.16x and 1.16x.  The parent's road, a loop of signature_sign on one
 *                  thread, is behind the call from 2^4 on in both modes: 5.05 ms and 5.63 ms there, 1.88x and 1.16x); ALEO_MI355X_MIN_SIGN overrides it, read
 *                  per call (a bad value: the default).
 *                  The check for equal seeds costs 15 ms at 2^20 seeds, inside a call of 61-66 ms (one key) or 99 ms (a key each). */
int32_t aleo_mi355x_signatures_sign(void* sigs128, uint8_t* flags, const void* key_seeds32, size_t key_stride, const void* messages, const uint64_t* offsets,
                                    const void* nonce_seeds32, size_t n);
int32_t aleo_mi355x_signatures_sign_host(void* sigs128, uint8_t* flags, const void* key_seeds32, size_t key_stride, const void* messages, const uint64_t* offsets,
                                         const void* nonce_seeds32, size_t n);
size_t aleo_mi355x_min_sign(void);

/* ---- accounts in batches: keys and addresses of many seeds in one call, and the search for an address with a chosen prefix ---------------------------------------
 * The first step of every record and signature call above: an account's sk_sig, view key and address, from the 32-byte seed of its private key — the reference's
 * account module (wasm/src/account/private_key.rs:38-86 PrivateKey::new, from_seed_unchecked, to_view_key, to_address; sdk/src/account.ts:82) — snarkVM 0.14.5
 * console/account [UPSTREAM-RECALL].  Pinned by data the reference holds: the derivation by the three accounts of tests/golden/reference_account.json, the private
 * key string of a seed by sdk/tests/data/account-data.ts:4,8 (tests/golden/reference_seed.json).  UNPINNED: seed_from_bytes for a value not below r (the reference's
 * one seed is below r).  A seed is the 32 bytes an "APrivateKey1…" string holds: a canonical little-endian field element.
 *   accounts_derive   n seeds of 32 bytes -> rows of 32 canonical little-endian bytes (sk_sig32, view_key32, address_x32), rows of the 63 ASCII characters "aleo1…"
 *                  with no terminator (address63), and flags: 0 derived; 3 the seed is not a canonical field element (its rows are zero).  Every output may be NULL.
 *                  n below min_accounts runs the host code inside the call and needs no device; else one kernel launch per 2^20 accounts (ALEO_MI355X_ACCOUNTS_CHUNK
 *                  caps it lower), one account per lane, the copies inside the call.  Thread-safe (one slot per call).
 *   accounts_derive_host   the same bytes, computed by the calling thread (aleo_mi355x_account_from_private_key's code); touches no device.  The definition.
 *   accounts_search   candidate i of [first, first + count) has the private-key seed "element i of the ChaCha20 stream under master32" (the prover's stream: counter i,
 *                  64 bits wide, rejection sampling below r — uniform over the field, as PrivateKey::new(rng) draws its seed); it matches when the characters after
 *                  "aleo1" of its address begin with `prefix`: 0 to 12 characters of qpzry9x8gf2tvdw0s3jn54khce6mua7l, anything else is ERR_BAD_ARG.  hit_index: the
 *                  first max_hits matching indices, ascending; hit_seed32 (may be NULL): their seeds; *n_hits; *next: the index after the last hit when
 *                  *n_hits == max_hits (first when max_hits is 0), first + count otherwise — a caller resumes from *next without seeing a candidate twice or skipping
 *                  one.  count below min_accounts runs on the host; else launches of at most 2^20 candidates (ALEO_MI355X_ACCOUNTS_CHUNK) until max_hits are found,
 *                  only the hits' indices come down, and every hit is derived again on the host before it is returned: one the host path does not confirm fails the
 *                  call with ERR_INTERNAL.  The result does not depend on scheduling or on the launch size.
 *   accounts_search_host   the same result, computed by the calling thread.  The definition.
 *   min_accounts   the batch size from which accounts_derive and accounts_search take the GPU: 16, the smallest power of two at which the GPU call beats the host
 *                  loop on one thread in both of two timings (profiles/accounts_derive.txt: a call costs 2.2-3.0 ms for any batch up to 2^12; the host loop 1.37 ms
 *                  at 2^3, 0.55x and 0.54x, 2.77 ms at 2^4, 1.10x and 1.14x, 5.57 ms at 2^5, 2.16x and 2.23x; with the strings asked for 2^4 is 0.93x);
 *                  ALEO_MI355X_MIN_ACCOUNTS overrides it, read per call (a bad value: the default).
 *   private_key_from_seed / private_key_seed   32 bytes <-> "APrivateKey1…" (base58 of 11 prefix bytes and the seed; cap: 60 bytes hold it).  Both refuse a seed that
 *                  is not a canonical field element; private_key_seed what account_from_private_key refuses.
 *   seed_from_bytes   32 arbitrary bytes, little-endian, reduced mod r: from_seed_unchecked (private_key.rs:47-55) [UPSTREAM-RECALL, UNPINNED above r].
 *   view_key_to_string   32 bytes -> "AViewKey1…" (cap: 54 bytes hold it). */
int32_t aleo_mi355x_accounts_derive(const void* seeds32, size_t n, void* sk_sig32, void* view_key32, void* address_x32, char* address63, uint8_t* flags);
int32_t aleo_mi355x_accounts_derive_host(const void* seeds32, size_t n, void* sk_sig32, void* view_key32, void* address_x32, char* address63, uint8_t* flags);
int32_t aleo_mi355x_accounts_search(const void* master32, uint64_t first, uint64_t count, const char* prefix, size_t max_hits, uint64_t* hit_index, void* hit_seed32, size_t* n_hits, uint64_t* next);
int32_t aleo_mi355x_accounts_search_host(const void* master32, uint64_t first, uint64_t count, const char* prefix, size_t max_hits, uint64_t* hit_index, void* hit_seed32, size_t* n_hits, uint64_t* next);
size_t aleo_mi355x_min_accounts(void);
int32_t aleo_mi355x_private_key_from_seed(char* out, size_t cap, const void* seed32);
int32_t aleo_mi355x_private_key_seed(void* seed32, const char* private_key);
int32_t aleo_mi355x_seed_from_bytes(void* seed32, const void* bytes32);
int32_t aleo_mi355x_view_key_to_string(char* out, size_t cap, const void* view_key32);

/* ---- private key ciphertexts: a private key encrypted under a secret, decrypted one at a time and opened in batches ------------------------------------------------
 * The reference's PrivateKeyCiphertext (wasm/src/account/private_key_ciphertext.rs:39-73 encryptPrivateKey, decryptToPrivateKey; wasm/src/account/private_key.rs:102-130
 * newEncrypted, toCiphertext, fromPrivateKeyCiphertext; the algorithm: rust/src/account/encryptor.rs:26-67) over snarkVM 0.14.5's Plaintext and Ciphertext
 * [UPSTREAM-RECALL]: the step between the "ciphertext1…" string a front end holds with a caller's password and accounts_derive.  Pinned by data the reference holds
 * (private_key_ciphertext.rs:115-128; tests/golden/reference_account.json "ciphertext_kat"): decryption, and encryption under the nonce that ciphertext holds, byte for
 * byte.  UNPINNED: a secret of more than 31 bytes (its bytes, little-endian, mod r; the reference's has 10), trailing payload bytes (refused), bit 252 of a decrypted
 * field (ignored).  REFUSED though upstream would accept it: a ciphertext whose plaintext holds the members `key` and `nonce` in a valid Plaintext shape other than the
 * one Encryptor::encrypt_field writes (csrc/key_ciphertext_lane.h).  A secret is any byte string, the empty one included.
 *   private_key_encrypt   host code, a function of its arguments: the 174 characters "ciphertext1…" and their terminator (cap at least 175) of an "APrivateKey1…"
 *                  string under `secret` and the nonce nonce32, a canonical little-endian field element the caller draws uniformly (upstream: Uniform::rand).
 *                  ERR_BAD_ARG: a key private_key_seed refuses, a nonce not below r, a smaller buffer.
 *   private_key_decrypt   host code: the "APrivateKey1…" string (cap: 60 bytes hold it).  ERR_BAD_ARG for what is no ciphertext string, ERR_NOT_OWNER where it does not
 *                  decrypt under this secret (record_decrypt's status where the reference's decryption fails).
 *   private_keys_open   n (ciphertext, secret) pairs: the ciphertexts as concatenated text with n + 1 offsets (as records_scan_strings takes its strings), the secrets
 *                  as concatenated bytes with n + 1 offsets.  Out: seeds32 (the 32 bytes an "APrivateKey1…" string holds), the rows of accounts_derive (sk_sig32,
 *                  view_key32, address_x32, address63) and flags: 0 opened; 1 a ciphertext that does not decrypt under this secret (one of a field count other than
 *                  3 included); 3 no ciphertext string (a character, the checksum, the prefix, the payload's length, a field element not below r, more than 2^20
 *                  characters).  Rows of a flagged pair are zero.  Every output may be NULL; n = 0 is fine; offsets that do not start at 0 or that decrease are
 *                  ERR_BAD_ARG.  n below min_key_ciphertexts runs the host code inside the call and needs no device; else per 2^20 pairs (ALEO_MI355X_ACCOUNTS_CHUNK
 *                  caps it lower) one launch of k_key_ciphertexts_open, one pair per lane, and, where an account row is asked for, one of k_accounts_derive behind
 *                  it over the seeds where they lie: seeds come down only into seeds32.  The copies are inside the call.  Thread-safe (one slot per call).
 *   private_keys_open_host   the same bytes, computed by the calling thread; touches no device.  The definition.
 *   min_key_ciphertexts   the batch size from which private_keys_open takes the GPU: 64, the smallest power of two at which the GPU call beats the host loop on one
 *                  thread in both of two timings, with the seeds alone and with the account outputs, the larger of the two (profiles/key_ciphertexts.txt: the seeds
 *                  alone cost the call 1.61-1.73 ms for any batch up to 2^12 and the host 46-48 us a pair: 1.47 ms at 2^5, 0.91x and 0.91x, 3.00 ms at 2^6, 1.86x and
 *                  1.86x; with every account output the call takes 3.8-4.4 ms and the host 221 us a pair: 3.55 ms at 2^4, 0.81x and 0.81x, 7.08 ms at 2^5, 1.62x
 *                  and 1.61x); ALEO_MI355X_MIN_KEY_CIPHERTEXTS overrides it, read per call (a bad value: the default).
 * No aleo_mi355x_last_error message of these calls holds a secret, a seed or a key. */
int32_t aleo_mi355x_private_key_encrypt(char* out, size_t cap, const char* private_key, const void* secret, size_t secret_len, const void* nonce32);
int32_t aleo_mi355x_private_key_decrypt(char* out, size_t cap, const char* ciphertext, const void* secret, size_t secret_len);
int32_t aleo_mi355x_private_keys_open(const char* text, const uint64_t* offsets, const void* secrets, const uint64_t* secret_offsets, size_t n, void* seeds32, void* sk_sig32,
                                      void* view_key32, void* address_x32, char* address63, uint8_t* flags);
int32_t aleo_mi355x_private_keys_open_host(const char* text, const uint64_t* offsets, const void* secrets, const uint64_t* secret_offsets, size_t n, void* seeds32, void* sk_sig32,
                                           void* view_key32, void* address_x32, char* address63, uint8_t* flags);
size_t aleo_mi355x_min_key_ciphertexts(void);

const char* aleo_mi355x_strerror(int32_t status);
const char* aleo_mi355x_last_error(void);   /* thread-local detail string of the last failure */
const char* aleo_mi355x_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ALEO_MI355X_H */
