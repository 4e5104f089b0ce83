// msm.hip — what ONE launch chain of the BLS12-377 G1 Pippenger multi-scalar multiplication does on the GPU (MI355X, gfx950).
// Replaces snarkvm-algorithms 0.14.5  algorithms/src/msm/variable_base/{mod,standard,batched}.rs
// `VariableBase::msm(bases, scalars)` [UPSTREAM-RECALL; pin /root/reference/Cargo.lock:2200], reached from
// /root/reference/rust/src/program/execute.rs:74,177 and transfer.rs:99 through Varuna's KZG commitments.
// Same mathematical function (sum_i s_i * P_i); the schedule is GPU-first, not a translation.  The scalar side (digits, sort, slices) is
// msm_sort.hip; which chains a request becomes and where they run is msm_request.hip; tables and base sets are built by g1_setup.hip; the slice-tree
// kernel, the plain path's reduction kernels and its host back end are msm_reduce.h, which g2.hip instantiates for G2.
//
//   tiers     a pinned set's fixed-base tables (rows 2^win_offset(w) * P_i): c = 20 / 17 for the whole set, c = 16 for its first 2^17 points, c = 13 for its
//             first 2^15, optionally a range table over a sub-range.  All windows of a result feed ONE set of 2^(c-1) buckets; a chain carries several results.
//             Without a tier: the plain schedule, c <= 16, every window its own buckets.
//   accum     one lane per slice, XYZZ mixed additions on 14 x 28-bit limbs (fp28.h), gathering 28-bit affine rows at a 128-byte stride.
//   tree      slices of multi-slice buckets are folded pairwise (short launches over the listed buckets only).
//   reduce    sum_b (b+1) * S_b.  Table path: running sums over chunks of S buckets, then the chunk weights by ONE sum tree from c >= 13 (k_prog_*), by lg(N)
//             masked pairwise trees below.  Plain path: chunk sums with a double-and-add of the chunk base, a pairwise tree per window.
//   tail      table path: lg(N) + 1 (sum tree) or lg(N) + 4 (masked) points per result land in pinned host memory, Horner on the host.  Plain: the W
//             window sums go to the host for the 2^c Horner chain (~250 dependent doublings are ~0.1 ms on a host core, ~4 ms on one GPU lane).
// HBM layout: bases n x 96 B (x|y Montgomery, AoS so a gathered point is 1-2 cache lines), their 28-bit rows and the tables' W x n x 128 B; sorted stream n*W x 4 B; partial sums
// #slices x 192 B (XYZZ) or 224 B (28-bit XYZZ).  Algorithmic bytes per point: 32 (scalar) + 96 (base).
#include "msm_table.h"
#include "msm_te.h"
#include "te28_host.hpp"

namespace aleo_mi355x {

// ---- bucket accumulation: one lane per slice, in the 14 x 28-bit representation (fp28.h) -----------------------------
// Point rows are 112 bytes (x'[14] | y'[14], value * 2^392 mod q as exact base-2^28 digits): table rows on the fixed-base path,
// the pinned set's own 28-bit rows on the plain path.  OUT28: the slice sum is stored as a 224-byte 28-bit XYZZ point (the
// table path's reduction continues in that form); otherwise it is converted to a 32-bit XYZZ point for the plain path's
// per-window reduction kernels.
__device__ __forceinline__ XYZZ xyzz28_to_xyzz(const XYZZ28& a) {
  XYZZ r; r.X = f28_to_fq(a.X); r.Y = f28_to_fq(a.Y); r.ZZ = f28_to_fq(a.ZZ); r.ZZZ = f28_to_fq(a.ZZZ); return r;     // all < 2q
}
__device__ __noinline__ void slice_slow_path28(const char* bases, const uint32_t* run, uint32_t j, uint32_t j1, const XYZZ28* acc28, XYZZ* acc_out, bool* inf_out) {
  XYZZ acc = xyzz28_to_xyzz(*acc28); bool inf = false;
  for (; j < j1; ++j) {
    uint32_t e = run[j];
    F28 x, y; load_affine28(bases + (size_t)(e & 0x7fffffffu) * ROW28, x, y);
    AffinePt p; p.x = Fq::reduce(f28_to_fq(x)); p.y = Fq::reduce(f28_to_fq(y));
    if (e >> 31) p.y = fq_neg_canonical(p.y);
    xyzz_madd(acc, inf, p.x, p.y);
  }
  *acc_out = acc; *inf_out = inf;
}


template <bool OUT28, bool SEED = false>
__global__ void __launch_bounds__(256) k_accum28(const char* __restrict__ bases, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ hist,
                                                 const uint2* __restrict__ scan_local, const uint2* __restrict__ scan_blk, const uint32_t* __restrict__ total_pairs, uint32_t M,
                                                 const uint32_t* __restrict__ meta, const uint32_t* __restrict__ order, const uint32_t* __restrict__ task_g,
                                                 char* __restrict__ partial, FrontChain seed) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= meta[0]) return;
  const uint32_t sid = order[t], g = task_g[sid];
  uint2 st = scan_at(scan_local, scan_blk, g);
  uint32_t cnt = hist[g], m = slices_of(cnt, pick_rule(total_pairs, M)), k = sid - st.y;
  uint32_t j0 = (uint32_t)(((uint64_t)k * cnt) / m), j1 = (uint32_t)(((uint64_t)(k + 1) * cnt) / m);
  const uint32_t* run = sorted + st.x;
  uint32_t e_next = run[j0];
  F28 xn, yn; load_affine28(bases + (size_t)(e_next & 0x7fffffffu) * ROW28, xn, yn);      // next point's 112-byte gather in flight under the current addition
  XYZZ28 acc; bool ok = true;
  uint32_t j = j0;
  bool seeded = false;
  if constexpr (SEED) {
    // first slice of the bucket: continue from what the earlier chunks of this request summed into the same bucket (a stored point: Y may be loose,
    // class L3 < 6q — one product by R brings it to the loop's invariant, exact digits < 2q); an empty or identity sum starts the usual way
    const char* sp = k == 0 ? chain_sum(seed, g) : nullptr;
    if (sp) {
      acc.ZZ = load_f28(sp + 112);
      if (!f28_is_zero_raw(acc.ZZ)) { acc.X = load_f28(sp); acc.Y = f28_mul(load_f28(sp + 56), f28_const(ONE28)); acc.ZZZ = load_f28(sp + 168); seeded = true; }
    }
  }
  if (!seeded) {   // first point of the slice: acc = (x, +-y, 1, 1)
    uint32_t e = e_next; F28 x = xn, y = yn;
    if (j + 1 < j1) { e_next = run[j + 1]; load_affine28(bases + (size_t)(e_next & 0x7fffffffu) * ROW28, xn, yn); }
    if (e >> 31) y = f28_sub<2, 1>(f28_const(Limbs14{}), y);                            // 2q - y: limbs < 2^29
    acc.X = x; acc.Y = y; acc.ZZ = f28_const(ONE28); acc.ZZZ = f28_const(ONE28);
    ++j;
  }
  for (; j < j1; ++j) {
    uint32_t e = e_next; F28 x = xn, y = yn;
    if (j + 1 < j1) { e_next = run[j + 1]; load_affine28(bases + (size_t)(e_next & 0x7fffffffu) * ROW28, xn, yn); }
    if (e >> 31) y = f28_sub<2, 1>(f28_const(Limbs14{}), y);
    if (!xyzz28_madd_fast(acc, x, y)) { ok = false; break; }
  }
  if (ok) {
    if constexpr (OUT28) store_xyzz28(partial + (size_t)sid * 224, acc);      // X exact < 12q, Y exact < 2q, ZZ / ZZZ exact < 2q: the stored invariant of fp28.h
    else xyzz_store_normalized(partial + (size_t)sid * 192, xyzz28_to_xyzz(acc), false);   // plain path: its reduction kernels work on 32-bit points
  } else {    // P == +-acc (repeated or opposite bases): finish the slice with the general 32-bit code, out of line
    XYZZ28 tmp = acc; XYZZ out; bool inf = false;
    slice_slow_path28(bases, run, j, j1, &tmp, &out, &inf);
    if constexpr (OUT28) store_xyzz28_from32(partial + (size_t)sid * 224, out, inf);
    else xyzz_store_normalized(partial + (size_t)sid * 192, out, inf);
  }
}

// (the kernels below are msm_table.h's bodies for 28-bit XYZZ points; msm_te.hip holds the Edwards tier's)
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_tree_rest(char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t list_len, const uint2* __restrict__ scan_local,
                                                   const uint2* __restrict__ scan_blk, uint32_t M, const uint32_t* __restrict__ meta) {
  tree_rest_body<Pt28, LANES>(partial, list, list_len, scan_local, scan_blk, M, meta);
}

__global__ void k_gather_super(const char* __restrict__ partial, const uint32_t* __restrict__ list, uint32_t len, const uint2* __restrict__ scan_local,
                               const uint2* __restrict__ scan_blk, uint32_t* __restrict__ dst) {
  gather_super_body(partial, list, len, scan_local, scan_blk, dst, nullptr);
}

template <bool F28> using PtFmt = std::conditional_t<F28, Pt28, Pt32>;      // the formats: msm_reduce.h
template <bool F28, uint32_t LANES = 2>
__global__ void __launch_bounds__(256) k_bucket_chunks(const char* __restrict__ partial, const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local,
                                                       const uint2* __restrict__ scan_blk, uint32_t B, uint32_t S, uint32_t nchunks_total, char* __restrict__ V,
                                                       uint32_t v_set_stride, char* __restrict__ Vrun, FrontChain older) {
  bucket_chunks_body<PtFmt<F28>, LANES>(partial, hist, scan_local, scan_blk, B, S, nchunks_total, V, v_set_stride, Vrun, older, 0u);
}

// Plain path (one window set per window): one lane per chunk, V = sum_{b in chunk} (b+1) * S_b with the chunk base applied
// by double-and-add.  (The pair form loses here: the double-and-add tail is most of the chain and would idle odd lanes.)
__global__ void __launch_bounds__(256) k_bucket_chunks_plain(const char* __restrict__ partial, const uint32_t* __restrict__ hist, const uint2* __restrict__ scan_local,
                                                             const uint2* __restrict__ scan_blk, uint32_t B, uint32_t S, uint32_t nchunks_total, char* __restrict__ V) {
  uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nchunks_total) return;
  uint32_t cpw = B / S, w = t / cpw, j = t % cpw;
  uint32_t g0 = w * B + j * S;
  XYZZ run = xyzz_infinity(), acc = xyzz_infinity();
  // steps 2k: run += S_b (b descending); steps 2k+1: acc += run   (one inlined xyzz_add call site)
  for (uint32_t k = 0; k < 2 * S; ++k) {
    bool odd = k & 1;
    XYZZ y;
    if (!odd) {
      uint32_t g = g0 + (S - 1 - (k >> 1));
      if (hist[g]) y = load_xyzz(partial + (size_t)scan_at(scan_local, scan_blk, g).y * 192); else y = xyzz_infinity();
    } else y = run;
    XYZZ x = odd ? acc : run;
    xyzz_add(x, y);
    if (odd) acc = x; else run = x;
  }
  uint32_t base = j * S;
  if (base) {
    XYZZ r = xyzz_infinity();
    for (int bit = 31 - __clz(base); bit >= 0; --bit) {
      xyzz_double_ni(&r);
      if ((base >> bit) & 1) xyzz_add_ni(&r, &run);
    }
    xyzz_add_ni(&acc, &r);
  }
  store_xyzz(V + (size_t)t * 192, acc);
}

// Fixed-base path: sum_j j * run_j = sum_l 2^l * T_l with T_l = sum of run_j over the j that have bit l set.  This
// kernel does the first pairwise level of all lg(N) masked sums at once: T_l[k] = run[ins_l(2k)] + run[ins_l(2k+1)],
// ins_l(x) = x with a 1 inserted at bit l.  The remaining levels are k_seg_pair_pass / k_seg_fold; the 2^l Horner runs
// on the host.
// (These kernels only run on the table path, whose points are 224-byte 28-bit XYZZ: PB below.)
// Sets (batched calls): set q reads Vrun[q * 2^lgN ...] and writes its lgN sums behind its chunk sums, at
// V[q * v_set_stride + 2^lgN ...] (v_set_stride = (lgN + 4) * 2^(lgN-2): the set's 4 + lgN segments are contiguous).
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_masked_pairs(const char* __restrict__ Vrun, uint32_t lgN, uint32_t nsets, char* __restrict__ V, uint32_t v_set_stride) {
  const uint32_t seg_len = 1u << (lgN - 2);
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> lg_lanes(LANES);
  if (op >= seg_len * lgN * nsets) return;
  const uint32_t q = op / (seg_len * lgN), r = op % (seg_len * lgN), l = r / seg_len, k = r % seg_len;
  auto ins = [&](uint32_t x) { return ((x >> l) << (l + 1)) | (1u << l) | (x & ((1u << l) - 1u)); };
  const char* run = Vrun + ((size_t)q << lgN) * PB28;
  Pt28::add<LANES>(run + (size_t)ins(2 * k) * PB28, run + (size_t)ins(2 * k + 1) * PB28, V + ((size_t)q * v_set_stride + (1u << lgN) + r) * PB28);
}
// One block folds up to 256 consecutive points of one segment into a single point: 8 tree levels through two LDS
// buffers, 128 lane pairs — the latency floor of the chain with no launch gaps.
// (the block has FOLD / 2 lane groups: 256 threads as pairs, 512 as quads — the quad form halves the latency of each of the 8 levels)
template <uint32_t LANES>
__global__ void __launch_bounds__(128 * LANES) k_seg_fold(const char* __restrict__ in, uint32_t in_stride, uint32_t L, uint32_t nseg,
                                                          char* __restrict__ out, uint32_t out_stride) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[2][(FOLD / 2) * PW28];
  const uint32_t bps = (L + FOLD - 1) / FOLD, seg = blockIdx.x / bps, blk = blockIdx.x % bps, pr = threadIdx.x >> lg_lanes(LANES);
  if (seg >= nseg) return;
  {
    const uint32_t e0 = blk * FOLD + 2 * pr;
    const char* src = in + ((size_t)seg * in_stride + e0) * PB28;
    char* dst = (char*)(lds[0] + pr * PW28);
    if (e0 + 1 < L) Pt28::add<LANES>(src, src + PB28, dst);
    else if (e0 < L) grp_copy<LANES, PB28>(src, dst);
    else grp_zero<LANES, PB28>(dst);
  }
  uint32_t cur = 0;
  for (uint32_t n = FOLD / 2; n > 1; n >>= 1) {
    __syncthreads();
    if (pr < (n >> 1)) Pt28::add<LANES>((const char*)(lds[cur] + (2 * pr) * PW28), (const char*)(lds[cur] + (2 * pr + 1) * PW28), (char*)(lds[cur ^ 1] + pr * PW28));
    cur ^= 1;
  }
  __syncthreads();
  if (pr == 0) grp_copy<LANES, PB28>((const char*)lds[cur], out + ((size_t)seg * out_stride + blk) * PB28);
}
// out[seg][i] = in[seg][2i] + in[seg][2i+1]: the wide (throughput-bound) levels of the segment sums
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_seg_pair_pass(const char* __restrict__ in, uint32_t in_stride, uint32_t L, uint32_t nseg,
                                                       char* __restrict__ out, uint32_t out_stride) {
  const uint32_t half = (L + 1) >> 1;
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> lg_lanes(LANES);
  if (op >= half * nseg) return;
  const uint32_t seg = op / half, i = op % half;
  const char* src = in + ((size_t)seg * in_stride + 2 * i) * PB28;
  char* dst = out + ((size_t)seg * out_stride + i) * PB28;
  if (2 * i + 1 < L) Pt28::add<LANES>(src, src + PB28, dst); else grp_copy<LANES, PB28>(src, dst);
}
// The chunk weights by ONE sum tree (msm_table.h prog_pass_body, prog_pass2_body, prog_final_body)
template <uint32_t LANES>
__global__ void __launch_bounds__(256) k_prog_pass(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                   const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                   char* __restrict__ out, uint32_t out_set_stride) {
  prog_pass_body<Pt28, LANES>(node, node_set_stride, A, a_set_stride, T, t_set_stride, nT, L, nsets, out, out_set_stride, nullptr);
}
__global__ void __launch_bounds__(256) k_prog_pass2(const char* __restrict__ node, uint32_t node_set_stride, const char* __restrict__ A, uint32_t a_set_stride,
                                                    const char* __restrict__ T, uint32_t t_set_stride, uint32_t nT, uint32_t L, uint32_t nsets,
                                                    char* __restrict__ out, uint32_t out_set_stride) {
  prog_pass2_body<Pt28>(node, node_set_stride, A, a_set_stride, T, t_set_stride, nT, L, nsets, out, out_set_stride, nullptr);
}
template <uint32_t LANES>
__global__ void __launch_bounds__(128 * LANES) k_prog_final(const char* __restrict__ in, uint32_t in_set_stride, uint32_t L, uint32_t nT, uint32_t lgL, uint32_t nsets,
                                                            char* __restrict__ out) {
  prog_final_body<Pt28, LANES>(in, in_set_stride, L, nT, lgL, nsets, out, nullptr, nullptr);
}
__global__ void k_gather_strided(const char* __restrict__ V, uint32_t stride, uint32_t count, char* __restrict__ out) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * 14) return;
  uint32_t w = t / 14, q = t % 14;
  ((uint4*)out)[t] = ((const uint4*)(V + (size_t)w * stride * PB28))[q];
}

int32_t msm_front_sort(Ctx* c, const PinnedBases& pb, const MsmJob& job, hipStream_t s, Front& f) {
  const uint32_t K = f.K = job.k;
  size_t n = 0, pts = 0; SegArgs segs{};
  if (K > MAX_SETS || job.nseg > MAX_SEGS) { g_last_error = "msm: too many sets / segments in one call"; return ALEO_MI355X_ERR_BAD_ARG; }
  for (uint32_t q = 0; q < job.nseg; ++q) {
    const MsmSeg& g = job.segs[q];
    if (g.len == 0) continue;
    if (g.out >= K || g.off + g.len >= (1ull << 31)) { g_last_error = "msm: segment out of range"; return ALEO_MI355X_ERR_BAD_ARG; }
    const uint32_t i = segs.nseg++;
    segs.ptr[i] = (const char*)g.d_ptr; segs.n[i] = (uint32_t)g.len; segs.off[i] = (uint32_t)g.off; segs.set[i] = (uint8_t)g.out;
    n = g.off + g.len > n ? g.off + g.len : n; pts += g.len;
  }
  if (n == 0) { f.empty = true; return ALEO_MI355X_OK; }
  if (job.tier_n > n && job.tier_n <= pb.n) n = job.tier_n;
  if (n > pb.n) { g_last_error = "msm: a segment reaches past the pinned bases"; return ALEO_MI355X_ERR_BAD_ARG; }
  // the fixed-base table serves any prefix of the pinned set (row stride = pinned count) as long as the prefix still
  // puts about one point into every bucket; shorter prefixes use the plain path with its small bucket count
  const PinnedBases::PreTable* T = nullptr;
  const uint8_t* d_inf = pb.d_inf;
  bool ranged = job.sparse && pb.range.d != nullptr;       // the narrow-window table of one sub-range, when every segment lies inside it
  for (uint32_t i = 0; ranged && i < segs.nseg; ++i) ranged = segs.off[i] >= pb.range_off && (size_t)segs.off[i] + segs.n[i] <= pb.range_off + pb.range.cover;
  if (ranged) {
    T = &pb.range; n = 0;
    for (uint32_t i = 0; i < segs.nseg; ++i) { segs.off[i] -= (uint32_t)pb.range_off; n = (size_t)segs.off[i] + segs.n[i] > n ? (size_t)segs.off[i] + segs.n[i] : n; }
    if (d_inf) d_inf += pb.range_off;
  } else T = msm_tier(pb, n);
  const bool pre = f.pre = T != nullptr;
  f.te = pre && T->te;
  if (K > 1 && (!pre || K > (ranged ? msm_range_sets(pb) : msm_max_sets(pb, n)))) { g_last_error = "msm: internal: batch without a table tier (or too many sets)"; return ALEO_MI355X_ERR_BAD_ARG; }
  MsmPlan& P = f.P; P = make_plan(pre ? n : pts, pre ? T->c : 0);
  if (pre) { P.W = K; P.M = K * P.B; }                       // after the sort a set is "a window with its own buckets"
  if (!pre && !pb.d_xy28) { g_last_error = "msm: pinned set without 28-bit rows"; return ALEO_MI355X_ERR_HIP; }
  f.bases = (const char*)(pre ? T->d : pb.d_xy28);          // 112-byte rows, or the Edwards tier's 168-byte ones (f.te)
  f.plain_tree = k_tree_pass<Pt32, 2>;
  const uint32_t cpw = f.cpw = P.B / P.S, nchunks = f.nchunks = cpw * P.W;
  uint32_t lgN = 0; while ((1u << lgN) < cpw) ++lgN;
  f.lgN = lgN;
  const bool masked = f.masked = pre && lgN >= 2 && (1u << lgN) == cpw;          // fixed-base path: weights by masked trees
  if (pre && !masked) { g_last_error = "msm: internal: table path without masked reduction"; return ALEO_MI355X_ERR_HIP; }
  int32_t rc;
  // table path, per set: [acc of its cpw chunks | lgN masked sums of cpw/4] = (lgN + 4) segments of tseg points
  const uint32_t tseg = f.tseg = cpw / 4, fseg = f.fseg = lgN + 4, nseg = f.nseg = K * fseg, setw = f.setw = fseg * tseg;
  // Sum trees (k_prog_*) against masked trees: reduce phase of the 2^20 MSM 0.464 -> 0.412 ms at S = 16 (S = 8: 0.537 -> 0.451, S = 4: 0.720 -> 0.508: the
  // chunk kernel is bound by its 2 additions per bucket, not by their order, so smaller chunks still lose); on the small tables too: 2^15-constraint proof
  // 6.47 -> 6.35 ms, eight instances at 2^13 7.19 -> 6.88 ms.  Below c = 13 the masked trees stay.
  constexpr uint32_t SUM_TREE_MIN_C = 13;
  f.prog = masked && P.c >= SUM_TREE_MIN_C && cpw > FOLD;      // (a set of <= 256 chunks would go straight to the final fold: the masked form keeps those)
  f.out_pts = f.prog ? 1 + lgN : fseg;                        // sum tree: sum_j acc_j and the lgN weights T_l; masked trees: every one of the set's segments
  f.vpoints = masked ? (size_t)K * setw + nchunks + (nseg + 1) + (size_t)nseg * (tseg / 2 + tseg / 4 + 2) + 3 * (size_t)nchunks + 64 : (size_t)nchunks + P.W;      // + the two buffers of the sum-tree passes (3 cpw / 2 points per set each)
  if ((rc = ensure_host_pinned(c, 64 + (size_t)(masked ? nseg : P.W) * 224 + ASIDE_MAX * 228 + 64 + (size_t)nseg * 4))) return rc;      // before the sort phase: its read-back lands in this buffer (behind the aside records: the Edwards tier's flag words)
  SortPhase& sp = f.sp;
  if ((rc = msm_sort_phase(c, segs, pts, job.mont, d_inf, (uint32_t)(pre ? T->cover : pb.n), P, pre, s, &sp, f.lean))) return rc;
  const uint32_t M = sp.M;
  if ((rc = c->partial.reserve(sp.slices_max * (pre ? 224 : 192)))) return rc;
  if ((rc = c->vbuf.reserve(f.vpoints * 224))) return rc;
  return ALEO_MI355X_OK;
}

int32_t msm_front_accum(Ctx* c, hipStream_t s, Front& f, const FrontChain* seed, hipEvent_t after) {
  const SortPhase& sp = f.sp; const uint32_t M = sp.M; const char* bases = f.bases;
  char* partial = c->partial.as<char>();
  if (after) HIPCHK(hipStreamWaitEvent(s, after, 0));
  if (!f.lean) HIPCHK(hipEventRecord(c->ev[6], s));          // ev[6]..ev[5] bracket k_accum28 alone (bench.py's roofline kernel)
  const bool seeded = f.pre && seed && seed->n;
  auto* const kern = seeded ? k_accum28<true, true> : f.pre ? k_accum28<true, false> : k_accum28<false, false>;
  if (f.te) te_accum(seeded, s, bases, sp, partial, seeded ? *seed : FrontChain{});
  else hipLaunchKernelGGL(kern, dim3(sp.slice_blocks), dim3(256), 0, s, bases, sp.sorted, sp.hist, sp.scan_local, sp.scan_blk, sp.total_pairs, M, sp.meta, sp.order, sp.task_g, partial, seeded ? *seed : FrontChain{});
  if (!f.lean) HIPCHK(hipEventRecord(c->ev[5], s));
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

int32_t msm_front_finish(Ctx* c, hipStream_t s, Front& f, bool allow_aside) {
  int32_t rc;
  const SortPhase& sp = f.sp; SliceMeta& sm = f.sm; const uint32_t M = sp.M; const bool pre = f.pre;
  uint32_t* heavy = sp.heavy; uint32_t* meta = sp.meta; uint2* scan_local = sp.scan_local; uint2* scan_blk = sp.scan_blk;
  char* partial = c->partial.as<char>();
  if ((rc = msm_wait_meta(c, sp, s, &sm))) return rc;
  // A handful of super-heavy buckets (witness-like scalars: the digit-1 bucket of the lowest window holds a fifth of the points) have a slice tree of
  // 10+ dependent levels while the common list is done after 4.  Then the long trees run ASIDE, on the slot's side stream, over slices 1.. of their
  // buckets; the reduction below goes ahead with slice 0 as those buckets' sums, and the host adds (b + 1) * (sum of slices 1..) to the result.
  const bool aside = f.aside = allow_aside && f.masked && sm.n_super >= 1 && sm.n_super <= ASIDE_MAX && !sm.super_overflow && sm.max_m >= 64;
  uint32_t* h_aside = (uint32_t*)((char*)c->h_pinned + 64 + (size_t)f.nseg * 224);
  if (aside) {
    if (f.lean) HIPCHK(hipEventRecord(c->ev[5], s));          // (nothing has been queued behind the accumulation yet: the same position)
    HIPCHK(hipStreamWaitEvent(c->side, c->ev[5], 0));
    for (uint32_t pass = 0, L = sm.max_m - 1; L > 1; ++pass, L = (L + 1) >> 1) {
      const uint64_t ops = (uint64_t)sm.n_super * (L >> 1);
      if (f.te) te_tree_pass(grp_lanes(ops), ops, c->side, partial, heavy, 0u, 0u, sp.super_list, sm.n_super, L >> 1, sp, pass, 1u);
      else launch_grp(grp_lanes(ops), k_tree_pass<Pt28, 4>, k_tree_pass<Pt28, 2>, ops, c->side, partial, heavy, 0u, 0u, sp.super_list, sm.n_super, L >> 1, scan_local, scan_blk, M, meta, pass, 1u);
    }
    uint32_t* dst = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&dst, h_aside, 0));
    if (f.te) te_gather_super(c->side, partial, sm.n_super, sp, dst);
    else hipLaunchKernelGGL(k_gather_super, dim3((sm.n_super * 57 + 255) / 256), dim3(256), 0, c->side, partial, sp.super_list, sm.n_super, scan_local, scan_blk, dst);
    HIPCHK(hipEventRecord(c->ev[4], c->side));
  }
  // the levels behind the first in one launch (k_tree_rest) when only the common list is left and no bucket has more than 8 slices
  const bool rest_ok = pre && !sm.super_overflow && (aside || sm.n_super == 0) && sm.n_heavy && sm.max_common > 2 && sm.max_common <= 8;
  if (sm.NT) {
    for (uint32_t pass = 0, L = sm.max_m, Lcm = sm.max_common; L > 1; ++pass, L = (L + 1) >> 1, Lcm = (Lcm + 1) >> 1) {
      if (rest_ok && pass == 1) {
        if (f.te) te_tree_rest(s, partial, heavy, sm.n_heavy, sp);
        else hipLaunchKernelGGL(k_tree_rest<4>, dim3((uint32_t)((4ull * sm.n_heavy + 255) / 256)), dim3(256), 0, s, partial, heavy, sm.n_heavy, scan_local, scan_blk, M, meta);
        break;
      }
      const uint32_t Lc = sm.super_overflow ? L : Lcm;       // longest bucket of the common list at this level
      const uint32_t len_a = (sm.n_heavy && Lc > 1) ? sm.n_heavy : 0, pairs_a = len_a ? Lc >> 1 : 0;
      const uint32_t len_b = aside ? 0 : sm.n_super, pairs_b = len_b ? L >> 1 : 0;
      const uint64_t ops = (uint64_t)len_a * pairs_a + (uint64_t)len_b * pairs_b;
      const uint32_t lanes = pre ? grp_lanes(ops) : 2u;                                                // quads while the level is latency-bound (28-bit points only)
      const uint64_t threads = lanes * ops;
      if (!threads) continue;
      if (threads >= (1ull << 32)) { (void)hipStreamSynchronize(s); g_last_error = "msm: slice tree too wide"; return ALEO_MI355X_ERR_HIP; }
      if (f.te) te_tree_pass(lanes, ops, s, partial, heavy, len_a, pairs_a, sp.super_list, len_b, pairs_b, sp, pass, 0u);
      else launch_grp(lanes, k_tree_pass<Pt28, 4>, pre ? k_tree_pass<Pt28, 2> : f.plain_tree, ops, s, partial, heavy, len_a, pairs_a, sp.super_list, len_b, pairs_b, scan_local, scan_blk, M, meta, pass, 0u);
    }
  }
  if (!f.lean) HIPCHK(hipEventRecord(c->ev[2], s));
  return ALEO_MI355X_OK;
}

// Table path: sum_b (b+1) S_b per set, queued on s behind the slice trees, ev[3] recorded behind the last launch.
int32_t msm_reduce_queue(Ctx* c, Front& f, hipStream_t s, const FrontChain& older) {
  const MsmPlan& P = f.P; const SortPhase& sp = f.sp;
  const uint32_t K = f.K, cpw = f.cpw, nchunks = f.nchunks, lgN = f.lgN, tseg = f.tseg, nseg = f.nseg, setw = f.setw;
  uint32_t* hist = sp.hist; uint2* scan_local = sp.scan_local; uint2* scan_blk = sp.scan_blk;
  char* partial = c->partial.as<char>(); char* V = c->vbuf.as<char>(); char* h_win = (char*)c->h_pinned + 64;
  // per set: sum_b (b+1) S_b = sum_j acc_j + S * sum_j j * run_j ; the second sum by lg(N) masked pairwise trees
  char* Vrun = V + (size_t)K * setw * PB28; char* Tout = Vrun + (size_t)nchunks * PB28;
  // 2^19 buckets keep the chip busy with one lane pair per chunk; the small bucket sets (<= 2^16) are pure latency and take the quad form
  // (masked => pre: the partial sums are 28-bit points)
  // every launch below picks lanes per addition by its own width (grp_lanes): four while it is latency-bound, two once the additions fill the chip
  // wide tables (2^19 buckets, S = 16): one lane pair per chunk (32 dependent additions) against two pairs one step apart (17): reduce phase 0.487 -> 0.460 ms
  // at 2^20; S = 8 / 32 / 4 with either form: 0.51-0.54 / 0.48-0.55 / 0.66-0.72 ms
  const uint32_t lanes = grp_lanes(2 * (uint64_t)nchunks), per_block = lanes == 4 ? 32u : CHUNK_QUADS;      // (its own geometry: two lane groups per chunk)
  auto* const chunks = lanes == 4 ? k_bucket_chunks<true, 4> : k_bucket_chunks<true, 2>;
  if (f.te && !f.prog) { g_last_error = "msm: internal: Edwards tier without the sum-tree reduction"; return ALEO_MI355X_ERR_HIP; }      // (the whole-set tier's windows always take it)
  if (f.te) te_bucket_chunks(lanes, s, partial, sp, P.B, P.S, nchunks, V, setw, Vrun, older);
  else hipLaunchKernelGGL(chunks, dim3((nchunks + per_block - 1) / per_block), dim3(256), 0, s, partial, hist, scan_local, scan_blk, P.B, P.S, nchunks, V, setw, Vrun, older);
  if (f.prog) {
    char* G0 = Tout; char* G1 = G0 + (size_t)K * (3 * (cpw / 2)) * PB28;      // ping-pong: a set is at most 3 segments of cpw / 2 points after the first pass
    const char* node = Vrun; uint32_t node_ss = cpw; const char* A = V; uint32_t a_ss = setw; const char* T = Vrun; uint32_t t_ss = 0, nT = 0, L = cpw;
    char* dstbuf = G0;
    while (L > FOLD) {
      const uint32_t half = L >> 1, out_ss = (3 + nT) * half; const uint64_t ops = (uint64_t)(2 + nT) * half * K;
      if ((L >> 2) >= FOLD && grp_lanes(ops) == 4) {      // two levels at once: L -> L / 4
        const uint32_t quarter = L >> 2, out2 = (4 + nT) * quarter; const uint64_t octs = (uint64_t)(2 + nT) * quarter * K;
        if (f.te) te_prog_pass2(octs, s, node, node_ss, A, a_ss, T, t_ss, nT, L, K, dstbuf, out2, sp);
        else hipLaunchKernelGGL(k_prog_pass2, dim3((uint32_t)((octs + 31) / 32)), dim3(256), 0, s, node, node_ss, A, a_ss, T, t_ss, nT, L, K, dstbuf, out2);
        node = dstbuf; node_ss = out2; A = dstbuf + (size_t)quarter * PB28; a_ss = out2; T = dstbuf + (size_t)2 * quarter * PB28; t_ss = out2; nT += 2; L = quarter;
        dstbuf = dstbuf == G0 ? G1 : G0;
        continue;
      }
      if (f.te) te_prog_pass(grp_lanes(ops), ops, s, node, node_ss, A, a_ss, T, t_ss, nT, L, K, dstbuf, out_ss, sp);
      else launch_grp(grp_lanes(ops), k_prog_pass<4>, k_prog_pass<2>, ops, s, node, node_ss, A, a_ss, T, t_ss, nT, L, K, dstbuf, out_ss);
      node = dstbuf; node_ss = out_ss; A = dstbuf + (size_t)half * PB28; a_ss = out_ss; T = dstbuf + (size_t)2 * half * PB28; t_ss = out_ss; ++nT; L = half;
      dstbuf = dstbuf == G0 ? G1 : G0;
    }
    uint32_t lgL = 0; while ((1u << lgL) < L) ++lgL;
    char* dst = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&dst, h_win, 0));
    if (f.te) te_prog_final(K * (1 + nT + lgL), s, node, node_ss, L, nT, lgL, K, dst, sp, (uint32_t*)(dst + (size_t)nseg * 224 + ASIDE_MAX * 228 + 64));      // (K (1 + lgN) <= nseg flag words behind the aside records)
    else hipLaunchKernelGGL(k_prog_final<4>, dim3(K * (1 + nT + lgL)), dim3(512), 0, s, node, node_ss, L, nT, lgL, K, dst);
  } else {
    const uint64_t mops = (uint64_t)tseg * lgN * K;
    launch_grp(grp_lanes(mops), k_masked_pairs<4>, k_masked_pairs<2>, mops, s, Vrun, lgN, K, V, setw);
    // K * (lgN+4) segment sums: pairwise launches while a level still fills the chip, then ONE block per segment folds the
    // last 256 points through LDS (8 levels of lane-pair additions: the latency floor of the chain, no launch gaps)
    char* F1 = Tout + (size_t)(nseg + 1) * PB28; char* F2 = F1 + (size_t)nseg * (tseg / 2 + 1) * PB28;
    const char* cur = V; uint32_t L = tseg, stride = tseg;
    while (L > FOLD) {
      char* dst = (cur == F1) ? F2 : F1; uint32_t half = (L + 1) >> 1;
      const uint64_t ops = (uint64_t)half * nseg;
      launch_grp(grp_lanes(ops), k_seg_pair_pass<4>, k_seg_pair_pass<2>, ops, s, cur, stride, L, nseg, dst, half);
      cur = dst; stride = half; L = half;
    }
    if (L > 1) {
      // the last fold leaves one point per segment, contiguous: it stores them straight into the slot's pinned host buffer (device-
      // mapped), so the result needs neither a gather launch nor a copy — the host's wait in msm_collect is all that is left
      char* dst = nullptr;
      HIPCHK(hipHostGetDevicePointer((void**)&dst, h_win, 0));
      hipLaunchKernelGGL(k_seg_fold<4>, dim3(nseg), dim3(512), 0, s, cur, stride, L, nseg, dst, 1u);
    } else {
      hipLaunchKernelGGL(k_gather_strided, dim3((nseg * 14 + 255) / 256), dim3(256), 0, s, cur, stride, nseg, Tout);
      HIPCHK(hipMemcpyAsync(h_win, Tout, (size_t)nseg * PB28, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHK(hipEventRecord(c->ev[3], s));
  if (f.lean && older.n == 0 && !f.aside) {                  // single-chain prover commitments: clear the sort's block for the next chain now, under the host tail (ev[3] sits in front of it; not with trees still running aside: they read the lists in that block)
    // (as much as the largest chain seen on this context needs, within the allocation: a proof's chains differ in size, and a chain larger than its predecessor would fill again)
    if (sp.zero_bytes > c->hist_zero_max) c->hist_zero_max = sp.zero_bytes;
    const size_t z = c->hist_zero_max <= c->hist.cap && (void*)sp.hist == c->hist.p ? c->hist_zero_max : sp.zero_bytes;
    HIPCHK(hipMemsetAsync(sp.hist, 0, z, s)); c->hist_clean = z; c->hist_clean_stream = s; c->hist_clean_ptr = (void*)sp.hist;
  }
  return ALEO_MI355X_OK;
}

int32_t phase_times(Ctx* c, const Front& f, std::chrono::steady_clock::time_point t_host0) {
  const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  float ms; MsmTiming tm;
  if (f.lean) { tm.host = host_ms; tm.total = host_ms; c->last_msm = tm; g_last_msm = tm; return ALEO_MI355X_OK; }      // no phase events were recorded
  HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); tm.sort = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); tm.accum = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); tm.reduce = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[5])); tm.accum_kernel = ms;
  tm.host = host_ms; tm.total = tm.sort + tm.accum + tm.reduce + tm.host;
  c->last_msm = tm; g_last_msm = tm;
  return ALEO_MI355X_OK;
}

// Table path: the reduction msm_reduce_queue queued arrives; hook, Horner, aside buckets, normalisation, phase times.
int32_t msm_collect(Ctx* c, uint64_t* out_jac18, Front& f, hipStream_t s, bool fire_tail, TailWait wait) {
  using namespace host;
  const MsmPlan& P = f.P; const SliceMeta& sm = f.sm; const uint32_t K = f.K, lgN = f.lgN, out_pts = f.out_pts; const bool prog = f.prog, aside = f.aside;
  const uint32_t* h_aside = (const uint32_t*)((char*)c->h_pinned + 64 + (size_t)f.nseg * 224);
  const char* h_win = (const char*)c->h_pinned + 64;
  if (fire_tail && c->tail_hook) {
    // the caller's next kernels go behind the fold; the host waits for the fold only (its result sits in pinned memory) and does the tail below while they run
    std::function<int32_t()> hook = std::move(c->tail_hook); c->tail_hook = nullptr;
    HT("msm: reduction queued");
    const int32_t hrc = hook();
    HT("msm: hook queued");
    HIPCHK(hipEventSynchronize(c->ev[3]));
    if (hrc) { (void)hipStreamSynchronize(s); return hrc; }
  } else if (wait == TailWait::event) HIPCHK(hipEventSynchronize(c->ev[3]));
  else HIPCHK(hipStreamSynchronize(s));
  if (aside) HIPCHK(hipEventSynchronize(c->ev[4]));
  HIPCHK(hipGetLastError());
  HT("msm: result arrived");
  const auto t_host0 = std::chrono::steady_clock::now();
  HXYZZ totals[MAX_SETS];
  // Edwards tier: a Z3 == 0 anywhere in the chain (the words k_prog_final's blocks and the side stream left) or in a point the tail reads -> rerun without tables
  std::atomic<bool> te_bad{false};
  if (f.te) {
    const uint32_t* fl = (const uint32_t*)(h_win + (size_t)f.nseg * 224 + ASIDE_MAX * 228 + 64);
    bool any = aside && h_aside[(size_t)sm.n_super * 57];
    for (uint32_t i = 0; i < K * out_pts; ++i) any = any || fl[i];
    te_bad.store(any);
  }
  auto point = [&](const char* p) { if (!f.te) return lazy_point28(p); bool z = false; const HXYZZ r = te_point28(p, &z); if (z) te_bad.store(true); return r; };
  // one Horner chain per result (~15 us): from 3 results on they are spread over the library's parked helper threads (a lockstep round has 8 x k of them)
  auto horner = [&](size_t q) {
    const char* hw = h_win + q * out_pts * PB28;
    const uint32_t na = prog ? 1u : 4u;                  // points that hold sum_j acc_j: one (k_prog_final) or the four segment sums of the masked form
    HXYZZ total = HXYZZ::infinity();
    for (int l = (int)lgN - 1; l >= 0; --l) { total = hdouble(total); total = hadd(total, point(hw + (size_t)(na + l) * PB28)); }
    for (uint32_t sft = P.S; sft > 1; sft >>= 1) total = hdouble(total);
    for (uint32_t r = 0; r < na; ++r) total = hadd(total, point(hw + (size_t)r * PB28));
    totals[q] = total;
  };
  constexpr uint32_t TAIL_POOL = 3;                      // results from which the pool is used (2^15 proof: 5.68 / 5.65 / 5.74 ms with 8 / 3 / 2, profiles/r05_tailpool_min_ab.txt)
  if (K >= TAIL_POOL) host_parallel_for(K, horner); else for (uint32_t q = 0; q < K; ++q) horner(q);
  for (uint32_t h = 0; aside && h < sm.n_super; ++h) {             // (b + 1) * (slices 1.. of super-heavy bucket b), by double-and-add
    const uint32_t* rec = h_aside + (size_t)h * 57; const uint32_t g = rec[56], q = g / P.B, wgt = g % P.B + 1;
    if (q >= K) { g_last_error = "msm: internal: super-heavy bucket outside the sets"; return ALEO_MI355X_ERR_HIP; }
    const HXYZZ T = point((const char*)rec); HXYZZ acc = HXYZZ::infinity();
    for (int bit = 31 - __builtin_clz(wgt); bit >= 0; --bit) { acc = hdouble(acc); if ((wgt >> bit) & 1u) acc = hadd(acc, T); }
    totals[q] = hadd(totals[q], acc);
  }
  HT("msm: horner done");
  if (te_bad.load()) { (void)phase_times(c, f, t_host0); return MSM_RERUN_WITHOUT_TABLES; }
  hstore_jacobian_normalized_batch(out_jac18, totals, K);          // one shared inversion for the K results
  HT("msm: normalised");
  return phase_times(c, f, t_host0);
}

// G1 on the plain back end (msm_reduce.h): 32-bit XYZZ partial sums, a lane per chunk
struct G1Plain {
  using PT = Pt32; using HF = host::HFq; static constexpr bool TIMED = true;
  static host::HXYZZ read(const char* p) { return host::lazy_point(p); }
  static void launch_chunks(Ctx* c, const Front& f, hipStream_t s, char* V, char*) {
    hipLaunchKernelGGL(k_bucket_chunks_plain, dim3((f.nchunks + 255) / 256), dim3(256), 0, s, c->partial.as<char>(), f.sp.hist, f.sp.scan_local, f.sp.scan_blk, f.P.B, f.P.S, f.nchunks, V);
  }
};

int32_t msm_back(Ctx* c, uint64_t* out_jac18, Front& f, hipStream_t s, bool fire_tail, const FrontChain& older) {
  if (!f.masked) return msm_back_plain<G1Plain>(c, out_jac18, f, s);
  const int32_t rc = msm_reduce_queue(c, f, s, older); return rc ? rc : msm_collect(c, out_jac18, f, s, fire_tail, TailWait::stream);
}

// ---- self-test of the 28-bit-limb mixed addition against the 32-bit formulas (test hook; tools/ubench/madd28_check.hip) ----
__device__ __forceinline__ uint32_t st_rng(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
__device__ __forceinline__ Fq st_rnd_fq(uint64_t& s) { Fq r; for (int i = 0; i < 12; ++i) r.v[i] = st_rng(s); r.v[11] &= 0x00ffffffu; return Fq::reduce(r); }
__device__ __forceinline__ bool st_same(const Fq& a, const Fq& b) { Fq x = Fq::reduce(a), y = Fq::reduce(b); uint32_t d = 0; for (int i = 0; i < 12; ++i) d |= x.v[i] ^ y.v[i]; return d == 0; }
__global__ void __launch_bounds__(256) k_selftest_madd28(uint32_t* bad, uint32_t steps, uint64_t seed) {
  uint64_t s = seed * (blockIdx.x * 256 + threadIdx.x + 1);
  Fq z = st_rnd_fq(s);
  if (!st_same(f28_to_fq(f28_from_fq(z)), z)) { atomicAdd(bad, 1u); return; }                 // representation round trip
  XYZZ a; a.X = st_rnd_fq(s); a.Y = st_rnd_fq(s); a.ZZ = Fq::one(); a.ZZZ = Fq::one();
  XYZZ28 b; b.X = f28_from_fq(a.X); b.Y = f28_from_fq(a.Y); b.ZZ = f28_const(ONE28); b.ZZZ = f28_const(ONE28);
  for (uint32_t it = 0; it < steps; ++it) {
    Fq x = st_rnd_fq(s), y = st_rnd_fq(s);
    F28 x28 = f28_from_fq(x), y28 = f28_from_fq(y);
    if (st_rng(s) & 1) { y = fq_neg_canonical(y); y28 = f28_sub<2, 1>(f28_const(Limbs14{}), y28); }
    if (it == steps / 2) { x = Fq::reduce(a.X); x28 = f28_from_fq(x); }                       // same x as acc (ZZ == 1 only at it == 0, so usually a plain point)
    const bool ok32 = xyzz_madd_fast(a, x, y), ok28 = xyzz28_madd_fast(b, x28, y28);
    if (ok32 != ok28) { atomicAdd(bad, 1u); return; }
    if (!ok32) break;
    if (!st_same(f28_to_fq(b.X), a.X) || !st_same(f28_to_fq(b.Y), a.Y) || !st_same(f28_to_fq(b.ZZ), a.ZZ) || !st_same(f28_to_fq(b.ZZZ), a.ZZZ)) { atomicAdd(bad, 1u); return; }
  }
  XYZZ c; c.X = st_rnd_fq(s); c.Y = st_rnd_fq(s); c.ZZ = Fq::one(); c.ZZZ = Fq::one();        // P == acc must be refused by both
  XYZZ28 d; d.X = f28_from_fq(c.X); d.Y = f28_from_fq(c.Y); d.ZZ = f28_const(ONE28); d.ZZZ = f28_const(ONE28);
  if (xyzz_madd_fast(c, c.X, c.Y) || xyzz28_madd_fast(d, d.X, d.Y)) atomicAdd(bad, 1u);
}
int32_t selftest_madd28(Ctx* c, uint32_t lanes, uint32_t steps, uint64_t seed, uint32_t* failures) {
  int32_t rc; if ((rc = c->scalars_stage.reserve(64))) return rc;
  uint32_t* d = c->scalars_stage.as<uint32_t>();
  HIPCHK(hipMemsetAsync(d, 0, 4, c->stream));
  hipLaunchKernelGGL(k_selftest_madd28, dim3((lanes + 255) / 256), dim3(256), 0, c->stream, d, steps, seed | 1ull);
  HIPCHK(hipMemcpyAsync(failures, d, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

// The lane-quad addition against the lane-pair one (which the MSM parity tests pin): same values mod q in all four coordinates, same
// infinity flag, over random operands and the special cases (either operand the identity, equal points, opposite points).
__global__ void __launch_bounds__(256) k_selftest_addquad(char* buf, uint32_t ops, uint64_t seed, uint32_t* bad) {
  const uint32_t op = (blockIdx.x * 256 + threadIdx.x) >> 2, q = threadIdx.x & 3u;
  if (op >= ops) return;
  char* A = buf + (size_t)op * 4 * PB28; char* B = A + PB28; char* O4 = B + PB28; char* O2 = O4 + PB28;
  if (q == 0) {
    uint64_t s = seed * (op + 1);
    XYZZ28 a, b;
    a.X = f28_from_fq(st_rnd_fq(s)); a.Y = f28_from_fq(st_rnd_fq(s)); a.ZZ = f28_from_fq(st_rnd_fq(s)); a.ZZZ = f28_from_fq(st_rnd_fq(s));
    b.X = f28_from_fq(st_rnd_fq(s)); b.Y = f28_from_fq(st_rnd_fq(s)); b.ZZ = f28_from_fq(st_rnd_fq(s)); b.ZZZ = f28_from_fq(st_rnd_fq(s));
    const uint32_t kind = op % 16;
    if (kind == 11) { a.ZZ = f28_const(Limbs14{}); }                                          // A the identity
    if (kind == 12) { b.ZZ = f28_const(Limbs14{}); }                                          // B the identity
    if (kind == 13) { a.ZZ = f28_const(Limbs14{}); b.ZZ = a.ZZ; }
    if (kind == 14) b = a;                                                                    // equal: doubling
    if (kind == 15) { b = a; b.Y = f28_normalise(f28_sub<2, 1>(f28_const(Limbs14{}), a.Y)); }   // opposite: the identity
    store_xyzz28(A, a); store_xyzz28(B, b);
  }
  pair_fence(); __syncthreads();
  xyzz28_add_quad(A, B, O4);
  if (q < 2) xyzz28_add_pair(A, B, O2);
  pair_fence(); __syncthreads();
  if (q == 0) {
    const bool i4 = f28_is_zero_raw(load_f28(O4 + 112)), i2 = f28_is_zero_raw(load_f28(O2 + 112));
    bool ok = i4 == i2;
    if (ok && !i4) for (int k = 0; k < 4; ++k) ok = ok && st_same(f28_to_fq(load_f28(O4 + 56 * k)), f28_to_fq(load_f28(O2 + 56 * k)));
    if (!ok) atomicAdd(bad, 1u);
  }
}
int32_t selftest_addquad(Ctx* c, uint32_t ops, uint64_t seed, uint32_t* failures) {
  ops = (ops + 63u) & ~63u;                                  // whole blocks: the kernel synchronises its threads
  int32_t rc; if ((rc = c->scalars_stage.reserve((size_t)ops * 4 * PB28 + 64))) return rc;
  char* buf = c->scalars_stage.as<char>() + 64; uint32_t* d = c->scalars_stage.as<uint32_t>();
  HIPCHK(hipMemsetAsync(d, 0, 4, c->stream));
  hipLaunchKernelGGL(k_selftest_addquad, dim3(ops / 64), dim3(256), 0, c->stream, buf, ops, seed | 1ull, d);
  HIPCHK(hipMemcpyAsync(failures, d, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
