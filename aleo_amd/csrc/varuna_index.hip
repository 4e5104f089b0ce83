// varuna_index.hip — key synthesis: the index of one circuit, built once per proving key (aleo_mi355x_varuna_index_build) and kept on the device —
// the matrices laid out on H, their transpose, the arithmetisation over the non-zero domains with its transforms, and the twelve index commitments.
// [UPSTREAM-RECALL: varuna/ahp/indexer — AHPForR1CS::index: matrix arithmetisation over the non-zero domain, index commitments; reached from
// Process::synthesize_key, the reference's wasm/src/programs/manager/mod.rs:164-177, rust/src/program/deploy.rs:142,151.]
#include "varuna_host.h"

namespace aleo_mi355x {

struct VarunaIndexOwner {
  aleo_mi355x_varuna_index view{};
  std::vector<uint32_t> positions; std::vector<uint8_t> vk, vk_aff;
  std::vector<void*> dev;                                  // every device allocation the index keeps
  std::vector<void*> tmp;                                  // scratch of the build (raw columns, C's forward arrays, cursors): freed when the build's stream has drained
  std::shared_ptr<PinnedOwner> key;                        // the committer key stays pinned while the index lives
  ~VarunaIndexOwner() { free_tmp(); for (void* p : dev) if (p) (void)hipFree(p); }
  void free_tmp() { for (void* p : tmp) if (p) (void)hipFree(p); tmp.clear(); }
  int32_t alloc(void** out, size_t bytes, bool scratch = false) { void* p = nullptr; HIPCHK(hipMalloc(&p, bytes ? bytes : 32)); (scratch ? tmp : dev).push_back(p); *out = p; return ALEO_MI355X_OK; }
};
void varuna_index_delete(VarunaIndexOwner* o) { delete o; }
const aleo_mi355x_varuna_index* varuna_index_view(const VarunaIndexOwner* o) { return &o->view; }
const std::vector<uint8_t>& varuna_index_vk(const VarunaIndexOwner* o) { return o->vk; }

static uint64_t pow2_at_least(uint64_t v, uint64_t lo) { uint64_t p = lo; while (p < v) p <<= 1; return p; }

// One synthesis in flight: the sizes, and the device arrays one phase hands to the next.  The phases are what ALEO_MI355X_INDEX_TIMING times (mark).
struct IndexBuild {
  Ctx* c; const PinnedBases& pb; hipStream_t s; VarunaIndexOwner* o; const aleo_mi355x_r1cs_matrix* abc;
  uint64_t n_constraints, n_vars, n_x, n_h, nnz[3], nnz_sum, nk[3], ko[3], k_sum;      // one non-zero domain per matrix; ko: elements of the earlier matrices
  void *kid, *kv, *he, *kpo;                               // over K: (row, column) indices | values (scratch) | the 12 polynomials;  he: the elements of H
  HFr r2; bool tim; double t_prev;
  void mark(const char* what) {                            // ALEO_MI355X_INDEX_TIMING: the stream drained, the phase's time to stderr
    if (tim) { (void)hipStreamSynchronize(s); const double t = now_ms(); fprintf(stderr, "index_build %-28s %8.2f ms\n", what, t - t_prev); t_prev = t; }
  }
  int32_t up(void** dst, const void* src, size_t bytes, bool scratch = false) {
    RC(o->alloc(dst, bytes, scratch)); if (bytes) HIPCHK(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s)); return ALEO_MI355X_OK;
  }
  int32_t to_mont(void* p, size_t n) { return fr_lin(c, p, n, nullptr, r2.l, p, nullptr, nullptr, s); }
  int32_t index_arithmetic(); int32_t vx_and_h(); int32_t arithmetise(); int32_t commitments();
};

// ---- the integer side of the arithmetisation: CSR rows -> (row, column position) pairs + column counts; inclusive scan; column-major scatter of (row, value) ----
// One lane per CSR row (rows of an R1CS matrix are short; the few long linear combinations cost their lane a loop, not the launch).
__global__ void __launch_bounds__(256) k_index_expand_rows(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const uint32_t* __restrict__ positions, uint32_t rows,
                                                           uint32_t* __restrict__ k_row, uint32_t* __restrict__ k_col, uint32_t* __restrict__ cpos, uint32_t* __restrict__ count_plus1) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  for (uint32_t e = row_ptr[r], end = row_ptr[r + 1]; e < end; ++e) {
    const uint32_t p = positions[col[e]];
    k_row[e] = r; k_col[e] = p; cpos[e] = p; atomicAdd(&count_plus1[p + 1], 1u);
  }
}
// a[i] += a[i - 1] over n entries, one block (n is a domain size: a few passes of 1024 lanes x 8 entries)
__global__ void __launch_bounds__(1024) k_index_scan_inclusive(uint32_t* __restrict__ a, uint32_t n) {
  __shared__ uint32_t wsum[16]; __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x; const int lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 8192) {
    uint32_t v[8], run = 0; const uint32_t i0 = base + tid * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n ? a[i0 + k] : 0u; run += v[k]; v[k] = run; }
    uint32_t inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t off = carry_s; for (int k = 0; k < wv; ++k) off += wsum[k];
    off += inc - run;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (i0 + k < n) a[i0 + k] = off + v[k];
    __syncthreads();
    if (tid == 1023) carry_s = off + run;
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_index_transpose_rows(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ cpos, const uint4* __restrict__ val, uint32_t rows, uint32_t row_base,
                                                              uint32_t* __restrict__ cursor, uint32_t* __restrict__ tcol, uint4* __restrict__ tval) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  for (uint32_t e = row_ptr[r], end = row_ptr[r + 1]; e < end; ++e) {
    const uint32_t at = atomicAdd(&cursor[cpos[e]], 1u);
    tcol[at] = row_base + r; tval[2 * (size_t)at] = val[2 * (size_t)e]; tval[2 * (size_t)at + 1] = val[2 * (size_t)e + 1];
  }
}
static int32_t index_expand_rows(Ctx* c, const uint32_t* d_row_ptr, const uint32_t* d_col, const uint32_t* d_positions, size_t rows, uint32_t* d_k_row, uint32_t* d_k_col, uint32_t* d_cpos, uint32_t* d_count_plus1, hipStream_t s) {
  (void)c; if (!rows) return ALEO_MI355X_OK;
  hipLaunchKernelGGL(k_index_expand_rows, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, s, d_row_ptr, d_col, d_positions, (uint32_t)rows, d_k_row, d_k_col, d_cpos, d_count_plus1);
  HIPCHK(hipGetLastError()); return ALEO_MI355X_OK;
}
static int32_t index_scan_inclusive(Ctx* c, uint32_t* d_a, size_t n, hipStream_t s) {
  (void)c; if (!n) return ALEO_MI355X_OK;
  hipLaunchKernelGGL(k_index_scan_inclusive, dim3(1), dim3(1024), 0, s, d_a, (uint32_t)n);
  HIPCHK(hipGetLastError()); return ALEO_MI355X_OK;
}
static int32_t index_transpose_rows(Ctx* c, const uint32_t* d_row_ptr, const uint32_t* d_cpos, const void* d_val, size_t rows, uint32_t row_base, uint32_t* d_cursor, uint32_t* d_tcol, void* d_tval, hipStream_t s) {
  (void)c; if (!rows) return ALEO_MI355X_OK;
  hipLaunchKernelGGL(k_index_transpose_rows, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, s, d_row_ptr, d_cpos, (const uint4*)d_val, (uint32_t)rows, row_base, d_cursor, d_tcol, (uint4*)d_tval);
  HIPCHK(hipGetLastError()); return ALEO_MI355X_OK;
}

// Index arithmetic on integers, on the device since round 3 (the host loops over the non-zeros were half of a 2^20-constraint key synthesis): per
// matrix the rows expand into (row, column position on H) pairs and count their columns; one scan turns the counts into the transpose's row
// pointers; a second pass drops every entry into its column's range (an atomic cursor per column: the order inside a column is whatever the
// hardware makes it, the products M^T v are exact field sums, so every proof byte is independent of it).
int32_t IndexBuild::index_arithmetic() {
  aleo_mi355x_varuna_index& V = o->view;
  std::vector<uint32_t> rp(n_h + 1);
  void *dpos, *dtp, *dcur, *dtcol, *dtval;
  RC(up(&dpos, o->positions.data(), n_vars * 4)); V.positions_device = dpos;
  RC(o->alloc(&kid, 2 * k_sum * 4)); RC(o->alloc(&kv, k_sum * 32, true)); RC(o->alloc(&dtp, (n_h + 1) * 4)); RC(o->alloc(&dtcol, nnz_sum * 4)); RC(o->alloc(&dtval, nnz_sum * 32));
  HIPCHK(hipMemsetAsync(kid, 0, 2 * k_sum * 4, s)); HIPCHK(hipMemsetAsync(kv, 0, k_sum * 32, s)); HIPCHK(hipMemsetAsync(dtp, 0, (n_h + 1) * 4, s));
  void *drp[3], *dcolraw[3], *dcol[3], *dval[3];
  for (int m = 0; m < 3; ++m) {                            // forward matrices with columns on H, rows padded to |H| (C only feeds the transpose and the arithmetisation)
    for (uint64_t i = 0; i <= n_h; ++i) rp[i] = i <= n_constraints ? abc[m].row_ptr[i] : (uint32_t)nnz[m];
    const bool fwd = m < 2;                                // A and B are kept as forward CSR (z_a, z_b); C's arrays, the raw columns and the cursors are scratch
    RC(up(&drp[m], rp.data(), (n_h + 1) * 4, !fwd)); RC(up(&dcolraw[m], abc[m].col, nnz[m] * 4, true)); RC(up(&dval[m], abc[m].val, nnz[m] * 32, !fwd)); RC(o->alloc(&dcol[m], nnz[m] * 4, !fwd));
    HIPCHK(hipStreamSynchronize(s));                       // rp is reused by the next matrix
    RC(index_expand_rows(c, (const uint32_t*)drp[m], (const uint32_t*)dcolraw[m], (const uint32_t*)dpos, n_constraints, (uint32_t*)kid + 2 * ko[m], (uint32_t*)kid + 2 * ko[m] + nk[m],
                         (uint32_t*)dcol[m], (uint32_t*)dtp, s));
    if (nnz[m]) HIPCHK(hipMemcpyAsync((char*)kv + ko[m] * 32, dval[m], nnz[m] * 32, hipMemcpyDeviceToDevice, s));      // canonical values: converted with the whole array below
  }
  RC(index_scan_inclusive(c, (uint32_t*)dtp, n_h + 1, s));
  RC(o->alloc(&dcur, (n_h + 1) * 4, true)); HIPCHK(hipMemcpyAsync(dcur, dtp, (n_h + 1) * 4, hipMemcpyDeviceToDevice, s));
  for (int m = 0; m < 3; ++m) RC(index_transpose_rows(c, (const uint32_t*)drp[m], (const uint32_t*)dcol[m], dval[m], n_constraints, (uint32_t)(m * n_h), (uint32_t*)dcur, (uint32_t*)dtcol, dtval, s));
  for (int m = 0; m < 2; ++m) RC(to_mont(dval[m], nnz[m]));
  V.a_row_ptr = drp[0]; V.a_col = dcol[0]; V.a_val = dval[0]; V.b_row_ptr = drp[1]; V.b_col = dcol[1]; V.b_val = dval[1];
  RC(to_mont(dtval, nnz_sum)); V.t_row_ptr = dtp; V.t_col = dtcol; V.t_val = dtval;
  return ALEO_MI355X_OK;
}

// 1 / v_X on H \ X (v_X(w^p) = wx^p − 1, wx = w^|X|; zeros stay zero through the batch inversion), elements of H
int32_t IndexBuild::vx_and_h() {
  void* vx; const HFr one = HFr::one();
  RC(o->alloc(&vx, n_h * 32)); RC(o->alloc(&he, n_h * 32, true));
  const HFr gen_h = domain_gen(n_h), wx = HFr::pow_u64(gen_h, n_x), neg1 = HFr::neg(one);
  RC(fr_powers(c, vx, n_h, one.l, wx.l, s)); RC(fr_lin(c, vx, n_h, neg1.l, one.l, vx, nullptr, nullptr, s)); RC(fr_batch_inverse(c, vx, n_h, s));
  RC(fr_powers(c, he, n_h, one.l, gen_h.l, s));
  o->view.vx_inv = vx;
  return ALEO_MI355X_OK;
}

// arithmetisation over K: row, col, val = M[r,c] col / |H|, row_col — padding: row = col = 1 (position 0), val = 0
int32_t IndexBuild::arithmetise() {
  void *kev, *k2;
  RC(o->alloc(&kev, 4 * k_sum * 32)); RC(o->alloc(&kpo, 4 * k_sum * 32)); RC(o->alloc(&k2, 8 * k_sum * 32));
  RC(to_mont(kv, k_sum));
  mark("alloc + upload K arrays");
  const HFr nh_inv = inv_pow2(lg2(n_h));
  HIPCHK(hipMemsetAsync(k2, 0, 8 * k_sum * 32, s));
  for (int m = 0; m < 3; ++m) {
    const uint64_t n = nk[m]; const uint32_t lg = lg2(n);
    char* e = (char*)kev + 4 * ko[m] * 32; const uint32_t* ri = (const uint32_t*)kid + 2 * ko[m]; const uint32_t* ci = ri + n;
    RC(fr_gather_mul(c, e, n, nullptr, he, ri, nullptr, nullptr, s));
    RC(fr_gather_mul(c, e + n * 32, n, nullptr, he, ci, nullptr, nullptr, s));
    RC(fr_vec_op(c, e + 2 * n * 32, (char*)kv + ko[m] * 32, e + n * 32, n, 0, s));
    RC(fr_lin(c, e + 2 * n * 32, n, nullptr, nh_inv.l, e + 2 * n * 32, nullptr, nullptr, s));
    RC(fr_vec_op(c, e + 3 * n * 32, e, e + n * 32, n, 0, s));
    char* po = (char*)kpo + 4 * ko[m] * 32; char* e2 = (char*)k2 + 8 * ko[m] * 32;
    HIPCHK(hipMemcpyAsync(po, e, 4 * n * 32, hipMemcpyDeviceToDevice, s));
    RC(p_ntt(c, pb, po, lg, 4, 1, 0, s));
    for (int j = 0; j < 4; ++j) HIPCHK(hipMemcpyAsync(e2 + (size_t)j * 2 * n * 32, po + (size_t)j * n * 32, n * 32, hipMemcpyDeviceToDevice, s));
    RC(p_ntt(c, pb, e2, lg + 1, 4, 0, 0, s));
  }
  aleo_mi355x_varuna_index& V = o->view;
  V.k_evals = kev; V.k_idx = kid; V.k_polys = kpo; V.k2_evals = k2;
  return ALEO_MI355X_OK;
}

// index commitments -> what the transcript absorbs first
int32_t IndexBuild::commitments() {
  o->vk_aff.assign(12 * 104, 0); uint8_t* aff = o->vk_aff.data();
  std::vector<MsmSeg> sg;
  for (int q = 0; q < 12; ++q) { const int m = q / 4, j = q % 4; sg.push_back(seg((char*)kpo + (4 * ko[m] + (size_t)j * nk[m]) * 32, nk[m], 0, q)); }
  RC(commit(c, pb, sg, 12, aff, s));
  HIPCHK(hipStreamSynchronize(s));
  o->free_tmp();                                           // nothing queued reads the scratch any more
  o->vk.resize(12 * 48 + 40);
  RC(aleo_mi355x_g1_compress(o->vk.data(), aff, 12));
  const uint64_t dims[5] = {n_h, nk[0], nk[1], nk[2], n_x}; std::memcpy(&o->vk[12 * 48], dims, 40);
  return ALEO_MI355X_OK;
}

int32_t varuna_index_build(Ctx* c, const PinnedBases& pb, std::shared_ptr<PinnedOwner> key, uint64_t key_handle, uint64_t max_degree, uint64_t gamma_offset,
                           uint64_t lagrange_offset, const aleo_mi355x_r1cs_matrix* abc, size_t n_constraints, size_t n_public, size_t n_private, uint32_t domain_flags, VarunaIndexOwner** out) {
  std::unique_ptr<VarunaIndexOwner> o(new VarunaIndexOwner()); o->key = std::move(key);
  IndexBuild b{c, pb, c->stream, o.get(), abc}; b.n_constraints = n_constraints;
  uint64_t *nnz = b.nnz, *nk = b.nk, *ko = b.ko, nnz_sum = 0;
  if (!n_constraints || !n_public || n_constraints >= (1ull << 28)) { g_last_error = "varuna_index: bad sizes"; return ALEO_MI355X_ERR_BAD_ARG; }
  const uint64_t n_vars = n_public + n_private, n_x = pow2_at_least(n_public, 1);
  uint64_t n_h = pow2_at_least(n_constraints, 2); n_h = pow2_at_least(n_x + n_private, n_h); n_h = pow2_at_least(2 * n_x, n_h);
  uint64_t max_row[3] = {1, 1, 1};                     // the longest row of A, B and of the stacked transpose (hints for the sparse products; >= 1 = known)
  std::vector<uint32_t> col_count(n_vars, 0);
  for (int m = 0; m < 3; ++m) {
    if (!abc[m].row_ptr || abc[m].row_ptr[0] != 0) { g_last_error = "varuna_index: row_ptr must start at 0"; return ALEO_MI355X_ERR_BAD_ARG; }
    nnz[m] = abc[m].row_ptr[n_constraints]; nnz_sum += nnz[m];
    if (nnz[m] && (!abc[m].col || !abc[m].val)) { g_last_error = "varuna_index: null matrix arrays"; return ALEO_MI355X_ERR_BAD_ARG; }
    for (uint64_t e = 0; e < nnz[m]; ++e) { if (abc[m].col[e] >= n_vars) { g_last_error = "varuna_index: column outside the variables"; return ALEO_MI355X_ERR_BAD_ARG; } ++col_count[abc[m].col[e]]; }
    for (size_t r = 0; r < n_constraints; ++r) {
      if (abc[m].row_ptr[r + 1] < abc[m].row_ptr[r]) { g_last_error = "varuna_index: row_ptr not monotone"; return ALEO_MI355X_ERR_BAD_ARG; }
      const uint64_t len = abc[m].row_ptr[r + 1] - abc[m].row_ptr[r]; if (m < 2 && len > max_row[m]) max_row[m] = len;
    }
  }
  for (uint32_t cnt : col_count) if (cnt > max_row[2]) max_row[2] = cnt;      // a row of the stacked transpose = every use of one variable in A, B and C
  uint64_t k_sum = 0, n_k = 0;
  for (int m = 0; m < 3; ++m) { nk[m] = pow2_at_least(nnz[m], 2); n_k = nk[m] > n_k ? nk[m] : n_k; }
  if (domain_flags == 2 || (domain_flags == 0 && n_k < (1ull << 18))) nk[0] = nk[1] = nk[2] = n_k;      // shared: latency-bound sizes (header)
  for (int m = 0; m < 3; ++m) { ko[m] = k_sum; k_sum += nk[m]; }
  if (3 * n_h > max_degree + 1 || n_k > max_degree + 1 || max_degree + 1 > pb.n || gamma_offset + 3 > pb.n) { g_last_error = "varuna_index: committer key too small for this circuit"; return ALEO_MI355X_ERR_BAD_ARG; }
  // variable -> position on H: public i -> i |H|/|X|, the j-th private one -> the j-th element of H \ X
  const uint64_t ratio = n_h / n_x;
  o->positions.resize(n_vars);
  for (uint64_t v = 0; v < n_vars; ++v) { if (v < n_public) o->positions[v] = (uint32_t)(v * ratio); else { const uint64_t j = v - n_public; o->positions[v] = (uint32_t)(j + j / (ratio - 1) + 1); } }
  std::memcpy(b.r2.l, host::HParams<4>::R2, 32);
  aleo_mi355x_varuna_index& V = o->view;
  for (int m = 0; m < 3; ++m) V.max_row[m] = max_row[m];
  V.n_h = n_h; V.n_k_a = nk[0]; V.n_k_b = nk[1]; V.n_k_c = nk[2]; V.n_x = n_x; V.n_public = n_public; V.n_vars = n_vars; V.committer_key = key_handle; V.max_degree = max_degree; V.gamma_offset = gamma_offset; V.lagrange_offset = lagrange_offset;
  if (lagrange_offset && lagrange_offset + n_h + 1 > pb.n) { g_last_error = "varuna_index: the Lagrange powers do not fit the committer key"; return ALEO_MI355X_ERR_BAD_ARG; }
  b.n_vars = n_vars; b.n_x = n_x; b.n_h = n_h; b.nnz_sum = nnz_sum; b.k_sum = k_sum; V.positions = o->positions.data();
  b.tim = std::getenv("ALEO_MI355X_INDEX_TIMING") != nullptr; b.t_prev = now_ms();
  RC(b.index_arithmetic()); b.mark("index arithmetic (device)");
  RC(b.vx_and_h()); b.mark("vx, H elements");
  RC(b.arithmetise()); b.mark("arithmetisation + transforms");
  RC(b.commitments()); b.mark("12 commitments");
  V.vk_bytes = o->vk.data(); V.vk_len = o->vk.size(); V.vk_affine = o->vk_aff.data();
  *out = o.release();
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x
