// sharded.hip — work of libaleo_mi355x.so that spans several devices of one process: base sets cut into shards, the persistent shard workers, the MSM and
// the commitments against a sharded set, the 4-step transform over devices (from a host buffer, and on data resident on one device), and their entry points.
#include "entry.h"
#include "host_field.hpp"
#include <chrono>
#include <cstring>
#include <deque>
#include <thread>

namespace aleo_mi355x {
namespace {
// ---- one MSM over several devices (BASELINE configs[4]) ------------------------------------------------------------------
// One process, G device contexts: the base set is cut into G contiguous shards, shard g pinned on devices[g]; an MSM runs the whole Pippenger
// per shard on its device (one host thread per shard: the runtime's current device is per thread) and the G partial sums — 144 bytes each —
// are added on the host in shard order, so the result's bytes do not depend on which device finished first.  No collective: inside one
// process the "all-gather" of SURVEY.md 8(e) is G stores into one host array.  (Ranks in separate processes exchange the same 144-byte
// partials over RCCL: aleo_amd/dist.py.)  A device may be listed more than once (how the tests rehearse G > 1 on one card).
struct ShardedSet { std::vector<int> devices; std::vector<uint64_t> handles; std::vector<size_t> first, count, ordinal; size_t n = 0; };      // ordinal[g]: shard g is the ordinal[g]-th shard on its device
std::mutex g_sh_mu; std::map<uint64_t, std::shared_ptr<ShardedSet>> g_sh; uint64_t g_sh_next = 1;

std::shared_ptr<ShardedSet> sharded_find(uint64_t h, bool take = false) {      // nullptr (and the error text) for an unknown handle
  std::shared_ptr<ShardedSet> S; std::lock_guard<std::mutex> lk(g_sh_mu);
  (void)handle_get(g_sh, h, "unknown sharded handle", &S, take);
  return S;
}
// Shard work runs on LONG-LIVED worker threads, one per (device, ordinal among the shards a call lists on that device): created on first use, bound to their
// device once, parked on a condition variable between calls.  (Rounds 3-4 started G std::threads per call: every commitment of a proof against a sharded key
// paid G thread creations — on one card 8 shards cost +19 % per 2^20-constraint proof.)  The pool is never destroyed: its threads are detached and sleep until
// the process ends.  Submission is serialised (g_pool_submit_mu) so that every worker's queue holds the calls in ONE global order — two calls whose shard bodies
// meet at barriers cannot interleave into a deadlock.
struct ShardWorker {
  std::mutex mu; std::condition_variable cv; std::deque<std::function<void()>> q; int device = -1; bool started = false;
  void loop() {
    (void)hipSetDevice(device);                              // a failure shows up again in the task (it sets the device itself and reports)
    for (;;) {
      std::function<void()> job;
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !q.empty(); }); job = std::move(q.front()); q.pop_front(); }
      job();
    }
  }
};
std::mutex g_pool_mu, g_pool_submit_mu; std::map<std::pair<int, size_t>, ShardWorker*> g_pool;
ShardWorker* shard_worker(int device, size_t ordinal) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  auto it = g_pool.find({device, ordinal});
  if (it != g_pool.end()) return it->second;
  ShardWorker* w = new ShardWorker(); w->device = device;      // leaked on purpose: lives as long as the process
  std::thread([w] { w->loop(); }).detach();                    // (throws std::system_error if no thread can be started: caught by the entry point's try)
  w->started = true; g_pool[{device, ordinal}] = w; return w;
}
// runs f(g) for every shard on that shard's worker with its device current and waits for all of them; the first failure's code and text come back.
// on_skip(g): called for a shard whose body could not run (its device could not be selected, an exception) — a body that meets the other shards at barriers
// passes one that drops the shard from them.
template <class F> int32_t for_each_shard(const ShardedSet& S, F&& f, std::function<void(size_t)> on_skip = nullptr) {
  const size_t G = S.devices.size();
  std::vector<int32_t> rcs(G, ALEO_MI355X_OK); std::vector<std::string> errs(G);
  std::vector<ShardWorker*> ws(G);
  try { for (size_t g = 0; g < G; ++g) ws[g] = shard_worker(S.devices[g], S.ordinal[g]); }
  catch (...) { g_last_error = "could not start a shard's thread"; return ALEO_MI355X_ERR_HIP; }      // nothing was queued: none runs
  std::mutex done_mu; std::condition_variable done_cv; size_t done = 0;
  {
    std::lock_guard<std::mutex> order(g_pool_submit_mu);
    for (size_t g = 0; g < G; ++g) {
      auto body = [&, g]() {
        bool ran = false;
        try {
          if (hipSetDevice(S.devices[g]) != hipSuccess) { rcs[g] = ALEO_MI355X_ERR_HIP; errs[g] = "hipSetDevice failed"; }
          else { ran = true; rcs[g] = f(g); if (rcs[g]) errs[g] = g_last_error; }
        } catch (...) { rcs[g] = ALEO_MI355X_ERR_HIP; errs[g] = "exception in a shard"; ran = false; }
        if (!ran && on_skip) { try { on_skip(g); } catch (...) {} }
        { std::lock_guard<std::mutex> lk(done_mu); ++done; done_cv.notify_one(); }      // notified under the lock: the waiter cannot return (and destroy the condition variable) before the call is over
      };
      { std::lock_guard<std::mutex> lk(ws[g]->mu); ws[g]->q.emplace_back(std::move(body)); }
      ws[g]->cv.notify_one();
    }
  }
  { std::unique_lock<std::mutex> lk(done_mu); done_cv.wait(lk, [&] { return done == G; }); }
  for (size_t g = 0; g < G; ++g) if (rcs[g]) { g_last_error = "shard " + std::to_string(g) + " (device " + std::to_string(S.devices[g]) + "): " + errs[g]; return rcs[g]; }
  return ALEO_MI355X_OK;
}
int32_t sharded_layout(ShardedSet& S, size_t n, const int32_t* devices, size_t n_devices) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { g_last_error = "no HIP device visible"; return ALEO_MI355X_ERR_NO_DEVICE; }
  if (n_devices < 1 || n_devices > 64) return bad_arg("sharded: 1..64 shards");
  S.n = n;
  for (size_t g = 0; g < n_devices; ++g) {
    const int dev = devices ? devices[g] : (int)(g % (size_t)count);
    if (dev < 0 || dev >= count) return bad_arg("sharded: device index out of range");
    S.devices.push_back(dev);
    const size_t lo = n * g / n_devices, hi = n * (g + 1) / n_devices;      // the split of aleo_amd/dist.py shard_range
    S.first.push_back(lo); S.count.push_back(hi - lo);
  }
  S.handles.assign(n_devices, 0); S.ordinal.assign(n_devices, 0);
  for (size_t g = 0; g < n_devices; ++g) for (size_t e = 0; e < g; ++e) S.ordinal[g] += S.devices[e] == S.devices[g];
  return ALEO_MI355X_OK;
}
uint64_t sharded_register(std::shared_ptr<ShardedSet> S) { std::lock_guard<std::mutex> lk(g_sh_mu); const uint64_t h = g_sh_next++; g_sh[h] = std::move(S); return h; }
void sharded_release(const ShardedSet& S) {
  (void)for_each_shard(S, [&](size_t g) -> int32_t { return S.handles[g] ? aleo_mi355x_bases_unpin(S.handles[g]) : ALEO_MI355X_OK; });
}
// A new sharded set of n points: pin_shard(first, count, &handle) puts the shard [first, first + count) on the calling thread's device; its table when asked for.
template <class Pin> int32_t make_sharded(size_t n, const int32_t* devices, size_t n_devices, int32_t precompute, uint64_t* handle, Pin&& pin_shard) {
  auto S = std::make_shared<ShardedSet>();
  int32_t rc = sharded_layout(*S, n, devices, n_devices); if (rc) return rc;
  rc = for_each_shard(*S, [&](size_t g) -> int32_t {
    int32_t r = pin_shard(S->first[g], S->count[g], &S->handles[g]);
    if (!r && precompute && S->count[g] >= 1024) r = aleo_mi355x_bases_precompute(S->handles[g]);
    return r;
  });
  if (rc) { const std::string keep = g_last_error; sharded_release(*S); g_last_error = keep; return rc; }
  *handle = sharded_register(std::move(S));
  return ALEO_MI355X_OK;
}

// A context of the calling thread's device for shard work on behalf of a call that holds `caller` (nullptr: it holds none): another one (acquire_other; waited for
// unless this is the caller's own device), else a turn on `caller` itself — every other context of its device may be held by workers of the very call this work
// belongs to (a lockstep proof), and `caller` is idle while its owner waits for the shards.
struct Borrowed { Device* d = nullptr; Ctx* c = nullptr; std::unique_lock<std::mutex> lk, turn; };
int32_t borrow_ctx(Ctx* caller, std::mutex& lend_mu, Borrowed& b) {
  int32_t r = get_device(&b.d); if (r) return r;
  if ((r = acquire_other(b.d, caller, &b.c, b.lk, !caller || b.d->device != caller->device))) return r;
  if (!b.c) { b.turn = std::unique_lock<std::mutex>(lend_mu); b.c = caller; }      // (only on the caller's device)
  return ALEO_MI355X_OK;
}
// [*lo, *hi): the bases of segment m that lie in shard g; false when there are none
bool seg_in_shard(const MsmSeg& m, const ShardedSet& S, size_t g, size_t* lo, size_t* hi) {
  *lo = m.off > S.first[g] ? m.off : S.first[g]; *hi = m.off + m.len < S.first[g] + S.count[g] ? m.off + m.len : S.first[g] + S.count[g];
  return *hi > *lo;
}

// ---- one transform over several devices of this process: the 4-step schedule of aleo_amd/dist.py ShardedDomain behind the C ABI --------------------
// n = R * C (R = 2^floor(lg n / 2)), G devices, natural order in and out of ONE host buffer:
//   device g uploads the coefficient COLUMNS c in [g C / G, (g + 1) C / G) of the R x C matrix x[r C + c] (a strided copy: its 1/G of the PCIe traffic),
//   transposes them, runs its C / G column transforms of length R, multiplies by w_n^(c k_r) and cuts the result into G blocks by k_r range;
//   block h goes to device h (one peer copy per pair: the all-to-all of SURVEY.md 8(e), G - 1 peers per device, one per xGMI link);
//   device h transposes what it received into rows k_r, runs its R / G row transforms of length C, transposes once more and stores X[k_c R + k_r]
//   straight into the host buffer (strided copy).  Coset shift and n^-1 as in the single-device transform (fr_grid_scale mode 1 / the batched inverse).
// Threads: one per shard and phase (the runtime's current device is per thread); phases are separated by joins, so no peer copy starts before
// every column transform has finished.  A device may be listed more than once (the tests: one card).
// The resident form (ntt_sharded_device) shares this schedule: the two differ only in how shard g's [Cg][R] column slab arrives in its buffer b (`load`) and how
// its [Rg][C] row block leaves buffer a (`store`; b is free by then).
struct NttShard { int dev = 0; hipStream_t st = nullptr; void *a = nullptr, *b = nullptr; };      // two buffers of n / G elements each, ping-pong (owned by the device's ShardWs)
std::mutex g_ntt_sh_mu;                                     // one sharded transform at a time: it occupies every listed device anyway
int32_t peer_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t s) {
  if (dst_dev == src_dev) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); }
  else { HIPCHK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s)); }
  return ALEO_MI355X_OK;
}
// the k-th shard workspace of the calling thread's current device (stream created once, buffers grow-only)
int32_t shard_ws(size_t ordinal, size_t bytes, NttShard* out) {
  Device* d = nullptr; { const int32_t rc = get_device(&d); if (rc) return rc; }
  ShardWs* w = nullptr;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    while (d->shard_ws.size() <= ordinal) d->shard_ws.emplace_back(new ShardWs());
    w = d->shard_ws[ordinal].get();
  }
  if (!w->st) HIPCHK(hipStreamCreateWithFlags(&w->st, hipStreamNonBlocking));
  { int32_t rc; if ((rc = w->a.reserve(bytes)) || (rc = w->b.reserve(bytes))) return rc; }
  out->dev = d->device; out->st = w->st; out->a = w->a.p; out->b = w->b.p;
  return ALEO_MI355X_OK;
}

using ShardIo = std::function<int32_t(size_t g, const NttShard& d, Ctx* cc)>;      // queues its copies and kernels on d.st; cc: a context for the kernels' scratch
struct ShardPlan {
  ShardedSet S; uint32_t lg_n = 0, lg_r = 0, lg_c = 0; size_t G = 0, R = 0, C = 0, Rg = 0, Cg = 0, per = 0;      // S: only its devices and ordinals; per = elements per shard (= R * Cg = Rg * C)
  std::unique_lock<std::mutex> one;                         // g_ntt_sh_mu, held for as long as the plan lives
};
// Checks, the R x C / G layout, the lock, and every listed device initialised (and selectable) before any shard thread starts: a thread must not drop out before
// the barriers.  Not part of sharded_run: the resident form's home-side steps come between the two.
int32_t sharded_plan(const std::string& who, const void* data, uint32_t lg_n, int32_t direction, int32_t type, const int32_t* devices, size_t n_devices, ShardPlan& P) {
  if (!data || lg_n < 2 || lg_n > 30 || direction < 0 || direction > 1 || type < 0 || type > 1) { g_last_error = who + ": bad argument"; return ALEO_MI355X_ERR_BAD_ARG; }
  if (n_devices < 1 || n_devices > 64 || (n_devices & (n_devices - 1))) { g_last_error = who + ": the number of shards must be a power of two (1..64)"; return ALEO_MI355X_ERR_BAD_ARG; }
  uint32_t lg_g = 0; while ((1u << lg_g) < n_devices) ++lg_g;
  P.lg_n = lg_n; P.lg_r = lg_n / 2; P.lg_c = lg_n - P.lg_r;
  if (P.lg_r < lg_g) { g_last_error = who + ": domain too small for this many shards"; return ALEO_MI355X_ERR_BAD_ARG; }
  int32_t rc = sharded_layout(P.S, (size_t)1 << lg_n, devices, n_devices); if (rc) return rc;
  P.G = n_devices; P.R = (size_t)1 << P.lg_r; P.C = (size_t)1 << P.lg_c; P.Rg = P.R / P.G; P.Cg = P.C / P.G; P.per = P.R * P.Cg;
  P.one = std::unique_lock<std::mutex>(g_ntt_sh_mu);
  int cur = 0; if (hipGetDevice(&cur) != hipSuccess) cur = 0;
  for (size_t g = 0; g < P.G && !rc; ++g) { Device* dd = nullptr; rc = init_device(P.S.devices[g], &dd); }
  (void)hipSetDevice(cur);
  return rc;
}
// One worker thread per shard for the whole call (the runtime's current device is per thread; the workers are the persistent ones of for_each_shard);
// the three phases are separated by barriers, so no peer copy starts before every column transform has finished and no buffer is overwritten
// before its reader is done.  A shard that fails keeps meeting the barriers (the others must not hang) and the first failure is returned; a shard
// that cannot even start, or leaves by an exception, is dropped from the barriers (Barrier::drop).
// The kernels of ONE phase run on a borrowed context (their scratch), given back before the barrier.  Every phase ends with its stream drained.
int32_t sharded_run(const ShardPlan& P, Ctx* caller, int32_t direction, const ShardIo& load, const ShardIo& store) {
  const size_t G = P.G, R = P.R, C = P.C, Rg = P.Rg, Cg = P.Cg;
  std::vector<NttShard> sh(G);
  Barrier bar(G); std::atomic<int> failed{0}; std::mutex lend_mu;
  return for_each_shard(P.S, [&](size_t g) -> int32_t {
    NttShard& d = sh[g]; int32_t r = ALEO_MI355X_OK; std::string err;
    auto phase = [&](const std::function<int32_t()>& f) { if (!r && !failed.load()) { r = f(); if (r) { err = g_last_error; failed.store(1); } } bar.wait(); };
    auto with_ctx = [&](const std::function<int32_t(Ctx*)>& f) -> int32_t { Borrowed b; if (int32_t q = borrow_ctx(caller, lend_mu, b)) return q; return f(b.c); };
    // phase 1: columns in, column transforms, twiddle, blocks by destination
    phase([&]() -> int32_t { return with_ctx([&](Ctx* cc) -> int32_t {
      int32_t q;
      if ((q = shard_ws(P.S.ordinal[g], P.per * 32, &d)) || (q = load(g, d, cc))) return q;                                                  // b = [Cg][R]: my columns
      if ((q = ntt_run(cc, d.b, P.lg_r, Cg, ALEO_NTT_ORDER_NN, direction, ALEO_NTT_STANDARD, d.st))) return q;                               // [c][k_r] (inverse: x R^-1)
      if ((q = fr_grid_scale(cc, d.b, P.lg_n, Cg, R, g * Cg, 0, 0, 0, direction, d.st))) return q;                                           // *= w_n^(+-c k_r)
      for (size_t h = 0; h < G; ++h)                                                                                                        // a = [h][Cg][Rg]: block h = my columns, device h's k_r range
        HIPCHK(hipMemcpy2DAsync((char*)d.a + h * Cg * Rg * 32, Rg * 32, (char*)d.b + h * Rg * 32, R * 32, Rg * 32, Cg, hipMemcpyDeviceToDevice, d.st));
      HIPCHK(hipStreamSynchronize(d.st));
      return ALEO_MI355X_OK;
    }); });
    // phase 2: the exchange — this device pulls its block of every device e into b = [e][Cg][Rg] = [C][Rg]; own block first, then the peers starting
    // with the next device, so that at any moment every link carries one copy
    phase([&]() -> int32_t {
      for (size_t k = 0; k < G; ++k) { const size_t e = (g + k) % G; const int32_t q = peer_copy((char*)d.b + e * Cg * Rg * 32, d.dev, (char*)sh[e].a + g * Cg * Rg * 32, sh[e].dev, Cg * Rg * 32, d.st); if (q) return q; }
      HIPCHK(hipStreamSynchronize(d.st));
      return ALEO_MI355X_OK;
    });
    // phase 3: row transforms, rows out
    phase([&]() -> int32_t { return with_ctx([&](Ctx* cc) -> int32_t {
      int32_t q;
      if ((q = fr_transpose(cc, d.a, d.b, C, Rg, d.st))) return q;                                                                           // a = [Rg][C]
      if ((q = ntt_run(cc, d.a, P.lg_c, Rg, ALEO_NTT_ORDER_NN, direction, ALEO_NTT_STANDARD, d.st))) return q;                               // [k_r][k_c] (inverse: x C^-1)
      if ((q = store(g, d, cc))) return q;
      HIPCHK(hipStreamSynchronize(d.st));
      return ALEO_MI355X_OK;
    }); });
    if (d.st) (void)hipStreamSynchronize(d.st);              // whatever happened, nothing of this call is left on the shard's stream
    if (r) g_last_error = err;
    return r;
  }, [&](size_t) { failed.store(1); bar.drop(); });          // a shard whose body never ran, or left by an exception, stops counting at the barriers: the others finish (and fail) instead of hanging
}
}  // namespace

// ---- commitments against a sharded committer key (row e2: a proof that spans devices) -------------------------------------------------------------------
// The scalar vectors live on ONE device (the prover's: `c`'s); the base set is cut over G devices (ShardedSet).  A segment [off, off + len) meets shard g
// in [max(off, first_g), min(off + len, first_g + count_g)): that piece of the scalars is pulled by device g (peer copy over xGMI — none when g is the
// scalars' own device) and multiplied there by the ordinary batched Pippenger against shard g's points and tables; what crosses back is k partial
// results of 144 bytes per shard, added on the host in shard order.  The sum of normalised partials is normalised again, so the bytes are those of
// the single-device commitment.
int32_t commit_sharded(Ctx* c, uint64_t sharded_handle, const MsmSeg* segs, uint32_t nseg, uint32_t k, bool mont, uint64_t* out_jac18, hipStream_t s, bool s_drain) {
  auto S = sharded_find(sharded_handle); if (!S) return ALEO_MI355X_ERR_BAD_HANDLE;
  const size_t G = S->devices.size(); const int home = c->device;
  for (uint32_t q = 0; q < nseg; ++q) if (segs[q].out >= k || segs[q].off + segs[q].len > S->n) return bad_arg("commit_sharded: segment out of range");
  if (s_drain) HIPCHK(hipStreamSynchronize(s));              // the scalars are complete (and whatever the caller queued before the commitment has landed)
  std::vector<uint64_t> part((size_t)18 * k * G);
  std::vector<char> busy(G, 0);                              // shards that hold a piece of some segment
  for (size_t g = 0, lo, hi; g < G; ++g) for (uint32_t q = 0; q < nseg && !busy[g]; ++q) busy[g] = seg_in_shard(segs[q], *S, g, &lo, &hi);
  std::mutex lend_mu;                                         // shards that find no free context on the caller's device take turns on the caller's own (idle while it waits here)
  const int32_t rc = for_each_shard(*S, [&](size_t g) -> int32_t {
    uint64_t* mine = &part[(size_t)18 * k * g];
    if (!busy[g]) { for (uint32_t q = 0; q < k; ++q) host::hstore_jacobian_normalized(mine + 18 * q, host::HXYZZ::infinity()); return ALEO_MI355X_OK; }
    Borrowed b; if (int32_t r = borrow_ctx(c, lend_mu, b)) return r;
    Device* d = b.d; Ctx* cc = b.c;
    FoundBases fb(d, S->handles[g]); if (fb.rc) return fb.rc;
    std::vector<MsmSeg> sub; size_t total = 0, lo, hi;
    for (uint32_t q = 0; q < nseg; ++q) {
      if (!seg_in_shard(segs[q], *S, g, &lo, &hi)) continue;
      MsmSeg m; m.d_ptr = (const char*)segs[q].d_ptr + (lo - segs[q].off) * 32; m.len = hi - lo; m.off = lo - S->first[g]; m.out = segs[q].out; sub.push_back(m); total += m.len;
    }
    if (d->device != home) {                                 // pull the pieces: one peer copy each, queued back to back on this shard's stream
      const int32_t r = cc->scalars_stage.reserve(total * 32); if (r) return r;
      size_t at = 0;
      for (auto& m : sub) {
        HIPCHK(hipMemcpyPeerAsync((char*)cc->scalars_stage.p + at * 32, d->device, m.d_ptr, home, m.len * 32, cc->stream));
        m.d_ptr = (const char*)cc->scalars_stage.p + at * 32; at += m.len;
      }
    }
    MsmJob j; j.segs = sub.data(); j.nseg = (uint32_t)sub.size(); j.k = k; j.mont = mont;
    return msm_batch(cc, mine, fb.pb, j, cc->stream);
  });
  if (rc) return rc;
  std::vector<host::HXYZZ> tot(k, host::HXYZZ::infinity());
  for (size_t g = 0; g < G; ++g) { if (!busy[g]) continue; for (uint32_t q = 0; q < k; ++q) tot[q] = host::hadd(tot[q], host::hfrom_jacobian(&part[(size_t)18 * (k * g + q)])); }
  host::hstore_jacobian_normalized_batch(out_jac18, tot.data(), k);
  return ALEO_MI355X_OK;
}

// ---- the same 4-step transform on data that is RESIDENT on the calling thread's device ("home"): row e2, a proof whose transforms span devices -----------
// n = R * C elements in natural order at d_inout on home.  Home (the caller's context and stream) transposes x[R][C] into T[C][R] in a scratch of its own
// (coset: g^j applied first, in place), so that shard g's coefficient columns are ONE contiguous slab T[g Cg .. (g + 1) Cg][R]:
//   phase 1  device g pulls its slab (hipMemcpyPeerAsync; same device: a plain copy), runs its Cg column transforms of length R, multiplies by w_n^(c k_r)
//            and cuts the result into G blocks by k_r range
//   phase 2  the exchange: device h pulls block h of every device (one peer copy per ordered pair — the all-to-all of SURVEY.md 8(e) over xGMI)
//   phase 3  device h transposes to rows k_r, runs its Rg row transforms of length C and pushes the [Rg][C] block back into home's scratch at row h Rg
// and home transposes the scratch [R][C] (k_r major) into d_inout [C][R] = X[k_c R + k_r], natural order (coset inverse: g^-o n^-1 fix-up in place).
// No host buffer anywhere.  Shard work runs on the persistent shard workers with contexts taken by acquire_other (never the caller's `c`, never blocking on one
// context: the caller may be a prover that holds `c` for the whole proof).  Blocking: the result is complete when the call returns.
int32_t ntt_sharded_device(Ctx* c, void* d_inout, uint32_t lg_n, int32_t direction, int32_t type, const int* devices, size_t n_devices, hipStream_t s) {
  ShardPlan P; int32_t rc = sharded_plan("ntt_fr_sharded_device", d_inout, lg_n, direction, type, devices, n_devices, P); if (rc) return rc;
  const size_t n = (size_t)1 << lg_n, R = P.R, C = P.C, Rg = P.Rg, Cg = P.Cg, per = P.per;
  const int home = c->device;
  enable_peer_access();
  if ((rc = c->dev->shard_home.reserve(n * 32))) return rc;
  char* T = c->dev->shard_home.as<char>(); char* x = (char*)d_inout;
  if (type == ALEO_NTT_COSET && direction == ALEO_NTT_FORWARD && (rc = fr_grid_scale(c, x, lg_n, R, C, 0, 0, C, 1, 0, s))) return rc;      // x[j] *= g^j
  if ((rc = fr_transpose(c, T, x, R, C, s))) return rc;                                                                                      // T[c][r]
  HIPCHK(hipStreamSynchronize(s));
  rc = sharded_run(P, c, direction,
    [&](size_t g, const NttShard& d, Ctx*) { return peer_copy(d.b, d.dev, T + g * Cg * R * 32, home, per * 32, d.st); },      // the slab T[g Cg .. (g + 1) Cg][R]
    [&](size_t g, const NttShard& d, Ctx*) { return peer_copy(T + g * Rg * C * 32, home, d.a, d.dev, per * 32, d.st); });     // home scratch [R][C], k_r major (T is dead: every slab was pulled before the first barrier)
  if (rc) return rc;
  if (hipSetDevice(home) != hipSuccess) { g_last_error = "hipSetDevice failed"; return ALEO_MI355X_ERR_HIP; }
  if ((rc = fr_transpose(c, x, T, R, C, s))) return rc;                                                                                      // x[k_c][k_r] = X[k_c R + k_r]
  if (type == ALEO_NTT_COSET && direction == ALEO_NTT_INVERSE && (rc = fr_grid_scale(c, x, lg_n, C, R, 0, 0, R, 1, 1, s))) return rc;        // g^-o (the n^-1 of the inverse came with the two batched transforms)
  HIPCHK(hipStreamSynchronize(s));
  return ALEO_MI355X_OK;
}
// the devices of a sharded base set (the prover routes its large transforms over the devices its committer key is spread over)
int32_t sharded_devices(uint64_t sharded_handle, std::vector<int>* out) {
  auto S = sharded_find(sharded_handle); if (!S) return ALEO_MI355X_ERR_BAD_HANDLE;
  *out = S->devices; return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_bases_pin_sharded(const void* bases, size_t base_stride, size_t n, const int32_t* devices, size_t n_devices, int32_t precompute, uint64_t* handle) {
  return guarded([&] {
    if (!handle || (!bases && n) || (base_stride != 104 && base_stride != 96)) return bad_arg("bases_pin_sharded: bad argument");
    return make_sharded(n, devices, n_devices, precompute, handle, [&](size_t first, size_t count, uint64_t* h) { return aleo_mi355x_bases_pin((const uint8_t*)bases + first * base_stride, base_stride, count, h); });
  });
}

int32_t aleo_mi355x_bases_generate_sharded(const void* base_affine104, uint64_t first_multiple, size_t n, const int32_t* devices, size_t n_devices, int32_t precompute, uint64_t* handle) {
  return guarded([&] {
    if (!handle || !base_affine104) return bad_arg("bases_generate_sharded: bad argument");
    return make_sharded(n, devices, n_devices, precompute, handle, [&](size_t first, size_t count, uint64_t* h) { return aleo_mi355x_bases_generate(base_affine104, first_multiple + first, count, h); });
  });
}

int32_t aleo_mi355x_bases_unpin_sharded(uint64_t handle) {
  return guarded([&] {
    auto S = sharded_find(handle, true); if (!S) return ALEO_MI355X_ERR_BAD_HANDLE;
    sharded_release(*S);
    return ALEO_MI355X_OK;
  });
}

// shard_info: out[0] = number of shards, then per shard: device, first point, point count (as much as cap allows); returns the number of values written
int32_t aleo_mi355x_bases_sharded_info(uint64_t handle, uint64_t* out, int32_t cap) {
  return guarded([&] {
    auto S = sharded_find(handle); if (!S || !out) return 0;
    int32_t w = 0;
    if (w < cap) out[w++] = S->devices.size();
    for (size_t g = 0; g < S->devices.size(); ++g) { const uint64_t v[3] = {(uint64_t)S->devices[g], S->first[g], S->count[g]}; for (uint64_t x : v) if (w < cap) out[w++] = x; }
    return w;
  }, 0);
}

// out: the sum as snarkVM's Projective (x, y, 1 / infinity (1, 1, 0)), 144 bytes; partials (optional, G x 144 bytes): each shard's own sum in shard order
int32_t aleo_mi355x_msm_g1_sharded(void* out_jacobian, uint64_t handle, const void* scalars, size_t n, void* partials_out) {
  return guarded([&] {
    if (!out_jacobian || (!scalars && n)) return bad_arg("msm_g1_sharded: bad argument");
    auto S = sharded_find(handle); if (!S) return ALEO_MI355X_ERR_BAD_HANDLE;
    if (n > S->n) return bad_arg("msm_g1_sharded: more scalars than pinned points");
    const size_t G = S->devices.size();
    std::vector<uint64_t> part(18 * G);
    int32_t rc = for_each_shard(*S, [&](size_t g) -> int32_t {
      const size_t lo = S->first[g] < n ? S->first[g] : n, hi = S->first[g] + S->count[g] < n ? S->first[g] + S->count[g] : n;      // a prefix of the set: shards past n contribute the identity
      return aleo_mi355x_msm_g1_pinned(&part[18 * g], S->handles[g], (const uint8_t*)scalars + lo * 32, hi - lo);
    });
    if (rc) return rc;
    if (partials_out) std::memcpy(partials_out, part.data(), part.size() * 8);
    return aleo_mi355x_g1_sum(out_jacobian, part.data(), G);
  });
}

int32_t aleo_mi355x_bases_attach_shards(uint64_t handle, uint64_t sharded_handle, size_t min_points) {
  return guarded([&] {
    Device* d = nullptr; { const int32_t rc = get_device(&d); if (rc) return rc; }
    size_t n_sh = 0;
    if (sharded_handle) { auto S = sharded_find(sharded_handle); if (!S) return ALEO_MI355X_ERR_BAD_HANDLE; n_sh = S->n; }
    std::shared_ptr<PinnedOwner> o; std::lock_guard<std::mutex> lk(d->mu);
    if (int32_t rc = handle_get(d->bases, handle, "unknown bases handle", &o)) return rc;
    if (sharded_handle && n_sh != o->pb.n) return bad_arg("bases_attach_shards: the sharded set must hold the same number of points");
    o->pb.shards = sharded_handle; o->pb.shard_min = min_points; o->pb.shard_ntt_min = (size_t)1 << 24;
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_bases_shard_transforms(uint64_t handle, size_t min_elements) {
  return guarded([&] {
    Device* d = nullptr; { const int32_t rc = get_device(&d); if (rc) return rc; }
    std::shared_ptr<PinnedOwner> o; std::lock_guard<std::mutex> lk(d->mu);
    if (int32_t rc = handle_get(d->bases, handle, "unknown bases handle", &o)) return rc;
    o->pb.shard_ntt_min = min_elements ? min_elements : (size_t)1 << 24;
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_kzg_commit_segments_sharded_device(void* out104, size_t n_out, uint64_t sharded_handle, const aleo_mi355x_commit_segment* segs, size_t n_segs, void* stream) {
  return guarded([&] {
    if (!n_out) return ALEO_MI355X_OK;
    if (!out104 || (!segs && n_segs) || n_out >= (1u << 20) || n_segs >= (1u << 22)) return bad_arg("commit_segments_sharded: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    std::vector<MsmSeg> sg(n_segs);
    for (size_t q = 0; q < n_segs; ++q) {
      if (!segs[q].scalars && segs[q].len) return bad_arg("commit_segments_sharded: null segment");
      sg[q].d_ptr = segs[q].scalars; sg[q].len = segs[q].len; sg[q].off = segs[q].base_offset; sg[q].out = segs[q].output;
    }
    std::vector<uint64_t> jac(18 * n_out);
    const int32_t rc = commit_sharded(sl.c, sharded_handle, sg.data(), (uint32_t)n_segs, (uint32_t)n_out, true, jac.data(), s, true);
    if (rc) return rc;
    jacobian_rows_to_affine104(out104, jac.data(), n_out);
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_kzg_commit_batch_sharded_device(void* out104, uint64_t sharded_handle, const void* const* d_coeffs, const size_t* lens, size_t k, void* stream) {
  return guarded([&] {
    int32_t rc = batch_args_ok(out104, d_coeffs, lens, k); if (rc || !k) return rc;
    std::vector<aleo_mi355x_commit_segment> sg(k);
    for (size_t q = 0; q < k; ++q) { sg[q].scalars = d_coeffs[q]; sg[q].len = lens[q]; sg[q].base_offset = 0; sg[q].output = (uint32_t)q; }
    return aleo_mi355x_kzg_commit_segments_sharded_device(out104, k, sharded_handle, sg.data(), k, stream);
  });
}

int32_t aleo_mi355x_ntt_fr_sharded(void* inout, uint32_t lg_n, int32_t direction, int32_t type, const int32_t* devices, size_t n_devices) {
  return guarded([&] {
    ShardPlan P; if (int32_t rc = sharded_plan("ntt_fr_sharded", inout, lg_n, direction, type, devices, n_devices, P)) return rc;
    const size_t R = P.R, C = P.C, Rg = P.Rg, Cg = P.Cg; const bool coset = type == ALEO_NTT_COSET; char* host = (char*)inout;
    return sharded_run(P, nullptr, direction,
      [&](size_t g, const NttShard& d, Ctx* cc) -> int32_t {      // my columns of the host's [R][C] matrix: a strided upload, the coset shift, a transpose
        int32_t q;
        HIPCHK(hipMemcpy2DAsync(d.a, Cg * 32, host + g * Cg * 32, C * 32, Cg * 32, R, hipMemcpyHostToDevice, d.st));          // a = [R][Cg] (the runtime stages the pageable buffer itself)
        if (coset && direction == ALEO_NTT_FORWARD && (q = fr_grid_scale(cc, d.a, lg_n, R, Cg, 0, g * Cg, C, 1, 0, d.st))) return q;
        return fr_transpose(cc, d.b, d.a, R, Cg, d.st);                                                                       // b = [Cg][R]
      },
      [&](size_t g, const NttShard& d, Ctx* cc) -> int32_t {      // natural order out: a transpose, the coset fix-up, a strided download
        int32_t q;
        if ((q = fr_transpose(cc, d.b, d.a, Rg, C, d.st))) return q;                                                          // b = [k_c][k_r local]: X[k_c R + k_r]
        if (coset && direction == ALEO_NTT_INVERSE && (q = fr_grid_scale(cc, d.b, lg_n, C, Rg, 0, g * Rg, R, 1, 1, d.st))) return q;
        HIPCHK(hipMemcpy2DAsync(host + g * Rg * 32, R * 32, d.b, Rg * 32, Rg * 32, C, hipMemcpyDeviceToHost, d.st));
        return ALEO_MI355X_OK;
      });
  });
}

int32_t aleo_mi355x_ntt_fr_sharded_device(void* d_inout, uint32_t lg_n, int32_t direction, int32_t type, const int32_t* devices, size_t n_devices, void* stream) {
  return guarded([&] {
    int32_t one = 0; if (!devices && n_devices == 1) { if (hipGetDevice(&one) != hipSuccess) one = 0; devices = &one; }      // NULL: the current device; for more shards the first n_devices visible devices, cyclically (sharded_layout)
    Slot sl; if (sl.rc) return sl.rc;
    hipStream_t s = nullptr; if (int32_t rcs = pick_stream(sl.c, stream, &s)) return rcs;
    return ntt_sharded_device(sl.c, d_inout, lg_n, direction, type, (const int*)devices, n_devices, s);
  });
}

}  // the entry points
