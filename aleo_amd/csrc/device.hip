// device.hip — the per-device state of libaleo_mi355x.so (ctx.h) at run time: devices and their initialisation, peer access, the stream / queue policy, the
// slots and helper contexts calls run on, slot scratch, and the host-side helpers every unit uses (last error, host trace, the small host pool).
#include "entry.h"
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <thread>

namespace aleo_mi355x {

thread_local std::string g_last_error;

bool g_host_trace_on = [] { const char* e = std::getenv("ALEO_MI355X_HOSTTRACE"); return e && e[0] == '1'; }();
namespace { thread_local std::vector<std::pair<const char*, double>> g_host_trace; }
void host_trace_mark(const char* label) {
  const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
  if (label) { g_host_trace.emplace_back(label, t); return; }
  // nullptr: print and clear
  for (size_t i = 0; i < g_host_trace.size(); ++i) fprintf(stderr, "hosttrace %9.1f us  +%7.1f  %s\n", g_host_trace[i].second - g_host_trace[0].second, i ? g_host_trace[i].second - g_host_trace[i - 1].second : 0.0, g_host_trace[i].first);
  g_host_trace.clear();
}

// ---- a small persistent pool for host-side loops -------------------------------------------------------------------------------------------------------
namespace {
struct HostPool {
  static constexpr int T = 3;
  std::mutex mu; std::condition_variable cv_work, cv_done; const std::function<void(size_t)>* f = nullptr; size_t n = 0; std::atomic<size_t> next{0}; int active = 0; uint64_t gen = 0; bool started = false;
  std::mutex call_mu;                                       // one parallel loop at a time (concurrent callers fall back to their own thread)
  void worker() {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(size_t)>* fn; size_t cnt;
      { std::unique_lock<std::mutex> lk(mu); cv_work.wait(lk, [&] { return gen != seen; }); seen = gen; fn = f; cnt = n; }
      for (size_t i; (i = next.fetch_add(1)) < cnt;) (*fn)(i);
      { std::lock_guard<std::mutex> lk(mu); if (--active == 0) cv_done.notify_all(); }
    }
  }
};
HostPool* g_host_pool = nullptr; std::once_flag g_host_pool_once;
}  // namespace
void host_parallel_for(size_t n, const std::function<void(size_t)>& f) {
  if (n < 2) { for (size_t i = 0; i < n; ++i) f(i); return; }
  std::call_once(g_host_pool_once, [] {
    HostPool* p = new HostPool();                            // leaked on purpose: its threads sleep until the process ends
    try { for (int t = 0; t < HostPool::T; ++t) std::thread([p] { p->worker(); }).detach(); p->started = true; } catch (...) { p->started = false; }
    g_host_pool = p;
  });
  HostPool* p = g_host_pool;
  std::unique_lock<std::mutex> one(p->call_mu, std::try_to_lock);
  if (!p->started || !one.owns_lock()) { for (size_t i = 0; i < n; ++i) f(i); return; }
  { std::lock_guard<std::mutex> lk(p->mu); p->f = &f; p->n = n; p->next.store(0); p->active = HostPool::T; ++p->gen; }
  p->cv_work.notify_all();
  for (size_t i; (i = p->next.fetch_add(1)) < n;) f(i);
  { std::unique_lock<std::mutex> lk(p->mu); p->cv_done.wait(lk, [&] { return p->active == 0; }); }
}

static std::mutex g_dev_mu;
static std::map<int, Device*> g_devs;
static int32_t create_streams_in_order(Device* d);

int32_t ensure_host_pinned(Ctx* c, size_t bytes) {
  if (bytes <= c->h_pinned_cap) return ALEO_MI355X_OK;
  if (c->h_pinned) (void)hipHostFree(c->h_pinned);
  c->h_pinned = nullptr; c->h_pinned_cap = 0;
  size_t want = bytes < 65536 ? 65536 : bytes;
  HIPCHK(hipHostMalloc(&c->h_pinned, want, hipHostMallocMapped));      // device-mapped: the last fold kernel of an MSM stores its result here
  c->h_pinned_cap = want; return ALEO_MI355X_OK;
}

int32_t resident_table(int device, ResidentTable kind, const std::vector<uint32_t>& (*words)(), const uint32_t** out) {
  static std::mutex mu; static std::map<std::pair<int, ResidentTable>, const uint32_t*> resident;
  const std::vector<uint32_t>& w = words();                 // built on the host at first use (a function-local static of its unit), outside the lock
  std::lock_guard<std::mutex> lk(mu);
  auto it = resident.find({device, kind});
  if (it == resident.end()) {
    DevTmp buf; if (int32_t rc = buf.alloc(w.size() * 4)) return rc;
    HIPCHK(hipMemcpy(buf.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    it = resident.emplace(std::make_pair(device, kind), (const uint32_t*)buf.release()).first;
  }
  *out = it->second; return ALEO_MI355X_OK;
}

// ---- slot scratch shared by asynchronous calls (ctx.h) --------------------------------------------------
int32_t scratch_acquire(Ctx* c, DevBuf& b, size_t bytes, hipStream_t s) {
  if (c->scratch_busy) {
    const bool grows = bytes > b.cap;
    if (c->scratch_stream && (grows || c->scratch_stream != s)) { HIPCHK(hipEventRecord(c->scratch_ev, c->scratch_stream)); c->scratch_stream = nullptr; }      // the deferred record: behind everything queued there so far
    if (grows) { HIPCHK(hipEventSynchronize(c->scratch_ev)); c->scratch_busy = false; }   // reserve() is about to free it
    else if (!c->scratch_stream) HIPCHK(hipStreamWaitEvent(s, c->scratch_ev, 0));
    // (same stream as the last user: stream order is the order)
  }
  return b.reserve(bytes);
}
int32_t scratch_release(Ctx* c, hipStream_t s) {
  c->scratch_busy = true;
  if (s && (s == c->stream || s == c->side || s == c->aux || s == c->hi)) { c->scratch_stream = s; return ALEO_MI355X_OK; }      // a stream the slot owns: it outlives the deferred record
  c->scratch_stream = nullptr;
  HIPCHK(hipEventRecord(c->scratch_ev, s)); return ALEO_MI355X_OK;      // a caller's stream may be gone by the next call: record now
}

int32_t init_device(int device, Device** out) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { g_last_error = "no HIP device visible"; return ALEO_MI355X_ERR_NO_DEVICE; }
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) { g_last_error = "hipGetDevice failed"; return ALEO_MI355X_ERR_NO_DEVICE; } }
  if (device >= count) return bad_arg("device index out of range");
  auto it = g_devs.find(device);
  if (it != g_devs.end()) { *out = it->second; (void)hipSetDevice(device); return ALEO_MI355X_OK; }      // "selects": the calling thread works on this device from here on
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_last_error = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only";
    return ALEO_MI355X_ERR_NO_DEVICE;
  }
  std::unique_ptr<Device> d(new Device());
  d->device = device;
  if (const char* e = std::getenv("ALEO_MI355X_SLOTS")) { int k = std::atoi(e); if (k >= 1 && k <= MAX_SLOTS) d->n_slots = k; }
  for (int i = 0; i < MAX_SLOTS; ++i) { d->slots[i].dev = d.get(); d->slots[i].device = device; d->helpers[i].dev = d.get(); d->helpers[i].device = device; }
  *out = d.get();
  g_devs[device] = d.release();
  return create_streams_in_order(*out);                      // the main streams first: a hardware queue each (see "streams" below)
}

// Direct peer access between every ordered pair of initialised devices (xGMI: hipMemcpyPeerAsync then moves data link to link instead of through a
// staging buffer; the sharded transform's exchange is one such copy per pair).  "Already enabled" is fine; a refusal (no link, IOMMU) is recorded and
// the copies fall back to the runtime's staged path — never fatal.  Idempotent: pairs are tried once.
static std::map<std::pair<int, int>, bool> g_peer;          // (device, peer) -> direct access enabled; guarded by g_dev_mu
void enable_peer_access() {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  int cur = 0; if (hipGetDevice(&cur) != hipSuccess) cur = 0;
  for (const auto& a : g_devs) for (const auto& b : g_devs) {
    if (a.first == b.first || g_peer.count({a.first, b.first})) continue;
    int can = 0; bool ok = false;
    if (hipDeviceCanAccessPeer(&can, a.first, b.first) == hipSuccess && can && hipSetDevice(a.first) == hipSuccess) {
      const hipError_t e = hipDeviceEnablePeerAccess(b.first, 0);
      ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
      (void)hipGetLastError();                               // "already enabled" must not linger as the thread's last error
    }
    g_peer[{a.first, b.first}] = ok;
  }
  (void)hipSetDevice(cur);
}

// GPU_MAX_HW_QUEUES (read by the HIP runtime when it initialises; default 4) is an environment REQUIREMENT of the host, documented in the header and in
// the library never touches the process environment (setenv from a loaded library races with getenv in the host's other threads).
// The Python package and bench.py set their own default before HIP starts.

int32_t get_device(Device** out) {
  int device = -1;
  if (hipGetDevice(&device) != hipSuccess) { g_last_error = "no HIP device visible"; return ALEO_MI355X_ERR_NO_DEVICE; }
  {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_devs.find(device);
    if (it != g_devs.end()) { *out = it->second; return ALEO_MI355X_OK; }
  }
  return init_device(device, out);
}

// ---- streams -------------------------------------------------------------------------------------------------------------------------------------------
// The runtime deals the streams of one priority onto at most GPU_MAX_HW_QUEUES hardware queues (to the queue with the fewest streams, so in creation order), and what shares a
// hardware queue runs in queue order.  Measured on this pool (profiles/r05_stream_order_*.txt, r05_hw_queues_ab.txt, r05_hi_priority_ab.txt):
//   * the MAIN streams are the ones that run side by side (lockstep groups and their workers, concurrent callers): created first — the slots', then as many helpers' — they get a
//     queue each; with every context creating stream | side | hi at its first use they collided: a lockstep call of 8 proofs 31.8 -> 28.0 ms, of 16 58.5 -> 54.0;
//   * more hardware queues than ~20 in all (GPU_MAX_HW_QUEUES >= 12, or a third priority level) and the same call takes 43-65 ms: the queues are oversubscribed;
//   * EIGHT high-priority streams created in a row (one per context) made a 2^20-constraint proof — whose chains' sorts run on them — take 1.1-2.5 s instead of 80 ms; at normal
//     priority the same arrangement is harmless.  So the device keeps a small POOL of high-priority streams (HI_POOL; chunked uploads need one per later
//     chunk) that its contexts share round-robin, slot i and helper i + 1 on different ones.
static constexpr int HI_POOL = 4;
static std::mutex g_stream_mu;
static int32_t create_streams_in_order(Device* d) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  if (d->slots[0].stream) return ALEO_MI355X_OK;
  for (int i = 0; i < d->n_slots; ++i) HIPCHK(hipStreamCreateWithFlags(&d->slots[i].stream, hipStreamNonBlocking));
  for (int i = 0; i < d->n_slots; ++i) HIPCHK(hipStreamCreateWithFlags(&d->helpers[i].stream, hipStreamNonBlocking));
  return ALEO_MI355X_OK;
}
static int32_t hi_stream_for(Ctx* c, hipStream_t* out) {
  Device* d = c->dev;
  if (!d) { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi); HIPCHK(hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi)); return ALEO_MI355X_OK; }
  std::lock_guard<std::mutex> lk(g_stream_mu);
  const bool helper = c >= &d->helpers[0] && c < &d->helpers[MAX_SLOTS];
  const int idx = helper ? (int)(c - &d->helpers[0]) + 1 : (int)(c - &d->slots[0]), k = idx % HI_POOL;      // slot i and helpers i, i + 1 (a pipeline's ring, a chunked call's later chunks) on different ones
  while (d->hi_made <= k) {
    int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // hi = the numerically lowest = highest priority
    HIPCHK(hipStreamCreateWithPriority(&d->hi_pool[d->hi_made], hipStreamNonBlocking, hi)); ++d->hi_made;
  }
  *out = d->hi_pool[k]; return ALEO_MI355X_OK;
}
static int32_t first_use(Ctx* c) {          // streams and events of a slot, created when it is first handed out (the device is current)
  if (c->ev[0]) return ALEO_MI355X_OK;
  if (c->dev) { const int32_t rc = create_streams_in_order(c->dev); if (rc) return rc; }
  if (!c->stream) HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (!c->side) HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  if (!c->aux) HIPCHK(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
  if (!c->hi) { const int32_t rc = hi_stream_for(c, &c->hi); if (rc) return rc; }
  for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventCreateWithFlags(&c->scratch_ev, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_hop, hipEventDisableTiming));
  return ALEO_MI355X_OK;
}

// Picks a free slot (or waits on one chosen by thread id) and locks it for the duration of the call.
static int32_t acquire_slot(Device* d, Ctx** out, std::unique_lock<std::mutex>& lk) {
  Ctx* c = nullptr;
  for (int i = 0; i < d->n_slots && !c; ++i) {
    std::unique_lock<std::mutex> t(d->slots[i].mu, std::try_to_lock);
    if (t.owns_lock()) { lk = std::move(t); c = &d->slots[i]; }
  }
  if (!c) {
    size_t i = std::hash<std::thread::id>()(std::this_thread::get_id()) % (size_t)d->n_slots;
    lk = std::unique_lock<std::mutex>(d->slots[i].mu); c = &d->slots[i];
  }
  if (hipSetDevice(d->device) != hipSuccess) { g_last_error = "hipSetDevice failed"; return ALEO_MI355X_ERR_HIP; }
  { const int32_t rc = first_use(c); if (rc) return rc; }
  *out = c; return ALEO_MI355X_OK;
}

// A context of device d for work done on behalf of a call that already holds `exclude` (a slot of the same device, or nullptr): free slots first, then
// helper contexts, never `exclude` itself — the holder is waiting for this work.  It never blocks on ONE context: the contexts of the caller's own device
// may all be held by workers of the very call this work belongs to (a lockstep call parked at its round barrier, waiting for the commitment this shard is
// part of — the round-4 form blocked on helpers[hash(tid) % 8] and could deadlock there).  `may_wait`: poll all of them until one is free (another device:
// whoever holds its contexts is an independent call and will finish); otherwise *out stays nullptr and the caller lends its own context (commit_sharded).
int32_t acquire_other(Device* d, const Ctx* exclude, Ctx** out, std::unique_lock<std::mutex>& lk, bool may_wait) {
  Ctx* c = nullptr; *out = nullptr;
  for (;;) {
    for (int i = 0; i < d->n_slots && !c; ++i) {
      if (&d->slots[i] == exclude) continue;
      std::unique_lock<std::mutex> t(d->slots[i].mu, std::try_to_lock);
      if (t.owns_lock()) { lk = std::move(t); c = &d->slots[i]; }
    }
    for (int i = 0; i < MAX_SLOTS && !c; ++i) {
      if (&d->helpers[i] == exclude) continue;
      std::unique_lock<std::mutex> t(d->helpers[i].mu, std::try_to_lock);
      if (t.owns_lock()) { lk = std::move(t); c = &d->helpers[i]; }
    }
    if (c || !may_wait) break;
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
  if (!c) return ALEO_MI355X_OK;
  if (hipSetDevice(d->device) != hipSuccess) { g_last_error = "hipSetDevice failed"; return ALEO_MI355X_ERR_HIP; }
  { const int32_t rc = first_use(c); if (rc) return rc; }
  *out = c; return ALEO_MI355X_OK;
}

int32_t acquire_helpers(Device* d, int want, HelperSet& hs) {
  for (int i = 0; i < MAX_SLOTS && (int)hs.ctx.size() < want; ++i) {
    std::unique_lock<std::mutex> t(d->helpers[i].mu, std::try_to_lock);
    if (!t.owns_lock()) continue;
    { const int32_t rc = first_use(&d->helpers[i]); if (rc) return rc; }
    hs.ctx.push_back(&d->helpers[i]); hs.locks.push_back(std::move(t));
  }
  return ALEO_MI355X_OK;
}

Slot::Slot() { if (!(rc = get_device(&d))) rc = acquire_slot(d, &c, lk); }

// The stream a call works on: the caller's, or the slot's own for NULL.  hipStreamLegacy is passed on as the null stream it
// names (this library is not built with a per-thread default stream): the runtime takes the special handle for launches but
// not for every event call.
// hipStreamPerThread is refused: it names a different stream on every host thread, and a slot's events may be waited on by another.
int32_t pick_stream(Ctx* c, void* stream, hipStream_t* out) {
  if ((hipStream_t)stream == hipStreamPerThread) return bad_arg("stream: hipStreamPerThread is not supported (pass a created stream, hipStreamLegacy or NULL)");
  *out = !stream ? c->stream : ((hipStream_t)stream == hipStreamLegacy ? (hipStream_t)nullptr : (hipStream_t)stream);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_init_device(int32_t device) {
  return guarded([&] { Device* d = nullptr; return init_device(device, &d); });
}

// init(n_devices, 0 = all).  Initialises the first n visible devices; the calling thread's current device is left as it was.
int32_t aleo_mi355x_init(int32_t n_devices) {
  return guarded([&] {
    int count = 0, cur = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { g_last_error = "no HIP device visible"; return ALEO_MI355X_ERR_NO_DEVICE; }
    if (n_devices < 0 || n_devices > count) return bad_arg("init: n_devices outside 0..visible devices (0 = all)");
    if (hipGetDevice(&cur) != hipSuccess) cur = 0;
    const int n = n_devices ? n_devices : count;
    int32_t rc = ALEO_MI355X_OK;
    for (int i = 0; i < n && !rc; ++i) { Device* d = nullptr; rc = init_device(i, &d); }
    if (!rc) enable_peer_access();
    (void)hipSetDevice(cur);
    return rc;
  });
}

int32_t aleo_mi355x_peer_info(int32_t* enabled_pairs, int32_t* refused_pairs) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    int32_t on = 0, off = 0;
    for (const auto& kv : g_peer) (kv.second ? on : off)++;
    if (enabled_pairs) *enabled_pairs = on;
    if (refused_pairs) *refused_pairs = off;
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_device_count(int32_t* visible, int32_t* initialised) {
  return guarded([&] {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
    if (visible) *visible = count;
    if (initialised) { std::lock_guard<std::mutex> lk(g_dev_mu); *initialised = (int32_t)g_devs.size(); }
    return ALEO_MI355X_OK;
  });
}

}  // the entry points
