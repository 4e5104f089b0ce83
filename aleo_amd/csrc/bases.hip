// bases.hip — base sets of libaleo_mi355x.so: staging point rows into HBM (pinned sets that own their buffers, the cold one-shot call's copy in the slot's),
// the G1 and G2 handle tables, fixed-base tables built once per set, the SRS cache, host-scalar MSMs against a set, and the bases_* entry points.
#include "entry.h"
#include "g2.h"
#include <cstdlib>
#include <cstring>

namespace aleo_mi355x {

// ---- row staging: rows up, unpacked on the device when they came in the strided form, infinities counted ----------------------------------------------
// A point set arrives as packed rows (x | y) or in snarkVM's strided form (the infinity byte + padding behind the coordinates).  `unpack` turns strided rows
// into packed ones plus one flag byte per row, and leaves the number of set flags in a uint32 behind the flags, at the next multiple of 4.
struct RowFormat { size_t packed, strided; int32_t (*unpack)(Ctx* c, const void* d_rows, void* d_xy, void* d_flags, size_t n, hipStream_t s); };
static int32_t unpack_g2_200(Ctx* c, const void* d_rows, void* d_xy, void* d_flags, size_t n, hipStream_t s) {
  return g2_unpack200(d_rows, d_xy, d_flags, (uint32_t*)((char*)d_flags + ((n + 3) & ~(size_t)3)), n, s);
}
static constexpr RowFormat G1_ROWS = {96, 104, unpack_affine104}, G2_ROWS = {192, 200, unpack_g2_200};

// n rows into d_xy on c->stream; *n_inf = how many are the point at infinity (flag bytes at d_flags).  d_raw (n strided rows) and d_flags (n + 8 bytes) are the
// caller's, touched for strided rows only.  Packed rows are left queued on the stream; strided ones have landed (the count was read back).
// The strided rows go up as they are (one copy at PCIe rate) and are unpacked on the device: a host loop that strips the flag byte + padding first cost 30 ms
// per 2^20 G1 points — the one-shot call of the two-line drop-in spent most of its time there — and ~ 60 of the 91 ms of a 2^20-point G2 call.
static int32_t stage_rows(Ctx* c, const RowFormat& f, const void* rows, size_t stride, size_t n, void* d_xy, void* d_raw, void* d_flags, uint32_t* n_inf) {
  *n_inf = 0;
  if (!n) return ALEO_MI355X_OK;
  if (stride == f.packed) { HIPCHK(hipMemcpyAsync(d_xy, rows, n * f.packed, hipMemcpyHostToDevice, c->stream)); return ALEO_MI355X_OK; }
  HIPCHK(hipMemcpyAsync(d_raw, rows, n * f.strided, hipMemcpyHostToDevice, c->stream));
  if (int32_t rc = f.unpack(c, d_raw, d_xy, d_flags, n, c->stream)) return rc;
  HIPCHK(hipMemcpyAsync(n_inf, (char*)d_flags + ((n + 3) & ~(size_t)3), 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ALEO_MI355X_OK;
}
// ... into buffers allocated here, which the caller then owns (a pinned set): *d_inf stays nullptr when no row is the point at infinity
static int32_t stage_rows_owned(Ctx* c, const RowFormat& f, const void* rows, size_t stride, size_t n, void** d_xy, uint8_t** d_inf) {
  DevTmp raw, flags; uint32_t n_inf = 0; int32_t rc;
  HIPCHK(hipMalloc(d_xy, (n ? n : 1) * f.packed));
  if (n && stride != f.packed && ((rc = raw.alloc(n * f.strided)) || (rc = flags.alloc(n + 8)))) return rc;
  if ((rc = stage_rows(c, f, rows, stride, n, *d_xy, raw.p, flags.p, &n_inf))) return rc;
  if (n_inf) *d_inf = (uint8_t*)flags.release();
  return ALEO_MI355X_OK;
}
// ... into the slot's grow-only buffers (one one-shot call per slot at a time, G1 or G2): rows at c->cold_xy.p, *d_inf = c->cold_flags.p or nullptr
static int32_t stage_rows_cold(Ctx* c, const RowFormat& f, const void* rows, size_t stride, size_t n, const uint8_t** d_inf) {
  uint32_t n_inf = 0; int32_t rc;
  if ((rc = c->cold_xy.reserve((n ? n : 1) * f.packed))) return rc;
  if (n && stride != f.packed && ((rc = c->cold_raw.reserve(n * f.strided)) || (rc = c->cold_flags.reserve(n + 16)))) return rc;
  if ((rc = stage_rows(c, f, rows, stride, n, c->cold_xy.p, c->cold_raw.p, c->cold_flags.p, &n_inf))) return rc;
  *d_inf = n_inf ? (const uint8_t*)c->cold_flags.p : nullptr;
  return ALEO_MI355X_OK;
}

// ---- pinned base sets (shared by all slots) ----------------------------------------------------------
static int32_t upload_bases(Ctx* c, const void* bases, size_t stride, size_t n, std::shared_ptr<PinnedOwner>* out) {
  auto o = std::make_shared<PinnedOwner>(); PinnedBases& pb = o->pb; pb.n = n; int32_t rc;
  if ((rc = stage_rows_owned(c, G1_ROWS, bases, stride, n, &pb.d_xy, &pb.d_inf)) || (rc = make_rows28(c, &pb))) return rc;      // (make_rows28 synchronises: packed rows have landed too)
  *out = std::move(o); return ALEO_MI355X_OK;
}
// The same into the slot's own buffers, as a view nobody owns (the cold one-shot call: aleo_mi355x_msm_g1 without the SRS cache)
static int32_t cold_bases(Ctx* c, const void* bases, size_t stride, size_t n, PinnedBases* pb) {
  *pb = PinnedBases(); pb->n = n; int32_t rc; const uint8_t* d_inf = nullptr;
  if ((rc = stage_rows_cold(c, G1_ROWS, bases, stride, n, &d_inf)) || (rc = c->cold_xy28.reserve((n ? n : 1) * ROW28))) return rc;
  pb->d_xy = c->cold_xy.p; pb->d_inf = (uint8_t*)d_inf;
  if ((rc = rows_to28_into(pb->d_xy, c->cold_xy28.p, n, c->stream))) return rc;
  pb->d_xy28 = c->cold_xy28.p;
  return ALEO_MI355X_OK;
}
// a new handle for a G1 or G2 set (the two tables share next_handle's counter)
template <class T> static uint64_t register_set(Device* d, std::map<uint64_t, std::shared_ptr<T>>& table, std::shared_ptr<T> o) {
  std::lock_guard<std::mutex> lk(d->mu);
  uint64_t h = d->next_handle++; table[h] = std::move(o); return h;
}
// The set behind a handle plus a snapshot of its fields (the table pointer may be published by another slot at any time).
int32_t find_bases(Device* d, uint64_t handle, std::shared_ptr<PinnedOwner>* keep, PinnedBases* snap) {
  std::lock_guard<std::mutex> lk(d->mu);
  if (int32_t rc = handle_get(d->bases, handle, "unknown bases handle", keep)) return rc;
  *snap = (*keep)->pb; return ALEO_MI355X_OK;
}
// drops a set from its table: `dead` is declared before the lock, so the set is freed after the lock is dropped
template <class T> static int32_t unpin(Device* d, std::map<uint64_t, std::shared_ptr<T>>& table, uint64_t handle, const char* unknown) {
  std::shared_ptr<T> dead;
  std::lock_guard<std::mutex> lk(d->mu);
  return handle_get(table, handle, unknown, &dead, true);
}
// Builds the fixed-base table of a set on slot c unless it exists or another slot is building it; publishes it under the lock.
static int32_t precompute_once(Ctx* c, const std::shared_ptr<PinnedOwner>& o) {
  Device* d = c->dev; PinnedBases work;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (o->pb.tabled || o->building) return ALEO_MI355X_OK;
    o->building = true; work = o->pb;
  }
  int32_t rc = msm_precompute(c, &work);
  std::lock_guard<std::mutex> lk(d->mu);
  o->building = false;
  if (rc == ALEO_MI355X_OK) { for (int i = 0; i < 3; ++i) o->pb.tab[i] = work.tab[i]; o->pb.tabled = true; }
  return rc;
}

// Canonical host scalars whose sample is mostly 0 / 1 / short (a witness: SURVEY.md §8d "witness-like") take the set's range table when it has one
// and covers the call: 257 scalars spread over the vector, sparse = at least half of them below 2^32.
static bool looks_sparse(const void* scalars, size_t n) {
  if (n < 4096) return false;
  const uint64_t* s = (const uint64_t*)scalars; size_t small = 0; const size_t step = n / 257;
  for (size_t i = 0; i < 257; ++i) { const uint64_t* v = s + 4 * (i * step); small += (v[1] | v[2] | v[3]) == 0 && v[0] < (1ull << 32); }
  return small >= 129;
}
int32_t msm_host_scalars(Ctx* c, void* out, const PinnedBases& pb, const void* scalars, size_t n, bool mont) {
  const bool skewed = !mont && looks_sparse(scalars, n);          // witness-like: the few huge buckets (their slice trees beside the reduction) decide, not the upload — one chain
  const bool sparse = skewed && pb.range.d && pb.range_off == 0 && n <= pb.range.cover;
  if (!n) return msm_run1(c, (uint64_t*)out, pb, nullptr, 0, mont, c->stream, false);
  return msm_run1_split(c, (uint64_t*)out, pb, nullptr, n, mont, c->stream, sparse, scalars, !skewed);      // uploads inside (whole, or in two halves that share one reduction)
}

// ---- SRS cache for the one-shot entry point ----------------------------------------------------------
static uint64_t hash96(const uint8_t* p) {      // FNV-1a over the 96 coordinate bytes of one point
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < 96; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
static constexpr size_t SRS_SAMPLES = 256, SRS_CACHE_ENTRIES = 8, SRS_MIN_N = 1024;

static bool srs_cache_enabled() {          // opt-in (see the header); read per call so a host can switch it around a phase
  const char* e = std::getenv("ALEO_MI355X_SRS_CACHE");
  return e && e[0] == '1';
}
// Caller holds d->mu.  Returns the cached entry for (bases, stride) that covers n points, or nullptr.
static SrsCacheEntry* srs_lookup(Device* d, const void* bases, size_t stride, size_t n) {
  for (auto& e : d->srs_cache) {
    if (e.host_ptr != bases || e.stride != stride || e.n < n) continue;
    bool ok = true; size_t checked = 0;
    for (auto& sm : e.samples) {                 // only samples inside the caller's slice may be read
      if (sm.first >= n) continue;
      ++checked;
      if (hash96((const uint8_t*)bases + sm.first * stride) != sm.second) { ok = false; break; }
    }
    if (ok && checked) return &e;
  }
  return nullptr;
}
// The resident set for a one-shot call's base array: a cache hit, or a fresh upload that replaces stale / least recently
// used entries.  `want_table` is set on the third use of a set large enough to repay the one-off table build.
static int32_t srs_get(Ctx* c, Device* d, const void* bases, size_t stride, size_t n, std::shared_ptr<PinnedOwner>* keep, bool* want_table) {
  *want_table = false;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (SrsCacheEntry* e = srs_lookup(d, bases, stride, n)) {
      e->last_use = ++d->srs_clock; e->hits++;
      *keep = d->bases[e->handle];
      *want_table = e->hits >= 3 && e->n >= (1u << 10) && !(*keep)->pb.tabled;
      return ALEO_MI355X_OK;
    }
  }
  std::shared_ptr<PinnedOwner> o;              // the bulk upload runs without the lock
  int32_t rc = upload_bases(c, bases, stride, n, &o);
  if (rc) return rc;
  SrsCacheEntry e; e.host_ptr = bases; e.stride = stride; e.n = n; e.hits = 1;
  // dense samples at the front (every prefix request can be checked), sparse ones over the rest
  for (size_t k = 0; k < SRS_SAMPLES; ++k) {
    size_t idx = k < 32 ? k : (size_t)((double)(k - 31) / (SRS_SAMPLES - 31) * (n - 1));
    if (idx >= n) break;
    e.samples.emplace_back(idx, hash96((const uint8_t*)bases + idx * stride));
  }
  std::vector<std::shared_ptr<PinnedOwner>> dead;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    auto drop = [&](size_t i) {
      auto it = d->bases.find(d->srs_cache[i].handle);
      if (it != d->bases.end()) { dead.push_back(std::move(it->second)); d->bases.erase(it); }
      d->srs_cache.erase(d->srs_cache.begin() + i);
    };
    for (size_t i = 0; i < d->srs_cache.size();) { if (d->srs_cache[i].host_ptr == bases) drop(i); else ++i; }
    if (d->srs_cache.size() >= SRS_CACHE_ENTRIES) {
      size_t lru = 0; for (size_t i = 1; i < d->srs_cache.size(); ++i) if (d->srs_cache[i].last_use < d->srs_cache[lru].last_use) lru = i;
      drop(lru);
    }
    e.handle = d->next_handle++; e.last_use = ++d->srs_clock;
    d->bases[e.handle] = o; d->srs_cache.push_back(e);
  }
  *keep = std::move(o);
  return ALEO_MI355X_OK;
}

// A G2 base set kept on the device (round 5): rows, infinity flags and the 28-bit rows of the accumulation stay in HBM, so a call moves only its scalars
// (the one-shot entry point aleo_mi355x_msm_g2 uploads 192-200 bytes per base and rebuilds the 28-bit rows every time: 3.8 + 0.4 of its 22 ms at 2^20).  Any prefix
// of the set can be multiplied.  G2 appears in SRS setup and verifying keys, never in the prover's loop: no window tables.
static int32_t g2_upload(Ctx* c, const void* bases, size_t base_stride, size_t n, std::shared_ptr<PinnedG2>* out) {
  auto o = std::make_shared<PinnedG2>(); o->n = n; int32_t rc;
  HIPCHK(hipMalloc(&o->d_rows28, (n ? n : 1) * 224));
  if ((rc = stage_rows_owned(c, G2_ROWS, bases, base_stride, n, &o->d_xy, &o->d_inf)) || (rc = g2_rows_to28(o->d_xy, o->d_rows28, n, c->stream))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  *out = std::move(o); return ALEO_MI355X_OK;
}

// ---- the one-shot calls' copy of their base array --------------------------------------------------------------------
int32_t one_shot_bases(Ctx* c, const void* bases, size_t stride, size_t n, std::shared_ptr<PinnedOwner>* keep, PinnedBases* pb) {
  Device* d = c->dev;
  if (n >= SRS_MIN_N && srs_cache_enabled()) {
    // ALEO_MI355X_SRS_CACHE=1 (opt-in): KZG10::commit multiplies against prefixes of one SRS, so the base array is kept in
    // HBM between calls, recognised by host pointer + sampled content.  Off by default: it reads caller memory the ABI
    // otherwise does not retain, and an array rewritten in place at unsampled entries would be served stale.
    bool want_table = false;
    int32_t rc = srs_get(c, d, bases, stride, n, keep, &want_table);
    if (rc) return rc;
    if (want_table) (void)precompute_once(c, *keep);                       // third use: worth the one-off table
    std::lock_guard<std::mutex> g(d->mu); *pb = (*keep)->pb;
    return ALEO_MI355X_OK;
  }
  // Nothing cached (the literal two-line drop-in): the call's copy of the bases lives in the SLOT's grow-only buffers (rows as uploaded, x | y rows, 28-bit rows, flags:
  // 337 bytes per point, kept by the slot like its other workspaces), not in hipMalloc / hipFree pairs per call — hipFree waits for the device, and the pairs were 0.x ms of a
  // 7.6 ms call at 2^20 (ALEO_MI355X_COLD_POOL=0: a PinnedOwner per call, as before).
  static const bool cold_pool = [] { const char* e = std::getenv("ALEO_MI355X_COLD_POOL"); return !(e && e[0] == '0'); }();
  if (cold_pool) return cold_bases(c, bases, stride, n, pb);
  int32_t rc = upload_bases(c, bases, stride, n, keep);
  if (!rc) *pb = (*keep)->pb;
  return rc;
}
// G2: always in the slot's grow-only buffers (shared with the cold G1 call: one call per slot at a time), not hipMalloc / hipFree pairs
int32_t one_shot_bases_g2(Ctx* c, const void* bases, size_t stride, size_t n, const void** d_xy, const uint8_t** d_inf) {
  const int32_t rc = stage_rows_cold(c, G2_ROWS, bases, stride, n, d_inf);
  *d_xy = c->cold_xy.p; return rc;
}

// bases_pin / bases_generate / bases_from_scalars: a slot, a new set filled by `fill` on it, its handle
template <class Fill> static int32_t pin_new(uint64_t* handle, Fill&& fill) {
  Slot sl; if (sl.rc) return sl.rc;
  std::shared_ptr<PinnedOwner> o;
  if (int32_t rc = fill(sl.c, &o)) return rc;
  *handle = register_set(sl.d, sl.d->bases, std::move(o));
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

int32_t aleo_mi355x_bases_pin(const void* bases, size_t base_stride, size_t n, uint64_t* handle) {
  return guarded([&] {
    if (!handle || (!bases && n) || (base_stride != 104 && base_stride != 96)) return bad_arg("bases_pin: bad argument");
    return pin_new(handle, [&](Ctx* c, std::shared_ptr<PinnedOwner>* o) { return upload_bases(c, bases, base_stride, n, o); });
  });
}

int32_t aleo_mi355x_bases_generate(const void* base104, uint64_t first, size_t n, uint64_t* handle) {
  return guarded([&] {
    if (!base104 || !handle) return ALEO_MI355X_ERR_BAD_ARG;
    return pin_new(handle, [&](Ctx* c, std::shared_ptr<PinnedOwner>* o) { *o = std::make_shared<PinnedOwner>(); return generate_multiples(c, base104, first, n, &(*o)->pb); });
  });
}

int32_t aleo_mi355x_bases_from_scalars(const void* base104, const void* scalars, size_t n, uint64_t* handle) {
  return guarded([&] {
    if (!base104 || !handle || !scalars) return ALEO_MI355X_ERR_BAD_ARG;
    return pin_new(handle, [&](Ctx* c, std::shared_ptr<PinnedOwner>* o) { *o = std::make_shared<PinnedOwner>(); return generate_from_scalars(c, base104, scalars, n, &(*o)->pb); });
  });
}

int32_t aleo_mi355x_bases_precompute(uint64_t handle) {
  return guarded([&] {
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    return precompute_once(sl.c, fb.keep);
  });
}

int32_t aleo_mi355x_bases_precompute_range(uint64_t handle, size_t offset, size_t n, int32_t window_bits) {
  return guarded([&] {
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<PinnedOwner> keep; PinnedBases work; { int32_t rcb = find_bases(sl.d, handle, &keep, &work); if (rcb) return rcb; }
    { std::lock_guard<std::mutex> g(sl.d->mu); if (keep->building) return bad_arg("bases_precompute_range: a table build is in flight"); keep->building = true; work = keep->pb; }
    int32_t rc = msm_precompute_range(sl.c, &work, offset, n, window_bits);
    std::lock_guard<std::mutex> g(sl.d->mu);
    keep->building = false;
    if (rc == ALEO_MI355X_OK) { keep->pb.range = work.range; keep->pb.range_off = work.range_off; }
    return rc;
  });
}

int32_t aleo_mi355x_bases_info(uint64_t handle, uint64_t* out, int32_t cap) {
  return guarded([&] {
    if (!out || cap <= 0) return 0;
    Device* d = nullptr; if (get_device(&d)) return 0;
    std::shared_ptr<PinnedOwner> keep; PinnedBases pb; if (find_bases(d, handle, &keep, &pb)) return 0;
    uint64_t v[8] = {pb.n, pb.n * (96 + ROW28) + (pb.d_inf ? pb.n : 0), 0, 0, 0, 0, 0, 0};
    int k = 0;
    for (const auto& t : pb.tab) if (t.d) { const uint64_t W = (254 + t.c - 1) / t.c; v[2] += W * t.cover * t.row; v[3 + k] = (uint64_t)t.c; ++k; }
    v[6] = (uint64_t)k;
    const int32_t m = cap < 8 ? cap : 8;
    for (int32_t i = 0; i < m; ++i) out[i] = v[i];
    return m;
  }, 0);
}

int32_t aleo_mi355x_bases_download(uint64_t handle, size_t offset, size_t n, void* out104) {
  return guarded([&] {
    if (!out104 && n) return ALEO_MI355X_ERR_BAD_ARG;
    Slot sl; if (sl.rc) return sl.rc;
    FoundBases fb(sl.d, handle); if (fb.rc) return fb.rc;
    if (offset + n > fb.pb.n) return bad_arg("bases_download: range");
    std::vector<uint8_t> xy(n * 96 + 1), inf(n + 1, 0);
    HIPCHK(hipMemcpy(xy.data(), (const char*)fb.pb.d_xy + offset * 96, n * 96, hipMemcpyDeviceToHost));
    if (fb.pb.d_inf) HIPCHK(hipMemcpy(inf.data(), fb.pb.d_inf + offset, n, hipMemcpyDeviceToHost));
    uint8_t* o = (uint8_t*)out104;
    for (size_t i = 0; i < n; ++i) { std::memcpy(o + i * 104, &xy[i * 96], 96); std::memset(o + i * 104 + 96, 0, 8); o[i * 104 + 96] = inf[i]; }
    return ALEO_MI355X_OK;
  });
}

int32_t aleo_mi355x_bases_unpin(uint64_t handle) {
  return guarded([&] { Slot sl; if (sl.rc) return sl.rc; return unpin(sl.d, sl.d->bases, handle, "unknown bases handle"); });
}

int32_t aleo_mi355x_bases_g2_pin(const void* bases, size_t base_stride, size_t n, uint64_t* handle) {
  return guarded([&] {
    if (!handle || (!bases && n) || (base_stride != 200 && base_stride != 192) || n >= (1ull << 31)) return bad_arg("bases_g2_pin: bad argument");
    Slot sl; if (sl.rc) return sl.rc;
    std::shared_ptr<PinnedG2> o;
    const int32_t rc = g2_upload(sl.c, bases, base_stride, n, &o);
    if (rc) return rc;
    *handle = register_set(sl.d, sl.d->g2_bases, std::move(o));
    return ALEO_MI355X_OK;
  });
}
int32_t aleo_mi355x_bases_g2_unpin(uint64_t handle) {
  return guarded([&] { Slot sl; if (sl.rc) return sl.rc; return unpin(sl.d, sl.d->g2_bases, handle, "unknown G2 bases handle"); });
}

}  // the entry points
