// msm_request.hip — which launch chains a G1 multi-scalar multiplication request becomes, and where they run.  Host code only: the steps of one
// chain are msm.hip's (msm_chain.h), the table tiers and their set capacities msm_sort.hip's (msm_common.h).
#include "host_field.hpp"
#include "msm_chain.h"
#include <cstring>
#include <thread>

namespace aleo_mi355x {

static void identity_results(uint64_t* out_jac18, size_t k, const uint32_t* where = nullptr) {      // an empty chain's results are the identity: result q of k at 18 * where[q] (or 18 * q)
  for (size_t q = 0; q < k; ++q) host::hstore_jacobian_normalized(out_jac18 + 18 * (size_t)(where ? where[q] : q), host::HXYZZ::infinity());
}

// Requests with the scalars already on the device run whole.  In chunks (the sort of the later chunks beside the accumulation of the earlier ones instead of
// in front of everything) they measured slower (round 4, resident uniform scalars, whole / chunked): 2^20 2.82 / 3.03 ms, 2^21 5.12 / 5.24, 2^22 9.41 / 9.51 —
// without an upload to hide, the seeded launches (+5 % accumulation time: shorter slices, a seed read and a product per bucket) and the sort that crawls
// beside an accumulation holding every wave slot cost more than the 0.3-1.0 ms of sort they move out of the way; holding a later chunk's sort until the
// previous accumulation starts (as run_chains does for whole chains) makes it worse (2^20 3.07, 2^21 5.91, 2^22 9.83 ms against 2.83 / 5.04 / 9.32 whole:
// tools/resident_ab.py).
// A pinned set as the plain path sees it: the same points, no tables.  Where a chain on the Edwards tier reports Z3 == 0 (msm_chain.h MSM_RERUN_WITHOUT_TABLES: bases
// outside the prime-order subgroup, which the tier's unified law does not cover) the request is computed again against this view — every result on the plain path,
// whose XYZZ law handles any curve points.
static PinnedBases without_tables(const PinnedBases& pb) {
  PinnedBases plain = pb;
  for (auto& t : plain.tab) t = PinnedBases::PreTable();
  plain.range = PinnedBases::PreTable(); plain.range_off = 0; plain.tabled = false; plain.shards = 0;
  return plain;
}
static int32_t msm_batch_tiers(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s);
static int32_t msm_run_tiers(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s);
int32_t msm_run(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s) {
  const int32_t rc = msm_run_tiers(c, out_jac18, pb, job, s);
  if (rc != MSM_RERUN_WITHOUT_TABLES) return rc;
  MsmJob again = job; again.fire_tail = false; again.tier_n = 0;
  return msm_batch_tiers(c, out_jac18, without_tables(pb), again, s);      // (one chain per result: the plain path holds one)
}
static int32_t msm_run_tiers(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s) {
  if (job.k == 0) return ALEO_MI355X_OK;
  Front f; int32_t rc;
  f.lean = job.lean;
  if ((rc = msm_front_sort(c, pb, job, s, f))) return rc;
  if (f.empty) { identity_results(out_jac18, job.k); return ALEO_MI355X_OK; }
  if ((rc = msm_front_accum(c, s, f, nullptr, nullptr))) return rc;
  if ((rc = msm_front_finish(c, s, f, true))) return rc;
  return msm_back(c, out_jac18, f, s, job.fire_tail, FrontChain{});
}

// ONE result from HOST scalars, uploaded and processed in Q chunks that share the buckets and one bucket reduction.  The upload (32 bytes per scalar at the
// link's rate: 0.6 ms of a 3.5 ms call at 2^20) cannot hide under the sort of the same scalars, but a later chunk's upload and sort can run under an
// earlier chunk's accumulation.  Chunk k goes up and through its own sort on its own context (chunk 0 on the caller's, the others on borrowed ones,
// on their high-priority streams: their sorts must get workgroups in while an accumulation fills the chip); its accumulation starts when chunk k - 1's
// bucket sums are final and is SEEDED with them (k_accum28<.., SEED>: the first slice of a bucket continues from the newest earlier sum of that bucket),
// so after the last chunk every bucket's total sits in the newest chunk that touched it and ONE reduction (+ host tail) follows, reading through the
// chain.  All chunks use the window of the whole request.  The chunks grow — each must hide its upload + sort under its predecessor's accumulation,
// which costs ~ 3x as much per point: 2 chunks of 37 / 63 % up to 2^20 points, 3 of 18 / 30 / 52 % beyond.  A copy from pageable memory keeps the calling
// thread inside the runtime until the bytes are staged, so the order of the calls below IS the schedule: copy, launches, next copy.
// Measured (2^20 points, host scalars, wall per call; one whole upload: 3.50 ms): this form 3.23 (2^21: 6.51 -> 5.49, 2^22: 12.37 -> 9.84 with three chunks);
// two halves with a merge kernel (2^19 lane-pair additions into a dense array) before the reduction 3.28; the copies from a thread of their own: no
// change; every kernel on ONE stream with only the copies beside it 3.74 — each extra sort costs ~0.17 ms of dependent ~10 us launches when nothing
// hides it.  What is left on the table: a sort queued beside an accumulation that holds every wave slot (248 VGPRs x 2 waves per SIMD, workgroups that
// live ~250 us) takes ~0.5 ms instead of 0.15, so the next accumulation starts ~0.2 ms late.  CU-masked streams do not recover it (hipExtStreamCreateWithCUMask,
// profiles/r04_chunk_cumask_ab.jsonl): sorts confined to 16-64 reserved CUs are 4-8x slower (2^20: 4.5 / 3.8 / 3.4 ms with 16 / 32 / 64 CUs against 3.26), and
// keeping the accumulations off 8-32 CUs while the sorts run anywhere changes nothing at 2^20 and costs 5-8 % beyond.
// (Round 3 ran two halves as two complete MSMs on two host threads: that paid the 0.4 ms bucket reduction twice and lost below 2^21 points.)
// First-chunk share re-measured on the one-launch slice ordering (msm_sort.hip k_slice_order; wall ms per call, bench steps of 20, the three builds alternated, two boxes;
// profiles/r06_sort_chain_ab.txt):   2^20, 7 runs each:  30 % 2.857-2.928 (median 2.884) | 33 % 2.807-2.983 (2.868) | 37 % 2.820-2.966 (2.917)
//                                    2^19, 3 runs each:  30 % 1.790-1.853 (1.790)       | 33 % 1.800-1.825 (1.809) | 37 % 1.785-1.868 (1.790)
// The medians differ by <= 0.05 ms where one share's own runs spread over 0.07-0.18: inside the noise, 37 / 63 stays.  The three-chunk split at 2^21 was not re-measured.
static int32_t msm_run_chunked(Ctx* c, HelperSet& hs, uint64_t* out_jac18, const PinnedBases& pb, size_t n, bool mont, hipStream_t s, const void* host_src) {
  const uint32_t Q = 1 + (uint32_t)hs.ctx.size();           // 2 or 3
  static const uint32_t share[4][3] = {{0, 0, 0}, {0, 0, 0}, {37, 63, 0}, {18, 30, 52}};
  Ctx* cx[3] = {c, Q > 1 ? hs.ctx[0] : nullptr, Q > 2 ? hs.ctx[1] : nullptr}; hipStream_t st[3] = {s, Q > 1 ? hs.ctx[0]->hi : nullptr, Q > 2 ? hs.ctx[1]->hi : nullptr};
  StreamDrainGuard guard; for (uint32_t k = 0; k < Q; ++k) { guard.add(st[k]); guard.add(cx[k]->side); }      // drains them on every early return below
  size_t lo[4] = {0, 0, 0, 0};
  for (uint32_t k = 0, acc = 0; k < Q; ++k) { acc += share[Q][k]; lo[k + 1] = k + 1 == Q ? n : (((size_t)((double)n * acc / 100.0)) + 255) & ~(size_t)255; if (lo[k + 1] > n) lo[k + 1] = n; }
  Front f[3]; MsmSeg seg[3]; int32_t rc;
  auto view = [&](uint32_t k) { return FrontView{cx[k]->partial.as<char>(), f[k].sp.hist, f[k].sp.scan_local, f[k].sp.scan_blk}; };
  auto chain_before = [&](uint32_t k) { FrontChain ch; for (uint32_t i = k; i-- > 0;) ch.v[ch.n++] = view(i); return ch; };      // newest first
  for (uint32_t k = 0; k < Q; ++k) {
    MsmJob j; j.mont = mont; j.tier_n = n; j.k = 1;
    const size_t len = lo[k + 1] - lo[k];
    if ((rc = cx[k]->scalars_stage.reserve((len ? len : 1) * 32))) return rc;
    if (hipMemcpyAsync(cx[k]->scalars_stage.p, (const char*)host_src + lo[k] * 32, len * 32, hipMemcpyHostToDevice, st[k]) != hipSuccess) { g_last_error = "msm: upload of a chunk failed"; return ALEO_MI355X_ERR_HIP; }
    seg[k].d_ptr = cx[k]->scalars_stage.p; seg[k].len = len; seg[k].off = lo[k];
    j.segs = &seg[k]; j.nseg = 1;
    if ((rc = msm_front_sort(cx[k], pb, j, st[k], f[k]))) return rc;
    if (f[k].empty || !f[k].masked || f[k].P.c != f[0].P.c || f[k].sp.M != f[0].sp.M) { g_last_error = "msm: internal: chunks without a shared table window"; return ALEO_MI355X_ERR_HIP; }
    if (k) { if ((rc = msm_front_finish(cx[k - 1], st[k - 1], f[k - 1], false))) return rc; }      // chunk k - 1's slice trees: its bucket sums are final at its ev[2]
    const FrontChain seed = chain_before(k);
    if ((rc = msm_front_accum(cx[k], st[k], f[k], &seed, k ? cx[k - 1]->ev[2] : nullptr))) return rc;
  }
  if ((rc = msm_front_finish(cx[Q - 1], st[Q - 1], f[Q - 1], false))) return rc;
  // the reduction runs where the newest sums are; it synchronises that stream, behind which (event by event) every earlier chunk has finished
  if ((rc = msm_back(cx[Q - 1], out_jac18, f[Q - 1], st[Q - 1], false, chain_before(Q - 1)))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  MsmTiming tm = cx[Q - 1]->last_msm; float ms = 0, kern = 0;
  for (uint32_t k = 0; k < Q; ++k) { HIPCHK(hipEventElapsedTime(&ms, cx[k]->ev[6], cx[k]->ev[5])); kern += ms; }
  tm.accum_kernel = kern / Q; tm.accum_launches = (int)Q;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); tm.sort = ms;                        // the first chunk's sort: the one nothing hides
  HIPCHK(hipEventElapsedTime(&ms, c->ev[1], cx[Q - 1]->ev[2])); tm.accum = ms;               // from there to the last chunk's final bucket sums
  tm.total = tm.sort + tm.accum + tm.reduce + tm.host;
  c->last_msm = tm; g_last_msm = tm;
  guard.dismiss();
  return ALEO_MI355X_OK;
}

// The launch chains of one request.  One chain: on the caller's slot and stream.  Several big ones: dealt to two host threads — the caller's on its
// slot, one more on a borrowed helper context (own stream and workspaces) — so that the sort, reduction and host tail of one chain run under the
// accumulation of the other (the accumulation is bound by VALU issue, the sort by memory: `concurrent_callers` in the bench line is the same effect
// across calls).  The helper stream waits for an event recorded on `s` first (the scalars may still be in flight there); both threads return
// with their streams drained, so the caller sees the usual synchronous call.
namespace {
struct Chain { std::vector<MsmSeg> segs; std::vector<uint32_t> results; size_t points = 0; bool sparse = false, fire_tail = false; };
void scatter_results(uint64_t* out_jac18, const Chain& ch, const uint64_t* res) {      // a chain's results (res, in chain order) to their places in the request's output
  for (size_t q = 0; q < ch.results.size(); ++q) std::memcpy(out_jac18 + 18 * (size_t)ch.results[q], res + 18 * q, 144);
}
}
// The pipelined form (round 4; the two host threads above remain for requests with a chain off the table tiers).  A 2^20-constraint proof showed what the two threads leave on
// the table (profiles/r04_varuna_2^20_timeline_two_threads.txt): both chains of a round sort first (2.6 ms with no accumulation running), then their accumulations
// share the chip, then both reductions trail — 28 of 80 ms per proof with no accumulation kernel on the card.  Here ONE host thread queues the chains so that
// the accumulations run back to back and everything else runs beside them:
//   chain i on context i mod R (R = 3: the caller's and two borrowed ones): sort + slice ordering on the context's HIGH-priority stream, the accumulation on
//   its normal-priority stream behind the previous chain's accumulation, slice trees + bucket reduction on the high-priority stream again.  Before the
//   host queues the sort of chain i + 1 it collects chain i + 1 - R (waits for its reduction; Horner, normalisation), whose context it takes over.  With
//   R = 3 that reduction ran beside accumulation i - 1, so sort i + 1 is queued when accumulation i starts and has all of it to finish; with R = 2 the
//   host would wait for reduction i - 1, which crawls beside accumulation i (an accumulation holds every wave slot: a 512-thread k_prog_final block waits
//   milliseconds for a whole CU to drain), and sort i + 1 would run exposed after it — measured: 1.3 ms gaps between the accumulations of an
//   8-instance round.
static int32_t run_chains_pipelined(Ctx* c, const std::vector<Ctx*>& helpers, uint64_t* out_jac18, const PinnedBases& pb, std::vector<Chain>& chains, bool mont, hipStream_t s) {
  auto SS = [&](Ctx* x) { return x->aux; };                 // the chains' sorts and reductions: normal priority (rounds 3-4 put them on the high-priority streams)
  const size_t n = chains.size(), R = 1 + helpers.size();   // a ring of R contexts: chain i on context i mod R
  std::vector<Ctx*> cx(R); std::vector<hipStream_t> acc_st(R);
  cx[0] = c; acc_st[0] = s; for (size_t k = 1; k < R; ++k) { cx[k] = helpers[k - 1]; acc_st[k] = helpers[k - 1]->stream; }
  StreamDrainGuard guard; for (size_t k = 0; k < R; ++k) { guard.add(SS(cx[k])); guard.add(acc_st[k]); guard.add(cx[k]->side); }      // also on an exception or an early return below
  std::vector<Front> f(n); std::vector<MsmJob> job(n); std::vector<char> live(n, 0);
  HIPCHK(hipEventRecord(c->ev[4], s));                       // the scalars may still be in flight on the caller's stream
  for (size_t k = 0; k < R; ++k) { HIPCHK(hipStreamWaitEvent(SS(cx[k]), c->ev[4], 0)); if (k) HIPCHK(hipStreamWaitEvent(acc_st[k], c->ev[4], 0)); }
  int32_t rc;
  auto sort_of = [&](size_t i) -> int32_t {
    Chain& ch = chains[i]; MsmJob& g = job[i];
    g.segs = ch.segs.data(); g.nseg = (uint32_t)ch.segs.size(); g.k = (uint32_t)ch.results.size(); g.mont = mont; g.sparse = ch.sparse; g.fire_tail = false;
    Ctx* cc = cx[i % R];
    const int32_t r = msm_front_sort(cc, pb, g, SS(cc), f[i]);
    if (r) return r;
    if (f[i].empty) { identity_results(out_jac18, ch.results.size(), ch.results.data()); return ALEO_MI355X_OK; }
    if (!f[i].masked) { g_last_error = "msm: internal: a pipelined chain without a table tier"; return ALEO_MI355X_ERR_HIP; }
    live[i] = 1;
    HIPCHK(hipEventRecord(cc->ev_hop, SS(cc)));
    return ALEO_MI355X_OK;
  };
  auto collect = [&](size_t i) -> int32_t {
    if (!live[i]) return ALEO_MI355X_OK;
    uint64_t res[MAX_SETS * 18]; Ctx* cc = cx[i % R];
    const int32_t r = msm_collect(cc, res, f[i], SS(cc), false, TailWait::event);
    if (r) return r;
    scatter_results(out_jac18, chains[i], res);
    live[i] = 0;
    return ALEO_MI355X_OK;
  };
  if ((rc = sort_of(0))) return rc;
  hipEvent_t prev_accum = nullptr; size_t collected = 0;     // chains [0, collected) are done
  for (size_t i = 0; i < n; ++i) {
    Ctx* cc = cx[i % R]; hipStream_t as = acc_st[i % R];
    if (live[i]) {
      HIPCHK(hipStreamWaitEvent(as, cc->ev_hop, 0));
      if ((rc = msm_front_accum(cc, as, f[i], nullptr, prev_accum))) return rc;
      prev_accum = cc->ev[5];
    }
    if (i + 1 < n) {
      for (; collected + R <= i + 1; ++collected) if ((rc = collect(collected))) return rc;       // the context of chain i + 1 must be free: chain i + 1 - R collected
      if (live[i]) HIPCHK(hipStreamWaitEvent(SS(cx[(i + 1) % R]), cc->ev[6], 0));      // not before accumulation i starts: two sorts side by side only delay the first accumulation
      if ((rc = sort_of(i + 1))) return rc;
    }
    if (live[i]) {
      HIPCHK(hipStreamWaitEvent(SS(cc), cc->ev[5], 0));
      if ((rc = msm_front_finish(cc, SS(cc), f[i], true))) return rc;
      if ((rc = msm_reduce_queue(cc, f[i], SS(cc), FrontChain{}))) return rc;
    }
  }
  for (; collected < n; ++collected) if ((rc = collect(collected))) return rc;
  return ALEO_MI355X_OK;
}
static int32_t run_chains(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, std::vector<Chain>& chains, bool mont, hipStream_t s, bool lean = false) {
  bool lean_now = false;                                    // chains run one after another on the caller's context keep MsmJob::lean; overlapped / pipelined chains order themselves by the phase events
  auto run_one = [&](Ctx* cc, Chain& ch, hipStream_t st) -> int32_t {
    uint64_t res[MAX_SETS * 18];
    MsmJob g; g.segs = ch.segs.data(); g.nseg = (uint32_t)ch.segs.size(); g.k = (uint32_t)ch.results.size(); g.mont = mont; g.sparse = ch.sparse; g.fire_tail = ch.fire_tail; g.lean = lean_now;
    const int32_t rc = msm_run(cc, res, pb, g, st);
    if (rc) return rc;
    scatter_results(out_jac18, ch, res);
    return ALEO_MI355X_OK;
  };
  size_t total = 0; for (auto& ch : chains) total += ch.points;
  HelperSet hs;
  if (chains.size() >= 2 && total >= ((size_t)1 << 20) && c->dev) { const int32_t rc = acquire_helpers(c->dev, chains.size() >= 3 ? 2 : 1, hs); if (rc) return rc; }
  if (hs.ctx.empty()) { lean_now = lean; for (auto& ch : chains) { const int32_t rc = run_one(c, ch, s); if (rc) return rc; } return ALEO_MI355X_OK; }
  Ctx* h = hs.ctx[0];
  bool all_tiered = true;                                   // every chain on a table tier (the grouping of msm_batch makes them so, except the tier-less singles)
  for (auto& ch : chains) {
    size_t reach = 0; for (auto& g : ch.segs) if (g.len) reach = g.off + g.len > reach ? g.off + g.len : reach;
    bool t_ok = reach == 0;                                 // (an empty chain: its results are the identity)
    if (reach && msm_tier(pb, reach)) t_ok = ch.results.size() <= 1 || ch.results.size() <= msm_max_sets(pb, reach);
    all_tiered = all_tiered && t_ok && ch.results.size() <= MAX_SETS;
  }
  if (all_tiered) return run_chains_pipelined(c, hs.ctx, out_jac18, pb, chains, mont, s);
  HIPCHK(hipEventRecord(c->ev[4], s));                     // ev[4] is free until this chain's own msm_run (which may use it for its aside trees) starts
  HIPCHK(hipStreamWaitEvent(h->stream, c->ev[4], 0));
  std::atomic<size_t> next{0}; int32_t rc_h = ALEO_MI355X_OK; std::string err_h; MsmTiming tm_h{};
  std::thread helper([&] {
    if (hipSetDevice(c->device) != hipSuccess) { rc_h = ALEO_MI355X_ERR_HIP; err_h = "hipSetDevice failed"; return; }
    try {
      for (size_t i; (i = next.fetch_add(1)) < chains.size();) { const int32_t rc = run_one(h, chains[i], h->stream); if (rc) { rc_h = rc; err_h = g_last_error; return; } }
    } catch (...) { rc_h = ALEO_MI355X_ERR_HIP; err_h = "msm: exception on the helper thread"; }
    tm_h = h->last_msm;
  });
  int32_t rc_m = ALEO_MI355X_OK;
  try { for (size_t i; !rc_m && (i = next.fetch_add(1)) < chains.size();) rc_m = run_one(c, chains[i], s); }
  catch (...) { rc_m = ALEO_MI355X_ERR_HIP; g_last_error = "msm: exception on the calling thread"; next.store(chains.size()); }      // never unwind past the joinable helper
  helper.join();
  (void)hipStreamSynchronize(h->stream);
  if (rc_m) return rc_m;
  if (rc_h) { g_last_error = err_h; return rc_h; }
  return ALEO_MI355X_OK;
}

// One result over n points.  Scalars already on the device: one launch chain.  HOST scalars against a table tier, from 2^MERGE_MIN_LG points: two (three
// from 2^CHUNKS3_MIN_LG) chunks on as many contexts that share the buckets and one bucket reduction (msm_run_chunked) — most of the upload disappears under
// the earlier chunks' kernels (measurements at msm_run_chunked).  Smaller or table-less requests upload whole.
static constexpr uint32_t MERGE_MIN_LG = 19, CHUNKS3_MIN_LG = 21;
int32_t msm_run1_split(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const void* d_scalars, size_t n, bool mont, hipStream_t s, bool sparse, const void* host_src, bool may_merge) {
  const bool tiered = msm_tier(pb, n) != nullptr;
  HelperSet hs;
  if (host_src && may_merge && !sparse && tiered && n >= ((size_t)1 << MERGE_MIN_LG) && c->dev) { const int32_t rc = acquire_helpers(c->dev, n >= ((size_t)1 << CHUNKS3_MIN_LG) ? 2 : 1, hs); if (rc) return rc; }
  if (!hs.ctx.empty()) {
    const int32_t rc = msm_run_chunked(c, hs, out_jac18, pb, n, mont, s, host_src);
    if (rc != MSM_RERUN_WITHOUT_TABLES) return rc;
    hs = HelperSet();                                      // the borrowed contexts go back; the rerun uploads whole
    return msm_run1_split(c, out_jac18, without_tables(pb), d_scalars, n, mont, s, sparse, host_src, false);
  }
  if (host_src) {
    const int32_t rc = c->scalars_stage.reserve((n ? n : 1) * 32); if (rc) return rc;
    if (n) HIPCHK(hipMemcpyAsync(c->scalars_stage.p, host_src, n * 32, hipMemcpyHostToDevice, s));
    d_scalars = c->scalars_stage.p;
  }
  return msm_run1(c, out_jac18, pb, d_scalars, n, mont, s, sparse);
}

// Cuts the results `ids` (taken in order) into launch chains of at most `cap` results, 2^26 points (2^32 pairs) and MAX_SEGS segments.  A chain's
// segments keep the request's order, `out` relabelled to the chain-local index of the result.  fire_tail: every result of the request in this one chain.
static int32_t cut_chains(const MsmJob& job, const std::vector<uint32_t>& ids, const std::vector<size_t>& points, const std::vector<uint32_t>& nsegs, size_t cap, bool sparse, std::vector<Chain>& chains) {
  for (size_t pos = 0; pos < ids.size();) {
    size_t take = 0, pts = 0, sg = 0;
    while (pos + take < ids.size() && take < cap && (take == 0 || (pts + points[ids[pos + take]] <= ((size_t)1 << 26) && sg + nsegs[ids[pos + take]] <= MAX_SEGS))) {
      pts += points[ids[pos + take]]; sg += nsegs[ids[pos + take]]; ++take;
    }
    if (sg > MAX_SEGS) { g_last_error = "msm: one result with more than 64 segments"; return ALEO_MI355X_ERR_BAD_ARG; }
    chains.emplace_back(); Chain& ch = chains.back(); ch.segs.reserve(sg); ch.points = pts; ch.sparse = sparse; ch.fire_tail = take == job.k;
    for (size_t i = 0; i < take; ++i) ch.results.push_back(ids[pos + i]);
    for (uint32_t q = 0; q < job.nseg; ++q) {
      const MsmSeg& g = job.segs[q];
      if (!g.len) continue;
      for (size_t i = 0; i < take; ++i) if (ch.results[i] == g.out) { MsmSeg h = g; h.out = (uint32_t)i; ch.segs.push_back(h); break; }
    }
    pos += take;
  }
  return ALEO_MI355X_OK;
}

// Arbitrary request: k results, each the sum of its segments.  Results are grouped by the table tier the bases they reach select
// (longest tier first) and every group goes through msm_run in chunks of msm_max_sets() results / MAX_SEGS segments; results no tier
// serves (no table, or fewer than 2^10 bases reached) run one by one.
int32_t msm_batch(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s) {
  const int32_t rc = msm_batch_tiers(c, out_jac18, pb, job, s);
  return rc == MSM_RERUN_WITHOUT_TABLES ? msm_batch_tiers(c, out_jac18, without_tables(pb), job, s) : rc;
}
static int32_t msm_batch_tiers(Ctx* c, uint64_t* out_jac18, const PinnedBases& pb, const MsmJob& job, hipStream_t s) {
  const uint32_t K = job.k;
  auto tier_of = [&](size_t n) { const PinnedBases::PreTable* t = msm_tier(pb, n); return t ? (int)(t - pb.tab) : -1; };
  std::vector<size_t> reach(K, 0), points(K, 0); std::vector<uint32_t> nsegs(K, 0);
  for (uint32_t q = 0; q < job.nseg; ++q) {
    const MsmSeg& g = job.segs[q];
    if (g.out >= K) { g_last_error = "msm: segment names a result that does not exist"; return ALEO_MI355X_ERR_BAD_ARG; }
    if (!g.len) continue;
    reach[g.out] = g.off + g.len > reach[g.out] ? g.off + g.len : reach[g.out]; points[g.out] += g.len; nsegs[g.out]++;
  }
  // Sparse hint + a range table that holds every segment: chains of up to its set capacity, whatever the reach (the table is indexed from range_off)
  if (job.sparse && pb.range.d) {
    bool inside = true;
    for (uint32_t q = 0; q < job.nseg && inside; ++q) { const MsmSeg& g = job.segs[q]; if (g.len) inside = g.off >= pb.range_off && g.off + g.len <= pb.range_off + pb.range.cover; }
    if (inside) {
      std::vector<uint32_t> all(K); for (uint32_t q = 0; q < K; ++q) all[q] = q;
      std::vector<Chain> chains;
      if (const int32_t rc = cut_chains(job, all, points, nsegs, msm_range_sets(pb), true, chains)) return rc;
      return run_chains(c, out_jac18, pb, chains, job.mont, s, job.lean);
    }
  }
  // Latency-bound requests (one prover round: a few results of <= 2^17 points each): ONE launch chain on the tier that covers the
  // longest reach beats one chain per tier — a second chain costs ~0.45 ms of dependent steps, a wider window than a short member
  // would have picked costs nothing measurable at these sizes.
  {
    size_t far = 0, pts = 0, sg = 0;
    for (uint32_t q = 0; q < K; ++q) { far = reach[q] > far ? reach[q] : far; pts += points[q]; sg += nsegs[q]; }
    if (K > 1 && K <= MAX_SETS && tier_of(far) >= 0 && K <= msm_max_sets(pb, far) && pts <= ((size_t)1 << 21) && sg <= MAX_SEGS) {
      bool split = false;
      for (uint32_t q = 0; q < K; ++q) if (points[q] && tier_of(reach[q]) != tier_of(far)) split = true;
      if (split) {
        std::vector<MsmSeg> segs; segs.reserve(sg);
        for (uint32_t q = 0; q < job.nseg; ++q) if (job.segs[q].len) segs.push_back(job.segs[q]);
        MsmJob g; g.segs = segs.data(); g.nseg = (uint32_t)segs.size(); g.k = K; g.mont = job.mont; g.fire_tail = true; g.lean = job.lean;
        return msm_run(c, out_jac18, pb, g, s);
      }
    }
  }
  std::vector<uint32_t> todo; todo.reserve(K); std::vector<Chain> chains;
  for (int t = -1; t < 3; ++t) {
    todo.clear();
    for (uint32_t q = 0; q < K; ++q) if (tier_of(reach[q]) == t) todo.push_back(q);
    if (todo.empty()) continue;
    const size_t cap = t < 0 ? 1 : msm_max_sets(pb, reach[todo[0]]);      // (chains of one set instead of two for the pipeline of run_chains: measured slower, 8 x 2^20 constraints 155 -> 160 ms)
    if (const int32_t rc = cut_chains(job, todo, points, nsegs, cap, false, chains)) return rc;
  }
  return run_chains(c, out_jac18, pb, chains, job.mont, s, job.lean);
}

}  // namespace aleo_mi355x
