// msm_chain.h — the steps of ONE G1 launch chain (msm.hip) as msm_request.hip schedules them.
#pragma once
#include "msm_common.h"
#include <chrono>

namespace aleo_mi355x {
#pragma GCC visibility push(hidden)      // seams between the library's own units stay out of its dynamic symbol table
// The bucket sums earlier launch chains of the SAME request left behind (msm_run_chunked: one MSM whose scalars arrive in chunks, every chunk sorted and
// accumulated on its own, all chunks addressing the same buckets): newest first.  The first slice of bucket g in the current chunk starts from the newest
// earlier sum of g instead of from its own first point, so after the last chunk a bucket's total sits in the newest chunk that touched it.
struct FrontView { const char* partial; const uint32_t* hist; const uint2* scan_local; const uint2* scan_blk; };
struct FrontChain { FrontView v[3]; uint32_t n = 0; };
// One launch chain in steps, so that several chains — the chunks of one request whose scalars are still arriving — can share buckets and one
// bucket reduction (msm_run_chunked), or take turns under one host thread (run_chains_pipelined):
//   msm_front_sort    checks, plan, sort, slice ordering — everything queued, nothing waited for
//   msm_front_accum   the accumulation kernel (optionally behind an event, optionally seeded with the bucket sums of earlier chains)
//   msm_front_finish  the slice metadata arrives (pinned buffer), the slice trees follow: bucket b's sum is then the first slice of b
//   msm_reduce_queue / msm_collect   table path: the bucket reduction queued, ev[3] behind it / the wait for it, host tail, phase times
//   msm_back          the two back to back, or the plain path's reduction and host tail (msm_reduce.h msm_back_plain, which G2 runs too)
struct Front {
  MsmPlan P{}; SortPhase sp; SliceMeta sm;
  uint32_t K = 0, cpw = 0, nchunks = 0, lgN = 0, tseg = 0, fseg = 0, nseg = 0, setw = 0; size_t vpoints = 0;
  uint32_t out_pts = 0;      // result points per set the host tail reads: lgN + 1 from the sum trees (prog), lgN + 4 from the masked trees
  bool pre = false, masked = false, prog = false, aside = false, empty = false, lean = false, te = false; const char* bases = nullptr;      // te: the chain's tier is in Edwards form (msm_te.h)
       // lean: MsmJob::lean of a single-chain request (no phase-timing events)
  // plain path: the lane-pair slice-tree kernel over the group's partial sums (msm_reduce.h k_tree_pass<PT, 2>) — how the group reaches msm_front_finish
  void (*plain_tree)(char*, const uint32_t*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t, const uint2*, const uint2*, uint32_t, const uint32_t*, uint32_t, uint32_t) = nullptr;
};
// Work queued on borrowed contexts must have finished before their locks are released, whatever way the function is left (an early HIPCHK return, an
// exception on its way to the C ABI's catch): the guard synchronises the listed streams in its destructor unless the normal path — which ends
// synchronised anyway — dismissed it.
struct StreamDrainGuard {
  std::vector<hipStream_t> streams; bool armed = true;
  ~StreamDrainGuard() { if (!armed) return; const std::string keep = g_last_error; for (hipStream_t st : streams) if (st) (void)hipStreamSynchronize(st); g_last_error = keep; }
  void add(hipStream_t st) { streams.push_back(st); }
  void dismiss() { armed = false; }
};
int32_t msm_front_sort(Ctx* c, const PinnedBases& pb, const MsmJob& job, hipStream_t s, Front& f);
// seed: bucket sums of the request's earlier chunks (table path only), complete once `after` has been reached
int32_t msm_front_accum(Ctx* c, hipStream_t s, Front& f, const FrontChain* seed, hipEvent_t after);
int32_t msm_front_finish(Ctx* c, hipStream_t s, Front& f, bool allow_aside);
// older: the earlier chunks of the same request (msm_run_chunked) — a bucket this chain did not touch keeps its sum there.
int32_t msm_reduce_queue(Ctx* c, Front& f, hipStream_t s, const FrontChain& older);
// What msm_collect (and so msm_back) returns when an addition of an Edwards-tier chain reported Z3 == 0 — bases outside the prime-order subgroup: the results are
// not written and msm_request.hip reruns the request without the tables.  Never leaves the library.
static constexpr int32_t MSM_RERUN_WITHOUT_TABLES = -1000;
enum class TailWait { stream, event };      // without a hook the host waits for the whole stream, or for ev[3] alone (other chains' work may be queued behind it; this chain's is all in front)
int32_t msm_collect(Ctx* c, uint64_t* out_jac18, Front& f, hipStream_t s, bool fire_tail, TailWait wait);
int32_t msm_back(Ctx* c, uint64_t* out_jac18, Front& f, hipStream_t s, bool fire_tail, const FrontChain& older);
// phase times of a G1 chain into Ctx::last_msm / g_last_msm: HIP events on the launch stream up to the result's arrival (ev[3], already complete: the host has
// waited for it), the host tail by the host clock — no further event round trip on the critical path of a small MSM
int32_t phase_times(Ctx* c, const Front& f, std::chrono::steady_clock::time_point t_host0);
#pragma GCC visibility pop
}  // namespace aleo_mi355x
