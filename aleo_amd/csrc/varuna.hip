// varuna.hip — the host side of one proof, native: the four AHP rounds, the evaluations and the two openings of `Varuna::prove_batch` (up to 32
// instances in any split over circuits) as ONE call of the C ABI (`aleo_mi355x_varuna_prove[_batch_indexed]`).  This file: the routed transforms and
// commitments, the prover's memory, the schedule and its one driver; varuna_rounds.hip, varuna_proof.hip, varuna_index.hip: what their names say.
//
// Replaces (shape, not bytes — see DESIGN.md §4d for what differs from upstream and why) snarkVM 0.14.5
//   algorithms/src/snark/varuna/varuna.rs                      Varuna::prove_batch
//   algorithms/src/snark/varuna/ahp/prover/round_functions/*   AHPForR1CS::prover_{first,second,third,fourth}_round   [UPSTREAM-RECALL]
// reached from the reference's rust/src/program/execute.rs:74 (`trace.prove_execution`) and transfer.rs:99.
// Every circuit-sized step is a kernel of msm_sort.hip / msm.hip / ntt.hip / frops.hip / fr_spmv.hip / fr_divide.hip / ahp_kernels.hip queued on the calling slot's stream; these files keep what
// upstream keeps on the CPU between them: the Fiat-Shamir transcript (upstream's Poseidon sponge over Fq, poseidon.hpp), the
// challenge-dependent constants (host Fr arithmetic, host_field.hpp), the blinding scalars (ChaCha20 under the proof's 32-byte seed, chacha.h)
// and the O(|X|) public-input polynomial.  aleo_amd/varuna.py is the same sequence written against the public entry points; both
// must produce the bytes of the restatement in oracle/varuna_ref.py (tests/test_varuna.py).
#include "varuna_host.h"
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

namespace aleo_mi355x {

thread_local double g_varuna_timing[8] = {};

// The prover's transforms.  With a sharded copy of the committer key attached (row e2: a proof that spans devices) a transform of >= shard_ntt_min elements (default 2^24, aleo_mi355x_bases_shard_transforms) runs over
// the devices the key is spread over (sharded.hip ntt_sharded_device: slabs pulled and pushed by peer copies, the coefficient vector stays on the prover's device
// between the rounds) — the "NTT coefficients" half of north_star's "large proofs shard MSM bases and NTT coefficients"; everything else, and any device list
// that is not a power of two, takes the single-device kernels.  Same values either way (tests: proofs byte-equal).
static bool ntt_routed(const PinnedBases& pb, uint32_t lg, std::vector<int>* devs) {
  if (!pb.shards || lg < 2 || ((size_t)1 << lg) < pb.shard_ntt_min) return false;
  if (sharded_devices(pb.shards, devs)) return false;
  const size_t G = devs->size();
  return G >= 1 && !(G & (G - 1)) && lg / 2 >= lg2(G);
}
int32_t p_ntt(Ctx* c, const PinnedBases& pb, void* data, uint32_t lg, size_t batch, int32_t direction, int32_t type, hipStream_t s) {
  std::vector<int> devs;
  if (!ntt_routed(pb, lg, &devs)) return ntt_run(c, data, lg, batch, ALEO_NTT_ORDER_NN, direction, type, s);
  for (size_t b = 0; b < batch; ++b) { const int32_t rc = ntt_sharded_device(c, (char*)data + (b << lg) * 32, lg, direction, type, devs.data(), devs.size(), s); if (rc) return rc; }
  return ALEO_MI355X_OK;
}
int32_t p_ntt_from(Ctx* c, const PinnedBases& pb, void* out, const void* src, size_t src_stride, size_t src_len, uint32_t lg, size_t batch, hipStream_t s) {
  std::vector<int> devs;
  if (!ntt_routed(pb, lg, &devs)) return ntt_run_from(c, out, src, src_stride, src_len, lg, batch, ALEO_NTT_FORWARD, ALEO_NTT_STANDARD, s);
  const size_t n = (size_t)1 << lg;
  for (size_t b = 0; b < batch; ++b) {                        // pad by hand (sizes where a fill and a copy are noise), then the sharded transform in place
    char* o = (char*)out + b * n * 32;
    if (src_len < n) HIPCHK(hipMemsetAsync(o + src_len * 32, 0, (n - src_len) * 32, s));
    if (src_len) HIPCHK(hipMemcpyAsync(o, (const char*)src + b * src_stride * 32, src_len * 32, hipMemcpyDeviceToDevice, s));
    const int32_t rc = ntt_sharded_device(c, o, lg, ALEO_NTT_FORWARD, ALEO_NTT_STANDARD, devs.data(), devs.size(), s); if (rc) return rc;
  }
  return ALEO_MI355X_OK;
}


// `behind`: kernels of the NEXT round that need no challenge of this one — queued behind the commitment's last kernel, so that they run while the host finishes
// the MSM's tail, compresses, hashes and derives the challenge (Ctx::tail_hook; a request that takes several launch chains runs them afterwards instead).
int32_t commit(Ctx* c, const PinnedBases& pb, const std::vector<MsmSeg>& segs, uint32_t k, uint8_t* out104, hipStream_t s, bool sparse,
               std::function<int32_t()> behind) {
  std::vector<uint64_t> jac(18 * (size_t)k);
  MsmJob j; j.segs = segs.data(); j.nseg = (uint32_t)segs.size(); j.k = k; j.mont = true; j.sparse = sparse; j.lean = true;      // lean: no phase-timing events between the chain's kernels
  const double t0 = now_ms();
  size_t points = 0; for (const MsmSeg& g : segs) points += g.len;
  if (pb.shards && points >= pb.shard_min) {
    // a sharded copy of the committer key is attached (row e2: a proof that spans devices): the coefficient vectors stay here, every device pulls its
    // slices and runs its own Pippenger, 144 bytes per result and shard come back.  `s` is drained first (the scalars are complete), so the kernels of `behind` — which
    // only read what the commitment reads and write fresh arena blocks — are queued at once and run on this device beside its own shard.
    HIPCHK(hipStreamSynchronize(s));
    if (behind) RC(behind());
    RC(commit_sharded(c, pb.shards, segs.data(), (uint32_t)segs.size(), k, true, jac.data(), s, false));
  } else {
    struct Clear { Ctx* c; ~Clear() { c->tail_hook = nullptr; } } clear{c};      // whatever happens below, no hook (it captures this proof's state) outlives the call
    c->tail_hook = std::move(behind);
    const int32_t rc = msm_batch(c, jac.data(), pb, j, s);
    std::function<int32_t()> left = std::move(c->tail_hook); c->tail_hook = nullptr;
    if (rc) return rc;
    if (left) RC(left());
    g_varuna_timing[7] += c->last_msm.host;                  // the host tails of the commitment calls (last chain of each call)
  }
  jacobian_rows_to_affine104(out104, jac.data(), k);
  g_varuna_timing[6] += now_ms() - t0;                       // time inside the commitment calls
  return ALEO_MI355X_OK;
}
// The slot's grow-only device workspace and pinned staging, sized for `ws_bytes` / `pin_bytes` (one proof, or the sum over the proofs of a lockstep call)
static int32_t reserve_prover_memory(Ctx* c, size_t ws_bytes, size_t pin_bytes) {
  RC(c->prover_ws.reserve(ws_bytes));
  if (c->prover_pin_cap < pin_bytes) {
    if (c->prover_pin) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->prover_pin); c->prover_pin = nullptr; c->prover_pin_cap = 0; }
    HIPCHK(hipHostMalloc(&c->prover_pin, pin_bytes + pin_bytes / 8, hipHostMallocMapped)); c->prover_pin_cap = pin_bytes + pin_bytes / 8;      // mapped: kernels store small read-backs into it
  }
  return ALEO_MI355X_OK;
}
// The commitments of one round for every proof that is still alive: job q of all of them in ONE launch chain (the results of proof p follow those
// of proof p - 1), the hooks of all of them behind the last chain.  Proofs whose job lists differ in shape (one splits its first round into the
// sparse witness chain + the mask chain, another does not) cannot share: the caller (prove_many) falls back to one proof at a time.
static int32_t run_commits(Ctx* c, const PinnedBases& pb, std::vector<Batch*>& bs, hipStream_t s) {
  if (bs.empty()) return ALEO_MI355X_OK;
  const int nj = bs[0]->njobs;
  for (int q = 0; q < nj; ++q) {
    std::vector<MsmSeg> all; uint32_t k = 0; const bool sparse = bs[0]->job[q].sparse;
    for (Batch* b : bs) { for (MsmSeg sg : b->job[q].segs) { sg.out += k; all.push_back(sg); } k += b->job[q].k; }
    std::function<int32_t()> behind = nullptr;
    if (q == nj - 1) behind = [&bs]() -> int32_t { for (Batch* b : bs) if (b->hook) RC(b->hook()); return ALEO_MI355X_OK; };
    if (bs.size() == 1) { RC(commit(c, pb, all, k, bs[0]->job[q].out, s, sparse, std::move(behind))); continue; }
    std::vector<uint8_t> out((size_t)104 * k);
    RC(commit(c, pb, all, k, out.data(), s, sparse, std::move(behind)));
    size_t at = 0;
    for (Batch* b : bs) { std::memcpy(b->job[q].out, out.data() + 104 * at, (size_t)104 * b->job[q].k); at += b->job[q].k; }
  }
  return ALEO_MI355X_OK;
}

// The schedule of a proof, written once.  A round: prepare, the commitments (run_commits), finish (varuna_host.h); the openings queue their evaluations
// and drain the stream before they prepare, and what finishes them is the proof's bytes.  `name` labels the host trace.
struct Step { const char* name; int32_t (Batch::*queue_first)(); int32_t (Batch::*prepare)(); int32_t (Batch::*finish)(); };
static const Step SCHEDULE[] = {{"round 1", nullptr, &Batch::first_prepare, &Batch::first_finish},
                                {"round 2", nullptr, &Batch::second_prepare, &Batch::second_finish},
                                {"round 3", nullptr, &Batch::third_prepare, &Batch::third_finish},
                                {"round 4", nullptr, &Batch::fourth_prepare, &Batch::fourth_finish},
                                {"openings", &Batch::open_evaluate, &Batch::open_prepare, &Batch::write}};

// The driver of every entry point: n INDEPENDENT proofs in lockstep (aleo_mi355x_varuna_prove_many), n = 1 for the single-proof calls.  Every proof
// keeps its own transcript, challenges, randomness and workspace slice; what they share is every commitment launch chain (round r of all proofs is
// one batched MSM: its sort, slice tree, reduction, host tail and stream synchronisation are paid once, not once per proof).  Between the commitments
// the proofs are independent, so they are dealt to W worker threads (the caller's thread is worker 0; the others borrow helper contexts of the
// device: own stream, own scratch): the transcripts — host Poseidon, the serial part of a proof — run W at a time and the small field / NTT kernels of
// different proofs overlap on the card.  The workers meet at a barrier before and after each round's commitments, which worker 0 launches on the
// slot's stream behind an event of every helper stream.  A proof that fails (unsatisfied assignment, bad argument) drops out with its status; the
// others go on.  One proof, or one worker: no thread, no helper context, no event — the caller's thread walks the schedule on the slot's stream.
static int32_t prove_lockstep(Ctx* c, const PinnedBases& pb, ProveRequest* rq, size_t n, int workers) {
  g_varuna_timing[6] = g_varuna_timing[7] = 0;
  HT("prove: enter");
  hipStream_t s = c->stream;
  HelperSet hs;
  if (workers > 1 && n > 1) RC(acquire_helpers(c->dev, (int)std::min<size_t>(n, (size_t)workers) - 1, hs));
  std::vector<Ctx*> wc{c}; for (Ctx* h : hs.ctx) wc.push_back(h);
  const size_t W = wc.size();
  std::vector<std::unique_ptr<Batch>> B(n); std::vector<char> alive(n, 0);
  size_t ws_total = 0, pin_total = 0;
  for (size_t p = 0; p < n; ++p) {
    B[p].reset(new Batch(wc[p % W], pb, rq[p]));
    rq[p].status = B[p]->setup();
    if (rq[p].status) { rq[p].error = g_last_error; continue; }
    alive[p] = 1; ws_total += B[p]->need_ws_bytes; pin_total += B[p]->need_pin_bytes;
  }
  if (!ws_total) return ALEO_MI355X_OK;                      // no request passed its checks: each carries its status
  RC(reserve_prover_memory(c, ws_total, pin_total));
  size_t ws_at = 0, pin_at = 0;
  for (size_t p = 0; p < n; ++p) {
    if (!alive[p]) continue;
    RC(B[p]->attach((char*)c->prover_ws.p + ws_at, B[p]->need_ws_bytes, (char*)c->prover_pin + pin_at));
    ws_at += B[p]->need_ws_bytes; pin_at += B[p]->need_pin_bytes;
  }
  HT("prove: setup done");
  Barrier bar(W); int32_t fatal = ALEO_MI355X_OK; std::string fatal_error;      // fatal: written by worker 0 between two barriers, read by all after the second
  // the commitments of one round, by worker 0 while the others wait: the helper streams' events first (their kernels wrote this round's scalars)
  auto commits = [&]() -> int32_t {
    std::vector<Batch*> live; for (size_t p = 0; p < n; ++p) if (alive[p]) live.push_back(B[p].get());
    if (live.empty()) return ALEO_MI355X_OK;
    for (size_t w = 1; w < W; ++w) HIPCHK(hipStreamWaitEvent(s, wc[w]->ev[0], 0));
    bool uniform = true;
    for (Batch* b : live) { uniform = uniform && b->njobs == live[0]->njobs; for (int q = 0; uniform && q < b->njobs; ++q) uniform = b->job[q].sparse == live[0]->job[q].sparse; }
    if (uniform) return run_commits(c, pb, live, s);
    for (Batch* b : live) { std::vector<Batch*> one{b}; RC(run_commits(c, pb, one, s)); }      // mixed shapes: one proof at a time for this round
    return ALEO_MI355X_OK;
  };
  auto worker = [&](size_t w) {
    auto fail_mine = [&](int32_t rc, const char* why) { for (size_t p = w; p < n; p += W) if (alive[p]) { alive[p] = 0; rq[p].status = rc; rq[p].error = why; } };
    if (w && hipSetDevice(c->device) != hipSuccess) fail_mine(ALEO_MI355X_ERR_HIP, "hipSetDevice failed");
    hipStream_t sw = wc[w]->stream;
    // one step of this worker's live proofs; a failure removes the proof and records its status (alive[p] is only written by p's worker, and read by
    // worker 0 behind a barrier)
    auto each = [&](int32_t (Batch::*step)()) {
      for (size_t p = w; p < n; p += W) {
        if (!alive[p]) continue;
        int32_t rc;
        try { rc = (B[p].get()->*step)(); }
        catch (...) { rc = ALEO_MI355X_ERR_HIP; g_last_error = "varuna_prove_many: exception in a worker"; }      // never past the barrier protocol
        if (rc) { rq[p].status = rc; rq[p].error = g_last_error; alive[p] = 0; }
      }
    };
    for (const Step& st : SCHEDULE) {
      if (!w) HT(st.name);
      if (st.queue_first) { each(st.queue_first); if (hipStreamSynchronize(sw) != hipSuccess) fail_mine(ALEO_MI355X_ERR_HIP, "hipStreamSynchronize failed"); }
      each(st.prepare);
      if (!w) HT("prepared");
      if (w && hipEventRecord(wc[w]->ev[0], sw) != hipSuccess) fail_mine(ALEO_MI355X_ERR_HIP, "hipEventRecord failed");
      bar.wait();
      if (w == 0) { try { fatal = commits(); } catch (...) { fatal = ALEO_MI355X_ERR_HIP; g_last_error = "varuna_prove_many: exception in the commitments"; } if (fatal) fatal_error = g_last_error; }
      if (!w) HT("committed");
      bar.wait();
      if (fatal) return;
      each(st.finish);
      if (!w) HT("transcript");
    }
  };
  // Helper threads wait at a gate until all of them exist: if one cannot be started, the ones that were leave at once (the barrier counts W threads) and
  // the call fails as a whole instead of unwinding past joinable threads.
  std::vector<std::thread> th; th.reserve(W); std::mutex gate_mu; std::condition_variable gate_cv; int gate = 0;      // 0 wait, 1 go, -1 leave
  bool started = true;
  for (size_t w = 1; w < W && started; ++w) {
    try { th.emplace_back([&, w] { { std::unique_lock<std::mutex> g(gate_mu); gate_cv.wait(g, [&] { return gate != 0; }); if (gate < 0) return; } worker(w); }); }
    catch (...) { started = false; }
  }
  { std::lock_guard<std::mutex> g(gate_mu); gate = started ? 1 : -1; } gate_cv.notify_all();
  if (started) worker(0);
  for (auto& t : th) t.join();
  if (!started) { g_last_error = "varuna_prove_many: could not start a worker thread"; return ALEO_MI355X_ERR_HIP; }
  for (size_t w = 1; w < W; ++w) (void)hipStreamSynchronize(wc[w]->stream);      // nothing of this call is left on a helper stream when it goes back to the pool
  if (fatal) { g_last_error = fatal_error; return fatal; }
  if (g_host_trace_on) host_trace_mark(nullptr);
  return ALEO_MI355X_OK;
}

int32_t varuna_prove_many(Ctx* c, const PinnedBases& pb, std::vector<ProveRequest>& rq, int workers) {
  const double t0 = now_ms();
  if (workers <= 0) { workers = 4; if (const char* e = std::getenv("ALEO_MI355X_LOCKSTEP_WORKERS")) { const int k = std::atoi(e); if (k >= 1 && k <= MAX_SLOTS + 1) workers = k; } }
  RC(prove_lockstep(c, pb, rq.data(), rq.size(), workers));
  for (int i = 0; i < 5; ++i) g_varuna_timing[i] = 0;      // the rounds of the proofs interleave: only the call's total means something
  g_varuna_timing[5] = now_ms() - t0;
  return ALEO_MI355X_OK;
}

// One proof: a lockstep call of one request and one worker; its status and error text are the call's.
int32_t varuna_prove_batch(Ctx* c, const PinnedBases& pb, const aleo_mi355x_varuna_index* const* ixs, size_t m, const void* const* assignments, const size_t* ks,
                           const uint8_t* seed32, uint8_t* out, size_t* out_len) {
  ProveRequest rq; rq.ixs.assign(ixs, ixs + m); rq.assignments = assignments; rq.ks = ks; rq.seed32 = seed32; rq.out = out; rq.out_len = out_len;
  RC(prove_lockstep(c, pb, &rq, 1, 1));
  if (rq.status) g_last_error = rq.error;
  return rq.status;
}

}  // namespace aleo_mi355x
