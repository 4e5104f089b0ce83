// entry.h — what the units with entry points of the C ABI share (device.hip, bases.hip, sharded.hip, api.hip): the guard at the C boundary, the slot a call runs
// on, its stream, handle lookup, and the functions that cross between those four files.  (Kernels and their hosts: ctx.h.)
#pragma once
#include "ctx.h"
#include <cstdlib>

namespace aleo_mi355x {

// No exception crosses the C boundary: every entry point runs its body in here (on_throw: 0 for the *_info / *_timing functions, which return a count).
template <class F> int32_t guarded(F&& body, int32_t on_throw = ALEO_MI355X_ERR_HIP) { try { return body(); } catch (...) { return on_throw; } }

inline int32_t bad_arg(const char* why) { g_last_error = why; return ALEO_MI355X_ERR_BAD_ARG; }      // a refused argument and the text that says which

// A size from the environment, read per call: `dflt` where the variable is unset, empty or no decimal number.
inline size_t env_size(const char* name, size_t dflt) { const char* e = std::getenv(name); if (!e || !*e) return dflt; char* end = nullptr; const unsigned long long v = std::strtoull(e, &end, 10); return end && *end == 0 ? (size_t)v : dflt; }

// The entry behind a handle in one of the handle tables (pinned G1 and G2 sets, circuit indices, sharded sets); `take` removes it from the table as well.  The caller
// holds the table's mutex; *out is the caller's, so what a `take` frees is freed after that lock is dropped, once no call uses it (hipFree synchronises).
template <class T> int32_t handle_get(std::map<uint64_t, std::shared_ptr<T>>& table, uint64_t handle, const char* unknown, std::shared_ptr<T>* out, bool take = false) {
  auto it = table.find(handle);
  if (it == table.end()) { g_last_error = unknown; return ALEO_MI355X_ERR_BAD_HANDLE; }
  *out = it->second; if (take) table.erase(it);
  return ALEO_MI355X_OK;
}

// device.hip
int32_t init_device(int device, Device** out);
int32_t get_device(Device** out);                            // the calling thread's current device, initialised on first use
void enable_peer_access();
int32_t acquire_other(Device* d, const Ctx* exclude, Ctx** out, std::unique_lock<std::mutex>& lk, bool may_wait);
// every entry point that computes: the calling thread's device, then a slot of it locked for the duration of the call (rc: why there is none)
struct Slot { Device* d = nullptr; Ctx* c = nullptr; std::unique_lock<std::mutex> lk; int32_t rc; Slot(); };
int32_t pick_stream(Ctx* c, void* stream, hipStream_t* out);
// bases.hip
int32_t find_bases(Device* d, uint64_t handle, std::shared_ptr<PinnedOwner>* keep, PinnedBases* snap);
struct FoundBases { std::shared_ptr<PinnedOwner> keep; PinnedBases pb; int32_t rc; FoundBases(Device* d, uint64_t handle) : rc(find_bases(d, handle, &keep, &pb)) {} };
int32_t msm_host_scalars(Ctx* c, void* out, const PinnedBases& pb, const void* scalars, size_t n, bool mont);
// the device copy of a one-shot call's base array: *pb is valid while the call holds the slot (and *keep, when the copy has an owner)
int32_t one_shot_bases(Ctx* c, const void* bases, size_t stride, size_t n, std::shared_ptr<PinnedOwner>* keep, PinnedBases* pb);
int32_t one_shot_bases_g2(Ctx* c, const void* bases, size_t stride, size_t n, const void** d_xy, const uint8_t** d_inf);
// api.hip
int32_t batch_args_ok(const void* out, const void* const* ptrs, const size_t* lens, size_t k);
// records.hip: *dK, the slot's device copy of the records constants (records_lane.h RK_*), uploaded on the slot's first use; every flow of the records units
// (scan, scan_many, scan_strings, decrypt_fields, decrypt_strings) gets the table here and nowhere else
int32_t records_constants(Ctx* c, const uint32_t** dK);

}  // namespace aleo_mi355x
