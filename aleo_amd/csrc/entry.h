// entry.h — what the units with entry points of the C ABI share (device.hip, bases.hip, sharded.hip, api.hip): the guard at the C boundary, the slot a call runs
// on (and on_slot, the form the records and signature units take it in), its stream, handle lookup, sizes and caps from the environment, the tables resident on a
// device, and the functions that cross between those four files.  (Kernels and their hosts: ctx.h, frops.h.)
#pragma once
#include "ctx.h"
#include <cstdlib>
#include <cstring>

namespace aleo_mi355x {

// No exception crosses the C boundary: every entry point runs its body in here (on_throw: 0 for the *_info / *_timing functions, which return a count).
template <class F> int32_t guarded(F&& body, int32_t on_throw = ALEO_MI355X_ERR_HIP) { try { return body(); } catch (...) { return on_throw; } }

inline int32_t bad_arg(const char* why) { g_last_error = why; return ALEO_MI355X_ERR_BAD_ARG; }      // a refused argument and the text that says which

// A string through the (out, in/out length) convention of the C ABI: *out_len in = the capacity of out, out = the string's length without the terminating 0, which is
// written as well; a buffer that is too short is BAD_ARG with the length in place
inline int32_t put_string(const std::string& s, char* out, size_t* out_len, const char* who) {
  const size_t cap = *out_len; *out_len = s.size();
  if (!out || cap < s.size() + 1) { g_last_error = std::string(who) + ": the output buffer is too short (out_len holds the string's length; one more byte ends it)"; return ALEO_MI355X_ERR_BAD_ARG; }
  std::memcpy(out, s.c_str(), s.size() + 1);
  return ALEO_MI355X_OK;
}

// A size from the environment, read per call: `dflt` where the variable is unset, empty or no decimal number.
inline size_t env_size(const char* name, size_t dflt) { const char* e = std::getenv(name); if (!e || !*e) return dflt; char* end = nullptr; const unsigned long long v = std::strtoull(e, &end, 10); return end && *end == 0 ? (size_t)v : dflt; }

// A cap on the size of one launch or chunk from the environment, read per call: the value where it lies in 1 .. max, else max.
inline size_t env_cap(const char* name, size_t max) { const size_t v = env_size(name, max); return v >= 1 && v <= max ? v : max; }

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
// The device part of a records or signature call: body(Ctx*) runs on a slot taken for it, and a body that fails returns only once the slot's stream has drained.
// Host memory may be the source or the target of an asynchronous copy the body queued before it failed; what the caller declared before this call — its own
// arrays, the results, the key tables and staging vectors of the function that calls this — is therefore never freed or reused under a copy in flight.
template <class F> int32_t on_slot(F&& body) {
  Slot sl; if (sl.rc) return sl.rc;
  const int32_t rc = body(sl.c);
  if (rc) (void)hipStreamSynchronize(sl.c->stream);
  return rc;
}
// The word table of a lane, resident on a device: uploaded once per (device, kind) from words() under a lock, never freed, and handed out only after the copy
// has completed.  Every flow of the records and signature units gets its table here and nowhere else; each of the others begins with the records constants.
enum class ResidentTable { RECORDS, SERIAL, COMMIT, SIGNATURE, ACCOUNT, KEY_CIPHERTEXT };      // records_lane.h RK_*, records_serial_lane.h SK_*, records_commit_lane.h CK_*, signature_lane.h SG_*, account_lane.h AC_*, key_ciphertext_lane.h KC_*
int32_t resident_table(int device, ResidentTable kind, const std::vector<uint32_t>& (*words)(), const uint32_t** out);
// bases.hip
int32_t find_bases(Device* d, uint64_t handle, std::shared_ptr<PinnedOwner>* keep, PinnedBases* snap);
struct FoundBases { std::shared_ptr<PinnedOwner> keep; PinnedBases pb; int32_t rc; FoundBases(Device* d, uint64_t handle) : rc(find_bases(d, handle, &keep, &pb)) {} };
int32_t msm_host_scalars(Ctx* c, void* out, const PinnedBases& pb, const void* scalars, size_t n, bool mont);
// the device copy of a one-shot call's base array: *pb is valid while the call holds the slot (and *keep, when the copy has an owner)
int32_t one_shot_bases(Ctx* c, const void* bases, size_t stride, size_t n, std::shared_ptr<PinnedOwner>* keep, PinnedBases* pb);
int32_t one_shot_bases_g2(Ctx* c, const void* bases, size_t stride, size_t n, const void** d_xy, const uint8_t** d_inf);
// api.hip
int32_t batch_args_ok(const void* out, const void* const* ptrs, const size_t* lens, size_t k);
// n byte strings one after another in `text`, string i at text[offsets[i] .. offsets[i + 1]): what every call over such a blob refuses before it looks at a string
int32_t strings_args_ok(const char* who, const char* text, const uint64_t* offsets, size_t n);

}  // namespace aleo_mi355x
