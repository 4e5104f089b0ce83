// accounts.hip — accounts in batches: sk_sig, view key, address and the "aleo1…" string of many private-key seeds in one call, and the search of a seed range for
// addresses with a chosen prefix — the first step of every record and signature flow (records_scan*, records_decrypt_strings*, records_unspent_*,
// signatures_verify take an account's sk_sig, view key and address), which the library computed one key at a time on one host thread.  The reference's account
// module: wasm/src/account/private_key.rs:38-86 (PrivateKey::new, from_seed_unchecked, to_view_key, to_address), sdk/src/account.ts:82 — snarkVM 0.14.5
// console/account [UPSTREAM-RECALL]; what is pinned by the reference's data and what is UNPINNED: account_host.hpp.
//
// The kernels (one account per lane: account_lane.h), their table (account_host.hpp: the signature table's words and the rate-2 constants, built on the host at
// first use and resident per device), the same bytes on the host (records_bits.hpp / account_host.hpp serial::account_from_seed — what small batches take, and the
// definition), the routing threshold, and the host-only calls: the strings and the reduction of 32 bytes to a seed.
#include "accounts.h"
#include "records_bits.hpp"
#include <algorithm>
#include <cstdlib>

namespace aleo_mi355x {

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------
// Account i of the chunk: its seed the 32 bytes at seeds + 32 i; rows of 32 bytes at sk, view, addr, of 63 characters at str, one flag byte at flags.
__global__ void __launch_bounds__(ACC_BLOCK) k_accounts_derive(char* base, uint32_t n, const uint32_t* K) {
  const uint32_t i = blockIdx.x * ACC_BLOCK + threadIdx.x;
  if (i >= n) return;                                          // no barrier and no wave-level operation below
  const AccChunk* head = (const AccChunk*)base;
  const uint32_t o_flag = head->flags + i;
  uint32_t seed[8];
  load_words8(seed, base + (head->seeds + 32u * i));
  AccountWords a;
  const uint32_t flag = account_lane(seed, K, a, [&] { base[o_flag] = (char)ACC_BAD_SEED; });      // provisional: account_lane.h phase()
  const AccChunk C = *head;
  if (C.sk != ACC_NONE) store_words8(base + (C.sk + 32u * i), a.sk_sig);
  if (C.view != ACC_NONE) store_words8(base + (C.view + 32u * i), a.view_key);
  if (C.addr != ACC_NONE) store_words8(base + (C.addr + 32u * i), a.address);
  if (C.str != ACC_NONE) {
    const uint32_t o_str = C.str + ACC_ADDRESS_CHARS * i;
    ac_address_string(a.address, [&](uint32_t at, uint32_t ch) { base[o_str + at] = (char)(flag ? 0u : ch); });      // a refused seed's row is zero
  }
  base[o_flag] = (char)flag;
}

// Candidates first .. first + n - 1 of a search under `master`: the offsets (from first) of those whose address begins with the prefix are appended to the list
// at `list`, whose length is the word at `counter` — in the order the lanes get there: the host sorts them.  mask / want: the prefix against the first 64 bits of
// the address's symbol stream (account_host.hpp Prefix), high word and low.  Nothing is written per candidate.
// The words of the comparison and of the list lie at the start of the buffer, as a derivation's offsets do.
struct SearchChunk { uint32_t n, counter, list, pad, mask_hi, mask_lo, want_hi, want_lo; };

__global__ void __launch_bounds__(ACC_BLOCK) k_accounts_search(char* base, Seed32 master, uint32_t first_lo, uint32_t first_hi, uint32_t n, const uint32_t* K) {
  const uint32_t i = blockIdx.x * ACC_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8];
  account_candidate_seed(seed, master.w, (((uint64_t)first_hi << 32) | first_lo) + i);
  uint32_t base_lo = (uint32_t)(uintptr_t)base, base_hi = (uint32_t)((uintptr_t)base >> 32);
  ac_lane_word(base_lo); ac_lane_word(base_hi);                // the buffer's address waits for the end in two of the lane's registers, not in two scalar ones
  AccountWords a;
  (void)account_lane(seed, K, a, [] { __asm__ volatile("" ::: "memory"); });      // no flag to store here: the compiler's own barrier keeps a phase's loads in their phase
  base = (char*)(((uintptr_t)base_hi << 32) | base_lo);
  const SearchChunk C = *(const SearchChunk*)base;
  uint32_t hi, lo;
  ac_stream_head(a.address, hi, lo);
  if ((hi & C.mask_hi) == C.want_hi && (lo & C.mask_lo) == C.want_lo) {
    const uint32_t at = atomicAdd((uint32_t*)(base + C.counter), 1u);
    if (at < C.n) ((uint32_t*)(base + C.list))[at] = i;          // every lane appends at most once: at < n
  }
}

int32_t account_table(int device, const uint32_t** out) {
  return resident_table(device, ResidentTable::ACCOUNT, []() -> const std::vector<uint32_t>& { return acct::account_tables().words; }, out);
}

void launch_accounts_derive(hipStream_t s, char* base, size_t m, const uint32_t* dK) {
  hipLaunchKernelGGL(k_accounts_derive, dim3((uint32_t)((m + ACC_BLOCK - 1) / ACC_BLOCK)), dim3(ACC_BLOCK), 0, s, base, (uint32_t)m, dK);
}

// ---- derive -------------------------------------------------------------------------------------------------------------------------------------------
// Chunk by chunk: the seeds go up, one launch runs, the rows asked for come down.
static int32_t derive_on_device(const uint8_t* seeds, size_t n, const AccOut& out, uint8_t* flags) {
  const size_t cap = env_cap("ALEO_MI355X_ACCOUNTS_CHUNK", ACC_CHUNK);
  AccChunk head;                                               // declared outside the slot: it outlives the copy that reads it
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = account_table(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    for (size_t lo = 0; lo < n;) {
      const size_t m = std::min(cap, n - lo);
      Carve cv;
      const size_t o_head = cv.part(sizeof(AccChunk)), o_seed = cv.part(m * 32), o_fl = cv.part(m);
      head = AccChunk{(uint32_t)o_seed, (uint32_t)o_fl, ACC_NONE, ACC_NONE, ACC_NONE, ACC_NONE, (uint32_t)m, 0u};
      out.carve(cv, head, m);
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      HIPCHK(hipMemcpyAsync(b + o_seed, seeds + lo * 32, m * 32, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b + o_head, &head, sizeof head, hipMemcpyHostToDevice, s));
      launch_accounts_derive(s, b, m, dK);
      HIPCHK(hipGetLastError());
      if (int32_t rc = out.download(s, b, head, lo, m)) return rc;
      if (flags) HIPCHK(hipMemcpyAsync(flags + lo, b + o_fl, m, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));                           // the next chunk reuses the buffer
      lo += m;
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t accounts_derive(const void* seeds32, size_t n, void* sk_sig32, void* view_key32, void* address_x32, char* address63, uint8_t* flags, bool may_route) {
  if (!n) return ALEO_MI355X_OK;
  if (!seeds32) return bad_arg("accounts_derive: null seeds");
  const uint8_t* seeds = (const uint8_t*)seeds32;
  const AccOut out{(uint8_t*)sk_sig32, (uint8_t*)view_key32, (uint8_t*)address_x32, address63};
  if (may_route && n >= aleo_mi355x_min_accounts()) return derive_on_device(seeds, n, out, flags);
  for (size_t i = 0; i < n; ++i) { const uint8_t flag = out.row_on_host(i, seeds + 32 * i, 0); if (flags) flags[i] = flag; }
  return ALEO_MI355X_OK;
}

// ---- search -------------------------------------------------------------------------------------------------------------------------------------------
// Launch by launch until max_hits are found or the range ends: the counter is cleared, one launch runs, the counter and that many offsets come down and are
// sorted.  What a launch found beyond the last hit wanted is dropped.
static int32_t search_on_device(const uint8_t* master32, uint64_t first, uint64_t count, const acct::Prefix& p, size_t max_hits, std::vector<uint64_t>& hits) {
  const size_t cap = env_cap("ALEO_MI355X_ACCOUNTS_CHUNK", ACC_CHUNK);
  std::vector<uint32_t> found;
  SearchChunk head; Seed32 key;
  return on_slot([&](Ctx* c) -> int32_t {
    const uint32_t* dK;
    if (int32_t rc = account_table(c->device, &dK)) return rc;
    hipStream_t s = c->stream;
    std::memcpy(key.w, master32, 32);
    for (uint64_t done = 0; done < count && hits.size() < max_hits;) {
      const size_t m = (size_t)std::min<uint64_t>(cap, count - done);
      Carve cv;
      const size_t o_head = cv.part(sizeof(SearchChunk)), o_count = cv.part(4), o_list = cv.part(m * 4);
      if (int32_t rc = c->scalars_stage.reserve(cv.total)) return rc;
      char* b = c->scalars_stage.as<char>();
      const uint64_t lo = first + done;
      head = SearchChunk{(uint32_t)m, (uint32_t)o_count, (uint32_t)o_list, 0u, (uint32_t)(p.mask >> 32), (uint32_t)p.mask, (uint32_t)(p.want >> 32), (uint32_t)p.want};
      HIPCHK(hipMemcpyAsync(b + o_head, &head, sizeof head, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemsetAsync(b + o_count, 0, 4, s));
      hipLaunchKernelGGL(k_accounts_search, dim3((uint32_t)((m + ACC_BLOCK - 1) / ACC_BLOCK)), dim3(ACC_BLOCK), 0, s, b, key, (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)m, dK);
      HIPCHK(hipGetLastError());
      uint32_t k = 0;
      HIPCHK(hipMemcpyAsync(&k, b + o_count, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (k > m) { g_last_error = "accounts_search: the kernel reports more hits than candidates"; return ALEO_MI355X_ERR_INTERNAL; }
      found.resize(k);
      if (k) { HIPCHK(hipMemcpyAsync(found.data(), b + o_list, (size_t)k * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
      std::sort(found.begin(), found.end());                     // the order of arrival is the scheduler's; the result is not
      for (size_t j = 0; j < found.size() && hits.size() < max_hits; ++j) hits.push_back(lo + found[j]);
      done += m;
    }
    return ALEO_MI355X_OK;
  });
}

static int32_t accounts_search(const void* master32, uint64_t first, uint64_t count, const char* prefix, size_t max_hits, uint64_t* hit_index, void* hit_seed32, size_t* n_hits,
                               uint64_t* next, bool may_route) {
  if (!master32 || !n_hits || !next || (max_hits && !hit_index)) return bad_arg("accounts_search: null buffer");
  acct::Prefix p;
  if (const char* why = acct::parse_prefix(p, prefix)) { g_last_error = std::string("accounts_search: ") + why; return ALEO_MI355X_ERR_BAD_ARG; }
  if (first + count < first) return bad_arg("accounts_search: the range passes 2^64");
  const uint8_t* master = (const uint8_t*)master32; uint8_t* seeds = (uint8_t*)hit_seed32;
  if (!(may_route && count >= aleo_mi355x_min_accounts()) || !max_hits) { acct::search_host(master, first, count, p, max_hits, hit_index, seeds, n_hits, next); return ALEO_MI355X_OK; }
  std::vector<uint64_t> hits;
  if (int32_t rc = search_on_device(master, first, count, p, max_hits, hits)) return rc;
  // every hit is derived again on the host before it is handed out: the call never returns a key whose address the host path would not give
  for (size_t j = 0; j < hits.size(); ++j) {
    uint8_t seed[32];
    if (!acct::candidate_matches(master, hits[j], p, seed)) { g_last_error = "accounts_search: the host path does not confirm a hit of the kernel"; return ALEO_MI355X_ERR_INTERNAL; }
    hit_index[j] = hits[j]; if (seeds) std::memcpy(seeds + 32 * j, seed, 32);
  }
  *n_hits = hits.size();
  *next = hits.size() == max_hits ? hits.back() + 1 : first + count;
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which a derivation or a search takes the GPU: the measured crossover against the host path on one thread, which is what a call below it runs
// (profiles/accounts_derive.txt: the GPU call takes 2.2-3.0 ms for any batch up to 2^12; the host loop 1.37 ms for 2^3 keys, 0.55x and 0.54x; 2.77 ms for 2^4, 1.10x
// and 1.14x; 5.57 ms for 2^5, 2.16x and 2.23x.  With the address strings asked for the call is 3.0 ms below 2^6 and the crossover one step later: 0.93x at 2^4)
size_t aleo_mi355x_min_accounts(void) { return env_size("ALEO_MI355X_MIN_ACCOUNTS", (size_t)1 << 4); }

int32_t aleo_mi355x_accounts_derive(const void* seeds32, size_t n, void* sk_sig32, void* view_key32, void* address_x32, char* address63, uint8_t* flags) {
  return guarded([&] { return accounts_derive(seeds32, n, sk_sig32, view_key32, address_x32, address63, flags, true); });
}
int32_t aleo_mi355x_accounts_derive_host(const void* seeds32, size_t n, void* sk_sig32, void* view_key32, void* address_x32, char* address63, uint8_t* flags) {
  return guarded([&] { return accounts_derive(seeds32, n, sk_sig32, view_key32, address_x32, address63, flags, false); });
}
int32_t aleo_mi355x_accounts_search(const void* master32, uint64_t first, uint64_t count, const char* prefix, size_t max_hits, uint64_t* hit_index, void* hit_seed32, size_t* n_hits,
                                    uint64_t* next) {
  return guarded([&] { return accounts_search(master32, first, count, prefix, max_hits, hit_index, hit_seed32, n_hits, next, true); });
}
int32_t aleo_mi355x_accounts_search_host(const void* master32, uint64_t first, uint64_t count, const char* prefix, size_t max_hits, uint64_t* hit_index, void* hit_seed32, size_t* n_hits,
                                         uint64_t* next) {
  return guarded([&] { return accounts_search(master32, first, count, prefix, max_hits, hit_index, hit_seed32, n_hits, next, false); });
}

int32_t aleo_mi355x_private_key_from_seed(char* out, size_t cap, const void* seed32) {
  return guarded([&] {
    if (!out || !seed32) return bad_arg("private_key_from_seed: null buffer");
    uint64_t v[4]; std::memcpy(v, seed32, 32);
    if (host::HFr::geq_p(v)) return bad_arg("private_key_from_seed: the seed is not a canonical field element");
    return string_out(out, cap, serial::private_key_string((const uint8_t*)seed32), "private_key_from_seed: output buffer too small");
  });
}
int32_t aleo_mi355x_private_key_seed(void* seed32, const char* private_key) {
  return guarded([&] {
    if (!seed32) return bad_arg("private_key_seed: null buffer");
    return serial::private_key_seed(seed32, private_key);
  });
}
int32_t aleo_mi355x_seed_from_bytes(void* seed32, const void* bytes32) {
  return guarded([&] {
    if (!seed32 || !bytes32) return bad_arg("seed_from_bytes: null buffer");
    acct::seed_from_bytes((uint8_t*)seed32, (const uint8_t*)bytes32);
    return (int32_t)ALEO_MI355X_OK;
  });
}
int32_t aleo_mi355x_view_key_to_string(char* out, size_t cap, const void* view_key32) {
  return guarded([&] {
    if (!out || !view_key32) return bad_arg("view_key_to_string: null buffer");
    return string_out(out, cap, serial::view_key_string((const uint8_t*)view_key32), "view_key_to_string: output buffer too small");
  });
}

}  // extern "C"
