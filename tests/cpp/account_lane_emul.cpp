// The account kernels' device lane (aleo_amd/csrc/account_lane.h) run on the HOST, account by account against the bytes the library's host path returned
// (aleo_mi355x_accounts_derive_host) and against account_host.hpp's derive_one_host compiled into this program, with the table built by account_host.hpp as the
// library builds it.  A search candidate is given as (master seed, index): the lane's own draw of its seed (account_candidate_seed) is checked against the seed the
// test computed, and the head of its address's symbol stream (what the search kernel compares with the prefix) against the address's first bytes.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the lane breaks shows as a count.  The lane must never put a character outside its row of 63.  Plain C++ for the host
// compiler, built once plain and once with the address and undefined-behaviour sanitizers and run as a program of its own (tests/test_accounts.py):
//   g++ -std=c++17 -O2 -fno-strict-aliasing -mbmi2 -madx [-fsanitize=address,undefined] -I aleo_amd/csrc tests/cpp/account_lane_emul.cpp
//   account_lane_emul <case file>
// The file: u32 count, then per account: u8 kind (0 a seed, 1 a candidate), [kind 1: the 32 bytes of the master seed, u64 index], the 32 bytes of the seed, u8 the
// flag wanted, 32 bytes each of sk_sig, view key and address x, the 63 characters of the address (zeros with flag 3).
#include "checked_f29.h"
#include "account_host.hpp"
#include <vector>


int main(int argc, char** argv) {
  uint32_t count = 0;
  std::FILE* f = open_cases(argc, argv, &count);
  if (!f) return 2;
  const acct::AccountTables& T = acct::account_tables();
  unsigned long flags[4] = {0, 0, 0, 0}, bad = 0, past = 0, candidates = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint8_t kind, master[32], seed[32], want_flag, want[96]; uint64_t index = 0; char want_str[63];
    if (!get(f, &kind, 1) || kind > 1) return 2;
    if (kind == 1 && (!get(f, master, 32) || !get(f, &index, 8))) return 2;
    if (!get(f, seed, 32) || !get(f, &want_flag, 1) || !get(f, want, 96) || !get(f, want_str, 63)) return 2;
    uint32_t seedw[8];
    if (kind == 1) {
      uint32_t key[8]; std::memcpy(key, master, 32);
      account_candidate_seed(seedw, key, index);
      ++candidates;
      if (std::memcmp(seedw, seed, 32)) { if (bad++ < 8) std::fprintf(stderr, "account %u: the candidate's seed differs\n", i); continue; }
    } else std::memcpy(seedw, seed, 32);
    AccountWords a;
    const uint32_t flag = account_lane(seedw, T.words.data(), a, [] {});
    uint8_t host[96];
    const uint32_t host_flag = acct::derive_one_host(seed, host, host + 32, host + 64);
    uint8_t got[96]; std::memcpy(got, a.sk_sig, 32); std::memcpy(got + 32, a.view_key, 32); std::memcpy(got + 64, a.address, 32);
    std::vector<char> str(63, 0);                                // exact: a write past the end is the sanitizer's
    uint32_t expect_at = 0;
    ac_address_string(a.address, [&](uint32_t at, uint32_t ch) { if (at >= 63 || at != expect_at++) { ++past; return; } str[at] = (char)(flag ? 0u : ch); });
    char host_str[63]; std::memset(host_str, 0, 63);
    if (!host_flag) acct::address_string(host_str, host + 64);
    uint32_t hi, lo; ac_stream_head(a.address, hi, lo);
    uint64_t head = 0; for (int k = 0; k < 8; ++k) head = (head << 8) | host[64 + k];
    const bool same = flag == want_flag && host_flag == want_flag && !std::memcmp(got, want, 96) && !std::memcmp(host, want, 96) && !std::memcmp(str.data(), want_str, 63) &&
                      !std::memcmp(host_str, want_str, 63) && expect_at == 63 && (((uint64_t)hi << 32) | lo) == head;
    if (!same && bad++ < 8) std::fprintf(stderr, "account %u: lane flag %u, host flag %u, wanted %u; lane rows %s, host rows %s, lane string %s\n", i, flag, host_flag, (unsigned)want_flag,
                                         std::memcmp(got, want, 96) ? "differ" : "equal", std::memcmp(host, want, 96) ? "differ" : "equal", std::memcmp(str.data(), want_str, 63) ? "differs" : "equal");
    ++flags[flag & 3u];
  }
  std::fclose(f);
  std::printf("account_lane_emul: %u accounts, %lu derived, %lu refused, %lu of them candidates, %lu mismatches, %lu reads past an end, %lu limb-rule violations\n",
              count, flags[0], flags[3], candidates, bad, past, g_violations);
  return bad || past || g_violations ? 1 : 0;
}
