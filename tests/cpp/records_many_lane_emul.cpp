// The grouped record scan's device lane (aleo_amd/csrc/records_many_lane.h) run on the HOST, against the library's host path key by key.
//
// The checked 29-bit-limb field is the one of checked_f29.h: every operand rule of
// fr29.h is a check there, so a bound the grouped lane breaks — its accumulators start at the neutral point, its inversion multiplies W denominators — shows as a count.
//   hipcc -x c++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/records_many_lane_emul.cpp   (tests/test_records_many.py builds and runs it).
#include "checked_f29.h"
#include "records_many_lane.h"

static unsigned long g_bad = 0, g_owned = 0, g_malformed = 0, g_pairs = 0;

struct Key { uint8_t vk[32], ax[32]; ScanArgs a; HFr addr; };
static bool make_key(Key& k, int kind) {                    // kind 0: random; 1: view key 1; 2: view key 0 (k = l)
  rnd_fr(k.vk); k.vk[31] &= 0x03;
  if (kind) { std::memset(k.vk, 0, 32); k.vk[0] = kind == 1; }
  rnd_fr(k.ax);
  if (const char* why = scan_args(k.a, k.addr, k.vk, k.ax)) { std::fprintf(stderr, "scan_args: %s\n", why); return false; }
  return true;
}

// `records` records against keys[0 .. live) in a group of width W (the places from `live` on are padding: zero masks)
template <int W> static void run_group(const char* what, const Key* keys, uint32_t live, int records) {
  const RecordsConsts& C = records_consts();
  ScanArgs A[W]; std::memset(A, 0, sizeof A);
  uint32_t len = 0;
  for (uint32_t j = 0; j < live; ++j) { A[j] = keys[j].a; if (A[j].naf_len > len) len = A[j].naf_len; }
  for (int i = 0; i < records; ++i) {
    uint8_t c0[32], nx[32], rvk[32];
    rnd_fr(c0); rnd_fr(nx);
    if (i == 0) std::memset(nx, 0, 32);                       // x = 0
    if (i == 1) std::memset(nx, 0xff, 32);                    // not below r
    if (i == 2) std::memset(c0, 0xff, 32);
    if (i == 3) std::memcpy(nx, host::HParams<4>::P, 32);     // exactly r
    const uint32_t mine = (uint32_t)(i / 4) % live;
    if (i % 4 == 0 && scan_one_host(rvk, c0, nx, keys[mine].a, keys[mine].addr, C) == 0) {      // make this one owned by exactly one key of the group (and by its repeats)
      HFr st[9]; for (int q = 0; q < 9; ++q) st[q] = C.s0[q];
      HFr rv; std::memcpy(rv.l, rvk, 32); st[2] = HFr::add(st[2], HFr::to_mont(rv));
      host::poseidon_permute<4, 8>(st);
      const HFr c = HFr::from_mont(HFr::add(keys[mine].addr, st[1])); std::memcpy(c0, c.l, 32);
      if (scan_one_host(rvk, c0, nx, keys[mine].a, keys[mine].addr, C) != 1) { std::fprintf(stderr, "host path: a record encrypted to the address is not owned\n"); ++g_bad; }
    }
    uint32_t c0w[8], nxw[8]; std::memcpy(c0w, c0, 32); std::memcpy(nxw, nx, 32);
    F29 parked[W], out[W]; uint32_t flag[W]; uint32_t emitted = 0, finished = 0;
    for (int j = 0; j < W; ++j) flag[j] = 9;
    records_scan_lane_many<W>(c0w, nxw, C.words.data(), A, live, len,
                              [&](int j, const F29& v) { parked[j] = v; }, [&](uint32_t j) { return parked[j]; },
                              [&](uint32_t j, const F29& v) { out[j] = v; emitted |= 1u << j; }, [&](uint32_t j, uint32_t f) { flag[j] = f; finished |= 1u << j; });
    if (emitted != (1u << live) - 1 || finished != emitted) { if (g_bad++ < 5) std::fprintf(stderr, "%s W %d record %d: keys answered %x / %x of %u\n", what, W, i, emitted, finished, live); continue; }
    for (uint32_t j = 0; j < live; ++j, ++g_pairs) {
      uint8_t want_rvk[32]; const uint8_t want = scan_one_host(want_rvk, c0, nx, keys[j].a, keys[j].addr, C);
      uint32_t ow[8]; f29_to_words(out[j], ow);
      if (flag[j] != want || std::memcmp(ow, want_rvk, 32)) { if (g_bad++ < 5) std::fprintf(stderr, "%s W %d record %d key %u: lane flag %u, host flag %u, rvk %s\n", what, W, i, j, flag[j], (unsigned)want, std::memcmp(ow, want_rvk, 32) ? "differs" : "equal"); }
      if (want == 1 && j != mine && std::memcmp(keys[j].vk, keys[mine].vk, 32)) { std::fprintf(stderr, "host path: a second key owns the record\n"); ++g_bad; }
      g_owned += want == 1; g_malformed += want == 2;
    }
  }
}

template <int W> static bool run_width() {
  Key k[8];
  for (int j = 0; j < W; ++j) if (!make_key(k[j], 0)) return false;
  k[0].vk[0] |= 1; k[1].vk[0] &= 0xfe;                       // an odd and an even key for sure
  if (scan_args(k[0].a, k[0].addr, k[0].vk, k[0].ax) || scan_args(k[1].a, k[1].addr, k[1].vk, k[1].ax)) return false;
  run_group<W>("random keys", k, W, 40);
  run_group<W>("a partial group", k, W - 1, 40);
  // view key 1 (one digit), view key 0 (k = l), a repeated key — at W = 2 in two groups
  Key s[8];
  if (!make_key(s[0], 1) || !make_key(s[1], 2)) return false;
  s[2] = k[0]; s[3] = k[0];
  for (int j = 4; j < W; ++j) s[j] = k[j];
  run_group<W>("view keys 1 and 0", s, W, 40);
  if (W == 2) { run_group<W>("a repeated key", s + 2, 2, 40); s[1] = s[0]; run_group<W>("view key 1 alone, twice", s, 2, 8); }
  return true;
}

int main() {
  if (!run_width<2>() || !run_width<4>() || !run_width<8>()) return 2;
  std::printf("records_many_lane_emul: %lu pairs, %lu owned, %lu malformed, %lu mismatches, %lu limb-rule violations\n", g_pairs, g_owned, g_malformed, g_bad, g_violations);
  return g_bad || g_violations || !g_owned || !g_malformed ? 1 : 0;
}
