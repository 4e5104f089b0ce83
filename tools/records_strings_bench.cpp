// C-level timings of the record search from strings (tools/records_strings_bench.py builds and runs this, and documents the figures):
//   records_strings_bench <library> [<library of the parent commit>] [--sizes 12,16,20] [--reps 7] [--scan-only N]
// Strings: copies of the reference's record shape (118 payload bytes, 202 characters) with the owner field, the entry's bytes and the nonce varied.  Every
// timing has host buffers, upload and download inside the timed call, one warm call before it, and is the median of `reps`.  The scan from strings (this
// library) and "loop of record_parse + records_scan" (the parent's library, which has no other way from strings) alternate, rep by rep.
// --scan-only N: N calls of records_scan_strings at the largest size and nothing else (the run a kernel trace is taken of).
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Lib {
  void* h = nullptr;
  int32_t (*init)(int32_t) = nullptr;
  int32_t (*encode)(char*, size_t, const char*, const void*, size_t) = nullptr;
  int32_t (*parse)(const char*, int32_t*, void*, void*) = nullptr;
  int32_t (*scan)(uint8_t*, void*, const void*, const void*, size_t, const void*, const void*) = nullptr;
  int32_t (*parse_many)(int8_t*, void*, void*, const char*, const uint64_t*, size_t) = nullptr;
  int32_t (*parse_many_host)(int8_t*, void*, void*, const char*, const uint64_t*, size_t) = nullptr;
  int32_t (*scan_strings)(uint8_t*, int8_t*, void*, const char*, const uint64_t*, size_t, const void*, const void*, size_t) = nullptr;
  const char* (*last_error)() = nullptr;
  bool open(const char* path, bool strings) {
    h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { std::fprintf(stderr, "%s\n", dlerror()); return false; }
    auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) std::fprintf(stderr, "%s: no %s\n", path, n); return p; };
    init = (decltype(init))sym("aleo_mi355x_init_device"); encode = (decltype(encode))sym("aleo_mi355x_bech32m_encode"); parse = (decltype(parse))sym("aleo_mi355x_record_parse");
    scan = (decltype(scan))sym("aleo_mi355x_records_scan"); last_error = (decltype(last_error))sym("aleo_mi355x_last_error");
    if (strings) {
      parse_many = (decltype(parse_many))sym("aleo_mi355x_records_parse_many"); parse_many_host = (decltype(parse_many_host))sym("aleo_mi355x_records_parse_many_host");
      scan_strings = (decltype(scan_strings))sym("aleo_mi355x_records_scan_strings");
    }
    return init && encode && parse && scan && last_error && (!strings || (parse_many && parse_many_host && scan_strings));
  }
};

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

#define MUST(call) do { const int32_t rc__ = (call); if (rc__) { std::fprintf(stderr, "%s failed: %d [%s]\n", #call, rc__, L.last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
  std::vector<std::string> paths; std::vector<int> sizes{12, 16, 20}; int reps = 7, scan_only = 0;
  for (int a = 1; a < argc; ++a) {
    if (!std::strcmp(argv[a], "--sizes") && a + 1 < argc) { sizes.clear(); for (char* t = std::strtok(argv[++a], ","); t; t = std::strtok(nullptr, ",")) sizes.push_back(std::atoi(t)); }
    else if (!std::strcmp(argv[a], "--reps") && a + 1 < argc) reps = std::atoi(argv[++a]);
    else if (!std::strcmp(argv[a], "--scan-only") && a + 1 < argc) scan_only = std::atoi(argv[++a]);
    else paths.push_back(argv[a]);
  }
  if (paths.empty() || paths.size() > 2 || sizes.empty() || reps < 1) { std::fprintf(stderr, "usage: records_strings_bench <library> [<parent library>] [--sizes 12,16,20] [--reps 7] [--scan-only N]\n"); return 2; }
  Lib L, P;
  if (!L.open(paths[0].c_str(), true)) return 2;
  const bool parent = paths.size() == 2;
  if (parent && !P.open(paths[1].c_str(), false)) return 2;
  MUST(L.init(-1));
  if (parent && P.init(-1)) { std::fprintf(stderr, "parent library: init failed [%s]\n", P.last_error()); return 1; }
  setenv("ALEO_MI355X_MIN_RECORDS", "0", 1);                // every routed call takes the device

  const int top = *std::max_element(sizes.begin(), sizes.end());
  const size_t n_max = (size_t)1 << top;
  // the strings: variant 1, count 1, c0 | 1 entry: "microcredits", 35 bytes | nonce
  std::string text; std::vector<uint64_t> offsets{0}; std::vector<std::string> each; each.reserve(n_max);
  {
    uint8_t payload[118] = {1, 1, 0}; char out[256];
    payload[35] = 1; payload[36] = 12; std::memcpy(payload + 37, "microcredits", 12); payload[49] = 35; payload[50] = 0;
    text.reserve(n_max * 202);
    for (size_t i = 0; i < n_max; ++i) {
      for (int q = 0; q < 4; ++q) { const uint64_t a = rnd(), b = rnd(), c = rnd(); std::memcpy(payload + 3 + 8 * q, &a, 8); std::memcpy(payload + 86 + 8 * q, &b, 8); std::memcpy(payload + 51 + 8 * q, &c, 8); }
      payload[34] &= 0x0f; payload[117] &= 0x0f;              // below 2^252: canonical
      MUST(L.encode(out, sizeof out, "record", payload, sizeof payload));
      each.emplace_back(out); text += out; offsets.push_back(text.size());
    }
  }
  uint8_t vk[32] = {0x57, 0x13, 0x21, 0x43, 0x65, 0x87, 0xa9, 0xcb, 0xed, 0x0f, 0x21, 0x43, 0x65, 0x87, 0xa9, 0x0b}, ax[32] = {5};
  std::vector<uint8_t> c0(32 * n_max), nx(32 * n_max), flags(n_max), flags_p(n_max), rvk(32 * n_max), rvk_p(32 * n_max), c0b(32 * n_max), nxb(32 * n_max);
  std::vector<int8_t> kinds(n_max), kinds_b(n_max);

  if (scan_only) {
    for (int r = 0; r < scan_only; ++r) MUST(L.scan_strings(flags.data(), kinds.data(), rvk.data(), text.data(), offsets.data(), n_max, vk, ax, 1));
    std::printf("scan-only: %d calls of records_scan_strings at n = 2^%d\n", scan_only, top);
    return 0;
  }
  std::printf("%-6s %-58s %12s %14s\n", "n", "what", "median ms", "M records/s");
  for (int lg : sizes) {
    const size_t n = (size_t)1 << lg;
    auto report = [&](const char* what, const std::vector<double>& t) { const double m = median(t); std::printf("2^%-4d %-58s %12.3f %14.3f\n", lg, what, m * 1e3, n / m / 1e6); std::fflush(stdout); return m; };
    auto loop_parse = [&](Lib& X, uint8_t* o, uint8_t* x) { int32_t kind; int32_t bad = 0; for (size_t i = 0; i < n; ++i) bad |= X.parse(each[i].c_str(), &kind, o + 32 * i, x + 32 * i); return bad; };
    std::vector<double> t;
    for (int r = -1; r < reps; ++r) { const double t0 = now(); MUST(loop_parse(L, c0.data(), nx.data())); if (r >= 0) t.push_back(now() - t0); }
    report("loop of record_parse", t); t.clear();
    for (int r = -1; r < reps; ++r) { const double t0 = now(); MUST(L.parse_many_host(kinds_b.data(), c0b.data(), nxb.data(), text.data(), offsets.data(), n)); if (r >= 0) t.push_back(now() - t0); }
    report("records_parse_many_host", t); t.clear();
    if (std::memcmp(c0.data(), c0b.data(), 32 * n) || std::memcmp(nx.data(), nxb.data(), 32 * n)) { std::fprintf(stderr, "parse_many_host differs from the loop\n"); return 1; }
    for (int r = -1; r < reps; ++r) { const double t0 = now(); MUST(L.parse_many(kinds.data(), c0b.data(), nxb.data(), text.data(), offsets.data(), n)); if (r >= 0) t.push_back(now() - t0); }
    report("records_parse_many (GPU)", t); t.clear();
    if (std::memcmp(c0.data(), c0b.data(), 32 * n) || std::memcmp(nx.data(), nxb.data(), 32 * n) || std::memcmp(kinds.data(), kinds_b.data(), n)) { std::fprintf(stderr, "parse_many differs from the loop\n"); return 1; }
    for (int r = -1; r < reps; ++r) { const double t0 = now(); MUST(L.scan(flags_p.data(), rvk_p.data(), c0.data(), nx.data(), n, vk, ax)); if (r >= 0) t.push_back(now() - t0); }
    report("records_scan on parsed rows (this library, no parsing)", t); t.clear();
    std::vector<double> tp;
    for (int r = -1; r < reps; ++r) {                          // alternating
      double t0 = now(); MUST(L.scan_strings(flags.data(), kinds.data(), rvk.data(), text.data(), offsets.data(), n, vk, ax, 1)); if (r >= 0) t.push_back(now() - t0);
      if (parent) { t0 = now(); if (loop_parse(P, c0b.data(), nxb.data()) || P.scan(flags_p.data(), rvk_p.data(), c0b.data(), nxb.data(), n, vk, ax)) { std::fprintf(stderr, "parent path failed [%s]\n", P.last_error()); return 1; } if (r >= 0) tp.push_back(now() - t0); }
    }
    const double mine = report("records_scan_strings, K = 1", t);
    if (std::memcmp(flags.data(), flags_p.data(), n) || std::memcmp(rvk.data(), rvk_p.data(), 32 * n)) { std::fprintf(stderr, "scan_strings differs from parse + scan\n"); return 1; }
    if (parent) { const double theirs = report("parent library: loop of record_parse + records_scan", tp); std::printf("2^%-4d %-58s %11.1fx\n", lg, "  scan_strings against the parent's path", theirs / mine); }
  }
  return 0;
}
