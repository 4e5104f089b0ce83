// host_group_test.cpp — the one XYZZ group law of aleo_amd/csrc/xyzz_law.h over the host's two fields (HFq: G1, HFq2: G2), as a program of its own
// (tests/test_host_group.py builds it plain and with -fsanitize=address,undefined and checks what it writes against oracle/pyref.py).
//   host_group_test <cases> <out>
// cases: 8 G1 points (x, y, 1) of 144 bytes | 8 G2 points of 288 bytes (the multiples 1..8 of the generators, Montgomery form) | uint64 n | n scalars
//        (uint64) | a G1 point as a 224-byte 28-bit row, the same row with q added to every coordinate in loose limbs | the same two for G2, 448 bytes each.
// out, G1 then G2, every point through law_store_jacobian_normalized: k * G for each scalar (double-and-add from the top bit) | (P + Q) + R | P + (Q + R) |
//        P + P | 2P | P + (-P) | identity + P   with P, Q, R = 1G, 2G, 5G | the two 28-bit rows through law_point28.
#include <cstdio>
#include <vector>
#include "host_field.hpp"

using namespace aleo_mi355x;
using namespace aleo_mi355x::host;

template <class F> static void run(const uint64_t* pts, const std::vector<uint64_t>& scalars, const char* rows28, std::vector<uint64_t>& out) {
  using Pt = XYZZOf<F>;
  constexpr int J = 3 * F::LIMBS;
  auto emit = [&](const Pt& p) { out.resize(out.size() + J); law_store_jacobian_normalized(out.data() + out.size() - J, p); };
  Pt m[8];
  for (int i = 0; i < 8; ++i) m[i] = law_from_jacobian<F>(pts + (size_t)J * i);
  for (uint64_t k : scalars) {
    Pt acc = Pt::infinity();
    for (int bit = 63; bit >= 0; --bit) { acc = law_double(acc); if ((k >> bit) & 1) acc = law_add(acc, m[0]); }
    emit(acc);
  }
  const Pt P = m[0], Q = m[1], R = m[4];
  Pt negP = P; negP.Y = F::sub(F::zero(), P.Y);
  emit(law_add(law_add(P, Q), R)); emit(law_add(P, law_add(Q, R)));
  emit(law_add(P, P)); emit(law_double(P));
  emit(law_add(P, negP));
  emit(law_add(Pt::infinity(), P));
  const size_t row = 4 * F::WORDS28 * 4;
  emit(law_point28<F>(rows28)); emit(law_point28<F>(rows28 + row));
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: host_group_test <cases> <out>\n"); return 2; }
  std::vector<char> in;
  if (FILE* f = std::fopen(argv[1], "rb")) { char buf[4096]; size_t n; while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + n); std::fclose(f); }
  const size_t head = 8 * 144 + 8 * 288 + 8;
  if (in.size() < head) { std::fprintf(stderr, "short case file\n"); return 2; }
  std::vector<uint64_t> w((in.size() + 7) / 8);
  std::memcpy(w.data(), in.data(), in.size());              // aligned copy: the readers take uint64_t / uint32_t pointers
  const uint64_t n = w[(8 * 144 + 8 * 288) / 8];
  if (n > 4096 || in.size() != head + 8 * n + 2 * 224 + 2 * 448) { std::fprintf(stderr, "bad case file\n"); return 2; }
  const std::vector<uint64_t> scalars(w.begin() + head / 8, w.begin() + head / 8 + n);
  const char* rows = (const char*)w.data() + head + 8 * n;
  std::vector<uint64_t> out;
  run<HFq>(w.data(), scalars, rows, out);
  run<HFq2>(w.data() + 8 * 18, scalars, rows + 2 * 224, out);
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size() || std::fclose(f)) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  return 0;
}
