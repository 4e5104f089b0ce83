// The rows of tests/ed29_rows.py — the ones aleo_mi355x_selftest_ed29_rows takes to the GPU — through the same shipped source on the HOST, over the bounded
// field of checked_f29.h: f29_mul, f29_tidy, f29_canonical, ed29_add onto ed29_cache, ed29_dbl, one row after the other, raw limbs in and raw limbs out.
// Every operand is tagged with the bounds of its class (the "sound" rule then says whether the row keeps them), so the run validates the rows' builders and the
// Python reference that checks the results without a GPU, and says of every rule that it holds over the whole class the rows were built for.
//   g++ -std=c++17 -O2 -mbmi2 -madx -I aleo_amd/csrc tests/cpp/ed29_rows_emul.cpp      ed29_rows_emul <case file> <result file>     (tests/test_ed29_bounds.py)
// The case file: u32 counts of the five kinds, then mul_a, mul_b, tidy, canon, p, q (u32 rows), neg (u8), d2 (9 u32), dbl (u32 rows), want_t (u8).
// The result file: the five outputs, u32 rows, in that order.
#include "checked_f29.h"
#include <vector>

static F29 lazy(const uint32_t* limbs, uint64_t limb_max, uint64_t vb) {      // limbs 0..7 up to limb_max, value below vb r
  F29 r; for (int i = 0; i < 9; ++i) { r.v[i] = limbs[i]; r.b[i] = limb_max; }
  r.vb = vb; r.b[8] = top_limb_below(vb); r.exact = false; return r;
}
static Ed29 point(const uint32_t* row) { Ed29 e; e.X = exact_below(row, 3 * UNIT); e.Y = exact_below(row + 9, 3 * UNIT); e.Z = exact_below(row + 18, 3 * UNIT); e.T = exact_below(row + 27, 3 * UNIT); return e; }

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  char* one[2] = {argv[0], argv[1]};
  std::FILE* f = open_cases(2, one);
  if (!f) return 2;
  uint32_t n[5];
  if (!get(f, n, sizeof n)) return 2;
  for (uint32_t k : n) if (k > (1u << 20)) return 2;
  std::vector<uint32_t> mul_a(9 * n[0]), mul_b(9 * n[0]), tidy(9 * n[1]), canon(9 * n[2]), p(36 * n[3]), q(36 * n[3]), dbl(36 * n[4]);
  std::vector<uint8_t> neg(n[3]), want_t(n[4]); uint32_t d2[9];
  if (!get(f, mul_a.data(), 4 * mul_a.size()) || !get(f, mul_b.data(), 4 * mul_b.size()) || !get(f, tidy.data(), 4 * tidy.size()) || !get(f, canon.data(), 4 * canon.size()) ||
      !get(f, p.data(), 4 * p.size()) || !get(f, q.data(), 4 * q.size()) || !get(f, neg.data(), neg.size()) || !get(f, d2, sizeof d2) || !get(f, dbl.data(), 4 * dbl.size()) ||
      !get(f, want_t.data(), want_t.size())) return 2;
  std::fclose(f);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  auto put = [&](const F29& a) { std::fwrite(a.v, 4, 9, o); };
  const uint64_t vb261 = vb_covering(TWO261) - 1;                // a multiplicand: limbs below 2^31.4, value below the last multiple of r / 2^32 that is not above 2^261
  for (uint32_t i = 0; i < n[0]; ++i) { t_formula = "f29_mul"; put(f29_mul(lazy(&mul_a[9 * i], LAZY_MAX - 1, vb261), exact_below(&mul_b[9 * i], VB_2_256))); }
  for (uint32_t i = 0; i < n[1]; ++i) { t_formula = "f29_tidy"; F29 a = lazy(&tidy[9 * i], 7 * (1ull << 29) - 1, 445 * UNIT); f29_tidy(a); put(a); }
  for (uint32_t i = 0; i < n[2]; ++i) { t_formula = "f29_canonical"; put(f29_canonical(lazy(&canon[9 * i], 5 * (1ull << 29) - 1, 438 * UNIT))); }
  for (uint32_t i = 0; i < n[3]; ++i) {
    Ed29 acc = point(&p[36 * i]);
    t_formula = "ed29_cache"; const Ed29Cached c = ed29_cache(point(&q[36 * i]), f29_limbs(d2));
    t_formula = "ed29_add"; ed29_add(acc, c, neg[i] != 0);
    put(acc.X); put(acc.Y); put(acc.Z); put(acc.T);
  }
  for (uint32_t i = 0; i < n[4]; ++i) {
    Ed29 acc = point(&dbl[36 * i]);
    t_formula = "ed29_dbl"; ed29_dbl(acc, want_t[i] != 0);
    put(acc.X); put(acc.Y); put(acc.Z); put(acc.T);
  }
  t_formula = nullptr;
  if (std::fclose(o)) return 2;
  std::printf("ed29_rows_emul: %u products, %u tidies, %u canonical forms, %u additions, %u doublings, %lu limb-rule violations\n", n[0], n[1], n[2], n[3], n[4], g_violations);
  return g_violations ? 1 : 0;
}
