// The pass plan and the choice of kernel configuration of the transform (aleo_amd/csrc/ntt_plan.h), host only:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I aleo_amd/csrc tests/cpp/ntt_plan_test.cpp
// For every lg_n in 1..30 and every tile that has a kernel instance (2^9, 2^11, 2^12 elements) the plan is compared with the launches the two drivers
// it replaces made — their three arms are restated below, launch by launch — and checked for what any plan must satisfy: the axes sum to lg_n,
// no axis is longer than min(lgTE, 11), a block's T transforms of length L fit the tile, and every pass covers the 2^lg_n elements exactly once.
// Three axes of a 2^9 tile reach 2^27: beyond it the old formulas give an axis of 2^10 (asserted here), which no tile of 2^9 holds, and the plan
// refuses (npass == 0).  The library never asks for it: that tile serves 2^10..2^18 only.
#include "ntt_plan.h"
#include <cstdio>

using namespace aleo_mi355x;

struct Launch { bool last; uint32_t lgL, lgBn_or_N1, lgN2, lgT, grid_x, tw_scale; bool src_tmp, dst_tmp; };
static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_bad; std::printf("FAIL lg_n %u lgTE %u: %s (line %d)\n", lg_n, lgTE, #cond, __LINE__); } } while (0)

// the drivers before the plan existed: returns the number of launches, 0 when an axis does not fit
static uint32_t old_launches(uint32_t lg_n, uint32_t lgTE, Launch* out) {
  const uint32_t maxL = lgTE < 11 ? lgTE : 11;
  const uint32_t npass = lg_n <= maxL ? 1 : (lg_n <= 2 * maxL ? 2 : 3);
  uint32_t s1 = 0, s2 = 0, s3 = 0;
  if (npass == 1) s3 = lg_n;
  else if (npass == 2) { s1 = (lg_n + 1) / 2; s3 = lg_n - s1; }
  else { s1 = (lg_n + 2) / 3; s2 = (lg_n - s1 + 1) / 2; s3 = lg_n - s1 - s2; }
  if (s1 > maxL || s2 > maxL || s3 > maxL) return 0;
  auto lgT_for = [lgTE](uint32_t lgL, uint32_t lg_limit) { uint32_t lgT = lgTE - lgL; return lgT < lg_limit ? lgT : lg_limit; };
  if (npass == 1) {
    out[0] = Launch{true, s3, 0, 0, 0, 1, 0, false, false};
  } else if (npass == 2) {
    const uint32_t lgBn = s3, lgT = lgT_for(s1, lgBn), lgTf = lgT_for(s3, s1);
    out[0] = Launch{false, s1, lgBn, 0, lgT, 1u << (lgBn - lgT), 1, false, true};
    out[1] = Launch{true, s3, s1, 0, lgTf, 1u << (s1 - lgTf), 0, true, false};
  } else {
    const uint32_t lgBn1 = s2 + s3, lgT1 = lgT_for(s1, lgBn1), lgBn2 = s3, lgT2 = lgT_for(s2, lgBn2), lgTf = lgT_for(s3, s1);
    out[0] = Launch{false, s1, lgBn1, 0, lgT1, 1u << (lgBn1 - lgT1), 1, false, false};
    out[1] = Launch{false, s2, lgBn2, 0, lgT2, (1u << s1) << (lgBn2 - lgT2), 1u << s1, false, true};
    out[2] = Launch{true, s3, s1, s2, lgTf, (1u << s2) << (s1 - lgTf), 0, true, false};
  }
  return npass;
}

static void check_plans() {
  const uint32_t tiles[3] = {9, 11, 12};
  for (uint32_t lgTE : tiles)
    for (uint32_t lg_n = 1; lg_n <= 30; ++lg_n) {
      const uint32_t maxL = lgTE < 11 ? lgTE : 11;
      Launch old[3];
      const uint32_t n_old = old_launches(lg_n, lgTE, old);
      const NttPlan p = plan_passes(lg_n, lgTE);
      CHECK(p.npass == n_old);
      CHECK((n_old == 0) == (lg_n > 3 * maxL));
      uint32_t sum = 0;
      for (uint32_t i = 0; i < p.npass; ++i) {
        const NttPass& a = p.pass[i]; const Launch& o = old[i];
        const bool last = i + 1 == p.npass;
        CHECK(o.last == last);
        CHECK(a.lgL == o.lgL && a.lgT == o.lgT && a.grid_x == o.grid_x && a.src_tmp == o.src_tmp && a.dst_tmp == o.dst_tmp);
        if (last) CHECK(a.lgN1 == o.lgBn_or_N1 && a.lgN2 == o.lgN2);
        else CHECK(a.lgBn == o.lgBn_or_N1 && a.tw_scale == o.tw_scale);
        sum += a.lgL;
        CHECK(a.lgL <= maxL);
        CHECK(a.lgT + a.lgL <= lgTE);                                              // T * L <= 2^lgTE
        CHECK(((uint64_t)a.grid_x << (a.lgT + a.lgL)) == ((uint64_t)1 << lg_n));      // gridDim.x * T * L = 2^lg_n
        CHECK(a.lgT <= (last ? a.lgN1 : a.lgBn));                                  // a tile is no wider than the axis it runs along
      }
      if (p.npass) CHECK(sum == lg_n);
    }
}

static void check_forms() {
  const uint32_t lgTE = 0;
  struct { uint32_t lg_n; uint64_t batch; NttForm form; } edges[] = {
    {9, 1, NttForm::Tile2048},  {10, 1, NttForm::Latency512}, {10, 512, NttForm::Latency512}, {10, 513, NttForm::Tile2048},
    {18, 2, NttForm::Latency512}, {18, 3, NttForm::Tile2048}, {19, 1, NttForm::Tile2048},     {20, 1, NttForm::Tile4096},
    {20, 4, NttForm::Tile4096}, {22, 1, NttForm::Tile4096},   {23, 1, NttForm::Tile2048}};
  for (const auto& e : edges) { const uint32_t lg_n = e.lg_n; CHECK(choose_form(e.lg_n, e.batch) == e.form); }
}

int main() {
  check_plans();
  check_forms();
  std::printf("ntt plan: 90 plans, 11 form edges, %d failures\n", g_bad);
  return g_bad ? 1 : 0;
}
