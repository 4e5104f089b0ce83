// The affine group law on y^2 = x^3 + 1 over host_field.hpp's HFq, with square roots and pseudo-random points: the reference of the host programs that check
// the G1 point formulas (tests/cpp/fp28_bounds_emul.cpp, te28_bounds_emul.cpp).  Included after checked_f28.h, whose generator it draws from.
#pragma once
struct Aff { bool inf; HFq x, y; };
static Aff aff_inf() { Aff r; r.inf = true; r.x = HFq::zero(); r.y = HFq::zero(); return r; }
static Aff aff_neg(const Aff& p) { Aff r = p; r.y = HFq::neg(p.y); return r; }
static Aff aff_add(const Aff& p, const Aff& q) {
  if (p.inf) return q;
  if (q.inf) return p;
  HFq lam;
  if (p.x == q.x) {
    if (!(p.y == q.y) || p.y.is_zero()) return aff_inf();                       // opposite points, the 2-torsion point (-1, 0) twice
    const HFq xx = HFq::sqr(p.x); lam = HFq::mul(HFq::add(HFq::dbl(xx), xx), HFq::inv(HFq::dbl(p.y)));
  } else lam = HFq::mul(HFq::sub(q.y, p.y), HFq::inv(HFq::sub(q.x, p.x)));
  Aff r; r.inf = false;
  r.x = HFq::sub(HFq::sub(HFq::sqr(lam), p.x), q.x);
  r.y = HFq::sub(HFq::mul(lam, HFq::sub(p.x, r.x)), p.y);
  return r;
}
static bool on_curve(const Aff& p) { return p.inf || HFq::sqr(p.y) == HFq::add(HFq::mul(HFq::sqr(p.x), p.x), HFq::one()); }
// Tonelli-Shanks: q - 1 = 2^46 t
static bool fq_sqrt(HFq& r, const HFq& a) {
  static uint64_t t[6], th[6], half[6]; static HFq c; static bool init = false;
  if (!init) {
    Big qm1 = QB; qm1.w[0] -= 1;
    const Big tb = big_shr(qm1, 46), thb = big_shr(tb, 1), hb = big_shr(qm1, 1);
    for (int i = 0; i < 6; ++i) { t[i] = tb.w[i]; th[i] = thb.w[i]; half[i] = hb.w[i]; }
    for (uint64_t z = 2;; ++z) { const HFq zz = HFq::from_u64(z); if (!(HFq::pow(zz, half, 6) == HFq::one())) { c = HFq::pow(zz, t, 6); break; } }
    init = true;
  }
  if (a.is_zero()) { r = a; return true; }
  if (!(HFq::pow(a, half, 6) == HFq::one())) return false;
  const HFq w = HFq::pow(a, th, 6);                          // a^((t - 1) / 2)
  HFq x = HFq::mul(a, w), b = HFq::mul(x, w), z = c; int m = 46;
  while (!(b == HFq::one())) {
    int k = 0; HFq b2 = b; while (!(b2 == HFq::one())) { b2 = HFq::sqr(b2); ++k; }
    HFq g = z; for (int i = 0; i < m - k - 1; ++i) g = HFq::sqr(g);
    x = HFq::mul(x, g); z = HFq::sqr(g); b = HFq::mul(b, z); m = k;
  }
  r = x; return true;
}
static Aff rnd_point() { for (;;) { Aff p; p.inf = false; p.x = rnd_fq(); if (fq_sqrt(p.y, HFq::add(HFq::mul(HFq::sqr(p.x), p.x), HFq::one()))) return p; } }
