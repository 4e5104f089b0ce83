// xyzz_law.h — the short-Weierstrass group law (a = 0) in extended Jacobian coordinates (X, Y, ZZ = Z^2, ZZZ = Z^3; x = X / ZZ, y = Y / ZZZ), written ONCE
// for every field whose operations return values the next operation accepts — no bound bookkeeping between them: HFq and HFq2 on the host
// (host_field.hpp, fully reduced) and the device's 32-bit Fq2 (g2.hip, components below 2q).  The lazy-bound G1 formulas of ec.h and the 28-bit forms
// of fp28.h / g2.hip carry their limb bounds step by step and stay their own text.
// A field F gives the static members zero, one, add, sub, dbl, mul, sqr (inv: to_affine only; load / store over LIMBS 64-bit words: the Jacobian
// readers only; from28 over WORDS28 32-bit words: law_point28 only) and the members is_zero() (zero mod q) and is_zero_raw() (all bits zero: how the
// identity's ZZ is stored; the same thing for a fully reduced field).  Plain C++: the CPU programs under tests/cpp include this through host_field.hpp.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#define ALEO_HD __host__ __device__
#else
#define ALEO_HD
#endif

namespace aleo_mi355x {

template <class F> struct XYZZOf {
  F X, Y, ZZ, ZZZ;
  ALEO_HD static XYZZOf infinity() { XYZZOf r; r.X = F::zero(); r.Y = r.X; r.ZZ = r.X; r.ZZZ = r.X; return r; }
  ALEO_HD bool is_inf() const { return ZZ.is_zero_raw(); }
};

template <class F> ALEO_HD inline XYZZOf<F> law_double(const XYZZOf<F>& p) {      // EFD dbl-2008-s-1
  if (p.is_inf()) return p;
  const F U = F::dbl(p.Y), V = F::sqr(U), W = F::mul(U, V), S = F::mul(p.X, V);
  const F xx = F::sqr(p.X), M = F::add(F::dbl(xx), xx);
  XYZZOf<F> r;
  r.X = F::sub(F::sqr(M), F::dbl(S));
  r.Y = F::sub(F::mul(M, F::sub(S, r.X)), F::mul(W, p.Y));
  r.ZZ = F::mul(V, p.ZZ); r.ZZZ = F::mul(W, p.ZZZ);
  if (r.ZZ.is_zero()) r = XYZZOf<F>::infinity();              // y == 0: a 2-torsion point
  return r;
}

template <class F> ALEO_HD inline XYZZOf<F> law_add(const XYZZOf<F>& a, const XYZZOf<F>& b) {      // EFD add-2008-s; the identity, doubling and cancellation included
  if (a.is_inf()) return b;
  if (b.is_inf()) return a;
  const F U1 = F::mul(a.X, b.ZZ), U2 = F::mul(b.X, a.ZZ), S1 = F::mul(a.Y, b.ZZZ), S2 = F::mul(b.Y, a.ZZZ);
  const F P = F::sub(U2, U1), R = F::sub(S2, S1);
  if (P.is_zero()) return R.is_zero() ? law_double(a) : XYZZOf<F>::infinity();
  const F PP = F::sqr(P), PPP = F::mul(P, PP), Q = F::mul(U1, PP);
  XYZZOf<F> r;
  r.X = F::sub(F::sub(F::sqr(R), PPP), F::dbl(Q));
  r.Y = F::sub(F::mul(R, F::sub(Q, r.X)), F::mul(S1, PPP));
  r.ZZ = F::mul(F::mul(a.ZZ, b.ZZ), PP);
  r.ZZZ = F::mul(F::mul(a.ZZZ, b.ZZZ), PPP);
  return r;
}

// (x, y) affine; false for the identity
template <class F> inline bool law_to_affine(const XYZZOf<F>& p, F& x, F& y) {
  if (p.is_inf()) return false;
  const F zi3 = F::inv(p.ZZZ), zi2 = F::sqr(F::mul(zi3, p.ZZ));      // 1 / Z^3, (Z^2 / Z^3)^2 = 1 / Z^2
  x = F::mul(p.X, zi2); y = F::mul(p.Y, zi3);
  return true;
}
// Jacobian (X, Y, Z) as snarkVM's Projective stores it (3 x F::LIMBS words) -> XYZZ
template <class F> inline XYZZOf<F> law_from_jacobian(const uint64_t* j) {
  XYZZOf<F> r; r.X = F::load(j); r.Y = F::load(j + F::LIMBS); const F Z = F::load(j + 2 * F::LIMBS);
  if (Z.is_zero()) return XYZZOf<F>::infinity();
  r.ZZ = F::sqr(Z); r.ZZZ = F::mul(r.ZZ, Z);
  return r;
}
// the affine-normalised point as Jacobian (x, y, 1); the identity as snarkVM's Projective::zero() = (1, 1, 0)
template <class F> inline void law_store_jacobian_normalized(uint64_t* j, const XYZZOf<F>& p) {
  F x = F::one(), y = F::one();
  const bool finite = law_to_affine(p, x, y);
  F::store(j, x); F::store(j + F::LIMBS, y); F::store(j + 2 * F::LIMBS, finite ? F::one() : F::zero());
}
// A point of the 28-bit forms as the device leaves it (fp28.h; G1's table path: 224 bytes, G2's pair form: 448): X | Y | ZZ | ZZZ, each coordinate
// F::WORDS28 words of loose 28-bit limbs; ZZ = 0 is the identity
template <class F> inline XYZZOf<F> law_point28(const char* p) {
  const uint32_t* w = (const uint32_t*)p;
  XYZZOf<F> v; v.X = F::from28(w); v.Y = F::from28(w + F::WORDS28); v.ZZ = F::from28(w + 2 * F::WORDS28); v.ZZZ = F::from28(w + 3 * F::WORDS28);
  if (v.ZZ.is_zero()) return XYZZOf<F>::infinity();
  return v;
}

}  // namespace aleo_mi355x
