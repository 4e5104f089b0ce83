// te28_host.hpp — the host's side of the Edwards tier (te28.h): an extended Edwards point as the device leaves it -> the XYZZ point of the same group
// element on y^2 = x^3 + 1, the inverse of the map of tools/te28_model.py written projectively (no inversion: the call's tail normalises once, at its end).
#pragma once
#include "host_field.hpp"
#include "te28_consts.h"

namespace aleo_mi355x {
namespace host {

inline HFq hfq_of32(const uint32_t (&w)[12]) { HFq r; for (int i = 0; i < 6; ++i) r.l[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32); return r; }

// (X : Y : Z : T), 56 bytes of loose 28-bit limbs each.  With u = (Z + Y) / (Z - Y) and v = f u Z / X:  x = sqrt(3) u - 1, y = sqrt(3) v, so over the
// common denominator J = (Z - Y) X:   x = (sqrt(3) (Z + Y) - (Z - Y)) X / J,   y = sqrt(3) f (Z + Y) Z / J   ->   XYZZ with ZZ = J^2, ZZZ = J^3.
// The identity (0 : Z : Z : 0) becomes the XYZZ identity; (0 : -Z : Z : 0), which no point of G1 reaches, is the 2-torsion point (-1, 0).
// *z_zero is set when Z == 0 (mod q): no point at all — an addition whose operands differed by a point of even order went unreported.
inline HXYZZ te_point28(const char* p, bool* z_zero) {
  const uint32_t* w = (const uint32_t*)p;
  const HFq X = HFq::from28(w), Y = HFq::from28(w + 14), Z = HFq::from28(w + 28);
  if (Z.is_zero()) { *z_zero = true; return HXYZZ::infinity(); }
  if (X.is_zero()) {
    if (Y == Z) return HXYZZ::infinity();
    HXYZZ t; t.X = HFq::neg(HFq::one()); t.Y = HFq::zero(); t.ZZ = HFq::one(); t.ZZZ = HFq::one(); return t;
  }
  static const HFq s3 = hfq_of32(TE_SQRT3_32), s3f = HFq::mul(hfq_of32(TE_SQRT3_32), hfq_of32(TE_F_32));
  const HFq zmy = HFq::sub(Z, Y), zpy = HFq::add(Z, Y), J = HFq::mul(zmy, X);
  HXYZZ r;
  r.ZZ = HFq::sqr(J); r.ZZZ = HFq::mul(r.ZZ, J);
  r.X = HFq::mul(HFq::mul(HFq::sub(HFq::mul(s3, zpy), zmy), X), J);
  r.Y = HFq::mul(HFq::mul(HFq::mul(s3f, zpy), Z), r.ZZ);
  return r;
}

}  // namespace host
}  // namespace aleo_mi355x
