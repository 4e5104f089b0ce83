"""The twisted Edwards model of BLS12-377 G1 (-x^2 + y^2 = 1 + d x^2 y^2) in Python integers: the ONE place its constants come from.

G1 is y^2 = x^3 + 1 over Fq.  It has the 2-torsion point (-1, 0) and 3 is a square mod q, so with s = 1/sqrt(3)
    u = s (x + 1), v = s y                 Montgomery   B v^2 = u^3 + A u^2 + u,   A = -3 s, B = s
    xt = u / v,  yt = (u - 1) / (u + 1)    Edwards      a xt^2 + yt^2 = 1 + dt xt^2 yt^2,   a = (A + 2) / B, dt = (A - 2) / B
    xe = f xt,  ye = yt,  f = sqrt(-a)     a = -1 form  -xe^2 + ye^2 = 1 + d xe^2 ye^2,      d = -dt / a
The two signs of sqrt(3) give two curves; both have -a a square.  The sign is fixed HERE (SQRT3, and F below) and everything else is derived:
tests/test_te28_model.py checks the derivation and the group laws against oracle/pyref.py, and `python tools/te28_model.py OUT` writes the
constants as limbs for the C++ side (aleo_amd/csrc/te28_consts.h) — the test reads them back from that file, they are typed nowhere.

d is a square (for either sign), so the unified law is NOT complete on all of E(Fq): a pair of points whose difference has even order gives Z3 = 0.
On the prime-order subgroup — all a snarkVM G1Affine can hold — it has no exception.  Two inputs have no finite image: (-1, 0) (v = 0) and any
point with u = -1; neither is in G1.
"""
import os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyref as R

Q = R.Q


def _inv(a): return pow(a % Q, -1, Q)
def _smaller_root(a):
    r = R.fq_sqrt(a)
    assert r is not None and r * r % Q == a % Q
    return min(r, Q - r)


# ---- the sign choices: the smaller root of 3, the smaller root of -a ---------------------------------------------------------------------
SQRT3 = _smaller_root(3)
S = _inv(SQRT3)
MONT_A, MONT_B = (-3 * S) % Q, S
TE_A, TE_D = (MONT_A + 2) * _inv(MONT_B) % Q, (MONT_A - 2) * _inv(MONT_B) % Q
F = _smaller_root(-TE_A)
D = (-TE_D) * _inv(TE_A) % Q          # d of the a = -1 form
K = 2 * D % Q                         # what the additions multiply T1 T2 by
IDENTITY = (0, 1)


def to_edwards(P):
    """affine short Weierstrass (None: infinity) -> affine (xe, ye); None when the point has no finite image"""
    if P is None: return IDENTITY
    x, y = P
    u, v = S * (x + 1) % Q, S * y % Q
    if v == 0 or (u + 1) % Q == 0: return None
    return (F * u * _inv(v) % Q, (u - 1) * _inv(u + 1) % Q)


def from_edwards(E):
    """affine (xe, ye) -> affine short Weierstrass; the identity (0, 1) -> None.  ((0, -1), the image of nothing finite above, is refused.)"""
    xe, ye = E
    if xe == 0:
        assert ye == 1, 'the 2-torsion point (0, -1) is not in the image of to_edwards'
        return None
    u = (1 + ye) * _inv(1 - ye) % Q
    v = F * u * _inv(xe) % Q
    return ((u * SQRT3 - 1) % Q, v * SQRT3 % Q)


def on_curve(E):
    x, y = E
    return (-x * x + y * y - 1 - D * x * x % Q * y * y) % Q == 0


def neg(E): return ((-E[0]) % Q, E[1])


# ---- extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z ---------------------------------------------------------------
def ext(E): return (E[0], E[1], 1, E[0] * E[1] % Q)
def row(E):
    """the precomputed affine row of the mixed addition: (y - x, y + x, 2 d x y); the identity's is (1, 1, 0)"""
    x, y = E
    return ((y - x) % Q, (y + x) % Q, K * x % Q * y % Q)
def row_neg(r): return (r[1], r[0], (-r[2]) % Q)


def _finish(A, B, C, Dd):
    E, Fv, G, H = (B - A) % Q, (Dd - C) % Q, (Dd + C) % Q, (B + A) % Q
    return (E * Fv % Q, G * H % Q, Fv * G % Q, E * H % Q)


def madd(P, r):
    """EFD madd-2008-hwcd-3 with Z2 = 1: seven products, unified (P == +-row's point included)"""
    X1, Y1, Z1, T1 = P
    return _finish((Y1 - X1) * r[0] % Q, (Y1 + X1) * r[1] % Q, T1 * r[2] % Q, 2 * Z1 % Q)


def add(P, S2):
    """EFD add-2008-hwcd-3: eight products and one by the constant k = 2d, unified"""
    X1, Y1, Z1, T1 = P; X2, Y2, Z2, T2 = S2
    return _finish((Y1 - X1) * (Y2 - X2) % Q, (Y1 + X1) * (Y2 + X2) % Q, T1 * K % Q * T2 % Q, 2 * Z1 * Z2 % Q)


def affine(P):
    """extended -> affine (xe, ye); None when Z == 0 (the exceptional pairs: operands that differ by a point of even order)"""
    X, Y, Z, T = P
    if Z % Q == 0: return None
    zi = _inv(Z)
    assert (X * Y - T * Z) % Q == 0
    return (X * zi % Q, Y * zi % Q)


# ---- the constants for the C++ side ------------------------------------------------------------------------------------------------------
# 28-bit form: value * 2^392 mod q as 14 exact base-2^28 digits (fp28.h); 32-bit form: value * 2^384 mod q as 12 words (fp.h)
CONSTANTS = {'TE_K': K, 'TE_D': D, 'TE_D_INV': _inv(D), 'TE_ONE': 1, 'TE_TWO': 2, 'TE_F': F, 'TE_F_INV': _inv(F), 'TE_S': S, 'TE_SQRT3': SQRT3}


def limbs28(v): m = v * (1 << 392) % Q; return [(m >> (28 * i)) & 0xfffffff for i in range(14)]
def limbs32(v): m = v * (1 << 384) % Q; return [(m >> (32 * i)) & 0xffffffff for i in range(12)]


def header_text():
    out = ['// te28_consts.h — written by tools/te28_model.py, which derives every value from its choice of sqrt(3) and sqrt(-a): do not edit.',
           '// NAME_28: value * 2^392 mod q, 14 x 28-bit digits (fp28.h); NAME_32: value * 2^384 mod q, 12 x 32-bit words (fp.h).',
           '#pragma once', '#include <stdint.h>', 'namespace aleo_mi355x {']
    for name, v in CONSTANTS.items():
        out.append('static constexpr uint32_t %s_28[14] = {%s};' % (name, ', '.join('0x%08xu' % w for w in limbs28(v))))
        out.append('static constexpr uint32_t %s_32[12] = {%s};' % (name, ', '.join('0x%08xu' % w for w in limbs32(v))))
    out.append('}  // namespace aleo_mi355x')
    return '\n'.join(out) + '\n'


if __name__ == '__main__':
    with open(sys.argv[1], 'w') as f:
        f.write(header_text())
