"""The 28-bit-limb point formulas (aleo_amd/csrc/fp28.h) on the GPU at the EDGES of their stated invariants, against the group law in Python integers.

The other tests of this code use pseudo-random canonical operands, so representatives near 2q / 6q / 12q, limbs near 3 * 2^28, the 2-torsion point and
points with an all-zero X never reach the kernels.  Here the host builds every limb (aleo_mi355x_selftest_f28_rows: raw limbs in, raw limbs out, the device
converts nothing): each coordinate of a point on y^2 = x^3 + 1 is lifted to the representatives the stored invariant allows, the special cases (same x,
identity operands, 2-torsion) sit in the first and the last quad (lane) of a wave next to ordinary neighbours, so the rare branch runs under divergence,
and every output row is checked exactly: invariant, ZZ^3 = ZZZ^2, the affine sum, pair == quad, the refusal flag of the mixed addition.
tests/test_fp28_bounds.py runs the same formulas on the host over bounds; this file runs the real kernels, product blocks included, over values.
"""
import ctypes
import numpy as np
import pytest

import aleo_amd
from aleo_amd import synth

pytestmark = pytest.mark.gpu

Q = synth.FQ_MODULUS
MASK = (1 << 28) - 1
R28 = (1 << 392) % Q                       # a residue v is stored as v * 2^392 mod q (+ k q)
R28_INV = pow(R28, -1, Q)
L3 = 3 << 28


# ---- the group law on y^2 = x^3 + 1, affine, None = the identity ----------------------------------------------------------------------------------
def add(p, q):
    if p is None: return q
    if q is None: return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if y1 != y2 or y1 == 0: return None                    # opposite points; (-1, 0) doubled
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return x3, (lam * (x1 - x3) - y1) % Q


def neg(p): return None if p is None else (p[0], -p[1] % Q)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------
def digits(v):
    assert v >> 364 < 1 << 32
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]


def value(limbs): return sum(int(l) << (28 * i) for i, l in enumerate(limbs))


def relimb_up(d):
    """Same value, limbs raised towards 3 * 2^28 - 1: every limb lends two units to the one below."""
    d = list(d)
    for i in range(12, -1, -1):
        k = min(2, d[i + 1]); d[i + 1] -= k; d[i] += k << 28
    return d


def spread_kq(K, S):
    d = digits(K * Q)
    return [d[i] + ((S << 28) if i < 13 else 0) - (S if i > 0 else 0) for i in range(14)]


def l2_negation(y_digits):                 # f28_sub<2, 1>(0, y): limb-wise 2q - y
    return [c - y for c, y in zip(spread_kq(2, 1), y_digits)]


# (k_X, k_Y, k_ZZ, k_ZZZ, Y re-limbed): canonical; the largest exact lift below 12q / 6q / 2q; the same with Y's limbs raised; a mix
REPS = [(0, 0, 0, 0, False), (11, 5, 1, 1, False), (11, 5, 1, 1, True), (0, 0, 1, 0, True)]


def point_row(p, z, rep):
    if p is None: return [0] * 56
    kx, ky, kzz, kzzz, relimb = rep
    zz, zzz = z * z % Q, z * z * z % Q
    y = digits(p[1] * zzz * R28 % Q + ky * Q)
    return digits(p[0] * zz * R28 % Q + kx * Q) + (relimb_up(y) if relimb else y) + digits(zz * R28 % Q + kzz * Q) + digits(zzz * R28 % Q + kzzz * Q)


def row_fields(row): return [[int(v) for v in row[14 * f:14 * f + 14]] for f in range(4)]


def check_point_row(row, want, y_exact_below_2q, where):
    """A stored point (or, with y_exact_below_2q, the accumulator of the mixed addition) against the invariant of fp28.h and the affine point `want`."""
    X, Y, ZZ, ZZZ = row_fields(row)
    if want is None:
        assert not any(ZZ), (where, 'expected the identity: ZZ all zero')
        return
    assert any(ZZ), (where, 'the identity where a finite point is expected')
    for name, f, bound in (('X', X, 12), ('ZZ', ZZ, 2), ('ZZZ', ZZZ, 2)):
        assert all(l <= MASK for l in f[:13]) and value(f) < bound * Q, (where, name, 'exact digits below %dq' % bound)
    if y_exact_below_2q: assert all(l <= MASK for l in Y[:13]) and value(Y) < 2 * Q, (where, 'Y exact digits below 2q')
    else: assert all(l < L3 for l in Y) and value(Y) < 6 * Q, (where, 'Y class L3 below 6q')
    x, y, zz, zzz = (value(f) * R28_INV % Q for f in (X, Y, ZZ, ZZZ))
    assert zz != 0, (where, 'ZZ is 0 mod q but not all zero')
    assert pow(zz, 3, Q) == zzz * zzz % Q, (where, 'ZZ^3 != ZZZ^2')
    assert (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q) == want, (where, 'not the affine sum')


def build_cases():
    """The rows and what they must sum to (no GPU)."""
    G1 = synth.G1_GENERATOR
    P = [G1]
    for _ in range(11): P.append(add(P[-1], G1))
    P[1] = add(G1, G1)
    T, W = (Q - 1, 0), (0, 1)                                   # 2-torsion; X all zero while ZZ is not
    zs = [1, 0x1234567 * R28 % Q, pow(3, 300, Q)]
    pt = lambda i: P[i % len(P)]

    # additions: specials in the first and the last quad of a wave (16 quads), ordinary sums of distinct points elsewhere
    special = []
    for a in range(4):
        for b in range(4):
            za, zb = zs[(a + b) % 3], zs[(a + 2 * b + 1) % 3]
            special += [(pt(a + b), za, REPS[a], pt(a + b), zb, REPS[b]),             # the same point, other representatives and Z: doubling
                        (pt(a + b), za, REPS[a], neg(pt(a + b)), zb, REPS[b]),        # opposite points: the identity
                        (T, za, REPS[a], T, zb, REPS[b]),                             # (-1, 0) + (-1, 0): the Y == 0 branch of the doubling
                        (W, za, REPS[a], W if a & 1 else neg(W), zb, REPS[b])]        # (0, +-1): X all zero
        special += [(None, 1, REPS[0], pt(a), zs[a % 3], REPS[a]), (pt(a), zs[a % 3], REPS[a], None, 1, REPS[0]), (None, 1, REPS[0], None, 1, REPS[0])]
    adds = []
    k = 0
    while special:
        for slot in range(16):
            if slot in (0, 15) and special: adds.append(special.pop())
            else:
                a, b = k % 4, (k // 4) % 4
                other = [pt(k + 1 + k % 5), T, W, neg(W)][(k // 16) % 4] if k % 3 == 0 else pt(k + 1 + k % 5)
                adds.append((pt(k), zs[k % 3], REPS[a], other, zs[(k // 3) % 3], REPS[b])); k += 1
    adds[-1], adds[-4] = adds[-4], adds[-1]
    adds = adds[:-3]                                            # the last block is not full, the last quad of the run is a special one
    assert len(adds) <= 4096 and all(pa is None or pb is None or pa[0] != pb[0] or s % 16 in (0, 15) or s == len(adds) - 1 for s, (pa, _, _, pb, _, _) in enumerate(adds))
    A = np.array([point_row(pa, za, ra) for pa, za, ra, _, _, _ in adds], dtype=np.uint32)
    B = np.array([point_row(pb, zb, rb) for _, _, _, pb, zb, rb in adds], dtype=np.uint32)
    add_want = [add(pa, pb) for pa, _, _, pb, _, _ in adds]

    # mixed additions: acc = point with Z (X below 12q, Y below 2q) or the slice's first point (x, +-y, 1, 1); the refused ones (P = +-acc) in the
    # first and the last lane of a wave
    def acc_row(p, z, lift, first, negated):
        if first:
            y = digits(-p[1] % Q * R28 % Q) if negated else digits(p[1] * R28 % Q)      # the entry of -p, negated limb-wise, is p again
            return digits(p[0] * R28 % Q) + (l2_negation(y) if negated else y) + digits(R28) + digits(R28)
        return point_row(p, z, (11 * lift, lift, lift, 1 - lift, False))

    def entry_row(p, negated):
        y = digits(-p[1] % Q * R28 % Q) if negated else digits(p[1] * R28 % Q)
        return digits(p[0] * R28 % Q) + (l2_negation(y) if negated else y)

    madds = []
    for lane in range(64 * 14 + 40):
        w, l = divmod(lane, 64)
        accp = [pt(lane), pt(lane), T, W][(lane // 7) % 4] if lane % 5 == 0 else pt(lane)
        first = lane % 3 == 1 and accp not in (T,)
        if l in (0, 63): p = accp if w & 1 else neg(accp)       # refused
        else: p = [pt(lane + 1 + lane % 4), W, T][(lane // 11) % 3] if lane % 4 == 2 else pt(lane + 1 + lane % 4)
        if p[0] == accp[0] and l not in (0, 63): p = pt(lane + 6)
        madds.append((acc_row(accp, zs[lane % 3], (lane // 2) & 1, first, lane & 1), entry_row(p, (lane // 3) & 1), accp, p))
    ACC = np.array([m[0] for m in madds], dtype=np.uint32)
    PT = np.array([m[1] for m in madds], dtype=np.uint32)

    return dict(adds=adds, add_want=add_want, A=A, B=B, madds=madds, ACC=ACC, PT=PT)


@pytest.fixture(scope='module')
def cases():
    """Inputs, expected sums and ONE run of the kernels, shared by every test below."""
    c = build_cases()
    L = aleo_amd.lib()
    aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    A, B, ACC, PT = c['A'], c['B'], c['ACC'], c['PT']
    out_pair, out_quad, out_acc, ok = np.zeros_like(A), np.zeros_like(A), np.zeros_like(ACC), np.zeros(len(ACC), dtype=np.uint8)
    aleo_amd._lib.check(L.aleo_mi355x_selftest_f28_rows(vp(A), vp(B), len(A), vp(out_pair), vp(out_quad), vp(ACC), vp(PT), len(ACC), vp(out_acc), vp(ok)), 'selftest_f28_rows')
    c.update(out_pair=out_pair, out_quad=out_quad, out_acc=out_acc, ok=ok)
    return c


def test_inputs_cover_the_edges(cases):
    """The row set itself: every branch and representative the issue of this test names is present, at a wave's edge where it is a rare one."""
    adds, want = cases['adds'], cases['add_want']
    kinds = {'double': 0, 'opposite': 0, 'two_torsion': 0, 'identity_operand': 0, 'x_zero': 0}
    for s, (pa, _, _, pb, _, _) in enumerate(adds):
        if pa is None or pb is None: kinds['identity_operand'] += 1
        elif pa == pb and pa[1] == 0: kinds['two_torsion'] += 1
        elif pa == pb: kinds['double'] += 1
        elif pa[0] == pb[0]: kinds['opposite'] += 1
        if pa is not None and pa[0] == 0: kinds['x_zero'] += 1
    assert all(v >= 8 for v in kinds.values()), kinds
    assert sum(w is None for w in want) >= 40 and len(adds) % 64 != 0
    rows = np.array([point_row(pa, za, ra) for pa, za, ra, _, _, _ in adds if pa is not None], dtype=np.uint64)
    assert rows[:, 14:27].max() >= L3 - (1 << 20) and max(value(r[:14]) for r in rows) > 11 * Q and max(value(r[14:28]) for r in rows) > 5 * Q
    refused = [m[2][0] == m[3][0] for m in cases['madds']]
    assert sum(refused) >= 28 and all(r == (i % 64 in (0, 63)) for i, r in enumerate(refused))


def test_pair_and_quad_sums_keep_the_stored_invariant_and_equal_the_group_law(cases):
    for form in ('out_pair', 'out_quad'):
        for i, (row, want) in enumerate(zip(cases[form], cases['add_want'])):
            check_point_row(row, want, False, (form, i))


def test_pair_and_quad_agree_as_residues(cases):
    for i, (rp, rq) in enumerate(zip(cases['out_pair'], cases['out_quad'])):
        fp, fq = row_fields(rp), row_fields(rq)
        assert any(fp[2]) == any(fq[2]), i
        if any(fp[2]): assert [value(f) % Q for f in fp] == [value(f) % Q for f in fq], i      # the same formulas: all four coordinates, not only the point


def test_mixed_addition_refuses_exactly_p_equal_plus_minus_acc_and_sums_the_rest(cases):
    for i, ((acc_in, _, accp, p), out, ok) in enumerate(zip(cases['madds'], cases['out_acc'], cases['ok'])):
        assert ok in (0, 1), (i, 'the flag was not written')
        assert bool(ok) == (accp[0] != p[0]), (i, 'refused' if not ok else 'accepted P == +-acc')
        if not ok: assert [int(v) for v in out] == acc_in, (i, 'acc changed by a refused addition')
        else: check_point_row(out, add(accp, p), True, ('madd', i))


def test_bad_arguments_are_refused():
    L = aleo_amd.lib()
    assert L.aleo_mi355x_selftest_f28_rows(None, None, 1, None, None, None, None, 0, None, None) == 2
    assert L.aleo_mi355x_selftest_f28_rows(None, None, 0, None, None, None, None, (1 << 20) + 1, None, None) == 2
