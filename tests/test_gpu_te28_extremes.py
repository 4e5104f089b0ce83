"""The Edwards-form point formulas (aleo_amd/csrc/te28.h) on the GPU at the EDGES of their stated invariants, against the group law in Python integers.

The MSM tests reach these formulas with whatever operands a sort produces.  Here the host builds every limb (aleo_mi355x_selftest_te28_rows: raw limbs in, raw
limbs out, the device converts nothing): each coordinate of an extended Edwards point is taken canonical or lifted by q to just below the invariant's 2q, with
Z = 1 and Z != 1; the cases the unified law must take in its stride (the same point, opposite points, the identity on either side or on both, an identity
base's row, negated rows, the first point of a slice) and the one it must REPORT (operands that differ by a point of order 2: Z3 == 0) sit in the first and the
last quad (lane) of a wave next to ordinary neighbours.  Every output row is checked exactly: exact digits below 2q, T Z = X Y, the affine sum carried back to
y^2 = x^3 + 1, pair == quad as points, the Z3 flag exactly where the model has it.  tests/test_te28_bounds.py runs the same formulas on the host over bounds;
this file runs the real kernels, product blocks included, over values."""
import ctypes, importlib.util, os
import numpy as np
import pytest

import aleo_amd
from oracle import pyref as p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('te28_model', os.path.join(ROOT, 'tools', 'te28_model.py'))
TE = importlib.util.module_from_spec(spec); spec.loader.exec_module(TE)
Q = p.Q
MASK = (1 << 28) - 1
R28 = (1 << 392) % Q
R28_INV = pow(R28, -1, Q)


def digits(v):
    assert v >> 364 < 1 << 32
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]


def value(limbs): return sum(int(l) << (28 * i) for i, l in enumerate(limbs))
def coord(v, lift): return digits(v * R28 % Q + lift * Q)          # canonical, or lifted by q: still below 2q


def point_row(P, z, lifts):
    """(x z : y z : z : x y z) of the Edwards image of the short-Weierstrass point P (None: the identity), coordinate i lifted by lifts[i] q"""
    x, y = TE.to_edwards(P)
    return coord(x * z, lifts[0]) + coord(y * z, lifts[1]) + coord(z, lifts[2]) + coord(x * y % Q * z, lifts[3])


def entry_row(P):
    r = TE.row(TE.to_edwards(P))
    return coord(r[0], 0) + coord(r[1], 0) + coord(r[2], 0)


def check_point_row(row, want, where):
    f = [[int(v) for v in row[14 * k:14 * k + 14]] for k in range(4)]
    for name, c in zip('XYZT', f):
        assert all(l <= MASK for l in c[:13]) and value(c) < 2 * Q, (where, name, 'not exact digits below 2q')
    X, Y, Z, T = (value(c) * R28_INV % Q for c in f)
    assert Z != 0, (where, 'Z is 0 mod q')
    assert T * Z % Q == X * Y % Q, (where, 'T Z != X Y')
    zi = pow(Z, -1, Q)
    e = (X * zi % Q, Y * zi % Q)
    assert TE.on_curve(e) and TE.from_edwards(e) == want, (where, 'not the affine sum')
    return e


LIFTS = [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)]


def build_cases():
    G1 = p.G1_GENERATOR
    P = [G1]
    for _ in range(11): P.append(p.g1_add(P[-1], G1))
    w = (p.fq_sqrt(-3 % Q) - 1) * pow(2, -1, Q) % Q
    S2 = next(T for T in ((-w % Q, 0), (-w * w % Q, 0)) if TE.to_edwards(p.g1_add(P[2], T)) is not None)      # order 2, at infinity of the Edwards model
    zs = [1, 0x1234567 * R28 % Q, pow(3, 300, Q)]
    pt = lambda i: P[i % len(P)]

    special = []
    for a in range(4):
        for b in range(4):
            za, zb = zs[(a + b) % 3], zs[(a + 2 * b + 1) % 3]
            special += [(pt(a + b), za, LIFTS[a], pt(a + b), zb, LIFTS[b]),                  # the same point: no doubling branch
                        (pt(a + b), za, LIFTS[a], p.g1_neg(pt(a + b)), zb, LIFTS[b]),        # opposite points: the identity comes out as a point
                        (pt(a + b), za, LIFTS[a], p.g1_add(pt(a + b), S2), zb, LIFTS[b])]    # the exceptional pair: Z3 == 0 must be reported
        special += [(None, zs[a % 3], LIFTS[a], pt(a), zs[(a + 1) % 3], LIFTS[(a + 1) % 4]), (pt(a), zs[a % 3], LIFTS[a], None, zs[(a + 2) % 3], LIFTS[(a + 2) % 4]),
                    (None, zs[a % 3], LIFTS[a], None, zs[(a + 1) % 3], LIFTS[3 - a])]
    adds, k = [], 0
    while special:
        for slot in range(16):
            if slot in (0, 15) and special: adds.append(special.pop())
            else: adds.append((pt(k), zs[k % 3], LIFTS[k % 4], pt(k + 1 + k % 5), zs[(k // 3) % 3], LIFTS[(k // 4) % 4])); k += 1
    adds[-1], adds[-4] = adds[-4], adds[-1]
    adds = adds[:-3]                                            # the last block is not full, the last quad of the run is a special one
    A = np.array([point_row(pa, za, la) for pa, za, la, _, _, _ in adds], dtype=np.uint32)
    B = np.array([point_row(pb, zb, lb) for _, _, _, pb, zb, lb in adds], dtype=np.uint32)
    add_zero = [TE.add(TE.ext(TE.to_edwards(pa)), TE.ext(TE.to_edwards(pb)))[2] == 0 for pa, _, _, pb, _, _ in adds]
    add_want = [p.g1_add(pa, pb) for pa, _, _, pb, _, _ in adds]

    madds = []                                                  # (acc point, entry point, negated, first)
    for lane in range(64 * 10 + 40):
        wv, l = divmod(lane, 64)
        accp = None if lane % 13 == 5 else pt(lane)
        neg, first = (lane // 3) & 1, lane % 7 == 3
        if l in (0, 63):
            e = [accp, p.g1_neg(accp), p.g1_add(accp, S2), None][wv % 4] if accp is not None else pt(lane + 1)      # P = acc, P = -acc, the exceptional pair, an identity base
            first = False
        else: e = None if lane % 17 == 9 else pt(lane + 1 + lane % 4)
        madds.append((accp, e, neg, first))
    ACC = np.array([point_row(a, zs[i % 3], LIFTS[(i // 2) % 4]) for i, (a, _, _, _) in enumerate(madds)], dtype=np.uint32)
    ROW = np.array([entry_row(e) for _, e, _, _ in madds], dtype=np.uint32)
    HOW = np.array([n | (2 if f else 0) for _, _, n, f in madds], dtype=np.uint8)
    signed = lambda e, n: p.g1_neg(e) if n else e
    madd_want = [signed(e, n) if f else p.g1_add(a, signed(e, n)) for a, e, n, f in madds]
    madd_zero = [(not f) and TE.madd(TE.ext(TE.to_edwards(a)), TE.row(TE.to_edwards(signed(e, n))))[2] == 0 for a, e, n, f in madds]
    return dict(adds=adds, add_want=add_want, add_zero=add_zero, A=A, B=B, madds=madds, madd_want=madd_want, madd_zero=madd_zero, ACC=ACC, ROW=ROW, HOW=HOW)


@pytest.fixture(scope='module')
def cases():
    """Inputs, expected sums and ONE run of the kernels, shared by every test below."""
    c = build_cases()
    L = aleo_amd.lib()
    aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    A, B, ACC, ROW, HOW = c['A'], c['B'], c['ACC'], c['ROW'], c['HOW']
    out_pair, out_quad, z_add = np.zeros_like(A), np.zeros_like(A), np.full(len(A), 0xA5A5A5A5, dtype=np.uint32)
    out_acc, z_madd = np.zeros_like(ACC), np.zeros(len(ACC), dtype=np.uint8)
    aleo_amd._lib.check(L.aleo_mi355x_selftest_te28_rows(vp(A), vp(B), len(A), vp(out_pair), vp(out_quad), vp(z_add), vp(ACC), vp(ROW), vp(HOW), len(ACC), vp(out_acc), vp(z_madd)),
                        'selftest_te28_rows')
    c.update(out_pair=out_pair, out_quad=out_quad, z_add=z_add, out_acc=out_acc, z_madd=z_madd)
    return c


def test_inputs_cover_the_edges(cases):
    adds = cases['adds']
    kinds = {'same': 0, 'opposite': 0, 'identity_operand': 0, 'both_identity': 0, 'exceptional': sum(cases['add_zero'])}
    for pa, _, _, pb, _, _ in adds:
        if pa is None and pb is None: kinds['both_identity'] += 1
        elif pa is None or pb is None: kinds['identity_operand'] += 1
        elif pa == pb: kinds['same'] += 1
        elif pa == p.g1_neg(pb): kinds['opposite'] += 1
    assert all(v >= 4 for v in kinds.values()) and kinds['exceptional'] >= 16, kinds
    assert len(adds) % 64 != 0 and all(s % 16 in (0, 15) or s == len(adds) - 1 for s, z in enumerate(cases['add_zero']) if z)
    assert max(value(r[:14]) for r in cases['A']) > Q and max(value(r[28:42]) for r in cases['B']) > Q      # lifted representatives
    m = cases['madds']
    assert sum(cases['madd_zero']) >= 2 and sum(f for _, _, _, f in m) >= 50 and sum(a is None for a, _, _, _ in m) >= 20 and sum(e is None for _, e, _, _ in m) >= 20
    assert sum(a is not None and a == e for a, e, _, _ in m) >= 2 and sum(w is None for w in cases['madd_want']) >= 2


def test_pair_and_quad_sums_keep_the_stored_invariant_and_equal_the_group_law(cases):
    for i, (want, zero, z) in enumerate(zip(cases['add_want'], cases['add_zero'], cases['z_add'])):
        assert int(z) == (3 if zero else 0), (i, 'Z3 == 0 reported by the wrong forms', int(z))
        if zero: continue
        ep = check_point_row(cases['out_pair'][i], want, ('pair', i))
        assert check_point_row(cases['out_quad'][i], want, ('quad', i)) == ep


def test_mixed_addition_and_first_point(cases):
    for i, (want, zero, z) in enumerate(zip(cases['madd_want'], cases['madd_zero'], cases['z_madd'])):
        assert int(z) == int(zero), (i, 'Z3 flag')
        if not zero: check_point_row(cases['out_acc'][i], want, ('madd', i, cases['madds'][i][2:]))


def test_bad_arguments_are_refused():
    L = aleo_amd.lib()
    assert L.aleo_mi355x_selftest_te28_rows(None, None, 1, None, None, None, None, None, None, 0, None, None) == 2
    assert L.aleo_mi355x_selftest_te28_rows(None, None, 0, None, None, None, None, None, None, (1 << 20) + 1, None, None) == 2
