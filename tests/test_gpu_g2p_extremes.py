"""The G2 lane-pair formulas (aleo_amd/csrc/g2p28.h) on the GPU at the EDGES of their stated invariant, against the group law in Python integers.

The other tests of this code (aleo_mi355x_selftest_g2pair, the G2 MSM against the oracle) use canonical points of the prime-order subgroup: no component
of a coordinate is ever 0, no y is 0, no representative is lifted, and one hand-written device form is compared with another.  Here the host builds every
limb (aleo_mi355x_selftest_g2p_rows: raw limbs in, raw limbs out, the device converts nothing).  The a = 0 formulas never use the curve's b, so every case
brings its own curve y^2 = x^3 + b over Fq2 on which both operands lie (asserted) — which makes the special inputs constructible without a square root:
pick x1, x2, w, then y1 = ((x2^3 - x1^3) / w - w) / 2 and y2 = y1 + w; y = 0 with b = -x^3 for 2-torsion; x = 0 with b = y^2.  Each component of each
coordinate is lifted on its own to the representatives the stored invariant allows (X < 12q, Y < 6q, ZZ / ZZZ < 2q), Z is 1, a base-field value or a
general one, the special cases sit in the first and the last lane pair of a wave next to ordinary neighbours, the last block is partial, and every output
row is checked exactly.  tests/test_g2p28_bounds.py runs the same source on the host over bounds; this file runs the real kernels over values.
"""
import ctypes, random
import numpy as np
import pytest

import aleo_amd
from aleo_amd import synth
from oracle import pyref as p

Q = synth.FQ_MODULUS
MASK = (1 << 28) - 1
R28 = (1 << 392) % Q                       # a residue v is stored as v * 2^392 mod q (+ k q)
R28_INV = pow(R28, -1, Q)
FILL = 0xA5A5A5A5
WAVE = 32                                  # lane pairs per wave; a block is two waves
assert pow(5, (Q - 1) // 2, Q) != 1        # 5 is a non-residue mod q, so a square of Fq2 (ZZ3 is one) is never (0, w) with w != 0: only (z, 0) can occur


# ---- Fq2 and the affine group law on y^2 = x^3 + b (b never enters), None = the identity ------------------------------------------------------------
def cube(x): return p.fq2_mul(p.fq2_mul(x, x), x)
def fneg(x): return (-x[0] % Q, -x[1] % Q)
def curve_b(P): return p.fq2_sub(p.fq2_mul(P[1], P[1]), cube(P[0]))
def same_curve(A, B): return A is None or B is None or curve_b(A) == curve_b(B)
def neg(P): return None if P is None else (P[0], fneg(P[1]))


def add(A, B):
    if A is None: return B
    if B is None: return A
    (x1, y1), (x2, y2) = A, B
    if x1 == x2:
        if y1 != y2 or y1 == (0, 0): return None               # opposite points; a 2-torsion point twice
        lam = p.fq2_mul(p.fq2_mul((3, 0), p.fq2_mul(x1, x1)), p.fq2_inv(p.fq2_add(y1, y1)))
    else:
        lam = p.fq2_mul(p.fq2_sub(y2, y1), p.fq2_inv(p.fq2_sub(x2, x1)))
    x3 = p.fq2_sub(p.fq2_sub(p.fq2_mul(lam, lam), x1), x2)
    return x3, p.fq2_sub(p.fq2_mul(lam, p.fq2_sub(x1, x3)), y1)


def pair_on_a_curve(x1, x2, w):
    """Two points with these x on one curve, their y apart by w."""
    y1 = p.fq2_mul(p.fq2_sub(p.fq2_mul(p.fq2_sub(cube(x2), cube(x1)), p.fq2_inv(w)), w), p.fq2_inv((2, 0)))
    A, B = (x1, y1), (x2, p.fq2_add(y1, w))
    assert same_curve(A, B) and x1 != x2
    return A, B


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------------
def digits(v):
    assert v >> 364 < 1 << 32
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]


def value(limbs): return sum(int(l) << (28 * i) for i, l in enumerate(limbs))


# the lift of each component, in the stored order X.a X.b Y.a Y.b ZZ.a ZZ.b ZZZ.a ZZZ.b: canonical; the largest exact lift below 12q / 6q / 2q; the
# a- and the b-components lifted differently, both ways; a mix
REPS = [(0,) * 8, (11, 11, 5, 5, 1, 1, 1, 1), (11, 0, 0, 5, 1, 0, 0, 1), (0, 11, 5, 0, 0, 1, 1, 0), (7, 3, 2, 4, 0, 0, 1, 1)]
BOUNDS = (12, 12, 6, 6, 2, 2, 2, 2)


def point_row(P, z, rep):
    """448 bytes: (x z^2, y z^3, z^2, z^3), component by component, each lifted by its k q."""
    if P is None: return [0] * 112
    zz = p.fq2_mul(z, z); zzz = p.fq2_mul(zz, z)
    X, Y = p.fq2_mul(P[0], zz), p.fq2_mul(P[1], zzz)
    row = []
    for v, k in zip((X[0], X[1], Y[0], Y[1], zz[0], zz[1], zzz[0], zzz[1]), rep): row += digits(v * R28 % Q + k * Q)
    return row


def entry_row(P, lifts=(0, 0, 0, 0)):
    """224 bytes: x.a | y.a | x.b | y.b, canonical or lifted by q (an entry is exact digits below 2q)."""
    return sum((digits(v * R28 % Q + k * Q) for v, k in zip((P[0][0], P[1][0], P[0][1], P[1][1]), lifts)), [])


def fields(row): return [[int(v) for v in row[14 * f:14 * f + 14]] for f in range(8)]


def check_point_row(row, want, where):
    """A stored point against the stored invariant of g2p28.h and the affine point `want`."""
    F = fields(row)
    if want is None:
        assert not any(int(v) for v in row), (where, 'expected the identity: every field all zero')
        return
    assert all(l != FILL for f in F for l in f), (where, 'a limb was left at the fill pattern')
    for name, f, bound in zip(('X.a', 'X.b', 'Y.a', 'Y.b', 'ZZ.a', 'ZZ.b', 'ZZZ.a', 'ZZZ.b'), F, BOUNDS):
        assert all(l <= MASK for l in f[:13]) and value(f) < bound * Q, (where, name, 'exact digits below %dq' % bound)
    assert any(F[4]) or any(F[5]), (where, 'the identity where a finite point is expected')
    X, Y, ZZ, ZZZ = (tuple(value(F[2 * i + c]) * R28_INV % Q for c in (0, 1)) for i in range(4))
    assert ZZ != (0, 0), (where, 'ZZ is 0 in Fq2 but not stored as the identity')
    assert cube(ZZ) == p.fq2_mul(ZZZ, ZZZ), (where, 'ZZ^3 != ZZZ^2')
    assert (p.fq2_mul(X, p.fq2_inv(ZZ)), p.fq2_mul(Y, p.fq2_inv(ZZZ))) == want, (where, 'not the affine sum')


def build_cases():
    """The rows, their kinds and what they must give (no GPU)."""
    rng = random.Random(0xA1E0377)
    f = lambda: rng.randrange(1, Q)
    f2 = lambda: (f(), f())
    zs = lambda i: [(1, 0), (f(), 0), f2()][i % 3]              # Z = 1, in the base field, general
    rep = lambda i: REPS[i % len(REPS)]

    def two_torsion():
        """T = (t, 0) on y^2 = x^3 - t^3 and a second point of that curve: with t = (s^3 - 1) m^2, (s t, (s^3 - 1)^2 m^3) lies on it."""
        s, m = f2(), f2(); s31 = p.fq2_sub(cube(s), (1, 0)); t = p.fq2_mul(s31, p.fq2_mul(m, m))
        T, Tp = (t, (0, 0)), (p.fq2_mul(s, t), p.fq2_mul(p.fq2_mul(s31, s31), cube(m)))
        assert same_curve(T, Tp)
        return T, Tp

    def zero_components():
        """x1, x2 in the base field and w = (0, w_b): both points have x.b = 0 and y.a = 0."""
        A, B = pair_on_a_curve((f(), 0), (f(), 0), (0, f()))
        assert A[0][1] == 0 and A[1][0] == 0 and B[1][0] == 0
        return A, B

    def ordinary(i): return pair_on_a_curve(f2(), f2(), f2())

    def case(kind, A, za, ra, B, zb, rb):
        assert same_curve(A, B), kind
        return dict(kind=kind, A=A, B=B, a=point_row(A, za, ra), b=point_row(B, zb, rb), want=add(A, B))

    # ---- additions
    special = []
    for i in range(10):
        A, B = ordinary(i); T, Tp = two_torsion(); W, Wp = pair_on_a_curve((0, 0), f2(), f2()); Za, Zb = zero_components()
        R1, R2 = pair_on_a_curve((f(), 0), (f(), 0), f2())     # x in the base field, y general: with Z in the base field too, ZZ3 = (z, 0)
        special += [
            case('same', A, zs(i), rep(i), A, zs(i + 1), rep(i + 2)),                      # other representatives, other Z -> doubling
            case('opposite', B, zs(i), rep(i + 1), neg(B), zs(i + 2), rep(i)),
            case('two_torsion', T, zs(i), rep(i), T, zs(i + 1), rep(i + 1)),               # (x, 0) added to itself -> the identity
            case('x_zero', W, zs(i), rep(i), [W, neg(W), Wp][i % 3], zs(i + 1), rep(i + 3)),
            case('identity_left', None, (1, 0), REPS[0], A, zs(i), rep(i)),
            case('identity_right', [B, T, W][i % 3], zs(i), rep(i), None, (1, 0), REPS[0]),
            case('identity_both', None, (1, 0), REPS[0], None, (1, 0), REPS[0]),
            case('zero_component', Za, zs(i), rep(i), [Zb, Za, neg(Za)][i % 3], zs(i + 1), rep(i + 1)),
            case('zz3_one_component_zero', R1, [(1, 0), (f(), 0)][i & 1], rep(i), R2, [(f(), 0), (1, 0)][(i >> 1) & 1], rep(i + 1)),
            case('two_torsion_operand', [T, Tp][i & 1], zs(i), rep(i), [Tp, T][i & 1], zs(i + 2), rep(i + 4)),
        ]
    last = special.pop()
    adds, k = [], 0
    while special or len(adds) % 64 != 40:
        if len(adds) % WAVE in (0, WAVE - 1) and special: adds.append(special.pop())
        else: A, B = ordinary(k); adds.append(case('ordinary', A, zs(k), rep(k), B, zs(k // 3), rep(k // 5))); k += 1
    adds.append(last)                                           # the last pair of a partial block is a special one too

    # ---- doublings
    special = []
    for i in range(10):
        T, _ = two_torsion(); W, _ = pair_on_a_curve((0, 0), f2(), f2()); Za, _ = zero_components()
        special += [dict(kind='two_torsion', A=T, a=point_row(T, zs(i), rep(i)), want=None),
                    dict(kind='identity', A=None, a=point_row(None, (1, 0), REPS[0]), want=None),
                    dict(kind='x_zero', A=W, a=point_row(W, zs(i), rep(i + 1)), want=add(W, W)),
                    dict(kind='zero_component', A=Za, a=point_row(Za, zs(i + 1), rep(i + 2)), want=add(Za, Za))]
    last = special.pop()
    dbls, k = [], 0
    while special or len(dbls) % 64 != 40:
        if len(dbls) % WAVE in (0, WAVE - 1) and special: dbls.append(special.pop())
        else: A, _ = ordinary(k); dbls.append(dict(kind='ordinary', A=A, a=point_row(A, zs(k), rep(k)), want=add(A, A))); k += 1
    dbls.append(last)

    # ---- mixed additions: acc (a stored point, or a slice's first point (x, +-y, 1, 1)) + an entry, negated on the device where the flag says so
    def mcase(kind, A, za, ra, E, negated, lifts=(0, 0, 0, 0)):
        P = neg(E) if negated else E
        assert same_curve(A, P), kind
        refused = A[0] == P[0]
        return dict(kind=kind, A=A, P=P, acc=point_row(A, za, ra), ent=entry_row(E, (0, 0, 0, 0) if negated else lifts), neg=int(negated), refused=refused,
                    want=None if refused else add(A, P))

    refused, accepted = [], []
    for i in range(10):
        A, B = ordinary(i); T, Tp = two_torsion(); W, Wp = pair_on_a_curve((0, 0), f2(), f2()); Za, Zb = zero_components()
        R1, R2 = pair_on_a_curve((f(), 0), (f(), 0), f2())
        lifts = [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0)][i % 4]
        refused += [mcase('refused_same', A, zs(i), rep(i), A if i & 1 else neg(A), not (i & 1), lifts),       # P == acc, as it is and through the device's negation
                    mcase('refused_opposite', B, zs(i), rep(i + 1), neg(B) if i & 1 else B, not (i & 1), lifts),
                    mcase('refused_first_point', A, (1, 0), REPS[0], A, False),                                 # the same base twice at the head of a slice
                    mcase('refused_two_torsion', T, zs(i), rep(i), T, bool(i & 1)),                             # y = 0; negated it is exactly 2q
                    mcase('refused_base_field', R1, (f(), 0), rep(i), R1 if i & 1 else neg(R1), bool(i & 2), lifts)]
        accepted += [mcase('zz3_one_component_zero', R1, [(1, 0), (f(), 0)][i & 1], rep(i), R2, bool(i & 2), lifts),
                     mcase('negated_zero_entry', Tp, zs(i), rep(i), T, True),                                   # the entry 2q - 0 = 2q, accepted and summed
                     mcase('zero_entry', Tp, zs(i), rep(i + 1), T, False, lifts),
                     mcase('acc_y_zero', T, zs(i), rep(i), Tp, bool(i & 1), lifts),
                     mcase('x_zero', [W, Wp][i & 1], zs(i), rep(i), [Wp, W][i & 1], bool(i & 2), lifts),
                     mcase('zero_component', Za, zs(i), rep(i), Zb, bool(i & 1), lifts)]
    last = refused.pop()
    madds, k = [], 0
    while refused or accepted or len(madds) % 64 != 40:
        s = len(madds) % WAVE
        if s in (0, WAVE - 1) and refused: madds.append(refused.pop())
        elif s in (1, WAVE - 2) and accepted: madds.append(accepted.pop())
        else:
            A, B = ordinary(k); first = k % 4 == 1
            madds.append(mcase('ordinary', A, (1, 0) if first else zs(k), REPS[0] if first else rep(k), B, bool(k & 1), [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1)][k % 3])); k += 1
    madds.append(last)
    assert len(adds) <= 4096 and len(dbls) <= 1024 and len(madds) <= 1024
    u32 = lambda rows: np.array(rows, dtype=np.uint32)
    return dict(adds=adds, dbls=dbls, madds=madds, A=u32([c['a'] for c in adds]), B=u32([c['b'] for c in adds]), D=u32([c['a'] for c in dbls]),
                ACC=u32([c['acc'] for c in madds]), ENT=u32([c['ent'] for c in madds]), NEG=np.array([c['neg'] for c in madds], dtype=np.uint8))


@pytest.fixture(scope='module')
def inputs():
    return build_cases()


@pytest.fixture(scope='module')
def run(inputs):
    """ONE run of the three kernels, shared by every GPU test below."""
    c = inputs
    L = aleo_amd.lib()
    aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out_add, out_dbl, out_acc, ok = np.zeros_like(c['A']), np.zeros_like(c['D']), np.zeros_like(c['ACC']), np.zeros(2 * len(c['ACC']), dtype=np.uint8)
    aleo_amd._lib.check(L.aleo_mi355x_selftest_g2p_rows(vp(c['A']), vp(c['B']), len(c['A']), vp(out_add), vp(c['D']), len(c['D']), vp(out_dbl),
                                                        vp(c['ACC']), vp(c['ENT']), vp(c['NEG']), len(c['ACC']), vp(out_acc), vp(ok)), 'selftest_g2p_rows')
    return dict(out_add=out_add, out_dbl=out_dbl, out_acc=out_acc, ok=ok)


def residues(row): return [tuple(value(fields(row)[2 * i + c]) * R28_INV % Q for c in (0, 1)) for i in range(4)]


def test_inputs_cover_the_edges(inputs):
    """The row set itself (no GPU): every kind is present at least 8 times, the rare ones in the first or the last lane pair of a wave, the last block partial."""
    adds, dbls, madds = inputs['adds'], inputs['dbls'], inputs['madds']
    for rows, kinds in ((adds, ('same', 'opposite', 'two_torsion', 'x_zero', 'identity_left', 'identity_right', 'identity_both', 'zero_component', 'zz3_one_component_zero', 'two_torsion_operand')),
                        (dbls, ('two_torsion', 'identity', 'x_zero', 'zero_component')),
                        (madds, ('refused_same', 'refused_opposite', 'refused_first_point', 'refused_two_torsion', 'refused_base_field', 'zz3_one_component_zero', 'negated_zero_entry', 'zero_entry',
                                 'acc_y_zero', 'x_zero', 'zero_component'))):
        count = {k: sum(c['kind'] == k for c in rows) for k in kinds}
        assert all(v >= 8 for v in count.values()), count
        assert len(rows) % 64 not in (0, 1) and rows[-1]['kind'] != 'ordinary', 'the last block is partial and ends with a special case'
        edge = ('refused',) if rows is madds else kinds
        assert all(s % WAVE in (0, WAVE - 1) or s == len(rows) - 1 for s, c in enumerate(rows) if c['kind'].startswith(edge)), 'a special case away from the edge of its wave'
        assert sum(c['kind'] == 'ordinary' for c in rows) > len(rows) // 2
    # what the kinds claim, recomputed from the rows
    for c in adds:
        if c['kind'] == 'same': assert c['A'] == c['B'] and c['a'] != c['b'] and c['want'] is not None
        if c['kind'] == 'opposite': assert c['A'][0] == c['B'][0] and c['A'][1] != c['B'][1] and c['want'] is None
        if c['kind'] == 'two_torsion': assert c['A'] == c['B'] and c['A'][1] == (0, 0) and c['want'] is None
        if c['kind'] == 'x_zero': assert c['A'][0] == (0, 0)
        if c['kind'] == 'zero_component': assert c['A'][0][1] == 0 and c['A'][1][0] == 0
        if c['kind'] == 'zz3_one_component_zero':
            (X1, _, ZZ1, _), (X2, _, ZZ2, _) = residues(c['a']), residues(c['b'])
            P = p.fq2_sub(p.fq2_mul(X2, ZZ1), p.fq2_mul(X1, ZZ2)); ZZ3 = p.fq2_mul(p.fq2_mul(ZZ1, ZZ2), p.fq2_mul(P, P))
            assert ZZ3[1] == 0 and ZZ3[0] != 0 and c['want'] is not None
    assert sum(c['want'] is None for c in adds) >= 30
    for c in madds:
        assert c['refused'] == c['kind'].startswith('refused')
        if c['kind'] == 'zz3_one_component_zero':
            X1, _, ZZ1, _ = residues(c['acc']); P = p.fq2_sub(p.fq2_mul(c['P'][0], ZZ1), X1); ZZ3 = p.fq2_mul(ZZ1, p.fq2_mul(P, P))
            assert ZZ3[1] == 0 and ZZ3[0] != 0
        if c['kind'] == 'negated_zero_entry': assert c['neg'] == 1 and not any(c['ent'][14:28]) and not any(c['ent'][42:56]) and not c['refused']
    assert sum(c['neg'] == 1 and c['kind'] == 'refused_two_torsion' for c in madds) >= 3
    # the representatives: every component reaches its largest lift, and the a- and b-components of one coordinate are lifted differently somewhere
    A = inputs['A'].astype(np.uint64)
    top = [max(value(r[14 * f:14 * f + 14]) for r in A) for f in range(8)]
    assert all(t > (b - 1) * Q for t, b in zip(top, BOUNDS)), top
    assert any(value(r[0:14]) > 11 * Q and value(r[14:28]) < Q for r in A) and any(value(r[0:14]) < Q and value(r[14:28]) > 11 * Q for r in A)


@pytest.mark.gpu
def test_sums_keep_the_stored_invariant_and_equal_the_group_law(inputs, run):
    for i, (c, row) in enumerate(zip(inputs['adds'], run['out_add'])):
        check_point_row(row, c['want'], ('add', i, c['kind']))


@pytest.mark.gpu
def test_doublings_keep_the_stored_invariant_and_equal_the_group_law(inputs, run):
    for i, (c, row) in enumerate(zip(inputs['dbls'], run['out_dbl'])):
        check_point_row(row, c['want'], ('double', i, c['kind']))


@pytest.mark.gpu
def test_mixed_addition_refuses_exactly_p_equal_plus_minus_acc_and_sums_the_rest(inputs, run):
    ok = run['ok'].reshape(-1, 2)
    for i, (c, out, flags) in enumerate(zip(inputs['madds'], run['out_acc'], ok)):
        where = ('madd', i, c['kind'])
        assert flags[0] in (0, 1) and flags[1] in (0, 1), (where, 'a flag was not written')
        assert flags[0] == flags[1], (where, 'the lanes of the pair disagree')
        assert bool(flags[0]) == (not c['refused']), (where, 'accepted P == +-acc' if flags[0] else 'refused a point whose x differs')
        if c['refused']: assert [int(v) for v in out] == c['acc'], (where, 'acc changed by a refused addition')
        else: check_point_row(out, c['want'], where)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    L = aleo_amd.lib()
    n = None
    assert L.aleo_mi355x_selftest_g2p_rows(n, n, 1, n, n, 0, n, n, n, n, 0, n, n) == 2
    assert L.aleo_mi355x_selftest_g2p_rows(n, n, 0, n, n, 1, n, n, n, n, 0, n, n) == 2
    assert L.aleo_mi355x_selftest_g2p_rows(n, n, 0, n, n, 0, n, n, n, n, (1 << 20) + 1, n, n) == 2
