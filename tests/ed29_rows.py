"""What the two row tests of the 29-bit-limb Edwards arithmetic share (tests/test_ed29_bounds.py on the host, tests/test_gpu_ed29_extremes.py on the GPU): the rows,
built limb by limb in Python integers at the edges of the operand classes of aleo_amd/csrc/fr29.h and edwards29.h, and the exact checks of what comes back.
A plain module: no GPU, no library; what runs the rows (a host program over tests/cpp/checked_f29.h, or aleo_mi355x_selftest_ed29_rows) is the tests' business.

An element is 9 limbs of 29 bits (the top limb takes what is left), Montgomery form with R = 2^261; a point is X | Y | Z | T on -x^2 + y^2 = 1 + 3021 x^2 y^2.
"""
import numpy as np
from aleo_amd import synth

R = synth.FR_MODULUS
M29 = (1 << 29) - 1
LAZY_MAX = 2833000000                      # fr29.h: a multiplicand's limbs are below 2^31.4
MONT = (1 << 261) % R
MONT_INV = pow(MONT, -1, R)
R_INV_261 = pow(R, -1, 1 << 261)
D = 3021
ORDER_L = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff       # the prime order of the subgroup; the curve has 4 l points
FR29_PAD = [0x40000013, 0x5a63fffe, 0x400004ed, 0x4da9d2de, 0x41019a78, 0x5ca06c0f, 0x55a4b584, 0x40ae2a06, 0x162b884]      # fr29.h: 19 r, limbs raised
ED29_V = 3                                 # edwards29.h: a coordinate is exact digits below 3 r
ROWS = 256                                 # four waves of each kernel
# The largest multiplicand: the host checker keeps value bounds as multiples of r / 2^32, and the last of those that is not above 2^261 lies 2^-39 of it below
MUL_TOP = (((1 << 293) // R) * R >> 32) - 1

# What tests/cpp/ed29_bounds_emul.cpp establishes for the coordinates ed29_add / ed29_dbl return when their operands keep the contract (its slack lines, quoted;
# tests/test_ed29_bounds.py fails when the program prints other figures):
#   slack ed29_add: ... largest returned X 1.1370 r, Y 1.1000 r, Z 1.1369 r, T 1.1001 r
#   slack ed29_dbl: ... largest returned X 1.1373 r, Y 1.0140 r, Z 1.0205 r, T 1.0934 r
RETURNED = {'ed29_add': (1.1370, 1.1000, 1.1369, 1.1001), 'ed29_dbl': (1.1373, 1.0140, 1.0205, 1.0934)}
PRINTED_TO = 1e-4                          # the figures are printed to four places: a bound is the figure plus one unit of the last place


# ---- elements -----------------------------------------------------------------------------------------------------------------------------------------------
def digits(v):
    assert 0 <= v and v >> 232 < 1 << 32
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def value(limbs): return sum(int(l) << (29 * i) for i, l in enumerate(limbs))


def relimb_up(d, units=4, cap=None):
    """Same value, limbs 0..7 raised: every limb lends `units` units of 2^29 to the one below — one more where that still stays below `cap`."""
    d = list(d)
    for i in range(7, -1, -1):
        k = min(units, d[i + 1])
        if cap is not None and d[i + 1] > units and d[i] + ((units + 1) << 29) < cap: k = units + 1
        d[i + 1] -= k; d[i] += k << 29
    return d


def mont_mul(a, b):
    """What the device's product leaves, limb for limb: (a b + m r) / 2^261 with m = -a b / r mod 2^261, limbs 0..7 digits, the rest in the top limb."""
    ab = value(a) * value(b)
    m = -ab * R_INV_261 % (1 << 261)
    t = ab + m * R
    assert t % (1 << 261) == 0
    return digits(t >> 261)


def tidy(a):
    """f29_tidy: the carries pushed, then q r taken away with q = mulhi(top limb, 0xdb6)."""
    v = value(a)
    q = ((v >> 232) * 0xdb6) >> 32
    return digits(v - q * R)


def canonical(a): return digits(value(a) * MONT_INV % R)


def mul_rows():
    """(A, B): multiplicands at the edge of their class (limbs 0..7 raised to 5 * 2^29 - 1 and, where the value allows, to just below LAZY_MAX; values just below
    2^261) against multipliers with every digit 2^29 - 1 and top limbs at the r, 2 r and 3 r edges; 0, 1, r - 1, r, 2^256 - 1 and FR29_PAD itself among them."""
    rnd = np.random.default_rng(0xED29)
    big = lambda: int.from_bytes(rnd.bytes(40), 'little')
    top = MUL_TOP
    special_a = [digits(v) for v in (0, 1, R - 1, R, (1 << 256) - 1)] + [list(FR29_PAD), relimb_up(digits(top)), relimb_up(digits(top), cap=LAZY_MAX - 1),
                                                                         relimb_up(digits(top - (M29 << 29 * 3)), cap=LAZY_MAX - 1)]
    special_b = [digits(v) for v in (0, 1, R - 1, R, (1 << 256) - 1)]
    for k in (1, 2, 3):                                             # every digit 2^29 - 1, the top limb the largest that keeps the value below k r
        t = (k * R - (1 << 232)) >> 232
        assert value([M29] * 8 + [t]) < k * R <= value([M29] * 8 + [t + 1])
        special_b.append([M29] * 8 + [t])
    A, B = [], []
    for i in range(ROWS):
        lane = i % 64
        if lane in (0, 63):                                         # specials against specials, at a wave's edges
            a, b = special_a[(i // 32) % len(special_a)], special_b[(i // 32 + lane) % len(special_b)]
        else:
            v = top - big() % (1 << (8 * (i % 30) + 1)) if i % 3 else big() % (1 << 261)      # next to 2^261, at every distance; or anywhere below it
            a = digits(v) if i % 4 == 3 else relimb_up(digits(v), cap=LAZY_MAX - 1 if i % 2 else None)
            if i % 7 == 0: a = special_a[(i // 7) % len(special_a)]
            b = special_b[i % len(special_b)] if i % 5 < 2 else digits(big() % (3 * R))
        assert all(l < LAZY_MAX for l in a) and value(a) <= MUL_TOP and all(l <= M29 for l in b[:8]) and value(b) < 1 << 256
        A.append(a); B.append(b)
    assert max(max(a[:8]) for a in A) >= 5 * (1 << 29) - 1 and max(max(a[:8]) for a in A) < LAZY_MAX
    return A, B


def tidy_rows():
    """Lazy limbs (every limb up to seven units of 2^29), values up to the last one below 445 r."""
    rnd = np.random.default_rng(0x71D1)
    rows = []
    for i in range(ROWS):
        x = [0, R - 1, 1][i % 64 % 3] if i % 64 in (0, 63) else int.from_bytes(rnd.bytes(40), 'little') % R
        k = [444, 0, 17, 444, 2, 438][i % 6]
        d = digits(x + k * R)
        rows.append(relimb_up(d, units=6) if i % 2 else d)
        assert value(rows[-1]) < 445 * R
    return rows


def canonical_rows():
    """Multiplicands: limbs up to 5 * 2^29 - 1, values up to the last one below 438 r (2^261 = 438.79 r); 0, r and 437 r themselves, which leave exactly r."""
    rnd = np.random.default_rng(0xCA11)
    rows = []
    for i in range(ROWS):
        x = [0, 0, R - 1, 1][(i // 32) % 4] if i % 64 in (0, 63) else int.from_bytes(rnd.bytes(40), 'little') % R
        k = [437, 1, 0, 437, 2, 33][i % 6]
        d = digits(x + k * R)
        rows.append(relimb_up(d) if i % 2 else d)
        assert value(rows[-1]) < 1 << 261 and max(rows[-1]) < LAZY_MAX
    return rows


# ---- the curve, affine, in integers ---------------------------------------------------------------------------------------------------------------------------
def sqrt_mod(a):
    """A square root of a modulo r (Tonelli-Shanks), or None."""
    a %= R
    if a == 0: return 0
    if pow(a, (R - 1) // 2, R) != 1: return None
    s, t = 0, R - 1
    while t % 2 == 0: s, t = s + 1, t // 2
    z = 2
    while pow(z, (R - 1) // 2, R) == 1: z += 1
    c, x, b, m = pow(z, t, R), pow(a, (t + 1) // 2, R), pow(a, t, R), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1: b2, i = b2 * b2 % R, i + 1
        e = pow(c, 1 << (m - i - 1), R)
        x, c = x * e % R, e * e % R
        b, m = b * c % R, i
    return x


def on_curve(p): return (p[1] * p[1] - p[0] * p[0]) % R == (1 + D * p[0] * p[0] * p[1] * p[1]) % R


def add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % R
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, R) % R, (y1 * y2 + x1 * x2) * pow(1 - t, -1, R) % R


def neg(p): return (-p[0] % R, p[1])


def times(p, n):
    acc = (0, 1)
    while n:
        if n & 1: acc = add(acc, p)
        p, n = add(p, p), n >> 1
    return acc


def curve_points():
    """name -> affine point: the identity, (0, -1), both points of order 4, points of order l, 2 l and 4 l, and ordinary ones."""
    found = []
    x = 2
    while len(found) < 4:
        y = sqrt_mod((1 + x * x) * pow(1 - D * x * x, -1, R))
        if y is not None: found.append((x, y))
        x += 1
    im = sqrt_mod(R - 1)
    pts = {'identity': (0, 1), 'order2': (0, R - 1), 'order4': (im, 0), 'order4_neg': (R - im, 0)}
    pts['order_l'] = times(found[0], 4)
    pts['order_2l'] = add(pts['order_l'], pts['order2'])
    pts['order_4l'] = add(pts['order_l'], pts['order4'])
    for i, p in enumerate(found[1:]): pts['ordinary%d' % i] = p
    assert all(on_curve(p) for p in pts.values())
    assert times(pts['order_l'], ORDER_L) == (0, 1) and pts['order_l'] != (0, 1)
    assert times(pts['order_2l'], ORDER_L) == pts['order2'] and times(pts['order_4l'], ORDER_L) in (pts['order4'], pts['order4_neg'])
    assert times(pts['order4'], 2) == pts['order2']
    return pts


REPS = [(0, 0, 0, 0), (2, 2, 2, 2), (2, 0, 1, 2)]      # the multiple of r added to X, Y, Z, T: canonical; the largest below 3 r; a mix
ZS = [1, 0x1234567 * MONT % R, pow(3, 300, R)]


def point_row(p, z, rep):
    x, y = p
    return sum((digits(c % R * MONT % R + k * R) for c, k in zip((x * z, y * z, z, x * y * z), rep)), [])


def add_rows():
    """(P rows, Q rows, neg flags, what each row is, the affine result wanted)."""
    pts = curve_points()
    names = list(pts)
    special = [(a, b) for a in names for b in names if a != b and ('ordinary' not in a or 'ordinary' not in b)]      # at least one of the two a special point
    same = [(a, a) for a in names]                                  # P + P and P + (-P) through the addition: the law is complete
    edge = same + special
    rows = []
    e = o = 0
    for i in range(ROWS):
        lane = i % 64
        if lane == 63 or lane % 2 == 0:                             # a special pair: at a wave's edges, and between ordinary neighbours inside it
            a, b = edge[e % len(edge)]; e += 1
            opposite = a == b and (e // len(edge) + i) % 2 == 1
            rows.append((a, b, opposite, (i // 2) % 2 == 1))
        else:
            a, b = 'ordinary%d' % (o % 3), ['order_l', 'order_2l', 'order_4l', 'ordinary%d' % ((o + 1) % 3)][(o // 3) % 4]; o += 1
            rows.append((a, b, False, o % 2 == 1))
    assert e >= len(edge)
    P, Q, NEG, what, want = [], [], [], [], []
    for i, (a, b, opposite, ng) in enumerate(rows):
        pa, pb = pts[a], neg(pts[b]) if opposite else pts[b]
        P.append(point_row(pa, ZS[i % 3], REPS[(i // 3) % 3])); Q.append(point_row(pb, ZS[(i // 2) % 3], REPS[(i // 5) % 3])); NEG.append(1 if ng else 0)
        what.append((a, ('-' if opposite else '') + b, ng)); want.append(add(pa, neg(pb) if ng else pb))
    return P, Q, NEG, what, want


def dbl_rows():
    """(rows, want-T flags, the names, the affine result wanted)."""
    pts = curve_points()
    names = list(pts)
    rows, T, what, want = [], [], [], []
    for i in range(ROWS):
        lane = i % 64
        name = names[(i // 32 + lane) % 7] if lane == 63 or lane % 2 == 0 else names[i % len(names)]
        rows.append(point_row(pts[name], ZS[i % 3], REPS[(i // 3) % 3])); T.append((i // 3 + i) % 2); what.append(name); want.append(add(pts[name], pts[name]))
    return rows, T, what, want


D2_ROW = digits(2 * D * MONT % R)


def build():
    """Every row set, as uint32 arrays, with what the checks below need."""
    A, B = mul_rows()
    P, Q, NEG, add_what, add_want = add_rows()
    DB, WT, dbl_what, dbl_want = dbl_rows()
    u = lambda rows: np.array(rows, dtype=np.uint32)
    return dict(mul_a=u(A), mul_b=u(B), tidy=u(tidy_rows()), canon=u(canonical_rows()), p=u(P), q=u(Q), neg=np.array(NEG, dtype=np.uint8), d2=u(D2_ROW),
                dbl=u(DB), want_t=np.array(WT, dtype=np.uint8), add_what=add_what, add_want=add_want, dbl_what=dbl_what, dbl_want=dbl_want)


OUTPUTS = (('out_mul', 'mul_a'), ('out_tidy', 'tidy'), ('out_canon', 'canon'), ('out_add', 'p'), ('out_dbl', 'dbl'))


def write_case_file(path, c):
    """u32 counts of the five kinds, then mul_a, mul_b, tidy, canon, p, q, neg, d2, dbl, want_t as they lie."""
    with open(path, 'wb') as f:
        f.write(np.array([len(c['mul_a']), len(c['tidy']), len(c['canon']), len(c['p']), len(c['dbl'])], dtype=np.uint32).tobytes())
        for k in ('mul_a', 'mul_b', 'tidy', 'canon', 'p', 'q', 'neg', 'd2', 'dbl', 'want_t'): f.write(c[k].tobytes())


def read_result_file(path, c):
    """The five outputs in the order of OUTPUTS, shaped like their inputs."""
    raw = np.fromfile(path, dtype=np.uint32)
    out, at = {}, 0
    for name, like in OUTPUTS:
        out[name] = raw[at:at + c[like].size].reshape(c[like].shape); at += c[like].size
    assert at == raw.size
    return out


# ---- the checks: every output exactly ----------------------------------------------------------------------------------------------------------------------------
def ints(row): return [int(v) for v in row]


def check_fields(c, out):
    for i, (a, b, got) in enumerate(zip(c['mul_a'], c['mul_b'], out['out_mul'])):
        assert ints(got) == mont_mul(ints(a), ints(b)), ('mul', i, ints(a), ints(b), ints(got))
    for i, (a, got) in enumerate(zip(c['tidy'], out['out_tidy'])):
        assert ints(got) == tidy(ints(a)), ('tidy', i, ints(a), ints(got))
        assert all(l <= M29 for l in ints(got)[:8]) and value(got) < 3 * R and value(got) % R == value(a) % R, ('tidy', i)
    for i, (a, got) in enumerate(zip(c['canon'], out['out_canon'])):
        assert ints(got) == canonical(ints(a)), ('canonical', i, ints(a), ints(got))


def check_point(row, want, bounds, where):
    f = [ints(row[9 * k:9 * k + 9]) for k in range(4)]
    for name, limbs, bound in zip('XYZT', f, bounds):
        assert all(l <= M29 for l in limbs[:8]), (where, name, 'not exact digits')
        if bound is not None: assert value(limbs) < (bound + PRINTED_TO) * R, (where, name, 'above the bound the host checker reports', value(limbs) / R)
    X, Y, Z, T = (value(l) * MONT_INV % R for l in f)
    assert Z != 0, (where, 'Z is 0 mod r')
    assert T * Z % R == X * Y % R, (where, 'T Z != X Y')
    zi = pow(Z, -1, R)
    assert (X * zi % R, Y * zi % R) == want, (where, 'not the affine sum')


def check_points(c, out):
    for i, (row, want) in enumerate(zip(out['out_add'], c['add_want'])):
        check_point(row, want, RETURNED['ed29_add'], ('add', i, c['add_what'][i]))
    for i, (row, want, t, src) in enumerate(zip(out['out_dbl'], c['dbl_want'], c['want_t'], c['dbl'])):
        if not t:                                                   # the T that came in, untouched; the point is checked with the T it should have had
            assert ints(row[27:36]) == ints(src[27:36]), ('dbl', i, 'T touched though it was not wanted')
            X, Y, Z = (value(ints(row[9 * k:9 * k + 9])) * MONT_INV % R for k in range(3))
            row = list(ints(row[:27])) + digits(X * Y * pow(Z, -1, R) % R * MONT % R)
        check_point(row, want, RETURNED['ed29_dbl'][:3] + ((RETURNED['ed29_dbl'][3],) if t else (None,)), ('dbl', i, c['dbl_what'][i]))


def check_coverage(c):
    """The row sets themselves hold what they are for."""
    what = c['add_what']
    firsts, seconds = {a for a, _, _ in what}, {b.lstrip('-') for _, b, _ in what}
    for name in ('identity', 'order2', 'order4', 'order4_neg', 'order_l', 'order_2l', 'order_4l'):
        assert name in firsts and name in seconds and name in c['dbl_what'], name
    assert any(a == b for a, b, _ in what) and any(b == '-' + a for a, b, _ in what)              # P + P and P + (-P)
    assert {ng for _, _, ng in what} == {False, True} and set(ints(c['want_t'])) == {0, 1}
    for i in range(ROWS):
        if i % 64 in (0, 63): assert 'ordinary' not in what[i][0] or 'ordinary' not in what[i][1], i
    for rows in (c['p'], c['q'], c['dbl']):
        vals = [value(ints(r[9 * k:9 * k + 9])) for r in rows for k in range(4)]
        assert max(vals) >= 2 * R and max(vals) < ED29_V * R and min(vals) < R
    assert len(c['mul_a']) == len(c['tidy']) == len(c['canon']) == len(c['p']) == len(c['dbl']) == ROWS
