"""The 32-bit-limb Fr vector kernels every proof runs between transforms (frops.hip, fr_spmv.hip, fr_divide.hip, ahp_kernels.hip) at the edges of the field.

The older tests of these kernels (test_gpu_parity.py) feed them uniform operands, on which a lazily reduced sum never equals r or 2r — the values at which the
conditional subtraction that ends every kernel must take its `equal` branch — and a carry never runs through all eight limbs.  Here the operands come from
tests/fr_edges.py: the edge set E in all ordered pairs (triples), rows whose true result is exactly 0 (one operand solved) with the two neighbours 1 and r - 1,
and long-carry rows.  Everything is in the stored (Montgomery) domain; expected values are Python integers (x (*) y = x y 2^-256 mod r), compared bit for bit.
The seven kernels that only the native prover launches are driven through aleo_mi355x_selftest_fr_step."""
import ctypes, random
import numpy as np
import pytest

import aleo_amd
from aleo_amd import msm as M, poly
from oracle import coracle as c
import fr_edges as E
import util

pytestmark = pytest.mark.gpu
R = E.R
mmul, msolve = E.mmul, E.msolve
BAD_ARG = 2


@pytest.fixture(scope='module', autouse=True)
def device():
    L = aleo_amd.lib()
    aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')     # no GPU -> hard failure, never a fallback


# ---- device buffers: a tensor is complete before the library (which works on streams of its own) sees it, and the entry points return with their work done ----
def dev_raw(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64).copy()).cuda(); torch.cuda.synchronize(); return t
def dev(vals): return dev_raw(E.limbs(vals))
def dev_u32(idx):
    import torch
    t = torch.from_numpy(np.asarray(idx, dtype=np.uint32).view(np.int32).copy()).cuda(); torch.cuda.synchronize(); return t
def zeros(n, fill=0):
    import torch
    t = torch.full((max(n, 1), 4), fill, dtype=torch.int64, device='cuda'); torch.cuda.synchronize(); return t
def back_raw(t, n=None):
    import torch
    torch.cuda.synchronize(); a = t.cpu().numpy().view(np.uint64).reshape(-1, 4); return a if n is None else a[:n]
def back(t, n=None): return E.ints(back_raw(t, n))
def k(v): return E.limbs([v])[0]                            # a host constant
def at(t, elem): return t.data_ptr() + 32 * elem


def fr_step(step, ptrs, sizes, consts=None):
    """aleo_mi355x_selftest_fr_step: its status."""
    P = (ctypes.c_void_p * max(len(ptrs), 1))(*[int(x) if x else None for x in ptrs]); S = (ctypes.c_size_t * max(len(sizes), 1))(*[int(s) for s in sizes])
    kk = None if consts is None else np.ascontiguousarray(E.limbs(consts))
    return aleo_amd.lib().aleo_mi355x_selftest_fr_step(step, P, S, None if kk is None else kk.ctypes.data_as(ctypes.c_void_p))
ADD_TILED, SUB_MUL, SCALE_ROWS, PICK, GATHER_MUL3, SCATTER, SPLIT = range(7)


def first_bad(got, want):
    """None, or the first row that differs (index, got, want in hex): what an assertion shows."""
    if got == want: return None
    if len(got) != len(want): return ('length', len(got), len(want))
    i = next(j for j in range(len(want)) if got[j] != want[j])
    return (i, hex(got[i]), hex(want[i]), sum(g != w for g, w in zip(got, want)))


# ---- fr_vec_op ----------------------------------------------------------------------------------------------------------------------------------------------
def test_fr_vec_op_edges_long_carries_and_cancelling_rows():
    ea, eb = E.edge_pairs()
    u, t = E.uniform(E.CANCEL_ROWS + 8, 101), E.targets()
    a = ea + [x for x, _, _ in E.CARRY_ADD] + [x for x, _, _ in E.CARRY_SUB] + E.E + u + u
    b = eb + [y for _, y, _ in E.CARRY_ADD] + [y for _, y, _ in E.CARRY_SUB] + E.E + [(w - x) % R for x, w in zip(u, t)] + [(x - w) % R for x, w in zip(u, t)]
    n = len(a); assert n == len(b) and n > 4096
    want = {poly.OP_MUL: [mmul(x, y) for x, y in zip(a, b)], poly.OP_ADD: [(x + y) % R for x, y in zip(a, b)], poly.OP_SUB: [(x - y) % R for x, y in zip(a, b)]}
    lo = len(ea) + 14 + 18                                   # the cancelling rows did cancel
    assert want[poly.OP_ADD][lo:lo + len(t)] == t and want[poly.OP_SUB][lo + len(t):] == t
    dA, dB, dst = dev(a), dev(b), zeros(n)
    for op in (poly.OP_MUL, poly.OP_ADD, poly.OP_SUB):
        poly.fr_vec_op_device(dst.data_ptr(), dA.data_ptr(), dB.data_ptr(), n, op)
        assert first_bad(back(dst), want[op]) is None, op
        d2 = dev(a)                                          # in place over a
        poly.fr_vec_op_device(d2.data_ptr(), d2.data_ptr(), dB.data_ptr(), n, op)
        assert first_bad(back(d2), want[op]) is None, ('in place', op)


# ---- fr_lin -------------------------------------------------------------------------------------------------------------------------------------------------
def test_fr_lin_edge_constants_and_operands_all_four_shapes():
    ea, eb = E.edge_pairs(); n = len(ea)
    dA, dB, dst = dev(ea), dev(eb), zeros(n)
    for i, c1 in enumerate(E.E):
        c0, c2 = E.E[(5 * i + 3) % 18], E.E[(7 * i + 1) % 18]
        k0 = None if i % 3 == 2 else k(c0); z0 = 0 if k0 is None else c0      # the constant term absent in a third of the launches
        poly.fr_lin_device(dst.data_ptr(), n, k0, k(c1), dA.data_ptr(), k(c2), dB.data_ptr())
        assert first_bad(back(dst), [(z0 + mmul(c1, x) + mmul(c2, y)) % R for x, y in zip(ea, eb)]) is None, i
        poly.fr_lin_device(dst.data_ptr(), n, k0, k(c1), dA.data_ptr())
        assert first_bad(back(dst), [(z0 + mmul(c1, x)) % R for x in ea]) is None, i
        poly.fr_lin_device(dst.data_ptr(), n, k0, None, 0, k(c2), dB.data_ptr())
        assert first_bad(back(dst), [(z0 + mmul(c2, y)) % R for y in eb]) is None, i
        poly.fr_lin_device(dst.data_ptr(), n, k0)
        assert back(dst) == [z0] * n, i
        d2 = dev(ea)                                         # in place over a
        poly.fr_lin_device(d2.data_ptr(), n, k0, k(c1), d2.data_ptr(), k(c2), dB.data_ptr())
        assert first_bad(back(d2), [(z0 + mmul(c1, x) + mmul(c2, y)) % R for x, y in zip(ea, eb)]) is None, ('in place', i)


def test_fr_lin_cancelling_rows():
    """c0 = -(c1 (*) a): c0 and c1 are constants of a launch, so each of the 2048 rows is a launch of its own (three elements: the solved a, and the two whose
    results are 1 and r - 1); tests/test_fr_edge_inputs.py shows that these rows put the lazy sum on r and on 2r.  Then the same through c2 and b, and the
    two-term forms, where b is solved per element and one launch holds every row."""
    rows = E.lin_one_term_cancelling()
    vec, want = [], []
    for c0, c1, a in rows:
        vec += [a, msolve((1 - c0) % R, c1), msolve((R - 1 - c0) % R, c1)]; want += [0, 1, R - 1]
    assert all((c0 + mmul(c1, vec[3 * i + j])) % R == want[3 * i + j] for i, (c0, c1, _) in enumerate(rows) for j in range(3))
    dV = dev(vec)
    for shape in ('a', 'b'):
        dst = zeros(len(vec), -1)
        for i, (c0, c1, _) in enumerate(rows):
            if shape == 'a': poly.fr_lin_device(at(dst, 3 * i), 3, k(c0), k(c1), at(dV, 3 * i))
            else: poly.fr_lin_device(at(dst, 3 * i), 3, k(c0), None, 0, k(c1), at(dV, 3 * i))
        assert first_bad(back(dst), want) is None, shape
    t = E.targets(); n = len(t)
    a = E.uniform(n, 201); c0, c1, c2 = E.uniform(3, 202, nonzero=True)
    dA, dst = dev(a), zeros(n, -1)
    dB = dev([msolve((w - c0 - mmul(c1, x)) % R, c2) for x, w in zip(a, t)])
    poly.fr_lin_device(dst.data_ptr(), n, k(c0), k(c1), dA.data_ptr(), k(c2), dB.data_ptr())
    assert first_bad(back(dst), t) is None
    dB = dev([msolve((w - mmul(c1, x)) % R, c2) for x, w in zip(a, t)])    # c0 absent: c2 (*) b = -(c1 (*) a)
    poly.fr_lin_device(dst.data_ptr(), n, None, k(c1), dA.data_ptr(), k(c2), dB.data_ptr())
    assert first_bad(back(dst), t) is None


# ---- fr_lincomb ---------------------------------------------------------------------------------------------------------------------------------------------
def _lincomb_want(n, c0, terms):
    want = [0] * n; want[0] = c0 % R
    for vals, l, kf in terms:
        for i in range(min(l, n)): want[i] = (want[i] + mmul(kf, vals[i])) % R
    return want


def test_fr_lincomb_edge_terms_and_cancelling_rows():
    n = 300
    for kt in (1, 2, 27, 28, 29):                            # 29: the wrapper carries dst along as a term of a second call
        T = [E.cycle(E.E, n, start=j, step=j % 17 + 1) for j in range(kt)]
        K = E.cycle(E.E, kt, start=3, step=5); lens = [n if j % 3 else max(1, 257 - j) for j in range(kt)]; lens[0] = n
        D = [dev(v) for v in T]; dst = zeros(n, -1); c0 = E.E[(kt + 1) % 18]
        poly.fr_lincomb_device(dst.data_ptr(), n, k(c0), [(D[j].data_ptr(), lens[j], k(K[j])) for j in range(kt)])
        assert first_bad(back(dst), _lincomb_want(n, c0, list(zip(T, lens, K)))) is None, kt
    # the last term's values solved: the running sum ends on a multiple of r in every row
    t = E.targets(); n = len(t)
    T = [E.uniform(n, 301), E.uniform(n, 302)]; K = E.uniform(3, 303, nonzero=True); c0 = E.uniform(1, 304)[0]
    part = _lincomb_want(n, c0, [(T[0], n, K[0]), (T[1], n, K[1])])
    T.append([msolve((w - s) % R, K[2]) for w, s in zip(t, part)])
    D = [dev(v) for v in T]; dst = zeros(n, -1)
    poly.fr_lincomb_device(dst.data_ptr(), n, k(c0), [(D[j].data_ptr(), n, k(K[j])) for j in range(3)])
    assert first_bad(back(dst), t) is None
    # the constant of element 0 solved: launches of two elements over windows of the same terms
    launches = 256; dst = zeros(2 * launches, -1); want = []
    for l in range(launches):
        w = 1 if l % 16 == 14 else (R - 1 if l % 16 == 15 else 0)
        k0 = (w - sum(mmul(K[j], T[j][2 * l]) for j in range(3))) % R
        poly.fr_lincomb_device(at(dst, 2 * l), 2, k(k0), [(at(D[j], 2 * l), 2, k(K[j])) for j in range(3)])
        want += [w, sum(mmul(K[j], T[j][2 * l + 1]) for j in range(3)) % R]
    assert first_bad(back(dst), want) is None


# ---- fr_gather_mul ------------------------------------------------------------------------------------------------------------------------------------------
def test_fr_gather_mul_tables_of_edges_every_pair_and_equal_indices():
    t1, t2 = E.E, E.cycle(E.E, 18, start=7, step=5)
    d1, d2 = dev(t1), dev(t2)
    cases = [([i // 18 % 18 for i in range(5832)], [i % 18 for i in range(5832)], [E.E[i // 324] for i in range(5832)])]      # every (scale, t1, t2) triple
    for v in (0, 17): cases.append(([v] * 324, [v] * 324, E.cycle(E.E, 324)))                                                   # every index equal: the first, the last entry
    cases.append(([0, 17] * 162, [17, 0] * 162, E.cycle(E.E, 324, step=5)))
    for i1, i2, sc in cases:
        n = len(i1); dS, di1, di2, dst = dev(sc), dev_u32(i1), dev_u32(i2), zeros(n, -1)
        poly.fr_gather_mul_device(dst.data_ptr(), n, dS.data_ptr(), d1.data_ptr(), di1.data_ptr(), d2.data_ptr(), di2.data_ptr())
        assert first_bad(back(dst), [mmul(mmul(t1[i1[i]], t2[i2[i]]), sc[i]) for i in range(n)]) is None
        poly.fr_gather_mul_device(dst.data_ptr(), n, 0, d1.data_ptr(), di1.data_ptr(), d2.data_ptr(), di2.data_ptr())
        assert first_bad(back(dst), [mmul(t1[i1[i]], t2[i2[i]]) for i in range(n)]) is None
        poly.fr_gather_mul_device(dst.data_ptr(), n, dS.data_ptr(), d1.data_ptr(), di1.data_ptr())
        assert first_bad(back(dst), [mmul(t1[i1[i]], sc[i]) for i in range(n)]) is None
        poly.fr_gather_mul_device(dst.data_ptr(), n, 0, d1.data_ptr(), di1.data_ptr())
        assert back(dst) == [t1[i1[i]] for i in range(n)]


# ---- fr_batch_inverse ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4095, 4096, 4097, 262144, 262145])
def test_fr_batch_inverse_lane_ownership_and_zero_patterns(n):
    """Both sides of "one element per lane" (4095 / 4096), of the first lane owning two (4097), and of T growing past 4096 lanes (262144 / 262145).  Lane t owns
    t, t + T, ...; zeros stay zero and do not enter the lane's shared inversion."""
    T = (n + 63) // 64
    if T < 4096: T = min(n, 4096)
    base = c.fr_to_mont(util.uniform_scalars(n, 40000 + n % 1000))
    nz = E.limbs(E.E_NONZERO)
    base[40:40 + len(nz)] = nz; base[n - len(nz):] = nz[::-1]         # ONE and r - ONE (what they stand for, 1 and -1, is its own inverse) and the rest of E: a lane's first, a lane's last element
    zeros_at = {
        'nowhere': [],
        'all': list(range(n)),
        'lanes': list(range(0, n, T)) + [5, 9 + (n - 10) // T * T],   # every element of lane 0; lane 5's first; lane 9's last
    }
    for name, where in zeros_at.items():
        inp = base.copy(); inp[where] = 0
        if name == 'lanes': assert (inp[T::T] == 0).all() and (inp[9 + (n - 10) // T * T] == 0).all() and 9 + (n - 10) // T * T + T >= n
        d = dev_raw(inp)
        poly.batch_inversion_device(d.data_ptr(), n)
        got = back_raw(d)
        assert (got == c.fr_batch_inverse(inp)).all(), (n, name)
        check = range(n) if n <= 4097 else list(range(64)) + list(range(n - 64, n)) + random.Random(n).sample(range(n), 256)
        vals = E.ints(inp)
        for i in check:
            assert E.ints(got[i])[0] == (E.minv(vals[i]) if vals[i] else 0), (n, name, i)


# ---- the two sumcheck numerators ------------------------------------------------------------------------------------------------------------------------------
def _first_want(vr, va, vb, vt, vz, eb, ec):
    return [(mmul(r_, (a + mmul(eb, b) + mmul(ec, mmul(a, b))) % R) - mmul(t, z)) % R for r_, a, b, t, z in zip(vr, va, vb, vt, vz)]


def test_ahp_first_sumcheck_edges_and_cancelling_rows():
    vr, va, vb = E.edge_triples(); n = len(vr)
    vt, vz = E.cycle(E.E, n, start=2, step=7), E.cycle(E.E, n, start=5, step=11)
    D = [dev(v) for v in (vr, va, vb, vt, vz)]; dst = zeros(n, -1)
    for i in range(6):
        eb, ec = E.E[(3 * i + 1) % 18], E.E[(5 * i + 3) % 18]
        poly.ahp_first_sumcheck_device(dst.data_ptr(), n, *[d.data_ptr() for d in D], k(eb), k(ec))
        assert first_bad(back(dst), _first_want(vr, va, vb, vt, vz, eb, ec)) is None, i
    t = E.targets(); n = len(t)
    vr, va, vb = (E.uniform(n, 400 + j) for j in range(3)); vt = E.uniform(n, 404, nonzero=True); eb, ec = E.uniform(2, 405)
    left = _first_want(vr, va, vb, vt, [0] * n, eb, ec)
    vz = [msolve((l - w) % R, x) for l, w, x in zip(left, t, vt)]             # t (*) z = the left product (less the target)
    D = [dev(v) for v in (vr, va, vb, vt, vz)]; dst = zeros(n, -1)
    poly.ahp_first_sumcheck_device(dst.data_ptr(), n, *[d.data_ptr() for d in D], k(eb), k(ec))
    assert first_bad(back(dst), t) is None
    poly.ahp_first_sumcheck_device(D[1].data_ptr(), n, *[d.data_ptr() for d in D], k(eb), k(ec))      # in place over z_a, as the prover runs it
    assert first_bad(back(D[1]), t) is None


def _matrix_want(n, present, IDX, F, consts):
    dl, (ab, na, nb, vv) = consts[:3], consts[3:]
    want = [0] * n
    for m in present:
        e, f = IDX[m], F[m]
        for i in range(n):
            bq = (ab + mmul(nb, e[i]) + mmul(na, e[n + i]) + e[3 * n + i]) % R
            want[i] = (want[i] + mmul(dl[m], (mmul(vv, e[2 * n + i]) - mmul(bq, f[i])) % R)) % R
    return want


def test_ahp_matrix_sumcheck_edges_absent_matrices_and_cancelling_rows():
    n = 648
    IDX = [E.cycle(E.E, 4 * n, start=m, step=2 * m + 1) for m in range(3)]; F = [E.cycle(E.E, n, start=4 + m, step=7 - 2 * m) for m in range(3)]
    DI, DF = [dev(v) for v in IDX], [dev(v) for v in F]; dst = zeros(n, -1)
    for s, sets in enumerate(([[0], [1], [2], [0, 1], [1, 2], [0, 2], [0, 1, 2]], [[0, 1, 2]], [[0, 1, 2], [1]])):
        consts = E.cycle(E.E, 7, start=2 + 5 * s, step=5)
        for present in sets:                                  # a null index pointer: the matrix is absent
            poly.ahp_matrix_sumcheck_device(dst.data_ptr(), n, [DI[m].data_ptr() if m in present else 0 for m in range(3)], n,
                                            [DF[m].data_ptr() if m in present else 0 for m in range(3)], E.limbs(consts))
            assert first_bad(back(dst), _matrix_want(n, present, IDX, F, consts)) is None, (s, present)
    # cancelling: row_col solved so that the bracket is 0 (1, r - 1); val solved so that a matrix's term is; the third matrix's val solved so that the whole sum is
    t = E.targets(); n = len(t)
    consts = E.uniform(7, 500, nonzero=True); dl, (ab, na, nb, vv) = consts[:3], consts[3:]
    IDX = [E.uniform(4 * n, 501 + m) for m in range(3)]; F = [E.uniform(n, 511 + m, nonzero=True) for m in range(3)]
    bracket = lambda e, i: (ab + mmul(nb, e[i]) + mmul(na, e[n + i]) + e[3 * n + i]) % R
    for variant in ('bracket', 'term', 'sum'):
        X = [list(v) for v in IDX]
        for i in range(n):
            if variant == 'bracket':
                for m in range(3): X[m][3 * n + i] = (t[i] - ab - mmul(nb, X[m][i]) - mmul(na, X[m][n + i])) % R
            elif variant == 'term':
                for m in range(3): X[m][2 * n + i] = msolve((t[i] + mmul(bracket(X[m], i), F[m][i])) % R, vv)
        if variant == 'sum':
            two = _matrix_want(n, [0, 1], X, F, consts)
            for i in range(n): X[2][2 * n + i] = msolve((msolve((t[i] - two[i]) % R, dl[2]) + mmul(bracket(X[2], i), F[2][i])) % R, vv)
        want = _matrix_want(n, [0, 1, 2], X, F, consts)
        if variant == 'sum': assert want == t
        if variant == 'bracket': assert all(bracket(X[m], i) == t[i] for m in range(3) for i in range(0, n, 97))
        DI, DF = [dev(v) for v in X], [dev(v) for v in F]; dst = zeros(n, -1)
        poly.ahp_matrix_sumcheck_device(dst.data_ptr(), n, [d.data_ptr() for d in DI], n, [d.data_ptr() for d in DF], E.limbs(consts))
        assert first_bad(back(dst), want) is None, variant


# ---- the layout kernels of the first two rounds -----------------------------------------------------------------------------------------------------------------
def test_fr_blind_rows_and_sumcheck_operands_at_zero_differences():
    n = 300; L = n + 1
    for rho, first in ((E.E, [E.E[7 * q % 18] for q in range(18)]),                      # rho from E against a first coefficient from E
                       (E.cycle(E.E, 24, start=3), E.cycle(E.E, 24, start=3))):          # rho = src[0]: the difference is 0
        rows = len(rho)
        src = [[first[q]] + E.cycle(E.E, n - 1, start=q, step=q % 5 + 1) for q in range(rows)]
        d_src = dev([v for row in src for v in row]); dst = zeros(rows * L, -1)
        poly.fr_blind_rows_device(dst.data_ptr(), d_src.data_ptr(), n, E.limbs(rho))
        want = []
        for q in range(rows): want += [(src[q][0] - rho[q]) % R] + src[q][1:] + [rho[q]]
        assert first_bad(back(dst), want) is None, rows
    inst = 2
    for n_x in (1, n):
        wit = []
        for i in range(inst):
            w = [E.E[(3 + i) % 18]] * 150 + E.cycle(E.E, L - 150, start=i, step=5)     # a constant run: w[j - 1] = w[j]
            w[0] = 0 if i == 0 else w[0]; w[n] = w[0]                                    # n_x = n: w[n - n_x] = w[n]
            w[200] = 0; w[201] = 0
            wit += [w, E.cycle(E.E, L, start=1 + i, step=7), E.cycle(E.E, L, start=2 + i, step=11)]
        xp = []
        for i in range(inst):
            x = [0] + [wit[3 * i][j] if j % 2 else E.E[j % 18] for j in range(1, n_x)]   # x̂ = 0 under w = 0 (the lazy value is exactly r); x̂ = w: -w + x̂ = 0
            if n_x > 200: x[200] = 0
            xp += x
        d_w, d_x = dev([v for row in wit for v in row]), dev(xp); out = zeros(3 * inst * 4 * n, -1)
        poly.ahp_sumcheck_operands_device(out.data_ptr(), d_w.data_ptr(), d_x.data_ptr(), n, n_x, inst)
        want = []
        for i in range(inst):
            w, za, zb = wit[3 * i:3 * i + 3]
            z = [0] * (4 * n)
            for j in range(4 * n):
                v = w[j - n_x] if n_x <= j < L + n_x else 0
                if j < L: v -= w[j]
                if j < n_x: v += xp[i * n_x + j]
                z[j] = v % R
            want += z + za + [0] * (4 * n - L) + zb + [0] * (4 * n - L)
        assert want[0] == 0 and want[201] == 0
        assert first_bad(back(out), want) is None, n_x


# ---- fr_spmv ------------------------------------------------------------------------------------------------------------------------------------------------
def test_fr_spmv_row_shapes_cancelling_pairs_and_edge_entries():
    """One matrix with rows on every path (a lane, a wave, the whole grid per row), rows whose entries cancel in adjacent pairs and across the halves of the row,
    a row of (r - 1) (r - 1) products, rows of zeros, and short rows of edge values, against the oracle."""
    ncols = 512; rng = random.Random(77)
    x = E.cycle(E.E, 64) + E.uniform(ncols - 64, 600)        # x[3] = r - 1
    rows, zero_rows = {}, []
    at_rows = iter(random.Random(78).sample(range(1, 2999), 60))
    def put(cols, vals, zero=False, where=None):
        i = next(at_rows) if where is None else where; rows[i] = (cols, vals)
        if zero: zero_rows.append(i)
    for j, l in enumerate((1, 2, 64, 65, 128, 8192, 8193, 20000)):
        put([rng.randrange(ncols) for _ in range(l)], E.uniform(l, 610 + j), where=2999 if l == 20000 else None)      # the longest as the very last row
    for j, l in enumerate((2, 64, 66, 128, 130, 8192, 8194, 20000)):
        cols, vals = [rng.randrange(ncols) for _ in range(l // 2)], E.uniform(l // 2, 620 + j, nonzero=True)
        put([q for q in cols for _ in range(2)], [w for v in vals for w in (v, R - v)], zero=True)                    # (v, x_j), (r - v, x_j) side by side
        put(cols + cols, vals + [R - v for v in vals], zero=True)                                                     # ... and half a row apart
    put([3] * 100, [R - 1] * 100); put([3] * 9000, [R - 1] * 9000)
    put([rng.randrange(ncols) for _ in range(70)], [0] * 70, zero=True); put([0, 1, 2, 3] * 2100, [0] * 8400, zero=True)
    put(list(range(64)), [0] * 64, zero=True, where=0)
    nrows = 3000
    for i in range(nrows):
        if i not in rows:
            l = i % 6                                         # short rows (empty ones too) of edge values against the edge part of x
            rows[i] = ([(i + 5 * q) % 64 for q in range(l)], [E.E[(i + 7 * q) % 18] for q in range(l)])
    lens = np.array([len(rows[i][0]) for i in range(nrows)], dtype=np.int64)
    row_ptr = np.zeros(nrows + 1, dtype=np.uint32); row_ptr[1:] = np.cumsum(lens)
    col = np.array([q for i in range(nrows) for q in rows[i][0]], dtype=np.uint32)
    vals = E.limbs([v for i in range(nrows) for v in rows[i][1]]); xs = E.limbs(x)
    exp = c.fr_spmv(row_ptr, col, vals, xs)
    assert (exp[zero_rows] == 0).all() and len(zero_rows) == 19
    for i in (1, 2, 3, 4, 5, 11, 2998):                      # the oracle itself against integers, on short rows
        if i in rows and len(rows[i][0]) <= 5: assert E.ints(exp[i])[0] == sum(mmul(v, x[q]) for q, v in zip(*rows[i])) % R
    d_rp, d_col, d_v, d_x, d_y = dev_u32(row_ptr), dev_u32(col), dev_raw(vals), dev_raw(xs), zeros(nrows, -1)
    poly.spmv_device(d_y.data_ptr(), d_rp.data_ptr(), d_col.data_ptr(), d_v.data_ptr(), d_x.data_ptr(), nrows)
    got = back_raw(d_y)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], [int(lens[i]) for i in bad[:8]])


# ---- fr_divide_by_linear, fr_eval_batch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 16, 17, 4096, 4097, (1 << 20) + 4097])
def test_divide_and_evaluate_edge_coefficients_edge_points_and_a_root(n):
    """Coefficients cycling through E at z in {0, 1, r - 1}; and (X - z) q(X), multiplied out in integers, whose value at z is 0 and whose quotient is q.
    The last size has two chunks per lane with a ragged last lane."""
    coeffs = np.resize(E.limbs(E.E), (n, 4))
    d_p = dev_raw(coeffs); d_q = zeros(n, -1); d_ev = zeros(1, -1); d_out = zeros(2, -1)
    for z_abs in (0, 1, R - 1):
        z = c.fr_to_mont(c.ints_to_limbs([z_abs], 4))[0]; zi = E.ints(z)[0]
        assert zi == E.stored(z_abs)
        polys = [(coeffs, d_p, None)]
        if 2 <= n <= 4097:
            q = E.cycle(E.E, n - 1, start=1, step=5) ; q[-1] = q[-1] or 1
            pz = [((q[i - 1] if i else 0) - (mmul(zi, q[i]) if i < n - 1 else 0)) % R for i in range(n)]      # (X - z) q(X)
            polys.append((E.limbs(pz), dev(pz), q))
        for f, d_f, q in polys:
            poly.divide_by_linear_device(d_q.data_ptr(), d_ev.data_ptr(), d_f.data_ptr(), n, z)
            eq, ee = c.fr_divide_by_linear(f, z)
            ev = back_raw(d_ev, 1)[0]
            assert (ev == ee).all(), (n, z_abs)
            if n > 1: assert (back_raw(d_q, n - 1) == eq).all(), (n, z_abs)
            if q is not None: assert E.ints(ev) == [0] and back(d_q, n - 1) == q, (n, z_abs)
        poly.fr_eval_batch_device(d_out.data_ptr(), [d_f.data_ptr() for _, d_f, _ in polys], [n] * len(polys), np.stack([z] * len(polys)))
        got = back_raw(d_out)
        for j, (f, _, q) in enumerate(polys):
            assert (got[j] == c.fr_divide_by_linear(f, z)[1]).all(), (n, z_abs, j)
            if q is not None: assert E.ints(got[j]) == [0]
    if n <= 4097:                                            # the oracle's evaluation itself against integers (Horner in the stored domain)
        z = E.uniform(1, 700 + n)[0]; acc = 0
        for v in reversed(E.ints(coeffs)): acc = (mmul(acc, z) + v) % R
        assert E.ints(c.fr_divide_by_linear(coeffs, k(z))[1]) == [acc]
        poly.divide_by_linear_device(0, d_ev.data_ptr(), d_p.data_ptr(), n, k(z))
        assert back(d_ev, 1) == [acc]


# ---- fr_powers ----------------------------------------------------------------------------------------------------------------------------------------------
def test_fr_powers_both_kernels_at_the_size_that_routes_between_them():
    """n = 2^26 is the largest size of k_fr_powers_fast (its last lane selects every one of the 24 host squarings); n = 2^26 + 17 the smallest of k_fr_powers.
    One buffer of 2 GiB holds both runs (different sequences, so a run cannot pass on what the other left); values are read back at chosen indices only."""
    import torch
    n_fast = 1 << 26; n_slow = n_fast + 17
    buf = torch.empty((n_slow, 4), dtype=torch.int64, device='cuda'); torch.cuda.synchronize()
    for n, seed in ((n_fast, 800), (n_slow, 810)):
        first, ratio = E.uniform(2, seed, nonzero=True)      # abstract values
        idx = {0} | set(range(n - 5, n)) | set(random.Random(seed + 1).sample(range(n), 2048))
        t = 1
        while 4 * t - 1 < n:
            idx |= {i for i in (4 * t - 1, 4 * t + 1, 16 * t - 1, 16 * t + 1) if i < n}; t *= 2
        idx = sorted(idx)
        poly.fr_powers_device(buf.data_ptr(), n, k(E.stored(first)), k(E.stored(ratio)))
        got = back(buf[torch.tensor(idx, dtype=torch.int64, device='cuda')])
        want = [E.stored(first * pow(ratio, i, R) % R) for i in idx]
        assert first_bad(got, want) is None, (n, [idx[j] for j in range(len(idx)) if got[j] != want[j]][:8])
    del buf
    n = 4099; dst = zeros(n, -1)
    for first, ratio in ((5, 0), (7, 1), (11, R - 1), (0, 3), (0, 0), (R - 1, R - 1)):
        poly.fr_powers_device(dst.data_ptr(), n, k(E.stored(first)), k(E.stored(ratio)))
        assert first_bad(back(dst), [E.stored(first * pow(ratio, i, R) % R) for i in range(n)]) is None, (first, ratio)


# ---- fr_mul / fq_mul on raw limbs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('field', ['fr', 'fq'])
def test_field_products_on_raw_limb_patterns(field):
    from oracle import pyref as p
    N, P, mask, bound, mul = (8, R, (1 << 254) - 1, 2 * R, M.fr_mul) if field == 'fr' else (12, p.FQ_MODULUS, (1 << 381) - 1, 4 * p.FQ_MODULUS, M.fq_mul)
    full = (1 << (32 * N)) - 1
    alt = sum(0xffffffff << (64 * i) for i in range(N // 2))
    pats = [0, full, alt, alt << 32] + [0xffffffff << (32 * i) for i in range(N)] + [P - 1, P, P + 1, 2 * P - 1]
    pats = [v & mask for v in pats]
    a = [x for x in pats for _ in pats]; b = [y for _ in pats for y in pats]
    for x, y in zip(a, b): assert x * y // (full + 1) + P < bound         # every pair is inside reduce()'s contract: none is left out
    rinv = pow(full + 1, -1, P)
    A, B = E.limbs(a, N // 2), E.limbs(b, N // 2)
    assert first_bad(E.ints(mul(A, B)), [x * y * rinv % P for x, y in zip(a, b)]) is None
    S = E.limbs(pats, N // 2)
    assert first_bad(E.ints(mul(S, S)), [x * x * rinv % P for x in pats]) is None      # the same buffer twice: the squaring block


# ---- the seven kernels that only the native prover launches, through aleo_mi355x_selftest_fr_step ----------------------------------------------------------------
def test_fr_step_refuses_unknown_steps_and_nulls():
    d = zeros(4)
    assert fr_step(7, [d.data_ptr()] * 4, [1]) == BAD_ARG
    L = aleo_amd.lib()
    assert L.aleo_mi355x_selftest_fr_step(0, None, (ctypes.c_size_t * 1)(1), None) == BAD_ARG
    assert L.aleo_mi355x_selftest_fr_step(0, (ctypes.c_void_p * 2)(d.data_ptr(), d.data_ptr()), None, None) == BAD_ARG
    assert fr_step(ADD_TILED, [d.data_ptr(), 0], [4, 4]) == BAD_ARG
    assert fr_step(SUB_MUL, [d.data_ptr(), d.data_ptr(), d.data_ptr(), 0], [4]) == BAD_ARG
    assert fr_step(SCALE_ROWS, [d.data_ptr(), d.data_ptr()], [1, 1]) == BAD_ARG          # no constants
    assert fr_step(PICK, [d.data_ptr(), 0], [1]) == BAD_ARG
    assert fr_step(GATHER_MUL3, [d.data_ptr(), 0] + [d.data_ptr()] * 4, [1, 1]) == BAD_ARG
    assert fr_step(GATHER_MUL3, [d.data_ptr(), d.data_ptr(), d.data_ptr(), 0, d.data_ptr(), d.data_ptr()], [1, 1]) == BAD_ARG
    assert fr_step(SCATTER, [d.data_ptr(), d.data_ptr(), 0, 0], [1]) == BAD_ARG
    assert fr_step(SPLIT, [d.data_ptr(), 0, d.data_ptr(), 0, 0], [1]) == BAD_ARG
    assert back(d) == [0] * 4


def test_fr_add_tiled():
    n = 4096
    ea, eb = E.edge_pairs(n); ea[-14:] = [x for x, _, _ in E.CARRY_ADD + E.CARRY_SUB]; eb[-14:] = [y for _, y, _ in E.CARRY_ADD + E.CARRY_SUB]
    d, s = dev(ea), dev(eb)
    assert fr_step(ADD_TILED, [d.data_ptr(), s.data_ptr()], [n, n]) == 0
    assert first_bad(back(d), [(x + y) % R for x, y in zip(ea, eb)]) is None
    for n_src in (1, 256, n):
        for j, blocks in enumerate((E.cycle(E.E, n_src, start=n_src % 7, step=5), E.uniform(n_src, 900 + n_src))):
            dst = E.uniform(n, 910 + j); dst[:18] = E.E
            d, s = dev(dst), dev(blocks)
            assert fr_step(ADD_TILED, [d.data_ptr(), s.data_ptr()], [n, n_src]) == 0
            assert first_bad(back(d), [(x + blocks[i % n_src]) % R for i, x in enumerate(dst)]) is None, (n_src, j)
        src = E.uniform(n_src, 920 + n_src); src[0] = 0       # src[i mod n_src] = r - dst[i]: every sum is r (0 + 0 aside), with the two neighbours
        dst = [(R - src[i % n_src]) % R for i in range(n)]; want = [0] * n
        for i, w in ((5, 1), (n - 3, R - 1), (n // 2, 1)): dst[i] = (dst[i] + w) % R; want[i] = w
        d, s = dev(dst), dev(src)
        assert fr_step(ADD_TILED, [d.data_ptr(), s.data_ptr()], [n, n_src]) == 0
        assert first_bad(back(d), want) is None, n_src
    keep = E.uniform(n, 930); d = dev(keep)                   # a block size that is no power of two, that does not divide n, that is 0
    for bad in (3, 96, 8192, 0):
        assert fr_step(ADD_TILED, [d.data_ptr(), s.data_ptr()], [n, bad]) == BAD_ARG, bad
    assert fr_step(ADD_TILED, [d.data_ptr(), s.data_ptr()], [n + 1, 2]) == BAD_ARG
    assert back(d) == keep


def test_fr_sub_mul():
    a, b, m = E.edge_triples()
    u = E.uniform(18 * 40, 1000)
    for j, w in enumerate(E.E):                               # per multiplier from E: a = b, a - b = 1, a - b = r - 1, on edge and uniform a
        xs = E.E + u[40 * j:40 * j + 22]
        for x in xs: a += [x, x, x]; b += [x, (x - 1) % R, (x + 1) % R]; m += [w] * 3
    n = len(a); assert n > 5832 + 2000
    want = [mmul((x - y) % R, w) for x, y, w in zip(a, b, m)]
    dA, dB, dM, dst = dev(a), dev(b), dev(m), zeros(n, -1)
    assert fr_step(SUB_MUL, [dst.data_ptr(), dA.data_ptr(), dB.data_ptr(), dM.data_ptr()], [n]) == 0
    assert first_bad(back(dst), want) is None
    assert fr_step(SUB_MUL, [dA.data_ptr(), dA.data_ptr(), dB.data_ptr(), dM.data_ptr()], [n]) == 0      # in place over a
    assert first_bad(back(dA), want) is None


def test_fr_scale_rows():
    n = 333                                                   # no multiple of the block
    src = E.cycle(E.E, n, step=5); d_src = dev(src)
    for rows in (1, 4):
        for s in range(5):
            K = E.cycle(E.E, rows, start=4 * s + (rows == 1))
            dst = zeros(rows * n + 1, -1)
            assert fr_step(SCALE_ROWS, [dst.data_ptr(), d_src.data_ptr()], [n, rows], K) == 0
            got = back(dst)
            assert first_bad(got[:rows * n], [mmul(kk, x) for kk in K for x in src]) is None, (rows, s)
            assert got[rows * n] == (1 << 256) - 1            # nothing behind the last row
    dst = zeros(5 * n, -1)
    assert fr_step(SCALE_ROWS, [dst.data_ptr(), d_src.data_ptr()], [n, 5], E.E[:5]) == BAD_ARG
    assert back(dst) == [(1 << 256) - 1] * (5 * n)


def test_fr_pick():
    vec = E.cycle(E.E, 300, start=3, step=7); v = dev(vec); other = dev(E.E)
    where = [(v, 0), (v, 299), (other, 17), (v, 150), (other, 0), (v, 298), (v, 1), (v, 299)]
    for count in (1, 8):
        for flip in (False, True):                           # the first source the vector's first element, or its last
            w = where[::-1][:count] if flip else where[:count]
            dst = zeros(9, -1)
            assert fr_step(PICK, [dst.data_ptr()] + [at(t, i) for t, i in w], [count]) == 0
            got = back(dst)
            assert got[:count] == [(vec if t is v else E.E)[i] for t, i in w] and got[count:] == [(1 << 256) - 1] * (9 - count)
    dst = zeros(9, -1)
    assert fr_step(PICK, [dst.data_ptr()] + [at(v, i) for i in range(9)], [9]) == BAD_ARG
    assert back(dst) == [(1 << 256) - 1] * 9


def test_fr_gather_mul3():
    """One to three ranges of lengths {0, 1, 257} in every position (the empty range first, in the middle, last, all empty) over tables of E: against integers,
    and element by element against fr_gather_mul_device on the same inputs."""
    t1, t2 = E.cycle(E.E, 18, start=1, step=7), E.cycle(E.E, 18, start=4, step=11)
    d1, d2 = dev(t1), dev(t2); top = 257; SENT = (1 << 256) - 1
    I1 = [[(i * (m + 1) + m) % 18 for i in range(top)] for m in range(3)]; I2 = [[(i // 3 + 5 * m) % 18 for i in range(top)] for m in range(3)]
    for m in range(3): I1[m][0], I2[m][0] = (0, 17) if m != 1 else (17, 0)
    SC = [E.cycle(E.E, top, start=2 * m, step=5) for m in range(3)]
    dI1, dI2, dSC = [dev_u32(v) for v in I1], [dev_u32(v) for v in I2], [dev(v) for v in SC]
    want = [[mmul(mmul(t1[I1[m][i]], t2[I2[m][i]]), SC[m][i]) for i in range(top)] for m in range(3)]
    ref = []
    for m in range(3):
        r_ = zeros(top, -1); poly.fr_gather_mul_device(r_.data_ptr(), top, dSC[m].data_ptr(), d1.data_ptr(), dI1[m].data_ptr(), d2.data_ptr(), dI2[m].data_ptr())
        ref.append(back(r_)); assert ref[m] == want[m]
    for count in (1, 2, 3):
        shapes = [[]]
        for _ in range(count): shapes = [s + [l] for s in shapes for l in (0, 1, 257)]
        for lens in shapes:
            D = [zeros(top, -1) for _ in range(count)]
            ptrs = [d1.data_ptr(), d2.data_ptr()]
            for m in range(count): ptrs += [D[m].data_ptr(), dSC[m].data_ptr(), dI1[m].data_ptr(), dI2[m].data_ptr()]
            assert fr_step(GATHER_MUL3, ptrs, [count] + lens) == 0, lens
            for m in range(count):
                got = back(D[m])
                assert got[:lens[m]] == ref[m][:lens[m]] and got[lens[m]:] == [SENT] * (top - lens[m]), (lens, m)
    D = zeros(top, -1)                                        # an empty range may come without pointers
    assert fr_step(GATHER_MUL3, [d1.data_ptr(), d2.data_ptr(), 0, 0, 0, 0, D.data_ptr(), dSC[1].data_ptr(), dI1[1].data_ptr(), dI2[1].data_ptr()], [2, 0, 257]) == 0
    assert back(D) == ref[1]
    for count in (0, 4):
        assert fr_step(GATHER_MUL3, [d1.data_ptr(), d2.data_ptr()] + [D.data_ptr(), dSC[0].data_ptr(), dI1[0].data_ptr(), dI2[0].data_ptr()] * 4, [count, 1, 1, 1, 1]) == BAD_ARG
    assert back(D) == ref[1]


def test_fr_scatter_to_mont_and_its_flag():
    import torch
    n, slots = 1000, 1500
    src = E.E + E.uniform(n - 18, 1100)                       # canonical values (0 and r - 1 among them): dst[pos[v]] = their stored form
    pos = random.Random(1101).sample(range(slots), n)
    want = [0] * slots
    for v, q in zip(src, pos): want[q] = E.stored(v)
    d_src, d_pos = dev(src), dev_u32(pos)
    def flag_tensor():
        f = torch.zeros(2, dtype=torch.int32, device='cuda'); torch.cuda.synchronize(); return f
    dst, flag = zeros(slots), flag_tensor()
    assert fr_step(SCATTER, [dst.data_ptr(), d_src.data_ptr(), d_pos.data_ptr(), flag.data_ptr()], [n]) == 0
    assert first_bad(back(dst), want) is None and flag.cpu().tolist() == [0, 0]      # untouched slots stay as the caller zeroed them
    dst = zeros(slots)                                        # without a flag
    assert fr_step(SCATTER, [dst.data_ptr(), d_src.data_ptr(), d_pos.data_ptr(), 0], [n]) == 0
    assert first_bad(back(dst), want) is None
    for where, v in ((0, R), (n - 1, R + 1), (517, (1 << 256) - 1)):      # one entry that is not below r raises the flag; every other entry is laid out all the same
        s2 = list(src); s2[where] = v; d_s2 = dev(s2)
        dst, flag = zeros(slots), flag_tensor()
        assert fr_step(SCATTER, [dst.data_ptr(), d_s2.data_ptr(), d_pos.data_ptr(), flag.data_ptr()], [n]) == 0
        assert flag.cpu().tolist() == [1, 0], hex(v)
        got = back(dst); got[pos[where]] = want[pos[where]]
        assert first_bad(got, want) is None
        assert fr_step(SCATTER, [dst.data_ptr(), d_s2.data_ptr(), d_pos.data_ptr(), 0], [n]) == 0


@pytest.mark.parametrize('n', [1, 255, 4096])
def test_fr_split_quotient(n):
    """hq = [p1 + p2 | p2], rq = p0 + p1 + p2 over the (masked) blocks, with rows built so that p1 + p2, p0 + p1 + p2 and p_k + mask_k are 0 mod r."""
    for masked in (False, True):
        for shift in range(4):
            P = [E.uniform(n, 1200 + 10 * shift + j) for j in range(3)]              # the blocks after the mask went in
            for i in range(n):
                kind = (i + shift) % 8
                if kind == 1: P[2][i] = (R - P[1][i]) % R                             # p1 + p2 = 0
                elif kind == 2: P[0][i] = (-P[1][i] - P[2][i]) % R                    # p0 + p1 + p2 = 0
                elif kind == 3: P[i % 3][i] = 0                                       # p_k + mask_k = 0
                elif kind == 4: P[0][i], P[1][i], P[2][i] = E.E[i % 18], E.E[i // 18 % 18], E.E[(i // 324 + 3) % 18]
                elif kind == 5: P[2][i] = (1 - P[1][i]) % R; P[0][i] = R - 2        # the neighbours: p1 + p2 = 1, the sum r - 1
                elif kind == 6: P[0][i] = P[1][i] = P[2][i] = 0
            mask = [E.uniform(n, 1250 + 10 * shift + j) for j in range(3)]
            q = [[(v - w) % R for v, w in zip(P[j], mask[j])] for j in range(3)] if masked else P
            d_q = dev(q[0] + q[1] + q[2]); d_m = dev(mask[0] + mask[1] + mask[2])
            want_hq = [(x + y) % R for x, y in zip(P[1], P[2])] + P[2]; want_rq = [(x + y + z) % R for x, y, z in zip(*P)]
            for with_sum in (True, False):
                hq, rq, hs = zeros(2 * n, -1), zeros(n, -1), zeros(1, -1)            # a device buffer stands in for the pinned host_sum
                assert fr_step(SPLIT, [hq.data_ptr(), rq.data_ptr(), d_q.data_ptr(), d_m.data_ptr() if masked else 0, hs.data_ptr() if with_sum else 0], [n]) == 0
                assert first_bad(back(hq), want_hq) is None and first_bad(back(rq), want_rq) is None, (masked, shift)
                assert back(hs) == ([want_rq[0]] if with_sum else [(1 << 256) - 1])
