"""The twisted Edwards model of G1 that the 7-product mixed addition rests on (tools/te28_model.py), against oracle/pyref.py in Python integers.

The constants the C++ side uses are the limbs in aleo_amd/csrc/te28_consts.h, written by the model; this test reads them back from that file (they
are typed nowhere) and checks them and the group laws: the curve equation on the images of 1..64 G, the map against its inverse, and the unified
mixed and general additions against g1_add — every pair of a small set with P + P, P - P and identity operands, and a 200-step random walk."""
import importlib.util, os, random, re
import pytest
from oracle import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('te28_model', os.path.join(ROOT, 'tools', 'te28_model.py'))
M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
HEADER = os.path.join(ROOT, 'aleo_amd', 'csrc', 'te28_consts.h')
Q, G = R.Q, R.G1_GENERATOR


def header_constants():
    """{name: integer} from the limbs of te28_consts.h, taken out of their Montgomery forms"""
    out = {}
    for name, n, body in re.findall(r'static constexpr uint32_t (\w+)\[(\d+)\] = \{([^}]*)\};', open(HEADER).read()):
        w = [int(t.strip().rstrip('u'), 16) for t in body.split(',')]
        assert len(w) == int(n)
        bits, radix = (28, 392) if name.endswith('_28') else (32, 384)
        assert all(x < (1 << bits) for x in w)
        v = sum(x << (bits * i) for i, x in enumerate(w))
        assert v < Q, name
        out[name] = v * pow(1 << radix, -1, Q) % Q
    return out


@pytest.fixture(scope='module')
def multiples():
    pts, P = [], None
    for _ in range(64):
        P = R.g1_add(P, G); pts.append(P)
    return pts


def test_header_is_what_the_model_writes_and_its_limbs_are_the_models_constants():
    assert open(HEADER).read() == M.header_text()
    C = header_constants()
    assert set(C) == {n + sfx for n in M.CONSTANTS for sfx in ('_28', '_32')}
    for n, v in M.CONSTANTS.items():
        assert C[n + '_28'] == v and C[n + '_32'] == v, n
    # and what the constants are, from the header's values alone
    s3, f, d, k = C['TE_SQRT3_28'], C['TE_F_28'], C['TE_D_28'], C['TE_K_28']
    assert s3 * s3 % Q == 3 and C['TE_S_28'] * s3 % Q == 1 and C['TE_F_INV_28'] * f % Q == 1 and k == 2 * d % Q and C['TE_D_INV_28'] * d % Q == 1 and C['TE_TWO_28'] == 2 and C['TE_ONE_28'] == 1
    s = C['TE_S_28']; A, B = -3 * s % Q, s
    a, dt = (A + 2) * pow(B, -1, Q) % Q, (A - 2) * pow(B, -1, Q) % Q
    assert f * f % Q == -a % Q and d == -dt * pow(a, -1, Q) % Q
    assert d in (0xcb5d5818b4d2796505bb385732fe3a1bbc34cc60d19690bf8b2d97f059909cb9aeca3c3871e9f27016092b426b700b,
                 0xe2dcedff103e7161354a88156e4b00fe66a526a0237cfe5f683497c9afb7635d5c9307f78e160e14f2b6d4bd949004)
    assert pow(d, (Q - 1) // 2, Q) == 1          # d is a square: the law is complete on the odd-order points only


def test_images_lie_on_the_curve_and_the_map_inverts(multiples):
    assert M.on_curve(M.IDENTITY) and M.from_edwards(M.to_edwards(None)) is None
    for P in multiples:
        E = M.to_edwards(P)
        assert E is not None and M.on_curve(E)
        assert M.from_edwards(E) == P
        assert M.to_edwards(R.g1_neg(P)) == M.neg(E)
        assert M.row_neg(M.row(E)) == M.row(M.neg(E))
    assert M.row(M.IDENTITY) == (1, 1, 0)
    assert M.to_edwards((Q - 1, 0)) is None      # the 2-torsion point has no finite image


def check_sum(P, S):
    exp = R.g1_add(P, S)
    ep, es = M.to_edwards(P), M.to_edwards(S)
    for got in (M.madd(M.ext(ep), M.row(es)), M.add(M.ext(ep), M.ext(es)), M.add(M.ext(es), M.ext(ep))):
        e = M.affine(got)
        assert e is not None and M.on_curve(e) and M.from_edwards(e) == exp
        if exp is None: assert got[0] % Q == 0 and got[3] % Q == 0 and got[1] == got[2] != 0      # (0 : Z : Z : 0)


def test_unified_additions_equal_g1_add_on_all_pairs_of_a_small_set():
    pts = [R.g1_mul(G, k) for k in (1, 2, 3, 5, 7, 11, 12345, (1 << 200) + 7)]
    pts = pts + [R.g1_neg(P) for P in pts] + [None]
    for P in pts:
        for S in pts:
            check_sum(P, S)          # P + P, P + (-P) and both identity operands are among them


def test_projective_operands_and_a_random_walk(multiples):
    rng = random.Random(0x7e28)
    acc_w, acc = None, M.ext(M.IDENTITY)
    run_w, run = None, M.ext(M.IDENTITY)
    for step in range(200):
        P = multiples[rng.randrange(64)]
        if rng.random() < 0.5: P = R.g1_neg(P)
        if step % 50 == 49: P = R.g1_neg(acc_w)                 # walk through the identity a few times
        acc = M.madd(acc, M.row(M.to_edwards(P))); acc_w = R.g1_add(acc_w, P)
        assert M.from_edwards(M.affine(acc)) == acc_w             # Z != 1 operands from here on
        run = M.add(run, acc); run_w = R.g1_add(run_w, acc_w)     # the general addition on two projective operands (the reduction's running sums)
        assert M.from_edwards(M.affine(run)) == run_w
    assert M.affine(M.add(acc, acc)) == M.to_edwards(R.g1_add(acc_w, acc_w))
