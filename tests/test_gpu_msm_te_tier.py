"""The whole-set table tier in twisted Edwards form (aleo_amd/csrc/te28.h, msm_te.hip) through the C ABI: the sizes and call shapes that reach it — the existing
table-path tests stop at 2^14 points, below it — with the operand patterns its unified law must take in its stride (duplicates, opposites, triples, identity bases,
a long run of one pair, all-equal scalars, everything cancelling), bit-exact against the oracle and against the calls that do not use the tier; and the two kinds
of set the tier is not for: bases outside the prime-order subgroup (an exceptional pair must end in a rerun without tables, never in a wrong sum) and a base
without an Edwards image (a point of even order: the set gets no tables at all, see the last test)."""
import importlib.util, os
import numpy as np
import pytest

import aleo_amd
from aleo_amd import msm as M
from oracle import coracle as c, pyref as p
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N17 = (1 << 17) + 128          # the smallest reach the whole-set tier serves: c = 17


@pytest.fixture(scope='module', autouse=True)
def device():
    aleo_amd._lib.check(aleo_amd.lib().aleo_mi355x_init_device(-1), 'init')


def neg_row(row):
    return c.affine_from_ints([p.g1_neg(c.affine_to_ints(row.reshape(1, 104))[0])])[0]


def plant(B, S, mult, pairs):
    """The patterns of test_table_path_repeated_opposite_and_infinity_bases on the index pairs (i, j): mult[] follows (base = mult * G)."""
    for t, (i, j) in enumerate(pairs):
        kind = t % 4
        if kind == 0: B[j] = B[i]; S[j] = S[i]; mult[j] = mult[i]                                   # P == acc
        elif kind == 1: B[j] = neg_row(B[i]); S[j] = S[i]; mult[j] = -mult[i]                       # P == -acc
        elif kind == 2: B[j] = B[i]; B[j + 1] = B[i]; S[j] = S[i]; S[j + 1] = S[i]; mult[j] = mult[i]; mult[j + 1] = mult[i]      # tripled
        else: B[j] = 0; B[j, 96] = 1; mult[j] = 0                                                   # an identity base


@pytest.fixture(scope='module')
def set17():
    """2^17 + 128 bases with the patterns planted, their scalars, and the oracle's sum — computed once"""
    B = util.multiples_bases(N17); S = util.uniform_scalars(N17, 9910); mult = [i + 1 for i in range(N17)]
    plant(B, S, mult, [(k, k + 1) for k in range(0, 4000, 8)])
    S[5000:5200] = S[5000]; B[5000:5200] = B[5000]                                                  # 200 copies of one (point, scalar)
    return B, S, c.jac_to_int_point(c.msm_g1(B, S, threads=8, variant=1))


def test_smallest_whole_set_tier_equals_the_oracle_and_the_plain_path(set17):
    B, S, exp = set17
    with M.PinnedBases(B) as pb:
        plain = M.VariableBase.msm(pb, S)
        assert c.jac_to_int_point(plain) == exp
        pb.precompute()
        assert pb.info()['tier_window_bits'][0] == 17
        got = M.VariableBase.msm(pb, S)
        assert c.jac_to_int_point(got) == exp and (got == plain).all()                              # bit-equal to the plain path
        Z = S.copy(); Z[:] = S[0]
        assert c.jac_to_int_point(M.VariableBase.msm(pb, Z)) == c.jac_to_int_point(c.msm_g1(B, Z, threads=8, variant=1))      # all-equal scalars


def test_everything_cancels_to_the_identity_on_the_whole_set_tier():
    B = util.multiples_bases(N17); B[1::2] = B[0::2]
    S = util.uniform_scalars(N17, 9911)
    ints = c.limbs_to_ints(S[0::2]); S[1::2] = c.ints_to_limbs([(p.FR_MODULUS - v) % p.FR_MODULUS for v in ints], 4)
    with M.PinnedBases(B) as pb:
        pb.precompute()
        assert c.jac_to_int_point(M.VariableBase.msm(pb, S)) is None


def test_seeded_chunks_with_patterns_across_the_chunks():
    """2^19 host scalars: c = 20, two chunks that share the buckets (the second accumulation is seeded with the first's sums).  Duplicates and opposites sit in
    different chunks.  Checked by the O(n) identity k * G in Python integers, and for equality with the call whose scalars are resident (one chain, no seeds)."""
    import torch
    n = 1 << 19
    B = util.multiples_bases(n); S = util.uniform_scalars(n, 9912); mult = [i + 1 for i in range(n)]
    plant(B, S, mult, [(8 * k, n // 2 + 8 * k) for k in range(500)])                                # i in the first 37 %, j in the second chunk
    S[n - 300:n - 100] = S[100]; B[n - 300:n - 100] = B[100]; mult[n - 300:n - 100] = [mult[100]] * 200      # 200 copies in the second chunk of a pair in the first
    k = sum(s * m for s, m in zip(c.limbs_to_ints(S), mult)) % p.FR_MODULUS
    exp = p.g1_mul(p.G1_GENERATOR, k)
    with M.PinnedBases(B) as pb:
        pb.precompute()
        assert pb.info()['tier_window_bits'][0] == 20
        got = M.VariableBase.msm(pb, S)
        assert c.jac_to_int_point(got) == exp
        assert aleo_amd.last_msm_timing()['accum_launches'] == 2
        d = torch.from_numpy(S.view(np.int64).copy()).cuda(); torch.cuda.synchronize()
        assert (M.VariableBase.msm_device(pb, d.data_ptr(), n) == got).all()


def test_a_batched_request_equals_its_single_calls(set17):
    import torch
    B, S, _ = set17
    vecs = [S, util.witness_like_scalars(N17, 9913), util.uniform_scalars(N17 - 77, 9914)]
    with M.PinnedBases(B) as pb:
        pb.precompute()
        d = [torch.from_numpy(v.view(np.int64).copy()).cuda() for v in vecs]; torch.cuda.synchronize()
        got = M.VariableBase.msm_batch_device(pb, [t.data_ptr() for t in d], [len(v) for v in vecs])
        for j, v in enumerate(vecs):
            assert (got[j] == M.VariableBase.msm_device(pb, d[j].data_ptr(), len(v))).all(), j


# ---- sets the tier is not for --------------------------------------------------------------------------------------------------------------------
def model():
    spec = importlib.util.spec_from_file_location('te28_model', os.path.join(ROOT, 'tools', 'te28_model.py'))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_an_exceptional_pair_outside_g1_still_gives_the_oracles_sum():
    """P = 3 G and P + S, S of order 2, as the first two bases with equal scalars: they meet at the head of their buckets' first slices, where the unified
    law has Z3 = 0 (asserted on the CPU model first).  The call must notice and return the right sum."""
    m = model(); Q = p.Q
    P = p.g1_mul(p.G1_GENERATOR, 3)
    w = (p.fq_sqrt(-3 % Q) - 1) * pow(2, -1, Q) % Q                                                 # a primitive cube root of unity
    torsion = [(Q - 1, 0), (-w % Q, 0), (-w * w % Q, 0)]                                            # the three points of order 2
    assert all(p.g1_is_on_curve(T) and p.g1_add(T, T) is None for T in torsion)
    S2 = next((T for T in torsion if m.to_edwards(p.g1_add(P, T)) is not None and
               m.madd(m.ext(m.to_edwards(P)), m.row(m.to_edwards(p.g1_add(P, T))))[2] == 0), None)
    assert S2 is not None, 'no point of order 2 makes the CPU model\'s Z3 vanish'
    PS = p.g1_add(P, S2)
    assert m.add(m.ext(m.to_edwards(P)), m.ext(m.to_edwards(PS)))[2] == 0 and not p.g1_in_subgroup(PS)
    B = util.multiples_bases(N17); S = util.uniform_scalars(N17, 9915)
    B[0:2] = c.affine_from_ints([P, PS]); S[1] = S[0]
    exp = c.jac_to_int_point(c.msm_g1(B, S, threads=8, variant=1))
    with M.PinnedBases(B) as pb:
        pb.precompute()
        assert c.jac_to_int_point(M.VariableBase.msm(pb, S)) == exp
        assert c.jac_to_int_point(M.VariableBase.msm(pb, S)) == exp                                 # and again: nothing sticks


def test_a_base_without_an_edwards_image_precomputes_and_multiplies_correctly():
    """(-1, 0) is on the curve, has order 2 and no finite Edwards image, so the set cannot get the Edwards tier.  It cannot get the XYZZ tiers either: on the
    parent commit the same set precomputes (table_bytes 604520448 at 2^17 + 128 points, 41943040 at 2^14) and then multiplies WRONGLY with its tables while the
    plain path is right — 2^k (-1, 0) is the identity, which an affine table row cannot hold and the sort does not drop.  Such a set (any base of even order
    whose multiples vanish inside a table) therefore gets no tables now: it precomputes without error and multiplies on the plain path."""
    B = util.multiples_bases(N17); S = util.uniform_scalars(N17, 9916)
    B[12345] = c.affine_from_ints([(p.Q - 1, 0)])[0]
    exp = c.jac_to_int_point(c.msm_g1(B, S, threads=8, variant=1))
    with M.PinnedBases(B) as pb:
        pb.precompute()
        assert pb.info()['table_bytes'] == 0
        assert c.jac_to_int_point(M.VariableBase.msm(pb, S)) == exp
