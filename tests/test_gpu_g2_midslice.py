"""The G2 accumulation kernel (k_g2_accum28) leaving its fast loop in the MIDDLE of a slice, with a lazily reduced accumulator.

When the loop meets P == +-acc it stores its accumulator (X up to 12q, Y up to 6q) and the even lane reloads both halves and finishes the slice in the
32-bit code.  In test_msm_g2_edge_cases every such refusal happens at the first addition of a slice, with an affine accumulator.  Here four bases
{a, b, s (a + b), d} with equal scalars share every bucket: n = 4 gives c = 2 (127 windows, 2 buckets) and a slice rule that keeps a bucket of four in one
slice, so every non-empty bucket is one slice of all four points.  Summed in the order a, b, s (a + b), d the third addition meets the running sum itself
(s = +1: the slow path doubles it) or its opposite (s = -1: it cancels to the identity, and d still follows).  The order inside a bucket is the sort's
business and not specified, so all 24 orders of the four bases are run: whatever deterministic order the sort applies to equal keys, some call presents
a, b, s (a + b) in that order.  Every result is compared with the known multiple of the generator in Python integers.
"""
import itertools
import numpy as np
import pytest

from aleo_amd import msm as M, synth
from oracle import coracle as c, pyref as p

pytestmark = pytest.mark.gpu

R = p.FR_MODULUS
MULT = {+1: (1, 2, 3, 7), -1: (1, 2, -3, 7)}                    # a, b, s (a + b), d as multiples of the generator


@pytest.fixture(scope='module')
def bases():
    G = p.G2_GENERATOR
    pts = {m: (p.g2_mul(G, m) if m > 0 else p.g2_neg(p.g2_mul(G, -m))) for m in (1, 2, 3, -3, 7)}
    return {s: c.g2_affine_from_ints([pts[m] for m in MULT[s]]) for s in MULT}


@pytest.fixture(scope='module')
def scalars():
    """One uniform scalar and r - 1 (every digit negated), each repeated for the four bases; with the integers."""
    u = synth.uniform_scalars(1, 17100); rm1 = c.ints_to_limbs([R - 1], 4)
    return [(np.tile(s, (4, 1)), c.limbs_to_ints(s)[0]) for s in (u, rm1)]


def expected(sign, k):
    m = sum(MULT[sign]) * k % R
    return p.g2_mul(p.G2_GENERATOR, m) if m else None


@pytest.mark.parametrize('sign', [+1, -1], ids=['sum_meets_itself', 'sum_cancels'])
def test_every_order_of_a_b_their_sum_and_d_in_one_slice(bases, scalars, sign):
    B = bases[sign]
    for S, k in scalars:
        want = expected(sign, k)
        for order in itertools.permutations(range(4)):
            got = M.msm_g2(B[list(order)], S)
            assert c.g2_jac_to_int_point(got) == want, (sign, k, order)
        assert c.g2_jac_to_int_point(c.msm_g2(B, S)) == want                 # one order also against the oracle's MSM
        assert (M.msm_g2(B, S) == M.msm_g2(B[[3, 2, 1, 0]], S)).all()


@pytest.mark.parametrize('sign', [+1, -1], ids=['sum_meets_itself', 'sum_cancels'])
def test_the_same_through_a_pinned_set(bases, scalars, sign):
    B = bases[sign]
    with M.PinnedG2Bases(B) as pg:
        for S, k in scalars:
            got = pg.msm(S)
            assert c.g2_jac_to_int_point(got) == expected(sign, k), (sign, k)
            assert (got == M.msm_g2(B, S)).all()
