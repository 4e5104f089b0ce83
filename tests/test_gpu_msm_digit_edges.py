"""The scalars at the edges of the signed-digit recoding (msm_sort_ref.edge_scalars: windows equal to B, B + 1, B - 1, 2^width - 1 in chains; 0, 1, 2, r - 1,
r - 2, (r +- 1) / 2) through the public entry points, at one size per path of a pinned, precomputed set: the plain path, the c = 13 tier and the c = 16 tier,
the Montgomery (`commit`) entry, and a G2 call.  test_gpu_msm_sort.py pins what the sort leaves behind; this ties that contract to the sums: bit-exact against
sum_i s_i (i + 1) G in integers (the bases are the multiples 1, 2, .. of the generator)."""
import numpy as np
import pytest

import aleo_amd
from aleo_amd import msm as M, synth
import msm_sort_ref as ref

pytestmark = pytest.mark.gpu
N_PIN = (1 << 15) + 64
SIZES = [(600, 5), (2049, 13), (1 << 15, 16)]      # (points, the window width the call sorts by: lg(600) - 4 on the plain path, the tiers' widths)


@pytest.fixture(scope='module')
def pinned():
    with aleo_amd.PinnedBases.generate_multiples(synth.generator_affine104(), 1, N_PIN) as pb:
        pb.precompute()
        yield pb


def _scalars(n, c):
    """The mix of width c with its edge scalars moved to the ends and the middle of the vector as well as the front."""
    s = ref.mix(c, n, 0xD161E000 + n)
    e = ref.to_limbs(ref.edge_scalars(c)); k = e.shape[0]
    s[n - k:] = e[::-1]; s[n // 2:n // 2 + k] = e
    return s


def _expected_g1(scalars):
    from oracle import pyref as p
    k = synth.weighted_scalar_sum(scalars, 1)
    assert k == sum(v * (i + 1) for i, v in enumerate(ref.to_ints(scalars))) % ref.R
    return p.g1_mul(p.G1_GENERATOR, k) if k else None


@pytest.mark.parametrize('n,c', SIZES)
def test_msm_edge_scalars_bit_exact(pinned, oracle, n, c):
    s = _scalars(n, c)
    assert oracle.jac_to_int_point(aleo_amd.VariableBase.msm(pinned, s)) == _expected_g1(s)


def test_commit_edge_scalars_bit_exact(pinned, oracle):
    """The same mix in Montgomery form through KZG10::commit: the sort converts before it recodes."""
    s = _scalars(2049, 13)
    got = aleo_amd.KZG10.commit(pinned, ref.to_mont(s))
    assert oracle.affine_to_ints(got)[0] == _expected_g1(s)


def test_msm_g2_edge_scalars(oracle):
    from oracle import pyref as p
    n, c = 255, 3                                    # lg(255) - 4
    B = oracle.g2_multiples(oracle.g2_affine_from_ints([p.G2_GENERATOR])[0], n)
    s = _scalars(n, c)
    got = oracle.g2_jac_to_int_point(M.msm_g2(B, s))
    assert got == oracle.g2_jac_to_int_point(oracle.msm_g2(B, s))
    assert got == p.g2_mul(p.G2_GENERATOR, synth.weighted_scalar_sum(s, 1))
