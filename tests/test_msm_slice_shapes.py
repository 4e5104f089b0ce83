"""End-to-end MSMs at the sizes where the slice stage changes shape: the c = 13 tier of a pinned set (4096 buckets = two scan tiles), prefixes that end inside
and on a tile of slices, scalar sets that leave one bucket, two neighbouring buckets across the scan-tile boundary, or none at all non-empty.  Bit-exact against
sum_i s_i * (i + 1) * G in big integers (the bases are the multiples 1, 2, .. of the generator)."""
import numpy as np
import pytest
import aleo_amd
from aleo_amd import synth

N_PIN = (1 << 15) + 64
PREFIXES = [1024, 2049, 1 << 15]


def _const(n, v):
    s = np.zeros((n, 4), dtype=np.uint64); s[:, 0] = v; return s
def _two_values(n):
    s = np.zeros((n, 4), dtype=np.uint64); s[:, 0] = 2048 + (np.arange(n) % 3 == 0); return s


SCALARS = {
    'uniform': lambda n: synth.uniform_scalars(n, 0x51CE0001),
    'all_one': lambda n: _const(n, 1),
    'only_2048_2049': _two_values,
    'all_zero': lambda n: _const(n, 0),
    'witness_like': lambda n: synth.witness_like_scalars(n, 0x51CE0002),
}


@pytest.fixture(scope='module')
def pinned():
    with aleo_amd.PinnedBases.generate_multiples(synth.generator_affine104(), 1, N_PIN) as pb:
        pb.precompute()
        yield pb


def _expected(oracle, scalars):
    from oracle import pyref as p
    k = sum(synth.limbs_to_int(row) * (i + 1) for i, row in enumerate(scalars)) % synth.FR_MODULUS
    return p.g1_mul(p.G1_GENERATOR, k) if k else None


@pytest.mark.gpu
@pytest.mark.parametrize('n', PREFIXES)
@pytest.mark.parametrize('kind', sorted(SCALARS))
def test_msm_prefix_bit_exact(pinned, oracle, kind, n):
    s = SCALARS[kind](n)
    got = aleo_amd.VariableBase.msm(pinned, s)
    assert oracle.jac_to_int_point(got) == _expected(oracle, s)


@pytest.mark.gpu
def test_msm_two_results_in_one_chain(pinned, oracle):
    """Two scalar vectors against the same set in one launch chain: 2 x 4096 buckets, one slice stage."""
    import torch
    n = 1 << 15
    vs = [SCALARS['uniform'](n), SCALARS['witness_like'](n)]
    d = [torch.from_numpy(v.view(np.int64).copy()).cuda() for v in vs]
    torch.cuda.synchronize()
    got = aleo_amd.VariableBase.msm_batch_device(pinned, [t.data_ptr() for t in d], [n, n])
    for q in range(2):
        assert oracle.jac_to_int_point(got[q]) == _expected(oracle, vs[q])
