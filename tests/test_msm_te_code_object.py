"""The code object of the Edwards tier's unit (aleo_amd/csrc/msm_te.hip), compiled here for gfx950: the accumulation kernel holds ONE table row per lane, so both
its instantiations must fit 256 VGPRs with no private segment at all (the XYZZ kernel it stands in for has 248 and 736 bytes), and none of the reduction's
kernels may spill either.  What the kernels of msm.hip need is pinned by tests/test_g2_code_object.py."""
import re
import pytest
import code_object as co


@pytest.fixture(scope='module')
def kernels():
    asm, blocks = co.compile_unit('msm_te')
    return {re.search(r'\.name:\s*(\S+)', b).group(1): b for b in blocks}


def test_accumulation_fits_the_register_file_without_scratch(kernels):
    acc = {k: b for k, b in kernels.items() if 'k_accum28_te' in k}
    assert len(acc) == 2, sorted(acc)                                     # seeded and unseeded
    for k, b in acc.items():
        print(co.registers(k, b))
        assert co.field(b, 'vgpr_count') <= 256 and co.field(b, 'private_segment_fixed_size') == 0, k
        assert co.field(b, 'vgpr_count') <= 168, (k, 'three waves per SIMD need at most 168 VGPRs')


def test_the_unit_holds_the_edwards_kernels_and_none_spills(kernels):
    for name in ('k_accum28_te', 'k_tree_pass', 'k_tree_rest_te', 'k_gather_super_te', 'k_bucket_chunks_te', 'k_prog_pass_te', 'k_prog_pass2_te', 'k_prog_final_te'):
        assert any(name in k for k in kernels), name
    for k, b in kernels.items():
        assert co.field(b, 'private_segment_fixed_size') == 0, k
