"""The code objects of the two MSM units after G2's reduction moved onto the plain path's kernels (aleo_amd/csrc/msm_reduce.h: k_tree_pass,
k_seg_tree_pass, k_gather_windows as templates over the point format), compiled here for gfx950: msm.hip holds the kernel set it held before, g2.hip its
accumulation, chunk, self-test, rows and unpack kernels plus its own instances of the three shared kernels — and none of the copies k_g2p_tree_pass,
k_g2p_seg_tree_pass, k_g2p_gather_windows; no kernel has more VGPRs or a larger private segment than it (or the copy it replaces) had before."""
import re
import pytest
import code_object as co

# (vgpr_count, private_segment_fixed_size) of every kernel of the two units BEFORE the fold, measured by compiling them with the flags of
# code_object.compile_unit (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S), under the names the kernels have now.  Three kernels of msm.hip became
# templates over a type (k_tree_pass<bool, LANES> -> <Pt28 | Pt32, LANES>; k_seg_tree_pass and k_gather_windows -> <Pt32>); the three G2 instances
# carry the figures of the copies they replace.
T = 'PcPKjjjS4_jjPK15HIP_vector_typeIjLj2EES8_jS4_jj'
PARENT = {
    'msm': {
        '_ZN11aleo_mi355x14k_gather_superEPKcPKjjPK15HIP_vector_typeIjLj2EES7_Pj': (8, 0),
        '_ZN11aleo_mi355x21k_bucket_chunks_plainEPKcPKjPK15HIP_vector_typeIjLj2EES7_jjjPc': (289, 800),
        '_ZN11aleo_mi355x15k_seg_tree_passINS_4Pt32EEEvPcjjj': (280, 240),
        '_ZN11aleo_mi355x12k_prog_pass2EPKcjS1_jS1_jjjjPcj': (173, 0),
        '_ZN11aleo_mi355x16k_gather_stridedEPKcjjPc': (8, 0),
        '_ZN11aleo_mi355x16k_gather_windowsINS_4Pt32EEEvPKcjjPc': (8, 0),
        '_ZN11aleo_mi355x17k_selftest_madd28EPjjm': (273, 0),
        '_ZN11aleo_mi355x18k_selftest_addquadEPcjmPj': (187, 0),
        '_ZN11aleo_mi355x9k_accum28ILb1ELb0EEEvPKcPKjS4_PK15HIP_vector_typeIjLj2EES8_S4_jS4_S4_S4_PcNS_10FrontChainE': (248, 736),
        '_ZN11aleo_mi355x9k_accum28ILb0ELb0EEEvPKcPKjS4_PK15HIP_vector_typeIjLj2EES8_S4_jS4_S4_S4_PcNS_10FrontChainE': (248, 736),
        '_ZN11aleo_mi355x9k_accum28ILb1ELb1EEEvPKcPKjS4_PK15HIP_vector_typeIjLj2EES8_S4_jS4_S4_S4_PcNS_10FrontChainE': (248, 736),
        '_ZN11aleo_mi355x11k_tree_passINS_4Pt28ELj4EEEv' + T: (161, 0),
        '_ZN11aleo_mi355x11k_tree_passINS_4Pt28ELj2EEEv' + T: (161, 0),
        '_ZN11aleo_mi355x11k_tree_passINS_4Pt32ELj2EEEv' + T: (280, 240),
        '_ZN11aleo_mi355x11k_tree_restILj4EEEvPcPKjjPK15HIP_vector_typeIjLj2EES7_jS3_': (175, 0),
        '_ZN11aleo_mi355x15k_bucket_chunksILb1ELj4EEEvPKcPKjPK15HIP_vector_typeIjLj2EES8_jjjPcjS9_NS_10FrontChainE': (185, 0),
        '_ZN11aleo_mi355x15k_bucket_chunksILb1ELj2EEEvPKcPKjPK15HIP_vector_typeIjLj2EES8_jjjPcjS9_NS_10FrontChainE': (181, 0),
        '_ZN11aleo_mi355x11k_prog_passILj4EEEvPKcjS2_jS2_jjjjPcj': (166, 0),
        '_ZN11aleo_mi355x11k_prog_passILj2EEEvPKcjS2_jS2_jjjjPcj': (166, 0),
        '_ZN11aleo_mi355x12k_prog_finalILj4EEEvPKcjjjjjPc': (181, 0),
        '_ZN11aleo_mi355x14k_masked_pairsILj4EEEvPKcjjPcj': (163, 0),
        '_ZN11aleo_mi355x14k_masked_pairsILj2EEEvPKcjjPcj': (163, 0),
        '_ZN11aleo_mi355x15k_seg_pair_passILj4EEEvPKcjjjPcj': (163, 0),
        '_ZN11aleo_mi355x15k_seg_pair_passILj2EEEvPKcjjjPcj': (163, 0),
        '_ZN11aleo_mi355x10k_seg_foldILj4EEEvPKcjjjPcj': (180, 0),
    },
    'g2': {
        '_ZN11aleo_mi355x12k_g2_accum28EPKcS1_PKjS3_PK15HIP_vector_typeIjLj2EES7_S3_jS3_S3_S3_Pc': (256, 4160),
        '_ZN11aleo_mi355x19k_g2p_bucket_chunksEPKcPKjPK15HIP_vector_typeIjLj2EES7_jjjPcS8_': (288, 420),
        '_ZN11aleo_mi355x11k_tree_passINS_4PtG2ELj2EEEv' + T: (288, 420),                     # was k_g2p_tree_pass
        '_ZN11aleo_mi355x15k_seg_tree_passINS_4PtG2EEEvPcjjj': (288, 420),                    # was k_g2p_seg_tree_pass
        '_ZN11aleo_mi355x14k_g2p_selftestEPKcjjPcPj': (288, 7152),
        '_ZN11aleo_mi355x14k_g2_rows_to28EPKcPcj': (84, 0),
        '_ZN11aleo_mi355x14k_g2_unpack200EPKcPcPhPjj': (54, 0),
        '_ZN11aleo_mi355x16k_gather_windowsINS_4PtG2EEEvPKcjjPc': (8, 0),                     # was k_g2p_gather_windows
    },
}


@pytest.fixture(scope='module')
def units():
    """unit -> {kernel name: metadata block}; each unit compiled once (compile_unit asserts the gfx950 target)"""
    out = {}
    for unit in PARENT:
        asm, blocks = co.compile_unit(unit)
        out[unit] = {re.search(r'\.name:\s*(\S+)', b).group(1): b for b in blocks}
        assert len(out[unit]) == len(blocks), unit
    return out


@pytest.mark.parametrize('unit', sorted(PARENT))
def test_the_unit_holds_exactly_its_kernels(units, unit):
    assert set(units[unit]) == set(PARENT[unit]), (sorted(set(PARENT[unit]) - set(units[unit])), sorted(set(units[unit]) - set(PARENT[unit])))


def test_g2_has_the_three_shared_kernels_and_none_of_its_copies(units):
    names = ' '.join(units['g2'])
    for gone in ('k_g2p_tree_pass', 'k_g2p_seg_tree_pass', 'k_g2p_gather_windows'):
        assert gone not in names, gone
    for shared in ('k_tree_pass', 'k_seg_tree_pass', 'k_gather_windows'):
        assert sum(shared + 'INS_4PtG2E' in k for k in units['g2']) == 1, shared
    for own in ('k_g2_accum28', 'k_g2p_bucket_chunks', 'k_g2p_selftest', 'k_g2_rows_to28', 'k_g2_unpack200'):
        assert sum(own in k for k in units['g2']) == 1, own


@pytest.mark.parametrize('unit', sorted(PARENT))
def test_no_kernel_needs_more_registers_or_private_memory_than_before(units, unit):
    for k, (vgprs, private) in PARENT[unit].items():
        print(co.registers('%s %s' % (unit, k), units[unit][k]))
        assert co.field(units[unit][k], 'vgpr_count') <= vgprs, (k, co.field(units[unit][k], 'vgpr_count'), vgprs)
        assert co.field(units[unit][k], 'private_segment_fixed_size') <= private, (k, co.field(units[unit][k], 'private_segment_fixed_size'), private)
