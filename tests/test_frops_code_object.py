"""The code objects of the Fr kernel units (aleo_amd/csrc/frops.hip, fr_spmv.hip, fr_divide.hip, ahp_kernels.hip, and the key-synthesis kernels of
varuna_index.hip), compiled here for gfx950: together they hold the kernels the one unit frops.hip held before it was split by job, less the three
single-polynomial division kernels (one division runs the job-array kernels with one job), each kernel in exactly one unit and none of them with more
VGPRs or a larger private segment than it had there."""
import re
import pytest
import code_object as co

# (vgpr_count, private_segment_fixed_size) of every kernel of the unsplit frops.hip, measured by compiling that file with the flags of
# code_object.compile_unit (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S).  The three kernels with a private segment call a __noinline__
# helper (fr_inverse_ni / fr_pow_u64_ni), whose operands pass through memory.
PARENT = {
    '_ZN11aleo_mi355x20k_ahp_first_sumcheckEPcmPKcS2_S2_S2_S2_NS_3FrKES3_': (95, 0),
    '_ZN11aleo_mi355x21k_ahp_matrix_sumcheckEPcmNS_7MatArgsE': (87, 0),
    '_ZN11aleo_mi355x12k_blind_rowsEPcPKcmjNS_9BlindArgsE': (36, 0),
    '_ZN11aleo_mi355x12k_div_blocksEPKcmNS_3FrKEPc': (56, 0),
    '_ZN11aleo_mi355x17k_div_blocks_manyENS_7DivJobsE': (56, 0),
    '_ZN11aleo_mi355x13k_div_carriesEPKcjjNS_3FrKEPc': (60, 0),
    '_ZN11aleo_mi355x18k_div_carries_manyENS_7DivJobsE': (60, 0),
    '_ZN11aleo_mi355x12k_div_finishEPKcmNS_3FrKES1_PcS3_': (72, 0),
    '_ZN11aleo_mi355x17k_div_finish_manyENS_7DivJobsE': (72, 0),
    '_ZN11aleo_mi355x13k_eval_blocksENS_8EvalArgsEPc': (56, 0),
    '_ZN11aleo_mi355x14k_eval_combineENS_8EvalArgsEPKcPc': (65, 48),
    '_ZN11aleo_mi355x8k_fp_mulINS_2FpINS_8FqParamsEEELb0EEEvPcPKcS6_j': (78, 0),
    '_ZN11aleo_mi355x8k_fp_mulINS_2FpINS_8FqParamsEEELb1EEEvPcPKcS6_j': (98, 0),
    '_ZN11aleo_mi355x8k_fp_mulINS_2FpINS_8FrParamsEEELb0EEEvPcPKcS6_j': (59, 0),
    '_ZN11aleo_mi355x8k_fp_mulINS_2FpINS_8FrParamsEEELb1EEEvPcPKcS6_j': (64, 0),
    '_ZN11aleo_mi355x14k_fr_add_tiledEPcmPKcm': (30, 0),
    '_ZN11aleo_mi355x18k_fr_batch_inverseEPcS0_mm': (80, 96),
    '_ZN11aleo_mi355x16k_fr_gather_mul3ENS_10GatherMul3EPKcS2_': (72, 0),
    '_ZN11aleo_mi355x15k_fr_gather_mulILb0ELb0EEEvPcmPKcS3_PKjS3_S5_': (46, 0),
    '_ZN11aleo_mi355x15k_fr_gather_mulILb0ELb1EEEvPcmPKcS3_PKjS3_S5_': (64, 0),
    '_ZN11aleo_mi355x15k_fr_gather_mulILb1ELb0EEEvPcmPKcS3_PKjS3_S5_': (64, 0),
    '_ZN11aleo_mi355x15k_fr_gather_mulILb1ELb1EEEvPcmPKcS3_PKjS3_S5_': (72, 0),
    '_ZN11aleo_mi355x8k_fr_linILb0ELb0EEEvPcmNS_3FrKES2_PKcS2_S4_': (36, 0),
    '_ZN11aleo_mi355x8k_fr_linILb0ELb1EEEvPcmNS_3FrKES2_PKcS2_S4_': (77, 0),
    '_ZN11aleo_mi355x8k_fr_linILb1ELb0EEEvPcmNS_3FrKES2_PKcS2_S4_': (77, 0),
    '_ZN11aleo_mi355x8k_fr_linILb1ELb1EEEvPcmNS_3FrKES2_PKcS2_S4_': (79, 0),
    '_ZN11aleo_mi355x12k_fr_lincombEPcmNS_6LcArgsENS_3FrKE': (62, 0),
    '_ZN11aleo_mi355x9k_fr_pickEPcNS_8PickArgsEj': (6, 0),
    '_ZN11aleo_mi355x11k_fr_powersEPcmNS_3FrKES1_': (65, 48),
    '_ZN11aleo_mi355x16k_fr_powers_fastEPcjNS_3FrKES1_NS_4FrSqE': (60, 0),
    '_ZN11aleo_mi355x11k_fr_randomEPcmNS_6Seed32Emi': (60, 0),
    '_ZN11aleo_mi355x15k_fr_scale_rowsEPcPKcmjNS_4FrK4E': (62, 0),
    '_ZN11aleo_mi355x12k_fr_sub_mulEPcPKcS2_S2_m': (46, 0),
    '_ZN11aleo_mi355x11k_fr_vec_opILi0EEEvPcPKcS3_m': (46, 0),
    '_ZN11aleo_mi355x11k_fr_vec_opILi1EEEvPcPKcS3_m': (32, 0),
    '_ZN11aleo_mi355x11k_fr_vec_opILi2EEEvPcPKcS3_m': (32, 0),
    '_ZN11aleo_mi355x19k_index_expand_rowsEPKjS1_S1_jPjS2_S2_S2_': (16, 0),
    '_ZN11aleo_mi355x22k_index_scan_inclusiveEPjj': (30, 0),
    '_ZN11aleo_mi355x22k_index_transpose_rowsEPKjS1_PK15HIP_vector_typeIjLj4EEjjPjS6_PS3_': (22, 0),
    '_ZN11aleo_mi355x17k_scatter_to_montEPcPKcPKjmPj': (61, 0),
    '_ZN11aleo_mi355x16k_split_quotientEPKcS1_mPcS2_S2_': (80, 0),
    '_ZN11aleo_mi355x16k_spmv_huge_foldEPcPKjS2_PKc': (41, 0),
    '_ZN11aleo_mi355x19k_spmv_huge_partialEPKjS1_PKcS3_S1_S1_Pc': (56, 0),
    '_ZN11aleo_mi355x11k_spmv_longEPcPKjS2_PKcS4_S2_S2_': (66, 0),
    '_ZN11aleo_mi355x11k_spmv_rowsEPcPKjS2_PKcS4_jPjS5_S5_': (68, 0),
    '_ZN11aleo_mi355x19k_sumcheck_operandsEPcPKcS2_mmmj': (48, 0),
}
FOLDED_AWAY = {'_ZN11aleo_mi355x12k_div_blocksEPKcmNS_3FrKEPc', '_ZN11aleo_mi355x13k_div_carriesEPKcjjNS_3FrKEPc', '_ZN11aleo_mi355x12k_div_finishEPKcmNS_3FrKES1_PcS3_'}
FR_UNITS = ('frops', 'fr_spmv', 'fr_divide', 'ahp_kernels')


@pytest.fixture(scope='module')
def units():
    """unit -> {kernel name: metadata block}; every unit compiled once (compile_unit asserts the gfx950 target)"""
    out = {}
    for unit in FR_UNITS + ('varuna_index',):
        asm, blocks = co.compile_unit(unit)
        out[unit] = {re.search(r'\.name:\s*(\S+)', b).group(1): b for b in blocks}
        assert len(out[unit]) == len(blocks), unit
    return out


def placed(units):
    """(unit, kernel) of every kernel this test is about: all of the four Fr units, the k_index_* kernels of varuna_index"""
    return [(u, k) for u in FR_UNITS for k in units[u]] + [('varuna_index', k) for k in units['varuna_index'] if 'k_index_' in k]


def test_the_four_fr_units_compile_for_gfx950_and_hold_kernels(units):
    for u in FR_UNITS:
        assert units[u], u


def test_the_units_hold_the_parents_kernels_less_the_single_division_each_once(units):
    names = [k for _, k in placed(units)]
    assert len(names) == len(set(names)), sorted(k for k in set(names) if names.count(k) > 1)      # none in two units
    want = set(PARENT) - FOLDED_AWAY
    assert FOLDED_AWAY <= set(PARENT) and len(want) == len(PARENT) - 3
    assert set(names) == want, (sorted(want - set(names)), sorted(set(names) - want))               # none missing, none extra
    assert sorted(k for k in units['varuna_index'] if 'k_index_' in k) == sorted(k for k in PARENT if 'k_index_' in k)


def test_no_kernel_needs_more_registers_or_private_memory_than_in_the_parent(units):
    for u, k in placed(units):
        print(co.registers('%s %s' % (u, k), units[u][k]))
        vgprs, private = PARENT[k]
        assert co.field(units[u][k], 'vgpr_count') <= vgprs, (k, co.field(units[u][k], 'vgpr_count'), vgprs)
        assert co.field(units[u][k], 'private_segment_fixed_size') <= private, (k, co.field(units[u][k], 'private_segment_fixed_size'), private)
