"""The code object of the transform's unit (aleo_amd/csrc/ntt.hip), compiled here for gfx950: which pass kernels it holds and what they cost in registers.
One kernel pair serves both limb forms; an instance that appears or disappears, a spill, or a form that grows past the registers its hand-copied
predecessor needed shows here before any GPU run."""
import re
import code_object as co

# VGPRs of the six pass kernels when each limb form still had kernels of its own: (kernel, limb form, tile elements) -> vgpr_count
PARENT_VGPRS = {('final', 'Limbs32', 512): 78, ('strided', 'Limbs32', 512): 62,
                ('strided', 'Limbs29', 4096): 191, ('final', 'Limbs29', 4096): 191,
                ('strided', 'Limbs29', 2048): 159, ('final', 'Limbs29', 2048): 159}


def test_ntt_unit_holds_six_pass_kernels_without_scratch_within_the_parents_registers():
    asm, blocks = co.compile_unit('ntt')                        # asserts the gfx950 target
    assert blocks
    passes = {}
    for b in blocks:
        name = re.search(r'\.name:\s*(\S+)', b).group(1)
        print(co.registers(name, b))
        assert co.field(b, 'private_segment_fixed_size') == 0, name
        m = re.search(r'k_ntt_(strided|final)INS_\d+(Limbs\d+)ELj(\d+)E', name)
        if m:
            key = (m.group(1), m.group(2), int(m.group(3)))
            assert key not in passes, name
            passes[key] = co.field(b, 'vgpr_count')
        else:
            assert 'k_ntt' not in name, name                    # a pass kernel this test cannot place
    assert set(passes) == set(PARENT_VGPRS), sorted(passes)     # exactly the six
    for key, vgprs in passes.items():
        assert vgprs <= PARENT_VGPRS[key], (key, vgprs, PARENT_VGPRS[key])
