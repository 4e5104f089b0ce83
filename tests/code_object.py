"""What the code-object tests of the kernel units share: a unit of aleo_amd/csrc compiled to gfx950 assembly with the flags of the library's device
code, the target it names, and the metadata block of every kernel in it.  What a test asserts about its kernels stays in the test."""
import os, re, subprocess, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'aleo_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
REGISTERS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size')


def compile_unit(unit):
    """(asm, blocks) of aleo_amd/csrc/<unit>.hip: the device assembly, which names gfx950 as its target, and one metadata block per kernel."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + '.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S', '-I' + CSRC, '-I' + os.path.join(ROOT, 'include'),
                        os.path.join(CSRC, unit + '.hip'), '-o', out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    assert '.amdgcn_target "amdgcn-amd-amdhsa--gfx950"' in asm
    return asm, re.findall(r'- \.agpr_count:.*?\.wavefront_size:\s*\d+', asm, flags=re.S)


def field(block, name):
    return int(re.search(r'\.%s:\s*(\d+)' % name, block).group(1))


def block_of(blocks, kernel):
    """the one block whose kernel's name contains `kernel`"""
    mine = [b for b in blocks if kernel in b]
    assert len(mine) == 1, '%s is not in the code object' % kernel
    return mine[0]


def registers(label, block, names=REGISTERS):
    """the line a test prints: 'label: name value, name value, ...'"""
    return '%s: %s' % (label, ', '.join('%s %d' % (n, field(block, n)) for n in names))
