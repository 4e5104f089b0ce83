"""What the tests of the batched units (accounts, signatures, private key ciphertexts, the record flows) share: where the sources lie, the byte helpers, the build
and run of a lane-emulation program of tests/cpp, the reads of a routing threshold, the run of a C++ mirror, the figures of a unit's code object that say
"no scratch, no spills", and two threads calling at once.  A plain module: what a test asserts about any of these stays in the test."""
import ctypes, os, subprocess, sys, threading
import code_object as co
from code_object import ROOT, CSRC, HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']      # host code only: a program of its own, never a GPU build


def le32(v) -> bytes: return int(v).to_bytes(32, 'little')
def num(b: bytes) -> int: return int.from_bytes(b, 'little')
def _vp(b: bytes): return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
def _p(a): return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def build_lane_emul(tmp_path, name, sanitized=False, opt=None, flags=('-fno-strict-aliasing',), hipcc=False):
    """tests/cpp/<name>.cpp built into tmp_path — by g++, or by hipcc as plain C++; at `opt`, or -O1 with the address and undefined-behaviour sanitizers compiled in
    and -O2 without; with `flags`: the program's path."""
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(([HIPCC, '-x', 'c++'] if hipcc else ['g++']) + ['-std=c++17', opt or ('-O1' if sanitized else '-O2')] + list(flags) + ['-mbmi2', '-madx']
                          + (SANITIZE if sanitized else []) + ['-I', CSRC, os.path.join(HERE, 'cpp', name + '.cpp'), '-o', exe])
    return exe


def run_lane_emul(tmp_path, name, args=(), **how):
    """That program built (`how`: build_lane_emul's) and run as a program of its own on `args` (its case file, as a rule): the completed process."""
    return subprocess.run([build_lane_emul(tmp_path, name, **how)] + [str(a) for a in args], capture_output=True, text=True, timeout=900)


def threshold_reads(getter, variable, values=('5', 'x')):
    """What aleo_mi355x_<getter>() returns in a fresh process with `variable` unset and with each of `values`: unset, '5' and 'x' give three numbers."""
    code = 'import aleo_amd; print(int(aleo_amd.lib().aleo_mi355x_%s()))' % getter
    def run(extra):
        env = dict(os.environ, PYTHONPATH=ROOT); env.pop(variable, None); env.update(extra)
        return int(subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout)
    return (run({}),) + tuple(run({variable: v}) for v in values)


def run_cpp_mirror(tmp_path, program, args, env):
    """tests/cpp/<program>.cpp over include/aleo_mi355x.hpp (test_abi.build_cpp_host_mirror), run on `args` with `env` added to the environment: the completed process."""
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, program)
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def scratch_and_spills(unit, kernels):
    """The code object of aleo_amd/csrc/<unit>.hip: how many kernels it holds, and {kernel: (private segment, VGPR spills, SGPR spills)} of the named ones, whose
    register figures are printed."""
    asm, blocks = co.compile_unit(unit)
    out = {}
    for kernel in kernels:
        b = co.block_of(blocks, kernel)
        print(co.registers(kernel, b))
        out[kernel] = tuple(co.field(b, f) for f in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count'))
    return len(blocks), out


def two_threads(call, rounds=3):
    """call(0) and call(1) on two threads at once, `rounds` times each: the last result of either."""
    got = [None, None]
    def work(i):
        for _ in range(rounds): got[i] = call(i)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    return got
