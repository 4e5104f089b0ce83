"""The host's group law (aleo_amd/csrc/xyzz_law.h: one XYZZ law over HFq for G1 and HFq2 for G2) without a GPU and without the library: the program
tests/cpp/host_group_test.cpp is built by g++ alone, once plain and once with the address and undefined-behaviour sanitizers compiled in, and run as a
program of its own on a case file written from oracle/pyref.py; every point it writes is compared byte for byte with pyref's."""
import os, struct, subprocess
import pytest
from oracle import pyref as p

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'aleo_amd', 'csrc')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']      # host code only: a program of its own, never a GPU build
Q = p.FQ_MODULUS
# a dozen scalars below 2^64: 0, 1, 2, two equal ones, the top bit, all ones
SCALARS = [0, 1, 2, 3, 8, 0xDEADBEEF, 0xDEADBEEF, 0x123456789ABCDEF, 1 << 63, (1 << 64) - 1, 0x8000000000000001, 377]


def fq_bytes(v):                                   # host Montgomery form, 48 bytes little-endian
    return (v * p.FQ_R % Q).to_bytes(48, 'little')


def jac(point, comps):
    """the normalised Jacobian bytes the host writes: (x, y, 1), or (1, 1, 0) for the identity; comps = 1 (Fq) or 2 (Fq2: c0 | c1)"""
    flat = (lambda e: [e]) if comps == 1 else (lambda e: list(e))
    one, zero = [1] + [0] * (comps - 1), [0] * comps
    coords = one + one + zero if point is None else flat(point[0]) + flat(point[1]) + one
    return b''.join(fq_bytes(v) for v in coords)


def row28(point, comps, loose):
    """X | Y | ZZ | ZZZ of the affine point (ZZ = ZZZ = 1) in the 28-bit form: value * 2^392 mod q as 14 limbs of 28 bits in 32-bit words; loose: q added
    to every component limb by limb, without carries (limbs up to 2^29: the same residue)"""
    flat = (lambda e: [e]) if comps == 1 else (lambda e: list(e))
    one = [1] + [0] * (comps - 1)
    out = b''
    for v in flat(point[0]) + flat(point[1]) + one + one:
        m = v * (1 << 392) % Q
        limbs = [(m >> (28 * i)) & 0xFFFFFFF for i in range(14)]
        if loose:
            limbs = [l + ((Q >> (28 * i)) & 0xFFFFFFF) for i, l in enumerate(limbs)]
        out += struct.pack('<14I', *limbs)
    return out


GROUPS = (('G1', 1, p.G1_GENERATOR, p.g1_mul, p.g1_add, p.g1_neg), ('G2', 2, p.G2_GENERATOR, p.g2_mul, p.g2_add, p.g2_neg))


@pytest.fixture(scope='module')
def case_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('host_group') / 'cases.bin')
    with open(path, 'wb') as f:
        for _, comps, gen, mul, _, _ in GROUPS:
            for k in range(1, 9):
                f.write(jac(mul(gen, k), comps))
        f.write(struct.pack('<Q', len(SCALARS)) + struct.pack('<%dQ' % len(SCALARS), *SCALARS))
        for _, comps, gen, mul, _, _ in GROUPS:
            f.write(row28(mul(gen, 3), comps, False) + row28(mul(gen, 3), comps, True))
    return path


@pytest.mark.parametrize('sanitized', [False, True], ids=['plain', 'asan_ubsan'])
def test_host_group_law_matches_pyref_for_g1_and_g2(case_file, tmp_path, sanitized):
    exe, out = str(tmp_path / 'host_group_test'), str(tmp_path / 'out.bin')
    subprocess.check_call(['g++', '-std=c++17', '-O1' if sanitized else '-O2', '-fno-strict-aliasing', '-mbmi2', '-madx', '-Wall'] + (SANITIZE if sanitized else [])
                          + ['-I', CSRC, os.path.join(HERE, 'cpp', 'host_group_test.cpp'), '-o', exe])
    subprocess.run([exe, case_file, out], check=True, timeout=120)       # its own process: the sanitizers' reports end it with a non-zero status
    data = open(out, 'rb').read()
    per = len(SCALARS) + 8
    assert len(data) == per * (144 + 288)
    pos = 0
    for name, comps, gen, mul, add, neg in GROUPS:
        J = 144 * comps
        pts = [data[pos + J * i: pos + J * (i + 1)] for i in range(per)]
        pos += J * per
        for k, got in zip(SCALARS, pts):
            assert got == jac(mul(gen, k), comps), (name, k)                 # k * G by double-and-add, read through from-Jacobian, written normalised
        lhs, rhs, p_plus_p, two_p, cancel, id_plus_p, tight, loose = pts[len(SCALARS):]
        P, Qp, R = mul(gen, 1), mul(gen, 2), mul(gen, 5)
        assert lhs == rhs == jac(add(add(P, Qp), R), comps) == jac(mul(gen, 8), comps), name      # (P + Q) + R = P + (Q + R)
        assert p_plus_p == two_p == jac(mul(gen, 2), comps), name                                  # P + P = 2P
        assert add(P, neg(P)) is None and cancel == jac(None, comps), name                         # P + (-P) = the identity, written (1, 1, 0)
        assert cancel[:48 * comps] == cancel[48 * comps: 96 * comps] == fq_bytes(1) + bytes(48 * (comps - 1)) and cancel[96 * comps:] == bytes(48 * comps)
        assert id_plus_p == jac(P, comps), name                                                    # identity + P = P
        assert tight == loose == jac(mul(gen, 3), comps), name                                     # from28: a value and the value + q in loose limbs
