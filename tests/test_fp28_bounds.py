"""The limb and value bounds of the 28-bit-limb point formulas (aleo_amd/csrc/fp28.h), checked mechanically on the host.

tests/cpp/fp28_bounds_emul.cpp (on tests/cpp/checked_f28.h) defines ALEO_F28_PROVIDED, supplies the primitives of the header's guarded block over limbs
that carry their bounds along, and includes the header: the shipped source of xyzz28_madd_fast, xyzz28_double_both, xyzz28_add_pair and xyzz28_add_quad then runs on the
host, every "class Lk", "< k q" and column claim turned into a check against the bounds, every result compared with the affine group law in HFq.
The negative controls patch a copy of the header and expect the checker to fire: a checker that never fires proves nothing.
"""
import os, re, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join(ROOT, 'aleo_amd', 'csrc')
EMUL = os.path.join(ROOT, 'tests', 'cpp', 'fp28_bounds_emul.cpp')

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')


def build_and_run(tmp_path, header=None):
    exe = os.path.join(str(tmp_path), 'fp28_bounds_emul')
    cmd = [HIPCC, '-x', 'c++', '-std=c++17', '-O2', '-mbmi2', '-madx', '-pthread', '-I', CSRC]
    if header:
        cmd.append('-DFP28_HEADER="%s"' % header)
    subprocess.check_call(cmd + [EMUL, '-o', exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def counts(line_start, out):
    line = next(l for l in out.splitlines() if l.startswith(line_start))
    return {k: int(v) for k, v in re.findall(r'(\w+) (\d+)', line[len(line_start):])}


def test_formulas_keep_their_bounds_and_match_the_group_law(tmp_path):
    r = build_and_run(tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    calls = counts('calls: ', r.stdout)
    assert all(calls[f] > 0 for f in ('madd', 'double', 'pair', 'quad')), calls
    branches = counts('branches: ', r.stdout)
    assert all(v > 0 for v in branches.values()) and len(branches) == 7, branches
    assert r.stdout.count('slack xyzz28_') == 4


# (what, the text in fp28.h, its replacement, the kinds of rule of which at least one must fire)
MUTATIONS = [
    ('the normalise around X3 in xyzz28_add_pair dropped: X3 is stored and subtracted with loose limbs',
     'F28 X3 = f28_normalise(f28_sub<6, 2>(f28_sub<4, 1>(RR, PPP), f28_add(Q, Q)));  // < 12q, exact digits\n',
     'F28 X3 = f28_sub<6, 2>(f28_sub<4, 1>(RR, PPP), f28_add(Q, Q));\n', ('closure',)),
    ('R of xyzz28_madd_fast with a one-unit spread: the first point\'s L2 negation has limbs up to 2^29 - 2',
     'F28 R = f28_sub<4, 2>(S2, acc.Y);', 'F28 R = f28_sub<4, 1>(S2, acc.Y);', ('limb',)),
    ('Q - X3 of xyzz28_add_quad padded with 8q: X3 goes up to 12q',
     'f28_sub<16, 1>(Q, X3));   // q0: Q - X3 (L3)', 'f28_sub<8, 1>(Q, X3));   // q0: Q - X3 (L3)', ('value',)),
    # none of the three above can break a column (they make operands smaller or leave them alone), so a fourth does: R in class L6, squared
    ('R of xyzz28_madd_fast padded with 8q spread by four units: class L6, whose square needs 7 * 2 * 36 + 14 = 518 of a column\'s 256',
     'F28 R = f28_sub<4, 2>(S2, acc.Y);', 'F28 R = f28_sub<8, 4>(S2, acc.Y);', ('column',)),
]


@pytest.mark.parametrize('what,old,new,kinds', MUTATIONS, ids=['pair_x3_not_normalised', 'madd_r_spread_1', 'quad_q_minus_x3_pad_8q', 'madd_r_class_l6'])
def test_a_broken_bound_is_reported(tmp_path, what, old, new, kinds):
    src = open(os.path.join(CSRC, 'fp28.h')).read()
    assert src.count(old) == 1, 'the text of the mutation must match fp28.h exactly once'
    patched = os.path.join(str(tmp_path), 'fp28_patched.h')
    with open(patched, 'w') as f:
        f.write(src.replace(old, new))
    r = build_and_run(tmp_path, patched)
    print(r.stdout, r.stderr)
    v = counts('violations: ', r.stdout)
    total = int(re.search(r'(\d+) limb-rule violations', r.stdout).group(1)) + int(re.search(r'(\d+) mismatches', r.stdout).group(1))
    assert r.returncode == 1 and total > 0, what
    assert any(v[k] > 0 for k in kinds), (what, v)
