"""The limb and value bounds of the Edwards-form point formulas (aleo_amd/csrc/te28.h), checked mechanically on the host.

tests/cpp/te28_bounds_emul.cpp takes the harness that tests/cpp/fp28_bounds_emul.cpp uses, tests/cpp/checked_f28.h (limbs that carry their bounds, a value bound in multiples of q,
an exact-digits flag, lanes as host threads), adds the stored invariant of an Edwards point and includes te28.h: the shipped source of te28_madd (in its two halves),
te28_first, te28_row_negate_if, te28_add_pair and te28_add_quad then runs on the host, every "class Lk", "< k q" and column claim turned into a check
against the bounds, every result compared with the affine group law carried through the map of tools/te28_model.py.  The negative controls patch a copy
of the header and expect the checker to fire.  The same program is also built with the address and undefined-behaviour sanitizers: it has its own main,
nothing is preloaded.
"""
import os, re, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join(ROOT, 'aleo_amd', 'csrc')
EMUL = os.path.join(ROOT, 'tests', 'cpp', 'te28_bounds_emul.cpp')
FORMULAS = ('te28_madd_rows', 'te28_madd_finish', 'te28_first', 'te28_row_negate_if', 'te28_add_pair', 'te28_add_quad')

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')


def build_and_run(tmp_path, header=None, extra=()):
    exe = os.path.join(str(tmp_path), 'te28_bounds_emul')
    cmd = [HIPCC, '-x', 'c++', '-std=c++17', '-O2', '-mbmi2', '-madx', '-pthread', '-I', CSRC, *extra]
    if header:
        cmd.append('-DTE28_HEADER="%s"' % header)
    subprocess.check_call(cmd + [EMUL, '-o', exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def counts(line_start, out):
    line = next(l for l in out.splitlines() if l.startswith(line_start))
    return {k: int(v) for k, v in re.findall(r'(\w+) (\d+)', line[len(line_start):])}


def check_clean(r):
    print(r.stdout)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    calls = counts('calls: ', r.stdout)
    assert all(calls[f] > 0 for f in ('madd', 'first', 'pair', 'quad')), calls
    branches = counts('branches: ', r.stdout)
    assert branches['z3_zero'] > 0 and branches['identity_results'] > 0, branches      # the exceptional pairs were reported, the identity came out as a point
    assert all(r.stdout.count('slack %s:' % f) == 1 for f in FORMULAS)


def test_formulas_keep_their_bounds_and_match_the_group_law(tmp_path):
    check_clean(build_and_run(tmp_path))


def test_the_same_program_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    r = build_and_run(tmp_path, extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'))
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    check_clean(r)


# (what, the text in te28.h, its replacement, the kinds of rule of which at least one must fire)
MUTATIONS = [
    ('F of te28_madd padded with q alone: a product is only known to be below (1 + eps) q, the top limb of the difference can go negative',
     'const F28 F = f28_sub<4, 1>(D, C);                               // D + 4q - C < 8q, class L4',
     'const F28 F = f28_sub<1, 1>(D, C);', ('value',)),
    ('the product that brings the first point\'s X back under the invariant replaced by a normalise: X is kept below 3q, not 2q',
     'acc.X = f28_mul(f28_sub<2, 1>(r1, r0), te28_const(TE_ONE_28));', 'acc.X = f28_normalise(f28_sub<2, 1>(r1, r0));', ('closure',)),
    ('F of te28_add_quad padded with 16q spread by four units: class L7, whose product with itself needs 14 * 49 + 14 = 700 of a column\'s 256',
     'const F28 F = f28_sub<4, 1>(D, C), G = f28_add(D, C);                       // < 8q, class L4; < 6q, class L3 (every lane)',
     'const F28 F = f28_sub<16, 4>(D, C), G = f28_add(D, C);', ('column',)),
    ('E of te28_add_pair subtracting the loose m1 (class L3, < 6q) instead of the exact A: a one-unit spread padded with 4q covers neither its limbs nor its value',
     'const F28 E = f28_sub<4, 1>(B, A), H = f28_add(B, A);                       // < 6q, class L3; < 4q, class L2\n',
     'const F28 E = f28_sub<4, 1>(B, m1), H = f28_add(B, A);\n', ('limb', 'value')),
]


@pytest.mark.parametrize('what,old,new,kinds', MUTATIONS, ids=['madd_f_pad_q', 'first_x_not_reduced', 'quad_f_class_l7', 'pair_e_loose_subtrahend'])
def test_a_broken_bound_is_reported(tmp_path, what, old, new, kinds):
    src = open(os.path.join(CSRC, 'te28.h')).read()
    assert src.count(old) == 1, 'the text of the mutation must match te28.h exactly once'
    patched = os.path.join(str(tmp_path), 'te28_patched.h')
    with open(patched, 'w') as f:
        f.write(src.replace(old, new))
    r = build_and_run(tmp_path, patched)
    print(r.stdout, r.stderr)
    v = counts('violations: ', r.stdout)
    total = int(re.search(r'(\d+) limb-rule violations', r.stdout).group(1)) + int(re.search(r'(\d+) mismatches', r.stdout).group(1))
    assert r.returncode == 1 and total > 0, what
    assert any(v[k] > 0 for k in kinds), (what, v)
