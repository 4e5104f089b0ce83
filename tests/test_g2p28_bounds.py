"""The limb and value bounds of the G2 lane-pair formulas (aleo_amd/csrc/g2p28.h), checked mechanically on the host.

tests/cpp/g2p28_bounds_emul.cpp takes the harness of tests/cpp/checked_f28.h (limbs that carry their bounds, a value bound in multiples of q, an
exact-digits flag, the two lanes of a pair as host threads) and includes g2p28.h: the shipped source of g2p_madd_fast, g2p_double, g2p_add, g2p_add_any
and g2p_double_any then runs on the host with its operands tagged with the full stated invariant (X exact < 12q, Y exact < 6q, ZZ / ZZZ exact < 2q,
entries exact < 2q, the negated entry as the code makes it), every "< k q", "limbs < k * 2^28" and column claim turned into a check against the bounds,
every result compared with the affine group law over HFq2.  The negative controls patch a copy of the header and expect the checker to fire: one per
kind of rule.  The same program is also built with the address and undefined-behaviour sanitizers: it has its own main, nothing is preloaded.
"""
import os, re, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join(ROOT, 'aleo_amd', 'csrc')
EMUL = os.path.join(ROOT, 'tests', 'cpp', 'g2p28_bounds_emul.cpp')
FORMULAS = ('g2p_madd_fast', 'g2p_double', 'g2p_add', 'g2p_add_any', 'g2p_double_any', 'g2p_negate_entry')
BRANCHES = ('madd_refused', 'madd_zz3_one_component_zero', 'negated_zero_entry', 'add_zz3_one_component_zero', 'identity_left', 'identity_right', 'same_doubled',
            'opposite_to_identity', 'same_two_torsion', 'double_identity', 'double_two_torsion')

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')


def build_and_run(tmp_path, header=None, extra=()):
    exe = os.path.join(str(tmp_path), 'g2p28_bounds_emul')
    cmd = [HIPCC, '-x', 'c++', '-std=c++17', '-O2', '-mbmi2', '-madx', '-pthread', '-I', CSRC, *extra]
    if header:
        cmd.append('-DG2P28_HEADER="%s"' % header)
    subprocess.check_call(cmd + [EMUL, '-o', exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def counts(line_start, out):
    line = next(l for l in out.splitlines() if l.startswith(line_start))
    return {k: int(v) for k, v in re.findall(r'(\w+) (\d+)', line[len(line_start):])}


def check_clean(r):
    print(r.stdout)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    calls = counts('calls: ', r.stdout)
    assert all(calls[f] > 0 for f in ('madd', 'add', 'double', 'add_any', 'double_any')), calls
    branches = counts('branches: ', r.stdout)
    assert set(branches) == set(BRANCHES) and all(v > 0 for v in branches.values()), branches
    assert all(r.stdout.count('slack %s:' % f) == 1 for f in FORMULAS)


def test_formulas_keep_their_bounds_and_match_the_group_law(tmp_path):
    check_clean(build_and_run(tmp_path))


def test_the_same_program_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    r = build_and_run(tmp_path, extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'))
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    check_clean(r)


X3 = 'const F28 X3 = f28_normalise(f28_sub<6, 2>(t0, f28_add(Q, Q)));                  // 2Q: limbs < 2 * 2^28, < 4q; X3 < 12q, exact digits\n'
# (what, the text in g2p28.h, its replacement, the kinds of rule of which at least one must fire)
MUTATIONS = [
    ('P P of g2p_madd_fast with K = 64: P goes up to 18q, so 5 P up to 90q is not below K q',
     'fq2p_mul<96>(P, P, odd)', 'fq2p_mul<64>(P, P, odd)', ('value',)),
    ('X3 of g2p_madd_fast with a one-unit spread: 2Q has limbs up to 2^29 - 2',
     X3, X3.replace('f28_sub<6, 2>', 'f28_sub<6, 1>'), ('limb',)),
    ('M of g2p_double left un-normalised: limbs up to 3 * 2^28 on both sides of a merged product',
     'const F28 M = f28_normalise(f28_add(f28_add(XX, XX), XX));', 'const F28 M = f28_add(f28_add(XX, XX), XX);', ('column',)),
    ('the normalise around X3 of g2p_madd_fast dropped: acc.X is kept with loose limbs',
     X3, 'const F28 X3 = f28_sub<6, 2>(t0, f28_add(Q, Q));\n', ('closure',)),
    ('the negation of an entry padded with q alone: with a one-unit spread the constant\'s top limb is one below q\'s, which a canonical y can reach',
     'return f28_normalise(f28_sub<2, 1>(f28_const(Limbs14{}), y));', 'return f28_normalise(f28_sub<1, 1>(f28_const(Limbs14{}), y));', ('value',)),
]


@pytest.mark.parametrize('what,old,new,kinds', MUTATIONS, ids=['madd_pp_k64', 'madd_x3_spread_1', 'double_m_not_normalised', 'madd_x3_not_normalised', 'negate_entry_pad_q'])
def test_a_broken_bound_is_reported(tmp_path, what, old, new, kinds):
    src = open(os.path.join(CSRC, 'g2p28.h')).read()
    assert src.count(old) == 1, 'the text of the mutation must match g2p28.h exactly once'
    patched = os.path.join(str(tmp_path), 'g2p28_patched.h')
    with open(patched, 'w') as f:
        f.write(src.replace(old, new))
    r = build_and_run(tmp_path, patched)
    print(r.stdout, r.stderr)
    v = counts('violations: ', r.stdout)
    total = int(re.search(r'(\d+) limb-rule violations', r.stdout).group(1)) + int(re.search(r'(\d+) mismatches', r.stdout).group(1))
    assert r.returncode == 1 and total > 0, what
    assert any(v[k] > 0 for k in kinds), (what, v)
