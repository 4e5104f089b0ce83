"""The limb and value bounds of the 29-bit-limb Edwards and Poseidon helpers (aleo_amd/csrc/edwards29.h, records_lane.h), checked mechanically on the host.

tests/cpp/ed29_bounds_emul.cpp (on tests/cpp/checked_f29.h) runs the shipped source of f29_tidy, f29_canonical, ed29_cache, ed29_add, ed29_dbl, f29_pow,
f29_sqrt_fixed, psd_pow17, psd_row, psd_full and the permutation over limbs that carry their bounds along, with operands tagged at the edge of each contract,
every stated operand rule turned into a check against the bounds and every result compared with HFr (the affine Edwards law, host::poseidon_permute<4, 8>).
The negative controls patch a copy of a header and expect the checker to fire: a checker that never fires proves nothing.
"""
import os, re, shutil, subprocess
import pytest
import ed29_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join(ROOT, 'aleo_amd', 'csrc')
EMUL = os.path.join(ROOT, 'tests', 'cpp', 'ed29_bounds_emul.cpp')
CHAIN = ('records_host.hpp', 'records_lane.h', 'edwards29.h')      # each includes the next by name: copies that lie together are used together

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')


def build_and_run(tmp_path, patched=None):
    """The program built over the shipped headers, or over copies of CHAIN in which `patched` = (file, old, new) is applied."""
    exe = os.path.join(str(tmp_path), 'ed29_bounds_emul')
    cmd = [HIPCC, '-x', 'c++', '-std=c++17', '-O2', '-mbmi2', '-madx', '-I', CSRC]
    if patched:
        name, old, new = patched
        d = os.path.join(str(tmp_path), 'patched'); os.makedirs(d)
        for f in CHAIN: shutil.copy(os.path.join(CSRC, f), d)
        src = open(os.path.join(d, name)).read()
        assert src.count(old) == 1, 'the text of the mutation must match %s exactly once' % name
        with open(os.path.join(d, name), 'w') as f: f.write(src.replace(old, new))
        cmd.append('-DF29_HEADER="%s"' % os.path.join(d, CHAIN[0]))
    subprocess.check_call(cmd + [EMUL, '-o', exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def counts(line_start, out):
    line = next(l for l in out.splitlines() if l.startswith(line_start))
    return {k: int(v) for k, v in re.findall(r'(\w+) (\d+)', line[len(line_start):])}


FORMULAS = ('f29_tidy', 'f29_canonical', 'ed29_cache', 'ed29_add', 'ed29_dbl', 'f29_pow', 'f29_sqrt_fixed', 'psd_pow17', 'psd_row', 'psd_full', 'psd_permute', 'psd_permute_take1')


def test_helpers_keep_their_bounds_at_the_edges_and_match_the_field(tmp_path):
    r = build_and_run(tmp_path)
    print(r.stdout)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    assert 'violations: limb 0, column 0, value 0, closure 0, sound 0' in r.stdout
    calls = counts('calls: ', r.stdout)
    assert len(calls) == 15 and all(v > 0 for v in calls.values()), calls
    branches = counts('branches: ', r.stdout)
    assert len(branches) == 9 and all(v > 0 for v in branches.values()), branches
    for f in FORMULAS:
        assert r.stdout.count('slack %s: largest column' % f) == 1, f
    for f in ('ed29_cache', 'ed29_add', 'ed29_dbl'):
        line = next(l for l in r.stdout.splitlines() if l.startswith('slack %s:' % f))
        m = re.search(r'largest returned X ([\d.]+) r, Y ([\d.]+) r, Z ([\d.]+) r, T ([\d.]+) r', line)
        assert m and all(float(v) < 3.0001 for v in m.groups()), line
        # the figures the GPU row test holds the kernels to are the ones this program prints
        if f in ed29_rows.RETURNED: assert tuple(float(v) for v in m.groups()) == ed29_rows.RETURNED[f], (line, ed29_rows.RETURNED[f])


def test_the_gpu_rows_pass_the_host_field_and_the_integer_reference(tmp_path):
    """The rows tests/test_gpu_ed29_extremes.py sends to the GPU, through the same source on the host (tests/cpp/ed29_rows_emul.cpp): every row keeps the class it
    was built for (the sound rule), no rule fires over those classes, and every output equals the integer reference limb for limb — the row builders and the
    reference are right before a GPU sees them."""
    c = ed29_rows.build()
    ed29_rows.check_coverage(c)
    cases, results = os.path.join(str(tmp_path), 'rows.bin'), os.path.join(str(tmp_path), 'out.bin')
    ed29_rows.write_case_file(cases, c)
    exe = os.path.join(str(tmp_path), 'ed29_rows_emul')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-O2', '-mbmi2', '-madx', '-I', CSRC, os.path.join(ROOT, 'tests', 'cpp', 'ed29_rows_emul.cpp'), '-o', exe])
    r = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and ' 0 limb-rule violations' in r.stdout and 'violations: limb 0, column 0, value 0, closure 0, sound 0' in r.stdout, r.stdout + r.stderr
    out = ed29_rows.read_result_file(results, c)
    ed29_rows.check_fields(c, out)
    ed29_rows.check_points(c, out)


# (what, the header, the text in it, its replacement, the kinds of rule of which at least one must fire)
MUTATIONS = [
    ('the normalise of X + Y in ed29_dbl dropped: a lazy sum squared, so a multiplier with limbs of 2^30',
     'edwards29.h', 'F29 xy = f29_add(p.X, p.Y); f29_normalise(xy);', 'F29 xy = f29_add(p.X, p.Y);', ('limb',)),
    ('the tidy of h in ed29_add dropped: a lazy sum as a multiplier',
     'edwards29.h', 'f29_tidy(f); f29_tidy(h);', 'f29_tidy(f);', ('limb',)),
    ('g of ed29_dbl normalised but not reduced: it stays near 20 r, and the subtrahend of f must be below 18 r',
     'edwards29.h', 'F29 g = f29_sub_pad(b, a); f29_tidy(g);', 'F29 g = f29_sub_pad(b, a); f29_normalise(g);', ('value',)),
    ('both intermediate normalises of psd_row dropped: the limbs of nine products summed pass 2^32',
     'records_lane.h', '    if (j == 3 || j == 6) f29_normalise(acc);\n', '', ('limb',)),
    ('the normalise of psd_pow17 dropped: a lazy sum squared, limbs of 2^30 on both sides of every column',
     'records_lane.h', '  f29_normalise(t);\n  F29 a = f29_sqr(t);', '  F29 a = f29_sqr(t);', ('column',)),
]


@pytest.mark.parametrize('what,header,old,new,kinds', MUTATIONS, ids=['dbl_xy_not_normalised', 'add_h_not_tidied', 'dbl_g_not_reduced', 'psd_row_no_carries', 'pow17_not_normalised'])
def test_a_broken_bound_is_reported(tmp_path, what, header, old, new, kinds):
    r = build_and_run(tmp_path, (header, old, new))
    print(r.stdout, r.stderr)
    v = counts('violations: ', r.stdout)
    assert r.returncode == 1 and int(re.search(r'(\d+) limb-rule violations', r.stdout).group(1)) > 0, what
    assert all(v[k] > 0 for k in kinds), (what, v)
    if 'psd_row' in what: assert 'wraps 32 bits' in r.stderr, r.stderr
