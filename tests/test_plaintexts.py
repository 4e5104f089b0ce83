"""Record PLAINTEXT strings read by the library: aleo_mi355x_record_plaintext_parse, _plaintext_commitment, _plaintexts_commitments, _plaintexts_serial_numbers and
their _host forms (csrc/plaintext_parse.hpp, plaintexts_lane.h, plaintexts.hip); RecordPlaintext.from_string, serial_number_string on any plaintext,
plaintext_commitments, plaintext_serial_numbers and plaintexts_unspent in aleo_amd/records.py; the same in include/aleo_mi355x.hpp.

Layers, each checked against the one before: the reference's data pins the host path (its three plaintext strings, their microcredits, the serial number of
wasm/src/record/record_plaintext.rs:131-140, the string it refuses); the ROUND TRIP ties the host path to the road the library already had (for every record it
decrypts and renders, the commitment of the rendered string is record_commitment of the ciphertext and its fields); tests/plaintext_ref.py restates grammar and
bits in Python integers; the host path, byte for byte, checks the device lane — emulated on the CPU, plain and under the sanitizers, here, and on the GPU in the
second half (ALEO_MI355X_MIN_PLAINTEXTS=0).  No test reads the reference tree."""
import ctypes, functools, json, os, random, re, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records
import plaintext_ref as PR
from test_records import R, L_ORDER
from test_records_decrypt import Built, TWO_LEVELS, account, literal_text, VIS
from test_records_commit import shapes, NAMES, PER, field, ints
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32

GOLD = json.load(open(os.path.join(HERE, 'golden', 'reference_plaintexts.json')))
SER = json.load(open(os.path.join(HERE, 'golden', 'reference_serial.json')))
SN = SER['serial_number']
RECORD = GOLD['plaintexts'][0]['string']
SCALAR = PR.SCALAR_MODULUS
LANE_CHARS, LANE_ENTRIES = 1024, 8                                                    # plaintexts_lane.h PT_MAX_CHARS, PT_MAX_ENTRIES


# ---- strings ------------------------------------------------------------------------------------------------------------------------------------------
def address(x): return literal_text(0, x)


def plaintext(entries, private=True, nonce=12345, owner=None, sep=('{\n  ', ',\n  ', '\n}')):
    """A record plaintext in render's layout (or with other separators): entries (name, visibility, literal text without its visibility | a struct's text as it stands)."""
    ax = account()[2] if owner is None else owner
    parts = ['owner: %s.%s' % (address(ax), 'private' if private else 'public')] + ['%s: %s' % (n, t if t.endswith('}') else t + '.' + VIS[v]) for n, v, t in entries] + ['_nonce: %dgroup.public' % nonce]
    return sep[0] + sep[1].join(parts) + sep[2]


# every literal type the lane computes, at its edges: 0, the maximum, the minimum of each signed type, modulus - 1
EDGES = [('field', (0, R - 1)), ('group', (0, 5, R - 1)), ('scalar', (0, SCALAR - 1)), ('u8', (0, 255)), ('u16', (0, 65535)), ('u32', (0, 2 ** 32 - 1)), ('u64', (0, 2 ** 64 - 1)),
         ('u128', (0, 2 ** 128 - 1)), ('i8', (-128, -1, 0, 127)), ('i16', (-32768, 32767)), ('i32', (-2 ** 31, 2 ** 31 - 1)), ('i64', (-2 ** 63, 2 ** 63 - 1)),
         ('i128', (-2 ** 127, -1, 2 ** 127 - 1))]


@functools.lru_cache(maxsize=None)
def computed_strings():
    """[(what, string, message bits under NAMES[0] or None)]: what the lane itself computes.  The last four are the iteration boundaries: 8 x 18 name bits + 539
    + per entry 8 |name| + 28 + its value's bits (a boolean's 1, a u8's 8, a field's 253)."""
    ax = account()[2]; out = [(g['name'], g['string'], None) for g in GOLD['plaintexts']]
    lits = [('v%d' % k, k % 3, '%d%s' % (v, suffix)) for k, (suffix, vs) in enumerate((s, v) for s, vals in EDGES for v in vals) for v in [vs]]
    lits += [('who', 2, address(ax)), ('zero', 1, address(0)), ('yes', 2, 'true'), ('no', 0, 'false')]
    for k in range(0, len(lits), LANE_ENTRIES): out.append(('edges %d' % k, plaintext(lits[k:k + LANE_ENTRIES], private=k % 16 == 0, nonce=R - 1 - k), None))
    out.append(('no entries, a public owner', plaintext([], private=False, nonce=0), None))
    out.append(('names of 1 and 31 characters', plaintext([('a', 2, '7u8'), ('b' * 31, 1, 'true'), ('C', 0, '5u64'), ('d_' * 15 + 'e', 2, '99field')]), None))
    out.append(('one line, two spaces', plaintext([('microcredits', 2, '2000000u64')], sep=('{  ', ',  ', '}')), None))
    out.append(('tabs, CR LF and no space at all', plaintext([('microcredits', 1, '9u64'), ('x', 2, '-5i8')]).replace('\n  ', '\r\n\t').replace(': ', ' :\t') + ' \r\n', None))
    out.append(('tight', plaintext([('microcredits', 2, '1u32'), ('t', 2, '3u8')], sep=('{', ',', '}')).replace(': ', ':'), None))
    out.append(('microcredits in a u32: no microcredits', plaintext([('microcredits', 2, '77u32')]), None))
    out.append(('exactly per bits', plaintext([('f' * 6, 2, 'true'), ('g' * 31, 2, '200u8')]), PER))
    out.append(('per + 1 bits', plaintext([('f' * 7, 2, 'false'), ('g' * 31, 1, 'true')], private=False), PER + 1))
    out.append(('2 per bits', plaintext([('a' * 31, 2, '1field'), ('b' * 29, 2, '2field'), ('c', 2, '3field'), ('d', 2, 'true'), ('e', 2, 'false')]), 2 * PER))
    out.append(('2 per + 1 bits', plaintext([('a' * 23, 2, '1field'), ('b', 2, '2field'), ('c', 2, '3field'), ('d', 0, '%dfield' % (R - 1)), ('e', 2, 'true'), ('f', 2, 'false')]), 2 * PER + 1))
    return out


@functools.lru_cache(maxsize=None)
def routed_strings():
    """What the lane hands to the host code, which computes it: structs, a quoted string, other spellings, strings over the lane's caps."""
    many = [('e%d' % k, 2, '%du8' % k) for k in range(LANE_ENTRIES + 1)]
    return [('a struct of two levels', plaintext([('s', 2, '{\n    amount: 42u64.private,\n    inner: {\n      flag: true.private,\n      deep: -5i64.private\n    },\n    tail: 3u8.private\n  }')])),
            ('a quoted string', plaintext([('memo', 1, '"hello, {world}: 1u8.private"')])),
            ('an underscore spelling', plaintext([('microcredits', 2, '1_500_000u64')])),
            ('an over-long string', plaintext([('microcredits', 2, '5u64')]) + ' ' * LANE_CHARS),
            ('a leading zero', plaintext([('x', 2, '007u8')])),
            ('minus zero', plaintext([('x', 2, '-0i8')])),
            ('one entry more than the lane takes', plaintext(many))]


@functools.lru_cache(maxsize=None)
def malformed_strings():
    good = plaintext([('x', 2, '1u8')]); addr = address(account()[2])
    flipped = addr[:-1] + ('q' if addr[-1] != 'q' else 'p')
    return [('value = modulus', plaintext([('x', 2, '%dfield' % R)])), ('scalar = its modulus', plaintext([('x', 2, '%dscalar' % SCALAR)])), ('78 digits', plaintext([('x', 2, '1' + '0' * 77 + 'field')])),
            ('a u8 of 256', plaintext([('x', 2, '256u8')])), ('an i8 of -129', plaintext([('x', 2, '-129i8')])), ('an i8 of 128', plaintext([('x', 2, '128i8')])),
            ('a bad checksum', good.replace(addr, flipped)), ('the prefix aleo2', GOLD['invalid']['string']), ('a duplicate name', plaintext([('x', 2, '1u8'), ('x', 2, '2u8')])),
            ('a missing nonce', good.replace('_nonce: 12345group.public', 'nonce: 12345group.public')), ('no nonce at all', '{\n  owner: %s.private,\n  x: 1u8.private\n}' % addr),
            ('trailing text', good + ' x'), ('a sign on a field', plaintext([('x', 2, '-1field')])), ('a sign on a u8', plaintext([('x', 2, '-1u8')])), ('a comment', good.replace('{', '{ // the owner', 1)),
            ('a name that is no identifier', plaintext([('9x', 2, '1u8')])), ('an entry named owner', plaintext([('owner', 2, '1u8')])), ('a constant owner', good.replace('.private,', '.constant,', 1)),
            ('a private nonce', good.replace('group.public', 'group.private')), ('mixed visibilities in a struct', plaintext([('s', 2, '{ a: 1u8.private, b: 2u8.public }')])),
            ('a comma behind the nonce', good.replace('group.public', 'group.public,')), ('no visibility', plaintext([('x', 2, '1u8')]).replace('1u8.private', '1u8')), ('the empty string', ''), ('a word', 'string')]


def host_rows(strings, names=NAMES[0]): return records.plaintext_commitments(strings, *names, host=True)


# ---- 1: pins ------------------------------------------------------------------------------------------------------------------------------------------
def test_pin_the_reference_s_serial_number_from_its_plaintext_string():
    p = records.RecordPlaintext.from_string(RECORD)
    assert p.ciphertext is None and p.serial_number_string(SN['private_key'], SN['program_id'], SN['record_name']) == SN['expected']
    assert p.serial_number_string(records.Account.from_private_key(SN['private_key']), SN['program_id'], SN['record_name']) == SN['expected']      # twice, as the reference runs it
    sn, cm, mc, flags = records.plaintext_serial_numbers([RECORD], SN['program_id'], SN['record_name'], SN['private_key'], host=True)
    assert flags.tolist() == [0] and ['%dfield' % v for v in ints(sn)] == [SN['expected']] and cm[0].tobytes() == records.plaintext_commitment(RECORD, SN['program_id'], SN['record_name'])


def test_pin_microcredits_and_the_string_the_reference_refuses():
    for g in GOLD['plaintexts']:
        p = records.RecordPlaintext.from_string(g['string'])
        assert p.microcredits() == g['microcredits'] and str(p) == g['string'], g['name']
    assert host_rows([g['string'] for g in GOLD['plaintexts']])[1].tolist() == [1500000000000000, 2000000001, 5]
    for bad in (GOLD['invalid']['string'], GOLD['invalid_message']['string']):
        with pytest.raises(aleo_amd.AleoMi355xError) as err: records.RecordPlaintext.from_string(bad)
        assert str(err.value).startswith(GOLD['invalid_message']['message'])
    assert host_rows([GOLD['invalid']['string']])[2].tolist() == [3]


def test_pin_the_three_error_messages():
    p = records.RecordPlaintext.from_string(RECORD)
    for e in SER['errors']:
        with pytest.raises(aleo_amd.AleoMi355xError) as err: p.serial_number_string(SN['private_key'], e['program_id'], e['record_name'])
        assert str(err.value) == e['message'], e['source']
        with pytest.raises(aleo_amd.AleoMi355xError) as err: records.plaintext_commitment(RECORD, e['program_id'], e['record_name'])
        assert str(err.value) == e['message'], e['source']
        for host in (True, False):                                                                 # one string: below min_plaintexts, the call stays on the host
            with pytest.raises(aleo_amd.AleoMi355xError) as err: records.plaintext_commitments([RECORD], e['program_id'], e['record_name'], host=host)
            assert str(err.value) == e['message'], e['source']
    with pytest.raises(aleo_amd.AleoMi355xError) as err: records.plaintext_commitment(GOLD['invalid_message']['string'], SN['program_id'], SN['record_name'])
    assert str(err.value) == GOLD['invalid_message']['message']


def test_parse_asks_for_points_of_the_subgroup_and_the_batch_calls_do_not():
    """A small x is canonical; whether it is the x of a point of the subgroup decides record_plaintext_parse alone (the reference's own strings pass it: above)."""
    L = aleo_amd.lib(); accepted = refused = 0
    for x in range(2, 40):
        s = plaintext([('g', 1, '%dgroup' % x)])
        rc = L.aleo_mi355x_record_plaintext_parse(s.encode(), None, None, None, None)
        assert host_rows([s])[2].tolist() == [0]
        accepted += rc == 0; refused += rc != 0
    assert accepted >= 3 and refused >= 3                                                               # about a quarter of all x are a subgroup point's
    kind = ctypes.c_int32(-1); owner = np.zeros(32, dtype=np.uint8); nonce = np.zeros(32, dtype=np.uint8); mc = ctypes.c_uint64(7)
    assert L.aleo_mi355x_record_plaintext_parse(RECORD.encode(), ctypes.byref(kind), bs._p(owner), bs._p(nonce), ctypes.byref(mc)) == 0
    p = records.RecordPlaintext(RECORD)
    assert kind.value == 1 and owner.tobytes() == records.address_x_bytes(p.owner) and nonce.tobytes() == le32(p.nonce) and mc.value == 1500000000000000


# ---- 2: the round trip --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_records():
    """Built records (ciphertexts) covering every literal type at its edges in every visibility, a struct of two levels, public and constant entries."""
    G, vk, ax = account(); out = []; types = {s: t for t, s in {2: 'field', 3: 'group', 14: 'scalar', **{4 + i: 'i%d' % (8 << i) for i in range(5)}, **{9 + i: 'u%d' % (8 << i) for i in range(5)}}.items()}
    lits = [('lit', types[s], v) for s, vals in EDGES for v in vals] + [('lit', 0, ax), ('lit', 0, 0), ('lit', 1, True), ('lit', 1, False), ('lit', 15, ''), ('lit', 15, 'a string, with: punctuation {and} braces')]
    for vis in (0, 1, 2):
        for k in range(0, len(lits), 6): out.append(Built(G, vk, ax, (k + vis) % 2 == 0, [('n%d' % (k + i), vis, lit) for i, lit in enumerate(lits[k:k + 6])], 7000 + 10 * k + vis))
    out.append(Built(G, vk, ax, True, [('s', 0, TWO_LEVELS), ('t', 1, TWO_LEVELS), ('u', 2, TWO_LEVELS), ('microcredits', 2, ('lit', 12, 2 ** 64 - 1))], 7999))
    return out


def rendered(strings):
    """[(ciphertext string, rendered plaintext string, its commitment through record_commitment)] of the account's records that decrypt and render."""
    G, vk, ax = account(); out = []
    found = records.decrypt_strings(strings, vk, ax, host=True, keep=True)
    cm, flags = records.found_commitments(strings, found, *NAMES[0], host=True)
    for k, i in enumerate(found.index.tolist()):
        if found.status[k] or flags[k]: continue
        try: pt = records.RecordCiphertext.from_string(strings[i]).plaintext(found.fields(k))
        except aleo_amd.AleoMi355xError: continue
        out.append((strings[i], pt.string, cm[k].tobytes(), int(found.microcredits[k])))
    return out


def test_round_trip_bits_of_parse_of_render_are_the_bits_of_the_decrypted_fields():
    cases = shapes()
    strings = [s for _, s, _, _ in cases] + [b.string for b in edge_records()]
    got = rendered(strings)
    assert len(got) >= len(strings) - 8 and {s for s, _, _, _ in got} >= {b.string for b in edge_records()}      # all but the shapes that are refused or do not render
    cm, mc, flags = host_rows([p for _, p, _, _ in got])
    assert not flags.any() and [r.tobytes() for r in cm] == [c for _, _, c, _ in got] and mc.tolist() == [m for _, _, _, m in got]
    # the iteration boundaries are among them, and records with public and constant entries
    by_string = {s: p for s, p, _, _ in got}
    for what, s, _, bits in cases:
        if bits is not None: assert 8 * 18 + len(PR.record_bits(by_string[s])) == bits, what
    assert sum('.constant' in p for p in by_string.values()) >= 5 and sum('.public,' in p for p in by_string.values()) >= 5
    # and the restatement agrees on every one of them
    for _, p, c, _ in got[::3]: assert le32(PR.commitment(p, *NAMES[0])) == c


# ---- 3: the restatement -----------------------------------------------------------------------------------------------------------------------------------
def random_plaintext(rng):
    ax = account()[2]
    def lit():
        suffix, vals = rng.choice(EDGES); ty = PR.SUFFIX[suffix]
        lo, hi = (-(1 << (PR.BITS[ty] - 1)), 1 << (PR.BITS[ty] - 1)) if 4 <= ty <= 8 else (0, R if ty in (2, 3) else SCALAR if ty == 14 else 1 << PR.BITS[ty])
        return rng.choice(['%d%s' % (rng.choice([rng.randrange(lo, hi), rng.choice(vals)]), suffix), 'true', 'false', address(rng.choice([ax, 0, 5])), '"%s"' % ('x' * rng.randrange(0, 9))])
    def value(vis, depth):
        if depth < 3 and rng.random() < 0.2: return '{' + ws() + (',' + ws()).join('m%d%s:%s%s' % (k, ws(), ws(), value(vis, depth + 1)) for k in range(rng.randrange(1, 4))) + ws() + '}'
        return lit() + '.' + VIS[vis]
    def ws(): return rng.choice(['', ' ', '\n  ', '\t', '\r\n', '  '])
    entries = ['e%d%s:%s%s' % (k, ws(), ws(), value(rng.randrange(3), 0)) for k in range(rng.randrange(0, 6))]
    parts = ['owner%s:%s%s.%s' % (ws(), ws(), address(ax), rng.choice(['public', 'private']))] + entries + ['_nonce%s:%s%dgroup.public' % (ws(), ws(), rng.randrange(R))]
    return ws() + '{' + ws() + (ws() + ',' + ws()).join(parts) + ws() + '}' + ws()


def test_restatement_equals_the_host_path_on_generated_strings_whitespace_variants_and_malformed_strings():
    rng = random.Random(20240); strings = [random_plaintext(rng) for _ in range(60)] + [s for _, s, _ in computed_strings()] + [s for _, s in routed_strings()]
    cm, mc, flags = host_rows(strings, NAMES[1])
    assert not flags.any()
    for s, row, m in zip(strings, cm, mc.tolist()): assert le32(PR.commitment(s, *NAMES[1])) == row.tobytes() and PR.microcredits(s) == m, s
    bad = [s for _, s in malformed_strings()]
    cm, mc, flags = host_rows(bad)
    assert flags.tolist() == [3] * len(bad) and not cm.any() and not mc.any()
    for what, s in malformed_strings():
        with pytest.raises(PR.Refused): PR.parse(s)
    # whitespace changes no bit
    base = computed_strings()[0][1]; want = host_rows([base])[0][0].tobytes()
    for variant in (base.replace('\n', ' '), base.replace('\n  ', '\r\n\t\t'), base.replace(': ', ':').replace('\n', '').replace(' ', ''), '\n\n' + base + '\n'):
        assert host_rows([variant])[0][0].tobytes() == want and le32(PR.commitment(variant, *NAMES[0])) == want


# ---- 4: the device lane, emulated on the host ---------------------------------------------------------------------------------------------------------
def batch(n):
    """n strings: the lane-computed shapes in turn, with — from 63 strings on — exactly 4 routed records (a struct, a quoted string, an underscore spelling, an
    over-long string) and 2 malformed ones (a value that is its modulus, a bad checksum) among the first 64: side by side in one wave.  Returns (strings, k + m)."""
    good = [s for _, s, _ in computed_strings()]; out = [good[i % len(good)] for i in range(n)]
    if n < 63: return out, 0
    special = [s for _, s in routed_strings()[:4]] + [malformed_strings()[0][1], malformed_strings()[6][1]]
    for j, s in enumerate(special): out[5 + 9 * j] = s
    return out, len(special)


def write_lane_cases(path, cases, names):
    """cases: [(string, routed by the lane)]; the rows are the host path's.  Returns how many the host path computes."""
    strings = [s for s, _ in cases]
    cm, mc, flags = host_rows(strings, names)
    with open(path, 'wb') as f:
        for text in names: f.write(struct.pack('<I', len(text)) + text.encode())
        f.write(struct.pack('<I', len(strings)))
        for k, (s, routed) in enumerate(cases):
            b = s.encode()
            f.write(struct.pack('<I', len(b)) + b + bytes([8 if routed else 0, int(flags[k])]) + cm[k].tobytes() + struct.pack('<Q', int(mc[k])))
    return int((flags == 0).sum())


def lane_counts(r):
    assert r.returncode == 0 and ' 0 mismatches, 0 reads past an end, 0 limb-rule violations' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    m = re.search(r'(\d+) strings, (\d+) computed, (\d+) refused, (\d+) routed.*iterations 1: (\d+), 2: (\d+), 3: (\d+), other: (\d+)', r.stdout)
    return [int(v) for v in m.groups()]


@pytest.mark.parametrize('sanitized', [False, True])
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path, sanitized):
    """tests/cpp/plaintexts_lane_emul.cpp: plaintexts_lane.h compiled for the CPU over the checked restatement of fr29.h, a program of its own, once plain and once
    with the address and undefined-behaviour sanitizers: every computed, routed and malformed string under the three name pairs, and the counts exactly."""
    good, routed, bad = computed_strings(), routed_strings(), malformed_strings()
    cases = [(s, False) for _, s, _ in good] + [(s, True) for _, s in routed] + [(s, True) for _, s in bad]
    exe = bs.build_lane_emul(tmp_path, 'plaintexts_lane_emul', sanitized=sanitized, flags=())
    for names in NAMES:
        path = os.path.join(str(tmp_path), 'cases.bin')
        assert write_lane_cases(path, cases, names) == len(good) + len(routed)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        got = lane_counts(r)
        assert got[:4] == [len(cases), len(good), len(bad), len(routed) + len(bad)], r.stdout[-400:]
        its = [(8 * (len(names[0]) - 1 + len(names[1])) + len(PR.record_bits(s)) + PER - 1) // PER for _, s, _ in good]      # from the restatement's bits
        assert got[4:] == [its.count(1), its.count(2), its.count(3), len(its) - its.count(1) - its.count(2) - its.count(3)] and min(got[4:7]) >= 1, r.stdout[-400:]
        if names == NAMES[0]:
            for what, s, bits in good:
                if bits is not None: assert 8 * 18 + len(PR.record_bits(s)) == bits and ': %d bits\n' % bits in r.stdout, what


def test_the_gpu_batches_hold_the_routed_and_malformed_strings_their_tests_count(tmp_path):
    """The batches of the GPU tests through the lane emulation: the host-side count of each is the k + m its test asserts of plaintexts_last_routed()."""
    exe = bs.build_lane_emul(tmp_path, 'plaintexts_lane_emul', flags=())
    for n in (1, 63, 65):
        strings, special = batch(n)
        path = os.path.join(str(tmp_path), 'batch.bin')
        routed = set(s for _, s in routed_strings()) | set(s for _, s in malformed_strings())
        computed = write_lane_cases(path, [(s, s in routed) for s in strings], NAMES[0])
        got = lane_counts(subprocess.run([exe, path], capture_output=True, text=True, timeout=600))
        assert got[:4] == [n, n - special, 2 if special else 0, special] and computed == n - (2 if special else 0) and 10 * special <= n


# ---- 5: thresholds, the code objects, the C++ mirror --------------------------------------------------------------------------------------------------------
def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_plaintexts', 'ALEO_MI355X_MIN_PLAINTEXTS') == (32, 5, 32)


def test_last_routed_counts_every_string_of_a_host_call():
    strings, _ = batch(7)
    records.plaintext_commitments(strings, *NAMES[0], host=True)
    assert records.plaintexts_last_routed() == 7
    records.plaintext_commitments(strings[:3], *NAMES[0])                                               # below the threshold: the host path
    assert records.plaintexts_last_routed() == 3


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_plaintext_and_commit_kernel_code_objects_are_gfx950_and_have_no_scratch():
    assert bs.scratch_and_spills('plaintexts', ['k_plaintexts_commit', 'k_plaintexts_flags']) == (2, {'k_plaintexts_commit': (0, 0, 0), 'k_plaintexts_flags': (0, 0, 0)})
    assert bs.scratch_and_spills('records_commit', ['k_records_commit']) == (1, {'k_records_commit': (0, 0, 0)})      # after the factoring of its hashing loop


def run_cpp_mirror(tmp_path, env):
    r = bs.run_cpp_mirror(tmp_path, 'plaintexts_test', [SN['private_key'], SN['program_id'], SN['record_name'], le32(field(SN['expected'])).hex(), 1500000000000000, RECORD, GOLD['invalid']['string']], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_PLAINTEXTS': '1000000'})


def test_refusals_and_edges():
    L = aleo_amd.lib(); b = records.RecordBatch.from_strings([RECORD] * 2); text = records._text_p(b); p = bs._p
    cm = np.zeros((2, 32), dtype=np.uint8); sn = np.zeros((2, 32), dtype=np.uint8); fl = np.zeros(2, dtype=np.uint8); sk = np.frombuffer(records.Account.from_private_key(SN['private_key']).sk_sig, dtype=np.uint8)
    for f in (L.aleo_mi355x_plaintexts_commitments, L.aleo_mi355x_plaintexts_commitments_host):
        assert f(None, None, p(fl), text, p(b.offsets), 2, b'credits.aleo', b'credits') != 0 and f(p(cm), None, None, text, p(b.offsets), 2, b'credits.aleo', b'credits') != 0
        assert f(p(cm), None, p(fl), text, None, 2, b'credits.aleo', b'credits') != 0 and f(p(cm), None, p(fl), text, p(b.offsets), 2, None, b'credits') != 0
        assert f(p(cm), None, p(fl), text, p(b.offsets), 2, b'credits.aleo', b'credits') == 0 and fl.tolist() == [0, 0]      # microcredits may be NULL
        assert f(None, None, None, None, p(b.offsets[:1]), 0, b'credits.aleo', b'credits') == 0                            # n = 0
    for f in (L.aleo_mi355x_plaintexts_serial_numbers, L.aleo_mi355x_plaintexts_serial_numbers_host):
        head = (text, p(b.offsets), 2, b'credits.aleo', b'credits')
        assert f(None, None, None, p(fl), *head, p(sk), None, 0) != 0 and f(p(sn), None, None, p(fl), *head, None, None, 0) != 0 and f(p(sn), None, None, p(fl), *head, p(sk), None, 1) != 0
        assert f(p(sn), None, None, p(fl), *head, p(np.frombuffer(le32(L_ORDER), dtype=np.uint8)), None, 0) != 0
        assert f(p(sn), None, None, p(fl), *head, p(sk), None, 0) == 0 and fl.tolist() == [0, 0] and ['%dfield' % v for v in ints(sn)] == [SN['expected']] * 2      # cm_out may be NULL
    idx, sns, mcs = records.plaintexts_unspent([records.RecordPlaintext(RECORD), GOLD['plaintexts'][2]['string'], 'string'], SN['program_id'], SN['record_name'], SN['private_key'],
                                              spent=[le32(field(SN['expected']))], host=True)
    assert idx.tolist() == [1] and mcs.tolist() == [5] and sns.shape == (1, 32)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_PLAINTEXTS', '0')
    for name in ('ALEO_MI355X_PLAINTEXTS_CHUNK', 'ALEO_MI355X_SERIAL_CHUNK'): monkeypatch.delenv(name, raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_plaintexts()) == 0
    return monkeypatch


def account_of_the_tests(): return records.Account(None, le32(0x1234567 | 1), le32(account()[1]), le32(account()[2]))


def check_kernel_equals_host(strings, special, spent=(), names=NAMES[0]):
    acct = account_of_the_tests()
    cm, mc, flags = records.plaintext_commitments(strings, *names)
    assert records.plaintexts_last_routed() == special
    want = records.plaintext_commitments(strings, *names, host=True)
    assert cm.tobytes() == want[0].tobytes() and mc.tolist() == want[1].tolist() and flags.tolist() == want[2].tolist()
    got = records.plaintext_serial_numbers(strings, *names, acct, spent)
    assert records.plaintexts_last_routed() == special
    want = records.plaintext_serial_numbers(strings, *names, acct, spent, host=True)
    for g, w in zip(got, want): assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert got[1].tobytes() == cm.tobytes()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_kernel_equals_the_host_path_at_wave_and_block_edges(on_kernel, n):
    strings, special = batch(n)
    sn, cm, mc, flags = check_kernel_equals_host(strings, special)
    assert sorted(set(flags.tolist())) == ([0, 3] if special else [0]) and int((flags == 3).sum()) == (2 if special else 0)


@pytest.mark.gpu
@pytest.mark.parametrize('names', NAMES[1:])
def test_kernel_under_names_that_leave_one_and_two_bits_in_hand(on_kernel, names):
    strings, special = batch(65)
    check_kernel_equals_host(strings, special, names=names)


@pytest.mark.gpu
def test_kernel_launches_of_one_wave_continue_the_rows(on_kernel):
    strings, special = batch(300)
    whole = check_kernel_equals_host(strings, special)
    on_kernel.setenv('ALEO_MI355X_PLAINTEXTS_CHUNK', '64'); on_kernel.setenv('ALEO_MI355X_SERIAL_CHUNK', '64')      # five launches, the last one partial
    cut = check_kernel_equals_host(strings, special)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cut, whole))


@pytest.mark.gpu
def test_kernel_spent_sets_some_a_stranger_and_none(on_kernel):
    strings, special = batch(70)
    sn, cm, mc, flags = check_kernel_equals_host(strings, special)
    rows = [r.tobytes() for r, f in zip(sn, flags) if f == 0]
    for spent in (rows[::3], [le32(11)], rows[:5] + [le32(11), le32(R - 1)] + rows[:5], ()):
        got = check_kernel_equals_host(strings, special, spent=spent)
        inside = set(spent)
        assert got[3].tolist() == [3 if f == 3 else int(r.tobytes() in inside) for r, f in zip(sn, flags)] and got[0].tobytes() == sn.tobytes()


@pytest.mark.gpu
def test_kernel_gives_the_reference_s_serial_number_among_64_others(on_kernel):
    strings, _ = batch(64); strings = strings[:40] + [RECORD] + strings[40:]
    sn, cm, mc, flags = records.plaintext_serial_numbers(strings, SN['program_id'], SN['record_name'], SN['private_key'])
    assert records.plaintexts_last_routed() == 6 and flags[40] == 0 and '%dfield' % ints(sn[40:41])[0] == SN['expected'] and mc[40] == 1500000000000000
    idx, _, _ = records.plaintexts_unspent(strings, SN['program_id'], SN['record_name'], SN['private_key'], spent=[le32(field(SN['expected']))])
    assert 40 not in idx.tolist() and idx.tolist() == [i for i in range(65) if flags[i] == 0 and strings[i] != RECORD]


@pytest.mark.gpu
def test_first_call_of_a_fresh_process_and_two_threads_at_once(on_kernel):
    """tests/helpers/plaintexts_first_calls.py, a process of its own: two threads whose first calls of the process are plaintext_serial_numbers, so the one-time
    table builds and uploads run under both."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_PLAINTEXTS='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'plaintexts_first_calls.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr
    strings, special = batch(130); acct = account_of_the_tests()
    want = records.plaintext_serial_numbers(strings, *NAMES[0], acct, host=True)
    got = bs.two_threads(lambda i: records.plaintext_serial_numbers(strings, *NAMES[0], acct))
    for g in got: assert all(a.tobytes() == b.tobytes() for a, b in zip(g, want))


@pytest.mark.gpu
def test_cpp_mirror_on_the_kernel(on_kernel, tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_PLAINTEXTS': '0'})
