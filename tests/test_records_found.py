"""decrypt_strings: the records one account owns among n "record1…" strings, decrypted, in one call (aleo_mi355x_records_decrypt_strings / _strings_host and the
aleo_mi355x_found_* accessors; FoundRecords, decrypt_strings, balance and the string road of decrypt_owned in aleo_amd/records.py).

The yardstick of the host path is the composition of the calls the library already had, written out in `composed` below: scan_strings(host=True), then per owned
string RecordCiphertext.fields (aleo_mi355x_record_fields), decrypt_fields(host=True), and RecordPlaintext(record_plaintext(…)).microcredits().  The yardstick of
the kernels is the host path, byte for byte.  The first half needs no GPU; the second half runs the kernels (ALEO_MI355X_MIN_RECORDS=0)."""
import ctypes, functools, os, random, re, struct, subprocess, tempfile
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps
import batch_support as bs
from batch_support import ROOT, HIPCC, CSRC, le32
from test_records import REF, R, L_ORDER, account_generator, synthetic_records
from test_records_strings import MAX_CHARS, encode, payload_of, reference_sized
from test_records_decrypt import Built, TWO_LEVELS, account, string_of_fields

ARRAYS = ('index', 'kind', 'rvk', 'offsets', 'plain', 'status', 'microcredits')


def same_found(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a.arrays(), b.arrays())) and (a.unparsed, a.first_unparsed) == (b.unparsed, b.first_unparsed)


def differences(a, b):
    return [name for name, x, y in zip(ARRAYS, a.arrays(), b.arrays()) if x.shape != y.shape or x.tobytes() != y.tobytes()] + ([] if (a.unparsed, a.first_unparsed) == (b.unparsed, b.first_unparsed) else ['unparsed'])


def private_entry(fields): return b'\x02' + struct.pack('<H', len(fields)) + b''.join(le32(f) for f in fields)


@functools.lru_cache(maxsize=None)
def off_curve_nonce():
    G, vk, ax = account()
    _, nxs, _, edge = synthetic_records(1, 1, vk, 77, G)
    return nxs[[i for i, name in edge.items() if name == 'x off the curve'][0]]


@functools.lru_cache(maxsize=None)
def case_list():
    """[(what, string, owned, status or None)] for the account of tests/test_records_decrypt.py: every shape the issue names, owned and foreign records mixed."""
    G, vk, ax = account(); rng = random.Random(2718)
    other_vk = 0x77777777777777777777 | 1; other_ax = ps.ed_mul(G, other_vk)[0]
    out = []
    def add(what, string, owned, status=0): out.append((what, string, owned, status if owned else None))
    seed = [600]
    def built(private, entries, key=vk, addr=ax): seed[0] += 1; return Built(G, key, addr, private, entries, seed[0]).string
    for m in (0, 1, 2, 8, 9, 17):                                  # private fields in all: a second permutation from 9, a third from 17
        if m >= 1: add('private owner, %d private fields' % m, built(True, [('pad', 2, string_of_fields(m - 1))] if m > 1 else []), True)
        add('public owner, %d private fields' % m, built(False, [('pad', 2, string_of_fields(m))] if m else [('memo', 1, ('lit', 15, 'in the clear'))]), True)
    add('public owner, no entries', built(False, []), True)
    add('a struct entry, private', built(True, [('s', 2, TWO_LEVELS)]), True)
    add('struct entries, private and constant, public owner', built(False, [('s', 2, TWO_LEVELS), ('t', 0, TWO_LEVELS)]), True)
    add('microcredits private u64', built(True, [('microcredits', 2, ('lit', 12, 1500000000000000))]), True)
    add('microcredits private u64, the largest', built(False, [('microcredits', 2, ('lit', 12, 2 ** 64 - 1)), ('memo', 1, ('lit', 15, 'hello'))]), True)
    add('microcredits private u64 behind other private entries', built(True, [('data', 2, TWO_LEVELS), ('pad', 2, string_of_fields(3)), ('microcredits', 2, ('lit', 12, 77))]), True)
    add('microcredits public u64', built(True, [('microcredits', 1, ('lit', 12, 123456789012))]), True)
    add('microcredits constant u64', built(False, [('microcredits', 0, ('lit', 12, 2 ** 63 + 5))]), True)
    add('microcredits private, a u128', built(True, [('microcredits', 2, ('lit', 13, 99))]), True)
    add('microcredits private, a field', built(True, [('microcredits', 2, ('lit', 2, 5))]), True)
    add('microcredits public, a u32', built(True, [('microcredits', 1, ('lit', 11, 7))]), True)
    add('microcredits a struct', built(True, [('microcredits', 2, ('struct', [('microcredits', ('lit', 12, 5))]))]), True)
    add('microcredits absent, a longer name that starts with it', built(True, [('microcredits_', 2, ('lit', 12, 5)), ('Microcredits', 2, ('lit', 12, 6))]), True)
    add('microcredits twice: the last one counts', built(True, [('microcredits', 2, ('lit', 12, 5)), ('microcredits', 1, ('lit', 12, 6))]), True)
    add('a foreign record, private owner', built(True, [('microcredits', 2, ('lit', 12, 1000))], other_vk, other_ax), False)
    add('a foreign record, public owner', built(False, [('microcredits', 2, ('lit', 12, 1000))], other_vk, other_ax), False)
    add('the reference\'s record, another account\'s', REF['records']['owner'], False)
    for _ in range(3): add('random bytes of the reference\'s shape', encode(reference_sized(rng)), False)
    # what record_fields refuses: status 4, no fields
    base = wire.bech32m_decode(built(True, [('microcredits', 2, ('lit', 12, 9)), ('pad', 2, string_of_fields(2))]))[1]
    # variant 0 | count 1..2 | owner 3..34 | entries 35 | name length 36 | name 37..48 | length 49..50 | visibility 51 | count 52..53 | field 54..85 | next entry 86
    assert base[36] == 12 and base[51] == 2 and base[52:54] == b'\x01\x00' and base[86] == 3
    add('a private field = r', encode(base[:54] + le32(R) + base[86:]), True, 4)
    add('a private field = 2^256 - 1 in the second entry', encode(base[:-64] + b'\xff' * 32 + base[-32:]), True, 4)
    add('an entry with visibility 3', encode(base[:51] + b'\x03' + base[52:]), True, 4)
    add('a private entry whose count does not fit its length', encode(base[:52] + b'\x02' + base[53:]), True, 4)
    add('a name with a character outside [0-9a-zA-Z_]', encode(base[:40] + b'-' + base[41:]), True, 4)
    pub = lambda nonce, entries: encode(payload_of(False, ax, nonce, entries))
    good_nonce = int.from_bytes(base[-32:], 'little')
    add('an empty name', pub(good_nonce, [(b'', b'\x01\x00\x09\x00\x05')]), True, 4)
    add('an entry of no bytes', pub(good_nonce, [(b'v', b'')]), True, 4)
    add('a private entry of two bytes', pub(good_nonce, [(b'v', b'\x02\x00')]), True, 4)
    # a public owner that is the account, and a nonce that is not on the curve: malformed only where there is something to decrypt
    add('public owner, nonce off the curve, a private field', pub(off_curve_nonce(), [(b'v', private_entry([rng.randrange(R)]))]), True, 2)
    add('public owner, nonce off the curve, 9 private fields', pub(off_curve_nonce(), [(b'a', private_entry([rng.randrange(R) for _ in range(4)])), (b'microcredits', private_entry([rng.randrange(R) for _ in range(5)]))]), True, 2)
    add('public owner, nonce off the curve, nothing private', pub(off_curve_nonce(), [(b'microcredits', b'\x01\x00\x0c\x00' + struct.pack('<Q', 31))]), True, 0)
    add('public owner, nonce x = 0, a private field of random bits', pub(0, [(b'microcredits', private_entry([rng.randrange(R)]))]), True, 0)
    add('public owner that is not the account', encode(payload_of(False, other_ax, good_nonce, [(b'v', private_entry([5]))])), False)
    # strings that do not parse
    add('garbage', 'garbage', False); add('the empty string', '', False); add('a record cut short', REF['records']['owner'][:-1], False)
    add('more than 2^20 characters', 'record1' + 'q' * (MAX_CHARS - 6), False)
    add('owner variant 2', encode(payload_of(True, ax, good_nonce, variant=2)), False)
    return out


def composed(strings, view_key, ax: bytes):
    """The existing host calls put together, one owned record at a time."""
    batch = records.RecordBatch.from_strings(strings)
    flags, kinds, rvk = records.scan_strings(batch, [view_key], [ax], host=True)
    index, kind, rows, offsets, plain, status, mc = [], [], [], [0], [], [], []
    for i in np.flatnonzero(flags[0] == 1).tolist():
        index.append(i); kind.append(int(kinds[i])); rows.append(rvk[0, i]); st, credits, mine = 0, 0, np.zeros((0, 32), dtype=np.uint8)
        rec = records.RecordCiphertext.from_string(strings[i])
        try: fields = rec.fields()
        except aleo_amd.AleoMi355xError: st = 4
        else:
            if kinds[i] == 0 and len(fields) and records.scan(np.frombuffer(rec.owner, dtype=np.uint8), np.frombuffer(rec.nonce, dtype=np.uint8), view_key, ax, want_rvk=False, host=True)[0][0] == 2:
                st, mine = 2, np.zeros_like(fields)
            else:
                mine, fl = records.decrypt_fields(rvk[0, i:i + 1], np.array([0, len(fields)], dtype=np.uint32), fields, host=True); st = int(fl[0])
        if st == 0:
            try: credits = rec.plaintext(mine).microcredits()
            except aleo_amd.AleoMi355xError: credits = 0
        offsets.append(offsets[-1] + len(mine)); plain.append(mine); status.append(st); mc.append(credits)
    unparsed = np.flatnonzero(flags[0] == 3)
    return records.FoundRecords(np.array(index, dtype=np.uint32), np.array(kind, dtype=np.int8), np.stack(rows).astype(np.uint8) if rows else np.zeros((0, 32), dtype=np.uint8), np.array(offsets, dtype=np.uint32),
                                np.concatenate(plain) if plain else np.zeros((0, 32), dtype=np.uint8), np.array(status, dtype=np.uint8), np.array(mc, dtype=np.uint64),
                                len(unparsed), int(unparsed[0]) if len(unparsed) else len(strings))


@functools.lru_cache(maxsize=None)
def shuffled_cases():
    G, vk, ax = account()
    cases = list(case_list()); random.Random(11).shuffle(cases)
    return cases, [s for _, s, _, _ in cases], vk, le32(ax)


# ---- the host half ----------------------------------------------------------------------------------------------------------------------------------
def test_host_path_equals_the_existing_host_calls_put_together():
    cases, strings, vk, ax = shuffled_cases()
    got = records.decrypt_strings(strings, vk, ax, host=True)
    want = composed(strings, vk, ax)
    assert same_found(got, want), differences(got, want)
    by_index = {int(i): k for k, i in enumerate(got.index)}
    for i, (what, _, owned, status) in enumerate(cases):
        assert (i in by_index) == owned, what
        if owned: assert got.status[by_index[i]] == status, (what, got.status[by_index[i]])
    k = lambda what: by_index[[w for w, _, _, _ in cases].index(what)]
    want_mc = {'microcredits private u64': 1500000000000000, 'microcredits private u64, the largest': 2 ** 64 - 1, 'microcredits private u64 behind other private entries': 77, 'microcredits public u64': 123456789012,
               'microcredits constant u64': 2 ** 63 + 5, 'microcredits twice: the last one counts': 6, 'public owner, nonce off the curve, nothing private': 31}
    for what, _, owned, status in cases:
        if owned: assert int(got.microcredits[k(what)]) == want_mc.get(what, 0), what
    assert {0, 1, 2, 8, 9, 17} <= {int(got.offsets[j + 1] - got.offsets[j]) for j in range(len(got)) if got.status[j] == 0}
    for j in np.flatnonzero(got.status == 2): assert not got.fields(j).any() and len(got.fields(j)) in (1, 9)
    for j in np.flatnonzero(got.status == 4): assert len(got.fields(j)) == 0
    for j in np.flatnonzero(got.kind == 1):
        if got.status[j] == 0: assert got.fields(j)[0].tobytes() == ax                                              # a private owner's first plain field is the address x
    assert got.unparsed == 5 and got.first_unparsed == min(i for i, (_, _, owned, _) in enumerate(cases) if not owned and cases[i][0] in ('garbage', 'the empty string', 'a record cut short', 'more than 2^20 characters', 'owner variant 2'))
    # every record alone, and nothing at all
    for i, s in enumerate(strings):
        if len(s) < 5000: assert same_found(records.decrypt_strings([s], vk, ax, host=True), composed([s], vk, ax)), cases[i][0]
    empty = records.decrypt_strings([], vk, ax, host=True)
    assert len(empty) == 0 and empty.offsets.tolist() == [0] and empty.plain.shape == (0, 32) and (empty.unparsed, empty.first_unparsed) == (0, 0)
    assert same_found(records.decrypt_strings([], vk, ax), empty)


def test_only_the_microcredits_entry_is_examined():
    """The one stated difference from RecordPlaintext.microcredits(): record_plaintext refuses a record in which ANY entry does not render, and the composition
    then says 0; decrypt_strings reads the microcredits entry alone.  Everything else of such a record is the composition's."""
    G, vk, ax = account()
    s = encode(payload_of(False, ax, 0, [(b'microcredits', b'\x01\x00\x0c\x00' + struct.pack('<Q', 44)), (b'junk', b'\x01\x07')]))      # a public entry of plaintext variant 7
    got = records.decrypt_strings([s], vk, le32(ax), host=True); want = composed([s], vk, le32(ax))
    assert differences(got, want) == ['microcredits'] and got.microcredits.tolist() == [44] and want.microcredits.tolist() == [0] and got.status.tolist() == [0]


def check_reference_record(host):
    strings = [REF['records']['sdk_foreign'], REF['records']['owner'], 'garbage']
    found = records.decrypt_strings(strings, REF['view_keys']['owner'], REF['addresses']['owner'], host=host)
    assert found.index.tolist() == [1] and found.kind.tolist() == [1] and found.status.tolist() == [0] and found.offsets.tolist() == [0, 2] and (found.unparsed, found.first_unparsed) == (1, 2)
    assert found.microcredits.tolist() == [1500000000000000]                                                         # record_plaintext.rs:126-129 of the reference
    pt = records.RecordCiphertext.from_string(strings[1]).plaintext(found.fields(0), REF['addresses']['owner'])
    assert str(pt) == REF['plaintexts']['owner'] and pt.microcredits() == 1500000000000000
    assert len(records.decrypt_strings(strings, REF['view_keys']['non_owner'], le32(5), host=host)) == 0
    G = account_generator(); vk = ps.view_key_scalar(REF['view_keys']['non_owner'])
    none = records.decrypt_strings(records.RecordBatch.from_strings(strings), vk, le32(ps.ed_mul(G, vk)[0]), host=host)
    assert len(none) == 0 and none.plain.shape == (0, 32) and none.unparsed == 1


def test_the_reference_s_record_on_the_host_path():
    check_reference_record(host=True)


def raw_cases():
    cases, strings, vk, ax = shuffled_cases()
    return [s.encode('latin-1') for s in strings]


def write_cases(path, raw):
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(raw)))
        for b in raw: f.write(struct.pack('<I', len(b))); f.write(b)


def test_device_lane_code_run_on_the_host_equals_record_fields(tmp_path):
    """tests/cpp/records_found_lane_emul.cpp: records_found_lane.h compiled for the CPU over every string of the case list that parses, against
    aleo_mi355x_record_fields: accept and refuse, the count (from the counting walk) and the bytes (from the gathering walk)."""
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, 'records_found_lane_emul')
    path = os.path.join(str(tmp_path), 'cases.bin'); write_cases(path, raw_cases())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ' 0 mismatches' in r.stdout, r.stdout + r.stderr
    accepted, refused = (int(re.search(r'(\d+) %s' % w, r.stdout).group(1)) for w in ('accepted', 'refused'))
    assert accepted >= 30 and refused >= 8, r.stdout                                                                # refused: the eight of the case list, and random entries


def test_host_path_and_lanes_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/records_found_fuzz.cpp, a program of its own built with -fsanitize=address,undefined from the host-only sources (tools/asan_records_found.sh): the
    case list, then mutated strings — bit flips and length bytes pointing past the payload, re-encoded with a valid checksum — and truncations go through the
    parse lane, the two walks and the whole host path.  Any sanitizer report fails the run."""
    path = os.path.join(str(tmp_path), 'cases.bin'); write_cases(path, [b for b in raw_cases() if len(b) < 5000])
    G, vk, ax = account()
    r = subprocess.run([os.path.join(ROOT, 'tools', 'asan_records_found.sh'), str(tmp_path), path, le32(vk).hex(), le32(ax).hex()], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'SANITIZED OK' in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '1000000'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '1000000')


def good_strings():
    cases, strings, vk, ax = shuffled_cases()
    return [s for (what, s, owned, status) in cases if ((status == 0 and 'random bits' not in what) or (not owned and len(s) > 100 and len(s) < 5000 and what not in ('a record cut short', 'owner variant 2')))]


def check_python_mirrors():
    cases, strings, vk, ax = shuffled_cases()
    good = good_strings()
    objects = [records.RecordCiphertext.from_string(s) for s in good]
    want = records.decrypt_owned(objects, vk, ax)                                                                     # the road that does not change
    assert len(want) >= 25 and records.decrypt_owned(good, vk, ax) == want == records.decrypt_owned(records.RecordBatch.from_strings(good), vk, ax)
    total, idx = records.balance(good, vk, ax)
    assert idx == [i for i, _ in want] and total == sum(pt.microcredits() for _, pt in want) and total > 2 ** 64                                         # no wrap at 64 bits
    assert records.balance(records.RecordBatch.from_strings(good), vk, ax) == (total, idx) == records.balance(objects, vk, ax)
    assert records.balance([], vk, ax) == (0, [])
    # what raised, raises: an unparsed string first, then per owned record in order
    for bad, match in (('garbage', 'record_parse'), ([s for w, s, _, _ in cases if w == 'an entry with visibility 3'][0], 'record_fields'),
                       ([s for w, s, _, _ in cases if w == 'public owner, nonce off the curve, a private field'][0], 'record 2 has a nonce that is not on the curve')):
        batch = good[:2] + [bad] + good[2:5]
        with pytest.raises(aleo_amd.AleoMi355xError, match=match) as loop: records.decrypt_owned([records.RecordCiphertext.from_string(t) for t in batch], vk, ax)
        with pytest.raises(aleo_amd.AleoMi355xError, match=match) as direct: records.decrypt_owned(batch, vk, ax)
        assert str(loop.value) == str(direct.value)
    with pytest.raises(aleo_amd.AleoMi355xError, match='record_parse'): records.balance(good[:3] + ['garbage'], vk, ax)
    with pytest.raises(TypeError): records.decrypt_strings(objects, vk, ax)


def test_python_mirrors_on_the_host_path(on_host):
    check_python_mirrors()


def run_cpp_mirror(tmp_path, env):
    """tests/cpp/records_found_test.cpp: decrypt_strings and balance of include/aleo_mi355x.hpp on the reference's strings."""
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']] * 25 + ['garbage']
    r = bs.run_cpp_mirror(tmp_path, 'records_found_test', [REF['view_keys']['owner'], REF['addresses']['owner'], REF['plaintexts']['owner'], '1500000000000000'] + strings, env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '1000000', 'ALEO_MI355X_MIN_DECRYPT': '1000000'})


def test_bad_arguments_are_refused_as_records_scan_strings_refuses_them():
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    GOOD = REF['records']['owner']
    text = (GOOD + 'garbage').encode(); tp = ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p)
    off = lambda *v: np.array(v, dtype=np.uint64)
    vk = np.frombuffer(le32(1), dtype=np.uint8); ax = np.frombuffer(le32(5), dtype=np.uint8); bad_vk = np.frombuffer(le32(L_ORDER), dtype=np.uint8); bad_ax = np.frombuffer(le32(R), dtype=np.uint8)
    flags = np.zeros(2, dtype=np.uint8)
    def both(call_found, call_scan):
        """The same status and the same message from the new call and from records_scan_strings."""
        rc = call_scan(); msg = L.aleo_mi355x_last_error()
        out = ctypes.c_void_p(1)
        assert call_found(ctypes.byref(out)) == rc != 0 and L.aleo_mi355x_last_error() == msg and out.value is None
        return msg
    for f, g in ((L.aleo_mi355x_records_decrypt_strings_host, L.aleo_mi355x_records_scan_strings_host), (L.aleo_mi355x_records_decrypt_strings, L.aleo_mi355x_records_scan_strings)):
        out = ctypes.c_void_p()
        assert f(ctypes.byref(out), tp, p(off(0, len(GOOD), len(text))), 2, p(vk), p(ax)) == 0 and L.aleo_mi355x_found_count(out) == 0 and L.aleo_mi355x_found_unparsed(out) == 1 and L.aleo_mi355x_found_first_unparsed(out) == 1
        L.aleo_mi355x_found_free(out)
        assert b'offsets[0]' in both(lambda o: f(o, tp, p(off(1, len(GOOD), len(text))), 2, p(vk), p(ax)), lambda: g(p(flags), None, None, tp, p(off(1, len(GOOD), len(text))), 2, p(vk), p(ax), 1))
        assert b'decrease' in both(lambda o: f(o, tp, p(off(0, len(text), len(GOOD))), 2, p(vk), p(ax)), lambda: g(p(flags), None, None, tp, p(off(0, len(text), len(GOOD))), 2, p(vk), p(ax), 1))
        assert b'null' in both(lambda o: f(o, None, p(off(0, 1, 2)), 2, p(vk), p(ax)), lambda: g(p(flags), None, None, None, p(off(0, 1, 2)), 2, p(vk), p(ax), 1))
        assert b'null' in both(lambda o: f(o, tp, None, 2, p(vk), p(ax)), lambda: g(p(flags), None, None, tp, None, 2, p(vk), p(ax), 1))
        assert b'null' in both(lambda o: f(o, tp, p(off(0, 1, 2)), 2, None, p(ax)), lambda: g(p(flags), None, None, tp, p(off(0, 1, 2)), 2, None, p(ax), 1))
        assert b'key 0' in both(lambda o: f(o, tp, p(off(0, 1, 2)), 2, p(bad_vk), p(ax)), lambda: g(p(flags), None, None, tp, p(off(0, 1, 2)), 2, p(bad_vk), p(ax), 1))
        assert b'key 0' in both(lambda o: f(o, tp, p(off(0, 1, 2)), 2, p(vk), p(bad_ax)), lambda: g(p(flags), None, None, tp, p(off(0, 1, 2)), 2, p(vk), p(bad_ax), 1))
        assert f(None, tp, p(off(0, 1, 2)), 2, p(vk), p(ax)) != 0
        out = ctypes.c_void_p()
        assert f(ctypes.byref(out), None, None, 0, p(vk), p(ax)) == 0 and out.value and L.aleo_mi355x_found_count(out) == 0 and L.aleo_mi355x_found_fields(out) == 0
        L.aleo_mi355x_found_free(out); L.aleo_mi355x_found_free(None)


NEW_KERNELS = ('k_found_count', 'k_found_offsets', 'k_found_gather', 'k_found_microcredits')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_found_kernels_are_gfx950_and_have_no_scratch():
    import code_object as co
    asm, blocks = co.compile_unit('records_found')
    assert len(blocks) == len(NEW_KERNELS)                                                                          # these four and no other
    for kernel in NEW_KERNELS:
        meta = co.block_of(blocks, kernel)
        print(co.registers(kernel, meta, ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')))
        assert co.field(meta, 'private_segment_fixed_size') == 0 and co.field(meta, 'vgpr_spill_count') == 0 and co.field(meta, 'sgpr_spill_count') == 0


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0')
    for name in ('ALEO_MI355X_SCAN_KEYS_PER_LANE', 'ALEO_MI355X_SCAN_CHUNK_CHARS', 'ALEO_MI355X_DECRYPT_CHUNK_FIELDS'): monkeypatch.delenv(name, raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0
    return monkeypatch


@functools.lru_cache(maxsize=None)
def pools():
    """(owned strings of every status, foreign strings) to lay patterns out of: the case list's, and random records of the reference's shape."""
    cases, strings, vk, ax = shuffled_cases(); rng = random.Random(5)
    owned = [s for _, s, o, _ in cases if o]
    foreign = [s for _, s, o, _ in cases if not o and len(s) < 5000] + [encode(reference_sized(rng)) for _ in range(200)]
    return owned, foreign


def pattern(n, which, seed=0):
    owned, foreign = pools(); rng = random.Random(1000 * n + seed)
    mine = {'nobody': lambda i: False, 'everybody': lambda i: True, 'last': lambda i: i == n - 1, 'first lane of every block': lambda i: i % 256 == 0,
            'a random tenth': lambda i: rng.random() < 0.1}[which]
    return [owned[(i * 7 + i // 256) % len(owned)] if mine(i) else foreign[rng.randrange(len(foreign))] for i in range(n)]


def check_kernel_equals_host(strings, vk, ax):
    batch = records.RecordBatch.from_strings(strings)
    want = records.decrypt_strings(batch, vk, ax, host=True)
    got = records.decrypt_strings(batch, vk, ax)
    assert same_found(got, want), differences(got, want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 4099])
def test_kernel_equals_the_host_path_at_block_and_wave_edges(on_kernel, n):
    cases, _, vk, ax = shuffled_cases()
    for which in ('nobody', 'everybody', 'last', 'first lane of every block', 'a random tenth'):
        want = check_kernel_equals_host(pattern(n, which), vk, ax)
        if which == 'nobody': assert len(want) == 0
        if which == 'everybody': assert len(want) == n and (n < 64 or {0, 2, 4} <= set(want.status.tolist()))
        if which == 'last': assert want.index.tolist() == [n - 1]
        if which == 'first lane of every block': assert want.index.tolist() == list(range(0, n, 256))


@pytest.mark.gpu
def test_kernel_chunks_continue_indices_and_offsets(on_kernel):
    """n = 4099 in at least three chunks of characters, one of them without an owned record, and several decrypt launches inside a chunk: the bytes depend on neither."""
    cases, _, vk, ax = shuffled_cases()
    owned, foreign = pools(); rng = random.Random(8)
    strings = pattern(4099, 'a random tenth', seed=1)
    for i in range(1500, 2600): strings[i] = foreign[rng.randrange(len(foreign))]                                   # the middle of the batch: nobody's
    batch = records.RecordBatch.from_strings(strings)
    want = records.decrypt_strings(batch, vk, ax, host=True)
    assert len(want) > 200 and int(want.offsets[-1]) > 600 and not ((want.index >= 1500) & (want.index < 2600)).any()
    assert same_found(records.decrypt_strings(batch, vk, ax), want)
    lens = np.diff(batch.offsets.astype(np.int64)); total = int(lens.sum())
    for chars, fields in ((total // 5, None), (total // 5, '64'), (None, '64'), (total // 3, '8')):
        if chars: on_kernel.setenv('ALEO_MI355X_SCAN_CHUNK_CHARS', str(chars))
        else: on_kernel.delenv('ALEO_MI355X_SCAN_CHUNK_CHARS', raising=False)
        if fields: on_kernel.setenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', fields)
        else: on_kernel.delenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', raising=False)
        got = records.decrypt_strings(batch, vk, ax)
        assert same_found(got, want), (chars, fields, differences(got, want))
    # the chunk of the middle fifth holds no owned record
    cum = np.cumsum(lens); first, last = int(np.searchsorted(cum, 2 * (total // 5))), int(np.searchsorted(cum, 3 * (total // 5)))
    assert 1500 < first and last < 2600


@pytest.mark.gpu
def test_kernel_walks_from_global_memory_where_a_block_s_strings_exceed_its_lds(on_kernel):
    cases, _, vk, ax = shuffled_cases(); G, _, ax_int = account()
    owned, foreign = pools(); rng = random.Random(6)
    long_foreign = lambda k: encode(payload_of(True, rng.randrange(R), rng.randrange(R), [(b'data', bytes(rng.randrange(256) for _ in range(k)))]))
    long_owned = [Built(G, vk, ax_int, i % 2 == 0, [('pad', 2, string_of_fields(8 + i)), ('microcredits', 2, ('lit', 12, 10 + i))], 800 + i).string for i in range(3)]
    strings = [long_owned[i % 3] if i % 50 == 7 else owned[i % len(owned)] if i % 9 == 0 else long_foreign(300) for i in range(256)] + pattern(300, 'a random tenth')
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])])
    spans = [int(off[min(b + 256, len(strings))] - (off[b] & ~15)) for b in range(0, len(strings), 256)]
    assert spans[0] > 65536 and spans[1] < 65536 and spans[2] < 65536
    want = check_kernel_equals_host(strings, vk, ax)
    assert (want.index < 256).sum() >= 30 and (want.index >= 256).sum() >= 10 and int(want.microcredits.max()) >= 12


@pytest.mark.gpu
def test_kernel_mixed_lengths_and_bad_records_in_one_wave(on_kernel):
    """Records of 0, 2 and 17 fields interleaved in one wave, a malformed and a refused record beside good ones: a bad record's rows are zero or absent and its
    neighbours' rows are what they are without it."""
    cases, _, vk, ax = shuffled_cases()
    by = {w: s for w, s, _, _ in cases}
    cycle = [by['public owner, 0 private fields'], by['private owner, 2 private fields'], by['private owner, 17 private fields']]
    strings = [cycle[i % 3] for i in range(64)]
    clean = check_kernel_equals_host(strings, vk, ax)
    assert np.diff(clean.offsets).tolist() == [(0, 2, 17)[i % 3] for i in range(64)] and not clean.status.any()
    strings[10] = by['public owner, nonce off the curve, 9 private fields']; strings[11] = by['an entry with visibility 3']; strings[40] = by['a private field = r']
    strings[41] = by['public owner, nonce off the curve, a private field']
    want = check_kernel_equals_host(strings, vk, ax)
    assert want.status[[10, 11, 40, 41]].tolist() == [2, 4, 4, 2] and want.status.sum() == 12
    assert len(want.fields(10)) == 9 and not want.fields(10).any() and len(want.fields(11)) == 0 and len(want.fields(40)) == 0 and len(want.fields(41)) == 1 and not want.fields(41).any()
    for j in range(64):
        if j not in (10, 11, 40, 41): assert want.fields(j).tobytes() == clean.fields(j).tobytes() and want.rvk[j].tobytes() == clean.rvk[j].tobytes(), j


@pytest.mark.gpu
def test_kernel_reference_record_and_mirrors(on_kernel, tmp_path):
    check_reference_record(host=False)
    check_python_mirrors()
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '0', 'ALEO_MI355X_MIN_DECRYPT': '0'})
