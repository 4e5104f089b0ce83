"""Unspent records from the strings alone: the commitments of owned records computed by the library (aleo_mi355x_records_commitments_found, _unspent_named[_many]
and their _host forms; found_commitments, unspent_named[_many] and FoundRecords.commitments in aleo_amd/records.py; the same in include/aleo_mi355x.hpp).

Three layers, each checked against the one before: the reference's data pins the host path (the transaction output's id, the serial number of
wasm/src/record/record_plaintext.rs:131-140); the host path equals the composition of the calls the library already had (record_commitment per record, then
unspent_strings_many), written out below; the host path, byte for byte, checks the device lane — emulated on the CPU, plain and under the sanitizers, here, and
on the GPU in the second half (ALEO_MI355X_MIN_RECORDS=0, MIN_SERIALS=0, MIN_COMMITMENTS=0).  No test reads the reference tree."""
import ctypes, functools, json, os, random, re, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records
from oracle import poseidon as ps
import serial_ref as S
from test_records import ENC_DOMAIN, R, L_ORDER
from test_records_strings import encode, payload_of
from test_records_decrypt import Built, TWO_LEVELS, account, string_of_fields, plaintext_bytes
from test_records_found import private_entry
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32

ACC = json.load(open(os.path.join(HERE, 'golden', 'reference_account.json')))
REC = json.load(open(os.path.join(HERE, 'golden', 'reference_records.json')))
SER = json.load(open(os.path.join(HERE, 'golden', 'reference_serial.json')))
TX, SN = SER['transaction_output'], SER['serial_number']
PER = 1044                                                                           # message bits per BHP1024 iteration
# 8 (|program name| + 4 + |record name|) = 0, 2, 1 (mod 3): the stream behind the pre-summed names starts with 0, 2 and 1 bits in hand
NAMES = [('credits.aleo', 'credits'), ('credit_s.aleo', 'credits'), ('credit_s.aleo', 'credit_s')]


def field(s: str) -> int: assert s.endswith('field'); return int(s[:-5])
def ints(a) -> list: return [int.from_bytes(r.tobytes(), 'little') for r in a]
def same(a, b): return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a.arrays(), b.arrays()))


def reference_account():
    """The reference's serial-number test signs with a key that is not the record's owner's: its sk_sig with the owner's view key and address."""
    return records.Account(None, records.Account.from_private_key(SN['private_key']).sk_sig, records.view_key_bytes(REC['view_keys']['owner']), records.address_x_bytes(REC['addresses']['owner']))


# ---- the records ------------------------------------------------------------------------------------------------------------------------------------
def raw_record(owner_private, entries, seed):
    """A record of the account of tests/test_records_decrypt.py from PLAIN FIELDS: entries (name, visibility, a list of plain fields | a value for plaintext_bytes |
    bytes as they stand).  What Built does, without going through values, so that an entry can hold fields no value encodes to."""
    G, vk, ax = account(); rng = random.Random(seed)
    N = ps.ed_mul(G, rng.randrange(1, L_ORDER)); rvk = ps.ed_mul(N, vk)[0]
    plain = ([ax] if owner_private else []) + [f for _, vis, body in entries if vis == 2 for f in body]
    rnd = ps.hash_many_psd8([ENC_DOMAIN, rvk], len(plain)) if plain else []
    cipher = [(p + r) % R for p, r in zip(plain, rnd)]
    at, out = (1 if owner_private else 0), []
    for name, vis, body in entries:
        if vis == 2: out.append((name.encode(), private_entry(cipher[at:at + len(body)]))); at += len(body)
        else: out.append((name.encode(), bytes([vis]) + (body if isinstance(body, bytes) else plaintext_bytes(body))))
    return encode(payload_of(owner_private, cipher[0] if owner_private else ax, N[0], out))


@functools.lru_cache(maxsize=None)
def shapes():
    """[(what, string, routed to the host, bits of the message under NAMES[0] or None)]: every shape the lane can go wrong at.  All are the account's."""
    G, vk, ax = account(); out = []; seed = [900]
    def built(what, private, entries, routed=False, bits=None): seed[0] += 1; out.append((what, Built(G, vk, ax, private, entries, seed[0]).string, routed, bits))
    def raw(what, private, entries, routed=False): seed[0] += 1; out.append((what, raw_record(private, entries, seed[0]), routed, None))
    for m in (0, 1, 2, 9, 17):
        built('private owner, %d private fields' % m, True, [('pad', 2, string_of_fields(m))] if m else [])
        built('public owner, %d private fields' % m, False, [('pad', 2, string_of_fields(m))] if m else [])
    built('a private struct entry', True, [('s', 2, TWO_LEVELS)])
    raw('two fields, the last one zero: the terminus sits in the first', True, [('v', 2, [(1 << 40) | 5, 0])])
    raw('three fields, the last one zero, the terminus is bit 251 of the second', False, [('v', 2, [R - 1, 1 << 251, 0])])
    raw('the terminus alone: a value of no bits', True, [('v', 2, [1])])
    raw('no terminus bit: one zero field', True, [('v', 2, [0])])
    raw('no terminus bit: only the bit 252 the data bits leave out', True, [('ok', 2, [3]), ('v', 2, [1 << 252, 0])])
    raw('an entry of no fields', True, [('v', 2, [])])
    built('names of 1 and 31 characters', True, [('a', 2, ('lit', 9, 7)), ('b' * 31, 2, ('lit', 1, True)), ('C', 2, ('lit', 12, 5)), ('d_' * 15 + 'e', 2, ('lit', 2, 99))])
    built('a constant entry', True, [('microcredits', 2, ('lit', 12, 77)), ('memo', 0, ('lit', 15, 'hello'))], routed=True)
    built('a public entry', False, [('memo', 1, ('lit', 12, 5)), ('s', 2, TWO_LEVELS)], routed=True)
    raw('a public entry that does not parse (literal type 99)', True, [('v', 1, b'\x00\x63\x00\x01')], routed=True)
    # the iteration boundaries under NAMES[0] (18 name bytes): 8 x 18 + 539 + per entry 8 |name| + 2 + its bits; a boolean's 27, a u8's 34, a string's 26 + 8 L
    built('exactly per bits', True, [('f' * 6, 2, ('lit', 1, True)), ('g' * 31, 2, ('lit', 9, 200))], bits=PER)
    built('per + 1 bits', False, [('f' * 7, 2, ('lit', 1, False)), ('g' * 31, 2, ('lit', 1, True))], bits=PER + 1)
    built('2 per bits', True, [('f', 2, ('lit', 1, True)), ('g', 2, ('lit', 9, 1)), ('h', 2, ('lit', 15, 'x' * 161))], bits=2 * PER)
    built('2 per + 1 bits', True, [('f', 2, ('lit', 1, True)), ('g', 2, ('lit', 1, True)), ('h', 2, ('lit', 9, 255)), ('i', 2, ('lit', 15, 'y' * 100)), ('j', 2, ('lit', 15, 'z' * 52))], bits=2 * PER + 1)
    return out


def strings_of(cases): return [s for _, s, _, _ in cases]


def test_the_chosen_shapes_have_the_lengths_they_are_chosen_for():
    """The restatement's record_bits (tests/serial_ref.py) on the boundary shapes; the record of nine private fields takes three iterations."""
    G, vk, ax = account()
    bits = lambda s: 8 * 18 + len(S.record_bits(s, S.record_decrypt_fields(s, vk)))
    for what, s, _, want in shapes():
        if want is not None: assert bits(s) == want, what
    nine = [s for what, s, _, _ in shapes() if what == 'private owner, 9 private fields'][0]
    assert 2 * PER < bits(nine) <= 3 * PER


def accounts(K):
    """K accounts over the same strings: the account of the built records under K different sk_sig (every one owns them all, with other serial numbers), the second
    of three or more a stranger who owns nothing."""
    G, vk, ax = account(); rng = random.Random(4242)
    out = [records.Account(None, le32(rng.randrange(1, L_ORDER)), le32(vk), le32(ax)) for _ in range(K)]
    if K >= 3: other = 0x77777777777777777777 | 1; out[1] = records.Account(None, out[1].sk_sig, le32(other), le32(ps.ed_mul(G, other)[0]))
    return out


# ---- 1: pins ------------------------------------------------------------------------------------------------------------------------------------------
def test_pin_the_transaction_output_s_id_through_the_host_call():
    a = ACC['accounts'][2]
    found = records.decrypt_strings([TX['value']], a['view_key'], a['address'], host=True, keep=True)
    cm, flags = records.found_commitments([TX['value']], found, TX['program_id'], TX['record_name'], host=True)
    assert flags.tolist() == [0] and ints(cm) == [field(TX['id'])]


def test_pin_the_reference_s_serial_number_and_the_spent_check_through_the_host_call():
    strings = [REC['records']['owner'], REC['records']['sdk_foreign'], REC['records']['owner']]
    got = records.unspent_named(strings, SN['program_id'], SN['record_name'], reference_account(), host=True)
    assert got.index.tolist() == [0, 2] and got.owned == 2 and ['%dfield' % v for v in ints(got.serials)] == [SN['expected']] * 2
    assert got.microcredits.tolist() == [1500000000000000] * 2 and got.commitments.shape == (2, 32)
    none = records.unspent_named(strings, SN['program_id'], SN['record_name'], reference_account(), spent=[le32(field(SN['expected']))], host=True)
    assert len(none) == 0 and none.owned == 2 and none.commitments.shape == (0, 32) and none.serials.shape == (0, 32)


# ---- 2: the host path equals the composition of the existing calls ---------------------------------------------------------------------------------------
def composed_commitments(strings, found, program_id, record_name):
    """record_commitment per record; a record whose status is not 0 gets its status and a zero row, a refused one 4."""
    cm, flags = np.zeros((len(found), 32), dtype=np.uint8), np.zeros(len(found), dtype=np.uint8)
    for k, i in enumerate(found.index.tolist()):
        if found.status[k]: flags[k] = found.status[k]; continue
        f = found.fields(k)
        try: cm[k] = np.frombuffer(records.record_commitment(strings[i], f if len(f) else np.zeros((0, 32), dtype=np.uint8), program_id, record_name), dtype=np.uint8)
        except aleo_amd.AleoMi355xError: flags[k] = 4
    return cm, flags


def composed_unspent(strings, accts, spent, program_id, record_name):
    """Per account: decrypt_strings, the commitments above scattered to rows of all strings, unspent_strings — minus the records whose commitment is refused."""
    out = []
    for a in accts:
        found = records.decrypt_strings(strings, a.view_key, a.address_x, host=True)
        cm, flags = composed_commitments(strings, found, program_id, record_name)
        rows = np.zeros((len(strings), 32), dtype=np.uint8); rows[found.index.astype(np.int64)] = cm
        u = records.unspent_strings(strings, rows, a, spent, host=True)
        refused = set(found.index[flags != 0].tolist())
        keep = [k for k, i in enumerate(u.index.tolist()) if i not in refused]
        out.append((u, keep, rows))
    return out


def check_against_composition(got, want, keep, rows):
    assert got.owned == want.owned and got.index.tolist() == want.index[keep].tolist()
    for name in ('kind', 'rvk', 'status', 'microcredits', 'serials'): assert getattr(got, name).tobytes() == getattr(want, name)[keep].tobytes(), name
    assert got.commitments.tobytes() == rows[got.index.astype(np.int64)].tobytes()
    assert [got.fields(k).tobytes() for k in range(len(got))] == [want.fields(k).tobytes() for k in keep]


@pytest.mark.parametrize('names', NAMES)
def test_commitments_found_host_equals_record_commitment_per_record(names):
    G, vk, ax = account(); strings = strings_of(shapes())
    found = records.decrypt_strings(strings, vk, ax, host=True, keep=True)
    assert len(found) == len(strings) and not found.status.any()
    cm, flags = records.found_commitments(strings, found, *names, host=True)
    want_cm, want_flags = composed_commitments(strings, found, *names)
    assert flags.tolist() == want_flags.tolist() and cm.tobytes() == want_cm.tobytes()
    refused = [what for (what, _, _, _), f in zip(shapes(), flags) if f]
    assert sorted(refused) == sorted(['no terminus bit: one zero field', 'no terminus bit: only the bit 252 the data bits leave out', 'an entry of no fields', 'a public entry that does not parse (literal type 99)'])
    assert not cm[flags != 0].any() and len({r.tobytes() for r in cm[flags == 0]}) == int((flags == 0).sum())


@pytest.mark.parametrize('K', [1, 3, 8])
def test_unspent_named_many_host_equals_unspent_strings_many_fed_those_commitments(K):
    strings = strings_of(shapes()) + [REC['records']['owner']]; accts = accounts(K)
    free = records.unspent_named_many(strings, *NAMES[0], accts, host=True)
    spent = [free[0].serials[1].tobytes(), le32(5), free[-1].serials[3].tobytes()]
    for sp, got in (((), free), (spent, records.unspent_named_many(strings, *NAMES[0], accts, spent, host=True))):
        for g, (want, keep, rows) in zip(got, composed_unspent(strings, accts, sp, *NAMES[0])): check_against_composition(g, want, keep, rows)
    assert len(free[0]) == len(shapes()) - 4 and (K < 3 or len(free[1]) == 0)


# ---- 3: the device lane, emulated on the host ---------------------------------------------------------------------------------------------------------
def write_lane_cases(path, names):
    G, vk, ax = account(); cases = shapes(); strings = strings_of(cases)
    found = records.decrypt_strings(strings, vk, ax, host=True, keep=True)
    cm, flags = records.found_commitments(strings, found, *names, host=True)
    with open(path, 'wb') as f:
        for text in names: f.write(struct.pack('<I', len(text)) + text.encode())
        f.write(struct.pack('<I', len(strings)))
        for k, (what, s, routed, _) in enumerate(cases):
            f.write(struct.pack('<I', len(s)) + s.encode() + struct.pack('<iI', int(found.kind[k]), len(found.fields(k))) + found.fields(k).tobytes())
            f.write(bytes([8 if routed else int(flags[k])]) + cm[k].tobytes())
    return len(strings), int((flags == 0).sum())


@pytest.mark.parametrize('sanitized', [False, True])
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path, sanitized):
    """tests/cpp/records_commit_lane_emul.cpp: records_commit_lane.h compiled for the CPU over the checked restatement of fr29.h, a program of its own, once plain and
    once with the address and undefined-behaviour sanitizers, on every shape under the three name pairs; the rows it is held against are the library's host path's."""
    exe = bs.build_lane_emul(tmp_path, 'records_commit_lane_emul', sanitized=sanitized, flags=())
    for names in NAMES:
        path = os.path.join(str(tmp_path), 'cases.bin'); n, computed = write_lane_cases(path, names)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and '%d records, ' % n in r.stdout and ' 0 mismatches, 0 reads past an end, 0 limb-rule violations' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
        assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
        m = re.search(r'(\d+) computed, (\d+) refused, (\d+) routed.*iterations 1: (\d+), 2: (\d+), 3: (\d+), other: (\d+)', r.stdout)
        got = [int(v) for v in m.groups()]
        assert got[0] == computed - 2 and got[1] == 3 and got[2] == 3 and min(got[3:]) >= 1, r.stdout[-400:]      # two of the routed records compute on the host
        if names == NAMES[0]:
            for want in (PER, PER + 1, 2 * PER, 2 * PER + 1): assert ': %d bits\n' % want in r.stdout, want


# ---- 4: refusals and edges ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_edges():
    G, vk, ax = account(); strings = strings_of(shapes())[:4]; acct = accounts(1)[0]
    found = records.decrypt_strings(strings, vk, ax, host=True, keep=True)
    for host in (True, False):                                                                   # four records: below min_commitments, the call stays on the host
        for e in SER['errors']:
            with pytest.raises(aleo_amd.AleoMi355xError) as err: records.found_commitments(strings, found, e['program_id'], e['record_name'], host=host)
            assert str(err.value) == e['message'], e['source']
            with pytest.raises(aleo_amd.AleoMi355xError) as err: records.unspent_named(strings, e['program_id'], e['record_name'], acct, host=True)
            assert str(err.value) == e['message'], e['source']
        with pytest.raises(aleo_amd.AleoMi355xError): records.found_commitments(strings[:3], found, *NAMES[0], host=host)      # a found_index not below n
    with pytest.raises(aleo_amd.AleoMi355xError): records.unspent_named(strings, *NAMES[0], records.Account(None, le32(L_ORDER), acct.view_key, acct.address_x), host=True)
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    b = records.RecordBatch.from_strings(strings); text = ctypes.cast(ctypes.c_char_p(b.text), ctypes.c_void_p)
    cm = np.zeros((4, 32), dtype=np.uint8); fl = np.zeros(4, dtype=np.uint8)
    for f in (L.aleo_mi355x_records_commitments_found, L.aleo_mi355x_records_commitments_found_host):
        assert f(p(cm), p(fl), None, text, p(b.offsets), 4, b'credits.aleo', b'credits') != 0
        assert f(None, p(fl), found._native, text, p(b.offsets), 4, b'credits.aleo', b'credits') != 0 and f(p(cm), None, found._native, text, p(b.offsets), 4, b'credits.aleo', b'credits') != 0
        assert f(p(cm), p(fl), found._native, text, p(b.offsets), 4, None, b'credits') != 0 and L.aleo_mi355x_last_error().decode() == 'Invalid ProgramID specified'
        assert f(p(cm), p(fl), found._native, text, p(b.offsets), 4, b'credits.aleo', None) != 0 and L.aleo_mi355x_last_error().decode() == 'Invalid Identifier specified for record'
        assert f(p(cm), p(fl), found._native, text, None, 4, b'credits.aleo', b'credits') != 0
    out = ctypes.c_void_p(); sk, v, a = (np.frombuffer(x, dtype=np.uint8) for x in (acct.sk_sig, acct.view_key, acct.address_x))
    for f in (L.aleo_mi355x_records_unspent_named, L.aleo_mi355x_records_unspent_named_host):
        assert f(None, text, p(b.offsets), 4, b'credits.aleo', b'credits', p(sk), p(v), p(a), None, 0) != 0
        assert f(ctypes.byref(out), text, p(b.offsets), 4, b'credits.aleo', b'credits', None, p(v), p(a), None, 0) != 0 and not out.value
        assert f(ctypes.byref(out), text, p(b.offsets), 4, b'credits.aleo', b'credits', p(sk), p(v), p(a), None, 1) != 0 and not out.value
    # n = 0, and a result that holds nothing
    for host in (True, False):
        empty = records.unspent_named([], *NAMES[0], acct, host=host)
        assert len(empty) == 0 and empty.owned == 0 and empty.commitments.shape == (0, 32)
        nothing = records.decrypt_strings([REC['records']['sdk_foreign']], vk, ax, host=True, keep=True)
        cm0, fl0 = records.found_commitments([REC['records']['sdk_foreign']], nothing, *NAMES[0], host=host)
        assert len(nothing) == 0 and cm0.shape == (0, 32) and fl0.shape == (0,)
    # found_commitments is NULL on the results of the older calls
    assert found.commitments is None and L.aleo_mi355x_found_commitments(found._native) is None and L.aleo_mi355x_found_commitments(None) is None
    rows = np.zeros((4, 32), dtype=np.uint8)
    assert records.unspent_strings(strings, rows, acct, host=True).commitments is None and records.decrypt_strings_many(strings, [vk], [le32(ax)], host=True)[0].commitments is None
    # a record whose status is not 0 gets its status as its flag
    bad = strings + [encode(payload_of(False, ax, 0x1234, [(b'v', b'\x03\x00')]))]
    fb = records.decrypt_strings(bad, vk, ax, host=True, keep=True)
    cmb, flb = records.found_commitments(bad, fb, *NAMES[0], host=True)
    assert fb.status.tolist() == [0, 0, 0, 0, 4] and flb.tolist() == [0, 0, 0, 0, 4] and not cmb[4].any() and cmb[:4].any(axis=1).all()


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_commitments', 'ALEO_MI355X_MIN_COMMITMENTS') == (32, 5, 32)


# ---- 5: the code object -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_commit_kernel_code_object_is_gfx950_and_has_no_scratch():
    assert bs.scratch_and_spills('records_commit', ['k_records_commit']) == (1, {'k_records_commit': (0, 0, 0)})      # this one and no other


# ---- 6: the C++ mirror ----------------------------------------------------------------------------------------------------------------------------------
def run_cpp_mirror(tmp_path, env):
    """tests/cpp/records_commit_test.cpp: found_commitments, unspent_named and unspent_named_many of include/aleo_mi355x.hpp on the reference's record, 70 copies among foreign ones."""
    strings = [REC['records']['owner'], REC['records']['sdk_foreign']] * 70
    plain = S.record_decrypt_fields(REC['records']['owner'], ps.view_key_scalar(REC['view_keys']['owner']))
    cm = S.record_commitment(REC['records']['owner'], plain, SN['program_id'], SN['record_name'])
    r = bs.run_cpp_mirror(tmp_path, 'records_commit_test', [SN['private_key'], REC['view_keys']['owner'], REC['addresses']['owner'], SN['program_id'], SN['record_name'], le32(cm).hex(), le32(field(SN['expected'])).hex()] + strings, env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '1000000', 'ALEO_MI355X_MIN_DECRYPT': '1000000', 'ALEO_MI355X_MIN_COMMITMENTS': '1000000'})


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    for name in ('RECORDS', 'DECRYPT', 'SERIALS', 'COMMITMENTS'): monkeypatch.setenv('ALEO_MI355X_MIN_' + name, '0')
    for name in ('ALEO_MI355X_SCAN_KEYS_PER_LANE', 'ALEO_MI355X_SCAN_CHUNK_CHARS', 'ALEO_MI355X_DECRYPT_CHUNK_FIELDS', 'ALEO_MI355X_SERIAL_CHUNK', 'ALEO_MI355X_COMMIT_CHUNK'): monkeypatch.delenv(name, raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0 and int(aleo_amd.lib().aleo_mi355x_min_serials()) == 0 and int(aleo_amd.lib().aleo_mi355x_min_commitments()) == 0
    return monkeypatch


@functools.lru_cache(maxsize=None)
def pool():
    """The shapes and the reference's own record (a stranger's), which tiles of any length are cut from: every third string is not the account's."""
    mine = strings_of(shapes())
    return mine, [REC['records']['owner'], REC['records']['sdk']]


def tiled(owned, seed=0):
    """Strings of which the account owns exactly `owned`, foreign ones in between; the shapes in an order that depends on the seed."""
    mine, foreign = pool(); rng = random.Random(seed); order = list(range(len(mine))); rng.shuffle(order)
    out = []
    for k in range(owned):
        out.append(mine[order[k % len(order)]])
        if k % 2: out.append(foreign[k % len(foreign)])
    return out


def check_kernels_equal_host(strings, K, spent=(), names=NAMES[0]):
    accts = accounts(K)
    got = records.unspent_named_many(strings, *names, accts, spent)
    want = records.unspent_named_many(strings, *names, accts, spent, host=True)
    for g, w in zip(got, want):
        assert same(g, w) and (g.unparsed, g.first_unparsed, g.owned) == (w.unparsed, w.first_unparsed, w.owned)
        assert g.serials.tobytes() == w.serials.tobytes() and g.commitments.tobytes() == w.commitments.tobytes()
    G, vk, ax = account()
    found = records.decrypt_strings(strings, vk, ax, keep=True)
    cm, flags = records.found_commitments(strings, found, *names)
    want_cm, want_flags = records.found_commitments(strings, found, *names, host=True)
    assert flags.tolist() == want_flags.tolist() and cm.tobytes() == want_cm.tobytes()
    return got, cm, flags


@pytest.mark.gpu
@pytest.mark.parametrize('owned,K', [(n, K) for n in (1, 63, 64, 65, 255, 256, 257) for K in (1, 3, 8)])
def test_kernels_equal_the_host_path_at_wave_and_block_edges(on_kernel, owned, K):
    got, cm, flags = check_kernels_equal_host(tiled(owned, seed=owned), K)
    assert len(flags) == owned and got[0].owned == owned


@pytest.mark.gpu
@pytest.mark.parametrize('names', NAMES)
def test_kernel_mixed_shapes_in_one_wave(on_kernel, names):
    """Every shape once, side by side in one wave: one to five iterations, refused records and records routed to the host."""
    strings = strings_of(shapes()); assert len(strings) <= 64
    got, cm, flags = check_kernels_equal_host(strings, 1, names=names)
    assert sorted(flags.tolist()) == [0] * (len(strings) - 4) + [4] * 4 and len(got[0]) == len(strings) - 4


@pytest.mark.gpu
def test_kernel_launches_of_one_wave_continue_ranks_and_offsets(on_kernel):
    whole = check_kernels_equal_host(tiled(200, seed=3), 3)
    on_kernel.setenv('ALEO_MI355X_COMMIT_CHUNK', '64')
    cut = check_kernels_equal_host(tiled(200, seed=3), 3)
    assert cut[1].tobytes() == whole[1].tobytes() and all(a.commitments.tobytes() == b.commitments.tobytes() and same(a, b) for a, b in zip(cut[0], whole[0]))


@pytest.mark.gpu
def test_both_sides_of_min_commitments_give_the_same_bytes(on_kernel):
    strings = tiled(100, seed=5)
    device = check_kernels_equal_host(strings, 3)
    on_kernel.setenv('ALEO_MI355X_MIN_COMMITMENTS', '1000')                                      # the rest of the flow stays on the device
    host_rows = check_kernels_equal_host(strings, 3)
    assert host_rows[1].tobytes() == device[1].tobytes() and all(a.commitments.tobytes() == b.commitments.tobytes() and a.serials.tobytes() == b.serials.tobytes() for a, b in zip(host_rows[0], device[0]))


@pytest.mark.gpu
def test_kernel_gives_the_reference_s_id_and_serial_number_in_every_lane(on_kernel):
    got = records.unspent_named([REC['records']['owner']] * 65, SN['program_id'], SN['record_name'], reference_account())
    plain = S.record_decrypt_fields(REC['records']['owner'], ps.view_key_scalar(REC['view_keys']['owner']))
    assert len(got) == 65 and ints(got.commitments) == [S.record_commitment(REC['records']['owner'], plain, SN['program_id'], SN['record_name'])] * 65
    assert ['%dfield' % v for v in ints(got.serials)] == [SN['expected']] * 65
    a = ACC['accounts'][2]
    found = records.decrypt_strings([TX['value']] * 65, a['view_key'], a['address'], keep=True)
    cm, flags = records.found_commitments([TX['value']] * 65, found, TX['program_id'], TX['record_name'])
    assert not flags.any() and ints(cm) == [field(TX['id'])] * 65


@pytest.mark.gpu
def test_kernel_spent_sets_empty_all_and_some(on_kernel):
    strings = tiled(70, seed=9)
    free, _, _ = check_kernels_equal_host(strings, 3)
    every = [r.tobytes() for f in free for r in f.serials]
    none, _, _ = check_kernels_equal_host(strings, 3, spent=every)
    assert all(len(f) == 0 for f in none) and none[0].owned == free[0].owned == 70
    some, _, _ = check_kernels_equal_host(strings, 3, spent=every[::3] + [le32(11)])
    assert 0 < len(some[0]) < len(free[0])


@pytest.mark.gpu
def test_python_and_cpp_mirrors_on_the_kernels(on_kernel, tmp_path):
    strings = [REC['records']['owner'], REC['records']['sdk_foreign']] * 70
    one = records.unspent_named(strings, SN['program_id'], SN['record_name'], reference_account())
    assert len(one) == 70 and ['%dfield' % v for v in ints(one.serials)] == [SN['expected']] * 70 and one.commitments.shape == (70, 32)
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '0', 'ALEO_MI355X_MIN_DECRYPT': '0', 'ALEO_MI355X_MIN_SERIALS': '0', 'ALEO_MI355X_MIN_COMMITMENTS': '0'})


@pytest.mark.gpu
def test_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    """tests/helpers/commit_two_threads.py, a process of its own: there the two calls are the first of the process, so the one-time table builds run under both."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SERIALS='0', ALEO_MI355X_MIN_RECORDS='0', ALEO_MI355X_MIN_DECRYPT='0', ALEO_MI355X_MIN_COMMITMENTS='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'commit_two_threads.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr


@pytest.mark.gpu
def test_first_calls_of_a_process_in_an_unusual_order_get_the_host_path_s_bytes():
    """tests/helpers/records_first_calls.py, a process of its own: signatures_verify, unspent_named_many (K = 3), serial_numbers and decrypt_strings are its first
    device calls, in that order, so the resident tables are uploaded and the slot's pinned words first used in an order no other test has."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SERIALS='0', ALEO_MI355X_MIN_RECORDS='0', ALEO_MI355X_MIN_DECRYPT='0', ALEO_MI355X_MIN_COMMITMENTS='0',
               ALEO_MI355X_MIN_SIGNATURES='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'records_first_calls.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr
