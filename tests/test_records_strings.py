"""The record search straight from "record1…" strings (aleo_mi355x_records_parse_many / _scan_strings and their _host forms; RecordBatch, parse_many,
scan_strings and the string roads of find_owned, find_owned_many, decrypt_owned in aleo_amd/records.py).

The yardstick of the parse is the one-record parser the library always had, RecordCiphertext.from_string (aleo_mi355x_record_parse): the same owner variant,
owner field and nonce x, and kind -1 exactly where it raises.  The yardstick of the scan is scan_many(host=True) on the parsed rows, with the two rules the scan
over strings adds: a public owner is compared with the account's address x, a string that does not parse gets flag 3 and a zero row.
The first half needs no GPU (host path, the lane code run on the host, the kernels' code object); the second half runs the kernels against the host path."""
import ctypes, os, random, re, struct, subprocess, tempfile
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps
import batch_support as bs
from batch_support import ROOT, HIPCC, CSRC, le32
from test_records import REF, R, L_ORDER, account_generator, reference_cases, synthetic_records

ALPHABET = 'qpzry9x8gf2tvdw0s3jn54khce6mua7l'
GOOD = REF['records']['owner']
MAX_CHARS = 1 << 20


# ---- a bech32m encoder at symbol level (BIP-350) --------------------------------------------------------------------------------------------------
def polymod(values):
    chk = 1
    for v in values:
        b = chk >> 25
        chk = ((chk & 0x1ffffff) << 5) ^ v
        for i, g in enumerate((0x3b6a57b2, 0x26508e6d, 0x1ea119fa, 0x3d4233dd, 0x2a1462b3)):
            if (b >> i) & 1: chk ^= g
    return chk


def to_symbols(payload: bytes):
    """The data symbols of a payload, zero padding in the last one."""
    acc = bits = 0; out = []
    for byte in payload:
        acc = (acc << 8) | byte; bits += 8
        while bits >= 5: bits -= 5; out.append((acc >> bits) & 31)
    if bits: out.append((acc << (5 - bits)) & 31)
    return out


def encode_symbols(symbols, hrp='record'):
    """hrp + '1' + the symbols + their bech32m checksum: whatever the symbols are, the checksum is right."""
    expanded = [ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp]
    pm = polymod(expanded + list(symbols) + [0] * 6) ^ 0x2bc830a3
    return hrp + '1' + ''.join(ALPHABET[s] for s in list(symbols) + [(pm >> (5 * (5 - i))) & 31 for i in range(6)])


def encode(payload: bytes, hrp='record'): return encode_symbols(to_symbols(payload), hrp)


def payload_of(private, owner, nonce, entries=(), count=1, variant=None):
    """The layout of wire.hip: variant, (field count), owner field, entry count, per entry (name length, name, u16 length, bytes), nonce."""
    head = bytes([variant if variant is not None else (1 if private else 0)]) + (struct.pack('<H', count) if private else b'')
    body = b''.join(bytes([len(name)]) + name + struct.pack('<H', len(data)) + data for name, data in entries)
    return head + le32(owner) + bytes([len(entries)]) + body + le32(nonce)


def reference_sized(rng, owner=None, nonce=None, private=True):
    """A record of the shape of the reference's own (118 payload bytes, 202 characters): one entry named microcredits of 35 bytes."""
    return payload_of(private, rng.randrange(R) if owner is None else owner, rng.randrange(R) if nonce is None else nonce, [(b'microcredits', bytes(rng.randrange(256) for _ in range(35)))])


def case_list():
    """[(what, string, parses)]: the reference's ciphertexts, synthetic payloads of every shape the walk distinguishes, and one refusal of every kind."""
    rng = random.Random(20240)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    own, non = rng.randrange(R), rng.randrange(R)
    out = [('reference ' + name, s, True) for name, s in REF['records'].items()]
    good = lambda what, payload: out.append((what, encode(payload), True))
    bad = lambda what, s: out.append((what, s, False))
    five = [(b'a', rb(3)), (b'', b''), (b'n' * 255, rb(1)), (b'big', rb(2000)), (b'last', rb(7))]
    for private in (False, True):
        who = 'private' if private else 'public'
        good(who + ', no entries', payload_of(private, own, non))
        good(who + ', five entries: names of 0 and 255 bytes, entries of 0, 1 and 2000 bytes', payload_of(private, own, non, five))
        for extra in range(5): good(who + ', one entry of %d bytes' % extra, payload_of(private, own, non, [(b'microcredits', rb(extra))]))
        good(who + ', owner = r - 1, nonce = r - 1', payload_of(private, R - 1, R - 1, [(b'x', rb(2))]))
        good(who + ', owner = 0, nonce = 0', payload_of(private, 0, 0, [(b'x', rb(4))]))
    valid = [wire.bech32m_decode(s)[1] for _, s, _ in out]
    assert {(5 * len(to_symbols(p))) % 8 for p in valid} == {0, 1, 2, 3, 4}                                   # every count of padding bits
    assert all(wire.bech32m_encode('record', p) == encode(p) for p in valid)                                    # the encoder above is the library's
    base = payload_of(True, own, non, [(b'microcredits', rb(35))]); assert len(base) == 118 and len(encode(base)) == 202
    s = encode(base)
    bad('a flipped character', s[:100] + ('q' if s[100] != 'q' else 'p') + s[101:])
    bad('a character outside the alphabet', s[:50] + 'b' + s[51:]); bad('a byte above 127', s[:50] + '\xe9' + s[51:])
    bad('an upper-case character', s[:60] + s[60].upper() + s[61:] if s[60].isalpha() else s[:60] + 'Q' + s[61:]); bad('all upper case', s.upper())
    bad('prefix recorc', encode(base, 'recorc')); bad('prefix proof', encode(base, 'proof')); bad('record without its 1', 'record' + s[7:])
    bad("a second '1' in the data", s[:80] + '1' + s[81:]); bad("a '1' before the prefix", '1' + s)
    bad('five symbols', 'record1' + s[-5:]); bad('only the prefix', 'record1'); bad('six symbols: an empty payload', encode(b''))
    sym = to_symbols(base); assert (5 * len(sym)) % 8 == 1
    bad('non-zero padding bits', encode_symbols(sym[:-1] + [sym[-1] | 1]))
    five_k = payload_of(True, own, non, [(b'microcredits', rb(37))]); assert len(five_k) % 5 == 0
    bad('a whole extra padding symbol', encode_symbols(to_symbols(five_k) + [0]))
    good('a payload of 5 k bytes, no padding', five_k)
    bad('owner variant 2', encode(payload_of(True, own, non, [(b'm', rb(3))], variant=2)))
    bad('private field count 0', encode(payload_of(True, own, non, count=0))); bad('private field count 2', encode(payload_of(True, own, non, count=2)))
    bad('owner = r', encode(payload_of(True, R, non))); bad('public owner = r', encode(payload_of(False, R, non))); bad('owner = 2^256 - 1', encode(payload_of(True, (1 << 256) - 1, non)))
    bad('nonce = r', encode(payload_of(True, own, R))); bad('nonce = r + 1', encode(payload_of(False, own, R + 1)))
    # base: variant 0 | count 1..2 | owner 3..34 | entries 35 | name length 36 | name 37..48 | length 49..50 | bytes 51..85 | nonce 86..117
    for cut in (1, 2, 3, 20, 35, 36, 37, 43, 49, 50, 51, 70, 86, 100, 117): bad('truncated after %d bytes' % cut, encode(base[:cut]))
    pub = payload_of(False, own, non, [(b'microcredits', rb(35))])
    for cut in (1, 17, 33, 34, 100, 115): bad('public owner, truncated after %d bytes' % cut, encode(pub[:cut]))
    bad('an entry running past the end', encode(base[:49] + b'\xff\xff' + base[51:])); bad('an entry one byte too long', encode(base[:49] + struct.pack('<H', 36 + 32) + base[51:]))
    bad('a name running past the end', encode(base[:36] + b'\xff' + base[37:])); bad('an entry count of 2 with one entry', encode(base[:35] + b'\x02' + base[36:]))
    bad('one trailing byte', encode(base + b'\0')); bad('the empty string', ''); bad('a NUL inside', s[:90] + '\0' + s[91:])
    bad('more than 2^20 characters', 'record1' + 'q' * (MAX_CHARS - 6))
    for name, t in REF['invalid'].items(): bad('reference ' + name, t)
    return out


CASES = case_list()


def one_by_one(strings):
    """(kinds, owner rows, nonce rows) from a loop of RecordCiphertext.from_string: -1 and zero rows where it raises."""
    kinds = np.zeros(len(strings), dtype=np.int8); owner = np.zeros((len(strings), 32), dtype=np.uint8); nonce = np.zeros((len(strings), 32), dtype=np.uint8)
    for i, s in enumerate(strings):
        try: rec = records.RecordCiphertext.from_string(s)
        except (aleo_amd.AleoMi355xError, ValueError): kinds[i] = -1; continue
        kinds[i] = rec.owner_kind; owner[i] = np.frombuffer(rec.owner, dtype=np.uint8); nonce[i] = np.frombuffer(rec.nonce, dtype=np.uint8)
    return kinds, owner, nonce


def same(a, b): return len(a) == len(b) and all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


# ---- the host half ----------------------------------------------------------------------------------------------------------------------------------
def test_host_parse_many_equals_the_one_record_parser_on_every_case():
    strings = [s for _, s, _ in CASES]
    batch = records.RecordBatch.from_strings(strings)
    assert len(batch) == len(strings) and all(batch.string(i) == s for i, s in enumerate(strings) if len(s) < 5000)
    kinds, owner, nonce = records.parse_many(batch, host=True)
    want = one_by_one(strings)
    for i, (what, _, parses) in enumerate(CASES):
        assert (kinds[i] >= 0) == parses == (want[0][i] >= 0), what
        assert kinds[i] == want[0][i] and owner[i].tobytes() == want[1][i].tobytes() and nonce[i].tobytes() == want[2][i].tobytes(), what
    assert (kinds == 0).sum() >= 9 and (kinds == 1).sum() >= 9 and not owner[kinds < 0].any() and not nonce[kinds < 0].any()
    for i, (what, _, _) in enumerate(CASES):                      # and every string alone
        k1, o1, n1 = records.parse_many(records.RecordBatch.from_strings([strings[i]]), host=True)
        assert (k1[0], o1[0].tobytes(), n1[0].tobytes()) == (kinds[i], owner[i].tobytes(), nonce[i].tobytes()), what


def test_host_calls_refuse_bad_arguments_and_nothing_else():
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    text = (GOOD + 'garbage').encode(); tp = ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p)
    kinds = np.zeros(2, dtype=np.int8); o = np.zeros((2, 32), dtype=np.uint8); x = np.zeros((2, 32), dtype=np.uint8); flags = np.zeros(2, dtype=np.uint8)
    off = lambda *v: np.array(v, dtype=np.uint64)
    vk = np.frombuffer(le32(1), dtype=np.uint8); ax = np.frombuffer(le32(5), dtype=np.uint8)
    for f in (L.aleo_mi355x_records_parse_many_host, L.aleo_mi355x_records_parse_many):      # two strings: below the threshold both run on the host
        assert f(p(kinds), p(o), p(x), tp, p(off(0, len(GOOD), len(text))), 2) == 0 and kinds.tolist() == [1, -1]
        assert f(p(kinds), p(o), p(x), tp, p(off(1, len(GOOD), len(text))), 2) != 0 and b'offsets[0]' in L.aleo_mi355x_last_error()
        assert f(p(kinds), p(o), p(x), tp, p(off(0, len(text), len(GOOD))), 2) != 0 and b'decrease' in L.aleo_mi355x_last_error()
        assert f(None, p(o), p(x), tp, p(off(0, 1, 2)), 2) != 0 and f(p(kinds), p(o), p(x), None, p(off(0, 1, 2)), 2) != 0 and f(p(kinds), p(o), p(x), tp, None, 2) != 0
        assert f(None, None, None, None, None, 0) == 0
    for f in (L.aleo_mi355x_records_scan_strings_host, L.aleo_mi355x_records_scan_strings):
        assert f(p(flags), None, None, tp, p(off(0, len(GOOD), len(text))), 2, p(vk), p(ax), 1) == 0 and flags.tolist() == [0, 3]
        assert f(p(flags), p(kinds), None, tp, p(off(0, len(text), len(GOOD))), 2, p(vk), p(ax), 1) != 0
        assert f(None, None, None, tp, p(off(0, len(GOOD), len(text))), 2, p(vk), p(ax), 1) != 0
        assert f(p(flags), None, None, tp, p(off(0, len(GOOD), len(text))), 2, p(vk), p(ax), 0) != 0 and f(p(flags), None, None, tp, p(off(0, 1, 2)), 2, p(vk), p(ax), 65) != 0
        bad_vk = np.frombuffer(le32(L_ORDER), dtype=np.uint8)
        assert f(p(flags), None, None, tp, p(off(0, len(GOOD), len(text))), 2, p(bad_vk), p(ax), 1) != 0 and b'key 0' in L.aleo_mi355x_last_error()
        assert f(None, None, None, None, None, 0, p(vk), p(ax), 1) == 0


def test_record_batch_from_text_round_trips():
    strings = [s for _, s, _ in CASES if '\n' not in s and '\0' not in s and 0 < len(s) < 5000]
    for text in ('\n'.join(strings), '\n'.join(strings) + '\n'):
        batch = records.RecordBatch.from_text(text.encode())
        assert len(batch) == len(strings) and [batch.string(i) for i in range(len(batch))] == strings
        assert same(records.parse_many(batch, host=True), records.parse_many(records.RecordBatch.from_strings(strings), host=True))
    with_empty = records.RecordBatch.from_text(b'a,,b,', sep=b',')
    assert [with_empty.string(i) for i in range(len(with_empty))] == ['a', '', 'b'] and with_empty.text == b'ab'
    assert len(records.RecordBatch.from_text(b'')) == 0 and len(records.RecordBatch.from_text(b'\n')) == 1 and len(records.RecordBatch.from_strings([])) == 0
    with pytest.raises(IndexError): with_empty.string(3)
    with pytest.raises(ValueError): records.RecordBatch(b'abc', np.array([0, 2], dtype=np.uint64))


@pytest.fixture(scope='module')
def three_accounts():
    """Three accounts and ~60 record strings by the recipe of tests/test_records.py: records encrypted to key 0 and to key 1, foreign ones, the recipe's edge
    cases (a nonce off the curve: flag 2; an owner field that is not canonical: the string does not parse), public owners — key 1's address among them, once
    with a nonce off the curve — and a few strings that are no records."""
    G = account_generator(); rng = random.Random(515)
    keys = [rng.randrange(1, L_ORDER) | 1, rng.randrange(2, L_ORDER) & ~1, rng.randrange(1, L_ORDER)]
    addrs = [ps.ed_mul(G, k)[0] for k in keys]
    payloads = []
    for j in (0, 1):
        c0s, nxs, ax, edge = synthetic_records(3, 5, keys[j], 3000 + j, G); assert ax == addrs[j]
        payloads += [reference_sized(rng, c0, nx) for c0, nx in zip(c0s, nxs)]
        off_curve = nxs[[i for i, name in edge.items() if name == 'x off the curve'][0]]
    payloads += [reference_sized(rng, addrs[1], nxs[0], private=False), reference_sized(rng, addrs[1], off_curve, private=False), reference_sized(rng, addrs[1], 0, private=False),
                 reference_sized(rng, rng.randrange(R), nxs[1], private=False), payload_of(False, addrs[0], nxs[2])]
    strings = [encode(p) for p in payloads] + [GOOD, 'garbage', '', GOOD[:-1]]
    rng.shuffle(strings)
    return keys, [le32(a) for a in addrs], strings


def expected_scan(strings, keys, addrs):
    """flags, kinds, rvk by the rule of the module docstring from parse_many(host=True) and scan_many(host=True)."""
    kinds, owner, nonce = records.parse_many(records.RecordBatch.from_strings(strings), host=True)
    ok = np.flatnonzero(kinds >= 0)
    f, r = records.scan_many(owner[ok], nonce[ok], keys, addrs, host=True)
    flags = np.full((len(keys), len(strings)), 3, dtype=np.uint8); rvk = np.zeros((len(keys), len(strings), 32), dtype=np.uint8)
    flags[:, ok] = f; rvk[:, ok] = r
    for j, a in enumerate(addrs):
        for i in np.flatnonzero(kinds == 0): flags[j, i] = 1 if owner[i].tobytes() == a else 0
    return flags, kinds, rvk


def test_host_scan_strings_equals_scan_many_on_the_parsed_rows_with_the_public_owner_and_refusal_rules(three_accounts, monkeypatch):
    keys, addrs, strings = three_accounts
    batch = records.RecordBatch.from_strings(strings)
    for K in (1, 3):
        want = expected_scan(strings, keys[:K], addrs[:K])
        got = records.scan_strings(batch, keys[:K], addrs[:K], host=True)
        assert same(got, want), K
        only = records.scan_strings(batch, keys[:K], addrs[:K], want_rvk=False, host=True)
        assert only[2] is None and same(only[:2], want[:2])
    flags, kinds, rvk = want
    assert (flags[0] == 1).sum() >= 4 and (flags[1] == 1).sum() >= 7 and (flags[2] == 1).sum() == 0 and (flags == 2).any() and (flags[0] == 3).sum() >= 5
    pub1 = [i for i in np.flatnonzero(kinds == 0) if flags[1, i] == 1]
    assert len(pub1) == 3 and (flags[0, pub1] == 0).all() and sum(1 for i in pub1 if not rvk[1, i].any()) == 2      # off the curve and x = 0: zero rows, owner all the same
    assert not rvk[:, flags[0] == 3].any() and not rvk[flags == 2].any()
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '1000000')      # below the threshold the routed call is the host path
    assert same(records.scan_strings(batch, keys[:1], addrs[:1]), expected_scan(strings, keys[:1], addrs[:1]))


def check_roads_agree(strings, keys, addrs):
    """find_owned, find_owned_many and decrypt_owned give on a list of strings and on a RecordBatch what they give on RecordCiphertext objects."""
    objects = [records.RecordCiphertext.from_string(s) for s in strings]
    batch = records.RecordBatch.from_strings(strings)
    accounts = list(zip(keys, addrs))
    want_many = records.find_owned_many(objects, accounts)
    assert records.find_owned_many(strings, accounts) == want_many == records.find_owned_many(batch, accounts)
    assert records.find_owned_many(strings, []) == [] == records.find_owned_many(objects, [])
    for j, (vk, ax) in enumerate(accounts):
        want = records.find_owned(objects, vk, ax)
        assert want == want_many[j] and records.find_owned(strings, vk, ax) == want == records.find_owned(batch, vk, ax) == records.find_owned(tuple(strings), vk, ax)
        dec = records.decrypt_owned(objects, vk, ax)
        assert [i for i, _ in dec] == want[0] and records.decrypt_owned(strings, vk, ax) == dec == records.decrypt_owned(batch, vk, ax)
    return want_many


def reference_strings_and_accounts():
    G = account_generator()
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']]
    accounts = {}
    for case, rec, vk, addr in reference_cases(G): accounts[case['view_key']] = (vk, addr)
    return strings, [a[0] for a in accounts.values()], [a[1] for a in accounts.values()], list(accounts)


def check_reference_expectations(pad=0):
    """The booleans the reference asserts (is_owner), its plaintext strings and microcredits(), from strings."""
    G = account_generator()
    for case, rec, vk, addr in reference_cases(G):
        idx, rvks = records.find_owned([str(rec)], vk, addr)
        assert (idx == [0]) == case['expected'] and len(rvks) == len(idx), case
        flags, kinds, _ = records.scan_strings(records.RecordBatch.from_strings([str(rec)]), [vk], [addr], want_rvk=False)
        assert bool(flags[0, 0] == 1) == case['expected'] and kinds[0] == 1
    strings, keys, addrs, names = reference_strings_and_accounts()
    padded = strings + [GOOD] * pad
    for name in REF['plaintexts']:
        got = records.decrypt_owned(padded, REF['view_keys'][name], REF['addresses'][name])
        assert [i for i, _ in got] == records.find_owned(records.RecordBatch.from_strings(padded), REF['view_keys'][name], REF['addresses'][name])[0] == [0] + list(range(2, len(padded)))
        assert all(str(pt) == REF['plaintexts'][name] and pt.microcredits() == 1500000000000000 and pt.owner == REF['addresses'][name] for _, pt in got)
    foreign = names.index('sdk_foreign')
    assert records.decrypt_owned(strings, keys[foreign], addrs[foreign]) == [] and records.find_owned(strings, keys[foreign], addrs[foreign]) == ([], [])


@pytest.fixture(scope='module')
def built_for_two(three_accounts):
    """~20 records made by encrypting (the builder of tests/test_records_decrypt.py), so that their owners can print them: for each of the first two accounts private
    owners with a private entry, public owners with and without one, and as many of a stranger's."""
    from test_records_decrypt import Built
    keys, addrs, _ = three_accounts
    G = account_generator(); out = []
    stranger = 0x5555555555555555 | 1
    for j, (vk, ax) in enumerate(list(zip(keys[:2], addrs[:2])) + [(stranger, le32(ps.ed_mul(G, stranger)[0]))] * 2):
        ax = int.from_bytes(ax, 'little')
        for t in range(3): out.append(Built(G, vk, ax, True, [('microcredits', 2, ('lit', 12, 100 * j + t)), ('memo', 1, ('lit', 15, 'hello'))], 7000 + 10 * j + t).string)
        out.append(Built(G, vk, ax, False, [('microcredits', 2, ('lit', 12, 7)), ('flag', 2, ('lit', 1, True))], 7100 + j).string)
        out.append(Built(G, vk, ax, False, [('memo', 1, ('lit', 15, 'in the clear'))], 7200 + j).string)
    random.Random(3).shuffle(out)
    return out


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '1000000'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '1000000')


def test_mirrors_return_from_strings_what_they_return_from_objects(on_host, three_accounts, built_for_two):
    keys, addrs, _ = three_accounts
    many = check_roads_agree(built_for_two, keys, addrs)
    assert [len(idx) for idx, _ in many] == [5, 5, 0] and all(sum(1 for v in rvks if v is None) == 2 for _, rvks in many[:2])
    rs, rk, ra, _ = reference_strings_and_accounts()
    check_roads_agree(rs, rk, ra)
    check_reference_expectations()


def test_a_bad_string_raises_from_strings_what_it_raises_from_the_loop(on_host, three_accounts):
    keys, addrs, _ = three_accounts
    for what, s, parses in CASES:
        if parses or len(s) > 5000: continue
        batch = [GOOD, GOOD, s, 'garbage']
        for call in (lambda b: records.find_owned(b, keys[0], addrs[0]), lambda b: records.find_owned_many(b, list(zip(keys, addrs))), lambda b: records.find_owned_many(b, []),
                     lambda b: records.decrypt_owned(b, keys[0], addrs[0])):
            with pytest.raises(Exception) as loop: call([records.RecordCiphertext.from_string(t) for t in batch])
            with pytest.raises(Exception) as direct: call(batch)
            with pytest.raises(Exception) as blob: call(records.RecordBatch.from_strings(batch))
            assert type(direct.value) is type(loop.value) is type(blob.value) and str(direct.value) == str(loop.value) == str(blob.value), what
            assert isinstance(loop.value, (aleo_amd.AleoMi355xError, ValueError))
    # decrypt_owned's own error: a public owner that is the account, a private entry, a nonce off the curve
    G = account_generator(); rng = random.Random(4)
    c0s, nxs, ax, edge = synthetic_records(1, 1, keys[0], 77, G)
    off_curve = nxs[[i for i, name in edge.items() if name == 'x off the curve'][0]]
    entry = (b'v', b'\x02' + struct.pack('<H', 1) + le32(rng.randrange(R)))                                  # private, one field
    for nonce, fails in ((off_curve, True), (0, False)):
        s = encode(payload_of(False, ax, nonce, [entry]))
        rec = records.RecordCiphertext.from_string(s)
        if not len(rec.fields()): pytest.fail('the entry above is not read as a private one')
        for road in ([rec], [s], records.RecordBatch.from_strings([s])):
            if fails:
                with pytest.raises(aleo_amd.AleoMi355xError, match='record 0 has a nonce that is not on the curve'): records.decrypt_owned(road, keys[0], le32(ax))
            else:
                try: got = records.decrypt_owned(road, keys[0], le32(ax))
                except aleo_amd.AleoMi355xError as e: got = str(e)
                if road == [rec]: first = got
                assert got == first


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_parse_and_resolve_kernels_are_gfx950_and_have_no_scratch():
    import code_object as co
    asm, blocks = co.compile_unit('records_strings')
    for kernel in ('k_records_parse', 'k_records_resolve'):
        meta = co.block_of(blocks, kernel)
        print(co.registers(kernel, meta, ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'max_flat_workgroup_size')))
        assert co.field(meta, 'private_segment_fixed_size') == 0 and co.field(meta, 'vgpr_spill_count') == 0


def test_device_lane_code_run_on_the_host_equals_the_one_record_parser(tmp_path):
    """tests/cpp/records_strings_lane_emul.cpp: records_strings_lane.h compiled for the CPU over the case list, string by string against aleo_mi355x_record_parse."""
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, 'records_strings_lane_emul')
    rng = random.Random(8)
    raw = [s.encode('latin-1') if all(ord(c) < 256 for c in s) else s.encode() for _, s, _ in CASES]
    raw += [GOOD[:k].encode() for k in range(0, len(GOOD), 9)] + [bytes(rng.randrange(256) for _ in range(k)) for k in (1, 7, 13, 200)]
    path = os.path.join(str(tmp_path), 'cases.bin')
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(raw)))
        for b in raw: f.write(struct.pack('<I', len(b))); f.write(b)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ' 0 mismatches' in r.stdout and '%d strings' % len(raw) in r.stdout, r.stdout + r.stderr


def run_cpp_mirror(tmp_path, env):
    """tests/cpp/records_strings_test.cpp: the RecordBatch overloads of include/aleo_mi355x.hpp on the reference's strings and on built records."""
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']] * 25
    r = bs.run_cpp_mirror(tmp_path, 'records_strings_test', [REF['view_keys']['owner'], REF['addresses']['owner'], REF['plaintexts']['owner']] + strings, env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_from_strings_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '1000000', 'ALEO_MI355X_MIN_DECRYPT': '1000000'})


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.delenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', raising=False); monkeypatch.delenv('ALEO_MI355X_SCAN_CHUNK_CHARS', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0
    return monkeypatch


def laid_out(n, cases, rng):
    """n strings: `cases` among reference-sized neighbours, refused ones on the first and the last lane of a wave where n reaches, the 2000-byte entries (and the
    over-long string) between 202-character neighbours."""
    out = [wire.bech32m_encode('record', reference_sized(rng)) for _ in range(n)]
    refused = [s for _, s, parses in cases if not parses]; rest = [s for _, s, parses in cases if parses]
    edges = sorted({i for i in (0, 63, 64, 127, 128, 191, 192, 255, 256, n - 1) if i < n})
    taken = set()
    for i, s in zip(edges, refused): out[i] = s; taken.add(i)
    others = refused[len(edges):] + rest
    free = [i for i in range(n) if i not in taken and i % 2 == 1] + [i for i in range(n) if i not in taken and i % 2 == 0]      # odd slots first: a neighbour on either side
    assert len(others) <= len(free)
    for i, s in zip(free, others): out[i] = s
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 4099])
def test_kernel_parse_many_equals_the_host_path(on_kernel, n):
    rng = random.Random(n)
    slices = [CASES[at:at + n] for at in range(0, len(CASES), n)] if n < len(CASES) + 10 else [CASES]      # every case at every n: in slices where n is small
    for cases in slices:
        strings = laid_out(n, cases, rng)
        batch = records.RecordBatch.from_strings(strings)
        got = records.parse_many(batch); want = records.parse_many(batch, host=True)
        assert same(got, want), (n, [what for what, _, _ in cases][:3])
        assert (want[0] < 0).sum() >= sum(1 for _, _, parses in cases if not parses)
    if n == 4099: assert want[0][0] == -1 and want[0][63] == -1 and want[0][64] == -1 and want[0][127] == -1 and (want[0] == 0).sum() >= 9


@pytest.mark.gpu
def test_kernel_parse_reads_from_global_memory_where_a_block_s_strings_exceed_its_lds(on_kernel):
    """k_records_parse stages a block's 256 strings in LDS where they take at most 64 KiB and parses from global memory otherwise: blocks of either kind, side by
    side, and one whose span is the budget to the byte (counted from the 16-byte boundary below its first character, as the kernel counts)."""
    rng = random.Random(6)
    short = lambda: wire.bech32m_encode('record', reference_sized(rng))
    long_ = lambda k: wire.bech32m_encode('record', payload_of(True, rng.randrange(R), rng.randrange(R), [(b'data', bytes(rng.randrange(256) for _ in range(k)))]))
    strings = [short() for _ in range(256)] + [long_(300) if i % 3 else 'record1' + 'q' * 900 for i in range(256)] + [short() for _ in range(256)]
    strings += [long_(60 + (i % 7)) for i in range(255)]
    lens = [len(s) for s in strings]
    start = sum(lens[:768]); fill = 65536 - (start % 16) - sum(lens[768:])                                         # the fourth block: 64 KiB from the boundary below its start
    assert 13 <= fill <= 20000
    strings.append('record1' + 'p' * (fill - 7)); strings += [short() for _ in range(40)] + [long_(2000)] * 30
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])])
    spans = [int(off[min(b + 256, len(strings))] - (off[b] & ~15)) for b in range(0, len(strings), 256)]
    assert spans[0] < 65536 < spans[1] and spans[2] < 65536 and spans[3] == 65536 and spans[4] > 65536 and len(spans) == 5
    batch = records.RecordBatch.from_strings(strings)
    want = records.parse_many(batch, host=True)
    assert same(records.parse_many(batch), want) and (want[0] == 1).sum() == len(strings) - 87 and (want[0] == -1).sum() == 87


@pytest.fixture(scope='module')
def scan_sets(three_accounts):
    """(n, K) -> (strings, keys, addresses, the host path's answer), built and computed once: the three accounts' records, the case list, random neighbours."""
    keys3, addrs3, mine = three_accounts
    G = account_generator(); rng = random.Random(99)
    keys = keys3 + [rng.randrange(1, L_ORDER) for _ in range(3)] + [1, 0]
    addrs = addrs3 + [le32(ps.ed_mul(G, k if k else L_ORDER)[0]) if k > 1 else le32(rng.randrange(R)) for k in keys[3:]]
    sets = {}
    def get(n, K):
        if (n, K) not in sets:
            r = random.Random(1000 * n + K)
            strings = laid_out(n, CASES if n > 1000 else CASES[:60], r)
            for i, s in zip(r.sample([i for i in range(300 if n > 1000 else 130, n - 1) if i % 64 not in (0, 63)], len(mine)), mine): strings[i] = s      # behind the cases
            batch = records.RecordBatch.from_strings(strings)
            sets[(n, K)] = (batch, keys[:K], addrs[:K], records.scan_strings(batch, keys[:K], addrs[:K], host=True))
        return sets[(n, K)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize('n,K', [(257, 1), (4099, 3), (8200, 8)])
@pytest.mark.parametrize('width', [1, 8])
def test_kernel_scan_strings_equals_the_host_path(on_kernel, scan_sets, n, K, width):
    batch, keys, addrs, want = scan_sets(n, K)
    on_kernel.setenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', str(width))
    got = records.scan_strings(batch, keys, addrs)
    assert same(got, want)
    only = records.scan_strings(batch, keys, addrs, want_rvk=False)
    assert only[2] is None and same(only[:2], want[:2])
    flags = want[0]
    assert (flags == 3).any() and (flags == 2).any() and (flags[0] == 1).sum() >= 4 and (flags == 0).any() and (K < 2 or (flags[1] == 1).sum() >= 7)


@pytest.mark.gpu
def test_kernel_chunks_are_cut_at_record_boundaries_and_one_string_may_exceed_the_cap(on_kernel, scan_sets):
    batch, keys, addrs, want = scan_sets(4099, 3)
    lens = np.diff(batch.offsets.astype(np.int64)); uploaded = lens[lens <= MAX_CHARS]
    cap = int(uploaded.sum()) // 3                                  # at least three chunks
    assert uploaded.max() > 3000 and (lens > MAX_CHARS).sum() == 1
    for chars in (cap, 3000):                                       # and a cap below the longest string that goes up: that chunk is that string alone
        on_kernel.setenv('ALEO_MI355X_SCAN_CHUNK_CHARS', str(chars))
        assert same(records.scan_strings(batch, keys, addrs), want), chars
        assert same(records.parse_many(batch), records.parse_many(batch, host=True)), chars


@pytest.mark.gpu
def test_kernel_mirrors_return_the_reference_s_expectations_from_strings(on_kernel, three_accounts, built_for_two):
    on_kernel.setenv('ALEO_MI355X_MIN_DECRYPT', '0')
    check_reference_expectations(pad=70)
    rs, rk, ra, _ = reference_strings_and_accounts()
    check_roads_agree(rs * 30, rk, ra)
    check_roads_agree(built_for_two * 4, three_accounts[0], three_accounts[1])


@pytest.mark.gpu
def test_kernel_cpp_mirror_from_strings(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '0', 'ALEO_MI355X_MIN_DECRYPT': '0'})
