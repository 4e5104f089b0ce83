"""Decrypting owned records (aleo_mi355x_records_decrypt_fields / _host, aleo_mi355x_min_decrypt, aleo_mi355x_record_fields, aleo_mi355x_record_plaintext,
aleo_mi355x_record_decrypt; aleo_amd/records.py) against the strings the reference's own tests hold (tests/golden/reference_records.json: `plaintexts`) and
against the rule written out with oracle/poseidon.py:

    the private fields of a record in randomizer order: the owner's one field if the owner is private, then every private entry's;  m of them
    randomizers = hash_many_psd8([domain_separator("AleoSymmetricEncryption0"), rvk], m);  plain_i = c_i - randomizers_i;  rvk = x(view_key * nonce)

Records other than the reference's two are made here, by a builder that writes the bit and byte layouts out (the layouts restated in oracle/poseidon.py:222-247
and csrc/records_plaintext.hpp) and encrypts with the oracle's hash.  The first half needs no GPU; the second half runs the kernel (ALEO_MI355X_MIN_DECRYPT=0)."""
import ctypes, functools, os, random, re, subprocess, tempfile
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps, pyref as P
import batch_support as bs
from batch_support import ROOT, HIPCC, CSRC, le32
from test_records import REF, R, L_ORDER, ENC_DOMAIN, account_generator, rows

NOT_OWNER, BAD_ARG = 7, 2
SUFFIX = {2: 'field', 3: 'group', 14: 'scalar', **{4 + i: 'i%d' % (8 << i) for i in range(5)}, **{9 + i: 'u%d' % (8 << i) for i in range(5)}}
BITS = {0: 253, 1: 1, 2: 253, 3: 253, 14: 251, **{4 + i: 8 << i for i in range(5)}, **{9 + i: 8 << i for i in range(5)}}
VIS = ['constant', 'public', 'private']


# ---- the builder: values -> bits / bytes -> fields -> a record string ---------------------------------------------------------------------------------
# a value: ('lit', type number, python value)  or  ('struct', [(name, value), ...])
def int_bits(v, n): return [(v >> i) & 1 for i in range(n)]


def raw_value(ty, v):
    """(the literal's value as a non-negative integer, its size in bits)."""
    if ty == 15: b = v.encode(); return int.from_bytes(b, 'little'), 8 * len(b)
    n = BITS[ty]
    return (int(v) & ((1 << n) - 1)), n                             # two's complement for the signed types


def plaintext_bits(val):
    if val[0] == 'lit':
        raw, n = raw_value(val[1], val[2])
        return [0, 0] + int_bits(val[1], 8) + int_bits(n, 16) + int_bits(raw, n)
    out = [0, 1] + int_bits(len(val[1]), 8)
    for name, member in val[1]:
        inner = plaintext_bits(member)
        out += int_bits(8 * len(name), 8) + int_bits(int.from_bytes(name.encode(), 'little'), 8 * len(name)) + int_bits(len(inner), 16) + inner
    return out


def plaintext_bytes(val):
    if val[0] == 'lit':
        raw, n = raw_value(val[1], val[2])
        head = b'\x00' + val[1].to_bytes(2, 'little')
        return head + ((n // 8).to_bytes(2, 'little') if val[1] == 15 else b'') + raw.to_bytes((n + 7) // 8, 'little')
    out = b'\x01' + bytes([len(val[1])])
    for name, member in val[1]:
        inner = plaintext_bytes(member)
        out += bytes([len(name)]) + name.encode() + len(inner).to_bytes(2, 'little') + inner
    return out


def bits_to_fields(bits):
    bits = bits + [1]                                               # the terminus
    bits += [0] * (-len(bits) % ps.FR_DATA_BITS)
    return [sum(b << i for i, b in enumerate(bits[k:k + ps.FR_DATA_BITS])) for k in range(0, len(bits), ps.FR_DATA_BITS)]


def literal_text(ty, v):
    if ty == 0: return P.bech32m_encode('aleo', le32(v))
    if ty == 1: return 'true' if v else 'false'
    if ty == 15: return '"%s"' % v
    return '%d%s' % (v, SUFFIX[ty])


def expected_entry(val, vis):
    """What RecordPlaintext.entries holds for this value: a literal's text with its visibility, a dict for a struct."""
    if val[0] == 'lit': return literal_text(val[1], val[2]) + '.' + VIS[vis]
    return {name: expected_entry(member, vis) for name, member in val[1]}


def text_to_value(text):
    """A rendered literal ("…<suffix>.<visibility>") back to (type number, python value, visibility): what the string says, read independently of how it was written."""
    lit, vis = text.rsplit('.', 1)
    if lit.startswith('aleo1'): hrp, raw = wire.bech32m_decode(lit); assert hrp == 'aleo'; return 0, int.from_bytes(raw, 'little'), VIS.index(vis)
    if lit in ('true', 'false'): return 1, lit == 'true', VIS.index(vis)
    if lit.startswith('"'): assert lit.endswith('"'); return 15, lit[1:-1], VIS.index(vis)
    m = re.fullmatch(r'(-?\d+)([a-z]+\d*)', lit)
    ty = {s: t for t, s in SUFFIX.items()}[m.group(2)]
    return ty, int(m.group(1)), VIS.index(vis)


def check_entry(got, val, vis):
    if val[0] == 'struct':
        assert isinstance(got, dict) and list(got) == [n for n, _ in val[1]]
        for name, member in val[1]: check_entry(got[name], member, vis)
    else: assert text_to_value(got) == (val[1], val[2], vis), (got, val)


class Built:
    """One record: string, what it holds, and everything the checks need of how it was encrypted."""
    def __init__(self, G, view_key, owner_x, owner_private, entries, seed):
        rng = random.Random(seed)
        N = ps.ed_mul(G, rng.randrange(1, L_ORDER))
        self.nonce, self.rvk = N[0], ps.ed_mul(N, view_key)[0]
        self.owner_x, self.owner_private, self.entries = owner_x, owner_private, entries
        self.plain = [owner_x] if owner_private else []
        per_entry = []
        for name, vis, val in entries:
            f = bits_to_fields(plaintext_bits(val)) if vis == 2 else None
            per_entry.append(f)
            if f: self.plain += f
        self.m = len(self.plain)
        self.rnd = ps.hash_many_psd8([ENC_DOMAIN, self.rvk], self.m) if self.m else []
        self.cipher = [(p + r) % R for p, r in zip(self.plain, self.rnd)]
        at = 1 if owner_private else 0
        payload = (b'\x01\x01\x00' + le32(self.cipher[0])) if owner_private else (b'\x00' + le32(owner_x))
        payload += bytes([len(entries)])
        for (name, vis, val), f in zip(entries, per_entry):
            if vis == 2: body = b'\x02' + len(f).to_bytes(2, 'little') + b''.join(le32(c) for c in self.cipher[at:at + len(f)]); at += len(f)
            else: body = bytes([vis]) + plaintext_bytes(val)
            payload += bytes([len(name)]) + name.encode() + len(body).to_bytes(2, 'little') + body
        self.string = wire.bech32m_encode('record', payload + le32(self.nonce))

    def check_plaintext(self, pt):
        assert pt.owner == P.bech32m_encode('aleo', le32(self.owner_x)) and pt.owner_visibility == ('private' if self.owner_private else 'public') and pt.nonce == self.nonce
        assert list(pt.entries) == [name for name, _, _ in self.entries]
        for name, vis, val in self.entries:
            check_entry(pt.entries[name], val, vis)
            assert pt.entries[name] == expected_entry(val, vis)


def string_of_fields(k):
    """A string literal whose private form takes exactly k fields: 2 + 8 + 16 + 8 L bits and the terminus."""
    L = (ps.FR_DATA_BITS * k - 27) // 8
    return ('lit', 15, ''.join(chr(97 + i % 26) for i in range(L)))


ALL_LITERALS = [('lit', 0, 0), ('lit', 1, True), ('lit', 1, False), ('lit', 2, R - 1), ('lit', 3, 5), ('lit', 4, -128), ('lit', 5, -2), ('lit', 6, 2 ** 31 - 1), ('lit', 7, -2 ** 63),
                ('lit', 8, -2 ** 127), ('lit', 8, 2 ** 127 - 1), ('lit', 9, 255), ('lit', 10, 65535), ('lit', 11, 7), ('lit', 12, 2 ** 64 - 1), ('lit', 13, 2 ** 128 - 1),
                ('lit', 14, L_ORDER - 1), ('lit', 15, 'a string, with: punctuation {and} braces'), ('lit', 15, '')]
TWO_LEVELS = ('struct', [('amount', ('lit', 12, 42)), ('inner', ('struct', [('flag', ('lit', 1, True)), ('who', ('lit', 2, 123456789)), ('deep', ('lit', 7, -5))])), ('tail', ('lit', 9, 3))])


@functools.lru_cache(maxsize=None)
def account():
    G = account_generator(); vk = 0x0123456789abcdef0fedcba9876543211357 | 1
    return G, vk, ps.ed_mul(G, vk)[0]


@functools.lru_cache(maxsize=None)
def built_records():
    """About 40 records: every literal type and a two-level struct in each visibility, public and private owners, and private field counts
    0, 1, 2, 7, 8, 9, 16, 17, 25 (the rate boundary, the second and the third permutation)."""
    G, vk, ax = account()
    ALL_LITERALS[0] = ('lit', 0, ax)
    out = []
    def add(owner_private, entries): out.append(Built(G, vk, ax, owner_private, entries, 500 + len(out)))
    for i, lit in enumerate(ALL_LITERALS): add(i % 3 != 0, [('v%d' % i, 2, lit)])                                   # one private literal each
    add(True, [('l%d' % i, i % 2, lit) for i, lit in enumerate(ALL_LITERALS)])                                        # all of them constant / public: m = 1
    add(False, [('l%d' % i, i % 2, lit) for i, lit in enumerate(ALL_LITERALS)])                                       # nothing private at all: m = 0
    add(False, [])                                                                                                    # no entries, m = 0
    add(True, [('s', 2, TWO_LEVELS)]); add(True, [('s', 1, TWO_LEVELS)]); add(False, [('s', 2, TWO_LEVELS), ('t', 0, TWO_LEVELS)])
    add(True, [('microcredits', 2, ('lit', 12, 77)), ('memo', 1, ('lit', 15, 'hello')), ('data', 2, TWO_LEVELS)])
    for m in (2, 7, 8, 9, 16, 17, 25):
        add(True, [('pad', 2, string_of_fields(m - 1))])                                                              # owner + one entry of m - 1 fields
        add(False, [('a', 2, ('lit', 12, m)), ('pad', 2, string_of_fields(m - 1))] if m > 2 else [('a', 2, ('lit', 12, 1)), ('b', 2, ('lit', 1, True))])
    return out


def p(a): return a.ctypes.data_as(ctypes.c_void_p)


def call_string(fn, *args, cap=4096):
    buf = ctypes.create_string_buffer(cap); ln = ctypes.c_size_t(cap)
    return fn(*args, buf, ctypes.byref(ln)), buf.value.decode(), ln.value


def c_record_decrypt(string, view_key, address, cap=4096):
    vk = np.frombuffer(records.view_key_bytes(view_key), dtype=np.uint8); ax = np.frombuffer(records.address_x_bytes(address), dtype=np.uint8)
    return call_string(aleo_amd.lib().aleo_mi355x_record_decrypt, string.encode(), p(vk), p(ax), cap=cap)


def flat_batch(recs):
    """(rvk rows, offsets, field rows, expected plain rows by the oracle's subtraction) of built records."""
    off = np.zeros(len(recs) + 1, dtype=np.uint32); off[1:] = np.cumsum([b.m for b in recs])
    want = [(c - r) % R for b in recs for c, r in zip(b.cipher, ps.hash_many_psd8([ENC_DOMAIN, b.rvk], b.m) if b.m else [])]
    return rows([b.rvk for b in recs]), off, rows([c for b in recs for c in b.cipher]), rows(want)


# ---- 1: the reference's strings -----------------------------------------------------------------------------------------------------------------------
def test_record_decrypt_returns_the_strings_the_reference_asserts():
    G = account_generator()
    for name in ('owner', 'sdk'):
        rc, s, ln = c_record_decrypt(REF['records'][name], REF['view_keys'][name], REF['addresses'][name])
        assert rc == 0 and s == REF['plaintexts'][name] and ln == len(s)
        pt = records.RecordCiphertext.from_string(REF['records'][name]).decrypt(REF['view_keys'][name], REF['addresses'][name])
        assert str(pt) == REF['plaintexts'][name] and pt.microcredits() == 1500000000000000                      # record_plaintext.rs:126-129
        assert pt.owner == REF['addresses'][name] and pt.nonce == int(REF['nonces'][name]) and pt.entries == {'microcredits': '1500000000000000u64.private'}
    for rec, foreign in (('owner', 'non_owner'), ('sdk', 'sdk_foreign')):                                         # record_ciphertext.rs:126-127
        vk = REF['view_keys'][foreign]
        own = le32(ps.ed_mul(G, ps.view_key_scalar(vk))[0])                                                       # the foreign account's own address, and the owner's
        for addr in (own, REF['addresses'][rec]):
            rc, s, _ = c_record_decrypt(REF['records'][rec], vk, addr)
            assert rc == NOT_OWNER and s == ''
        with pytest.raises(records.NotOwner): records.RecordCiphertext.from_string(REF['records'][rec]).decrypt(vk, own)
    assert c_record_decrypt(REF['records']['owner'], REF['view_keys']['owner'], le32(5))[0] == NOT_OWNER         # the right key, another address
    assert aleo_amd.lib().aleo_mi355x_strerror(NOT_OWNER) == b"the record's owner is not the given address"


# ---- 2: the host path against the oracle --------------------------------------------------------------------------------------------------------------
def test_host_path_equals_the_oracle_on_built_records():
    G, vk, ax = account(); recs = built_records()
    assert 35 <= len(recs) <= 45 and {0, 1, 2, 7, 8, 9, 16, 17, 25} <= {b.m for b in recs}
    assert {v[1] for b in recs for _, vis, v in b.entries if vis == 2 and v[0] == 'lit'} == set(range(16))
    rvk, off, fields, want = flat_batch(recs)
    plain, flags = records.decrypt_fields(rvk, off, fields, host=True)
    assert not flags.any() and plain.tobytes() == want.tobytes()
    assert plain.tobytes() == rows([v for b in recs for v in b.plain]).tobytes()                                   # and they are what was encrypted
    for i, b in enumerate(recs):
        rec = records.RecordCiphertext.from_string(b.string)
        assert rec.owner_kind == int(b.owner_private) and rec.fields().tobytes() == fields[off[i]:off[i + 1]].tobytes()
        pt = rec.plaintext(plain[off[i]:off[i + 1]], ax)
        b.check_plaintext(pt)
        assert rec.decrypt(vk, ax) == pt and rec.plaintext(plain[off[i]:off[i + 1]]) == pt                          # the one-record path; no address given
        with pytest.raises(records.NotOwner): rec.plaintext(plain[off[i]:off[i + 1]], le32(ax ^ 1))
        with pytest.raises(records.NotOwner): rec.decrypt(vk, le32(ax ^ 1))
    # the scan's record view key is the builder's
    flags1, rvk1 = records.scan(rows([b.cipher[0] for b in recs if b.owner_private][:3]), rows([b.nonce for b in recs if b.owner_private][:3]), vk, ax, host=True)
    assert (flags1 == 1).all() and rvk1.tobytes() == rows([b.rvk for b in recs if b.owner_private][:3]).tobytes()
    # a struct renders one member per line, two spaces deeper per level, the brace at the entry's own indentation
    s = str(records.RecordCiphertext.from_string(next(b for b in recs if b.entries and b.entries[0][2] is TWO_LEVELS and b.entries[0][1] == 1).string).decrypt(vk, ax))
    assert '  s: {\n    amount: 42u64.public,\n    inner: {\n      flag: true.public,\n      who: 123456789field.public,\n      deep: -5i64.public\n    },\n    tail: 3u8.public\n  },\n  _nonce: ' in s


def test_host_path_flags_malformed_records_and_refuses_bad_offsets():
    recs = [b for b in built_records() if b.m in (1, 2, 9, 17)][:6]
    rvk, off, fields, want = flat_batch(recs)
    good, _ = records.decrypt_fields(rvk, off, fields, host=True)
    assert good.tobytes() == want.tobytes()
    bad_rvk, bad_field = 1, 4
    assert off[bad_field + 1] - off[bad_field] >= 2
    rvk2, fields2 = rvk.copy(), fields.copy()
    rvk2[bad_rvk] = np.frombuffer(le32(R), dtype=np.uint8); fields2[off[bad_field + 1] - 1] = 0xff                 # rvk = r; the record's last field = 2^256 - 1
    plain, flags = records.decrypt_fields(rvk2, off, fields2, host=True)
    assert flags.tolist() == [2 if i in (bad_rvk, bad_field) else 0 for i in range(len(recs))]
    for i in range(len(recs)):
        mine = plain[off[i]:off[i + 1]]
        if i in (bad_rvk, bad_field): assert not mine.any()
        else: assert mine.tobytes() == want[off[i]:off[i + 1]].tobytes()
    L = aleo_amd.lib(); fl = np.zeros(len(recs), dtype=np.uint8); out = np.zeros_like(fields)
    for fn in (L.aleo_mi355x_records_decrypt_fields_host, L.aleo_mi355x_records_decrypt_fields):
        o = off.copy(); o[0] = 1
        assert fn(p(out), p(fl), p(rvk), p(o), p(fields), len(recs)) == BAD_ARG                                     # does not start at 0
        o = off.copy(); o[2], o[3] = off[3], off[2]
        assert o[3] < o[2] and fn(p(out), p(fl), p(rvk), p(o), p(fields), len(recs)) == BAD_ARG                     # decreases
        o = np.array([0, 65536], dtype=np.uint32)
        assert fn(p(out), p(fl), p(rvk), p(o), p(fields), 1) == BAD_ARG                                             # more than 65 535 fields
        assert fn(None, p(fl), p(rvk), p(off), p(fields), len(recs)) == BAD_ARG


# ---- 3: small behaviours ------------------------------------------------------------------------------------------------------------------------------
def test_small_behaviours(monkeypatch):
    L = aleo_amd.lib(); G, vk, ax = account()
    b = next(b for b in built_records() if len(b.entries) == 3)                                                    # owner, microcredits (private), memo (public), data (private struct)
    n = ctypes.c_size_t(99)
    assert L.aleo_mi355x_record_fields(b.string.encode(), None, 0, ctypes.byref(n)) == 0 and n.value == b.m > 3
    out = np.zeros((b.m, 32), dtype=np.uint8)
    assert L.aleo_mi355x_record_fields(b.string.encode(), p(out), b.m - 1, ctypes.byref(n)) == BAD_ARG and n.value == b.m      # too little room: the count comes back
    assert L.aleo_mi355x_record_fields(b.string.encode(), p(out), b.m, ctypes.byref(n)) == 0
    assert out.tobytes() == rows(b.cipher).tobytes()                                                                # owner first, then the entries' fields in entry order
    assert L.aleo_mi355x_record_fields(b'garbage', None, 0, ctypes.byref(n)) != 0
    payload = wire.bech32m_decode(REF['records']['owner'])[1]
    assert payload[51] == 2 and L.aleo_mi355x_record_fields(wire.bech32m_encode('record', payload[:51] + b'\x03' + payload[52:]).encode(), None, 0, ctypes.byref(n)) == BAD_ARG     # visibility 3
    assert L.aleo_mi355x_record_fields(wire.bech32m_encode('record', payload[:52] + b'\x02' + payload[53:]).encode(), None, 0, ctypes.byref(n)) == BAD_ARG                        # two fields in 35 bytes
    # a short buffer: BAD_ARG and the length; then exactly enough
    want = REF['plaintexts']['owner']
    for cap in (1, 10, len(want)):
        rc, s, ln = c_record_decrypt(REF['records']['owner'], REF['view_keys']['owner'], REF['addresses']['owner'], cap=cap)
        assert rc == BAD_ARG and ln == len(want)
    rc, s, ln = c_record_decrypt(REF['records']['owner'], REF['view_keys']['owner'], REF['addresses']['owner'], cap=len(want) + 1)
    assert rc == 0 and s == want
    # an entry that does not parse is refused and named
    plain = rows(b.plain); plain[1] = 0x0f                                                                          # variant bits (1, 1)
    fields = np.ascontiguousarray(plain)
    rc, s, _ = call_string(L.aleo_mi355x_record_plaintext, b.string.encode(), p(fields), b.m, None)
    assert rc == BAD_ARG and "'microcredits'" in L.aleo_mi355x_last_error().decode()
    assert call_string(L.aleo_mi355x_record_plaintext, b.string.encode(), p(fields), b.m - 1, None)[0] == BAD_ARG  # not the record's count
    # the threshold: a default, its override read per call, and what is below it needs no device
    monkeypatch.delenv('ALEO_MI355X_MIN_DECRYPT', raising=False)
    default = int(L.aleo_mi355x_min_decrypt())
    assert 1 <= default <= 1 << 22 and default & (default - 1) == 0
    monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '12345'); assert int(L.aleo_mi355x_min_decrypt()) == 12345
    monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0'); assert int(L.aleo_mi355x_min_decrypt()) == 0
    monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', 'nonsense'); assert int(L.aleo_mi355x_min_decrypt()) == default
    monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '1000000')
    rvk, off, f, want_rows = flat_batch([b])
    got, flags = records.decrypt_fields(rvk, off, f)                                                                # routed: on the host
    assert got.tobytes() == want_rows.tobytes() and flags.tolist() == [0]
    # n = 0
    for host in (True, False):
        got, flags = records.decrypt_fields(np.zeros((0, 32), dtype=np.uint8), np.zeros(1, dtype=np.uint32), np.zeros((0, 32), dtype=np.uint8), host=host)
        assert got.shape == (0, 32) and flags.shape == (0,)
    assert L.aleo_mi355x_records_decrypt_fields(None, None, None, None, None, 0) == 0
    assert records.decrypt_owned([], vk, ax) == []


# ---- 4, 5: the lane's code on the host, and the kernel's code object ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path):
    """tests/cpp/records_decrypt_lane_emul.cpp: records_decrypt_lane.h compiled for the CPU over the field of checked_f29.h, which checks every limb bound."""
    r = bs.run_lane_emul(tmp_path, 'records_decrypt_lane_emul', flags=(), hipcc=True)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_decrypt_kernel_code_object_is_gfx950_and_has_no_scratch():
    import code_object as co
    asm, blocks = co.compile_unit('records_decrypt')
    meta = co.block_of(blocks, 'k_records_decrypt')
    print(co.registers('k_records_decrypt', meta))
    assert co.field(meta, 'private_segment_fixed_size') == 0 and co.field(meta, 'vgpr_spill_count') == 0


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0')
    monkeypatch.delenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_decrypt()) == 0


COUNTS = (0, 1, 2, 7, 8, 9, 16, 17, 24, 25)
BAD_RVK, BAD_FIELD = 37, 263                                       # one in each block; 263 has 7 fields (263 % 10 = 3)


@functools.lru_cache(maxsize=None)
def batch_300():
    """300 records (two blocks of lanes, the second partial) of random fields, their counts cycling through COUNTS, and the oracle's subtraction, computed once."""
    rng = random.Random(300)
    rvks = [rng.randrange(R) for _ in range(300)]; counts = [COUNTS[i % len(COUNTS)] for i in range(300)]
    cipher = [[rng.randrange(R) for _ in range(m)] for m in counts]
    cipher[5][0] = 0                                                # a difference that wraps below zero for sure
    want = [[(c - r) % R for c, r in zip(cs, ps.hash_many_psd8([ENC_DOMAIN, k], len(cs)) if cs else [])] for cs, k in zip(cipher, rvks)]
    rvks[BAD_RVK] = R + 1; cipher[BAD_FIELD][6] = (1 << 256) - 1
    assert counts[BAD_FIELD] == 7 and counts[BAD_RVK] == 17
    for i in (BAD_RVK, BAD_FIELD): want[i] = [0] * counts[i]
    off = np.zeros(301, dtype=np.uint32); off[1:] = np.cumsum(counts)
    flags = np.zeros(300, dtype=np.uint8); flags[[BAD_RVK, BAD_FIELD]] = 2
    out = (rows(rvks), off, rows([c for cs in cipher for c in cs]), rows([w for ws in want for w in ws]), flags)
    for a in out: a.setflags(write=False)
    return out


@pytest.mark.gpu
def test_kernel_equals_the_host_path_and_the_oracle(on_kernel):
    rvk, off, fields, want, want_flags = batch_300()
    plain, flags = records.decrypt_fields(rvk, off, fields)
    hplain, hflags = records.decrypt_fields(rvk, off, fields, host=True)
    assert flags.tobytes() == hflags.tobytes() == want_flags.tobytes()
    assert plain.tobytes() == hplain.tobytes()
    assert plain.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_kernel_chunks_are_cut_at_record_boundaries(on_kernel, monkeypatch):
    rvk, off, fields, want, want_flags = batch_300()
    monkeypatch.setenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', '64')      # ~55 chunks; a record of 25 fields after 40 starts a new one
    plain, flags = records.decrypt_fields(rvk, off, fields)
    assert flags.tobytes() == want_flags.tobytes() and plain.tobytes() == want.tobytes()
    monkeypatch.setenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', '8')       # below the longest record: such a record is a chunk of its own
    plain, flags = records.decrypt_fields(rvk, off, fields)
    assert flags.tobytes() == want_flags.tobytes() and plain.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_kernel_edge_sizes(on_kernel):
    rvk, off, fields, want, want_flags = batch_300()
    for i in (1, 9):                                                # n = 1: one field, and 25
        m = int(off[i + 1] - off[i]); assert m == COUNTS[i]
        plain, flags = records.decrypt_fields(rvk[i:i + 1], np.array([0, m], dtype=np.uint32), fields[off[i]:off[i + 1]])
        assert flags.tolist() == [0] and plain.tobytes() == want[off[i]:off[i + 1]].tobytes()
    # 257 records without a field: nothing to write, the flags still say which rvk is malformed
    rv = np.ascontiguousarray(rvk[:257])
    plain, flags = records.decrypt_fields(rv, np.zeros(258, dtype=np.uint32), np.zeros((0, 32), dtype=np.uint8))
    hplain, hflags = records.decrypt_fields(rv, np.zeros(258, dtype=np.uint32), np.zeros((0, 32), dtype=np.uint8), host=True)
    assert plain.shape == (0, 32) and flags.tobytes() == hflags.tobytes() and flags.tolist() == [2 if i == BAD_RVK else 0 for i in range(257)]


@pytest.mark.gpu
def test_decrypt_owned_end_to_end_and_its_cpp_mirror(on_kernel, tmp_path):
    G, vk, ax = account(); rng = random.Random(9)
    other_vk = 0x77777777777777777777 | 1; other_ax = ps.ed_mul(G, other_vk)[0]
    mine = built_records()
    foreign = [Built(G, other_vk, other_ax, i % 5 != 0, [('microcredits', 2, ('lit', 12, 1000 + i)), ('memo', i % 2, ('lit', 15, 'not yours'))], 9000 + i) for i in range(66)]
    assert len(mine) + len(foreign) >= 100
    batch = [(b.string, b) for b in mine] + [(b.string, None) for b in foreign]
    rng.shuffle(batch)
    strings = [s for s, _ in batch]
    got = records.decrypt_owned(strings, vk, ax)
    idx, _ = records.find_owned(strings, vk, ax)
    assert [i for i, _ in got] == idx == [i for i, (_, b) in enumerate(batch) if b is not None]
    for i, pt in got:
        rc, s, _ = c_record_decrypt(strings[i], vk, le32(ax), cap=16384)
        assert rc == 0 and s == str(pt)
        batch[i][1].check_plaintext(pt)
    assert sum(pt.microcredits() for _, pt in got) == 77
    # the reference's records among them, under the reference's account
    ref_strings = strings[:50] + [REF['records']['owner']] + strings[50:] + [REF['records']['sdk_foreign'], REF['records']['sdk']]
    got = records.decrypt_owned(ref_strings, REF['view_keys']['owner'], REF['addresses']['owner'])
    assert [i for i, _ in got] == [50, len(ref_strings) - 1] == records.find_owned(ref_strings, REF['view_keys']['owner'], REF['addresses']['owner'])[0]
    assert all(str(pt) == REF['plaintexts']['owner'] and pt.microcredits() == 1500000000000000 for _, pt in got)
    # the C++ mirror: view key, address, expected indices, then the records
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, 'records_decrypt_test')
    env = dict(os.environ, ALEO_MI355X_MIN_RECORDS='0', ALEO_MI355X_MIN_DECRYPT='0')
    r = subprocess.run([exe, REF['view_keys']['owner'], REF['addresses']['owner'], '50,%d' % (len(ref_strings) - 1), REF['plaintexts']['owner']] + ref_strings, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, ps.view_key_string(vk), P.bech32m_encode('aleo', le32(ax)), ','.join(str(i) for i in idx), ''] + strings, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr
