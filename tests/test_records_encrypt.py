"""Record plaintexts encrypted to record1… strings: aleo_mi355x_record_encrypt, _record_encrypt_symmetric, _record_nonce, _records_encrypt and its _host form
(csrc/record_encrypt_host.hpp, records_encrypt_lane.h, records_encrypt.hip); RecordPlaintext.encrypt / encrypt_symmetric, record_nonce and encrypt_many in
aleo_amd/records.py; encrypt_record and encrypt_records in include/aleo_mi355x.hpp.

Layers, each checked against the one before.  The reference's data pins the symmetric half: its own plaintext under x(view key . nonce) gives its own record1…
string character for character.  The builder of tests/test_records_decrypt.py (the layouts written out in Python, the oracle's hash) is the restatement: every
record it builds comes back from its rendered plaintext and its randomizer.  The ROUND TRIP through the host scan and decryption ties nonce = x(r G) and
rvk = x(r Owner), which no reference-held answer reaches, to the road the library already had.  The host path, byte for byte, checks the two device lanes —
emulated on the CPU, plain and under the sanitizers, here, and on the GPU in the second half (ALEO_MI355X_MIN_ENCRYPT=0).  No test reads the reference tree."""
import ctypes, functools, os, random, re, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps
import plaintext_ref as PR
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32
from test_records import REF, R, L_ORDER, ENC_DOMAIN, find_x
from test_records_decrypt import built_records, account
from test_plaintexts import plaintext, address, computed_strings, routed_strings, malformed_strings, random_plaintext, LANE_CHARS, LANE_ENTRIES

BAD_ARG = 2
NONCE = re.compile(r'(_nonce\s*:\s*)\d+(group)')
INVALID = 'The record plaintext string provided was invalid'


def with_nonce(s, r): return NONCE.sub(lambda m: m.group(1) + str(records.record_nonce(r)) + m.group(2), s)
def rows32(vals): return np.frombuffer(b''.join(le32(v) for v in vals), dtype=np.uint8).reshape(-1, 32).copy() if len(vals) else np.zeros((0, 32), dtype=np.uint8)
def strings_of(batch): return [batch.string(i) for i in range(len(batch))]
def payload_of(record1): return wire.bech32m_decode(record1)[1]


def lane_routes(s):
    """Whether the device lane hands this (well-formed) string to the host code: a struct or a quoted string, more characters or entries than the lane takes."""
    pt = records.RecordPlaintext(s)
    return len(s.encode()) > LANE_CHARS or len(pt.entries) > LANE_ENTRIES or any(isinstance(v, dict) or v.startswith('"') for v in pt.entries.values())


def call_string(fn, *args, cap=4096):
    buf = ctypes.create_string_buffer(cap); ln = ctypes.c_size_t(cap)
    return fn(*args, buf, ctypes.byref(ln)), buf.value.decode(), ln.value


def same(got, want):
    """Two results of encrypt_many, byte for byte."""
    return got[0].text == want[0].text and got[0].offsets.tobytes() == want[0].offsets.tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()


# ---- 1: the pin -----------------------------------------------------------------------------------------------------------------------------------------------
def test_pin_the_reference_s_plaintexts_under_their_record_view_keys_are_its_ciphertexts():
    for name in ('owner', 'sdk'):
        rvk = ps.ed_mul(ps.ed_from_x(int(REF['nonces'][name])), ps.view_key_scalar(REF['view_keys'][name]))[0]
        rc, s, ln = call_string(aleo_amd.lib().aleo_mi355x_record_encrypt_symmetric, REF['plaintexts'][name].encode(), bs._vp(le32(rvk)))
        assert rc == 0 and s == REF['records'][name] and ln == len(s) == 202
        assert str(records.RecordPlaintext(REF['plaintexts'][name]).encrypt_symmetric(rvk)) == REF['records'][name]
    assert call_string(aleo_amd.lib().aleo_mi355x_record_encrypt_symmetric, REF['plaintexts']['owner'].encode(), bs._vp(le32(R)))[0] == BAD_ARG      # a key that is no field element


# ---- 2: the restatement -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built_plaintexts():
    """[(the builder's record, its randomizer, its plaintext as the library renders it)] of tests/test_records_decrypt.py's about 40 records."""
    G, vk, ax = account()
    return [(b, random.Random(500 + i).randrange(1, L_ORDER), str(records.RecordCiphertext.from_string(b.string).decrypt(vk, ax))) for i, b in enumerate(built_records())]


def test_host_path_equals_the_restatement_on_built_records():
    built = built_plaintexts()
    assert 35 <= len(built) <= 45 and {0, 1, 2, 7, 8, 9, 16, 17, 25} <= {b.m for b, _, _ in built}
    for b, r, text in built:
        assert records.record_nonce(r) == b.nonce
        rc, s, ln = call_string(aleo_amd.lib().aleo_mi355x_record_encrypt, text.encode(), bs._vp(le32(r)), 0, cap=16384)
        assert rc == 0 and s == b.string and ln == len(s)
    batch, flags, rvk = records.encrypt_many([t for _, _, t in built], [r for _, r, _ in built], host=True)
    assert not flags.any() and strings_of(batch) == [b.string for b, _, _ in built] and rvk.tobytes() == rows32([b.rvk for b, _, _ in built]).tobytes()
    assert records.encrypt_last_routed() == len(built)
    assert str(records.RecordPlaintext(built[0][2]).encrypt(built[0][1])) == built[0][0].string


# ---- 3: flags and edges -------------------------------------------------------------------------------------------------------------------------------------------
TEMPLATE_ENTRIES = [('microcredits', 2, '1500000u64'), ('memo', 1, '7field'), ('flag', 0, 'true')]
EDGE_RANDOMIZERS = (0, 1, L_ORDER - 1, L_ORDER, (1 << 256) - 1)


def test_randomizers_at_the_edges_of_the_scalar_field():
    G, vk, ax = account(); template = plaintext(TEMPLATE_ENTRIES)
    batch, flags, rvk = records.encrypt_many([template] * 5, EDGE_RANDOMIZERS, set_nonce=True, host=True)
    assert flags.tolist() == [0, 0, 0, 2, 2] and not rvk[3:].any() and strings_of(batch)[3:] == ['', '']
    owner = ps.ed_from_x(ax)
    for i, r in enumerate(EDGE_RANDOMIZERS[:3]):                     # r = 0 is computed by the formula: the identity twice, nonce 0 and rvk 0
        nonce, key = (ps.ed_mul(G, r)[0], ps.ed_mul(owner, r)[0]) if r else (0, 0)
        rec = records.RecordCiphertext.from_string(batch.string(i))
        assert records.record_nonce(r) == nonce == int.from_bytes(rec.nonce, 'little') and rvk[i].tobytes() == le32(key)
        c0 = (ax + ps.hash_many_psd8([ENC_DOMAIN, key], 2)[0]) % R
        assert rec.owner_kind == 1 and rec.fields()[0].tobytes() == le32(c0)
    L = aleo_amd.lib(); out = np.zeros(32, dtype=np.uint8)
    for r in EDGE_RANDOMIZERS[3:]:
        assert L.aleo_mi355x_record_nonce(bs._p(out), bs._vp(le32(r))) == BAD_ARG
        assert call_string(L.aleo_mi355x_record_encrypt, template.encode(), bs._vp(le32(r)), 1)[0] == BAD_ARG


def test_a_nonce_off_by_one_and_owners_that_are_no_points():
    G, vk, ax = account(); r = 0x1234567890abcdef; good = with_nonce(plaintext(TEMPLATE_ENTRIES), r)
    off = NONCE.sub(lambda m: m.group(1) + str(records.record_nonce(r) + 1) + m.group(2), good)
    rng = random.Random(11); no_curve, no_prime = find_x(rng, 'off'), find_x(rng, 'no_prime')
    strings = [good, off, plaintext(TEMPLATE_ENTRIES, owner=no_curve), plaintext(TEMPLATE_ENTRIES, owner=no_prime, private=False), with_nonce(plaintext([], owner=0), r)]
    b0, f0, k0 = records.encrypt_many(strings, [r] * 5, host=True)
    b1, f1, k1 = records.encrypt_many(strings, [r] * 5, set_nonce=True, host=True)
    assert f0.tolist() == [0, 1, 2, 2, 0] and f1.tolist() == [0, 0, 2, 2, 0]
    assert b0.string(0) == b1.string(0) == b1.string(1) and b0.string(1) == '' and not k0[1].any() and k1[1].tobytes() == k0[0].tobytes()      # mode 1: the nonce replaced
    assert not k0[4].any() and payload_of(b0.string(4))[3:35] == le32(ps.hash_many_psd8([ENC_DOMAIN, 0], 1)[0])      # the owner x = 0 is the identity: rvk 0
    rc, s, _ = call_string(aleo_amd.lib().aleo_mi355x_record_encrypt, off.encode(), bs._vp(le32(r)), 0)
    assert rc == BAD_ARG and s == '' and 'nonce' in aleo_amd.lib().aleo_mi355x_last_error().decode()
    with pytest.raises(aleo_amd.AleoMi355xError): records.RecordPlaintext(off).encrypt(r)
    assert str(records.RecordPlaintext(off).encrypt(r, set_nonce=True)) == b0.string(0)


WRAP_TEMPLATE_ENTRIES, WRAP_RANDOMIZERS = [('v', 2, '%dfield' % (R - 1))], list(range(2, 14))


def test_a_sum_that_wraps_past_the_modulus():
    """plain + randomizer >= r for the owner's field: found among a few randomizers from what the host path itself says the record view key is."""
    G, vk, ax = account(); template = plaintext(WRAP_TEMPLATE_ENTRIES); wrapped = straight = 0
    batch, flags, rvk = records.encrypt_many([template] * 12, WRAP_RANDOMIZERS, set_nonce=True, host=True)
    for i in range(12):
        key = int.from_bytes(rvk[i].tobytes(), 'little'); rnd = ps.hash_many_psd8([ENC_DOMAIN, key], 3)
        bits = [0, 0] + [(2 >> k) & 1 for k in range(8)] + [(253 >> k) & 1 for k in range(16)] + [((R - 1) >> k) & 1 for k in range(253)] + [1]
        plain = [ax] + [sum(b << k for k, b in enumerate(bits[f:f + 252])) for f in (0, 252)]
        got = records.RecordCiphertext.from_string(batch.string(i)).fields()
        assert [int.from_bytes(g.tobytes(), 'little') for g in got] == [(p + q) % R for p, q in zip(plain, rnd)]
        wrapped += sum(p + q >= R for p, q in zip(plain, rnd)); straight += sum(p + q < R for p, q in zip(plain, rnd))
    assert wrapped >= 3 and straight >= 3


def test_malformed_strings_short_buffers_null_arguments_and_no_strings():
    L = aleo_amd.lib(); bad = [s for _, s in malformed_strings()]; r = le32(5)
    for mode in (False, True):
        batch, flags, rvk = records.encrypt_many(bad, [5] * len(bad), set_nonce=mode, host=True)
        assert flags.tolist() == [3] * len(bad) and batch.text == b'' and not batch.offsets.any() and not rvk.any()
    rc, s, _ = call_string(L.aleo_mi355x_record_encrypt, bad[0].encode(), bs._vp(r), 1)
    assert rc == BAD_ARG and s == '' and L.aleo_mi355x_last_error().decode().startswith(INVALID)
    assert call_string(L.aleo_mi355x_record_encrypt_symmetric, bad[0].encode(), bs._vp(r))[0] == BAD_ARG and L.aleo_mi355x_last_error().decode().startswith(INVALID)
    # a short buffer: BAD_ARG and the length; then exactly enough
    good = plaintext(TEMPLATE_ENTRIES).encode(); want = call_string(L.aleo_mi355x_record_encrypt, good, bs._vp(r), 1)[1]
    for cap in (1, 10, len(want)):
        rc, s, ln = call_string(L.aleo_mi355x_record_encrypt, good, bs._vp(r), 1, cap=cap)
        assert rc == BAD_ARG and ln == len(want)
    assert call_string(L.aleo_mi355x_record_encrypt, good, bs._vp(r), 1, cap=len(want) + 1)[:2] == (0, want)
    # null arguments, an unknown mode
    buf = ctypes.create_string_buffer(4096); ln = ctypes.c_size_t(4096)
    assert L.aleo_mi355x_record_encrypt(None, bs._vp(r), 1, buf, ctypes.byref(ln)) == BAD_ARG and L.aleo_mi355x_record_encrypt(good, None, 1, buf, ctypes.byref(ln)) == BAD_ARG
    assert L.aleo_mi355x_record_encrypt(good, bs._vp(r), 1, buf, None) == BAD_ARG and L.aleo_mi355x_record_encrypt(good, bs._vp(r), 2, buf, ctypes.byref(ln)) == BAD_ARG
    assert L.aleo_mi355x_record_encrypt_symmetric(good, None, buf, ctypes.byref(ln)) == BAD_ARG and L.aleo_mi355x_record_nonce(None, bs._vp(r)) == BAD_ARG
    b = records.RecordBatch.from_strings([good.decode()] * 2); text = records._text_p(b); rr = rows32([5, 6]); out = ctypes.c_void_p(7)
    for f in (L.aleo_mi355x_records_encrypt, L.aleo_mi355x_records_encrypt_host):
        assert f(None, text, bs._p(b.offsets), 2, bs._p(rr), 1) == BAD_ARG
        for args in ((text, None, 2, bs._p(rr), 1), (None, bs._p(b.offsets), 2, bs._p(rr), 1), (text, bs._p(b.offsets), 2, None, 1), (text, bs._p(b.offsets), 2, bs._p(rr), 2)):
            out.value = 7
            assert f(ctypes.byref(out), *args) == BAD_ARG and out.value is None
        assert f(ctypes.byref(out), None, bs._p(b.offsets[:1]), 0, None, 0) == 0 and out.value                     # n = 0: an empty result
        assert np.frombuffer(ctypes.string_at(L.aleo_mi355x_encrypted_offsets(out), 8), dtype=np.uint64).tolist() == [0]
        L.aleo_mi355x_encrypted_free(out)
    assert L.aleo_mi355x_encrypted_text(None) is None and L.aleo_mi355x_encrypted_free(None) is None
    for host in (True, False):
        batch, flags, rvk = records.encrypt_many([], [], host=host)
        assert len(batch) == 0 and flags.shape == (0,) and rvk.shape == (0, 32)


# ---- 4: the round trip --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def round_trip_rows():
    """(60 generated plaintexts — free whitespace, addresses 0 and 5 as values, structs and quoted strings among literals —, their randomizers)."""
    rng = random.Random(4242); strings = [random_plaintext(rng) for _ in range(60)]
    return strings, [rng.randrange(L_ORDER) for _ in strings]


def test_round_trip_through_the_host_scan_and_decryption():
    G, vk, ax = account(); strings, rs = round_trip_rows()
    batch, flags, rvk = records.encrypt_many(strings, rs, set_nonce=True, host=True)
    assert not flags.any()
    found = records.decrypt_strings(batch, vk, ax, host=True)
    assert found.index.tolist() == list(range(60)) and not found.status.any() and found.unparsed == 0
    assert found.rvk.tobytes() == rvk.tobytes()                                                                  # x(view key . nonce point) is x(r Owner)
    assert found.microcredits.tolist() == [PR.microcredits(s) for s in strings]
    privates = 0
    for k, s in enumerate(strings):
        want = records.RecordPlaintext(s); got = records.RecordCiphertext.from_string(batch.string(k)).plaintext(found.fields(k), ax)
        assert got.entries == want.entries and got.owner == want.owner and got.owner_visibility == want.owner_visibility and got.nonce == records.record_nonce(rs[k])
        if want.owner_visibility == 'private': assert found.fields(k)[0].tobytes() == le32(ax)
        privates += len(found.fields(k))
    assert privates >= 60
    stranger = 0x77777777777777777777 | 1
    f, kinds, _ = records.scan_strings(batch, [stranger], [le32(ps.ed_mul(G, stranger)[0])], host=True)
    assert not f.any() and set(kinds.tolist()) == {0, 1}


# ---- 5: the device lanes, emulated on the host ------------------------------------------------------------------------------------------------------------------------
def shaped(m):
    """A record of exactly m private fields: eight (m >= 16) or four two-field entries under a private (odd m) or public owner; m = 1: a private owner alone; 0: nothing private."""
    if m == 0: return plaintext([('a', 1, '5u64'), ('b', 0, 'true')], private=False)
    return plaintext([('f%d' % k, 2, '%dfield' % (R - 1 - k)) for k in range(m // 2)], private=m % 2 == 1)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(string, randomizer, set_nonce, routed by the lane)]: what the lanes compute — every literal type at its edges, whitespace variants, payloads of every length
    mod 5, m = 0, 1, 8, 9, 16, 17, the randomizers, owners and wrapping sums of test 3, the literal-only strings of test 4 — and what they route: the builder's
    structs and strings, test_plaintexts' routed and malformed, the strings of test 4 that hold a struct or a quoted string."""
    rng = random.Random(77); out = []
    for k, (_, s, _) in enumerate(computed_strings()): out.append((s, rng.randrange(L_ORDER), True, False))
    for k, (_, s, _) in enumerate(computed_strings()[:6]): r = rng.randrange(L_ORDER); out.append((with_nonce(s, r), r, False, False))
    out.append((computed_strings()[0][1], 99, False, False))                                                      # mode 0 and not the nonce: flag 1
    for n in range(1, 6): out.append((plaintext([('n' * n, 2, '200u8')]), rng.randrange(L_ORDER), True, False))   # the symbol writer's tail and padding
    for m in (0, 1, 8, 9, 16, 17): out.append((shaped(m), rng.randrange(L_ORDER), True, False))
    template = plaintext(TEMPLATE_ENTRIES)
    for r in EDGE_RANDOMIZERS: out.append((template, r, True, False))
    out.append((plaintext(TEMPLATE_ENTRIES, owner=find_x(rng, 'off')), 5, True, False)); out.append((plaintext(TEMPLATE_ENTRIES, owner=find_x(rng, 'no_prime'), private=False), 5, True, False))
    out.append((with_nonce(plaintext([], owner=0), 7), 7, False, False))
    for b, r, text in built_plaintexts(): out.append((text, r, False, lane_routes(text)))
    for _, s in routed_strings(): out.append((s, rng.randrange(L_ORDER), True, True))
    for _, s in malformed_strings(): out.append((s, rng.randrange(L_ORDER), True, True))
    for s, r in zip(*round_trip_rows()): out.append((s, r, True, lane_routes(s)))                                  # test 4's strings
    for r in WRAP_RANDOMIZERS: out.append((plaintext(WRAP_TEMPLATE_ENTRIES), r, True, False))                      # test 3's sums that wrap
    return out


def write_lane_cases(path, cases):
    """The case file of tests/cpp/records_encrypt_lane_emul.cpp, the rows the host path's; returns how many strings the lanes are to route."""
    want = {}
    for mode in (False, True):
        idx = [i for i, c in enumerate(cases) if c[2] == mode]
        batch, flags, rvk = records.encrypt_many([cases[i][0] for i in idx], [cases[i][1] for i in idx], set_nonce=mode, host=True)
        for k, i in enumerate(idx): want[i] = (int(flags[k]), batch.string(k).encode(), rvk[k].tobytes())
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for i, (s, r, mode, routed) in enumerate(cases):
            b = s.encode(); flag, text, key = want[i]
            f.write(struct.pack('<I', len(b)) + b + le32(r) + bytes([int(mode), 8 if routed else flag, flag]) + struct.pack('<I', len(text)) + text + key)
    return sum(1 for c in cases if c[3])


def lane_counts(r):
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    m = re.search(r'(\d+) strings, (\d+) encrypted, (\d+) nonce mismatches, (\d+) bad keys, (\d+) routed, (\d+) of them refused.*squeezes 0: (\d+), 1: (\d+), 2: (\d+), 3: (\d+)', r.stdout)
    return [int(v) for v in m.groups()]


@pytest.mark.parametrize('sanitized', [False, True])
def test_device_lanes_emulated_on_the_host_match_the_host_path(tmp_path, sanitized):
    """tests/cpp/records_encrypt_lane_emul.cpp: records_encrypt_lane.h compiled for the CPU over the checked restatement of fr29.h, a program of its own, once plain
    and once with the address and undefined-behaviour sanitizers, over the case file of tests 2-4's strings; the counts exactly."""
    cases = edge_cases(); path = os.path.join(str(tmp_path), 'cases.bin')
    routed = write_lane_cases(path, cases)
    r = bs.run_lane_emul(tmp_path, 'records_encrypt_lane_emul', [path], sanitized=sanitized)
    got = lane_counts(r)
    assert got[0] == len(cases) and got[4] == routed and got[5] == len(malformed_strings()) and got[2] == 1 and got[3] == 4, r.stdout[-600:]
    assert got[1] == len(cases) - routed - 5 and min(got[6:]) >= 1, r.stdout[-600:]                                # no squeeze, one, two and the third


def rows_of(n, mode=True):
    """n rows tiled from the edge set under one mode: (strings, randomizers, how many the lanes route).  From 63 rows on six routed and malformed strings stand
    between computed ones in the first wave."""
    cases = tiled(n, mode)
    return [c[0] for c in cases], [c[1] for c in cases], sum(1 for c in cases if c[3])


def tiled(n, mode):
    mine = [c for c in edge_cases() if c[2] == mode and not c[3]]; special = [c for c in edge_cases() if c[3]]
    out = [mine[i % len(mine)] for i in range(n)]
    if n >= 63:
        for j, c in enumerate(special[::len(special) // 6][:6]): out[5 + 9 * j] = c[:2] + (mode, True)
    return out


def test_the_gpu_batches_hold_the_routed_strings_their_tests_count(tmp_path):
    """The batches of the GPU tests through the lane emulation: what it routes of each is what its test asserts of records_encrypt_last_routed()."""
    exe = bs.build_lane_emul(tmp_path, 'records_encrypt_lane_emul')
    for n, mode in ((1, True), (63, True), (65, False)):
        path = os.path.join(str(tmp_path), 'batch.bin')
        assert write_lane_cases(path, tiled(n, mode)) == rows_of(n, mode)[2] == (6 if n >= 63 else 0)
        got = lane_counts(subprocess.run([exe, path], capture_output=True, text=True, timeout=600))
        assert got[0] == n and got[4] == rows_of(n, mode)[2]


# ---- 6-8: the code object, the threshold, the C++ mirror -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_encrypt_kernel_code_objects_are_gfx950_and_have_no_scratch():
    kernels = ['k_records_encrypt_keys', 'k_records_encrypt_sums', 'k_records_encrypt_text']
    assert bs.scratch_and_spills('records_encrypt', kernels) == (3, {k: (0, 0, 0) for k in kernels})


def test_routing_threshold_and_its_environment_override():
    default, five, nonsense = bs.threshold_reads('min_encrypt', 'ALEO_MI355X_MIN_ENCRYPT')
    assert five == 5 and nonsense == default and 1 <= default <= 1 << 20 and default & (default - 1) == 0


def test_last_routed_counts_every_string_of_a_host_call():
    strings, rs, _ = rows_of(7)
    records.encrypt_many(strings, rs, set_nonce=True, host=True)
    assert records.encrypt_last_routed() == 7
    records.encrypt_many(strings[:3], rs[:3], set_nonce=True)                                                     # below the threshold: the host path
    assert records.encrypt_last_routed() == 3


def run_cpp_mirror(tmp_path, env):
    r = bs.run_cpp_mirror(tmp_path, 'records_encrypt_test', [REF['view_keys']['owner'], REF['addresses']['owner'], REF['plaintexts']['owner'], REF['records']['owner'],
                                                             routed_strings()[0][1], 'string'], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_ENCRYPT': '1000000', 'ALEO_MI355X_MIN_RECORDS': '1000000'})


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_ENCRYPT', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0')
    monkeypatch.delenv('ALEO_MI355X_ENCRYPT_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_encrypt()) == 0
    return monkeypatch


def check_kernel_equals_host(strings, rs, routed, mode=True):
    got = records.encrypt_many(strings, rs, set_nonce=mode)
    assert records.encrypt_last_routed() == routed
    want = records.encrypt_many(strings, rs, set_nonce=mode, host=True)
    assert got[1].tolist() == want[1].tolist() and got[2].tobytes() == want[2].tobytes() and got[0].offsets.tolist() == want[0].offsets.tolist() and got[0].text == want[0].text
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_kernel_equals_the_host_path_at_wave_and_block_edges(on_kernel, n):
    strings, rs, routed = rows_of(n)
    batch, flags, rvk = check_kernel_equals_host(strings, rs, routed)
    assert set(flags.tolist()) == ({0, 2, 3} if n >= 63 else {0})
    strings, rs, routed = rows_of(n, False)                                                                          # upstream's encrypt: the nonce compared
    batch, flags, rvk = check_kernel_equals_host(strings, rs, routed, mode=False)
    assert set(flags.tolist()) == ({0, 1, 3} if n >= 63 else {0})


@pytest.mark.gpu
def test_kernel_launches_of_one_wave_continue_the_offsets(on_kernel):
    strings, rs, routed = rows_of(257)
    whole = check_kernel_equals_host(strings, rs, routed)
    on_kernel.setenv('ALEO_MI355X_ENCRYPT_CHUNK', '64')                                                              # five launches, the last one of one row
    cut = check_kernel_equals_host(strings, rs, routed)
    assert same(cut, whole)


@pytest.mark.gpu
def test_kernel_payloads_of_every_length_mod_5_and_every_squeeze_count(on_kernel):
    tails = [plaintext([('n' * n, 2, '200u8')]) for n in range(1, 6)]; shapes = [shaped(m) for m in (0, 1, 8, 9, 16, 17)]
    strings = [(tails + shapes)[i % 11] for i in range(66)]; rs = list(range(1000, 1066))
    batch, flags, rvk = check_kernel_equals_host(strings, rs, 0)
    assert not flags.any() and {len(payload_of(batch.string(i))) % 5 for i in range(5)} == {0, 1, 2, 3, 4}
    assert [len(records.RecordCiphertext.from_string(batch.string(i)).fields()) for i in range(5, 11)] == [0, 1, 8, 9, 16, 17]


@pytest.mark.gpu
def test_kernel_routes_structs_strings_and_long_strings_between_computed_rows(on_kernel):
    good = [c for c in edge_cases() if c[2] and not c[3]]; routed = [(s, 5 + k, True, True) for k, (_, s) in enumerate(routed_strings())]
    rows = []
    for k in range(70): rows.append(routed[(k // 7) % len(routed)] if k % 7 == 3 else good[k % len(good)])
    batch, flags, rvk = check_kernel_equals_host([c[0] for c in rows], [c[1] for c in rows], 10)
    assert all(flags[k] == 0 and batch.string(k).startswith('record1') for k in range(3, 70, 7))


@pytest.mark.gpu
def test_kernel_encrypts_the_reference_s_plaintext_and_the_device_decrypts_it(on_kernel):
    strings, rs, routed = rows_of(64); strings = strings[:40] + [REF['plaintexts']['owner']] + strings[40:]; rs = rs[:40] + [0xfeedface] + rs[40:]
    batch, flags, rvk = check_kernel_equals_host(strings, rs, routed)
    assert flags[40] == 0
    found = records.decrypt_strings(batch, REF['view_keys']['owner'], REF['addresses']['owner'])
    theirs = [i for i in range(65) if flags[i] == 0 and REF['addresses']['owner'] in strings[i]]                  # the reference's three plaintexts are among the edge set
    k = theirs.index(40)
    assert found.index.tolist() == theirs and found.microcredits[k] == 1500000000000000 and found.rvk[k].tobytes() == rvk[40].tobytes() and not found.status.any()
    mine = records.decrypt_strings(batch, account()[1], account()[2])
    assert mine.index.tolist() == [i for i in range(65) if flags[i] == 0 and i not in theirs] and not mine.status.any() and len(mine) >= 40


@pytest.mark.gpu
def test_first_call_of_a_fresh_process_and_two_threads_at_once(on_kernel):
    """tests/helpers/records_encrypt_first_calls.py, a process of its own: two threads whose first calls of the process are encrypt_many, so the one-time table build
    and upload run under both."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_ENCRYPT='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'records_encrypt_first_calls.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr
    strings, rs, routed = rows_of(130)
    want = records.encrypt_many(strings, rs, set_nonce=True, host=True)
    for g in bs.two_threads(lambda i: records.encrypt_many(strings, rs, set_nonce=True)): assert same(g, want)


@pytest.mark.gpu
def test_cpp_mirror_on_the_kernel(on_kernel, tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_ENCRYPT': '0', 'ALEO_MI355X_MIN_RECORDS': '0'})
