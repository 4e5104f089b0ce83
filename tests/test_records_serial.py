"""A record's serial number: Record::serial_number for batches (aleo_mi355x_records_serial_numbers / _host, found_serial_numbers), with the host-only calls around it
(record_commitment, record_checksum, account_from_private_key) and their mirrors in aleo_amd/records.py (serial_numbers, Account, unspent, …).

Three layers, each checked against the one before:  the reference's own data (tests/golden/reference_serial.json, reference_account.json, reference_records.json)
pins the restatement in plain Python integers (tests/serial_ref.py), stage by stage;  the restatement and the same data check the product's host path through the
C ABI;  the host path, byte for byte, checks the device lane — emulated on the CPU under the sanitizers here, and on the GPU in the second half
(ALEO_MI355X_MIN_SERIALS=1).  No test reads the reference tree."""
import ctypes, functools, json, os, random, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records
from oracle import poseidon as ps, pyref as P
import serial_ref as S
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32

ACC = json.load(open(os.path.join(HERE, 'golden', 'reference_account.json')))
REC = json.load(open(os.path.join(HERE, 'golden', 'reference_records.json')))
SER = json.load(open(os.path.join(HERE, 'golden', 'reference_serial.json')))
R, L_ORDER = P.FR_MODULUS, ps.ED_SUBGROUP_ORDER
TX, SN = SER['transaction_output'], SER['serial_number']


def field(s: str) -> int: assert s.endswith('field'); return int(s[:-5])
def rows(vals) -> np.ndarray: return np.frombuffer(b''.join(le32(v) for v in vals), dtype=np.uint8).reshape(-1, 32).copy() if len(vals) else np.zeros((0, 32), dtype=np.uint8)
def ints(a) -> list: return [int.from_bytes(r.tobytes(), 'little') for r in a]


# ---- 1: the restatement alone, against what the reference holds ---------------------------------------------------------------------------------------------
def test_pin_1_hash_to_curve_gives_the_account_generator_and_every_reference_account():
    a0 = ACC['accounts'][0]
    G = ps.ed_mul(ps.address_point(a0['address']), pow(ps.view_key_scalar(a0['view_key']), -1, L_ORDER))      # view_key^-1 * address, as tests/test_poseidon.py recovers it
    assert S.account_generator() == G
    for a in ACC['accounts']:
        _, view, addr = S.account_from_private_key(a['private_key'])
        assert (ps.view_key_string(view), ps.address_string(addr)) == (a['view_key'], a['address']), a['source']


def test_pin_2_bhp1024_of_the_ciphertext_bits_is_the_transaction_output_s_checksum():
    assert S.record_checksum(TX['value']) == field(TX['checksum'])


def test_pin_3_the_plaintext_s_commitment_is_the_transaction_output_s_id():
    a = ACC['accounts'][2]
    plain = S.record_decrypt_fields(TX['value'], ps.view_key_scalar(a['view_key']))
    assert plain[0] == ps.address_point(a['address'])[0]                                        # the third account owns it
    assert ps.plaintext_from_fields(plain[1:]) == ('literal', 12, 1, 64)                        # its one private entry: 1u64
    assert S.record_commitment(TX['value'], plain, TX['program_id'], TX['record_name']) == field(TX['id'])


@functools.lru_cache(maxsize=None)
def reference_commitment() -> int:
    plain = S.record_decrypt_fields(REC['records']['owner'], ps.view_key_scalar(REC['view_keys']['owner']))
    return S.record_commitment(REC['records']['owner'], plain, SN['program_id'], SN['record_name'])


@functools.lru_cache(maxsize=None)
def reference_sk_sig() -> int: return S.account_from_private_key(SN['private_key'])[0]


def test_pin_4_the_serial_number_of_the_reference_s_test():
    assert S.serial_number(reference_sk_sig(), reference_commitment()) == field(SN['expected'])


# ---- 2: the product's host path, through the C ABI -------------------------------------------------------------------------------------------------------------
def test_account_from_private_key_reproduces_the_reference_accounts():
    for a in ACC['accounts']:
        acct = records.Account.from_private_key(a['private_key'])
        assert (acct.view_key_string, acct.address) == (a['view_key'], a['address']), a['source']
        assert acct.view_key == records.view_key_bytes(a['view_key']) and acct.address_x == records.address_x_bytes(a['address'])
        assert int.from_bytes(acct.sk_sig, 'little') == S.account_from_private_key(a['private_key'])[0]
    L = aleo_amd.lib(); only = np.zeros(32, dtype=np.uint8)                                      # any output may be NULL
    assert L.aleo_mi355x_account_from_private_key(SN['private_key'].encode(), None, None, only.ctypes.data_as(ctypes.c_void_p)) == 0 and only.any()
    for bad in ('garbage', SN['private_key'][:-1], 'AViewKey1' + SN['private_key'][9:], ''):
        with pytest.raises(aleo_amd.AleoMi355xError): records.Account.from_private_key(bad)


def test_record_checksum_is_the_transaction_output_s():
    assert records.record_checksum(TX['value']) == le32(field(TX['checksum']))
    with pytest.raises(aleo_amd.AleoMi355xError): records.record_checksum('garbage')


def test_record_commitment_is_the_transaction_output_s_id():
    a = ACC['accounts'][2]
    plain = records.RecordCiphertext.from_string(TX['value']).decrypt(a['view_key'], a['address'])
    assert plain.microcredits() == 1
    fields = records.RecordCiphertext.from_string(TX['value']).decrypted_fields(a['view_key'])
    assert records.record_commitment(TX['value'], fields, TX['program_id'], TX['record_name']) == le32(field(TX['id']))
    with pytest.raises(aleo_amd.AleoMi355xError): records.record_commitment(TX['value'], fields[:1], TX['program_id'], TX['record_name'])      # not the record's own count


def test_the_chain_through_the_product_gives_the_reference_s_serial_number():
    rec = records.RecordCiphertext.from_string(REC['records']['owner'])
    fields = rec.decrypted_fields(REC['view_keys']['owner'])
    cm = records.record_commitment(rec, fields, SN['program_id'], SN['record_name'])
    assert cm == le32(reference_commitment())
    acct = records.Account.from_private_key(SN['private_key'])
    sn, flags = records.serial_numbers([cm], acct.sk_sig, host=True)
    assert flags.tolist() == [0] and '%dfield' % ints(sn)[0] == SN['expected']
    plain = rec.decrypt(REC['view_keys']['owner'], REC['addresses']['owner'])
    assert plain.string == REC['plaintexts']['owner']
    assert plain.serial_number_string(SN['private_key'], SN['program_id'], SN['record_name']) == SN['expected']
    assert plain.serial_number_string(acct, SN['program_id'], SN['record_name']) == SN['expected']      # twice with the same key (record_plaintext.rs:143-151)


def test_serial_number_string_raises_with_the_reference_s_messages():
    plain = records.RecordCiphertext.from_string(REC['records']['owner']).decrypt(REC['view_keys']['owner'], REC['addresses']['owner'])
    assert len(SER['errors']) == 2
    for e in SER['errors']:
        with pytest.raises(aleo_amd.AleoMi355xError) as err: plain.serial_number_string(SN['private_key'], e['program_id'], e['record_name'])
        assert str(err.value) == e['message'], e['source']
    for program_id in ('credits', 'credits.eth', '.aleo', '1credits.aleo', 'a' * 32 + '.aleo'):
        with pytest.raises(aleo_amd.AleoMi355xError) as err: plain.serial_number_string(SN['private_key'], program_id, 'credits')
        assert str(err.value) == SER['errors'][0]['message']
    for name in ('', '_credits', '9lives', 'a' * 32):
        with pytest.raises(aleo_amd.AleoMi355xError) as err: plain.serial_number_string(SN['private_key'], 'credits.aleo', name)
        assert str(err.value) == SER['errors'][1]['message']


# ---- 3: the host path against the restatement ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def commitments_64() -> tuple:
    rng = random.Random(0x5E41A1)
    return tuple([0, 1, R - 1, reference_commitment(), field(TX['id'])] + [rng.randrange(R) for _ in range(59)])


def keys() -> list: return [0, 1, L_ORDER - 1, reference_sk_sig()]


@functools.lru_cache(maxsize=None)
def restated(sk: int, cms: tuple) -> tuple:
    """The restatement's (serial numbers, flags), computed once per (key, commitments) and shared."""
    out = [S.serial_number(sk, c) for c in cms]
    return tuple(0 if v is None else v for v in out), tuple(2 if v is None else 0 for v in out)


@pytest.mark.parametrize('which', range(4))
def test_host_path_equals_the_restatement_on_64_commitments(which):
    sk, cms = keys()[which], commitments_64()
    sn, flags = records.serial_numbers(rows(cms), le32(sk), host=True)
    want_sn, want_flags = restated(sk, cms)
    assert flags.tolist() == list(want_flags) and ints(sn) == list(want_sn)
    assert len(set(ints(sn))) == 64


# ---- 4: refusals and edges -------------------------------------------------------------------------------------------------------------------------------------
EDGE = {3: R, 9: 2 ** 256 - 1}


def with_edges(n: int, seed: int, at: dict) -> np.ndarray:
    """n seeded commitments: the edge set first (0, 1, r - 1, the two reference commitments), the malformed ones of `at` at their places."""
    rng = random.Random(seed)
    vals = ([0, 1, R - 1, reference_commitment(), field(TX['id'])] + [rng.randrange(R) for _ in range(n)])[:n]
    for i, v in at.items(): vals[i] = v
    return rows(vals)


def check_malformed(sn, flags, cm, at):
    for i in range(len(cm)):
        if i in at: assert flags[i] == 2 and not sn[i].any(), i
        else: assert flags[i] == 0 and sn[i].any(), i


def test_malformed_commitments_get_flag_2_and_a_zero_row_and_leave_their_neighbours_alone():
    sk = le32(reference_sk_sig())
    cm = with_edges(12, 4, EDGE)
    sn, flags = records.serial_numbers(cm, sk, host=True)
    check_malformed(sn, flags, cm, EDGE)
    clean = with_edges(12, 4, {})
    sn2, flags2 = records.serial_numbers(clean, sk, host=True)
    keep = [i for i in range(12) if i not in EDGE]
    assert (sn[keep] == sn2[keep]).all() and not flags2.any()


def test_a_key_that_is_not_below_the_subgroup_order_refuses_the_call_and_an_empty_batch_is_fine():
    cm = with_edges(3, 5, {})
    for host in (True, False):                                                                   # three commitments: below min_serials, the call stays on the host
        with pytest.raises(aleo_amd.AleoMi355xError): records.serial_numbers(cm, le32(L_ORDER), host=host)
        with pytest.raises(aleo_amd.AleoMi355xError): records.serial_numbers(cm, le32(2 ** 256 - 1), host=host)
        sn, flags = records.serial_numbers(rows([]), le32(1), host=host)
        assert sn.shape == (0, 32) and flags.shape == (0,)
    L = aleo_amd.lib()
    assert L.aleo_mi355x_records_serial_numbers_host(None, None, None, 0, le32(1)) == 0
    assert L.aleo_mi355x_records_serial_numbers_host(None, None, None, 1, le32(1)) != 0
    assert L.aleo_mi355x_records_serial_numbers_host(None, None, None, 0, None) != 0


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_serials', 'ALEO_MI355X_MIN_SERIALS') == (64, 5, 64)


# ---- 5: the device lane, emulated on the host under the sanitizers ------------------------------------------------------------------------------------------------
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path):
    """tests/cpp/records_serial_lane_emul.cpp: records_serial_lane.h compiled for the CPU (plain C++, the host compiler, as tools/asan_records_found.sh builds its
    program) over the checked restatement of fr29.h, with the address and undefined-behaviour sanitizers, and run as a program of its own on the 64 commitments of
    part 3 (the reference's sk_sig first among its keys); what its host path writes is what the library returns."""
    cms, out, key = (os.path.join(str(tmp_path), name) for name in ('commitments.bin', 'host_rows.bin', 'key.bin'))
    exe = bs.build_lane_emul(tmp_path, 'records_serial_lane_emul', sanitized=True, flags=())
    open(cms, 'wb').write(rows(commitments_64()).tobytes()); open(key, 'wb').write(le32(reference_sk_sig()))
    r = subprocess.run([exe, cms, out, key], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and ' 0 mismatches, 0 table mismatches, 0 limb-rule violations' in r.stdout and '256 commitments' in r.stdout, r.stdout + r.stderr
    sn, flags = records.serial_numbers(rows(commitments_64()), le32(reference_sk_sig()), host=True)
    want = b''.join(bytes([int(f)]) + s.tobytes() for f, s in zip(flags, sn))
    assert open(out, 'rb').read() == want
    # its built-in commitments hold the malformed rows, and the lane-level Elligator2 on 0, which no hash reaches
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and ' 8 refused, 0 mismatches, 0 table mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_serial_kernel_code_object_is_gfx950_and_has_no_scratch():
    assert bs.scratch_and_spills('records_serial', ['k_records_serial'])[1]['k_records_serial'][:2] == (0, 0)      # no private segment, no VGPR spills


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_SERIALS', '1'); monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0')
    monkeypatch.delenv('ALEO_MI355X_SERIAL_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_serials()) == 1
    return monkeypatch


def check_kernel_equals_host(cm, sk):
    want_sn, want_flags = records.serial_numbers(cm, sk, host=True)
    sn, flags = records.serial_numbers(cm, sk)
    assert flags.tobytes() == want_flags.tobytes() and sn.tobytes() == want_sn.tobytes(), np.flatnonzero((sn != want_sn).any(axis=1) | (flags != want_flags)).tolist()[:8]
    return sn, flags


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 300])
def test_kernel_equals_the_host_path_at_wave_and_block_edges(on_kernel, n):
    cm, sk = with_edges(n, 100 + n, {}), le32(reference_sk_sig())
    sn, flags = check_kernel_equals_host(cm, sk)
    assert not flags.any() and len({r.tobytes() for r in sn}) == n
    if n == 300:                                                                                 # three launches, the last one partial
        on_kernel.setenv('ALEO_MI355X_SERIAL_CHUNK', '128')
        again, _ = check_kernel_equals_host(cm, sk)
        assert again.tobytes() == sn.tobytes()


@pytest.mark.gpu
def test_one_key_through_the_segmented_kernel_in_one_wave_launches(on_kernel):
    """One key is one segment of the kernel that records_unspent.hip launches over several: at ALEO_MI355X_SERIAL_CHUNK=64, 129 commitments are chunks of 64, 64 and 1,
    each one launch of one wave over one segment, the last wave holding one lane."""
    on_kernel.setenv('ALEO_MI355X_SERIAL_CHUNK', '64')
    cm, sk = with_edges(129, 229, {}), le32(reference_sk_sig())
    sn, flags = check_kernel_equals_host(cm, sk)
    assert not flags.any() and len({r.tobytes() for r in sn}) == 129


@pytest.mark.gpu
def test_kernel_malformed_rows_at_lane_0_at_lane_63_and_in_the_last_partial_wave(on_kernel):
    at = {0: R, 63: 2 ** 256 - 1, 64: R + 1, 297: 2 ** 256 - 1, 299: R}
    cm = with_edges(300, 7, at)
    sn, flags = check_kernel_equals_host(cm, le32(reference_sk_sig()))
    check_malformed(sn, flags, cm, at)


@pytest.mark.gpu
@pytest.mark.parametrize('sk', [0, 1, L_ORDER - 1])
def test_kernel_edge_keys(on_kernel, sk):
    sn, flags = check_kernel_equals_host(with_edges(65, 11, {}), le32(sk))
    assert not flags.any()
    with pytest.raises(aleo_amd.AleoMi355xError): records.serial_numbers(with_edges(65, 11, {}), le32(L_ORDER))


@pytest.mark.gpu
def test_kernel_gives_the_reference_s_serial_number_in_every_lane(on_kernel):
    sn, flags = records.serial_numbers([reference_commitment()] * 65, records.Account.from_private_key(SN['private_key']))
    assert not flags.any() and ints(sn) == [field(SN['expected'])] * 65


@functools.lru_cache(maxsize=None)
def found_batch():
    """200 strings laid out of the pools of tests/test_records_found.py (those that parse: a record read off the chain does), about a quarter of them the
    account's; a seeded commitment for each."""
    from test_records_found import pools, shuffled_cases
    _, _, vk, ax = shuffled_cases()
    owned, foreign = pools(); rng = random.Random(20077)
    foreign = [s for s, k in zip(foreign, records.parse_many(records.RecordBatch.from_strings(foreign), host=True)[0]) if k >= 0]
    strings = [owned[(i * 7) % len(owned)] if rng.random() < 0.25 else foreign[rng.randrange(len(foreign))] for i in range(200)]
    return records.RecordBatch.from_strings(strings), rows([rng.randrange(R) for _ in range(200)]), vk, ax


@pytest.mark.gpu
def test_found_serial_numbers_equal_the_host_path_on_the_gathered_commitments(on_kernel):
    batch, cm, vk, ax = found_batch()
    sk = le32(reference_sk_sig())
    found = records.decrypt_strings(batch, vk, ax)
    assert 30 <= len(found) <= 70
    want_sn, want_flags = records.serial_numbers(cm[found.index.astype(np.int64)], sk, host=True)
    sn, flags = records.found_serial_numbers(found, cm, sk)
    assert sn.tobytes() == want_sn.tobytes() and flags.tobytes() == want_flags.tobytes() and not flags.any()
    # and the C call, on a result the library still owns
    L = aleo_amd.lib(); out = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    vkb, axb = np.frombuffer(records.view_key_bytes(vk), dtype=np.uint8), np.frombuffer(records.address_x_bytes(ax), dtype=np.uint8)
    aleo_amd._lib.check(L.aleo_mi355x_records_decrypt_strings(ctypes.byref(out), ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p), p(batch.offsets), len(batch), p(vkb), p(axb)), 'records_decrypt_strings')
    try:
        c = int(L.aleo_mi355x_found_count(out)); assert c == len(found)
        sn2 = np.zeros((c, 32), dtype=np.uint8); fl2 = np.full(c, 9, dtype=np.uint8); skb = np.frombuffer(sk, dtype=np.uint8)
        aleo_amd._lib.check(L.aleo_mi355x_found_serial_numbers(out, p(cm), len(batch), p(skb), p(sn2), p(fl2)), 'found_serial_numbers')
        assert sn2.tobytes() == want_sn.tobytes() and fl2.tobytes() == want_flags.tobytes()
        assert L.aleo_mi355x_found_serial_numbers(out, p(cm), int(found.index.max()), p(skb), p(sn2), p(fl2)) != 0      # fewer commitments than strings
    finally:
        L.aleo_mi355x_found_free(out)


def check_unspent(host):
    batch, cm, vk, ax = found_batch()
    acct = records.Account(None, le32(reference_sk_sig()), records.view_key_bytes(vk), records.address_x_bytes(ax))
    found = records.decrypt_strings(batch, vk, ax, host=True)
    all_sn, all_flags = records.serial_numbers(cm[found.index.astype(np.int64)], acct.sk_sig, host=True)
    spent = {s.tobytes() for s in all_sn[::2]}                                                   # every second serial number is on chain
    want = [(int(i), all_sn[k].tobytes(), int(found.microcredits[k])) for k, i in enumerate(found.index) if found.status[k] == 0 and all_flags[k] == 0 and all_sn[k].tobytes() not in spent]
    got, total = records.unspent(batch, cm, acct, lambda s: s in spent, host=host)
    assert got == want and total == sum(m for _, _, m in want) and 0 < len(got) < len(found) and total > 0
    assert records.unspent(batch, cm, acct, lambda s: True, host=host) == ([], 0)
    everything, _ = records.unspent(batch, cm, acct, lambda s: False, host=host)
    assert len(everything) == int(((found.status == 0) & (all_flags == 0)).sum()) > len(got)
    with pytest.raises(aleo_amd.AleoMi355xError): records.unspent(['garbage'], cm[:1], acct, lambda s: False, host=host)      # as balance: a string that does not parse raises


def test_unspent_on_the_host_path():
    check_unspent(True)


@pytest.mark.gpu
def test_unspent_equals_the_same_computation_done_with_the_host_calls(on_kernel):
    check_unspent(False)


@pytest.mark.gpu
def test_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    """tests/helpers/serial_two_threads.py, a process of its own: there the two calls are the first of the process, so the one-time table build runs under both."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SERIALS='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'serial_two_threads.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr
