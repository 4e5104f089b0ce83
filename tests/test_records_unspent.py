"""unspent_strings / unspent_strings_many: the records each of K accounts owns among n "record1…" strings that decrypt, whose serial number computes and is not
in a set of spent serial numbers, in one call (aleo_mi355x_records_unspent_strings[_many][_host], found_serials, found_owned; unspent_strings[_many] in
aleo_amd/records.py and include/aleo_mi355x.hpp).

The yardstick is code from before these calls: for account j the one-account host result of decrypt_strings (Wanted.of of tests/test_records_found_many.py),
records.serial_numbers(cm[index], sk, host=True) over it, a Python set of the spent rows, and the rows the contract keeps: status 0, flag 0, not in the set.
The first half needs no GPU; the second half runs the kernels (ALEO_MI355X_MIN_RECORDS=0, MIN_DECRYPT=0, MIN_SERIALS=1) and compares every result with it."""
import ctypes, functools, os, random, re, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records
from test_records_found import same_found, differences
from test_records_found_many import MAIN, Wanted, key_bytes, keys_for, laid_out, layouts, mixed, pool_of
import batch_support as bs
from batch_support import SANITIZE, CSRC, HIPCC, le32
from test_records_serial import REC, SN, R, L_ORDER, field, rows, ints, reference_commitment, reference_sk_sig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def sk_for(j: int) -> int:
    """The sk_sigs cycle through the reference's, 0, 1, l - 1 and a seeded one."""
    return [reference_sk_sig(), 0, 1, L_ORDER - 1, random.Random(77).randrange(L_ORDER)][j % 5]


def account_of(who, sk: int) -> records.Account:
    vk, ax = key_bytes(who)
    return records.Account(None, le32(sk), records.view_key_bytes(vk), ax)


def seeded_commitments(n: int, seed: int) -> np.ndarray:
    rng = random.Random(seed)
    return rows([rng.randrange(R) for _ in range(n)])


class Yard:
    """The yardstick over one batch: per account its decrypt_strings host result and the host serial numbers of everything it owns, computed once."""
    def __init__(self, strings, whos, cm=None, seed=1):
        self.wanted = Wanted(strings); self.whos = list(whos); self.sks = [sk_for(j) for j in range(len(whos))]
        self.cm = seeded_commitments(len(strings), 900 + seed) if cm is None else cm
        self.accounts = [account_of(w, sk) for w, sk in zip(self.whos, self.sks)]
        self._sn = {}

    def owned(self, j):
        """(F, serial numbers, flags) of account j over everything it owns."""
        key = (self.whos[j], self.sks[j])
        if key not in self._sn:
            F = self.wanted.of(self.whos[j])
            self._sn[key] = (F,) + records.serial_numbers(self.cm[F.index.astype(np.int64)], le32(self.sks[j]), host=True)
        return self._sn[key]

    def want(self, j, spent: set) -> records.FoundRecords:
        F, sn, fl = self.owned(j)
        keep = [k for k in range(len(F)) if F.status[k] == 0 and fl[k] == 0 and sn[k].tobytes() not in spent]
        counts = [int(F.offsets[k + 1]) - int(F.offsets[k]) for k in keep]
        plain = np.concatenate([F.fields(k) for k in keep]) if keep else np.zeros((0, 32), dtype=np.uint8)
        return records.FoundRecords(F.index[keep], F.kind[keep], F.rvk[keep].reshape(-1, 32), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), plain.reshape(-1, 32),
                                    F.status[keep], F.microcredits[keep], F.unparsed, F.first_unparsed, sn[keep].reshape(-1, 32), len(F))

    def every_second(self, seed=5, foreign=40, duplicates=10) -> np.ndarray:
        """S: every second serial number of every account, `foreign` random rows, `duplicates` rows once more, shuffled."""
        rng = random.Random(seed); out = []
        for j in range(len(self.whos)):
            _, sn, fl = self.owned(j)
            out += [s.tobytes() for s, f in list(zip(sn, fl))[::2] if f == 0]
        out += [le32(rng.randrange(R)) for _ in range(foreign)]
        out += [out[rng.randrange(len(out))] for _ in range(duplicates)]
        rng.shuffle(out)
        return np.frombuffer(b''.join(out), dtype=np.uint8).reshape(-1, 32).copy()

    def call(self, spent, host=False):
        return records._unspent_found(self.wanted.batch, self.cm, self.accounts, spent, host)

    def check(self, spent, host=False):
        got = self.call(spent, host=host)
        S = {r.tobytes() for r in records._rows32(spent)}
        assert len(got) == len(self.whos)
        for j in range(len(self.whos)):
            want = self.want(j, S)
            assert same_found(got[j], want), ('key %d' % j, self.whos[j], differences(got[j], want), got[j].index.tolist()[:8], want.index.tolist()[:8])
            assert got[j].serials is not None and got[j].serials.shape == want.serials.shape and got[j].serials.tobytes() == want.serials.tobytes(), ('serials of key %d' % j, self.whos[j])
            assert got[j].owned == want.owned and not got[j].status.any(), ('owned of key %d' % j, got[j].owned, want.owned)
        return got


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------------------
def test_host_calls_equal_the_yardstick_on_the_mixed_batch():
    y = Yard(mixed(), [MAIN, 0, 1, 2])
    S = y.every_second()
    got = y.check(S, host=True)
    assert all(0 < len(g) < g.owned for g in got[:3]) and got[0].unparsed >= 7
    assert {0, 2, 4} <= set(y.owned(1)[0].status.tolist())                                     # the pools hold records that are never kept
    everything = y.check(np.zeros((0, 32), dtype=np.uint8), host=True)
    for j, g in enumerate(everything): assert len(g) == int((y.owned(j)[0].status == 0).sum()) > len(got[j])
    one = Yard(mixed(), [MAIN]); one.check(one.every_second(), host=True)                       # the one-account entry


def test_python_mirror_returns_what_unspent_returns():
    from test_records_serial import found_batch
    batch, cm, vk, ax = found_batch()
    acct = records.Account(None, le32(reference_sk_sig()), records.view_key_bytes(vk), records.address_x_bytes(ax))
    found = records.decrypt_strings(batch, vk, ax, host=True)
    all_sn, _ = records.serial_numbers(cm[found.index.astype(np.int64)], acct.sk_sig, host=True)
    spent = {s.tobytes() for s in all_sn[::2]}
    want, total = records.unspent(batch, cm, acct, lambda s: s in spent, host=True)
    for form in (list(spent), b''.join(spent), np.frombuffer(b''.join(spent), dtype=np.uint8).reshape(-1, 32)):
        got = records.unspent_strings(batch, cm, acct, form, host=True)
        assert [(int(i), s.tobytes(), int(m)) for i, s, m in zip(got.index, got.serials, got.microcredits)] == want and int(got.microcredits.astype(object).sum()) == total > 0
        assert got.owned == len(found) > len(got) > 0
    many = records.unspent_strings_many(batch, cm, [acct, acct], list(spent), host=True)
    assert len(many) == 2 and all(same_found(m, got) and m.serials.tobytes() == got.serials.tobytes() for m in many)
    assert len(records.unspent_strings(batch, cm, acct, host=True)) == len(records.unspent(batch, cm, acct, lambda s: False, host=True)[0])
    with pytest.raises(aleo_amd.AleoMi355xError): records.unspent_strings(['garbage'], cm[:1], acct, host=True)      # as unspent: a string that does not parse raises
    with pytest.raises(ValueError): records.unspent_strings(batch, cm[:5], acct, host=True)
    with pytest.raises(TypeError): records.unspent_strings([records.RecordCiphertext.from_string(REC['records']['owner'])], cm[:1], acct, host=True)
    # a result of decrypt_strings has no serial numbers, and owns what it holds
    assert found.serials is None and found.owned == len(found)


def reference_account() -> records.Account:
    """The reference's serial-number test signs with a private key that is not the record's owner's (wasm/src/record/record_plaintext.rs:131-140): its sk_sig,
    with the view key and the address that own the record."""
    return records.Account(None, records.Account.from_private_key(SN['private_key']).sk_sig, records.view_key_bytes(REC['view_keys']['owner']), records.address_x_bytes(REC['addresses']['owner']))


def check_reference_vector(copies: int, host: bool):
    strings = [REC['records']['owner']] * copies; acct = reference_account()
    cm = rows([reference_commitment()] * copies)
    expected = field(SN['expected'])
    got = records.unspent_strings(strings, cm, acct, host=host)
    assert got.index.tolist() == list(range(copies)) and ints(got.serials) == [expected] * copies and got.owned == copies
    assert got.microcredits.tolist() == [1500000000000000] * copies
    none = records.unspent_strings(strings, cm, acct, [le32(expected)], host=host)
    assert len(none) == 0 and none.owned == copies and none.serials.shape == (0, 32) and none.offsets.tolist() == [0]
    if host: assert len(records.unspent_strings(strings, cm, SN['private_key'], host=True)) == 0      # a private key string is an account too: this one owns nothing here


def test_the_reference_s_own_vector_on_the_host_path():
    check_reference_vector(1, host=True)


def test_refusals_and_edges():
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    GOOD = REC['records']['owner']
    text = (GOOD + 'garbage').encode(); tp = ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p)
    off = np.array([0, len(GOOD), len(text)], dtype=np.uint64)
    r32 = lambda *v: np.frombuffer(b''.join(le32(x) for x in v), dtype=np.uint8)
    cm = r32(reference_commitment(), 5); sk = r32(1, 0, L_ORDER - 1); vk = r32(1, 3, 5); ax = r32(5, 6, 7); sp = r32(9, 9)
    many65 = r32(*[1] * 65)
    for f, one in ((L.aleo_mi355x_records_unspent_strings_many_host, L.aleo_mi355x_records_unspent_strings_host), (L.aleo_mi355x_records_unspent_strings_many, L.aleo_mi355x_records_unspent_strings)):
        def refused(*args, K=3):
            out = (ctypes.c_void_p * 65)(*[1] * 65)
            assert f(out, *args) != 0
            assert all(out[j] is None for j in range(K)) and all(out[j] == 1 for j in range(K, 65))
            return L.aleo_mi355x_last_error()
        out = (ctypes.c_void_p * 3)()
        assert f(out, tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), 3, p(sp), 2) == 0
        for j in range(3):
            h = ctypes.c_void_p(out[j])
            assert L.aleo_mi355x_found_count(h) == 0 and L.aleo_mi355x_found_owned(h) == 0 and L.aleo_mi355x_found_unparsed(h) == 1 and L.aleo_mi355x_found_first_unparsed(h) == 1
            assert L.aleo_mi355x_found_serials(h)                                             # not NULL, even with nothing kept
            L.aleo_mi355x_found_free(h)
        assert b'null' in refused(tp, p(off), 2, None, p(sk), p(vk), p(ax), 3, p(sp), 2)
        assert b'null' in refused(tp, p(off), 2, p(cm), None, p(vk), p(ax), 3, p(sp), 2)
        assert b'null' in refused(tp, p(off), 2, p(cm), p(sk), None, p(ax), 3, p(sp), 2)
        assert b'null' in refused(tp, p(off), 2, p(cm), p(sk), p(vk), None, 3, p(sp), 2)
        assert b'null' in refused(None, p(off), 2, p(cm), p(sk), p(vk), p(ax), 3, p(sp), 2)
        assert b'null' in refused(tp, None, 2, p(cm), p(sk), p(vk), p(ax), 3, p(sp), 2)
        assert b'null spent set' in refused(tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), 3, None, 2)
        assert b'2^30' in refused(tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), 3, p(sp), 2 ** 30 + 1)
        for bad in (L_ORDER, 2 ** 256 - 1):
            msg = refused(tp, p(off), 2, p(cm), p(r32(1, 0, bad)), p(vk), p(ax), 3, p(sp), 2)
            assert b'subgroup order' in msg and b'key 2' in msg
        assert b'key 1' in refused(tp, p(off), 2, p(cm), p(sk), p(r32(1, L_ORDER, 5)), p(ax), 3, p(sp), 2)
        assert b'1..64' in refused(tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), 0, p(sp), 2, K=0)
        assert b'1..64' in refused(tp, p(off), 2, p(cm), p(many65), p(many65), p(many65), 65, p(sp), 2, K=65)
        assert f(None, tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), 3, p(sp), 2) != 0 and b'null result pointer' in L.aleo_mi355x_last_error()
        # n = 0, with and without a spent set; the one-account entry and its own refusal
        for spent_args in ((p(sp), 2), (None, 0)):
            out = (ctypes.c_void_p * 3)()
            assert f(out, None, None, 0, p(cm), p(sk), p(vk), p(ax), 3, *spent_args) == 0
            for j in range(3):
                h = ctypes.c_void_p(out[j])
                assert h.value and L.aleo_mi355x_found_count(h) == 0 and L.aleo_mi355x_found_fields(h) == 0 and L.aleo_mi355x_found_owned(h) == 0
                L.aleo_mi355x_found_free(h)
        h = ctypes.c_void_p()
        assert one(ctypes.byref(h), tp, p(off), 2, p(cm), p(sk), p(vk), p(ax), None, 0) == 0 and L.aleo_mi355x_found_count(h) == 0
        L.aleo_mi355x_found_free(h)
        assert one(ctypes.byref(h), tp, p(off), 2, p(cm), p(r32(L_ORDER)), p(vk), p(ax), None, 0) != 0 and b'key 0' in L.aleo_mi355x_last_error() and h.value is None
    # the accessors on the result of another call
    h = ctypes.c_void_p()
    a = reference_account()
    assert L.aleo_mi355x_records_decrypt_strings_host(ctypes.byref(h), tp, p(off), 2, p(np.frombuffer(a.view_key, dtype=np.uint8)), p(np.frombuffer(a.address_x, dtype=np.uint8))) == 0
    assert L.aleo_mi355x_found_count(h) == 1 and L.aleo_mi355x_found_owned(h) == 1 and not L.aleo_mi355x_found_serials(h)
    L.aleo_mi355x_found_free(h)
    assert not L.aleo_mi355x_found_serials(None) and L.aleo_mi355x_found_owned(None) == 0


def test_spent_lane_emulated_on_the_host_matches_std_set(tmp_path):
    """tests/cpp/records_spent_lane_emul.cpp: records_spent_lane.h compiled by the host compiler with the address and undefined-behaviour sanitizers, run as a
    program of its own; every answer is checked against std::set."""
    exe = os.path.join(str(tmp_path), 'records_spent_lane_emul')
    subprocess.check_call(['g++', '-std=c++17', '-O1'] + SANITIZE + ['-I', CSRC, os.path.join(HERE, 'cpp', 'records_spent_lane_emul.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ' 0 wrong answers' in r.stdout and 'wrapped' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_new_kernels_code_objects_are_gfx950_and_have_no_scratch():
    import code_object as co
    asm, blocks = co.compile_unit('records_unspent')
    for kernel in ('k_spent_insert', 'k_unspent_keep', 'k_unspent_scatter'):      # the serial-number kernel is records_serial.hip's: tests/test_records_serial.py
        meta = co.block_of(blocks, kernel)
        print(co.registers(kernel, meta))
        assert co.field(meta, 'private_segment_fixed_size') == 0 and co.field(meta, 'vgpr_spill_count') == 0, kernel


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '1000000', 'ALEO_MI355X_MIN_DECRYPT': '1000000'})


def run_cpp_mirror(tmp_path, env):
    """tests/cpp/records_unspent_test.cpp: unspent_strings and unspent_strings_many of include/aleo_mi355x.hpp on the reference's record, 70 copies among foreign ones."""
    strings = [REC['records']['owner'], REC['records']['sdk_foreign']] * 70
    r = bs.run_cpp_mirror(tmp_path, 'records_unspent_test', [SN['private_key'], REC['view_keys']['owner'], REC['addresses']['owner'], le32(reference_commitment()).hex(), le32(field(SN['expected'])).hex()] + strings, env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_DECRYPT', '0'); monkeypatch.setenv('ALEO_MI355X_MIN_SERIALS', '1')
    for name in ('ALEO_MI355X_SCAN_KEYS_PER_LANE', 'ALEO_MI355X_SCAN_CHUNK_CHARS', 'ALEO_MI355X_DECRYPT_CHUNK_FIELDS', 'ALEO_MI355X_SERIAL_CHUNK'): monkeypatch.delenv(name, raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0 and int(aleo_amd.lib().aleo_mi355x_min_serials()) == 1
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize('n,K', [(n, K) for n in (1, 63, 65, 257, 4099) for K in (1, 2, 3, 9)] + [(257, 64)])
def test_kernel_equals_the_yardstick_at_block_edges_and_key_counts(on_kernel, n, K):
    whos = keys_for(K)
    for what, strings in layouts(n, K):
        y = Yard(strings, whos, seed=n + K)
        got = y.check(y.every_second())
        if what.startswith('record i') and n >= 257:
            assert all(g.owned for g in got) and any(0 < len(g) < g.owned for g in got)
            if K >= 4: assert got[0].owned == got[3].owned and got[0].serials.tobytes() != got[3].serials.tobytes()      # the repeated account under another sk_sig


def segments_layout():
    """One chunk in which the keys own 0, 1, 63, 64, 65 and 130 records, in that key order, among foreign strings."""
    whos = [('filler', 40), ('filler', 1), 0, 1, 2, MAIN]
    slots = [s for s, c in enumerate((0, 1, 63, 64, 65, 130)) for _ in range(c)] + [None] * 77
    random.Random(12).shuffle(slots)
    return whos, laid_out(len(slots), whos, lambda i: slots[i])


@pytest.mark.gpu
def test_kernel_segment_boundaries_off_the_wave_grid(on_kernel):
    whos, strings = segments_layout()
    y = Yard(strings, whos)
    assert [len(y.owned(j)[0]) for j in range(6)] == [0, 1, 63, 64, 65, 130]
    got = y.check(y.every_second())
    assert [g.owned for g in got] == [0, 1, 63, 64, 65, 130]
    y.check(np.zeros((0, 32), dtype=np.uint8))
    on_kernel.setenv('ALEO_MI355X_SERIAL_CHUNK', '128')                                          # launches of two waves: they span the key boundaries
    y.check(y.every_second())


@pytest.mark.gpu
def test_kernel_spent_sets(on_kernel):
    whos = keys_for(3)
    y = Yard(laid_out(600, whos, lambda i: i % 4), whos)
    all_sn = [[s.tobytes() for s, f in zip(y.owned(j)[1], y.owned(j)[2]) if f == 0] for j in range(3)]
    # no set at all: a null pointer
    got = y.check(())
    assert all(len(g) == int((y.owned(j)[0].status == 0).sum()) for j, g in enumerate(got))
    # everything spent
    got = y.check([s for mine in all_sn for s in mine])
    assert all(len(g) == 0 and g.owned == len(y.owned(j)[0]) and g.unparsed == y.owned(j)[0].unparsed for j, g in enumerate(got)) and got[0].unparsed > 0
    # one row; and a serial number of account 0 leaves account 1's records alone
    one = y.owned(0)[1][[k for k in range(len(y.owned(0)[0])) if y.owned(0)[0].status[k] == 0][3]].tobytes()
    got = y.check([one])
    full = y.check(())
    assert len(got[0]) == len(full[0]) - 1 and same_found(got[1], full[1]) and same_found(got[2], full[2])
    # a chain of 70 crafted rows that share their first word with a REAL spent serial number, and wraps the table's end (72 rows: 256 slots); a row that differs
    # from another record's serial number in the last word only
    kept0 = full[0].serials
    wrap = [k for k in range(len(kept0)) if (int.from_bytes(kept0[k, :4].tobytes(), 'little') & 255) >= 256 - 40]
    assert wrap, 'no serial number of the batch starts near the end of a 256-slot table'
    a, b = wrap[0], (wrap[0] + 1) % len(kept0)
    rng = random.Random(8)
    crafted = [kept0[a, :4].tobytes() + bytes(rng.randrange(256) for _ in range(28)) for _ in range(70)]
    near = bytearray(kept0[b].tobytes()); near[31] ^= 1
    S = crafted[:35] + [kept0[a].tobytes()] + crafted[35:] + [bytes(near)]
    got = y.check(S)
    assert int(full[0].index[a]) not in got[0].index.tolist() and int(full[0].index[b]) in got[0].index.tolist() and len(got[0]) == len(full[0]) - 1


@pytest.mark.gpu
def test_kernel_malformed_commitments_at_wave_edges(on_kernel):
    """Rows r, r + 1 and 2^256 - 1 at the owned records of compact ranks 0, 63 and 64 (key 0 owns 100 records) and in the last partial wave of key 1's 100."""
    whos = [MAIN, 0]
    strings = laid_out(260, whos, lambda i: 0 if i < 100 else 1 if i < 200 else None)
    clean = Yard(strings, whos)
    F0, F1 = clean.owned(0)[0], clean.owned(1)[0]
    assert len(F0) == 100 and len(F1) == 100
    cm = clean.cm.copy()
    at = {int(F0.index[0]): R, int(F0.index[63]): R + 1, int(F0.index[64]): 2 ** 256 - 1, int(F1.index[97]): R, int(F1.index[99]): 2 ** 256 - 1}
    for i, v in at.items(): cm[i] = np.frombuffer(le32(v), dtype=np.uint8)
    y = Yard(strings, whos, cm=cm)
    assert [int(y.owned(j)[2].sum()) for j in range(2)] == [6, 4]                              # flag 2 each
    got = y.check(())
    want_clean = [clean.want(j, set()) for j in range(2)]
    for j in range(2):
        gone = set(at) & set(want_clean[j].index.tolist())
        assert gone and not (set(got[j].index.tolist()) & set(at))
        keep = [k for k, i in enumerate(want_clean[j].index.tolist()) if i not in at]
        assert got[j].index.tolist() == want_clean[j].index[keep].tolist() and got[j].serials.tobytes() == want_clean[j].serials[keep].tobytes()      # the neighbours are unchanged


@pytest.mark.gpu
def test_kernel_never_keeps_records_of_status_2_and_4(on_kernel):
    whos = [MAIN, 0, 1]
    y = Yard(laid_out(300, whos, lambda i: i % 3), whos)
    got = y.check(())
    seen = set()
    for j, g in enumerate(got):
        F = y.owned(j)[0]; seen |= set(F.status.tolist())
        assert g.index.tolist() == F.index[F.status == 0].tolist() and len(g) > 0
    assert {0, 2, 4} <= seen


@pytest.mark.gpu
def test_kernel_chunks(on_kernel):
    """The (4099, 3) layout of test_kernel_chunks_continue_indices_and_offsets_per_key in chunks of a fifth and a third of the text: an empty chunk, and a key with
    nothing in later chunks; serial launches of 128 lanes span the key boundaries, decrypt launches of 8 fields run alongside."""
    whos = keys_for(3); rng = random.Random(9)
    slot = [None if 1500 <= i < 2600 else 2 if i < 700 and i % 9 == 0 else rng.randrange(2) if rng.random() < 0.12 else None for i in range(4099)]
    y = Yard(laid_out(4099, whos, lambda i: slot[i]), whos)
    assert all(len(y.owned(j)[0]) > 70 for j in range(3)) and int(y.owned(2)[0].index.max()) < 700
    S = y.every_second()
    y.check(S)
    total = int(np.diff(y.wanted.batch.offsets.astype(np.int64)).sum())
    for chars, serial, fields in ((total // 5, None, None), (total // 5, '128', None), (total // 3, '128', '8'), (None, '128', '8')):
        for name, v in (('ALEO_MI355X_SCAN_CHUNK_CHARS', chars), ('ALEO_MI355X_SERIAL_CHUNK', serial), ('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', fields)):
            if v: on_kernel.setenv(name, str(v))
            else: on_kernel.delenv(name, raising=False)
        y.check(S)


@pytest.mark.gpu
def test_kernel_and_host_serial_numbers_inside_the_call_give_the_same_bytes(on_kernel):
    """Below min_serials owned pairs the calling thread computes the serial numbers inside the device flow: both sides of the boundary."""
    whos, strings = segments_layout()
    y = Yard(strings, whos)
    pairs = sum(len(y.owned(j)[0]) for j in range(6))
    S = y.every_second()
    for threshold in (pairs, pairs + 1):
        on_kernel.setenv('ALEO_MI355X_MIN_SERIALS', str(threshold))
        y.check(S)


@pytest.mark.gpu
def test_kernel_gives_the_reference_s_serial_number_in_every_lane(on_kernel):
    check_reference_vector(65, host=False)


@pytest.mark.gpu
def test_kernel_mirrors(on_kernel, tmp_path):
    test_python_mirror_returns_what_unspent_returns()
    from test_records_serial import found_batch
    batch, cm, vk, ax = found_batch()
    acct = records.Account(None, le32(reference_sk_sig()), records.view_key_bytes(vk), records.address_x_bytes(ax))
    want, total = records.unspent(batch, cm, acct, lambda s: False, host=True)
    got = records.unspent_strings(batch, cm, acct)
    assert [(int(i), s.tobytes(), int(m)) for i, s, m in zip(got.index, got.serials, got.microcredits)] == want
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '0', 'ALEO_MI355X_MIN_DECRYPT': '0', 'ALEO_MI355X_MIN_SERIALS': '1'})


@pytest.mark.gpu
def test_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    """tests/helpers/unspent_two_threads.py, a process of its own: there the two calls are the first of the process, so the one-time table build and the
    spent-set build run under both."""
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SERIALS='1', ALEO_MI355X_MIN_RECORDS='0', ALEO_MI355X_MIN_DECRYPT='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'helpers', 'unspent_two_threads.py')], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok'], r.stdout + r.stderr
