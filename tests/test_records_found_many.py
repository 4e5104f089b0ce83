"""decrypt_strings_many: the records each of K accounts owns among n "record1…" strings, decrypted, in one call (aleo_mi355x_records_decrypt_strings_many /
_many_host; decrypt_strings_many, balances and decrypt_owned_many in aleo_amd/records.py; decrypt_strings_many and balances in include/aleo_mi355x.hpp).

The one contract: result j is, byte for byte — every array, unparsed and first_unparsed — what the one-account host call (decrypt_strings(…, host=True), the
yardstick of tests/test_records_found.py) returns for key j alone over the same strings.  The first half needs no GPU; the second half runs the kernels
(ALEO_MI355X_MIN_RECORDS=0) and compares every result with the host path."""
import ctypes, functools, os, random, struct, subprocess
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps
import batch_support as bs
from batch_support import le32
from test_records import REF, R, L_ORDER, account_generator
from test_records_strings import encode, payload_of
from test_records_decrypt import Built, account, string_of_fields
from test_records_found import shuffled_cases, pools, pattern, same_found, differences, good_strings, off_curve_nonce, private_entry, on_host, on_kernel      # noqa: F401 (the last two: fixtures)

MAIN = 'main'                                                                                                      # the account of the case list


@functools.lru_cache(maxsize=None)
def extra_accounts():
    """Three more accounts under the generator of the case list's: view key 1 (its address is the generator), and two of ordinary size."""
    G = account_generator()
    return [(vk, ps.ed_mul(G, vk)[0]) for vk in (1, 0x55555555555555555555555555555 | 1, 0x31415926535897932384626433 | 1)]


@functools.lru_cache(maxsize=None)
def pool_of(who):
    """(view key, address x, the strings the account owns, their statuses).  MAIN: the case list's pool, every status and 0…17 fields.  0, 1, 2: an extra account
    with records of 0, 1, 2, 3 and 5 private fields, one that record_fields refuses and one whose nonce is not on the curve.  ('filler', t): an account that
    owns one record with a public owner and nothing private — its view key has nothing to do with its address, which a public owner never asks."""
    G = account_generator()
    if who == MAIN:
        cases, _, vk, ax = shuffled_cases()
        return vk, int.from_bytes(ax, 'little'), [s for _, s, o, _ in cases if o], [st for _, _, o, st in cases if o]
    if isinstance(who, tuple):
        rng = random.Random(4000 + who[1]); ax = rng.randrange(R)
        return 3 + 2 * who[1], ax, [encode(payload_of(False, ax, rng.randrange(R), [(b'microcredits', b'\x01\x00\x0c\x00' + struct.pack('<Q', 100 + who[1]))]))], [0]
    vk, ax = extra_accounts()[who]; rng = random.Random(3000 + who)
    built = lambda private, entries, seed: Built(G, vk, ax, private, entries, 900 + 10 * who + seed).string
    first = built(True, [('microcredits', 2, ('lit', 12, 9 + who)), ('pad', 2, string_of_fields(2))], 0)             # the layout the case list's refusals are cut from
    base = wire.bech32m_decode(first)[1]
    assert base[36] == 12 and base[51] == 2
    strings = [first, built(True, [], 1), built(False, [('pad', 2, string_of_fields(5))], 2), built(True, [('microcredits', 2, ('lit', 12, 7000 + who))], 3),
               encode(payload_of(False, ax, int.from_bytes(base[-32:], 'little'), [(b'microcredits', b'\x01\x00\x0c\x00' + struct.pack('<Q', 31 + who))])),
               encode(base[:51] + b'\x03' + base[52:]),
               encode(payload_of(False, ax, off_curve_nonce(), [(b'v', private_entry([rng.randrange(R)]))]))]
    return vk, ax, strings, [0, 0, 0, 0, 0, 4, 2]


def keys_for(K):
    """K accounts: the case list's first, view key 1 next, a repeated key from four on, fillers from six on."""
    order = [MAIN, 0, 1, MAIN, 2] + [('filler', t) for t in range(K)]
    return order[:K]


def key_bytes(who):
    vk, ax, _, _ = pool_of(who)
    return vk, le32(ax)


@functools.lru_cache(maxsize=None)
def foreign_strings():
    return pools()[1]


def laid_out(n, whos, slot_of, seed=0):
    """n strings: record i is drawn from the pool of whos[slot_of(i)], or from the foreign strings where slot_of(i) is None or past the last key."""
    rng = random.Random(7000 * n + len(whos) + seed); foreign = foreign_strings()[:48]                             # the case list's, unparsable ones among them, and random ones
    out = []
    for i in range(n):
        s = slot_of(i)
        if s is None or s >= len(whos): out.append(foreign[rng.randrange(len(foreign))]); continue
        mine = pool_of(whos[s])[2]
        out.append(mine[(i * 7 + i // 256) % len(mine)])
    return out


@functools.lru_cache(maxsize=None)
def alone(who, string):
    """The one-account host call over this one string."""
    return records.decrypt_strings([string], *key_bytes(who), host=True)


def assembled(strings, who):
    """What the one-account host call returns over `strings`, put together from its answers for every distinct string alone: the host path looks at one record
    at a time (tests/test_records_found.py compares it with a record-by-record composition), so the batches here, which repeat a few hundred strings, need one
    host scan per distinct (key, string) and not per pair.  test_host_path_… below holds this against the call itself."""
    index, kind, rvk, offsets, plain, status, mc, unparsed, first = [], [], [], [0], [], [], [], 0, len(strings)
    for i, s in enumerate(strings):
        f = alone(who, s)
        if f.unparsed: unparsed += 1; first = min(first, i)
        if len(f): index.append(i); kind.append(f.kind[0]); rvk.append(f.rvk[0]); plain.append(f.plain); offsets.append(offsets[-1] + len(f.plain)); status.append(f.status[0]); mc.append(f.microcredits[0])
    return records.FoundRecords(np.array(index, dtype=np.uint32), np.array(kind, dtype=np.int8), np.stack(rvk) if rvk else np.zeros((0, 32), dtype=np.uint8), np.array(offsets, dtype=np.uint32),
                                np.concatenate(plain) if plain else np.zeros((0, 32), dtype=np.uint8), np.array(status, dtype=np.uint8), np.array(mc, dtype=np.uint64), unparsed, first)


class Wanted:
    """The one-account host result per distinct key over one batch, computed once per key."""
    def __init__(self, strings):
        self.strings = strings; self.batch = records.RecordBatch.from_strings(strings); self.by_key = {}

    def of(self, who):
        if who not in self.by_key: self.by_key[who] = assembled(self.strings, who)
        return self.by_key[who]


def check_many(wanted, whos, host=False):
    got = records.decrypt_strings_many(wanted.batch, [key_bytes(w)[0] for w in whos], [key_bytes(w)[1] for w in whos], host=host)
    assert len(got) == len(whos)
    for j, w in enumerate(whos):
        want = wanted.of(w)
        assert same_found(got[j], want), ('key %d' % j, w, differences(got[j], want))
    return got


# ---- the host half ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed():
    """The case list's strings, the records of the other accounts, foreign and unparsable strings, shuffled."""
    cases, strings, _, _ = shuffled_cases()
    out = list(strings) + [s for who in (0, 1, 2, ('filler', 0)) for s in pool_of(who)[2]] + foreign_strings()[:20] + ['record1qqqq', 'x']
    random.Random(31).shuffle(out)
    return out


def test_host_path_equals_the_single_host_call_for_every_key():
    strings = mixed(); wanted = Wanted(strings)
    nobody = ('filler', 63)                                                                                         # owns nothing here
    whos = [MAIN, 0, 1, MAIN, 2, nobody, ('filler', 0)]
    got = check_many(wanted, whos, host=True)
    for w in whos: assert same_found(wanted.of(w), records.decrypt_strings(wanted.batch, *key_bytes(w), host=True)), w      # the yardstick of every test here is the call itself
    rows = Wanted(laid_out(300, whos, lambda i: i % 8))
    for w in whos: assert same_found(rows.of(w), records.decrypt_strings(rows.batch, *key_bytes(w), host=True)), w
    check_many(rows, whos, host=True)
    assert len(got[5]) == 0 and got[5].unparsed == got[0].unparsed >= 7 and len(got[6]) == 1 and same_found(got[0], got[3])
    for j, w in enumerate(whos[:5]):
        _, _, mine, statuses = pool_of(w)
        assert got[j].status.tolist() == [statuses[mine.index(strings[i])] for i in got[j].index.tolist()], w
        assert sorted(strings[i] for i in got[j].index.tolist()) == sorted(mine), w                                 # nobody else's records, and all of its own
    assert {0, 2, 4} <= set(got[1].status.tolist()) and int(got[1].microcredits.max()) == 7000
    # K = 1 and K = 64 (the repeated key 59 more times), nothing at all, and every string alone
    check_many(wanted, [1], host=True)
    check_many(wanted, keys_for(5) + [MAIN] * 59, host=True)
    for K in (1, 3):
        empty = records.decrypt_strings_many([], [key_bytes(w)[0] for w in keys_for(K)], [key_bytes(w)[1] for w in keys_for(K)], host=True)
        routed = records.decrypt_strings_many([], [key_bytes(w)[0] for w in keys_for(K)], [key_bytes(w)[1] for w in keys_for(K)])
        assert len(empty) == K
        for e, r in zip(empty, routed): assert len(e) == 0 and e.offsets.tolist() == [0] and e.plain.shape == (0, 32) and (e.unparsed, e.first_unparsed) == (0, 0) and same_found(e, r)
    for s in strings:
        if len(s) < 5000: check_many(Wanted([s]), [MAIN, 0, 1], host=True)


def test_bad_arguments_are_refused_as_records_scan_strings_refuses_them():
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    GOOD = REF['records']['owner']
    text = (GOOD + 'garbage').encode(); tp = ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p)
    off = lambda *v: np.array(v, dtype=np.uint64)
    rows = lambda *v: np.frombuffer(b''.join(le32(x) for x in v), dtype=np.uint8)
    vk = rows(1, 3, 5); ax = rows(5, 6, 7); flags = np.zeros(2 * 65, dtype=np.uint8)
    many_vk = rows(*[1] * 65); many_ax = rows(*[5] * 65)
    def both(call_found, call_scan, K=3):
        """The same status and the same message from the new call and from records_scan_strings, and every out[j] null afterwards."""
        rc = call_scan(); msg = L.aleo_mi355x_last_error()
        out = (ctypes.c_void_p * 65)(*[1] * 65)
        assert call_found(out) == rc != 0 and L.aleo_mi355x_last_error() == msg, (msg, L.aleo_mi355x_last_error())
        assert all(out[j] is None for j in range(K)) and all(out[j] == 1 for j in range(K, 65))
        return msg
    for f, g in ((L.aleo_mi355x_records_decrypt_strings_many_host, L.aleo_mi355x_records_scan_strings_host), (L.aleo_mi355x_records_decrypt_strings_many, L.aleo_mi355x_records_scan_strings)):
        out = (ctypes.c_void_p * 3)()
        assert f(out, tp, p(off(0, len(GOOD), len(text))), 2, p(vk), p(ax), 3) == 0
        for j in range(3):
            h = ctypes.c_void_p(out[j])
            assert L.aleo_mi355x_found_count(h) == 0 and L.aleo_mi355x_found_unparsed(h) == 1 and L.aleo_mi355x_found_first_unparsed(h) == 1
            L.aleo_mi355x_found_free(h)
        o2 = p(off(0, 1, 2))
        assert b'offsets[0]' in both(lambda o: f(o, tp, p(off(1, len(GOOD), len(text))), 2, p(vk), p(ax), 3), lambda: g(p(flags), None, None, tp, p(off(1, len(GOOD), len(text))), 2, p(vk), p(ax), 3))
        assert b'decrease' in both(lambda o: f(o, tp, p(off(0, len(text), len(GOOD))), 2, p(vk), p(ax), 3), lambda: g(p(flags), None, None, tp, p(off(0, len(text), len(GOOD))), 2, p(vk), p(ax), 3))
        assert b'null' in both(lambda o: f(o, None, o2, 2, p(vk), p(ax), 3), lambda: g(p(flags), None, None, None, o2, 2, p(vk), p(ax), 3))
        assert b'null' in both(lambda o: f(o, tp, None, 2, p(vk), p(ax), 3), lambda: g(p(flags), None, None, tp, None, 2, p(vk), p(ax), 3))
        assert b'null' in both(lambda o: f(o, tp, o2, 2, None, p(ax), 3), lambda: g(p(flags), None, None, tp, o2, 2, None, p(ax), 3))
        assert b'null' in both(lambda o: f(o, tp, o2, 2, p(vk), None, 3), lambda: g(p(flags), None, None, tp, o2, 2, p(vk), None, 3))
        bad_vk = rows(1, 3, L_ORDER); bad_ax = rows(5, R, 7)
        assert b'key 2' in both(lambda o: f(o, tp, o2, 2, p(bad_vk), p(ax), 3), lambda: g(p(flags), None, None, tp, o2, 2, p(bad_vk), p(ax), 3))
        assert b'key 1' in both(lambda o: f(o, tp, o2, 2, p(vk), p(bad_ax), 3), lambda: g(p(flags), None, None, tp, o2, 2, p(vk), p(bad_ax), 3))
        assert b'1..64' in both(lambda o: f(o, tp, o2, 2, p(vk), p(ax), 0), lambda: g(p(flags), None, None, tp, o2, 2, p(vk), p(ax), 0), K=0)
        assert b'1..64' in both(lambda o: f(o, tp, o2, 2, p(many_vk), p(many_ax), 65), lambda: g(p(flags), None, None, tp, o2, 2, p(many_vk), p(many_ax), 65), K=65)
        assert f(None, tp, o2, 2, p(vk), p(ax), 3) != 0 and b'null result pointer' in L.aleo_mi355x_last_error()
        out = (ctypes.c_void_p * 3)()
        assert f(out, None, None, 0, p(vk), p(ax), 3) == 0
        for j in range(3):
            h = ctypes.c_void_p(out[j])
            assert h.value and L.aleo_mi355x_found_count(h) == 0 and L.aleo_mi355x_found_fields(h) == 0
            L.aleo_mi355x_found_free(h)


def check_python_mirrors():
    """balances and decrypt_owned_many equal balance and decrypt_owned account by account, what they raise included."""
    cases, _, _, _ = shuffled_cases()
    whos = [0, MAIN, 1, MAIN]
    accounts = [key_bytes(w) for w in whos]
    good = good_strings() + [s for w in (0, 1) for s, st in zip(pool_of(w)[2], pool_of(w)[3]) if st == 0]
    random.Random(3).shuffle(good)
    batch = records.RecordBatch.from_strings(good)
    want_b = [records.balance(batch, vk, ax) for vk, ax in accounts]; want_d = [records.decrypt_owned(batch, vk, ax) for vk, ax in accounts]
    assert [len(d) for d in want_d] == [5, len(want_d[1]), 5, len(want_d[1])] and len(want_d[1]) >= 25 and want_b[1][0] > 2 ** 64
    assert records.balances(batch, accounts) == want_b == records.balances(good, accounts) == records.balances([records.RecordCiphertext.from_string(s) for s in good], accounts)
    assert records.decrypt_owned_many(batch, accounts) == want_d == records.decrypt_owned_many(good, accounts)
    assert records.decrypt_owned_many([records.RecordCiphertext.from_string(s) for s in good], accounts) == want_d
    assert records.balances(batch, []) == [] and records.decrypt_owned_many(batch, []) == [] and records.balances([], accounts) == [(0, [])] * 4
    many = accounts * 17                                                                                            # 68 accounts: two calls
    assert records.balances(batch, many) == want_b * 17
    by = {w: s for w, s, _, _ in cases}
    for bad in ('garbage', by['an entry with visibility 3'], by['public owner, nonce off the curve, a private field'], pool_of(1)[2][5], pool_of(1)[2][6]):
        strings = good[:2] + [bad] + good[2:7]
        for one, several in ((records.decrypt_owned, records.decrypt_owned_many), (records.balance, records.balances)):
            try: loop = [one(strings, vk, ax) for vk, ax in accounts]
            except aleo_amd.AleoMi355xError as e: loop = e
            if isinstance(loop, Exception):
                with pytest.raises(aleo_amd.AleoMi355xError) as direct: several(strings, accounts)
                assert str(direct.value) == str(loop) and type(direct.value) is type(loop)
            else: assert several(strings, accounts) == loop and one is records.balance and bad != 'garbage'
    with pytest.raises(TypeError): records.decrypt_strings_many([records.RecordCiphertext.from_string(good[0])], [accounts[0][0]], [accounts[0][1]])
    with pytest.raises(ValueError): records.decrypt_strings_many(batch, [1, 3], [le32(5)])


def test_python_mirrors_on_the_host_path(on_host):
    check_python_mirrors()


def run_cpp_mirror(tmp_path, env):
    """tests/cpp/records_found_many_test.cpp: decrypt_strings_many and balances of include/aleo_mi355x.hpp on the reference's strings, for the reference's two
    accounts and the first of them once more."""
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']] * 25 + ['garbage']
    keys = [REF['view_keys']['owner'], REF['addresses']['owner'], REF['view_keys']['sdk'], REF['addresses']['sdk'], REF['view_keys']['owner'], REF['addresses']['owner']]
    r = bs.run_cpp_mirror(tmp_path, 'records_found_many_test', ['3'] + keys + strings, env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '1000000', 'ALEO_MI355X_MIN_DECRYPT': '1000000'})


def check_reference_record(host):
    strings = [REF['records']['sdk_foreign'], REF['records']['owner'], 'garbage']
    G = account_generator(); other = ps.view_key_scalar(REF['view_keys']['non_owner'])
    mine, none = records.decrypt_strings_many(strings, [REF['view_keys']['owner'], other], [REF['addresses']['owner'], le32(ps.ed_mul(G, other)[0])], host=host)
    assert mine.index.tolist() == [1] and mine.kind.tolist() == [1] and mine.status.tolist() == [0] and mine.offsets.tolist() == [0, 2] and (mine.unparsed, mine.first_unparsed) == (1, 2)
    assert mine.microcredits.tolist() == [1500000000000000]                                                          # record_plaintext.rs:126-129 of the reference
    pt = records.RecordCiphertext.from_string(strings[1]).plaintext(mine.fields(0), REF['addresses']['owner'])
    assert str(pt) == REF['plaintexts']['owner'] and pt.microcredits() == 1500000000000000
    assert len(none) == 0 and none.plain.shape == (0, 32) and none.offsets.tolist() == [0] and (none.unparsed, none.first_unparsed) == (1, 2)


def test_the_reference_s_record_on_the_host_path():
    check_reference_record(host=True)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------
def layouts(n, K):
    """(what, the strings) per way of laying ownership out across K keys."""
    whos = keys_for(K)
    out = [('record i is key i mod (K + 1)\'s, K: nobody\'s', laid_out(n, whos, lambda i: i % (K + 1))),
           ('the first lane of every block is the last key\'s, the rest nobody\'s', laid_out(n, whos, lambda i: K - 1 if i % 256 == 0 else None))]
    if n <= 257: out.append(('one key owns everything, the others nothing', laid_out(n, whos, lambda i: 0)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n,K', [(n, K) for n in (1, 63, 65, 257, 4099) for K in (1, 2, 3, 8, 9)] + [(257, 64)])
def test_kernel_equals_the_host_path_at_block_edges_and_key_counts(on_kernel, n, K):
    whos = keys_for(K); statuses, counts = set(), set()
    for what, strings in layouts(n, K):
        got = check_many(Wanted(strings), whos)
        for f in got: statuses |= set(f.status.tolist()); counts |= set(np.diff(f.offsets.astype(np.int64)).tolist())
        if what.startswith('the first lane'):
            for j, f in enumerate(got): assert f.index.tolist() == (list(range(0, n, 256)) if whos[j] == whos[K - 1] else []), (what, j)
        if what.startswith('one key'):
            greedy = whos[0]
            for j, f in enumerate(got): assert len(f) == (n if whos[j] == greedy else 0), (what, j)
        if what.startswith('record i') and n >= 63:
            assert all(len(f) for f in got)
            if K >= 4: assert same_found(got[0], got[3]) and len(got[0]) >= 2 * (n // (K + 1))                      # the repeated key: both results, the records of both slots
    if n >= 257: assert {0, 2, 4} <= statuses and {0, 1, 2, 8, 9, 17} <= counts, (statuses, counts)


@pytest.mark.gpu
@pytest.mark.parametrize('n,K', [(4099, 8), (257, 3), (257, 1)])
def test_kernel_bytes_do_not_depend_on_the_keys_one_lane_takes(on_kernel, n, K):
    """K = 3 under W = 4 and W = 8: a group padded with keys of no digits.  K = 1: the shape of the one-account call, one live key and W - 1 of no digits."""
    whos = keys_for(K); wanted = Wanted(laid_out(n, whos, lambda i: i % (K + 1)))
    for w in ('1', '2', '4', '8'):
        on_kernel.setenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', w)
        check_many(wanted, whos)


@pytest.mark.gpu
def test_kernel_chunks_continue_indices_and_offsets_per_key(on_kernel):
    """(4099, 3) in chunks of a fifth and a third of the text: the middle of the batch is nobody's, so one chunk holds no owned pair; key 2 owns records only near
    the start, so later chunks hold something for keys 0 and 1 and nothing for it.  Decrypt launches of 64 and 8 fields span the key boundaries."""
    whos = keys_for(3); rng = random.Random(9)
    slot = [None if 1500 <= i < 2600 else 2 if i < 700 and i % 9 == 0 else rng.randrange(2) if rng.random() < 0.12 else None for i in range(4099)]
    wanted = Wanted(laid_out(4099, whos, lambda i: slot[i]))
    want = [wanted.of(w) for w in whos]
    assert all(len(f) > 70 for f in want) and sum(int(f.offsets[-1]) for f in want) > 600 and int(want[2].index.max()) < 700 and int(want[0].index.max()) > 3000
    assert not any(((f.index >= 1500) & (f.index < 2600)).any() for f in want)
    check_many(wanted, whos)
    lens = np.diff(wanted.batch.offsets.astype(np.int64)); total = int(lens.sum())
    for chars, fields in ((total // 5, None), (total // 5, '64'), (None, '64'), (total // 3, '8')):
        if chars: on_kernel.setenv('ALEO_MI355X_SCAN_CHUNK_CHARS', str(chars))
        else: on_kernel.delenv('ALEO_MI355X_SCAN_CHUNK_CHARS', raising=False)
        if fields: on_kernel.setenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', fields)
        else: on_kernel.delenv('ALEO_MI355X_DECRYPT_CHUNK_FIELDS', raising=False)
        check_many(wanted, whos)
    # the chunk of the middle fifth holds no owned pair; the chunks behind the first fifth hold nothing of key 2
    cum = np.cumsum(lens); first, last = int(np.searchsorted(cum, 2 * (total // 5))), int(np.searchsorted(cum, 3 * (total // 5)))
    assert 1500 < first and last < 2600 and int(np.searchsorted(cum, total // 5)) > 700


@pytest.mark.gpu
def test_kernel_walks_from_global_memory_where_a_block_s_strings_exceed_its_lds(on_kernel):
    """One block whose span exceeds 64 KiB with owned pairs of two different keys in it, beside blocks that fit."""
    whos = keys_for(3); rng = random.Random(6)
    long_foreign = lambda k: encode(payload_of(True, rng.randrange(R), rng.randrange(R), [(b'data', bytes(rng.randrange(256) for _ in range(k)))]))
    head = laid_out(256, whos, lambda i: 0 if i % 9 == 0 else 1 if i % 9 == 4 else None)
    strings = [s if i % 9 in (0, 4) else long_foreign(300) for i, s in enumerate(head)] + laid_out(300, whos, lambda i: i % 20, seed=1)
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])])
    spans = [int(off[min(b + 256, len(strings))] - (off[b] & ~15)) for b in range(0, len(strings), 256)]
    assert spans[0] > 65536 and spans[1] < 65536 and spans[2] < 65536, spans
    got = check_many(Wanted(strings), whos)
    for f in got[:2]: assert (f.index < 256).sum() >= 25 and (f.index >= 256).sum() >= 10
    assert (got[2].index < 256).sum() == 0 and len(got[2]) >= 10


@pytest.mark.gpu
def test_kernel_reference_record_and_mirrors(on_kernel, tmp_path):
    check_reference_record(host=False)
    check_python_mirrors()
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_RECORDS': '0', 'ALEO_MI355X_MIN_DECRYPT': '0'})
