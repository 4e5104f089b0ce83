"""The ownership scan for several accounts in one call (aleo_mi355x_records_scan_many / _many_host; aleo_amd.records.scan_many, find_owned_many;
csrc/records_many.hip, records_many_lane.h).  The contract is one sentence — row j of the result is byte for byte what the single-key host path
(aleo_mi355x_records_scan_host, itself pinned to the reference's vectors and to the rule written with the oracle by tests/test_records.py) returns for key j
alone — so every check below is an equality of bytes: against the host path, against K single scans of the kernel, and on a sample against the Python rule.
The first half needs no GPU (host path, refusals, reference vectors, the lane emulated on the host, the code object, routing); the second half runs the kernels
at every width: ALEO_MI355X_SCAN_KEYS_PER_LANE forces the keys one lane takes, unset leaves it to the library's rule."""
import ctypes, json, os, random, re, subprocess, sys, tempfile
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps
import batch_support as bs
from batch_support import ROOT, HIPCC, CSRC, le32
from test_records import REF, R, L_ORDER, rows, randomizer, account_generator, reference_cases, synthetic_records, big_batch, oracle_rule

WIDTHS = (1, 2, 4, 8)
REF_JSON = os.path.join(ROOT, 'tests', 'golden', 'reference_records.json')


def same(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def singles(C0, NX, keys, addrs, host):
    """(flags [K, n], rvk [K, n, 32]) from K single-key scans"""
    out = [records.scan(C0, NX, vk, ax, host=host) for vk, ax in zip(keys, addrs)]
    return np.stack([f for f, _ in out]), np.stack([r for _, r in out])


def reference_accounts(G):
    """The four view keys the reference's tests hold, each with the address reference_cases derives for it, and all of its record strings."""
    names = list(REF['view_keys'])
    addr = {}
    for case, rec, vk, a in reference_cases(G): addr.setdefault(case['view_key'], a)
    assert sorted(addr) == sorted(names) and len(names) == 4
    return names, [REF['view_keys'][k] for k in names], [addr[k] for k in names], list(REF['records'])


def encrypt_to(c0s, nxs, at, vk, G):
    """make record `at` one that the account of view key vk owns (its nonce stays)"""
    N = ps.ed_from_x(nxs[at])
    c0s[at] = (ps.ed_mul(G, vk)[0] + randomizer(ps.ed_mul(N, vk)[0])) % R


# ---- 1: the host path -----------------------------------------------------------------------------------------------------------------------------
def test_host_path_of_five_keys_equals_five_single_host_scans():
    G = account_generator(); rng = random.Random(31)
    odd, even = rng.randrange(1, L_ORDER) | 1, rng.randrange(2, L_ORDER) & ~1
    c0s, nxs, ax_odd, edge = synthetic_records(40, 79, odd, 1001, G)
    assert len(c0s) >= 128
    keys = [odd, even, 0, 1, odd]                                                            # view key 0 means k = l, view key 1 has one digit, one key twice
    addrs = [ax_odd, ps.ed_mul(G, even)[0], 0, G[0], ax_odd]
    for at, j in ((41, 1), (42, 2), (43, 3)): encrypt_to(c0s, nxs, at, keys[j], G)          # three of the foreign records now belong to the other keys
    C0, NX = rows(c0s), rows(nxs)
    got = records.scan_many(C0, NX, keys, addrs, host=True); want = singles(C0, NX, keys, addrs, host=True)
    assert got[0].shape == (5, len(c0s)) and got[1].shape == (5, len(c0s), 32) and same(got, want)
    assert (got[0][0, :40] == 1).all() and got[0][1, 41] == 1 and got[0][2, 42] == 1 and got[0][3, 43] == 1 and same((got[0][4], got[1][4]), (got[0][0], got[1][0]))
    assert (got[0][:, 41:44] == 1).sum() == 3 and (got[0] == 2).any() and not got[1][got[0] == 2].any()
    only_flags, none = records.scan_many(C0, NX, keys, addrs, want_rvk=False, host=True)     # rvk_out = NULL
    assert none is None and only_flags.tobytes() == got[0].tobytes()
    L = aleo_amd.lib(); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    z = np.zeros((1, 32), dtype=np.uint8); f = np.zeros(65, dtype=np.uint8); VK, AX = rows(keys), rows(addrs)
    for fn in (L.aleo_mi355x_records_scan_many_host, L.aleo_mi355x_records_scan_many):
        assert fn(None, None, None, None, 0, p(VK), p(AX), 5) == 0                           # n = 0 needs no buffers
        assert fn(p(f), None, p(z), p(z), 1, p(VK), p(AX), 0) != 0 and b'n_keys' in L.aleo_mi355x_last_error()
        assert fn(p(f), None, p(z), p(z), 1, p(rows([1] * 65)), p(rows([0] * 65)), 65) != 0 and b'n_keys' in L.aleo_mi355x_last_error()
        bad_vk = rows(keys[:3] + [L_ORDER] + keys[4:]); bad_ax = rows(addrs[:3] + [R] + addrs[4:])
        assert fn(p(f), None, p(z), p(z), 1, p(bad_vk), p(AX), 5) != 0
        err = L.aleo_mi355x_last_error().decode(); assert 'view key' in err and re.search(r'\bkey 3\b', err), err
        assert fn(p(f), None, p(z), p(z), 1, p(VK), p(bad_ax), 5) != 0
        err = L.aleo_mi355x_last_error().decode(); assert 'address' in err and re.search(r'\bkey 3\b', err), err


# ---- 2: the reference's vectors ---------------------------------------------------------------------------------------------------------------------
def check_reference_assertions(host):
    G = account_generator()
    names, vks, addrs, recs = reference_accounts(G)
    parsed = [records.RecordCiphertext.from_string(REF['records'][r]) for r in recs]
    C0 = np.frombuffer(b''.join(r.owner for r in parsed), dtype=np.uint8).reshape(-1, 32); NX = np.frombuffer(b''.join(r.nonce for r in parsed), dtype=np.uint8).reshape(-1, 32)
    flags, rvk = records.scan_many(C0, NX, vks, addrs, host=host)
    assert len(REF['is_owner']) == 4 and set(flags.ravel().tolist()) <= {0, 1}
    for case in REF['is_owner']:
        assert bool(flags[names.index(case['view_key']), recs.index(case['record'])] == 1) == case['expected'], case
    return flags, rvk


def test_one_call_answers_every_is_owner_assertion_of_the_reference():
    flags, rvk = check_reference_assertions(host=True)
    assert flags.sum() >= 2


# ---- 3: the lane on the host ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_grouped_lane_emulated_on_the_host_matches_the_host_path(tmp_path):
    """tests/cpp/records_many_lane_emul.cpp: records_many_lane.h at W = 2, 4, 8 over the checked field of checked_f29.h, key by key against scan_one_host."""
    r = bs.run_lane_emul(tmp_path, 'records_many_lane_emul', flags=(), hipcc=True)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    pairs, owned, malformed = (int(re.search(r'(\d+) %s' % w, r.stdout).group(1)) for w in ('pairs', 'owned', 'malformed'))
    assert pairs >= 3 * 3 * 40 and owned and malformed


# ---- 4: the code object -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_grouped_kernels_are_gfx950_and_have_no_scratch_at_any_width():
    """The kernels of records_many.hip; the figures of W = 1, which is the one-account scan's kernel too, are asserted by tests/test_records.py as well."""
    import code_object as co
    asm, blocks = co.compile_unit('records_many')
    built = set()
    for m in (b for b in blocks if 'k_records_scan_many' in b):
        w = int(re.search(r'k_records_scan_manyILi(\d+)E', m).group(1))
        built.add(w)
        print('k_records_scan_many<%d>: vgpr_count %d, agpr_count %d, sgpr_count %d, group_segment_fixed_size (LDS) %d, private_segment_fixed_size %d'
              % (w, co.field(m, 'vgpr_count'), co.field(m, 'agpr_count'), co.field(m, 'sgpr_count'), co.field(m, 'group_segment_fixed_size'), co.field(m, 'private_segment_fixed_size')))
        assert co.field(m, 'private_segment_fixed_size') == 0 and co.field(m, 'vgpr_spill_count') == 0, w
        assert co.field(m, 'group_segment_fixed_size') == (0 if w == 1 else w * 9 * 256 * 4) <= 160 * 1024       # the parked x of W keys, 9 words a lane
    assert sorted(built) == list(WIDTHS)
    src = open(os.path.join(CSRC, 'records_many.hip')).read()
    for w in WIDTHS: assert 'launch_many<%d>' % w in src                                                     # every width the rule or the switch can ask for is built


# ---- 5: routing -------------------------------------------------------------------------------------------------------------------------------------
def test_small_calls_run_on_the_host_and_need_no_device():
    code = ('import json; from aleo_amd import records; R = json.load(open(%r)); '
            's = [R["records"]["owner"], R["records"]["sdk_foreign"], R["records"]["sdk"]]; acc = [(R["view_keys"][k], R["addresses"][k]) for k in ("sdk", "owner")]; '
            'print(json.dumps([i for i, _ in records.find_owned_many(s, acc)]))' % REF_JSON)
    base = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_RECORDS='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    base.pop('ALEO_MI355X_SCAN_KEYS_PER_LANE', None)
    for extra in ({}, {'ALEO_MI355X_SCAN_KEYS_PER_LANE': 'nonsense'}, {'ALEO_MI355X_SCAN_KEYS_PER_LANE': '4'}):
        r = subprocess.run([sys.executable, '-c', code], env=dict(base, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and json.loads(r.stdout) == [[0, 2], [0, 2]], r.stdout + r.stderr
    assert records.find_owned_many([], [(1, 0)]) == [([], [])] and records.find_owned_many([REF['records']['sdk']], []) == []


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0'); monkeypatch.delenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0
    return lambda w: monkeypatch.setenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', str(w)) if w else monkeypatch.delenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', raising=False)


@pytest.fixture(scope='module')
def nine_keys():
    """Nine different accounts: three that own records below, view key 1, view key 0, four more."""
    G = account_generator(); rng = random.Random(2024)
    keys = [rng.randrange(1, L_ORDER) | 1, rng.randrange(2, L_ORDER) & ~1, rng.randrange(1, L_ORDER), 1, 0] + [rng.randrange(1, L_ORDER) for _ in range(4)]
    return G, keys, [ps.ed_mul(G, k)[0] if k else 0 for k in keys]


@pytest.fixture(scope='module')
def small_set(nine_keys):
    """257 records of big_batch with its edge cases, a few of them encrypted to each of the first three keys; the host path's answer for all nine keys (2 313 pairs)."""
    G, keys, addrs = nine_keys
    c0s, nxs, _, owned, where = big_batch(257, keys[0], 77, G)
    free = [i for i in range(257) if i not in owned and i not in where]
    mine = {0: free[:1] + free[100:102], 1: free[1:2] + [i for i in free if i >= 63][:2], 2: [i for i in free if i >= 250][-3:]}
    for j, at in mine.items():
        for i in at: encrypt_to(c0s, nxs, i, keys[j], G)
    mine[0] = sorted(mine[0] + owned)
    C0, NX = rows(c0s), rows(nxs)
    hf, hr = records.scan_many(C0, NX, keys, addrs, host=True)
    for j in range(3): assert sorted(np.nonzero(hf[j] == 1)[0].tolist()) == sorted(mine[j] + ([i for i, name in where.items() if 'owner' in name or name.endswith(', owned')] if j == 0 else [])), j
    assert (hf[:, sorted(sum(mine.values(), []))] == 1).sum(axis=0).tolist() == [1] * sum(len(v) for v in mine.values())      # a record owned by key j is owned by no other key
    bad = hf[0] == 2
    assert bad.sum() == 5 and (hf[:, bad] == 2).all() and (hf[:, ~bad] != 2).all() and not hr[:, bad].any()                   # flag 2 is the record's: every key reports it, with zero rvk
    return C0, NX, hf, hr


@pytest.mark.gpu
@pytest.mark.parametrize('width', WIDTHS)
def test_every_width_equals_the_host_path_at_wave_and_block_edges(on_kernel, nine_keys, small_set, width):
    G, keys, addrs = nine_keys; C0, NX, hf, hr = small_set
    on_kernel(width)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for k in (1, 2, 3, 5, 8, 9):                                                          # a partial last group at every width
            f, r = records.scan_many(C0[:n], NX[:n], keys[:k], addrs[:k])
            assert f.tobytes() == hf[:k, :n].tobytes() and r.tobytes() == hr[:k, :n].tobytes(), (width, n, k)
    f, none = records.scan_many(C0, NX, keys, addrs, want_rvk=False)
    assert none is None and f.tobytes() == hf.tobytes()
    f, r = records.scan_many(C0, NX, [keys[0], keys[3], keys[0], keys[4]], [addrs[0], addrs[3], addrs[0], addrs[4]])      # a repeated key beside view keys 1 and 0
    assert f.tobytes() == hf[[0, 3, 0, 4]].tobytes() and r.tobytes() == hr[[0, 3, 0, 4]].tobytes()


@pytest.fixture(scope='module')
def base_4096(nine_keys):
    """4 096 synthetic records (about 1 % encrypted to key 0, the edge cases among them), three more encrypted to each of keys 1 and 2: what the large shapes tile."""
    G, keys, addrs = nine_keys
    c0s, nxs, _, owned, where = big_batch(4096, keys[0], 4243, G)
    free = [i for i in range(4096) if i not in owned and i not in where]
    for j in (1, 2):
        for i in free[40 * j:40 * j + 3]: encrypt_to(c0s, nxs, i, keys[j], G)
    return c0s, nxs, sorted(owned + list(where) + free[40:43] + free[80:83])                  # ... and which of them are not plain foreign records


def tiled(base, n, seed):
    c0s, nxs = base[:2]
    idx = np.random.RandomState(seed).randint(0, len(c0s), size=n)
    return rows(c0s)[idx], rows(nxs)[idx], idx


@pytest.mark.gpu
def test_the_rule_and_the_wider_groups_at_a_chip_filling_size(on_kernel, nine_keys, base_4096):
    """n = 2^14 + 3, K = 8: the rule takes two keys per lane (4 x 16 387 >= 65 536 > 2 x 16 387); then four and eight forced."""
    G, keys, addrs = nine_keys
    n = (1 << 14) + 3
    C0, NX, idx = tiled(base_4096, n, 7)
    want = singles(C0, NX, keys[:8], addrs[:8], host=False)                                    # the single-key kernel, pinned to the host path by tests/test_records.py
    special = np.nonzero(np.isin(idx, base_4096[2]))[0][:96]                                   # owned records and edge cases first, then any
    sample = np.concatenate([special, np.setdiff1d(np.random.RandomState(8).choice(n, 256, replace=False), special)[:256 - len(special)]])      # 256 records: 2 048 pairs
    assert len(sample) == 256 and len(special) > 32
    hf, hr = records.scan_many(C0[sample], NX[sample], keys[:8], addrs[:8], host=True)
    assert same((want[0][:, sample], want[1][:, sample]), (hf, hr)) and (hf == 1).any() and (hf == 2).any()
    for width in (0, 4, 8, 'nonsense'):
        on_kernel(width)
        got = records.scan_many(C0, NX, keys[:8], addrs[:8])
        assert same(got, want), width
    rng = random.Random(9); c0s, nxs = base_4096[:2]
    for _ in range(32):
        j, s = rng.randrange(8), int(sample[rng.randrange(256)])
        i = int(idx[s])
        assert (int(got[0][j, s]), int.from_bytes(got[1][j, s].tobytes(), 'little')) == oracle_rule(c0s[i], nxs[i], keys[j], addrs[j]), (j, s)


@pytest.mark.gpu
def test_a_call_of_more_than_one_chunk_equals_nine_single_scans(on_kernel, nine_keys, base_4096):
    """n = 2^19 + 5, K = 9: more than 2^22 pairs, so the records go through in at least two chunks and every row is stitched from them."""
    G, keys, addrs = nine_keys
    n = (1 << 19) + 5
    assert n * 9 > 1 << 22
    C0, NX, _ = tiled(base_4096, n, 11)
    flags, rvk = records.scan_many(C0, NX, keys, addrs)
    for j in range(9):
        f, r = records.scan(C0, NX, keys[j], addrs[j])
        assert f.tobytes() == flags[j].tobytes() and r.tobytes() == rvk[j].tobytes(), j
    assert (flags[0] == 1).sum() > 1000 and (flags[1] == 1).any() and (flags[2] == 1).any() and not (flags[3:] == 1).any()


@pytest.mark.gpu
def test_nothing_stale_and_nothing_shared(on_kernel, nine_keys, small_set, base_4096):
    G, keys, addrs = nine_keys; C0, NX, hf, hr = small_set
    on_kernel(4)
    B0, BX, _ = tiled(base_4096, 300, 13)
    sets = [(C0, NX, keys[:5], addrs[:5]), (B0, BX, keys[2:9], addrs[2:9])]
    alone = [records.scan_many(*s) for s in sets]
    assert same(alone[0], (hf[:5], hr[:5])) and same(alone[1], records.scan_many(*sets[1], host=True))
    got = bs.two_threads(lambda i: records.scan_many(*sets[i]))
    for i in range(2): assert same(got[i], alone[i]), i
    # the grouped scan and the plain one in turn on one slot: neither leaves the other a stale table, state or result
    for _ in range(2):
        assert same(records.scan_many(C0, NX, keys[:5], addrs[:5]), (hf[:5], hr[:5]))
        assert same(records.scan(C0, NX, keys[6], addrs[6]), (hf[6], hr[6]))
    assert same(records.scan_many(C0, NX, keys[5:], addrs[5:]), (hf[5:], hr[5:]))


@pytest.mark.gpu
def test_mirrors_on_the_reference_strings(on_kernel, tmp_path):
    G = account_generator()
    flags, _ = check_reference_assertions(host=False)                                          # the reference's four assertions from one call of the kernel
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']]
    accounts = [(REF['view_keys'][k], REF['addresses'][k]) for k in ('sdk', 'owner')]
    got = records.find_owned_many(strings, accounts)
    assert got == [records.find_owned(strings, vk, a) for vk, a in accounts] and got[0][0] == [0, 2]
    foreign = REF['view_keys']['sdk_foreign']
    assert records.find_owned_many(strings[2:], [(foreign, le32(ps.ed_mul(G, ps.view_key_scalar(foreign))[0])), accounts[0]]) == [([], []), records.find_owned(strings[2:], *accounts[0])]
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, 'records_scan_many_test')
    args = []                                                      # record, view key, address, expected — the reference's four assertions
    for case, rec, vk, addr in reference_cases(G):
        args += [str(rec), vk, addr if isinstance(addr, str) else wire.bech32m_encode('aleo', addr), '1' if case['expected'] else '0']
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=dict(os.environ, ALEO_MI355X_MIN_RECORDS='0'))
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr
