"""Accounts in batches and the search for an address with a chosen prefix (aleo_mi355x_accounts_derive[_host], _accounts_search[_host], _min_accounts,
_private_key_from_seed, _private_key_seed, _seed_from_bytes, _view_key_to_string; aleo_amd/account.py; the same in include/aleo_mi355x.hpp).

What the reference's data pins comes first: its three accounts and its one seed with the private key string made from it.  Then the product against the
restatement in Python integers (tests/serial_ref.py, pinned stage by stage), at the edges of the seed and of the view key's reduction; the search against a
restatement built here from oracle.varuna_ref.random_fr, that derivation and a bech32 symbol split; the strings; the threshold; the code object.  The host path,
byte for byte, checks the device lane: emulated on the CPU, plain and under the sanitizers, here, and on the GPU in the second half (ALEO_MI355X_MIN_ACCOUNTS=0).
No test reads the reference tree."""
import ctypes, functools, json, os, random, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import account as acct, records, wire
from oracle import poseidon as ps
from oracle import varuna_ref as V
import serial_ref as S
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32, num, _p, _vp

ACC = json.load(open(os.path.join(HERE, 'golden', 'reference_account.json')))['accounts']
SEED = json.load(open(os.path.join(HERE, 'golden', 'reference_seed.json')))
R, L = ps.R, ps.ED_SUBGROUP_ORDER
CHARSET = 'qpzry9x8gf2tvdw0s3jn54khce6mua7l'
MASTER = bytes((7 * i + 3) & 0xff for i in range(32))
FAR = (1 << 32) - 100                                                                # a range that crosses 2^32
RANGES = {0: 256, FAR: 200}                                                          # first -> count


# ---- through the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def derive_raw(seeds, host=True, want=('sk', 'vk', 'ax', 'str', 'flags')):
    """aleo_mi355x_accounts_derive[_host] on raw seeds: (status, {name: bytes}); the outputs not in `want` are passed as NULL."""
    n = len(seeds)
    out = {'sk': np.full((n, 32), 9, np.uint8), 'vk': np.full((n, 32), 9, np.uint8), 'ax': np.full((n, 32), 9, np.uint8), 'str': np.full((n, 63), 9, np.uint8), 'flags': np.full(n, 9, np.uint8)}
    L_ = aleo_amd.lib(); call = L_.aleo_mi355x_accounts_derive_host if host else L_.aleo_mi355x_accounts_derive
    rc = call(_vp(b''.join(seeds)), n, *[_p(out[k]) if k in want else None for k in ('sk', 'vk', 'ax', 'str', 'flags')])
    return rc, {k: out[k].tobytes() for k in want}


def search_raw(first, count, prefix, max_hits, host=True, master=MASTER):
    """aleo_mi355x_accounts_search[_host]: (status, indices, seeds, next)."""
    idx = np.zeros(max(max_hits, 1), np.uint64); seeds = np.zeros((max(max_hits, 1), 32), np.uint8)
    n = ctypes.c_size_t(12345); nxt = ctypes.c_uint64(12345)
    L_ = aleo_amd.lib(); call = L_.aleo_mi355x_accounts_search_host if host else L_.aleo_mi355x_accounts_search
    rc = call(_vp(master), first, count, prefix.encode() if prefix is not None else None, max_hits, _p(idx), _p(seeds), ctypes.byref(n), ctypes.byref(nxt))
    if rc: return rc, None, None, None
    return rc, [int(i) for i in idx[:n.value]], [seeds[j].tobytes() for j in range(n.value)], int(nxt.value)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------
def py_account(seed: int):
    """(sk_sig, view key, address x) by tests/serial_ref.account_from_private_key, which is pinned by the reference's accounts."""
    sk, view, address = S.account_from_private_key(ps.private_key_string(seed))
    return sk, view, address[0]


@functools.lru_cache(maxsize=None)
def g_powers():
    pts = [S.account_generator()]
    for _ in range(251): pts.append(S.ed_add(pts[-1], pts[-1]))
    return pts


def mul_g(k: int):
    """k G from the doublings of G: the same point S.ed_mul gives, at a tenth of the time (the search's restatement derives hundreds of accounts)."""
    acc, i = (0, 1), 0
    while k:
        if k & 1: acc = S.ed_add(acc, g_powers()[i])
        k >>= 1; i += 1
    return acc


@functools.lru_cache(maxsize=None)
def py_parts(seed: int):
    """(sk_sig, r_sig, sk_prf, view key, address x): serial_ref's six lines with the fixed-base multiplication above; test 2 checks it against serial_ref itself."""
    sk = ps.hash_to_scalar(2, [ps.domain_separator('AleoAccountSignatureSecretKey0'), seed])
    rs = ps.hash_to_scalar(2, [ps.domain_separator('AleoAccountSignatureRandomizer0.0'), seed])
    prf = ps.hash_to_scalar(4, [mul_g(sk)[0], mul_g(rs)[0]])
    view = (sk + rs + prf) % L
    return sk, rs, prf, view, mul_g(view)[0]


def symbols(x32: bytes):
    """The 52 symbols of an address: its 32 bytes as a bit stream, the most significant bit of each byte first, five bits at a time, the last one padded."""
    bits = ''.join('{:08b}'.format(b) for b in x32) + '0000'
    return [int(bits[i:i + 5], 2) for i in range(0, 260, 5)]


def py_search(first, count, prefix, max_hits):
    """(indices, next) of the result's definition, from the restatement alone."""
    hits = []
    for i in range(first, first + count):
        if len(hits) == max_hits: break
        ax = le32(py_parts(V.random_fr(MASTER, i))[4])
        if ''.join(CHARSET[s] for s in symbols(ax))[:len(prefix)] == prefix: hits.append(i)
    return hits, (hits[-1] + 1 if max_hits and len(hits) == max_hits else (first + count if max_hits else first))


@functools.lru_cache(maxsize=None)
def two_character_prefix(first):
    """The first two characters after "aleo1" of candidate first + 50: a prefix with at least one hit in the range."""
    return wire.bech32m_encode('aleo', le32(py_parts(V.random_fr(MASTER, first + 50))[4]))[5:7]


def prefixes(first): return ['', 'q', two_character_prefix(first)]


# ---- the seeds ------------------------------------------------------------------------------------------------------------------------------------------------
GENERATOR_SEED = 1                                             # chosen on the CPU: its 64 seeds hold view-key sums with 0, 1 and 2 subtractions of l (the companion test)


@functools.lru_cache(maxsize=None)
def edge_seeds():
    """[(seed bytes, canonical)]: 64 from a fixed generator, 0, 1, r - 1, and r, r + 1, 2^256 - 1, which are no field elements: at most one wave of them."""
    rng = random.Random(GENERATOR_SEED)
    out = [(le32(rng.randrange(R)), True) for _ in range(64)] + [(le32(v), True) for v in (0, 1, R - 1)] + [(le32(v), False) for v in (R, R + 1, (1 << 256) - 1)]
    assert len(out) <= 64 + 6
    return out


def mixed_seeds(n, seed=7):
    """n seeds, every seventh no field element."""
    rng = random.Random(seed * 1000 + n)
    return [le32(rng.randrange(R, 1 << 256)) if i % 7 == 3 else le32(rng.randrange(R)) for i in range(n)]


# ---- 1: what the reference's data pins -------------------------------------------------------------------------------------------------------------------------
def test_the_three_reference_accounts_from_their_private_keys():
    seeds = [acct.private_key_seed(a['private_key']) for a in ACC]
    rc, out = derive_raw(seeds)
    assert rc == 0 and out['flags'] == bytes(3)
    for i, a in enumerate(ACC):
        assert acct.view_key_string(out['vk'][32 * i:32 * i + 32]) == a['view_key'] == ps.view_key_string(num(out['vk'][32 * i:32 * i + 32]))
        assert wire.bech32m_encode('aleo', out['ax'][32 * i:32 * i + 32]) == a['address']
        assert out['str'][63 * i:63 * i + 63].decode() == a['address']
        old = records.Account.from_private_key(a['private_key'])                   # the one-key call keeps its bytes
        assert (old.sk_sig, old.view_key, old.address_x) == (out['sk'][32 * i:32 * i + 32], out['vk'][32 * i:32 * i + 32], out['ax'][32 * i:32 * i + 32])
    got = acct.accounts_from_private_keys([a['private_key'] for a in ACC], host=True)
    assert [(g.private_key, g.view_key_string, g.address) for g in got] == [(a['private_key'], a['view_key'], a['address']) for a in ACC]


def test_the_reference_seed_gives_the_reference_private_key():
    seed = bytes(SEED['seed'])
    assert len(seed) == 32 and num(seed) < R
    assert acct.private_key_from_seed(seed) == SEED['private_key'] == ACC[2]['private_key']
    assert acct.private_key_seed(SEED['private_key']) == seed
    a = records.Account.from_seed(seed)                                              # new Account({seed}) of the reference's SDK
    assert (a.private_key, a.view_key_string, a.address) == (ACC[2]['private_key'], ACC[2]['view_key'], ACC[2]['address'])


# ---- 2: against the restatement ------------------------------------------------------------------------------------------------------------------------------------
def test_derive_host_equals_the_restatement_at_the_edges():
    seeds = edge_seeds()
    rc, out = derive_raw([s for s, _ in seeds])
    assert rc == 0
    for i, (s, canonical) in enumerate(seeds):
        rows = (out['sk'][32 * i:32 * i + 32], out['vk'][32 * i:32 * i + 32], out['ax'][32 * i:32 * i + 32])
        if not canonical:
            assert out['flags'][i] == 3 and rows == (bytes(32),) * 3 and out['str'][63 * i:63 * i + 63] == bytes(63), i
            continue
        sk, view, ax = py_account(num(s))
        assert out['flags'][i] == 0 and rows == (le32(sk), le32(view), le32(ax)), i
        assert py_parts(num(s))[0::3] == (sk, view) and py_parts(num(s))[4] == ax       # the faster restatement is the pinned one
        assert out['str'][63 * i:63 * i + 63].decode() == wire.bech32m_encode('aleo', le32(ax))
    sk, vk, ax, flags, text = acct.derive_many([s for s, _ in seeds], strings=True, host=True)
    assert (sk.tobytes(), vk.tobytes(), ax.tobytes(), flags.tobytes()) == (out['sk'], out['vk'], out['ax'], out['flags'])
    assert text == [out['str'][63 * i:63 * i + 63].decode() if c else '' for i, (_, c) in enumerate(seeds)]
    with pytest.raises(ValueError): acct.accounts_from_seeds([s for s, _ in seeds], host=True)


def test_the_chosen_seeds_hold_every_number_of_subtractions_of_the_group_order():
    """sk_sig + r_sig + sk_prf is below 3 l: the view key takes no, one or two subtractions (about 0.26, 0.69 and 0.05 of uniform hashes)."""
    taken = [sum(py_parts(num(s))[:3]) // L for s, canonical in edge_seeds() if canonical]
    assert set(taken) == {0, 1, 2}, {k: taken.count(k) for k in set(taken)}


# ---- 3: the device lane on the CPU -----------------------------------------------------------------------------------------------------------------------------
def lane_rows():
    """Every case of tests 1 and 2 and every candidate of test 4, with the bytes the library's host path gives them."""
    seeds = [acct.private_key_seed(a['private_key']) for a in ACC] + [s for s, _ in edge_seeds()]
    rows = [(0, b'', s) for s in seeds]
    for first, count in RANGES.items():
        rows += [(1, MASTER + struct.pack('<Q', i), le32(V.random_fr(MASTER, i))) for i in range(first, first + count)]
    rc, out = derive_raw([r[2] for r in rows])
    assert rc == 0
    return [(kind, head, s, out['flags'][i:i + 1] + out['sk'][32 * i:32 * i + 32] + out['vk'][32 * i:32 * i + 32] + out['ax'][32 * i:32 * i + 32] + out['str'][63 * i:63 * i + 63])
            for i, (kind, head, s) in enumerate(rows)]


@pytest.mark.parametrize('sanitized', [False, True], ids=['plain', 'sanitizers'])
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path, sanitized):
    """tests/cpp/account_lane_emul.cpp: account_lane.h compiled for the CPU over the checked restatement of fr29.h, once plain and once with the address and
    undefined-behaviour sanitizers compiled into that program, run as a program of its own.  (-fno-strict-aliasing: as for signature_lane_emul.)"""
    data = os.path.join(str(tmp_path), 'cases.bin')
    rows = lane_rows()
    with open(data, 'wb') as f:
        f.write(struct.pack('<I', len(rows)))
        for kind, head, s, want in rows: f.write(bytes([kind]) + head + s + want)
    r = bs.run_lane_emul(tmp_path, 'account_lane_emul', [data], sanitized=sanitized)
    print(r.stdout)
    assert r.returncode == 0 and '%d accounts' % len(rows) in r.stdout and '%d of them candidates' % sum(RANGES.values()) in r.stdout, r.stdout + r.stderr
    assert ' 0 mismatches, 0 reads past an end, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr


# ---- 4: the search on the host path --------------------------------------------------------------------------------------------------------------------------------
def search_cases(first):
    """[(prefix, max_hits)]: each prefix with max_hits of 1, of exactly its number of hits in the range, and of more."""
    out = []
    for prefix in prefixes(first):
        hits = py_search(first, RANGES[first], prefix, 1 << 30)[0]
        assert len(hits) >= (2 if len(prefix) < 2 else 1), (prefix, hits)
        out += [(prefix, 1), (prefix, len(hits)), (prefix, len(hits) + 5)]
    return out


@pytest.mark.parametrize('first', list(RANGES), ids=['from 0', 'across 2^32'])
def test_search_host_equals_the_restatement(first):
    count = RANGES[first]
    for prefix, max_hits in search_cases(first):
        rc, idx, seeds, nxt = search_raw(first, count, prefix, max_hits)
        want, want_next = py_search(first, count, prefix, max_hits)
        assert rc == 0 and (idx, nxt) == (want, want_next), (prefix, max_hits)
        assert seeds == [le32(V.random_fr(MASTER, i)) for i in want]
        assert want_next == (want[-1] + 1 if len(want) == max_hits else first + count)
    # resuming from `next` sees every candidate once
    prefix = 'q'; seen, at = [], first
    while at < first + count:
        rc, idx, _, at2 = search_raw(at, first + count - at, prefix, 1)
        assert rc == 0 and at2 > at
        seen += idx; at = at2
    assert seen == py_search(first, count, prefix, 1 << 30)[0]
    assert search_raw(first, count, 'q', 0)[1:] == ([], [], first) and search_raw(first, 0, 'q', 3)[1:] == ([], [], first)


def test_search_returns_accounts_with_their_private_keys():
    hits, nxt = acct.search(MASTER, 'q', 0, RANGES[0], max_hits=2, host=True)
    want, want_next = py_search(0, RANGES[0], 'q', 2)
    assert [h.index for h in hits] == want and nxt == want_next
    for h in hits:
        assert h.address.startswith('aleo1q') and records.Account.from_private_key(h.private_key).address == h.address
        assert acct.private_key_seed(h.private_key) == le32(V.random_fr(MASTER, h.index))


def test_search_refuses_what_is_no_prefix():
    lib = aleo_amd.lib()
    for bad in ('b', 'i', 'o', '1', 'qb', 'Q', 'q' * 13, None):
        assert search_raw(0, 8, bad, 1)[0] == 2, bad
        assert search_raw(0, 8, bad, 1, host=False)[0] == 2, bad
        assert b'accounts_search' in lib.aleo_mi355x_last_error()
    assert search_raw(0, 8, 'q' * 12, 1)[0] == 0 and search_raw((1 << 64) - 4, 8, '', 1)[0] == 2
    with pytest.raises(aleo_amd.AleoMi355xError): acct.search(MASTER, 'b', 0, 8, host=True)
    with pytest.raises(ValueError): acct.search(MASTER[:31], 'q', 0, 8, host=True)


# ---- 5: strings ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_key_strings_round_trip_and_refuse_what_is_no_key():
    rng = random.Random(11)
    for v in [0, 1, R - 1] + [rng.randrange(R) for _ in range(8)]:
        key = acct.private_key_from_seed(le32(v))
        assert key == ps.private_key_string(v) and key.startswith('APrivateKey1') and acct.private_key_seed(key) == le32(v)
        assert acct.view_key_string(le32(v % L)) == ps.view_key_string(v % L)
    for v in (R, R + 1, (1 << 256) - 1):
        with pytest.raises(aleo_amd.AleoMi355xError): acct.private_key_from_seed(le32(v))
        with pytest.raises(aleo_amd.AleoMi355xError): acct.private_key_seed(ps.base58_encode(ps.PRIVATE_KEY_PREFIX + le32(v)))      # a key string whose seed is no field element
    for bad in ('', 'APrivateKey1nonsense', ACC[0]['view_key'], ACC[0]['address'], ACC[0]['private_key'][:-1], ACC[0]['private_key'] + 'z', ACC[0]['private_key'].replace('z', '0', 1)):
        with pytest.raises(aleo_amd.AleoMi355xError): acct.private_key_seed(bad)
    out = ctypes.create_string_buffer(59)                       # one short of the 59 characters and their terminator
    assert aleo_amd.lib().aleo_mi355x_private_key_from_seed(out, len(out), _vp(le32(5))) == 2
    with pytest.raises(ValueError): acct.private_key_from_seed(bytes(31))


def test_seed_from_bytes_reduces_modulo_the_field_order():
    rng = random.Random(12)
    for v in [0, 1, R - 1, R, R + 1, 2 * R, 2 * R + 5, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(16)]:
        assert acct.seed_from_bytes(le32(v)) == le32(v % R), v
    raw = le32((1 << 256) - 7)
    assert records.Account.from_seed(raw).private_key == ps.private_key_string(((1 << 256) - 7) % R)


# ---- 6: the threshold, the code object, the C++ mirror -------------------------------------------------------------------------------------------------------------
DEFAULT_MIN_ACCOUNTS = 16


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_accounts', 'ALEO_MI355X_MIN_ACCOUNTS') == (DEFAULT_MIN_ACCOUNTS, 5, DEFAULT_MIN_ACCOUNTS)
    # below the threshold the calls compute on the host: no device is needed for them
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_ACCOUNTS='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    code = ('from aleo_amd import account as a; k = %r; print(a.accounts_from_private_keys([k, k])[1].address, a.search(bytes(32), "", 5, 9, max_hits=2)[1])' % ACC[0]['private_key'])
    assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300).stdout.split() == [ACC[0]['address'], '7']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_account_kernels_code_object_is_gfx950_and_has_no_scratch_and_no_spills():
    kernels = ('k_accounts_derive', 'k_accounts_search')
    assert bs.scratch_and_spills('accounts', kernels) == (2, {k: (0, 0, 0) for k in kernels})      # these two and no other


def run_cpp_mirror(tmp_path, env, n):
    """tests/cpp/accounts_test.cpp: derive_accounts, accounts_from_private_keys, account_from_seed, search_accounts and the strings of include/aleo_mi355x.hpp."""
    r = bs.run_cpp_mirror(tmp_path, 'accounts_test', [ACC[0]['private_key'], ACC[0]['address'], n], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_ACCOUNTS': '1000000'}, 12)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_ACCOUNTS', '0')
    monkeypatch.delenv('ALEO_MI355X_ACCOUNTS_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_accounts()) == 0
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_gpu_derive_equals_the_host_path_at_wave_and_block_edges(on_kernel, n):
    seeds = mixed_seeds(n)
    host = derive_raw(seeds, host=True)
    got = derive_raw(seeds, host=False)
    assert host[0] == 0 and got == host
    if n >= 63: assert set(host[1]['flags']) == {0, 3}
    if n == 65:                                                 # some outputs NULL: the others are the same bytes
        for want in (('vk', 'ax', 'flags'), ('str',), ('sk', 'flags'), ()):
            part = derive_raw(seeds, host=False, want=want)
            assert part == (0, {k: host[1][k] for k in want}) and derive_raw(seeds, host=True, want=want) == part


@pytest.mark.gpu
def test_gpu_one_wave_of_every_edge_seed_at_once(on_kernel):
    seeds = [s for s, _ in edge_seeds()][:64]
    rest = [s for s, _ in edge_seeds()][64:]
    assert derive_raw(seeds, host=False) == derive_raw(seeds, host=True)
    assert derive_raw(rest + seeds[:58], host=False) == derive_raw(rest + seeds[:58], host=True)      # the six edges and the refused seeds in one wave with 58 others


@pytest.mark.gpu
def test_gpu_both_sides_of_the_threshold_and_chunked_launches_return_the_same_bytes(monkeypatch):
    seeds = mixed_seeds(40)
    host = derive_raw(seeds, host=True)
    monkeypatch.setenv('ALEO_MI355X_MIN_ACCOUNTS', '41'); assert derive_raw(seeds, host=False) == host      # below: the host code inside the call
    monkeypatch.setenv('ALEO_MI355X_MIN_ACCOUNTS', '40'); assert derive_raw(seeds, host=False) == host      # at it: the kernel
    monkeypatch.setenv('ALEO_MI355X_ACCOUNTS_CHUNK', '7'); assert derive_raw(seeds, host=False) == host     # six launches
    sk, vk, ax, flags, text = acct.derive_many(seeds, strings=True)                                         # the Python mirror on the kernel
    assert (sk.tobytes(), vk.tobytes(), ax.tobytes(), flags.tobytes()) == tuple(host[1][k] for k in ('sk', 'vk', 'ax', 'flags'))
    assert ''.join(text).encode() == host[1]['str'].replace(b'\0', b'')
    good = [s for s in seeds if num(s) < R]
    assert [(a.sk_sig, a.view_key, a.address_x, a.private_key) for a in acct.accounts_from_seeds(good)] == [(a.sk_sig, a.view_key, a.address_x, a.private_key) for a in acct.accounts_from_seeds(good, host=True)]


@pytest.mark.gpu
@pytest.mark.parametrize('chunk', [None, '128'], ids=['one launch', 'launches of 128'])
@pytest.mark.parametrize('first', list(RANGES), ids=['from 0', 'across 2^32'])
def test_gpu_search_equals_the_host_search(on_kernel, first, chunk):
    if chunk: on_kernel.setenv('ALEO_MI355X_ACCOUNTS_CHUNK', chunk)
    count = 300                                                 # not a multiple of 64
    for prefix in prefixes(first):
        everything = search_raw(first, count, prefix, 1 << 20, host=True)
        assert everything[0] == 0 and len(everything[1]) >= 1
        for max_hits in (1, len(everything[1]), len(everything[1]) + 5):
            host = search_raw(first, count, prefix, max_hits, host=True)
            got = search_raw(first, count, prefix, max_hits, host=False)
            assert host[0] == 0 and got == host, (prefix, max_hits)
            assert host[3] == (host[1][-1] + 1 if len(host[1]) == max_hits else first + count)


@pytest.mark.gpu
def test_gpu_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    seeds = mixed_seeds(130, seed=8)
    want = [derive_raw(seeds, host=True), search_raw(FAR, 300, 'q', 4, host=True)]
    assert bs.two_threads(lambda i: derive_raw(seeds, host=False) if i == 0 else search_raw(FAR, 300, 'q', 4, host=False)) == want


@pytest.mark.gpu
def test_gpu_cpp_mirror_on_the_kernel(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_ACCOUNTS': '0'}, 70)
