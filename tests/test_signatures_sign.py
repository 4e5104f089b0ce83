"""Account signatures in batches: one key signing many messages, or many keys signing one message each (aleo_mi355x_signatures_sign[_host], _min_sign;
aleo_amd.signature.sign_many, Account.sign_many; sign_many in include/aleo_mi355x.hpp).

Row i of a batch is defined as what the one-signature call returns for (key i, message i, nonce seed i), so the host path is held against that call and against
the restatement of signing in Python integers (tests/test_signatures.py, imported as it stands: ref_sign under its own ChaCha20 nonce_of_seed), every row is
verified, and the device lanes — the product modulo the group order first, alone, against Python integers — are emulated on the CPU, plain and under the
sanitizers, on the same cases.  The second half runs the kernels (ALEO_MI355X_MIN_SIGN=1) against the host path.  No test reads the reference tree."""
import ctypes, functools, os, random, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, signature as sg
from oracle import poseidon as ps
import test_signatures as ts
import batch_support as bs
from batch_support import ROOT, HIPCC, le32, num

ACC, R, L = ts.ACC, ts.R, ts.L
CAP = ts.CAP_BYTES
LENGTHS = ts.CHUNK_EDGE_BYTES + ts.BLOCK_EDGE_BYTES              # the field boundaries, then the sponge-block boundaries: the signing preimage has verify's four leading elements
BAD_KEY = le32(R)                                                # the smallest seed that is no canonical field element


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_pool():
    """[(private key, its 32 seed bytes, address x)]: the reference's three accounts and three random keys."""
    rng = random.Random(11)
    keys = [a['private_key'] for a in ACC] + [ts.random_private_key(rng) for _ in range(3)]
    return [(k, le32(ps.private_key_seed(k)), records.Account.from_private_key(k).address_x) for k in keys]


def rejections(seed: bytes) -> int:
    """How many candidates of the seed's ChaCha20 stream are not below the group order before the first that is."""
    count = 0
    while True:
        blk = ts.chacha20_block(seed, count // 2)
        for h in (0, 1):
            if count % 2 == h:
                if (num(blk[32 * h:32 * h + 32]) & ((1 << 251) - 1)) < L: return count
                count += 1


@functools.lru_cache(maxsize=None)
def seeds_of_kind():
    """{kind: [seeds]}: accepted at candidate 0, at candidate 1 (the second half of block 0), at candidate 2 (counter 1), after 4 rejections or more; found by search."""
    out = {0: [], 1: [], 2: [], 4: []}
    i = 0
    while min(len(v) for v in out.values()) < 3:
        i += 1
        seed = le32(0x5eed0000 + i); r = rejections(seed)
        kind = r if r < 3 else 4 if r >= 4 else None
        if kind is not None and len(out[kind]) < 40: out[kind].append(seed)
    return out


def fresh_seeds(n, salt):
    """n distinct nonce seeds that mix the four kinds: the first of each kind in turn, then random ones."""
    rng = random.Random(1000 + salt)
    kinds = seeds_of_kind()
    out = [kinds[k][j] for j in range(3) for k in (0, 1, 2, 4)][:n]
    while len(out) < n: out.append(rng.randbytes(32))
    return out


@functools.lru_cache(maxsize=None)
def batch(n, each, salt=0):
    """(key strings or None per row, key seed rows, messages, nonce seeds) of n rows: lengths from LENGTHS in turn; from n = 63 on one message one byte over the cap
    and, with a key each, one key seed that is no field element."""
    rng = random.Random(2000 + 10 * n + each + 100 * salt)
    pool = key_pool()
    msgs = [rng.randbytes(LENGTHS[(i + salt) % len(LENGTHS)]) for i in range(n)]
    keys = [pool[i % len(pool) if each else salt % len(pool)] for i in range(n)]
    names, rows = [k[0] for k in keys], [k[1] for k in keys]
    if n >= 63:
        msgs[17] = bytes(CAP + 1)
        if each: names[29], rows[29] = None, BAD_KEY
    return names, rows, msgs, fresh_seeds(n, n + salt)


def sign_raw(key_rows, msgs, seeds, host=True, stride=None, offsets=None, null=()):
    """aleo_mi355x_signatures_sign[_host] on raw rows: (status, n x 128 bytes, flags)."""
    n = len(msgs); kb = b''.join(key_rows); text = b''.join(msgs); sb = b''.join(seeds)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    if offsets is not None: off = np.asarray(offsets, dtype=np.uint64)
    rows = np.full((n, 128), 0xee, dtype=np.uint8); flags = np.full(n, 9, dtype=np.uint8)
    L_ = aleo_amd.lib(); call = L_.aleo_mi355x_signatures_sign_host if host else L_.aleo_mi355x_signatures_sign
    args = {'rows': rows.ctypes.data_as(ctypes.c_void_p), 'flags': flags.ctypes.data_as(ctypes.c_void_p), 'keys': ts._vp(kb), 'text': ts._vp(text),
            'off': off.ctypes.data_as(ctypes.c_void_p), 'seeds': ts._vp(sb)}
    for name in null: args[name] = None
    rc = call(args['rows'], args['flags'], args['keys'], (32 if len(key_rows) == n and n > 1 else 0) if stride is None else stride, args['text'], args['off'], args['seeds'], n)
    return rc, [rows[i].tobytes() for i in range(n)], flags.tolist()


@functools.lru_cache(maxsize=None)
def host_rows(n, each, salt=0):
    names, rows, msgs, seeds = batch(n, each, salt)
    rc, out, flags = sign_raw(rows if each else rows[:1], msgs, seeds, host=True, stride=32 if each else 0)
    assert rc == 0
    return out, flags


def wanted_flags(names, msgs): return [3 if name is None or len(m) > CAP else 0 for name, m in zip(names, msgs)]


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(key string or None, key seed, message, nonce seed)]: every length of LENGTHS, the cap and one byte over it under the reference's accounts and random keys in
    turn, a key seed that is no field element, and two seeds of each of the four kinds of nonce seed."""
    rng = random.Random(12)
    pool = key_pool(); kinds = seeds_of_kind()
    out = [(pool[i % len(pool)][0], pool[i % len(pool)][1], rng.randbytes(n), rng.randbytes(32)) for i, n in enumerate(LENGTHS + [CAP, CAP + 1])]
    out.append((None, BAD_KEY, b'no key signs this', rng.randbytes(32)))
    out.append((None, le32((1 << 256) - 1), b'', rng.randbytes(32)))
    for j, kind in enumerate((0, 1, 2, 4, 0, 1, 2, 4)): out.append((pool[j % len(pool)][0], pool[j % len(pool)][1], rng.randbytes(32), kinds[kind][2 - j // 4]))
    return out


@functools.lru_cache(maxsize=None)
def edge_rows():
    c = edge_cases()
    rc, rows, flags = sign_raw([x[1] for x in c], [x[2] for x in c], [x[3] for x in c], host=True, stride=32)
    assert rc == 0
    return rows, flags


# ---- 1: the host path against the one-signature call and against the restatement --------------------------------------------------------------------------------
def test_the_search_finds_every_kind_of_nonce_seed():
    kinds = seeds_of_kind()
    assert [rejections(kinds[k][0]) for k in (0, 1, 2)] == [0, 1, 2] and rejections(kinds[4][0]) >= 4
    for k in kinds: assert ts.nonce_of_seed(kinds[k][0]) < L


def test_host_rows_equal_the_one_signature_call_under_both_strides():
    c = edge_cases(); rows, flags = edge_rows()
    assert flags == wanted_flags([x[0] for x in c], [x[2] for x in c]) and flags.count(3) == 3
    for (key, _, m, seed), row, flag in zip(c, rows, flags):
        assert row == (bytes(128) if flag else sg.sign(key, m, seed).bytes), len(m)
    # one key for all: every message and seed of the cases under the second reference account
    key, key_seed, _ = key_pool()[1]
    rc, rows, flags = sign_raw([key_seed], [x[2] for x in c], [x[3] for x in c], host=True, stride=0)
    assert rc == 0 and flags == [3 if len(x[2]) > CAP else 0 for x in c]
    for (_, _, m, seed), row, flag in zip(c, rows, flags):
        assert row == (bytes(128) if flag else sg.sign(key, m, seed).bytes), len(m)
    # one key that is none: every row is refused
    rc, rows, flags = sign_raw([BAD_KEY], [b'a', b'b'], [bytes(32), bytes([1]) * 32], host=True, stride=0)
    assert (rc, rows, flags) == (0, [bytes(128)] * 2, [3, 3])


def test_host_rows_equal_the_restatement_in_python_integers():
    c = edge_cases(); rows, flags = edge_rows()
    keys = {k[0]: ts.Keys.of_private_key(k[0]) for k in key_pool()}
    checked = 0
    for (key, _, m, seed), row, flag in zip(c, rows, flags):
        if flag: continue
        assert row == ts.ref_sign(keys[key], m, ts.nonce_of_seed(seed)), len(m)      # the message of exactly the cap included: 4161 fields hashed once
        checked += 1
    assert checked == len(c) - 3


def test_every_row_verifies_under_its_address_and_not_with_a_byte_flipped():
    c = edge_cases(); rows, flags = edge_rows()
    addr = {k[0]: k[2] for k in key_pool()}
    good = [(row, addr[x[0]], x[2]) for x, row, flag in zip(c, rows, flags) if not flag]
    assert ts.verify_raw([g[0] for g in good], [g[1] for g in good], [g[2] for g in good], stride=32) == (0, [0] * len(good))
    flipped = [(s, a, m[:len(m) // 2] + bytes([m[len(m) // 2] ^ 0x10]) + m[len(m) // 2 + 1:]) for s, a, m in good if m]
    assert len(flipped) == len(good) - 1                         # all but the message of no bytes
    assert ts.verify_raw([g[0] for g in flipped], [g[1] for g in flipped], [g[2] for g in flipped], stride=32) == (0, [1] * len(flipped))


def test_one_batch_of_64_mixes_the_four_kinds_of_nonce_seed():
    names, key_rows, msgs, seeds = batch(64, True)
    assert {min(rejections(s), 4) for s in seeds[:12]} == {0, 1, 2, 4}
    rows, flags = host_rows(64, True)
    assert flags == wanted_flags(names, msgs) and flags.count(3) == 2
    keys = {k[0]: ts.Keys.of_private_key(k[0]) for k in key_pool()}
    for i in range(12): assert rows[i] == ts.ref_sign(keys[names[i]], msgs[i], ts.nonce_of_seed(seeds[i])), i
    for i in (12, 40, 63): assert rows[i] == sg.sign(names[i], msgs[i], seeds[i]).bytes
    names, key_rows, msgs, seeds = batch(64, False)             # and under one key
    rows, flags = host_rows(64, False)
    assert flags == wanted_flags(names, msgs) and flags.count(3) == 1
    for i in (0, 1, 2, 3, 50): assert rows[i] == sg.sign(names[i], msgs[i], seeds[i]).bytes


def test_the_python_mirror_takes_one_key_a_list_of_keys_or_seed_rows():
    names, key_rows, msgs, seeds = batch(5, True)
    want, _ = host_rows(5, True)
    for keys in (names, np.frombuffer(b''.join(key_rows), dtype=np.uint8).reshape(-1, 32)):
        rows, flags = sg.sign_many(keys, msgs, b''.join(seeds), host=True)
        assert rows.shape == (5, 128) and [r.tobytes() for r in rows] == want and flags.tolist() == [0] * 5
    acct = records.Account.from_private_key(names[0])
    rows, flags = acct.sign_many(msgs, np.frombuffer(b''.join(seeds), dtype=np.uint8).reshape(-1, 32), host=True)
    assert [r.tobytes() for r in rows] == [sg.sign(names[0], m, s).bytes for m, s in zip(msgs, seeds)]
    rows, flags = sg.sign_many(names[0], msgs, host=True)      # seeds drawn from os.urandom: the rows verify
    assert sg.verify_many(rows, acct.address, msgs, host=True).tolist() == [0] * 5
    with pytest.raises(ValueError): sg.sign_many(names[:2], msgs, host=True)
    with pytest.raises(ValueError): sg.sign_many(names[0], msgs, bytes(32 * 4), host=True)
    with pytest.raises(ValueError): records.Account(None, b'', b'', acct.address_x).sign_many(msgs)
    assert sg.sign_many(names[0], [], host=True)[0].shape == (0, 128) and sg.sign_many(names[0], [])[0].shape == (0, 128)


# ---- 2: what the calls refuse ---------------------------------------------------------------------------------------------------------------------------------
def test_what_the_calls_refuse():
    names, key_rows, msgs, seeds = batch(5, True)
    last = lambda: aleo_amd.lib().aleo_mi355x_last_error()
    for host in (True, False):
        for name in ('rows', 'flags', 'keys', 'off', 'seeds', 'text'):
            assert sign_raw(key_rows, msgs, seeds, host=host, null=(name,))[0] == 2, name
        assert sign_raw(key_rows, msgs, seeds, host=host, stride=16)[0] == 2 and b'stride' in last()
        lens = np.cumsum([0] + [len(m) for m in msgs]).tolist()
        assert sign_raw(key_rows, msgs, seeds, host=host, offsets=[1] + lens[1:])[0] == 2 and b'offsets[0]' in last()
        assert sign_raw(key_rows, msgs, seeds, host=host, offsets=lens[:3] + [lens[2] - 1] + lens[4:])[0] == 2 and b'offsets decrease' in last()
        assert sign_raw(key_rows, msgs, seeds[:3] + [seeds[2]] + seeds[4:], host=host)[0] == 2 and b'seeds 2 and 3 ' in last()      # adjacent
        assert sign_raw([], [], [], host=host)[0] == 0 and sign_raw([], [], [], host=host, null=('rows', 'flags', 'keys', 'off', 'seeds', 'text'))[0] == 0      # n = 0
    # far apart, and under different keys: 300 rows, the last seed the second again
    names, key_rows, msgs, seeds = batch(300, True)
    rc, rows, flags = sign_raw(key_rows, msgs, seeds[:299] + [seeds[1]], host=True)
    assert rc == 2 and b'seeds 1 and 299 ' in last() and key_rows[1] != key_rows[299]
    assert rows == [bytes([0xee]) * 128] * 300                   # refused before anything is written
    with pytest.raises(aleo_amd.AleoMi355xError): sg.sign_many(names[0], [b'a', b'b'], bytes(64), host=True)


# ---- 3: the device lanes on the CPU -----------------------------------------------------------------------------------------------------------------------------
def product_rows():
    """[(k, c, s)]: the operands of response = k - c s mod l at their edges, and 1000 random rows."""
    rng = random.Random(13)
    top = (1 << 250) - 1                                         # the largest challenge and the largest sk_sig: hash_to_scalar keeps 250 bits
    c0, s0 = rng.randrange(top), rng.randrange(top)
    t0 = c0 * s0 % L
    rows = [(0, c0, s0), (rng.randrange(L), 0, s0), (rng.randrange(L), c0, 0), (0, 0, 0), (L - 1, top, top), (0, top, top), (L - 1, 1, 1),
            (t0 - 1, c0, s0),                                    # k < c s mod l: the subtraction borrows
            (t0, c0, s0), (top * top % L, top, top),             # k = c s mod l: the response is 0
            (L - 1, L - 1, L - 1), (5, (1 << 256) - 1, (1 << 256) - 1), (L - 1, L, 1), (0, 2 * L, (1 << 256) // L)]      # beyond what signing reaches: any two eight-word numbers
    assert t0 > 0 and rows[7][0] < t0
    rows += [(rng.randrange(L), rng.randrange(top + 1), rng.randrange(top + 1)) for _ in range(1000)]
    return rows


def case_file(path):
    products = product_rows(); c = edge_cases(); rows, flags = edge_rows()
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(products)))
        for k, cc, s in products: f.write(le32(k) + le32(cc) + le32(s) + le32((k - cc * s) % L))
        f.write(struct.pack('<I', len(c)))
        for (_, key_seed, m, seed), row, flag in zip(c, rows, flags): f.write(key_seed + seed + struct.pack('<I', len(m)) + m + bytes([flag]) + row)
    return len(products), len(c)


@pytest.mark.parametrize('sanitized', [False, True], ids=['plain', 'sanitizers'])
def test_device_lane_code_emulated_on_the_host_matches_python_integers_and_the_host_path(tmp_path, sanitized):
    """tests/cpp/signature_sign_lane_emul.cpp: signature_sign_lane.h and account_lane.h with its sink compiled for the CPU over the checked restatement of fr29.h,
    once plain and once with the address and undefined-behaviour sanitizers compiled into that program, run as a program of its own on the products and on every
    case above.  (-fno-strict-aliasing: as tests/test_signatures.py says.)"""
    data = os.path.join(str(tmp_path), 'cases.bin')
    products, count = case_file(data)
    r = bs.run_lane_emul(tmp_path, 'signature_sign_lane_emul', [data], sanitized=sanitized)
    print(r.stdout)
    assert r.returncode == 0 and '%d products, %d signatures, %d signed, 3 refused, 0 mismatches, 0 reads past an end, 0 limb-rule violations' % (products, count, count - 3) in r.stdout, r.stdout + r.stderr


# ---- 4: the threshold, the code object, the C++ mirror ----------------------------------------------------------------------------------------------------------
DEFAULT_MIN_SIGN = 64


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_sign', 'ALEO_MI355X_MIN_SIGN') == (DEFAULT_MIN_SIGN, 5, DEFAULT_MIN_SIGN)
    # below the threshold the call computes on the host: no device is needed for it
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SIGN='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    code = ('from aleo_amd import signature as sg, records; k = %r; rows, flags = sg.sign_many(k, [b"m", b"n"], bytes(range(64))); '
            'print(sg.verify_many(rows, records.Account.from_private_key(k).address, [b"m", b"m"], host=True).tolist(), flags.tolist())' % ACC[0]['private_key'])
    assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300).stdout.split() == ['[0,', '1]', '[0,', '0]']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_signing_kernels_code_object_is_gfx950_and_has_no_scratch_and_no_spills():
    kernels = ('k_signatures_sign', 'k_signer_keys')
    assert bs.scratch_and_spills('signatures_sign', kernels) == (2, {k: (0, 0, 0) for k in kernels})      # these two and no other


def run_cpp_mirror(tmp_path, env, n):
    """tests/cpp/signatures_sign_test.cpp: sign_many and PrivateAccount::sign_many of include/aleo_mi355x.hpp."""
    r = bs.run_cpp_mirror(tmp_path, 'signatures_sign_test', [ACC[0]['private_key'], ACC[1]['private_key'], ACC[0]['address'], n], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_SIGN': '1000000', 'ALEO_MI355X_MIN_SIGNATURES': '1000000'}, 12)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_SIGN', '1')
    monkeypatch.delenv('ALEO_MI355X_SIGN_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_sign()) == 1
    return monkeypatch


def device_rows(n, each, salt=0):
    names, rows, msgs, seeds = batch(n, each, salt)
    rc, out, flags = sign_raw(rows if each else rows[:1], msgs, seeds, host=False, stride=32 if each else 0)
    assert rc == 0, aleo_amd.lib().aleo_mi355x_last_error()
    return out, flags


@pytest.mark.gpu
@pytest.mark.parametrize('each', [False, True], ids=['one key', 'a key each'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_gpu_rows_equal_the_host_path_at_wave_and_block_edges(on_kernel, n, each):
    names, rows, msgs, seeds = batch(n, each)
    want = host_rows(n, each)
    got = device_rows(n, each)
    assert got[1] == want[1] and [i for i in range(n) if got[0][i] != want[0][i]] == []
    if n >= 63:
        assert want[1].count(3) == (2 if each else 1) and {min(rejections(s), 4) for s in seeds[:12]} == {0, 1, 2, 4} and {len(m) for m in msgs} >= set(LENGTHS)


@pytest.mark.gpu
def test_gpu_one_wave_of_every_edge_case_at_once(on_kernel):
    """Messages from 0 bytes to the cap and one over it, both kinds of refused row and every kind of nonce seed in one wave, a key each."""
    c = edge_cases(); want = edge_rows()
    assert len(c) <= 64
    rc, rows, flags = sign_raw([x[1] for x in c], [x[2] for x in c], [x[3] for x in c], host=False, stride=32)
    assert rc == 0 and flags == want[1] and [len(x[2]) for x, a, b in zip(c, rows, want[0]) if a != b] == []


@pytest.mark.gpu
def test_gpu_both_sides_of_the_threshold_and_chunked_launches_return_the_same_bytes(monkeypatch):
    monkeypatch.delenv('ALEO_MI355X_SIGN_CHUNK', raising=False)
    for each in (False, True):
        want = host_rows(257, each)
        monkeypatch.setenv('ALEO_MI355X_MIN_SIGN', '258'); assert device_rows(257, each) == want      # below: the host code inside the call
        monkeypatch.setenv('ALEO_MI355X_MIN_SIGN', '257'); assert device_rows(257, each) == want      # at it: the kernel
        monkeypatch.setenv('ALEO_MI355X_SIGN_CHUNK', '100'); assert device_rows(257, each) == want    # three launches
        monkeypatch.delenv('ALEO_MI355X_SIGN_CHUNK')
    names, key_rows, msgs, seeds = batch(257, True)
    rows, flags = sg.sign_many(np.frombuffer(b''.join(key_rows), dtype=np.uint8).reshape(-1, 32), msgs, b''.join(seeds))      # the Python mirror on the kernel
    assert ([r.tobytes() for r in rows], flags.tolist()) == host_rows(257, True)


@pytest.mark.gpu
def test_gpu_the_rows_verify_on_the_gpu(on_kernel):
    on_kernel.setenv('ALEO_MI355X_MIN_SIGNATURES', '0')
    names, key_rows, msgs, seeds = batch(257, True)
    rows, flags = device_rows(257, True)
    addr = {k[0]: k[2] for k in key_pool()}
    good = [i for i in range(257) if not flags[i]]
    assert len(good) == 255
    assert ts.verify_raw([rows[i] for i in good], [addr[names[i]] for i in good], [msgs[i] for i in good], host=False, stride=32) == (0, [0] * 255)


@pytest.mark.gpu
def test_gpu_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    want = [host_rows(130, True, 1), host_rows(90, False, 2)]
    assert bs.two_threads(lambda i: device_rows(130, True, 1) if i == 0 else device_rows(90, False, 2)) == want


@pytest.mark.gpu
def test_gpu_cpp_mirror_on_the_kernel(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_SIGN': '1', 'ALEO_MI355X_MIN_SIGNATURES': '0'}, 70)
