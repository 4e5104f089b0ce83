"""The ownership scan of record ciphertexts (aleo_mi355x_record_parse, aleo_mi355x_records_scan / _scan_host, aleo_mi355x_min_records;
aleo_amd/records.py) against the data the reference's own tests hold (tests/golden/reference_records.json, written by
tests/golden/gen_reference_records.py) and against the rule written out with oracle/poseidon.py:

    private owner c0, nonce x:  N = the prime-order point with that x;  rvk = x(view_key * N);
    randomizer = hash_many_psd8([domain_separator("AleoSymmetricEncryption0"), rvk], 1)[0];  owner <=> c0 - randomizer == address x

and, for an on-curve x without a prime-order point, the same with k = the odd one of {view_key, view_key + l} on either root.
The first half needs no GPU (parser, host path, threshold, the kernel's code object and its lane code emulated on the host); the second half runs the kernel."""
import ctypes, json, os, random, re, subprocess, sys, tempfile
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, wire
from oracle import poseidon as ps, pyref as P
import batch_support as bs
from batch_support import ROOT, HIPCC, le32

REF = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_records.json')))
R, L_ORDER = P.FR_MODULUS, ps.ED_SUBGROUP_ORDER
ENC_DOMAIN = ps.domain_separator('AleoSymmetricEncryption0')


def account_generator():
    """The account generator G, recovered from a reference-held (view key, address) pair as tests/test_poseidon.py does."""
    return ps.ed_mul(ps.address_point(REF['addresses']['owner']), pow(ps.view_key_scalar(REF['view_keys']['owner']), -1, L_ORDER))


def rows(vals): return np.frombuffer(b''.join(le32(v) for v in vals), dtype=np.uint8).reshape(-1, 32).copy() if len(vals) else np.zeros((0, 32), dtype=np.uint8)
def randomizer(rvk): return ps.hash_many_psd8([ENC_DOMAIN, rvk], 1)[0]


def oracle_rule(c0, nx, view_key, addr_x):
    """(flag, rvk) by the rule of the module docstring, in Python integers."""
    if c0 >= R or nx >= R: return 2, 0
    y = P.fr_sqrt((1 + nx * nx) * pow((1 - ps.ED_D * nx * nx) % R, -1, R) % R)
    if y is None: return 2, 0
    try:
        rvk = ps.ed_mul(ps.ed_from_x(nx), view_key)[0]                                     # upstream's rule where upstream accepts the nonce
    except ValueError:
        rvk = ps.ed_mul((nx, y), view_key if view_key & 1 else view_key + L_ORDER)[0]      # the scan's contract everywhere else
    return (1 if (c0 - randomizer(rvk)) % R == addr_x else 0), rvk


def find_x(rng, want):
    """An x that is 'off' the curve, or on it with 'no_prime' point of prime order."""
    while True:
        x = rng.randrange(R)
        y = P.fr_sqrt((1 + x * x) * pow((1 - ps.ED_D * x * x) % R, -1, R) % R)
        if want == 'off':
            if y is None: return x
        elif y is not None:
            try: ps.ed_from_x(x)
            except ValueError: return x


def synthetic_records(n_owned, n_foreign, view_key, seed, G):
    """Records made by encrypting: nonce = s G, c0 = address x + randomizer(x(view_key * nonce)) for the owned ones and for another account's address for
    the foreign ones; then the edge cases.  Returns (c0 list, nonce list, address x, names of the edge cases by index)."""
    rng = random.Random(seed)
    A = ps.ed_mul(G, view_key); other = ps.ed_mul(G, rng.randrange(1, L_ORDER))[0]
    c0s, nxs, wrapped = [], [], 0
    made = 0
    while made < n_owned or not wrapped:                         # keep encrypting until one owner field wrapped: c0 = address + randomizer - r < randomizer
        N = ps.ed_mul(G, rng.randrange(1, L_ORDER)); rnd = randomizer(ps.ed_mul(N, view_key)[0])
        wraps = A[0] + rnd >= R
        if made >= n_owned and not wraps: continue
        c0s.append((A[0] + rnd) % R); nxs.append(N[0]); made += 1; wrapped += wraps
    for _ in range(n_foreign):
        N = ps.ed_mul(G, rng.randrange(1, L_ORDER)); c0s.append((other + randomizer(ps.ed_mul(N, view_key)[0])) % R); nxs.append(N[0])
    edge = {}
    def add(name, c0, nx): edge[len(c0s)] = name; c0s.append(c0); nxs.append(nx)
    add('nonce x = 0, not owned', rng.randrange(R), 0)
    add('nonce x = 0, owned', (A[0] + randomizer(0)) % R, 0)                                    # x(k (0, +-1)) = 0
    add('x off the curve', rng.randrange(R), find_x(rng, 'off'))
    xn = find_x(rng, 'no_prime'); add('on the curve, no prime-order point', rng.randrange(R), xn)
    y = P.fr_sqrt((1 + xn * xn) * pow((1 - ps.ED_D * xn * xn) % R, -1, R) % R)
    k = view_key if view_key & 1 else view_key + L_ORDER
    add('no prime-order point, owner by the formula', (A[0] + randomizer(ps.ed_mul((xn, y), k)[0])) % R, xn)
    add('c0 = r', R, nxs[0]); add('c0 = 2^256 - 1', (1 << 256) - 1, nxs[0]); add('nonce = r', c0s[0], R); add('nonce = 2^256 - 1', c0s[0], (1 << 256) - 1)
    return c0s, nxs, A[0], edge


# ---- 1, 4: the parser -----------------------------------------------------------------------------------------------------------------------------
def test_parser_reads_the_reference_ciphertexts_and_they_re_encode():
    for name, s in REF['records'].items():
        rec = records.RecordCiphertext.from_string(s)
        assert rec.owner_kind == records.OWNER_PRIVATE and str(rec) == s
        if name in REF['nonces']: assert int.from_bytes(rec.nonce, 'little') == int(REF['nonces'][name]), name      # the `_nonce` literal of the reference's plaintext
        hrp, payload = wire.bech32m_decode(s)
        assert hrp == 'record' and wire.bech32m_encode('record', payload) == s
        assert payload[0] == 1 and payload[1:3] == b'\x01\x00' and payload[3:35] == rec.owner and payload[-32:] == rec.nonce
    assert len(wire.bech32m_decode(REF['records']['owner'])[1]) == 118


def test_parser_refuses_what_is_not_a_record():
    L = aleo_amd.lib()
    def status(s):
        kind = ctypes.c_int32(0); a = np.zeros(32, dtype=np.uint8); b = np.zeros(32, dtype=np.uint8)
        return L.aleo_mi355x_record_parse(s.encode(), ctypes.byref(kind), a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p))
    good = REF['records']['owner']
    assert status(good) == 0
    for s in REF['invalid'].values(): assert status(s) != 0, s                                  # the reference's own invalid_bech32 and "garbage"
    payload = wire.bech32m_decode(good)[1]
    enc = lambda b, hrp='record': wire.bech32m_encode(hrp, bytes(b))
    assert status(enc(payload)) == 0
    bad = {
        'truncated': payload[:-1], 'truncated to the owner': payload[:35], 'empty': b'', 'trailing byte': payload + b'\0',
        'field count 2': payload[:1] + b'\x02\x00' + payload[3:], 'owner variant 2': b'\x02' + payload[1:],
        'owner field not canonical': payload[:3] + b'\xff' * 32 + payload[35:], 'nonce not canonical': payload[:-32] + le32(R),
    }
    assert payload[36] == 12 and payload[37:49] == b'microcredits' and int.from_bytes(payload[49:51], 'little') == 35      # where the entry's length sits
    bad['entry length past the end'] = payload[:49] + b'\xff\xff' + payload[51:]
    for why, b in bad.items(): assert status(enc(b)) != 0, why
    assert status(enc(payload, 'rekord')) != 0 and status(good[:-1] + ('q' if good[-1] != 'q' else 'p')) != 0 and status(good[:40]) != 0 and status('') != 0
    pub = b'\x00' + payload[3:35] + payload[35:]                                                # a public owner: the same record with the address in the clear
    rec = records.RecordCiphertext.from_string(enc(pub))
    assert rec.owner_kind == records.OWNER_PUBLIC and rec.owner == payload[3:35] and rec.is_owner(1, rec.owner) and not rec.is_owner(1, le32(5))
    with pytest.raises(aleo_amd.AleoMi355xError): records.RecordCiphertext.from_string('garbage')


# ---- 2, 3: the host path --------------------------------------------------------------------------------------------------------------------------
def reference_cases(G):
    for case in REF['is_owner']:
        rec = records.RecordCiphertext.from_string(REF['records'][case['record']])
        vk = REF['view_keys'][case['view_key']]
        addr = REF['addresses'][case['address']] if case['address'] else le32(ps.ed_mul(G, ps.view_key_scalar(vk))[0])      # the non-owner's own address: view key x G
        yield case, rec, vk, addr


def check_reference_vectors(host):
    G = account_generator()
    for case, rec, vk, addr in reference_cases(G):
        flags, rvk = records.scan(np.frombuffer(rec.owner, dtype=np.uint8), np.frombuffer(rec.nonce, dtype=np.uint8), vk, addr, host=host)
        assert bool(flags[0] == 1) == case['expected'] and flags[0] in (0, 1), case
        want = oracle_rule(int.from_bytes(rec.owner, 'little'), int.from_bytes(rec.nonce, 'little'), ps.view_key_scalar(vk), int.from_bytes(records.address_x_bytes(addr), 'little'))
        assert (int(flags[0]), int.from_bytes(rvk[0].tobytes(), 'little')) == want
    assert ps.ed_mul(G, ps.view_key_scalar(REF['view_keys']['sdk']))[0] == int.from_bytes(records.address_x_bytes(REF['addresses']['sdk']), 'little')


def test_host_path_reproduces_the_booleans_the_reference_asserts():
    check_reference_vectors(host=True)
    # the owner's key against the other account's address, and the reverse: neither owns it
    rec = records.RecordCiphertext.from_string(REF['records']['owner']); G = account_generator()
    other = le32(ps.ed_mul(G, ps.view_key_scalar(REF['view_keys']['non_owner']))[0])
    f = lambda vk, a: int(records.scan(np.frombuffer(rec.owner, dtype=np.uint8), np.frombuffer(rec.nonce, dtype=np.uint8), vk, a, host=True)[0][0])
    assert f(REF['view_keys']['owner'], other) == 0 and f(REF['view_keys']['non_owner'], REF['addresses']['owner']) == 0


def check_against_oracle(c0s, nxs, vk, ax, flags, rvk, idx):
    for i in idx:
        want = oracle_rule(c0s[i], nxs[i], vk, ax)
        assert (int(flags[i]), int.from_bytes(rvk[i].tobytes(), 'little')) == want, (i, c0s[i], nxs[i])


def test_host_path_equals_the_rule_written_with_the_oracle_on_256_synthetic_records():
    G = account_generator(); rng = random.Random(77)
    total = 0
    for vk in (rng.randrange(1, L_ORDER) | 1, rng.randrange(2, L_ORDER) & ~1):                 # an odd and an even view key
        c0s, nxs, ax, edge = synthetic_records(40, 79, vk, 1000 + (vk & 1), G)
        flags, rvk = records.scan(rows(c0s), rows(nxs), vk, ax, host=True)
        check_against_oracle(c0s, nxs, vk, ax, flags, rvk, range(len(c0s)))
        names = {v: k for k, v in edge.items()}
        expect = {'nonce x = 0, not owned': 0, 'nonce x = 0, owned': 1, 'x off the curve': 2, 'on the curve, no prime-order point': 0, 'no prime-order point, owner by the formula': 1,
                  'c0 = r': 2, 'c0 = 2^256 - 1': 2, 'nonce = r': 2, 'nonce = 2^256 - 1': 2}
        for name, want in expect.items(): assert flags[names[name]] == want, name
        assert not rvk[flags == 2].any() and rvk[names['nonce x = 0, owned']].tobytes() == bytes(32)
        n_owned = len(c0s) - 79 - len(edge)
        assert (flags[:n_owned] == 1).all() and (flags[n_owned:n_owned + 79] == 0).all()
        assert any(c0s[i] < randomizer(int.from_bytes(rvk[i].tobytes(), 'little')) for i in range(n_owned))      # c0 - randomizer wrapped below zero
        total += len(c0s)
    assert total >= 256
    L = aleo_amd.lib(); z = np.zeros((1, 32), dtype=np.uint8); f = np.zeros(1, dtype=np.uint8); p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.aleo_mi355x_records_scan_host(p(f), None, p(z), p(z), 0, p(rows([1])), p(z)) == 0                    # n = 0, no rvk_out
    assert L.aleo_mi355x_records_scan_host(p(f), None, p(z), p(z), 1, p(rows([L_ORDER])), p(z)) != 0              # the view key is not below l
    assert L.aleo_mi355x_records_scan_host(p(f), None, p(z), p(z), 1, p(rows([1])), p(rows([R]))) != 0            # the address x is not canonical
    assert L.aleo_mi355x_records_scan_host(p(f), None, p(z), p(z), 1, p(rows([0])), p(z)) == 0                    # view key 0: k = l


# ---- 5: the threshold -------------------------------------------------------------------------------------------------------------------------------
def test_routing_threshold_and_its_environment_override():
    default, large, zero, nonsense = bs.threshold_reads('min_records', 'ALEO_MI355X_MIN_RECORDS', ('65536', '0', 'nonsense'))
    assert 1 <= default <= 1 << 22 and (large, zero, nonsense) == (65536, 0, default)
    # below the threshold the call computes on the host: no device is needed for it
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_RECORDS='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    code = ('import numpy as np, json; from aleo_amd import records; R = json.load(open(%r)); r = records.RecordCiphertext.from_string(R["records"]["owner"]); '
            'print(r.is_owner(R["view_keys"]["owner"], R["addresses"]["owner"]))' % os.path.join(ROOT, 'tests', 'golden', 'reference_records.json'))
    assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300).stdout.split() == ['True']


# ---- 6: the kernel's code object, and its lane code on the host ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_scan_kernel_code_object_is_gfx950_and_has_no_scratch():
    import code_object as co
    asm, blocks = co.compile_unit('records_many')                         # the one-account scan runs the K-account kernel at one key per lane
    meta = co.block_of(blocks, 'k_records_scan_manyILi1E')
    print(co.registers('k_records_scan_many<1>', meta))
    assert co.field(meta, 'private_segment_fixed_size') == 0 and co.field(meta, 'vgpr_spill_count') == 0
    start = re.search(r'^_Z\w*k_records_scan_manyILi1E\w*:', asm, flags=re.M).start()
    body = asm[start:asm.index('.Lfunc_end', start)]
    code = [l.split(';')[0].strip() for l in body.split('\n')]
    assert sum(1 for l in code if l.startswith('v_mad_u64_u32')) > 10000                                   # the arithmetic is there, inline


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path):
    """tests/cpp/records_lane_emul.cpp: records_lane.h compiled for the CPU over a restatement of fr29.h that checks every limb bound."""
    r = bs.run_lane_emul(tmp_path, 'records_lane_emul', flags=(), hipcc=True)
    assert r.returncode == 0 and ' 0 mismatches, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_RECORDS', '0')
    assert int(aleo_amd.lib().aleo_mi355x_min_records()) == 0


def big_batch(n, vk, seed, G):
    """n records with nonces (s + i) G: about one in a hundred encrypted to the account, the rest random owner fields, the edge cases of the small set sprinkled in."""
    rng = random.Random(seed)
    A = ps.ed_mul(G, vk); s = rng.randrange(1, L_ORDER)
    N, VN = ps.ed_mul(G, s), ps.ed_mul(A, s)                      # nonce and view_key * nonce, both stepped by one generator at a time
    c0s, nxs, owned = [], [], []
    for i in range(n):
        nxs.append(N[0])
        if rng.randrange(100) == 0: c0s.append((A[0] + randomizer(VN[0])) % R); owned.append(i)
        else: c0s.append(rng.randrange(R))
        N, VN = ps.ed_add(N, G), ps.ed_add(VN, A)
    e_c0, e_nx, _, edge = synthetic_records(2, 2, vk, seed + 1, G)
    first = len(e_c0) - len(edge); where = {}
    for j, k in enumerate(sorted(edge)):
        at = rng.randrange(n)
        while at in owned or at in where: at = rng.randrange(n)
        c0s[at], nxs[at] = e_c0[k], e_nx[k]; where[at] = edge[k]
    return c0s, nxs, A[0], owned, where


@pytest.mark.gpu
def test_kernel_reproduces_the_booleans_the_reference_asserts(on_kernel):
    check_reference_vectors(host=False)


@pytest.mark.gpu
def test_kernel_equals_the_host_path_and_the_oracle(on_kernel):
    G = account_generator(); rng = random.Random(5)
    n = (1 << 16) + 3
    vk = rng.randrange(2, L_ORDER) & ~1
    c0s, nxs, ax, owned, where = big_batch(n, vk, 4242, G)
    C0, NX = rows(c0s), rows(nxs)
    flags, rvk = records.scan(C0, NX, vk, ax)
    hflags, hrvk = records.scan(C0, NX, vk, ax, host=True)
    assert flags.tobytes() == hflags.tobytes() and rvk.tobytes() == hrvk.tobytes()
    assert sorted(np.nonzero(flags == 1)[0].tolist()) == sorted(owned + [i for i, name in where.items() if 'owner' in name or name.endswith(', owned')])
    assert 500 < len(owned) < 800 and (flags == 2).sum() == 5
    sample = list(where) + owned[:40]
    sample += [i for i in rng.sample(range(n), 300) if i not in sample][:256 - len(sample)]
    assert len(sample) == 256
    check_against_oracle(c0s, nxs, vk, ax, flags, rvk, sample)
    for m in (0, 1, 63, 64, 65):                                  # the tail lanes of the last wave
        lo = max(owned[0] - 1, 0)
        f, r = records.scan(C0[lo:lo + m], NX[lo:lo + m], vk, ax)
        assert f.tobytes() == hflags[lo:lo + m].tobytes() and r.tobytes() == hrvk[lo:lo + m].tobytes(), m
    vk2 = vk | 1                                                   # an odd key, the same address: other digits, nothing stale
    f2, r2 = records.scan(C0[:4096], NX[:4096], vk2, ax); h2, hr2 = records.scan(C0[:4096], NX[:4096], vk2, ax, host=True)
    assert f2.tobytes() == h2.tobytes() and r2.tobytes() == hr2.tobytes() and r2.tobytes() != rvk[:4096].tobytes()


@pytest.mark.gpu
def test_kernel_small_behaviours(on_kernel):
    G = account_generator()
    sets = []
    for t, vk in enumerate((0x1234567 | 1, 0x7654320)):
        c0s, nxs, ax, owned, where = big_batch(3000 + 17 * t, vk, 900 + t, G)
        C0, NX = rows(c0s), rows(nxs)
        sets.append((C0, NX, vk, ax, records.scan(C0, NX, vk, ax)))
    C0, NX, vk, ax, (flags, rvk) = sets[0]
    only_flags, none = records.scan(C0, NX, vk, ax, want_rvk=False)                # rvk_out = NULL
    assert none is None and only_flags.tobytes() == flags.tobytes()
    hf, hr = records.scan(C0, NX, vk, ax, host=True)
    assert flags.tobytes() == hf.tobytes() and rvk.tobytes() == hr.tobytes() and (flags == 1).any()
    # two threads, different batches and keys at once: each gets the bytes it gets alone
    got = bs.two_threads(lambda i: records.scan(*sets[i][:4]))
    for i in range(2): assert got[i][0].tobytes() == sets[i][4][0].tobytes() and got[i][1].tobytes() == sets[i][4][1].tobytes()
    # another view key on the same records right after: neither stale digits nor a stale state
    again = records.scan(C0, NX, sets[1][2], ax); want = records.scan(C0, NX, sets[1][2], ax, host=True)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes() and again[1].tobytes() != rvk.tobytes()


@pytest.mark.gpu
def test_one_account_scan_through_the_many_key_flow_at_every_width(on_kernel, monkeypatch):
    """records.scan runs scan_many_on_device with a table of one key: at ALEO_MI355X_SCAN_KEYS_PER_LANE = 2, 4, 8 that key is padded with zero entries."""
    G = account_generator()
    vk = 0x2468ACE | 1
    c0s, nxs, ax, owned, where = big_batch(257, vk, 31337, G)
    C0, NX = rows(c0s), rows(nxs)
    hf, _ = records.scan(C0, NX, vk, ax, host=True)
    own, bad = np.nonzero(hf == 1)[0].tolist(), np.nonzero(hf == 2)[0].tolist()
    assert len(own) >= 3 and bad
    order = list(range(257))
    for src, dst in ((own[0], 0), (bad[0], 1), (own[1], 64), (own[2], 256)):      # an owned record first, a malformed nonce, an owned record in the last partial wave of 65 and of 257
        a, b = order.index(src), dst
        order[a], order[b] = order[b], order[a]
    C0, NX = C0[order].copy(), NX[order].copy()
    hf, hr = records.scan(C0, NX, vk, ax, host=True)
    assert hf[0] == 1 and hf[1] == 2 and hf[64] == 1 and hf[256] == 1
    for width in (None, '2', '4', '8'):
        if width is None: monkeypatch.delenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', raising=False)
        else: monkeypatch.setenv('ALEO_MI355X_SCAN_KEYS_PER_LANE', width)
        for n in (1, 64, 65, 257):
            f, r = records.scan(C0[:n], NX[:n], vk, ax)
            assert f.tobytes() == hf[:n].tobytes() and r.tobytes() == hr[:n].tobytes(), (width, n)
            only_flags, none = records.scan(C0[:n], NX[:n], vk, ax, want_rvk=False)
            assert none is None and only_flags.tobytes() == hf[:n].tobytes(), (width, n)


@pytest.mark.gpu
def test_mirrors_on_the_reference_strings(on_kernel, tmp_path):
    G = account_generator()
    strings = [REF['records']['owner'], REF['records']['sdk_foreign'], REF['records']['sdk']]
    idx, rvks = records.find_owned(strings, REF['view_keys']['sdk'], REF['addresses']['sdk'])      # isOwner(viewKey) is true for the account's record ...
    assert idx == [0, 2] and rvks[0] == rvks[1] and len(rvks[0]) == 32
    rec = records.RecordCiphertext.from_string(strings[0])
    assert int.from_bytes(rvks[0], 'little') == ps.ed_mul(ps.ed_from_x(int.from_bytes(rec.nonce, 'little')), ps.view_key_scalar(REF['view_keys']['sdk']))[0]
    foreign = REF['view_keys']['sdk_foreign']                                                        # ... and false for the foreign view key
    assert records.find_owned(strings[2:], foreign, le32(ps.ed_mul(G, ps.view_key_scalar(foreign))[0])) == ([], [])
    for case, rec, vk, addr in reference_cases(G): assert rec.is_owner(vk, addr) == case['expected']
    from test_abi import build_cpp_host_mirror
    exe = build_cpp_host_mirror(tmp_path, 'records_scan_test')
    args = []                                                      # record, view key, address, expected — the reference's four assertions
    for case, rec, vk, addr in reference_cases(G):
        args += [str(rec), vk, addr if isinstance(addr, str) else wire.bech32m_encode('aleo', addr), '1' if case['expected'] else '0']
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=dict(os.environ, ALEO_MI355X_MIN_RECORDS='0'))
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr
