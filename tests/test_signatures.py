"""Account signatures: sign, the sign1… string and the verification of many signatures in one call (aleo_mi355x_signature_sign, _signature_to_string,
_signature_from_string, _signatures_verify[_host]; aleo_amd/signature.py, Account.sign / verify in aleo_amd/records.py; the same in include/aleo_mi355x.hpp).

The reference holds no signature: its own tests are round trips (wasm/src/account/signature.rs:98-115).  So the product is tied to code it does not share — a
restatement of signing and verification in Python integers below (affine twisted-Edwards arithmetic written here, Poseidon from oracle/poseidon.py, the generator
recovered from the first reference account as view_key^-1 address, the nonce's ChaCha20 written here) — in both directions; the reference's own assertion follows
on its three accounts; then the flags, the edges of the arithmetic and the strings.  The host path, flag for flag, checks the device lane: emulated on the CPU,
plain and under the sanitizers, here, and on the GPU in the second half (ALEO_MI355X_MIN_SIGNATURES=0).  No test reads the reference tree."""
import ctypes, functools, json, os, random, re, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import records, signature as sg
from oracle import poseidon as ps
from oracle import pyref as P
import batch_support as bs
from batch_support import HERE, ROOT, CSRC, HIPCC, SANITIZE, le32, num, _vp

ACC = json.load(open(os.path.join(HERE, 'golden', 'reference_account.json')))['accounts']
R, L, D = ps.R, ps.ED_SUBGROUP_ORDER, ps.ED_D
MAX_FIELDS = 128 * 1024 * 8 // 252                                                  # 4161
CAP_BYTES = MAX_FIELDS * 252 // 8                                                   # 131071: the longest message of at most that many fields


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------------
def add(p, q):
    """-x^2 + y^2 = 1 + d x^2 y^2, affine: complete, since -1 is a square and d is not."""
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 % R * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R) % R, (y1 * y2 + x1 * x2) * pow(1 - k, -1, R) % R)


def mul(p, k: int):
    acc = (0, 1)
    for i in reversed(range(k.bit_length())):
        acc = add(acc, acc)
        if (k >> i) & 1: acc = add(acc, p)
    return acc


def from_x(x: int):
    """The point of the prime-order subgroup with this x-coordinate, or None."""
    y = P.fr_sqrt((1 + x * x) * pow((1 - D * x * x) % R, -1, R) % R)
    if y is None: return None
    for yy in (y, (R - y) % R):
        if mul((x, yy), L) == (0, 1): return (x, yy)
    return None


@functools.lru_cache(maxsize=None)
def generator():
    a = ACC[0]
    return mul(ps.address_point(a['address']), pow(ps.view_key_scalar(a['view_key']), -1, L))


def fields_of(message: bytes):
    """Bits little-endian within a byte, 252 to a field, the last one short; none for no bytes."""
    v, n = num(message), 8 * len(message)
    return [(v >> (252 * j)) & ((1 << 252) - 1) for j in range((n + 251) // 252)]


def challenge_of(grx, pkx, prx, ax, message): return ps.hash_to_scalar(8, [grx, pkx, prx, ax] + fields_of(message))


class Keys:
    """sk_sig and r_sig, and what follows from them."""
    def __init__(self, sk_sig: int, r_sig: int):
        G = generator()
        self.sk, self.pk, self.pr = sk_sig, mul(G, sk_sig), mul(G, r_sig)
        self.view = (sk_sig + r_sig + ps.hash_to_scalar(4, [self.pk[0], self.pr[0]])) % L
        self.ax = mul(G, self.view)[0]

    @classmethod
    def of_private_key(cls, private_key: str):
        seed = ps.private_key_seed(private_key)
        return cls(ps.hash_to_scalar(2, [ps.domain_separator('AleoAccountSignatureSecretKey0'), seed]), ps.hash_to_scalar(2, [ps.domain_separator('AleoAccountSignatureRandomizer0.0'), seed]))


def ref_sign(keys: Keys, message: bytes, nonce: int) -> bytes:
    c = challenge_of(mul(generator(), nonce)[0], keys.pk[0], keys.pr[0], keys.ax, message)
    return le32(c) + le32((nonce - c * keys.sk) % L) + le32(keys.pk[0]) + le32(keys.pr[0])


def ref_verify(sig: bytes, ax: int, message: bytes) -> int:
    c, s, pkx, prx = (num(sig[32 * i:32 * i + 32]) for i in range(4))
    if c >= L or s >= L or pkx >= R or prx >= R or ax >= R or len(fields_of(message)) > MAX_FIELDS: return 3
    pk, pr = from_x(pkx), from_x(prx)
    if pk is None or pr is None: return 3
    G = generator()
    gr = add(mul(G, s), mul(pk, c))
    candidate = add(add(pk, pr), mul(G, ps.hash_to_scalar(4, [pkx, prx])))
    return 0 if challenge_of(gr[0], pkx, prx, ax, message) == c and candidate[0] == ax else 1


def chacha20_block(key: bytes, counter: int) -> bytes:
    """D. J. Bernstein's ChaCha20, 64-bit counter, nonce 0."""
    rot = lambda v, n: ((v << n) | (v >> (32 - n))) & 0xffffffff
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(struct.unpack('<8I', key)) + [counter & 0xffffffff, counter >> 32, 0, 0]
    x = list(init)
    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rot(x[d] ^ x[a], 16); x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rot(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rot(x[d] ^ x[a], 8); x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rot(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15); qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack('<16I', *[(a + b) & 0xffffffff for a, b in zip(x, init)])


def nonce_of_seed(seed: bytes) -> int:
    """The first candidate below the group order: 32-byte blocks of the stream, the low 251 bits of each."""
    counter = 0
    while True:
        blk = chacha20_block(seed, counter); counter += 1
        for h in (0, 1):
            v = num(blk[32 * h:32 * h + 32]) & ((1 << 251) - 1)
            if v < L: return v


# ---- through the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def verify_raw(sigs, addrs, messages, host=True, stride=None, offsets=None):
    """aleo_mi355x_signatures_verify[_host] on raw rows: (status, flags)."""
    n = len(sigs); sb = b''.join(sigs); ab = b''.join(addrs); text = b''.join(messages)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    if offsets is not None: off = np.asarray(offsets, dtype=np.uint64)
    flags = np.full(n, 9, dtype=np.uint8)
    L_ = aleo_amd.lib(); call = L_.aleo_mi355x_signatures_verify_host if host else L_.aleo_mi355x_signatures_verify
    rc = call(flags.ctypes.data_as(ctypes.c_void_p), _vp(sb), _vp(ab), (32 if len(addrs) == n and n > 1 else 0) if stride is None else stride, _vp(text), off.ctypes.data_as(ctypes.c_void_p), n)
    return rc, flags.tolist()


def host_flag(sig: bytes, ax, message: bytes) -> int:
    rc, flags = verify_raw([sig], [le32(ax) if isinstance(ax, int) else ax], [message])
    assert rc == 0
    return flags[0]


@functools.lru_cache(maxsize=None)
def reference_accounts():
    """[(private key, Keys, address x bytes)] of the three reference accounts; the restatement's derivation gives the addresses the reference holds."""
    out = []
    for a in ACC:
        k = Keys.of_private_key(a['private_key'])
        assert le32(k.ax) == records.address_x_bytes(a['address']) and ps.view_key_string(k.view) == a['view_key']
        out.append((a['private_key'], k, le32(k.ax)))
    return out


def random_private_key(rng) -> str: return ps.private_key_string(rng.randrange(R))


# ---- 1: the product against the restatement, both ways --------------------------------------------------------------------------------------------------
def test_signatures_made_by_the_restatement_verify_through_the_host_call():
    rng = random.Random(1)
    for i, (_, keys, ax) in enumerate(reference_accounts()):
        m = rng.randbytes(32)
        s = ref_sign(keys, m, rng.randrange(L))
        assert ref_verify(s, keys.ax, m) == 0 and host_flag(s, ax, m) == 0
        assert host_flag(s, ax, m[:-1] + bytes([m[-1] ^ 1])) == 1
    odd = Keys(rng.randrange(L), rng.randrange(L))                 # an account of no private key: any two scalars
    m = b'any two scalars make an account'
    assert host_flag(ref_sign(odd, m, rng.randrange(L)), odd.ax, m) == 0


def test_signatures_made_by_the_product_verify_in_the_restatement_and_equal_it_under_the_same_nonce():
    rng = random.Random(2)
    for key, keys, ax in list(reference_accounts()) + [(k, Keys.of_private_key(k), None) for k in (random_private_key(rng) for _ in range(2))]:
        m, seed = rng.randbytes(rng.randrange(0, 80)), rng.randbytes(32)
        s = sg.sign(key, m, seed)
        assert s.bytes == ref_sign(keys, m, nonce_of_seed(seed))            # challenge, response and both x-coordinates
        assert ref_verify(s.bytes, keys.ax, m) == 0
        assert s.verify(le32(keys.ax), m) and sg.sign(key, m, seed) == s and sg.sign(key, m, rng.randbytes(32)) != s
        assert records.Account.from_private_key(key).address_x == le32(keys.ax)


def test_the_nonce_is_rejection_sampled_below_the_group_order():
    """Among a few hundred seeds some must reject their first block (l / 2^251 = 0.58): the product's signatures equal the restatement's for those too."""
    key, keys, _ = reference_accounts()[0]
    rejecting = [s for s in (le32(i + 1) for i in range(40)) if (num(chacha20_block(s, 0)[:32]) & ((1 << 251) - 1)) >= L]
    assert len(rejecting) >= 5
    for seed in rejecting[:3]: assert sg.sign(key, b'm', seed).bytes == ref_sign(keys, b'm', nonce_of_seed(seed))


# ---- 2: the reference's own assertion ---------------------------------------------------------------------------------------------------------------------
def test_round_trips_as_the_reference_tests_them():
    """signature.rs:98-115 on the three reference accounts and random keys: a signature verifies under its account's address, and not over another message, under
    another account's address, or with any one of its four parts taken from another valid signature."""
    rng = random.Random(3)
    keys = [a[0] for a in reference_accounts()] + [random_private_key(rng) for _ in range(3)]
    accts = [records.Account.from_private_key(k) for k in keys]
    msgs = [rng.randbytes(32) for _ in keys]
    sigs = [a.sign(m, rng.randbytes(32)) for a, m in zip(accts, msgs)]
    n = len(keys)
    assert sg.verify_many(sigs, [a.address for a in accts], msgs, host=True).tolist() == [0] * n
    assert sg.verify_many([str(s) for s in sigs], [a.address_x for a in accts], msgs, host=True).tolist() == [0] * n
    assert all(a.verify(m, s) and a.verify(m, str(s)) for a, m, s in zip(accts, msgs, sigs))
    assert sg.verify_many(sigs, [a.address for a in accts], [rng.randbytes(32) for _ in keys], host=True).tolist() == [1] * n
    assert sg.verify_many(sigs, [a.address for a in accts[1:] + accts[:1]], msgs, host=True).tolist() == [1] * n
    assert sg.verify_many(sigs, accts[0].address, msgs, host=True).tolist() == [0] + [1] * (n - 1)      # one address for all
    for part in range(4):
        mixed = [s.bytes[:32 * part] + t.bytes[32 * part:32 * part + 32] + s.bytes[32 * part + 32:] for s, t in zip(sigs, sigs[1:] + sigs[:1])]
        assert sg.verify_many(np.frombuffer(b''.join(mixed), dtype=np.uint8).reshape(-1, 128), [a.address for a in accts], msgs, host=True).tolist() == [1] * n, part
    assert sg.verify_many([], accts[0].address, [], host=True).tolist() == [] and sg.verify_many([], accts[0].address, []).tolist() == []


# ---- 3: the cases: flags, edges, lengths --------------------------------------------------------------------------------------------------------------------
def small_x(want):
    """The smallest x > 1 that is `want`: 'off' the curve, or 'outside': on it with both points outside the prime-order subgroup."""
    for x in range(2, 400):
        y = P.fr_sqrt((1 + x * x) * pow((1 - D * x * x) % R, -1, R) % R)
        if want == 'off' and y is None: return x
        if want == 'outside' and y is not None and all(mul((x, yy), L) != (0, 1) for yy in (y, R - y)): return x
    return None


BLOCK_EDGE_BYTES = [126, 127, 378, 379, 630, 631]      # 4 | 5, 12 | 13, 20 | 21 fields: 8 + 4 + m elements fill 2 | 3, 3 | 4, 4 | 5 blocks of the rate-8 sponge
CHUNK_EDGE_BYTES = [0, 1, 31, 32, 63, 64]              # 0, 1, 1, 2, 2, 3 fields


@functools.lru_cache(maxsize=None)
def cases():
    """[(what, signature, address x, message, the flag wanted)]: at most one wave of them."""
    rng = random.Random(4)
    key, keys, ax = reference_accounts()[1]
    other_key, other, _ = reference_accounts()[2]
    m32 = rng.randbytes(32)
    good = sg.sign(key, m32, rng.randbytes(32)).bytes
    another = sg.sign(other_key, m32, rng.randbytes(32)).bytes
    part = lambda s, i, b: s[:32 * i] + b + s[32 * i + 32:]
    out = [('a valid signature', good, ax, m32, 0), ('another message', good, ax, m32[::-1], 1), ('another address', good, le32(other.ax), m32, 1)]
    for i, name in enumerate(('challenge', 'response', 'pk_sig', 'pr_sig')): out.append(('the %s of another signature' % name, part(good, i, another[32 * i:32 * i + 32]), ax, m32, 1))
    # no signature
    out.append(('challenge = the group order', part(good, 0, le32(L)), ax, m32, 3))
    out.append(('response = 2^256 - 1', part(good, 1, b'\xff' * 32), ax, m32, 3))
    out.append(('pk_sig.x = r', part(good, 2, le32(R)), ax, m32, 3))
    out.append(('pr_sig.x = r', part(good, 3, le32(R)), ax, m32, 3))
    out.append(('the address x = r', good, le32(R), m32, 3))
    out.append(('pk_sig.x on no curve point', part(good, 2, le32(small_x('off'))), ax, m32, 3))
    out.append(('pr_sig.x with both points outside the subgroup', part(good, 3, le32(small_x('outside'))), ax, m32, 3))
    out.append(('pk_sig.x with both points outside the subgroup', part(good, 2, le32(small_x('outside'))), ax, m32, 3))
    out.append(('a message one field over the cap', good, ax, bytes(CAP_BYTES + 1), 3))
    # the edges of the arithmetic
    out.append(('nonce 0: g_r is the identity', ref_sign(keys, m32, 0), ax, m32, 0))
    out.append(('nonce 1', ref_sign(keys, m32, 1), ax, m32, 0))
    out.append(('nonce l - 1', ref_sign(keys, m32, L - 1), ax, m32, 0))
    out.append(('response = 0: a forgery', part(good, 1, le32(0)), ax, m32, 1))
    out.append(('challenge = 0: a forgery', part(good, 0, le32(0)), ax, m32, 1))
    out.append(('challenge = l - 1, response = l - 1', part(part(good, 0, le32(L - 1)), 1, le32(L - 1)), ax, m32, 1))
    out.append(('pk_sig.x = 0: the identity', part(good, 2, le32(0)), ax, m32, 1))
    out.append(('pr_sig.x = 0: the identity', part(good, 3, le32(0)), ax, m32, 1))
    zero = Keys(0, 5)                                              # sk_sig = 0: pk_sig is the identity and the response is the nonce
    out.append(('an account with sk_sig = 0', ref_sign(zero, m32, 77), le32(zero.ax), m32, 0))
    for n in CHUNK_EDGE_BYTES + BLOCK_EDGE_BYTES:
        m = rng.randbytes(n)
        out.append(('a message of %d bytes' % n, sg.sign(key, m, rng.randbytes(32)).bytes, ax, m, 0))
        if n: out.append(('a message of %d bytes, its last bit changed' % n, out[-1][1], ax, m[:-1] + bytes([m[-1] ^ 0x80]), 1))
    m = rng.randbytes(CAP_BYTES)
    out.append(('a message of exactly the cap', sg.sign(key, m, rng.randbytes(32)).bytes, ax, m, 0))
    out.append(('a message of the cap, one bit changed in the middle', out[-1][1], ax, m[:70000] + bytes([m[70000] ^ 4]) + m[70001:], 1))
    assert len(out) <= 64
    return out


def test_the_chosen_lengths_straddle_the_boundaries_they_are_chosen_for():
    """poseidon.hpp's absorb: the preimage [domain, count, 0 x 6 | g_r.x, pk_sig.x, pr_sig.x, address.x | m fields] enters eight elements to a permutation."""
    nf = lambda n: len(fields_of(bytes(n)))
    assert [nf(n) for n in CHUNK_EDGE_BYTES] == [0, 1, 1, 2, 2, 3]
    blocks = lambda n: (8 + 4 + nf(n) + 7) // 8
    assert [blocks(n) for n in BLOCK_EDGE_BYTES] == [2, 3, 3, 4, 4, 5]
    assert nf(CAP_BYTES) == MAX_FIELDS and nf(CAP_BYTES + 1) == MAX_FIELDS + 1 and sg.MAX_MESSAGE_BYTES == CAP_BYTES
    assert small_x('off') is not None and small_x('outside') is not None


def test_every_case_has_the_flag_wanted_on_the_host_path_and_in_the_restatement():
    for what, s, ax, m, want in cases():
        assert host_flag(s, ax, m) == want, what
        if len(m) <= 1024: assert ref_verify(s, num(ax), m) == want, what
    what, s, ax, m, want = [c for c in cases() if c[0] == 'a message of exactly the cap'][0]
    assert ref_verify(s, num(ax), m) == 0                          # the restatement hashes all 4161 fields once
    rc, flags = verify_raw([c[1] for c in cases()], [c[2] for c in cases()], [c[3] for c in cases()])
    assert rc == 0 and flags == [c[4] for c in cases()]


def test_what_the_calls_refuse():
    key, keys, ax = reference_accounts()[0]
    s = sg.sign(key, b'abc', bytes(32)).bytes
    assert verify_raw([s, s], [ax], [b'abc', b'abc'], offsets=[0, 3, 2])[0] == 2 and b'offsets decrease' in aleo_amd.lib().aleo_mi355x_last_error()
    assert verify_raw([s, s], [ax], [b'abc', b'abc'], offsets=[1, 3, 6])[0] == 2
    assert verify_raw([s, s], [ax, ax], [b'abc', b'abc'], stride=16)[0] == 2
    assert verify_raw([s, s], [ax], [b'abc', b'abc']) == (0, [0, 0])
    with pytest.raises(aleo_amd.AleoMi355xError): sg.sign(key, bytes(CAP_BYTES + 1), bytes(32))
    with pytest.raises(aleo_amd.AleoMi355xError): sg.sign('APrivateKey1nonsense', b'abc', bytes(32))
    assert sg.sign(key, bytes(CAP_BYTES), bytes(32)).verify(ax, bytes(CAP_BYTES))
    with pytest.raises(ValueError): sg.sign(key, b'abc', bytes(31))
    with pytest.raises(ValueError): records.Account(None, b'', b'', ax).sign(b'abc')


# ---- 4: strings -----------------------------------------------------------------------------------------------------------------------------------------------
def test_strings_round_trip_and_refuse_what_is_no_signature():
    from aleo_amd import wire
    key, keys, ax = reference_accounts()[0]
    s = sg.sign(key, b'hello', bytes(32))
    text = str(s)
    assert text.startswith('sign1') and len(text) == 5 + 205 + 6 and sg.Signature.from_string(text) == s and sg.Signature.from_string(text).bytes == s.bytes
    assert wire.bech32m_decode(text) == ('sign', s.bytes)
    flipped = text[:40] + ('q' if text[40] != 'q' else 'p') + text[41:]
    for bad in (flipped, ACC[0]['address'], wire.bech32m_encode('sign', s.bytes[:127]), wire.bech32m_encode('sign', s.bytes + b'\0'), wire.bech32m_encode('sigm', s.bytes), '', 'sign1'):
        with pytest.raises(aleo_amd.AleoMi355xError): sg.Signature.from_string(bad)
    with pytest.raises(ValueError): sg.Signature(s.bytes[:127])


# ---- 5: the device lane on the CPU ------------------------------------------------------------------------------------------------------------------------------
def case_file(path, rows):
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(rows)))
        for s, ax, m, want in rows: f.write(s + ax + struct.pack('<I', len(m)) + m + bytes([want]))


def lane_rows():
    """The cases, with the flags the library's host path gives them, and sixty random signatures of which a third are spoiled."""
    rows = [(s, ax, m, want) for _, s, ax, m, want in cases()]
    sigs, addrs, msgs = mixed_batch(60, per_signature=True)
    rc, flags = verify_raw(sigs, addrs, msgs)
    assert rc == 0 and set(flags) == {0, 1, 3}
    return rows + list(zip(sigs, addrs, msgs, flags))


@pytest.mark.parametrize('sanitized', [False, True], ids=['plain', 'sanitizers'])
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path, sanitized):
    """tests/cpp/signature_lane_emul.cpp: signature_lane.h compiled for the CPU over the checked restatement of fr29.h, once plain and once with the address and
    undefined-behaviour sanitizers compiled into that program, run as a program of its own on every case above.  (-fno-strict-aliasing: host_field.hpp reads
    its uint64_t limbs through unsigned long long pointers for the carry-chain intrinsics, which g++ at -O2 may reorder; the library is built by clang.)"""
    data = os.path.join(str(tmp_path), 'cases.bin')
    rows = lane_rows(); case_file(data, rows)
    r = bs.run_lane_emul(tmp_path, 'signature_lane_emul', [data], sanitized=sanitized)
    print(r.stdout)
    assert r.returncode == 0 and '%d signatures' % len(rows) in r.stdout and ' 0 mismatches, 0 reads past an end, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr


# ---- 6: the threshold, the code object, the C++ mirror ----------------------------------------------------------------------------------------------------------
DEFAULT_MIN_SIGNATURES = 32


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_signatures', 'ALEO_MI355X_MIN_SIGNATURES') == (DEFAULT_MIN_SIGNATURES, 5, DEFAULT_MIN_SIGNATURES)
    # below the threshold the call computes on the host: no device is needed for it
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_SIGNATURES='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    code = ('from aleo_amd import signature as sg; k = %r; s = sg.sign(k, b"m", bytes(32)); from aleo_amd import records; '
            'print(sg.verify_many([s, s], records.Account.from_private_key(k).address, [b"m", b"n"]).tolist())' % ACC[0]['private_key'])
    assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300).stdout.split() == ['[0,', '1]']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_signature_kernel_code_object_is_gfx950_and_has_no_scratch():
    assert bs.scratch_and_spills('signatures', ['k_signatures_verify']) == (1, {'k_signatures_verify': (0, 0, 0)})      # this one and no other


def run_cpp_mirror(tmp_path, env, n):
    """tests/cpp/signature_test.cpp: Signature, sign, verify, verify_many and the account's methods of include/aleo_mi355x.hpp."""
    r = bs.run_cpp_mirror(tmp_path, 'signature_test', [ACC[0]['private_key'], ACC[0]['address'], n], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_SIGNATURES': '1000000'}, 12)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_SIGNATURES', '0')
    monkeypatch.delenv('ALEO_MI355X_SIGNATURES_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_signatures()) == 0
    return monkeypatch


@functools.lru_cache(maxsize=None)
def pool():
    """Four accounts (the reference's three and one more) and 24 valid signatures of each over messages of 0 to 70 bytes: what the batches are drawn from."""
    rng = random.Random(5)
    keys = [a[0] for a in reference_accounts()] + [random_private_key(rng)]
    accts = [records.Account.from_private_key(k) for k in keys]
    out = []
    for a in accts:
        for j in range(24):
            m = rng.randbytes(rng.choice([0, 1, 31, 32, 32, 32, 33, 64, 70]))
            out.append((a.sign(m, rng.randbytes(32)).bytes, a.address_x, m))
    return accts, out


def mixed_batch(n, per_signature, seed=6):
    """n signatures, valid, invalid and malformed mixed: under the first account's address alone (so three quarters fail for that already), or each under its own."""
    rng = random.Random(seed * 1000 + n)
    accts, valid = pool()
    sigs, addrs, msgs = [], [], []
    for i in range(n):
        s, ax, m = valid[rng.randrange(len(valid))]
        kind = rng.randrange(6)
        if kind == 1: m = m + b'!'
        if kind == 2: s = s[:32] + le32((num(s[32:64]) + 1) % L) + s[64:]
        if kind == 3: s = s[:64] + le32(R + rng.randrange(5)) + s[96:]
        if kind == 4: s = le32(L + rng.randrange(1 << 200)) + s[32:]
        if kind == 5 and per_signature: ax = accts[rng.randrange(4)].address_x
        sigs.append(s); addrs.append(ax); msgs.append(m)
    return sigs, (addrs if per_signature else [accts[0].address_x]), msgs


@pytest.mark.gpu
@pytest.mark.parametrize('per_signature', [False, True], ids=['one address', 'an address each'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_gpu_flags_equal_the_host_path_at_wave_and_block_edges(on_kernel, n, per_signature):
    sigs, addrs, msgs = mixed_batch(n, per_signature)
    host = verify_raw(sigs, addrs, msgs, host=True, stride=32 if per_signature else 0)
    got = verify_raw(sigs, addrs, msgs, host=False, stride=32 if per_signature else 0)
    assert host[0] == 0 and got == host
    if n >= 63: assert set(host[1]) == {0, 1, 3}


@pytest.mark.gpu
def test_gpu_one_wave_of_every_edge_case_at_once(on_kernel):
    """Messages from 0 bytes to the cap in one wave: the divergent loops, the idling of the lanes with flag 3 and the streaming absorb."""
    c = cases()
    got = verify_raw([x[1] for x in c], [x[2] for x in c], [x[3] for x in c], host=False)
    assert got == (0, [x[4] for x in c]), [x[0] for x, f in zip(c, got[1]) if f != x[4]]


@pytest.mark.gpu
def test_gpu_both_sides_of_the_threshold_and_chunked_launches_return_the_same_bytes(monkeypatch):
    sigs, addrs, msgs = mixed_batch(40, True)
    host = verify_raw(sigs, addrs, msgs, host=True)
    monkeypatch.setenv('ALEO_MI355X_MIN_SIGNATURES', '41'); assert verify_raw(sigs, addrs, msgs, host=False) == host      # below: the host code inside the call
    monkeypatch.setenv('ALEO_MI355X_MIN_SIGNATURES', '40'); assert verify_raw(sigs, addrs, msgs, host=False) == host      # at it: the kernel
    monkeypatch.setenv('ALEO_MI355X_SIGNATURES_CHUNK', '7'); assert verify_raw(sigs, addrs, msgs, host=False) == host     # six launches
    assert sg.verify_many(np.frombuffer(b''.join(sigs), dtype=np.uint8).reshape(-1, 128), addrs, msgs).tolist() == host[1]      # the Python mirror on the kernel


@pytest.mark.gpu
def test_gpu_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    batches = [mixed_batch(130, True, seed=7), mixed_batch(90, False, seed=8)]
    want = [verify_raw(*b, host=True) for b in batches]
    assert bs.two_threads(lambda i: verify_raw(*batches[i], host=False)) == want


@pytest.mark.gpu
def test_gpu_cpp_mirror_on_the_kernel(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_SIGNATURES': '0'}, 70)
