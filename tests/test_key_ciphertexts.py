"""Private key ciphertexts (aleo_mi355x_private_key_encrypt, _private_key_decrypt, _private_keys_open[_host], _min_key_ciphertexts; aleo_amd/key_ciphertext.py; the
same in include/aleo_mi355x.hpp).

What the reference's data pins comes first: its one private key, secret, ciphertext and corrupted ciphertext, decrypted and — under the nonce recovered from that
ciphertext — encrypted byte for byte.  Then encryption against the restatement in Python integers (tests/key_ciphertext_ref.py), opened again by the oracle's own
decryption, at the edges of the secret's length, of the seed and of the nonce; the batched opening on the host path over one batch that holds every case; the
threshold; the code object.  The host path, byte for byte, checks the device lane: emulated on the CPU, plain and under the sanitizers, here, and on the GPU in the
second half (ALEO_MI355X_MIN_KEY_CIPHERTEXTS=0).  No test reads the reference tree."""
import ctypes, functools, json, os, random, struct, subprocess, sys
import numpy as np
import pytest
import aleo_amd
from aleo_amd import account as acct, key_ciphertext as kc, records
from oracle import poseidon as ps
from oracle import pyref as P
import key_ciphertext_ref as ref
import batch_support as bs
from batch_support import HERE, ROOT, HIPCC, le32, num, _p, _vp

GOLD = json.load(open(os.path.join(HERE, 'golden', 'reference_account.json')))
ACC, KAT = GOLD['accounts'], GOLD['ciphertext_kat']
RECORD = json.load(open(os.path.join(HERE, 'golden', 'reference_records.json')))['records']['owner']
R = ps.R
SECRET_LENGTHS = (0, 1, 31, 32, 33, 62, 63, 100)
OUTPUTS = ('seeds', 'sk', 'vk', 'ax', 'str', 'flags')
NULL_SUBSETS = (('vk', 'ax', 'flags'), ('str',), ('sk', 'flags'), (), ('seeds',), ('seeds', 'flags'), ('flags',))      # test_accounts' subsets, and the seeds alone


def raw(s) -> bytes: return s.encode() if isinstance(s, str) else bytes(s)


# ---- through the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def blob(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if items: off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64)
    return b''.join(items), off


def open_raw(pairs, host=True, want=OUTPUTS):
    """aleo_mi355x_private_keys_open[_host] on (ciphertext, secret) pairs: (status, {name: bytes}); the outputs not in `want` are passed as NULL."""
    n = len(pairs)
    text, off = blob([raw(c) for c, _ in pairs]); sec, soff = blob([raw(s) for _, s in pairs])
    out = {k: np.full((n, 63 if k == 'str' else 32), 9, np.uint8) for k in OUTPUTS[:-1]}; out['flags'] = np.full(n, 9, np.uint8)
    L_ = aleo_amd.lib(); call = L_.aleo_mi355x_private_keys_open_host if host else L_.aleo_mi355x_private_keys_open
    rc = call(_vp(text), _p(off), _vp(sec), _p(soff), n, *[_p(out[k]) if k in want else None for k in OUTPUTS])
    return rc, {k: out[k].tobytes() for k in want}


def nonce_of_the_reference_ciphertext() -> int:
    kind, members = ps.decrypt_symmetric(KAT['ciphertext'], ps.domain_separator(KAT['secret']))
    return members['nonce'][2]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------
def secret_of_length(n: int, rng) -> bytes:
    """n bytes, the first and the last of them at least 0x80 (no UTF-8 text, and a number of n whole bytes)."""
    b = bytearray(rng.randrange(256) for _ in range(n))
    if n: b[0] |= 0x80; b[-1] |= 0x80
    return bytes(b)


@functools.lru_cache(maxsize=None)
def good_cases():
    """[(ciphertext, secret, seed)] by the restatement: the reference's three accounts, a secret of every length, the edges of the seed and of the nonce."""
    rng = random.Random(41)
    out = [(KAT['ciphertext'], raw(KAT['secret']), ps.private_key_seed(KAT['private_key']))]
    for i, a in enumerate(ACC):
        seed = ps.private_key_seed(a['private_key']); secret = ('pass word %d' % i).encode()
        out.append((ref.encrypt(seed, secret, rng.randrange(R)), secret, seed))
    for n in SECRET_LENGTHS:
        seed, secret = rng.randrange(R), secret_of_length(n, rng)
        out.append((ref.encrypt(seed, secret, rng.randrange(R)), secret, seed))
    for seed in (0, 1, R - 1):
        for nonce in (0, R - 1):
            out.append((ref.encrypt(seed, b'edge', nonce), b'edge', seed))
    return out


@functools.lru_cache(maxsize=None)
def flagged_cases():
    """[(what, ciphertext, secret, flag)]: everything that must not open."""
    rng = random.Random(42)
    key, nonce, sec = rng.randrange(R), rng.randrange(R), b'crafted'
    good = ref.key_plaintext_bits(key, nonce)
    lit = ref.literal_field_bits
    def with_bits(at, n, v): b = list(good); b[at:at + n] = ref.bits_le(v, n); return b
    upper = KAT['ciphertext'][:20] + KAT['ciphertext'][20:].replace('q', 'Q', 1)
    padded = ref.fields_of_bits(good); padded[2] |= 1 << (700 - 2 * ref.DATA_BITS)
    big = [rng.randrange(R), R, rng.randrange(R)]
    out = [
        ('a wrong secret', KAT['ciphertext'], raw(KAT['wrong_secret']), 1),
        ('the reference\'s corrupted ciphertext', KAT['bad_ciphertext'], raw(KAT['secret']), 3),
        ('a record string', RECORD, raw(KAT['secret']), 3),
        ('the empty string', '', raw(KAT['secret']), 3),
        ('an upper-case character', upper, raw(KAT['secret']), 3),
        ('the prefix alone', 'ciphertext1', sec, 3),
        ('a valid ciphertext of two fields', ref.encrypt_fields([rng.randrange(R), rng.randrange(R)], sec), sec, 1),
        ('a valid ciphertext of four fields', ref.encrypt_fields([rng.randrange(R) for _ in range(4)], sec), sec, 1),
        ('a valid ciphertext of no field', ref.ciphertext_string([]), sec, 1),
        ('a field element not below r', P.bech32m_encode('ciphertext', (3).to_bytes(2, 'little') + b''.join(le32(v) for v in big)), sec, 3),
        ('a count that does not match the payload', P.bech32m_encode('ciphertext', (4).to_bytes(2, 'little') + b''.join(le32(v % R) for v in big)), sec, 3),
        ('one trailing byte', P.bech32m_encode('ciphertext', (3).to_bytes(2, 'little') + b''.join(le32(v % R) for v in big) + b'\0'), sec, 3),
        ('members swapped', ref.encrypt_bits(ref.struct_bits([('nonce', lit(nonce)), ('key', lit(key))]), sec), sec, 1),
        ('member count 3', ref.encrypt_bits(with_bits(2, 8, 3), sec), sec, 1),
        ('literal type 3', ref.encrypt_bits(with_bits(60, 8, 3), sec), sec, 1),
        ('key not below r', ref.encrypt_bits(ref.key_plaintext_bits(R, nonce), sec), sec, 1),
        ('nonce not below r', ref.encrypt_bits(ref.key_plaintext_bits(key, R + 1), sec), sec, 1),
        ('terminus missing', ref.encrypt_bits(good, sec, terminus=False, n_fields=3), sec, 1),
        ('one padding bit set', ref.encrypt_fields(padded, sec), sec, 1),
        ('bit 680 moved', ref.encrypt_bits(good + [0], sec), sec, 1),
    ]
    assert ref.encrypt_bits(good, sec) == ref.encrypt(key * pow(ref.blinding(nonce, ref.sep(sec)), -1, R) % R, sec, nonce)      # the crafting itself is the restatement's
    return out


@functools.lru_cache(maxsize=None)
def edge_batch():
    """[(ciphertext, secret, flag, seed bytes)]: every case above, good and flagged interleaved, at most one wave of them."""
    good = [(c, s, 0, le32(seed)) for c, s, seed in good_cases()]; bad = [(c, s, flag, bytes(32)) for _, c, s, flag in flagged_cases()]
    out = []
    while good or bad:
        if good: out.append(good.pop(0))
        if bad: out.append(bad.pop(0))
    assert len(out) <= 64
    return out


@functools.lru_cache(maxsize=None)
def mixed_pairs(n, seed=7):
    """n pairs; from 63 up about one in eight with a wrong secret and one in eight a broken string."""
    rng = random.Random(seed * 1000 + n)
    base = [(c, s) for c, s, _ in good_cases()]
    out = []
    for i in range(n):
        c, s = base[rng.randrange(len(base))]
        if n >= 63 and i % 8 == 3: s = s + b'!'
        if n >= 63 and i % 8 == 6: at = rng.randrange(11, len(c)); c = c[:at] + ('q' if c[at] != 'q' else 'p') + c[at + 1:]
        out.append((c, s))
    return out


# ---- 1: what the reference's data pins -------------------------------------------------------------------------------------------------------------------------
def test_the_reference_known_answer_decrypts_and_encrypts_byte_for_byte():
    assert kc.decrypt(KAT['ciphertext'], KAT['secret']) == KAT['private_key']
    with pytest.raises(aleo_amd.AleoMi355xError) as e: kc.decrypt(KAT['ciphertext'], 'badpassword')
    assert e.value.status == 7 and isinstance(e.value, records.NotOwner)
    with pytest.raises(aleo_amd.AleoMi355xError) as e: kc.decrypt(KAT['bad_ciphertext'], KAT['secret'])
    assert e.value.status == 2
    nonce = nonce_of_the_reference_ciphertext()
    assert kc.encrypt(KAT['private_key'], KAT['secret'], nonce) == KAT['ciphertext'] and len(KAT['ciphertext']) == kc.CHARS
    assert ref.encrypt(ps.private_key_seed(KAT['private_key']), KAT['secret'], nonce) == KAT['ciphertext']      # the restatement is pinned by the same string
    a = records.Account.from_ciphertext(KAT['ciphertext'], KAT['secret'])
    assert a.private_key == KAT['private_key'] and a.to_ciphertext(KAT['secret'], nonce) == KAT['ciphertext']


# ---- 2: against the restatement ------------------------------------------------------------------------------------------------------------------------------------
def test_encrypt_equals_the_restatement_and_the_oracle_opens_it():
    rng = random.Random(5)
    triples = [(rng.randrange(R), bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40))), rng.randrange(R)) for _ in range(32)]
    triples += [(rng.randrange(R), secret_of_length(n, rng), rng.randrange(R)) for n in SECRET_LENGTHS]
    triples += [(rng.randrange(R), ('pässwörd' * k).encode(), rng.randrange(R)) for k in (1, 4, 13)]      # 10, 40 and 130 bytes of UTF-8
    triples += [(seed, b'edge', nonce) for seed in (0, 1, R - 1) for nonce in (0, R - 1)]
    through_the_oracle = 0
    for seed, secret, nonce in triples:
        key = ps.private_key_string(seed)
        text = kc.encrypt(key, secret, nonce)
        assert text == ref.encrypt(seed, secret, nonce) and len(text) == kc.CHARS, (seed, secret, nonce)
        assert kc.decrypt(text, secret) == key
        try: as_text = secret.decode()
        except UnicodeDecodeError: continue
        assert ps.decrypt_private_key(text, as_text) == key
        through_the_oracle += 1
    assert through_the_oracle >= 8


def test_the_reference_s_round_trip_properties():
    """private_key_ciphertext.rs:131-231: different nonces give different strings and the same key; a wrong secret fails; a drawn nonce is a field element."""
    key = ACC[0]['private_key']
    one, two = kc.encrypt(key, 'mypassword'), kc.encrypt(key, 'mypassword')
    assert one != two and kc.decrypt(one, 'mypassword') == kc.decrypt(two, 'mypassword') == key
    assert kc.encrypt(key, 'mypassword', 7) == kc.encrypt(key, 'mypassword', le32(7)) != kc.encrypt(key, 'mypassword', 8)
    for wrong in ('badpassword', '', 'mypassword ', b'\0mypassword'):
        with pytest.raises(records.NotOwner): kc.decrypt(one, wrong)
    assert kc.decrypt(one, b'mypassword\0') == key              # a secret is a little-endian number: zero bytes at its end do not change it (upstream's separator alike)
    assert num(kc.random_nonce()) < R and kc.random_nonce() != kc.random_nonce()
    a = records.Account.from_private_key(key)
    b = records.Account.from_ciphertext(a.to_ciphertext('s3cret'), 's3cret')
    assert (b.private_key, b.sk_sig, b.view_key, b.address_x) == (a.private_key, a.sk_sig, a.view_key, a.address_x)


def test_encrypt_and_decrypt_refuse_what_they_should():
    L_ = aleo_amd.lib(); out = ctypes.create_string_buffer(200)
    key = ACC[0]['private_key'].encode()
    assert L_.aleo_mi355x_private_key_encrypt(out, 175, key, _vp(b'pw'), 2, _vp(le32(5))) == 0 and len(out.value) == 174
    assert L_.aleo_mi355x_private_key_encrypt(out, 174, key, _vp(b'pw'), 2, _vp(le32(5))) == 2                      # one short
    for nonce in (R, R + 1, (1 << 256) - 1): assert L_.aleo_mi355x_private_key_encrypt(out, 200, key, _vp(b'pw'), 2, _vp(le32(nonce))) == 2
    for bad in (b'', b'APrivateKey1nonsense', ACC[0]['view_key'].encode(), key[:-1], ps.base58_encode(ps.PRIVATE_KEY_PREFIX + le32(R)).encode()):
        assert L_.aleo_mi355x_private_key_encrypt(out, 200, bad, _vp(b'pw'), 2, _vp(le32(5))) == 2, bad
    assert L_.aleo_mi355x_private_key_encrypt(None, 200, key, _vp(b'pw'), 2, _vp(le32(5))) == 2
    assert L_.aleo_mi355x_private_key_encrypt(out, 200, key, None, 2, _vp(le32(5))) == 2 and L_.aleo_mi355x_private_key_encrypt(out, 200, key, None, 0, _vp(le32(5))) == 0
    text = out.value
    assert L_.aleo_mi355x_private_key_decrypt(out, 200, text, None, 0) == 0 and out.value == key                    # the empty secret is a secret
    assert L_.aleo_mi355x_private_key_decrypt(out, 59, text, None, 0) == 2                                           # 59 characters and their terminator need 60
    assert L_.aleo_mi355x_private_key_decrypt(out, 200, None, None, 0) == 2
    for what, c, s, flag in flagged_cases():
        assert L_.aleo_mi355x_private_key_decrypt(out, 200, raw(c), _vp(s), len(s)) == (7 if flag == 1 else 2), what


def test_last_error_names_no_secret_and_no_key():
    L_ = aleo_amd.lib(); out = ctypes.create_string_buffer(200)
    secret = b'a-very-recognisable-secret'
    text = kc.encrypt(ACC[1]['private_key'], secret, 3)
    def clean(msg):
        assert msg.startswith('private_key_decrypt') and 'secret' not in msg.replace('this secret', '') and secret.decode() not in msg
        assert 'APrivateKey1' not in msg and ACC[1]['private_key'] not in msg and text not in msg and text[11:40] not in msg
    assert L_.aleo_mi355x_private_key_decrypt(out, 200, text.encode(), _vp(secret + b'x'), len(secret) + 1) == 7
    clean(L_.aleo_mi355x_last_error().decode())
    assert L_.aleo_mi355x_private_key_decrypt(out, 10, text.encode(), _vp(secret), len(secret)) == 2              # it decrypts, and the buffer is too small
    clean(L_.aleo_mi355x_last_error().decode())
    assert L_.aleo_mi355x_private_key_decrypt(out, 200, text[:-1].encode(), _vp(secret), len(secret)) == 2
    clean(L_.aleo_mi355x_last_error().decode())
    assert L_.aleo_mi355x_private_key_encrypt(out, 200, ACC[1]['private_key'].encode(), _vp(secret), len(secret), _vp(le32(R))) == 2
    msg = L_.aleo_mi355x_last_error().decode()
    assert 'APrivateKey1' not in msg and secret.decode() not in msg


# ---- 3: the batched opening on the host path ---------------------------------------------------------------------------------------------------------------------
def test_open_host_on_one_batch_of_every_case():
    batch = edge_batch()
    rc, out = open_raw([(c, s) for c, s, _, _ in batch])
    assert rc == 0
    names = {c: what for what, c, _, _ in flagged_cases()}
    for i, (c, s, flag, seed) in enumerate(batch):
        rows = tuple(out[k][32 * i:32 * i + 32] for k in ('seeds', 'sk', 'vk', 'ax'))
        assert out['flags'][i] == flag, names.get(c, 'a good pair')
        if flag:
            assert rows == (bytes(32),) * 4 and out['str'][63 * i:63 * i + 63] == bytes(63), names[c]
            continue
        a = records.Account.from_private_key(ps.private_key_string(num(seed)))
        assert rows == (seed, a.sk_sig, a.view_key, a.address_x) and out['str'][63 * i:63 * i + 63].decode() == a.address, i
    # the reference's three accounts, encrypted by the restatement: their view keys and addresses
    opened = kc.accounts_from_ciphertexts([(c, s) for c, s, _ in good_cases()[1:4]], host=True)
    assert [(a.private_key, a.view_key_string, a.address) for a in opened] == [(a['private_key'], a['view_key'], a['address']) for a in ACC]
    # the Python mirror returns the same bytes, and None where a pair does not open
    seeds, sk, vk, ax, flags, text = kc.open_many([c for c, _, _, _ in batch], [s for _, s, _, _ in batch], strings=True, host=True)
    assert (seeds.tobytes(), sk.tobytes(), vk.tobytes(), ax.tobytes(), flags.tobytes()) == tuple(out[k] for k in ('seeds', 'sk', 'vk', 'ax', 'flags'))
    assert ''.join(text).encode() == out['str'].replace(b'\0', b'')
    got = kc.accounts_from_ciphertexts([(c, s) for c, s, _, _ in batch], host=True)
    assert [g is None for g in got] == [flag != 0 for _, _, flag, _ in batch]
    assert all(g.private_key == ps.private_key_string(num(seed)) for g, (_, _, flag, seed) in zip(got, batch) if not flag)
    # some outputs NULL: the others are the same bytes
    for want in NULL_SUBSETS:
        assert open_raw([(c, s) for c, s, _, _ in batch], want=want) == (0, {k: out[k] for k in want}), want


def test_open_accepts_no_pair_and_refuses_bad_arguments():
    L_ = aleo_amd.lib()
    assert open_raw([]) [0] == 0
    for call in (L_.aleo_mi355x_private_keys_open_host, L_.aleo_mi355x_private_keys_open):
        assert call(None, None, None, None, 0, None, None, None, None, None, None) == 0
        text, off = blob([KAT['ciphertext'].encode()] * 2); sec, soff = blob([b'mypassword', b''])
        flags = np.zeros(2, np.uint8)
        args = lambda t=_vp(text), o=off, s=_vp(sec), so=soff: (t, _p(o), s, _p(so), 2, None, None, None, None, None, _p(flags))
        assert call(*args()) == 0 and flags.tolist() == [0, 1]
        assert call(*args(t=None)) == 2 and call(*args(o=None)) == 2 and call(*args(s=None)) == 2 and call(*args(so=None)) == 2
        assert b'private_keys_open' in L_.aleo_mi355x_last_error()
        for which in ('o', 'so'):
            moved = (off if which == 'o' else soff).copy(); moved[0] = 1
            assert call(*args(**{which: moved})) == 2                                       # does not start at 0
            down = (off if which == 'o' else soff).copy(); down[1] = down[2] + 1
            assert call(*args(**{which: down})) == 2                                        # decreases
    with pytest.raises(ValueError): kc.open_many([KAT['ciphertext']], [], host=True)


# ---- 4: the device lane on the CPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sanitized', [False, True], ids=['plain', 'sanitizers'])
def test_device_lane_code_emulated_on_the_host_matches_the_host_path(tmp_path, sanitized):
    """tests/cpp/key_ciphertext_lane_emul.cpp: key_ciphertext_lane.h compiled for the CPU over the checked restatement of fr29.h, once plain and once with the
    address and undefined-behaviour sanitizers compiled into that program, run as a program of its own.  (-fno-strict-aliasing: as for account_lane_emul.)"""
    data = os.path.join(str(tmp_path), 'cases.bin')
    pairs = [(c, s) for c, s, _, _ in edge_batch()] + list(mixed_pairs(65))
    rc, out = open_raw(pairs, want=('seeds', 'flags'))
    assert rc == 0
    with open(data, 'wb') as f:
        f.write(struct.pack('<I', len(pairs)))
        for i, (c, s) in enumerate(pairs): f.write(struct.pack('<I', len(raw(c))) + raw(c) + struct.pack('<I', len(s)) + s + out['flags'][i:i + 1] + out['seeds'][32 * i:32 * i + 32])
    r = bs.run_lane_emul(tmp_path, 'key_ciphertext_lane_emul', [data], sanitized=sanitized)
    print(r.stdout)
    assert r.returncode == 0 and '%d pairs' % len(pairs) in r.stdout, r.stdout + r.stderr
    assert ' 0 mismatches, 0 reads past an end, 0 limb-rule violations' in r.stdout, r.stdout + r.stderr
    assert ' 0 opened' not in r.stdout and ' 0 not decrypted' not in r.stdout and ' 0 no ciphertext' not in r.stdout


# ---- 5: the threshold, the code object, the C++ mirror -------------------------------------------------------------------------------------------------------------
DEFAULT_MIN_KEY_CIPHERTEXTS = 64


def test_routing_threshold_and_its_environment_override():
    assert bs.threshold_reads('min_key_ciphertexts', 'ALEO_MI355X_MIN_KEY_CIPHERTEXTS') == (DEFAULT_MIN_KEY_CIPHERTEXTS, 5, DEFAULT_MIN_KEY_CIPHERTEXTS)
    # below the threshold the call computes on the host: no device is needed for it
    env = dict(os.environ, PYTHONPATH=ROOT, ALEO_MI355X_MIN_KEY_CIPHERTEXTS='1000000', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
    code = 'from aleo_amd import key_ciphertext as k; c = %r; print([a and a.private_key for a in k.accounts_from_ciphertexts([(c, "mypassword"), (c, "x")])])' % KAT['ciphertext']
    assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300).stdout.strip() == repr([KAT['private_key'], None])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_key_ciphertext_kernel_code_object_is_gfx950_and_has_no_scratch_and_no_spills():
    import code_object as co
    assert bs.scratch_and_spills('key_ciphertexts', ['k_key_ciphertexts_open']) == (1, {'k_key_ciphertexts_open': (0, 0, 0)})      # this one and no other: the account kernel is accounts.hip's
    asm, blocks = co.compile_unit('accounts')
    assert len(blocks) == 2 and all(len([b for b in blocks if k in b]) == 1 for k in ('k_accounts_derive', 'k_accounts_search'))


def run_cpp_mirror(tmp_path, env, n):
    """tests/cpp/key_ciphertexts_test.cpp: encrypt_private_key, decrypt_private_key, open_private_keys and the two PrivateAccount methods of include/aleo_mi355x.hpp."""
    r = bs.run_cpp_mirror(tmp_path, 'key_ciphertexts_test', [KAT['private_key'], KAT['secret'], KAT['ciphertext'], KAT['bad_ciphertext'], n], env)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_on_the_host_path(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_KEY_CIPHERTEXTS': '1000000'}, 12)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_kernel(monkeypatch):
    monkeypatch.setenv('ALEO_MI355X_MIN_KEY_CIPHERTEXTS', '0')
    monkeypatch.setenv('ALEO_MI355X_MIN_ACCOUNTS', '0')
    monkeypatch.delenv('ALEO_MI355X_ACCOUNTS_CHUNK', raising=False)
    assert int(aleo_amd.lib().aleo_mi355x_min_key_ciphertexts()) == 0
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_gpu_open_equals_the_host_path_at_wave_and_block_edges(on_kernel, n):
    pairs = list(mixed_pairs(n))
    host = open_raw(pairs, host=True)
    got = open_raw(pairs, host=False)
    assert host[0] == 0 and got == host
    if n >= 63: assert set(host[1]['flags']) == {0, 1, 3}
    if n == 65:                                                 # some outputs NULL: the others are the same bytes
        for want in NULL_SUBSETS:
            part = open_raw(pairs, host=False, want=want)
            assert part == (0, {k: host[1][k] for k in want}) and open_raw(pairs, host=True, want=want) == part


@pytest.mark.gpu
def test_gpu_one_wave_of_every_edge_case_and_every_secret_length_at_once(on_kernel):
    pairs = [(c, s) for c, s, _, _ in edge_batch()]
    host = open_raw(pairs, host=True)
    assert open_raw(pairs, host=False) == host and list(host[1]['flags']) == [flag for _, _, flag, _ in edge_batch()]
    assert {len(s) for _, s, flag, _ in edge_batch() if not flag} >= set(SECRET_LENGTHS)
    long_text = [('ciphertext1' + 'q' * 300, b'x')] * 64 + pairs[:6]                     # a block whose span does not fit the staging buffer: read from global memory
    assert open_raw(long_text, host=False) == open_raw(long_text, host=True)


@pytest.mark.gpu
def test_gpu_both_sides_of_the_threshold_and_chunked_launches_return_the_same_bytes(monkeypatch):
    pairs = list(mixed_pairs(40, seed=9))
    pairs[5] = (pairs[5][0], pairs[5][1] + b'?'); pairs[11] = ('ciphertext1qqqqqq', b'')
    host = open_raw(pairs, host=True)
    assert set(host[1]['flags']) == {0, 1, 3}
    monkeypatch.setenv('ALEO_MI355X_MIN_KEY_CIPHERTEXTS', '41'); assert open_raw(pairs, host=False) == host      # below: the host code inside the call
    monkeypatch.setenv('ALEO_MI355X_MIN_KEY_CIPHERTEXTS', '40'); assert open_raw(pairs, host=False) == host      # at it: the kernels
    monkeypatch.setenv('ALEO_MI355X_ACCOUNTS_CHUNK', '7'); assert open_raw(pairs, host=False) == host             # six launches
    seeds, sk, vk, ax, flags, text = kc.open_many([c for c, _ in pairs], [s for _, s in pairs], strings=True)       # the Python mirror on the kernels
    assert (seeds.tobytes(), sk.tobytes(), vk.tobytes(), ax.tobytes(), flags.tobytes()) == tuple(host[1][k] for k in ('seeds', 'sk', 'vk', 'ax', 'flags'))
    assert ''.join(text).encode() == host[1]['str'].replace(b'\0', b'')
    key = lambda a: a and (a.private_key, a.sk_sig, a.view_key, a.address_x)
    assert [key(a) for a in kc.accounts_from_ciphertexts(pairs)] == [key(a) for a in kc.accounts_from_ciphertexts(pairs, host=True)]


@pytest.mark.gpu
def test_gpu_two_threads_at_once_get_the_host_path_s_bytes(on_kernel):
    pairs = list(mixed_pairs(130, seed=8))
    rng = random.Random(3); seeds = [le32(rng.randrange(R)) for _ in range(130)]
    def derive(host):
        n = len(seeds); out = [np.full((n, 32), 9, np.uint8) for _ in range(3)]; flags = np.full(n, 9, np.uint8)
        L_ = aleo_amd.lib(); call = L_.aleo_mi355x_accounts_derive_host if host else L_.aleo_mi355x_accounts_derive
        return call(_vp(b''.join(seeds)), n, _p(out[0]), _p(out[1]), _p(out[2]), None, _p(flags)), [o.tobytes() for o in out], flags.tobytes()
    want = [open_raw(pairs, host=True), derive(True)]
    assert bs.two_threads(lambda i: open_raw(pairs, host=False) if i == 0 else derive(False)) == want


@pytest.mark.gpu
def test_gpu_cpp_mirror_on_the_kernel(tmp_path):
    run_cpp_mirror(tmp_path, {'ALEO_MI355X_MIN_KEY_CIPHERTEXTS': '0', 'ALEO_MI355X_MIN_ACCOUNTS': '0'}, 70)
