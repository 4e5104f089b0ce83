"""Private key ciphertexts: the mirror of the reference's PrivateKeyCiphertext (wasm/src/account/private_key_ciphertext.rs:39-73 encryptPrivateKey,
decryptToPrivateKey; wasm/src/account/private_key.rs:102-130 newEncrypted, toCiphertext, fromPrivateKeyCiphertext) — a private key encrypted under a secret,
"ciphertext1…" — and the batched opening a front end needs that holds one ciphertext and one password per request: n (ciphertext, secret) pairs in, the seeds of
their private keys and the accounts of those seeds out, in one call.
aleo_mi355x_private_key_encrypt / _decrypt: host code; aleo_mi355x_private_keys_open: csrc/key_ciphertexts.hip, one pair per GPU lane, with the account kernel
behind it; small batches and host=True run the host path on the calling thread, which is the definition.  A secret is a str (its UTF-8 bytes) or any bytes."""
from __future__ import annotations
import ctypes, os
import numpy as np
from ._lib import lib, check, _p, _vp, _blob
from .records import Account
from .account import private_key_from_seed

OPENED, NOT_DECRYPTED, NO_CIPHERTEXT = 0, 1, 3
CHARS = 174


def _secret(s) -> bytes: return s.encode() if isinstance(s, str) else bytes(s)


def random_nonce() -> bytes:
    """A uniform field element, as upstream draws the nonce with Uniform::rand: element 0 of the library's ChaCha20 Fr stream under 32 bytes from the OS."""
    out = np.zeros(32, dtype=np.uint8)
    check(lib().aleo_mi355x_fr_random(_p(out), 1, _vp(os.urandom(32)), 0), 'fr_random')
    return out.tobytes()


def encrypt(private_key: str, secret, nonce=None) -> str:
    """PrivateKeyCiphertext.encryptPrivateKey: the "ciphertext1…" string of an "APrivateKey1…" string under a secret.  nonce: 32 canonical little-endian bytes or
    an int below r (tests: a repeated nonce repeats the string); None draws one."""
    if nonce is None: nonce = random_nonce()
    elif not isinstance(nonce, (bytes, bytearray)): nonce = int(nonce).to_bytes(32, 'little')
    if len(nonce) != 32: raise ValueError('a nonce has 32 bytes')
    sec = _secret(secret); out = ctypes.create_string_buffer(CHARS + 1)
    check(lib().aleo_mi355x_private_key_encrypt(out, len(out), private_key.encode(), _vp(sec), len(sec), _vp(bytes(nonce))), 'private_key_encrypt')
    return out.value.decode()


def decrypt(ciphertext: str, secret) -> str:
    """PrivateKeyCiphertext.decryptToPrivateKey: the "APrivateKey1…" string.  Raises NotOwner where the ciphertext does not decrypt under this secret, AleoMi355xError
    (status 2) for what is no ciphertext string."""
    sec = _secret(secret); out = ctypes.create_string_buffer(64)
    check(lib().aleo_mi355x_private_key_decrypt(out, len(out), ciphertext.encode(), _vp(sec), len(sec)), 'private_key_decrypt')
    return out.value.decode()


def open_many(ciphertexts, secrets, strings: bool = False, host: bool = False):
    """(seeds, sk_sig, view_key, address_x, flags[, addresses]): n x 32 arrays of canonical little-endian bytes, flags (0 opened; 1 the ciphertext does not decrypt
    under its secret; 3 no ciphertext string: the rows of a flagged pair are zero) and, with strings=True, the n "aleo1…" strings ('' where flagged)."""
    texts = [c.encode() if isinstance(c, str) else bytes(c) for c in ciphertexts]; secs = [_secret(s) for s in secrets]
    if len(texts) != len(secs): raise ValueError('one secret per ciphertext')
    n = len(texts)
    text, off = _blob(texts); sblob, soff = _blob(secs)
    seeds, sk, vk, ax = (np.zeros((n, 32), dtype=np.uint8) for _ in range(4))
    flags = np.zeros(n, dtype=np.uint8); addr = np.zeros((n, 63), dtype=np.uint8) if strings else None
    L = lib(); call = L.aleo_mi355x_private_keys_open_host if host else L.aleo_mi355x_private_keys_open
    check(call(_vp(text), _p(off), _vp(sblob), _p(soff), n, _p(seeds), _p(sk), _p(vk), _p(ax), _p(addr), _p(flags)), 'private_keys_open')
    if not strings: return seeds, sk, vk, ax, flags
    return seeds, sk, vk, ax, flags, [addr[i].tobytes().decode() if flags[i] == OPENED else '' for i in range(n)]


def accounts_from_ciphertexts(pairs, host: bool = False):
    """The accounts of n (ciphertext, secret) pairs, with their private key strings; None where a pair does not open."""
    pairs = list(pairs)
    seeds, sk, vk, ax, flags = open_many([c for c, _ in pairs], [s for _, s in pairs], host=host)
    return [Account(private_key_from_seed(seeds[i].tobytes()), sk[i].tobytes(), vk[i].tobytes(), ax[i].tobytes()) if flags[i] == OPENED else None for i in range(len(pairs))]
