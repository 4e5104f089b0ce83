"""Account signatures: the mirror of the reference's Signature.sign / verify / to_string (wasm/src/account/signature.rs:37-48), Address.verify
(wasm/src/account/address.rs:69-71), PrivateKey.sign (wasm/src/account/private_key.rs:244-248) and Account.sign / verify (sdk/src/account.ts:195,211-213) —
and, for a front end that answers for many accounts at once, verify_many: n signatures under one or n addresses over n messages in one call
(aleo_mi355x_signatures_verify: csrc/signatures.hip, one signature per GPU lane; small batches and host=True run csrc/signature_host.hpp on the calling thread),
and sign_many: n messages signed under one key or under a key each in one call (aleo_mi355x_signatures_sign: csrc/signatures_sign.hip, likewise).
A signature is 128 bytes, challenge | response | pk_sig.x | pr_sig.x, and a "sign1…" string (bech32m)."""
from __future__ import annotations
import ctypes, os
import numpy as np
from ._lib import lib, check, _p, _blob
from .records import address_x_bytes

VERIFIES, DOES_NOT_VERIFY, NOT_A_SIGNATURE = 0, 1, 3
MAX_MESSAGE_BYTES = 131071                                       # 4161 fields of 252 bits


def _message(m) -> bytes: return m.encode() if isinstance(m, str) else bytes(m)


class Signature:
    """128 bytes: challenge | response | pk_sig.x | pr_sig.x, canonical little-endian."""

    def __init__(self, raw: bytes):
        if len(raw) != 128: raise ValueError('a signature has 128 bytes')
        self.raw = bytes(raw)

    @classmethod
    def from_string(cls, s: str) -> 'Signature':
        out = np.zeros(128, dtype=np.uint8)
        check(lib().aleo_mi355x_signature_from_string(_p(out), s.encode()), 'signature_from_string')
        return cls(out.tobytes())

    def __str__(self) -> str:
        out = ctypes.create_string_buffer(256); raw = np.frombuffer(self.raw, dtype=np.uint8)
        check(lib().aleo_mi355x_signature_to_string(out, len(out), _p(raw)), 'signature_to_string')
        return out.value.decode()

    def __repr__(self): return 'Signature(%r)' % str(self)
    def __eq__(self, other): return isinstance(other, Signature) and other.raw == self.raw
    def __hash__(self): return hash(self.raw)

    @property
    def bytes(self) -> bytes: return self.raw

    def verify(self, address, message) -> bool:
        """Signature.verify(address, message) of the reference: one signature, on the calling thread."""
        return int(verify_many([self], address, [message], host=True)[0]) == VERIFIES


def sign(private_key: str, message, seed: bytes = None) -> Signature:
    """PrivateKey.sign(message): the signature of the message's bytes under the account of an "APrivateKey1…" string.  The nonce comes from `seed` (32 bytes;
    os.urandom(32) when None) alone, so signing is reproducible — and a seed must NEVER be used for two messages."""
    seed = os.urandom(32) if seed is None else bytes(seed)
    if len(seed) != 32: raise ValueError('the seed has 32 bytes')
    m = _message(message); out = np.zeros(128, dtype=np.uint8)
    check(lib().aleo_mi355x_signature_sign(_p(out), private_key.encode(), ctypes.cast(ctypes.c_char_p(m), ctypes.c_void_p), len(m), ctypes.cast(ctypes.c_char_p(seed), ctypes.c_void_p)), 'signature_sign')
    return Signature(out.tobytes())


def _key_seed_rows(private_keys) -> np.ndarray:
    """n x 32: the seeds of one "APrivateKey1…" string, of a list of them, or an array of seed rows as it stands."""
    from .account import private_key_seed
    if isinstance(private_keys, np.ndarray): return np.ascontiguousarray(private_keys, dtype=np.uint8).reshape(-1, 32)
    keys = [private_keys] if isinstance(private_keys, str) else list(private_keys)
    return np.frombuffer(b''.join(private_key_seed(k) for k in keys), dtype=np.uint8).reshape(-1, 32).copy()


def sign_many(private_keys, messages, seeds=None, host: bool = False):
    """(rows, flags): row i (of an n x 128 array) is sign(key i, message i, seed i).bytes, flags[i] 0; or zeros with flags[i] 3 where the key's seed is no field
    element or the message is longer than MAX_MESSAGE_BYTES.  private_keys: one "APrivateKey1…" string (one key for all messages), a list of n of them, or an
    n x 32 array of their seeds (a 1 x 32 array: one key for all).  seeds: n x 32 bytes (an array, or the bytes joined), one nonce seed per signature;
    os.urandom(32 * n) when None.  Two equal seeds in one call are refused: a seed must NEVER be used for two messages."""
    msgs = [_message(m) for m in messages]; n = len(msgs)
    keys = _key_seed_rows(private_keys)
    if keys.shape[0] not in (1, n): raise ValueError('one private key, or one per message')
    stride = 32 if keys.shape[0] == n and not isinstance(private_keys, str) and n != 1 else 0
    if seeds is None: seeds = os.urandom(32 * n)
    sd = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1) if isinstance(seeds, np.ndarray) else np.frombuffer(bytes(seeds), dtype=np.uint8)
    if sd.size != 32 * n: raise ValueError('one seed of 32 bytes per message')
    text, offsets = _blob(msgs); rows = np.zeros((n, 128), dtype=np.uint8); flags = np.zeros(n, dtype=np.uint8)
    L = lib(); call = L.aleo_mi355x_signatures_sign_host if host else L.aleo_mi355x_signatures_sign
    check(call(_p(rows), _p(flags), _p(keys), stride, ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p), _p(offsets), _p(sd), n), 'signatures_sign')
    return rows, flags


def _signature_rows(signatures) -> np.ndarray:
    if isinstance(signatures, np.ndarray): return np.ascontiguousarray(signatures, dtype=np.uint8).reshape(-1, 128)
    rows = [s.raw if isinstance(s, Signature) else Signature.from_string(s).raw if isinstance(s, str) else Signature(bytes(s)).raw for s in signatures]
    return np.frombuffer(b''.join(rows), dtype=np.uint8).reshape(-1, 128).copy()


def verify_many(signatures, addresses, messages, host: bool = False) -> np.ndarray:
    """flags[i]: 0 signature i verifies under its address over message i, 1 it does not, 3 it is no signature.  signatures: Signature objects, "sign1…" strings or
    an n x 128 array; addresses: one address or n, "aleo1…" strings or 32-byte x rows; messages: n byte strings."""
    sigs = _signature_rows(signatures); n = sigs.shape[0]
    if isinstance(addresses, np.ndarray): addr = np.ascontiguousarray(addresses, dtype=np.uint8).reshape(-1, 32)
    elif isinstance(addresses, (str, bytes, bytearray, int)): addr = np.frombuffer(address_x_bytes(addresses), dtype=np.uint8).reshape(1, 32).copy()
    else: addr = np.frombuffer(b''.join(address_x_bytes(a) for a in addresses), dtype=np.uint8).reshape(-1, 32).copy()
    if addr.shape[0] not in (1, n): raise ValueError('one address, or one per signature')
    stride = 32 if addr.shape[0] == n and n != 1 else 0
    msgs = [_message(m) for m in messages]
    if len(msgs) != n: raise ValueError('one message per signature')
    text, offsets = _blob(msgs); flags = np.zeros(n, dtype=np.uint8)
    L = lib(); call = L.aleo_mi355x_signatures_verify_host if host else L.aleo_mi355x_signatures_verify
    check(call(_p(flags), _p(sigs), _p(addr), stride, ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p), _p(offsets), n), 'signatures_verify')
    return flags
