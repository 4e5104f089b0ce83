"""Accounts in batches: the mirror of the reference's account module — PrivateKey::new / from_seed_unchecked / to_view_key / to_address
(wasm/src/account/private_key.rs:38-86) and `new Account({seed})` (sdk/src/account.ts:82) — for callers that derive many at once: a front end answering for many
callers, a wallet restoring a range of keys, a service handing out deposit addresses, a search for an address with a chosen prefix.
aleo_mi355x_accounts_derive / _accounts_search: csrc/accounts.hip, one account per GPU lane; small batches and host=True run the code of
records.Account.from_private_key on the calling thread, which is the definition.  A seed is the 32 bytes an "APrivateKey1…" string holds (a canonical
little-endian field element); records.Account is what the calls return."""
from __future__ import annotations
import ctypes, os
import numpy as np
from ._lib import lib, check, _p, _vp
from .records import Account

DERIVED, BAD_SEED = 0, 3
PREFIX_CHARSET = 'qpzry9x8gf2tvdw0s3jn54khce6mua7l'
MAX_PREFIX = 12


def _seed_rows(seeds) -> np.ndarray:
    if isinstance(seeds, np.ndarray): return np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
    if isinstance(seeds, (bytes, bytearray)): seeds = [seeds]
    rows = [s if isinstance(s, (bytes, bytearray)) else int(s).to_bytes(32, 'little') for s in seeds]
    if any(len(r) != 32 for r in rows): raise ValueError('a seed has 32 bytes')
    return np.frombuffer(b''.join(bytes(r) for r in rows), dtype=np.uint8).reshape(-1, 32).copy()


def private_key_from_seed(seed: bytes) -> str:
    """The "APrivateKey1…" string of a seed; a seed that is not a canonical field element is refused."""
    if len(seed) != 32: raise ValueError('a seed has 32 bytes')
    out = ctypes.create_string_buffer(64)
    check(lib().aleo_mi355x_private_key_from_seed(out, len(out), _vp(bytes(seed))), 'private_key_from_seed')
    return out.value.decode()


def private_key_seed(private_key: str) -> bytes:
    """The 32 seed bytes of an "APrivateKey1…" string."""
    out = np.zeros(32, dtype=np.uint8)
    check(lib().aleo_mi355x_private_key_seed(_p(out), private_key.encode()), 'private_key_seed')
    return out.tobytes()


def seed_from_bytes(raw: bytes) -> bytes:
    """from_seed_unchecked's reduction (private_key.rs:47-55): 32 arbitrary bytes, little-endian, mod r.  UNPINNED for a value not below r."""
    if len(raw) != 32: raise ValueError('32 bytes')
    out = np.zeros(32, dtype=np.uint8)
    check(lib().aleo_mi355x_seed_from_bytes(_p(out), _vp(bytes(raw))), 'seed_from_bytes')
    return out.tobytes()


def view_key_string(view_key: bytes) -> str:
    out = ctypes.create_string_buffer(64)
    check(lib().aleo_mi355x_view_key_to_string(out, len(out), _vp(bytes(view_key))), 'view_key_to_string')
    return out.value.decode()


def derive_many(seeds, strings: bool = False, host: bool = False):
    """(sk_sig, view_key, address_x, flags[, addresses]): n x 32 arrays of canonical little-endian bytes, flags (0 derived; 3 the seed is not a canonical field
    element: its rows are zero) and, with strings=True, the n "aleo1…" strings ('' where the flag is 3)."""
    rows = _seed_rows(seeds); n = rows.shape[0]
    sk, vk, ax = (np.zeros((n, 32), dtype=np.uint8) for _ in range(3))
    flags = np.zeros(n, dtype=np.uint8); text = np.zeros((n, 63), dtype=np.uint8) if strings else None
    L = lib(); call = L.aleo_mi355x_accounts_derive_host if host else L.aleo_mi355x_accounts_derive
    check(call(_p(rows), n, _p(sk), _p(vk), _p(ax), _p(text) if strings else None, _p(flags)), 'accounts_derive')
    if not strings: return sk, vk, ax, flags
    return sk, vk, ax, flags, [text[i].tobytes().decode() if flags[i] == DERIVED else '' for i in range(n)]


def accounts_from_seeds(seeds, host: bool = False):
    """The accounts of n seeds, with their private key strings; a seed that is not a canonical field element raises."""
    rows = _seed_rows(seeds)
    sk, vk, ax, flags = derive_many(rows, host=host)
    if flags.any(): raise ValueError('seed %d is not a canonical field element' % int(np.flatnonzero(flags)[0]))
    return [Account(private_key_from_seed(rows[i].tobytes()), sk[i].tobytes(), vk[i].tobytes(), ax[i].tobytes()) for i in range(rows.shape[0])]


def accounts_from_private_keys(keys, host: bool = False):
    """The accounts of n "APrivateKey1…" strings: the strings are decoded on the host and the accounts derived in one call."""
    keys = list(keys)
    sk, vk, ax, flags = derive_many([private_key_seed(k) for k in keys], host=host)
    return [Account(k, sk[i].tobytes(), vk[i].tobytes(), ax[i].tobytes()) for i, k in enumerate(keys)]


def account_from_seed(seed: bytes) -> Account:
    """`new Account({seed})` of the reference's SDK: the account whose private key holds these 32 bytes, reduced mod r as from_seed_unchecked reduces them."""
    return accounts_from_seeds([seed_from_bytes(seed)], host=True)[0]


def search(master: bytes, prefix: str, first: int = 0, count: int = 1 << 20, max_hits: int = 1, host: bool = False):
    """(hits, next): the accounts (with their private key strings and, as .index, their position) of the first max_hits candidates of [first, first + count) whose
    address begins with "aleo1" + prefix, and the index to resume from.  Candidate i's private-key seed is element i of the ChaCha20 stream under the 32-byte
    master seed: keep the master seed secret, it regenerates every key found."""
    if len(master) != 32: raise ValueError('the master seed has 32 bytes')
    idx = np.zeros(max(max_hits, 1), dtype=np.uint64); seeds = np.zeros((max(max_hits, 1), 32), dtype=np.uint8)
    n = ctypes.c_size_t(0); nxt = ctypes.c_uint64(0)
    L = lib(); call = L.aleo_mi355x_accounts_search_host if host else L.aleo_mi355x_accounts_search
    check(call(_vp(bytes(master)), first, count, prefix.encode() if prefix is not None else None, max_hits, _p(idx), _p(seeds), ctypes.byref(n), ctypes.byref(nxt)), 'accounts_search')
    hits = accounts_from_seeds(seeds[:n.value], host=True) if n.value else []
    for a, i in zip(hits, idx[:n.value]): a.index = int(i)
    return hits, int(nxt.value)
