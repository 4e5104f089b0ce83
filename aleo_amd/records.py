"""Which records does an account own?  The mirror of the reference's RecordCiphertext.isOwner (wasm/src/record/record_ciphertext.rs:63-66) and of the
loop around `record.is_owner_with_address_x_coordinate` in rust/src/api/blocking.rs:213-218, :274-276 — for a whole batch at a time, through the C ABI
(aleo_mi355x_record_parse, aleo_mi355x_records_scan: csrc/wire.hip, csrc/records.hip).  View keys (base58, "AViewKey1…") and addresses (bech32m,
"aleo1…") are decoded here; the address of a view key is NOT derived (that needs upstream's hash-to-curve generator), so callers pass both, as the
reference's call sites do.  scan_many / find_owned_many ask for several accounts over the same records in one call (aleo_mi355x_records_scan_many:
csrc/records_many.hip), as a front end does that runs the search for several callers (rust/develop/src/routes.rs:112, :143, :194-220 of the reference)."""
from __future__ import annotations
import ctypes
import numpy as np
from ._lib import lib, check, AleoMi355xError
from . import wire

_B58 = '123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz'
_VIEW_KEY_PREFIX = bytes([14, 138, 223, 204, 247, 224, 122])      # "AViewKey1"
OWNER_PUBLIC, OWNER_PRIVATE = 0, 1


def _p(a): return a.ctypes.data_as(ctypes.c_void_p)


def view_key_bytes(view_key) -> bytes:
    """The 32 little-endian bytes of a view key's scalar, from its string (or the bytes / integer themselves)."""
    if isinstance(view_key, (bytes, bytearray)) and len(view_key) == 32: return bytes(view_key)
    if isinstance(view_key, int): return view_key.to_bytes(32, 'little')
    v = 0
    for ch in view_key:
        d = _B58.find(ch)
        if d < 0: raise ValueError('not a base58 string')
        v = v * 58 + d
    raw = v.to_bytes(39, 'big') if v < (1 << 312) else b''
    if len(raw) != 39 or raw[:7] != _VIEW_KEY_PREFIX: raise ValueError('not an Aleo view key')
    return raw[7:]


def address_x_bytes(address) -> bytes:
    """The 32 little-endian bytes of an address's x-coordinate, from its "aleo1…" string (or the bytes / integer themselves)."""
    if isinstance(address, (bytes, bytearray)) and len(address) == 32: return bytes(address)
    if isinstance(address, int): return address.to_bytes(32, 'little')
    hrp, raw = wire.bech32m_decode(address)
    if hrp != 'aleo' or len(raw) != 32: raise ValueError('not an Aleo address')
    return raw


def scan(owner_c0: np.ndarray, nonce_x: np.ndarray, view_key, address, want_rvk: bool = True, host: bool = False):
    """flags (uint8[n]: 1 owner, 0 not owner, 2 malformed) and, when want_rvk, the record view keys' x (uint8[n, 32], zeros where the flag is 2) of n
    private-owner records given as canonical 32-byte rows.  host=True computes on the CPU (aleo_mi355x_records_scan_host), else the library routes."""
    c0 = np.ascontiguousarray(owner_c0, dtype=np.uint8).reshape(-1, 32); nx = np.ascontiguousarray(nonce_x, dtype=np.uint8).reshape(-1, 32)
    if c0.shape != nx.shape: raise ValueError('owner_c0 and nonce_x differ in length')
    n = c0.shape[0]
    flags = np.zeros(n, dtype=np.uint8); rvk = np.zeros((n, 32), dtype=np.uint8) if want_rvk else None
    vk = np.frombuffer(view_key_bytes(view_key), dtype=np.uint8); ax = np.frombuffer(address_x_bytes(address), dtype=np.uint8)
    f = lib().aleo_mi355x_records_scan_host if host else lib().aleo_mi355x_records_scan
    check(f(_p(flags), _p(rvk) if want_rvk else None, _p(c0), _p(nx), n, _p(vk), _p(ax)), 'records_scan')
    return flags, rvk


def scan_many(owner_c0: np.ndarray, nonce_x: np.ndarray, view_keys, addresses, want_rvk: bool = True, host: bool = False):
    """scan for several accounts over the same n records in one call (aleo_mi355x_records_scan_many / _many_host): flags (uint8[K, n]) and, when want_rvk,
    the record view keys' x (uint8[K, n, 32]); row j is what scan returns for (view_keys[j], addresses[j]) alone.  1 <= K <= 64; keys may repeat."""
    c0 = np.ascontiguousarray(owner_c0, dtype=np.uint8).reshape(-1, 32); nx = np.ascontiguousarray(nonce_x, dtype=np.uint8).reshape(-1, 32)
    if c0.shape != nx.shape: raise ValueError('owner_c0 and nonce_x differ in length')
    if len(view_keys) != len(addresses): raise ValueError('view_keys and addresses differ in length')
    n, k = c0.shape[0], len(view_keys)
    flags = np.zeros((k, n), dtype=np.uint8); rvk = np.zeros((k, n, 32), dtype=np.uint8) if want_rvk else None
    vk = np.frombuffer(b''.join(view_key_bytes(v) for v in view_keys), dtype=np.uint8); ax = np.frombuffer(b''.join(address_x_bytes(a) for a in addresses), dtype=np.uint8)
    f = lib().aleo_mi355x_records_scan_many_host if host else lib().aleo_mi355x_records_scan_many
    check(f(_p(flags), _p(rvk) if want_rvk else None, _p(c0), _p(nx), n, _p(vk), _p(ax), k), 'records_scan_many')
    return flags, rvk


class RecordCiphertext:
    """A parsed "record1…" string: the owner variant, the owner field (address x, or the one field of the owner ciphertext) and the nonce x."""

    def __init__(self, string: str, owner_kind: int, owner: bytes, nonce: bytes):
        self.string, self.owner_kind, self.owner, self.nonce = string, owner_kind, owner, nonce

    @classmethod
    def from_string(cls, s: str) -> 'RecordCiphertext':
        kind = ctypes.c_int32(-1); owner = np.zeros(32, dtype=np.uint8); nonce = np.zeros(32, dtype=np.uint8)
        check(lib().aleo_mi355x_record_parse(s.encode(), ctypes.byref(kind), _p(owner), _p(nonce)), 'record_parse')
        return cls(s, kind.value, owner.tobytes(), nonce.tobytes())

    def __str__(self): return self.string

    def is_owner(self, view_key, address) -> bool:
        """RecordCiphertext.isOwner: a public owner is compared with the address, a private one goes through the scan."""
        if self.owner_kind == OWNER_PUBLIC: return self.owner == address_x_bytes(address)
        flags, _ = scan(np.frombuffer(self.owner, dtype=np.uint8), np.frombuffer(self.nonce, dtype=np.uint8), view_key, address, want_rvk=False)
        return int(flags[0]) == 1


def find_owned(ciphertexts, view_key, address):
    """The indices of the records the account owns, and their record view keys' x (32 little-endian bytes each; None for a public owner, whose record is
    not encrypted to anyone): the batch form of the reference's record search.  `ciphertexts`: strings or RecordCiphertext objects; a string that does
    not parse raises."""
    recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
    ax = address_x_bytes(address)
    priv = [i for i, r in enumerate(recs) if r.owner_kind == OWNER_PRIVATE]
    owned = {i: None for i, r in enumerate(recs) if r.owner_kind == OWNER_PUBLIC and r.owner == ax}
    if priv:
        c0 = np.frombuffer(b''.join(recs[i].owner for i in priv), dtype=np.uint8).reshape(-1, 32)
        nx = np.frombuffer(b''.join(recs[i].nonce for i in priv), dtype=np.uint8).reshape(-1, 32)
        flags, rvk = scan(c0, nx, view_key, ax)
        for j, i in enumerate(priv):
            if flags[j] == 1: owned[i] = rvk[j].tobytes()
    idx = sorted(owned)
    return idx, [owned[i] for i in idx]


def find_owned_many(ciphertexts, accounts):
    """find_owned for several accounts over the same records: `accounts` is a sequence of (view_key, address) pairs, the result a list with, for each of
    them, what find_owned returns.  Every string is parsed once and the private owners of all accounts go through one scan_many call."""
    recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
    accounts = [(vk, address_x_bytes(a)) for vk, a in accounts]
    priv = [i for i, r in enumerate(recs) if r.owner_kind == OWNER_PRIVATE]
    owned = [{i: None for i, r in enumerate(recs) if r.owner_kind == OWNER_PUBLIC and r.owner == ax} for _, ax in accounts]
    if priv and accounts:
        c0 = np.frombuffer(b''.join(recs[i].owner for i in priv), dtype=np.uint8).reshape(-1, 32)
        nx = np.frombuffer(b''.join(recs[i].nonce for i in priv), dtype=np.uint8).reshape(-1, 32)
        flags, rvk = scan_many(c0, nx, [vk for vk, _ in accounts], [ax for _, ax in accounts])
        for a, mine in enumerate(owned):
            for j in np.nonzero(flags[a] == 1)[0]: mine[priv[j]] = rvk[a, j].tobytes()
    return [(sorted(mine), [mine[i] for i in sorted(mine)]) for mine in owned]
