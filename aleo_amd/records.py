"""Which records does an account own?  The mirror of the reference's RecordCiphertext.isOwner (wasm/src/record/record_ciphertext.rs:63-66) and of the
loop around `record.is_owner_with_address_x_coordinate` in rust/src/api/blocking.rs:213-218, :274-276 — for a whole batch at a time, through the C ABI
(aleo_mi355x_record_parse, aleo_mi355x_records_scan: csrc/wire.hip, csrc/records.hip).  View keys (base58, "AViewKey1…") and addresses (bech32m,
"aleo1…") are decoded here, and callers pass both, as the reference's call sites do; Account.from_private_key (below) derives both, and sk_sig, from an
"APrivateKey1…" string.  scan_many / find_owned_many ask for several accounts over the same records in one call (aleo_mi355x_records_scan_many:
csrc/records_many.hip), as a front end does that runs the search for several callers (rust/develop/src/routes.rs:112, :143, :194-220 of the reference).
What the reference does with an owned record next — `record.decrypt(&view_key)`, `microcredits()` (rust/src/api/blocking.rs:274-283; RecordCiphertext.decrypt
of the wasm) — is RecordCiphertext.decrypt, decrypt_fields and decrypt_owned here (aleo_mi355x_record_decrypt, aleo_mi355x_records_decrypt_fields,
aleo_mi355x_record_fields, aleo_mi355x_record_plaintext: csrc/records_decrypt.hip), down to RecordPlaintext strings.
Callers that hold "record1…" strings — what the chain hands out — pass them as they are: RecordBatch puts them into one blob, parse_many / scan_strings
(aleo_mi355x_records_parse_many, aleo_mi355x_records_scan_strings: csrc/records_strings.hip) decode them on the device, and find_owned, find_owned_many and
decrypt_owned take that road for a RecordBatch or a sequence of strings, building RecordCiphertext objects only for the records they return or decrypt.
decrypt_strings and balance (aleo_mi355x_records_decrypt_strings: csrc/records_found.hip) go from the strings of one account's search to the plain fields and
microcredits of the records it owns in one call, and bring back only those; decrypt_owned on strings is that call and the rendering of the strings.
decrypt_strings_many, balances and decrypt_owned_many (aleo_mi355x_records_decrypt_strings_many: csrc/records_found.hip, the same flow with K keys) are the same for several accounts
over the same strings: one upload and parse, one grouped scan, one gather and decryption of every owned (account, record) pair.
What the reference needs before it can use an owned record — its serial number, to ask the chain whether it is spent (rust/src/api/blocking.rs:277-278;
RecordPlaintext.serialNumberString of the wasm) — is serial_numbers, found_serial_numbers and unspent here (aleo_mi355x_records_serial_numbers,
aleo_mi355x_found_serial_numbers: csrc/records_serial.hip), with record_commitment, record_checksum and Account.from_private_key on the host beside them.
Callers that hold record PLAINTEXT strings — what every write call of the reference takes, what findUnspentRecords hands back and a wallet stores — pass those:
RecordPlaintext.from_string reads one, serial_number_string works on any plaintext, and plaintext_commitments, plaintext_serial_numbers and plaintexts_unspent
take a batch of them through one call (aleo_mi355x_plaintexts_commitments, aleo_mi355x_plaintexts_serial_numbers: csrc/plaintexts.hip).
The other direction — what every execute, transfer, split and join runs for each output record (rust/src/program/execute.rs:74,177, transfer.rs:99-106) — is
RecordPlaintext.encrypt / encrypt_symmetric, record_nonce and, for a batch, encrypt_many (aleo_mi355x_record_encrypt, aleo_mi355x_records_encrypt:
csrc/records_encrypt.hip): plaintext strings and randomizers in, a RecordBatch of "record1…" strings out that scan_strings and decrypt_strings take as it is."""
from __future__ import annotations
import ctypes, weakref
import numpy as np
from ._lib import lib, check, _p, AleoMi355xError, NotOwner      # noqa: F401
from . import wire

_B58 = '123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz'
_VIEW_KEY_PREFIX = bytes([14, 138, 223, 204, 247, 224, 122])      # "AViewKey1"
OWNER_PUBLIC, OWNER_PRIVATE = 0, 1


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

    def fields(self) -> np.ndarray:
        """The record's private fields in randomizer order (uint8[m, 32]): the owner's if it is private, then every private entry's."""
        n = ctypes.c_size_t(0)
        check(lib().aleo_mi355x_record_fields(self.string.encode(), None, 0, ctypes.byref(n)), 'record_fields')
        out = np.zeros((n.value, 32), dtype=np.uint8)
        if n.value: check(lib().aleo_mi355x_record_fields(self.string.encode(), _p(out), n.value, ctypes.byref(n)), 'record_fields')
        return out

    def plaintext(self, plain_fields: np.ndarray, address=None) -> 'RecordPlaintext':
        """The RecordPlaintext of this record from its decrypted fields (aleo_mi355x_record_plaintext); with an address, NotOwner unless the owner is it."""
        f = np.ascontiguousarray(plain_fields, dtype=np.uint8).reshape(-1, 32)
        ax = np.frombuffer(address_x_bytes(address), dtype=np.uint8) if address is not None else None
        return RecordPlaintext(_string_out(lambda buf, ln: lib().aleo_mi355x_record_plaintext(self.string.encode(), _p(f), f.shape[0], _p(ax) if ax is not None else None, buf, ln), 'record_plaintext'),
                               self.string, f.copy())

    def decrypt(self, view_key, address) -> 'RecordPlaintext':
        """RecordCiphertext.decrypt(viewKey), on the host (aleo_mi355x_record_decrypt): NotOwner when the view key does not decrypt the owner to the address."""
        vk = np.frombuffer(view_key_bytes(view_key), dtype=np.uint8); ax = np.frombuffer(address_x_bytes(address), dtype=np.uint8)
        return RecordPlaintext(_string_out(lambda buf, ln: lib().aleo_mi355x_record_decrypt(self.string.encode(), _p(vk), _p(ax), buf, ln), 'record_decrypt'),
                               self.string, lambda: self.decrypted_fields(view_key))

    def decrypted_fields(self, view_key) -> np.ndarray:
        """The record's private fields decrypted with the view key, on the host (uint8[m, 32]): what record_commitment takes beside the string."""
        fields = self.fields()
        if not len(fields): return fields
        vk = np.frombuffer(view_key_bytes(view_key), dtype=np.uint8)
        flags = np.zeros(1, dtype=np.uint8); rvk = np.zeros((1, 32), dtype=np.uint8)
        c0 = np.frombuffer(self.owner if self.owner_kind == OWNER_PRIVATE else bytes(32), dtype=np.uint8); nx = np.frombuffer(self.nonce, dtype=np.uint8)
        check(lib().aleo_mi355x_records_scan_host(_p(flags), _p(rvk), _p(c0), _p(nx), 1, _p(vk), _p(np.zeros(32, dtype=np.uint8))), 'records_scan')
        plain, bad = decrypt_fields(rvk, [0, len(fields)], fields, host=True)
        if flags[0] == 2 or bad[0]: raise AleoMi355xError('decrypted_fields: the record is malformed')
        return plain


class RecordBatch:
    """n "record1…" strings as the C ABI takes them: the text of all of them one after another (bytes) and n + 1 uint64 offsets."""

    def __init__(self, text: bytes, offsets: np.ndarray):
        self.text = bytes(text); self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if self.offsets.ndim != 1 or len(self.offsets) < 1 or self.offsets[0] != 0 or int(self.offsets[-1]) != len(self.text) or (np.diff(self.offsets.astype(np.int64)) < 0).any():
            raise ValueError('offsets must start at 0, not decrease and end at the length of the text')

    @classmethod
    def from_strings(cls, strings) -> 'RecordBatch':
        """One join of all strings; the lengths by numpy (encoded one by one only when a string is not ASCII, which no record is)."""
        strings = list(strings)
        text = ''.join(strings).encode()
        lens = np.fromiter(map(len, strings), dtype=np.uint64, count=len(strings))
        if int(lens.sum()) != len(text): lens = np.fromiter((len(s.encode()) for s in strings), dtype=np.uint64, count=len(strings))
        offsets = np.zeros(len(strings) + 1, dtype=np.uint64); np.cumsum(lens, out=offsets[1:])
        return cls(text, offsets)

    @classmethod
    def from_text(cls, text: bytes, sep: bytes = b'\n') -> 'RecordBatch':
        """The strings of a text that holds one per line (or between any other one-byte separator): the separators are dropped, a trailing one is ignored."""
        if len(sep) != 1: raise ValueError('the separator is one byte')
        a = np.frombuffer(bytes(text), dtype=np.uint8)
        is_sep = a == sep[0]
        ends = np.flatnonzero(is_sep)
        if len(a) and not is_sep[-1]: ends = np.append(ends, len(a))
        starts = np.concatenate([[0], ends[:-1] + 1]) if len(ends) else ends
        offsets = np.zeros(len(ends) + 1, dtype=np.uint64); np.cumsum(ends - starts, out=offsets[1:])
        return cls(a[~is_sep].tobytes(), offsets)

    def __len__(self): return len(self.offsets) - 1

    def string(self, i: int) -> str:
        if not 0 <= i < len(self): raise IndexError(i)
        return self.text[int(self.offsets[i]):int(self.offsets[i + 1])].decode(errors='replace')


def _text_p(batch): return ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p)


def parse_many(batch: RecordBatch, host: bool = False):
    """kinds (int8[n]: 0 public owner, 1 private owner, -1 a string that does not parse), the owner fields and the nonces' x (uint8[n, 32] each, zeros where the
    kind is -1) of a batch of strings: what RecordCiphertext.from_string reads out of each, in one call (aleo_mi355x_records_parse_many / _many_host)."""
    n = len(batch)
    kinds = np.zeros(n, dtype=np.int8); owner = np.zeros((n, 32), dtype=np.uint8); nonce = np.zeros((n, 32), dtype=np.uint8)
    f = lib().aleo_mi355x_records_parse_many_host if host else lib().aleo_mi355x_records_parse_many
    check(f(_p(kinds), _p(owner), _p(nonce), _text_p(batch), _p(batch.offsets), n), 'records_parse_many')
    return kinds, owner, nonce


def scan_strings(batch: RecordBatch, view_keys, addresses, want_rvk: bool = True, host: bool = False):
    """scan_many straight from strings (aleo_mi355x_records_scan_strings / _strings_host): flags (uint8[K, n]: 0 not owner, 1 owner, 2 malformed, 3 the string does
    not parse), kinds (int8[n], as parse_many) and, when want_rvk, the record view keys' x (uint8[K, n, 32]).  A public owner is compared with the address."""
    if len(view_keys) != len(addresses): raise ValueError('view_keys and addresses differ in length')
    n, k = len(batch), len(view_keys)
    flags = np.zeros((k, n), dtype=np.uint8); kinds = np.zeros(n, dtype=np.int8); rvk = np.zeros((k, n, 32), dtype=np.uint8) if want_rvk else None
    vk = np.frombuffer(b''.join(view_key_bytes(v) for v in view_keys), dtype=np.uint8); ax = np.frombuffer(b''.join(address_x_bytes(a) for a in addresses), dtype=np.uint8)
    f = lib().aleo_mi355x_records_scan_strings_host if host else lib().aleo_mi355x_records_scan_strings
    check(f(_p(flags), _p(kinds), _p(rvk) if want_rvk else None, _text_p(batch), _p(batch.offsets), n, _p(vk), _p(ax), k), 'records_scan_strings')
    return flags, kinds, rvk


def _as_batch(ciphertexts):
    """The RecordBatch of a RecordBatch or of a sequence that holds only strings, else None (RecordCiphertext objects take the road they always took)."""
    if isinstance(ciphertexts, RecordBatch): return ciphertexts
    if isinstance(ciphertexts, (list, tuple)) and all(isinstance(c, str) for c in ciphertexts): return RecordBatch.from_strings(ciphertexts)
    return None


def _raise_unparsed(batch: RecordBatch, unparsed: np.ndarray):
    """What RecordCiphertext.from_string raises for the first string that does not parse."""
    bad = np.flatnonzero(unparsed)
    if len(bad): RecordCiphertext.from_string(batch.string(int(bad[0])))


def _string_out(call, what: str) -> str:
    """A string through the (out, in/out length) convention of the C ABI: a first try with room for most records, a second with the length the first returned."""
    cap = 4096
    for _ in range(2):
        buf = ctypes.create_string_buffer(cap); ln = ctypes.c_size_t(cap)
        rc = call(buf, ctypes.byref(ln))
        if rc == 0: return buf.value.decode()
        if rc != 2 or ln.value < cap: break
        cap = ln.value + 1
    check(rc, what)


class RecordPlaintext:
    """A decrypted record: its string as the reference prints it, the owner's address, the nonce's x, and the entries by name — a literal as its text with the
    visibility ("1500000000000000u64.private"), a struct as a dict of the same."""

    def __init__(self, string: str, ciphertext=None, plain_fields=None):
        self.string = string
        self.ciphertext, self._plain_fields = ciphertext, plain_fields      # what it was decrypted from: the "record1…" string, its plain fields (or a call that gives them)
        body, at = _parse_plaintext(string, 0)
        if not isinstance(body, dict) or string[at:].strip() or 'owner' not in body or '_nonce' not in body: raise ValueError('not a record plaintext')
        self.owner, self.owner_visibility = body.pop('owner').rsplit('.', 1)
        nonce = body.pop('_nonce')
        if not nonce.endswith('group.public'): raise ValueError('not a record plaintext')
        self.nonce = int(nonce[:-len('group.public')])
        self.entries = body

    def __str__(self): return self.string
    def __repr__(self): return 'RecordPlaintext(%r)' % self.string
    def __eq__(self, other): return isinstance(other, RecordPlaintext) and other.string == self.string
    def __hash__(self): return hash(self.string)

    @classmethod
    def from_string(cls, s: str) -> 'RecordPlaintext':
        """RecordPlaintext.fromString (wasm/src/record/record_plaintext.rs:45-50): the string read by the library (aleo_mi355x_record_plaintext_parse, which also
        asks that the owner, the nonce and group values are x-coordinates of points of the subgroup).  Raises AleoMi355xError with a text that begins with the
        reference's "The record plaintext string provided was invalid"."""
        if lib().aleo_mi355x_record_plaintext_parse(str(s).encode(), None, None, None, None): raise AleoMi355xError(lib().aleo_mi355x_last_error().decode())
        return cls(str(s))

    def microcredits(self) -> int:
        """The value of a u64 entry named microcredits, else 0 (RecordPlaintext.microcredits of the wasm)."""
        v = self.entries.get('microcredits')
        if not isinstance(v, str): return 0
        lit = v.rsplit('.', 1)[0]
        return int(lit[:-3]) if lit.endswith('u64') and lit[:-3].isdigit() else 0

    def encrypt(self, randomizer, set_nonce: bool = False) -> RecordCiphertext:
        """Record::encrypt(randomizer) on the host (aleo_mi355x_record_encrypt): the randomizer is a scalar below the subgroup order (an integer or 32 little-endian
        bytes) and x(randomizer G) must be this string's _nonce — or, with set_nonce, replaces it."""
        r = np.frombuffer(view_key_bytes(randomizer), dtype=np.uint8)
        return RecordCiphertext.from_string(_string_out(lambda buf, ln: lib().aleo_mi355x_record_encrypt(self.string.encode(), _p(r), 1 if set_nonce else 0, buf, ln), 'record_encrypt'))

    def encrypt_symmetric(self, rvk) -> RecordCiphertext:
        """Record::encrypt_symmetric_unchecked(record view key) on the host (aleo_mi355x_record_encrypt_symmetric): rvk is the key's x (an integer or 32 bytes); the
        nonce stays what the string says."""
        k = np.frombuffer(address_x_bytes(rvk), dtype=np.uint8)
        return RecordCiphertext.from_string(_string_out(lambda buf, ln: lib().aleo_mi355x_record_encrypt_symmetric(self.string.encode(), _p(k), buf, ln), 'record_encrypt_symmetric'))

    def serial_number_string(self, private_key, program_id: str, record_name: str) -> str:
        """RecordPlaintext.serialNumberString(privateKey, programId, recordName): "<decimal>field" (wasm/src/record/record_plaintext.rs:64-82).  The commitment is
        taken over the record's bits: of a plaintext that RecordCiphertext.decrypt / plaintext or decrypt_owned returned, from the "record1…" string and the
        decrypted fields it carries; of any other (RecordPlaintext.from_string), from the text itself (aleo_mi355x_plaintexts_serial_numbers_host).  private_key: an "APrivateKey1…" string or an
        Account.  Raises AleoMi355xError with the reference's messages: "Invalid ProgramID specified", "Invalid Identifier specified for record", "Serial number
        derivation failed"."""
        account = private_key if isinstance(private_key, Account) else Account.from_private_key(private_key)
        if self.ciphertext is None:                                 # from the text alone (RecordPlaintext.from_string): aleo_mi355x_plaintexts_serial_numbers_host
            sn, _, _, flags = plaintext_serial_numbers([self.string], program_id, record_name, account, host=True)
            if flags[0] == 3: raise AleoMi355xError(_PLAINTEXT_INVALID)
            if flags[0]: raise AleoMi355xError('Serial number derivation failed')
            return '%dfield' % int.from_bytes(sn[0].tobytes(), 'little')
        fields = self._plain_fields() if callable(self._plain_fields) else self._plain_fields
        sn, flags = serial_numbers(record_commitment(self.ciphertext, fields, program_id, record_name), account.sk_sig, host=True)
        if flags[0]: raise AleoMi355xError('Serial number derivation failed')
        return '%dfield' % int.from_bytes(sn[0].tobytes(), 'little')


def _parse_plaintext(s: str, at: int):
    """One value of a plaintext string from position `at`: ('{' name: value, ... '}') -> dict, anything else -> the literal's text.  Returns (value, next position)."""
    while s[at] in ' \t\r\n': at += 1
    if s[at] != '{':
        start = at; quoted = False
        while at < len(s) and (quoted or s[at] not in ',\n}'):
            if s[at] == '"': quoted = not quoted
            at += 1
        return s[start:at].strip(), at
    out = {}; at += 1
    while True:
        while s[at] in ' \t\r\n,': at += 1
        if s[at] == '}': return out, at + 1
        colon = s.index(':', at)
        name = s[at:colon].strip()
        out[name], at = _parse_plaintext(s, colon + 1)


def decrypt_fields(rvk: np.ndarray, offsets, fields: np.ndarray, host: bool = False):
    """The plain fields (uint8[total, 32]) and the flags (uint8[n]: 0 decrypted, 2 malformed, its rows zeros) of n records: record i has the record view key x
    rvk[i] and the private fields fields[offsets[i]:offsets[i + 1]] in randomizer order.  host=True computes on the CPU (aleo_mi355x_records_decrypt_fields_host),
    else the library routes; the bytes are the same."""
    rv = np.ascontiguousarray(rvk, dtype=np.uint8).reshape(-1, 32); f = np.ascontiguousarray(fields, dtype=np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    n = rv.shape[0]
    if off.shape != (n + 1,): raise ValueError('offsets must hold one entry more than there are records')
    if n and int(off.max()) > f.shape[0]: raise ValueError('offsets reach past the fields')
    plain = np.zeros_like(f); flags = np.zeros(n, dtype=np.uint8)
    fn = lib().aleo_mi355x_records_decrypt_fields_host if host else lib().aleo_mi355x_records_decrypt_fields
    check(fn(_p(plain), _p(flags), _p(rv), _p(off), _p(f), n), 'records_decrypt_fields')
    return plain, flags


class FoundRecords:
    """What decrypt_strings returns, as numpy copies: for the c records the account owns, in ascending record index, index (uint32[c]), kind (int8[c]: 0 public
    owner, 1 private), rvk (uint8[c, 32]), offsets (uint32[c + 1]) into plain (uint8[fields, 32]: the decrypted private fields in randomizer order), status
    (uint8[c]: 0 decrypted, 2 malformed, 4 the structure is refused) and microcredits (uint64[c]); unparsed / first_unparsed: the strings that do not parse.
    From unspent_strings[_many] the c records are those left of the `owned` the account owns, and serials (uint8[c, 32]) their serial numbers; from any other
    call serials is None and owned is c.  From unspent_named[_many] commitments (uint8[c, 32]) are the kept records' commitments as well; else None.
    A result made with keep=True also holds the library's own copy (for found_commitments), released with the object."""

    def __init__(self, index, kind, rvk, offsets, plain, status, microcredits, unparsed: int, first_unparsed: int, serials=None, owned=None, commitments=None):
        self.index, self.kind, self.rvk, self.offsets, self.plain, self.status, self.microcredits = index, kind, rvk, offsets, plain, status, microcredits
        self.unparsed, self.first_unparsed = unparsed, first_unparsed
        self.serials, self.owned, self.commitments = serials, len(index) if owned is None else owned, commitments
        self._native = None

    def __len__(self): return len(self.index)

    def fields(self, k: int) -> np.ndarray:
        """The plain fields of the k-th owned record."""
        return self.plain[int(self.offsets[k]):int(self.offsets[k + 1])]

    def arrays(self): return (self.index, self.kind, self.rvk, self.offsets, self.plain, self.status, self.microcredits)


def decrypt_strings(batch, view_key, address, host: bool = False, keep: bool = False) -> FoundRecords:
    """The records one account owns among a RecordBatch (or a sequence of strings), decrypted, in one call (aleo_mi355x_records_decrypt_strings / _strings_host):
    the scan, the owned records' private fields, their decryption and their microcredits, all on the device; only the owned records come back.  A string that
    does not parse is counted (unparsed, first_unparsed), not raised."""
    b = _as_batch(batch)
    if b is None: raise TypeError('decrypt_strings takes a RecordBatch or a sequence of strings')
    vk = np.frombuffer(view_key_bytes(view_key), dtype=np.uint8); ax = np.frombuffer(address_x_bytes(address), dtype=np.uint8)
    L = lib(); out = ctypes.c_void_p()
    f = L.aleo_mi355x_records_decrypt_strings_host if host else L.aleo_mi355x_records_decrypt_strings
    check(f(ctypes.byref(out), _text_p(b), _p(b.offsets), len(b), _p(vk), _p(ax)), 'records_decrypt_strings')
    return _found_of(L, out, keep)


def _found_of(L, out, keep: bool = False) -> FoundRecords:
    """The numpy copies of a result of the library, which is released — with `keep`, when the FoundRecords is."""
    found = None
    try:
        c, nf = int(L.aleo_mi355x_found_count(out)), int(L.aleo_mi355x_found_fields(out))
        def copy(name, dtype, count, shape):
            size = count * np.dtype(dtype).itemsize
            return np.frombuffer(ctypes.string_at(getattr(L, 'aleo_mi355x_found_' + name)(out), size) if size else b'', dtype=dtype).reshape(shape).copy()
        found = FoundRecords(copy('index', np.uint32, c, (c,)), copy('kind', np.int8, c, (c,)), copy('rvk', np.uint8, 32 * c, (c, 32)), copy('offsets', np.uint32, c + 1, (c + 1,)),
                            copy('plain', np.uint8, 32 * nf, (nf, 32)), copy('status', np.uint8, c, (c,)), copy('microcredits', np.uint64, c, (c,)),
                             int(L.aleo_mi355x_found_unparsed(out)), int(L.aleo_mi355x_found_first_unparsed(out)),
                             copy('serials', np.uint8, 32 * c, (c, 32)) if L.aleo_mi355x_found_serials(out) else None, int(L.aleo_mi355x_found_owned(out)),
                             copy('commitments', np.uint8, 32 * c, (c, 32)) if L.aleo_mi355x_found_commitments(out) else None)
        return found
    finally:
        if keep and found is not None:
            found._native = out; weakref.finalize(found, L.aleo_mi355x_found_free, out)
        else: L.aleo_mi355x_found_free(out)


def decrypt_strings_many(batch, view_keys, addresses, host: bool = False) -> list:
    """decrypt_strings for several accounts over the same RecordBatch (or sequence of strings) in one call (aleo_mi355x_records_decrypt_strings_many / _many_host):
    the text goes up and is parsed once, one grouped scan answers all keys, and the owned (account, record) pairs of all accounts are gathered and decrypted in
    one pass.  Entry j of the list is, byte for byte, what decrypt_strings returns for (view_keys[j], addresses[j]) alone.  1 <= K <= 64; keys may repeat."""
    b = _as_batch(batch)
    if b is None: raise TypeError('decrypt_strings_many takes a RecordBatch or a sequence of strings')
    if len(view_keys) != len(addresses): raise ValueError('view_keys and addresses differ in length')
    k = len(view_keys)
    vk = np.frombuffer(b''.join(view_key_bytes(v) for v in view_keys), dtype=np.uint8); ax = np.frombuffer(b''.join(address_x_bytes(a) for a in addresses), dtype=np.uint8)
    L = lib(); out = (ctypes.c_void_p * max(k, 1))()
    f = L.aleo_mi355x_records_decrypt_strings_many_host if host else L.aleo_mi355x_records_decrypt_strings_many
    check(f(out, _text_p(b), _p(b.offsets), len(b), _p(vk), _p(ax), k), 'records_decrypt_strings_many')
    found = []
    try:
        for j in range(k): found.append(_found_of(L, ctypes.c_void_p(out[j])))
    finally:
        for j in range(len(found) + 1, k): L.aleo_mi355x_found_free(ctypes.c_void_p(out[j]))      # _found_of released the one it was reading
    return found


def _found_many(batch: RecordBatch, accounts):
    """decrypt_strings_many for any number of (view key, address x) pairs: 64 to a call."""
    found = []
    for at in range(0, len(accounts), 64): found += decrypt_strings_many(batch, [vk for vk, _ in accounts[at:at + 64]], [ax for _, ax in accounts[at:at + 64]])
    return found


def balance(ciphertexts, view_key, address):
    """(the sum of the microcredits of the records the account owns, their indices) over a RecordBatch or a sequence of strings: the reference's
    get_unspent_records sum (rust/src/api/blocking.rs:274-283) without the spent check (`unspent` makes it), in one decrypt_strings call.  Only records with
    status 0 count; a string that does not parse raises what RecordCiphertext.from_string raises."""
    b = _as_batch(ciphertexts)
    if b is None: b = RecordBatch.from_strings([str(c) for c in ciphertexts])
    return _balance_of(b, decrypt_strings(b, view_key, address))


def _balance_of(b: RecordBatch, found: FoundRecords):
    if found.unparsed: RecordCiphertext.from_string(b.string(found.first_unparsed))
    return sum(int(v) for v in found.microcredits[found.status == 0]), found.index.tolist()


def balances(ciphertexts, accounts):
    """balance for several accounts over the same records: `accounts` is a sequence of (view_key, address) pairs, the result a list with, for each of them, what
    balance returns — from one decrypt_strings_many call per 64 accounts.  What balance would raise for an account alone is raised, for the first such account."""
    accounts = [(vk, address_x_bytes(a)) for vk, a in accounts]
    b = _as_batch(ciphertexts)
    if b is None: b = RecordBatch.from_strings([str(c) for c in ciphertexts])
    return [_balance_of(b, found) for found in _found_many(b, accounts)]


def decrypt_owned(ciphertexts, view_key, address):
    """[(index, RecordPlaintext)] of the records the account owns: the batch form of the reference's `if record.is_owner(..) { record.decrypt(..) }` loop.
    From strings or a RecordBatch it is one decrypt_strings call and the rendering of the owned records; from RecordCiphertext objects every string is parsed once, one
    scan says which private owners are the account and hands back their record view keys, one decrypt_fields call decrypts the fields of all owned records, and the
    strings are put together on the host.  A record with a public owner equal to the address is included (its owner needs
    no hash; its private entries, if any, do).  An owned record whose decrypted entries do not parse raises."""
    ax = address_x_bytes(address)
    batch = _as_batch(ciphertexts)
    if batch is not None: return _decrypt_owned_strings(batch, view_key, ax)
    recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
    fields = {i: r.fields() for i, r in enumerate(recs) if r.owner_kind == OWNER_PUBLIC and r.owner == ax}      # public owners that match: usually no private field
    scanned = [i for i, r in enumerate(recs) if r.owner_kind == OWNER_PRIVATE or (i in fields and len(fields[i]))]
    rvks = {}
    if scanned:
        c0 = np.frombuffer(b''.join(recs[i].owner for i in scanned), dtype=np.uint8).reshape(-1, 32)
        nx = np.frombuffer(b''.join(recs[i].nonce for i in scanned), dtype=np.uint8).reshape(-1, 32)
        flags, rvk = scan(c0, nx, view_key, ax)
        for j, i in enumerate(scanned):
            if i in fields:
                if flags[j] == 2: raise AleoMi355xError('decrypt_owned: record %d has a nonce that is not on the curve' % i)
                rvks[i] = rvk[j]
            elif flags[j] == 1: rvks[i] = rvk[j]; fields[i] = recs[i].fields()
    return _decrypt_found(recs, fields, rvks, ax)


def decrypt_owned_many(ciphertexts, accounts):
    """decrypt_owned for several accounts over the same records: `accounts` is a sequence of (view_key, address) pairs, the result a list with, for each of them,
    what decrypt_owned returns.  From strings or a RecordBatch it is one decrypt_strings_many call per 64 accounts and the rendering of every account's owned
    records; RecordCiphertext objects take decrypt_owned's road account by account.  What decrypt_owned would raise for an account alone is raised, for the first
    such account."""
    accounts = [(vk, address_x_bytes(a)) for vk, a in accounts]
    batch = _as_batch(ciphertexts)
    if batch is None:
        recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
        return [decrypt_owned(recs, vk, ax) for vk, ax in accounts]
    return [_render_found(batch, found, ax) for found, (_, ax) in zip(_found_many(batch, accounts), accounts)]


def _decrypt_owned_strings(batch: RecordBatch, view_key, ax: bytes):
    """decrypt_owned from strings: one decrypt_strings call finds, gathers and decrypts; the host renders the owned records' strings and nothing else.  What the
    road over scan_strings raised is raised still, in the same order: the first string that does not parse, then per owned record what record_fields refuses or
    the nonce that is not on the curve, then a malformed record, then what record_plaintext refuses."""
    return _render_found(batch, decrypt_strings(batch, view_key, ax), ax)


def _render_found(batch: RecordBatch, found: FoundRecords, ax: bytes):
    if found.unparsed: RecordCiphertext.from_string(batch.string(found.first_unparsed))
    for k, i in enumerate(found.index.tolist()):
        if found.status[k] == 4: RecordCiphertext.from_string(batch.string(i)).fields()
        if found.status[k] == 2 and found.kind[k] == OWNER_PUBLIC: raise AleoMi355xError('decrypt_owned: record %d has a nonce that is not on the curve' % i)
    bad = np.flatnonzero(found.status != 0)
    if len(bad): raise AleoMi355xError('decrypt_owned: record %d is malformed' % int(found.index[bad[0]]))
    return [(i, RecordCiphertext(batch.string(i), int(found.kind[k]), b'', b'').plaintext(found.fields(k), ax)) for k, i in enumerate(found.index.tolist())]


def _decrypt_found(recs, fields, rvks, ax: bytes):
    """The tail of decrypt_owned: fields[i] the private fields of every owned record i, rvks[i] its record view key x (absent where there is no private field)."""
    idx = sorted(fields)
    offsets = np.zeros(len(idx) + 1, dtype=np.uint32)
    if idx: offsets[1:] = np.cumsum([len(fields[i]) for i in idx])
    flat = np.concatenate([fields[i] for i in idx]) if idx else np.zeros((0, 32), dtype=np.uint8)
    zero = np.zeros(32, dtype=np.uint8)
    plain, flags = decrypt_fields(np.stack([rvks.get(i, zero) for i in idx]) if idx else np.zeros((0, 32), dtype=np.uint8), offsets, flat)
    if (flags != 0).any(): raise AleoMi355xError('decrypt_owned: record %d is malformed' % idx[int(np.nonzero(flags)[0][0])])
    return [(i, recs[i].plaintext(plain[offsets[k]:offsets[k + 1]], ax)) for k, i in enumerate(idx)]


def find_owned(ciphertexts, view_key, address):
    """The indices of the records the account owns, and their record view keys' x (32 little-endian bytes each; None for a public owner, whose record is
    not encrypted to anyone): the batch form of the reference's record search.  `ciphertexts`: strings or RecordCiphertext objects; a string that does
    not parse raises."""
    ax = address_x_bytes(address)
    batch = _as_batch(ciphertexts)
    if batch is not None: return _find_owned_strings(batch, [(view_key, ax)])[0]
    recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
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
    accounts = [(vk, address_x_bytes(a)) for vk, a in accounts]
    batch = _as_batch(ciphertexts)
    if batch is not None: return _find_owned_strings(batch, accounts)
    recs = [c if isinstance(c, RecordCiphertext) else RecordCiphertext.from_string(c) for c in ciphertexts]
    priv = [i for i, r in enumerate(recs) if r.owner_kind == OWNER_PRIVATE]
    owned = [{i: None for i, r in enumerate(recs) if r.owner_kind == OWNER_PUBLIC and r.owner == ax} for _, ax in accounts]
    if priv and accounts:
        c0 = np.frombuffer(b''.join(recs[i].owner for i in priv), dtype=np.uint8).reshape(-1, 32)
        nx = np.frombuffer(b''.join(recs[i].nonce for i in priv), dtype=np.uint8).reshape(-1, 32)
        flags, rvk = scan_many(c0, nx, [vk for vk, _ in accounts], [ax for _, ax in accounts])
        for a, mine in enumerate(owned):
            for j in np.nonzero(flags[a] == 1)[0]: mine[priv[j]] = rvk[a, j].tobytes()
    return [(sorted(mine), [mine[i] for i in sorted(mine)]) for mine in owned]


def _find_owned_strings(batch: RecordBatch, accounts):
    """find_owned_many from strings: one scan_strings call; a public owner's record has no record view key (None)."""
    if not accounts:
        _raise_unparsed(batch, parse_many(batch)[0] < 0)
        return []
    flags, kinds, rvk = scan_strings(batch, [vk for vk, _ in accounts], [ax for _, ax in accounts])
    _raise_unparsed(batch, flags[0] == 3)
    out = []
    for a in range(len(accounts)):
        idx = np.flatnonzero(flags[a] == 1).tolist()
        out.append((idx, [rvk[a, i].tobytes() if kinds[i] == OWNER_PRIVATE else None for i in idx]))
    return out


# ---- serial numbers: which of the owned records are unspent ---------------------------------------------------------------------------------------------------
class Account:
    """PrivateKey -> (sk_sig, view key, address): what get_unspent_records is handed (a private key) and what the search and the serial numbers need of it."""

    def __init__(self, private_key: str, sk_sig: bytes, view_key: bytes, address_x: bytes):
        self.private_key, self.sk_sig, self.view_key, self.address_x = private_key, sk_sig, view_key, address_x

    @classmethod
    def from_private_key(cls, private_key: str) -> 'Account':
        sk = np.zeros(32, dtype=np.uint8); vk = np.zeros(32, dtype=np.uint8); ax = np.zeros(32, dtype=np.uint8)
        check(lib().aleo_mi355x_account_from_private_key(private_key.encode(), _p(sk), _p(vk), _p(ax)), 'account_from_private_key')
        return cls(private_key, sk.tobytes(), vk.tobytes(), ax.tobytes())

    @classmethod
    def from_seed(cls, seed: bytes) -> 'Account':
        """`new Account({seed})` of the reference's SDK (sdk/src/account.ts:82): aleo_amd.account.account_from_seed."""
        from . import account
        return account.account_from_seed(seed)

    @classmethod
    def from_ciphertext(cls, ciphertext: str, secret) -> 'Account':
        """PrivateKey.fromPrivateKeyCiphertext (wasm/src/account/private_key.rs:124-130): the account of the key a "ciphertext1…" string holds under a secret;
        raises as aleo_amd.key_ciphertext.decrypt does."""
        from . import key_ciphertext
        return cls.from_private_key(key_ciphertext.decrypt(ciphertext, secret))

    def to_ciphertext(self, secret, nonce=None) -> str:
        """PrivateKey.toCiphertext (wasm/src/account/private_key.rs:113-118): this account's private key encrypted under a secret (aleo_amd.key_ciphertext.encrypt)."""
        from . import key_ciphertext
        if self.private_key is None: raise ValueError('this account holds no private key')
        return key_ciphertext.encrypt(self.private_key, secret, nonce)

    @property
    def view_key_string(self) -> str:
        v = int.from_bytes(_VIEW_KEY_PREFIX + self.view_key, 'big'); out = ''
        while v: v, d = divmod(v, 58); out = _B58[d] + out
        return out

    @property
    def address(self) -> str: return wire.bech32m_encode('aleo', self.address_x)

    def sign(self, message, seed: bytes = None):
        """Account.sign of the reference's SDK (sdk/src/account.ts:195): aleo_amd.signature.sign under this account's private key."""
        from . import signature
        if self.private_key is None: raise ValueError('this account holds no private key')
        return signature.sign(self.private_key, message, seed)

    def sign_many(self, messages, seeds=None, host: bool = False):
        """Account.sign over many messages in one call: aleo_amd.signature.sign_many under this account's private key — (n x 128 rows, flags)."""
        from . import signature
        if self.private_key is None: raise ValueError('this account holds no private key')
        return signature.sign_many(self.private_key, messages, seeds, host)

    def verify(self, message, signature) -> bool:
        """Account.verify (sdk/src/account.ts:211-213): does the signature (a Signature or a "sign1…" string) verify under this account's address?"""
        from . import signature as sg
        return (signature if isinstance(signature, sg.Signature) else sg.Signature.from_string(signature)).verify(self.address_x, message)


_PLAINTEXT_INVALID = 'The record plaintext string provided was invalid'      # RecordPlaintext.fromString's refusal (wasm/src/record/record_plaintext.rs:178)


def _raise_reference_message():
    """The two refusals whose text the reference's tests read are raised with that text alone."""
    L = lib(); msg = L.aleo_mi355x_last_error().decode()
    if msg in ('Invalid ProgramID specified', 'Invalid Identifier specified for record', _PLAINTEXT_INVALID):
        e = AleoMi355xError(msg); e.status = 2
        raise e


def record_commitment(ciphertext, plain_fields, program_id: str, record_name: str) -> bytes:
    """The commitment of a record (32 little-endian bytes): to_commitment(program_id, record_name) of its plaintext, from the "record1…" string and its decrypted
    fields in randomizer order (aleo_mi355x_record_commitment).  A bad program id or record name raises with the reference's message."""
    f = np.ascontiguousarray(plain_fields, dtype=np.uint8).reshape(-1, 32); out = np.zeros(32, dtype=np.uint8)
    rc = lib().aleo_mi355x_record_commitment(_p(out), str(ciphertext).encode(), _p(f) if len(f) else None, f.shape[0], program_id.encode(), record_name.encode())
    if rc: _raise_reference_message()
    check(rc, 'record_commitment')
    return out.tobytes()


def record_checksum(ciphertext) -> bytes:
    """hash_bhp1024 of a record ciphertext's bits (32 little-endian bytes): the "checksum" of a transaction's record output (aleo_mi355x_record_checksum)."""
    out = np.zeros(32, dtype=np.uint8)
    check(lib().aleo_mi355x_record_checksum(_p(out), str(ciphertext).encode()), 'record_checksum')
    return out.tobytes()


def _rows32(rows) -> np.ndarray:
    if isinstance(rows, (bytes, bytearray)): rows = np.frombuffer(bytes(rows), dtype=np.uint8)
    elif isinstance(rows, (list, tuple)): rows = np.frombuffer(b''.join(r if isinstance(r, (bytes, bytearray)) else int(r).to_bytes(32, 'little') for r in rows), dtype=np.uint8)
    return np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 32)


def serial_numbers(commitments, sk_sig, host: bool = False):
    """The serial numbers (uint8[n, 32]) and flags (uint8[n]: 0 computed, 2 refused, its row zeros) of n commitments under one account's sk_sig (32 bytes, or an
    Account): Record::serial_number for a batch (aleo_mi355x_records_serial_numbers / _host).  host=True computes on the CPU, else the library routes."""
    cm = _rows32(commitments); n = cm.shape[0]
    sk = np.frombuffer(sk_sig.sk_sig if isinstance(sk_sig, Account) else view_key_bytes(sk_sig), dtype=np.uint8)
    sn = np.zeros((n, 32), dtype=np.uint8); flags = np.zeros(n, dtype=np.uint8)
    f = lib().aleo_mi355x_records_serial_numbers_host if host else lib().aleo_mi355x_records_serial_numbers
    check(f(_p(sn), _p(flags), _p(cm), n, _p(sk)), 'records_serial_numbers')
    return sn, flags


def found_serial_numbers(found: FoundRecords, commitments, sk_sig, host: bool = False):
    """serial_numbers of the records a decrypt_strings result holds: `commitments` are those of ALL the strings the result was made from (n x 32 bytes); the
    rows at found.index are gathered (what aleo_mi355x_found_serial_numbers does with a result the library still owns)."""
    cm = _rows32(commitments)
    if len(found) and int(found.index.max()) >= cm.shape[0]: raise ValueError('the result was made from more strings than there are commitments')
    return serial_numbers(cm[found.index.astype(np.int64)], sk_sig, host=host)


def unspent(batch, commitments, account, is_spent, host: bool = False):
    """The mirror of the reference's get_unspent_records (rust/src/api/blocking.rs:229-325) over strings already fetched: decrypt_strings for the account, the
    serial numbers of the records found, and of those the ones for which the caller's is_spent(serial number: 32 bytes) is false — the reference asks the chain
    with find_transition_id.  commitments: those of all strings of the batch (the chain's record ids).  Returns ([(index, serial number, microcredits)], their
    sum of microcredits); records whose status is not 0 or whose serial number is refused are dropped, as the reference's `.ok()?` drops them."""
    b = _as_batch(batch)
    if b is None: raise TypeError('unspent takes a RecordBatch or a sequence of strings')
    account = account if isinstance(account, Account) else Account.from_private_key(account)
    found = decrypt_strings(b, account.view_key, account.address_x, host=host)
    if found.unparsed: RecordCiphertext.from_string(b.string(found.first_unparsed))
    sn, flags = found_serial_numbers(found, commitments, account, host=host)
    out = []
    for k, i in enumerate(found.index.tolist()):
        if found.status[k] != 0 or flags[k] != 0: continue
        s = sn[k].tobytes()
        if not is_spent(s): out.append((i, s, int(found.microcredits[k])))
    return out, sum(m for _, _, m in out)


def _unspent_found(b: RecordBatch, commitments, accounts, spent, host: bool) -> list:
    """The call behind unspent_strings[_many]: one FoundRecords per account, unparsed strings counted and not raised.  One account takes the one-account entry."""
    k = len(accounts)
    cm = _rows32(commitments); sp = _rows32(spent)
    if cm.shape[0] < len(b): raise ValueError('fewer commitments than strings')
    if not cm.shape[0]: cm = np.zeros((1, 32), dtype=np.uint8)                                  # no string: a row nobody reads, the pointer is not null
    sk, vk, ax = (np.frombuffer(b''.join(getattr(a, name) for a in accounts), dtype=np.uint8) for name in ('sk_sig', 'view_key', 'address_x'))
    L = lib(); out = (ctypes.c_void_p * max(k, 1))()
    head = (out, _text_p(b), _p(b.offsets), len(b), _p(cm), _p(sk), _p(vk), _p(ax)); tail = (_p(sp) if sp.shape[0] else None, sp.shape[0])
    if k == 1: check((L.aleo_mi355x_records_unspent_strings_host if host else L.aleo_mi355x_records_unspent_strings)(*head, *tail), 'records_unspent_strings')
    else: check((L.aleo_mi355x_records_unspent_strings_many_host if host else L.aleo_mi355x_records_unspent_strings_many)(*head, k, *tail), 'records_unspent_strings_many')
    found = []
    try:
        for j in range(k): found.append(_found_of(L, ctypes.c_void_p(out[j])))
    finally:
        for j in range(len(found) + 1, k): L.aleo_mi355x_found_free(ctypes.c_void_p(out[j]))      # _found_of released the one it was reading
    return found


def unspent_strings_many(batch, commitments, accounts, spent=(), host: bool = False) -> list:
    """The unspent records of several accounts (Account objects or private key strings, at most 64) over the same RecordBatch (or sequence of strings) in ONE
    call (aleo_mi355x_records_unspent_strings_many / _many_host): the search, the decryption, the serial numbers of all accounts' owned records in one launch, and
    the check against `spent` — bytes, an array, or a list of 32-byte serial numbers, in any order — all on the device; only the unspent records come down.
    commitments: those of all strings of the batch.  Entry j is a FoundRecords of account j's records that decrypt (status 0), whose serial number computes and is
    not in `spent`, with .serials and .owned.  A string that does not parse raises, as `unspent` raises."""
    b = _as_batch(batch)
    if b is None: raise TypeError('unspent_strings_many takes a RecordBatch or a sequence of strings')
    found = _unspent_found(b, commitments, [a if isinstance(a, Account) else Account.from_private_key(a) for a in accounts], spent, host)
    if found and found[0].unparsed: RecordCiphertext.from_string(b.string(found[0].first_unparsed))
    return found


def unspent_strings(batch, commitments, account, spent=(), host: bool = False) -> FoundRecords:
    """unspent_strings_many for one account (an Account or a private key string): aleo_mi355x_records_unspent_strings, that call with one key."""
    return unspent_strings_many(batch, commitments, [account], spent, host=host)[0]


def found_commitments(batch, found: FoundRecords, program_id: str, record_name: str, host: bool = False):
    """The commitments (uint8[c, 32]) and flags (uint8[c]: 0 computed; 4 refused as record_commitment refuses the record; a status that is not 0 is the flag;
    a refused row is zeros) of the records a result holds, under (program_id, record_name), from the strings it was made from
    (aleo_mi355x_records_commitments_found / _host).  `found`: a result that still holds the library's copy — decrypt_strings(..., keep=True).  A bad program id
    or record name raises with the reference's message."""
    b = _as_batch(batch)
    if b is None: raise TypeError('found_commitments takes a RecordBatch or a sequence of strings')
    if found._native is None: raise ValueError('found_commitments takes a result made with keep=True')
    c = len(found); cm = np.zeros((c, 32), dtype=np.uint8); flags = np.zeros(c, dtype=np.uint8)
    L = lib(); f = L.aleo_mi355x_records_commitments_found_host if host else L.aleo_mi355x_records_commitments_found
    rc = f(_p(cm), _p(flags), found._native, _text_p(b), _p(b.offsets), len(b), program_id.encode(), record_name.encode())
    if rc: _raise_reference_message()
    check(rc, 'records_commitments_found')
    return cm, flags


def unspent_named_many(batch, program_id: str, record_name: str, accounts, spent=(), host: bool = False) -> list:
    """unspent_strings_many for a caller that has no commitments — the position of the wasm SDK's findUnspentRecords: every owned record's commitment is computed
    from its plaintext under (program_id, record_name), on the device, in front of the serial numbers (aleo_mi355x_records_unspent_named_many / _many_host).
    Entry j is a FoundRecords of account j's unspent records with .serials, .commitments and .owned.  A string that does not parse raises."""
    b = _as_batch(batch)
    if b is None: raise TypeError('unspent_named_many takes a RecordBatch or a sequence of strings')
    accounts = [a if isinstance(a, Account) else Account.from_private_key(a) for a in accounts]
    k = len(accounts); sp = _rows32(spent)
    sk, vk, ax = (np.frombuffer(b''.join(getattr(a, name) for a in accounts), dtype=np.uint8) for name in ('sk_sig', 'view_key', 'address_x'))
    L = lib(); out = (ctypes.c_void_p * max(k, 1))()
    head = (out, _text_p(b), _p(b.offsets), len(b), program_id.encode(), record_name.encode(), _p(sk), _p(vk), _p(ax)); tail = (_p(sp) if sp.shape[0] else None, sp.shape[0])
    if k == 1: rc = (L.aleo_mi355x_records_unspent_named_host if host else L.aleo_mi355x_records_unspent_named)(*head, *tail)
    else: rc = (L.aleo_mi355x_records_unspent_named_many_host if host else L.aleo_mi355x_records_unspent_named_many)(*head, k, *tail)
    if rc: _raise_reference_message()
    check(rc, 'records_unspent_named')
    found = []
    try:
        for j in range(k): found.append(_found_of(L, ctypes.c_void_p(out[j])))
    finally:
        for j in range(len(found) + 1, k): L.aleo_mi355x_found_free(ctypes.c_void_p(out[j]))      # _found_of released the one it was reading
    if found and found[0].unparsed: RecordCiphertext.from_string(b.string(found[0].first_unparsed))
    return found


def unspent_named(batch, program_id: str, record_name: str, account, spent=(), host: bool = False) -> FoundRecords:
    """unspent_named_many for one account (an Account or a private key string): aleo_mi355x_records_unspent_named."""
    return unspent_named_many(batch, program_id, record_name, [account], spent, host=host)[0]


# ---- record plaintext strings: commitments, serial numbers and the spent check from the text alone (csrc/plaintexts.hip) ---------------------------------------
def _plaintext_batch(strings) -> RecordBatch:
    """The blob of a RecordBatch (text plus offsets, as it stands) or of a sequence of strings and RecordPlaintext objects."""
    if isinstance(strings, RecordBatch): return strings
    return RecordBatch.from_strings([str(s) for s in strings])


def plaintext_commitment(plaintext, program_id: str, record_name: str) -> bytes:
    """to_commitment(program_id, record_name) of the record a plaintext string says (32 little-endian bytes), on the host (aleo_mi355x_plaintext_commitment).
    Raises with the reference's three messages: a bad program id, a bad record name, a string that is no record plaintext."""
    out = np.zeros(32, dtype=np.uint8)
    rc = lib().aleo_mi355x_plaintext_commitment(_p(out), str(plaintext).encode(), program_id.encode(), record_name.encode())
    if rc: _raise_reference_message()
    check(rc, 'plaintext_commitment')
    return out.tobytes()


def plaintext_commitments(strings, program_id: str, record_name: str, host: bool = False):
    """The commitments (uint8[n, 32]), microcredits (uint64[n]) and flags (uint8[n]: 0 computed; 3 not a record plaintext, its row zeros) of n plaintext strings
    — a sequence of strings or RecordPlaintext objects, or a RecordBatch — in one call (aleo_mi355x_plaintexts_commitments / _host)."""
    b = _plaintext_batch(strings); n = len(b)
    cm = np.zeros((n, 32), dtype=np.uint8); mc = np.zeros(n, dtype=np.uint64); flags = np.zeros(n, dtype=np.uint8)
    L = lib(); f = L.aleo_mi355x_plaintexts_commitments_host if host else L.aleo_mi355x_plaintexts_commitments
    rc = f(_p(cm), _p(mc), _p(flags), _text_p(b), _p(b.offsets), n, program_id.encode(), record_name.encode())
    if rc: _raise_reference_message()
    check(rc, 'plaintexts_commitments')
    return cm, mc, flags


def plaintext_serial_numbers(strings, program_id: str, record_name: str, account, spent=(), host: bool = False):
    """(serial numbers uint8[n, 32], commitments uint8[n, 32], microcredits uint64[n], flags uint8[n]) of n plaintext strings under one account (an Account, a
    private key string or 32 bytes of sk_sig) and a set of spent serial numbers: flags 0 computed and not in the set, 1 computed and in the set, 2 the serial
    number is refused, 3 not a record plaintext; a row that is not computed is zeros (aleo_mi355x_plaintexts_serial_numbers / _host)."""
    b = _plaintext_batch(strings); n = len(b); sp = _rows32(spent)
    if isinstance(account, str): account = Account.from_private_key(account)
    sk = np.frombuffer(account.sk_sig if isinstance(account, Account) else view_key_bytes(account), dtype=np.uint8)
    sn = np.zeros((n, 32), dtype=np.uint8); cm = np.zeros((n, 32), dtype=np.uint8); mc = np.zeros(n, dtype=np.uint64); flags = np.zeros(n, dtype=np.uint8)
    L = lib(); f = L.aleo_mi355x_plaintexts_serial_numbers_host if host else L.aleo_mi355x_plaintexts_serial_numbers
    rc = f(_p(sn), _p(cm), _p(mc), _p(flags), _text_p(b), _p(b.offsets), n, program_id.encode(), record_name.encode(), _p(sk), _p(sp) if sp.shape[0] else None, sp.shape[0])
    if rc: _raise_reference_message()
    check(rc, 'plaintexts_serial_numbers')
    return sn, cm, mc, flags


def plaintexts_unspent(strings, program_id: str, record_name: str, account, spent=(), host: bool = False):
    """Which of the plaintexts a wallet holds are still unspent: (index uint32[c], serial numbers uint8[c, 32], microcredits uint64[c]) of the strings whose serial
    number computes under the account and is not in `spent` — plaintext_serial_numbers' rows with flag 0."""
    sn, _, mc, flags = plaintext_serial_numbers(strings, program_id, record_name, account, spent, host=host)
    keep = np.flatnonzero(flags == 0)
    return keep.astype(np.uint32), sn[keep], mc[keep]


def plaintexts_last_routed() -> int:
    """How many strings of this thread's last plaintext batch call the host code computed or refused (all of them below aleo_mi355x_min_plaintexts())."""
    return int(lib().aleo_mi355x_plaintexts_last_routed())


# ---- encryption: plaintext strings and randomizers to record1… strings (csrc/records_encrypt.hip) ---------------------------------------------------------------
def record_nonce(randomizer) -> int:
    """x(randomizer G): the _nonce of a record encrypted under this randomizer (aleo_mi355x_record_nonce)."""
    r = np.frombuffer(view_key_bytes(randomizer), dtype=np.uint8); out = np.zeros(32, dtype=np.uint8)
    check(lib().aleo_mi355x_record_nonce(_p(out), _p(r)), 'record_nonce')
    return int.from_bytes(out.tobytes(), 'little')


def encrypt_many(strings, randomizers, set_nonce: bool = False, host: bool = False):
    """n plaintext strings (a sequence of strings or RecordPlaintext objects, or a RecordBatch) under n randomizers (integers, 32-byte strings, or uint8[n, 32]) in one
    call (aleo_mi355x_records_encrypt / _host): (RecordBatch of the record1… strings, flags uint8[n], rvk uint8[n, 32]).  flags: 0 encrypted; 1 x(r G) is not the
    string's nonce (never with set_nonce); 2 the randomizer is not below the subgroup order or the owner is no point of the subgroup; 3 not a record plaintext.  A
    row with a flag is the empty string and a zero rvk.  The batch goes into scan_strings / decrypt_strings as it stands.  Equal randomizers are not looked for."""
    b = _plaintext_batch(strings); n = len(b)
    if isinstance(randomizers, np.ndarray): r = np.ascontiguousarray(randomizers, dtype=np.uint8).reshape(-1, 32)
    else: r = np.frombuffer(b''.join(view_key_bytes(v) for v in randomizers), dtype=np.uint8).reshape(-1, 32)
    if r.shape[0] != n: raise ValueError('one randomizer per string')
    L = lib(); out = ctypes.c_void_p()
    f = L.aleo_mi355x_records_encrypt_host if host else L.aleo_mi355x_records_encrypt
    check(f(ctypes.byref(out), _text_p(b), _p(b.offsets), n, _p(r) if n else None, 1 if set_nonce else 0), 'records_encrypt')
    try:
        offsets = np.frombuffer(ctypes.string_at(L.aleo_mi355x_encrypted_offsets(out), 8 * (n + 1)), dtype=np.uint64).copy()
        total = int(offsets[-1])
        text = ctypes.string_at(L.aleo_mi355x_encrypted_text(out), total) if total else b''
        flags = np.frombuffer(ctypes.string_at(L.aleo_mi355x_encrypted_flags(out), n) if n else b'', dtype=np.uint8).copy()
        rvk = np.frombuffer(ctypes.string_at(L.aleo_mi355x_encrypted_rvk(out), 32 * n) if n else b'', dtype=np.uint8).reshape(n, 32).copy()
    finally: L.aleo_mi355x_encrypted_free(out)
    return RecordBatch(text, offsets), flags, rvk


def encrypt_last_routed() -> int:
    """How many strings of this thread's last encrypt_many the host code encrypted or refused (all of them below aleo_mi355x_min_encrypt())."""
    return int(lib().aleo_mi355x_records_encrypt_last_routed())
