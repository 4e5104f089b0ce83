"""A restatement of aleo_amd/csrc/plaintext_parse.hpp in Python integers: the grammar of a RecordPlaintext string, the RECORD BITS it comes to and its commitment
over serial_ref.py's BHP1024.  Written from the header's grammar with a regular-expression tokenizer, so that it shares no walk with the C++ reader.
parse(s) -> (owner_private, owner x, [(name, visibility, value)], nonce x) or raises Refused; a value is ('lit', type, python value) or ('struct', [(name, value)])
as tests/test_records_decrypt.py writes them."""
import re
import serial_ref as S
from oracle import poseidon as P

R = S.R
SCALAR_MODULUS = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff
SUFFIX = {'field': 2, 'group': 3, 'scalar': 14, **{'i%d' % (8 << i): 4 + i for i in range(5)}, **{'u%d' % (8 << i): 9 + i for i in range(5)}}
BITS = {0: 253, 1: 1, 2: 253, 3: 253, 14: 251, **{4 + i: 8 << i for i in range(5)}, **{9 + i: 8 << i for i in range(5)}}
VIS = ['constant', 'public', 'private']
MAX_DEPTH, MAX_ENTRIES, MAX_STRING = 32, 255, 8191
_B32 = 'qpzry9x8gf2tvdw0s3jn54khce6mua7l'
_TOKEN = re.compile(r'[ \t\r\n]*(?:(?P<punct>[{}:,])|(?P<string>"[^"]*")|(?P<word>[-A-Za-z0-9_]+))')
_VISIBILITY = re.compile(r'\.([A-Za-z0-9_]*)')


class Refused(Exception): pass


def _polymod(values):
    chk = 1
    for v in values:
        b = chk >> 25
        chk = ((chk & 0x1ffffff) << 5) ^ v
        for i, g in enumerate((0x3b6a57b2, 0x26508e6d, 0x1ea119fa, 0x3d4233dd, 0x2a1462b3)):
            if (b >> i) & 1: chk ^= g
    return chk


def address_x(text: str) -> int:
    if len(text) != 63 or not text.startswith('aleo1') or any(c not in _B32 for c in text[5:]): raise Refused('address')
    data = [_B32.index(c) for c in text[5:]]
    if _polymod([ord(c) >> 5 for c in 'aleo'] + [0] + [ord(c) & 31 for c in 'aleo'] + data) != 0x2bc830a3: raise Refused('checksum')
    v = 0
    for d in data[:-6]: v = (v << 5) | d                        # 260 bits, big-endian: 32 bytes and 4 zero bits
    if v & 15: raise Refused('padding')
    x = int.from_bytes((v >> 4).to_bytes(32, 'big'), 'little')
    if x >= R: raise Refused('address not below r')
    return x


class _Reader:
    def __init__(self, s): self.s, self.at = s, 0

    def token(self):
        m = _TOKEN.match(self.s, self.at)
        if not m: return None, None
        self.at = m.end()
        return m.lastgroup, m.group(m.lastgroup)

    def peek(self):
        at = self.at; t = self.token(); self.at = at
        return t

    def expect(self, punct):
        kind, text = self.token()
        if kind != 'punct' or text != punct: raise Refused('expected ' + punct)

    def visibility(self):
        m = _VISIBILITY.match(self.s, self.at)
        if not m or m.group(1) not in VIS: raise Refused('visibility')
        self.at = m.end()
        return VIS.index(m.group(1))

    def literal(self):
        kind, text = self.token()
        if kind == 'string':
            body = text[1:-1]
            if any(ord(c) < 0x20 or ord(c) == 0x7f for c in body) or len(body.encode()) > MAX_STRING: raise Refused('string')
            return ('lit', 15, body), self.visibility()
        if kind != 'word': raise Refused('no literal')
        if text.startswith('aleo'): return ('lit', 0, address_x(text)), self.visibility()
        if text in ('true', 'false'): return ('lit', 1, text == 'true'), self.visibility()
        m = re.fullmatch(r'(-?)([0-9][0-9_]*)([a-z][a-z0-9]*)', text)
        if not m or m.group(3) not in SUFFIX: raise Refused('literal')
        ty, v = SUFFIX[m.group(3)], int(m.group(2).replace('_', ''))
        if v >= 1 << 256: raise Refused('too large')
        signed = 4 <= ty <= 8
        if m.group(1):
            if not signed: raise Refused('sign')
            v = -v
        lo, hi = (-(1 << (BITS[ty] - 1)), 1 << (BITS[ty] - 1)) if signed else (0, R if ty in (2, 3) else SCALAR_MODULUS if ty == 14 else 1 << BITS[ty])
        if not lo <= v < hi: raise Refused('range')
        return ('lit', ty, v), self.visibility()

    def name(self):
        kind, text = self.token()
        if kind != 'word' or not S.identifier_ok(text): raise Refused('name')
        return text

    def value(self, vis, depth):
        """(value, the visibility of its literals); vis: what the entry's earlier literals said, or None."""
        if self.peek() == ('punct', '{'):
            if depth >= MAX_DEPTH: raise Refused('depth')
            self.token(); members = []
            while True:
                name = self.name()
                if name in [n for n, _ in members]: raise Refused('duplicate member')
                self.expect(':')
                member, vis = self.value(vis, depth + 1)
                members.append((name, member))
                if len(members) > 255: raise Refused('members')
                kind, text = self.token()
                if (kind, text) == ('punct', '}'): return ('struct', members), vis
                if (kind, text) != ('punct', ','): raise Refused('struct')
        lit, mine = self.literal()
        if vis is not None and vis != mine: raise Refused('mixed visibility')
        return lit, mine


def parse(s: str):
    r = _Reader(s)
    r.expect('{')
    if r.token() != ('word', 'owner'): raise Refused('owner')
    r.expect(':')
    owner, vis = r.literal()
    if owner[1] != 0 or vis == 0: raise Refused('owner')
    r.expect(',')
    entries = []
    while True:
        if r.peek() == ('word', '_nonce'):
            r.token(); r.expect(':')
            nonce, nvis = r.literal()
            if nonce[1] != 3 or nvis != 1: raise Refused('nonce')
            break
        name = r.name()
        if name == 'owner' or name in [n for n, _, _ in entries] or len(entries) == MAX_ENTRIES: raise Refused('entry name')
        r.expect(':')
        value, evis = r.value(None, 0)
        r.expect(',')
        entries.append((name, evis, value))
    r.expect('}')
    if s[r.at:].strip(' \t\r\n'): raise Refused('trailing text')
    return vis == 2, owner[2], entries, nonce[2]


def value_bits(val):
    if val[0] == 'lit':
        ty, v = val[1], val[2]
        if ty == 15: b = v.encode(); return [0, 0] + S.bits_le(ty, 8) + S.bits_le(8 * len(b), 16) + S.bytes_bits(b)
        return [0, 0] + S.bits_le(ty, 8) + S.bits_le(BITS[ty], 16) + S.bits_le(int(v) & ((1 << BITS[ty]) - 1), BITS[ty])
    out = [0, 1] + S.bits_le(len(val[1]), 8)
    for name, member in val[1]:
        inner = value_bits(member)
        if len(inner) > 65535: raise Refused('member too long')
        out += S.bits_le(8 * len(name), 8) + S.bytes_bits(name.encode()) + S.bits_le(len(inner), 16) + inner
    return out


def record_bits(s: str):
    private, owner, entries, nonce = parse(s)
    data = []
    for name, vis, value in entries: data += S.bytes_bits(name.encode()) + [int(vis == 2), int(vis == 1)] + value_bits(value)
    return [int(private)] + S.bits_le(owner, 253) + S.bits_le(len(data), 32) + data + S.bits_le(nonce, 253)


def microcredits(s: str) -> int:
    for name, _, value in parse(s)[2]:
        if name == 'microcredits': return value[2] if value[:2] == ('lit', 12) else 0
    return 0


def commitment(s: str, program_id: str, record_name: str) -> int:
    name, network = S.program_id_parts(program_id)
    assert S.identifier_ok(record_name)
    return S.bhp1024().hash(S.bytes_bits(name.encode()) + S.bytes_bits(network.encode()) + S.bytes_bits(record_name.encode()) + record_bits(s))
