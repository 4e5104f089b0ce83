"""A restatement, in Python integers, of the reference's private key encryption (Encryptor::encrypt_private_key_with_secret, rust/src/account/encryptor.rs:26-43,
over snarkVM 0.14.5's Plaintext::to_fields and Ciphertext [UPSTREAM-RECALL]): bits, fields, randomizers, bech32m — over oracle.poseidon's hash_many and
domain_separator and oracle.pyref's bech32m_encode.  Pinned by the reference's own known answer (tests/test_key_ciphertexts.py: with the nonce recovered from the
reference's ciphertext it reproduces that string byte for byte), and inverted by oracle.poseidon.decrypt_private_key, which no test here wrote.
A secret is bytes (or a str: its UTF-8 bytes).  The builders at the end craft plaintexts the library must refuse."""
from oracle import poseidon as ps
from oracle import pyref as P

R = ps.R
DATA_BITS = ps.FR_DATA_BITS                                     # 252


def sep(b) -> int:
    """Field::new_domain_separator: the bytes, little-endian, mod r."""
    return int.from_bytes(b.encode() if isinstance(b, str) else bytes(b), 'little') % R


def bits_le(v: int, n: int): return [(v >> i) & 1 for i in range(n)]


def literal_field_bits(v: int):
    """Plaintext::Literal(Field) to_bits_le: variant 0,0 | type u8 | size u16 | the 253 bits of the value."""
    return [0, 0] + bits_le(ps.LITERAL_FIELD, 8) + bits_le(253, 16) + bits_le(v, 253)


def struct_bits(members):
    """Plaintext::Struct to_bits_le: variant 0,1 | member count u8 | per member: name size in bits u8, name, value size u16, value.  members: [(name, value bits)]."""
    out = [0, 1] + bits_le(len(members), 8)
    for name, value in members:
        raw = name.encode()
        out += bits_le(8 * len(raw), 8) + bits_le(int.from_bytes(raw, 'little'), 8 * len(raw)) + bits_le(len(value), 16) + list(value)
    return out


def fields_of_bits(bits):
    """Plaintext::to_fields: the bits, the terminus 1, cut into fields of 252 bits, the last one padded with zeros."""
    bits = list(bits) + [1]
    return [sum(b << i for i, b in enumerate(bits[at:at + DATA_BITS])) for at in range(0, len(bits), DATA_BITS)]


def randomizers(s: int, n: int): return ps.hash_many(8, [ps.domain_separator('AleoSymmetricEncryption0'), s], n)


def blinding(nonce: int, s: int) -> int: return ps.hash_many(2, [ps.domain_separator('private_key'), nonce, s], 1)[0]


def ciphertext_string(fields) -> str:
    return P.bech32m_encode('ciphertext', len(fields).to_bytes(2, 'little') + b''.join(f.to_bytes(32, 'little') for f in fields))


def encrypt_fields(plain, secret) -> str:
    """Ciphertext of given plaintext fields under sep(secret): c_i = p_i + randomizer_i."""
    rnd = randomizers(sep(secret), len(plain))
    return ciphertext_string([(p + r) % R for p, r in zip(plain, rnd)])


def key_plaintext_bits(key: int, nonce: int):
    return struct_bits([('key', literal_field_bits(key)), ('nonce', literal_field_bits(nonce))])


def encrypt(seed: int, secret, nonce: int) -> str:
    """The "ciphertext1…" string of the private key with this seed."""
    key = blinding(nonce, sep(secret)) * seed % R
    return encrypt_fields(fields_of_bits(key_plaintext_bits(key, nonce)), secret)


def encrypt_bits(bits, secret, terminus=True, n_fields=None) -> str:
    """A ciphertext of arbitrary plaintext bits (terminus=False: the bits as they are, padded with zeros to whole fields)."""
    if terminus: plain = fields_of_bits(bits)
    else: plain = [sum(b << i for i, b in enumerate(bits[at:at + DATA_BITS])) for at in range(0, max(len(bits), 1), DATA_BITS)]
    while n_fields and len(plain) < n_fields: plain.append(0)
    return encrypt_fields(plain, secret)
