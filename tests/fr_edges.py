"""Edge operands for the 32-bit-limb Fr vector kernels (frops.hip, fr_spmv.hip, fr_divide.hip, ahp_kernels.hip), shared by tests/test_gpu_fr_edges.py and
tests/test_fr_edge_inputs.py.  A plain module: no fixtures.

Everything here lives in the STORED (Montgomery) domain, because what matters is the limb pattern a kernel loads: a stored value x stands for x / 2^256 mod r.
The reference product is x (*) y = x y 2^-256 mod r on Python integers (`mmul`), sums and differences are plain mod r, and an expected output is the canonical
stored value, compared bit for bit.  `redc_lazy` is the integer model of the device's lazily reduced product (fp.h: no final subtraction), which
tests/test_fr_edge_inputs.py uses to show that the cancelling rows built here do land a kernel's running sum on exactly r and exactly 2r."""
import random
import numpy as np

R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
W = 1 << 256
RINV = pow(W, -1, R)
ONE = W % R                                                 # the stored form of 1
_NPRIME = (-pow(R, -1, W)) % W


def mmul(x, y): return x * y * RINV % R                     # the stored form of the product of what x and y stand for
def msolve(t, y): return t * W * pow(y, -1, R) % R          # the x with x (*) y = t (y != 0)
def minv(x): return pow(x, -1, R) * W * W % R               # the stored form of the inverse of what x stands for (x != 0)
def stored(v): return v * W % R                             # abstract value -> stored value
def redc_lazy(a, b):                                        # (ab + m r) / 2^256 with m = -ab / r mod 2^256: what Fr::mul leaves, below (ab / 2^256 + r)
    ab = a * b
    return (ab + (ab % W) * _NPRIME % W * R) >> 256


# Canonical stored values at which a limb, a carry chain or a conditional subtraction sits at an end of its range.
E = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2,
     (1 << 32) - 1, 1 << 32, (1 << 64) - 1, (1 << 128) - 1, (1 << 252) - 1, 1 << 252,
     ONE, R - ONE,
     (0x12ab655d << 224) | ((1 << 224) - 1),                # the largest value below r whose seven low limbs are all ones
     R - (1 << 32), R - (1 << 224)]
E_NONZERO = [v for v in E if v]


def cycle(vals, n, start=0, step=1): return [vals[(start + i * step) % len(vals)] for i in range(n)]


def edge_pairs(min_rows=257):
    """All ordered pairs of E as two lists, cycled until there are at least min_rows (more than one block of 256 lanes)."""
    pairs = [(x, y) for x in E for y in E]
    n = max(min_rows, len(pairs))
    return cycle([q[0] for q in pairs], n), cycle([q[1] for q in pairs], n)


def edge_triples():
    """All ordered triples of E as three lists (5832 rows)."""
    t = [(x, y, z) for x in E for y in E for z in E]
    return [q[0] for q in t], [q[1] for q in t], [q[2] for q in t]


def uniform(n, seed, nonzero=False):
    rng = random.Random(seed)
    return [rng.randrange(1 if nonzero else 0, R) for _ in range(n)]


CANCEL_ROWS = 2048
def targets(n=CANCEL_ROWS, neighbours=8):
    """What the true results of n + neighbours cancelling rows are: 0 for the first n, then 1 and r - 1 in turn (the two neighbours of 0)."""
    return [0] * n + [1, R - 1] * (neighbours // 2)


# Long carries.  (a, b, k): a + b resp. a - b carries (borrows) out of every one of the k / 32 low limbs.
CARRY_ADD = [((1 << k) - 1, 1, k) for k in range(32, 225, 32)]
CARRY_SUB = [(1 << k, 1, k) for k in range(32, 225, 32)]


def limbs32(v, n=8): return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def carry_limbs(a, b):
    """The limbs out of which the limb-wise sum a + b carries."""
    out, c = [], 0
    for i, (x, y) in enumerate(zip(limbs32(a), limbs32(b))):
        c = (x + y + c) >> 32
        if c: out.append(i)
    return out


def borrow_limbs(a, b):
    """The limbs out of which the limb-wise difference a - b borrows."""
    out, br = [], 0
    for i, (x, y) in enumerate(zip(limbs32(a), limbs32(b))):
        br = 1 if x - y - br < 0 else 0
        if br: out.append(i)
    return out


def lin_one_term_cancelling(n=CANCEL_ROWS, seed=0xF1E1D):
    """Rows (c0, c1, a) of dst = c0 + c1 a, uniform c1 and a (c1 != 0), with c0 = -(c1 (*) a): the true result is 0, so the kernel's lazy sum
    c0 + redc(c1, a) is a multiple of r.  (c0 and c1 are constants of a launch: every row is a launch of its own.)"""
    c1, a = uniform(n, seed, nonzero=True), uniform(n, seed + 1)
    return [((-mmul(k, x)) % R, k, x) for k, x in zip(c1, a)]


def lazy_sum_counts(rows):
    """How many of those rows put c0 + redc(c1, a) on exactly r, and on exactly 2r."""
    sums = [c0 + redc_lazy(c1, a) for c0, c1, a in rows]
    return sum(s == R for s in sums), sum(s == 2 * R for s in sums)


# ---- integers <-> limb arrays -------------------------------------------------------------------------------------------------------------------------------
def limbs(vals, words=4):
    """uint64[n, words] little-endian limbs of a list of integers."""
    if not len(vals): return np.zeros((0, words), dtype=np.uint64)
    return np.frombuffer(b''.join(int(v).to_bytes(8 * words, 'little') for v in vals), dtype=np.uint64).reshape(-1, words).copy()


def ints(arr):
    """The integers of uint64[n, words] little-endian limbs."""
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    if arr.ndim == 1: arr = arr[None, :]
    raw, step = arr.tobytes(), 8 * arr.shape[1]
    return [int.from_bytes(raw[i:i + step], 'little') for i in range(0, len(raw), step)]
