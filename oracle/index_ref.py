"""TEST INFRASTRUCTURE — the index of a circuit (AHPForR1CS::index: the arithmetisation of A, B, C over K and the twelve index commitments)
recomputed on the CPU at the sizes the prover runs (|K| = 2^21 in seconds), independently of the device's key synthesis
(aleo_mi355x_varuna_index_build).  Only tests/ may import this module; the product package never does.

Every rule is the one oracle/varuna_ref.py states (domain_sizes, h_position, Index, _point_bytes); what differs is the arithmetic: numpy arrays
of Montgomery Fr (uint64[n, 4]) through the C oracle (oracle/coracle.py) instead of Python integers, so that varuna_ref.Index and IndexRef agree
value for value where both run (tests/test_index.py) and IndexRef reaches the sizes Index cannot.  The setup is the synthetic one of the
tests (known trapdoor tau): an index commitment is p(tau)·G, so p(tau) — one dot product of the coefficients with a table of tau powers —
replaces the MSM.

Array layouts are the device view's (include/aleo_mi355x.h aleo_mi355x_varuna_index), so a test compares whole buffers:
  k_idx     uint32, matrix after matrix (matrix M from 2·off_M): |K_M| row positions on H, then |K_M| column positions; padding 0
  k_evals   Fr, matrix after matrix (from 4·off_M): row, col, val, row_col on K_M (|K_M| values each); padding row = col = 1, val = 0
  k_polys   the same four polynomials as coefficients (inverse NTT over K_M), same layout
  k2_evals  (from 8·off_M) each polynomial's values on the subgroup of size 2|K_M|, natural order: the first |K_M| coefficients zero-padded
            to 2|K_M| and transformed forward without a coset shift — what varuna_index.hip's p_ntt(..., lg + 1, 4, 0, 0) computes
  vx_inv    1 / v_X(h) for h in H, natural order (h = w_H^p), and 0 on X (where v_X vanishes)
with off_M = |K_A| + ... (the earlier matrices' domains)."""
from __future__ import annotations
import os
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from . import coracle as C
from .varuna_ref import R, domain_sizes, h_position, _point_bytes, vk_points_of

MUL, ADD, SUB = 0, 1, 2
KEYS = ('row', 'col', 'val', 'row_col')


def mont(vals) -> np.ndarray:
    """Python ints -> Montgomery Fr rows."""
    return C.fr_to_mont(C.ints_to_limbs([int(v) % R for v in vals], 4))


def ints(arr) -> list:
    """Montgomery Fr rows -> Python ints."""
    return C.limbs_to_ints(C.fr_from_mont(np.asarray(arr, dtype=np.uint64).reshape(-1, 4)))


def powers(base: int, n: int, threads: int) -> np.ndarray:
    """base^0 .. base^(n-1), Montgomery, n a power of two: a table of base^j (j < B) times a table of base^(iB)."""
    B = 1 << ((n.bit_length() - 1) // 2)
    lo, hi, a = [], [], 1
    for _ in range(B): lo.append(a); a = a * base % R
    b = 1
    for _ in range(n // B): hi.append(b); b = b * a % R
    return C.fr_vec_op_mt(np.tile(mont(lo), (n // B, 1)), np.repeat(mont(hi), B, axis=0), MUL, threads)


def _ntt(a, direction, threads):
    return C.ntt_fr(a, 0, direction, 0, threads=threads)


def canonical_rows(row_ptr, col, val):
    """(col, val) of a CSR matrix with each row's entries sorted by (column, value): the order inside a row of the device's transpose is
    whatever its atomic cursors made it, the row as a multiset is fixed."""
    rp = np.asarray(row_ptr, dtype=np.int64); col = np.asarray(col); val = np.asarray(val, dtype=np.uint64).reshape(-1, 4)
    key = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)) * (int(col.max()) + 1 if len(col) else 1) + col
    order = np.argsort(key, kind='stable'); k = key[order]
    dup = np.flatnonzero(k[1:] == k[:-1])
    if dup.size:                                                                # one variable twice in a constraint: those runs by value
        at = np.unique(np.concatenate([dup, dup + 1])); sub = order[at]; v = val[sub]
        order[at] = sub[np.lexsort((v[:, 3], v[:, 2], v[:, 1], v[:, 0], key[sub]))]
    return col[order], val[order]


class IndexRef:
    """The index of one circuit.  csr[m] = (row_ptr uint32[n_constraints + 1], col uint32[nnz] variable indices, val uint64[nnz, 4] canonical)
    for m in 'abc' — what NativeCircuitIndex takes.  domains: 'auto', 'shared' or 'per_matrix' (varuna_ref.domain_sizes)."""

    def __init__(self, csr, n_constraints: int, n_public: int, n_private: int, tau: int, max_degree: int, domains: str = 'auto', threads: int = None):
        self.threads = T = threads or min(16, os.cpu_count() or 1)
        self.n_constraints, self.n_public, self.n_private = n_constraints, n_public, n_private
        self.csr = {m: (np.asarray(csr[m][0], dtype=np.int64), np.asarray(csr[m][1], dtype=np.int64), np.asarray(csr[m][2], dtype=np.uint64).reshape(-1, 4)) for m in 'abc'}
        for m, (rp, col, val) in self.csr.items():
            assert len(rp) == n_constraints + 1 and rp[0] == 0 and (np.diff(rp) >= 0).all() and len(col) == rp[-1] == len(val), m
            assert not len(col) or col.max() < n_public + n_private, m
        self.nnz = {m: len(self.csr[m][1]) for m in 'abc'}
        self.n_x, self.n_h, nkm = domain_sizes(n_constraints, n_public, n_private, self.nnz, domains)
        self.n_k_m = [nkm[m] for m in 'abc']
        self.k_off = [0, self.n_k_m[0], self.n_k_m[0] + self.n_k_m[1]]; self.k_sum = sum(self.n_k_m)
        assert 3 * self.n_h <= max_degree + 1 and max(self.n_k_m) <= max_degree + 1, 'committer key too small for this circuit'
        n_h, n_vars = self.n_h, n_public + n_private
        self.positions = np.fromiter((h_position(v, n_public, self.n_x, n_h) for v in range(n_vars)), dtype=np.int64, count=n_vars).astype(np.uint32)
        e1 = np.zeros((n_h, 4), dtype=np.uint64); e1[1] = mont([1])[0]
        self.h_elems = _ntt(e1, 0, T)                                            # w_H^p, p < |H|: the transform of the polynomial X
        one, nh_inv = mont([1])[0], mont([pow(n_h, -1, R)])[0]
        self.k_idx = np.zeros(2 * self.k_sum, dtype=np.uint32)
        self.k_evals = np.zeros((4 * self.k_sum, 4), dtype=np.uint64)
        self.rows, self.cols = {}, {}
        for k, m in enumerate('abc'):
            rp, col, val = self.csr[m]; nk, o, nz = self.n_k_m[k], self.k_off[k], self.nnz[m]
            r = np.repeat(np.arange(n_constraints, dtype=np.int64), np.diff(rp)); cp = self.positions[col].astype(np.int64)
            self.rows[m], self.cols[m] = r, cp
            self.k_idx[2 * o:2 * o + nz] = r; self.k_idx[2 * o + nk:2 * o + nk + nz] = cp
            ev = self.k_evals[4 * o:4 * o + 4 * nk].reshape(4, nk, 4)
            ev[0] = one; ev[1] = one                                             # padding: row = col = 1 (position 0), val = 0
            ev[0, :nz] = self.h_elems[r]; ev[1, :nz] = self.h_elems[cp]
            v = C.fr_vec_op_mt(C.fr_to_mont(val), ev[1, :nz], MUL, T)          # M[r,c] / u_H(col, col) = M[r,c] col / |H|
            ev[2, :nz] = C.fr_vec_op_mt(v, np.broadcast_to(nh_inv, v.shape), MUL, T)
            ev[3] = C.fr_vec_op_mt(ev[0], ev[1], MUL, T)
        self.k_polys = np.zeros_like(self.k_evals)
        for k in range(3):
            nk, o = self.n_k_m[k], self.k_off[k]
            for j in range(4):
                at = 4 * o + j * nk
                self.k_polys[at:at + nk] = _ntt(self.k_evals[at:at + nk], 1, T)
        # the commitment scalars p(tau): one single-row sparse product per polynomial against the powers of tau
        taus = powers(tau % R, max(self.n_k_m), T)
        def dot(kj):
            k, j = kj; nk = self.n_k_m[k]; at = 4 * self.k_off[k] + j * nk
            return C.fr_spmv(np.array([0, nk], dtype=np.uint32), np.arange(nk, dtype=np.uint32), self.k_polys[at:at + nk], taus[:nk])[0]
        with ThreadPoolExecutor(T) as ex: sc = list(ex.map(dot, [(k, j) for k in range(3) for j in range(4)]))
        self.commit_scalars = {(m, key): s for (m, key), s in zip([(m, key) for m in 'abc' for key in KEYS], ints(np.stack(sc)))}

    def evals(self, m: str, key: str) -> np.ndarray:
        k, j = 'abc'.index(m), KEYS.index(key); nk = self.n_k_m[k]; at = 4 * self.k_off[k] + j * nk
        return self.k_evals[at:at + nk]

    def polys(self, m: str, key: str) -> np.ndarray:
        k, j = 'abc'.index(m), KEYS.index(key); nk = self.n_k_m[k]; at = 4 * self.k_off[k] + j * nk
        return self.k_polys[at:at + nk]

    def vk_bytes(self) -> bytes:
        """Index.vk_bytes: the twelve compressed commitments, then |H|, |K_A|, |K_B|, |K_C|, |X| as u64 LE (616 bytes)."""
        if getattr(self, '_vk', None) is None:
            out = b''.join(_point_bytes(self.commit_scalars[(m, key)]) for m in 'abc' for key in KEYS)
            self._vk = out + b''.join(int(v).to_bytes(8, 'little') for v in (self.n_h, *self.n_k_m, self.n_x))
        return self._vk

    def vk_affine(self) -> np.ndarray:
        """The twelve commitments as uint8[12, 104] G1Affine (Montgomery coordinates, infinity byte)."""
        return C.affine_from_ints(vk_points_of(self.vk_bytes()))

    def k2_evals(self, k: int) -> np.ndarray:
        """Matrix k's block of k2_evals (8 |K_M| values: row, col, val, row_col on the subgroup of size 2 |K_M|)."""
        nk, o = self.n_k_m[k], self.k_off[k]
        out = np.zeros((8 * nk, 4), dtype=np.uint64)
        for j in range(4):
            a = np.zeros((2 * nk, 4), dtype=np.uint64); a[:nk] = self.k_polys[4 * o + j * nk:4 * o + (j + 1) * nk]
            out[2 * j * nk:2 * (j + 1) * nk] = _ntt(a, 0, self.threads)
        return out

    def vx_inv(self) -> np.ndarray:
        """1 / v_X(w_H^p) = 1 / (w_X'^p − 1) with w_X' = w_H^|X| of order |H| / |X|: the values repeat with that period, 0 where p is a multiple of it."""
        period = self.n_h // self.n_x
        v = self.h_elems[(np.arange(period, dtype=np.int64) * self.n_x) % self.n_h]
        v = C.fr_batch_inverse_mt(C.fr_vec_op_mt(v, np.broadcast_to(mont([1])[0], v.shape), SUB, self.threads), self.threads)
        return np.tile(v, (self.n_x, 1))

    def forward(self, m: str):
        """A or B as the prover reads it: (row_ptr padded to |H| + 1 entries, columns as positions on H, values in Montgomery form)."""
        rp, col, val = self.csr[m]
        p = np.full(self.n_h + 1, rp[-1], dtype=np.uint32); p[:len(rp)] = rp
        return p, self.positions[col], C.fr_to_mont(val)

    def transpose(self):
        """The stacked transpose [A^T | B^T | C^T] over H: row p lists every use of the variable at position p as (M·|H| + constraint, value);
        (row_ptr, col, val) with each row in canonical_rows order."""
        pos = np.concatenate([self.cols[m] for m in 'abc'])
        col = np.concatenate([self.rows[m] + k * self.n_h for k, m in enumerate('abc')]).astype(np.uint32)
        val = C.fr_to_mont(np.concatenate([self.csr[m][2] for m in 'abc']))
        order = np.argsort(pos, kind='stable')
        rp = np.zeros(self.n_h + 1, dtype=np.uint32); rp[1:] = np.cumsum(np.bincount(pos, minlength=self.n_h))
        return (rp,) + canonical_rows(rp, col[order], val[order])

    def max_row(self):
        """The longest row of A, B and of the stacked transpose, at least 1 (the prover's hints for its sparse products)."""
        lens = [np.diff(self.csr[m][0]) for m in 'ab'] + [np.bincount(np.concatenate([self.cols[m] for m in 'abc']), minlength=1)]
        return [max(1, int(x.max()) if len(x) else 0) for x in lens]
