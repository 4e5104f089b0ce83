"""The circuit index (key synthesis: aleo_mi355x_varuna_index_build, and the step-by-step CircuitIndex of aleo_amd/varuna.py) against an independent
CPU reference, oracle/index_ref.py, at the sizes the prover runs.  Proofs alone cannot judge an index: a verifier handed the verifying key of a wrong
index accepts valid proofs of that wrong circuit.  So every exported array is compared with the reference — the verifying key, the positions on H,
the forward and transposed matrices, 1 / v_X, the arithmetisation over K (indices, evaluations, coefficients, values on 2K) and the sparse-product
hints.  CPU: the reference equals the restatement's Index (oracle/varuna_ref.py) wherever that one runs."""
import ctypes, zlib
import numpy as np
import pytest
from aleo_amd import synth
from oracle import varuna_ref as V, index_ref as IR

TAU, S_GAMMA = 0x1F3A9C0D5E7B24681357ACE02468BDF013579BDF02468ACE1234567, 0x0FEDCBA9876543210123456789ABCDEF55AA
D = (1 << 22) - 1                      # one committer key for every shape: 3 |H| <= 2^22 at 2^20 constraints


def _rows(csr, m, n):
    ptr, col, val = csr[m]
    return [[(int(col[k]), synth.limbs_to_int(val[k])) for k in range(ptr[i], ptr[i + 1])] for i in range(n)]


def _lens(rng, n, nnz, fixed=None):
    """Row lengths of n rows summing to nnz: the rows in `fixed` as given, the rest a random split (so: empty rows, a few long ones)."""
    fixed = fixed or {}
    free = np.array([i for i in range(n) if i not in fixed]) if fixed else np.arange(n)
    rest = nnz - sum(fixed.values()); assert rest >= 0
    cuts = np.sort(rng.integers(0, rest + 1, len(free) - 1))
    lens = np.zeros(n, dtype=np.int64); lens[free] = np.diff(np.concatenate([[0], cuts, [rest]]))
    for i, v in fixed.items(): lens[i] = v
    return lens


def _matrix(rng, lens, n_vars, seed):
    """CSR with random columns and values: canonical uniform scalars with zeros, ones and -1 mixed in."""
    rp = np.zeros(len(lens) + 1, dtype=np.uint32); rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    col = rng.integers(0, n_vars, nnz).astype(np.uint32)
    val = synth.uniform_scalars(nnz, seed)
    val[::7] = 0; val[3::11] = 0; val[3::11, 0] = 1; val[5::13] = synth.int_to_limbs(V.R - 1, 4)
    return rp, col, val


def _one_per_row(n, first_var):
    """C of a compiled program: row i assigns the new variable first_var + i."""
    return np.arange(n + 1, dtype=np.uint32), np.arange(first_var, first_var + n, dtype=np.uint32), np.tile(synth.int_to_limbs(1, 4), (n, 1))


# ---- the shapes: (csr, n_constraints, n_public, n_private, domains, what the shape must have) -------------------------------------------------------
def _shape(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == 'synthetic_2_15':                       # compiled-program shape with long linear combinations; shared K
        n = (1 << 15) - 64; csr, z = synth.synthetic_r1cs(n, 3, 911, long_rows=4)
        return csr, n, 3, len(z) - 3, 'auto', {'shared': True}
    if name == 'bits_2_15':                            # NOT gates on the constant: a transposed row of > 8192 entries
        n = (1 << 15) - 64; csr, z = synth.synthetic_r1cs_bits(n, 4, 912)
        return csr, n, 4, len(z) - 4, 'auto', {'shared': True, 't_row_over': 8192}
    if name == 'edges':
        # |H| set by |X| + n_private (not by the constraints); empty rows; most variables unused; one variable 100 times in one row, another twice;
        # A rows longer than 64 and one longer than 8192; nnz(A) exactly 2^15, nnz(B) = 2^14 + 1, C without a single non-zero
        n, n_pub, n_priv = 3000, 5, 40000
        la = _lens(rng, n, 1 << 15, {0: 0, 1: 9000, **{i: 100 for i in range(2, 10)}})
        a = _matrix(rng, la, n_pub + n_priv, 921); b = _matrix(rng, _lens(rng, n, (1 << 14) + 1, {0: 0}), n_pub + n_priv, 922)
        a[1][a[0][3]:a[0][4]] = 7; a[1][a[0][4]:a[0][4] + 2] = n_pub + 11
        c = (np.zeros(n + 1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
        return {'a': a, 'b': b, 'c': c}, n, n_pub, n_priv, 'auto', {'shared': True, 'n_h': 1 << 16, 'a_row_over': 8192, 'nnz': [1 << 15, (1 << 14) + 1, 0]}
    if name == 'long_transpose':
        # the constant 1 in every row of B and in the long rows of A: one transposed row of > 2 x 10^4 entries; an A row of 8193; nnz(A) = 2^17,
        # the largest non-zero count that keeps the automatic choice on one shared K
        n, n_pub = (1 << 14) + 100, 2
        a = _matrix(rng, _lens(rng, n, 1 << 17, {5: 8193, **{i: 65 for i in range(10, 40)}}), n_pub + n, 931)
        a[1][a[0][5]:a[0][5] + 3000] = 0
        b = (np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32), synth.uniform_scalars(n, 932))
        return {'a': a, 'b': b, 'c': _one_per_row(n, n_pub)}, n, n_pub, n, 'auto', {'shared': True, 'n_k': [1 << 17] * 3, 'a_row_over': 8192, 't_row_over': 10000}
    if name == 'switch_2_17p1':                        # one non-zero over 2^17: |K_A| = 2^18 and the automatic switch to one domain per matrix
        n, n_pub = (1 << 16) - 10, 4
        a = _matrix(rng, _lens(rng, n, (1 << 17) + 1), n_pub + n, 941); b = _matrix(rng, _lens(rng, n, 1 << 16), n_pub + n, 942)
        c = _matrix(rng, _lens(rng, n, (1 << 15) - 1), n_pub + n, 943)
        return {'a': a, 'b': b, 'c': c}, n, n_pub, n, 'auto', {'shared': False, 'n_k': [1 << 18, 1 << 16, 1 << 15]}
    if name == 'shared_2_18m1':                        # the largest non-zero count under 2^18 on one shared K, asked for ('auto' separates from 2^17 + 1 non-zeros on)
        n, n_pub = (1 << 17) - 3, 4
        a = _matrix(rng, _lens(rng, n, (1 << 18) - 1), n_pub + n, 951); b = _matrix(rng, _lens(rng, n, (1 << 16) + 1), n_pub + n, 952)
        c = _matrix(rng, _lens(rng, n, 5), n_pub + n, 953)
        return {'a': a, 'b': b, 'c': c}, n, n_pub, n, 'shared', {'shared': True, 'n_k': [1 << 18] * 3}
    if name == 'above_2_18':                           # just above 2^18 non-zeros, three different |K_M|
        n, n_pub = (1 << 17) - 5, 4
        a = _matrix(rng, _lens(rng, n, (1 << 18) + 1, {7: 300}), n_pub + n, 961); b = _matrix(rng, _lens(rng, n, (1 << 17) + 3), n_pub + n, 962)
        return {'a': a, 'b': b, 'c': _one_per_row(n, n_pub)}, n, n_pub, n, 'auto', {'shared': False, 'n_k': [1 << 19, 1 << 18, 1 << 17]}
    if name == 'bench_2_20':                           # the size bench.py proves: |H| = 2^20, |K_A| = |K_B| = 2^21, |K_C| = 2^20
        n, n_pub = (1 << 20) - 64, 4
        a = _matrix(rng, _lens(rng, n, (1 << 21) - 5, {3: 200, 9: 9000}), n_pub + n, 971); b = _matrix(rng, _lens(rng, n, 3 << 19), n_pub + n, 972)
        b[1][::50] = 0
        return {'a': a, 'b': b, 'c': _one_per_row(n, n_pub)}, n, n_pub, n, 'auto', {'shared': False, 'n_k': [1 << 21, 1 << 21, 1 << 20], 't_row_over': 8192}
    raise KeyError(name)


SHAPES = ['synthetic_2_15', 'bits_2_15', 'edges', 'long_transpose', 'switch_2_17p1', 'shared_2_18m1', 'above_2_18', 'bench_2_20']


def _expect(ref, want):
    """The shape has what it was built for (so that a change of a generator cannot quietly drop an edge)."""
    if 'shared' in want: assert (len(set(ref.n_k_m)) == 1) == want['shared'], ref.n_k_m
    if 'n_k' in want: assert ref.n_k_m == want['n_k']
    if 'n_h' in want: assert ref.n_h == want['n_h'] and ref.n_h > ref.n_constraints
    if 'nnz' in want: assert [ref.nnz[m] for m in 'abc'] == want['nnz']
    mr = ref.max_row()
    if 'a_row_over' in want: assert mr[0] > want['a_row_over']
    if 't_row_over' in want: assert mr[2] > want['t_row_over']


# ---- CPU: the reference against the restatement ----------------------------------------------------------------------------------------------------
def _small_random(n, n_pub, n_priv, seed, nnz):
    rng = np.random.default_rng(seed)
    csr = {m: _matrix(rng, _lens(rng, n, k, {0: 0}), n_pub + n_priv, seed + i) for i, (m, k) in enumerate(zip('abc', nnz))}
    if nnz[0] > 3: csr['a'][1][csr['a'][0][1]:csr['a'][0][1] + 2] = n_pub             # a variable twice in one row
    return csr, n, n_pub, n_priv


def _small_cases():
    out = []
    for n, n_pub, seed in ((40, 3, 11), (60, 5, 6), (40, 33, 5)):     # the last: |H| = 2 |X| (set by the public inputs)
        csr, z = synth.synthetic_r1cs(n, n_pub, seed, long_rows=1)
        out.append((csr, n, n_pub, len(z) - n_pub))
    out.append(_small_random(30, 2, 200, 71, (64, 65, 0)))           # |H| set by |X| + n_private, nnz 2^6 and 2^6 + 1, an empty C
    out.append(_small_random(100, 9, 100, 72, (250, 17, 1)))
    return out


@pytest.mark.parametrize('domains', ['shared', 'per_matrix'])
@pytest.mark.parametrize('case', range(5))
def test_reference_index_equals_the_restatement(case, domains):
    csr, n, n_pub, n_priv = _small_cases()[case]
    c = V.Circuit(n, n_pub, n_priv, _rows(csr, 'a', n), _rows(csr, 'b', n), _rows(csr, 'c', n), domains=domains)
    if case == 2: assert c.n_h == 2 * c.n_x and c.n_h > max(n, c.n_x + n_priv)
    if case == 3: assert c.n_h == 256 > n
    idx = V.Index(c, V.Setup(TAU, S_GAMMA, D))
    ref = IR.IndexRef(csr, n, n_pub, n_priv, TAU, D, domains)
    assert (ref.n_h, ref.n_x, ref.n_k_m) == (c.n_h, c.n_x, [c.n_k_m[m] for m in 'abc'])
    assert ref.vk_bytes() == idx.vk_bytes()
    pts = idx.commit_points()
    assert IR.C.affine_to_ints(ref.vk_affine()) == [pts[(m, key)] for m in 'abc' for key in IR.KEYS]
    for m in 'abc':
        for key in IR.KEYS:
            assert IR.ints(ref.evals(m, key)) == idx.evals[m][key], (m, key)
            assert IR.ints(ref.polys(m, key)) == idx.polys[m][key], (m, key)
        k = 'abc'.index(m); nk = ref.n_k_m[k]; K2 = V.Domain(2 * nk)
        assert IR.ints(ref.k2_evals(k)) == [v for key in IR.KEYS for v in K2.fft(idx.polys[m][key])], m
        kid = ref.k_idx[2 * ref.k_off[k]:2 * ref.k_off[k] + 2 * nk]
        ent = idx.entries[m]
        assert list(kid[:nk]) == [r for r, _, _ in ent] + [0] * (nk - len(ent)) and list(kid[nk:]) == [p for _, p, _ in ent] + [0] * (nk - len(ent))
    # 1 / v_X on H, zero on X
    H = V.Domain(c.n_h); X = V.Domain(c.n_x)
    assert IR.ints(ref.vx_inv()) == [0 if X.vanishing(h) == 0 else V.inv(X.vanishing(h)) for h in H.elements()]
    # the matrices as the prover reads them, and the hints
    for m in 'ab':
        rp, col, val = ref.forward(m)
        assert list(rp) == [0] + list(np.cumsum([len(r) for r in c.m[m]])) + [len(idx.entries[m])] * (c.n_h - n)
        assert [(int(p), v) for p, v in zip(col, IR.ints(val))] == [(p, v) for _, p, v in idx.entries[m]]
    rp, col, val = ref.transpose()
    want = sorted((p, k * c.n_h + r, v) for k, m in enumerate('abc') for r, p, v in idx.entries[m])
    assert sorted(zip(np.repeat(np.arange(c.n_h), np.diff(rp.astype(np.int64))).tolist(), col.tolist(), IR.ints(val))) == want
    assert ref.max_row() == [max(1, max(len(r) for r in c.m['a'])), max(1, max(len(r) for r in c.m['b'])), max(1, int(np.bincount([p for p, _, _ in want] or [0]).max()))]


def test_reference_index_shapes_have_their_edges():
    """The GPU shapes' claims, checked where they are cheap to build (the large ones are checked beside the device build)."""
    for name in ('edges', 'long_transpose'):
        csr, n, n_pub, n_priv, domains, want = _shape(name)
        _expect(IR.IndexRef(csr, n, n_pub, n_priv, TAU, D, domains), want)


# ---- GPU: the library's index against the reference ------------------------------------------------------------------------------------------------
_HIP = None


def _hip():
    """The HIP runtime torch loaded — the one libaleo_mi355x runs on (aleo_amd/_lib.py) — for copies out of the library's device pointers."""
    global _HIP
    if _HIP is None:
        import torch
        torch.cuda.init()
        path = next(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l.rsplit('/', 1)[-1])
        L = ctypes.CDLL(path)
        L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]; L.hipMemcpy.restype = ctypes.c_int
        L.hipDeviceSynchronize.argtypes = []; L.hipDeviceSynchronize.restype = ctypes.c_int
        _HIP = L
    return _HIP


def device_array(ptr, n, dtype=np.uint64, width=4) -> np.ndarray:
    """n elements (Fr: uint64[n, 4]; indices: uint32[n] with width=1) copied from device memory at ptr."""
    out = np.empty((n, width) if width > 1 else (n,), dtype=dtype)
    if n:
        L = _hip(); assert L.hipDeviceSynchronize() == 0
        assert ptr, 'null device pointer'
        assert L.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0, 'hipMemcpy device -> host'     # 2: hipMemcpyDeviceToHost
    return out


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if len(got) else []
    assert len(bad) == 0, '%s: %d of %d entries differ, first at %d' % (what, len(bad), len(got), bad[0])


def _export(nx):
    from aleo_amd import lib, varuna
    from aleo_amd._lib import check
    view = varuna._NativeIndex(); check(lib().aleo_mi355x_varuna_index_export(nx.handle, ctypes.byref(view)), 'varuna_index_export')
    return view


def _check_view(view, ref):
    """Every array of an exported index against the reference, sizes from the view."""
    n_h, nk, ks = view.n_h, [view.n_k_a, view.n_k_b, view.n_k_c], ref.k_sum
    assert (n_h, nk, view.n_x, view.n_public, view.n_vars) == (ref.n_h, ref.n_k_m, ref.n_x, ref.n_public, ref.n_public + ref.n_private)
    assert ctypes.string_at(view.vk_bytes, view.vk_len) == ref.vk_bytes()
    aff, want = np.frombuffer(ctypes.string_at(view.vk_affine, 12 * 104), dtype=np.uint8).reshape(12, 104), ref.vk_affine()
    assert (aff[:, 96] == want[:, 96]).all() and (aff[want[:, 96] == 0, :96] == want[want[:, 96] == 0, :96]).all()
    n_vars = view.n_vars
    _same('positions', np.ctypeslib.as_array((ctypes.c_uint32 * n_vars).from_address(view.positions)), ref.positions)
    _same('positions_device', device_array(view.positions_device, n_vars, np.uint32, 1), ref.positions)
    for m in 'ab':
        rp_w, col_w, val_w = ref.forward(m)
        rp = device_array(getattr(view, m + '_row_ptr'), n_h + 1, np.uint32, 1); _same(m + '_row_ptr', rp, rp_w)
        _same(m + '_col', device_array(getattr(view, m + '_col'), int(rp[-1]), np.uint32, 1), col_w)
        _same(m + '_val', device_array(getattr(view, m + '_val'), int(rp[-1])), val_w)
    rp_w, col_w, val_w = ref.transpose()
    rp = device_array(view.t_row_ptr, n_h + 1, np.uint32, 1); _same('t_row_ptr', rp, rp_w)
    col, val = IR.canonical_rows(rp, device_array(view.t_col, int(rp[-1]), np.uint32, 1), device_array(view.t_val, int(rp[-1])))
    _same('t_col (rows as multisets)', col, col_w); _same('t_val (rows as multisets)', val, val_w)
    _same('vx_inv', device_array(view.vx_inv, n_h), ref.vx_inv())
    _same('k_idx', device_array(view.k_idx, 2 * ks, np.uint32, 1), ref.k_idx)
    _same('k_evals', device_array(view.k_evals, 4 * ks), ref.k_evals)
    _same('k_polys', device_array(view.k_polys, 4 * ks), ref.k_polys)
    for k in range(3):
        _same('k2_evals of ' + 'abc'[k], device_array(view.k2_evals + 32 * 8 * ref.k_off[k], 8 * nk[k]), ref.k2_evals(k))
    assert list(view.max_row) == ref.max_row()


@pytest.fixture(scope='module')
def ck():
    from aleo_amd import varuna
    k = varuna.synthetic_committer_key(TAU, S_GAMMA, D)
    yield k
    k.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', SHAPES)
def test_native_index_equals_the_reference(name, ck):
    from aleo_amd import varuna
    csr, n, n_pub, n_priv, domains, want = _shape(name)
    ref = IR.IndexRef(csr, n, n_pub, n_priv, TAU, D, domains)
    _expect(ref, want)
    with varuna.NativeCircuitIndex(csr, n, n_pub, n_priv, ck, domains=domains) as nx:
        assert nx.vk_bytes == ref.vk_bytes()
        _check_view(_export(nx), ref)


@pytest.mark.gpu
def test_python_circuit_index_equals_the_reference(ck):
    """The step-by-step CircuitIndex (aleo_amd/varuna.py: the same index through the public entry points) at 2^15 constraints."""
    from aleo_amd import varuna
    csr, n, n_pub, n_priv, domains, _ = _shape('synthetic_2_15')
    ref = IR.IndexRef(csr, n, n_pub, n_priv, TAU, D, domains)
    ix = varuna.CircuitIndex(csr, n, n_pub, n_priv, ck, domains=domains)
    assert ix.vk_bytes == ref.vk_bytes()
    _check_view(varuna.native_index(ix), ref)


@pytest.mark.gpu
def test_unknown_sparse_product_hints_give_the_same_proof(ck):
    """A caller-built view may leave the hints max_row at 0 (unknown): the prover then zeroes its long/huge-row counters and launches every sparse-product
    kernel.  With a transposed row of > 8192 entries (NOT gates on the constant) the proof must be byte-equal to the one made with the exact hints."""
    from aleo_amd import lib, varuna
    from aleo_amd._lib import check, seed32
    csr, n, n_pub, n_priv, domains, want = _shape('bits_2_15')
    _, z = synth.synthetic_r1cs_bits(n, n_pub, 912)
    zz = np.stack([synth.int_to_limbs(v, 4) for v in z])
    with varuna.NativeCircuitIndex(csr, n, n_pub, n_priv, ck, domains=domains) as nx:
        view = _export(nx)
        assert view.max_row[2] > 8192 and min(view.max_row) >= 1
        blind = varuna._NativeIndex.from_buffer_copy(view)
        for i in range(3): blind.max_row[i] = 0
        ptrs = (ctypes.c_void_p * 1)(zz.ctypes.data)
        out = np.zeros(1100, dtype=np.uint8); ln = ctypes.c_size_t(out.shape[0])
        check(lib().aleo_mi355x_varuna_prove(ctypes.byref(blind), ptrs, 1, seed32(31), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ln)), 'varuna_prove')
        got = out[:ln.value].tobytes()
        assert got == nx.prove(zz, 31)
    assert V.verify(V.VerifyingKey(IR.IndexRef(csr, n, n_pub, n_priv, TAU, D, domains).vk_bytes(), n_pub), V.Setup(TAU, S_GAMMA, D), z[:n_pub], got)
