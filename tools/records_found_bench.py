#!/usr/bin/env python3
"""The measurements of decrypt_strings (profiles/records_found.txt is this tool's output).

    python tools/records_found_bench.py [--baseline-lib PATH] [--sizes 12,16,20] [--reps 7] [--python-n 65536] [--out FILE]
    python tools/records_found_bench.py --trace-case        # one warm and three timed calls of the 2^20 / 1 % case and nothing else: the run to put under
                                                            # rocprofv3 --kernel-trace --stats, in a run of its own
    python tools/records_found_bench.py --keys K [--baseline-lib PATH] [--sizes 20] [--fractions 0.001,0.01,0.1] [--reps 7] [--out FILE]
                                                            # decrypt_strings_many for K accounts (profiles/records_found_many.txt); --trace-case with it: the
                                                            # 2^20 / 1 % case of K accounts alone

n strings of the shape of a credits.aleo record (202 characters: a private owner and one private entry, microcredits), a fraction of them the account's: the owned
ones are the reference's own record under the reference's account (tests/golden/reference_records.json), repeated — neither road remembers a record — the others
random bytes in the same layout.  Two roads to the plain fields and microcredits of the owned records:
  new      aleo_mi355x_records_decrypt_strings, then aleo_mi355x_found_free: upload, kernels and the download of the owned records inside the timed call
  parent   what a caller of the parent commit's library ran (--baseline-lib: a build of that commit; without it this build's same functions): records_scan_strings,
           then aleo_mi355x_record_fields per owned string, then records_decrypt_fields.  The per-string calls go through ctypes (about a microsecond each on top of
           the call); reading the microcredits out of the plain fields is left out, in the parent's favour.
and, up to --python-n strings, records.decrypt_owned of this build on a RecordBatch beside them (it renders every owned record's string on the host).
With --keys K: K accounts under the reference's generator, each owning the given fraction of the strings (a credits record of its own, private owner, encrypted
here with oracle/poseidon.py), and three roads to every account's owned records, plain fields and microcredits:
  many     aleo_mi355x_records_decrypt_strings_many and K x aleo_mi355x_found_free; with --baseline-lib the same road through the baseline library beside it
           ("many, baseline"), which shows whether the K-account call itself moved
  calls    K calls of aleo_mi355x_records_decrypt_strings of the baseline library (road a)
  scan     one aleo_mi355x_records_scan_strings of the baseline library with K keys, then per account the host tail of `parent` above (road b)
and road (a) once more through this build, with its own min..max, which shows whether the one-account call itself moved.
Every timing: host buffers, copies inside the timed call, one warm call, the median of --reps with min..max, the roads alternating, no profiler.  Bytes downloaded
per call are counted from the sizes, not measured.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, json, os, random, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['ALEO_MI355X_MIN_RECORDS'] = '0'; os.environ['ALEO_MI355X_MIN_DECRYPT'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records, wire                      # noqa: E402
from oracle import poseidon as ps                       # noqa: E402

REF = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_records.json')))
FRACTIONS = (0.001, 0.01, 0.1, 1.0)
L_ORDER = ps.ED_SUBGROUP_ORDER                          # view keys are scalars below it


def p(a): return a.ctypes.data_as(ctypes.c_void_p)


def make(n, fraction, pool):
    rng = random.Random(n)
    owned = set(range(n)) if fraction >= 1 else set(rng.sample(range(n), max(1, round(n * fraction))))
    return records.RecordBatch.from_strings([REF['records']['owner'] if i in owned else pool[rng.randrange(len(pool))] for i in range(n)]), len(owned)


def foreign_pool(k=4096):
    rng = random.Random(1)
    head = b'\x01\x01\x00'; entry = b'\x01\x0cmicrocredits\x23\x00'
    field = lambda: rng.getrandbits(252).to_bytes(32, 'little')
    return [wire.bech32m_encode('record', head + field() + entry + rng.getrandbits(280).to_bytes(35, 'little') + field()) for _ in range(k)]


def bind(path):
    B = ctypes.CDLL(os.path.abspath(path))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    B.aleo_mi355x_records_scan_strings.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, sz]
    B.aleo_mi355x_record_fields.argtypes = [ctypes.c_char_p, vp, sz, ctypes.POINTER(sz)]
    B.aleo_mi355x_records_decrypt_fields.argtypes = [vp, vp, vp, vp, vp, sz]
    B.aleo_mi355x_version.restype = ctypes.c_char_p
    return B


def roads(L, B, batch, vk, ax):
    n = len(batch); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p)
    flags = np.zeros(n, dtype=np.uint8); kinds = np.zeros(n, dtype=np.int8); rvk = np.zeros((n, 32), dtype=np.uint8)
    cuts = batch.offsets.astype(np.int64)
    state = {}

    def new():
        out = ctypes.c_void_p()
        aleo_amd._lib.check(L.aleo_mi355x_records_decrypt_strings(ctypes.byref(out), tp, p(batch.offsets), n, p(vk), p(ax)), 'records_decrypt_strings')
        state['new'] = (int(L.aleo_mi355x_found_count(out)), int(L.aleo_mi355x_found_fields(out)), sum(int(v) for v in np.frombuffer(ctypes.string_at(L.aleo_mi355x_found_microcredits(out), 8 * int(L.aleo_mi355x_found_count(out))), dtype=np.uint64)[:4]))
        L.aleo_mi355x_found_free(out)

    def parent():
        assert B.aleo_mi355x_records_scan_strings(p(flags), p(kinds), p(rvk), tp, p(batch.offsets), n, p(vk), p(ax), 1) == 0
        idx = np.flatnonzero(flags == 1)
        fields = np.zeros((2 * len(idx) + 8, 32), dtype=np.uint8); off = np.zeros(len(idx) + 1, dtype=np.uint32); m = ctypes.c_size_t(0); at = 0
        base = fields.ctypes.data
        for k, i in enumerate(idx.tolist()):
            assert B.aleo_mi355x_record_fields(batch.text[cuts[i]:cuts[i + 1]], base + 32 * at, 8, ctypes.byref(m)) == 0
            at += m.value; off[k + 1] = at
        keys = np.ascontiguousarray(rvk[idx]); plain = np.zeros((at, 32), dtype=np.uint8); fl = np.zeros(len(idx), dtype=np.uint8)
        assert B.aleo_mi355x_records_decrypt_fields(p(plain), p(fl), p(keys), p(off), p(fields), len(idx)) == 0
        state['parent'] = (len(idx), at)

    return new, parent, state


def accounts_of(K):
    """K (view key scalar, address x) under the reference's generator, and a credits record of each: a private owner and a private u64 named microcredits."""
    G = ps.ed_mul(ps.address_point(REF['addresses']['owner']), pow(ps.view_key_scalar(REF['view_keys']['owner']), -1, L_ORDER))
    dom = ps.domain_separator('AleoSymmetricEncryption0'); le = lambda v: v.to_bytes(32, 'little')
    out = []
    for j in range(K):
        rng = random.Random(100 + j)
        vk = rng.randrange(1, L_ORDER); ax = ps.ed_mul(G, vk)[0]
        N = ps.ed_mul(G, rng.randrange(1, L_ORDER)); rvk = ps.ed_mul(N, vk)[0]
        value = 1000 + j                                        # PLAINTEXT BITS of a u64 literal: variant 00, type 12, size 64, the value, the terminus
        plain = [ax, (12 << 2) | (64 << 10) | (value << 26) | (1 << 90)]
        c = [(a + b) % ps.R for a, b in zip(plain, ps.hash_many_psd8([dom, rvk], 2))]
        payload = b'\x01\x01\x00' + le(c[0]) + b'\x01\x0cmicrocredits\x23\x00\x02\x01\x00' + le(c[1]) + le(N[0])
        out.append((vk, ax, wire.bech32m_encode('record', payload), value))
    return out


def make_many(n, fraction, pool, accounts):
    """Every account owns round(n x fraction) strings of its own; no string has two owners."""
    rng = random.Random(n + len(accounts)); per = max(1, round(n * fraction))
    picked = rng.sample(range(n), per * len(accounts))
    strings = [pool[rng.randrange(len(pool))] for _ in range(n)]
    for j, (_, _, mine, _) in enumerate(accounts):
        for i in picked[j * per:(j + 1) * per]: strings[i] = mine
    return records.RecordBatch.from_strings(strings), per


def roads_many(L, B, batch, accounts):
    n = len(batch); K = len(accounts); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p)
    vks = np.frombuffer(b''.join(a[0].to_bytes(32, 'little') for a in accounts), dtype=np.uint8); axs = np.frombuffer(b''.join(a[1].to_bytes(32, 'little') for a in accounts), dtype=np.uint8)
    flags = np.zeros((K, n), dtype=np.uint8); kinds = np.zeros(n, dtype=np.int8); rvk = np.zeros((K, n, 32), dtype=np.uint8)
    cuts = batch.offsets.astype(np.int64)
    state = {}
    def summary(Lib, out): return (int(Lib.aleo_mi355x_found_count(out)), int(Lib.aleo_mi355x_found_fields(out)), int(np.frombuffer(ctypes.string_at(Lib.aleo_mi355x_found_microcredits(out), 8), dtype=np.uint64)[0]))

    def many(Lib=L, name='many'):
        out = (ctypes.c_void_p * K)()
        assert Lib.aleo_mi355x_records_decrypt_strings_many(out, tp, p(batch.offsets), n, p(vks), p(axs), K) == 0
        state[name] = [summary(Lib, ctypes.c_void_p(out[j])) for j in range(K)]
        for j in range(K): Lib.aleo_mi355x_found_free(ctypes.c_void_p(out[j]))

    def calls(Lib=B, name='calls'):
        got = []
        for j in range(K):
            out = ctypes.c_void_p()
            assert Lib.aleo_mi355x_records_decrypt_strings(ctypes.byref(out), tp, p(batch.offsets), n, p(vks[32 * j:32 * j + 32].copy()), p(axs[32 * j:32 * j + 32].copy())) == 0
            got.append(summary(Lib, out)); Lib.aleo_mi355x_found_free(out)
        state[name] = got

    def scan():
        assert B.aleo_mi355x_records_scan_strings(p(flags), p(kinds), p(rvk), tp, p(batch.offsets), n, p(vks), p(axs), K) == 0
        got = []
        for j in range(K):
            idx = np.flatnonzero(flags[j] == 1)
            fields = np.zeros((2 * len(idx) + 8, 32), dtype=np.uint8); off = np.zeros(len(idx) + 1, dtype=np.uint32); m = ctypes.c_size_t(0); at = 0
            base = fields.ctypes.data
            for k, i in enumerate(idx.tolist()):
                assert B.aleo_mi355x_record_fields(batch.text[cuts[i]:cuts[i + 1]], base + 32 * at, 8, ctypes.byref(m)) == 0
                at += m.value; off[k + 1] = at
            keys = np.ascontiguousarray(rvk[j][idx]); plain = np.zeros((at, 32), dtype=np.uint8); fl = np.zeros(len(idx), dtype=np.uint8)
            assert B.aleo_mi355x_records_decrypt_fields(p(plain), p(fl), p(keys), p(off), p(fields), len(idx)) == 0
            got.append((len(idx), at))
        state['scan'] = got

    return many, calls, scan, (lambda: calls(L, 'calls_here')), (lambda: many(B, 'many_base')), state


def main_many(a, L, pool):
    K = a.keys; accounts = accounts_of(K)
    if a.trace_case:
        batch, per = make_many(1 << 20, 0.01, pool, accounts)
        many, _, _, _, _, state = roads_many(L, L, batch, accounts)
        for _ in range(4): many()
        print('trace case: 2^20 strings, %d accounts, %d owned and %d fields each' % ((K,) + state['many'][0][:2]))
        return
    B = bind(a.baseline_lib) if a.baseline_lib else L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    B.aleo_mi355x_records_decrypt_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp]
    B.aleo_mi355x_records_decrypt_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, sz]
    for name in ('count', 'fields'): getattr(B, 'aleo_mi355x_found_' + name).argtypes = [vp]; getattr(B, 'aleo_mi355x_found_' + name).restype = sz
    B.aleo_mi355x_found_microcredits.argtypes = [vp]; B.aleo_mi355x_found_microcredits.restype = vp; B.aleo_mi355x_found_free.argtypes = [vp]; B.aleo_mi355x_found_free.restype = None
    lines = ['# records_found_bench --keys %d --sizes %s --fractions %s --reps %d%s' % (K, a.sizes, a.fractions, a.reps, ' --baseline-lib (the parent commit\'s build)' if a.baseline_lib else ''),
             '# many: %s' % L.aleo_mi355x_version().decode(), '# calls (a) and scan (b) through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of the roads alternating; % owned: per account; bytes down: counted per call', '']
    for lg in [int(v) for v in a.sizes.split(',')]:
        n = 1 << lg
        for fr in [float(v) for v in a.fractions.split(',')]:
            batch, per = make_many(n, fr, pool, accounts)
            many, calls, scan, calls_here, many_base, state = roads_many(L, B, batch, accounts)
            fns = {'many': many, 'calls': calls, 'scan': scan, 'calls_here': calls_here}
            if a.baseline_lib: fns['many_base'] = many_base
            r = timed(fns, a.reps)
            want = [(per, 2 * per, acc[3]) for acc in accounts]
            assert state['many'] == want == state['calls'] == state['calls_here'] == state.get('many_base', want) and state['scan'] == [w[:2] for w in want], (state, per)
            c = per * K
            down_many = 16 + 8 * K + c * (4 + 1 + 32 + 4 + 1 + 8) + 4 + 32 * 2 * c; down_calls = K * 16 + c * (4 + 1 + 32 + 4 + 1 + 8) + 4 * K + 32 * 2 * c; down_scan = n * (33 * K + 1) + 32 * 2 * c + c
            best = min(r['calls'][0], r['scan'][0])
            row = '2^%-2d x %d keys %5.1f %% owned (%7d each)  many %9.3f (%.3f..%.3f)  calls (a) %10.3f (%.3f..%.3f)  scan (b) %10.3f (%.3f..%.3f)  %5.2fx of the better   (a) through this build %10.3f (%.3f..%.3f)%s   down: many %10d B  (a) %10d B  (b) %10d B' % (
                lg, K, 100 * fr, per, r['many'][0] * 1e3, r['many'][1] * 1e3, r['many'][2] * 1e3, r['calls'][0] * 1e3, r['calls'][1] * 1e3, r['calls'][2] * 1e3, r['scan'][0] * 1e3, r['scan'][1] * 1e3, r['scan'][2] * 1e3,
                best / r['many'][0], r['calls_here'][0] * 1e3, r['calls_here'][1] * 1e3, r['calls_here'][2] * 1e3,
                '   many, baseline %9.3f (%.3f..%.3f)' % tuple(v * 1e3 for v in r['many_base']) if a.baseline_lib else '', down_many, down_calls, down_scan)
            lines.append(row); print(row, flush=True)
        lines.append('')
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n')


def timed(fns, reps):
    for f in fns.values(): f()
    ts = {k: [] for k in fns}
    for rep in range(reps):                                     # the roads alternate in a new order every round (seeded): none always runs behind the same one
        order = list(fns.items()); random.Random(rep).shuffle(order)
        for k, f in order:
            t0 = time.perf_counter(); f(); ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-lib'); ap.add_argument('--sizes', default='12,16,20'); ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--python-n', type=int, default=1 << 16); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    ap.add_argument('--keys', type=int, default=0); ap.add_argument('--fractions', default='0.001,0.01,0.1')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    vk = np.frombuffer(records.view_key_bytes(REF['view_keys']['owner']), dtype=np.uint8); ax = np.frombuffer(records.address_x_bytes(REF['addresses']['owner']), dtype=np.uint8)
    pool = foreign_pool()
    if a.keys: return main_many(a, L, pool)
    if a.trace_case:
        batch, c = make(1 << 20, 0.01, pool)
        new, _, state = roads(L, L, batch, vk, ax)
        for _ in range(4): new()
        print('trace case: 2^20 strings, %d owned, %d fields' % state['new'][:2])
        return
    B = bind(a.baseline_lib) if a.baseline_lib else L
    lines = ['# records_found_bench --sizes %s --reps %d%s' % (a.sizes, a.reps, ' --baseline-lib (the parent commit\'s build)' if a.baseline_lib else ''),
             '# new: %s' % L.aleo_mi355x_version().decode(), '# parent road through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max); bytes down: counted per call; decrypt_owned: Python, this build, up to 2^%d strings' % (a.python_n.bit_length() - 1), '']
    for lg in [int(v) for v in a.sizes.split(',')]:
        n = 1 << lg
        for fr in FRACTIONS:
            batch, c = make(n, fr, pool)
            new, parent, state = roads(L, B, batch, vk, ax)
            r = timed({'new': new, 'parent': parent}, a.reps)
            assert state['new'][:2] == state['parent'] == (c, 2 * c) and state['new'][2] == 1500000000000000 * min(c, 4), (state, c)
            chunks = 1
            down_new = 16 * chunks + c * (4 + 1 + 32 + 4 + 1 + 8) + 4 + 32 * 2 * c; down_parent = n * 34 + 32 * 2 * c + c
            row = '2^%-2d %5.1f %% owned (%7d)  new %9.3f (%.3f..%.3f)  parent %10.3f (%.3f..%.3f)  %6.2fx   down: new %10d B  parent %10d B' % (
                lg, 100 * fr, c, r['new'][0] * 1e3, r['new'][1] * 1e3, r['new'][2] * 1e3, r['parent'][0] * 1e3, r['parent'][1] * 1e3, r['parent'][2] * 1e3, r['parent'][0] / r['new'][0], down_new, down_parent)
            if n <= a.python_n:
                py = timed({'py': lambda: records.decrypt_owned(batch, vk.tobytes(), ax.tobytes())}, max(3, a.reps // 2))['py']
                row += '   decrypt_owned %10.3f' % (py[0] * 1e3)
            lines.append(row); print(row, flush=True)
        lines.append('')
    text = '\n'.join(lines) + '\n'
    if a.out:
        with open(a.out, 'w') as f: f.write(text)


if __name__ == '__main__':
    main()
