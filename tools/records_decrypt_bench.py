#!/usr/bin/env python3
"""Records per second of the batch decryption (aleo_mi355x_records_decrypt_fields), and the size from which the GPU wins (the default of aleo_mi355x_min_decrypt).

Four ways to the same plain fields:
  gpu       aleo_mi355x_records_decrypt_fields with the threshold forced to 0: host buffers in, plain fields and flags out — upload, kernel and download inside the timed call
  baseline  what a caller had before: aleo_mi355x_poseidon_hash_fr(8, [domain, rvk], 2, out, m) once per record from one thread, through --baseline-lib when given
            (another build of the library, for instance the parent commit's), else through this build, whose poseidon_hash_fr is the same code.  The subtraction
            c - randomizer is left out, in the baseline's favour
  host x1   aleo_mi355x_records_decrypt_fields_host on one thread (what a call below the threshold runs)
  host x16  the same on 16 threads, each with its own slice of the batch (the calls release the GIL)
The configurations of a shape are warmed up once and then timed in turn, round after round, so that whatever else the machine does falls on all of them alike;
output buffers are allocated once, outside the timed calls; a figure is the median over the rounds with min..max.  The per-record baseline and the host paths are
TIMED up to 2^--host-lg records; above that their time is the rate measured there times n, and the table marks it (~).  No profiler is attached; the kernel's own time
per launch comes from a separate run under rocprofv3 --kernel-trace --stats.

  python tools/records_decrypt_bench.py [--rounds 7] [--baseline-lib PATH] [--out profiles/records_decrypt.txt]"""
import argparse, ctypes, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['ALEO_MI355X_MIN_DECRYPT'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records                            # noqa: E402

DOMAIN = int.from_bytes(b'AleoSymmetricEncryption0', 'little').to_bytes(32, 'little')


def p(a): return a.ctypes.data_as(ctypes.c_void_p)


def make(n, m, seed=5):
    rng = np.random.default_rng(seed)
    rvk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); rvk[:, 31] &= 0x0f      # below r
    fields = rng.integers(0, 256, size=(n * m, 32), dtype=np.uint8); fields[:, 31] &= 0x0f
    return rvk, (np.arange(n + 1, dtype=np.uint64) * m).astype(np.uint32), fields


def median_of(fns, rounds):
    """{name: (median, min, max)} of the callables, warmed up once each and then timed in turn within every round."""
    for f in fns.values(): f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t0 = time.perf_counter(); f(); ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7); ap.add_argument('--min-lg', type=int, default=4); ap.add_argument('--max-lg', type=int, default=20)
    ap.add_argument('--host-lg', type=int, default=12, help='up to this size the per-record baseline and the host paths are timed, beyond it extrapolated')
    ap.add_argument('--baseline-lib', default=None); ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'records_decrypt.txt'))
    a = ap.parse_args()
    assert a.rounds >= 7, 'medians of at least 7 rounds'
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    base = L
    if a.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        base.aleo_mi355x_poseidon_hash_fr.restype = ctypes.c_int32
        base.aleo_mi355x_poseidon_hash_fr.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        base.aleo_mi355x_version.restype = ctypes.c_char_p
        base.aleo_mi355x_records_decrypt_fields.restype = ctypes.c_int32; base.aleo_mi355x_records_decrypt_fields.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    pool = ThreadPoolExecutor(16)
    lines = ['records_decrypt_bench: aleo_mi355x_records_decrypt_fields (host buffers, upload and download inside the timed call, threshold 0) against one',
             'aleo_mi355x_poseidon_hash_fr call per record on one thread (%s; the subtraction left out),' % ('baseline library: %s' % base.aleo_mi355x_version().decode() if a.baseline_lib else 'this build'),
             'and against the new host path on 1 and 16 threads.  ms per call: median (min..max) over %d rounds, the configurations timed in turn within a round; ~ = rate at 2^%d times n.' % (a.rounds, a.host_lg),
             '%s' % L.aleo_mi355x_version().decode(), '']

    def shape(lg, m, rates):
        n = 1 << lg
        rvk, off, fields = make(n, m)
        plain = np.zeros_like(fields); flags = np.zeros(n, dtype=np.uint8); hplain = np.zeros_like(fields); hflags = np.zeros(n, dtype=np.uint8)
        inp = np.zeros((n, 2, 32), dtype=np.uint8); inp[:, 0] = np.frombuffer(DOMAIN, dtype=np.uint8); inp[:, 1] = rvk
        rnd = np.zeros((m, 32), dtype=np.uint8)
        def gpu(): aleo_amd._lib.check(L.aleo_mi355x_records_decrypt_fields(p(plain), p(flags), p(rvk), p(off), p(fields), n), 'records_decrypt_fields')
        def host1(): aleo_amd._lib.check(L.aleo_mi355x_records_decrypt_fields_host(p(hplain), p(hflags), p(rvk), p(off), p(fields), n), 'records_decrypt_fields_host')
        per = max(n // 16, 1); parts = [(k, min(k + per, n)) for k in range(0, n, per)]
        def part(lo_hi):
            lo, hi = lo_hi; o = (off[lo:hi + 1] - off[lo]).astype(np.uint32)
            return L.aleo_mi355x_records_decrypt_fields_host(p(hplain[off[lo]:]), p(hflags[lo:]), p(rvk[lo:]), p(o), p(fields[off[lo]:]), hi - lo)
        def host16(): assert not any(pool.map(part, parts))
        hash_fr, pin, prnd = base.aleo_mi355x_poseidon_hash_fr, [inp[i].ctypes.data for i in range(n)] if lg <= a.host_lg else [], rnd.ctypes.data
        def baseline():
            for q in pin: hash_fr(8, q, 2, prnd, m)
        def gpu_base(): assert base.aleo_mi355x_records_decrypt_fields(p(plain), p(flags), p(rvk), p(off), p(fields), n) == 0
        fns = {'gpu': gpu}
        if a.baseline_lib: fns['gpu, baseline library'] = gpu_base      # the same call through the other build: whether the call itself moved
        if lg <= a.host_lg: fns.update({'baseline': baseline, 'host x1': host1, 'host x16': host16})
        r = median_of(fns, a.rounds)
        if lg <= a.host_lg:
            assert plain.tobytes() == hplain.tobytes() and flags.tobytes() == hflags.tobytes(), 'the kernel and the host path disagree at 2^%d x %d' % (lg, m)
            for k in ('baseline', 'host x1', 'host x16'): rates[k] = r[k][0] / n
        g = r['gpu'][0]
        row = '2^%-2d x %-2d  gpu %9.3f (%.3f..%.3f)  %8.2f M records/s |' % (lg, m, g * 1e3, r['gpu'][1] * 1e3, r['gpu'][2] * 1e3, n / g / 1e6)
        out = {}
        for k in ('baseline', 'host x1', 'host x16'):
            if k in r: t, mark, spread = r[k][0], ' ', ' (%.3f..%.3f)' % (r[k][1] * 1e3, r[k][2] * 1e3)
            else: t, mark, spread = rates[k] * n, '~', ''
            out[k] = t
            row += ' %s %10.3f%s%s %7.2fx |' % (k, t * 1e3, mark, spread, t / g)
        if a.baseline_lib: row += ' gpu, baseline library %9.3f (%.3f..%.3f) |' % tuple(v * 1e3 for v in r['gpu, baseline library'][:3])
        lines.append(row); print(row, flush=True)
        return g, out

    rates, cross = {}, None
    for lg in range(a.min_lg, a.max_lg + 1):
        g, o = shape(lg, 2, rates)
        if o['host x1'] > g and cross is None: cross = lg
        if o['host x1'] <= g: cross = None                  # the crossover is the size from which the GPU wins at EVERY larger size
        last = (lg, g, o)
    lines.append('')
    rates17 = {}
    shape(min(a.host_lg, 10), 17, rates17)                 # the rates of 17-field records for the extrapolation below
    shape(min(a.max_lg, 18), 17, rates17)
    lg, g, o = last
    lines += ['', 'crossover against the host path on one thread (what a call below the threshold runs): %s records of 2 fields = that many permutations'
              % ('2^%d' % cross if cross is not None else 'none up to 2^%d' % a.max_lg),
              'at 2^%d x 2 the GPU call takes %.1f ms, 16 host threads ~%.1f ms: the GPU %s 16 host threads there (%.1fx)' % (lg, g * 1e3, o['host x16'] * 1e3, 'beats' if g < o['host x16'] else 'does NOT beat', o['host x16'] / g)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    # where a large call's time goes: the same buffers through the runtime's copies alone
    import torch
    n = 1 << lg; rvk, off, fields = make(n, 2)
    d = torch.empty(fields.nbytes + rvk.nbytes + off.nbytes, dtype=torch.uint8, device='cuda'); hf = torch.from_numpy(fields.reshape(-1)); hr = torch.from_numpy(rvk.reshape(-1)); back = torch.empty(fields.nbytes, dtype=torch.uint8)
    def up(): d[:hf.numel()].copy_(hf); d[hf.numel():hf.numel() + hr.numel()].copy_(hr); torch.cuda.synchronize()
    def down(): back.copy_(d[:back.numel()]); torch.cuda.synchronize()
    c = median_of({'up': up, 'down': down}, a.rounds)
    lines.append('the copies alone at that size (pageable host memory, torch): upload of fields and keys %.1f ms, download of the plain fields %.1f ms; the rest of the call is the kernel, the offsets and the synchronisation'
                 % (c['up'][0] * 1e3, c['down'][0] * 1e3))
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-4:]))


if __name__ == '__main__':
    main()
