#!/usr/bin/env python3
"""Records per second of the ownership scan, and the batch size from which the GPU wins (the default of aleo_mi355x_min_records).

Three paths on the same records, the same algorithm each time:
  gpu       aleo_mi355x_records_scan with the threshold forced to 0: host buffers in, flags and record view keys out — upload, kernel and download inside the timed call
  host x1   aleo_mi355x_records_scan_host on one thread
  host x16  the same on 16 threads, each with its own slice of the batch (the calls release the GIL)
The baseline is the host path on the box's own cores, never an earlier number of the kernel.  Every nonce is on the curve (an x off it leaves the host path
after the square root, which would flatter it); the kernel's time does not depend on the data.  Each timed call ends in the library's stream synchronise;
every shape is warmed up once; a figure is the median of at least three calls and at least half a second of work.
Up to 2^--host-lg records the one-thread host path is TIMED at every size (so a call's fixed costs — ctypes, the recoding of the key — are in the crossover);
above it, and for 16 threads everywhere, the host time is the measured rate times n, and the table says so.

  python tools/records_scan_bench.py [--max-lg 22] [--out profiles/records_scan.txt]

With --keys the tool measures the grouped scan instead (aleo_mi355x_records_scan_many: K accounts over the same records in one call) against what it replaces,
K calls of aleo_mi355x_records_scan over those records — made through --baseline-lib when given (another build of the library, for instance the parent
commit's; its own grouped scan is then timed too, as "rule, baseline"), else through this build, whose single-key kernel is the same code.  Shapes are lg n:K pairs; at each shape the baseline, the library's own rule and
every forced width (ALEO_MI355X_SCAN_KEYS_PER_LANE = 1, 2, 4, 8) are warmed up once and then timed in turn, round after round, so that whatever else the
machine does falls on all of them alike; output buffers are allocated once, outside the timed calls.  A figure is the median over the rounds, with min..max.

  python tools/records_scan_bench.py --keys [--shapes 20:8,20:3,18:8,16:16,12:8] [--rounds 7] [--baseline-lib PATH] [--out profiles/records_scan_many.txt]"""
import argparse, ctypes, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['ALEO_MI355X_MIN_RECORDS'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records                            # noqa: E402
from oracle import poseidon as ps                       # noqa: E402  (test-side arithmetic: it only MAKES the inputs)


def make_records(n, pool=1 << 12, seed=11):
    """n records whose nonces are multiples of a subgroup point (all on the curve), `pool` distinct ones tiled; random owner fields; the view key and address."""
    rng = np.random.default_rng(seed)
    G = ps.ed_from_x(next(x for x in range(2, 1000) if _has_prime_point(x)))
    vk = int.from_bytes(rng.bytes(31), 'little') % ps.ED_SUBGROUP_ORDER
    A = ps.ed_mul(G, vk)
    N, xs = ps.ed_mul(G, 12345), []
    for _ in range(min(pool, n)): xs.append(N[0].to_bytes(32, 'little')); N = ps.ed_add(N, G)
    nx = np.frombuffer(b''.join(xs), dtype=np.uint8).reshape(-1, 32)
    nx = np.ascontiguousarray(np.tile(nx, ((n + len(xs) - 1) // len(xs), 1))[:n])
    c0 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); c0[:, 31] &= 0x0f      # below r
    return c0, nx, vk, A[0]


def _has_prime_point(x):
    try: ps.ed_from_x(x); return True
    except ValueError: return False


def timed(f, min_time=0.5, min_reps=3):
    f()                                                  # warm-up of this shape
    ts, t_all = [], 0.0
    while len(ts) < min_reps or t_all < min_time:
        t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
        ts.append(dt); t_all += dt
        if len(ts) >= 50: break
    return statistics.median(ts), min(ts), max(ts), len(ts)


def many_keys(k, seed=23):
    """k different accounts: view keys below the subgroup order, any canonical field element as address x (the scan's time does not depend on it)"""
    rng = np.random.default_rng(seed)
    vks = [int.from_bytes(rng.bytes(31), 'little') % ps.ED_SUBGROUP_ORDER for _ in range(k)]
    to_rows = lambda vals: np.frombuffer(b''.join(int(v).to_bytes(32, 'little') for v in vals), dtype=np.uint8).reshape(-1, 32).copy()
    return to_rows(vks), to_rows([int.from_bytes(rng.bytes(31), 'little') for _ in range(k)])


def bench_many(a):
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    base = L
    if a.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        for name in ('aleo_mi355x_records_scan', 'aleo_mi355x_records_scan_many', 'aleo_mi355x_init_device'): getattr(base, name).restype = ctypes.c_int32
        base.aleo_mi355x_records_scan_many.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t]
        base.aleo_mi355x_records_scan.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        base.aleo_mi355x_init_device.argtypes = [ctypes.c_int32]
        base.aleo_mi355x_version.restype = ctypes.c_char_p
        assert base.aleo_mi355x_init_device(-1) == 0
    shapes = [tuple(int(v) for v in s.split(':')) for s in a.shapes.split(',')]
    c0, nx, _, _ = make_records(1 << max(lg for lg, _ in shapes))
    p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    configs = ['K single scans', 'rule', 'W=1', 'W=2', 'W=4', 'W=8'] + (['rule, baseline'] if a.baseline_lib else [])      # the last: the grouped scan of the baseline library
    lines = ['records_scan_bench --keys: aleo_mi355x_records_scan_many (K accounts, n records, one call; host buffers, upload and download inside the timed call) against',
             'K calls of aleo_mi355x_records_scan over the same records (%s).  ms per call: median (min..max) over %d rounds, the configurations timed in turn within a round;'
             % ('baseline library: %s' % base.aleo_mi355x_version().decode() if a.baseline_lib else 'this build', a.rounds),
             'x = the baseline\'s median over the configuration\'s.  W = keys per lane forced by ALEO_MI355X_SCAN_KEYS_PER_LANE; rule = unset.', '%s' % L.aleo_mi355x_version().decode(), '']
    for lg, k in shapes:
        n = 1 << lg
        vk, ax = many_keys(k)
        C0, NX = c0[:n], nx[:n]
        flags = np.zeros((k, n), dtype=np.uint8); rvk = np.zeros((k, n, 32), dtype=np.uint8)
        bflags = np.ones((k, n), dtype=np.uint8); brvk = np.ones((k, n, 32), dtype=np.uint8)
        def run(cfg):
            if cfg == 'K single scans':
                for j in range(k): assert base.aleo_mi355x_records_scan(p(bflags[j]), p(brvk[j]), p(C0), p(NX), n, p(vk[j]), p(ax[j])) == 0
                return
            if cfg.startswith('rule'): os.environ.pop('ALEO_MI355X_SCAN_KEYS_PER_LANE', None)
            else: os.environ['ALEO_MI355X_SCAN_KEYS_PER_LANE'] = cfg[2:]
            if cfg == 'rule, baseline': assert base.aleo_mi355x_records_scan_many(p(flags), p(rvk), p(C0), p(NX), n, p(vk), p(ax), k) == 0
            else: aleo_amd._lib.check(L.aleo_mi355x_records_scan_many(p(flags), p(rvk), p(C0), p(NX), n, p(vk), p(ax), k), 'records_scan_many')
        run(configs[0])
        for cfg in configs[1:]:                              # warm-up of every shape and width, and the parity of what is about to be timed
            flags[:] = 7; run(cfg)
            assert flags.tobytes() == bflags.tobytes() and rvk.tobytes() == brvk.tobytes(), 'records_scan_many (%s) and K single scans disagree at n = 2^%d, K = %d' % (cfg, lg, k)
        ts = {cfg: [] for cfg in configs}
        for _ in range(a.rounds):
            for cfg in configs:
                t0 = time.perf_counter(); run(cfg); ts[cfg].append(time.perf_counter() - t0)
        os.environ.pop('ALEO_MI355X_SCAN_KEYS_PER_LANE', None)
        b = statistics.median(ts[configs[0]])
        lines.append('n = 2^%d, K = %d  (%d pairs)' % (lg, k, n * k))
        for cfg in configs:
            m = statistics.median(ts[cfg])
            lines.append('  %-15s %10.3f  (%.3f..%.3f)  %6.2fx  %8.2f M pairs/s' % (cfg, m * 1e3, min(ts[cfg]) * 1e3, max(ts[cfg]) * 1e3, b / m, n * k / m / 1e6))
        lines.append('  spread of the baseline: %.1f %% of its median' % ((max(ts[configs[0]]) - min(ts[configs[0]])) / b * 100))
        print('\n'.join(lines[-len(configs) - 2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keys', action='store_true', help='measure the grouped scan (records_scan_many) against K single scans')
    ap.add_argument('--shapes', default='20:8,20:3,18:8,16:16,12:8', help='with --keys: lg n:K pairs')
    ap.add_argument('--rounds', type=int, default=7); ap.add_argument('--baseline-lib', default=None, help='with --keys: the library that makes the K single scans')
    ap.add_argument('--min-lg', type=int, default=2); ap.add_argument('--max-lg', type=int, default=22)
    ap.add_argument('--host-lg', type=int, default=12, help='size of the one-thread host measurement (its rate does not depend on the size)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'records_scan.txt'))
    a = ap.parse_args()
    if a.keys:
        if a.out == ap.get_default('out'): a.out = os.path.join(ROOT, 'profiles', 'records_scan_many.txt')
        return bench_many(a)
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    c0, nx, vk, ax = make_records(1 << a.max_lg)
    lines = ['records_scan_bench: records/s of the ownership scan; gpu = aleo_mi355x_records_scan on host buffers (upload and download inside the call), '
             'host = aleo_mi355x_records_scan_host', '%s' % L.aleo_mi355x_version().decode(), '']
    # the host path
    n1 = 1 << a.host_lg
    t1, lo, hi, reps = timed(lambda: records.scan(c0[:n1], nx[:n1], vk, ax, host=True), min_time=1.0)
    rate1 = n1 / t1
    lines.append('host x1 : 2^%d records in %.1f ms (median of %d, %.1f..%.1f)  -> %.0f records/s' % (a.host_lg, t1 * 1e3, reps, lo * 1e3, hi * 1e3, rate1))
    n16 = 1 << min(a.max_lg, 16); per = n16 // 16
    pool = ThreadPoolExecutor(16)
    def host16(): list(pool.map(lambda k: records.scan(c0[k * per:(k + 1) * per], nx[k * per:(k + 1) * per], vk, ax, host=True), range(16)))
    t16, lo, hi, reps = timed(host16, min_time=1.0)
    rate16 = n16 / t16
    lines.append('host x16: 2^%d records in %.1f ms (median of %d, %.1f..%.1f)  -> %.0f records/s' % (min(a.max_lg, 16), t16 * 1e3, reps, lo * 1e3, hi * 1e3, rate16))
    # parity at the first size, so that the table times the right answer
    f_g, r_g = records.scan(c0[:n1], nx[:n1], vk, ax); f_h, r_h = records.scan(c0[:n1], nx[:n1], vk, ax, host=True)
    assert f_g.tobytes() == f_h.tobytes() and r_g.tobytes() == r_h.tobytes(), 'the kernel and the host path disagree'
    lines += ['', 'host x1 ms: timed at this size up to 2^%d, beyond it n / (host x1 rate) [marked ~]; host x16 is n / (host x16 rate) at every size' % a.host_lg,
              '   n      gpu ms (median, min..max, calls)      gpu records/s   host x1 ms   vs host x1   vs host x16']
    cross1 = cross16 = None
    for lg in range(a.min_lg, a.max_lg + 1):
        n = 1 << lg
        t, lo, hi, reps = timed(lambda: records.scan(c0[:n], nx[:n], vk, ax))
        if lg <= a.host_lg: h1, mark = timed(lambda: records.scan(c0[:n], nx[:n], vk, ax, host=True), min_time=0.2)[0], ' '
        else: h1, mark = n / rate1, '~'
        s1, s16 = h1 / t, (n / rate16) / t
        if s1 > 1 and cross1 is None: cross1 = lg
        if s1 <= 1: cross1 = None                            # the crossover is the size from which the GPU wins at EVERY larger size
        if s16 > 1 and cross16 is None: cross16 = lg
        if s16 <= 1: cross16 = None
        lines.append('2^%-3d  %9.3f  (%.3f..%.3f, %d)  %14.0f  %10.3f%s  %9.2fx  %9.2fx' % (lg, t * 1e3, lo * 1e3, hi * 1e3, reps, n / t, h1 * 1e3, mark, s1, s16))
        print(lines[-1], flush=True)
    big = 1 << min(a.max_lg, 20)
    tb = timed(lambda: records.scan(c0[:big], nx[:big], vk, ax))[0]
    lines += ['', 'at 2^%d records the GPU path takes %.1f ms, 16 host threads would take %.0f ms: the GPU %s 16 host threads there (%.0fx)' % (min(a.max_lg, 20), tb * 1e3, big / rate16 * 1e3, 'beats' if tb < big / rate16 else 'does NOT beat', (big / rate16) / tb)]
    lines += ['', 'crossover against the host path on one thread  (what a call below the threshold runs): %s' % ('2^%d' % cross1 if cross1 is not None else 'none up to 2^%d' % a.max_lg),
              'crossover against the host path on 16 threads: %s' % ('2^%d' % cross16 if cross16 is not None else 'none up to 2^%d' % a.max_lg)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:6] + lines[-4:]))


if __name__ == '__main__':
    main()
