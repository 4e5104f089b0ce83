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

  python tools/records_scan_bench.py [--max-lg 22] [--out profiles/records_scan.txt]"""
import argparse, os, statistics, sys, time
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-lg', type=int, default=2); ap.add_argument('--max-lg', type=int, default=22)
    ap.add_argument('--host-lg', type=int, default=12, help='size of the one-thread host measurement (its rate does not depend on the size)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'records_scan.txt'))
    a = ap.parse_args()
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
