#!/usr/bin/env python3
"""The measurements of aleo_mi355x_signatures_sign (profiles/signatures_sign.txt is this tool's output).

    python tools/signatures_sign_bench.py [--sizes 4,5,...,20] [--long 16] [--reps 8] [--threads 16] [--out FILE]
    python tools/signatures_sign_bench.py --trace-case [--sizes 16]   # one warm and three timed calls per size and mode and nothing else: the run to put under
                                                                       # rocprofv3 --kernel-trace --stats, in a run of its own (the program after --)

2^k signatures of 32-byte messages (and 2^--long of 1024-byte ones), in both modes: one key for all, and a key each out of 64 accounts.  Four roads to the rows,
which must agree byte for byte:
  kernel     aleo_mi355x_signatures_sign with ALEO_MI355X_MIN_SIGN=1: host buffers, the copies inside the call
  host       aleo_mi355x_signatures_sign_host on one thread: what a batch below min_sign runs inside the call
  loop       the parent commit's road: a loop of aleo_mi355x_signature_sign, one call per message, on one thread
  loop x T   the same over T threads, a slice of the batch each (2^10 and more only)
The two columns are two timings of each set: min_sign is the smallest power of two at which the kernel beats the one-thread host path and the loop in both, in
both modes.  Every timing: one warm call, the median of --reps rounds with min..max, the roads in a new seeded order every round, no profiler.  From 2^10 on the
host roads are timed on a slice of 2^9 signatures and scaled (they are linear in n; the line says so).  The check for equal nonce seeds is timed as the refusal of
2^20 seeds of which the last repeats the first: the call returns right after it.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys, threading, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_SIGN'] = '1'
import aleo_amd                                         # noqa: E402
from aleo_amd import account                            # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import timed, p                # noqa: E402
from records_unspent_bench import ms                    # noqa: E402

ACCOUNTS, HOST_SLICE = 64, 1 << 9


def keys():
    rng = random.Random(11)
    names = [ps.private_key_string(rng.randrange(ps.R)) for _ in range(ACCOUNTS)]
    return names, [account.private_key_seed(k) for k in names]


def batch(n, each, message_bytes, names, seeds32):
    rng = np.random.default_rng(n + each)
    msgs = rng.integers(0, 256, size=n * message_bytes, dtype=np.uint8)
    nonce = rng.integers(0, 256, size=32 * n, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * message_bytes
    key_rows = np.frombuffer(b''.join(seeds32[i % ACCOUNTS] for i in range(n)) if each else seeds32[0], dtype=np.uint8).copy()
    return key_rows, msgs, off, nonce, [names[i % ACCOUNTS if each else 0].encode() for i in range(min(n, HOST_SLICE))]


def roads(L, B, n, each, message_bytes, threads):
    key_rows, msgs, off, nonce, key_names = B
    hn = min(n, HOST_SLICE); stride = 32 if each else 0
    state = {k: np.zeros((n if k == 'kernel' else hn, 128), dtype=np.uint8) for k in ('kernel', 'host', 'loop', 'threads')}
    flags = {k: np.zeros(n, dtype=np.uint8) for k in ('kernel', 'host')}
    base = {k: v.ctypes.data for k, v in state.items()}; m0, s0 = msgs.ctypes.data, nonce.ctypes.data

    def kernel(): aleo_amd._lib.check(L.aleo_mi355x_signatures_sign(p(state['kernel']), p(flags['kernel']), p(key_rows), stride, p(msgs), p(off), p(nonce), n), 'signatures_sign')
    def host(): aleo_amd._lib.check(L.aleo_mi355x_signatures_sign_host(p(state['host']), p(flags['host']), p(key_rows), stride, p(msgs), p(off), p(nonce), hn), 'signatures_sign_host')
    def one(road, i): L.aleo_mi355x_signature_sign(base[road] + 128 * i, key_names[i], m0 + message_bytes * i, message_bytes, s0 + 32 * i)
    def loop():
        for i in range(hn): one('loop', i)
    def many():
        per = (hn + threads - 1) // threads
        def work(t):
            for i in range(t * per, min(hn, (t + 1) * per)): one('threads', i)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts: t.start()
        for t in ts: t.join()
    return kernel, host, loop, many, state, flags, hn


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default=','.join(str(k) for k in range(4, 21))); ap.add_argument('--long', default='16'); ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--threads', type=int, default=16); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    names, seeds32 = keys()
    shown = [arg for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# signatures_sign_bench %s' % ' '.join(shown), '# %s' % L.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; %d accounts; loop: the parent commit\'s road, one aleo_mi355x_signature_sign per message' % (a.reps, ACCOUNTS), '']
    def emit(row): lines.append(row); print(row, flush=True)
    cases = [(int(v), 32) for v in a.sizes.split(',') if v] + [(int(v), 1024) for v in a.long.split(',') if v]
    for lg, message_bytes in cases:
        n = 1 << lg
        for each in (0, 1):
            kernel, host, loop, many, state, flags, hn = roads(L, batch(n, each, message_bytes, names, seeds32), n, each, message_bytes, a.threads)
            label = '2^%-2d x %4d B, %s' % (lg, message_bytes, 'a key each' if each else 'one key   ')
            if a.trace_case:
                for _ in range(4): kernel()
                host(); assert state['kernel'][:hn].tobytes() == state['host'].tobytes() and not flags['kernel'].any()
                print('trace case: %s' % label); continue
            scale = n / hn
            fns = {'kernel': kernel, 'host': host, 'loop': loop}
            if n >= 1 << 10: fns['threads'] = many
            pairs = [timed(fns, a.reps) for _ in range(2)]
            assert state['kernel'][:hn].tobytes() == state['host'].tobytes() == state['loop'].tobytes() and not flags['kernel'].any(), 'the roads disagree'
            if 'threads' in fns: assert state['threads'].tobytes() == state['host'].tobytes()
            up = lambda t: tuple(v * scale for v in t)
            row = label + '   ' + '   '.join('kernel %s  host, one thread %s  %6.2fx  loop, one thread %s  %6.2fx' % (ms(r['kernel']), ms(up(r['host'])), r['host'][0] * scale / r['kernel'][0], ms(up(r['loop'])), r['loop'][0] * scale / r['kernel'][0]) for r in pairs)
            if 'threads' in fns: row += '   loop, %d threads %s  %6.2fx' % (a.threads, ms(up(pairs[0]['threads'])), pairs[0]['threads'][0] * scale / pairs[0]['kernel'][0])
            if scale != 1: row += '   (host roads: 2^9 signatures timed, x %d)' % scale
            row += '   %.3f M signatures/s through the call' % (n / pairs[0]['kernel'][0] / 1e6)
            emit(row)
    if not a.trace_case:
        n = 1 << 20
        nonce = np.random.default_rng(3).integers(0, 256, size=(n, 32), dtype=np.uint8); nonce[n - 1] = nonce[0]
        off = np.zeros(n + 1, dtype=np.uint64); rows = np.zeros((n, 128), dtype=np.uint8); flags = np.zeros(n, dtype=np.uint8); key = np.frombuffer(seeds32[0], dtype=np.uint8).copy()
        ts = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); rc = L.aleo_mi355x_signatures_sign(p(rows), p(flags), p(key), 0, p(rows), p(off), p(nonce), n); ts.append(time.perf_counter() - t0)
            assert rc == 2 and b' 0 and %d ' % (n - 1) in L.aleo_mi355x_last_error()
        ts = sorted(ts[1:])
        emit('the check for equal nonce seeds, 2^20 seeds, the last equal to the first (the refusal: the call returns after the check)   %s ms' % ms((ts[len(ts) // 2], ts[0], ts[-1])))
    if a.out and not a.trace_case:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
