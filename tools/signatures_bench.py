#!/usr/bin/env python3
"""The measurements of aleo_mi355x_signatures_verify (profiles/signatures_verify.txt is this tool's output).

    python tools/signatures_bench.py [--sizes 4,5,6,7,8,9,10,16,20] [--reps 8] [--threads 16] [--out FILE]
    python tools/signatures_bench.py --trace-case [--sizes 16]      # one warm and three timed calls of one size and nothing else: the run to put under
                                                                     # rocprofv3 --kernel-trace --stats, in a run of its own (the program after --)

2^k signatures of 32-byte messages under 64 accounts, an address per signature; a sixteenth do not verify (another message) and a sixty-fourth are malformed, so the
flags are checked too.  Three roads to the flags, which must agree byte for byte:
  kernel     aleo_mi355x_signatures_verify with ALEO_MI355X_MIN_SIGNATURES=0: host buffers, the copies inside the call
  host       aleo_mi355x_signatures_verify_host on one thread: what a batch below min_signatures runs inside the call
  host x T   the same over T threads, a slice of the batch each (2^10 and more only)
The two columns are two timings of each pair: min_signatures is the smallest power of two at which the kernel beats the one-thread host path in both.  Every
timing: one warm call, the median of --reps rounds with min..max, the roads in a new seeded order every round, no profiler.  From 2^16 on the host roads are
timed on a slice of 2^12 signatures and scaled (they are linear in n; the line says so).  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys, threading
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_SIGNATURES'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records, signature as sg           # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import timed, p                # noqa: E402
from records_unspent_bench import ms                    # noqa: E402

ACCOUNTS, POOL, HOST_SLICE = 64, 4096, 1 << 12


def pool():
    """POOL (signature, address x, message) triples, valid, under ACCOUNTS seeded accounts."""
    rng = random.Random(11)
    accts = [records.Account.from_private_key(ps.private_key_string(rng.randrange(ps.R))) for _ in range(ACCOUNTS)]
    out = []
    for k in range(POOL):
        a = accts[k % ACCOUNTS]; m = rng.randbytes(32)
        out.append((sg.sign(a.private_key, m, rng.randbytes(32)).bytes, a.address_x, m))
    return out


def batch(n, triples):
    rng = random.Random(n)
    sigs, addrs, msgs, want = [], [], [], np.zeros(n, dtype=np.uint8)
    for i in range(n):
        s, ax, m = triples[rng.randrange(POOL)]
        if i % 16 == 5: m = m[::-1]; want[i] = 1
        if i % 64 == 9: s = s[:32] + b'\xff' * 32 + s[64:]; want[i] = 3
        sigs.append(s); addrs.append(ax); msgs.append(m)
    off = np.arange(n + 1, dtype=np.uint64) * 32
    return (np.frombuffer(b''.join(sigs), dtype=np.uint8).copy(), np.frombuffer(b''.join(addrs), dtype=np.uint8).copy(), np.frombuffer(b''.join(msgs), dtype=np.uint8).copy(), off, want)


def roads(L, B, n, threads):
    sigs, addrs, msgs, off, want = B
    state = {k: np.zeros(n, dtype=np.uint8) for k in ('kernel', 'host', 'threads')}
    hn = min(n, HOST_SLICE)

    def kernel(): aleo_amd._lib.check(L.aleo_mi355x_signatures_verify(p(state['kernel']), p(sigs), p(addrs), 32, p(msgs), p(off), n), 'signatures_verify')
    def host(): aleo_amd._lib.check(L.aleo_mi355x_signatures_verify_host(p(state['host']), p(sigs), p(addrs), 32, p(msgs), p(off), hn), 'signatures_verify_host')
    def many():
        per = (hn + threads - 1) // threads
        def work(t):
            lo, hi = t * per, min(hn, (t + 1) * per)
            if lo < hi: L.aleo_mi355x_signatures_verify_host(p(state['threads'][lo:hi]), p(sigs[128 * lo:]), p(addrs[32 * lo:]), 32, p(msgs[32 * lo:]), p(off[:hi - lo + 1]), hi - lo)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts: t.start()
        for t in ts: t.join()
    return kernel, host, many, state, want, hn


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='4,5,6,7,8,9,10,16,20'); ap.add_argument('--reps', type=int, default=8); ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    triples = pool()
    shown = [arg for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# signatures_bench %s' % ' '.join(shown), '# %s' % L.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; 32-byte messages, an address per signature, %d accounts' % (a.reps, ACCOUNTS), '']
    def emit(row): lines.append(row); print(row, flush=True)
    for lg in [int(v) for v in a.sizes.split(',')]:
        n = 1 << lg
        kernel, host, many, state, want, hn = roads(L, batch(n, triples), n, a.threads)
        if a.trace_case:
            for _ in range(4): kernel()
            assert state['kernel'].tobytes() == want.tobytes()
            print('trace case: 2^%d signatures' % lg); continue
        scale = n / hn
        fns = {'kernel': kernel, 'host': host}
        if n >= 1 << 10: fns['threads'] = many
        pairs = [timed(fns, a.reps) for _ in range(2)]
        assert state['kernel'].tobytes() == want.tobytes() and state['host'][:hn].tobytes() == want[:hn].tobytes(), 'the roads disagree'
        if 'threads' in fns: assert state['threads'][:hn].tobytes() == want[:hn].tobytes()
        up = lambda t: tuple(v * scale for v in t)
        row = '2^%-2d signatures   ' % lg + '   '.join('kernel %s  host, one thread %s  %6.2fx' % (ms(r['kernel']), ms(up(r['host'])), r['host'][0] * scale / r['kernel'][0]) for r in pairs)
        if 'threads' in fns: row += '   host, %d threads %s' % (a.threads, ms(up(pairs[0]['threads'])))
        if scale != 1: row += '   (host roads: 2^12 signatures timed, x %d)' % scale
        row += '   %.3f M signatures/s through the call' % (n / pairs[0]['kernel'][0] / 1e6)
        emit(row)
    if a.out and not a.trace_case:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
