#!/usr/bin/env python3
"""The measurements of aleo_mi355x_accounts_derive and aleo_mi355x_accounts_search (profiles/accounts_derive.txt is this tool's output).

    python tools/accounts_bench.py [--baseline-lib PARENT.so] [--sizes 0,1,2,3,4,5,6,7,8,10,12,16,20] [--search 20,24] [--reps 8] [--threads 16] [--out FILE]
    python tools/accounts_bench.py --trace-case [--sizes 20] [--search 20]     # one warm and three timed calls of each and nothing else: the run to put under
                                                                               # rocprofv3 --kernel-trace --stats, in a run of its own (the program after --)

2^k private keys from a seeded generator.  Roads to the accounts, which must agree byte for byte:
  kernel     aleo_mi355x_accounts_derive with ALEO_MI355X_MIN_ACCOUNTS=0: host buffers, the copies inside the call; with and without the "aleo1…" strings
  host       a loop of aleo_mi355x_account_from_private_key over the keys' strings on one thread — of the library given with --baseline-lib (the parent commit's
             build), else of this one: what a caller had before, and what a batch below min_accounts runs inside the call; with strings, plus one
             aleo_mi355x_bech32m_encode per address
  host x T   the same over T threads, a slice of the keys each (2^10 and more only)
The two columns are two timings of each pair: min_accounts is the smallest power of two at which the kernel beats the one-thread host loop in both.  Every timing:
one warm call, the median of --reps rounds with min..max, the roads in a new seeded order every round, no profiler.  From 2^12 on the host roads are timed on a
slice of 2^10 keys and scaled (they are linear in n; the line says so).  A search: candidates per second through the call for a three-character prefix, every hit
handed out.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys, threading
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_ACCOUNTS'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import account as acct                    # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import timed, p                # noqa: E402
from records_unspent_bench import ms                    # noqa: E402

HOST_SLICE = 1 << 10
PREFIX = 'qpz'


def bind_parent(path):
    """The two calls the host road makes, of another build of the library."""
    B = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    B.aleo_mi355x_account_from_private_key.argtypes = [ctypes.c_char_p, vp, vp, vp]; B.aleo_mi355x_account_from_private_key.restype = ctypes.c_int32
    B.aleo_mi355x_bech32m_encode.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, vp, sz]; B.aleo_mi355x_bech32m_encode.restype = ctypes.c_int32
    B.aleo_mi355x_version.restype = ctypes.c_char_p
    return B


def roads(L, B, n, threads):
    rng = random.Random(n)
    seeds = np.frombuffer(b''.join(rng.randrange(ps.R).to_bytes(32, 'little') for _ in range(n)), dtype=np.uint8).reshape(n, 32).copy()
    hn = min(n, HOST_SLICE)
    keys = [ps.private_key_string(int.from_bytes(seeds[i].tobytes(), 'little')).encode() for i in range(hn)]
    new = lambda m: {k: np.zeros((m, w), dtype=np.uint8) for k, w in (('sk', 32), ('vk', 32), ('ax', 32), ('str', 63))}
    K, H, T = new(n), new(hn), new(hn)
    flags = np.zeros(n, dtype=np.uint8)

    def kernel(strings):
        return lambda: aleo_amd._lib.check(L.aleo_mi355x_accounts_derive(p(seeds), n, p(K['sk']), p(K['vk']), p(K['ax']), p(K['str']) if strings else None, p(flags)), 'accounts_derive')
    def loop(out, lo, hi, strings):
        buf = ctypes.create_string_buffer(80)
        sk, vk, ax, text = (out[k].ctypes.data for k in ('sk', 'vk', 'ax', 'str'))      # plain addresses: the loop's own cost stays a few percent of a key's
        for i in range(lo, hi):
            B.aleo_mi355x_account_from_private_key(keys[i], sk + 32 * i, vk + 32 * i, ax + 32 * i)
            if strings:
                B.aleo_mi355x_bech32m_encode(buf, 80, b'aleo', ax + 32 * i, 32); ctypes.memmove(text + 63 * i, buf, 63)
    def host(strings): return lambda: loop(H, 0, hn, strings)
    def many(strings):
        def run():
            per = (hn + threads - 1) // threads
            ts = [threading.Thread(target=loop, args=(T, t * per, min(hn, (t + 1) * per), strings)) for t in range(threads)]
            for t in ts: t.start()
            for t in ts: t.join()
        return run
    return kernel, host, many, (K, H, T, flags), hn


def search_call(L, master, count, max_hits):
    idx = np.zeros(max_hits, dtype=np.uint64); seeds = np.zeros((max_hits, 32), dtype=np.uint8); n = ctypes.c_size_t(0); nxt = ctypes.c_uint64(0)
    def run(): aleo_amd._lib.check(L.aleo_mi355x_accounts_search(p(master), 0, count, PREFIX.encode(), max_hits, p(idx), p(seeds), ctypes.byref(n), ctypes.byref(nxt)), 'accounts_search')
    return run, n, nxt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-lib'); ap.add_argument('--sizes', default='0,1,2,3,4,5,6,7,8,10,12,16,20'); ap.add_argument('--search', default='20,24')
    ap.add_argument('--reps', type=int, default=8); ap.add_argument('--threads', type=int, default=16); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    B = bind_parent(a.baseline_lib) if a.baseline_lib else L
    shown = [arg if not arg.endswith('.so') else "(the parent commit's build)" for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# accounts_bench %s' % ' '.join(shown), '# new: %s' % L.aleo_mi355x_version().decode(), '# host road through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    master = np.frombuffer(bytes((7 * i + 3) & 0xff for i in range(32)), dtype=np.uint8).copy()
    sizes = [int(v) for v in a.sizes.split(',') if v != '']
    searches = [int(v) for v in a.search.split(',') if v != '']
    if a.trace_case:
        for lg in sizes:
            kernel = roads(L, B, 1 << lg, a.threads)[0]
            for strings in (False, True):
                for _ in range(4): kernel(strings)()
            print('trace case: 2^%d accounts, without and with strings' % lg)
        for lg in searches:
            run, n, nxt = search_call(L, master, 1 << lg, 1 << 12)
            for _ in range(4): run()
            print('trace case: 2^%d candidates, %d hits' % (lg, n.value))
        return
    for strings in (False, True):
        emit('== derive, %s' % ('sk_sig, view key, address x, flags and the 63-character address strings' if strings else 'sk_sig, view key, address x and flags'))
        for lg in sizes:
            n = 1 << lg
            kernel, host, many, (K, H, T, flags), hn = roads(L, B, n, a.threads)
            fns = {'kernel': kernel(strings), 'host': host(strings)}
            if n >= 1 << 10: fns['threads'] = many(strings)
            pairs = [timed(fns, a.reps) for _ in range(2)]
            names = ('sk', 'vk', 'ax') + (('str',) if strings else ())
            assert not flags.any() and all(K[k][:hn].tobytes() == H[k].tobytes() for k in names), 'the roads disagree'
            if 'threads' in fns: assert all(T[k].tobytes() == H[k].tobytes() for k in names)
            scale = n / hn
            up = lambda t: tuple(v * scale for v in t)
            row = '2^%-2d accounts   ' % lg + '   '.join('kernel %s  host, one thread %s  %6.2fx' % (ms(r['kernel']), ms(up(r['host'])), r['host'][0] * scale / r['kernel'][0]) for r in pairs)
            if 'threads' in fns: row += '   host, %d threads %s' % (a.threads, ms(up(pairs[0]['threads'])))
            if scale != 1: row += '   (host roads: 2^10 keys timed, x %d)' % scale
            row += '   %.3f M accounts/s through the call, %.1f us per key on the host' % (n / pairs[0]['kernel'][0] / 1e6, pairs[0]['host'][0] / hn * 1e6)
            emit(row)
        emit('')
    emit('== search, the prefix "%s", every hit handed out (derived again on the host inside the call)' % PREFIX)
    for lg in searches:
        run, n, nxt = search_call(L, master, 1 << lg, 1 << 12)
        r = timed({'search': run}, max(3, a.reps // 2))['search']
        assert nxt.value == 1 << lg
        emit('2^%-2d candidates   search %s   %d hits   %.3f M candidates/s through the call' % (lg, ms(r), n.value, (1 << lg) / r[0] / 1e6))
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
