#!/usr/bin/env python3
"""The measurements of aleo_mi355x_private_keys_open (profiles/key_ciphertexts.txt is this tool's output).

    python tools/key_ciphertexts_bench.py [--baseline-lib PARENT.so] [--sizes 4,5,6,7,8,9,10,11,12,16,20] [--reps 8] [--out FILE]
    python tools/key_ciphertexts_bench.py --trace-case [--sizes 10,16,20]      # one warm and three timed calls of each and nothing else: the run to put under
                                                                               # rocprofv3 --kernel-trace --stats, in a run of its own (the program after --)

2^k (ciphertext, secret) pairs: a pool of up to 2^12 different private keys, each encrypted by the library's host code under a secret of its own of 8 to 24 bytes and
a nonce of its own, repeated in a seeded order up to the size (no lane's work depends on its neighbours'); every pair opens.  Roads, which must agree byte for byte:
  open          aleo_mi355x_private_keys_open with ALEO_MI355X_MIN_KEY_CIPHERTEXTS=0: host buffers, the copies inside the call — the seeds alone, and every
                account output (sk_sig, view key, address x, the address strings) with them
  host          aleo_mi355x_private_keys_open_host on one thread: what a batch below min_key_ciphertexts runs inside the call.  From 2^10 on it is timed on a slice
                of 2^8 pairs and scaled (it is linear in n; the line says so)
  derive        the floor for the account half: aleo_mi355x_accounts_derive (ALEO_MI355X_MIN_ACCOUNTS=0) on the same seeds with the same account outputs — of the
                library given with --baseline-lib (the parent commit's build), else of this one.  The combined call should cost no more than this plus the
                seeds-only open: it saves a download and an upload of the seeds
The two columns are two timings of each pair: min_key_ciphertexts is the smallest power of two at which the open call beats the one-thread host road in both, with
the seeds alone and with the account outputs, the larger of the two.  Every timing: one warm call, the median of --reps rounds with min..max, the roads in a new
seeded order every round, no profiler.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_KEY_CIPHERTEXTS'] = '0'
os.environ['ALEO_MI355X_MIN_ACCOUNTS'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import key_ciphertext as kc               # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import timed, p                # noqa: E402
from records_unspent_bench import ms                    # noqa: E402

POOL, HOST_SLICE = 1 << 12, 1 << 8


def bind_parent(path):
    B = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    B.aleo_mi355x_accounts_derive.argtypes = [vp, sz, vp, vp, vp, vp, vp]; B.aleo_mi355x_accounts_derive.restype = ctypes.c_int32
    B.aleo_mi355x_version.restype = ctypes.c_char_p
    return B


def make_pool(k):
    rng = random.Random(17)
    out = []
    for _ in range(k):
        seed = rng.randrange(ps.R); secret = bytes(rng.randrange(33, 127) for _ in range(rng.randrange(8, 25)))
        out.append((kc.encrypt(ps.private_key_string(seed), secret, rng.randrange(ps.R)).encode(), secret, seed.to_bytes(32, 'little')))
    return out


def roads(L, B, pool, n):
    rng = random.Random(n)
    picks = [pool[rng.randrange(len(pool))] for _ in range(n)] if n > len(pool) else pool[:n]
    hn = min(n, HOST_SLICE) if n >= 1 << 10 else n
    def blobs(items):
        text = b''.join(c for c, _, _ in items); sec = b''.join(s for _, s, _ in items)
        off = np.zeros(len(items) + 1, np.uint64); off[1:] = np.cumsum([len(c) for c, _, _ in items], dtype=np.uint64)
        soff = np.zeros(len(items) + 1, np.uint64); soff[1:] = np.cumsum([len(s) for _, s, _ in items], dtype=np.uint64)
        return np.frombuffer(text, np.uint8).copy(), off, np.frombuffer(sec, np.uint8).copy(), soff
    text, off, sec, soff = blobs(picks); htext, hoff, hsec, hsoff = blobs(picks[:hn])
    want = np.frombuffer(b''.join(s for _, _, s in picks), np.uint8).reshape(n, 32).copy()
    new = lambda m: {k: np.zeros((m, w), np.uint8) for k, w in (('seeds', 32), ('sk', 32), ('vk', 32), ('ax', 32), ('str', 63))}
    K, H, D = new(n), new(hn), new(n)
    flags, hflags, dflags = np.zeros(n, np.uint8), np.zeros(hn, np.uint8), np.zeros(n, np.uint8)
    acc = lambda O, on: [p(O[k]) if on else None for k in ('sk', 'vk', 'ax', 'str')]
    def opened(accounts): return lambda: aleo_amd._lib.check(L.aleo_mi355x_private_keys_open(p(text), p(off), p(sec), p(soff), n, p(K['seeds']), *acc(K, accounts), p(flags)), 'private_keys_open')
    def host(accounts): return lambda: aleo_amd._lib.check(L.aleo_mi355x_private_keys_open_host(p(htext), p(hoff), p(hsec), p(hsoff), hn, p(H['seeds']), *acc(H, accounts), p(hflags)), 'private_keys_open_host')
    def derive(): return lambda: aleo_amd._lib.check(B.aleo_mi355x_accounts_derive(p(want), n, *acc(D, True), p(dflags)), 'accounts_derive')
    return opened, host, derive, (K, H, D, flags, hflags, dflags, want), hn


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-lib'); ap.add_argument('--sizes', default='4,5,6,7,8,9,10,11,12,16,20'); ap.add_argument('--reps', type=int, default=8); ap.add_argument('--out')
    ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    B = bind_parent(a.baseline_lib) if a.baseline_lib else L
    shown = [arg if not arg.endswith('.so') else "(the parent commit's build)" for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# key_ciphertexts_bench %s' % ' '.join(shown), '# new: %s' % L.aleo_mi355x_version().decode(), '# derive road through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    sizes = [int(v) for v in a.sizes.split(',') if v != '']
    pool = make_pool(min(POOL, 1 << max(sizes)))
    if a.trace_case:
        for lg in sizes:
            opened = roads(L, B, pool, 1 << lg)[0]
            for accounts in (False, True):
                for _ in range(4): opened(accounts)()
            print('trace case: 2^%d pairs, the seeds alone and with the account outputs' % lg)
        return
    alone = {}
    for accounts in (False, True):
        emit('== open, %s' % ('seeds, sk_sig, view key, address x, the 63-character address strings and flags' if accounts else 'seeds and flags'))
        for lg in sizes:
            n = 1 << lg
            opened, host, derive, (K, H, D, flags, hflags, dflags, want), hn = roads(L, B, pool, n)
            fns = {'open': opened(accounts), 'host': host(accounts)}
            if accounts: fns['derive'] = derive()
            pairs = [timed(fns, a.reps) for _ in range(2)]
            names = ('seeds',) + (('sk', 'vk', 'ax', 'str') if accounts else ())
            assert not flags.any() and not hflags.any() and K['seeds'].tobytes() == want.tobytes() and all(K[k][:hn].tobytes() == H[k].tobytes() for k in names), 'the roads disagree'
            if accounts: assert not dflags.any() and all(K[k].tobytes() == D[k].tobytes() for k in names[1:]), 'the account kernel behind the open disagrees with accounts_derive'
            scale = n / hn
            up = lambda t: tuple(v * scale for v in t)
            row = '2^%-2d pairs   ' % lg + '   '.join('open %s  host, one thread %s  %6.2fx' % (ms(r['open']), ms(up(r['host'])), r['host'][0] * scale / r['open'][0]) for r in pairs)
            if accounts:
                row += '   accounts_derive alone %s' % ms(pairs[0]['derive'])
                if lg in alone: row += '   + the seeds-only open %.3f = %.3f ms against %.3f' % (alone[lg] * 1e3, (alone[lg] + pairs[0]['derive'][0]) * 1e3, pairs[0]['open'][0] * 1e3)
            else: alone[lg] = pairs[0]['open'][0]
            if scale != 1: row += '   (host road: 2^8 pairs timed, x %d)' % scale
            row += '   %.3f M pairs/s through the call, %.1f us per pair on the host' % (n / pairs[0]['open'][0] / 1e6, pairs[0]['host'][0] / hn * 1e6)
            emit(row)
        emit('')
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
