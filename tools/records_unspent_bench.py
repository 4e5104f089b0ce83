#!/usr/bin/env python3
"""The measurements of unspent_strings / unspent_strings_many (profiles/records_unspent.txt is this tool's output).

    python tools/records_unspent_bench.py --keys K [--baseline-lib PATH] [--sizes 20] [--fractions 0.001,0.01,0.1,1] [--spent 16,22] [--reps 8] [--out FILE]
    python tools/records_unspent_bench.py --few 1,8,32 [--baseline-lib PATH] [--sizes 16]      # K = 1 and that many owned records: the serial numbers on the
                                                                                               # device (ALEO_MI355X_MIN_SERIALS=1) and on the host inside the call
    python tools/records_unspent_bench.py --keys 8 --trace-case      # one warm and three timed calls of the 2^20 / 1 % case and nothing else: the run to put under
                                                                     # rocprofv3 --kernel-trace --stats, in a run of its own

The strings, the accounts and their records are those of tools/records_found_bench.py --keys K: n strings of the shape of a credits.aleo record, every account
owning the given fraction of them.  A seeded commitment per string; every account signs with a seeded sk_sig; half of every account's records are spent, and the
set S of 2^spent rows holds their serial numbers among random rows, shuffled.  Two roads to every account's unspent records, serial numbers and microcredits:
  new      aleo_mi355x_records_unspent_strings_many (K = 1: _strings) and K x aleo_mi355x_found_free
  parent   what a caller of the parent commit's library ran (--baseline-lib: a build of that commit; without it this build's same functions):
           records_decrypt_strings_many (K = 1: records_decrypt_strings), then found_serial_numbers per account, then a filter in Python through a set of the
           32-byte rows of S (built outside the timed call, in the parent's favour), then the frees
Both roads must keep the same records.  Every timing: host buffers, copies inside the timed call, one warm call, the median of --reps rounds with min..max, the
roads in a new seeded order every round, no profiler.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_RECORDS'] = '0'; os.environ['ALEO_MI355X_MIN_DECRYPT'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records                            # noqa: E402
from records_found_bench import accounts_of, make_many, foreign_pool, timed, p, L_ORDER      # noqa: E402


def bind(path):
    B = ctypes.CDLL(os.path.abspath(path))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    B.aleo_mi355x_records_decrypt_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp]
    B.aleo_mi355x_records_decrypt_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, sz]
    B.aleo_mi355x_found_serial_numbers.argtypes = [vp, vp, sz, vp, vp, vp]
    for name in ('count', 'fields'): getattr(B, 'aleo_mi355x_found_' + name).argtypes = [vp]; getattr(B, 'aleo_mi355x_found_' + name).restype = sz
    for name in ('index', 'status', 'microcredits'): getattr(B, 'aleo_mi355x_found_' + name).argtypes = [vp]; getattr(B, 'aleo_mi355x_found_' + name).restype = vp
    B.aleo_mi355x_found_free.argtypes = [vp]; B.aleo_mi355x_found_free.restype = None
    B.aleo_mi355x_version.restype = ctypes.c_char_p
    return B


def seeded_rows(n, seed):
    """n rows of 32 bytes below r (the top byte below 0x12)."""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    return a


def roads(L, B, batch, accounts, cm, sks, S):
    n = len(batch); K = len(accounts); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p)
    vks = np.frombuffer(b''.join(a[0].to_bytes(32, 'little') for a in accounts), dtype=np.uint8); axs = np.frombuffer(b''.join(a[1].to_bytes(32, 'little') for a in accounts), dtype=np.uint8)
    spent_set = {r.tobytes() for r in S}                        # the parent road's caller holds S like this
    state = {}

    def new(S=S):
        out = (ctypes.c_void_p * K)()
        tail = (p(S) if len(S) else None, len(S))
        if K == 1: rc = L.aleo_mi355x_records_unspent_strings(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), *tail)
        else: rc = L.aleo_mi355x_records_unspent_strings_many(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), K, *tail)
        aleo_amd._lib.check(rc, 'records_unspent_strings')
        got = []
        for j in range(K):
            h = ctypes.c_void_p(out[j]); c = int(L.aleo_mi355x_found_count(h))
            got.append((np.frombuffer(ctypes.string_at(L.aleo_mi355x_found_index(h), 4 * c), dtype=np.uint32).copy(), np.frombuffer(ctypes.string_at(L.aleo_mi355x_found_serials(h), 32 * c), dtype=np.uint8).reshape(-1, 32).copy(),
                        int(L.aleo_mi355x_found_owned(h))))
            L.aleo_mi355x_found_free(h)
        state['new'] = got

    def parent():
        out = (ctypes.c_void_p * K)()
        if K == 1: assert B.aleo_mi355x_records_decrypt_strings(out, tp, p(batch.offsets), n, p(vks), p(axs)) == 0
        else: assert B.aleo_mi355x_records_decrypt_strings_many(out, tp, p(batch.offsets), n, p(vks), p(axs), K) == 0
        got = []
        for j in range(K):
            h = ctypes.c_void_p(out[j]); c = int(B.aleo_mi355x_found_count(h))
            sn = np.zeros((c, 32), dtype=np.uint8); fl = np.zeros(c, dtype=np.uint8)
            assert B.aleo_mi355x_found_serial_numbers(h, p(cm), n, p(sks[32 * j:32 * j + 32].copy()), p(sn), p(fl)) == 0
            index = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_index(h), 4 * c), dtype=np.uint32); status = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_status(h), c), dtype=np.uint8)
            mc = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_microcredits(h), 8 * c), dtype=np.uint64)
            raw = sn.tobytes()
            keep = [k for k in range(c) if status[k] == 0 and fl[k] == 0 and raw[32 * k:32 * k + 32] not in spent_set]
            got.append((index[keep], sn[keep], c, int(mc[keep].sum(dtype=np.uint64)) if keep else 0))
            B.aleo_mi355x_found_free(h)
        state['parent'] = got

    return new, parent, state


def shape(L, B, n, K, fraction, lg_spent, pool, accounts, owned_each=None):
    batch, per = make_many(n, fraction, pool, accounts) if owned_each is None else make_many(n, owned_each / n, pool, accounts)
    cm = seeded_rows(n, 7 * n + K); rng = random.Random(n + K)
    sks = np.frombuffer(b''.join(rng.randrange(L_ORDER).to_bytes(32, 'little') for _ in range(K)), dtype=np.uint8)
    nothing = np.zeros((0, 32), dtype=np.uint8)
    new, _, state = roads(L, B, batch, accounts, cm, sks, nothing)
    new()                                                       # setup: every account's serial numbers
    half = np.concatenate([sn[::2] for _, sn, _ in state['new']])
    n_spent = max(1 << lg_spent, len(half)) if lg_spent is not None else len(half)
    S = np.concatenate([half, seeded_rows(n_spent - len(half), 3)]); np.random.default_rng(5).shuffle(S)
    return batch, per, cm, sks, np.ascontiguousarray(S)


def same_kept(state, K):
    return all(state['new'][j][0].tobytes() == state['parent'][j][0].tobytes() and state['new'][j][1].tobytes() == state['parent'][j][1].tobytes() and state['new'][j][2] == state['parent'][j][2] for j in range(K))


def ms(t): return '%9.3f (%.3f..%.3f)' % tuple(v * 1e3 for v in t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-lib'); ap.add_argument('--keys', type=int, default=1); ap.add_argument('--sizes', default='20'); ap.add_argument('--fractions', default='0.01')
    ap.add_argument('--spent', default='16'); ap.add_argument('--reps', type=int, default=8); ap.add_argument('--few'); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    B = bind(a.baseline_lib) if a.baseline_lib else L
    pool = foreign_pool(); K = a.keys; accounts = accounts_of(K)
    lines = ['# records_unspent_bench %s' % ' '.join(arg if not arg.endswith('.so') else '(the parent commit\'s build)' for arg in sys.argv[1:]),
             '# new: %s' % L.aleo_mi355x_version().decode(), '# parent road through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; %% owned: per account; half of the owned spent' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    if a.trace_case:
        batch, per, cm, sks, S = shape(L, B, 1 << 20, K, 0.01, 16, pool, accounts)
        new, _, state = roads(L, L, batch, accounts, cm, sks, S)
        for _ in range(4): new()
        print('trace case: 2^20 strings, %d accounts, %d owned and %d kept each, 2^16 spent rows' % (K, state['new'][0][2], len(state['new'][0][0])))
        return
    if a.few:
        for lg in [int(v) for v in a.sizes.split(',')]:
            for owned in [int(v) for v in a.few.split(',')]:
                batch, per, cm, sks, S = shape(L, B, 1 << lg, 1, None, None, pool, accounts[:1], owned_each=owned)
                new, parent, state = roads(L, B, batch, accounts[:1], cm, sks, S)
                def on(threshold): os.environ['ALEO_MI355X_MIN_SERIALS'] = threshold; new()
                r = timed({'device': lambda: on('1'), 'host': lambda: on('1000000'), 'parent': parent}, a.reps)
                os.environ.pop('ALEO_MI355X_MIN_SERIALS')
                parent(); new(); assert same_kept(state, 1), 'the roads keep different records'
                emit('2^%-2d x 1 key %4d owned, %4d spent rows   new, serial numbers on the device %s   new, on the host inside the call %s   parent (its own routing) %s' % (lg, per, len(S), ms(r['device']), ms(r['host']), ms(r['parent'])))
    else:
        for lg in [int(v) for v in a.sizes.split(',')]:
            for fr in [float(v) for v in a.fractions.split(',')]:
                for lg_spent in [int(v) for v in a.spent.split(',')]:
                    batch, per, cm, sks, S = shape(L, B, 1 << lg, K, fr, lg_spent, pool, accounts)
                    new, parent, state = roads(L, B, batch, accounts, cm, sks, S)
                    r = timed({'new': new, 'parent': parent}, a.reps)
                    assert same_kept(state, K) and all(len(g[0]) == per - (per + 1) // 2 for g in state['new']), 'the roads keep different records'
                    spread = r['parent'][2] - r['parent'][1]
                    verdict = 'slower by more than the parent road\'s spread' if r['new'][0] > r['parent'][0] + spread else ''
                    emit('2^%-2d x %d keys %5.1f %% owned (%7d each)  2^%-2d spent rows   new %s   parent %s   %5.2fx  %s' % (lg, K, 100 * fr, per, lg_spent, ms(r['new']), ms(r['parent']), r['parent'][0] / r['new'][0], verdict))
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
