#!/usr/bin/env python3
"""The measurements of aleo_mi355x_plaintexts_serial_numbers (profiles/records_plaintexts.txt is this tool's output).

    python tools/plaintexts_bench.py [--sizes 6,8,10,12,14,16,18,20] [--host-max 12] [--threads-max 16] [--reps 7] [--out FILE]
    python tools/plaintexts_bench.py --threshold 3,4,5,6,7 [--out FILE]      # 2^k strings, the GPU road (ALEO_MI355X_MIN_PLAINTEXTS=0) against the host twin on one
                                                                              # thread: the serial-number call with the 2^16 spent rows (the host twin sorts them
                                                                              # in every call), without a spent set, and the commitments call
    python tools/plaintexts_bench.py --trace-case      # one warm and three timed calls of 2^20 strings and nothing else: the run to put under
                                                       # rocprofv3 --kernel-trace --stats, in a run of its own

n plaintext strings of the shape of a credits.aleo record — a private owner, a private u64 named microcredits, sixteen values and nonces in turn, in the layout
record_plaintext renders — under one seeded sk_sig; the set S of 2^16 rows holds the serial numbers of eight of the sixteen among random rows, shuffled.  Roads
to every string's commitment, serial number, microcredits and flag:
  gpu       aleo_mi355x_plaintexts_serial_numbers with ALEO_MI355X_MIN_PLAINTEXTS=0
  host 1    its _host twin on this one thread (up to 2^--host-max strings: 0.2 ms per string)
  host 16   the _host twin over sixteen slices of the batch on sixteen threads of the same build (up to 2^--threads-max)
The parent commit has no road from a plaintext string, so there is no parent column.  All roads must return the same bytes.  Every timing: host buffers, copies
inside the timed call, one warm call, the median of --reps rounds with min..max, the roads in a new seeded order every round, no profiler.  Needs a gfx950
device: there is no fallback."""
import argparse, ctypes, os, random, sys, threading
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import aleo_amd                                         # noqa: E402
from aleo_amd import records, wire                      # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import REF, timed, p, L_ORDER  # noqa: E402
from records_unspent_bench import seeded_rows, ms       # noqa: E402

PROGRAM, RECORD, VARIANTS, THREADS = b'credits.aleo', b'credits', 16, 16


def variants():
    rng = random.Random(77); owner = REF['addresses']['owner']
    return ['{\n  owner: %s.private,\n  microcredits: %du64.private,\n  _nonce: %dgroup.public\n}' % (owner, rng.randrange(1 << 50), rng.randrange(ps.R)) for _ in range(VARIANTS)]


def roads(L, batch, sk, S, threads=THREADS):
    n = len(batch); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p); state = {}
    def buffers(): return np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    tail = (p(sk), p(S) if len(S) else None, len(S))

    def gpu():
        sn, cm, mc, fl = buffers()
        aleo_amd._lib.check(L.aleo_mi355x_plaintexts_serial_numbers(p(sn), p(cm), p(mc), p(fl), tp, p(batch.offsets), n, PROGRAM, RECORD, *tail), 'plaintexts_serial_numbers')
        state['gpu'] = (sn, cm, mc, fl); state['routed'] = int(L.aleo_mi355x_plaintexts_last_routed())

    def host():
        sn, cm, mc, fl = buffers()
        aleo_amd._lib.check(L.aleo_mi355x_plaintexts_serial_numbers_host(p(sn), p(cm), p(mc), p(fl), tp, p(batch.offsets), n, PROGRAM, RECORD, *tail), 'plaintexts_serial_numbers_host')
        state['host'] = (sn, cm, mc, fl)

    cut = [n * t // threads for t in range(threads + 1)]          # the slices' own offsets (from 0) and where their text begins: a caller's bookkeeping, outside the timing
    slices = [(np.ascontiguousarray(batch.offsets[cut[t]:cut[t + 1] + 1] - batch.offsets[cut[t]]), ctypes.c_void_p(tp.value + int(batch.offsets[cut[t]]))) for t in range(threads)]

    def host_threads():
        sn, cm, mc, fl = buffers(); rcs = [0] * threads
        def work(t):
            lo, hi = cut[t], cut[t + 1]
            if hi > lo: rcs[t] = L.aleo_mi355x_plaintexts_serial_numbers_host(p(sn[lo:hi]), p(cm[lo:hi]), p(mc[lo:hi]), p(fl[lo:hi]), slices[t][1], p(slices[t][0]), hi - lo, PROGRAM, RECORD, *tail)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts: t.start()
        for t in ts: t.join()
        assert not any(rcs)
        state['threads'] = (sn, cm, mc, fl)

    def commitments(f, key):
        def call():
            _, cm, mc, fl = buffers()
            aleo_amd._lib.check(f(p(cm), p(mc), p(fl), tp, p(batch.offsets), n, PROGRAM, RECORD), 'plaintexts_commitments')
            state[key] = (cm, mc, fl)
        return call
    state['commitments'] = (commitments(L.aleo_mi355x_plaintexts_commitments, 'cm gpu'), commitments(L.aleo_mi355x_plaintexts_commitments_host, 'cm host'))
    return gpu, host, host_threads, state


def setup(L, n):
    rng = random.Random(n); sk = np.frombuffer(rng.randrange(L_ORDER).to_bytes(32, 'little'), dtype=np.uint8)
    v = variants()
    sn, _, _, flags = records.plaintext_serial_numbers(v, PROGRAM.decode(), RECORD.decode(), sk.tobytes(), host=True)
    assert not flags.any()
    S = np.concatenate([sn[::2], seeded_rows((1 << 16) - len(sn[::2]), 3)]); np.random.default_rng(5).shuffle(S)
    return records.RecordBatch.from_strings([v[i % VARIANTS] for i in range(n)]), sk, np.ascontiguousarray(S)


def same(state, a, b): return all(x.tobytes() == y.tobytes() for x, y in zip(state[a], state[b]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='6,8,10,12,14,16,18,20'); ap.add_argument('--host-max', type=int, default=12); ap.add_argument('--threads-max', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7); ap.add_argument('--threshold'); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    os.environ['ALEO_MI355X_MIN_PLAINTEXTS'] = '0'
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    shown = [arg for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# plaintexts_bench %s' % ' '.join(shown), '# %s' % L.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; half of the strings spent, 2^16 spent rows' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    if a.trace_case:
        batch, sk, S = setup(L, 1 << 20)
        gpu, _, _, state = roads(L, batch, sk, S)
        for _ in range(4): gpu()
        print('trace case: 2^20 strings, %d routed, %d spent' % (state['routed'], int((state['gpu'][3] == 1).sum())))
        return
    if a.threshold:
        for lg in [int(v) for v in a.threshold.split(',')]:
            batch, sk, S = setup(L, 1 << lg)
            gpu, host, _, state = roads(L, batch, sk, S)
            with_set = timed({'gpu': gpu, 'host': host}, a.reps)
            assert same(state, 'gpu', 'host') and state['routed'] == 0
            gpu0, host0, _, state0 = roads(L, batch, sk, S[:0])
            no_set = timed({'gpu': gpu0, 'host': host0}, a.reps)
            cm = timed({'gpu': state0['commitments'][0], 'host': state0['commitments'][1]}, a.reps)
            assert same(state0, 'gpu', 'host') and same(state0, 'cm gpu', 'cm host') and state0['cm gpu'][0].tobytes() == state0['gpu'][1].tobytes()
            emit('2^%-2d strings   ' % lg + '   '.join('%s: gpu %s  host, one thread %s  %5.2fx' % (what, ms(r['gpu']), ms(r['host']), r['host'][0] / r['gpu'][0])
                                                     for what, r in (('serial numbers, 2^16 spent rows', with_set), ('serial numbers, no set', no_set), ('commitments', cm))))
    else:
        for lg in [int(v) for v in a.sizes.split(',')]:
            batch, sk, S = setup(L, 1 << lg)
            gpu, host, host_threads, state = roads(L, batch, sk, S)
            fns = {'gpu': gpu}
            if lg <= a.host_max: fns['host'] = host
            if lg <= a.threads_max: fns['threads'] = host_threads
            r = timed(fns, a.reps)
            assert all(same(state, 'gpu', k) for k in fns if k != 'gpu') and state['routed'] == 0 and int((state['gpu'][3] == 1).sum()) == (1 << lg) // 2 and not (state['gpu'][3] > 1).any()
            one = 'host, one thread %s  %7.2fx' % (ms(r['host']), r['host'][0] / r['gpu'][0]) if 'host' in r else 'host, one thread   not measured'
            many = 'host, %d threads %s  %7.2fx' % (THREADS, ms(r['threads']), r['threads'][0] / r['gpu'][0]) if 'threads' in r else 'host, %d threads   not measured' % THREADS
            emit('2^%-2d strings   gpu %s  %8.3f us per string   %s   %s' % (lg, ms(r['gpu']), r['gpu'][0] * 1e6 / (1 << lg), one, many))
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
