#!/usr/bin/env python3
"""The measurements of aleo_mi355x_records_encrypt (profiles/records_encrypt.txt is this tool's output).

    python tools/records_encrypt_bench.py [--sizes 5,6,8,10,12,14,16,18,20] [--host-max 12] [--threads-max 16] [--reps 7] [--out FILE]
    python tools/records_encrypt_bench.py --threshold 3,4,5,6,7 [--out FILE]      # 2^k strings, the GPU road (ALEO_MI355X_MIN_ENCRYPT=0) against the host twin on one thread
    python tools/records_encrypt_bench.py --trace-case [--trace-lg 20]      # one warm and three timed calls of 2^20 (2^--trace-lg) strings and nothing else: the run
                                                            # to put under rocprofv3 --kernel-trace --stats, in a run of its own, for the kernel-alone times

n plaintext strings of the shape of a credits.aleo record — a private owner, a private u64 named microcredits, sixteen values in turn, in the layout
record_plaintext renders — each under a randomizer of its own (seeded), mode ALEO_MI355X_ENCRYPT_SET_NONCE: what a producer with a template does.  Roads to every
string's record1… string, flag and record view key:
  gpu       aleo_mi355x_records_encrypt with ALEO_MI355X_MIN_ENCRYPT=0
  host 1    its _host twin on this one thread (up to 2^--host-max strings)
  host 16   the _host twin over sixteen slices of the batch on sixteen threads of the same build (up to 2^--threads-max)
The parent commit has no road from a plaintext to a ciphertext, so there is no parent column.  All roads must return the same bytes.  Every timing: host buffers,
copies inside the timed call, the result read through its accessors and freed, one warm call, the median of --reps rounds with min..max, the roads in a new seeded
order every round, no profiler.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys, threading
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import aleo_amd                                         # noqa: E402
from aleo_amd import records                            # noqa: E402
from records_found_bench import REF, timed, p  # noqa: E402
from records_unspent_bench import ms                    # noqa: E402

VARIANTS, THREADS, MODE = 16, 16, 1


def variants():
    rng = random.Random(78); owner = REF['addresses']['owner']
    return ['{\n  owner: %s.private,\n  microcredits: %du64.private,\n  _nonce: 0group.public\n}' % (owner, rng.randrange(1 << 50)) for _ in range(VARIANTS)]


def setup(n):
    v = variants()
    rs = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8); rs[:, 31] &= 0x03      # below 2^250 < l
    return records.RecordBatch.from_strings([v[i % VARIANTS] for i in range(n)]), np.ascontiguousarray(rs)


def read(L, out, n):
    """What a caller does with a result: the offsets, the text, the flags and the keys copied out, the result freed."""
    off = np.frombuffer(ctypes.string_at(L.aleo_mi355x_encrypted_offsets(out), 8 * (n + 1)), dtype=np.uint64)
    got = (ctypes.string_at(L.aleo_mi355x_encrypted_text(out), int(off[-1])), off, ctypes.string_at(L.aleo_mi355x_encrypted_flags(out), n), ctypes.string_at(L.aleo_mi355x_encrypted_rvk(out), 32 * n))
    L.aleo_mi355x_encrypted_free(out)
    return got


def roads(L, batch, rs, threads=THREADS):
    n = len(batch); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p); state = {}

    def call(f, key):
        def run():
            out = ctypes.c_void_p()
            aleo_amd._lib.check(f(ctypes.byref(out), tp, p(batch.offsets), n, p(rs), MODE), 'records_encrypt')
            state[key] = read(L, out, n)
            if key == 'gpu': state['routed'] = int(L.aleo_mi355x_records_encrypt_last_routed())
        return run

    cut = [n * t // threads for t in range(threads + 1)]          # the slices' own offsets (from 0) and where their text begins: a caller's bookkeeping, outside the timing
    slices = [(np.ascontiguousarray(batch.offsets[cut[t]:cut[t + 1] + 1] - batch.offsets[cut[t]]), ctypes.c_void_p(tp.value + int(batch.offsets[cut[t]]))) for t in range(threads)]

    def host_threads():
        parts = [None] * threads
        def work(t):
            lo, hi = cut[t], cut[t + 1]
            if hi == lo: return
            out = ctypes.c_void_p()
            if L.aleo_mi355x_records_encrypt_host(ctypes.byref(out), slices[t][1], p(slices[t][0]), hi - lo, p(rs[lo:hi]), MODE) == 0: parts[t] = read(L, out, hi - lo)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts: t.start()
        for t in ts: t.join()
        parts = [q for t, q in enumerate(parts) if cut[t + 1] > cut[t]]
        assert all(q is not None for q in parts)
        state['threads'] = (b''.join(q[0] for q in parts), None, b''.join(q[2] for q in parts), b''.join(q[3] for q in parts))
    return call(L.aleo_mi355x_records_encrypt, 'gpu'), call(L.aleo_mi355x_records_encrypt_host, 'host'), host_threads, state


def same(state, a, b): return all(x is None or y is None or bytes(x) == bytes(y) for x, y in zip(state[a], state[b]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='5,6,8,10,12,14,16,18,20'); ap.add_argument('--host-max', type=int, default=12); ap.add_argument('--threads-max', type=int, default=16)
    ap.add_argument('--reps', type=int, default=7); ap.add_argument('--threshold'); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true'); ap.add_argument('--trace-lg', type=int, default=20)
    a = ap.parse_args()
    os.environ['ALEO_MI355X_MIN_ENCRYPT'] = '0'
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    shown = [arg for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']
    lines = ['# records_encrypt_bench %s' % ' '.join(shown), '# %s' % L.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; a randomizer per string, the nonce set' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    if a.trace_case:
        batch, rs = setup(1 << a.trace_lg)
        gpu, _, _, state = roads(L, batch, rs)
        for _ in range(4): gpu()
        print('trace case: 2^%d strings, %d routed, %d characters out' % (a.trace_lg, state['routed'], len(state['gpu'][0])))
        return
    if a.threshold:
        for lg in [int(v) for v in a.threshold.split(',')]:
            batch, rs = setup(1 << lg)
            gpu, host, _, state = roads(L, batch, rs)
            r = timed({'gpu': gpu, 'host': host}, a.reps)
            assert same(state, 'gpu', 'host') and state['routed'] == 0 and not any(state['gpu'][2])
            emit('2^%-2d strings   gpu %s  host, one thread %s  %5.2fx' % (lg, ms(r['gpu']), ms(r['host']), r['host'][0] / r['gpu'][0]))
    else:
        for lg in [int(v) for v in a.sizes.split(',')]:
            batch, rs = setup(1 << lg)
            gpu, host, host_threads, state = roads(L, batch, rs)
            fns = {'gpu': gpu}
            if lg <= a.host_max: fns['host'] = host
            if lg <= a.threads_max: fns['threads'] = host_threads
            r = timed(fns, a.reps)
            assert all(same(state, 'gpu', k) for k in fns if k != 'gpu') and state['routed'] == 0 and not any(state['gpu'][2])
            one = 'host, one thread %s  %7.2fx' % (ms(r['host']), r['host'][0] / r['gpu'][0]) if 'host' in r else 'host, one thread   not measured'
            many = 'host, %d threads %s  %7.2fx' % (THREADS, ms(r['threads']), r['threads'][0] / r['gpu'][0]) if 'threads' in r else 'host, %d threads   not measured' % THREADS
            emit('2^%-2d strings   gpu %s  %8.3f us per string   %s   %s' % (lg, ms(r['gpu']), r['gpu'][0] * 1e6 / (1 << lg), one, many))
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
