#!/usr/bin/env python3
"""The measurements of unspent_named / unspent_named_many and of records_commitments_found (profiles/records_commit.txt is this tool's output).

    python tools/records_commit_bench.py --keys K [--baseline-lib PATH] [--sizes 20] [--fractions 0.001,0.01,0.1] [--reps 8] [--out FILE]
    python tools/records_commit_bench.py --threshold 4,5,6,7,8,10,14 [--out FILE]      # the stand-alone call over 2^k owned records: the kernel
                                                                                        # (ALEO_MI355X_MIN_COMMITMENTS=0) against the host path on one thread, twice
    python tools/records_commit_bench.py --keys 8 --trace-case      # one warm and three timed calls of the 2^20 / 1 % case and nothing else: the run to put under
                                                                    # rocprofv3 --kernel-trace --stats, in a run of its own

n strings of the shape of a credits.aleo record (tools/records_found_bench.py's foreign pool); every account owns the given fraction of them, drawn from 16
records of its own (a private owner, a private u64 named microcredits, sixteen values and nonces).  Every account signs with a seeded sk_sig; the serial numbers
of eight of its sixteen records are spent — half of what it owns — and the set S of 2^16 rows holds them among random rows, shuffled.  Three roads to every
account's unspent records, commitments and serial numbers:
  new      aleo_mi355x_records_unspent_named_many (K = 1: _named) and K x aleo_mi355x_found_free
  parent   what a caller without commitments ran on the parent commit's library (--baseline-lib: a build of that commit; without it this build's same
           functions): records_decrypt_strings_many (K = 1: records_decrypt_strings), aleo_mi355x_record_commitment per owned record on this one thread, the rows
           scattered to a row per string, records_unspent_strings_many (K = 1: _strings), the frees
  floor    this build's records_unspent_strings[_many] handed those commitments for free: what is left of `new` is what the commitment stage costs
All roads must keep the same records with the same serial numbers.  Every timing: host buffers, copies inside the timed call, one warm call, the median of
--reps rounds with min..max, the roads in a new seeded order every round, no profiler.  Needs a gfx950 device: there is no fallback."""
import argparse, ctypes, os, random, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
os.environ['ALEO_MI355X_MIN_RECORDS'] = '0'; os.environ['ALEO_MI355X_MIN_DECRYPT'] = '0'
import aleo_amd                                         # noqa: E402
from aleo_amd import records, wire                      # noqa: E402
from oracle import poseidon as ps                       # noqa: E402
from records_found_bench import REF, foreign_pool, timed, p, L_ORDER      # noqa: E402
from records_unspent_bench import seeded_rows, ms       # noqa: E402

PROGRAM, RECORD, VARIANTS = b'credits.aleo', b'credits', 16


def bind(path):
    B = ctypes.CDLL(os.path.abspath(path))
    vp, sz, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    B.aleo_mi355x_records_decrypt_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp]
    B.aleo_mi355x_records_decrypt_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, sz]
    B.aleo_mi355x_records_unspent_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, vp, vp, vp, sz]
    B.aleo_mi355x_records_unspent_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, vp, vp, sz, vp, sz]
    B.aleo_mi355x_record_commitment.argtypes = [vp, cp, vp, sz, cp, cp]
    for name in ('count', 'fields', 'owned'): getattr(B, 'aleo_mi355x_found_' + name).argtypes = [vp]; getattr(B, 'aleo_mi355x_found_' + name).restype = sz
    for name in ('index', 'status', 'offsets', 'plain', 'serials'): getattr(B, 'aleo_mi355x_found_' + name).argtypes = [vp]; getattr(B, 'aleo_mi355x_found_' + name).restype = vp
    B.aleo_mi355x_found_free.argtypes = [vp]; B.aleo_mi355x_found_free.restype = None
    B.aleo_mi355x_version.restype = ctypes.c_char_p
    return B


def accounts_of(K):
    """K (view key scalar, address x, its VARIANTS credits records) under the reference's generator."""
    G = ps.ed_mul(ps.address_point(REF['addresses']['owner']), pow(ps.view_key_scalar(REF['view_keys']['owner']), -1, L_ORDER))
    dom = ps.domain_separator('AleoSymmetricEncryption0'); le = lambda v: v.to_bytes(32, 'little')
    out = []
    for j in range(K):
        rng = random.Random(100 + j)
        vk = rng.randrange(1, L_ORDER); ax = ps.ed_mul(G, vk)[0]; mine = []
        for v in range(VARIANTS):
            N = ps.ed_mul(G, rng.randrange(1, L_ORDER)); rvk = ps.ed_mul(N, vk)[0]
            plain = [ax, (12 << 2) | (64 << 10) | ((1000 * j + v) << 26) | (1 << 90)]      # PLAINTEXT BITS of a u64 literal and the terminus
            c = [(a + b) % ps.R for a, b in zip(plain, ps.hash_many_psd8([dom, rvk], 2))]
            mine.append(wire.bech32m_encode('record', b'\x01\x01\x00' + le(c[0]) + b'\x01\x0cmicrocredits\x23\x00\x02\x01\x00' + le(c[1]) + le(N[0])))
        out.append((vk, ax, mine))
    return out


def make_many(n, fraction, pool, accounts):
    """Every account owns round(n x fraction) strings, its records in turn; no string has two owners."""
    rng = random.Random(n + len(accounts)); per = max(1, round(n * fraction))
    picked = rng.sample(range(n), per * len(accounts))
    strings = [pool[rng.randrange(len(pool))] for _ in range(n)]
    for j, (_, _, mine) in enumerate(accounts):
        for k, i in enumerate(picked[j * per:(j + 1) * per]): strings[i] = mine[k % VARIANTS]
    return records.RecordBatch.from_strings(strings), per


def results(Lib, out, K, commitments=False):
    got = []
    for j in range(K):
        h = ctypes.c_void_p(out[j]); c = int(Lib.aleo_mi355x_found_count(h))
        got.append((np.frombuffer(ctypes.string_at(Lib.aleo_mi355x_found_index(h), 4 * c), dtype=np.uint32).copy(),
                    np.frombuffer(ctypes.string_at(Lib.aleo_mi355x_found_serials(h), 32 * c), dtype=np.uint8).reshape(-1, 32).copy(), int(Lib.aleo_mi355x_found_owned(h)),
                    np.frombuffer(ctypes.string_at(Lib.aleo_mi355x_found_commitments(h), 32 * c), dtype=np.uint8).reshape(-1, 32).copy() if commitments else None))
        Lib.aleo_mi355x_found_free(h)
    return got


def roads(L, B, batch, accounts, sks, S):
    n = len(batch); K = len(accounts); tp = ctypes.cast(ctypes.c_char_p(batch.text), ctypes.c_void_p)
    vks = np.frombuffer(b''.join(a[0].to_bytes(32, 'little') for a in accounts), dtype=np.uint8); axs = np.frombuffer(b''.join(a[1].to_bytes(32, 'little') for a in accounts), dtype=np.uint8)
    tail = lambda: (p(S) if len(S) else None, len(S))
    state = {}

    def new():
        out = (ctypes.c_void_p * K)()
        if K == 1: rc = L.aleo_mi355x_records_unspent_named(out, tp, p(batch.offsets), n, PROGRAM, RECORD, p(sks), p(vks), p(axs), *tail())
        else: rc = L.aleo_mi355x_records_unspent_named_many(out, tp, p(batch.offsets), n, PROGRAM, RECORD, p(sks), p(vks), p(axs), K, *tail())
        aleo_amd._lib.check(rc, 'records_unspent_named')
        state['new'] = results(L, out, K, True)

    def parent():
        out = (ctypes.c_void_p * K)()
        if K == 1: assert B.aleo_mi355x_records_decrypt_strings(out, tp, p(batch.offsets), n, p(vks), p(axs)) == 0
        else: assert B.aleo_mi355x_records_decrypt_strings_many(out, tp, p(batch.offsets), n, p(vks), p(axs), K) == 0
        cm = np.zeros((n, 32), dtype=np.uint8); row = np.zeros(32, dtype=np.uint8)
        for j in range(K):
            h = ctypes.c_void_p(out[j]); c = int(B.aleo_mi355x_found_count(h)); nf = int(B.aleo_mi355x_found_fields(h))
            index = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_index(h), 4 * c), dtype=np.uint32); status = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_status(h), c), dtype=np.uint8)
            off = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_offsets(h), 4 * (c + 1)), dtype=np.uint32); plain = np.frombuffer(ctypes.string_at(B.aleo_mi355x_found_plain(h), 32 * nf), dtype=np.uint8).reshape(-1, 32)
            for k in range(c):
                if status[k]: continue
                i = int(index[k]); f = np.ascontiguousarray(plain[off[k]:off[k + 1]])
                if B.aleo_mi355x_record_commitment(p(row), batch.text[int(batch.offsets[i]):int(batch.offsets[i + 1])], p(f), len(f), PROGRAM, RECORD) == 0: cm[i] = row
            B.aleo_mi355x_found_free(h)
        out = (ctypes.c_void_p * K)()
        if K == 1: assert B.aleo_mi355x_records_unspent_strings(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), *tail()) == 0
        else: assert B.aleo_mi355x_records_unspent_strings_many(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), K, *tail()) == 0
        state['parent'] = results(B, out, K); state['cm'] = cm

    def floor():
        out = (ctypes.c_void_p * K)(); cm = state['cm']
        if K == 1: rc = L.aleo_mi355x_records_unspent_strings(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), *tail())
        else: rc = L.aleo_mi355x_records_unspent_strings_many(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), K, *tail())
        aleo_amd._lib.check(rc, 'records_unspent_strings')
        state['floor'] = results(L, out, K)

    return new, parent, floor, state


def shape(L, n, K, fraction, pool, accounts, lg_spent=16):
    batch, per = make_many(n, fraction, pool, accounts)
    rng = random.Random(n + K)
    sks = np.frombuffer(b''.join(rng.randrange(L_ORDER).to_bytes(32, 'little') for _ in range(K)), dtype=np.uint8)
    # setup: the serial numbers of every account's records, from a small batch that holds them all once
    small = records.RecordBatch.from_strings([s for a in accounts for s in a[2]])
    new, _, _, state = roads(L, L, small, accounts, sks, np.zeros((0, 32), dtype=np.uint8))
    new()
    half = np.concatenate([sn[::2] for _, sn, _, _ in state['new']])
    S = np.concatenate([half, seeded_rows(max(1 << lg_spent, len(half)) - len(half), 3)]); np.random.default_rng(5).shuffle(S)
    return batch, per, sks, np.ascontiguousarray(S)


def same_kept(state, K, a, b):
    return all(state[a][j][0].tobytes() == state[b][j][0].tobytes() and state[a][j][1].tobytes() == state[b][j][1].tobytes() and state[a][j][2] == state[b][j][2] for j in range(K))


def threshold(L, a, emit):
    """The stand-alone call over 2^k owned records of one account: the kernel against the host path on one thread, two timings of each."""
    acct = accounts_of(1)
    for lg in [int(v) for v in a.threshold.split(',')]:
        count = 1 << lg
        batch = records.RecordBatch.from_strings([acct[0][2][k % VARIANTS] for k in range(count)])
        found = records.decrypt_strings(batch, acct[0][0].to_bytes(32, 'little'), acct[0][1].to_bytes(32, 'little'), keep=True)
        assert len(found) == count
        def call(host):
            def f(): state[host] = records.found_commitments(batch, found, PROGRAM.decode(), RECORD.decode(), host=host)
            return f
        state = {}
        os.environ['ALEO_MI355X_MIN_COMMITMENTS'] = '0'
        pairs = [timed({'device': call(False), 'host': call(True)}, a.reps) for _ in range(2)]
        os.environ.pop('ALEO_MI355X_MIN_COMMITMENTS')
        assert state[False][0].tobytes() == state[True][0].tobytes() and not state[False][1].any()
        emit('2^%-2d owned records   ' % lg + '   '.join('kernel %s  host, one thread %s  %5.2fx' % (ms(r['device']), ms(r['host']), r['host'][0] / r['device'][0]) for r in pairs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline-lib'); ap.add_argument('--keys', type=int, default=1); ap.add_argument('--sizes', default='20'); ap.add_argument('--fractions', default='0.01')
    ap.add_argument('--reps', type=int, default=8); ap.add_argument('--threshold'); ap.add_argument('--out'); ap.add_argument('--trace-case', action='store_true')
    a = ap.parse_args()
    L = aleo_amd.lib(); aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')      # no GPU, no numbers
    B = bind(a.baseline_lib) if a.baseline_lib else L
    shown = [arg for k, arg in enumerate(sys.argv[1:], 1) if arg != '--out' and sys.argv[k - 1] != '--out']      # what was measured, not where it was written
    lines = ['# records_commit_bench %s' % ' '.join(arg if not arg.endswith('.so') else '(the parent commit\'s build)' for arg in shown),
             '# new: %s' % L.aleo_mi355x_version().decode(), '# parent road through: %s' % B.aleo_mi355x_version().decode(),
             '# ms per call: median (min..max) of %d rounds, the roads in a new seeded order every round; %% owned: per account; half of the owned spent, 2^16 spent rows' % a.reps, '']
    def emit(row): lines.append(row); print(row, flush=True)
    if a.threshold: threshold(L, a, emit)
    else:
        pool = foreign_pool(); K = a.keys; accounts = accounts_of(K)
        if a.trace_case:
            batch, per, sks, S = shape(L, 1 << 20, K, 0.01, pool, accounts)
            new, _, _, state = roads(L, L, batch, accounts, sks, S)
            for _ in range(4): new()
            print('trace case: 2^20 strings, %d accounts, %d owned and %d kept each, 2^16 spent rows' % (K, state['new'][0][2], len(state['new'][0][0])))
            return
        for lg in [int(v) for v in a.sizes.split(',')]:
            for fr in [float(v) for v in a.fractions.split(',')]:
                batch, per, sks, S = shape(L, 1 << lg, K, fr, pool, accounts)
                new, parent, floor, state = roads(L, B, batch, accounts, sks, S)
                parent()                                        # the floor's commitments
                r = timed({'new': new, 'parent': parent, 'floor': floor}, a.reps)
                assert same_kept(state, K, 'new', 'parent') and same_kept(state, K, 'new', 'floor'), 'the roads keep different records'
                assert all(g[2] == per and 0 < len(g[0]) < per or per < 2 for g in state['new']) and all(g[3].tobytes() == state['cm'][g[0].astype(np.int64)].tobytes() for g in state['new'])
                spread = r['parent'][2] - r['parent'][1]
                verdict = 'slower by more than the parent road\'s spread' if r['new'][0] > r['parent'][0] + spread else ''
                emit('2^%-2d x %d keys %5.1f %% owned (%7d each)   new %s   parent %s   %6.2fx   floor %s   the stage costs %7.3f ms  %s' %
                     (lg, K, 100 * fr, per, ms(r['new']), ms(r['parent']), r['parent'][0] / r['new'][0], ms(r['floor']), (r['new'][0] - r['floor'][0]) * 1e3, verdict))
    if a.out:
        with open(a.out, 'a') as f: f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
