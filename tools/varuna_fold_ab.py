#!/usr/bin/env python3
"""The prover's calls through this build and through another build of the library (the parent commit's), in one process
(profiles/varuna_fold.txt is this tool's output).

    python tools/varuna_fold_ab.py PARENT_LIB OUT [lg]

Per call shape — aleo_mi355x_varuna_prove_indexed with 1 and with 4 instances, aleo_mi355x_varuna_prove_many with 8 requests, one
aleo_mi355x_varuna_index_build, all at 2^lg constraints (15) — one warm call through each library, whose bytes are compared; then 7 rounds, the
libraries in a new seeded order every round, each timing a window of enough calls for about 0.25 s (64 at the most); ms per call, median (min..max) of
the rounds.  The parent's min..max is its spread in that session.  FOLD_PARENT_AGAIN=PATH times a second copy of the parent's library (a copy of the
file under another name) beside them: what two loads of the same code differ by.  Inputs: bench.py's _varuna_instance.  Host wall clock, no profiler.
Needs a gfx950 device: there is no fallback."""
import os, random, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aleo_amd                                         # noqa: E402
from aleo_amd import _lib, synth, varuna                # noqa: E402
import bench                                            # noqa: E402

ROUNDS = 7


def load(path):
    """another build of the library behind the package's own bindings"""
    _lib.LIB_PATH, _lib._LIB = path, None
    return _lib.lib()


def ab(label, calls, libs, out):
    """calls[name]() makes one call through library `name` and returns the bytes to compare (only looked at outside the timed windows)"""
    def run(name): _lib._LIB = libs[name]; return calls[name]()
    got = {name: run(name) for name in calls}                              # warm-up of this shape in all, and the parity of what is timed
    same = got['result'] == got['parent']
    t0 = time.perf_counter(); run('parent'); one = time.perf_counter() - t0
    inner = max(1, min(64, int(0.25 / max(one, 1e-4))))
    ts = {name: [] for name in calls}
    for r in range(ROUNDS):
        order = list(calls); random.Random(r).shuffle(order)
        for name in order:
            t0 = time.perf_counter()
            for _ in range(inner): run(name)
            ts[name].append((time.perf_counter() - t0) / inner)
    med = {k: statistics.median(v) for k, v in ts.items()}
    lo, hi = min(ts['parent']), max(ts['parent'])
    inside = lo <= med['result'] <= hi
    row = '%-44s result %8.3f (%.3f..%.3f)   parent %8.3f (%.3f..%.3f)   %+5.1f %%   %s   bytes %s   [%d calls per window]' % (
        label, med['result'] * 1e3, min(ts['result']) * 1e3, max(ts['result']) * 1e3, med['parent'] * 1e3, lo * 1e3, hi * 1e3, (med['result'] / med['parent'] - 1) * 100,
        'within the parent\'s min..max' if inside else ('below the parent\'s min' if med['result'] < lo else 'ABOVE THE PARENT\'S MAX'), 'equal' if same else 'DIFFER', inner)
    if 'parent again' in ts:
        v = ts['parent again']
        row += '   parent again %8.3f (%.3f..%.3f)  %+5.1f %% of the parent' % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, (statistics.median(v) / med['parent'] - 1) * 100)
    print(row, flush=True); out.write(row + '\n'); out.flush()
    return (inside or med['result'] < lo) and same


def main():
    parent, out_path = sys.argv[1], sys.argv[2]; lg = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    paths = {'result': _lib.LIB_PATH, 'parent': parent}
    if os.environ.get('FOLD_PARENT_AGAIN'): paths['parent again'] = os.environ['FOLD_PARENT_AGAIN']
    libs = {name: load(path) for name, path in paths.items()}
    n, csr, z, zz, ck0, D = bench._varuna_instance(synth, lg, 40 + lg); ck0.close()
    build = lambda ck: varuna.NativeCircuitIndex(csr, n, 4, len(z) - 4, ck)
    cks, nxs = {}, {}
    for name, B in libs.items():                                             # a committer key and an index per library: handles belong to the build that made them
        _lib._LIB = B; cks[name] = varuna.synthetic_committer_key(bench.VARUNA_TAU, bench.VARUNA_S, D); nxs[name] = build(cks[name])
    def rebuild(name):
        with build(cks[name]) as nx: return nx.vk_bytes
    ok = True
    with open(out_path, 'w') as out:
        head = 'varuna_fold_ab: 2^%d constraints (%d), ms per call: median (min..max) of %d rounds' % (lg, n, ROUNDS)
        print(head); out.write(head + '\n')
        ok &= ab('prove_indexed, 1 instance', {k: (lambda k=k: nxs[k].prove(zz, 7)) for k in libs}, libs, out)
        ok &= ab('prove_indexed, 4 instances', {k: (lambda k=k: nxs[k].prove([zz] * 4, 8)) for k in libs}, libs, out)
        ok &= ab('prove_many, 8 requests', {k: (lambda k=k: b''.join(varuna.prove_many_native([([nxs[k]], [[zz]], 100 + i) for i in range(8)]))) for k in libs}, libs, out)
        ok &= ab('index_build', {k: (lambda k=k: rebuild(k)) for k in libs}, libs, out)
        tail = 'every median inside the parent\'s min..max (or below it), bytes equal' if ok else 'A ROW MISSED: see above'
        print(tail); out.write(tail + '\n')
    for name, B in libs.items(): _lib._LIB = B; nxs[name].close(); cks[name].close()
    _lib._LIB = libs['result']
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
