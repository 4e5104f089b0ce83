#!/usr/bin/env python3
"""The same record-search calls through this build and through another build of the library (the parent commit's), in one process
(profiles/records_fold.txt is this tool's output).

    python tools/records_fold_ab.py PARENT_LIB OUT [scan] [serial] [found] [unspent]

Per shape: one warm call through each library, whose bytes are compared; then 7 rounds, the libraries in a new seeded order every round, each timing a
window of enough calls for about 0.25 s (64 at the most); ms per call, median (min..max) of the rounds.  The parent's min..max is its spread in that
session.  FOLD_PARENT_AGAIN=PATH times a second copy of the parent's library beside them: what two loads of the same code differ by.  FOLD_DRY=1 is a
rehearsal without a device (tiny shapes on the host paths).  Inputs: those of records_scan_bench.py, records_found_bench.py and records_unspent_bench.py.
Host buffers, copies inside the timed calls, no profiler.  Needs a gfx950 device: there is no fallback."""
import ctypes, os, random, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
DRY = os.environ.get('FOLD_DRY') == '1'                  # a rehearsal without a device: tiny shapes on the host paths
THRESH = '1000000' if DRY else None
import aleo_amd                                         # noqa: E402
import records_scan_bench as SB                         # noqa: E402
import records_found_bench as FB                        # noqa: E402
import records_unspent_bench as UB                      # noqa: E402
from records_found_bench import p                       # noqa: E402

os.environ['ALEO_MI355X_MIN_RECORDS'] = THRESH or '0'; os.environ['ALEO_MI355X_MIN_DECRYPT'] = THRESH or '0'; os.environ['ALEO_MI355X_MIN_SERIALS'] = THRESH or '1'
ROUNDS = 2 if DRY else 7
vp, sz = ctypes.c_void_p, ctypes.c_size_t


def bind(B):
    B.aleo_mi355x_records_scan.argtypes = [vp] * 4 + [sz] + [vp] * 2
    B.aleo_mi355x_records_scan_many.argtypes = [vp] * 4 + [sz] + [vp] * 2 + [sz]
    B.aleo_mi355x_records_serial_numbers.argtypes = [vp, vp, vp, sz, vp]
    B.aleo_mi355x_records_decrypt_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp]
    B.aleo_mi355x_records_decrypt_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, sz]
    B.aleo_mi355x_records_unspent_strings.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, vp, vp, vp, sz]
    B.aleo_mi355x_records_unspent_strings_many.argtypes = [ctypes.POINTER(vp), vp, vp, sz, vp, vp, vp, vp, sz, vp, sz]
    for name in ('count', 'fields', 'owned'): f = getattr(B, 'aleo_mi355x_found_' + name); f.argtypes = [vp]; f.restype = sz
    for name in ('index', 'status', 'microcredits', 'serials', 'plain', 'rvk', 'offsets', 'kind'): f = getattr(B, 'aleo_mi355x_found_' + name); f.argtypes = [vp]; f.restype = vp
    B.aleo_mi355x_found_free.argtypes = [vp]; B.aleo_mi355x_found_free.restype = None
    B.aleo_mi355x_version.restype = ctypes.c_char_p; B.aleo_mi355x_init_device.argtypes = [ctypes.c_int32]
    assert DRY or B.aleo_mi355x_init_device(-1) == 0
    return B


def found_bytes(B, h, serials):
    c, f = int(B.aleo_mi355x_found_count(h)), int(B.aleo_mi355x_found_fields(h))
    parts = [ctypes.string_at(B.aleo_mi355x_found_index(h), 4 * c), ctypes.string_at(B.aleo_mi355x_found_kind(h), c), ctypes.string_at(B.aleo_mi355x_found_rvk(h), 32 * c),
             ctypes.string_at(B.aleo_mi355x_found_offsets(h), 4 * (c + 1)), ctypes.string_at(B.aleo_mi355x_found_plain(h), 32 * f), ctypes.string_at(B.aleo_mi355x_found_status(h), c),
             ctypes.string_at(B.aleo_mi355x_found_microcredits(h), 8 * c), b'%d' % int(B.aleo_mi355x_found_owned(h))]
    if serials: parts.append(ctypes.string_at(B.aleo_mi355x_found_serials(h), 32 * c))
    return b'|'.join(parts)


def ab(label, make_call, libs, out):
    """make_call(lib) -> f() that makes one call and returns the bytes to compare (only looked at outside the timed windows)"""
    calls = {name: make_call(B) for name, B in libs.items()}
    got = {name: f(True) for name, f in calls.items()}                     # warm-up of this shape in both, and the parity of what is timed
    same = got['result'] == got['parent']
    t0 = time.perf_counter(); calls['parent'](False); one = time.perf_counter() - t0
    inner = max(1, min(64, int(0.25 / max(one, 1e-4))))
    ts = {name: [] for name in calls}
    for r in range(ROUNDS):
        order = list(calls.items()); random.Random(r).shuffle(order)
        for name, f in order:
            t0 = time.perf_counter()
            for _ in range(inner): f(False)
            ts[name].append((time.perf_counter() - t0) / inner)
    med = {k: statistics.median(v) for k, v in ts.items()}
    lo, hi = min(ts['parent']), max(ts['parent'])
    ok = lo <= med['result'] <= hi or med['result'] <= med['parent'] + (hi - lo)
    row = '%-58s result %9.3f (%.3f..%.3f)   parent %9.3f (%.3f..%.3f)   %+5.1f %%   %s   bytes %s   [%d calls per window]' % (
        label, med['result'] * 1e3, min(ts['result']) * 1e3, max(ts['result']) * 1e3, med['parent'] * 1e3, lo * 1e3, hi * 1e3, (med['result'] / med['parent'] - 1) * 100,
        'within the parent\'s min..max' if lo <= med['result'] <= hi else ('below the parent\'s min' if med['result'] < lo else ('above, within its spread' if ok else 'ABOVE THE PARENT\'S SPREAD')),
        'equal' if same else 'DIFFER', inner)
    if 'parent again' in ts:                                               # a second copy of the parent's library: what two loads of the same code differ by
        v = ts['parent again']; row += '   parent again %9.3f (%.3f..%.3f)  %+5.1f %% of the parent' % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, (statistics.median(v) / med['parent'] - 1) * 100)
    print(row, flush=True); out.write(row + '\n'); out.flush()
    return ok and same


def part_scan(libs, out):
    c0, nx, vk, ax = SB.make_records(1 << (8 if DRY else 21))
    vkb = np.frombuffer(int(vk).to_bytes(32, 'little'), dtype=np.uint8).copy(); axb = np.frombuffer(int(ax).to_bytes(32, 'little'), dtype=np.uint8).copy()
    c0[::97] = 0xff                                                          # malformed owner fields among them: flag 2, zero rows
    for lg in (6,) if DRY else (8, 12, 16, 20, 21):
        n = 1 << lg; C0, NX = c0[:n], nx[:n]
        def make(B, n=n, C0=C0, NX=NX):
            flags = np.zeros(n, dtype=np.uint8); rvk = np.zeros((n, 32), dtype=np.uint8)
            def f(want):
                assert B.aleo_mi355x_records_scan(p(flags), p(rvk), p(C0), p(NX), n, p(vkb), p(axb)) == 0
                return flags.tobytes() + rvk.tobytes() if want else None
            return f
        ab('records_scan  n = 2^%d, one account%s' % (lg, ' (two chunks)' if lg == 21 else ''), make, libs, out)
    vks, axs = SB.many_keys(8); lg8 = 6 if DRY else 20; n = 1 << lg8
    def make8(B):
        flags = np.zeros((8, n), dtype=np.uint8); rvk = np.zeros((8, n, 32), dtype=np.uint8)
        def f(want):
            assert B.aleo_mi355x_records_scan_many(p(flags), p(rvk), p(c0[:n]), p(nx[:n]), n, p(vks), p(axs), 8) == 0
            return flags.tobytes() + rvk.tobytes() if want else None
        return f
    ab('records_scan_many  n = 2^%d, K = 8' % lg8, make8, libs, out)


def part_serial(libs, out):
    sk = np.frombuffer(random.Random(9).randrange(FB.L_ORDER).to_bytes(32, 'little'), dtype=np.uint8).copy()
    cm_all = UB.seeded_rows(1 << 20, 77); cm_all[5] = 0xff
    for lg in (5,) if DRY else (7, 10, 14, 17, 20):
        n = 1 << lg; cm = np.ascontiguousarray(cm_all[:n])
        def make(B, n=n, cm=cm):
            sn = np.zeros((n, 32), dtype=np.uint8); fl = np.zeros(n, dtype=np.uint8)
            def f(want):
                assert B.aleo_mi355x_records_serial_numbers(p(sn), p(fl), p(cm), n, p(sk)) == 0
                return sn.tobytes() + fl.tobytes() if want else None
            return f
        ab('records_serial_numbers  n = 2^%d' % lg, make, libs, out)


def found_call(B, batch, accounts, unspent=None):
    n = len(batch); K = len(accounts); tp = ctypes.cast(ctypes.c_char_p(batch.text), vp)
    vks = np.frombuffer(b''.join(a[0].to_bytes(32, 'little') for a in accounts), dtype=np.uint8); axs = np.frombuffer(b''.join(a[1].to_bytes(32, 'little') for a in accounts), dtype=np.uint8)
    def f(want):
        out = (vp * K)()
        if unspent is None:
            rc = B.aleo_mi355x_records_decrypt_strings(out, tp, p(batch.offsets), n, p(vks), p(axs)) if K == 1 else B.aleo_mi355x_records_decrypt_strings_many(out, tp, p(batch.offsets), n, p(vks), p(axs), K)
        else:
            cm, sks, S = unspent
            rc = (B.aleo_mi355x_records_unspent_strings(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), p(S), len(S)) if K == 1
                  else B.aleo_mi355x_records_unspent_strings_many(out, tp, p(batch.offsets), n, p(cm), p(sks), p(vks), p(axs), K, p(S), len(S)))
        assert rc == 0
        got = b'#'.join(found_bytes(B, vp(out[j]), unspent is not None) for j in range(K)) if want else None
        for j in range(K): B.aleo_mi355x_found_free(vp(out[j]))
        return got
    return f


def part_found(libs, out, unspent):
    pool = FB.foreign_pool(); L = libs['result']
    for K, lg, fr in ((1, 7, 0.1), (8, 7, 0.05)) if DRY else ((1, 16, 0.01), (1, 20, 0.01), (1, 20, 1.0), (8, 20, 0.01)) if not unspent else ((1, 16, 0.01), (1, 20, 0.01), (8, 20, 0.01)):
        accounts = FB.accounts_of(K)
        if unspent:
            batch, per, cm, sks, S = UB.shape(L, L, 1 << lg, K, fr, 16, pool, accounts)
            ab('unspent_strings%s  n = 2^%d, K = %d, %g %% owned each, half spent, 2^16 spent rows' % ('_many' if K > 1 else '', lg, K, 100 * fr),
               lambda B: found_call(B, batch, accounts, (cm, sks, S)), libs, out)
        else:
            batch, per = FB.make_many(1 << lg, fr, pool, accounts)
            ab('decrypt_strings%s  n = 2^%d, K = %d, %g %% owned each' % ('_many' if K > 1 else '', lg, K, 100 * fr), lambda B: found_call(B, batch, accounts), libs, out)


def main():
    parent, out_path, parts = sys.argv[1], sys.argv[2], sys.argv[3:] or ['scan', 'serial', 'found', 'unspent']
    L = bind(aleo_amd.lib()); P = bind(ctypes.CDLL(os.path.abspath(parent)))
    libs = {'result': L, 'parent': P}
    if os.environ.get('FOLD_PARENT_AGAIN'): libs['parent again'] = bind(ctypes.CDLL(os.path.abspath(os.environ['FOLD_PARENT_AGAIN'])))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as out:
        head = '# result: %s\n# parent: %s\n# ms per call: median (min..max) of %d rounds\n' % (L.aleo_mi355x_version().decode(), P.aleo_mi355x_version().decode(), ROUNDS)
        print(head, flush=True); out.write(head)
        for part in parts:
            if part == 'scan': part_scan(libs, out)
            elif part == 'serial': part_serial(libs, out)
            elif part == 'found': part_found(libs, out, False)
            elif part == 'unspent': part_found(libs, out, True)


if __name__ == '__main__':
    main()
