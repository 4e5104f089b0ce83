#!/usr/bin/env python3
"""The measurements of the record search from strings (profiles/records_strings.txt is this tool's output; DESIGN §11 reads it).

    python tools/records_strings_bench.py [--parent-lib PATH] [--sizes 12,16,20] [--reps 7] [--python-n 65536] [--out FILE]
    python tools/records_strings_bench.py --trace-command          # prints the command a kernel trace is taken of (run it under rocprofv3, in a run of its own)

C level (tools/records_strings_bench.cpp, built here with g++): a loop of aleo_mi355x_record_parse, _records_parse_many_host, _records_parse_many on the GPU,
aleo_mi355x_records_scan on rows already parsed, and _records_scan_strings with K = 1 against "loop of record_parse + records_scan" by the library of the parent
commit (--parent-lib: a build of the commit before this feature; without it that row is left out), alternating in one process.
Python level: records.find_owned on --python-n strings, the road a list of strings took before (every string through RecordCiphertext.from_string, then the scan
of the private owners: the parent's find_owned, which this library still runs for RecordCiphertext objects) against the road it takes now.
Every timing: host buffers, upload and download inside the timed call, one warm call, the median of --reps, no profiler.  Needs a gfx950 device: there is no
fallback, and a figure from a CPU would say nothing."""
import argparse, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, 'tools', 'records_strings_bench.cpp')
EXE = os.path.join(ROOT, 'tools', 'records_strings_bench')


def build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        subprocess.check_call(['g++', '-std=c++17', '-O2', SRC, '-o', EXE, '-ldl'])
    return EXE


def python_level(n, reps):
    import random
    import aleo_amd
    from aleo_amd import records, wire
    aleo_amd._lib.check(aleo_amd.lib().aleo_mi355x_init_device(-1), 'init')
    os.environ['ALEO_MI355X_MIN_RECORDS'] = '0'
    rng = random.Random(1)
    head = b'\x01\x01\x00'; entry = b'\x01\x0cmicrocredits\x23\x00'
    field = lambda: rng.getrandbits(252).to_bytes(32, 'little')
    strings = [wire.bech32m_encode('record', head + field() + entry + rng.getrandbits(280).to_bytes(35, 'little') + field()) for _ in range(n)]
    vk, ax = 0x0b0a09080706050403020157, (5).to_bytes(32, 'little')
    before = lambda: records.find_owned([records.RecordCiphertext.from_string(s) for s in strings], vk, ax)
    now = lambda: records.find_owned(strings, vk, ax)
    assert before() == now()                                       # warm, and the same answer
    t_before, t_now = [], []
    for _ in range(reps):                                          # alternating
        t0 = time.perf_counter(); before(); t_before.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); now(); t_now.append(time.perf_counter() - t0)
    b, a = statistics.median(t_before), statistics.median(t_now)
    return ['find_owned on %d strings (Python): every string through RecordCiphertext.from_string, then the scan   %10.1f ms' % (n, b * 1e3),
            'find_owned on %d strings (Python): one RecordBatch through records_scan_strings                        %10.1f ms   (%.1fx)' % (n, a * 1e3, b / a)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-lib'); ap.add_argument('--sizes', default='12,16,20'); ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--python-n', type=int, default=1 << 16); ap.add_argument('--out'); ap.add_argument('--trace-command', action='store_true')
    a = ap.parse_args()
    import aleo_amd
    lib = aleo_amd._lib.LIB_PATH
    exe = build()
    if a.trace_command:
        print(' '.join([exe, lib, '--sizes', a.sizes.split(',')[-1], '--scan-only', '3']))
        return
    cmd = [exe, lib] + ([a.parent_lib] if a.parent_lib else []) + ['--sizes', a.sizes, '--reps', str(a.reps)]
    lines = ['# ' + ' '.join(os.path.relpath(c, ROOT) if os.path.isabs(c) else c for c in cmd), '# ' + aleo_amd.lib().aleo_mi355x_version().decode()]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines += r.stdout.rstrip().split('\n')
    if r.returncode: sys.stderr.write(r.stderr); sys.exit('the C-level run failed')
    if a.python_n: lines += [''] + python_level(a.python_n, a.reps)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f: f.write(text)


if __name__ == '__main__':
    main()
