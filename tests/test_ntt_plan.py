"""The transform's pass plan and choice of kernel configuration (aleo_amd/csrc/ntt_plan.h) are plain C++: tests/cpp/ntt_plan_test.cpp checks them against
the formulas of the drivers they replaced, as a program of its own built with the address and undefined-behaviour sanitizers."""
import os, subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'aleo_amd', 'csrc')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']      # host code only: a program of its own, never a GPU build


def test_ntt_plan_matches_the_old_drivers_and_covers_every_size(tmp_path):
    exe = os.path.join(str(tmp_path), 'ntt_plan_test')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall'] + SANITIZE + ['-I', CSRC, os.path.join(HERE, 'cpp', 'ntt_plan_test.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and '90 plans, 11 form edges, 0 failures' in r.stdout, r.stdout + r.stderr
