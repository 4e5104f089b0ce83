"""The slice stage of the MSM sort on its own (aleo_mi355x_selftest_slice_order): bucket scan, top scan, slice ordering on histograms from the host,
checked on the host against a recount.  `order` mis-sorted, or a bucket missing from a multi-slice list's expected place, leaves every MSM result right
and only costs time, so the result tests cannot see it: the hook counts violations of
  order is a permutation of the slice ids | slice lengths never increase along it | task_g[sid] is the bucket that owns sid |
  len_count, meta[0..6] (device and host copy) and both multi-slice lists (as sets) equal the host's recount."""
import ctypes
import numpy as np
import pytest
import aleo_amd


def _ones(): return np.ones(4096, dtype=np.uint32)
def _random():
    x = np.arange(4096, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)
    x ^= x >> np.uint64(29); x *= np.uint64(0xBF58476D1CE4E5B9); x ^= x >> np.uint64(32)
    return (x % np.uint64(41)).astype(np.uint32)
def _one_bucket():
    h = np.zeros(4096, dtype=np.uint32); h[0] = 40000; return h
def _boundary(v):
    h = np.zeros(4096, dtype=np.uint32); h[2047] = h[2048] = v; return h
def _alternating():
    h = np.zeros(8192, dtype=np.uint32); h[1::2] = 65; return h
def _sparse():      # first and last of 32768 buckets: a block's stretch of buckets is longer than it walks (STRETCH_CAP = 8192), so the lanes search it
    h = np.zeros(32768, dtype=np.uint32); h[0] = 3000; h[-1] = 3000; h[20000] = 1; return h
def _many_super():      # 5000 > SUPER_CAP (4096) buckets of 26 slices each (5000 points cut at 197), some ordinary multi-slice buckets behind them; the hook checks that exactly 5000 - SUPER_CAP of them went over to the common list
    h = np.zeros(8192, dtype=np.uint32); h[:5000] = 5000; h[5000:6000] = 700; h[6000:7000] = 3; return h


CASES = {
    'ones': _ones, 'random_0_40': _random, 'one_bucket_40000': _one_bucket, 'tile_boundary_1': lambda: _boundary(1), 'tile_boundary_100': lambda: _boundary(100),
    'alternating_0_65': _alternating, 'partial_tile_254': lambda: (np.arange(254, dtype=np.uint32) * 7) % 23, 'all_zero': lambda: np.zeros(4096, dtype=np.uint32),
    'more_than_super_cap': _many_super, 'sparse_32768': _sparse,
}


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1], ids=['top_scan_launch', 'top_scan_fused'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_slice_order_invariants(case, fused):
    h = np.ascontiguousarray(CASES[case](), dtype=np.uint32)
    bad = ctypes.c_uint32(0xffffffff)
    aleo_amd._lib.check(aleo_amd.lib().aleo_mi355x_selftest_slice_order(h.ctypes.data_as(ctypes.c_void_p), h.size, int(h.sum()), fused, ctypes.byref(bad)), 'selftest_slice_order')
    assert bad.value == 0, f'{bad.value} violations'
