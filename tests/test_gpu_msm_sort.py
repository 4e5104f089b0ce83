"""The scalar sort every G1 and G2 multi-scalar multiplication shares (csrc/msm_sort.hip), run alone through aleo_mi355x_selftest_sort_pairs and compared with
the integer reference tests/msm_sort_ref.py: hist[] equal, the pair count equal to its sum, every bucket's run of the index stream equal as a multiset, nothing
written behind the last pair.  The MSM result tests see the sort only through sums, and only at the window widths, tiles and segment shapes their sizes reach:
here all 19 width instances, the three level-1 tile sizes, the workgroup dealing, the equal-key and many-part paths of level 2, offset infinity flags and full
set capacity run on a few thousand scalars whose windows sit on the edges of the digit recoding."""
import ctypes
import numpy as np
import pytest

import aleo_amd
from aleo_amd import synth
import msm_sort_ref as ref

pytestmark = pytest.mark.gpu
BAD_ARG = 2
SENTINEL = 0x7FFFFFFF       # no index takes it: windows * row_stride stays far below 2^31 here


@pytest.fixture(scope='module', autouse=True)
def device():
    aleo_amd._lib.check(aleo_amd.lib().aleo_mi355x_init_device(-1), 'init')     # no GPU -> hard failure, never a fallback


def sort_pairs(segs, c, pre, k_sets=1, row_stride=0, inf=None, mont=False, tile=0):
    """(status, hist, stream, pairs) of one call of the hook; the stream comes back whole, sentinel and all."""
    W = -(-254 // c)                                             # (not ref.geometry: a refused width may have none)
    scalars = np.ascontiguousarray(np.concatenate([q.scalars for q in segs]))
    seg_n = np.array([q.n for q in segs], dtype=np.uint32); seg_off = np.array([q.off for q in segs], dtype=np.uint32); seg_set = np.array([q.set for q in segs], dtype=np.uint8)
    M = (k_sets if pre else W) << (c - 1)
    hist = np.full(M, 0xA5A5A5A5, dtype=np.uint32)
    cap = min(scalars.shape[0], 1 << 20) * W + 64
    stream = np.full(cap, SENTINEL, dtype=np.uint32)
    got = ctypes.c_uint32(0xFFFFFFFF)
    if inf is not None: inf = np.ascontiguousarray(inf, dtype=np.uint8); assert inf.size == row_stride
    p = aleo_amd._lib._p
    st = aleo_amd.lib().aleo_mi355x_selftest_sort_pairs(p(scalars), p(seg_n), p(seg_off), p(seg_set), len(segs), c, int(pre), int(mont), k_sets, row_stride, p(inf), tile,
                                                        p(hist), p(stream), cap, ctypes.byref(got))
    return st, hist, stream, got.value


def check(segs, c, pre, k_sets=1, row_stride=None, inf=None, mont=False, tile=0):
    if row_stride is None: row_stride = max(q.off + q.n for q in segs) + 11
    want_hist, want_stream = ref.expected(segs, c, pre, k_sets, row_stride, inf, mont)
    st, hist, stream, npairs = sort_pairs(segs, c, pre, k_sets, row_stride, inf, mont, tile)
    aleo_amd._lib.check(st, 'selftest_sort_pairs')
    total = int(want_hist.sum())
    assert (hist == want_hist).all(), f'hist differs in {int((hist != want_hist).sum())} of {hist.size} buckets (device sum {int(hist.sum(dtype=np.uint64))}, expected {total})'
    assert npairs == total
    assert (stream[total:] == SENTINEL).all(), 'the sort wrote behind its last pair'
    assert (ref.canonical(hist, stream[:total]) == want_stream).all(), 'a bucket run holds other indices than the reference'
    return total


def const(n, v):
    s = np.zeros((n, 4), dtype=np.uint64); s[:] = synth.int_to_limbs(v, 4); return s


INSTANCES = [(False, c) for c in ref.PLAIN_WIDTHS] + [(True, c) for c in ref.TABLE_WIDTHS]
def _id(pc): return ('table' if pc[0] else 'plain') + '_c%d' % pc[1]


@pytest.mark.parametrize('pre,c', INSTANCES, ids=[_id(x) for x in INSTANCES])
def test_every_width_instance(pre, c):
    """One segment of two tiles and 37 scalars (the last block is partial), edge and carry-chain scalars of this width in front."""
    n = 2 * 2048 + 37
    assert check([ref.Seg(ref.mix(c, n, 0x5027A000 + 64 * pre + c))], c, pre, row_stride=n + 11) > n


SKEW_PATHS = [(True, 13), (False, 8)]
SKEW = {
    'equal_9000': lambda c: const(9000, int(ref.to_ints(synth.uniform_scalars(1, 0x5027B000 + c))[0])),     # one bucket per window: lds_rank's equal-key path, coarse bins of > BIN_PART items
    'all_one': lambda c: const(9000, 1),
    'only_2048_2049': lambda c: np.concatenate([const(1, 2048), const(1, 2049)] * 2500 + [const(1, 2049)] * 7),      # two coarse bins at c = 13
    'all_zero': lambda c: const(5000, 0),
}


@pytest.mark.parametrize('pre,c', SKEW_PATHS, ids=[_id(x) for x in SKEW_PATHS])
@pytest.mark.parametrize('kind', sorted(SKEW))
def test_skewed_scalars(kind, pre, c):
    total = check([ref.Seg(SKEW[kind](c))], c, pre)
    assert (total == 0) == (kind == 'all_zero')


@pytest.mark.parametrize('pre,c', SKEW_PATHS, ids=[_id(x) for x in SKEW_PATHS])
def test_all_flagged_infinite(pre, c):
    n = 2048 + 300
    assert check([ref.Seg(ref.mix(c, n, 0x5027C000 + c), off=3)], c, pre, row_stride=n + 20, inf=np.ones(n + 20, dtype=np.uint8)) == 0


GRID_PATHS = [(True, 13), (False, 11)]      # (11 = the plain width of 2^15 points)
@pytest.mark.parametrize('pre,c', GRID_PATHS, ids=[_id(x) for x in GRID_PATHS])
@pytest.mark.parametrize('n', [16 * 2048, 17 * 2048 - 1], ids=['16_tiles', '17_tiles_less_1'])
def test_grid_widths(n, pre, c):
    """16 blocks: a grid width that is a multiple of 8, so the workgroups are dealt over the XCDs; 17 * 2048 - 1: they are not, and the last block is partial."""
    check([ref.Seg(ref.mix(c, n, 0x5027D000 + c + n))], c, pre)


@pytest.mark.parametrize('sets', [1, 2])
def test_two_unequal_segments_table(sets):
    """16 tiles and 3 tiles side by side: the grid is as wide as the longer one (the shorter one's blocks past its end leave early), dealt over the XCDs; feeding
    one set (the second segment's columns stand behind the first's) or two."""
    a, b = 16 * 2048, 3 * 2048
    segs = [ref.Seg(ref.mix(13, a, 0x5027E000), off=0, set=0), ref.Seg(ref.mix(13, b, 0x5027E100), off=a if sets == 1 else 5, set=sets - 1)]
    check(segs, 13, True, k_sets=sets)


def test_two_unequal_segments_plain():
    a, b = 16 * 2048, 3 * 2048
    check([ref.Seg(ref.mix(11, a, 0x5027E200), off=0), ref.Seg(ref.mix(11, b, 0x5027E300), off=a)], 11, False)


@pytest.mark.parametrize('pre,c', SKEW_PATHS, ids=[_id(x) for x in SKEW_PATHS])
def test_infinity_flags_at_the_segment_offset(pre, c):
    """Flags are read at off + i.  Flagged: the first and the last scalar of the segment and a few inside; the bytes at i itself (below off) and behind the segment
    are set as well and must not matter."""
    n, off = 2048 + 100, 777
    stride = off + n + 11
    inf = np.zeros(stride, dtype=np.uint8)
    inf[[off, off + 1, off + 255, off + 256, off + 2047, off + 2048, off + n - 1]] = 1
    inf[[0, 1, 2, 300, 776, off + n, stride - 1]] = 1
    s = ref.mix(c, n, 0x5027F000 + c)
    s[[0, 1, n - 1]] = synth.uniform_scalars(3, 0x5027F100)          # the flagged ends would emit pairs if they were read
    check([ref.Seg(s, off=off)], c, pre, row_stride=stride, inf=inf)


TILE_PATHS = [(True, 16), (False, 10)]
@pytest.mark.parametrize('pre,c', TILE_PATHS, ids=[_id(x) for x in TILE_PATHS])
@pytest.mark.parametrize('two', [False, True], ids=['one_segment', 'two_segments'])
@pytest.mark.parametrize('tile', [4096, 8192])
def test_level1_tiles(tile, two, pre, c):
    """The tiles of chains of >= 2^21 / 2^22 points, on two tiles and 5 scalars; and beside a shorter segment that ends inside its first tile."""
    n = 2 * tile + 5
    segs = [ref.Seg(ref.mix(c, n, 0x50280000 + tile + c))]
    if two: segs.append(ref.Seg(ref.mix(c, tile // 2 + 3, 0x50280100 + tile + c), off=n))
    check(segs, c, pre, tile=tile)


def test_montgomery_scalars():
    s = ref.mix(13, 2 * 2048 + 37, 0x50281000)
    check([ref.Seg(ref.to_mont(s))], 13, True, mont=True)


@pytest.mark.parametrize('c,k', [(13, 32), (20, 2)])
def test_set_capacity(c, k):
    """As many sets as a chain of the width holds, 300 scalars each; at 32 sets one in the middle is all zero."""
    segs = [ref.Seg(const(300, 0) if (k > 2 and q == 7) else ref.mix(c, 300, 0x50282000 + 16 * q + c), off=q, set=q) for q in range(k)]
    want_hist, _ = ref.expected(segs, c, True, k, 400)
    B = 1 << (c - 1)
    if k > 2: assert want_hist[7 * B:8 * B].sum() == 0 and want_hist[6 * B:7 * B].sum() > 0 and want_hist[8 * B:9 * B].sum() > 0
    check(segs, c, True, k_sets=k, row_stride=400)


def _refused(*a, **kw):
    st, hist, stream, npairs = sort_pairs(*a, **kw)
    assert st == BAD_ARG
    assert (hist == 0xA5A5A5A5).all() and (stream == SENTINEL).all() and npairs == 0xFFFFFFFF      # nothing came back


def test_refusals():
    s = ref.mix(13, 100, 0x50283000)
    _refused([ref.Seg(s)], 18, True, row_stride=111)                                         # no table instance of c = 18
    _refused([ref.Seg(s)], 17, False, row_stride=111)                                        # no plain instance above 16
    _refused([ref.Seg(s[:3], off=q, set=q) for q in range(33)], 13, True, k_sets=33, row_stride=111)      # 33 sets
    _refused([ref.Seg(s)], 20, True, k_sets=3, row_stride=111)                               # c = 20 holds two
    _refused([ref.Seg(s, set=1)], 8, False, row_stride=111)                                  # the plain path has one set
    _refused([ref.Seg(s)], 8, False, k_sets=2, row_stride=111)
    _refused([ref.Seg(s, off=12)], 13, True, row_stride=111)                                 # the segment reaches past row_stride
    _refused([ref.Seg(s)], 13, True, row_stride=111, tile=1024)
    _refused([ref.Seg(np.zeros(((1 << 20) + 1, 4), dtype=np.uint64))], 13, True, row_stride=(1 << 20) + 1)      # more than 2^20 scalars
