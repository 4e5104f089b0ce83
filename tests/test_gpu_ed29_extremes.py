"""The 29-bit-limb product and the Edwards helpers of aleo_amd/csrc/edwards29.h on the GPU at the EDGES of their operand classes, against Python integers.

Every account-side kernel (record scan, decrypt, serial numbers, commitments, signatures, accounts, key ciphertexts, plaintexts) reaches this arithmetic with
canonical inputs and whatever its own formulas produce, so multiplicands with limbs of 5 * 2^29 - 1 next to 2^261, multipliers whose every digit is 2^29 - 1,
coordinates at the largest representative below 3 r, the identity and the points of order 2 and 4 never reach the kernels.  Here the host builds every limb
(tests/ed29_rows.py; aleo_mi355x_selftest_ed29_rows: raw limbs in, raw limbs out, the device converts nothing), 256 rows — four waves — per kernel with the special
rows in the first and the last lane of a wave and between ordinary neighbours, and every output is checked exactly: the product limb for limb against
(a b + m r) / 2^261, tidy and canonical against their definitions, a point against the affine law, T Z = X Y, exact digits and the value bound the host checker
(tests/test_ed29_bounds.py) establishes for that formula.  The same rows pass through the host's bounded field in tests/test_ed29_bounds.py, which validates the
rows and this reference without a GPU.
"""
import ctypes
import numpy as np
import pytest

import aleo_amd
import ed29_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cases():
    """The rows, what they must give and ONE run of the five kernels, shared by every test below."""
    c = ed29_rows.build()
    L = aleo_amd.lib()
    aleo_amd._lib.check(L.aleo_mi355x_init_device(-1), 'init')
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = {name: np.zeros_like(c[like]) for name, like in ed29_rows.OUTPUTS}
    aleo_amd._lib.check(L.aleo_mi355x_selftest_ed29_rows(vp(c['mul_a']), vp(c['mul_b']), len(c['mul_a']), vp(out['out_mul']), vp(c['tidy']), len(c['tidy']), vp(out['out_tidy']),
                                                         vp(c['canon']), len(c['canon']), vp(out['out_canon']), vp(c['p']), vp(c['q']), vp(c['neg']), vp(c['d2']), len(c['p']),
                                                         vp(out['out_add']), vp(c['dbl']), vp(c['want_t']), len(c['dbl']), vp(out['out_dbl'])), 'selftest_ed29_rows')
    return c, out


def test_inputs_cover_the_edges(cases):
    ed29_rows.check_coverage(cases[0])


def test_products_tidies_and_canonical_forms_equal_the_integers_limb_for_limb(cases):
    ed29_rows.check_fields(*cases)


def test_additions_and_doublings_keep_the_contract_and_equal_the_affine_law(cases):
    ed29_rows.check_points(*cases)


def test_bad_arguments_are_refused():
    L = aleo_amd.lib()
    n = None
    assert L.aleo_mi355x_selftest_ed29_rows(n, n, 1, n, n, 0, n, n, 0, n, n, n, n, n, 0, n, n, n, 0, n) == 2
    assert L.aleo_mi355x_selftest_ed29_rows(n, n, 0, n, n, 0, n, n, 0, n, n, n, n, n, 1, n, n, n, 0, n) == 2
    assert L.aleo_mi355x_selftest_ed29_rows(n, n, 0, n, n, 0, n, n, 0, n, n, n, n, n, 0, n, n, n, (1 << 20) + 1, n) == 2
