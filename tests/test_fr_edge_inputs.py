"""The inputs of tests/test_gpu_fr_edges.py reach the edges they are built for (no GPU, nothing about a kernel): the cancelling rows put a lazily reduced sum
on exactly r and on exactly 2r — the two values at which a conditional subtraction takes its `equal` branch — the edge set is canonical, and every long-carry
row carries through the limbs it names."""
import fr_edges as E


def test_redc_model_is_a_montgomery_product_without_the_final_subtraction():
    for a, b in zip(E.uniform(200, 1) + E.E, E.uniform(200, 2) + E.E[::-1]):
        t = E.redc_lazy(a, b)
        assert t % E.R == E.mmul(a, b) and t < a * b // E.W + E.R + 1 and t < 2 * E.R


def test_cancelling_rows_of_the_one_term_lin_land_on_r_and_on_2r():
    rows = E.lin_one_term_cancelling()
    assert len(rows) == E.CANCEL_ROWS == 2048
    assert all((c0 + E.mmul(c1, a)) % E.R == 0 and c0 < E.R and 0 < c1 < E.R and a < E.R for c0, c1, a in rows)
    at_r, at_2r = E.lazy_sum_counts(rows)
    print('lazy sums of %d rows: %d at r, %d at 2r' % (len(rows), at_r, at_2r))
    assert at_r + at_2r == len(rows) - sum(c0 == 0 for c0, _, _ in rows)      # a row is on one of the two unless it is 0 + 0
    assert at_r >= 8 and at_2r >= 8


def test_edge_set_is_canonical_and_holds_what_it_names():
    assert len(E.E) == 18 and len(set(E.E)) == 18
    assert all(0 <= v < E.R for v in E.E)
    assert E.ONE == (1 << 256) % E.R and E.mmul(E.ONE, E.ONE) == E.ONE and E.mmul(E.ONE, 12345) == 12345
    assert (E.R - 1) // 2 + (E.R + 1) // 2 == E.R
    ones = E.E[15]
    assert E.limbs32(ones)[:7] == [0xffffffff] * 7 and ones < E.R <= ones + (1 << 224)      # the largest such value below r
    for v in E.E:
        for w in E.E_NONZERO: assert E.mmul(E.msolve(v, w), w) == v
    for w in E.E_NONZERO: assert E.mmul(E.minv(w), w) == E.ONE
    a, b = E.edge_pairs()
    assert len(a) == len(b) >= 257 and set(zip(a, b)) == {(x, y) for x in E.E for y in E.E}
    assert len(set(zip(*E.edge_triples()))) == 18 ** 3
    t = E.targets()
    assert t.count(0) == 2048 and t.count(1) >= 2 and t.count(E.R - 1) >= 2
    assert E.ints(E.limbs(E.E)) == E.E and E.ints(E.limbs([E.R * 2 - 1, (1 << 381) - 1], 6)) == [E.R * 2 - 1, (1 << 381) - 1]


def test_long_carry_rows_carry_through_the_limbs_they_name():
    assert [k for _, _, k in E.CARRY_ADD] == [k for _, _, k in E.CARRY_SUB] == [32, 64, 96, 128, 160, 192, 224]
    for a, b, k in E.CARRY_ADD:
        assert a < E.R and b < E.R and E.carry_limbs(a, b) == list(range(k // 32)) and a + b == 1 << k
    for a, b, k in E.CARRY_SUB:
        assert a < E.R and b < E.R and E.borrow_limbs(a, b) == list(range(k // 32)) and a - b == (1 << k) - 1
    # a - a borrows nowhere, and r + a - a (what the device forms) is r itself: the value the last conditional subtraction must take away
    for a in E.E: assert E.borrow_limbs(a, a) == [] and E.carry_limbs(E.R, 0) == []
    # r - 1 + 1 = r: the sum of two canonical values that lands on r with a carry through the low limb
    assert E.carry_limbs(E.R - 1, 1) == [] and E.carry_limbs((1 << 252) - 1, 1) == list(range(7))
