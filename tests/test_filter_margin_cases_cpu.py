"""The designed near-tie inputs of tests/filter_margin_cases.py are what they claim to be (no GPU): exact six-slice columns,
deterministic, an exact reference that equals the oracle where the oracle is exact, and -- so that the GPU tests cannot pass
vacuously -- a large share of all compares next to each decision margin."""
import numpy as np
import pytest

import filter_margin_cases as fm
from oracle import safe_oracle as orc


@pytest.mark.parametrize('name', sorted(set(fm.CASES) - {'Z-exact'}))
def test_columns_are_exact_six_slice_images(name):
    """k_mfma_colfinish: unit = the lowest set bit of a column when top bit - lowest bit + 1 <= 47; six slices above 30 bits.
    One odd value and a maximum in [2^31, 2^46): the image is the value itself."""
    case = fm.CASES[name]()
    q, present = fm.image(case.b)
    assert case.xy.shape[0] == q.shape[0] >= 257                        # the matrix-core forms do not run below that
    for j in range(q.shape[1]):
        col = q[present[:, j], j]
        assert (col & 1).any(), (name, j)
        span = int(np.abs(col).max()).bit_length()
        assert 30 < span <= 46, (name, j, span)
    hi, lo = fm.split_digits(q)
    assert (hi * (1 << 24) + lo == q).all()
    assert lo.min() >= -fm.MF_LO_MAX and lo.max() <= fm.LO_TOP
    assert hi.min() >= -fm.MF_LO_MAX and hi.max() <= fm.LO_TOP       # three balanced digits each


def test_low_parts_sit_at_their_extremes():
    for make in (fm.s_offset, fm.s_dense, fm.s_zero):
        case = make()
        q, present = fm.image(case.b)
        _, lo = fm.split_digits(q)
        plain = np.ones(q.shape[1], dtype=bool)
        plain[[3, 5, 7]] = False                                        # (the designed columns of S-zero and S-offset)
        plain[-1] = case.name != 'S-zero'                               # (negated: the ends swap, + 1)
        lo = lo[1:, plain][present[1:, plain]]
        assert 0.3 < np.mean(lo == -fm.MF_LO_MAX) < 0.4 and 0.3 < np.mean(lo == fm.LO_TOP) < 0.4, case.name


def test_generators_are_deterministic():
    for name, make in fm.CASES.items():
        first = make()
        getattr(make, 'cache_clear', fm.s_top.cache_clear)()
        again = make()
        assert again is not first
        np.testing.assert_array_equal(first.xy, again.xy)
        np.testing.assert_array_equal(first.b, again.b)
        assert (first.seed, first.nperms, first.radius) == (again.seed, again.nperms, again.radius)


def test_layouts_have_the_member_counts_they_are_built_for():
    cnt = fm.s_offset().a.sum(axis=1)
    assert cnt.min() >= 1 and 20 <= cnt.max() <= 32 and 12 <= cnt.mean() <= 18
    cnt = fm.s_dense().a.sum(axis=1)
    assert cnt.max() >= 3 * cnt.min() and cnt.max() < 2048              # two densities
    for hub in (2047, 2048):
        cnt = fm.s_top(hub).a.sum(axis=1)
        assert cnt.max() == hub and np.count_nonzero(cnt == hub) == hub and np.sort(cnt)[-hub - 1] < 100
    case = fm.z_count()
    values = case.a @ (~np.isnan(case.b)).astype(np.int64)
    assert values.min() == 0 and values.max() >= 5
    assert 0.2 < np.mean(values >= 3) < 0.8                             # the count of present values crosses 3 all over


def test_s_zero_has_observed_sums_of_both_signs_and_exact_zeros():
    case = fm.s_zero()
    obs = fm.exact_sums(case.a, case.b)
    for j in range(obs.shape[1]):
        assert (obs[:, j] < 0).any() and (obs[:, j] > 0).any(), j
    assert np.count_nonzero(obs[:, 3] == 0) >= 20
    assert case.b[0, -1] == -2.0 ** 40 and np.abs(case.b[1:, -1]).max() < 2.0 ** 28


def test_s_top_reaches_the_top_of_the_range():
    case = fm.s_top(2047)
    obs = fm.exact_sums(case.a, case.b)
    assert np.abs(case.b).max() < 2.0 ** 46 and np.abs(case.b).min() > 2.0 ** 46 - 2.0 ** 35
    assert obs[:, 0].max() > 2046 * (2 ** 46 - 2 ** 35) and obs[:, 1].min() < -2046 * (2 ** 46 - 2 ** 35)   # ~ 2^57


@pytest.mark.parametrize('name', ['S-offset', 'S-dense', 'S-zero'])
def test_exact_counts_equal_the_oracle_where_its_sums_are_exact(name):
    """(Sums below 2^52: the oracle's f64 products and sums are exact.)"""
    case = fm.CASES[name]()
    assert np.abs(fm.exact_sums(case.a, case.b)).max() < 2 ** 52
    tables = orc.permutation_index_table(case.b, fm.NPERM, case.seed)
    neg, pos = fm.exact_counts(case.a, case.b, tables)
    neg_w, pos_w = orc.run_permutations(case.a, case.b, 'sum', fm.NPERM, case.seed)
    np.testing.assert_array_equal(neg, neg_w)
    np.testing.assert_array_equal(pos, pos_w)
    np.testing.assert_array_equal(fm.exact_sums(case.a, case.b), orc.compute_neighborhood_score(case.a, case.b, 'sum'))
    assert (neg + pos >= fm.NPERM).all()


def test_the_all_equal_column_ties_everywhere_and_the_spike_saturates_a_counter():
    case = fm.s_offset()
    tables = orc.permutation_index_table(case.b, 255, case.seed)
    neg, pos = fm.exact_counts(case.a, case.b[:, [5, 7]], tables)
    assert (neg[:, 0] == 255).all() and (pos[:, 0] == 255).all()
    assert np.count_nonzero((neg[:, 1] == 255) & (pos[:, 1] == 0)) >= 1  # #< = 255: an 8-bit field at its top before the flush


# ---------------------------------------------------------------------------------------------------------------------
# density: the share of all live compares in each band next to the margin.  Conditions on the INPUTS, about half of what the
# generators give (S-offset 39 / 30 / 26 %, S-dense 38 / 29 / 27 %, S-zero 32 / 26 / 29 %, Z-near 9.1 / 6.5 / 5.9 % when the
# families were designed); if a parameter changes, retune the parameter, not the condition.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['S-offset', 'S-dense', 'S-zero'])
def test_sum_families_put_15_percent_of_their_compares_in_every_band(name):
    share = fm.band_census(fm.CASES[name]())
    assert (share >= 0.15).all(), dict(zip(fm.SUM_BANDS, share))


def test_z_near_puts_3_percent_of_its_compares_in_every_band():
    share = fm.band_census(fm.z_near())
    assert (share >= 0.03).all(), dict(zip(fm.Z_BANDS, share))
