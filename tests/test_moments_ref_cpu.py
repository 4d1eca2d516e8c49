"""The reference of the analytic test (tests/moments_ref.py) and the host side of how = 'analytic' where no GPU exists: the
closed-form moments against ALL permutations and against scipy's hypergeometric moments, the measured constant K_ref of the
p-value bound, the coverage of the GPU test's designed cells, the refusals that need no device, and the two new symbols."""
import ctypes
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_inputs():
    """(column, flags, members) with n_v <= 7, rows without a value, NaN cells inside the population."""
    nan = float('nan')
    yield [1.0, 0.0, 2.5, nan, -3.0], [1, 1, 1, 0, 1], [1, 0, 1, 1, 0]
    yield [0.25, nan, nan, 4.0, 1.0, 1.0, -2.0, 7.0, nan], [1, 1, 0, 1, 1, 1, 1, 1, 0], [1, 1, 1, 0, 0, 1, 0, 1, 1]
    yield [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [1] * 7, [1, 0, 1, 0, 1, 0, 0]
    yield [3.0, 3.0, 3.0, 3.0], [1] * 4, [1, 1, 0, 0]                               # constant: variance 0
    yield [5.0, nan, 1.0], [1, 0, 1], [0, 1, 0]                                     # k = 0
    yield [5.0, nan, 1.0, 2.0], [1, 0, 1, 1], [1, 1, 1, 1]                          # k = n_v
    rng = np.random.default_rng(3)
    for n_v in (2, 3, 5, 6, 7):
        col = np.round(rng.normal(size=n_v + 2), 2)
        flags = np.ones(n_v + 2, dtype=int)
        flags[[1, n_v]] = 0
        col[[1, n_v]] = np.nan
        col[0] = np.nan                                                             # a NaN cell in a row that counts
        for members in (rng.uniform(size=n_v + 2) < 0.5, rng.uniform(size=n_v + 2) < 0.8):
            yield col.tolist(), flags.tolist(), members.astype(int).tolist()


def test_formulas_equal_the_moments_of_every_permutation():
    seen = 0
    for column, flags, members in small_inputs():
        pop = [0.0 if v != v else v for v, f in zip(column, flags) if f]
        n_v, k = len(pop), sum(1 for f, mem in zip(flags, members) if f and mem)
        assert n_v <= 7
        mu, q = mr.exact_column(pop)
        mean, var = mr.enumerated_moments(column, flags, members)
        assert mean == k * mu, (column, flags, members)
        assert var == mr.exact_var(k, n_v, q), (column, flags, members)
        seen += 1
    assert seen >= 16


def test_moments_of_01_columns_are_the_hypergeometric_ones():
    from scipy.stats import hypergeom
    case = mr.designed()[0]
    for j, ones in enumerate(mr.ONES):
        assert case.mu[j] * case.n_v == ones
        for k in (1, 2, 7, 64, 1000, 2047):
            assert float(k * case.mu[j]) == pytest.approx(hypergeom.mean(case.n_v, ones, k), rel=1e-12)
            assert float(mr.exact_var(k, case.n_v, case.q[j])) == pytest.approx(hypergeom.var(case.n_v, ones, k), rel=1e-12)


def test_exact_z_and_tails_on_hand_checked_values():
    # n_v = 4, values 1 0 0 0: mu = 1/4, Q = 3/4; k = 1, x = 1: var = 3/12 * 3/4 = 3/16, z = (3/4) / sqrt(3/16) = sqrt 3
    z, sd, kmu = mr.exact_z(Fraction(1), 1, 4, Fraction(1, 4), Fraction(3, 4))
    assert abs(z - mr.MP.sqrt(3)) < mr.MP.mpf(10) ** -45 and abs(sd - mr.MP.sqrt(3) / 4) < mr.MP.mpf(10) ** -45 and kmu == 0.25
    assert mr.exact_z(Fraction(0), 1, 4, Fraction(1, 4), Fraction(3, 4))[0] < 0
    for degenerate in ((1, 1, 1), (0, 4, 1), (4, 4, 1), (2, 4, 0)):
        k, n_v, q = degenerate
        assert mr.exact_z(Fraction(1), k, n_v, Fraction(1, 4), Fraction(q)) == (None, None, None)
    assert float(mr.small_side(0)) == 0.5
    assert float(mr.small_side(-1.959963984540054)) == pytest.approx(0.025, rel=1e-15)
    assert float(mr.upper_tail(-1.959963984540054)) == pytest.approx(0.975, rel=1e-15)
    assert 0 < float(mr.small_side(37.6)) < mr.SMALL_MAX < float(mr.small_side(37.5))


def test_measured_constant_of_the_p_value_bound():
    """K_ref: scipy.special.ndtr(-z) against mpmath over the GPU test's own z list, in units of (1 + z^2) 2^-53."""
    k = mr.designed_k_ref()
    print('K_ref = %.3f over %d designed z values' % (k, int((np.abs(mr.designed_z()[0]) <= mr.Z_EDGE).sum())))
    assert np.isfinite(k) and 0 < k < 16
    libm = mr.k_ref(mr.designed_z()[0], tail=lambda z: 0.5 * math.erfc(z * 0.7071067811865476))
    print('the C library\'s erfc used the same way: %.3f' % libm)


def test_designed_cells_cover_what_the_gpu_test_claims():
    z, kinds = mr.designed_z()
    inside = z[(z >= -8) & (z <= mr.Z_EDGE)]
    assert len(inside) >= 200
    assert inside.min() <= -7.5 and inside.max() >= 37.0
    assert (np.histogram(inside, bins=[-8, -4, 0, 4, 8, 16, 24, 32, mr.Z_EDGE])[0] > 0).all()
    assert (z < 0).any() and (z > 0).any() and (np.abs(z) < 1e-3).any()
    assert all(count >= 1 for count in kinds.values()), kinds
    assert (np.abs(z) > mr.Z_EDGE).sum() >= 5
    # P[Z >= 37.5] = 4.6e-308 is still above SMALL_MAX; the tail passes it at |z| = 37.519, so no designed cell sits between
    assert not ((np.abs(z) > mr.Z_EDGE) & (np.abs(z) <= 37.52)).any()
    case = mr.designed()[0]
    assert case.n_v == mr.N_V and (np.abs(np.nan_to_num(case.b)) <= 1024).all()
    assert (np.nan_to_num(case.b) == np.floor(np.nan_to_num(case.b))).all()
    for j in range(case.b.shape[1]):                             # every mean and every Q is an exact double
        assert Fraction(float(case.mu[j])) == case.mu[j] and Fraction(float(case.q[j])) == case.q[j]


def test_p_cut_and_decisions():
    assert mr.p_cut(0.05) == pytest.approx(0.05, rel=1e-14)
    pp, pn = np.array([0.01, 0.5, 0.999, 0.0]), np.array([0.99, 0.5, 0.001, 1.0])
    nes = mr.nes_of(pp, pn, 'both')
    assert np.array_equal(mr.decisions(pp, pn, nes, 'highest', 0.05), [1, 0, 0, 1])
    assert np.array_equal(mr.decisions(pp, pn, nes, 'lowest', 0.05), [0, 0, 1, 0])
    assert np.array_equal(mr.decisions(pp, pn, nes, 'both', 0.05), [1, 0, 1, 1]) and nes[3] == np.inf


def test_periodic_cases_have_few_distinct_cells():
    for n, m in ((1, 1), (2, 63), (33, 1024)):
        case = mr.periodic_case(n, m, 1)
        assert case.a.shape == (n, n) and case.b.shape == (n, m)
        assert len({(i % 5, j % 7) for i, j in itertools.product(range(n), range(m))}) <= 35
        assert np.array_equal(case.a, case.a[np.arange(n) % 5]) and np.array_equal(mr.row_flags(case.b), case.flags)
        both_nan = np.isnan(case.b) & np.isnan(case.b[:, np.arange(m) % 7])
        assert ((case.b == case.b[:, np.arange(m) % 7]) | both_nan).all()


# ---- the host side ----------------------------------------------------------------------------------------------------------

def test_analytic_with_z_scores_is_refused_before_any_device_work():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.node2attribute = np.zeros((4, 2))
    with pytest.raises(ValueError, match="'sum' only"):
        sf.compute_pvalues(how='analytic', neighborhood_score_type='z-score')
    with pytest.raises(ValueError, match="'sum' only"):
        sf.compute_pvalues_by_moments()                          # (the setting sticks, as every kwarg of compute_pvalues does)
    assert hasattr(safepy_amd.SAFE, 'compute_pvalues_by_moments')


def test_the_sharded_route_refuses_analytic():
    from safepy_amd import sharding
    with pytest.raises(ValueError, match='analytic'):
        sharding.sharded_compute_pvalues(None, None, np.zeros((4, 2)), 2, enrichment_type='analytic')


def test_header_binding_and_library_agree_on_the_new_symbols():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in {'safe_attr_column_moments': 5, 'safe_moments_test': 14}.items():
        m = re.search(r'\bint %s\s*\(([^;]*)\);' % name, code)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        assert hasattr(raw, name), name
    test = _lib.PROTOTYPES['safe_moments_test'][1]
    assert test[3] is ctypes.c_int and test[4] is ctypes.c_double and test[5] is ctypes.c_int64 and test[6] is ctypes.c_int64
    assert hasattr(backend, 'moments_test') and hasattr(backend.Attributes, 'column_moments')
    assert 'safe_moments_test' in header[:header.index('#ifndef SAFE_HIP_H')]      # returns once the stream has drained
    # NULL arguments are refused before a device is touched
    assert _lib.lib.safe_attr_column_moments(None, 0, 1, None, None) == _lib.E_INVALID
    assert _lib.lib.safe_moments_test(None, None, None, 2, 0.05, 0, 1, *[None] * 7) == _lib.E_INVALID
    # the symbols are additive: header, binding and library agree on one ABI version
    version = int(re.search(r'#define SAFE_HIP_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == raw.safe_abi_version()
