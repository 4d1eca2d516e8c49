"""tests/weights_ref.py checks itself, and the parts of neighborhood_weighting that need no device: the closed-form moments of
the weighted score against brute force, the weight kinds against a lattice worked out by hand, the promises the designed inputs
of tests/test_gpu_weights.py make, the settings, and the new symbols.  Seconds, no device."""
import ctypes
import itertools
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as mr
import weights_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKETS = (0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 24.0, 32.0)
NEW_SYMBOLS = ('safe_nbr_weights_from_xy', 'safe_nbr_weights_from_distances', 'safe_nbr_set_weights', 'safe_nbr_weights',
               'safe_nbr_clear_weights', 'safe_score_weighted', 'safe_moments_test_weighted', 'safe_permtest_counts_weighted')


# ---- the moments ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_v', [2, 3, 4, 5, 6, 7])
def test_closed_form_equals_the_enumeration_of_all_permutations(n_v):
    rng = np.random.default_rng(n_v)
    for trial in range(3 if n_v < 7 else 1):
        ws = [Fraction(int(v), 7) for v in rng.integers(0, 9, size=n_v)]
        ws[rng.integers(0, n_v)] = Fraction(0)                  # a non-member
        vals = [Fraction(int(v), 5) for v in rng.integers(-6, 7, size=n_v)]
        assert wr.exact_mean_var(ws, vals) == wr.enumerated_mean_var(ws, vals), (n_v, trial)
    # the whole population at one weight: no permutation moves the score
    assert wr.exact_mean_var([Fraction(1, 10)] * n_v, vals)[1] == 0


def test_closed_form_against_sampled_permutations():
    rng = np.random.default_rng(40)
    n_v, draws = 40, 20000
    w = np.where(rng.uniform(size=n_v) < 0.4, 1.0 - rng.uniform(size=n_v), 0.0)
    v = np.round(rng.normal(size=n_v) * 3, 3)
    mean, var = (float(f) for f in wr.exact_mean_var([Fraction(x) for x in w.tolist()], [Fraction(x) for x in v.tolist()]))
    s = np.array([w @ v[rng.permutation(n_v)] for _ in range(draws)])
    assert abs(s.mean() - mean) <= 5 * np.sqrt(var / draws)
    dev2 = (s - mean) ** 2
    assert abs(dev2.mean() - var) <= 5 * dev2.std() / np.sqrt(draws)


def test_unit_weights_reduce_to_the_unweighted_variance():
    for n_v, k in itertools.product((1, 2, 5, 40), (0, 1, 3, 5, 40)):
        if k > n_v:
            continue
        q = Fraction(17, 3)
        g = wr.exact_row([1.0] * k, n_v)[2]
        assert g * q == mr.exact_var(k, n_v, q), (n_v, k)
    # and in f64 the numerator n_v k - k k is the exact integer k (n_v - k): g has the bits of f
    indptr, indices = wr.csr_of(np.triu(np.ones((50, 50))))
    g = wr.row_sums(indptr, indices, np.ones(len(indices)), np.ones(50, dtype=bool), 50)[3]
    k = np.arange(50, 0, -1).astype(np.float64)
    assert np.array_equal(g, np.where(k < 50, (k * (50 - k)) / (50.0 * 49.0), 0.0))


# ---- the weight kinds -------------------------------------------------------------------------------------------------------

def test_weight_kinds_on_a_lattice_worked_out_by_hand():
    xy = np.array([(x, y) for y in range(3) for x in range(3)], dtype=np.float64)      # node 4 is the centre
    a = np.zeros((9, 9), dtype=np.int64)
    a[4] = 1                                                    # radius 2 under `<=`: every node (corners at sqrt 2)
    a[0, [0, 1, 3]] = 1                                         # radius 1 under `<=`: d == r members
    a[8, 8] = 1                                                 # radius 0
    a[np.arange(9), np.arange(9)] = 1
    radii = np.array([1, 1, 1, 1, 2, 1, 1, 1, 0], dtype=np.float64)
    indptr, indices = wr.csr_of(a)
    d = wr.euclidean_member_distances(xy, indptr, indices)
    row = lambda w, i: w[indptr[i]:indptr[i + 1]].tolist()      # noqa: E731
    s2 = np.sqrt(2.0)
    assert row(d, 4) == [s2, 1, s2, 1, 0, 1, s2, 1, s2] and row(d, 0) == [0, 1, 1]
    tri = wr.member_weights('triangular', d, indptr, radii)
    assert row(tri, 0) == [1.0, 0.0, 0.0]                       # d == r: weight 0, still a member
    assert row(tri, 4) == [1 - s2 / 2, 0.5, 1 - s2 / 2, 0.5, 1.0, 0.5, 1 - s2 / 2, 0.5, 1 - s2 / 2]
    assert row(tri, 8) == [1.0]                                 # r = 0: u = 0, never 0 / 0
    epa = wr.member_weights('epanechnikov', d, indptr, radii)
    u = s2 / 2
    assert row(epa, 4) == [1 - u * u, 0.75, 1 - u * u, 0.75, 1.0, 0.75, 1 - u * u, 0.75, 1 - u * u] and row(epa, 0) == [1.0, 0.0, 0.0]
    gau = wr.member_weights('gaussian', d, indptr, radii, h=0.5)
    assert row(gau, 0) == [1.0, np.exp(-2.0), np.exp(-2.0)] and row(gau, 8) == [1.0]
    assert row(gau, 4)[1] == np.exp(-0.5) and row(gau, 4)[0] == np.exp(-0.5 * ((u / 0.5) * (u / 0.5)))
    assert (wr.member_weights('uniform', d, indptr, radii) == 1.0).all()
    assert not np.isnan(np.concatenate([tri, epa, gau])).any()
    with pytest.raises(ValueError):
        wr.weights('cosine', d, 1.0)


def test_k_exp_ref():
    k = wr.k_exp_ref()
    print('K_exp_ref = %.3f ulp' % k)
    assert 0.0 < k < 1.0                                        # (0.65 measured: np.exp is faithfully rounded here)
    a = wr.gaussian_test_arguments()
    assert len(a) == 4000 and a.min() >= -8.0 and a.max() <= 0.0
    assert wr.exp_error_ulps(a[:50], wr.exp_correctly_rounded(a[:50])) <= 0.5


# ---- the designed inputs keep their promises --------------------------------------------------------------------------------

def test_designed_case_keeps_its_promises():
    case, indptr, indices, w = wr.designed()
    x, rows, z = wr.designed_cells()
    assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() < 2.0 ** 40           # every x a multiple of 1/8
    assert set(np.unique(w * 8).tolist()) <= set(range(1, 9))
    assert max(case.n_v * r[1] for r in rows) < 2 ** 21                                      # n_v W2
    # the f64 row sums are the rationals, so g differs from the exact one by its single division
    w1, w2, c, g = wr.row_sums(indptr, indices, w, case.flags, case.n_v)
    assert all(Fraction(a) == r[0] and Fraction(b) == r[1] for a, b, r in zip(w1.tolist(), w2.tolist(), rows))
    assert np.array_equal(c, case.k)
    g_zero = np.array([r[2] == 0 for r in rows])
    assert np.array_equal(g_zero, g == 0.0)
    q_zero = np.array([q == 0 for q in case.q])
    degenerate = g_zero[:, None] | q_zero[None, :]
    share = degenerate.mean()
    print('degenerate cells: %.1f %%' % (100 * share))
    assert share <= 0.07
    zs = np.array(sorted(set(float(v[0]) for v in z.values() if v[0] is not None)))
    assert (zs > 0).any() and (zs < 0).any()
    found = [len(np.unique(np.abs(zs)[(np.abs(zs) >= lo) & (np.abs(zs) < hi)])) for lo, hi in zip(BUCKETS, BUCKETS[1:] + (np.inf,))]
    print('distinct |z| per bucket:', dict(zip(BUCKETS, found)))
    assert min(found) >= 200, found
    # the degenerate kinds are all present: n_v of the whole population at one weight needs weights of its own (GPU test)
    assert any(r[2] == 0 and r[0] == 0 for r in rows) and q_zero.sum() == 2


def test_order_sensitive_input_is_sensitive_to_the_order():
    for members, floor in ((64, 0.5), (300, 0.5), (2049, 0.5)):
        n = max(members, 80)
        a, b, indptr, indices, w = wr.order_sensitive(n, 5, seed=members, big_row=members)
        big = np.diff(indptr) >= 64
        up = wr.score(indptr, indices, w, b)
        down = wr.score(indptr, indices, w, b, descending=True)
        share = (up[big] != down[big]).mean()
        print('%d members: %.2f of the cells differ' % (members, share))
        assert big.any() and share >= floor
        np.testing.assert_allclose(up, down, rtol=1e-9, atol=1e-9)


def test_score_restatement_against_a_plain_loop():
    a, b, indptr, indices, w = wr.order_sensitive(30, 3, seed=1)
    b[3, 1] = np.nan
    want = np.zeros((30, 3))
    for i in range(30):
        for j in range(3):
            acc = 0.0
            for e in range(indptr[i], indptr[i + 1]):
                v = b[indices[e], j]
                acc = acc + w[e] * (0.0 if v != v else v)
            want[i, j] = acc
    assert np.array_equal(wr.score(indptr, indices, w, b), want)
    t = np.random.default_rng(0).permutation(30)
    assert np.array_equal(wr.score(indptr, indices, w, b, source_rows=t), wr.score(indptr, indices, w, b[t]))
    x, neg, pos = wr.counts(indptr, indices, w, b, [np.arange(30), t])
    assert (neg >= 1).all() and (pos >= 1).all() and (neg + pos >= 2).all()


# ---- settings, pickling, refusals without a device --------------------------------------------------------------------------

@pytest.fixture()
def sf():
    import safepy_amd
    return safepy_amd.SAFE(verbose=False)


def test_validate_config_restores_the_defaults(sf):
    assert sf.neighborhood_weighting == 'none' and sf.neighborhood_weight_bandwidth == 0.5 and sf.neighborhood_weights is None
    for kind in ('none', 'uniform', 'triangular', 'epanechnikov', 'gaussian', 'custom'):
        sf.neighborhood_weighting = kind
        sf.validate_config()
    for bad in ('cosine', None, 3, ['gaussian']):
        sf.neighborhood_weighting = bad
        with pytest.raises(ValueError, match='neighborhood_weighting'):
            sf.validate_config()
        assert sf.neighborhood_weighting == 'none'
    for bad in (0, -1.0, np.inf, np.nan, '0.5', None, True):
        sf.neighborhood_weight_bandwidth = bad
        with pytest.raises(ValueError, match='neighborhood_weight_bandwidth'):
            sf.validate_config()
        assert sf.neighborhood_weight_bandwidth == 0.5
    sf.neighborhood_weight_bandwidth = 2
    sf.validate_config()


def test_pickling_keeps_the_settings_and_old_pickles_get_the_defaults(sf):
    sf.neighborhood_weighting, sf.neighborhood_weight_bandwidth = 'gaussian', 0.25
    sf._weights_host = (np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1.0, 0.0]))
    back = pickle.loads(pickle.dumps(sf))
    assert back.neighborhood_weighting == 'gaussian' and back.neighborhood_weight_bandwidth == 0.25
    w = back.neighborhood_weights
    assert w.shape == (2, 2) and w.nnz == 2 and w.data.tolist() == [1.0, 0.0]               # the explicit zero is kept
    state = sf.__getstate__()
    for name in ('neighborhood_weighting', 'neighborhood_weight_bandwidth', '_weights_host'):
        del state[name]
    old = type(sf).__new__(type(sf))
    old.__setstate__(state)
    assert old.neighborhood_weighting == 'none' and old.neighborhood_weight_bandwidth == 0.5 and old.neighborhood_weights is None
    old.validate_config()


def test_refusals_that_need_no_device(sf):
    with pytest.raises(ValueError, match='set_neighborhood_weights'):
        sf.define_neighborhoods(neighborhood_weighting='custom')
    assert sf._nbr is None and sf.neighborhoods is None
    sf.neighborhood_weighting = 'triangular'
    with pytest.raises(ValueError, match='carry no weights'):   # the setting alone, on neighborhoods without weights
        sf.compute_pvalues(how='analytic')
    sf._weights_host = (np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1.0]))
    with pytest.raises(ValueError, match="'analytic' or how = 'randomization'"):
        sf.compute_pvalues(how='hypergeometric')
    with pytest.raises(ValueError, match='z-score'):
        sf.compute_pvalues(how='randomization', neighborhood_score_type='z-score')
    assert sf.ns is None and sf.nes is None and sf.pvalues_pos is None
    # assigning neighborhoods drops the weights; 'custom' goes back to 'none'
    sf.neighborhood_weighting = 'custom'
    sf.neighborhoods = np.eye(3, dtype=np.int64)
    assert sf.neighborhood_weighting == 'none' and sf._weights_host is None and sf.neighborhood_weights is None


def test_member_weights_of_a_custom_matrix():
    from scipy import sparse
    from safepy_amd.safe import _member_weights
    a = np.array([[1, 1, 0], [0, 1, 0], [1, 1, 1]])
    indptr, indices = wr.csr_of(a)
    w = np.array([[0.5, 0.0, 0.0], [0.0, 2.0, 0.0], [0.25, 0.0, 1.0]])
    want = [0.5, 0.0, 2.0, 0.25, 0.0, 1.0]
    assert _member_weights(w, indptr, indices).tolist() == want
    assert _member_weights(sparse.csr_array(w), indptr, indices).tolist() == want               # members W does not store get 0
    assert _member_weights(sparse.coo_matrix(w), indptr, indices).tolist() == want
    for bad in (np.where(a, -1.0, 0.0), np.where(a, np.nan, 0.0), np.where(a, np.inf, 0.0), np.ones((3, 3)), np.ones((2, 3)),
                np.ones(3), sparse.csr_array(np.ones((3, 3))), sparse.csr_array(np.where(a, -1.0, 0.0))):
        with pytest.raises(ValueError):
            _member_weights(bad, indptr, indices)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_in_header_binding_and_library():
    from safepy_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'safe_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.WEIGHT_KINDS == {'uniform': 0, 'triangular': 1, 'epanechnikov': 2, 'gaussian': 3}
    for kind, value in _lib.WEIGHT_KINDS.items():
        assert re.search(r'#define SAFE_WEIGHT_%s %d\b' % (kind.upper(), value), header)
