"""The count-to-distance formulas of safe_profile_distances (tests/domain_metrics_ref.py, the table the kernel's epilogue
restates) against live scipy.spatial.distance.pdist, called on f64 0/1 matrices as linkage(m, metric=...) calls it: a few
thousand count quadruples -- every pair of random profiles of several densities at lengths on both sides of a bit word,
plus designed quadruples with every combination of zero counts (all the zero denominators).  Bit for bit; NaN only where
SciPy gives NaN.  Needs no device: this pins the operation order and the zero-denominator values, not the kernel."""
import itertools

import numpy as np
import pytest
from scipy.spatial.distance import pdist

from domain_metrics_ref import METRICS, distance_from_counts, profiles_from_counts

pytestmark = pytest.mark.filterwarnings('ignore:The sokalmichener metric:DeprecationWarning')


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def pair_counts(x):
    """ntt, ntf, nft of every pair of rows of the 0/1 matrix x in pdist's condensed order."""
    i, j = np.triu_indices(x.shape[0], 1)
    b = x != 0
    ntt = (b[i] & b[j]).sum(axis=1)
    ntf = (b[i] & ~b[j]).sum(axis=1)
    nft = (~b[i] & b[j]).sum(axis=1)
    return ntt, ntf, nft


@pytest.mark.parametrize('metric', METRICS)
def test_formula_equals_scipy_on_random_profiles(metric):
    rng = np.random.default_rng(7)
    checked = 0
    for n in (1, 2, 63, 64, 65, 200, 1001):
        dens = rng.choice([0.0, 0.02, 0.3, 0.5, 0.9, 1.0], size=40)
        x = (rng.uniform(size=(40, n)) < dens[:, None]).astype(np.float64)
        ntt, ntf, nft = pair_counts(x)
        assert same_bits(distance_from_counts(metric, ntt, ntf, nft, n), pdist(x, metric)), n
        checked += ntt.size
    assert checked >= 5000


@pytest.mark.parametrize('metric', METRICS)
def test_formula_equals_scipy_where_counts_are_zero(metric):
    for ntt, ntf, nft, nff in itertools.product((0, 1, 5, 64), repeat=4):
        n = ntt + ntf + nft + nff
        if n == 0:
            continue
        want = pdist(profiles_from_counts(ntt, ntf, nft, nff), metric)
        assert same_bits(distance_from_counts(metric, [ntt], [ntf], [nft], [n]), want), (ntt, ntf, nft, nff, want)
