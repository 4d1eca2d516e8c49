"""tests/linkage_ref.py (the NumPy restatement of average linkage that linkage.hip's NN-chain kernel and its host epilogue
follow) against live SciPy: the bits of Z and the flat clusters, on distances of random binary profiles -- small rationals,
so that tied distances are the normal case and the tie rules are what is tested.  No GPU needed."""
import numpy as np
import pytest

from linkage_ref import linkage_average

SIZES = (2, 3, 17, 64, 65, 150, 200)
METRICS = ('jaccard', 'hamming', 'dice')


def cases():
    """(n, metric, repeat, condensed distances): profiles of 5 .. 40 rows, first row set everywhere (no empty profile, so
    dice stays finite)."""
    rng = np.random.default_rng(20240607)
    from scipy.spatial.distance import pdist
    out = []
    for n in SIZES:
        for rep in range(3):
            rows = int(rng.integers(5, 41))
            x = rng.random((n, rows)) < rng.uniform(0.2, 0.6)
            x[:, 0] = True
            for metric in METRICS:
                out.append((n, metric, rep, pdist(x, metric)))
    return out


CASES = cases()


@pytest.mark.parametrize('n, metric, rep, d', CASES, ids=['%s-n%d-%d' % (c[1], c[0], c[2]) for c in CASES])
def test_restatement_equals_scipy_bit_for_bit(n, metric, rep, d):
    from scipy.cluster.hierarchy import fcluster, linkage
    assert np.isfinite(d).all()
    want = linkage(d, method='average')
    got = linkage_average(d, n)
    assert got.shape == want.shape == (n - 1, 4)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    max_d = np.max(want[:, 2] * 0.75)
    assert np.array_equal(fcluster(got, max_d, criterion='distance'), fcluster(want, max_d, criterion='distance'))


def test_most_cases_have_tied_distances():
    tied = sum(len(np.unique(d)) < len(d) for _, _, _, d in CASES)
    assert len(CASES) == 63 and 2 * tied >= len(CASES), (tied, len(CASES))
