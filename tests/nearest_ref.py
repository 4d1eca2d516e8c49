"""The rule of neighborhood_radius_type = 'nearest' restated in NumPy, and the inputs its tests share.  NumPy / SciPy only:
nothing here touches the library.

D is the node-distance matrix of a metric, on the bits: squareform(pdist(xy)) for 'euclidean', the all-pairs shortest-path
lengths (+inf where unreached) otherwise.  For node i, cand_i = {D[i, j] : j != i} -- node i is left out by INDEX, a coincident
node at distance 0 is a candidate; for the shortest-path metrics only the finite entries count -- and

    r_i = sorted(cand_i)[min(k, len(cand_i)) - 1],        0.0 when cand_i is empty;
    A[i, j] = 1  iff  D[i, j] <= r_i                      (and, for a shortest-path matrix, j reached from i).

Every comparison built on this module is on bits."""
import numpy as np
from scipy.spatial.distance import pdist, squareform

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 2049)     # both sides of the wave, the 256-thread sweep, the 2048 bins
TIE_XY = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 2.0 ** -26), (5.0, 5.0), (-7.0, 3.0)])
# from node 0 the squares to nodes 1 and 2 are 1.0 and 1 + 2^-52: different doubles with the same correctly rounded root


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def euclid(xy):
    xy = np.asarray(xy, dtype=np.float64)
    with np.errstate(over='ignore'):
        return squareform(pdist(xy)) if xy.shape[0] > 1 else np.zeros((xy.shape[0],) * 2)


def ks_for(n):
    """The k of the selection tests at n nodes: the ends, around n - 1 candidates, past them, and the row widths at which the
    permutation kernels change form."""
    ks = {1, 2, n - 2, n - 1, n, n + 5} | {k for k in (1022, 1023, 2047) if k <= n + 5}
    return sorted(k for k in ks if k >= 1)


def sorted_candidates(dmat, reached_only):
    """(S, cnt): row i of S starts with sorted(cand_i), cnt[i] = len(cand_i).  Entries that are no candidates become NaN, which
    np.sort puts behind everything, +inf included."""
    d = np.array(dmat, dtype=np.float64)
    n = d.shape[0]
    out = np.eye(n, dtype=bool)
    if reached_only:
        out |= ~np.isfinite(d)
    d[out] = np.nan
    return np.sort(d, axis=1), (n - out.sum(axis=1)).astype(np.int64)


def radii_from_sorted(sc, k):
    s, cnt = sc
    n = s.shape[0]
    pick = np.maximum(np.minimum(int(k), cnt) - 1, 0)
    return np.where(cnt > 0, s[np.arange(n), pick], 0.0)


def radii(dmat, k, reached_only):
    return radii_from_sorted(sorted_candidates(dmat, reached_only), k)


def membership(dmat, r, reached_only):
    d = np.asarray(dmat, dtype=np.float64)
    a = d <= np.asarray(r, dtype=np.float64)[:, None]
    if reached_only:
        a &= np.isfinite(d)
    return a.astype(np.int64)


def masked(dmat, a):
    """What a handle that keeps distances holds: D where A is 1, +inf elsewhere."""
    return np.where(np.asarray(a) != 0, dmat, np.inf)


def radii_brute(dmat, k, reached_only):
    """The rule again, one row at a time with Python's sorted()."""
    n = len(dmat)
    out = []
    for i in range(n):
        cand = [float(dmat[i][j]) for j in range(n) if j != i and not (reached_only and np.isinf(dmat[i][j]))]
        out.append(sorted(cand)[min(int(k), len(cand)) - 1] if cand else 0.0)
    return np.array(out, dtype=np.float64)


def component_graph(n, seed=0):
    """shortpath_ref.Graph of n nodes: two components (a path plus chords each), then isolated nodes (one at least from n = 3);
    weights are multiples of 1/16, so path sums are exact and many paths have equal lengths.  One edge per pair, every weight
    positive: SciPy's Dijkstra reads it as the library does."""
    import shortpath_ref as sp
    rng = np.random.default_rng([seed, n])
    iso = 0 if n < 3 else max(1, n // 16)
    m = n - iso
    eu, ev = [], []
    for lo, hi in ((0, (m + 1) // 2), ((m + 1) // 2, m)):
        size = hi - lo
        eu += list(range(lo, hi - 1))
        ev += list(range(lo + 1, hi))
        if size > 3:
            cu, cv = rng.integers(lo, hi, size=size // 2), rng.integers(lo, hi, size=size // 2)
            eu += cu[cu != cv].tolist()
            ev += cv[cu != cv].tolist()
    eu, ev = np.array(eu, dtype=np.int64), np.array(ev, dtype=np.int64)
    first = np.sort(np.unique(np.minimum(eu, ev) * n + np.maximum(eu, ev), return_index=True)[1]) if eu.size else []
    eu, ev = eu[first], ev[first]
    return sp._graph(n, eu, ev, rng.integers(1, 17, size=eu.shape[0]) / 16.0)
