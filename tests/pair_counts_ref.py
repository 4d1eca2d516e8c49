"""Reference for the enriched-pair counts behind attribute_unimodality_metric = 'radius' (safe_enriched_pair_counts[_dev],
SAFE.define_top_attributes) and the designed inputs of their tests.  NumPy / SciPy / networkx only: nothing here touches the
library.  Every comparison built on this module is exact integer or boolean equality.

Definition.  W is the within-reach relation: the membership define_neighborhoods would produce under the current metric with
the radius t = attribute_unimodality_radius_multiple x neighborhood_radius_resolved.  For a column a of nes_binary,
E_a = {i : nes_binary[i, a] > 0} (NaN, 0, -0.0 and negatives are not enriched; the reference's test at safe.py:641),
    e_a = |E_a|,   q_a = sum_{i in E_a} sum_{j in E_a} W[i, j]   (ordered pairs, the diagonal included),
    pairs_a = e_a (e_a - 1) / 2,   within_a = (q_a - e_a) / 2    (exact: W is symmetric with a full diagonal),
and the attribute fails iff within_a < attribute_unimodality_min_fraction * pairs_a in f64."""
import numpy as np
from scipy.spatial.distance import pdist, squareform

DEFAULT_MULTIPLE = 2.0
DEFAULT_MIN_FRACTION = 0.65
# what a column may hold: only 1, 2.5 and +inf are enriched
ODD_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 2.5, np.nan, np.inf, -np.inf])
ODD_ENRICHED = np.array([False, False, True, False, True, False, True, False])


def pair_counts(values, cols, w):
    """(q, e) int64 [len(cols)] of the columns `cols` of values [n, m] against the 0/1 matrix w [n, n] (any matrix: the raw
    quadratic form)."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    with np.errstate(invalid='ignore'):
        e_mat = np.asarray(values)[:, cols] > 0
    et = np.ascontiguousarray(e_mat.T).astype(np.int64)
    q = ((et @ np.asarray(w).astype(np.int64)) * et).sum(1)
    return q.astype(np.int64), et.sum(1).astype(np.int64)


def pairs_within(q, e):
    """(pairs, within) for a symmetric W with a full diagonal."""
    q, e = np.asarray(q, dtype=np.int64), np.asarray(e, dtype=np.int64)
    assert np.all((q - e) % 2 == 0) and np.all(q >= e)
    return e * (e - 1) // 2, (q - e) // 2


def fails(pairs, within, min_fraction=DEFAULT_MIN_FRACTION):
    return np.asarray(within).astype(np.float64) < float(min_fraction) * np.asarray(pairs).astype(np.float64)


def fraction(pairs, within):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.asarray(within).astype(np.float64) / np.asarray(pairs).astype(np.float64)


def table(values, cols, w, min_fraction=DEFAULT_MIN_FRACTION):
    """dict(pairs, within, fraction, fails) of the columns `cols`."""
    pairs, within = pairs_within(*pair_counts(values, cols, w))
    return dict(pairs=pairs, within=within, fraction=fraction(pairs, within), fails=fails(pairs, within, min_fraction))


# ---------------------------------------------------------------------------------------------- within-reach relations ----

def within_euclidean(xy, t):
    """safe.py:397-399 with t for the radius: squareform(pdist(xy)) < t (the diagonal, 0 < t, is kept)."""
    return (squareform(pdist(np.ascontiguousarray(xy, dtype=np.float64))) < t).astype(np.int64)


def within_shortpath(G, t, weight):
    """safe.py:406-417 with t for the cutoff: the pairs nx.all_pairs_dijkstra_path_length reaches (length <= t; the source
    itself at 0).  weight: 'length' for 'shortpath_weighted_layout', 'weight' (absent: hops) for 'shortpath'."""
    import networkx as nx
    n = G.number_of_nodes()
    w = np.zeros((n, n), dtype=np.int64)
    for s, row in nx.all_pairs_dijkstra_path_length(G, cutoff=t, weight=weight):
        w[s, list(row)] = 1
    return w


def x_range(xy):
    x = np.asarray(xy, dtype=np.float64)[:, 0]
    return np.max(x) - np.min(x)


# ------------------------------------------------------------------------------------------------------ designed inputs ----

def two_clusters(per=150, seed=5):
    """xy [2 per, 2]: two tight clusters (diameter < 0.05) whose centres are 1 apart in x, so that the x-range is ~1 and a
    neighborhood_radius of 0.03 gives 2 r ~ 0.06 > a cluster's diameter."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, size=2 * per)
    rad = 0.02 * np.sqrt(rng.uniform(size=2 * per))
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    xy[per:, 0] += 1.0
    return xy


CLUSTER_RADIUS = 0.03


def designed_attributes(per=150):
    """nes_binary [2 per, 3] and num_neighborhoods_enriched [3] of the three designed attributes:
    A: 12 nodes of cluster 1 -> every pair within reach: 66 / 66 = 1.0, kept;
    B: 12 nodes of each cluster -> 2 x 66 of 276 pairs: 132 / 276 < 0.65, dropped;
    C: 12 nodes of cluster 1 and one of cluster 2 -> 66 of 78 pairs: 66 / 78 >= 0.65, kept (two components: 'connectivity'
       drops it)."""
    nb = np.zeros((2 * per, 3))
    first = np.arange(3, 3 + 12 * 7, 7)                                   # 12 nodes of cluster 1
    second = per + np.arange(5, 5 + 12 * 11, 11)                          # 12 nodes of cluster 2
    assert first.max() < per and second.max() < 2 * per
    nb[first, 0] = 1
    nb[first, 1] = 1
    nb[second, 1] = 1
    nb[first, 2] = 1
    nb[second[0], 2] = 1
    return nb, (nb > 0).sum(0).astype(np.int64)


DESIGNED_PAIRS = np.array([66, 276, 78], dtype=np.int64)
DESIGNED_WITHIN = np.array([66, 132, 66], dtype=np.int64)
DESIGNED_FAILS = np.array([False, True, False])


def cluster_graph(xy, per=150, k=3):
    """A networkx graph on two_clusters' layout: inside each cluster every node is joined to its k nearest neighbours and the
    cluster's nodes are chained in index order (so a cluster is connected); no edge joins the clusters.  Edges carry 'length'
    = the Euclidean length."""
    import networkx as nx
    d = squareform(pdist(xy))
    G = nx.Graph()
    for i in range(xy.shape[0]):
        G.add_node(i, x=float(xy[i, 0]), y=float(xy[i, 1]), label='n%d' % i, label_orf='ORF%d' % i)
    for c0 in (0, per):
        block = d[c0:c0 + per, c0:c0 + per]
        for i in range(per):
            for j in np.argsort(block[i])[1:k + 1].tolist():
                G.add_edge(c0 + i, c0 + int(j), length=float(block[i, j]))
            if i + 1 < per:
                G.add_edge(c0 + i, c0 + i + 1, length=float(block[i, i + 1]))
    return G


def flow_graph(n=300, seed=11, lonely=12):
    """A networkx graph for the whole flows: n nodes with x, y in the unit square, three nearest neighbours joined among the
    first n - lonely nodes (edge 'length' = Euclidean), a separate path on the last `lonely` ones (unreached pairs)."""
    import networkx as nx
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    d = squareform(pdist(xy))
    G = nx.Graph()
    for i in range(n):
        G.add_node(i, x=float(xy[i, 0]), y=float(xy[i, 1]), label='n%d' % i, label_orf='ORF%d' % i)
    head = n - lonely
    for i in range(head):
        for j in np.argsort(d[i, :head])[1:4].tolist():
            G.add_edge(i, int(j), length=float(d[i, j]))
    for i in range(head, n - 1):
        G.add_edge(i, i + 1, length=float(d[i, i + 1]))
    return G, xy


def flow_attributes(xy, m=24, seed=12):
    """0/1 annotations [n, m] with spatial structure (so that neighborhoods come out enriched): column a marks the nodes near
    one or two random centres, plus a little noise."""
    rng = np.random.default_rng(seed)
    n = xy.shape[0]
    b = np.zeros((n, m))
    for a in range(m):
        for _ in range(1 + a % 2):
            c = rng.uniform(0.15, 0.85, size=2)
            b[np.hypot(xy[:, 0] - c[0], xy[:, 1] - c[1]) < rng.uniform(0.08, 0.16), a] = 1
        b[rng.uniform(size=n) < 0.01, a] = 1
    return b


# -------------------------------------------------------------------------------------------------- column patterns ----

def pattern_columns(n, seed=0):
    """(values [n, k], names): one column per pattern of the kernel tests."""
    rng = np.random.default_rng(seed)
    cols, names = [], []

    def add(name, v):
        names.append(name)
        cols.append(np.asarray(v, dtype=np.float64))
    add('empty', np.zeros(n))
    add('full', np.ones(n))
    one = np.zeros(n)
    one[n // 2] = 1
    add('one_node', one)
    last = np.zeros(n)
    last[n - 1] = 1
    add('last_row', last)
    b63 = np.zeros(n)
    b63[63::64] = 1
    add('bit63', b63)
    add('alternating', (np.arange(n) % 2).astype(np.float64))
    add('random_0.01', rng.uniform(size=n) < 0.01)
    add('random_0.5', rng.uniform(size=n) < 0.5)
    add('odd_values', ODD_VALUES[rng.integers(0, ODD_VALUES.size, size=n)])
    add('odd_values_cycle', ODD_VALUES[np.arange(n) % ODD_VALUES.size])
    return np.stack(cols, axis=1), names
