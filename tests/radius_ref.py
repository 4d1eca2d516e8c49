"""References for the radius types of define_neighborhoods (neighborhood_radius_type 'absolute' / 'percentile') and for the
device selection behind them.  NumPy / SciPy / networkx only: nothing here touches the library.

The multiset v of a metric is the node distances of the unordered pairs i < j: scipy's pdist(xy) for 'euclidean', the finite
entries D[i, j], i < j, of the all-pairs shortest-path matrix otherwise (row i = the search from source i).  Every
comparison built on this module is on bits."""
import numpy as np
from scipy.spatial.distance import pdist

QS = (0, 0.1, 0.5, 1, 2.5, 10, 33.3, 50, 75, 99.9, 100)
KINDS = ('uniform', 'scaled_2m30', 'scaled_2p40', 'scaled_37p5', 'coincident', 'far_node', 'tiny')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def xy_input(kind, n, seed=0):
    """Coordinates [n, 2] of one input family of the selection tests."""
    rng = np.random.default_rng(1000 * seed + n)
    xy = rng.uniform(size=(n, 2))
    if kind == 'uniform':
        return xy
    if kind == 'scaled_2m30':
        return xy * 2.0 ** -30
    if kind == 'scaled_2p40':
        return xy * 2.0 ** 40
    if kind == 'scaled_37p5':
        return xy * 37.5
    if kind == 'coincident':                     # every distance is 0
        return np.tile(xy[:1], (n, 1))
    if kind == 'far_node':                       # a bin of the first digit that holds few keys, far from the others
        xy[n - 1] = (1e12, 0.5)
        return xy
    if kind == 'tiny':                           # squares underflow: subnormal and zero keys
        return xy * 1e-160
    if kind == 'lattice':                        # 8 x 8 integer lattice (n = 64): massive exact ties
        assert n == 64
        g = np.arange(8, dtype=np.float64)
        return np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(64, 2)
    raise ValueError(kind)


def sorted_pdist(xy):
    return np.sort(pdist(np.asarray(xy, dtype=np.float64)))


def finite_upper(dmat):
    """The finite entries above the diagonal of a distance matrix, ascending."""
    iu, ju = np.triu_indices(dmat.shape[0], 1)
    v = dmat[iu, ju]
    return np.sort(v[np.isfinite(v)])


def ranks_for(sv, every_below=0, extra=0, seed=0):
    """Ranks to ask of a sorted multiset: the ends and the middle, both sides of every boundary between distinct values
    (at most 64 boundaries, spread evenly, when there are more), every rank when there are at most `every_below` of them,
    `extra` random ones -- unsorted, with a repeat."""
    count = sv.shape[0]
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    if count <= every_below:
        return np.arange(count, dtype=np.int64)[::-1].copy()
    want = {0, min(1, count - 1), count // 2, max(count - 2, 0), count - 1}
    edges = np.nonzero(bits(sv)[1:] != bits(sv)[:-1])[0]              # sv[e] != sv[e + 1]
    if edges.size > 64:
        edges = edges[np.linspace(0, edges.size - 1, 64).astype(np.int64)]
    for e in edges.tolist():
        want.update((e, e + 1))
    rng = np.random.default_rng(seed)
    want.update(rng.integers(0, count, size=extra).tolist())
    out = np.array(sorted(want), dtype=np.int64)
    rng.shuffle(out)
    return np.concatenate([out, out[:1]])


def percentile_by_ranks(sv, q, ranks_fn, lerp_fn):
    """np.percentile(v, q) rebuilt from the product's rank function and interpolation on the sorted values."""
    k, k1, gamma = ranks_fn(sv.shape[0], q)
    return lerp_fn(sv[k], sv[k1], gamma)


def safe_graph(n=250, tail=10, seed=3):
    """A networkx graph of n nodes, ids 0..n-1, with x, y in the unit square: a random neighbour graph on the first n - tail
    nodes and a path on the last `tail` ones, with no edge between the two parts."""
    import networkx as nx
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    G = nx.Graph()
    for i in range(n):
        G.add_node(i, x=float(xy[i, 0]), y=float(xy[i, 1]), label='n%d' % i, label_orf='ORF%d' % i)
    head = n - tail
    d = np.sqrt(((xy[:head, None, :] - xy[None, :head, :]) ** 2).sum(axis=2))
    for i in range(head):
        for j in np.argsort(d[i])[1:4].tolist():                      # three nearest neighbours
            G.add_edge(i, int(j))
    for i in range(head, n - 1):
        G.add_edge(i, i + 1)
    return G, xy


def nx_all_pairs(G, weight, cutoff=None):
    """Dense f64 [n, n] of nx.all_pairs_dijkstra_path_length (inf where unreached), row s = the search from s."""
    import networkx as nx
    n = G.number_of_nodes()
    out = np.full((n, n), np.inf)
    for s, row in nx.all_pairs_dijkstra_path_length(G, weight=weight, cutoff=cutoff):
        for t, dist in row.items():
            out[s, t] = dist
    return out


def dense_of(node_distances, n):
    out = np.full((n, n), np.inf)
    for s, row in node_distances.items():
        for t, dist in row.items():
            out[s, t] = dist
    return out
