"""Designed graphs and references for the bounded all-pairs shortest-path kernel (k_shortpath, K2 in DESIGN.md), shared by
tests/test_shortpath_ref_cpu.py and tests/test_gpu_shortpath.py.  Written from the definition of the operation -- networkx's
bounded Dijkstra as oracle/safe_oracle.py restates it -- not from nbr.hip.

The kernel launches W = min(n, 8 * num_cu) one-wave workers; worker k serves the sources k, k + W, k + 2 W, ... in turn on
the same private scratch, which it puts back by hand after each search.  rung_graph() is built so that a wrong clean-up
shows: the sources one worker serves are neighbours.

Two references:
  oracle_reference   oracle.safe_oracle.neighborhoods_shortpath, any graph.
  scipy_reference    scipy.sparse.csgraph.dijkstra(directed=False, limit=cutoff): much faster, but csr_matrix sums the
                     entries of a repeated pair and csgraph reads a stored zero as "no edge", so it is allowed only where
                     scipy_allowed() says so: every weight strictly positive, no pair of nodes with two edges.  Both are
                     Dijkstra: both give the minimum over paths of the f64 sum taken edge by edge from the source, so on
                     such graphs they agree on the bits (test_shortpath_ref_cpu.py holds them to that)."""
import collections

import numpy as np

from oracle import safe_oracle as orc

Graph = collections.namedtuple('Graph', 'n eu ev ew')

RUNG_REMAINDER = {1: 61, 2: 3}          # rung_graph(W, k).n = k * W + RUNG_REMAINDER[k]
STAR_LEAVES = (63, 64, 65, 128, 129, 300)   # frontier sizes around the 64 lanes a worker relaxes a frontier with


def _graph(n, eu, ev, ew):
    return Graph(int(n), np.asarray(eu, dtype=np.int32), np.asarray(ev, dtype=np.int32), np.asarray(ew, dtype=np.float64))


def _weights(rng, kind, count):
    if kind == 'dyadic':                                    # k / 16: every path sum is exact, many paths tie
        return rng.integers(1, 17, size=count) / 16.0
    if kind == 'real':                                      # path sums round, differently along different paths
        return rng.uniform(0.01, 1.0, size=count)
    assert kind == 'ones', kind
    return np.ones(count)


def bits(a):
    """The f64 bit patterns: equality on them tells -0.0 from 0.0."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ builders ----

def rung_graph(W, k, weights='dyadic', seed=0):
    """n = k * W + RUNG_REMAINDER[k] nodes: the ring (i, i + 1 mod n), a rung (i, i + W) for every i < n - W, and n / 2
    random chords; one edge per pair (ring and rungs are kept, a chord that repeats a pair is dropped).  With W workers,
    the sources i and i + W of one worker are adjacent."""
    n = k * W + RUNG_REMAINDER[k]
    assert W >= 2 and n >= 3
    rng = np.random.default_rng([seed, W, k])
    i = np.arange(n)
    cu, cv = rng.integers(0, n, size=n // 2), rng.integers(0, n, size=n // 2)
    eu = np.concatenate([i, i[:n - W], cu[cu != cv]])
    ev = np.concatenate([(i + 1) % n, i[:n - W] + W, cv[cu != cv]])
    lo, hi = np.minimum(eu, ev), np.maximum(eu, ev)
    first = np.sort(np.unique(lo * n + hi, return_index=True)[1])
    eu, ev = eu[first], ev[first]
    return _graph(n, eu, ev, _weights(rng, weights, eu.shape[0]))


def star_graph(L, chords=5, seed=0):
    """K(1, L): hub 0, leaves 1..L, plus `chords` leaf-to-leaf edges; dyadic weights.  The hub's first frontier has L
    entries, a leaf's second one L - 1."""
    rng = np.random.default_rng([seed, L])
    eu, ev = [0] * L, list(range(1, L + 1))
    seen = set()
    while len(seen) < chords:
        a, b = sorted(int(x) for x in rng.integers(1, L + 1, size=2))
        if a != b and (a, b) not in seen:
            seen.add((a, b))
            eu.append(a)
            ev.append(b)
    return _graph(L + 1, eu, ev, _weights(rng, 'dyadic', len(eu)))


def bipartite_graph(a=70, b=70, seed=0):
    """Complete bipartite K(a, b), dyadic weights: every frontier is a whole side, and most nodes are relabelled."""
    rng = np.random.default_rng([seed, a, b])
    eu, ev = np.divmod(np.arange(a * b), b)
    return _graph(a + b, eu, ev + a, _weights(rng, 'dyadic', a * b))


def path_graph(n=1500, seed=0):
    """0 - 1 - ... - (n - 1) with weights integers(1, 17) / 16: a search from i runs max(i, n - 1 - i) rounds."""
    rng = np.random.default_rng([seed, n])
    return _graph(n, np.arange(n - 1), np.arange(1, n), _weights(rng, 'dyadic', n - 1))


def path_closed_form(g):
    """|P[i] - P[j]| of the prefix sums P: all of them are multiples of 1/16 far below 2^53 / 16, so nothing rounds."""
    p = np.concatenate([[0.0], np.cumsum(g.ew)])
    return np.abs(p[:, None] - p[None, :])


def skip_graph(n=513):
    """Edges (i, i + 2^j) for every j with i + 2^j < n, weight 2^j / 16 + j / 64.  The coarse hop labels a node first (fewer
    rounds), the finer paths -- shorter by j / 64 and more -- improve the label later, several times over."""
    eu, ev, ew = [], [], []
    j = 0
    while (1 << j) < n:
        i = np.arange(n - (1 << j))
        eu.append(i)
        ev.append(i + (1 << j))
        ew.append(np.full(i.shape[0], (1 << j) / 16.0 + j / 64.0))
        j += 1
    return _graph(n, np.concatenate(eu), np.concatenate(ev), np.concatenate(ew))


def skip_closed_form(n):
    """Every hop costs at least its span / 16, and the unit hops cost exactly that: D[i][j] = |i - j| / 16."""
    i = np.arange(n, dtype=np.float64)
    return np.abs(i[:, None] - i[None, :]) / 16.0


def star_closed_form(g):
    """Of a star WITHOUT chords: the spoke, or the sum of two spokes (dyadic: exact in either order)."""
    w = np.concatenate([[0.0], g.ew])
    d = w[:, None] + w[None, :]
    d[np.diag_indices(g.n)] = 0.0
    return d


def rounding_path():
    """A 12-node path whose weights are multiples of 0.1 (the sums round, and differently from the two ends), with two
    chords that are never shorter.  ROUNDING_CUTOFF is the sum from node 0 to node 3, taken as Dijkstra takes it."""
    ew = [0.1, 0.2, 0.3, 0.7, 0.1, 0.1, 0.1, 0.4, 0.3, 0.6, 0.9, 5.0, 5.0]
    return _graph(12, list(range(11)) + [0, 2], list(range(1, 12)) + [6, 11], ew)


ROUNDING_CUTOFF = (0.1 + 0.2) + 0.3                         # 0.6000000000000001; from node 3 the sum is 0.6


def zero_mix():
    """Zero-weight edges (a zero cycle 0-1-2-0, a zero chain 5-6-7 hanging off a positive edge) among positive ones."""
    eu = [0, 1, 2, 2, 3, 4, 5, 6, 7, 8]
    ev = [1, 2, 0, 3, 4, 5, 6, 7, 8, 0]
    ew = [0.0, 0.0, 0.0, 0.25, 0.5, 0.125, 0.0, 0.0, 0.75, 1.0]
    return _graph(10, eu, ev, ew)


def zero_components():
    """Three components whose every edge weighs 0.0 -- a 7-cycle with chords, a complete K5, a pair -- and one isolated
    node: every distance inside a component is 0.0."""
    eu = [0, 1, 2, 3, 4, 5, 6, 0, 1]
    ev = [1, 2, 3, 4, 5, 6, 0, 3, 5]
    for a in range(7, 12):
        for b in range(a + 1, 12):
            eu.append(a)
            ev.append(b)
    eu += [12]
    ev += [13]
    return _graph(15, eu, ev, np.zeros(len(eu)))


def negative_zero():
    """-0.0 weights beside 0.0 and positive ones: 0.0 + -0.0 is 0.0, so no distance is -0.0."""
    eu = [0, 1, 2, 3, 0]
    ev = [1, 2, 3, 4, 4]
    return _graph(6, eu, ev, [-0.0, -0.0, 0.0, 0.5, -0.0])


def subnormal():
    """Weights that are small multiples of the smallest subnormal, 5e-324 (their sums are exact), beside one normal edge."""
    tiny = np.float64(5e-324)
    eu = [0, 1, 2, 3, 4, 0, 5]
    ev = [1, 2, 3, 4, 5, 5, 6]
    return _graph(7, eu, ev, [tiny * 1, tiny * 3, tiny * 2, tiny * 7, tiny * 1, tiny * 20, 1.0])


SUBNORMAL_CUTOFF = float(np.float64(5e-324) * 6)           # 0-1-2-3 is exactly this long; 0-1-2-3-4 is longer


def loops_and_isolated():
    """Self loops (also on the only node of a component, also of weight 0), isolated nodes (first, last and in between)."""
    eu = [1, 1, 2, 3, 3, 5, 7, 7]
    ev = [1, 2, 3, 3, 4, 5, 7, 8]
    ew = [0.5, 1.0, 2.0, 0.0, 1.5, 0.25, 3.0, 0.5]
    return _graph(10, eu, ev, ew)


def single_node(loop=False):
    return _graph(1, [0] if loop else [], [0] if loop else [], [2.0] if loop else [])


def two_nodes(edge=True):
    return _graph(2, [0] if edge else [], [1] if edge else [], [0.75] if edge else [])


def no_edges(n=9):
    return _graph(n, [], [], [])


def parallel_edges():
    """Two edges between one pair with different weights, the lighter one first (0-1), last (1-2) and given in the other
    direction (2-3): the C entry point and the oracle's adjacency lists keep both, so the lighter one counts."""
    eu = [0, 0, 1, 1, 2, 3, 3]
    ev = [1, 1, 2, 2, 3, 2, 4]
    ew = [0.25, 1.0, 2.0, 0.5, 4.0, 0.125, 1.0]
    return _graph(5, eu, ev, ew)


# name -> (graph, cutoffs): the small graphs around the comparison cand > cutoff
def edge_cases():
    inf = np.inf
    return {
        'rounding_path': (rounding_path(), [ROUNDING_CUTOFF, float(np.nextafter(ROUNDING_CUTOFF, 0)), 0.6, inf]),
        'zero_mix': (zero_mix(), [0.0, -1.0, 0.125, 0.25, inf]),
        'zero_components': (zero_components(), [0.0, -1.0, 1.0, inf]),
        'negative_zero': (negative_zero(), [0.0, -1.0, 0.5, inf]),
        'subnormal': (subnormal(), [0.0, SUBNORMAL_CUTOFF, float(np.nextafter(SUBNORMAL_CUTOFF, 0)), 1.0, inf]),
        'loops_and_isolated': (loops_and_isolated(), [0.0, -1.0, 1.0, 3.0, inf]),
        'single_node': (single_node(), [0.0, -1.0, inf]),
        'single_node_loop': (single_node(loop=True), [0.0, -1.0, 2.0, inf]),
        'two_nodes': (two_nodes(), [0.0, -1.0, 0.75, float(np.nextafter(0.75, 0)), inf]),
        'two_nodes_apart': (two_nodes(edge=False), [0.0, inf]),
        'no_edges': (no_edges(), [0.0, -1.0, 1.0, inf]),
        'parallel_edges': (parallel_edges(), [0.25, 0.75, 0.875, inf]),
    }


# ---------------------------------------------------------------------------------------- references ----

def oracle_reference(g, cutoff):
    """(A int64 [n, n], D f64 [n, n] with +inf where unreached)."""
    return orc.neighborhoods_shortpath(g.n, g.eu, g.ev, g.ew, cutoff)


def scipy_allowed(g):
    lo, hi = np.minimum(g.eu, g.ev).astype(np.int64), np.maximum(g.eu, g.ev).astype(np.int64)
    return bool((g.ew > 0).all()) and np.unique(lo * g.n + hi).shape[0] == g.eu.shape[0]


def scipy_reference(g, cutoff):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    assert scipy_allowed(g), 'csgraph would sum parallel edges or drop zero-weight ones'
    assert cutoff >= 0, 'csgraph takes no negative limit'
    m = csr_matrix((g.ew, (g.eu, g.ev)), shape=(g.n, g.n))
    d = dijkstra(m, directed=False, limit=cutoff)
    return np.isfinite(d).astype(np.int64), d


def forms(a):
    """What a handle reports about the membership A: row counts, CSR (columns ascending in a row), nnz, widest row."""
    a = np.asarray(a)
    counts = a.sum(axis=1).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    col = np.nonzero(a)[1].astype(np.int32)
    return {'row_counts': counts, 'row_ptr': row_ptr, 'col': col, 'nnz': int(counts.sum()),
            'max_row_count': int(counts.max()) if counts.size else 0}
