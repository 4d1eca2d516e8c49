"""NumPy restatement of networkx 3.4.2's Kamada-Kawai cost function (drawing/layout.py: _kamada_kawai_costfn, dim = 2) with
every sum written out in the order NumPy takes it, and the graphs the Kamada-Kawai tests share.  Written from networkx's
definition, not from kk.hip.  For positions pos [n, 2] and invdist = 1 / (dist_mtx + eye * 1e-3):

  dx, dy   pos_i - pos_j for all pairs
  sep      sqrt(dx*dx + dy*dy)                      np.linalg.norm(delta, axis=-1)
  inv      1 / (sep + eye * 1e-3)
  dir      (dx, dy) * inv                           a product, not a quotient by sep
  off      sep * invdist - 1, 0 on the diagonal
  t        (invdist * off) * dir                    einsum multiplies its operands left to right
  g[i]     ((0 + t[i, 0]) + t[i, 1]) + ...          einsum "ij,ij,ijk->ik": strictly sequential in j
  h[j]     ((0 + t[0, j]) + t[1, j]) + ...          einsum "ij,ij,ijk->jk": strictly sequential in i
  grad     (g - h) + 1e-3 * sumpos                  sumpos = np.sum(pos, axis=0)
  cost     0.5 * S + (0.5 * 1e-3) * np.sum(sumpos**2)
  S        np.sum(off**2): the row-major flat array in buffers of 8192 elements (they cross row ends), each summed by
           numpy's pairwise routine -- np.add.reduce of the slice, numpy being the reference for that order -- and the
           buffer sums added in order from 0

tests/test_kk_ref_cpu.py holds kk_costfn_ref to the real function on the bits of cost and gradient, so the GPU tests
(tests/test_gpu_kk.py) can compare the device against it at sizes and positions live networkx is slow for."""
import functools

import numpy as np

BUF = 8192                  # elements NumPy reduces at a time
EPS = 1e-3                  # eye * 1e-3, and networkx's meanweight
UNREACHED = 1e6             # dist_mtx where a node is not reached

# sizes of the cost-function tests: around numpy's 8-element and 128-element pairwise thresholds, N^2 on both sides of
# 8192 (90, 91), exactly two buffers (128), N^2 on both sides of 4 * 8192 (181, 182), several buffers with a ragged tail
SIZES = (1, 2, 3, 7, 8, 9, 90, 91, 128, 129, 130, 181, 182, 300, 513)
WEIGHTS = (0.1, 0.3, 1.7)   # non-dyadic: path sums round, and differently along different paths


def invdist_of(dist_mtx):
    """_kamada_kawai_solve's costargs[1]."""
    with np.errstate(divide='ignore'):
        return 1 / (dist_mtx + np.eye(dist_mtx.shape[0]) * EPS)


def kk_costfn_ref(pos_vec, invdist):
    """(cost, grad [2n]) = _kamada_kawai_costfn(pos_vec, np, invdist, 1e-3, 2), bit for bit."""
    n = invdist.shape[0]
    pos = np.asarray(pos_vec, dtype=np.float64).reshape(n, 2)
    with np.errstate(all='ignore'):
        dx = pos[:, None, 0] - pos[None, :, 0]
        dy = pos[:, None, 1] - pos[None, :, 1]
        sep = np.sqrt(dx * dx + dy * dy)
        inv = 1 / (sep + np.eye(n) * EPS)
        off = sep * invdist - 1.0
        off[np.diag_indices(n)] = 0
        c = invdist * off
        grad = np.empty((n, 2))
        for k, d in enumerate((dx, dy)):
            t = c * (d * inv)
            g = np.zeros(n)
            for j in range(n):                  # row i's chain over j, all rows at once
                g = g + t[:, j]
            h = np.zeros(n)
            for i in range(n):                  # column j's chain over i, all columns at once
                h = h + t[i, :]
            grad[:, k] = g - h
        flat = (off * off).ravel()
        s = 0.0
        for k in range(0, flat.size, BUF):
            s = s + np.add.reduce(flat[k:k + BUF])
        sumpos = np.sum(pos, axis=0)
        cost = 0.5 * s
        cost = cost + 0.5 * EPS * np.sum(sumpos ** 2)
        grad = grad + EPS * sumpos
    return cost, grad.ravel()


def sparse_edges(n, seed, weighted=False):
    """(edge_u, edge_v, edge_w or None) of a G(n, 4/n) graph whose last node (two nodes from n = 8) has no edge, so that
    dist_mtx holds 1e6 entries; weighted: weights drawn from WEIGHTS."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 4.0 / max(n, 1)
    cut = n - (2 if n >= 8 else 1)
    keep &= (iu < cut) & (ju < cut)
    eu, ev = iu[keep].astype(np.int64), ju[keep].astype(np.int64)
    ew = np.asarray(WEIGHTS)[rng.integers(0, len(WEIGHTS), size=eu.size)] if weighted else None
    return eu, ev, ew


def nx_graph(n, eu, ev, ew=None):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    if ew is None:
        G.add_edges_from(zip(eu.tolist(), ev.tolist()))
    else:
        G.add_weighted_edges_from(zip(eu.tolist(), ev.tolist(), ew.tolist()))
    return G


def nx_dist_mtx(G):
    """kamada_kawai_layout's dist_mtx: all-pairs Dijkstra lengths, 1e6 where unreached."""
    import networkx as nx
    nodes = list(G)
    dist = dict(nx.shortest_path_length(G, weight='weight'))
    m = UNREACHED * np.ones((len(nodes), len(nodes)))
    for r, a in enumerate(nodes):
        for c, b in enumerate(nodes):
            if b in dist[a]:
                m[r][c] = dist[a][b]
    return m


def positions(n, kind, seed=0):
    """Test positions [n, 2]: 'random' in [-1, 1]^2, or 'circle' (nx.circular_layout's start)."""
    if kind == 'random':
        return np.random.default_rng(seed).uniform(-1, 1, size=(n, 2))
    import networkx as nx
    pos = nx.circular_layout(range(n))
    return np.array([pos[i] for i in range(n)], dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    """Bit equality of two f64 arrays, except that a NaN matches any NaN (payloads are not compared)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))
