"""NumPy restatement of safe_nbr_diffusion's contract (include/safe_hip.h), with the order of every sum explicit: no `@`, no BLAS,
one vectorised pass per entry slot of the CSR rows, so that every element sees exactly the operations the contract lists, in its
order.  `dtype` = np.float64 gives the bytes the device must give; np.longdouble gives a more precise run of the same operations
(tests/test_diffusion_ref_cpu.py measures the rounding of the f64 run against it).

  csr(n, eu, ev, w)                       (ptr, col, weight): one entry per direction, a self-loop once, duplicates kept; a row's
                                          entries by (neighbor id, input order)
  scaled(ptr, col, weight)                (r, s): d_i added in entry order, r_i = 1 / sqrt(d_i) (0 where d_i == 0), s = (w r_i) r_k
  kernel(n, eu, ev, w, restart, steps)    K = X_steps
  distance(K)                             D from the upper triangle of K
  members(D, cutoff) / kept(D, cutoff)    the membership (int64) and the matrix the handle keeps
  hops(n, eu, ev)                         unweighted hop distances (breadth-first), +inf where unreached
"""
import numpy as np


def csr(n, eu, ev, w=None):
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    w = np.ones(len(eu), dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64)
    rows, cols, wts, seq = [], [], [], []
    for e, (u, v) in enumerate(zip(eu.tolist(), ev.tolist())):
        rows.append(u), cols.append(v), wts.append(w[e]), seq.append(e)
        if u != v:
            rows.append(v), cols.append(u), wts.append(w[e]), seq.append(e)
    rows, cols, seq = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(seq, dtype=np.int64)
    wts = np.asarray(wts, dtype=np.float64)
    order = np.lexsort((seq, cols, rows))                     # by row, then neighbor id, then input order
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return ptr, cols[order], wts[order]


def _slots(ptr):
    """For slot = 0, 1, ...: (the rows that have an entry in that slot, the entries' positions)."""
    deg = np.diff(ptr)
    for slot in range(int(deg.max()) if len(deg) else 0):
        rows = np.nonzero(deg > slot)[0]
        yield rows, ptr[rows] + slot


def scaled(ptr, col, weight, dtype=np.float64):
    n = len(ptr) - 1
    weight = np.asarray(weight, dtype=dtype)
    d = np.zeros(n, dtype=dtype)
    for rows, e in _slots(ptr):
        d[rows] = d[rows] + weight[e]
    with np.errstate(divide='ignore'):
        r = np.where(d == 0, dtype(0), dtype(1) / np.sqrt(d))
    row_of = np.repeat(np.arange(n), np.diff(ptr))
    s = (weight * r[row_of]) * r[col]
    return r, s


def kernel(n, eu, ev, w, restart, steps, dtype=np.float64):
    ptr, col, weight = csr(n, eu, ev, w)
    _, s = scaled(ptr, col, weight, dtype)
    alpha = dtype(restart)
    beta = dtype(1) - alpha
    x = np.eye(n, dtype=dtype)
    diag = np.arange(n)
    for _ in range(int(steps)):
        acc = np.zeros((n, n), dtype=dtype)
        for rows, e in _slots(ptr):
            acc[rows] = acc[rows] + s[e][:, None] * x[col[e]]
        y = beta * acc
        y[diag, diag] = alpha + y[diag, diag]
        x = y
    return x


def distance(k):
    n = k.shape[0]
    a, b = np.triu_indices(n, 1)
    kab, diag = k[a, b], k.diagonal()
    with np.errstate(invalid='ignore', divide='ignore'):
        d = 1.0 - kab / np.sqrt(diag[a] * diag[b])
    d = np.where(d < 0, 0.0, d)
    d = np.where(kab == 0, np.inf, d)
    out = np.zeros((n, n), dtype=k.dtype)
    out[a, b] = d
    out[b, a] = d
    return out


def members(d, cutoff):
    a = (d <= cutoff) & np.isfinite(d)
    np.fill_diagonal(a, True)
    return a.astype(np.int64)


def kept(d, cutoff):
    return np.where(members(d, cutoff) == 1, d, np.inf)


def hops(n, eu, ev):
    adj = [[] for _ in range(n)]
    for u, v in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist()):
        adj[u].append(v)
        adj[v].append(u)
    out = np.full((n, n), np.inf)
    for src in range(n):
        out[src, src] = 0
        frontier, depth = [src], 0
        while frontier:
            depth += 1
            nxt = []
            for u in frontier:
                for v in adj[u]:
                    if out[src, v] == np.inf:
                        out[src, v] = depth
                        nxt.append(v)
            frontier = nxt
    return out


# ------------------------------------------------------------------------------------------------ graphs of the tests ----

def path_graph(n):
    i = np.arange(n - 1)
    return i, i + 1


def star_graph(n):
    """Hub 0 with n - 1 leaves."""
    leaves = np.arange(1, n)
    return np.zeros(n - 1, dtype=np.int64), leaves


def ring_lattice(n, reach=2):
    i = np.arange(n)
    return np.concatenate([i] * reach), np.concatenate([(i + k) % n for k in range(1, reach + 1)])


def grid_graph(rows, cols):
    idx = np.arange(rows * cols).reshape(rows, cols)
    eu = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    ev = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return eu, ev


def random_sparse(n, mean_degree, seed, weighted=True):
    """A ring (so that the graph is connected) plus random chords; non-dyadic weights."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    extra = max(0, int(n * (mean_degree - 2) / 2))
    eu = np.concatenate([i, rng.integers(0, n, size=extra)])
    ev = np.concatenate([(i + 1) % n, rng.integers(0, n, size=extra)])
    if n == 1:
        eu, ev = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    w = rng.uniform(0.1, 3.0, size=len(eu)) if weighted else None
    return eu, ev, w


def awkward_graph(n, seed):
    """Two components plus an isolated last node; self-loops, duplicate edges (in both orientations), a zero-weight edge,
    non-dyadic weights.  n >= 8."""
    rng = np.random.default_rng(seed)
    half = (n - 1) // 2
    a, b = np.arange(half), np.arange(half, n - 1)
    eu = [a[:-1], b[:-1], rng.integers(0, half, size=half), rng.integers(half, n - 1, size=len(b))]
    ev = [a[1:], b[1:], rng.integers(0, half, size=half), rng.integers(half, n - 1, size=len(b))]
    eu, ev = np.concatenate(eu), np.concatenate(ev)
    eu = np.concatenate([eu, [0, 1, 2, 2, half, 3]])          # duplicate 0-1 both ways, self-loops at 2 (twice) and half, 3-4 at weight 0
    ev = np.concatenate([ev, [1, 0, 2, 2, half, 4]])
    w = rng.uniform(0.1, 3.0, size=len(eu))
    w[-1] = 0.0
    return eu, ev, w
