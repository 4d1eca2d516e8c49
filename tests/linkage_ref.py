"""NumPy restatement of scipy.cluster.hierarchy.linkage(d, method='average') (SciPy 1.15) for a condensed distance vector
d of n points: what safe_linkage_average (linkage.hip) computes, step for step.

SciPy runs _hierarchy.nn_chain on a copy of d, stable-sorts the merges by height and relabels them with a union-find:

  state    D = the distances, size[i] = 1, an empty chain.
  start    when the chain is empty it starts at the smallest i with size[i] > 0.
  scan     x = chain top.  With a chain predecessor p: y = p, cur = D[x, p]; without: cur = +inf.  Then i = 0 .. n - 1
           (live, i != x) replaces (y, cur) only when D[x, i] < cur, strictly: the result is p unless a live i is strictly
           closer, and then the smallest index that attains the row minimum.  y == p ends the chain, otherwise y is pushed.
  merge    pop both, order them x < y, record (x, y, cur); size[y] += size[x], x dies; for every live i != y
           D[i, y] = (nx * D[i, x] + ny * D[i, y]) / (nx + ny), every f64 operation rounded on its own.
  after    mergesort by height (equal heights keep merge order); row i then gets the current cluster ids of its two
           members, smaller first, the new cluster is n + i and column 3 its size.

The working matrix here is the square symmetric [n, n] form the kernel uses (a row is one contiguous scan); SciPy
updates the condensed copy in place, which is the same arithmetic.  tests/test_linkage_ref_cpu.py holds this file to
live SciPy on the bits of Z, so it documents the kernel and is not its reference: the GPU tests compare with SciPy."""
import numpy as np


def square_from_condensed(d, n):
    sq = np.zeros((n, n), dtype=np.float64)
    iu = np.triu_indices(n, 1)
    sq[iu] = d
    sq[(iu[1], iu[0])] = d
    return sq


def nn_chain_merges(d, n):
    """The unsorted merge list [(x, y, height)] of SciPy's nn_chain for method='average'."""
    D = square_from_condensed(np.asarray(d, dtype=np.float64), n)
    size = np.ones(n, dtype=np.int64)
    chain, merges = [], []
    for _ in range(n - 1):
        if not chain:
            chain = [int(np.flatnonzero(size > 0)[0])]
        while True:
            x = chain[-1]
            cand = np.where(size > 0, D[x], np.inf)
            cand[x] = np.inf
            i = int(np.argmin(cand))                           # the first index that attains the row minimum
            if len(chain) > 1:
                y, cur = chain[-2], D[x, chain[-2]]
                if cand[i] < cur:
                    y, cur = i, cand[i]
                if y == chain[-2]:
                    break
            else:
                y, cur = i, cand[i]
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        merges.append((x, y, float(cur)))
        size[x], size[y] = 0, nx + ny
        live = size > 0
        live[y] = False
        new = (np.float64(nx) * D[x, live] + np.float64(ny) * D[y, live]) / np.float64(nx + ny)
        D[y, live] = new
        D[live, y] = new
    return merges


def label_merges(merges, n):
    """Stable sort by height and union-find relabel: the linkage matrix Z f64 [n - 1, 4]."""
    order = sorted(range(n - 1), key=lambda k: merges[k][2])                 # sorted() is stable, like mergesort
    parent = list(range(2 * n - 1))
    size = [1] * (2 * n - 1)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            x, parent[x] = parent[x], root
        return root

    z = np.empty((n - 1, 4), dtype=np.float64)
    for i, k in enumerate(order):
        a, b = find(merges[k][0]), find(merges[k][1])
        parent[a] = parent[b] = n + i
        size[n + i] = size[a] + size[b]
        z[i] = (min(a, b), max(a, b), merges[k][2], size[n + i])
    return z


def linkage_average(d, n=None):
    d = np.asarray(d, dtype=np.float64)
    if n is None:
        n = int(round((1 + np.sqrt(1 + 8 * d.shape[0])) / 2))
    assert n * (n - 1) // 2 == d.shape[0]
    return label_merges(nn_chain_merges(d, n), n)
