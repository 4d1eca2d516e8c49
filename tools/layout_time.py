"""Time per spring-embedded layout on the device (safe_layout_spring: nx.spring_layout(k=0.2, iterations=100),
safepy/safe_io.py:288-308) on random geometric graphs of mean degree ~20, one line per N.

  device ms   HIP events on the context stream around the call (uploads, 100 launches, download)
  call ms     host clock around the whole call (adds the host-side CSR / neighbour-list build)
  networkx s  nx.spring_layout on this host's CPU for the same graph and seed (only N <= --nx-max)

usage: python tools/layout_time.py [--sizes 1000,3971,20000] [--repeats 3] [--nx-max 2000]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def geometric_csr(n, degree, seed):
    """CSR of a random geometric graph (grid-bucketed, O(N * degree)): both directions, sorted columns."""
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    r = np.sqrt(degree / (np.pi * n))
    cells = max(1, int(1 / r))
    cell = np.minimum((xy * cells).astype(np.int64), cells - 1)
    key = cell[:, 0] * cells + cell[:, 1]
    order = np.argsort(key, kind='stable')
    start = np.searchsorted(key[order], np.arange(cells * cells + 1))
    rows, cols = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            cx, cy = cell[:, 0] + dx, cell[:, 1] + dy
            ok = (cx >= 0) & (cx < cells) & (cy >= 0) & (cy < cells)
            for i in np.flatnonzero(ok):
                k = cx[i] * cells + cy[i]
                js = order[start[k]:start[k + 1]]
                js = js[(js != i) & (((xy[js] - xy[i]) ** 2).sum(1) < r * r)]
                rows.append(np.full(js.size, i))
                cols.append(js)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sps.csr_array((np.ones(rows.size), (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,3971,20000')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--nx-max', type=int, default=2000)
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    for n in [int(s) for s in args.sizes.split(',')]:
        A = geometric_csr(n, 20, n)
        pos0 = np.random.RandomState(n).rand(n, 2)
        dtype = np.float32 if n >= 500 else np.float64
        dev, call = [], []
        for rep in range(args.repeats + 1):                 # the first call warms up
            t0 = time.perf_counter()
            ctx.timer_start()
            pos, ran = ctx.layout_spring(A.indptr, A.indices, A.data, pos0, 0.2, 100, 1e-4, dtype)
            ms = ctx.timer_stop_ms()
            if rep:
                dev.append(ms)
                call.append(1e3 * (time.perf_counter() - t0))
        line = 'N=%6d  edges=%7d  iterations=%3d  device ms min %.2f median %.2f  call ms median %.2f' % (
            n, A.nnz // 2, ran, min(dev), float(np.median(dev)), float(np.median(call)))
        if n <= args.nx_max:
            import networkx as nx
            G = nx.from_scipy_sparse_array(A)
            t0 = time.perf_counter()
            nx.spring_layout(G, k=0.2, iterations=100, seed=np.random.RandomState(n))
            line += '  networkx s %.2f' % (time.perf_counter() - t0)
        print(line, flush=True)


if __name__ == '__main__':
    main()
