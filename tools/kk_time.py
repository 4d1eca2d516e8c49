"""Time of safe_io.kamada_kawai_layout (nx.kamada_kawai_layout, safepy/safe_io.py:288-308) on random geometric graphs of
mean degree ~20 (tools/layout_time.py's), one line per N.

  set-up s        all-pairs shortest paths on the device + invdist and its transpose (until the first evaluation starts)
  evaluations     cost-function calls SciPy's L-BFGS-B made
  ms/evaluation   host clock around safe_kk_eval (upload of the positions, two kernels, download), mean and minimum
  total s         the whole call
  networkx s      nx.kamada_kawai_layout on this host's CPU for the same graph (only N <= --nx-max: it takes minutes beyond)

usage: python tools/kk_time.py [--sizes 1000,3971,20000] [--nx-max 1000]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,3971,20000')
    ap.add_argument('--nx-max', type=int, default=1000)
    args = ap.parse_args()
    import scipy.sparse as sps
    import safepy_amd
    from layout_time import geometric_csr
    from safepy_amd import backend as be, safe_io
    be.Context.default(0)
    plain = be.KamadaKawai.evaluate
    for n in [int(s) for s in args.sizes.split(',')]:
        A = sps.triu(geometric_csr(n, 20, n), 1).tocoo()
        G = safepy_amd.LayoutGraph(np.zeros((n, 2)), A.row, A.col)
        spans = []

        def timed(self, pos):
            t = time.perf_counter()
            out = plain(self, pos)
            spans.append((t, time.perf_counter()))
            return out

        be.KamadaKawai.evaluate = timed
        try:
            t0 = time.perf_counter()
            safe_io.kamada_kawai_layout(G)
            total = time.perf_counter() - t0
        finally:
            be.KamadaKawai.evaluate = plain
        ms = np.array([1e3 * (b - a) for a, b in spans[1:]] or [np.nan])     # the first evaluation warms up
        line = 'N=%6d  edges=%7d  set-up s %.3f  evaluations %4d  ms/evaluation mean %.3f min %.3f  total s %.3f' % (
            n, A.nnz, spans[0][0] - t0, len(spans), float(ms.mean()), float(ms.min()), total)
        if n <= args.nx_max:
            import networkx as nx
            H = nx.Graph()
            H.add_nodes_from(range(n))
            H.add_edges_from(zip(A.row.tolist(), A.col.tolist()))
            t0 = time.perf_counter()
            want = nx.kamada_kawai_layout(H)
            line += '  networkx s %.2f  bit-equal %s' % (time.perf_counter() - t0,
                                                        all(np.array_equal(want[i], G.xy[i]) for i in range(n)))
        print(line, flush=True)


if __name__ == '__main__':
    main()
