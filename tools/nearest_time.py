"""Time of neighborhood_radius_type = 'nearest' (SAFE.define_neighborhoods): the per-row selection kernel of nbr.hip (K3b), the
per-row membership build, and the whole call, beside the same call under 'diameter' and the host route.  Every figure is the
median of --passes passes after one warm-up pass, all in one process.

  euclidean, clustered layouts (workloads.clustered_layout), one line per N and k:
    select ms     safe_row_distance_select_xy between the context's timer events (upload, the one launch, read-back, n roots)
    build ms      safe_nbr_euclidean_rows, likewise (upload, bit matrix, CSR / SELL forms)
    define ms     SAFE.define_neighborhoods(neighborhood_radius_type='nearest'), host clock
    diameter ms   the same call with neighborhood_radius_type='diameter', neighborhood_radius=0.1
    host s        np.partition over squareform(pdist(xy)) on this host's CPU (only N <= --host-max), and whether its radii
                  agree with the device's on the bits
  shortpath_weighted_layout on workloads.costanzo_surrogate (N = 3971), one line per k:
    unbounded s   the all-pairs search with cutoff = +inf that keeps the distances on the device (the same for every k)
    select ms     safe_nbr_row_distance_select on that handle
    build ms      safe_nbr_from_distances_rows with keep_distances
    define s / diameter s   the whole calls

usage: python tools/nearest_time.py [--sizes 3971,20000] [--ks 50,500] [--passes 5] [--host-max 20000]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_of(passes, fn):
    """(median of `passes` timed runs of fn after one untimed run, the last result); fn returns (seconds or ms, result)."""
    fn()
    runs = [fn() for _ in range(passes)]
    return float(np.median([t for t, _ in runs])), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='3971,20000')
    ap.add_argument('--ks', default='50,500')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--host-max', type=int, default=20000)
    args = ap.parse_args()
    from scipy.spatial.distance import pdist, squareform
    import safepy_amd
    from safepy_amd import backend as be, workloads
    ctx = be.Context.default(0)
    ks = [int(s) for s in args.ks.split(',')]

    def device_ms(call):
        def once():
            ctx.timer_start()
            out = call()
            return ctx.timer_stop_ms(), out
        return once

    def host_clock(call, scale=1.0):
        def once():
            t0 = time.perf_counter()
            out = call()
            return scale * (time.perf_counter() - t0), out
        return once

    def closing(build):
        def call():
            nbr = build()
            stats = (nbr.nnz / nbr.n, nbr.max_row_count)
            nbr.close()
            return stats
        return call

    def define(graph, metric, kind, radius):
        sf = safepy_amd.SAFE(verbose=False)
        sf.graph = graph

        def call():
            sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type=kind, neighborhood_radius=radius)
            return sf._nbr.nnz / sf._nbr.n, sf._nbr.max_row_count
        return call

    for n in [int(s) for s in args.sizes.split(',')]:
        xy = workloads.clustered_layout(np.random.default_rng(n), n)
        graph = safepy_amd.LayoutGraph(xy)
        diameter_ms, (dia_mean, dia_max) = median_of(args.passes, host_clock(define(graph, 'euclidean', 'diameter', 0.1), 1e3))
        dmat = squareform(pdist(xy)) if n <= args.host_max else None
        for k in ks:
            select_ms, radii = median_of(args.passes, device_ms(lambda: ctx.row_distance_select(xy, k)))
            build_ms, (mean, widest) = median_of(args.passes, device_ms(closing(lambda: be.Neighborhoods.euclidean_rows(ctx, xy, radii))))
            define_ms, _ = median_of(args.passes, host_clock(define(graph, 'euclidean', 'nearest', k), 1e3))
            line = ('euclidean  N=%6d  k=%4d  select ms %.3f  build ms %.3f  define ms %.3f  diameter ms %.3f  neighbors per node '
                    '%.1f (max %d; diameter 0.1: %.1f, max %d)' % (n, k, select_ms, build_ms, define_ms, diameter_ms, mean, widest,
                                                                  dia_mean, dia_max))
            if dmat is not None:
                def host():
                    d = dmat.copy()
                    np.fill_diagonal(d, np.inf)                          # node i is no candidate of its own row
                    kk = min(k, n - 1) - 1
                    return np.partition(d, kk, axis=1)[:, kk]
                host_s, want = median_of(1, host_clock(host))
                line += '  host s %.2f (after pdist)  bit-equal %s' % (host_s, want.tobytes() == radii.tobytes())
            print(line, flush=True)

    w = workloads.costanzo_surrogate()
    n = w['xy'].shape[0]
    graph = safepy_amd.LayoutGraph(w['xy'], w['edge_u'], w['edge_v'], length=w['length'])
    metric = 'shortpath_weighted_layout'
    src = None

    def search():
        nonlocal src
        if src is not None:
            src.close()
        src = be.Neighborhoods.shortpath(ctx, n, w['edge_u'], w['edge_v'], w['length'], np.inf, keep_distances=True)
    unbounded_s, _ = median_of(args.passes, host_clock(search))
    diameter_s, (dia_mean, dia_max) = median_of(args.passes, host_clock(define(graph, metric, 'diameter', 0.1)))
    for k in ks:
        select_ms, radii = median_of(args.passes, device_ms(lambda: src.row_distance_select(k)))
        build_ms, (mean, widest) = median_of(args.passes, device_ms(closing(
            lambda: be.Neighborhoods.from_distances_rows(src, radii, keep_distances=True))))
        define_s, _ = median_of(args.passes, host_clock(define(graph, metric, 'nearest', k)))
        print('%s  N=%6d  edges=%6d  k=%4d  unbounded s %.3f  select ms %.3f  build ms %.3f  define s %.3f  diameter s %.3f  '
              'neighbors per node %.1f (max %d; diameter 0.1: %.1f, max %d)' % (metric, n, w['edge_u'].shape[0], k, unbounded_s,
                                                                               select_ms, build_ms, define_s, diameter_s, mean, widest,
                                                                               dia_mean, dia_max), flush=True)
    src.close()


if __name__ == '__main__':
    main()
