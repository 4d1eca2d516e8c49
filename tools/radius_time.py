"""Time of resolving neighborhood_radius_type = 'percentile' (SAFE.define_neighborhoods / node_distance_percentile): the exact
selection kernels of nbr.hip beside the host route they replace.

  euclidean, uniform layouts, one line per N:
    count ms / select ms   safe_pair_distance_select_xy with no rank (one sweep) and with the two ranks of the percentile
                           (six sweeps), between the context's timer events (upload, sweeps, read-backs)
    host s                 np.percentile(pdist(xy), q) on this host's CPU (only N <= --host-max: 8 bytes x N (N - 1) / 2)
    radius                 the resolved radius, and whether the two agree on the bits
  shortpath_weighted_layout on workloads.costanzo_surrogate (N = 3971), host clock:
    unbounded s            the all-pairs search with cutoff = +inf that keeps the distances on the device
    select ms              safe_nbr_distance_select on that handle (count + the two ranks)
    bounded s              the final search with cutoff = the resolved radius

usage: python tools/radius_time.py [--sizes 3971,20000] [--q 2.5] [--host-max 20000]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='3971,20000')
    ap.add_argument('--q', type=float, default=2.5)
    ap.add_argument('--host-max', type=int, default=20000)
    args = ap.parse_args()
    from scipy.spatial.distance import pdist
    from safepy_amd import backend as be, safe as S, workloads
    ctx = be.Context.default(0)
    ctx.pair_distance_select(workloads.uniform_layout(0, 512), [0])                     # (first launch of the kernels)
    for n in [int(s) for s in args.sizes.split(',')]:
        xy = workloads.uniform_layout(n, n)
        ctx.timer_start()
        count = ctx.pair_distance_select(xy, [])[1]
        count_ms = ctx.timer_stop_ms()
        plan = S._percentile_plan(count, [args.q])
        ctx.timer_start()
        values = ctx.pair_distance_select(xy, plan[0])[0]
        select_ms = ctx.timer_stop_ms()
        radius = S._percentile_values(plan, values)[0]
        line = 'euclidean  N=%6d  pairs=%11d  q=%g  count ms %.3f  select ms %.3f  radius %r' % (
            n, count, args.q, count_ms, select_ms, radius)
        if n <= args.host_max:
            t0 = time.perf_counter()
            want = float(np.percentile(pdist(xy), args.q))
            line += '  host s %.2f  bit-equal %s' % (time.perf_counter() - t0, np.float64(want).tobytes() == np.float64(radius).tobytes())
        print(line, flush=True)

    w = workloads.costanzo_surrogate()
    n = w['xy'].shape[0]
    t0 = time.perf_counter()
    nbr = be.Neighborhoods.shortpath(ctx, n, w['edge_u'], w['edge_v'], w['length'], np.inf, keep_distances=True)
    t1 = time.perf_counter()
    plan = S._percentile_plan(nbr.distance_select([])[1], [args.q])
    radius = S._percentile_values(plan, nbr.distance_select(plan[0])[0])[0]
    t2 = time.perf_counter()
    nbr.close()
    t3 = time.perf_counter()
    nbr = be.Neighborhoods.shortpath(ctx, n, w['edge_u'], w['edge_v'], w['length'], radius, keep_distances=True)
    t4 = time.perf_counter()
    print('shortpath_weighted_layout  N=%6d  edges=%6d  q=%g  unbounded s %.3f  select ms %.3f  bounded s %.3f  radius %r  '
          'neighbors per node %.1f' % (n, w['edge_u'].shape[0], args.q, t1 - t0, 1e3 * (t2 - t1), t4 - t3, radius,
                                       nbr.nnz / n), flush=True)
    nbr.close()


if __name__ == '__main__':
    main()
