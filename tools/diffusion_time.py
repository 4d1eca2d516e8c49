"""Time of node_distance_metric = 'diffusion' (SAFE.define_neighborhoods): the whole call, the step kernel and the distance
transform of diffusion.hip against their traffic floors, beside the same call under 'shortpath_weighted_layout' and a scipy.sparse
restatement on this host's CPU.  Every device figure is the median of --passes passes after one warm-up pass, all in one process.

  one line per network (workloads.costanzo_surrogate, N = 3971; a clustered layout of --big nodes with radius edges):
    define s      SAFE.define_neighborhoods('diffusion', 'nearest', k), host clock: the kernel call with cutoff = +inf, the per-row
                  selection, the membership from the kept matrix
    step ms       k_diffusion_step per iteration (all launches between two events / steps, safe_last_diffusion_stats), and its
                  16 N^2 bytes (one read of X, one write of Y) per second as a fraction of 8 TB/s; the neighbor rows read again
                  are expected from cache and are not in the floor
    transform ms  k_diffusion_transform, and its floor: the upper triangle of K read (4 N^2 bytes), the kept matrix written
                  (8 N^2) and the bit matrix (N^2 / 8), likewise
    shortpath s   the same call with node_distance_metric = 'shortpath_weighted_layout'
    host s        X <- alpha I + beta (S @ X) with S a scipy.sparse CSR matrix and X dense, `steps` times, then the distance
                  transform in NumPy, one pass (only N <= --host-max; not a tuned baseline), and the largest difference of its
                  K from the device's
  matrices held on the device at peak: three N x N f64 (two iterates, the kept distances).

usage: python tools/diffusion_time.py [--big 20000] [--k 50] [--restart 0.5] [--steps 32] [--passes 5] [--host-max 3971]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_of(passes, fn):
    """(median of `passes` timed runs of fn after one untimed run, the last result); fn returns (seconds, result)."""
    fn()
    runs = [fn() for _ in range(passes)]
    return float(np.median([t for t, _ in runs])), runs[-1][1]


def host_kernel(n, eu, ev, restart, steps):
    """The scipy.sparse restatement: (seconds, K).  S @ X sums a row's products in CSR order too, duplicates merged first."""
    from scipy import sparse
    t0 = time.perf_counter()
    keep = eu != ev
    rows = np.concatenate([eu, ev[keep]])
    cols = np.concatenate([ev, eu[keep]])
    a = sparse.csr_array((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    deg = np.asarray(a.sum(axis=1)).reshape(-1)
    with np.errstate(divide='ignore'):
        r = np.where(deg == 0, 0.0, 1.0 / np.sqrt(deg))
    s = sparse.diags_array(r) @ a @ sparse.diags_array(r)
    x = np.eye(n)
    for _ in range(steps):
        x = (1.0 - restart) * (s @ x)
        x[np.arange(n), np.arange(n)] += restart
    diag = x.diagonal()
    with np.errstate(divide='ignore', invalid='ignore'):
        d = 1.0 - x / np.sqrt(diag[:, None] * diag[None, :])
    d[d < 0] = 0.0
    d[x == 0] = np.inf
    np.fill_diagonal(d, 0.0)
    return time.perf_counter() - t0, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--big', type=int, default=20000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--restart', type=float, default=0.5)
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--host-max', type=int, default=3971)
    args = ap.parse_args()
    import safepy_amd
    from safepy_amd import backend as be, workloads
    ctx = be.Context.default(0)

    def define(graph, metric):
        sf = safepy_amd.SAFE(verbose=False)
        sf.graph = graph

        def once():
            t0 = time.perf_counter()
            sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=args.k,
                                    diffusion_restart=args.restart, diffusion_steps=args.steps)
            seconds = time.perf_counter() - t0
            return seconds, (sf._nbr.nnz / sf._nbr.n, sf._nbr.max_row_count, ctx.last_diffusion_stats())
        return once

    networks = []
    w = workloads.costanzo_surrogate()
    networks.append(('costanzo_surrogate', w['xy'], w['edge_u'], w['edge_v'], w['length']))
    if args.big > 0:
        rng = np.random.default_rng(args.big)
        xy = workloads.clustered_layout(rng, args.big)
        eu, ev = workloads.radius_edges(xy, 7 * args.big, rng, reach=0.05)
        dx, dy = xy[eu, 0] - xy[ev, 0], xy[eu, 1] - xy[ev, 1]
        networks.append(('clustered_%d' % args.big, xy, eu, ev, np.sqrt(dx * dx + dy * dy)))

    for name, xy, eu, ev, length in networks:
        n = xy.shape[0]
        graph = safepy_amd.LayoutGraph(xy, eu, ev, length=length)
        define_s, (mean, widest, (steps_ms, steps, transform_ms)) = median_of(args.passes, define(graph, 'diffusion'))
        shortpath_s, (sp_mean, sp_widest, _) = median_of(args.passes, define(graph, 'shortpath_weighted_layout'))
        step_ms = steps_ms / max(steps, 1)
        step_floor, transform_floor = 16.0 * n * n, (4.0 + 8.0 + 0.125) * n * n
        degree = np.bincount(np.concatenate([eu, ev]), minlength=n)
        line = ('%s  N=%6d  edges=%7d (largest degree %d)  k=%d  restart %.2f  steps %d  define s %.3f  step ms %.3f (%.1f %% of 8 TB/s '
                'over 16 N^2 B)  transform ms %.3f (%.1f %% over 12.125 N^2 B)  neighbors per node %.1f (max %d)  shortpath_weighted_layout '
                's %.3f (neighbors %.1f, max %d)  matrices at peak 3 x %.2f GB'
                % (name, n, len(eu), degree.max(), args.k, args.restart, steps, define_s, step_ms, 100 * step_floor / (step_ms * 1e-3) / 8e12,
                   transform_ms, 100 * transform_floor / (transform_ms * 1e-3) / 8e12, mean, widest, shortpath_s, sp_mean, sp_widest,
                   8.0 * n * n / 1e9))
        if n <= args.host_max:
            host_s, k_host = host_kernel(n, np.asarray(eu), np.asarray(ev), args.restart, args.steps)
            nbr, k_dev = be.Neighborhoods.diffusion(ctx, n, eu, ev, None, args.restart, args.steps, np.inf, want_kernel=True)
            nbr.close()
            line += '  host s %.2f (scipy.sparse, one pass; max |K - K_device| %.2e)' % (host_s, float(np.abs(k_host - k_dev).max()))
        print(line, flush=True)


if __name__ == '__main__':
    main()
