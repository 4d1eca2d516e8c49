"""Times of the distance-weighted entry points next to their flat neighbours, in one process, on device-resident inputs and
outputs (quantitative f64 attributes, triangular weights unless said otherwise).

  configs[1]  3971 x 4373 on the Costanzo surrogate's shortest-path network (the default metric; weights from the kept matrix)
  configs[4]  20 000 x 6250, one rank's share, euclidean r = 0.1 (weights from the coordinates)

Per configuration, the median (min .. max) of --passes passes after one discarded warm-up pass, kernel times from the
context's event pair (safe_last_kernel_stats):
  score       k_score_weighted next to safe_score 'sum' on the same handle, and its floor -- one read of the attribute matrix
              plus one write of ns -- as a fraction of 8 TB/s.  What lies between the floor and the time is member rows read
              again and again, served from cache.
  analytic    safe_moments_test_weighted next to safe_moments_test: call ms, and the emit kernel alone (40 B per cell in both)
  counts      k_permtest_weighted with UNIT weights next to k_permtest_gather<16,false> (SAFE_HIP_FORCE_PATH=gather) on the
              same handle, tables and columns, in fs per member x attribute x permutation.  The gather kernel is the
              yardstick: one more load and one more multiply per member.  The flat call on its default route (the exact
              fixed-point matrix-core kernels, which do not apply to real weights) stands beside them: the limit's measured
              ratio.  --permutations and --work bound the time: the columns of this part are cut to
              work / (members x permutations), a multiple of 16.

There is no pass / fail time here.

usage: python tools/weights_time.py [--configs 1,4] [--passes 5] [--permutations 1000] [--work 4e12] [--json FILE]"""
import argparse
import json
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


def make_config(config, be, ctx):
    """(SAFE instance that owns the weighted membership handle, membership handle, attribute handle)"""
    import safepy_amd
    from safepy_amd import workloads
    sf = safepy_amd.SAFE(verbose=False)
    if config == 4:
        n, m = 20000, 6250
        sf.graph = safepy_amd.LayoutGraph(workloads.uniform_layout(4, n))
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1, neighborhood_weighting='triangular')
        b = workloads.quantitative_attributes(3, n, m)
    else:
        data = workloads.costanzo_surrogate(seed=0)
        sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
        sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_weighting='triangular')
        b = workloads.quantitative_attributes(3, *data['attributes'].shape)
    return sf, sf._device_neighborhoods(), be.Attributes.from_host(ctx, b)


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def timed(ctx, fn):
    """(host ms of the call up to its return, kernel name, kernel ms)"""
    import time
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    call_ms = 1e3 * (time.perf_counter() - t0)
    kernel, kernel_ms, launches = ctx.last_kernel()
    return call_ms, kernel, kernel_ms * max(int(launches), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,4')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--permutations', type=int, default=1000)
    ap.add_argument('--work', type=float, default=4e12, help='member x attribute x permutation units of one counts call, at most')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    report = {}
    for config in [int(c) for c in args.configs.split(',')]:
        sf, nbr, attr = make_config(config, be, ctx)
        n, m, P = attr.n, attr.m, args.permutations
        cols = int(min(m, max(16, (args.work / (max(nbr.nnz, 1) * P)) // 16 * 16)))
        bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
        ptrs = [b.ptr for b in bufs]
        perms = be.Permutations(ctx, n, attr.row_flags(), P, 0)
        triangular = nbr.weights()
        calls = {
            'safe_score': lambda: be.score(ctx, nbr, attr, 'sum', ptrs[0]),
            'safe_score_weighted': lambda: be.score_weighted(ctx, nbr, attr, ptrs[0]),
            'safe_moments_test': lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs),
            'safe_moments_test_weighted': lambda: be.moments_test_weighted(ctx, nbr, attr, 'both', 0.05, ptrs),
            'safe_permtest_counts (default)': lambda: be.permtest_counts(ctx, nbr, attr, perms, 'sum', ptrs[0], ptrs[1], ptrs[2], 0, cols),
            'safe_permtest_counts (gather)': lambda: be.permtest_counts(ctx, nbr, attr, perms, 'sum', ptrs[0], ptrs[1], ptrs[2], 0, cols),
            'safe_permtest_counts_weighted': lambda: be.permtest_counts_weighted(ctx, nbr, attr, perms, ptrs[0], ptrs[1], ptrs[2], 0, cols),
        }
        rows = {name: ([], []) for name in calls}
        kernels = {}
        try:
            for k in range(args.passes + 1):
                for name, fn in calls.items():
                    counts = 'permtest' in name
                    if counts:
                        nbr.set_weights(np.ones(nbr.nnz))       # unit weights: the same sums as the yardstick
                    if 'gather' in name:
                        os.environ['SAFE_HIP_FORCE_PATH'] = 'gather'
                    try:
                        call_ms, kernels[name], kernel_ms = timed(ctx, fn)
                    finally:
                        os.environ.pop('SAFE_HIP_FORCE_PATH', None)
                        if counts:
                            nbr.set_weights(triangular)
                    if k:
                        rows[name][0].append(call_ms)
                        rows[name][1].append(kernel_ms)
        finally:
            perms.close()
            for b in bufs:
                b.free()
            attr.close()
            nnz = nbr.nnz
            sf.neighborhoods = None                             # gives the membership handle back
        print('configs[%d]: %d x %d, %d members (%.1f per neighborhood)' % (config, n, m, nnz, nnz / n))
        for name, (call, kern) in rows.items():
            line = '  %-30s call ms %s   %s ms %s' % (name, spread(call), kernels[name], spread(kern))
            med = 1e-3 * float(np.median(kern))
            if name == 'safe_score_weighted':
                floor = 16.0 * n * m
                line += '   floor %.2f GB: %.2f TB/s = %.3f of 8 TB/s' % (floor / 1e9, floor / med / 1e12, floor / med / PEAK_BYTES_PER_S)
            if name == 'safe_moments_test_weighted':
                line += '   emit %.2f TB/s (40 B per cell)' % (40.0 * n * m / med / 1e12)
            if 'permtest' in name:
                line += '   %.2f fs per member x attribute x permutation (%d columns, %d permutations)' % (med / (nnz * cols * P) * 1e15, cols, P)
            print(line)
            report['configs[%d] %s' % (config, name)] = {'call_ms': call, 'kernel': kernels[name], 'kernel_ms': kern}
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
