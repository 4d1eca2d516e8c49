"""Times of the max-statistic adjustment (familywise_adjustment = 'maxT') next to the weighted permutation counts, in one
process, on device-resident inputs and outputs (quantitative f64 attributes, flat neighborhoods carrying UNIT weights so that
both kernels run the same sums on the same handle, tables and columns).

  configs[1]  3971 x 4373 on the Costanzo surrogate's shortest-path network (the default metric)
  configs[4]  20 000 x 6250, one rank's share, euclidean r = 0.1

Per configuration, the median (min .. max) of --passes passes after one discarded warm-up pass, kernel times from the context's
event pair (safe_last_kernel_stats):
  extremes    k_maxt_extremes (safe_permtest_extremes) next to k_permtest_weighted (safe_permtest_counts_weighted), in fs per
              member x attribute x permutation.  k_permtest_weighted is the yardstick: the new kernel does the same gathers
              plus the standardisation and the reduction over the rows.  Its bound is the yardstick's own: one 128-byte tile
              row gathered per member, 16 columns and permutation.
  counts      k_maxt_counts (safe_counts_from_extremes), both scopes, in ps per cell x permutation
  call        SAFE.compute_pvalues(how='randomization', familywise_adjustment='maxT') on the same columns, host ms, next to the
              same call without the adjustment (which takes the exact fixed-point kernels: the limit's measured ratio)
--permutations and --work bound the time: the columns are cut to work / (members x permutations), a multiple of 16.

There is no pass / fail time here.

usage: python tools/maxt_time.py [--configs 1,4] [--passes 5] [--permutations 1000] [--work 4e12] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_config(config):
    """(SAFE instance that owns the flat membership handle, attribute values f64 [n, m])"""
    import safepy_amd
    from safepy_amd import workloads
    sf = safepy_amd.SAFE(verbose=False)
    if config == 4:
        n, m = 20000, 6250
        sf.graph = safepy_amd.LayoutGraph(workloads.uniform_layout(4, n))
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1)
        b = workloads.quantitative_attributes(3, n, m)
    else:
        data = workloads.costanzo_surrogate(seed=0)
        sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
        sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout')
        b = workloads.quantitative_attributes(3, *data['attributes'].shape)
    return sf, b


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def timed(ctx, fn):
    """(host ms of the call up to its return, kernel name, kernel ms)"""
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
    ap.add_argument('--work', type=float, default=4e12, help='member x attribute x permutation units of one call, at most')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    report = {}
    for config in [int(c) for c in args.configs.split(',')]:
        sf, b = make_config(config)
        nbr = sf._device_neighborhoods()
        n, P = b.shape[0], args.permutations
        cols = int(min(b.shape[1], max(16, (args.work / (max(nbr.nnz, 1) * P)) // 16 * 16)))
        b = np.ascontiguousarray(b[:, :cols])
        attr = be.Attributes.from_host(ctx, b)
        bufs = [ctx.alloc_f64(n, cols) for _ in range(4)] + [ctx.alloc(n * cols), ctx.alloc_f64(P, cols), ctx.alloc_f64(P, cols),
                                                               ctx.alloc_f64(2 * cols)]
        ns, neg, pos, z, live, tmax, tmin, least = [x.ptr for x in bufs]
        perms = be.Permutations(ctx, n, attr.row_flags(), P, 0)
        sf.random_seed, sf.num_permutations = 0, P
        sf.load_attributes(attribute_file=b)

        def api(adjustment):
            sf.compute_pvalues(how='randomization', familywise_adjustment=adjustment)

        calls = {
            'safe_permtest_counts_weighted': lambda: be.permtest_counts_weighted(ctx, nbr, attr, perms, ns, neg, pos),
            'safe_permtest_extremes': lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, tmax, tmin),
            'safe_counts_from_extremes (neighborhoods)': lambda: be.counts_from_extremes(ctx, n, cols, P, 'neighborhoods', z, live, tmax, tmin,
                                                                                         neg, pos, least, least + 8 * cols),
            'safe_counts_from_extremes (all)': lambda: be.counts_from_extremes(ctx, n, cols, P, 'all', z, live, tmax, tmin, neg, pos,
                                                                               least, least + 8 * cols),
            "compute_pvalues 'none'": lambda: api('none'),
            "compute_pvalues 'maxT'": lambda: api('maxT'),
        }
        rows = {name: ([], []) for name in calls}
        kernels = {}
        nnz = nbr.nnz
        try:
            for k in range(args.passes + 1):
                for name, fn in calls.items():
                    unit = name.startswith('safe_permtest')
                    if unit:
                        nbr.set_weights(np.ones(nbr.nnz))       # unit weights: the same sums in both kernels
                    try:
                        call_ms, kernels[name], kernel_ms = timed(ctx, fn)
                    finally:
                        if unit:
                            nbr.clear_weights()
                    if k:
                        rows[name][0].append(call_ms)
                        rows[name][1].append(kernel_ms)
        finally:
            perms.close()
            for x in bufs:
                x.free()
            attr.close()
            sf.neighborhoods = None                             # gives the membership handle back
        print('configs[%d]: %d x %d of %d columns, %d members (%.1f per neighborhood), %d permutations'
              % (config, n, cols, b.shape[1], nnz, nnz / n, P))
        for name, (call, kern) in rows.items():
            line = '  %-42s call ms %s' % (name, spread(call))
            med = 1e-3 * float(np.median(kern))
            if name.startswith('safe_permtest'):
                line += '   %s ms %s   %.2f fs per member x attribute x permutation' % (kernels[name], spread(kern), med / (nnz * cols * P) * 1e15)
            elif name.startswith('safe_counts'):
                line += '   %s ms %s   %.2f ps per cell x permutation' % (kernels[name], spread(kern), med / (n * cols * P) * 1e12)
            print(line)
            report['configs[%d] %s' % (config, name)] = {'call_ms': call, 'kernel': kernels[name], 'kernel_ms': kern}
        ratio = float(np.median(rows['safe_permtest_extremes'][1])) / float(np.median(rows['safe_permtest_counts_weighted'][1]))
        print('  k_maxt_extremes / k_permtest_weighted = %.3f' % ratio)
        report['configs[%d] ratio' % config] = ratio
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
