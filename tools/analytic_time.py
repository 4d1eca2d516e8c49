"""Time of the analytic test (safe_moments_test, attribute_sign = 'both') next to the permutation test it stands in for
(safe_randomization, 'sum' scores, 1000 seeded permutations) in the same process, on device-resident inputs and outputs.

  configs[1]  3971 x 4373 quantitative f64 attributes (5 % rows without a value, 1 % NaN cells) on the Costanzo surrogate's
              shortest-path network
  configs[4]  20 000 x 6250 quantitative f64 attributes, one rank's share, euclidean r = 0.1 (bench.py's mfma_kernel inputs)

Per configuration, the median (min .. max) of --passes passes after one discarded warm-up pass:
  call ms     the whole entry point, up to its return (both return once the stream has drained); the permutation handle of
              safe_randomization is made outside the timed region
  emit ms     k_moments_emit alone (safe_last_kernel_stats), and its bytes / s as a fraction of 8 TB/s: it reads ns (8 B per
              cell) and writes four matrices (32 B per cell), five with z (--with-z: 48 B per cell) -- the arithmetic floor

There is no pass / fail time here.

usage: python tools/analytic_time.py [--configs 1,4] [--passes 5] [--with-z] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12
NUM_PERMUTATIONS = 1000


def make_config(config, be, ctx):
    """(SAFE instance that owns the membership handle, membership handle, attribute handle)"""
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
    return sf, sf._device_neighborhoods(), be.Attributes.from_host(ctx, b)


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,4')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--with-z', action='store_true')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    report = {}
    cell_bytes = 48.0 if args.with_z else 40.0
    for config in [int(c) for c in args.configs.split(',')]:
        sf, nbr, attr = make_config(config, be, ctx)
        n, m = attr.n, attr.m
        bufs = [ctx.alloc_f64(n, m) for _ in range(6 if args.with_z else 5)] + [ctx.alloc_f64(m)]
        ptrs = [b.ptr for b in bufs[:5]] + [bufs[-1].ptr]
        z_ptr = bufs[5].ptr if args.with_z else None
        rows = {'safe_randomization': ([], []), 'safe_moments_test': ([], [])}
        kernels = {}
        try:
            for k in range(args.passes + 1):
                perms = be.Permutations(ctx, n, attr.row_flags(), NUM_PERMUTATIONS, 0)
                try:
                    for name, fn in (('safe_randomization', lambda: be.randomization(ctx, nbr, attr, perms, 'sum', 'both', 0.05, ptrs)),
                                     ('safe_moments_test', lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs, z_ptr=z_ptr))):
                        ctx.sync()
                        t0 = time.perf_counter()
                        fn()
                        ctx.sync()
                        call_ms = 1e3 * (time.perf_counter() - t0)
                        kernel, kernel_ms, launches = ctx.last_kernel()
                        kernels[name] = kernel
                        if k:
                            rows[name][0].append(call_ms)
                            rows[name][1].append(kernel_ms * max(int(launches), 1))
                finally:
                    perms.close()
        finally:
            for b in bufs:
                b.free()
            attr.close()
            sf.neighborhoods = None                             # gives the membership handle back
        print('configs[%d]: %d x %d' % (config, n, m))
        for name, (call, kern) in rows.items():
            line = '  %-20s call ms %s   %s ms %s' % (name, spread(call), kernels[name], spread(kern))
            if name == 'safe_moments_test':
                rate = cell_bytes * n * m / (1e-3 * float(np.median(kern)))
                line += '   %.2f TB/s = %.2f of 8 TB/s (%d B per cell: %.2f GB)' % (rate / 1e12, rate / PEAK_BYTES_PER_S, cell_bytes,
                                                                                    cell_bytes * n * m / 1e9)
            print(line)
            report['configs[%d] %s' % (config, name)] = {'call_ms': call, 'kernel': kernels[name], 'kernel_ms': kern}
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
