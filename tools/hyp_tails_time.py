"""Time of the two-tailed hypergeometric call (safe_hypergeom_tails, attribute_sign = 'both', the evaluator chosen by the
library) next to safe_hypergeom in the same process, on device-resident inputs and outputs.

  configs[1]  3971 x 4373 Costanzo surrogate made 0/1 (NaN kept), shortest-path network
  configs[3]  20 000 x 10 000 binary, 1 % ones, euclidean r = 0.1 (bench.py's dropin_extras inputs)

Per configuration, the median (min .. max) of --passes passes after one discarded warm-up pass:
  call ms     the whole entry point, up to its return (both return once the stream has drained)
  emit ms     the emit kernel alone (safe_last_kernel_stats), and its bytes / s as a fraction of 8 TB/s: it reads ns (8 B per cell)
              and writes four matrices (32 B per cell) -- 40 B x 2e8 cells = 8 GB at configs[3], the arithmetic floor

There is no pass / fail time here.

usage: python tools/hyp_tails_time.py [--configs 1,3] [--passes 5] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


def make_config(config, be, ctx):
    """(SAFE instance that owns the membership handle, membership handle, attribute handle)"""
    import safepy_amd
    from safepy_amd import workloads
    sf = safepy_amd.SAFE(verbose=False)
    if config == 3:
        n, m = 20000, 10000
        b = (np.random.default_rng(5).uniform(size=(n, m)) < 0.01).astype(np.uint8)
        sf.graph = safepy_amd.LayoutGraph(workloads.uniform_layout(4, n))
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1)
    else:
        data = workloads.costanzo_surrogate(seed=0)
        sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
        sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout')
        b = data['attributes'].astype(np.float64)
        b = np.where(np.isnan(b), np.nan, (b != 0).astype(np.float64))
    return sf, sf._device_neighborhoods(), be.Attributes.from_host(ctx, b)


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,3')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    report = {}
    for config in [int(c) for c in args.configs.split(',')]:
        sf, nbr, attr = make_config(config, be, ctx)
        n, m = attr.n, attr.m
        bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
        ptrs = [b.ptr for b in bufs]
        rows = {'safe_hypergeom': ([], []), 'safe_hypergeom_tails': ([], [])}
        kernels = {}
        try:
            for k in range(args.passes + 1):
                for name, fn in (('safe_hypergeom', lambda: be.hypergeom(ctx, nbr, attr, 0.05, ptrs[2:])),
                                 ('safe_hypergeom_tails', lambda: be.hypergeom_tails(ctx, nbr, attr, 'both', 0.05, ptrs))):
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
            for b in bufs:
                b.free()
            attr.close()
            sf.neighborhoods = None                             # gives the membership handle back
        print('configs[%d]: %d x %d' % (config, n, m))
        for name, (call, kern) in rows.items():
            line = '  %-22s call ms %s   %s ms %s' % (name, spread(call), kernels[name], spread(kern))
            if name == 'safe_hypergeom_tails':
                rate = 40.0 * n * m / (1e-3 * float(np.median(kern)))
                line += '   %.2f TB/s = %.2f of 8 TB/s (40 B per cell: %.2f GB)' % (rate / 1e12, rate / PEAK_BYTES_PER_S, 40.0 * n * m / 1e9)
            print(line)
            report['configs[%d] %s' % (config, name)] = {'call_ms': call, 'kernel': kernels[name], 'kernel_ms': kern}
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
