"""Time of attribute_transform = 'rank': the three kernels of safe_attr_rank, the whole call, the analytic test with and
without the transform, and scipy.stats.rankdata of the same matrix on the same host.

  configs[1]  3971 x 4373 quantitative f64 attributes (5 % rows without a value, 1 % NaN cells) on the Costanzo surrogate's
              shortest-path network
  configs[4]  20 000 x 6250 quantitative f64 attributes, one rank's share, euclidean r = 0.1

Per configuration, the median (min .. max) of --passes passes after one discarded warm-up pass:
  k_rank_keys / k_rank_sort / k_rank_emit   each kernel between two events on the context's stream (safe_last_rank_stats), and
              its bytes / s against its own traffic floor, as a fraction of 8 TB/s.  Floors per cell of the f64 source:
                keys  16 B: the source read, the keys written
                sort  8 + 8 p B: the keys read, the sorted chunks written (p = padded rows / rows)
                emit  16 + 8 p B: the keys read, every sorted chunk read once, the ranks written (the chunks are in fact read
                      once per cell chunk, from L2 after the first)
  safe_attr_rank   the whole call up to its return (it synchronises), the handle's release outside the timed region; floor
              16 B per cell: one read of the source, one write of R (2.0 GB at configs[4]'s share)
  compute_pvalues(how='analytic')   wall time on the resident matrix, with attribute_transform = 'none' and 'rank'
  scipy.stats.rankdata(axis=0)      --host-passes passes (default 1: it takes seconds) on the host matrix

There is no pass / fail time here.

usage: python tools/rank_time.py [--configs 1,4] [--passes 5] [--host-passes 1] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


def make_config(config):
    """SAFE instance with neighborhoods defined and the quantitative matrix resident on the device."""
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
    sf.load_attributes(attribute_file=b, keep_on_device=True)
    return sf


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def rate(bytes_, ms_values):
    r = bytes_ / (1e-3 * float(np.median(ms_values)))
    return '%.2f TB/s = %.2f of 8 TB/s (floor %.2f GB)' % (r / 1e12, r / PEAK_BYTES_PER_S, bytes_ / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,4')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--host-passes', type=int, default=1)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from scipy.stats import rankdata
    from safepy_amd import _lib
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    report = {}
    for config in [int(c) for c in args.configs.split(',')]:
        sf = make_config(config)
        attr = sf._attr_dev
        n, m = attr.n, attr.m
        esz = sf.node2attribute.dtype.itemsize
        padded = -(-n // _lib.RANK_CHUNK) * _lib.RANK_CHUNK / float(n)
        cells = float(n) * m
        floors = {'k_rank_keys': (esz + 8) * cells, 'k_rank_sort': (8 + 8 * padded) * cells, 'k_rank_emit': (16 + 8 * padded) * cells,
                  'safe_attr_rank': (esz + 8) * cells}
        rows = {name: [] for name in list(floors) + ["analytic 'none'", "analytic 'rank'"]}
        for k in range(args.passes + 1):
            ctx.sync()
            t0 = time.perf_counter()
            r = attr.rank()
            call_ms = 1e3 * (time.perf_counter() - t0)
            parts = ctx.last_rank_stats()
            r.close()
            walls = {}
            for transform in ('none', 'rank'):
                ctx.sync()
                t0 = time.perf_counter()
                sf.compute_pvalues(how='analytic', attribute_transform=transform)
                ctx.sync()
                walls[transform] = 1e3 * (time.perf_counter() - t0)
            if k:
                for name, ms in zip(('k_rank_keys', 'k_rank_sort', 'k_rank_emit'), parts):
                    rows[name].append(ms)
                rows['safe_attr_rank'].append(call_ms)
                rows["analytic 'none'"].append(walls['none'])
                rows["analytic 'rank'"].append(walls['rank'])
        host = []
        for _ in range(args.host_passes):
            t0 = time.perf_counter()
            rankdata(sf.node2attribute, method='average', axis=0, nan_policy='omit')
            host.append(1e3 * (time.perf_counter() - t0))
        print('configs[%d]: %d x %d %s, %d chunk(s) of %d rows per column' % (config, n, m, sf.node2attribute.dtype, -(-n // _lib.RANK_CHUNK),
                                                                            _lib.RANK_CHUNK))
        for name, ms in rows.items():
            line = '  %-18s ms %s' % (name, spread(ms))
            if name in floors:
                line += '   ' + rate(floors[name], ms)
            print(line)
        if host:
            print('  %-18s ms %s   (host, scipy.stats.rankdata(axis=0))' % ('rankdata', spread(host)))
        print("  the transform takes the analytic call from %.1f to %.1f ms (x %.2f)"
              % (np.median(rows["analytic 'none'"]), np.median(rows["analytic 'rank'"]),
                 np.median(rows["analytic 'rank'"]) / np.median(rows["analytic 'none'"])))
        report['configs[%d]' % config] = dict(rows, rankdata_host_ms=host, floors_bytes=floors)
        sf._drop_device_attributes()
        sf.neighborhoods = None                                 # gives the membership handle back
        for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
            setattr(sf, name, None)                             # ... and the result matrices
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
