"""Time of define_top_attributes under attribute_unimodality_metric = 'radius' (enriched-pair counts on the device) on the
inputs of tools/domains_time.py: shaped like BASELINE.json configs[1] (3971 x 4373) and configs[3] (20 000 x 10 000),
Euclidean metric, hypergeometric path, spatial attributes.  One process, one device.

Per config, medians of --passes passes (default 5) after one warm-up pass:
  * building the within-reach relation W at 2 r (backend.Neighborhoods.euclidean; host clock around a synchronised call);
  * the pack + count kernels (k_profile_pack + k_pair_count) on the resident nes_binary: the context's event pair; with the
    stream of W rows the count kernel is compared with ("Enriched-pair counts"): set bits x words x 8 bytes, and
    the rate that makes;
  * define_top_attributes as a whole under 'radius' and under 'connectivity' (host clock, nes_binary resident);
  * the host route: nes_binary downloaded once, then `(pdist(xy[idx]) < t).sum()` per candidate attribute.  With
    --host-sample K (default 300; 0 = all) the loop runs on K evenly spaced candidates and its time is scaled by
    candidates / K: the line says so.  Its counts are checked against the device's.

usage: python tools/unimodality_time.py [--configs 1,3] [--passes 5] [--host-sample 300] [--cache DIR] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def median_ms(fn, sync, passes):
    out = []
    for rep in range(-1, passes):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep >= 0:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def run_config(amd, g, config, passes, host_sample):
    import pandas as pd
    from scipy.spatial.distance import pdist
    from safepy_amd.safe import _DeviceResult
    be = amd.backend
    xy, eu, ev = g['xy'], g['edge_u'], g['edge_v']
    n, m = xy.shape[0], g['attributes'].shape[1]
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1)))
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.05 if config == 1 else 0.02)
    sf.load_attributes(attribute_file=g['attributes'].astype(np.float64))
    sf.attributes = pd.DataFrame({'id': np.arange(m), 'name': ['term %d' % j for j in range(m)]})
    sf.compute_pvalues(how='hypergeometric')
    ctx = sf._ctx()
    row = {'config': config, 'n': int(n), 'm': int(m), 'passes': passes}
    resident = lambda: isinstance(sf.__dict__.get('_r_nes_binary'), _DeviceResult)
    assert resident()

    t = sf.attribute_unimodality_radius_multiple * sf.neighborhood_radius_resolved
    made = []

    def build():
        made.append(be.Neighborhoods.euclidean(ctx, xy, t))

    def closing():
        for h in made:
            h.close()
        made.clear()
    ms = []
    for rep in range(-1, passes):
        ctx.sync()
        t0 = time.perf_counter()
        build()
        ctx.sync()
        if rep >= 0:
            ms.append((time.perf_counter() - t0) * 1e3)
        if rep < passes - 1:
            closing()
    row['build_within_ms'] = float(np.median(ms))
    within = made[0]
    row['within_nnz'] = int(within.nnz)

    cand = sf.attributes.index.values[(sf.attributes['num_neighborhoods_enriched'] >= sf.attribute_enrichment_min_size).values]
    src = sf.__dict__['_r_nes_binary']
    kernel = []
    for rep in range(-1, passes):
        q, e, k_ms = ctx.enriched_pair_counts_dev(within, src.buf.ptr, n, m, cand)
        if rep >= 0:
            kernel.append(k_ms)
    closing()
    words = (n + 63) // 64
    row['candidates'] = int(cand.size)
    row['enriched_cells'] = int(e.sum())
    row['pack_and_count_kernel_ms'] = float(np.median(kernel))
    row['w_row_stream_bytes'] = int(e.sum()) * words * 8
    row['w_row_stream_gb_per_s'] = row['w_row_stream_bytes'] / 1e9 / (row['pack_and_count_kernel_ms'] / 1e3)

    for metric in ('radius', 'connectivity'):
        row['define_top_attributes_%s_ms' % metric] = median_ms(
            lambda: sf.define_top_attributes(attribute_unimodality_metric=metric), ctx.sync, passes)
        row['top_%s' % metric] = int(sf.attributes['top'].sum())
        assert resident()

    # the host route (last: reading nes_binary moves it to the host)
    t0 = time.perf_counter()
    nb = sf.nes_binary
    row['host_download_ms'] = (time.perf_counter() - t0) * 1e3
    pick = cand if not host_sample or host_sample >= cand.size else cand[np.linspace(0, cand.size - 1, host_sample).astype(np.int64)]
    pos = {a: i for i, a in enumerate(cand.tolist())}
    t0 = time.perf_counter()
    counts = []
    for a in pick.tolist():
        idx = np.flatnonzero(nb[:, a] > 0)
        counts.append(int((pdist(xy[idx]) < t).sum()) if idx.size > 1 else 0)
    loop_ms = (time.perf_counter() - t0) * 1e3
    for a, c in zip(pick.tolist(), counts):
        assert (q[pos[a]] - e[pos[a]]) // 2 == c, 'the host loop and the device disagree on attribute %d' % a
    row['host_loop_attributes'] = int(pick.size)
    row['host_loop_ms'] = loop_ms
    row['host_loop_scaled_ms'] = loop_ms * cand.size / max(pick.size, 1)
    for s in ('nes', 'nes_binary', 'ns', 'pvalues_pos', 'pvalues_neg'):
        setattr(sf, s, None)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,3')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--host-sample', type=int, default=300)
    ap.add_argument('--cache', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import domains_time
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'unimodality_time.py needs a HIP device'
    rows = []
    for config in (int(c) for c in args.configs.split(',')):
        row = run_config(safepy_amd, domains_time.make_inputs(config, args.cache), config, args.passes, args.host_sample)
        rows.append(row)
        sampled = row['host_loop_attributes'] < row['candidates']
        print('configs[%d] %dx%d, %d candidates, %d enriched cells, nnz(W) %d (medians of %d passes):\n'
              '  build W at 2 r %.2f ms; pack + count kernels %.3f ms (W-row stream %.2f GB: %.0f GB/s);\n'
              "  define_top_attributes 'radius' %.1f ms (top %d), 'connectivity' %.1f ms (top %d);\n"
              '  host route: download %.1f ms + pdist loop %.1f ms%s'
              % (config, row['n'], row['m'], row['candidates'], row['enriched_cells'], row['within_nnz'], row['passes'],
                 row['build_within_ms'], row['pack_and_count_kernel_ms'], row['w_row_stream_bytes'] / 1e9, row['w_row_stream_gb_per_s'],
                 row['define_top_attributes_radius_ms'], row['top_radius'], row['define_top_attributes_connectivity_ms'],
                 row['top_connectivity'], row['host_download_ms'], row['host_loop_scaled_ms'],
                 ' (SCALED from %d of %d candidates: %.1f ms measured)' % (row['host_loop_attributes'], row['candidates'], row['host_loop_ms'])
                 if sampled else ' (all candidates)'), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
