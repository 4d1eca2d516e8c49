"""Time of the domain stage, compute_pvalues -> define_top_attributes -> define_domains -> trim_domains, on inputs shaped
like BASELINE.json configs[1] (3971 x 4373, the Costanzo surrogate's layout and edges) and configs[3] (20 000 x 10 000,
uniform layout), hypergeometric path.  The attributes are spatial (every attribute annotates the nodes of one or two discs
of the layout), so that a few thousand of them are enriched in one region and the stage has real work: random annotations
give no top attribute at all.

Per repeat, one line: host-clock time of each stage (each ends in a device synchronise), the bytes the stage copied from
the device to the host and uploaded again (DeviceBuffer.download, the host forms' uploads, the small result tables), the
kernels' busy time of the device forms (ctx.last_kernel_busy_ms after each call -- for define_domains that includes the
linkage kernel of profile_linkage, whose only download is Z; the host forms record none) and whether
nes / nes_binary are still on the device afterwards.  The script uses the public SAFE interface only, so the same file
times any commit of the package: `--package DIR` imports safepy_amd from another checkout's root.

usage: python tools/domains_time.py [--configs 1,3] [--repeats 2] [--package DIR] [--cache DIR] [--json FILE] [--tag NAME]
One warm-up pass per config is always run first and not reported.  --cache DIR keeps the generated inputs as .npy files
(a second process, e.g. the other commit, then loads instead of generating); --tag names the lines and JSON rows."""
import argparse
import json
import os
import sys
import time

import numpy as np


def spatial_attributes(rng, xy, m):
    """u8 [n, m]: attribute j = the nodes within r_j of a random node (30 %: of either of two), thinned to 50-100 %."""
    n = xy.shape[0]
    b = np.zeros((n, m), dtype=np.uint8)
    span = np.ptp(xy[:, 0])
    for j0 in range(0, m, 250):
        j1 = min(m, j0 + 250)
        k = j1 - j0
        r = span * rng.uniform(0.02, 0.07, size=k)
        hit = np.zeros((n, k), dtype=bool)
        for second in (False, True):
            c = xy[rng.integers(n, size=k)]
            d2 = (xy[:, None, 0] - c[None, :, 0]) ** 2 + (xy[:, None, 1] - c[None, :, 1]) ** 2
            use = np.ones(k, dtype=bool) if not second else rng.uniform(size=k) < 0.3
            hit |= (d2 < (r * r)[None, :]) & use[None, :]
        hit &= rng.uniform(size=(n, k)) < rng.uniform(0.5, 1.0, size=k)[None, :]
        b[:, j0:j1] = hit
    return b


def make_inputs(config, cache):
    names = ('xy', 'edge_u', 'edge_v', 'attributes')
    if cache and all(os.path.exists(os.path.join(cache, 'domains_time_c%d_%s.npy' % (config, k))) for k in names):
        return {k: np.load(os.path.join(cache, 'domains_time_c%d_%s.npy' % (config, k))) for k in names}
    from safepy_amd import workloads
    rng = np.random.default_rng(100 + config)
    if config == 1:
        n, m = 3971, 4373
        xy = workloads.clustered_layout(rng, n)
        eu, ev = workloads.radius_edges(xy, 28202, rng)
    else:
        n, m = 20000, 10000
        xy = workloads.uniform_layout(7, n)
        eu, ev = workloads.radius_edges(xy, 140000, rng, reach=0.03)
    g = {'xy': xy, 'edge_u': eu, 'edge_v': ev, 'attributes': spatial_attributes(rng, xy, m)}
    if cache:
        os.makedirs(cache, exist_ok=True)
        for k in names:
            np.save(os.path.join(cache, 'domains_time_c%d_%s.npy' % (config, k)), g[k])
    return g


class Meter:
    """Counts the bytes the package moves between device and host and the kernel time of the device forms, by wrapping the
    backend functions safe.py goes through (those that exist in the package under test)."""

    def __init__(self, be):
        self.be, self.down, self.up, self.busy = be, 0, 0, 0.0
        self.undo = []
        meter = self

        def wrap(owner, name, make):
            if hasattr(owner, name):
                real = getattr(owner, name)
                setattr(owner, name, make(real))
                self.undo.append((owner, name, real))

        def download(real):
            def f(buf, shape, dtype=np.float64, out=None):
                got = real(buf, shape, dtype, out)
                meter.down += got.nbytes
                return got
            return f

        def host_form(real):                      # enriched_components(ctx, n, eu, ev, member) / jaccard_condensed(ctx, x)
            def f(*a):
                got = real(*a)
                meter.up += np.asarray(a[-1]).nbytes
                meter.down += got.nbytes
                return got
            return f

        def device_form(real):                    # Context methods: results..., kernel ms
            def f(ctx, *a):
                got = real(ctx, *a)
                meter.down += sum(x.nbytes for x in got[:-1])
                meter.busy += ctx.last_kernel_busy_ms()
                return got
            return f
        wrap(be.DeviceBuffer, 'download', download)
        wrap(be, 'enriched_components', host_form)
        wrap(be, 'jaccard_condensed', host_form)
        for name in ('enriched_components_dev', 'profile_distances', 'profile_linkage', 'node_domains'):
            wrap(be.Context, name, device_form)

    def take(self):
        got = (self.down, self.up, self.busy)
        self.down, self.up, self.busy = 0, 0, 0.0
        return got

    def close(self):
        for owner, name, real in self.undo:
            setattr(owner, name, real)


def run_once(amd, g, config):
    import pandas as pd
    from safepy_amd.safe import _DeviceResult
    sf = amd.SAFE(verbose=False)
    xy, eu, ev = g['xy'], g['edge_u'], g['edge_v']
    length = np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1))
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.05 if config == 1 else 0.02)
    sf.load_attributes(attribute_file=g['attributes'].astype(np.float64))
    m = g['attributes'].shape[1]
    sf.attributes = pd.DataFrame({'id': np.arange(m), 'name': ['term %d of group %d' % (j, j % 97) for j in range(m)]})
    meter = Meter(amd.backend)
    row = {'config': config, 'n': int(xy.shape[0]), 'm': int(m)}
    try:
        for stage, call in (('compute_pvalues', lambda: sf.compute_pvalues(how='hypergeometric')),
                            ('define_top_attributes', sf.define_top_attributes),
                            ('define_domains', sf.define_domains),
                            ('trim_domains', sf.trim_domains)):
            sf._ctx().sync()
            t0 = time.perf_counter()
            call()
            sf._ctx().sync()
            ms = (time.perf_counter() - t0) * 1e3
            down, up, busy = meter.take()
            row[stage] = {'ms': round(ms, 2), 'downloaded_bytes': int(down), 'uploaded_bytes': int(up), 'kernel_busy_ms': round(busy, 3)}
    finally:
        meter.close()
    row['top_attributes'] = int(sf.attributes['top'].sum())
    row['domains'] = int(len(sf.domains))
    row['resident_after'] = bool(all(isinstance(sf.__dict__.get(s), _DeviceResult) for s in ('_r_nes', '_r_nes_binary')))
    row['checksum'] = [int(sf.attributes['domain'].sum()), int(sf.node2domain['primary_domain'].sum()),
                       float(np.nansum(sf.node2domain['primary_nes'].values))]
    for s in ('nes', 'nes_binary', 'ns', 'pvalues_pos', 'pvalues_neg'):
        setattr(sf, s, None)                                  # frees the device copies before the next repeat
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,3')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--package', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--cache', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'domains_time.py needs a HIP device'
    rows = []
    for config in (int(c) for c in args.configs.split(',')):
        g = make_inputs(config, args.cache)
        for rep in range(-1, args.repeats):
            row = run_once(safepy_amd, g, config)
            if rep < 0:
                continue                                      # warm-up: code objects, pinned buffers, pandas and SciPy imports
            row['tag'], row['repeat'] = args.tag, rep
            rows.append(row)
            stages = ('compute_pvalues', 'define_top_attributes', 'define_domains', 'trim_domains')
            print('%s configs[%d] %dx%d rep %d: ' % (args.tag, config, row['n'], row['m'], rep)
                  + ', '.join('%s %.1f ms (down %.1f MB, up %.1f MB, kernels %.2f ms)'
                              % (s, row[s]['ms'], row[s]['downloaded_bytes'] / 1e6, row[s]['uploaded_bytes'] / 1e6, row[s]['kernel_busy_ms'])
                              for s in stages)
                  + '; top %d, domains %d, resident afterwards: %s, checksum %s'
                  % (row['top_attributes'], row['domains'], row['resident_after'], row['checksum']), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
