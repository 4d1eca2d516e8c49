"""Time of the device parts of the plot methods (plot.hip), one line per measurement:

  kde     plot_composite_network_contours' density grids: k_kde_grid for every domain in one launch (HIP events) and the
          whole method call (host clock: SciPy kernels, launch, matplotlib contours, network drawing), against SciPy's
          gaussian_kde evaluated on the same grids on this host's CPU.  Domain sets shaped like configs[1] (3971 nodes,
          domain 0 holding most of them) and like N = 20 000.
  counts  plot_composite_network's per-node domain counts: k_domain_counts over a device-resident 0/1 [N, M] matrix
          (HIP events; call = host clock incl. the [N, D] download) against pandas' groupby(level='domain', axis=1).sum(),
          at configs[1] (3971 x 4373) and configs[3] (20 000 x 10 000).
  sample  plot_sample_attributes(attributes=1) on a device-resident configs[3] nes (the whole call, host clock) and the
          column gather alone.

usage: python tools/plot_time.py [--skip-host] [--repeats 2]
--skip-host: leave out the SciPy / pandas baselines (minutes of CPU at the large shapes)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def domain_case(rng, n, sizes):
    """A SAFE object with a LayoutGraph of n nodes (no edges) and domains: domain 0 = the nodes no other domain takes,
    domain k = a cluster of sizes[k - 1] nodes around a random centre."""
    import pandas as pd
    import safepy_amd
    xy = rng.uniform(size=(n, 2))
    member = np.zeros((n, len(sizes) + 1), dtype=np.float64)
    free = np.ones(n, dtype=bool)
    for k, s in enumerate(sizes, start=1):
        c = xy[rng.integers(n)]
        order = np.argsort(((xy - c) ** 2).sum(axis=1))
        take = order[free[order]][:s]
        member[take, k] = 1
        free[take] = False
    member[free, 0] = 1
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(xy)
    d = len(sizes) + 1
    sf.attributes = pd.DataFrame({'id': np.arange(d), 'name': ['a%d' % k for k in range(d)], 'domain': np.arange(d)})
    sf.node2domain = pd.DataFrame(member, columns=pd.Index(np.arange(d), name='domain'))
    sf.node2domain['primary_domain'] = np.argmax(member, axis=1)
    sf.domains = pd.DataFrame({'id': np.arange(d), 'label': ['domain %d' % k for k in range(d)]})
    return sf, xy, member


def time_kde(args, rng, n, sizes, tag):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from scipy.stats import gaussian_kde
    from safepy_amd import backend as be
    sf, xy, member = domain_case(rng, n, sizes)
    kernel_ms = []
    real = be.Context.kde_grid

    def spy(self, *a):
        z, ms = real(self, *a)
        kernel_ms.append(ms)
        return z, ms
    be.Context.kde_grid = spy
    try:
        calls = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            sf.plot_composite_network_contours()
            calls.append((time.perf_counter() - t0) * 1e3)
            plt.close('all')
    finally:
        be.Context.kde_grid = real
    host = float('nan')
    if not args.skip_host:
        t0 = time.perf_counter()
        for k in range(member.shape[1]):
            pos3 = xy[member[:, k] > 0]
            X, Y = np.mgrid[pos3[:, 0].min():pos3[:, 0].max():100j, pos3[:, 1].min():pos3[:, 1].max():100j]
            gaussian_kde(pos3.T)(np.vstack([X.ravel(), Y.ravel()]))
        host = (time.perf_counter() - t0) * 1e3
    print('kde %s: N=%d domains=%d (domain 0: %d nodes) kernel %.2f ms, whole call %.1f ms, SciPy evaluate on the host %.0f ms'
          % (tag, n, member.shape[1], int(member[:, 0].sum()), min(kernel_ms), min(calls), host), flush=True)


def time_counts(args, rng, n, m, d):
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    x = (rng.uniform(size=(n, m)) < 0.05).astype(np.float64)
    dom = np.sort(rng.integers(0, d, size=m))
    buf = ctx.alloc_f64(n, m)
    try:
        buf.upload(x)
        ctx.domain_counts(buf.ptr, dom, d, n, m)
        ks, calls = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            got, ms = ctx.domain_counts(buf.ptr, dom, d, n, m)
            calls.append((time.perf_counter() - t0) * 1e3)
            ks.append(ms)
    finally:
        buf.free()
    host = float('nan')
    if not args.skip_host:
        import pandas as pd
        import warnings
        warnings.simplefilter('ignore')
        frame = pd.DataFrame(x, columns=[np.arange(m), dom])
        frame.columns.names = [None, 'domain']
        t0 = time.perf_counter()
        want = frame.T.groupby(level='domain').sum().T                # groupby(level='domain', axis=1).sum() (axis=1 is deprecated)
        host = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(want.values, got)
    gb = n * m * 8 / 1e9
    print('counts %dx%d D=%d: kernel %.3f ms (%.2f TB/s of the %.2f GB read), call %.2f ms; pandas groupby on the host %.0f ms'
          % (n, m, d, min(ks), gb / min(ks), gb, min(calls), host), flush=True)


def time_sample(args, rng, n, m):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import pandas as pd
    import safepy_amd
    from safepy_amd.safe import _DeviceResult
    ctx = safepy_amd.Context.default(0)
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(rng.uniform(size=(n, 2)))
    sf.attributes = pd.DataFrame({'id': np.arange(m), 'name': ['attribute %d' % j for j in range(m)]})
    buf = ctx.alloc_f64(n, m)
    block = -np.log10(rng.integers(1, 1001, size=(n, 1000)) / 1000.0)
    full = np.tile(block, (1, -(-m // 1000)))[:, :m]
    buf.upload(np.ascontiguousarray(full))
    del full
    sf.__dict__['_r_nes'] = _DeviceResult(buf, (n, m))
    calls = []
    for s in range(args.repeats):
        np.random.seed(s)
        t0 = time.perf_counter()
        sf.plot_sample_attributes(show_network_contour=True)
        calls.append((time.perf_counter() - t0) * 1e3)
        plt.close('all')
    assert isinstance(sf.__dict__['_r_nes'], _DeviceResult)
    _, ms = ctx.gather_columns(buf.ptr, [m // 2], n, m)
    print('sample %dx%d (device-resident nes): plot_sample_attributes(attributes=1) %.0f ms whole call, column gather kernel '
          '%.3f ms (instead of a %.2f GB download)' % (n, m, min(calls), ms, n * m * 8 / 1e9), flush=True)
    sf.__dict__['_r_nes'].drop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--repeats', type=int, default=2)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    time_kde(args, rng, 3971, [int(s) for s in rng.integers(20, 200, size=24)], 'configs[1]')
    time_kde(args, rng, 20000, [int(s) for s in rng.integers(50, 600, size=40)], 'N=20000')
    time_counts(args, rng, 3971, 4373, 25)
    time_counts(args, rng, 20000, 10000, 41)
    time_sample(args, rng, 20000, 10000)


if __name__ == '__main__':
    main()
