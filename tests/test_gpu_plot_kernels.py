"""The plot kernels (plot.hip) against their host definitions: k_kde_grid against SciPy's gaussian_kde.evaluate,
k_domain_counts against nes_binary @ onehot, k_gather_columns against slicing.  Needs an MI355X."""
import math

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.stats import gaussian_kde

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import safepy_amd
    from safepy_amd import backend as be
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return be.Context.default(0)


def kde_inputs(sets, grids):
    """safe_kde_grid's inputs for SciPy kernels of the point sets (each [n, 2]) at the grids (each [G, 2]) -- the whitening
    and normalisation gaussian_kernel_estimate does -- and SciPy's own values."""
    offsets, pts, w, norm, xi, want = [0], [], [], [], [], []
    for p, x in zip(sets, grids):
        k = gaussian_kde(p.T)
        cho = k.cho_cov
        pts.append(solve_triangular(cho, k.dataset, lower=True).T)
        w.append(k.weights)
        norm.append(math.pow(2 * math.pi, -1.0) / cho[0, 0] / cho[1, 1])
        xi.append(solve_triangular(cho, np.ascontiguousarray(x.T), lower=True).T)
        want.append(k.evaluate(np.ascontiguousarray(x.T)))
        offsets.append(offsets[-1] + p.shape[0])
    return offsets, np.concatenate(pts), np.concatenate(w), norm, np.stack(xi), np.stack(want)


def check_kde(ctx, sets, g, rng):
    grids = []
    for p in sets:
        lo, hi = p.min(axis=0), p.max(axis=0)
        grids.append(lo + (hi - lo) * rng.uniform(-0.1, 1.1, size=(g, 2)))
    offsets, pts, w, norm, xi, want = kde_inputs(sets, grids)
    z, ms = ctx.kde_grid(offsets, pts, w, norm, xi)
    assert z.shape == want.shape and ms >= 0
    err = np.abs(z - want)
    assert np.all(err <= 1e-12 * np.abs(want)), float(np.max(err / np.maximum(np.abs(want), 1e-300)))   # (0 where SciPy's is 0)
    z2, _ = ctx.kde_grid(offsets, pts, w, norm, xi)
    assert np.array_equal(z, z2)                                  # no atomics: the same bits on every run
    return int(np.sum(z == want)), z.size


def test_kde_grid_against_scipy(ctx):
    rng = np.random.default_rng(7)
    equal = total = 0
    # one launch, several sets of 3 .. 20 000 points; the large one is summed in chunks
    sets = [rng.standard_normal((3, 2)),
            rng.standard_normal((17, 2)) * [1.0, 0.01],                                   # skewed covariance
            np.repeat(rng.standard_normal((40, 2)), 3, axis=0) + rng.standard_normal((120, 2)) * 1e-3,   # duplicates
            rng.standard_normal((257, 2)) @ np.array([[1.0, 0.9], [0.0, 0.2]]),
            rng.standard_normal((20000, 2))]
    sets[2][:5] = sets[2][5]                                      # exact duplicate points
    e, t = check_kde(ctx, sets, 9999, rng)                        # odd grid
    equal += e
    total += t
    # many sets: enough grid points to fill the device, one thread per grid point over all the points in order
    e, t = check_kde(ctx, [rng.standard_normal((int(n), 2)) for n in rng.integers(3, 2000, size=60)], 10000, rng)
    equal += e
    total += t
    # one set alone (the chunked path)
    e, t = check_kde(ctx, [rng.standard_normal((5000, 2)) * [3.0, 0.5]], 101, rng)
    equal += e
    total += t
    print('k_kde_grid: %d of %d values bit-equal to SciPy (%.1f %%)' % (equal, total, 100.0 * equal / total))


def test_kde_grid_edge_shapes(ctx):
    z, _ = ctx.kde_grid([0], np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros((0, 5, 2)))
    assert z.shape == (0, 5)
    z, _ = ctx.kde_grid([0, 0, 2], np.ones((2, 2)), np.ones(2), [1.0, 2.0], np.zeros((2, 3, 2)))
    assert np.array_equal(z[0], np.zeros(3))                      # an empty set sums to 0
    assert np.allclose(z[1], 4 * math.exp(-1.0), rtol=1e-15, atol=0)     # (device exp: within an ulp of the host's)


@pytest.mark.parametrize('n,m,d', [(257, 1000, 1), (300, 4373, 7), (64, 6000, 4096)])
def test_domain_counts_exact(ctx, n, m, d):
    rng = np.random.default_rng(n + m + d)
    x = (rng.uniform(size=(n, m)) < 0.3).astype(np.float64)
    dom = rng.integers(0, d, size=m)
    dom[:min(d, m)] = np.arange(min(d, m))
    onehot = (dom[:, None] == np.arange(d)[None, :]).astype(np.float64)
    want = x @ onehot
    got, ms = ctx.domain_counts(x, dom, d)                        # host input, uploaded
    assert np.array_equal(got, want) and ms >= 0
    buf = ctx.alloc_f64(n, m)                                     # device-resident input, read in place
    try:
        buf.upload(x)
        got, _ = ctx.domain_counts(buf.ptr, dom, d, n, m)
    finally:
        buf.free()
    assert np.array_equal(got, want)


def test_domain_counts_limits(ctx):
    from safepy_amd import SafeHipError
    x = np.ones((3, 5))
    with pytest.raises(SafeHipError, match='limit of 4096'):
        ctx.domain_counts(x, np.zeros(5), 4097)
    with pytest.raises(SafeHipError, match='not in'):
        ctx.domain_counts(x, np.array([0, 1, 2, 3, 4]), 4)
    x[1, 2] = np.nan                                              # NaN is skipped, like pandas' sum
    got, _ = ctx.domain_counts(x, np.array([0, 0, 0, 1, 1]), 2)
    assert np.array_equal(got, [[3, 2], [2, 2], [3, 2]])


def test_gather_columns_exact(ctx):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1001, 77))
    x[5, 3] = np.nan
    cols = [3, 0, 76, 3, 40]
    got, _ = ctx.gather_columns(x, cols)
    assert np.array_equal(got, x[:, cols], equal_nan=True)
    buf = ctx.alloc_f64(*x.shape)
    try:
        buf.upload(x)
        got, _ = ctx.gather_columns(buf.ptr, [76], *x.shape)
        assert np.array_equal(got[:, 0], x[:, 76])
        from safepy_amd import SafeHipError
        with pytest.raises(SafeHipError, match='out of'):
            ctx.gather_columns(buf.ptr, [77], *x.shape)
    finally:
        buf.free()


def test_contour_plot_does_not_evaluate_on_the_host(ctx, monkeypatch):
    """plot_composite_network_contours builds SciPy's kernels but evaluates them on the device only."""
    import os
    import sys
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_plotting import replay
    import safepy_amd

    def refuse(self, points):
        raise AssertionError('gaussian_kde.evaluate ran on the host')
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plots.npz')))
    sf = replay(safepy_amd, g, 'dom_')
    monkeypatch.setattr(gaussian_kde, 'evaluate', refuse)
    monkeypatch.setattr(gaussian_kde, '__call__', refuse)
    try:
        sf.plot_composite_network_contours()
        assert len(plt.gcf().axes[1].collections) == len(sf.domains)
    finally:
        plt.close('all')
