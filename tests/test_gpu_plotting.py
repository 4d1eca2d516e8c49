"""The reference's plot methods on the device path against the real reference (tests/golden/plots.npz, made by
make_plot_golden.py): the seeded 300-node cases go through safepy_amd.SAFE and every figure's artist record must equal the
reference's -- offsets, colours, sizes, segments, circles, texts, legends, colour-bar ticks, limits.  The contour method,
which raises in the reference, is compared with SciPy's own densities.  Needs an MI355X."""
import os
import random
import re
import sys

import matplotlib
matplotlib.use('Agg')
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import pytest  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'plots.npz')
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_plot_golden import CALLS, build_graph, compact, figure_record  # noqa: E402


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(autouse=True)
def close_figures():
    yield
    plt.close('all')


def replay(amd, g, tag, layout_graph=False):
    """The case through safepy_amd: compute_pvalues on the device, then the domains when the case has them."""
    nperm, seed, domains = (int(v) for v in g[tag + 'meta'])
    xy, eu, ev = g[tag + 'xy'], g[tag + 'edge_u'], g[tag + 'edge_v']
    keys, labels = list(g[tag + 'keys']), list(g[tag + 'labels'])
    length = np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1))
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length, keys=keys, labels=labels)
    sf.random_seed = seed
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
    sf.load_attributes(attribute_file=g[tag + 'attributes'].copy())
    sf.attributes = pd.DataFrame({'id': np.arange(len(g[tag + 'names'])), 'name': list(g[tag + 'names'])})
    sf.compute_pvalues(how='randomization', num_permutations=nperm)
    if domains:
        sf.define_top_attributes()
        sf.define_domains()
        sf.trim_domains()
    if not layout_graph:
        import networkx as nx
        sf.graph = build_graph(nx, xy, eu, ev, keys, labels)
    return sf


def run_call(sf, g, tag, call, seed, method, kwargs):
    names = list(g[tag + 'names'])
    sel = {'NAME0': names[0], 'NAME1': names[1]}
    kwargs = dict(kwargs)
    a = kwargs.get('attributes')
    if isinstance(a, str):
        kwargs['attributes'] = sel.get(a, a)
    elif isinstance(a, list):
        kwargs['attributes'] = [sel[x] for x in a]
    np.random.seed(seed)
    random.seed(seed)
    plt.close('all')
    getattr(sf, method)(**kwargs)
    return compact(figure_record(plt.gcf(), '%s%s_' % (tag, call)))


def assert_record(got, golden, prefix):
    own = re.compile(re.escape(prefix) + r'(fig_facecolor|n_axes|a\d+_)')        # not the records of calls named prefix + '...'
    want = {k: v for k, v in golden.items() if own.match(k)}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    bad = [k for k in want if not (got[k].shape == want[k].shape and
                                   (np.array_equal(got[k], want[k], equal_nan=True) if got[k].dtype.kind == 'f'
                                    else np.array_equal(got[k], want[k])))]
    assert not bad, [(k, got[k], want[k]) for k in bad[:3]]


@pytest.mark.parametrize('tag', ['dom_', 'nes_'])
def test_figures_equal_the_reference(amd, golden, tmp_path, tag):
    from safepy_amd.safe import _DeviceResult
    sf = replay(amd, golden, tag)
    sf.output_dir = str(tmp_path)
    for call, seed, method, kwargs in CALLS[tag]:
        got = run_call(sf, golden, tag, call, seed, method, kwargs)
        assert_record(got, golden, '%s%s_' % (tag, call))
        if method == 'plot_composite_network':
            assert np.array_equal(np.array(sf.domains['rgba'].tolist()), golden['%s%s_rgba' % (tag, call)])
        if kwargs.get('save_fig'):
            assert (tmp_path / kwargs['save_fig']).stat().st_size > 0
        plt.close('all')
    if tag == 'nes_':
        # no domain step read the results: plot_sample_attributes gathered its columns on the device
        assert isinstance(sf.__dict__['_r_nes'], _DeviceResult)
        assert isinstance(sf.__dict__['_r_nes_binary'], _DeviceResult)


def test_layout_graph_figures_equal_the_reference(amd, golden):
    """The same figures with self.graph a LayoutGraph (drawn as the networkx graph of its edge list)."""
    sf = replay(amd, golden, 'dom_', layout_graph=True)
    for call, seed, method, kwargs in CALLS['dom_']:
        if call in ('net', 'netlab', 'sa_top', 'cn_each'):
            assert_record(run_call(sf, golden, 'dom_', call, seed, method, kwargs), golden, 'dom_%s_' % call)
            plt.close('all')


def test_composite_network_reads_nes_binary_in_place(amd, golden):
    """With compute_pvalues' results still on the device, plot_composite_network counts the domains from the device-resident
    nes_binary and downloads neither matrix; the figure is the reference's."""
    from safepy_amd.safe import _DeviceResult
    sf = replay(amd, golden, 'dom_')
    kept = sf.attributes.copy(), sf.node2domain.copy(), sf.domains.copy()
    sf.compute_pvalues(how='randomization', num_permutations=int(golden['dom_meta'][0]))
    sf.attributes, sf.node2domain, sf.domains = kept
    assert isinstance(sf.__dict__['_r_nes_binary'], _DeviceResult)
    for call, seed, method, kwargs in CALLS['dom_']:
        if method == 'plot_composite_network':
            assert_record(run_call(sf, golden, 'dom_', call, seed, method, kwargs), golden, 'dom_%s_' % call)
            plt.close('all')
    assert isinstance(sf.__dict__['_r_nes'], _DeviceResult)
    assert isinstance(sf.__dict__['_r_nes_binary'], _DeviceResult)


def test_composite_contours_match_scipy(amd, golden, monkeypatch):
    """plot_composite_network_contours: the domains' node sets and grids are the reference's, the device densities are
    SciPy's gaussian_kde values within 1e-12 (relative, per grid point), and the 1e-6 contours drawn from them have the same
    paths and vertex counts as the contours of SciPy's densities, vertices within 1e-9 of the domain's extent."""
    from scipy.stats import gaussian_kde
    from safepy_amd import backend as be
    sf = replay(amd, golden, 'dom_')
    captured = []
    real = be.Context.kde_grid

    def spy(self, *args):
        z, ms = real(self, *args)
        captured.append(z.copy())
        return z, ms
    monkeypatch.setattr(be.Context, 'kde_grid', spy)
    np.random.seed(int(golden['dom_contour_seed'][0]))
    sf.plot_composite_network_contours()
    assert np.array_equal(np.array(sf.domains['rgba'].tolist()), golden['dom_contour_rgba'])
    assert len(captured) == 1                                     # every domain in one launch
    n = int(golden['dom_n_contours'][0])
    fig = plt.gcf()
    sets = [c for c in fig.axes[1].collections if type(c).__name__ in ('QuadContourSet', 'ContourSet')]
    assert len(sets) == n and captured[0].shape == (n, 10000)
    node_xy = np.asarray(golden['dom_xy'])
    ref_fig, ref_ax = plt.subplots()
    for k in range(n):
        members = sf.node2domain.loc[sf.node2domain.loc[:, k] > 0].index.values
        assert np.array_equal(members, golden['dom_contour%d_members' % k])
        pos3 = node_xy[members]
        kernel = gaussian_kde(pos3.T)
        X, Y = np.mgrid[np.min(pos3[:, 0]):np.max(pos3[:, 0]):100j, np.min(pos3[:, 1]):np.max(pos3[:, 1]):100j]
        assert np.array_equal([X[0, 0], X[-1, 0], Y[0, 0], Y[0, -1]], golden['dom_contour%d_bounds' % k])
        want = kernel(np.vstack([X.ravel(), Y.ravel()]))
        pick = golden['dom_contour%d_pick' % k]
        assert np.array_equal(want[pick], golden['dom_contour%d_z' % k])      # SciPy here is the generator's SciPy
        got = captured[0][k]
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), np.max(np.abs(got - want) / np.abs(want))
        ref = ref_ax.contour(X, Y, want.reshape(X.shape), [1e-6], colors=sf.domains.loc[k, 'rgba'], alpha=1)
        gp, rp = sets[k].get_paths(), ref.get_paths()
        assert len(gp) == len(rp)
        extent = max(np.ptp(pos3[:, 0]), np.ptp(pos3[:, 1]))
        for a, b in zip(gp, rp):
            assert a.vertices.shape == b.vertices.shape and np.array_equal(a.codes, b.codes)
            assert np.max(np.abs(a.vertices - b.vertices), initial=0) <= 1e-9 * extent
        assert np.array_equal(sets[k].get_edgecolor(), ref.get_edgecolor())
    plt.close(ref_fig)
