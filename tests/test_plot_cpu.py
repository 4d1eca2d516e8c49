"""The plot helpers' host parts against the real reference (tests/golden/plots.npz, make_plot_golden.py): colours, the
colour-scale normalisation and the network circle, plus `import safepy_amd` without matplotlib.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'plots.npz')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def test_import_does_not_load_matplotlib():
    code = 'import sys, safepy_amd; assert "safepy_amd.safe_io" in sys.modules; print("matplotlib" in sys.modules)'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == 'False'


def test_get_colors_matches_the_reference(golden):
    """get_colors draws from NumPy's global stream: seeded as before the reference's composite calls, the same colours."""
    from safepy_amd.safe_colormaps import get_colors
    for key in ('dom_cn', 'dom_cn_each'):
        want = golden[key + '_rgba']
        np.random.seed(int(golden[key + '_seed'][0]))
        got = get_colors('hsv', want.shape[0])
        assert np.array_equal(got, want)
    np.random.seed(int(golden['dom_contour_seed'][0]))
    assert np.array_equal(get_colors('hsv', golden['dom_contour_rgba'].shape[0]), golden['dom_contour_rgba'])
    # the first colour is black and the rest is a permutation of cmap(k / n)
    np.random.seed(0)
    c = get_colors('hsv', 7)
    assert np.array_equal(c[0], [0, 0, 0, 1]) and c.shape == (7, 4)


def test_midpoint_range_normalize():
    from safepy_amd.safe_colormaps import MidpointRangeNormalize
    norm = MidpointRangeNormalize(midrange=[np.log10(0.05), 0, -np.log10(0.05)], vmin=-3, vmax=2.5)
    x = np.array([-5, -3, np.log10(0.05), -0.5, 0, 0.7, -np.log10(0.05), 2.5, 9])
    got = norm(x)
    assert isinstance(got, np.ma.MaskedArray)
    want = np.interp(x, [-3, np.log10(0.05), 0, -np.log10(0.05), 2.5], [0, 0.25, 0.5, 0.75, 1])
    assert np.array_equal(np.asarray(got), want)
    assert np.asarray(got)[1] == 0 and np.asarray(got)[4] == 0.5 and np.asarray(got)[-1] == 1


@pytest.mark.parametrize('as_layout', [False, True])
def test_network_circle_matches_the_reference(golden, as_layout):
    """plot_network_contour's fmin circle (host SciPy) equals the circle in the reference's figures, for a networkx graph
    and for a LayoutGraph."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import networkx as nx
    from safepy_amd import LayoutGraph
    from safepy_amd.safe_io import plot_network_contour
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from make_plot_golden import build_graph
    tag = 'dom_'
    xy, eu, ev = golden[tag + 'xy'], golden[tag + 'edge_u'], golden[tag + 'edge_v']
    if as_layout:
        g = LayoutGraph(xy, eu, ev, keys=list(golden[tag + 'keys']), labels=list(golden[tag + 'labels']))
    else:
        g = build_graph(nx, xy, eu, ev, list(golden[tag + 'keys']), list(golden[tag + 'labels']))
    fig, ax = plt.subplots()
    for bg, fg in (('#000000', (1, 1, 1, 1)), ('#ffffff', (0, 0, 0, 1))):
        xf, yf, rf = plot_network_contour(g, ax, background_color=bg)
        assert np.array_equal(golden['dom_sa_a1_circles'][0], [xf, yf, rf * 1.01])
        assert np.array_equal(ax.patches[-1].get_edgecolor(), fg)
    plt.close(fig)
