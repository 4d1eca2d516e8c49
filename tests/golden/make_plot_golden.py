#!/usr/bin/env python3
"""Generate tests/golden/plots.npz by running the REAL reference's plot methods (safepy/safe.py:747-1265, safe_io.py:433-691).

Run in the build container only (needs /root/reference, networkx, pandas, matplotlib; imports the reference like
make_golden.py):

    python tests/golden/make_plot_golden.py

The two seeded 300-node randomization cases of output_files.npz (make_output_golden.py), inputs copied:
  dom_   binary attributes, define_top_attributes -> define_domains -> trim_domains first
  nes_   quantitative attributes with NaN rows
Before each plot call np.random and random are seeded (the seed is stored); each figure is stored as its artist record
(`figure_record`, which tests/test_gpu_plotting.py applies to safepy_amd's figures).  plot_composite_network_contours
raises TypeError in the reference (it draws on `ax[1]` with ax one Axes), so for it the generator stores what that method
computes before drawing: each domain's node set and grid bounds, and SciPy gaussian_kde values at a few grid points.
The reference's get_colors calls cm.get_cmap, which matplotlib 3.9 removed: it is pointed at matplotlib.colormaps (the
same colour maps).  Only data is written: no reference source travels."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SMALL = 64          # float arrays with more values are stored as a digest of their bytes (exact comparison, small file)

# (call tag, seed, method, kwargs) per case; the labels include one the network does not have
LABELS = ['n5', 'n40', 'n123', 'not-a-node']
CALLS = {
    'dom_': [
        ('net', 1, 'plot_network', {}),
        ('netlab', 2, 'plot_network', {'labels': LABELS[:3], 'kind': ['label']}),
        ('sa', 3, 'plot_sample_attributes', {}),
        ('sa_sig', 4, 'plot_sample_attributes', {'show_significant_nodes': True}),
        ('sa_raw', 5, 'plot_sample_attributes', {'show_raw_data': True}),
        ('sa_white', 6, 'plot_sample_attributes', {'background_color': '#ffffff', 'colors': ['ff0000', '0000ff'],
                                                   'save_fig': 'sample.png'}),
        ('sa_top', 7, 'plot_sample_attributes', {'attributes': 3, 'top_attributes_only': True, 'labels': LABELS}),
        ('sa_names', 8, 'plot_sample_attributes', {'attributes': ['NAME1', 'NAME0'], 'show_network': False}),
        ('cn', 9, 'plot_composite_network', {}),
        ('cn_each', 10, 'plot_composite_network', {'show_each_domain': True, 'labels': LABELS}),
    ],
    'nes_': [
        ('sa2', 11, 'plot_sample_attributes', {'attributes': 2, 'show_raw_data': True, 'show_significant_nodes': True}),
        ('sa_name', 12, 'plot_sample_attributes', {'attributes': 'NAME0', 'vmin': -3, 'vmax': 3}),
        ('sa_all', 13, 'plot_sample_attributes', {'attributes': 100, 'show_colorbar': False, 'show_network_contour': False}),
    ],
}


def _rgba(c):
    from matplotlib.colors import to_rgba
    return np.asarray(to_rgba(c), dtype=np.float64)


def figure_record(fig, prefix):
    """{name: array} of a drawn figure's artists: per axes (in the figure's order) title text and colour, facecolor, limits,
    axis and frame state, collections (type, offsets, face / edge colours, sizes, line segments), circles (centre, radius),
    texts (string, position, colour), legend texts and title, tick positions and labels of colour-bar axes.  Contour sets
    are left out (tests/test_gpu_plotting.py compares them with a tolerance)."""
    from matplotlib.contour import ContourSet
    from matplotlib.patches import Circle
    fig.canvas.draw()
    rec = {prefix + 'fig_facecolor': np.asarray(fig.get_facecolor(), dtype=np.float64),
           prefix + 'n_axes': np.array([len(fig.axes)])}
    for i, ax in enumerate(fig.axes):
        p = '%sa%d_' % (prefix, i)
        rec[p + 'title'] = np.array([ax.get_title()])
        rec[p + 'title_color'] = _rgba(ax.title.get_color())
        rec[p + 'facecolor'] = np.asarray(ax.get_facecolor(), dtype=np.float64)
        rec[p + 'lim'] = np.array([*ax.get_xlim(), *ax.get_ylim()], dtype=np.float64)
        rec[p + 'state'] = np.array([ax.axison, ax.get_frame_on()])
        colls = [c for c in ax.collections if not isinstance(c, ContourSet)]
        rec[p + 'n_coll'] = np.array([len(colls)])
        for j, c in enumerate(colls):
            q = '%sc%d_' % (p, j)
            rec[q + 'type'] = np.array([type(c).__name__])
            rec[q + 'offsets'] = np.asarray(c.get_offsets(), dtype=np.float64)
            rec[q + 'face'] = np.asarray(c.get_facecolors(), dtype=np.float64)
            rec[q + 'edge'] = np.asarray(c.get_edgecolors(), dtype=np.float64)
            if hasattr(c, 'get_sizes'):
                rec[q + 'sizes'] = np.asarray(c.get_sizes(), dtype=np.float64)
            if hasattr(c, 'get_segments'):
                segs = c.get_segments()
                rec[q + 'segments'] = np.concatenate(segs).astype(np.float64) if segs else np.zeros((0, 2))
        circles = [pa for pa in ax.patches if isinstance(pa, Circle)]
        rec[p + 'circles'] = np.array([[*pa.center, pa.radius] for pa in circles], dtype=np.float64).reshape(-1, 3)
        rec[p + 'circle_color'] = np.array([pa.get_edgecolor() for pa in circles], dtype=np.float64).reshape(-1, 4)
        rec[p + 'texts'] = np.array([t.get_text() for t in ax.texts] or [''])
        rec[p + 'text_pos'] = np.array([t.get_position() for t in ax.texts], dtype=np.float64).reshape(-1, 2)
        rec[p + 'text_color'] = np.array([_rgba(t.get_color()) for t in ax.texts]).reshape(-1, 4)
        leg = ax.get_legend()
        if leg is not None:
            rec[p + 'legend'] = np.array([leg.get_title().get_text()] + [t.get_text() for t in leg.get_texts()])
            rec[p + 'legend_color'] = np.array([_rgba(t.get_color()) for t in [leg.get_title()] + leg.get_texts()])
        if ax.get_label() == '<colorbar>':
            rec[p + 'ticks'] = np.asarray(ax.get_xticks(), dtype=np.float64)
            rec[p + 'ticklabels'] = np.array([t.get_text() for t in ax.get_xticklabels()])
            rec[p + 'xlabel'] = np.array([ax.get_xlabel()])
    return rec


def compact(rec):
    """Float arrays of more than SMALL values become 'sha1:<digest of shape and bytes>'."""
    out = {}
    for k, v in rec.items():
        v = np.asarray(v)
        if v.dtype.kind == 'f' and v.size > SMALL:
            v = np.ascontiguousarray(v, dtype=np.float64)
            h = hashlib.sha1(repr(v.shape).encode() + v.tobytes()).hexdigest()
            v = np.array(['sha1:' + h])
        out[k] = v
    return out


def build_graph(nx, xy, eu, ev, keys, labels):
    g = nx.Graph()
    for i in range(xy.shape[0]):
        g.add_node(i, x=float(xy[i, 0]), y=float(xy[i, 1]), key=keys[i], label=labels[i])
    for u, v in zip(eu, ev):
        g.add_edge(int(u), int(v))
    return g


def main():
    import random
    import tempfile
    import warnings
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.cm
    import matplotlib.pyplot as plt
    warnings.simplefilter('ignore')
    from make_golden import import_reference
    safe, _, safe_io = import_reference()
    import networkx as nx
    import pandas as pd
    from scipy.stats import gaussian_kde
    matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]

    src = dict(np.load(os.path.join(HERE, 'output_files.npz')))
    out = {}
    for tag in ('dom_', 'nes_'):
        for k in ('xy', 'edge_u', 'edge_v', 'attributes', 'names', 'keys', 'labels', 'meta'):
            out[tag + k] = src[tag + k]
        nperm, seed, domains = (int(v) for v in src[tag + 'meta'])
        xy, eu, ev = src[tag + 'xy'], src[tag + 'edge_u'], src[tag + 'edge_v']
        keys, labels = list(src[tag + 'keys']), list(src[tag + 'labels'])
        g = safe_io.calculate_edge_lengths(build_graph(nx, xy, eu, ev, keys, labels), verbose=False)
        names = list(src[tag + 'names'])
        sel = {'NAME0': names[0], 'NAME1': names[1]}
        sf = safe.SAFE(verbose=False)
        sf.graph = g
        sf.random_seed = seed
        sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
        sf.node2attribute = src[tag + 'attributes'].copy()
        sf.attributes = pd.DataFrame({'id': np.arange(len(names)), 'name': names})
        sf.compute_pvalues(how='randomization', num_permutations=nperm)
        if domains:
            sf.define_top_attributes()
            sf.define_domains()
            sf.trim_domains()
        with tempfile.TemporaryDirectory() as tmp:
            sf.output_dir = tmp
            for call, s, method, kwargs in CALLS[tag]:
                kwargs = dict(kwargs)
                if 'attributes' in kwargs:
                    a = kwargs['attributes']
                    kwargs['attributes'] = sel.get(a, a) if isinstance(a, str) else \
                        [sel[x] for x in a] if isinstance(a, list) else a
                np.random.seed(s)
                random.seed(s)
                plt.close('all')
                getattr(sf, method)(**kwargs)
                fig = plt.gcf()
                out.update(compact(figure_record(fig, '%s%s_' % (tag, call))))
                out['%s%s_seed' % (tag, call)] = np.array([s])
                if method == 'plot_composite_network':
                    out['%s%s_rgba' % (tag, call)] = np.array(sf.domains['rgba'].tolist())
                if kwargs.get('save_fig'):
                    assert os.path.exists(os.path.join(tmp, kwargs['save_fig']))
                plt.close('all')
        if domains:
            # what plot_composite_network_contours computes before it raises (safe.py:822-827)
            node_xy = safe_io.get_node_coordinates(sf.graph)
            np.random.seed(21)
            try:
                plt.close('all')
                sf.plot_composite_network_contours()
                raise AssertionError('the reference contour method was expected to raise')
            except TypeError:
                pass
            out[tag + 'contour_seed'] = np.array([21])
            out[tag + 'contour_rgba'] = np.array(sf.domains['rgba'].tolist())
            rng = np.random.default_rng(0)
            for k in range(len(sf.domains)):
                members = sf.node2domain.loc[sf.node2domain.loc[:, k] > 0].index.values
                pos3 = node_xy[members, :]
                kernel = gaussian_kde(pos3.T)
                X, Y = np.mgrid[np.min(pos3[:, 0]):np.max(pos3[:, 0]):100j, np.min(pos3[:, 1]):np.max(pos3[:, 1]):100j]
                pick = np.sort(rng.choice(X.size, 32, replace=False))
                positions = np.vstack([X.ravel()[pick], Y.ravel()[pick]])
                out['%scontour%d_members' % (tag, k)] = members.astype(np.int64)
                out['%scontour%d_bounds' % (tag, k)] = np.array([X[0, 0], X[-1, 0], Y[0, 0], Y[0, -1]])
                out['%scontour%d_pick' % (tag, k)] = pick
                out['%scontour%d_z' % (tag, k)] = kernel(positions)
            out[tag + 'n_contours'] = np.array([len(sf.domains)])
        plt.close('all')
    np.savez_compressed(os.path.join(HERE, 'plots.npz'), **out)


if __name__ == '__main__':
    main()
