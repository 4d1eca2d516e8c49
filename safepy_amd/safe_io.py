"""Callers and data formats either side of the hot path.

Host-side mirror of the pieces of `safepy/safe_io.py` that feed `define_neighborhoods()` /
`compute_pvalues()`, with their data-parallel steps on the device:

  calculate_edge_lengths      safe_io.py:311-333   per-edge kernel instead of the N x N pdist matrix,
                                                   the dense adjacency and the Python ndenumerate loop
  load_network_from_scatter   safe_io.py:271-285   (host parse, pandas like the reference)
  load_network_from_txt       safe_io.py:30-121    edge lists (.txt / .tsv, optionally .gz): host parse with pandas
                                                   like the reference, then the layout and the edge lengths
  apply_network_layout        safe_io.py:288-308   'spring_embedded': networkx 3.4.2's spring_layout(k=0.2,
                                                   iterations=100) on the device (layout.hip), coordinates equal
                                                   to networkx's bit for bit
  kamada_kawai_layout         safe_io.py:288-308   the other layout, nx.kamada_kawai_layout: all-pairs distances and
                                                   the cost function + gradient on the device (kk.hip), SciPy's
                                                   L-BFGS-B on the host as in networkx; coordinates equal to
                                                   networkx's bit for bit.  load_network_from_txt(layout=
                                                   'kamada_kawai') uses it
  euclidean_pseudo_network    safe.py:302-309      the `.scatter` pseudo-network: all-pairs distance +
                                                   threshold kernel, edges read back from the device CSR
  read_attributes             safe_io.py:336-430   parse with pandas like the reference; the alignment to
                                                   network node order (`reindex` + `.values`) and the value
                                                   census of the log run on the device, and the aligned
                                                   matrix can stay resident for compute_pvalues

and the plot helpers of the reference (matplotlib is imported inside them only, so `import safepy_amd` does
not load it):

  plot_network                safe_io.py:433-486   nx.draw of the network (a LayoutGraph is drawn as the networkx
                                                   graph of its edge list)
  plot_network_contour        safe_io.py:489-529   convex hull + fmin circle fit, on the host
  mark_nodes                  safe_io.py:589-646
  get_node_coordinates        safe_io.py:649-691   both branches (labels=[] and the label lookup)

The plot methods of SAFE put their data-parallel parts on the device (plot.hip: domain density grids, domain counts,
column reads of the device-resident results).  The Cytoscape / MATLAB loaders stay out of scope.
There is no CPU fallback: every function that computes needs a HIP device.
"""
import logging
import os
import pickle

import numpy as np

from . import backend as be


def _xy_in_node_order(G):
    x = np.array([v for _, v in G.nodes.data('x')], dtype=np.float64)
    y = np.array([v for _, v in G.nodes.data('y')], dtype=np.float64)
    return np.stack([x, y], axis=1) if len(x) else np.zeros((0, 2))


def get_node_coordinates(graph, labels=[]):
    """safe_io.py:649-691.  labels empty: [N,2] (x, y) in node order.  Otherwise ([k,2] coordinates, labels found): the
    nodes whose 'label' is one of `labels`, in the order of `labels` (a label several nodes share names the last of them,
    as the reference's label -> node dictionary does); the labels not found are logged."""
    from .safe import LayoutGraph
    xy = graph.xy if isinstance(graph, LayoutGraph) else _xy_in_node_order(graph)
    if len(labels) == 0:
        return xy
    if isinstance(graph, LayoutGraph):
        node_of = {lab: i for i, lab in enumerate(graph.labels)}
    else:
        import networkx as nx
        node_of = {lab: node for node, lab in nx.get_node_attributes(graph, 'label').items()}
    found = [lab for lab in labels if lab in node_of]
    missing = [lab for lab in labels if lab not in node_of]
    if missing:
        logging.warning('These labels are missing from the network (case sensitive): %s' % ', '.join(missing))
    # the reference indexes the node-order x / y lists with the node id (ids 0..N-1)
    idx = [node_of[lab] for lab in found]
    return np.vstack([xy[idx, 0].tolist(), xy[idx, 1].tolist()]).T, found


def _as_networkx(graph):
    """A networkx graph to draw: the graph itself, or one built from a LayoutGraph (nodes 0..N-1, its edges in order)."""
    from .safe import LayoutGraph
    if not isinstance(graph, LayoutGraph):
        return graph
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(graph.number_of_nodes()))
    g.add_edges_from(zip(graph.edge_u.tolist(), graph.edge_v.tolist()))
    return g


def plot_network(G, ax=None, foreground_color='#ffffff', background_color='#000000', random_sampling_edges_min=30000,
                 title='Network', node_size=10, alpha=0.2):
    """safe_io.py:433-486: the network drawn with nx.draw at the node coordinates; with random_sampling_edges_min edges or
    more, a tenth of them drawn with Python's global `random`.  A new 20 x 10 figure when ax is None.  Returns the axes.
    (Like the reference, it turns off the axis of pyplot's current axes too: plt.axis('off').)"""
    import random
    import matplotlib.pyplot as plt
    import networkx as nx
    if background_color == '#ffffff':
        foreground_color = '#000000'
    node_xy = get_node_coordinates(G)
    fig = None
    if ax is None:
        fig, ax = plt.subplots(figsize=(20, 10), facecolor=background_color, edgecolor=foreground_color)
        fig.set_facecolor(background_color)
    g = _as_networkx(G)
    edges = tuple(g.edges())
    if len(edges) >= random_sampling_edges_min:
        logging.warning('Edges are randomly sampled because the network (edges=%d) is too big (random_sampling_edges_min=%d).'
                        % (len(edges), random_sampling_edges_min))
        edges = random.sample(edges, int(len(edges) * 0.1))
    nx.draw(g, ax=ax, pos=node_xy, edgelist=edges, node_color=foreground_color, edge_color=foreground_color,
            node_size=node_size, width=1, alpha=alpha)
    ax.set_aspect('equal')
    ax.set_facecolor(background_color)
    ax.grid(False)
    ax.invert_yaxis()
    ax.margins(0.1, 0.1)
    ax.set_title(title, color=foreground_color)
    plt.axis('off')
    if fig is not None:
        fig.set_facecolor(background_color)
    return ax


def plot_network_contour(graph, ax, background_color='#000000'):
    """safe_io.py:489-529: a circle around the network -- the circle least-squares fitted (scipy.optimize.fmin, started
    at the hull vertices' centroid and mean radius) to the vertices of the nodes' convex hull -- drawn with 1 % more
    radius.  Returns (xf, yf, rf)."""
    import matplotlib.pyplot as plt
    from scipy.optimize import fmin
    from scipy.spatial import ConvexHull
    from .safe import LayoutGraph
    foreground_color = '#000000' if background_color == '#ffffff' else '#ffffff'
    xy = get_node_coordinates(graph)
    nodes = range(xy.shape[0]) if isinstance(graph, LayoutGraph) else list(graph.nodes)
    pos = dict(zip(nodes, xy))
    hull = ConvexHull(xy)
    # the reference looks the hull's vertex positions up as node ids
    vx = np.array([pos.get(v)[0] for v in hull.vertices])
    vy = np.array([pos.get(v)[1] for v in hull.vertices])
    xm, ym = np.nanmean(vx), np.nanmean(vy)
    rm = np.nanmean(np.sqrt((vx - xm) ** 2 + (vy - ym) ** 2))

    def err(p):
        w, v, r = p
        return (np.array([np.linalg.norm([x - w, y - v]) - r for x, y in zip(vx, vy)]) ** 2).sum()

    xf, yf, rf = fmin(err, [xm, ym, rm], disp=False)
    ax.add_patch(plt.Circle((xf, yf), radius=rf * 1.01, color=foreground_color, linewidth=1, fill=False))
    return xf, yf, rf


def mark_nodes(x, y, kind, ax=None, foreground_color='#ffffff', background_color='#000000', labels=None, label_va='center',
               legend_label=None, test=False, **kws):
    """safe_io.py:589-646: kind 'mark' scatters the points (kws go to scatter), 'label' writes labels[i] at each point
    (bold, size 14, white on '#000000', else black); legend_label adds a 'Significance' legend for the marks.
    ax None: pyplot's current axes.  Returns the axes."""
    import matplotlib.pyplot as plt
    if ax is None:
        ax = plt.gca()
    if isinstance(kind, str):
        kind = [kind]
    marks = None
    if 'mark' in kind:
        marks = ax.scatter(x, y, **kws)
    if 'label' in kind:
        if test:
            print(x, y, labels)
        assert len(x) == len(labels), f"len(x)!=len(labels): {len(x)}!={len(labels)}"
        if test:
            ax.plot(x, y, 'r*')
        font = {'color': 'white' if background_color == '#000000' else 'k', 'size': 14, 'weight': 'bold'}
        for i, label in enumerate(labels):
            ax.text(x[i], y[i], label, fontdict=font, ha='center', va=label_va)
    if legend_label is not None:
        _legend(ax, [marks], [legend_label], 'Significance', foreground_color, background_color)
    return ax


def _legend(ax, handles, texts, title, foreground_color, background_color):
    """The legends of the plot methods (safe_io.py:633-642, safe.py:1163-1172): upper left, texts and title in the
    foreground colour on the background colour."""
    leg = ax.legend(handles, texts, loc='upper left', bbox_to_anchor=(0, 1), title=title, scatterpoints=1, fancybox=False,
                    facecolor=background_color, edgecolor=background_color)
    for t in leg.get_texts():
        t.set_color(foreground_color)
    leg.get_title().set_color(foreground_color)
    return leg


def calculate_edge_lengths(G, verbose=True, device=0):
    """safepy/safe_io.py:311-333: sets edge attribute 'length' = Euclidean distance between the
    end points (times the edge's 'weight' when it has one -- the reference multiplies the distance
    matrix by `nx.adjacency_matrix(G)`, whose entries are the weights -- and edges of weight 0 get
    no length).  Node ids must be 0..N-1 in node order: the reference addresses edges by matrix
    index (`np.ndenumerate`), which only names the right edge under that numbering.
    Accepts a networkx graph or a `LayoutGraph`; returns it."""
    from .safe import LayoutGraph
    if verbose:
        logging.info('Calculating edge lengths...')
    ctx = be.Context.default(device)
    if isinstance(G, LayoutGraph):
        d = ctx.edge_lengths(G.xy, G.edge_u, G.edge_v) if G.edge_u.size else np.zeros(0)
        if G.weight is not None:
            d = d * G.weight
        G.length = d
        return G
    nodes = list(G)
    if nodes != list(range(len(nodes))):
        raise ValueError('calculate_edge_lengths: node ids must be 0..N-1 in node order '
                         '(the reference indexes edges by adjacency-matrix position, safe_io.py:330)')
    xy = _xy_in_node_order(G)
    edges = list(G.edges(data='weight', default=1))
    if not edges:
        return G
    eu = np.fromiter((e[0] for e in edges), dtype=np.int64, count=len(edges))
    ev = np.fromiter((e[1] for e in edges), dtype=np.int64, count=len(edges))
    w = np.array([e[2] for e in edges], dtype=np.float64)
    d = ctx.edge_lengths(xy, eu, ev)
    with np.errstate(invalid='ignore'):
        val = d * w                                    # np.multiply(node_distances, adjacency_matrix), safe_io.py:328
    keep = (w != 0) & ~np.isnan(val)                   # zero entries of the adjacency become NaN and are dropped (:326, :330)
    for u, v, x, k in zip(eu.tolist(), ev.tolist(), val.tolist(), keep.tolist()):
        if k:
            G[u][v]['length'] = x
    return G


def load_network_from_gpickle(filename, verbose=True):
    """safepy/safe_io.py:124-130."""
    with open(os.path.expanduser(filename), 'rb') as f:
        return pickle.load(f)


def _random_state(seed):
    """networkx's np_random_state conversion: None -> NumPy's global RandomState (so the caller's stream
    advances as under the reference), an int -> RandomState(seed), a RandomState -> itself."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, np.random.RandomState):
        return seed
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return np.random.RandomState(seed)
    raise ValueError('%r cannot be used to create a numpy.random.RandomState instance' % (seed,))


def _rescale_layout(pos, scale=1, center=None):
    """networkx rescale_layout(pos, scale=scale) (drawing/layout.py), in the array's dtype, then `+ center`."""
    pos -= pos.mean(axis=0)
    lim = np.abs(pos).max()
    if lim > 0:
        pos *= scale / lim
    return pos + (np.zeros(2) if center is None else center)


def _spring_layout(n, row_ptr, col, weight, seed, device):
    """nx.spring_layout(G, k=0.2, iterations=100, seed=seed) for a graph of n nodes given as CSR (node order):
    [n,2] f64.  networkx draws the initial positions only for n >= 2 and runs its f64 form below 500 nodes,
    the f32 one from 500 (layout.py: spring_layout)."""
    if n == 0:
        return np.zeros((0, 2))
    if n == 1:
        return np.zeros((1, 2))
    pos0 = _random_state(seed).rand(n, 2)
    dtype = np.float32 if n >= 500 else np.float64
    pos, _ = be.Context.default(device).layout_spring(row_ptr, col, weight, pos0, k=0.2, iterations=100,
                                                      threshold=1e-4, dtype=dtype)
    return _rescale_layout(np.ascontiguousarray(pos))


def kamada_kawai_layout(G, dist=None, pos=None, weight='weight', scale=1, center=None, device=0):
    """nx.kamada_kawai_layout(G, dist, pos, weight, scale, center) for dim = 2 (the layout safepy/safe_io.py:288-308 applies by
    default), coordinates equal to networkx 3.4.2's bit for bit: the cost function and its gradient are evaluated on
    the device (kk.hip) in NumPy's rounding and summation order, and SciPy's L-BFGS-B drives them from the host exactly as
    _kamada_kawai_solve does.

    G: an undirected networkx graph -- returns {node: position} like networkx -- or a `LayoutGraph` -- sets its `.xy` and
    returns it.  dist: None = all-pairs shortest path lengths over edge attribute `weight` (missing = 1; None = every edge
    1; a LayoutGraph: its `.weight`), computed and kept on the device; or networkx's two-level dict {node: {node: distance}}
    (missing pairs count as 1e6).  pos: None = nx.circular_layout, or {node: (x, y)}.  No nodes: {}."""
    import networkx as nx
    import scipy.optimize
    from .safe import LayoutGraph
    center = np.zeros(2) if center is None else np.asarray(center)
    if len(center) != 2:
        raise ValueError('length of center coordinates must match dimension of layout')
    is_layout = isinstance(G, LayoutGraph)
    if not is_layout and (G.is_directed() or G.is_multigraph()):
        raise NotImplementedError('kamada_kawai_layout: directed graphs and multigraphs are not supported')
    nodes = list(range(G.number_of_nodes())) if is_layout else list(G)
    n = len(nodes)
    if n == 0:
        if is_layout:
            G.xy = np.zeros((0, 2))
            return G
        return {}
    if n > be.KamadaKawai.MAX_NODES:
        raise be._lib.SafeHipError(be._lib.E_UNSUPPORTED, 'kamada_kawai_layout: %d nodes exceed the limit of %d'
                              % (n, be.KamadaKawai.MAX_NODES))
    ctx = be.Context.default(device)
    if dist is None:
        if is_layout:
            eu, ev = G.edge_u, G.edge_v
            ew = None if weight is None or G.weight is None else G.weight
        else:
            index = {node: i for i, node in enumerate(nodes)}
            edges = list(G.edges(data=True))
            eu = np.fromiter((index[e[0]] for e in edges), dtype=np.int64, count=len(edges))
            ev = np.fromiter((index[e[1]] for e in edges), dtype=np.int64, count=len(edges))
            ew = None
            if weight is not None and any(weight in e[2] for e in edges):
                ew = np.array([e[2].get(weight, 1) for e in edges], dtype=np.float64)
        nbr = be.Neighborhoods.shortpath(ctx, n, eu, ev, ew, np.inf, keep_distances=True)
        try:
            kk = be.KamadaKawai.from_neighborhoods(ctx, nbr)
        finally:
            nbr.close()
    else:
        dist_mtx = 1e6 * np.ones((n, n))
        for row, nr in enumerate(nodes):
            if nr not in dist:
                continue
            rdist = dist[nr]
            for col, nc in enumerate(nodes):
                if nc in rdist:
                    dist_mtx[row][col] = rdist[nc]
        kk = be.KamadaKawai.from_distances(ctx, dist_mtx)
    try:
        if pos is None:
            pos = nx.circular_layout(nodes)
        pos_arr = np.array([pos[node] for node in nodes], dtype=np.float64)
        result = scipy.optimize.minimize(kk.evaluate, pos_arr.ravel(), method='L-BFGS-B', jac=True)
    finally:
        kk.close()
    xy = _rescale_layout(result.x.reshape((-1, 2)), scale=scale, center=center)
    if is_layout:
        G.xy = np.ascontiguousarray(xy)
        return G
    return dict(zip(nodes, xy))


def apply_network_layout(G, layout='kamada_kawai', seed=None, verbose=True, device=0):
    """safepy/safe_io.py:288-308.  'spring_embedded' runs nx.spring_layout(G, k=0.2, iterations=100,
    seed=seed) on the device: the adjacency is the graph's, in node order, with edge attribute 'weight'
    (default 1); the initial positions are drawn with NumPy from `seed` (None = the global stream, an int,
    or a RandomState).  Sets node attributes 'x' / 'y' (a `LayoutGraph`: its `.xy`) and returns G.
    'kamada_kawai' still raises here: the layout itself is `kamada_kawai_layout` (which load_network_from_txt calls for
    layout='kamada_kawai'); routing this function's own default to it is left to a later change."""
    from .safe import LayoutGraph
    if layout == 'kamada_kawai':
        raise NotImplementedError("apply_network_layout does not run the Kamada-Kawai layout; call "
                                  "safe_io.kamada_kawai_layout(G), or use layout='spring_embedded'")
    if layout != 'spring_embedded':
        raise ValueError("unknown layout %r (supported: 'spring_embedded')" % (layout,))
    if verbose:
        logging.info('Applying the spring-embedded network layout...')
    import scipy.sparse as sps
    if isinstance(G, LayoutGraph):
        n = G.number_of_nodes()
        w = np.ones(G.edge_u.size) if G.weight is None else G.weight
        loops = G.edge_u == G.edge_v
        rows = np.concatenate([G.edge_u, G.edge_v[~loops]])
        cols = np.concatenate([G.edge_v, G.edge_u[~loops]])
        A = sps.csr_array((np.concatenate([w, w[~loops]]), (rows, cols)), shape=(n, n))
    else:
        import networkx as nx
        n = G.number_of_nodes()
        A = nx.to_scipy_sparse_array(G, weight='weight', dtype=np.float64, format='csr') if n else None
    if n >= 2:
        A.sum_duplicates()
        A.sort_indices()
        pos = _spring_layout(n, A.indptr, A.indices, A.data, seed, device)
    else:
        pos = _spring_layout(n, None, None, None, seed, device)
    if isinstance(G, LayoutGraph):
        G.xy = np.ascontiguousarray(pos)
        return G
    nodes = list(G)
    for name, values in (('x', pos[:, 0]), ('y', pos[:, 1])):
        for node, v in zip(nodes, values):
            G.nodes[node][name] = v
    return G


def _read_edge_list(filename):
    """The parse of safe_io.py:47-107: (edge table with node_index1 / node_index2, node table in index order
    with node_label1 / node_key1).  '.txt' has no header, '.tsv' one; 3 columns (key1, key2, weight; the
    labels are the keys) or 5 (label1, key1, label2, key2, weight); '.gz' compressed either way."""
    import gzip
    import pandas as pd
    from pathlib import Path
    filename = os.path.expanduser(filename)
    opener = gzip.open if Path(filename).suffix == '.gz' else open
    with opener(filename, 'rt') as f:
        num_cols = len(f.readline().split('\t'))
    ext = Path(filename).suffixes[0]
    if ext == '.txt':
        kws = dict(header=None)
    elif ext == '.tsv':
        kws = dict(header=0, names=range(num_cols))
    else:
        raise ValueError(f'extension {ext} not supported')
    if num_cols == 3:
        data = pd.read_table(filename, sep='\t', dtype={0: str, 1: str, 2: float}, **kws)
        data = data.rename(columns={0: 'node_key1', 1: 'node_key2', 2: 'edge_weight'})
        data['node_label1'] = data['node_key1']
        data['node_label2'] = data['node_key2']
    elif num_cols == 5:
        data = pd.read_table(filename, sep='\t', **kws)
        data = data.rename(columns={0: 'node_label1', 1: 'node_key1', 2: 'node_label2', 3: 'node_key2', 4: 'edge_weight'})
    else:
        raise ValueError('Unknown network file format. 3 or 5 columns are expected.')
    t1 = data[['node_label1', 'node_key1']]
    t2 = data[['node_label2', 'node_key2']].rename(columns={'node_label2': 'node_label1', 'node_key2': 'node_key1'})
    nodes = pd.concat([t1, t2], ignore_index=True).drop_duplicates().reset_index(drop=True)
    by_label = nodes.reset_index().set_index('node_label1')
    data['node_index1'] = by_label.loc[data['node_label1'], 'index'].values
    data['node_index2'] = by_label.loc[data['node_label2'], 'index'].values
    return data, nodes


def load_network_from_txt(filename, layout='spring_embedded', node_key_attribute='key', seed=None, verbose=True,
                          device=0):
    """safepy/safe_io.py:30-121: a tab-separated edge list -> networkx graph with nodes 0..N-1 numbered in order
    of first appearance, node attributes 'label' and `node_key_attribute`, unweighted edges (the file's weight
    column is read but not attached, as in the reference), the layout ('spring_embedded': apply_network_layout;
    'kamada_kawai': kamada_kawai_layout; both on the device) and edge 'length' (calculate_edge_lengths)."""
    import networkx as nx
    data, nodes = _read_edge_list(filename)
    G = nx.Graph()
    n = len(nodes)
    G.add_nodes_from(range(n))
    nx.set_node_attributes(G, dict(zip(range(n), nodes['node_label1'].to_numpy())), 'label')
    nx.set_node_attributes(G, dict(zip(range(n), nodes['node_key1'].to_numpy())), node_key_attribute)
    G.add_edges_from(zip(data['node_index1'].tolist(), data['node_index2'].tolist()))
    if layout == 'kamada_kawai':
        if verbose:
            logging.info('Applying the Kamada-Kawai network layout...')
        for node, xy in kamada_kawai_layout(G, device=device).items():
            G.nodes[node]['x'], G.nodes[node]['y'] = xy[0], xy[1]
    else:
        G = apply_network_layout(G, layout=layout, seed=seed, verbose=verbose, device=device)
    return calculate_edge_lengths(G, verbose=verbose, device=device)


def load_network_from_scatter(filename, node_key_attribute='key', verbose=True):
    """safepy/safe_io.py:271-285: tab-separated file with a header line and four columns
    (key, x, y, label) -> an edgeless networkx graph, nodes 0..N-1 with those attributes."""
    import networkx as nx
    import pandas as pd
    if verbose:
        logging.info('Loading the file of node coordinates...')
    scatter = pd.read_csv(os.path.expanduser(filename), sep='\t')
    scatter.columns = ['key', 'x', 'y', 'label']
    G = nx.Graph()
    G.add_nodes_from([(i, row) for i, row in scatter.T.to_dict().items()])
    return G


def euclidean_pseudo_network(graph, neighborhood_radius, device=0, as_networkx=True):
    """The pseudo-network `load_network` attaches to `.scatter` inputs (safepy/safe.py:302-309):
    nodes closer than `neighborhood_radius * (max(coords) - min(coords))` -- the extent is taken
    over x AND y values together (safe.py:306) -- are connected; every node also gets a self loop
    (distance 0 < radius), and every edge weight 1.0, as `nx.from_numpy_array` produces.
    The all-pairs distances and the threshold run in the K1 kernel; the edge list is read back
    from the device CSR (u <= v).  as_networkx=False returns a `LayoutGraph` (arrays only)."""
    from .safe import LayoutGraph
    xy = np.ascontiguousarray(get_node_coordinates(graph), dtype=np.float64)
    n = xy.shape[0]
    nr = neighborhood_radius * (np.max(xy.ravel()) - np.min(xy.ravel()))
    ctx = be.Context.default(device)
    nbr = be.Neighborhoods.euclidean(ctx, xy, nr)
    try:
        row_ptr, col = nbr.csr()
    finally:
        nbr.close()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    col = col.astype(np.int64)
    upper = col >= rows
    eu, ev = rows[upper], col[upper]
    if not as_networkx:
        return LayoutGraph(xy, eu, ev, weight=np.ones(eu.size))
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(eu.tolist(), ev.tolist()), weight=1.0)
    return G


# ------------------------------------------------------------------------------------------------
# read_attributes
# ------------------------------------------------------------------------------------------------
def _numeric_table_from_text(path):
    """A tab-separated attribute file (first column = node labels, header = attribute names) as a
    label-indexed frame of floats.  Non-numeric cells become NaN and every column is stored in the
    narrowest float type that holds it -- which is why matrices loaded from text are float32
    (safe_io.py:358-365)."""
    import pandas as pd
    raw = pd.read_csv(path, sep='\t', dtype={0: str})
    raw = raw.set_index(raw.columns[0], drop=True)
    return raw.apply(pd.to_numeric, downcast='float', errors='coerce')


def _parse_attribute_source(attribute_file):
    """(attributes frame [id, name], label-indexed numeric table) from a `.txt` / `.gz` path or a
    DataFrame indexed by node label -- the input half of read_attributes (safe_io.py:338-388).  The
    text-to-float conversion and the averaging of repeated labels are pandas' own, as in the
    reference; columns are renamed 0..M-1 for files and kept for DataFrames."""
    import pandas as pd
    if isinstance(attribute_file, pd.DataFrame):
        table, names = attribute_file, attribute_file.columns
    elif isinstance(attribute_file, str):
        path = os.path.expanduser(attribute_file)
        ext = os.path.splitext(path)[1]
        if ext == '.mat':
            raise NotImplementedError('MATLAB attribute files (safe_io.py:346-356) are out of scope; '
                                      'pass a .txt / .gz file or a DataFrame')
        if ext not in ('.txt', '.gz'):
            raise ValueError("Only attribute files with the following extensions are accepted: .mat, .txt, .gz.")
        table = _numeric_table_from_text(path)
        names = table.columns
        table.columns = np.arange(table.shape[1])
    else:
        raise ValueError('attribute_file must be a path or a pandas DataFrame, got %s' % type(attribute_file))
    attributes = pd.DataFrame({'id': np.arange(len(names)), 'name': pd.Index(names).astype(str)})
    table = table.apply(pd.to_numeric, errors='coerce')
    if table.index.has_duplicates:
        logging.info('\nThe attribute file contains multiple values for the same labels. Their values will be averaged.')
        table = table.groupby(level=0).mean()
    return attributes, table


def read_attributes_device(attribute_file='', node_label_order=None, mask_duplicates=False, fill_value=np.nan,
                           verbose=True, device=0):
    """`read_attributes` that also returns the device-resident aligned matrix:
    (attributes, node_label_order, node2attribute, backend.Attributes).  The caller owns the handle."""
    import pandas as pd
    attributes, table = _parse_attribute_source(attribute_file)
    if node_label_order is None or len(node_label_order) == 0:       # `if not node_label_order`, safe_io.py:390
        node_label_order = table.index.values
    node_label_in_file = table.index.values
    known = set(node_label_order)
    node_label_not_mapped = [x for x in node_label_in_file if x not in known]     # :394 (a set instead of a list scan)

    # ---- the alignment, safe_io.py:396 `reindex(index=node_label_order, fill_value=...)` + :412 `.values`
    values = table.to_numpy()
    if values.dtype not in (np.float32, np.float64):
        values = values.astype(np.float64)            # integer / mixed tables: the reference's reindex with NaN upcasts too
    row_map = table.index.get_indexer(pd.Index(node_label_order)).astype(np.int64)      # -1 = label not in the file
    if mask_duplicates:                               # :399-409: one random node per label keeps its values
        idx = np.random.permutation(np.arange(len(row_map)))
        mask_dups = pd.Index(node_label_order)[idx].duplicated(keep='first')
        logging.info('\nThe network contains %d nodes with duplicate labels. '
                     'Only one random node per label will be considered. '
                     'The attribute values of all other nodes will be set to NaN.' % mask_dups.sum())
        row_map[idx[mask_dups]] = -2
    ctx = be.Context.default(device)
    if values.shape[0] == 0:                          # empty file: every node is "not in the file"
        values = np.full((1, values.shape[1]), fill_value, dtype=values.dtype)
    # memory order of the result: whatever pandas' `.values` yields for this frame (Fortran for a frame
    # that is one block per dtype straight from the parser, C after a group-by) -- a two-row probe of
    # the same call tells, since the order depends on the block structure, not on the row count
    probe = table.iloc[:2].reindex(index=list(node_label_order[:2]), fill_value=fill_value).values
    order = 'C' if (probe.flags['C_CONTIGUOUS'] and not probe.flags['F_CONTIGUOUS']) else 'F'
    attr, node2attribute = be.Attributes.reindexed(ctx, values, row_map, fill_value=fill_value, order=order)

    if verbose:                                       # the summary of safe_io.py:414-431; the value census is one device pass
        n_file, n_attr, n_lost = len(node_label_in_file), attributes.shape[0], len(node_label_not_mapped)
        logging.info('\nAttribute data provided: %d labels x %d attributes' % (n_file, n_attr))
        if n_lost:
            shown = [str(x) for x in node_label_not_mapped[:3]]
            logging.info('%s and %d other labels in the attribute file were not found in the network.'
                         % (', '.join(shown), n_lost - len(shown)))
        logging.info('\nAttribute data mapped onto the network: %d labels x %d attributes' % (n_file - n_lost, n_attr))
        for what, count in zip(('NaNs', 'zeros', 'positives', 'negatives'), attr.value_counts()):
            logging.info('Values: %d %s' % (count, what))
    return attributes, node_label_order, node2attribute, attr


def read_attributes(attribute_file='', node_label_order=None, mask_duplicates=False, fill_value=np.nan, verbose=True,
                    device=0):
    """safepy/safe_io.py:336-430.  Returns (attributes, node_label_order, node2attribute) like the
    reference; node2attribute is [len(node_label_order), M] in the table's float dtype (f32 for
    text files whose columns pandas can down-cast, else f64), Fortran order like pandas' `.values`
    of a single-dtype frame."""
    attributes, node_label_order, node2attribute, attr = read_attributes_device(
        attribute_file=attribute_file, node_label_order=node_label_order, mask_duplicates=mask_duplicates,
        fill_value=fill_value, verbose=verbose, device=device)
    attr.close()
    return attributes, node_label_order, node2attribute
