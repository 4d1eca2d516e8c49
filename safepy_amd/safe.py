"""`SAFE` -- host-side mirror of the reference class for the hot path.

Same constructor signature, attribute names, method names, kwargs, array layouts and
error behaviour as `safepy.safe.SAFE` (safepy/safe.py:37-608) for
`define_neighborhoods()` / `compute_pvalues()` (+ the additive `compute_node_distances()` and
`node_distance_percentile()`); the arithmetic runs in libsafe_hip.so on an MI355X.  One departure:
`neighborhood_radius_type`, which the reference reads and ignores, acts here ('absolute' and 'percentile'
radii, and 'nearest': every node's own radius, out to its k-th nearest node; 'diameter' is the reference's rule).  `print_output_files()` writes the reference's
three tables, the node-by-attribute text made on the device; `save()` pickles the object.  The plot methods
(`plot_network`, `plot_sample_attributes`, `plot_composite_network`, `plot_composite_network_contours`) draw with
matplotlib, imported when they run; their data-parallel parts run on the device (plot.hip).  Additive:
`enriched_pairs()` / `enriched_table()` return the enriched (node, attribute) pairs as a scipy.sparse array / a long
DataFrame, compacted on the device while the result matrices are still there (pairs.hip).  Additive:
`neighborhood_weighting` gives every member of a neighborhood a distance-decay weight (`neighborhood_weights`,
`set_neighborhood_weights`; weights.hip) and `compute_pvalues` tests the weighted sum.  The MATLAB / Cytoscape
loaders are out of scope.
"""
import configparser
import logging
import os
import pickle
import sys

import numpy as np
import pandas as pd        # noqa: F401  at import, like the reference (safepy/safe.py:19): the first compute_pvalues() of a process
                           # used to pay for it -- 166 of its 178 ms

from . import backend as be
from ._lib import E_UNSUPPORTED, E_VALUE, METRIC_IDS, SafeHipError

_DEFAULTS = {
    # the [DEFAULT] section of safepy/safe_default.ini:1-24, restated (the shipped .ini is not copied):
    # every key read_config looks up, with the reference's default value
    'safe_data': '',
    'networkfile': 'networks/Costanzo_Science_2016.gpickle',
    'annotationfile': 'attributes/hoepfner_movva_2014_doxorubucin.txt',
    'annotationsign': 'both',
    'randomSeed': '',
    'background': 'attribute_file',
    'nodeDistanceType': 'shortpath_weighted_layout',
    'neighborhoodRadius': '0.1',
    'neighborhoodRadiusType': 'diameter',
    'unimodalityType': 'connectivity',
    'groupDistanceType': 'jaccard',
    'groupDistanceThreshold': '0.75',
    # additive (no counterpart in the reference's file): restricted permutations, see SAFE.compute_pvalues
    'permutationStrata': '',
    'permutationStrataBins': '10',
    'familywiseAdjustment': 'none',
    'familywiseScope': 'neighborhoods',
    # additive: the procedure of multiple_testing, see SAFE.compute_pvalues
    'multipleTestingMethod': 'fdr_bh',
    # additive: the random-walk-with-restart kernel of node_distance_metric = 'diffusion', see SAFE.define_neighborhoods
    'diffusionRestart': '0.5',
    'diffusionSteps': '32',
}


_WEIGHTINGS = ('none', 'uniform', 'triangular', 'epanechnikov', 'gaussian', 'custom')     # neighborhood_weighting
_MT_METHODS = ('fdr_bh', 'fdr_by', 'holm', 'hochberg', 'bonferroni')                      # multiple_testing_method (backend.MT_METHODS)


def _member_weights(w, indptr, indices):
    """set_neighborhood_weights: the weights of W -- scipy.sparse or dense [N, N] -- on the members of a CSR membership, f64
    [nnz] in its order, 0 where W stores nothing.  ValueError for a wrong shape, a negative, NaN or infinite value, and a
    non-zero entry outside the membership."""
    n = len(indptr) - 1
    if np.ndim(w) != 2 or tuple(np.shape(w)) != (n, n):
        raise ValueError('neighborhood weights must be a [%d, %d] matrix, got shape %s' % (n, n, tuple(np.shape(w))))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    if be._is_sparse(w):
        from scipy import sparse
        w = sparse.csr_array(w, dtype=np.float64)
        w.sum_duplicates()
        stored = w.data
        data = np.asarray(w[rows, indices], dtype=np.float64).reshape(-1) if len(rows) else np.zeros(0)
        outside = np.count_nonzero(stored) != np.count_nonzero(data)      # every member entry is a stored one or 0
    else:
        w = np.asarray(w, dtype=np.float64)
        stored = w
        data = w[rows, indices]
        mask = np.ones(w.shape, dtype=bool)
        mask[rows, indices] = False
        outside = bool(np.any(w[mask] != 0))
    if not np.all(np.isfinite(stored)) or np.any(stored < 0):
        raise ValueError('neighborhood weights must be finite and >= 0')
    if outside:
        raise ValueError('neighborhood weights hold a non-zero entry outside the membership: a node that is not a member of a '
                         'neighborhood cannot carry weight in it')
    return np.ascontiguousarray(data, dtype=np.float64)


def _neighborhood_size_strata(counts, bins):
    """permutation_strata = 'neighborhood_size': int32 [N], the stratum of every node -- the nodes in ascending (neighborhood
    size, node index) order (a stable argsort), cut into `bins` groups by np.array_split.  Exact: no quantile arithmetic."""
    order = np.argsort(np.asarray(counts), kind='stable')
    strata = np.empty(len(order), dtype=np.int32)
    for b, part in enumerate(np.array_split(order, bins)):
        strata[part] = b
    return strata


def _factorise_strata(labels, n):
    """Array-like stratum labels in node order -> int32 [N] ranks among the distinct labels (np.unique).  ValueError for a wrong
    length and for missing labels (None, NaN)."""
    arr = np.asarray(labels)
    if arr.ndim != 1 or arr.shape[0] != n:
        raise ValueError('permutation_strata needs one label per node in node order: expected length %d, got shape %s'
                         % (n, arr.shape))
    if arr.dtype == object:
        missing = any(v is None or (isinstance(v, (float, np.floating)) and v != v) for v in arr)
    else:
        missing = bool(np.issubdtype(arr.dtype, np.floating) and np.isnan(arr).any())
    if missing:
        raise ValueError('permutation_strata holds missing labels (None / NaN): every node needs a stratum')
    try:
        ranks = np.unique(arr, return_inverse=True)[1]
    except TypeError as exc:
        raise ValueError('permutation_strata labels cannot be ordered against each other (%s)' % exc)
    return np.ascontiguousarray(ranks.reshape(-1), dtype=np.int32)


def _is_real(v):
    """An int or a float (NumPy's included), not a bool."""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _is_percentage(q):
    return isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, bool) and 0 <= q <= 100


def _is_neighbor_count(k):
    """A real number with an integral value of at least 1 (50, 50.0): the k of neighborhood_radius_type = 'nearest'."""
    return _is_real(k) and np.isfinite(k) and k >= 1 and float(k) == int(k)


def _percentile_ranks(count, q):
    """The two order statistics np.percentile(v, q) -- NumPy 2.2, method 'linear' -- interpolates between for len(v) = count,
    and the weight: (previous, next, gamma), 0-based ranks of sorted v.  As numpy.lib._function_base_impl does it: the
    virtual index (count - 1) * (q / 100) in f64, its floor and the rank after it, gamma the difference; an index at or
    above count - 1 takes the last element twice (NumPy's index -1, whence its gamma = index + 1 there)."""
    if count < 1:
        raise ValueError('no pair of nodes has a distance: the percentile of an empty set is undefined')
    h = float((count - 1) * np.true_divide(q, 100))
    if h >= count - 1:
        return count - 1, count - 1, h + 1.0
    k = int(np.floor(h))
    return k, k + 1, h - k


def _lerp(a, b, t):
    """numpy.lib._function_base_impl._lerp for f64 scalars: a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5."""
    a, b, t = float(a), float(b), float(t)
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def _percentile_plan(count, qs):
    """(the distinct ranks to select, ascending; per q: (position of previous, position of next, gamma))."""
    triples = [_percentile_ranks(count, q) for q in qs]
    ranks = sorted({r for k, k1, _ in triples for r in (k, k1)})
    pos = {r: i for i, r in enumerate(ranks)}
    return ranks, [(pos[k], pos[k1], g) for k, k1, g in triples]


def _percentile_values(plan, values):
    return [_lerp(values[i], values[i1], g) for i, i1, g in plan[1]]


class LayoutGraph:
    """Minimal stand-in for the networkx graph the reference keeps in `self.graph`: node
    coordinates in node order plus an undirected edge list with optional per-edge
    'length' / 'weight'.  `SAFE` accepts either this or a networkx.Graph."""

    def __init__(self, xy, edge_u=None, edge_v=None, length=None, weight=None, keys=None, labels=None):
        self.xy = np.ascontiguousarray(xy, dtype=np.float64)
        if self.xy.ndim != 2 or self.xy.shape[1] != 2:
            raise ValueError('xy must be [N,2]')
        n = self.xy.shape[0]
        self.edge_u = np.zeros(0, np.int64) if edge_u is None else np.asarray(edge_u, dtype=np.int64)
        self.edge_v = np.zeros(0, np.int64) if edge_v is None else np.asarray(edge_v, dtype=np.int64)
        self.length = None if length is None else np.asarray(length, dtype=np.float64)
        self.weight = None if weight is None else np.asarray(weight, dtype=np.float64)
        self.keys = list(range(n)) if keys is None else list(keys)
        self.labels = [str(k) for k in self.keys] if labels is None else list(labels)

    def number_of_nodes(self):
        return self.xy.shape[0]


def _graph_arrays(graph):
    """(xy [N,2] in node order, edge_u, edge_v, length or None, weight or None) from a
    LayoutGraph or a networkx graph.  Follows the reference's access pattern: x/y via
    graph.nodes.data (safe.py:390-396), edges indexed by node id (safe.py:412-415)."""
    if isinstance(graph, LayoutGraph):
        return graph.xy, graph.edge_u, graph.edge_v, graph.length, graph.weight
    if hasattr(graph, 'is_directed') and graph.is_directed():
        raise NotImplementedError('directed graphs are not supported (the reference networks are undirected)')
    n = graph.number_of_nodes()
    x = np.array([v for _, v in graph.nodes.data('x')], dtype=np.float64)
    y = np.array([v for _, v in graph.nodes.data('y')], dtype=np.float64)
    xy = np.stack([x, y], axis=1) if n else np.zeros((0, 2))
    eu, ev, el, ew = [], [], [], []
    has_len = has_w = False
    for u, v, data in graph.edges(data=True):
        eu.append(u)
        ev.append(v)
        # networkx _weight_function: data.get(weight, 1) (weighted.py:78)
        el.append(data.get('length', 1))
        ew.append(data.get('weight', 1))
        has_len = has_len or ('length' in data)
        has_w = has_w or ('weight' in data)
    eu = np.asarray(eu, dtype=np.int64) if eu else np.zeros(0, np.int64)
    ev = np.asarray(ev, dtype=np.int64) if ev else np.zeros(0, np.int64)
    length = np.asarray(el, dtype=np.float64) if has_len else None
    weight = np.asarray(ew, dtype=np.float64) if has_w else None
    return xy, eu, ev, length, weight


def _x_extent(xy):
    x = xy[:, 0]
    return np.max(x) - np.min(x)                        # safe.py:390-391, 404-405


class _DistanceSource:
    """Where the node distances of a neighborhood definition come from: the one object that define_neighborhoods,
    compute_node_distances, node_distance_percentile and the within-reach relation ask for radii, membership handles and
    weights (SAFE._distance_source picks it).  A context manager: leaving it releases whatever it opened on the device."""
    keeps_distances = False       # the handles it builds keep the N x N distances on the device (what node_distances then is)
    rule = '<'                    # how a distance compares with a scalar radius (safe.py:399 against networkx's cutoff)
    layout_hint = None            # the layout a new handle should be told of, or None (it knows it already, or there is none)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        pass

    def percentiles(self, qs):
        """np.percentile(v, q), bit for bit, for every q of `qs`.  v is the multiset of node distances of the pairs i < j:
        pdist(xy), or the finite D[i, j] of the kept matrix (row i = the search from i).  v is never stored: the device
        counts it, then selects the order statistics the interpolations need."""
        plan = _percentile_plan(self.select([])[1], qs)
        return _percentile_values(plan, self.select(plan[0])[0])


class _LayoutDistances(_DistanceSource):
    """'euclidean': scipy's pdist of the layout coordinates, recomputed by every device call; nothing stays on the device."""

    def __init__(self, ctx, xy):
        self.ctx, self.xy = ctx, xy

    def diameter_radius(self, fraction):
        return fraction * _x_extent(self.xy)

    def select(self, ranks):
        return self.ctx.pair_distance_select(self.xy, ranks)

    def nearest_radii(self, k):
        return self.ctx.row_distance_select(self.xy, k)

    def members(self, radius, keep_distances=True):
        return be.Neighborhoods.euclidean(self.ctx, self.xy, radius)

    def members_rows(self, radii):
        return be.Neighborhoods.euclidean_rows(self.ctx, self.xy, radii)

    def set_weights(self, nbr, kind, radii, bandwidth):
        nbr.set_weights_from_xy(self.xy, kind, radii, bandwidth)

    def dense_distances(self, radius):
        """f64 [N, N] == squareform(pdist(xy)) (safe.py:397)"""
        n = self.xy.shape[0]
        d_xy = self.ctx.alloc(self.xy.nbytes)
        d_out = self.ctx.alloc_f64(n, n)
        try:
            d_xy.upload(self.xy)
            self.ctx.euclidean_dense(d_xy.ptr, n, radius, None, d_out.ptr)
            return d_out.download((n, n))
        finally:
            d_xy.free()
            d_out.free()

    def check_reach(self, r, t):
        if not np.isfinite(self.xy).all():
            raise ValueError("attribute_unimodality_metric = 'radius' with node_distance_metric = 'euclidean' needs finite "
                             'x and y coordinates for every node')
        if not t > 0:                                # `distance < t` would drop the diagonal: no node within its own reach
            raise ValueError("attribute_unimodality_metric = 'radius' with node_distance_metric = 'euclidean' needs a "
                             'neighborhood radius greater than 0: it resolved to %r' % (r,))


class _NetworkDistances(_DistanceSource):
    """The network metrics: all-pairs shortest paths bounded by a cutoff over the edge weights `w` (None = 1 per edge), or,
    with diffusion = (restart, steps), the random-walk-with-restart distance of 'diffusion' (the graph's 'weight' edge
    attribute; 'length' is never used) with members D <= cutoff.  Percentiles and per-node radii read ONE unbounded search
    whose matrix stays on the device: made when first asked for, owned here, and closed before a bounded handle is built, once
    the per-row handle is built from it, and on close()."""
    keeps_distances = True
    rule = '<='

    def __init__(self, ctx, xy, eu, ev, w, diffusion=None, diameter_in_layout_units=True):
        self.ctx, self.xy, self.eu, self.ev, self.w, self.diffusion = ctx, xy, eu, ev, w, diffusion
        self.diameter_in_layout_units = diameter_in_layout_units
        self._unbounded = None
        # the layout only orders the nodes on the device.  'diffusion' needs none: an edge list without finite coordinates gets no hint
        self.layout_hint = xy if diffusion is None or np.isfinite(xy).all() else None

    def _open(self, cutoff, keep_distances=True):
        n, eu, ev = self.xy.shape[0], self.eu, self.ev
        if eu.size and (eu.min() < 0 or ev.min() < 0 or eu.max() >= n or ev.max() >= n):
            raise ValueError('shortest-path metrics index the neighborhood matrix by node id: ids must be 0..N-1')
        if self.diffusion is not None:
            return be.Neighborhoods.diffusion(self.ctx, n, eu, ev, self.w, self.diffusion[0], self.diffusion[1], cutoff)
        return be.Neighborhoods.shortpath(self.ctx, n, eu, ev, self.w, cutoff, keep_distances=keep_distances)

    def _all_pairs(self):
        if self._unbounded is None:
            self._unbounded = self._open(np.inf)
        return self._unbounded

    def close(self):
        nbr, self._unbounded = self._unbounded, None
        if nbr is not None:
            nbr.close()

    def diameter_radius(self, fraction):
        if not self.diameter_in_layout_units:
            return fraction                             # 'shortpath' + 'diameter': the reference's hop cutoff, safe.py:409
        return fraction * _x_extent(self.xy)

    def select(self, ranks):
        return self._all_pairs().distance_select(ranks)

    def nearest_radii(self, k):
        return self._all_pairs().row_distance_select(k)

    def members(self, radius, keep_distances=True):
        self.close()
        return self._open(radius, keep_distances)

    def members_rows(self, radii):
        """A[i, j] = (D[i, j] <= r_i); the handle keeps the masked distances (D where A is 1)."""
        try:
            return be.Neighborhoods.from_distances_rows(self._all_pairs(), radii, keep_distances=True)
        finally:
            self.close()

    def set_weights(self, nbr, kind, radii, bandwidth):
        nbr.set_weights_from_distances(kind, radii, bandwidth)

    def check_reach(self, r, t):
        pass


class _DeviceResult:
    """An [n, m] float64 result of compute_pvalues still on the device: copied to the host the first
    time the attribute is read (see `_LazyArray`).  Owns its device buffer."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape

    def get(self, into=None):
        host = self.buf.download(self.shape, out=into)
        self.buf.free()
        return host

    def drop(self):
        self.buf.free()


def _local_only_refcount():
    probe = np.empty(1)
    return sys.getrefcount(probe)


_LOCAL_ONLY_REFCOUNT = _local_only_refcount()


class _LazyArray:
    """Descriptor behind SAFE.ns / pvalues_neg / pvalues_pos / nes / nes_binary.  To the caller these
    are plain attributes holding host `float64 [N, M]` arrays (or None) exactly as in the reference
    (safe.py:530-554, 596-608, 468-472); compute_pvalues() leaves the matrices on the device and the
    copy (139 MB each at 3971 x 4373, 1.6 GB each at 20 000 x 10 000 -- ten to a hundred times the
    compute) happens on the first read of each one, so results that are never looked at are never
    moved.  `SAFE.lazy_outputs = False` restores the eager copies.

    Host arrays are recycled: when a result this descriptor handed out is replaced (the next compute_pvalues(), or the caller
    setting the attribute to None) the instance keeps the array, and the next read of the same shape copies into it -- IF nobody
    else holds a reference to it (sys.getrefcount), so an array the caller kept (`old = sf.nes`) is never written again.  A
    fresh 139 MB array costs 34 000 page faults on its first write (the copy runs at 35 GB/s) and as much again when it is
    freed; into resident pages the same copy runs at the link's 56 GB/s."""

    def __init__(self, name):
        self.slot = '_r_' + name
        self.made = '_made_' + name          # the host array this descriptor produced last (None: the caller's own value)
        self.spare = '_spare_' + name        # a produced array that was replaced: may be written again if no one else holds it

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        d = obj.__dict__
        v = d.get(self.slot)
        if isinstance(v, _DeviceResult):
            into = d.pop(self.spare, None)
            # (no reference outside this function: the count a fresh local array shows on THIS interpreter, measured once --
            # 2 on CPython 3.10 (local name + getrefcount's argument), possibly 1 where references are borrowed)
            if not (isinstance(into, np.ndarray) and into.shape == tuple(v.shape) and into.dtype == np.float64
                    and into.flags.c_contiguous and into.flags.owndata and sys.getrefcount(into) == _LOCAL_ONLY_REFCOUNT):
                into = None
            v = v.get(into)
            del into
            d[self.slot] = v
            d[self.made] = v
        return v

    def __set__(self, obj, value):
        d = obj.__dict__
        old = d.get(self.slot)
        if isinstance(old, _DeviceResult):
            old.drop()
        elif old is not None and old is d.get(self.made):
            d[self.spare] = old                                   # ours: kept for the next read of this attribute
        d[self.made] = None
        d[self.slot] = value


class SAFE:
    """Defines an instance of SAFE analysis (hot path only); see module docstring."""

    ns = _LazyArray('ns')
    pvalues_neg = _LazyArray('pvalues_neg')
    pvalues_pos = _LazyArray('pvalues_pos')
    nes = _LazyArray('nes')
    nes_binary = _LazyArray('nes_binary')
    familywise_statistic = _LazyArray('familywise_statistic')

    def __init__(self, path_to_ini_file='', path_to_safe_data=None, verbose=True, device=0):
        self.verbose = verbose
        self.default_config = None
        self.path_to_safe_data = path_to_safe_data
        self.path_to_network_file = None
        self.view_name = None
        self.path_to_attribute_file = None

        self.graph = None
        self.graph_euclidean = None
        self.node_key_attribute = 'label_orf'

        self.attributes = None
        self.nodes = None
        self.node2attribute = None
        self.num_nodes_per_attribute = None
        self.attribute_sign = 'both'

        self.node_distance_metric = 'shortpath_weighted_layout'
        self.neighborhood_radius_type = None
        self.neighborhood_radius = None
        self.neighborhood_radius_resolved = None     # the radius the last define_neighborhoods / compute_node_distances used (float)
        self.neighborhood_radii = None               # 'nearest' only: every node's own radius, f64 [N] (resolved = their median)
        # distance-weighted neighborhood scores (define_neighborhoods, set_neighborhood_weights): 'none' (flat, the reference),
        # 'uniform', 'triangular', 'epanechnikov', 'gaussian' (with neighborhood_weight_bandwidth), 'custom'
        self.neighborhood_weighting = 'none'
        self.neighborhood_weight_bandwidth = 0.5
        # node_distance_metric = 'diffusion' only: the restart probability alpha in (0, 1) and the number of steps T >= 1 of the
        # truncated random-walk-with-restart kernel X_{t+1} = alpha I + (1 - alpha) S X_t, X_0 = I, K = X_T (define_neighborhoods)
        self.diffusion_restart = 0.5
        self.diffusion_steps = 32

        self.background = 'attribute_file'
        self.num_permutations = 1000
        self.multiple_testing = False
        # read only when multiple_testing is on: the family one Benjamini-Hochberg run adjusts -- 'attributes' (every node's row, the
        # reference), 'neighborhoods' (every attribute's column), 'all' (the whole matrix); compute_pvalues
        self.multiple_testing_scope = 'attributes'
        # read only when multiple_testing is on: the procedure -- 'fdr_bh' (Benjamini-Hochberg, the reference), 'fdr_by'
        # (Benjamini-Yekutieli: FDR under any dependence), 'holm', 'hochberg', 'bonferroni' (family-wise error rate); compute_pvalues
        self.multiple_testing_method = 'fdr_bh'
        # restricted permutations of how='randomization' (compute_pvalues): None, one label per node, or 'neighborhood_size'
        # (nodes binned into permutation_strata_bins groups by the size of their neighborhood)
        self.permutation_strata = None
        self.permutation_strata_bins = 10
        self.permutation_strata_resolved = None      # int32 [N]: every node's stratum in the last stratified call
        self.permutation_strata_sizes = None         # int64 [S]: movable rows per stratum in that call
        # family-wise error control of how='randomization' (compute_pvalues): 'none', or 'maxT' -- Westfall-Young single-step
        # max-statistic adjusted p-values over familywise_scope: 'neighborhoods' (every attribute's column) or 'all' (the matrix)
        self.familywise_adjustment = 'none'
        self.familywise_scope = 'neighborhoods'
        self.familywise_statistic = None             # 'maxT' only: the observed standardised score z [N, M] of the last call
        self.neighborhood_score_type = 'sum'
        self.enrichment_type = 'auto'
        self.hypergeom_tails = 'upper'   # 'attribute_sign': the hypergeometric test follows attribute_sign (both tails, ns, signed nes)
        self.attribute_transform = 'none'   # 'rank': compute_pvalues tests the per-column midranks of node2attribute (ranked on the device)
        self.enrichment_threshold = 0.05
        self.enrichment_max_log10 = 16
        self.attribute_enrichment_min_size = 10
        self.random_seed = None

        self.ns = None
        self.pvalues_neg = None
        self.pvalues_pos = None
        self.nes = None
        self.nes_threshold = None
        self.nes_binary = None

        self.graph_euclidean = None      # Euclidean pseudo-network of .scatter inputs (safe.py:67, 302-309), if any
        self.attribute_unimodality_metric = 'connectivity'
        # 'radius' only: enriched nodes within attribute_unimodality_radius_multiple x the neighborhood radius of each other are
        # "within reach"; an attribute is one region when at least attribute_unimodality_min_fraction of its enriched pairs are
        self.attribute_unimodality_radius_multiple = 2.0
        self.attribute_unimodality_min_fraction = 0.65
        self.attribute_distance_metric = 'jaccard'
        self.attribute_distance_threshold = 0.75
        self.domains = None
        self.node2domain = None
        self.output_dir = ''
        self.output_timing = None        # print_output_files: time split of the last node table made on the device

        # device state (never pickled)
        self.device = device
        self.lazy_outputs = True         # result matrices stay on the device until first read (_LazyArray)
        self._nbr = None                 # backend.Neighborhoods matching _neighborhoods_host / lazily downloaded
        self._neighborhoods_host = None
        self._weights_host = None        # (indptr, indices, data) of neighborhood_weights once fetched or given; pickled
        self._node_distances = None
        self._pending_binary = None
        self._maxt_pending = None        # (observed statistic buffer, smallest adjusted p-values [2, M]) between the device call and the results
        self._attr_dev = None            # resident node2attribute (load_attributes(keep_on_device=True))
        self._attr_dev_host = None
        self._missing_rows = None        # sparse node2attribute only: uint8 [N], 1 = the node's whole row is missing (NaN)

        self.read_config(path_to_ini_file, path_to_safe_data=self.path_to_safe_data)
        self.validate_config()

    # ------------------------------------------------------------------ config ----
    def read_config(self, path_to_ini_file, path_to_safe_data=None):
        """safepy/safe.py:116-188.  Three sources, later wins: the built-in defaults, the user's INI
        (sections 'Input files' and 'Analysis parameters'), the constructor's `path_to_safe_data`."""
        parser_options = dict(allow_no_value=True, comment_prefixes=('#', ';', '{'), inline_comment_prefixes='#')
        builtin = configparser.ConfigParser(**parser_options)
        builtin.read_dict({'DEFAULT': _DEFAULTS})
        self.default_config = builtin['DEFAULT']
        user = configparser.ConfigParser(defaults=self.default_config, **parser_options)
        if path_to_ini_file:
            user.read(path_to_ini_file)

        def option(section, key):
            # a section the user's file lacks answers with the defaults
            if not user.has_section(section):
                user.add_section(section)
            return user.get(section, key)

        # -- input files: relative to the data folder when there is one, else taken as given (safe.py:149-165)
        data_dir = path_to_safe_data if path_to_safe_data is not None else (option('Input files', 'safe_data') or None)
        self.path_to_safe_data = data_dir
        network_file, attribute_file = option('Input files', 'networkfile'), option('Input files', 'annotationfile')
        if data_dir is not None:
            assert data_dir.endswith('/'), "path_to_safe_data should end with '/' (it is joined with the file names)"
            network_file, attribute_file = os.path.join(data_dir, network_file), os.path.join(data_dir, attribute_file)
        self.path_to_network_file, self.path_to_attribute_file = network_file, attribute_file
        self.attribute_sign = option('Input files', 'annotationsign')

        # -- analysis parameters (safe.py:169-184)
        self.background = option('Analysis parameters', 'background')
        self.node_distance_metric = option('Analysis parameters', 'nodeDistanceType')
        self.neighborhood_radius_type = option('Analysis parameters', 'neighborhoodRadiusType')
        self.neighborhood_radius = float(option('Analysis parameters', 'neighborhoodRadius'))
        try:
            self.random_seed = int(option('Analysis parameters', 'randomSeed'))
        except (ValueError, TypeError):                    # empty = unseeded
            self.random_seed = None
        self.attribute_unimodality_metric = option('Analysis parameters', 'unimodalityType')
        self.attribute_distance_metric = option('Analysis parameters', 'groupDistanceType')
        self.attribute_distance_threshold = float(option('Analysis parameters', 'groupDistanceThreshold'))
        self.permutation_strata = option('Analysis parameters', 'permutationStrata') or None      # empty = free shuffle
        bins = option('Analysis parameters', 'permutationStrataBins')
        try:
            self.permutation_strata_bins = int(bins)
        except (ValueError, TypeError):                    # validate_config names the bad value
            self.permutation_strata_bins = bins
        self.familywise_adjustment = option('Analysis parameters', 'familywiseAdjustment') or 'none'     # empty = none
        self.familywise_scope = option('Analysis parameters', 'familywiseScope') or 'neighborhoods'
        self.multiple_testing_method = option('Analysis parameters', 'multipleTestingMethod') or 'fdr_bh'      # empty = fdr_bh
        restart, steps = option('Analysis parameters', 'diffusionRestart'), option('Analysis parameters', 'diffusionSteps')
        try:
            self.diffusion_restart = float(restart)
        except (ValueError, TypeError):                    # validate_config names the bad value
            self.diffusion_restart = restart
        try:
            self.diffusion_steps = int(steps)
        except (ValueError, TypeError):
            self.diffusion_steps = steps

        # the reference falls back on its package folder (safe.py:186-188); here: this package's
        self.output_dir = os.path.dirname(path_to_ini_file) if path_to_ini_file else ''
        if not self.output_dir:
            self.output_dir = os.path.dirname(os.path.abspath(__file__))

    def validate_config(self):
        """safepy/safe.py:190-235: invalid option -> restore the default, raise ValueError."""
        if self.background not in ['attribute_file', 'network']:
            bad, self.background = self.background, self.default_config.get('background')
            raise ValueError('%s is not a valid setting for background. '
                             'Valid options are: attribute_file, network.' % bad)
        if self.node_distance_metric not in ['euclidean', 'shortpath', 'shortpath_weighted_layout', 'diffusion']:
            bad, self.node_distance_metric = self.node_distance_metric, self.default_config.get('nodeDistanceType')
            raise ValueError('%s is not a valid setting for node_distance_metric. '
                             'Valid options are: euclidean, shortpath, shortpath_weighted_layout, diffusion' % bad)
        restart = getattr(self, 'diffusion_restart', 0.5)
        if not _is_real(restart) or not (0 < restart < 1):
            self.diffusion_restart = 0.5
            raise ValueError('diffusion_restart = %r is not valid: it must be a number in the (0, 1) range.' % (restart,))
        steps = getattr(self, 'diffusion_steps', 32)
        if not isinstance(steps, (int, np.integer)) or isinstance(steps, (bool, np.bool_)) or steps < 1:
            self.diffusion_steps = 32
            raise ValueError('diffusion_steps = %r is not valid: it must be an integer equal or greater than 1.' % (steps,))
        if self.neighborhood_radius_type not in [None, 'diameter', 'absolute', 'percentile', 'nearest']:
            bad, self.neighborhood_radius_type = self.neighborhood_radius_type, self.default_config.get('neighborhoodRadiusType')
            raise ValueError('%s is not a valid setting for neighborhood_radius_type. '
                             'Valid options are: diameter, absolute, percentile, nearest' % bad)
        if self.neighborhood_radius_type == 'nearest' and not _is_neighbor_count(self.neighborhood_radius):
            bad, self.neighborhood_radius = self.neighborhood_radius, float(self.default_config.get('neighborhoodRadius'))
            self.neighborhood_radius_type = self.default_config.get('neighborhoodRadiusType')
            raise ValueError('neighborhood_radius = %r is not a number of nodes: with neighborhood_radius_type = nearest '
                             'it must be a whole number of at least 1.' % (bad,))
        if self.neighborhood_radius_type == 'percentile' and not _is_percentage(self.neighborhood_radius):
            bad, self.neighborhood_radius = self.neighborhood_radius, float(self.default_config.get('neighborhoodRadius'))
            self.neighborhood_radius_type = self.default_config.get('neighborhoodRadiusType')
            raise ValueError('neighborhood_radius = %r is not a percentile: with neighborhood_radius_type = percentile '
                             'it must be a number in the [0, 100] range.' % (bad,))
        if self.attribute_sign not in ['highest', 'lowest', 'both']:
            bad, self.attribute_sign = self.attribute_sign, self.default_config.get('annotationsign')
            raise ValueError('%s is not a valid setting for attribute_sign. '
                             'Valid options are: highest, lowest, both' % bad)
        if getattr(self, 'hypergeom_tails', 'upper') not in ['upper', 'attribute_sign']:
            bad, self.hypergeom_tails = self.hypergeom_tails, 'upper'
            raise ValueError('%s is not a valid setting for hypergeom_tails. '
                             'Valid options are: upper, attribute_sign' % (bad,))
        scope = getattr(self, 'multiple_testing_scope', 'attributes')
        if not isinstance(scope, str) or scope not in ['attributes', 'neighborhoods', 'all']:
            self.multiple_testing_scope = 'attributes'
            raise ValueError('%s is not a valid setting for multiple_testing_scope. '
                             'Valid options are: attributes, neighborhoods, all' % (scope,))
        method = getattr(self, 'multiple_testing_method', 'fdr_bh')
        if not isinstance(method, str) or method not in _MT_METHODS:
            self.multiple_testing_method = 'fdr_bh'
            raise ValueError('%s is not a valid setting for multiple_testing_method. '
                             'Valid options are: %s' % (method, ', '.join(_MT_METHODS)))
        strata = getattr(self, 'permutation_strata', None)
        if isinstance(strata, str) and strata != 'neighborhood_size':
            self.permutation_strata = None
            raise ValueError('%s is not a valid setting for permutation_strata. Valid options are: None, '
                             'neighborhood_size, or one label per node.' % (strata,))
        if strata is not None and not isinstance(strata, str) and np.ndim(strata) != 1:
            self.permutation_strata = None
            raise ValueError('permutation_strata must be None, neighborhood_size or a one-dimensional array-like with one '
                             'label per node, not %r' % (strata,))
        bins = getattr(self, 'permutation_strata_bins', 10)
        if not isinstance(bins, (int, np.integer)) or isinstance(bins, (bool, np.bool_)) or bins < 1:
            self.permutation_strata_bins = 10
            raise ValueError('permutation_strata_bins = %r is not valid: it must be an integer equal or greater than 1.' % (bins,))
        adjustment = getattr(self, 'familywise_adjustment', 'none')
        if not isinstance(adjustment, str) or adjustment not in ['none', 'maxT']:
            self.familywise_adjustment = 'none'
            raise ValueError('%s is not a valid setting for familywise_adjustment. '
                             'Valid options are: none, maxT' % (adjustment,))
        family = getattr(self, 'familywise_scope', 'neighborhoods')
        if not isinstance(family, str) or family not in ['neighborhoods', 'all']:
            self.familywise_scope = 'neighborhoods'
            raise ValueError('%s is not a valid setting for familywise_scope. '
                             'Valid options are: neighborhoods, all' % (family,))
        weighting = getattr(self, 'neighborhood_weighting', 'none')
        if not isinstance(weighting, str) or weighting not in _WEIGHTINGS:
            self.neighborhood_weighting = 'none'
            raise ValueError('%s is not a valid setting for neighborhood_weighting. '
                             'Valid options are: %s' % (weighting, ', '.join(_WEIGHTINGS)))
        bandwidth = getattr(self, 'neighborhood_weight_bandwidth', 0.5)
        if not _is_real(bandwidth) or not np.isfinite(bandwidth) or bandwidth <= 0:
            self.neighborhood_weight_bandwidth = 0.5
            raise ValueError('neighborhood_weight_bandwidth = %r is not valid: it must be a finite number greater than 0.'
                             % (bandwidth,))
        if getattr(self, 'attribute_transform', 'none') not in ['none', 'rank']:
            bad, self.attribute_transform = self.attribute_transform, 'none'
            raise ValueError('%s is not a valid setting for attribute_transform. '
                             'Valid options are: none, rank' % (bad,))
        multiple = getattr(self, 'attribute_unimodality_radius_multiple', 2.0)
        if not _is_real(multiple) or not np.isfinite(multiple) or multiple <= 0:
            self.attribute_unimodality_radius_multiple = 2.0
            raise ValueError('attribute_unimodality_radius_multiple = %r is not valid: it must be a finite number greater than 0.'
                             % (multiple,))
        fraction = getattr(self, 'attribute_unimodality_min_fraction', 0.65)
        if not _is_real(fraction) or not (0 < fraction <= 1):
            self.attribute_unimodality_min_fraction = 0.65
            raise ValueError('attribute_unimodality_min_fraction = %r is not valid: it must be a number in the (0, 1] range.'
                             % (fraction,))
        if not isinstance(self.num_permutations, int) or (self.num_permutations < 10):
            self.num_permutations = 1000
            raise ValueError('num_permutations must be an integer equal or greater than 10.')
        if not isinstance(self.enrichment_threshold, float) or (self.enrichment_threshold <= 0) \
                or (self.enrichment_threshold >= 1):
            self.enrichment_threshold = 0.05
            raise ValueError('enrichment_threshold must be in the (0,1) range.')
        if not isinstance(self.enrichment_max_log10, (int, float)):
            self.enrichment_max_log10 = 16
            raise ValueError('enrichment_max_log10 must be a number.')
        if not isinstance(self.attribute_enrichment_min_size, int) or (self.attribute_enrichment_min_size < 2):
            self.attribute_enrichment_min_size = 10
            raise ValueError('attribute_enrichment_min_size must be an integer equal or greater than 2.')
        if not isinstance(self.attribute_distance_threshold, float) or (self.attribute_distance_threshold <= 0) \
                or (self.attribute_distance_threshold >= 1):
            self.attribute_distance_threshold = 0.75
            raise ValueError('attribute_enrichment_min_size must be a float number in the (0,1) range.')

    # pickling drops device handles (the reference pickles the whole object, safe.py:237-242)
    def __getstate__(self):
        for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'familywise_statistic'):
            getattr(self, name)              # results still on the device come to the host first
        self.neighborhood_weights            # (weights still on the device become _weights_host: host arrays)
        nd = self._node_distances
        if isinstance(nd, tuple) and nd[0] == 'device-shortpath':
            self._node_distances = ('dense-shortpath', nd[1].distances())
        state = self.__dict__.copy()
        if state.get('_neighborhoods_host') is None and state.get('_nbr') is not None:
            state['_neighborhoods_host'] = self._nbr.to_dense()
        for key in [k for k in state if k.startswith('_spare_') or k.startswith('_made_')]:
            del state[key]                   # recycled host arrays and their bookkeeping are not part of the object's value
        state['_nbr'] = None
        state['_attr_dev'] = None
        state['_attr_dev_host'] = None
        state['default_config'] = dict(self.default_config) if self.default_config is not None else None
        return state

    def save(self, output_file='', **kwargs):
        """safepy/safe.py:237-242: pickles the object (device results come to the host first: __getstate__)."""
        if not output_file:
            output_file = os.path.join(os.getcwd(), 'safe_output.p')
        with open(output_file, 'wb') as handle:
            pickle.dump(self, handle)

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault('hypergeom_tails', 'upper')     # (objects pickled before the setting existed)
        self.__dict__.setdefault('attribute_transform', 'none')
        self.__dict__.setdefault('multiple_testing_scope', 'attributes')
        self.__dict__.setdefault('multiple_testing_method', 'fdr_bh')
        self.__dict__.setdefault('attribute_unimodality_radius_multiple', 2.0)
        self.__dict__.setdefault('attribute_unimodality_min_fraction', 0.65)
        self.__dict__.setdefault('neighborhood_radii', None)
        self.__dict__.setdefault('permutation_strata', None)
        self.__dict__.setdefault('permutation_strata_bins', 10)
        self.__dict__.setdefault('permutation_strata_resolved', None)
        self.__dict__.setdefault('permutation_strata_sizes', None)
        self.__dict__.setdefault('familywise_adjustment', 'none')
        self.__dict__.setdefault('familywise_scope', 'neighborhoods')
        self.__dict__.setdefault('_r_familywise_statistic', None)
        self.__dict__.setdefault('neighborhood_weighting', 'none')
        self.__dict__.setdefault('neighborhood_weight_bandwidth', 0.5)
        self.__dict__.setdefault('_weights_host', None)
        self.__dict__.setdefault('diffusion_restart', 0.5)
        self.__dict__.setdefault('diffusion_steps', 32)
        if isinstance(self.default_config, dict):
            cp = configparser.ConfigParser()
            cp.read_dict({'DEFAULT': self.default_config})
            self.default_config = cp['DEFAULT']

    # ------------------------------------------------------------------ inputs ----
    def load_network(self, **kwargs):
        """safepy/safe.py:244-324 for in-memory graphs (`graph=` / `network_file=` a networkx.Graph
        with node attributes x, y -- and edge attribute 'length' for the default metric -- or a
        `LayoutGraph`), `.gpickle` files, edge lists (`.txt` / `.tsv`, optionally `.gz`: parsed, laid
        out with the spring-embedded layout on the device from self.random_seed -- or, additive, with `layout='kamada_kawai'`
        passed here -- edge lengths added; safe.py:289-293, safe_io.py:30-121) and `.scatter` files (with their Euclidean pseudo-network,
        safe.py:296-309, built on the device).  The MATLAB and Cytoscape loaders (safe_io.py:124-268)
        are out of scope.  Sets self.graph, self.graph_euclidean (for .scatter) and self.nodes
        (safe.py:311-324)."""
        import pandas as pd
        from . import safe_io
        if 'network_file' in kwargs and isinstance(kwargs['network_file'], str):
            if self.path_to_safe_data is None:
                self.path_to_network_file = kwargs['network_file']
            else:
                self.path_to_network_file = os.path.join(self.path_to_safe_data, kwargs['network_file'])
        if 'view_name' in kwargs:
            self.view_name = kwargs['view_name']
        if 'node_key_attribute' in kwargs:
            self.node_key_attribute = kwargs['node_key_attribute']
        self.validate_config()
        graph = kwargs.get('graph', kwargs.get('network_file'))
        self.graph_euclidean = None
        if graph is None and self.path_to_network_file and os.path.exists(self.path_to_network_file):
            graph = self.path_to_network_file          # the configured network (INI networkfile / safe_data), safe.py:263-264
        if graph is None:
            raise NotImplementedError('safepy_amd.SAFE.load_network needs graph=<networkx.Graph | LayoutGraph> or '
                                      'network_file=<.gpickle | .txt | .tsv | .scatter>; the default safe-data network is not bundled')
        if isinstance(graph, str):
            path = self.path_to_network_file
            assert os.path.exists(path), path
            suffixes = [x for x in os.path.basename(path).split('.')[1:]]
            ext = '.' + suffixes[0] if suffixes else ''
            if self.verbose:
                logging.info('Loading network from %s' % path)
            if ext == '.gpickle':
                graph = safe_io.load_network_from_gpickle(path, verbose=self.verbose)
            elif ext in ('.txt', '.tsv'):
                graph = safe_io.load_network_from_txt(path, layout=kwargs.get('layout', 'spring_embedded'),
                                                      node_key_attribute=self.node_key_attribute,
                                                      seed=self.random_seed, verbose=self.verbose, device=self.device)
            elif ext == '.scatter':
                graph = safe_io.load_network_from_scatter(path, node_key_attribute=self.node_key_attribute,
                                                          verbose=self.verbose)
                self.graph_euclidean = safe_io.euclidean_pseudo_network(
                    graph, self.neighborhood_radius, device=self.device,
                    as_networkx=kwargs.get('pseudo_network', 'networkx') == 'networkx')
            else:
                raise NotImplementedError('network files of type %r need the reference\'s MATLAB / Cytoscape loaders, '
                                          'which are out of scope (supported: .gpickle, .txt, .tsv, .scatter)' % ext)
        self.graph = graph
        self._invalidate_neighborhoods()
        if isinstance(graph, LayoutGraph):
            ids, keys, labels = list(range(graph.number_of_nodes())), list(graph.keys), list(graph.labels)
        else:
            key_list = dict(graph.nodes.data(self.node_key_attribute))
            key_list = {k: v for k, v in key_list.items() if v is not None}
            if not key_list:
                raise Exception('The specified node key attribute (%s) does not exist in this network. '
                                'Set node_key_attribute to one of the attributes the nodes carry.'
                                % self.node_key_attribute)
            for k, v in key_list.items():
                graph.nodes[k]['key'] = v
            label_list = {k: v for k, v in graph.nodes.data('label') if v is not None}
            ids, keys, labels = list(label_list.keys()), list(key_list.values()), list(label_list.values())
        self.nodes = pd.DataFrame(data={'id': ids, 'key': keys, 'label': labels})

    def load_attributes(self, **kwargs):
        """safepy/safe.py:334-367 over `read_attributes` (safe_io.py:336-430): `attribute_file=` a
        `.txt` / `.gz` path, a pandas DataFrame indexed by node key, or (additive) a ready [N,M]
        ndarray in node order, or (additive) a `utils.make_go.GoMatrix` built with `node_label_order=` this network's node
        keys (its sparse matrix, missing rows and term ids / names are taken as they are; with `keep_on_device=True` the
        device matrix comes from its `to_attributes`), or (additive) a scipy.sparse [N,M] matrix in node order, which stays sparse:
        `self.node2attribute` is that object, only its stored entries are uploaded and the dense matrix exists on
        the device alone; `missing_rows=` (bool / 0-1 [N], sparse input only) marks the nodes whose whole row is
        missing (NaN), what `fill_value=NaN` gives the nodes a file does not list.  Other kwargs
        (`mask_duplicates`, `fill_value`) are forwarded.
        The alignment to node order runs on the device.  `keep_on_device=True` (additive) keeps the
        aligned matrix resident for compute_pvalues(), which then skips the upload; the host
        `self.node2attribute` is made read-only in exchange (assign a new array to replace it)."""
        import pandas as pd
        from . import safe_io
        from .utils.make_go import GoMatrix
        keep = bool(kwargs.pop('keep_on_device', False))
        missing_rows = kwargs.pop('missing_rows', None)
        self._drop_device_attributes()
        self._missing_rows = None
        if 'attribute_file' in kwargs:
            src = kwargs.pop('attribute_file')
            if self.path_to_safe_data is None or isinstance(src, (pd.DataFrame, np.ndarray, GoMatrix)) or be._is_sparse(src):
                self.path_to_attribute_file = src
            elif isinstance(src, str):
                self.path_to_attribute_file = os.path.join(self.path_to_safe_data, src)
            else:
                raise ValueError(type(src))
        src = self.path_to_attribute_file
        if isinstance(src, str):
            assert os.path.exists(src), src
        self.validate_config()
        if isinstance(src, GoMatrix):
            if missing_rows is not None:
                raise TypeError('missing_rows goes with a scipy.sparse attribute_file; a GoMatrix carries its own')
            keys = self._node_keys() if self.graph is not None else None
            if src.node_label_order is None or keys is None or list(src.loci) != list(keys):
                raise ValueError('the rows of this GoMatrix do not follow the nodes of the loaded network: build it with '
                                 'make_go_matrix(..., node_label_order=<the node keys of the network, in node order>) '
                                 '(SAFE.nodes[\'key\']) after load_network')
            a = src.matrix
            self.node2attribute = a
            self._missing_rows = np.ascontiguousarray(src.missing_rows, dtype=np.uint8) if np.any(src.missing_rows) else None
            self._missing_rows_of = a
            self.attributes = pd.DataFrame({'id': list(src.go_details['id']), 'name': list(src.go_details['name'])})
            if keep:
                self._attr_dev = src.to_attributes(self._ctx())
                self._attr_dev_host = a
                self._attr_dev_sig = (a.shape, a.nnz)
            return
        if missing_rows is not None and not be._is_sparse(src):
            raise TypeError('missing_rows goes with a scipy.sparse attribute_file; a dense matrix carries its missing values as NaN')
        if be._is_sparse(src):
            if missing_rows is not None:
                missing_rows = np.ascontiguousarray(np.asarray(missing_rows) != 0, dtype=np.uint8)
                if missing_rows.shape != (src.shape[0],):
                    raise ValueError('missing_rows: expected %d flags, got shape %s' % (src.shape[0], missing_rows.shape))
            self.node2attribute = src
            self._missing_rows = missing_rows
            self._missing_rows_of = src          # (the flags belong to this object: a matrix assigned later has none)
            self.attributes = pd.DataFrame({'id': np.arange(src.shape[1]),
                                            'name': [str(j) for j in range(src.shape[1])]})
            if keep:
                self._attr_dev = be.Attributes.from_sparse(self._ctx(), src, missing_rows)
                self._attr_dev_host = src
                self._attr_dev_sig = (src.shape, src.nnz)
            return
        if isinstance(src, np.ndarray):
            self.node2attribute = src
            self.attributes = pd.DataFrame({'id': np.arange(src.shape[1]),
                                            'name': [str(j) for j in range(src.shape[1])]})
            if keep:
                self._attr_dev = be.Attributes.from_host(self._ctx(), src)
                self._attr_dev_host = src
                src.flags.writeable = False
            return
        if self.verbose and isinstance(src, str):
            logging.info('Loading attributes from %s' % src)
        self.attributes, _, self.node2attribute, attr = safe_io.read_attributes_device(
            node_label_order=self._node_keys(), verbose=self.verbose, attribute_file=src, device=self.device, **kwargs)
        if keep:
            self._attr_dev = attr
            self._attr_dev_host = self.node2attribute
            self.node2attribute.flags.writeable = False
        else:
            attr.close()

    def _drop_device_attributes(self):
        attr = self.__dict__.get('_attr_dev')
        if attr is not None:
            attr.close()
        self._attr_dev = None
        self._attr_dev_host = None

    def _resident_attributes(self):
        """The handle load_attributes(keep_on_device=True) left on the device, if it still mirrors
        self.node2attribute (same object, still read-only)."""
        attr = self.__dict__.get('_attr_dev')
        if attr is None:
            return None
        host = self.node2attribute
        if host is self._attr_dev_host and isinstance(host, np.ndarray) and not host.flags.writeable:
            return attr
        if host is self._attr_dev_host and be._is_sparse(host) and (host.shape, host.nnz) == self.__dict__.get('_attr_dev_sig'):
            return attr                  # (a sparse object cannot be made read-only: same object, same shape and entry count)
        self._drop_device_attributes()
        return None

    def _missing_rows_for(self, a):
        """The missing-row flags load_attributes recorded for the sparse matrix `a`, or None."""
        return self.__dict__.get('_missing_rows') if self.__dict__.get('_missing_rows_of') is a else None

    def _upload_attributes(self):
        """A device handle of self.node2attribute: a dense array as it is, a sparse matrix by its stored entries."""
        if be._is_sparse(self.node2attribute):
            return be.Attributes.from_sparse(self._ctx(), self.node2attribute, self._missing_rows_for(self.node2attribute))
        return be.Attributes.from_host(self._ctx(), self.node2attribute)

    def _node_keys(self):
        if isinstance(self.graph, LayoutGraph):
            return list(self.graph.keys)
        return [v for _, v in self.graph.nodes.data(self.node_key_attribute)]

    # ------------------------------------------------------- neighborhoods state ----
    @property
    def neighborhoods(self):
        """int64 [N,N] 0/1, C order (safe.py:387,430); downloaded from the device on first
        access after define_neighborhoods()."""
        if self._neighborhoods_host is None and self._nbr is not None:
            self._neighborhoods_host = self._nbr.to_dense()
        return self._neighborhoods_host

    @neighborhoods.setter
    def neighborhoods(self, value):
        self._invalidate_neighborhoods()
        self._neighborhoods_host = value
        if getattr(self, 'neighborhood_weighting', 'none') == 'custom':      # the weights went with the membership they were for
            self.neighborhood_weighting = 'none'

    @property
    def neighborhood_weights(self):
        """Additive, read-only: the weights of the members of every neighborhood as a scipy.sparse.csr_array, f64 [N, N], with
        the pattern of the membership -- a member at weight 0 is a stored zero -- or None under neighborhood_weighting = 'none'
        (and for a membership that carries no weights).  Fetched from the device on first read."""
        if getattr(self, 'neighborhood_weighting', 'none') == 'none':
            return None
        if self._weights_host is None:
            if self._nbr is None or not self._nbr.has_weights:
                return None
            indptr, indices = self._nbr.csr()
            self._weights_host = (indptr, indices, self._nbr.weights())
        from scipy import sparse
        indptr, indices, data = self._weights_host
        n = len(indptr) - 1
        return sparse.csr_array((data.copy(), indices.copy(), indptr.copy()), shape=(n, n))

    def set_neighborhood_weights(self, W):
        """Additive: custom weights for the members of the current neighborhoods (after define_neighborhoods, or an assigned
        `neighborhoods`).  W: scipy.sparse or dense [N, N], finite and >= 0; members W does not store get 0 and stay members.
        A wrong shape, a negative, NaN or infinite value, or a non-zero entry outside the membership is a ValueError that
        changes nothing.  Sets neighborhood_weighting = 'custom'."""
        nbr = self._device_neighborhoods()
        indptr, indices = nbr.csr()
        data = _member_weights(W, indptr, indices)
        nbr.set_weights(data)
        self._weights_host = (indptr, indices, data)
        self.neighborhood_weighting = 'custom'

    def _weighted(self):
        """True when compute_pvalues scores the neighborhoods with weights; ValueError when the setting asks for weights that
        the current membership does not carry."""
        if getattr(self, 'neighborhood_weighting', 'none') == 'none':
            return False
        if self._weights_host is None and (self._nbr is None or not self._nbr.has_weights):
            raise ValueError("neighborhood_weighting = '%s' but the neighborhoods carry no weights: call define_neighborhoods() "
                             "or set_neighborhood_weights()" % self.neighborhood_weighting)
        return True

    def _invalidate_neighborhoods(self):
        self._weights_host = None
        nd = self._node_distances
        if isinstance(nd, tuple) and nd[0] == 'device-shortpath':     # still on the device, owned by the handle that goes away
            self._node_distances = ('dense-shortpath', nd[1].distances()) if nd[1] is self._nbr and nd[1].handle else None
        if self._nbr is not None:
            self._nbr.close()
        self._nbr = None
        self._neighborhoods_host = None

    def _ctx(self):
        return be.Context.default(self.device)

    def _device_neighborhoods(self):
        if self._nbr is None:
            if self._neighborhoods_host is None:
                raise RuntimeError('neighborhoods are not defined: call define_neighborhoods() first')
            self._nbr = be.Neighborhoods.from_dense(self._ctx(), self._neighborhoods_host)
            if self._weights_host is not None:        # (an unpickled object: the weights travel as host arrays)
                self._nbr.set_weights(self._weights_host[2])
            try:                         # a layout, when the graph has one, only orders the nodes on the device
                xy = _graph_arrays(self.graph)[0]
                if xy.shape == (self._nbr.n, 2) and np.isfinite(xy).all():
                    self._nbr.set_layout(xy)
            except Exception:
                pass
        return self._nbr

    @property
    def node_distances(self):
        """Shortest-path metrics: dict-of-dicts {source: {target: distance}} over reached
        pairs (safe.py:417).  Euclidean (additive, via compute_node_distances): f64 [N,N]."""
        nd = self._node_distances
        if isinstance(nd, tuple) and nd[0] == 'device-shortpath':     # the [N,N] f64 copy (126 MB at 3971 nodes) is made on first read
            nd = self._node_distances = ('dense-shortpath', nd[1].distances())
        if isinstance(nd, tuple) and nd[0] == 'dense-shortpath':
            dmat = nd[1]
            rows, cols = np.nonzero(np.isfinite(dmat))
            out = {int(s): {} for s in range(dmat.shape[0])}
            for s, t in zip(rows.tolist(), cols.tolist()):
                out[s][t] = float(dmat[s, t])
            self._node_distances = out
        return self._node_distances

    @node_distances.setter
    def node_distances(self, value):
        self._node_distances = value

    def _override_neighborhood_settings(self, kwargs):
        for name in ('node_distance_metric', 'neighborhood_radius_type', 'neighborhood_radius', 'neighborhood_weighting',
                     'neighborhood_weight_bandwidth', 'diffusion_restart', 'diffusion_steps'):
            if name in kwargs:
                setattr(self, name, kwargs[name])
        self.validate_config()

    def _distance_source(self):
        """The _DistanceSource of the current node_distance_metric over the graph's arrays; no device work yet."""
        xy, eu, ev, length, weight = _graph_arrays(self.graph)
        ctx, metric = self._ctx(), self.node_distance_metric
        if metric == 'euclidean':
            return _LayoutDistances(ctx, xy)
        if metric == 'diffusion':
            return _NetworkDistances(ctx, xy, eu, ev, weight, diffusion=(self.diffusion_restart, self.diffusion_steps))
        if metric == 'shortpath_weighted_layout':
            return _NetworkDistances(ctx, xy, eu, ev, length)           # weight='length', missing -> 1 (networkx)
        return _NetworkDistances(ctx, xy, eu, ev, weight, diameter_in_layout_units=False)   # default weight attr 'weight', missing -> 1

    def _radius_type(self):
        return self.neighborhood_radius_type or 'diameter'              # None: the reference's default

    def _refuse_diffusion_diameter(self):
        """'diffusion' distances are 1 - a similarity, in [0, 1]: a fraction of the layout's extent ('diameter') means nothing."""
        if self.node_distance_metric == 'diffusion' and self._radius_type() == 'diameter':
            raise ValueError("neighborhood_radius_type = 'diameter' is not defined for node_distance_metric = 'diffusion' (the "
                             "distance does not come from a layout): use 'percentile', 'nearest' or 'absolute'")

    def _nearest_radii(self, src):
        """neighborhood_radius_type = 'nearest': every node's distance to its k-th nearest other node, f64 [N],
        k = int(neighborhood_radius)."""
        return src.nearest_radii(min(int(self.neighborhood_radius), 2 ** 62))

    def _set_nearest_radii(self, radii):
        self.neighborhood_radii = radii
        self.neighborhood_radius_resolved = float(np.median(radii))
        return self.neighborhood_radius_resolved

    def _resolve_radius(self, src):
        """The radius in distance units (the hop cutoff for 'shortpath') that neighborhood_radius stands for under
        neighborhood_radius_type; kept as self.neighborhood_radius_resolved."""
        kind = self._radius_type()
        self._refuse_diffusion_diameter()
        if kind == 'nearest':                           # one radius per node: the typical one stands for them
            return self._set_nearest_radii(self._nearest_radii(src))
        self.neighborhood_radii = None
        if kind == 'percentile':
            r = src.percentiles([self.neighborhood_radius])[0]
        elif kind == 'absolute':
            r = self.neighborhood_radius
        else:
            r = src.diameter_radius(self.neighborhood_radius)
        self.neighborhood_radius_resolved = float(r)
        return r

    def _build_neighborhoods(self, src):
        """The membership handle under the current radius type: A[i, j] = (D[i, j] <= r_i) for 'nearest', the source's rule
        against the resolved radius otherwise; sets neighborhood_radii and neighborhood_radius_resolved."""
        if self._radius_type() != 'nearest':
            return src.members(self._resolve_radius(src))
        radii = self._nearest_radii(src)
        nbr = src.members_rows(radii)
        self._set_nearest_radii(radii)
        return nbr

    def node_distance_percentile(self, q):
        """Additive: np.percentile(v, q) (linear method, bit for bit) of the distances v of all node pairs i < j under the
        current node_distance_metric -- scipy's pdist(xy) for 'euclidean', the finite all-pairs shortest-path lengths
        D[i, j] otherwise -- computed on the device without storing v.  q: a number or a sequence in [0, 100]; returns a
        float or an array.  What neighborhood_radius_type = 'percentile' resolves its radius with; touches neither
        neighborhoods nor node_distances nor any setting."""
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if qs.ndim != 1 or not all(_is_percentage(v) for v in qs.tolist()):
            raise ValueError('Percentiles must be in the range [0, 100]')
        with self._distance_source() as src:
            out = np.array(src.percentiles(qs.tolist()), dtype=np.float64)
        return float(out[0]) if np.ndim(q) == 0 else out

    def define_neighborhoods(self, **kwargs):
        """safepy/safe.py:369-430.  kwargs: node_distance_metric, neighborhood_radius_type,
        neighborhood_radius (persisted on self).  Sets self.neighborhoods (and, for the
        shortest-path metrics, self.node_distances); returns None.

        neighborhood_radius_type = 'nearest' (additive): k = int(neighborhood_radius); node i's radius r_i is the distance to its
        k-th nearest other node (the farthest reached one where fewer exist, 0.0 where none does; node i is left out by index, so a
        coincident node counts), and j is a member of row i iff D[i, j] <= r_i -- the diagonal always, every tie at the k-th
        distance, never an unreached node.  The membership is in general not symmetric.  Sets neighborhood_radii (f64 [N]) and
        neighborhood_radius_resolved (their median); node_distances holds the distances inside every node's own radius.

        node_distance_metric = 'diffusion' (additive), with the settings / keywords diffusion_restart (alpha, default 0.5, in (0, 1))
        and diffusion_steps (T, default 32, an integer >= 1; INI keys diffusionRestart / diffusionSteps): a layout-free, continuous
        distance from the truncated random-walk-with-restart kernel K = X_T of X_{t+1} = alpha I + (1 - alpha) S X_t, X_0 = I, S the
        symmetrically normalised adjacency (the 'weight' edge attribute, 1 where missing): D[i, j] = 1 - K[i, j] / sqrt(K[i, i] K[j, j]), +inf
        where no walk of at most T steps joins i and j, computed on the device in f64 with a fixed order of operations
        (include/safe_hip.h, safe_nbr_diffusion).  It orders nodes at equal hop distance by the number of paths that join them.
        Radius types 'percentile' (over the finite D[i, j], i < j), 'nearest' and 'absolute' (a radius in [0, 1) is a
        "1 - similarity") apply as for the shortest-path metrics, members are D <= radius, and node_distances holds the kept
        distances; 'diameter' is a ValueError before any device work.  Holds three N x N f64 matrices on the device at peak.

        neighborhood_weighting (additive; keyword or setting, default 'none' = flat neighborhoods and today's bytes), with
        neighborhood_weight_bandwidth (default 0.5, finite and > 0, read by 'gaussian' only): a distance-decay weight for every
        member k of every neighborhood i, from u = D[i, k] / r_i (u = 0 where r_i = 0), D the node distance of the metric and
        r_i = neighborhood_radius_resolved, or neighborhood_radii[i] under 'nearest':
          'uniform' 1 | 'triangular' max(0, 1 - u) | 'epanechnikov' max(0, 1 - u u) | 'gaussian' exp(-0.5 (u / h)^2)
        built on the device beside the membership and read back as neighborhood_weights.  A member at weight 0 stays a member.
        compute_pvalues then tests the weighted 'sum' score.  'custom' here is a ValueError: build the neighborhoods first, then
        call set_neighborhood_weights(W).  The shortest-path metrics build the weights from the N x N matrix the handle keeps."""
        self._override_neighborhood_settings(kwargs)
        self._refuse_diffusion_diameter()                # before any device work; nothing changes
        weighting = self.neighborhood_weighting
        if weighting == 'custom':                    # before any device work; nothing changes
            raise ValueError("neighborhood_weighting = 'custom' is not something define_neighborhoods can build: define the "
                             "neighborhoods under another setting (or 'none'), then give the weights to set_neighborhood_weights()")
        nearest = self._radius_type() == 'nearest'
        with self._distance_source() as src:
            if src.keeps_distances:
                self._node_distances = None          # replaced below (a copy still on the device is not fetched first)
            self._invalidate_neighborhoods()
            self.neighborhood_radii = None           # (a call that fails below leaves no radii of an earlier one behind)
            if nearest:
                self.neighborhood_radius_resolved = None
            self._nbr = self._build_neighborhoods(src)
            if src.layout_hint is not None:
                self._nbr.set_layout(src.layout_hint)
            if src.keeps_distances:
                self._node_distances = ('device-shortpath', self._nbr)
            if weighting != 'none':
                radii = self.neighborhood_radii if nearest else self.neighborhood_radius_resolved
                src.set_weights(self._nbr, weighting, radii, self.neighborhood_weight_bandwidth)
        if self.verbose:
            num_neighbors = self._nbr.row_counts()
            logging.info('Node distance metric: %s' % self.node_distance_metric)
            if nearest:
                logging.info('Neighborhood definition: %d nearest nodes' % int(self.neighborhood_radius))
                logging.info('Neighborhood radii in distance units (min / median / max): %r / %r / %r'
                             % (float(np.min(self.neighborhood_radii)), self.neighborhood_radius_resolved,
                                float(np.max(self.neighborhood_radii))))
            else:
                logging.info('Neighborhood definition: %.2f x %s' % (self.neighborhood_radius, self.neighborhood_radius_type))
            if self._radius_type() not in ('diameter', 'nearest'):
                logging.info('Neighborhood radius in distance units: %r' % self.neighborhood_radius_resolved)
            logging.info('Number of nodes per neighborhood (mean +/- std): %.2f +/- %.2f'
                         % (np.mean(num_neighbors), np.std(num_neighbors)))

    def compute_node_distances(self, **kwargs):
        """Additive (named by the north star; absent from the reference at this commit):
        fills self.node_distances without touching self.neighborhoods.  Euclidean: dense
        f64 [N,N] == squareform(pdist(xy)) (safe.py:397).  Shortest-path metrics: the same
        dict-of-dicts define_neighborhoods stores (safe.py:417)."""
        self._override_neighborhood_settings(kwargs)
        self._refuse_diffusion_diameter()
        with self._distance_source() as src:
            if not src.keeps_distances:
                self._node_distances = src.dense_distances(self._resolve_radius(src))
                return
            nbr = self._build_neighborhoods(src)     # its kept matrix: the distances inside the radius (every node's own under 'nearest')
            try:
                self._node_distances = ('dense-shortpath', nbr.distances())
            finally:
                nbr.close()

    # -------------------------------------------------------------- enrichment ----
    def compute_pvalues(self, **kwargs):
        """safepy/safe.py:432-472.

        attribute_transform = 'rank' (additive; keyword or setting, default 'none'): the test runs on the per-column midranks
        of node2attribute -- scipy.stats.rankdata(method='average', axis=0, nan_policy='omit'), NaN kept -- computed on the
        device after background = 'network' has been applied; node2attribute and a resident handle are not touched.  ns then
        holds rank sums (rank z-scores with neighborhood_score_type = 'z-score'), not sums of attribute values.
        how = 'analytic' on ranks is the tie-corrected Wilcoxon / Mann-Whitney rank-sum test of every attribute in every
        neighborhood, how = 'randomization' its permutation form.  'auto' still looks at the raw values; a hypergeometric
        route (how = 'hypergeometric', or 'auto' on 0/1 data) is refused with a ValueError: ranks are not counts.

        multiple_testing_scope (additive; keyword or setting, default 'attributes'; read only when multiple_testing is on): the
        family that one Benjamini-Hochberg run adjusts, on every route that honours multiple_testing.
          'attributes'     each node's row across the attributes -- np.apply_along_axis(lambda r: fdrcorrection(r)[1], 1, p), the
                           reference (safe.py:536-542, 599-605) and the bytes of a call without the keyword;
          'neighborhoods'  each attribute's column across the nodes (the same along axis 0): "in which neighborhoods is this
                           attribute enriched?", what num_neighborhoods_enriched and define_top_attributes read;
          'all'            the whole matrix as one family of N M tests -- fdrcorrection(p.ravel())[1].reshape(p.shape): "which
                           (node, attribute) calls can I trust?", what nes_binary and enriched_pairs are.
        nes, nes_binary and num_neighborhoods_enriched are recomputed from the adjusted values as for 'attributes', and the
        results stay on the device under lazy_outputs.  The NaN rule is the row rule applied to the family: one NaN p-value (a
        node without a score) turns its whole family NaN -- its column under 'neighborhoods', the WHOLE matrix under 'all'.
        The attribute-sharded drivers (safepy_amd.sharding, run_batch.py) keep the row scope and do not take the keyword.

        multiple_testing_method (additive; keyword, setting or INI key multipleTestingMethod, default 'fdr_bh' = today's bytes;
        read only when multiple_testing is on): the procedure that adjusts every family of multiple_testing_scope, each
        statsmodels' multipletests operation by operation, on every route that honours multiple_testing (randomization flat
        and weighted, both hypergeometric routes, how = 'analytic') at Benjamini-Hochberg's cost.
          'fdr_bh'      Benjamini-Hochberg: the false discovery rate under independence or positive dependence;
          'fdr_by'      Benjamini-Yekutieli: the false discovery rate under ANY dependence -- overlapping neighborhoods included --
                        BH with the constant sum 1 / i over the family (backend.by_constant);
          'holm'        Holm's step-down and
          'hochberg'    Hochberg's step-up procedure: the family-wise error rate;
          'bonferroni'  p times the size of the family: the family-wise error rate, element-wise.
        nes, nes_binary and num_neighborhoods_enriched come from the adjusted values through the same epilogue.  NaN rule:
        under 'fdr_bh', 'fdr_by' and 'hochberg' one NaN turns its family NaN (np.minimum.accumulate carries it); under 'holm'
        and 'bonferroni' only the NaN cell itself is NaN and the numbers are adjusted as members of the full family, NaNs
        counted.  What refuses multiple_testing refuses it under every method (familywise_adjustment = 'maxT' with it
        included); the attribute-sharded drivers and safe_extras keep 'fdr_bh' on rows and do not take the keyword.

        permutation_strata (additive; keyword or setting, default None = the free shuffle and its bytes; with
        permutation_strata_bins): a RESTRICTED permutation null for how = 'randomization' -- the attribute rows are shuffled only
        among nodes of one stratum, so an attribute that merely tracks a node property that also shapes the neighborhoods
        (degree, neighborhood size, batch, gene family) is not called enriched for that property's geography.
          array-like       one label per node in node order; any labels np.unique can order (ints, strings); None / NaN labels
                           and a wrong length raise ValueError;
          'neighborhood_size'  the nodes in ascending (size of their current neighborhood, node index) order, cut into
                           permutation_strata_bins (an int >= 1, default 10) groups by np.array_split; needs
                           define_neighborhoods first.
        The tables are generated on the device (backend.Permutations.stratified), every stratum shuffled on its own by the
        unseeded route's generator; everything behind the tables -- counting kernels, multiple_testing and its scope,
        attribute_transform = 'rank', background = 'network', both score types, the three signs, lazy_outputs -- is unchanged.
        Key: random_seed = None uses device_stream_key or OS entropy like the unseeded route; an integer random_seed IS the
        key (zero-extended to 64 bits) -- there is no NumPy stream to reproduce under strata, so a seeded stratified call is
        simply repeatable, and SAFE_HIP_DEVICE_STREAM=0 does not apply.  After the call permutation_strata_resolved (int32 [N]:
        every node's stratum, its rank among the distinct labels) and permutation_strata_sizes (int64 [S]: the rows that hold a
        value, per stratum) are set.  Refused with a ValueError that leaves every result as it was: how = 'analytic' (the
        stratified moments are not implemented), a hypergeometric route ('auto' on 0/1 data included: pass
        how = 'randomization'), more than 65535 rows that hold a value.  The attribute-sharded drivers do not take the
        keyword.

        neighborhood_weighting other than 'none' (additive; a setting of define_neighborhoods / set_neighborhood_weights): the
        neighborhoods carry weights and ns holds the weighted sums x_ij = sum_k w_ik v_kj, added over the members in ascending
        node order.  how = 'analytic' evaluates the exact permutation moments of that weighted sum (mean W1_i mu_j, variance
        (n_v W2_i - W1_i^2) / (n_v (n_v - 1)) Q_j) and normal tails; how = 'randomization', and 'auto' on values other than
        0/1, count the permuted weighted scores.  multiple_testing and its scope, permutation_strata, attribute_transform =
        'rank', background = 'network', the three signs and lazy_outputs work as without weights.  Refused with a ValueError
        before any result changes: a hypergeometric route ('auto' on 0/1 data included: pass how = 'analytic' or
        how = 'randomization') and neighborhood_score_type = 'z-score'.  safe_extras, safepy_amd.sharding and run_batch.py do
        not take the setting: they score flat neighborhoods.

        familywise_adjustment = 'maxT' (additive; keyword or setting, default 'none' = today's bytes; with familywise_scope):
        Westfall-Young single-step max-statistic adjusted p-values on the randomization route.  Every permutation is a joint
        draw of all N scores of a column, so comparing each observed statistic with the per-permutation extreme over the whole
        family controls the family-wise error rate under any dependence between the overlapping neighborhoods.  The scores
        are made comparable across neighborhoods of different sizes by their exact permutation mean and variance (those of
        how = 'analytic'): z = (S - loc_i mu_j) / sqrt(scale_i Q_j).
          familywise_scope = 'neighborhoods' (default)  the family is the N neighborhoods of one attribute;
          familywise_scope = 'all'                      the family is all N M cells.
        ns is the observed score; pvalues_pos = #{p : max over the family of z_p >= z_obs} / P and pvalues_neg = #{p : min over
        the family of z_p <= z_obs} / P; nes, nes_binary and num_neighborhoods_enriched follow from them through the usual
        epilogue (its 1 / P substitution included) for all three attribute_sign values; a cell that cannot vary gets p = 1.
        attributes['familywise_pvalue_pos'] / ['familywise_pvalue_neg'] hold the smallest adjusted p-value of every attribute --
        its p-value for "enriched (depleted) somewhere on the network" -- and familywise_statistic the observed z [N, M], on
        the device until read like the other results.  permutation_strata, attribute_transform = 'rank', background =
        'network', neighborhood_weighting and every kind of permutation table work unchanged.  Under permutation_strata the
        standardiser stays the unrestricted moments: the adjustment is valid with any fixed per-cell transform, because the
        observed and the permuted scores pass through the same one.  Refused with a ValueError before any device work, every
        result left as it was: how = 'analytic', a hypergeometric route ('auto' on 0/1 data included: pass
        how = 'randomization'), neighborhood_score_type = 'z-score', and multiple_testing = True.  The attribute-sharded
        drivers and safe_extras do not take the keyword."""
        for name in ('permutation_strata', 'permutation_strata_bins'):
            if name in kwargs:
                setattr(self, name, kwargs[name])
        if 'multiple_testing_scope' in kwargs:
            self.multiple_testing_scope = kwargs['multiple_testing_scope']
        if 'multiple_testing_method' in kwargs:
            self.multiple_testing_method = kwargs['multiple_testing_method']
        for name in ('familywise_adjustment', 'familywise_scope'):
            if name in kwargs:
                setattr(self, name, kwargs[name])
        if 'how' in kwargs:
            self.enrichment_type = kwargs['how']
        if 'neighborhood_score_type' in kwargs:
            self.neighborhood_score_type = kwargs['neighborhood_score_type']
        if 'multiple_testing' in kwargs:
            self.multiple_testing = kwargs['multiple_testing']
        if 'background' in kwargs:
            self.background = kwargs['background']
        if 'hypergeom_tails' in kwargs:
            self.hypergeom_tails = kwargs['hypergeom_tails']
        if 'attribute_transform' in kwargs:
            self.attribute_transform = kwargs['attribute_transform']
        self.validate_config()
        if self.enrichment_type == 'analytic':
            self._require_sum_scores_for_moments()             # before any device work
        ranked = self.attribute_transform == 'rank'
        if ranked and self.enrichment_type == 'hypergeometric':
            self._refuse_hypergeom_on_ranks()                  # before any device work
        stratified = self.permutation_strata is not None
        if stratified:                                         # before any device work, too
            if self.enrichment_type == 'analytic':
                raise ValueError("permutation_strata does not go with how = 'analytic': the stratified permutation moments are "
                                 "not implemented; use how = 'randomization'")
            if self.enrichment_type == 'hypergeometric':
                self._refuse_hypergeom_on_strata()
            self._resolve_permutation_strata(self.node2attribute.shape[0], check_only=True)     # (bad labels are refused here)
        weighted = self._weighted()                            # before any device work, too
        if weighted:
            self._require_sum_scores_for_weights()
            if self.enrichment_type == 'hypergeometric':
                self._refuse_hypergeom_on_weights()
        maxt = self.familywise_adjustment == 'maxT'            # before any device work, too
        if maxt:
            self._require_randomization_sums_for_maxt()
            if self.enrichment_type == 'hypergeometric':
                self._refuse_hypergeom_on_maxt()

        resident = self._resident_attributes()
        if self.background == 'network':
            logging.info('Setting all null attribute values to 0. Using the network as background for enrichment.')
            if be._is_sparse(self.node2attribute):
                # the sparse form of the same step: the missing rows become rows of zeros (nothing stored), stored NaNs
                # become stored zeros -- on the host object and on the resident handle; never densified
                if resident is not None:
                    resident.nan_to_zero()
                a = self.node2attribute
                if a.format not in ('csc', 'csr', 'coo'):
                    raise TypeError("background='network' edits the stored values of the sparse node2attribute in place and knows "
                                    "the CSC, CSR and COO layouts; convert this %s with .tocsc()" % type(a).__name__)
                missing = self._missing_rows_for(a)
                if missing is not None and missing.any():                 # what a missing row stores is missing too: NaN -> 0
                    rows = {'csc': lambda: a.indices, 'coo': lambda: a.row,
                            'csr': lambda: np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))}[a.format]()
                    a.data[missing[rows] != 0] = 0
                self._missing_rows = None
                if np.issubdtype(a.data.dtype, np.floating):
                    a.data[np.isnan(a.data)] = 0
            else:
                if resident is not None:                                       # both copies, the host one stays read-only
                    resident.nan_to_zero()
                    self.node2attribute.flags.writeable = True
                if np.issubdtype(self.node2attribute.dtype, np.floating):      # (a uint8 / bool matrix has no missing values)
                    self.node2attribute[np.isnan(self.node2attribute)] = 0     # in place, like safe.py:451
                if resident is not None:
                    self.node2attribute.flags.writeable = False

        raw = resident if resident is not None else self._upload_attributes()
        attr = raw
        try:
            stats = raw.stats()
            if stats['max_nan_col'] / self.node2attribute.shape[0] > 0.5:
                logging.warning("WARNING: more than 50% of nodes in the network are set to NaN and "
                                "will be ignored for calculating enrichment.\n"
                                "Consider setting sf.background = 'network'.")
            hypergeom = (self.enrichment_type == 'hypergeometric') or \
                ((self.enrichment_type == 'auto') and (stats['n_other'] == 0))      # ('auto' looks at the raw values)
            if stratified and hypergeom:
                self._refuse_hypergeom_on_strata()
            if weighted and hypergeom:
                self._refuse_hypergeom_on_weights()
            if maxt and hypergeom:
                self._refuse_hypergeom_on_maxt()
            if ranked:
                if hypergeom:
                    self._refuse_hypergeom_on_ranks()
                attr = raw.rank()
            self._pending_binary = None
            if self.enrichment_type == 'analytic':              # additive and opt-in: 'auto' never chooses it
                self.compute_pvalues_by_moments(_attr=attr, **kwargs)
            elif hypergeom:
                self.compute_pvalues_by_hypergeom(_attr=attr, **kwargs)
            else:
                self.compute_pvalues_by_randomization(_attr=attr, **kwargs)
        finally:
            if attr is not raw:
                attr.close()
            if resident is None:
                raw.close()

        # safe.py:468-472 -- computed by the same kernels, from the same nes
        self.nes_binary, enriched = self._pending_binary
        self._pending_binary = None
        if self.attributes is None:
            self.attributes = pd.DataFrame({'id': np.arange(len(enriched)), 'name': [str(j) for j in range(len(enriched))]})
        self.attributes['num_neighborhoods_enriched'] = enriched

    def _result(self, buf, shape):
        """A finished [n, m] device buffer as the value of a result attribute: left on the device
        (lazy_outputs, the default) or copied to the host right away."""
        return _DeviceResult(buf, shape) if self.lazy_outputs else buf.download(shape)

    def _fdr_adjust(self, ctx, n, m, num_permutations, out_ptrs):
        """multiple_testing on the randomization and the upper-tail hypergeometric route: Benjamini-Hochberg along
        multiple_testing_scope, then nes, nes_binary and the counts from the adjusted values.  The library chooses the form of
        every scope; 'attributes' gives the bytes of backend.fdr_adjust, the reference's behaviour.  Another
        multiple_testing_method takes the same path with its own per-entry arithmetic (backend.mt_adjust_scope)."""
        if self.multiple_testing_method == 'fdr_bh':
            be.fdr_adjust_scope(ctx, n, m, num_permutations, self.attribute_sign, self.enrichment_threshold,
                                self.multiple_testing_scope, out_ptrs)
        else:
            be.mt_adjust_scope(ctx, n, m, num_permutations, self.attribute_sign, self.enrichment_threshold,
                               self.multiple_testing_scope, self.multiple_testing_method, out_ptrs)

    def compute_pvalues_by_randomization(self, _attr=None, **kwargs):
        """safepy/safe.py:474-554 (no 1 s sleep, no multiprocessing split: `processes` is
        accepted and ignored -- the reference's own split is broken at this commit)."""
        if kwargs:
            logging.warning('Current settings (possibly overwriting global ones):')
            for k in kwargs:
                logging.warning('\t%s=%s' % (k, str(kwargs[k])))
        logging.info('Using randomization to calculate enrichment...')
        if 'num_permutations' in kwargs:
            self.num_permutations = kwargs['num_permutations']
        for name in ('permutation_strata', 'permutation_strata_bins', 'familywise_adjustment', 'familywise_scope'):
            if name in kwargs:
                setattr(self, name, kwargs[name])
        self.validate_config()
        score_type = 'z-score' if self.neighborhood_score_type == 'z-score' else 'sum'
        weighted = self._weighted()                        # (refusals come before any device work)
        if weighted:
            self._require_sum_scores_for_weights()
        maxt = self.familywise_adjustment == 'maxT'
        if maxt:
            self._require_randomization_sums_for_maxt(direct=True)

        strata = None
        if self.permutation_strata is not None:            # (refusals come before any device work)
            strata = self._resolve_permutation_strata(_attr.n if _attr is not None else self.node2attribute.shape[0])
        ctx = self._ctx()
        nbr = self._device_neighborhoods()
        attr = _attr if _attr is not None else self._upload_attributes()
        n, m = attr.n, attr.m
        try:
            perms = self._permutations(ctx, attr, strata)
        except Exception:
            if _attr is None:
                attr.close()
            raise
        bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
        try:
            if maxt:                                   # the adjusted counts, then the epilogue every count route shares
                self._maxt_counts(ctx, nbr, attr, perms, weighted, bufs)
            elif weighted:                             # the weighted counts, then the epilogue every count route shares
                counts = [ctx.alloc_f64(n, m) for _ in range(2)]
                try:
                    be.permtest_counts_weighted(ctx, nbr, attr, perms, bufs[0].ptr, counts[0].ptr, counts[1].ptr)
                    be.outputs_from_counts(ctx, n, m, self.num_permutations, self.attribute_sign, self.enrichment_threshold,
                                           counts[0].ptr, counts[1].ptr, bufs[0].ptr, [b.ptr for b in bufs[1:]])
                finally:
                    for b in counts:
                        b.free()
            else:
                be.randomization(ctx, nbr, attr, perms, score_type, self.attribute_sign, self.enrichment_threshold,
                                 [b.ptr for b in bufs])
            if self.multiple_testing:                 # safe.py:536-542, then 546-554 and 468-472 on the adjusted values
                logging.info('Running FDR-adjustment of p-values...')
                self._fdr_adjust(ctx, n, m, self.num_permutations, [b.ptr for b in bufs[1:]])
            enriched = bufs[5].download((m,))
            res = [self._result(b, (n, m)) for b in bufs[:5]]
            bufs = bufs[5:] if self.lazy_outputs else bufs       # handed over: the results own their buffers now
            self.ns, self.pvalues_neg, self.pvalues_pos, self.nes = res[:4]
            self._pending_binary = (res[4], enriched)
            if maxt:
                self._publish_maxt(n, m)
        finally:
            self._maxt_pending = None
            for b in bufs:
                b.free()
            perms.close()
            if _attr is None:
                attr.close()

    def _maxt_counts(self, ctx, nbr, attr, perms, weighted, bufs):
        """familywise_adjustment = 'maxT': the observed score, the extremes of the standardised permuted scores of all M columns
        (familywise_scope = 'all' needs them complete), the adjusted counts and the shared epilogue into bufs = (ns,
        pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched).  The observed statistic and the columns' smallest counts
        wait in _maxt_pending until the results are published."""
        n, m, P = attr.n, attr.m, self.num_permutations
        z = ctx.alloc_f64(n, m)
        work = [ctx.alloc(n * m), ctx.alloc_f64(P, m), ctx.alloc_f64(P, m), ctx.alloc_f64(n, m), ctx.alloc_f64(n, m), ctx.alloc_f64(2 * m)]
        live, tmax, tmin, neg, pos, least = work
        try:
            if weighted:
                be.score_weighted(ctx, nbr, attr, bufs[0].ptr)
            else:
                be.score(ctx, nbr, attr, 'sum', bufs[0].ptr)
            be.permtest_extremes(ctx, nbr, attr, perms, z.ptr, live.ptr, tmax.ptr, tmin.ptr)
            be.counts_from_extremes(ctx, n, m, P, self.familywise_scope, z.ptr, live.ptr, tmax.ptr, tmin.ptr, neg.ptr, pos.ptr,
                                    least.ptr, least.ptr + 8 * m)
            be.outputs_from_counts(ctx, n, m, P, self.attribute_sign, self.enrichment_threshold, neg.ptr, pos.ptr, bufs[0].ptr,
                                   [b.ptr for b in bufs[1:]])
            self._maxt_pending = (z, least.download((2, m)) / P)
        except Exception:
            z.free()
            raise
        finally:
            for b in work:
                b.free()

    def _publish_maxt(self, n, m):
        z, least = self._maxt_pending
        self.familywise_statistic = self._result(z, (n, m))
        if not self.lazy_outputs:
            z.free()
        if self.attributes is None:
            self.attributes = pd.DataFrame({'id': np.arange(m), 'name': [str(j) for j in range(m)]})
        self.attributes['familywise_pvalue_neg'] = least[0]
        self.attributes['familywise_pvalue_pos'] = least[1]

    def _require_randomization_sums_for_maxt(self, direct=False):
        if self.enrichment_type == 'analytic' and not direct:
            raise ValueError("familywise_adjustment = 'maxT' compares with the extremes of the permuted scores; how = 'analytic' "
                             "draws no permutation: pass how = 'randomization'")
        if self.neighborhood_score_type == 'z-score':
            raise ValueError("familywise_adjustment = 'maxT' is defined for neighborhood_score_type = 'sum' only (it standardises "
                             "the sums with their exact permutation moments); it does not go with 'z-score'")
        if self.multiple_testing:
            raise ValueError("familywise_adjustment = 'maxT' and multiple_testing = True are two corrections of the same p-values: "
                             "choose one")

    def _refuse_hypergeom_on_maxt(self):
        raise ValueError("familywise_adjustment = 'maxT' compares with the extremes of the permuted scores; this call takes the "
                         "hypergeometric test (how = '%s'%s), which has none: pass how = 'randomization'"
                         % (self.enrichment_type, ' on 0/1 attribute values' if self.enrichment_type == 'auto' else ''))

    def compute_pvalues_by_hypergeom(self, _attr=None, **kwargs):
        """safepy/safe.py:556-608.  Sets pvalues_pos and nes only (ns / pvalues_neg untouched) -- the reference's behaviour,
        hypergeom_tails = 'upper' (the default).  hypergeom_tails = 'attribute_sign' (additive; 0/1 data, NaN allowed) makes the
        test follow attribute_sign the way the randomization route does: ns, pvalues_pos = P[H >= x], pvalues_neg = P[H <= x],
        nes = -log10 of the side the sign names ('both': the difference), multiple_testing adjusts both matrices."""
        if kwargs:
            if 'verbose' in kwargs:
                self.verbose = kwargs['verbose']
            if 'hypergeom_tails' in kwargs:
                self.hypergeom_tails = kwargs['hypergeom_tails']
            if self.verbose:
                logging.warning('Overwriting global settings:')
                for k in kwargs:
                    logging.warning('\t%s=%s' % (k, str(kwargs[k])))
        self.validate_config()
        if self._weighted():                               # before any device work
            self._refuse_hypergeom_on_weights()
        if self.verbose:
            logging.info('Using the hypergeometric test to calculate enrichment...')
        ctx = self._ctx()
        nbr = self._device_neighborhoods()
        attr = _attr if _attr is not None else self._upload_attributes()
        n, m = attr.n, attr.m
        if self.hypergeom_tails == 'attribute_sign':
            try:
                self._hypergeom_both_tails(ctx, nbr, attr)
            finally:
                if _attr is None:
                    attr.close()
            return
        bufs = [ctx.alloc_f64(n, m) for _ in range(3)] + [ctx.alloc_f64(m)]
        try:
            be.hypergeom(ctx, nbr, attr, self.enrichment_threshold, [b.ptr for b in bufs])
            if self.multiple_testing:                  # safe.py:599-605, then 608 and 468-472 on the adjusted values
                if self.verbose:
                    logging.info('Running FDR-adjustment of p-values...')
                self._fdr_adjust(ctx, n, m, 0, [None] + [b.ptr for b in bufs])
            enriched = bufs[3].download((m,))
            res = [self._result(b, (n, m)) for b in bufs[:3]]
            bufs = bufs[3:] if self.lazy_outputs else bufs       # handed over: the results own their buffers now
            self.pvalues_pos, self.nes = res[:2]
            self._pending_binary = (res[2], enriched)
        finally:
            for b in bufs:
                b.free()
            if _attr is None:
                attr.close()

    def _permutations(self, ctx, attr, strata):
        """The permutation tables of a randomization call over the rows of `attr` that hold a value.  strata = None: the free
        shuffle -- the NumPy-compatible stream of an integer random_seed, or (random_seed = None, the default, like the
        reference's) tables generated on the device; `device_stream_key` (None = OS entropy) makes such a run repeatable for
        tests and debugging.  strata = int32 [N] ranks: restricted permutations generated on the device, keyed by the integer
        random_seed or, without one, like the unseeded route; sets permutation_strata_resolved / permutation_strata_sizes."""
        flags = attr.row_flags()
        if strata is None:
            return be.Permutations(ctx, attr.n, flags, self.num_permutations, self.random_seed,
                                   device_key=getattr(self, 'device_stream_key', None))
        movable = int(np.count_nonzero(flags))
        if movable > 65535:
            raise ValueError('permutation_strata: %d rows hold a value, the restricted permutations are generated for at most '
                             '65535' % movable)
        key = getattr(self, 'device_stream_key', None)
        if self.random_seed is not None:
            key = int(self.random_seed)
            if key < 0 or key > 0xFFFFFFFF:
                raise ValueError('Seed must be between 0 and 2**32 - 1')
        perms = be.Permutations.stratified(ctx, attr.n, flags, strata, self.num_permutations, key)
        self.permutation_strata_resolved = strata
        self.permutation_strata_sizes = np.bincount(strata[flags != 0], minlength=int(strata.max()) + 1).astype(np.int64)
        return perms

    def _resolve_permutation_strata(self, n, check_only=False):
        """int32 [N]: every node's stratum under the current permutation_strata setting (not None).  ValueError for labels that
        do not fit the nodes and for 'neighborhood_size' without neighborhoods.  check_only: the refusals alone, nothing read
        from the device."""
        if isinstance(self.permutation_strata, str):       # 'neighborhood_size' (validate_config)
            if self._nbr is None and self._neighborhoods_host is None:
                raise ValueError("permutation_strata = 'neighborhood_size' needs neighborhoods: call define_neighborhoods() first")
            if check_only:
                return None
            counts = self._device_neighborhoods().row_counts()
            if len(counts) != n:
                raise ValueError('permutation_strata: the neighborhoods cover %d nodes, the attributes %d' % (len(counts), n))
            return _neighborhood_size_strata(counts, int(self.permutation_strata_bins))
        return _factorise_strata(self.permutation_strata, n)

    def _refuse_hypergeom_on_strata(self):
        raise ValueError("permutation_strata restricts the permutations of the randomization test; this call takes the "
                         "hypergeometric test (how = '%s'%s), which has none: pass how = 'randomization'"
                         % (self.enrichment_type, ' on 0/1 attribute values' if self.enrichment_type == 'auto' else ''))

    def _refuse_hypergeom_on_weights(self):
        raise ValueError("neighborhood_weighting = '%s' scores neighborhoods with real weights; this call takes the "
                         "hypergeometric test (how = '%s'%s), which counts members: pass how = 'analytic' or how = 'randomization'"
                         % (self.neighborhood_weighting, self.enrichment_type,
                            ' on 0/1 attribute values' if self.enrichment_type == 'auto' else ''))

    def _require_sum_scores_for_weights(self):
        if self.neighborhood_score_type == 'z-score':
            raise ValueError("neighborhood_weighting = '%s' is defined for neighborhood_score_type = 'sum' only; use "
                             "neighborhood_weighting = 'none' with 'z-score'" % self.neighborhood_weighting)

    def _require_sum_scores_for_moments(self):
        if self.neighborhood_score_type != 'sum':
            raise ValueError("how = 'analytic' is defined for neighborhood_score_type = 'sum' only (the permutation null of "
                             "'%s' is not a sum of draws); use how = 'randomization'" % self.neighborhood_score_type)

    def _refuse_hypergeom_on_ranks(self):
        raise ValueError("attribute_transform = 'rank' does not go with the hypergeometric test (how = '%s'%s): ranks are not "
                         "counts; use how = 'analytic' or how = 'randomization', or attribute_transform = 'none'"
                         % (self.enrichment_type, ' on 0/1 attribute values' if self.enrichment_type == 'auto' else ''))

    def compute_pvalues_by_moments(self, _attr=None, **kwargs):
        """how = 'analytic' (additive; no counterpart in the reference): the randomization test of 'sum' scores without
        permutations.  The null that run_permutations samples (safe_extras.py:36-70) has closed-form mean and variance per
        cell; pvalues_pos / pvalues_neg are the normal tails of the exact z, so they are deterministic, need no seed and run
        down to the smallest double instead of 1 / num_permutations (num_permutations and random_seed are ignored).  Sets ns,
        pvalues_neg, pvalues_pos, nes and nes_binary under the rules of hypergeom_tails = 'attribute_sign'; multiple_testing
        adjusts every row of both p matrices.  neighborhood_score_type = 'z-score' is refused: its null is not a sum."""
        if kwargs:
            if 'verbose' in kwargs:
                self.verbose = kwargs['verbose']
            if 'neighborhood_score_type' in kwargs:
                self.neighborhood_score_type = kwargs['neighborhood_score_type']
            if self.verbose:
                logging.warning('Overwriting global settings:')
                for k in kwargs:
                    logging.warning('\t%s=%s' % (k, str(kwargs[k])))
        self.validate_config()
        self._require_sum_scores_for_moments()                   # before any device work
        test = be.moments_test_weighted if self._weighted() else be.moments_test
        if self.verbose:
            logging.info('Using the exact permutation moments to calculate enrichment...')
        ctx = self._ctx()
        nbr = self._device_neighborhoods()
        attr = _attr if _attr is not None else self._upload_attributes()
        try:
            self._two_sided_results(ctx, attr.n, attr.m, lambda out_ptrs: test(
                ctx, nbr, attr, self.attribute_sign, self.enrichment_threshold, out_ptrs))
        finally:
            if _attr is None:
                attr.close()

    def _hypergeom_both_tails(self, ctx, nbr, attr):
        """hypergeom_tails = 'attribute_sign': ns, both p matrices, the signed nes and its binarisation from one device call
        (backend.hypergeom_tails), finished by _two_sided_results."""
        if attr.stats()['n_other'] != 0:                   # before anything is launched
            raise ValueError("hypergeom_tails = 'attribute_sign' needs 0/1 attribute values (NaN allowed): the matrix holds "
                             "%d other values" % attr.stats()['n_other'])
        self._two_sided_results(ctx, attr.n, attr.m, lambda out_ptrs: be.hypergeom_tails(
            ctx, nbr, attr, self.attribute_sign, self.enrichment_threshold, out_ptrs))

    def _two_sided_results(self, ctx, n, m, device_call):
        """The part the two-sided tests share (hypergeom_tails = 'attribute_sign', how = 'analytic'): device_call(out_ptrs) fills
        (ns, pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched); multiple_testing adjusts both p matrices along
        multiple_testing_scope (by default every row: fdrcorrection(row)[1], as safe.py:538-542 does for randomization) and recomputes nes, nes_binary and the counts from the
        adjusted values; the matrices become the results, on the device until read."""
        bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
        try:
            device_call([b.ptr for b in bufs])
            if self.multiple_testing:
                if self.verbose:
                    logging.info('Running FDR-adjustment of p-values...')
                for b in bufs[1:3]:
                    if self.multiple_testing_method == 'fdr_bh':
                        be.fdr_adjust_matrix(ctx, n, m, self.multiple_testing_scope, b.ptr)
                    else:
                        be.mt_adjust_matrix(ctx, n, m, self.multiple_testing_scope, self.multiple_testing_method, b.ptr)
                be.hypergeom_outputs(ctx, n, m, self.attribute_sign, self.enrichment_threshold, bufs[1].ptr, bufs[2].ptr,
                                     [b.ptr for b in bufs[3:]])
            enriched = bufs[5].download((m,))
            res = [self._result(b, (n, m)) for b in bufs[:5]]
            bufs = bufs[5:] if self.lazy_outputs else bufs       # handed over: the results own their buffers now
            self.ns, self.pvalues_neg, self.pvalues_pos, self.nes = res[:4]
            self._pending_binary = (res[4], enriched)
        finally:
            for b in bufs:
                b.free()

    # ------------------------------------------------------------------------------------
    # consumers of nes_binary
    # ------------------------------------------------------------------------------------
    def _graph_edges(self):
        """Edge list used for the connectivity of enriched nodes: self.graph, or the Euclidean
        pseudo-network of .scatter inputs when one is set (safe.py:643-645)."""
        g = getattr(self, 'graph_euclidean', None)
        if g is None:
            g = self.graph
        if isinstance(g, LayoutGraph):
            return g.edge_u, g.edge_v
        eu = np.fromiter((u for u, _ in g.edges()), dtype=np.int64, count=g.number_of_edges())
        ev = np.fromiter((v for _, v in g.edges()), dtype=np.int64, count=g.number_of_edges())
        return eu, ev

    def _within_reach(self):
        """The within-reach relation of attribute_unimodality_metric = 'radius' as a device membership handle (the caller closes
        it): what define_neighborhoods would build under the current node_distance_metric with the radius
        t = attribute_unimodality_radius_multiple x neighborhood_radius_resolved in place of the radius -- the same constructors,
        so `<` against `<=`, the kept diagonal and unreached pairs are the neighborhood rule.  Returns (handle, t, '<' or '<=')."""
        with self._distance_source() as src:
            r = self._resolve_radius(src)
            t = float(self.attribute_unimodality_radius_multiple) * float(r)
            if not np.isfinite(t):
                raise ValueError("attribute_unimodality_metric = 'radius' needs a finite neighborhood radius: it resolved to %r "
                                 '(does every node have x and y coordinates?)' % (r,))
            src.check_reach(r, t)
            return src.members(t, keep_distances=False), t, src.rule

    def _enriched_pair_counts(self, cand):
        """(pairs, within) int64 [len(cand)] of the candidate columns `cand` of nes_binary: the unordered pairs of a column's
        enriched nodes (nes_binary > 0), and those of them that are within reach of each other.  One device call on the
        device-resident nes_binary while nobody has read it (it stays there), else on the host slice."""
        ctx = self._ctx()
        within_nbr, t, rule = self._within_reach()
        try:
            if self.verbose:
                logging.info('Within reach: %s distance %s %r (%r x the neighborhood radius %r)'
                             % (self.node_distance_metric, rule, t,
                                self.attribute_unimodality_radius_multiple, self.neighborhood_radius_resolved))
            src = self.__dict__.get('_r_nes_binary')
            if isinstance(src, _DeviceResult) and cand.dtype.kind in 'iu' and cand.min() >= 0 and cand.max() < src.shape[1]:
                if src.shape[0] != within_nbr.n:
                    raise ValueError('nes_binary has %d rows, the network %d nodes' % (src.shape[0], within_nbr.n))
                q, e, _ = ctx.enriched_pair_counts_dev(within_nbr, src.buf.ptr, src.shape[0], src.shape[1], cand)
            else:
                q, e = be.enriched_pair_counts(ctx, within_nbr, self.nes_binary[:, cand])
        finally:
            within_nbr.close()
        # W is symmetric with a full diagonal: q counts every unordered pair twice and every enriched node once
        return e * (e - 1) // 2, (q - e) // 2

    def define_top_attributes(self, **kwargs):
        """safepy/safe.py:610-659.  kwargs: attribute_unimodality_metric, attribute_enrichment_min_size,
        attribute_unimodality_radius_multiple, attribute_unimodality_min_fraction.

        'connectivity' (the default, the reference's): adds the columns 'top', 'num_connected_components',
        'size_connected_components' (object: sizes in descending order) and 'num_large_connected_components' to
        self.attributes.  The connected components of all candidate attributes are found in one device call, straight from the
        device-resident nes_binary while nobody has read it (it stays on the device).

        'radius' (additive; the reference reads the setting and ignores it): an attribute stays top when at least
        attribute_unimodality_min_fraction of the pairs of its enriched nodes are within reach of each other -- within
        attribute_unimodality_radius_multiple x neighborhood_radius_resolved under the current node_distance_metric, by the
        rule define_neighborhoods applies to its own radius.  Adds 'top', 'num_enriched_pairs', 'num_enriched_pairs_within'
        (int64) and 'fraction_enriched_pairs_within' (f64); attributes that fail requirement 1 get 0, 0 and NaN.  All candidate
        attributes are counted in one device call (backend.enriched_pair_counts).  Raises, with self.attributes untouched, when
        the relation cannot be built (no usable coordinates, a refusal of the constructor).

        Any other value skips requirement 2, as in the reference."""
        for option in ('attribute_unimodality_metric', 'attribute_enrichment_min_size', 'attribute_unimodality_radius_multiple',
                       'attribute_unimodality_min_fraction'):
            if option in kwargs:
                setattr(self, option, kwargs[option])
        self.validate_config()
        min_size = self.attribute_enrichment_min_size
        if self.verbose:
            logging.info('Top attributes need >= %d enriched neighborhoods that form one region (%s)'
                         % (min_size, self.attribute_unimodality_metric))
        attrs = self.attributes
        if self.attribute_unimodality_metric == 'radius':
            top = np.asarray((attrs['num_neighborhoods_enriched'] >= min_size).values, dtype=bool)   # requirement 1
            m_all = len(attrs)
            pairs = np.zeros(m_all, dtype=np.int64)
            within = np.zeros(m_all, dtype=np.int64)
            cand = attrs.index.values[top]
            if len(cand):
                pairs[top], within[top] = self._enriched_pair_counts(cand)
            min_fraction = float(self.attribute_unimodality_min_fraction)
            with np.errstate(invalid='ignore', divide='ignore'):
                fraction = np.where(top, within.astype(np.float64) / pairs.astype(np.float64), np.nan)
            fails = top & (within.astype(np.float64) < min_fraction * pairs.astype(np.float64))
            if self.verbose:
                logging.info('One region: >= %r of the pairs of enriched neighborhoods within reach (%d of %d candidates fail)'
                             % (min_fraction, np.count_nonzero(fails), np.count_nonzero(top)))
            attrs['top'] = top & ~fails
            attrs['num_enriched_pairs'] = pairs
            attrs['num_enriched_pairs_within'] = within
            attrs['fraction_enriched_pairs_within'] = fraction
            if self.verbose:
                logging.info('Number of top attributes: %d' % np.sum(attrs['top']))
            return
        attrs['top'] = (attrs['num_neighborhoods_enriched'] >= min_size).values           # requirement 1 (safe.py:628-629)

        if self.attribute_unimodality_metric == 'connectivity':                         # requirement 2 (safe.py:632-656)
            m_all = len(attrs)
            num_cc = np.zeros(m_all, dtype=np.int64)
            num_large = np.zeros(m_all, dtype=np.int64)
            sizes = np.empty(m_all, dtype=object)
            sizes[:] = None
            # like the reference, attribute index values are column positions of nes_binary
            cand = attrs.index.values[attrs['top'].values]
            if len(cand):
                eu, ev = self._graph_edges()
                src = self.__dict__.get('_r_nes_binary')
                if isinstance(src, _DeviceResult) and cand.dtype.kind in 'iu' and cand.min() >= 0 and cand.max() < src.shape[1]:
                    # the candidate columns are read in place on the device: nes_binary stays there
                    labels, _ = self._ctx().enriched_components_dev(src.buf.ptr, src.shape[0], src.shape[1], cand, eu, ev)
                else:
                    n = self.nes_binary.shape[0]
                    labels = be.enriched_components(self._ctx(), n, eu, ev, self.nes_binary[:, cand])
                pos_of = {a: i for i, a in enumerate(attrs.index.values)}
                for row, a in enumerate(cand):
                    lab = labels[row]
                    comp = np.bincount(lab[lab >= 0])
                    comp = np.sort(comp[comp > 0])[::-1]                  # (a few components, not the n bins, are sorted)
                    i = pos_of[a]
                    num_cc[i] = len(comp)
                    sizes[i] = comp
                    num_large[i] = int(np.sum(comp >= min_size))
            attrs['num_connected_components'] = num_cc
            attrs['size_connected_components'] = sizes
            attrs['num_large_connected_components'] = num_large
            attrs.loc[attrs['num_connected_components'] > 1, 'top'] = False              # safe.py:656
        if self.verbose:
            logging.info('Number of top attributes: %d' % np.sum(attrs['top']))

    def define_domains(self, **kwargs):
        """safepy/safe.py:661-713.  Average-linkage clustering of the top attributes on the distance
        between their binarised enrichment profiles (default: Jaccard, computed on the device in
        SciPy's condensed order; fcluster is SciPy's, as in the reference), then every node's domain
        sums, primary domain and primary NES.  While compute_pvalues' nes_binary and nes are still on
        the device (nobody has read them) both steps read them there -- distances of the boolean metrics
        and their average linkage in backend.Context.profile_linkage (Z equals SciPy's linkage bit for
        bit; distances SciPy would refuse, or more than Context.LINKAGE_MAX_POINTS top attributes, go
        through backend.Context.profile_distances and SciPy's linkage), then
        backend.Context.node_domains -- and they stay there; otherwise the host arrays and SciPy's
        linkage are used as before."""
        import pandas as pd
        from scipy.cluster.hierarchy import linkage, fcluster
        if 'attribute_distance_threshold' in kwargs:
            self.attribute_distance_threshold = kwargs['attribute_distance_threshold']
        self.validate_config()
        attrs = self.attributes
        top = attrs['top'].values.astype(bool)
        metric = self.attribute_distance_metric
        src_b = self.__dict__.get('_r_nes_binary')
        if isinstance(src_b, _DeviceResult) and isinstance(metric, str) and metric in METRIC_IDS and np.count_nonzero(top) >= 2:
            # the top columns are packed, compared and clustered in place on the device: nes_binary stays there and only Z comes back
            where = (src_b.buf.ptr, src_b.shape[0], src_b.shape[1], np.flatnonzero(top), metric)
            try:
                z, _ = self._ctx().profile_linkage(*where)
            except SafeHipError as err:
                if err.code not in (E_VALUE, E_UNSUPPORTED):
                    raise
                # distances SciPy refuses (it raises below, as before) or more profiles than the linkage kernel takes
                cond, _ = self._ctx().profile_distances(*where)
                z = linkage(cond, method='average')
        else:
            m = self.nes_binary[:, top].T
            if metric == 'jaccard' and m.shape[0] >= 2:
                z = linkage(be.jaccard_condensed(self._ctx(), m), method='average')
            else:
                z = linkage(m, method='average', metric=metric)
        max_d = np.max(z[:, 2] * self.attribute_distance_threshold)
        domains = fcluster(z, max_d, criterion='distance')
        attrs['domain'] = 0
        attrs.loc[attrs['top'], 'domain'] = domains

        # a node belongs to the domain holding most of the attributes it is enriched for (safe.py:693-698)
        dom = attrs['domain'].values
        ids = np.unique(dom)
        src_b, src_nes = self.__dict__.get('_r_nes_binary'), self.__dict__.get('_r_nes')   # (read again: the slice above may have downloaded)
        if (isinstance(src_b, _DeviceResult) and isinstance(src_nes, _DeviceResult) and tuple(src_b.shape) == tuple(src_nes.shape)
                and len(ids) <= be.Context.NODE_DOMAINS_MAX):
            # sums, primary domain and primary NES in one pass over the two resident matrices (safe_node_domains)
            sums, primary, primary_nes, _ = self._ctx().node_domains(src_b.buf.ptr, src_nes.buf.ptr, src_b.shape[0], src_b.shape[1],
                                                                     dom, ids)
            node2domain = pd.DataFrame(sums, columns=pd.Index(ids, name='domain'))
            primary = primary.astype(ids.dtype)
            node2domain['primary_domain'] = primary
            if np.any(~np.isin(primary, ids)):
                raise KeyError(0)                                 # as below
        else:
            onehot = (dom[:, None] == ids[None, :]).astype(np.float64)
            sums = self.nes_binary @ onehot
            node2domain = pd.DataFrame(sums, columns=pd.Index(ids, name='domain'))
            real = ids >= 1
            t = sums[:, real]
            t_max = t.max(axis=1)
            primary = ids[real][np.argmax(t, axis=1)]                # first maximum, like DataFrame.idxmax
            primary = np.where(t_max == 0, 0, primary)
            node2domain['primary_domain'] = primary
            # the highest NES among the attributes of the primary domain (safe.py:703-705); NaNs are skipped.  Only the
            # (node, primary domain) pairs are evaluated: a domain's columns for the nodes that have it as primary domain
            # (all columns of every domain for every node -- domain 0 holds most of the matrix -- took 0.23 s at 3971 x 4373)
            if np.any(~np.isin(primary, ids)):
                raise KeyError(0)                                     # the reference's o.loc[row, 0] with no attribute outside the domains
            primary_nes = np.full(primary.shape[0], np.nan)
            with np.errstate(invalid='ignore'):
                for d in ids:
                    rows = np.nonzero(primary == d)[0]
                    if rows.size == 0:
                        continue
                    block = self.nes[np.ix_(rows, np.nonzero(dom == d)[0])]
                    nan = np.isnan(block)
                    primary_nes[rows] = np.where(nan.all(axis=1), np.nan, np.where(nan, -np.inf, block).max(axis=1))
        node2domain['primary_nes'] = primary_nes
        self.node2domain = node2domain
        if self.verbose:
            per_domain = attrs.loc[attrs['domain'] > 0].groupby('domain')['id'].count()
            logging.info('Number of domains: %d (containing %d-%d attributes)'
                         % (len(np.unique(domains)), per_domain.min(), per_domain.max()))

    def trim_domains(self, **kwargs):
        """safepy/safe.py:715-745: a domain that is the primary domain of fewer than
        attribute_enrichment_min_size nodes is dissolved into domain 0; the survivors are renumbered
        0..D in ascending order and labelled with the five most frequent words of their attribute names
        (chop_and_filter, safe_io.py:735-745).  Sets self.domains."""
        import pandas as pd
        attrs, n2d = self.attributes, self.node2domain
        min_nodes = self.attribute_enrichment_min_size
        # how many nodes chose each domain id (ids are 0..D before trimming, safe.py:718-720)
        n_ids = attrs['domain'].nunique()
        votes = np.bincount(n2d['primary_domain'].to_numpy(dtype=np.int64), minlength=n_ids)[:n_ids]
        small = np.flatnonzero(votes < min_nodes)
        attrs.loc[attrs['domain'].isin(small), 'domain'] = 0
        n2d.loc[n2d['primary_domain'].isin(small), ['primary_domain', 'primary_nes']] = 0
        # dense renumbering of what is left (safe.py:729-734; the per-domain columns of node2domain keep their names there too)
        kept = np.sort(attrs['domain'].unique())
        stray = np.setdiff1d(n2d['primary_domain'].to_numpy(), kept)
        if stray.size:                                            # the reference's renumbering dictionary has no such key
            raise KeyError(int(stray[0]))
        attrs['domain'] = np.searchsorted(kept, attrs['domain'].to_numpy())
        n2d['primary_domain'] = np.searchsorted(kept, n2d['primary_domain'].to_numpy())
        labels = attrs.groupby('domain')['name'].apply(_domain_label)
        self.domains = pd.DataFrame({'id': np.arange(len(kept)), 'label': labels})
        if self.verbose:
            logging.info('Removed %d domains because they were the top choice for less than %d neighborhoods.'
                         % (len(small), min_nodes))

    # ------------------------------------------------------------------ sparse results ----
    PAIR_VALUES = ('nes', 'pvalues_pos', 'pvalues_neg', 'ns', 'nes_binary')

    def enriched_pairs(self, values='nes', format='csr', threshold=None, side='both'):
        """The enriched (node, attribute) pairs as a scipy.sparse array of shape [N, M] (no counterpart in the reference,
        whose users run np.nonzero(nes_binary) and nes[rows, cols] on the dense matrices; the comparison is that of
        safepy/safe.py:470).

        Selection.  threshold=None: the cells where nes_binary > 0.  threshold=t (a float >= 0, or inf): the cells of nes
        with |nes| > t (side='both'), nes > t ('positive') or nes < -t ('negative').  The comparison is strict; NaN is never
        selected, -0.0 is not selected at t = 0, +-inf are.

        values names the result matrix whose cells become `data` ('nes', 'pvalues_pos', 'pvalues_neg', 'ns', 'nes_binary'),
        copied bit for bit, as float64.  values=None gives the pattern alone: data is int8 ones.  The stored entries are
        exactly the selected cells: a selected cell whose value is 0 is still stored, as an explicit zero (so `.nnz` counts
        the selection; `.eliminate_zeros()` would drop such cells).

        format: 'csr' (csr_array), 'csc' (csc_array) or 'coo' (coo_array, row-major order).  Indices are sorted inside every
        row / column and int32.

        While every matrix the call needs -- nes_binary or nes for the selection, and the values matrix -- is still on the
        device (nobody has read it), the pairs are compacted there (backend.Context.enriched_pairs) and only they cross the
        link; the matrices stay on the device.  Otherwise the host arrays are indexed with NumPy."""
        import scipy.sparse as sp
        if values is not None and values not in self.PAIR_VALUES:
            raise ValueError('enriched_pairs: values=%r is not None or one of %s' % (values, ', '.join(self.PAIR_VALUES)))
        if format not in ('csr', 'csc', 'coo'):
            raise ValueError("enriched_pairs: format=%r is not 'csr', 'csc' or 'coo'" % (format,))
        if side not in ('both', 'positive', 'negative'):
            raise ValueError("enriched_pairs: side=%r is not 'both', 'positive' or 'negative'" % (side,))
        if threshold is None:
            selector, mode, t = 'nes_binary', be.Pairs.MODES['positive_nonzero'], 0.0
        else:
            t = float(threshold)
            if not t >= 0.0:
                raise ValueError('enriched_pairs: threshold=%r is not a number >= 0' % (threshold,))
            selector, mode = 'nes', be.Pairs.MODES[side]
        needed = [selector] + ([values] if values is not None and values != selector else [])
        slots = [self.__dict__.get('_r_' + name) for name in needed]
        for name, slot in zip(needed, slots):
            if slot is None:
                raise ValueError('enriched_pairs: %s is not set (run compute_pvalues first; the hypergeometric test leaves '
                                 'ns and pvalues_neg unset)' % name)
        shape = tuple(int(d) for d in slots[0].shape)
        if len(shape) != 2 or any(tuple(s.shape) != shape for s in slots):
            raise ValueError('enriched_pairs: %s do not share one [N, M] shape' % ' and '.join(needed))

        axis = 1 if format == 'csc' else 0
        if all(isinstance(s, _DeviceResult) for s in slots):
            sel_ptr = slots[0].buf.ptr
            val_ptr = None if values is None else slots[-1].buf.ptr
            indptr, indices, data, _ = self._ctx().enriched_pairs(sel_ptr, val_ptr, shape[0], shape[1], mode, t, axis)
        else:
            sel = np.asarray(getattr(self, selector))
            with np.errstate(invalid='ignore'):
                mask = (sel > 0, np.abs(sel) > t, sel > t, sel < -t)[mode]
            major, minor = np.nonzero(mask.T if axis else mask)
            indptr = np.zeros(shape[1 if axis else 0] + 1, dtype=np.int32)
            np.cumsum(np.bincount(major, minlength=indptr.shape[0] - 1), out=indptr[1:])
            indices = minor.astype(np.int32)
            data = None
            if values is not None:
                rows, cols = (minor, major) if axis else (major, minor)
                data = np.ascontiguousarray(np.asarray(getattr(self, values), dtype=np.float64)[rows, cols])
        if data is None:
            data = np.ones(indices.shape[0], dtype=np.int8)
        if format == 'coo':
            row = np.repeat(np.arange(shape[0], dtype=np.int32), np.diff(indptr))
            out = sp.coo_array((data, (row, indices)), shape=shape)
            out.has_canonical_format = True                        # row-major, no duplicates: by construction
            return out
        return (sp.csc_array if axis else sp.csr_array)((data, indices, indptr), shape=shape)

    def enriched_table(self, values='nes', threshold=None, side='both'):
        """enriched_pairs as a long pandas.DataFrame, one row per pair in row-major order: 'node' (row index), 'key' and
        'label' (of self.nodes), 'attribute' (column index), 'name' (of self.attributes), a column named after `values`
        (none for values=None) and, when self.attributes has it, 'domain'.  Built on the host from the COO form."""
        pairs = self.enriched_pairs(values=values, format='coo', threshold=threshold, side=side)
        row, col = pairs.row, pairs.col
        nodes = self.nodes
        if nodes is not None and 'key' in nodes and 'label' in nodes and len(nodes) == pairs.shape[0]:
            keys, labels = nodes['key'].to_numpy(), nodes['label'].to_numpy()
        elif self.graph is not None:
            _, keys, labels = self._graph_keys_labels()
            keys, labels = np.asarray(keys, dtype=object), np.asarray(labels, dtype=object)
        else:
            raise ValueError('enriched_table: neither self.nodes nor self.graph names the %d nodes' % pairs.shape[0])
        attrs = self.attributes
        if attrs is None or 'name' not in attrs or len(attrs) != pairs.shape[1]:
            raise ValueError('enriched_table: self.attributes does not name the %d attributes' % pairs.shape[1])
        table = {'node': row, 'key': keys[row], 'label': labels[row], 'attribute': col, 'name': attrs['name'].to_numpy()[col]}
        if values is not None:
            table[values] = pairs.data
        if 'domain' in attrs:
            table['domain'] = attrs['domain'].to_numpy()[col]
        return pd.DataFrame(table)

    # ------------------------------------------------------------------ plots ----
    def _columns(self, name, cols):
        """{column: [N] f64} of the result matrix `name` ('nes' / 'nes_binary') for the column indices cols: gathered on the
        device (backend.Context.gather_columns) while the matrix is still there, so a plot never downloads it whole;
        sliced from the host array otherwise."""
        cols = list(dict.fromkeys(int(c) for c in cols))
        src = self.__dict__.get('_r_' + name)
        if isinstance(src, _DeviceResult):
            n, m = src.shape
            got, _ = self._ctx().gather_columns(src.buf.ptr, cols, n, m)
        else:
            if src is None:
                raise ValueError('%s is not set: run compute_pvalues first' % name)
            got = np.asarray(src)[:, cols]
        return {c: got[:, i] for i, c in enumerate(cols)}

    def plot_network(self, foreground_color='#ffffff', background_color='#000000', labels=[], node_size=10, alpha=0.2,
                     **kwargs_mark_nodes):
        """safepy/safe.py:747-784: the network (safe_io.plot_network) and, when `labels` are given, those nodes marked
        (safe_io.mark_nodes with kwargs_mark_nodes, which must name `kind` as in the reference).  Returns the axes."""
        from . import safe_io
        ax = safe_io.plot_network(self.graph, background_color=background_color, node_size=node_size, alpha=alpha)
        if len(labels) > 0:
            xy, found = safe_io.get_node_coordinates(graph=self.graph, labels=labels)
            ax = safe_io.mark_nodes(x=xy[:, 0], y=xy[:, 1], labels=found, ax=ax, foreground_color=foreground_color,
                                    background_color=background_color, **kwargs_mark_nodes)
        return ax

    def _domain_colors(self):
        """(sorted domain ids of the attributes, their colours): safe_colormaps.get_colors('hsv', D) -- NumPy's global
        stream -- stored in self.domains['rgba'] (safe.py:804-810, 869-875)."""
        from .safe_colormaps import get_colors
        domains = np.sort(self.attributes['domain'].unique())
        domain2rgb = get_colors('hsv', len(domains))
        self.domains['rgba'] = domain2rgb.tolist()
        return domains, domain2rgb

    @staticmethod
    def _figure(num_plots, background_color):
        """The reference's grid of 10 x 10 panels, two per row, sharing both axes: (figure, flat array of axes)."""
        import matplotlib.pyplot as plt
        nrows = int(np.ceil(num_plots / 2))
        ncols = np.min([num_plots, 2])
        fig, axes = plt.subplots(nrows=nrows, ncols=ncols, figsize=(10 * ncols, 10 * nrows), sharex=True, sharey=True,
                                 facecolor=background_color)
        return fig, (axes.ravel() if isinstance(axes, np.ndarray) else np.array([axes]))

    def plot_composite_network_contours(self, save_fig=None, clabels=False, background_color='#000000'):
        """safepy/safe.py:786-849: the network, and beside it one contour per domain at density 1e-6 of SciPy's
        gaussian_kde of the domain's nodes on a 100 x 100 grid over their extent.  The node set of domain number k
        (k = 0 .. len(self.domains) - 1, domain 0 included) is the nodes with node2domain column k > 0.  Sets
        self.domains['rgba'].

        The kernel density estimates are SciPy's own objects (bandwidth, covariance factor, weights and errors, e.g.
        LinAlgError for a domain of collinear nodes); their evaluation on the grids -- O(members x 10^4) exponentials per
        domain -- runs on the device for every domain in one launch (backend.Context.kde_grid, plot.hip's k_kde_grid).

        Deliberate difference: the reference draws each contour with ax[1].contour where ax is one Axes, which raises
        TypeError after the first domain's estimate; here the contours are drawn on the second panel (axes[1]), which is
        what that code means."""
        import math
        import matplotlib.pyplot as plt
        from scipy.linalg import solve_triangular
        from scipy.stats import gaussian_kde
        from . import safe_io
        self._domain_colors()
        node_xy = safe_io.get_node_coordinates(self.graph)
        fig, axes = self._figure(2, background_color)
        ax = safe_io.plot_network(self.graph, ax=axes[0], background_color=background_color)

        labels = self.domains['label'].values
        grids, pts, weights, norms, offsets = [], [], [], [], [0]
        for n_domain in range(len(labels)):
            members = self.node2domain.loc[self.node2domain.loc[:, n_domain] > 0].index.values
            pos3 = node_xy[members, :]
            kernel = gaussian_kde(pos3.T)
            X, Y = np.mgrid[np.min(pos3[:, 0]):np.max(pos3[:, 0]):100j, np.min(pos3[:, 1]):np.max(pos3[:, 1]):100j]
            positions = np.vstack([X.ravel(), Y.ravel()])
            # what gaussian_kernel_estimate does before its loop: whitened points and grid, the normalisation
            cho = kernel.cho_cov
            pts.append(solve_triangular(cho, kernel.dataset, lower=True).T)
            grids.append((X, Y, solve_triangular(cho, positions, lower=True).T))
            weights.append(kernel.weights)
            norms.append(math.pow(2 * math.pi, -kernel.d / 2.0) / cho[0, 0] / cho[1, 1])
            offsets.append(offsets[-1] + pos3.shape[0])
        if labels.shape[0]:
            z, _ = self._ctx().kde_grid(offsets, np.concatenate(pts), np.concatenate(weights), norms,
                                        np.stack([g[2] for g in grids]))
        for n_domain, domain in enumerate(labels):
            X, Y, _ = grids[n_domain]
            Z = z[n_domain].reshape(X.shape)
            C = axes[1].contour(X, Y, Z, [1e-6], colors=self.domains.loc[n_domain, 'rgba'], alpha=1)
            if clabels:
                C.levels = [n_domain + 1]
                plt.clabel(C, C.levels, inline=True, fmt='%d', fontsize=16)
                print('%d -- %s' % (n_domain + 1, domain))
        fig.set_facecolor(background_color)
        if save_fig:
            print('Output path: %s' % save_fig)
            plt.savefig(save_fig, facecolor=background_color)

    def plot_composite_network(self, show_each_domain=False, show_domain_ids=True, show_network_contour=True, save_fig=None,
                               labels=[], foreground_color='#ffffff', background_color='#000000'):
        """safepy/safe.py:851-1003: the network, and beside it every node coloured by the domains of the attributes it is
        enriched for (mean of the domain colours weighted by those counts, brightened, brightest on top); with
        show_each_domain one more panel per domain > 0 with the nodes it is the primary domain of.  Sets
        self.domains['rgba'].

        The per-node domain counts -- nes_binary [N, M] summed over each domain's columns, the reference's
        groupby(level='domain', axis=1).sum() -- are made on the device from the device-resident nes_binary, read in place
        (backend.Context.domain_counts, plot.hip's k_domain_counts; a host nes_binary is uploaded).  The NES frame the
        reference builds for a per-domain alpha it then discards is not built."""
        import matplotlib.pyplot as plt
        from . import safe_io
        if background_color == '#ffffff':
            foreground_color = '#000000'
        domains, domain2rgb = self._domain_colors()
        column_domain = np.searchsorted(domains, self.attributes['domain'].to_numpy())
        src = self.__dict__.get('_r_nes_binary')
        if isinstance(src, _DeviceResult):
            counts, _ = self._ctx().domain_counts(src.buf.ptr, column_domain, len(domains), *src.shape)
        else:
            if src is None:
                raise ValueError('nes_binary is not set: run compute_pvalues first')
            counts, _ = self._ctx().domain_counts(np.asarray(src, dtype=np.float64), column_domain, len(domains))
        total = np.reshape(counts.sum(axis=1), (-1, 1))
        with np.errstate(divide='ignore', invalid='ignore'):
            c = np.matmul(counts, domain2rgb) / total
        t = np.sum(c, axis=1)
        c[np.isnan(t) | np.isinf(t), :] = [0, 0, 0, 0]
        coeff_brightness = 0.1 / np.nanmean(np.ravel(c[:, :-1]))
        if coeff_brightness > 1:
            c = c * coeff_brightness
        c = np.clip(c, None, 1)
        ix = np.argsort(np.sum(c, axis=1))

        node_xy = safe_io.get_node_coordinates(self.graph)
        num_plots = 2 + (len(domains) - 1 if show_each_domain else 0)
        fig, axes = self._figure(num_plots, background_color)
        safe_io.plot_network(self.graph, ax=axes[0], background_color=background_color)

        def decorate(ax):
            if show_network_contour:
                safe_io.plot_network_contour(self.graph, ax, background_color=background_color)
            if len(labels) != 0:
                xy, found = safe_io.get_node_coordinates(graph=self.graph, labels=labels)
                safe_io.mark_nodes(x=xy[:, 0], y=xy[:, 1], kind=['label'], labels=found, ax=ax, foreground_color=foreground_color,
                                   background_color=background_color)

        axes[1].scatter(node_xy[ix, 0], node_xy[ix, 1], c=c[ix], s=60, edgecolor=None)
        axes[1].set_aspect('equal')
        axes[1].set_facecolor(background_color)
        decorate(axes[1])
        primary = self.node2domain['primary_domain']
        if show_domain_ids:
            for domain in domains[domains > 0]:
                idx = primary == domain
                axes[1].text(np.nanmean(node_xy[idx, 0]), np.nanmean(node_xy[idx, 1]), str(domain),
                             fontdict={'size': 16, 'color': foreground_color, 'weight': 'bold'})
        if show_each_domain:
            for domain in domains[domains > 0]:
                ax = axes[1 + domain]
                idx = primary == domain
                colour = np.repeat(np.reshape(domain2rgb[domain, :], (1, 4)), node_xy.shape[0], axis=0)
                ax.scatter(node_xy[idx, 0], node_xy[idx, 1], c=colour[idx], s=60, edgecolor=None)
                ax.set_aspect('equal')
                ax.set_facecolor(background_color)
                ax.set_title('Domain %d\n%s' % (domain, self.domains.loc[domain, 'label']), color=foreground_color)
                decorate(ax)
        fig.set_facecolor(background_color)
        if save_fig:
            logging.info('Output path: %s' % save_fig)
            plt.savefig(save_fig, facecolor=background_color)

    def plot_sample_attributes(self, attributes=1, top_attributes_only=False, show_network=True, show_network_contour=True,
                               show_costanzo2016=False, show_costanzo2016_colors=True, show_costanzo2016_clabels=False,
                               show_nes=True, show_raw_data=False, show_significant_nodes=False, show_colorbar=True,
                               colors=['82add6', 'facb66'], foreground_color='#ffffff', background_color='#000000',
                               labels: list = [], save_fig=None, **kwargs):
        """safepy/safe.py:1005-1265: one panel per attribute -- its NES on the network, optionally the raw values and the
        significant nodes -- after the network.  attributes: an int k draws k attribute ids with np.random.choice from
        NumPy's global stream (all of them when k is not smaller than their count); a name or a list of names selects by
        name.  kwargs vmin / vmax / midrange set the colour scale.  save_fig is relative to self.output_dir.

        The nes (and, with show_significant_nodes, nes_binary) columns of the chosen attributes are gathered on the device
        while compute_pvalues' results are still there (backend.Context.gather_columns): the matrices are not downloaded.
        show_costanzo2016=True needs the reference's safe-data repository and raises NotImplementedError."""
        import re
        import textwrap
        import matplotlib.pyplot as plt
        from matplotlib.colors import LinearSegmentedColormap
        from . import safe_io
        from .safe_colormaps import MidpointRangeNormalize
        if show_costanzo2016:
            raise NotImplementedError('show_costanzo2016 draws the Costanzo 2016 network annotations from the safe-data '
                                      'repository, which safepy_amd does not ship')
        if background_color == '#ffffff':
            foreground_color = '#000000'

        all_attributes = self.attributes.index.values
        if top_attributes_only:
            all_attributes = all_attributes[self.attributes['top']]
        if isinstance(attributes, int):
            if attributes < len(all_attributes):
                attributes = np.random.choice(all_attributes, attributes, replace=False)
            else:
                attributes = np.arange(len(all_attributes))
        elif isinstance(attributes, str):
            attributes = [list(self.attributes['name'].values).index(attributes)]
        elif isinstance(attributes, list):
            names = list(self.attributes['name'].values)
            attributes = [names.index(a) for a in attributes]

        node_xy = safe_io.get_node_coordinates(self.graph)
        nax = 1 if show_network else 0
        fig, axes = self._figure(len(attributes) + nax, background_color)
        if show_network:
            safe_io.plot_network(self.graph, ax=axes[0], background_color=background_color)

        nes = self._columns('nes', attributes) if len(attributes) else {}
        nes_binary = self._columns('nes_binary', attributes) if show_significant_nodes and len(attributes) else {}
        for idx_attribute, attribute in enumerate(attributes):
            ax = axes[idx_attribute + nax]
            score = nes[int(attribute)]
            if show_nes:
                vmin = kwargs['vmin'] if 'vmin' in kwargs else \
                    np.nanmin([np.log10(1 / self.num_permutations), np.nanmin(-np.abs(score))])
                vmax = kwargs['vmax'] if 'vmax' in kwargs else \
                    np.nanmax([-np.log10(1 / self.num_permutations), np.nanmax(np.abs(score))])
                midrange = kwargs['midrange'] if 'midrange' in kwargs else [np.log10(0.05), 0, -np.log10(0.05)]
                idx = np.argsort(np.abs(score))                   # the brightest points on top
                hexes = [re.sub(r'^#', '', h) for h in [colors[0]] + [background_color] * 3 + [colors[1]]]
                cmap = LinearSegmentedColormap.from_list('my_cmap', [tuple(int(h[i:i + 2], 16) / 255 for i in (0, 2, 4))
                                                                     for h in hexes])
                sc = ax.scatter(node_xy[idx, 0], node_xy[idx, 1], c=score[idx], s=60, cmap=cmap,
                                norm=MidpointRangeNormalize(midrange=midrange, vmin=vmin, vmax=vmax), edgecolors=None)
            if show_colorbar:
                self._colorbar(fig, ax, sc, vmin, vmax, midrange, foreground_color)
            if show_raw_data:
                self._raw_data(ax, node_xy, attribute, foreground_color, background_color)
            if show_significant_nodes:
                with np.errstate(divide='ignore', invalid='ignore'):
                    idx = np.abs(nes_binary[int(attribute)]) > 0
                safe_io.mark_nodes(node_xy[idx, 0], node_xy[idx, 1], kind=['mark'], ax=ax,
                                   legend_label=('p < %.2e' % self.enrichment_threshold), foreground_color=foreground_color,
                                   background_color=background_color, marker='+')
            if show_network_contour:
                safe_io.plot_network_contour(self.graph, ax, background_color=background_color)
            if len(labels) != 0:
                xy, found = safe_io.get_node_coordinates(graph=self.graph, labels=labels)
                ax = safe_io.mark_nodes(x=xy[:, 0], y=xy[:, 1], kind=['label'], labels=found, ax=ax,
                                        foreground_color=foreground_color, background_color=background_color)
            ax.set_aspect('equal')
            ax.set_facecolor(background_color)
            ax.grid(False)
            ax.margins(0.1, 0.1)
            if idx_attribute + nax == 0:
                ax.invert_yaxis()
            ax.set_title('\n'.join(textwrap.wrap(self.attributes.loc[attribute, 'name'], width=30)), color=foreground_color)
            ax.set_frame_on(False)
        fig.set_facecolor(background_color)
        if save_fig:
            path = save_fig if os.path.isabs(save_fig) else os.path.join(self.output_dir, save_fig)
            logging.info('Output path: %s' % path)
            plt.savefig(path, facecolor=background_color)

    @staticmethod
    def _colorbar(fig, ax, sc, vmin, vmax, midrange, foreground_color):
        """The horizontal NES colour bar along the bottom of a panel (safe.py:1100-1136)."""
        import matplotlib.pyplot as plt
        box = ax.get_position()
        w = box.width * 0.75
        cax = fig.add_axes([box.x0 + (box.width - w) / 2, box.y0, w, box.height * 0.05])
        cb = plt.colorbar(sc, cax=cax, orientation='horizontal', ticks=[vmin, midrange[0], midrange[1], midrange[2], vmax],
                          drawedges=False)
        cb.set_label('Neighborhood enrichment p-value', color=foreground_color)
        cax.xaxis.set_tick_params(color=foreground_color)
        cb.outline.set_edgecolor(foreground_color)
        cb.outline.set_linewidth(1)
        plt.setp(plt.getp(cb.ax.axes, 'xticklabels'), color=foreground_color)
        cb.ax.set_xticklabels([r'$10^{%d}$' % vmin, r'$10^{%d}$' % midrange[0], r'$1$', r'$10^{%d}$' % -midrange[2],
                               r'$10^{-%d}$' % vmax])
        cax.text(cax.get_xlim()[0], 1, 'Lower than random', verticalalignment='bottom', fontdict={'color': foreground_color})
        cax.text(cax.get_xlim()[1], 1, 'Higher than random', verticalalignment='bottom', horizontalalignment='right',
                 fontdict={'color': foreground_color})

    def _raw_data(self, ax, node_xy, attribute, foreground_color, background_color):
        """The attribute's own values as dots, sized by magnitude, green above 0, red below (safe.py:1138-1172)."""
        import matplotlib.pyplot as plt
        from .safe_io import _legend
        with np.errstate(divide='ignore', invalid='ignore'):
            s_zero, s_min, s_max = 5, 5, 55
            if be._is_sparse(self.node2attribute):                            # one column of a sparse matrix, never the whole of it
                a = self.node2attribute if self.node2attribute.format in ('csc', 'csr', 'lil', 'dok') else self.node2attribute.tocsc()
                values = np.asarray(a[:, [int(attribute)]].toarray()).reshape(-1).astype(np.float64)
                mis = self._missing_rows_for(self.node2attribute)
                if mis is not None:
                    values[mis != 0] = np.nan
            else:
                values = self.node2attribute[:, attribute]
            mag = np.abs(values)
            if set(np.unique(mag[~np.isnan(mag)])).issubset([0, 1]):          # binary attribute
                s = np.zeros(len(mag))
                s[mag > 0] = s_max
                n_min, n_max = 0, 1
            else:                                                             # quantitative: 5th-95th percentile to sizes
                n_min, n_max = np.nanpercentile(np.unique(mag), [5, 95])
                a = (s_max - s_min) / (n_max - n_min)
                s = a * mag + (s_min - a * n_min)
                s[s < s_min] = s_min
                s[s > s_max] = s_max
            neg_color, pos_color, zero_color = '#ff1d23', '#00ff44', foreground_color
            idx = values < 0
            ax.scatter(node_xy[idx, 0], node_xy[idx, 1], s=s[idx], c=neg_color, marker='.')
            idx = values > 0
            ax.scatter(node_xy[idx, 0], node_xy[idx, 1], s=s[idx], c=pos_color, marker='.')
            idx = values == 0
            ax.scatter(node_xy[idx, 0], node_xy[idx, 1], s=s_zero, c=zero_color, marker='.')
            handles = [plt.scatter([], [], s=size, c=col, edgecolors='none')
                       for size, col in ((s_max, pos_color), (s_min, pos_color), (s_zero, zero_color), (s_min, neg_color),
                                         (s_max, neg_color))]
            texts = ['{0:.2f}'.format(v) for v in [n_max, n_min, 0, -n_min, -n_max]]
            _legend(ax, handles, texts, 'Raw data', foreground_color, background_color)

    # ------------------------------------------------------------------ outputs ----
    def _graph_keys_labels(self):
        """(ids, keys, labels) of the graph's nodes, as print_output_files reads them (safe.py:1286-1291)."""
        if isinstance(self.graph, LayoutGraph):
            return list(range(self.graph.number_of_nodes())), list(self.graph.keys), list(self.graph.labels)
        import networkx as nx
        t = nx.get_node_attributes(self.graph, 'key')
        return list(t.keys()), list(t.values()), list(nx.get_node_attributes(self.graph, 'label').values())

    def print_output_files(self, **kwargs):
        """safepy/safe.py:1267-1306: domain_properties_annotation.txt (when domains are defined: their row 0 is dropped in
        place first), attribute_properties_annotation.txt and node_properties_annotation.txt in self.output_dir (kwarg
        `output_dir` sets it), then self.nodes = the node table.  Without domains the node table is [N, M] NES values: its
        text is made on the device (backend.Context.format_tsv) from the device-resident nes when compute_pvalues left it
        there -- read in place, not downloaded first -- and written in chunks of at most `budget_bytes` (additive kwarg);
        the header, the index / key / label fields and the small tables are pandas', as in the reference.  Byte-identical
        to the reference's files."""
        if 'output_dir' in kwargs:
            self.output_dir = kwargs['output_dir']

        path_domains = os.path.join(self.output_dir, 'domain_properties_annotation.txt')
        if self.domains is not None:
            self.domains.drop(labels=[0], axis=0, inplace=True, errors='ignore')
            self.domains.to_csv(path_domains, sep='\t')
            logging.info(path_domains)

        path_attributes = os.path.join(self.output_dir, 'attribute_properties_annotation.txt')
        self.attributes.to_csv(path_attributes, sep='\t')
        logging.info(path_attributes)

        path_nodes = os.path.join(self.output_dir, 'node_properties_annotation.txt')
        ids, keys, labels = self._graph_keys_labels()
        if self.node2domain is not None:
            domains = self.node2domain['primary_domain'].values
            ness = self.node2domain['primary_nes'].values
            num_domains = self.node2domain[self.domains['id']].sum(axis=1).values
            self.nodes = pd.DataFrame(data={'id': ids, 'key': keys, 'label': labels, 'domain': domains,
                                            'nes': ness, 'num_domains': num_domains})
            self.nodes.to_csv(path_nodes, sep='\t')
        else:
            self._write_nes_table(path_nodes, keys, labels, kwargs.get('budget_bytes'))
            self.nodes = pd.DataFrame(self.nes)
            self.nodes.columns = self.attributes['name']
            self.nodes.insert(loc=0, column='key', value=keys)
            self.nodes.insert(loc=1, column='label', value=labels)
        logging.info(path_nodes)

    def _write_nes_table(self, path, keys, labels, budget_bytes=None):
        """node_properties_annotation.txt without domains: pandas' to_csv(sep='\t') of DataFrame(nes) with the attribute
        names as columns and 'key' / 'label' inserted in front (safe.py:1297-1306).  pandas writes the header line and each
        row's index / key / label fields (quoted where QUOTE_MINIMAL asks); the device writes the values."""
        src = self.__dict__.get('_r_nes')
        if isinstance(src, _DeviceResult):
            n, m = src.shape
            host = None
        else:
            if src is None:
                raise ValueError('print_output_files needs nes: run compute_pvalues first')
            host = np.asarray(src)
            if host.ndim != 2 or host.dtype != np.float64:
                raise TypeError('nes must be a float64 [N, M] array (got %s %s)' % (host.dtype, host.shape))
            n, m = host.shape
        # the header from an empty frame built like the reference's (its column checks raise as the reference's do)
        head = pd.DataFrame(np.empty((0, m)))
        head.columns = self.attributes['name']
        if len(keys) != n or len(labels) != n:
            raise ValueError('Length of values (%d) does not match length of index (%d)'
                             % (len(keys) if len(keys) != n else len(labels), n))
        head.insert(loc=0, column='key', value=[])
        head.insert(loc=1, column='label', value=[])
        header = head.to_csv(sep='\t').encode('utf-8')
        prefixes, offsets = _row_prefixes(keys, labels, n)

        ctx = self._ctx()
        tmp = None
        try:
            if host is not None:
                tmp = ctx.alloc_f64(n, m)
                tmp.upload(host)
                ptr = tmp.ptr
            else:
                ptr = src.buf.ptr
            with open(path, 'wb') as f:
                f.write(header)
                f.flush()
                self.output_timing = ctx.format_tsv(ptr, n, m, prefixes, offsets, f.fileno(), budget_bytes=budget_bytes)
        finally:
            if tmp is not None:
                tmp.free()


_ROW_END = '\t\x01\n'      # a sentinel field no key or label text is expected to hold


def _row_prefixes(keys, labels, n):
    """(utf-8 bytes, int64 offsets [n + 1]) of each row's index, key and label fields exactly as pandas writes them in
    to_csv(sep='\t') of the node table: pandas writes them (one call, a sentinel column marks the row ends); rows whose
    fields hold the sentinel are written one at a time."""
    frame = pd.DataFrame({'key': keys, 'label': labels, 'end': '\x01'})
    text = frame.to_csv(sep='\t', header=False)
    rows = text.split(_ROW_END)
    if len(rows) != n + 1 or rows[-1]:
        rows = [frame.iloc[i:i + 1].to_csv(sep='\t', header=False)[:-len(_ROW_END)] for i in range(n)] + ['']
    rows = [r.encode('utf-8') for r in rows[:n]]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return b''.join(rows), offsets


def _domain_label(names):
    """The five most frequent words of a domain's attribute names, most frequent first, ties in order
    of first appearance, without a few stop words (safe_io.py:735-745)."""
    import re
    from collections import Counter
    words = re.findall(r"[\w']+", names.str.cat(sep=' '))
    counts = Counter(words)
    ranked = sorted(counts, key=counts.get, reverse=True)
    skip = ('of', 'a', 'the', 'an', ',', 'via', 'to', 'into', 'from')
    return ', '.join([w for w in ranked if w not in skip][:5])
