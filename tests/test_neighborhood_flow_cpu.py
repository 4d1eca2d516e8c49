"""The device work behind define_neighborhoods, compute_node_distances and node_distance_percentile, pinned without a device:
safepy_amd.safe.be is replaced by a stand-in that records every backend call, and the ordered list of calls -- with their
radius / cutoff / keep_distances arguments and the handle each method was called on -- is compared with the sequence written
down here for every metric x radius type x weighting on a 5-node path graph.  Handles are named h1, h2, ... in the order they
are made.  A call that raises part-way must leave no handle open that it did not hand to the SAFE object."""
import types

import numpy as np
import pytest

import safepy_amd
from safepy_amd import safe as safe_mod

N = 5
XY = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.5]])
EXTENT = 4.0                                            # max x - min x
EU, EV = np.array([0, 1, 2, 3]), np.array([1, 2, 3, 4])
LENGTH, WEIGHT = np.array([1.0, 1.0, 1.0, 1.25]), np.array([2.0, 3.0, 4.0, 5.0])
RADII = np.array([1.0, 2.0, 3.0, 4.0, 5.0])             # what the stand-in's row selections return; median 3.0
N_PAIRS = N * (N - 1) // 2
INF = float('inf')

METRICS = ('euclidean', 'shortpath', 'shortpath_weighted_layout', 'diffusion')
NETWORK = METRICS[1:]
# radius type -> (neighborhood_radius, the scalar radius it resolves to on a layout metric)
KINDS = {'diameter': (0.25, 0.25 * EXTENT), 'absolute': (1.5, 1.5), 'percentile': (50, 4.5), 'nearest': (2, 3.0)}
RANKS = [4, 5]                                          # np.percentile(v, 50) of 10 values interpolates ranks 4 and 5: 4.5
WEIGHTINGS = ('none', 'gaussian')
BANDWIDTH = 0.5


class Boom(Exception):
    pass


class Recorder:
    def __init__(self, fail_at=None):
        self.calls, self.handles, self.fail_at, self.count = [], [], fail_at, 0

    def log(self, *entry):
        if entry[0].split('.')[-1] not in ('close', 'free'):      # releasing never fails
            self.count += 1
            if self.count == self.fail_at:
                raise Boom(entry[0])
        self.calls.append(entry)


def _radius_arg(r):
    return tuple(np.asarray(r, dtype=np.float64).tolist()) if np.ndim(r) else float(r)


def _weights_name(w):
    return 'length' if w is LENGTH else 'weight' if w is WEIGHT else repr(w)


def make_backend(rec):
    class Buffer:
        def __init__(self, name):
            self.name, self.ptr = name, name

        def upload(self, host):
            pass

        def download(self, shape):
            return np.zeros(shape)

        def free(self):
            rec.log('%s.free' % self.name)

    class Context:
        @classmethod
        def default(cls, device):
            return cls()

        def pair_distance_select(self, xy, ranks):
            assert xy is XY or np.array_equal(xy, XY, equal_nan=True)
            rec.log('ctx.pair_distance_select', list(ranks))
            return np.asarray(ranks, dtype=np.float64), N_PAIRS

        def row_distance_select(self, xy, k):
            rec.log('ctx.row_distance_select', k)
            return RADII.copy()

        def alloc(self, nbytes):
            rec.log('ctx.alloc', nbytes)
            return Buffer('xy_buf')

        def alloc_f64(self, *shape):
            rec.log('ctx.alloc_f64', shape)
            return Buffer('out_buf')

        def euclidean_dense(self, xy_ptr, n, nr, mask_ptr=None, dist_ptr=None):
            rec.log('ctx.euclidean_dense', xy_ptr, n, float(nr), mask_ptr, dist_ptr)

    class Neighborhoods:
        def __init__(self, ctx=None):
            self.ctx, self.n, self.handle, self.has_weights = ctx, N, True, False
            rec.handles.append(self)
            self.name = 'h%d' % len(rec.handles)

        @classmethod
        def euclidean(cls, ctx, xy, nr):
            rec.log('euclidean', float(nr))
            return cls(ctx)

        @classmethod
        def euclidean_rows(cls, ctx, xy, radii):
            rec.log('euclidean_rows', _radius_arg(radii))
            return cls(ctx)

        @classmethod
        def shortpath(cls, ctx, n, edge_u, edge_v, edge_w, cutoff, keep_distances=False):
            rec.log('shortpath', n, _weights_name(edge_w), float(cutoff), keep_distances)
            return cls(ctx)

        @classmethod
        def diffusion(cls, ctx, n, edge_u, edge_v, edge_w, restart, steps, cutoff, want_kernel=False):
            rec.log('diffusion', n, _weights_name(edge_w), restart, steps, float(cutoff))
            return cls(ctx)

        @classmethod
        def from_distances_rows(cls, src, radii, keep_distances=False):
            rec.log('from_distances_rows', src.name, _radius_arg(radii), keep_distances)
            return cls(src.ctx)

        def distance_select(self, ranks):
            rec.log('%s.distance_select' % self.name, list(ranks))
            return np.asarray(ranks, dtype=np.float64), N_PAIRS

        def row_distance_select(self, k):
            rec.log('%s.row_distance_select' % self.name, k)
            return RADII.copy()

        def set_layout(self, xy):
            rec.log('%s.set_layout' % self.name)

        def set_weights_from_xy(self, xy, kind, radii, bandwidth=0.5):
            rec.log('%s.set_weights_from_xy' % self.name, kind, _radius_arg(radii), bandwidth)
            self.has_weights = True

        def set_weights_from_distances(self, kind, radii, bandwidth=0.5):
            rec.log('%s.set_weights_from_distances' % self.name, kind, _radius_arg(radii), bandwidth)
            self.has_weights = True

        def distances(self):
            rec.log('%s.distances' % self.name)
            return np.zeros((N, N))

        def close(self):
            rec.log('%s.close' % self.name)
            self.handle = None

    return types.SimpleNamespace(Context=Context, Neighborhoods=Neighborhoods)


def make_safe(monkeypatch, metric, kind, weighting='none', xy=XY, fail_at=None):
    rec = Recorder(fail_at)
    monkeypatch.setattr(safe_mod, 'be', make_backend(rec))
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(xy, EU, EV, length=LENGTH, weight=WEIGHT)
    sf.node_distance_metric = metric
    sf.neighborhood_radius_type = kind
    sf.neighborhood_radius = KINDS[kind or 'diameter'][0]
    sf.neighborhood_weighting = weighting
    sf.neighborhood_weight_bandwidth = BANDWIDTH
    return sf, rec


# ---- the sequences, written down ----
def network_build(metric, cutoff):
    """the constructor call of a network metric's handle at a cutoff"""
    if metric == 'diffusion':
        return ('diffusion', N, 'weight', 0.5, 32, float(cutoff))
    return ('shortpath', N, 'length' if metric == 'shortpath_weighted_layout' else 'weight', float(cutoff), True)


def scalar_radius(metric, kind):
    """the scalar radius a radius type resolves to: 'shortpath' takes neighborhood_radius as its hop cutoff under 'diameter' too"""
    return KINDS[kind][0] if (metric == 'shortpath' and kind == 'diameter') else KINDS[kind][1]


def resolution(metric, kind):
    """(calls that resolve the radius of a type other than 'nearest', handles opened by them)"""
    if kind != 'percentile':
        return [], 0
    if metric == 'euclidean':
        return [('ctx.pair_distance_select', []), ('ctx.pair_distance_select', RANKS)], 0
    return [network_build(metric, INF), ('h1.distance_select', []), ('h1.distance_select', RANKS), ('h1.close',)], 1


def expected_define(metric, kind, weighting, finite=True):
    radii = tuple(RADII.tolist())
    if kind == 'nearest':
        if metric == 'euclidean':
            calls, final, r = [('ctx.row_distance_select', 2), ('euclidean_rows', radii)], 'h1', radii
        else:
            calls = [network_build(metric, INF), ('h1.row_distance_select', 2), ('from_distances_rows', 'h1', radii, True),
                     ('h1.close',)]
            final, r = 'h2', radii
    else:
        calls, opened = resolution(metric, kind)
        r = scalar_radius(metric, kind)
        calls.append(('euclidean', r) if metric == 'euclidean' else network_build(metric, r))
        final = 'h%d' % (opened + 1)
    if metric != 'euclidean' and (metric != 'diffusion' or finite):
        calls.append(('%s.set_layout' % final,))
    if weighting != 'none':
        how = 'set_weights_from_xy' if metric == 'euclidean' else 'set_weights_from_distances'
        calls.append(('%s.%s' % (final, how), weighting, r, BANDWIDTH))
    return calls, final


def expected_distances(metric, kind):
    radii = tuple(RADII.tolist())
    if metric != 'euclidean' and kind == 'nearest':
        return [network_build(metric, INF), ('h1.row_distance_select', 2), ('from_distances_rows', 'h1', radii, True), ('h1.close',),
                ('h2.distances',), ('h2.close',)]
    if kind == 'nearest':
        calls, opened = [('ctx.row_distance_select', 2)], 0
    else:
        calls, opened = resolution(metric, kind)
    r = scalar_radius(metric, kind)
    if metric == 'euclidean':
        return calls + [('ctx.alloc', XY.nbytes), ('ctx.alloc_f64', (N, N)), ('ctx.euclidean_dense', 'xy_buf', N, r, None, 'out_buf'),
                        ('xy_buf.free',), ('out_buf.free',)]
    h = 'h%d' % (opened + 1)
    return calls + [network_build(metric, r), ('%s.distances' % h,), ('%s.close' % h,)]


CASES = [(m, k) for m in METRICS for k in KINDS if not (m == 'diffusion' and k == 'diameter')]


@pytest.mark.parametrize('weighting', WEIGHTINGS)
@pytest.mark.parametrize('metric,kind', CASES)
def test_define_neighborhoods_calls(monkeypatch, metric, kind, weighting):
    sf, rec = make_safe(monkeypatch, metric, kind, weighting)
    sf.define_neighborhoods()
    calls, final = expected_define(metric, kind, weighting)
    assert rec.calls == calls
    assert sf._nbr.name == final and sf._nbr.handle
    assert [h.name for h in rec.handles if h.handle] == [final]
    assert sf.neighborhood_radius_resolved == scalar_radius(metric, kind)
    if kind == 'nearest':
        assert np.array_equal(sf.neighborhood_radii, RADII)
    else:
        assert sf.neighborhood_radii is None
    if metric == 'euclidean':
        assert sf._node_distances is None
    else:
        assert sf._node_distances[0] == 'device-shortpath' and sf._node_distances[1] is sf._nbr


@pytest.mark.parametrize('metric', METRICS[:3])
def test_radius_type_none_is_diameter(monkeypatch, metric):
    sf, rec = make_safe(monkeypatch, metric, None)
    sf.define_neighborhoods()
    assert rec.calls == expected_define(metric, 'diameter', 'none')[0]


@pytest.mark.parametrize('metric', NETWORK)
def test_layout_hint_without_finite_coordinates(monkeypatch, metric):
    """'diffusion' needs no layout: it takes the hint only when every coordinate is finite; the shortest-path metrics always do"""
    xy = XY.copy()
    xy[2, 1] = np.nan
    sf, rec = make_safe(monkeypatch, metric, 'absolute', xy=xy)
    sf.define_neighborhoods()
    assert rec.calls == expected_define(metric, 'absolute', 'none', finite=False)[0]


@pytest.mark.parametrize('kind', (None, 'diameter'))
def test_diffusion_diameter_is_refused_before_any_call(monkeypatch, kind):
    for method in ('define_neighborhoods', 'compute_node_distances'):
        sf, rec = make_safe(monkeypatch, 'diffusion', kind)
        with pytest.raises(ValueError):
            getattr(sf, method)()
        assert rec.calls == [] and rec.handles == []


@pytest.mark.parametrize('metric,kind', CASES)
def test_compute_node_distances_calls(monkeypatch, metric, kind):
    sf, rec = make_safe(monkeypatch, metric, kind)
    sf.compute_node_distances()
    assert rec.calls == expected_distances(metric, kind)
    assert [h.name for h in rec.handles if h.handle] == []
    assert sf._nbr is None
    if metric == 'euclidean':
        assert sf._node_distances.shape == (N, N)
    else:
        assert sf._node_distances[0] == 'dense-shortpath' and sf._node_distances[1].shape == (N, N)


@pytest.mark.parametrize('metric', METRICS)
def test_node_distance_percentile_calls(monkeypatch, metric):
    sf, rec = make_safe(monkeypatch, metric, 'absolute')
    assert sf.node_distance_percentile(50) == 4.5
    assert rec.calls == resolution(metric, 'percentile')[0]
    assert [h.name for h in rec.handles if h.handle] == []
    assert sf._nbr is None and sf._node_distances is None


@pytest.mark.parametrize('weighting', WEIGHTINGS)
@pytest.mark.parametrize('metric,kind', CASES)
def test_define_neighborhoods_raising_part_way_leaves_no_handle_open(monkeypatch, metric, kind, weighting):
    total = len([c for c in expected_define(metric, kind, weighting)[0] if not c[0].endswith('.close')])
    for fail_at in range(1, total + 1):
        sf, rec = make_safe(monkeypatch, metric, kind, weighting, fail_at=fail_at)
        with pytest.raises(Boom):
            sf.define_neighborhoods()
        assert [h for h in rec.handles if h.handle and h is not sf._nbr] == [], fail_at


@pytest.mark.parametrize('method', ('compute_node_distances', 'node_distance_percentile'))
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('kind', ('percentile', 'nearest'))
def test_second_call_raising_leaves_no_handle_open(monkeypatch, metric, kind, method):
    sf, rec = make_safe(monkeypatch, metric, kind, fail_at=2)
    with pytest.raises(Boom):
        sf.node_distance_percentile(50) if method == 'node_distance_percentile' else sf.compute_node_distances()
    assert len(rec.calls) >= 1
    assert [h for h in rec.handles if h.handle] == []
