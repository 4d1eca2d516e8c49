"""neighborhood_radius_type 'absolute' and 'percentile' on the device: the exact selection kernels of nbr.hip against sorted
host arrays, and SAFE end to end against SciPy / networkx.  Every comparison is on bits.  Needs an MI355X.

Tile edges of the selection kernel from coordinates: 64 rows x 256 columns per tile, 64 lanes per wave; up to four prefixes
per sweep (so more than four ranks with different leading digits take several sweeps per pass)."""
import numpy as np
import pytest

import kk_ref
import radius_ref as rr

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1025, 2049)


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


def _check_xy(ctx, xy, seed=0):
    sv = rr.sorted_pdist(xy)
    n = xy.shape[0]
    assert ctx.pair_distance_select(xy, [])[1] == n * (n - 1) // 2 == sv.shape[0]
    ranks = rr.ranks_for(sv, every_below=65 * 64 // 2, extra=8, seed=seed)
    got, count = ctx.pair_distance_select(xy, ranks)
    assert count == sv.shape[0]
    bad = np.nonzero(rr.bits(got) != rr.bits(sv[ranks]))[0]
    assert bad.size == 0, (ranks[bad[:5]], got[bad[:5]], sv[ranks][bad[:5]])


# ------------------------------------------------------------------ 1. selection from coordinates ----

@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', rr.KINDS)
def test_select_from_coordinates_matches_sorted_pdist(ctx, kind, n):
    _check_xy(ctx, rr.xy_input(kind, n), seed=n)


def test_select_on_the_integer_lattice_every_tie_boundary(ctx):
    xy = rr.xy_input('lattice', 64)
    sv = rr.sorted_pdist(xy)
    assert np.unique(sv).size < 40                                      # 2016 distances, a few dozen values
    _check_xy(ctx, xy)                                                  # every rank (n <= 65)
    # and again as a few ranks per call: both sides of every boundary between distinct values
    ranks = rr.ranks_for(sv, every_below=0)
    got, _ = ctx.pair_distance_select(xy, ranks)
    assert np.array_equal(rr.bits(got), rr.bits(sv[ranks]))


def test_select_from_coordinates_refusals(amd, ctx):
    xy = rr.xy_input('uniform', 5)
    for bad in ([10], [-1], [0, 3, 10]):
        with pytest.raises(amd.SafeHipError) as err:
            ctx.pair_distance_select(xy, bad)
        assert err.value.code == -1                                     # SAFE_E_INVALID
    got, count = ctx.pair_distance_select(xy[:1], [])                   # one node: no pair, nothing to select
    assert count == 0 and got.shape == (0,)
    with pytest.raises(amd.SafeHipError):
        ctx.pair_distance_select(xy[:1], [0])
    with pytest.raises(amd.SafeHipError) as err:
        ctx.pair_distance_select(np.zeros((65537, 2)), [])
    assert err.value.code == -4                                         # SAFE_E_UNSUPPORTED
    xy[2, 1] = np.nan
    with pytest.raises(amd.SafeHipError) as err:
        ctx.pair_distance_select(xy, [0])
    assert err.value.code == -5                                         # SAFE_E_VALUE


# ------------------------------------------------------------------ 2. wide counters ----

def test_wide_counters_at_65536_nodes(ctx):
    """32 768 nodes at (0, 0) and 32 768 at (1, 0): 1 073 709 056 distances are 0.0 and 1 073 741 824 are 1.0 -- the counts
    are known without any host array of distances."""
    n = 65536
    xy = np.zeros((n, 2))
    xy[n // 2:, 0] = 1.0
    zeros = 2 * ((n // 2) * (n // 2 - 1) // 2)
    assert zeros == 1073709056
    ranks = [0, 1073709055, 1073709056, 2147450879]
    got, count = ctx.pair_distance_select(xy, ranks)
    assert count == 2147450880
    assert np.array_equal(rr.bits(got), rr.bits([0.0, 0.0, 1.0, 1.0]))


# ------------------------------------------------------------------ 3. selection from a handle ----

@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n', [2, 17, 91, 129, 257, 1025])
def test_select_from_a_handle_matches_its_own_distances(amd, ctx, n, weighted):
    eu, ev, ew = kk_ref.sparse_edges(n, seed=n, weighted=weighted)
    nbr = amd.Neighborhoods.shortpath(ctx, n, eu, ev, ew, np.inf, keep_distances=True)
    try:
        dmat = nbr.distances()
        assert np.isinf(dmat[n - 1, :n - 1]).all()                      # the part sparse_edges cuts off
        sv = rr.finite_upper(dmat)
        assert nbr.distance_select([])[1] == sv.shape[0]
        if sv.shape[0] == 0:
            with pytest.raises(amd.SafeHipError):
                nbr.distance_select([0])
            return
        ranks = rr.ranks_for(sv, every_below=17 * 16 // 2, extra=32, seed=n)
        got, count = nbr.distance_select(ranks)
        assert count == sv.shape[0]
        assert np.array_equal(rr.bits(got), rr.bits(sv[ranks]))
        with pytest.raises(amd.SafeHipError) as err:
            nbr.distance_select([count])
        assert err.value.code == -1
    finally:
        nbr.close()


def test_select_from_a_handle_refusals(amd, ctx):
    none = np.zeros(0, dtype=np.int32)
    nbr = amd.Neighborhoods.shortpath(ctx, 9, none, none, None, np.inf, keep_distances=True)     # edgeless: no finite pair
    try:
        got, count = nbr.distance_select([])
        assert count == 0 and got.shape == (0,)
        for rank in (0, 5, -1):
            with pytest.raises(amd.SafeHipError) as err:
                nbr.distance_select([rank])
            assert err.value.code == -1
    finally:
        nbr.close()
    eu, ev, _ = kk_ref.sparse_edges(17, seed=1)
    nbr = amd.Neighborhoods.shortpath(ctx, 17, eu, ev, None, np.inf, keep_distances=False)
    try:
        with pytest.raises(amd.SafeHipError) as err:
            nbr.distance_select([0])
        assert err.value.code == -1 and 'keep_distances' in str(err.value)
    finally:
        nbr.close()


# ------------------------------------------------------------------ 4. SAFE end to end ----

METRIC_WEIGHT = {'shortpath_weighted_layout': 'length', 'shortpath': 'weight'}
SETTINGS = [('absolute', 0.3), ('percentile', 0.5), ('percentile', 10), ('percentile', 50), ('percentile', 0),
            ('percentile', 100)]


@pytest.fixture(scope='module')
def world(amd):
    """The graph (with edge lengths), its coordinates, and the unbounded networkx matrices of both shortest-path metrics."""
    from safepy_amd import safe_io
    G, xy = rr.safe_graph()
    G = safe_io.calculate_edge_lengths(G, verbose=False)
    unbounded = {metric: rr.nx_all_pairs(G, weight) for metric, weight in METRIC_WEIGHT.items()}
    assert np.isinf(unbounded['shortpath'][0, G.number_of_nodes() - 1])               # one component is cut off
    return G, xy, unbounded


def _safe(amd, graph):
    sf = amd.SAFE(verbose=False)
    sf.graph = graph
    return sf


def _want_radius(world, metric, kind, value):
    from scipy.spatial.distance import pdist
    _, xy, unbounded = world
    if kind == 'absolute':
        return float(value)
    v = pdist(xy) if metric == 'euclidean' else rr.finite_upper(unbounded[metric])
    return float(np.percentile(v, value))


@pytest.mark.parametrize('kind,value', SETTINGS)
def test_safe_euclidean_radius_types(amd, world, kind, value):
    from scipy.spatial.distance import pdist, squareform
    G, xy, _ = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type=kind, neighborhood_radius=value)
    r = _want_radius(world, 'euclidean', kind, value)
    assert isinstance(sf.neighborhood_radius_resolved, float)
    assert rr.bits(sf.neighborhood_radius_resolved)[0] == rr.bits(r)[0]
    assert np.array_equal(sf.neighborhoods, (squareform(pdist(xy)) < r).astype(np.int64))


@pytest.mark.parametrize('kind,value', SETTINGS)
@pytest.mark.parametrize('metric', sorted(METRIC_WEIGHT))
def test_safe_shortpath_radius_types(amd, world, metric, kind, value):
    G, _, _ = world
    n = G.number_of_nodes()
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type=kind, neighborhood_radius=value)
    r = _want_radius(world, metric, kind, value)
    assert rr.bits(sf.neighborhood_radius_resolved)[0] == rr.bits(r)[0]
    want = rr.nx_all_pairs(G, METRIC_WEIGHT[metric], cutoff=r)
    assert np.array_equal(sf.neighborhoods, np.isfinite(want).astype(np.int64))
    assert np.array_equal(rr.bits(rr.dense_of(sf.node_distances, n)), rr.bits(want))
    # compute_node_distances resolves the radius the same way
    other = _safe(amd, G)
    other.compute_node_distances(node_distance_metric=metric, neighborhood_radius_type=kind, neighborhood_radius=value)
    assert rr.bits(other.neighborhood_radius_resolved)[0] == rr.bits(r)[0]
    assert np.array_equal(rr.bits(rr.dense_of(other.node_distances, n)), rr.bits(want))


@pytest.mark.parametrize('metric', ['euclidean'] + sorted(METRIC_WEIGHT))
def test_node_distance_percentile_is_read_only(amd, world, metric):
    G, _, _ = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius=0.15)
    before = sf.neighborhoods.copy()
    settings = (sf.node_distance_metric, sf.neighborhood_radius_type, sf.neighborhood_radius, sf.neighborhood_radius_resolved)
    got = sf.node_distance_percentile([1, 50])
    want = [_want_radius(world, metric, 'percentile', q) for q in (1, 50)]
    assert isinstance(got, np.ndarray) and np.array_equal(rr.bits(got), rr.bits(want))
    one = sf.node_distance_percentile(50)
    assert isinstance(one, float) and rr.bits(one)[0] == rr.bits(want[1])[0]
    assert np.array_equal(sf.neighborhoods, before)
    assert settings == (sf.node_distance_metric, sf.neighborhood_radius_type, sf.neighborhood_radius,
                        sf.neighborhood_radius_resolved)
    with pytest.raises(ValueError):
        sf.node_distance_percentile(101)


@pytest.mark.parametrize('metric', ['euclidean'] + sorted(METRIC_WEIGHT))
def test_diameter_and_none_are_the_call_without_the_setting(amd, world, metric):
    G, _, _ = world
    radius = 2 if metric == 'shortpath' else 0.15
    plain = _safe(amd, G)
    plain.define_neighborhoods(node_distance_metric=metric, neighborhood_radius=radius)
    for kind in ('diameter', None):
        sf = _safe(amd, G)
        sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type=kind, neighborhood_radius=radius)
        assert np.array_equal(sf.neighborhoods, plain.neighborhoods)
        if metric != 'euclidean':
            assert sf.node_distances == plain.node_distances
        assert sf.neighborhood_radius_resolved == plain.neighborhood_radius_resolved


def test_settings_errors_and_the_one_node_graph(amd, world):
    G, _, _ = world
    sf = _safe(amd, G)
    with pytest.raises(ValueError):
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='radius')
    assert sf.neighborhood_radius_type == 'diameter'
    with pytest.raises(ValueError):
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='percentile', neighborhood_radius=100.5)
    assert sf.neighborhood_radius_type == 'diameter' and sf.neighborhood_radius == 0.1
    for metric in ['euclidean'] + sorted(METRIC_WEIGHT):
        lone = _safe(amd, amd.LayoutGraph(np.array([[0.25, 0.5]])))
        with pytest.raises(ValueError):
            lone.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='percentile', neighborhood_radius=50)


def test_resolved_radius_is_logged_and_pickles(amd, world, caplog):
    import logging
    import pickle
    G, _, _ = world
    sf = amd.SAFE(verbose=True)
    sf.graph = G
    with caplog.at_level(logging.INFO):
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='percentile', neighborhood_radius=10)
    assert repr(sf.neighborhood_radius_resolved) in caplog.text and '10.00 x percentile' in caplog.text
    clone = pickle.loads(pickle.dumps(sf))
    assert clone.neighborhood_radius_resolved == sf.neighborhood_radius_resolved and clone.neighborhood_radius_type == 'percentile'


# ------------------------------------------------------------------ 5. busy caller stream ----

def test_selection_on_a_busy_caller_stream(amd, ctx):
    """Both selection calls after safe_ctx_set_stream on a caller's stream that still has work queued (a chain of matrix
    products, as tests/test_gpu_stream_order.py builds its delay): they are synchronous, so they must return the quiet answer."""
    import torch
    xy = rr.xy_input('uniform', 1025)
    sv = rr.sorted_pdist(xy)
    ranks = rr.ranks_for(sv, extra=8)
    eu, ev, ew = kk_ref.sparse_edges(257, seed=5, weighted=True)
    nbr = amd.Neighborhoods.shortpath(ctx, 257, eu, ev, ew, np.inf, keep_distances=True)
    sd = rr.finite_upper(nbr.distances())
    dranks = rr.ranks_for(sd, extra=8)
    s = torch.cuda.Stream()
    a = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device='cuda')
    c = torch.empty_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):                                          # one link of the chain, timed: the delay lasts 30 ms
        for _ in range(3):
            torch.mm(a, a, out=c)
        e0.record(s)
        for _ in range(4):
            torch.mm(a, a, out=c)
        e1.record(s)
    e1.synchronize()
    links = int(np.ceil(30.0 / max(e0.elapsed_time(e1) / 4.0, 0.02)))
    torch.cuda.synchronize()
    try:
        ctx.set_stream(s.cuda_stream)
        for select, want in ((lambda: ctx.pair_distance_select(xy, ranks), sv[ranks]), (lambda: nbr.distance_select(dranks), sd[dranks])):
            with torch.cuda.stream(s):
                for _ in range(links):
                    torch.mm(a, a, out=c)
                queued = torch.cuda.Event()
                queued.record(s)
            busy = not queued.query()
            got, _ = select()
            assert busy, 'the delay chain had drained before the call: nothing was tested'
            assert queued.query()                                       # synchronous on the caller's stream
            assert np.array_equal(rr.bits(got), rr.bits(want))
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        nbr.close()
