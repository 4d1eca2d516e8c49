"""neighborhood_radius_type = 'nearest' through SAFE, and the conventions every entry point of this library keeps: the whole
flow against SciPy / networkx through the restatement of tests/nearest_ref.py, compute_pvalues on the (asymmetric) result
against the CPU oracle, the four new entry points on a busy caller stream, steady device allocations, identical bytes from
identical calls, and refusals that write nothing.  Needs an MI355X."""
import ctypes as C
import logging
import pickle

import numpy as np
import pytest

import nearest_ref as nr
import pair_counts_ref as pc
import radius_ref as rr
import shortpath_ref as sp
from oracle import safe_oracle as orc

pytestmark = pytest.mark.gpu

METRIC_WEIGHT = {'shortpath_weighted_layout': 'length', 'shortpath': 'weight'}
METRICS = ['euclidean'] + sorted(METRIC_WEIGHT)
N_FLOW = 300
POISON = 0x7FF8DEADBEEF0001                                             # a NaN no computation makes


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(scope='module')
def world(amd):
    """The graph (with edge lengths), its coordinates, and the node-distance matrix of every metric from SciPy / networkx."""
    from safepy_amd import safe_io
    G, xy = rr.safe_graph(n=N_FLOW, tail=10)
    G = safe_io.calculate_edge_lengths(G, verbose=False)
    dmat = {metric: rr.nx_all_pairs(G, weight) for metric, weight in METRIC_WEIGHT.items()}
    dmat['euclidean'] = nr.euclid(xy)
    assert np.isinf(dmat['shortpath'][0, N_FLOW - 1])                   # one component is cut off
    for d in dmat.values():
        d.flags.writeable = False
    return G, xy, dmat


def _safe(amd, graph, **settings):
    sf = amd.SAFE(verbose=False)
    sf.graph = graph
    for key, value in settings.items():
        setattr(sf, key, value)
    return sf


def _want(world, metric, k):
    d = world[2][metric]
    reached = metric != 'euclidean'
    r = nr.radii(d, k, reached)
    return d, r, nr.membership(d, r, reached)


# ------------------------------------------------------------------ 4. whole flow ----

@pytest.mark.parametrize('k', [1, 10, 299, 400])
@pytest.mark.parametrize('metric', METRICS)
def test_define_neighborhoods_nearest(amd, world, metric, k):
    G, xy, _ = world
    d, r, a = _want(world, metric, k)
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=k)
    assert (sf.neighborhood_radius_type, sf.neighborhood_radius) == ('nearest', k)
    assert sf.neighborhood_radii.dtype == np.float64 and np.array_equal(nr.bits(sf.neighborhood_radii), nr.bits(r))
    assert isinstance(sf.neighborhood_radius_resolved, float)
    assert nr.bits(sf.neighborhood_radius_resolved)[0] == nr.bits(float(np.median(r)))[0]
    assert np.array_equal(sf.neighborhoods, a)
    assert (a.sum(axis=1) >= np.minimum(k, nr.sorted_candidates(d, metric != 'euclidean')[1]) + 1).all()
    other = _safe(amd, G)
    other.compute_node_distances(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=k)
    assert np.array_equal(nr.bits(other.neighborhood_radii), nr.bits(r))
    if metric == 'euclidean':
        assert np.array_equal(nr.bits(other.node_distances), nr.bits(d))              # the dense matrix, as under every type
    else:
        want = nr.masked(d, a)                                                        # the reached pairs inside every node's radius
        assert np.array_equal(nr.bits(rr.dense_of(sf.node_distances, N_FLOW)), nr.bits(want))
        assert np.array_equal(nr.bits(rr.dense_of(other.node_distances, N_FLOW)), nr.bits(want))
    if k == 10:
        assert not np.array_equal(a, a.T)                              # the flow below runs on an asymmetric membership


def test_other_types_leave_neighborhood_radii_unset(amd, world):
    G, _, _ = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=5)
    assert sf.neighborhood_radii is not None
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='diameter', neighborhood_radius=0.1)
    assert sf.neighborhood_radii is None
    plain = _safe(amd, G)
    plain.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1)
    assert np.array_equal(sf.neighborhoods, plain.neighborhoods)
    assert sf.neighborhood_radius_resolved == plain.neighborhood_radius_resolved


def _attributes(kind, n, m, seed):
    rng = np.random.default_rng(seed)
    if kind == 'binary':
        b = (rng.uniform(size=(n, m)) < rng.uniform(0.03, 0.3, size=m)).astype(np.float64)
    else:
        b = rng.normal(size=(n, m))
    b[rng.choice(n, 12, replace=False)] = np.nan
    return b


@pytest.mark.parametrize('metric', METRICS)
def test_compute_pvalues_hypergeometric_on_nearest(amd, world, metric):
    G, _, _ = world
    _, _, a = _want(world, metric, 10)
    b = _attributes('binary', N_FLOW, 40, 1)
    want = orc.compute_pvalues(a, b.copy())
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=10)
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='hypergeometric')
    np.testing.assert_allclose(sf.pvalues_pos, want['pvalues_pos'], rtol=1e-6, atol=1e-300)
    np.testing.assert_allclose(sf.nes, want['nes'], rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(sf.nes_binary, want['nes_binary'])
    np.testing.assert_array_equal(sf.attributes['num_neighborhoods_enriched'].values, want['num_neighborhoods_enriched'])


@pytest.mark.parametrize('kind,score', [('binary', 'sum'), ('quantitative', 'sum'), ('quantitative', 'z-score')])
@pytest.mark.parametrize('metric', METRICS)
def test_compute_pvalues_seeded_randomization_on_nearest(amd, world, metric, kind, score):
    G, _, _ = world
    _, _, a = _want(world, metric, 10)
    nperm, seed = 25, 7
    b = _attributes(kind, N_FLOW, 30, 2)
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type=score,
                               num_permutations=nperm, random_seed=seed)
    sf = _safe(amd, G, random_seed=seed)
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=10)
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='randomization', neighborhood_score_type=score, num_permutations=nperm, verbose=False)
    if kind == 'binary':
        np.testing.assert_array_equal(sf.ns, want['ns'])
    else:
        np.testing.assert_allclose(sf.ns, want['ns'], rtol=1e-9, atol=1e-12, equal_nan=True)
    for key in ('pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):    # counts / P: a flipped comparison shows as >= 1 / P
        np.testing.assert_array_equal(getattr(sf, key), want[key], err_msg=key)
    np.testing.assert_array_equal(sf.attributes['num_neighborhoods_enriched'].values, want['num_neighborhoods_enriched'])


@pytest.mark.parametrize('k,expect', [(1022, 'k_permtest_bits_blk'), (1023, 'k_permtest_bits_pre')])
def test_binary_randomization_on_wide_nearest_rows(amd, ctx, k, expect):
    """Rows of k + 1 members (untied uniform coordinates) on both sides of the blocked bit-sliced kernel's 1023: the asymmetric
    membership reaches the blocked and the sixteen-wave pre-permuted kernel, the shapes of
    test_gpu_parity.test_hub_neighborhoods_of_1024_to_2047_members_stay_bit_sliced; everything against the oracle."""
    rng = np.random.default_rng(k)
    n, m, nperm, seed = 2600, 70, 40, 21
    xy = rng.uniform(size=(n, 2))
    d = nr.euclid(xy)
    a = nr.membership(d, nr.radii(d, k, False), False)
    assert a.sum(axis=1).max() == k + 1 and not np.array_equal(a, a.T)
    b = (rng.uniform(size=(n, m)) < np.linspace(0.005, 0.99, m)).astype(np.float32)
    b[rng.choice(n, 30, replace=False)] = np.nan
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', num_permutations=nperm, random_seed=seed)
    sf = _safe(amd, amd.LayoutGraph(xy), random_seed=seed)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=k)
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='randomization', num_permutations=nperm, verbose=False)
    assert ctx.last_kernel()[0] == expect
    assert np.array_equal(sf.neighborhoods, a)
    for key in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
        np.testing.assert_array_equal(getattr(sf, key), want[key], err_msg=key)


def test_radius_unimodality_uses_the_median_radius(amd):
    import pandas as pd
    G, xy = pc.flow_graph()
    b = pc.flow_attributes(xy)
    k = 12
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=k)
    sf.load_attributes(attribute_file=b.copy())
    sf.attributes = pd.DataFrame({'id': np.arange(b.shape[1]), 'name': ['a%d' % i for i in range(b.shape[1])]})
    sf.compute_pvalues()
    sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_enrichment_min_size=10)
    median = float(np.median(nr.radii(nr.euclid(xy), k, False)))
    assert sf.neighborhood_radius_resolved == median
    num = sf.attributes['num_neighborhoods_enriched'].values
    cand = num >= 10
    assert cand.sum() >= 5                                             # the flow has candidates to judge
    t = pc.table(sf.nes_binary, np.flatnonzero(cand), pc.within_euclidean(xy, 2.0 * median), 0.65)
    top = cand.copy()
    top[cand] = ~t['fails']
    assert np.array_equal(sf.attributes['top'].values, top)
    assert np.array_equal(sf.attributes['num_enriched_pairs'].values[cand], t['pairs'])
    assert np.array_equal(sf.attributes['num_enriched_pairs_within'].values[cand], t['within'])


def test_nearest_is_logged_and_pickles(amd, world, caplog):
    G, _, _ = world
    sf = amd.SAFE(verbose=True)
    sf.graph = G
    with caplog.at_level(logging.INFO):
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=10.0)
    r = sf.neighborhood_radii
    assert '10 nearest nodes' in caplog.text
    assert '%r / %r / %r' % (float(r.min()), float(np.median(r)), float(r.max())) in caplog.text
    clone = pickle.loads(pickle.dumps(sf))
    assert np.array_equal(nr.bits(clone.neighborhood_radii), nr.bits(r)) and clone.neighborhood_radius_type == 'nearest'
    assert clone.neighborhood_radius_resolved == sf.neighborhood_radius_resolved
    assert np.array_equal(clone.neighborhoods, sf.neighborhoods)


# ------------------------------------------------------------------ 5. conventions ----

def _entry_points(amd, ctx, n=257, k=9):
    """name -> (call, expected bytes) of the four entry points on one input each; the calls return bytes."""
    xy = rr.xy_input('uniform', n)
    d = nr.euclid(xy)
    r = nr.radii(d, k, False)
    g = nr.component_graph(n)
    dg = sp.scipy_reference(g, np.inf)[1]
    rg = nr.radii(dg, k, True)
    src = amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, g.ew, np.inf, keep_distances=True)

    def built(nbr, keep):
        try:
            rp, col = nbr.csr()
            return nbr.to_dense().tobytes() + rp.tobytes() + col.tobytes() + (nbr.distances().tobytes() if keep else b'')
        finally:
            nbr.close()

    a, ag = nr.membership(d, r, False), nr.membership(dg, rg, True)
    fa, fg = sp.forms(a), sp.forms(ag)
    calls = {
        'safe_row_distance_select_xy': (lambda: ctx.row_distance_select(xy, k).tobytes(), r.tobytes()),
        'safe_nbr_row_distance_select': (lambda: src.row_distance_select(k).tobytes(), rg.tobytes()),
        'safe_nbr_euclidean_rows': (lambda: built(amd.Neighborhoods.euclidean_rows(ctx, xy, r), False),
                                    a.tobytes() + fa['row_ptr'].tobytes() + fa['col'].tobytes()),
        'safe_nbr_from_distances_rows': (lambda: built(amd.Neighborhoods.from_distances_rows(src, rg, keep_distances=True), True),
                                         ag.tobytes() + fg['row_ptr'].tobytes() + fg['col'].tobytes() + nr.masked(dg, ag).tobytes()),
    }
    return calls, src


def test_entry_points_on_a_busy_caller_stream(amd, ctx):
    """Each of the four after safe_ctx_set_stream on a caller's stream that still has a chain of matrix products queued (the
    delay of tests/test_gpu_radius.py): they are synchronous on that stream, so they return the quiet answer.

    Nothing is poisoned here, unlike in tests/test_gpu_stream_order.py: these entry points take host arrays (coordinates, radii)
    and a handle's own kept matrix, which the library wrote itself and no call of the interface can overwrite, so none of their
    inputs is produced on the caller's stream and there is no device buffer to poison and refill behind the delay."""
    import torch
    calls, src = _entry_points(amd, ctx)
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
        for name, (call, want) in calls.items():
            with torch.cuda.stream(s):
                for _ in range(links):
                    torch.mm(a, a, out=c)
                queued = torch.cuda.Event()
                queued.record(s)
            busy = not queued.query()
            got = call()
            assert busy, 'the delay chain had drained before the call: nothing was tested'
            assert queued.query(), name                                 # synchronous on the caller's stream
            assert got == want, name
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        src.close()


def test_identical_calls_give_identical_bytes_and_steady_allocations(amd, ctx):
    from safepy_amd import backend as be
    calls, src = _entry_points(amd, ctx, n=129, k=5)
    try:
        for name, (call, want) in calls.items():
            first = call()                                              # (warm-up: the context's scratch may grow once)
            assert first == want, name
            before = be.device_live_alloc_count()
            for _ in range(3):
                assert call() == first, name
            assert be.device_live_alloc_count() == before, name
    finally:
        src.close()


def _raw(amd):
    from safepy_amd import _lib
    from safepy_amd.backend import _ptr
    return _lib, _ptr


def test_refusals_write_nothing_and_keep_allocations_steady(amd, ctx):
    from safepy_amd import backend as be
    _lib, _ptr = _raw(amd)
    n = 9
    xy = rr.xy_input('uniform', n)
    nan_xy = xy.copy()
    nan_xy[4, 1] = np.nan
    good = np.full(n, 0.5)
    none = np.zeros(0, dtype=np.int32)
    kept = amd.Neighborhoods.shortpath(ctx, n, none, none, None, np.inf, keep_distances=True)
    bare = amd.Neighborhoods.shortpath(ctx, n, none, none, None, np.inf, keep_distances=False)
    poison = np.full(n, POISON, dtype=np.uint64)

    def select_xy(coords, k):
        out = poison.copy()
        rc = _lib.lib.safe_row_distance_select_xy(ctx.handle, _ptr(coords), n, k, _ptr(out))
        assert np.array_equal(out, poison)
        return rc

    def select_nbr(nbr, k):
        out = poison.copy()
        rc = _lib.lib.safe_nbr_row_distance_select(nbr.handle, k, _ptr(out))
        assert np.array_equal(out, poison)
        return rc

    def build_xy(radii):
        h = C.c_void_p(12345)
        rc = _lib.lib.safe_nbr_euclidean_rows(ctx.handle, _ptr(xy), n, _ptr(radii), C.byref(h))
        assert not h.value                                              # no handle comes back
        return rc

    def build_nbr(nbr, radii):
        h = C.c_void_p(12345)
        rc = _lib.lib.safe_nbr_from_distances_rows(nbr.handle, _ptr(radii), 1, C.byref(h))
        assert not h.value
        return rc

    def with_radius(value):
        r = good.copy()
        r[n - 1] = value
        return r

    refusals = [(lambda: select_xy(xy, 0), _lib.E_INVALID), (lambda: select_xy(xy, -3), _lib.E_INVALID),
                (lambda: select_xy(nan_xy, 2), _lib.E_VALUE),
                (lambda: select_nbr(kept, 0), _lib.E_INVALID), (lambda: select_nbr(bare, 2), _lib.E_INVALID),
                (lambda: build_xy(with_radius(-1.0)), _lib.E_VALUE), (lambda: build_xy(with_radius(np.nan)), _lib.E_VALUE),
                (lambda: build_nbr(kept, with_radius(-0.5)), _lib.E_VALUE), (lambda: build_nbr(kept, with_radius(np.nan)), _lib.E_VALUE),
                (lambda: build_nbr(bare, good), _lib.E_INVALID)]
    try:
        for t, (call, code) in enumerate(refusals):
            assert call() == code, t                                    # (warm-up)
            before = be.device_live_alloc_count()
            for _ in range(3):
                assert call() == code, t
            assert be.device_live_alloc_count() == before, t
        assert 'keep_distances' in _lib.lib.safe_last_error().decode()
        # a radii length other than n never reaches the library
        for r in (np.zeros(n - 1), np.zeros(n + 1), np.zeros((n, 1)), 0.5):
            with pytest.raises(ValueError):
                amd.Neighborhoods.euclidean_rows(ctx, xy, r)
            with pytest.raises(ValueError):
                amd.Neighborhoods.from_distances_rows(kept, r)
        # and the handles still answer
        assert np.array_equal(kept.row_distance_select(3), np.zeros(n))
        assert np.array_equal(kept.to_dense(), np.eye(n, dtype=np.int64))
    finally:
        kept.close()
        bare.close()


def test_refused_settings_are_restored_on_a_safe_instance(amd, world):
    G, xy, _ = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.15)
    before = sf.neighborhoods.copy()
    for bad in (0, -3, 2.5, float('nan')):
        with pytest.raises(ValueError):
            sf.define_neighborhoods(neighborhood_radius_type='nearest', neighborhood_radius=bad)
        assert (sf.neighborhood_radius_type, sf.neighborhood_radius) == ('diameter', 0.1)
        assert np.array_equal(sf.neighborhoods, before) and sf.neighborhood_radii is None     # refused before any device work
    with pytest.raises(ValueError):
        sf.define_neighborhoods(neighborhood_radius_type='k-nearest', neighborhood_radius=5)
    assert sf.neighborhood_radius_type == 'diameter'
    bad_xy = xy.copy()
    bad_xy[7, 0] = np.nan
    lone = _safe(amd, amd.LayoutGraph(bad_xy))
    with pytest.raises(amd.SafeHipError) as err:
        lone.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=5)
    assert err.value.code == -5 and lone.neighborhoods is None and lone.neighborhood_radii is None
    lone.validate_config()                                              # what is left is a valid configuration
    # a call that fails after one that succeeded leaves none of the earlier call's radii behind
    again = _safe(amd, amd.LayoutGraph(xy))
    again.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='nearest', neighborhood_radius=5)
    assert again.neighborhood_radii is not None and again.neighborhood_radius_resolved is not None
    again.graph = amd.LayoutGraph(bad_xy)
    with pytest.raises(amd.SafeHipError):
        again.define_neighborhoods()
    assert again.neighborhoods is None and again.neighborhood_radii is None and again.neighborhood_radius_resolved is None
    one = _safe(amd, amd.LayoutGraph(np.array([[0.25, 0.5]])))
    for metric in METRICS:                                              # a single node: no candidate, radius 0.0, itself
        one.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='nearest', neighborhood_radius=3)
        assert np.array_equal(one.neighborhood_radii, [0.0]) and np.array_equal(one.neighborhoods, [[1]])
