"""neighborhood_weighting through SAFE: neighborhood_weights against the restatement of tests/weights_ref.py from SciPy /
networkx distances, a designed pair of attributes that only weights can tell apart, whole compute_pvalues calls against the
restated scores, counts and the library-level entry points (themselves pinned in tests/test_gpu_weights.py), the default,
pickling, refusals that leave the results, and steady device memory.  Needs an MI355X."""
import math
import pickle

import numpy as np
import pytest

import fdr_scope_ref as fsr
import moments_ref as mr
import nearest_ref as nr
import radius_ref as rr
import weights_ref as wr

pytestmark = pytest.mark.gpu

METRIC_WEIGHT = {'shortpath_weighted_layout': 'length', 'shortpath': 'weight'}
METRICS = ['euclidean'] + sorted(METRIC_WEIGHT)
N_FLOW = 256                                    # a power of two: the mean of a 0/1 column is exact (the designed pair)
DIAMETER_RADIUS = {'euclidean': 0.15, 'shortpath_weighted_layout': 0.15, 'shortpath': 2}
RESULTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')
NPERM, SEED = 50, 5


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


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
    return G, xy, dmat


@pytest.fixture(scope='module')
def values():
    rng = np.random.default_rng(77)
    b = np.round(rng.normal(size=(N_FLOW, 6)) * 3, 3)
    b[rng.choice(N_FLOW, 15, replace=False)] = np.nan
    b[rng.uniform(size=b.shape) < 0.03] = np.nan
    return b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    assert np.array_equal(bits(got), bits(want)), what


def _safe(amd, graph, **settings):
    sf = amd.SAFE(verbose=False)
    sf.graph = graph
    for key, value in settings.items():
        setattr(sf, key, value)
    return sf


def _weighted(amd, world, values, kind='triangular', **settings):
    sf = _safe(amd, world[0], **settings)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.15, neighborhood_weighting=kind)
    sf.load_attributes(attribute_file=values.copy())
    return sf


def _results(sf):
    return {name: np.array(getattr(sf, name), dtype=np.float64) for name in RESULTS}


def _csr_weights(sf):
    w = sf.neighborhood_weights
    return w.indptr.astype(np.int64), w.indices.astype(np.int64), w.data.copy()


# ---- neighborhood_weights ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('radius_type', ['diameter', 'nearest'])
@pytest.mark.parametrize('metric', METRICS)
def test_neighborhood_weights_against_the_restatement(amd, world, metric, radius_type):
    G, xy, dmat = world
    d = dmat[metric]
    radius = 10 if radius_type == 'nearest' else DIAMETER_RADIUS[metric]
    for kind, h in (('uniform', 0.5), ('triangular', 0.5), ('epanechnikov', 0.5), ('gaussian', 0.25), ('gaussian', 2.0)):
        sf = _safe(amd, G)
        sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type=radius_type, neighborhood_radius=radius,
                                neighborhood_weighting=kind, neighborhood_weight_bandwidth=h)
        assert (sf.neighborhood_weighting, sf.neighborhood_weight_bandwidth) == (kind, h)
        w = sf.neighborhood_weights
        indptr, indices = wr.csr_of(sf.neighborhoods)
        assert w.shape == (N_FLOW, N_FLOW) and w.dtype == np.float64 and w.format == 'csr'
        assert np.array_equal(w.indptr, indptr) and np.array_equal(w.indices, indices)      # the membership's pattern, zeros kept
        radii = sf.neighborhood_radii if radius_type == 'nearest' else sf.neighborhood_radius_resolved
        dist = wr.matrix_member_distances(d, indptr, indices)
        assert np.isfinite(dist).all()
        what = '%s %s %s' % (metric, radius_type, kind)
        if kind != 'gaussian':
            same_bits(w.data, wr.member_weights(kind, dist, indptr, radii), what)
            if kind == 'triangular' and radius_type == 'nearest':
                assert (w.data == 0).any()                      # the k-th nearest node: d == r, weight 0, still a member
        else:
            r = np.broadcast_to(np.asarray(radii, dtype=np.float64), (N_FLOW,))[wr.rows_of(indptr)]
            arg = wr.gaussian_argument(dist, r, h)
            ua, first = np.unique(arg, return_index=True)
            pick = np.arange(len(ua))[::max(1, len(ua) // 300)]
            assert wr.exp_error_ulps(ua[pick], w.data[first][pick]) <= wr.k_exp_ref() + 1.0, what
        w.data[:] = -1                                          # a copy: the object's weights are read-only
        assert (sf.neighborhood_weights.data >= 0).all()


# ---- the designed pair ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('how', ['analytic', 'randomization'])
def test_weights_tell_near_members_from_far_ones(amd, world, how):
    G, xy, dmat = world
    d = dmat['euclidean']
    a = (d < 0.15 * (xy[:, 0].max() - xy[:, 0].min()))
    c = int(np.argmax(a.sum(axis=1)))
    members = np.nonzero(a[c])[0]
    assert len(members) >= 12
    by_distance = members[np.argsort(d[c, members], kind='stable')]
    b = np.zeros((N_FLOW, 2))                                   # (five ones among 256 rows: mean and css are exact, so the two
    b[by_distance[:5], 0] = 1                                   #  columns have the same moments bit for bit); the five nearest
    b[by_distance[-5:], 1] = 1                                  # on the five farthest
    nes = {}
    for kind in ('none', 'triangular'):
        sf = _safe(amd, G, random_seed=SEED)
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.15, neighborhood_weighting=kind)
        sf.load_attributes(attribute_file=b.copy())
        sf.compute_pvalues(how=how, num_permutations=200)
        res = _results(sf)
        if kind == 'none':
            for name in RESULTS:
                same_bits(res[name][c, 0], res[name][c, 1], 'flat neighborhoods: %s differs between the two attributes' % name)
        nes[kind] = res['nes'][c]
    assert nes['triangular'][0] > nes['triangular'][1] > 0, nes


# ---- whole calls ------------------------------------------------------------------------------------------------------------

def _library_moments(be, ctx, sf, b, sign):
    """safe_moments_test_weighted on a handle of the test's own with the object's weights."""
    n, m = b.shape
    nbr = be.Neighborhoods.from_dense(ctx, sf.neighborhoods)
    attr = be.Attributes.from_host(ctx, b)
    bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
    try:
        nbr.set_weights(sf.neighborhood_weights.data)
        be.moments_test_weighted(ctx, nbr, attr, sign, 0.05, [x.ptr for x in bufs])
        return [x.download((n, m)) for x in bufs[:5]] + [bufs[5].download((m,))]
    finally:
        for x in bufs:
            x.free()
        attr.close()
        nbr.close()


def _from_counts(be, x, neg, pos, count, sign, thr=0.05):
    tab = be.nes_table(count)
    ep, en = tab[pos.astype(np.int64)], tab[neg.astype(np.int64)]
    nes = ep if sign == 'highest' else en if sign == 'lowest' else ep - en
    return {'ns': x, 'pvalues_neg': neg / float(count), 'pvalues_pos': pos / float(count), 'nes': nes,
            'nes_binary': (np.abs(nes) > -math.log10(thr)).astype(np.float64)}


@pytest.mark.parametrize('sign', mr.SIGNS)
def test_analytic_call(amd, be, ctx, world, values, sign):
    sf = _weighted(amd, world, values, attribute_sign=sign)
    sf.compute_pvalues(how='analytic')
    got = _results(sf)
    indptr, indices, w = _csr_weights(sf)
    same_bits(got['ns'], wr.score(indptr, indices, w, values), 'ns')
    want = _library_moments(be, ctx, sf, values, sign)
    for name, v in zip(RESULTS, want):
        same_bits(got[name], v, '%s %s' % (sign, name))
    assert np.array_equal(sf.attributes['num_neighborhoods_enriched'].values, want[5])
    z_sign = np.sign(got['pvalues_neg'] - got['pvalues_pos'])
    assert (z_sign > 0).any() and (z_sign < 0).any()


@pytest.mark.parametrize('sign', mr.SIGNS)
def test_randomization_call(amd, be, ctx, world, values, sign):
    sf = _weighted(amd, world, values, attribute_sign=sign, random_seed=SEED)
    sf.compute_pvalues(how='randomization', num_permutations=NPERM)
    got = _results(sf)
    indptr, indices, w = _csr_weights(sf)
    perms = be.Permutations(ctx, N_FLOW, mr.row_flags(values).astype(np.uint8), NPERM, SEED)
    try:
        tables = perms.read().astype(np.int64)
    finally:
        perms.close()
    want = _from_counts(be, *wr.counts(indptr, indices, w, values, tables), NPERM, sign)
    for name in RESULTS:
        same_bits(got[name], want[name], '%s %s' % (sign, name))
    assert np.array_equal(sf.attributes['num_neighborhoods_enriched'].values, want['nes_binary'].sum(axis=0))
    auto = _weighted(amd, world, values, attribute_sign=sign, random_seed=SEED)
    auto.compute_pvalues(num_permutations=NPERM)                # 'auto' on values other than 0/1
    for name in RESULTS:
        same_bits(_results(auto)[name], got[name], "'auto': " + name)


@pytest.mark.parametrize('scope', ['neighborhoods', 'all'])
@pytest.mark.parametrize('how', ['analytic', 'randomization'])
def test_multiple_testing_scopes(amd, world, values, how, scope):
    b = np.nan_to_num(values)                                   # (a NaN p-value would turn its whole family NaN)
    plain = _weighted(amd, world, b, random_seed=SEED)
    plain.compute_pvalues(how=how, num_permutations=NPERM)
    sf = _weighted(amd, world, b, random_seed=SEED)
    sf.compute_pvalues(how=how, num_permutations=NPERM, multiple_testing=True, multiple_testing_scope=scope)
    same_bits(sf.ns, plain.ns, 'ns')
    for name in ('pvalues_neg', 'pvalues_pos'):
        np.testing.assert_allclose(getattr(sf, name), fsr.want(getattr(plain, name), scope), rtol=1e-12, atol=0, err_msg=name)
    assert not np.array_equal(sf.pvalues_pos, plain.pvalues_pos)


def test_ranks_background_strata_custom_weights_and_eager_outputs(amd, be, ctx, world, values):
    from scipy import sparse, stats
    # ranks
    sf = _weighted(amd, world, values)
    sf.compute_pvalues(how='analytic', attribute_transform='rank')
    indptr, indices, w = _csr_weights(sf)
    ranked = stats.rankdata(values, method='average', axis=0, nan_policy='omit')
    same_bits(sf.ns, wr.score(indptr, indices, w, ranked), 'rank sums')
    # background = 'network'
    sf = _weighted(amd, world, values)
    sf.compute_pvalues(how='analytic', background='network')
    same_bits(sf.ns, wr.score(indptr, indices, w, values), 'ns under the network background')
    want = _library_moments(be, ctx, sf, np.nan_to_num(values), 'both')
    same_bits(sf.pvalues_pos, want[2], 'network background: every row is in the population')
    # strata
    labels = np.arange(N_FLOW) % 4
    sf = _weighted(amd, world, values, random_seed=SEED)
    sf.compute_pvalues(how='randomization', num_permutations=NPERM, permutation_strata=labels)
    flags = mr.row_flags(values).astype(np.uint8)
    perms = be.Permutations.stratified(ctx, N_FLOW, flags, labels.astype(np.int32), NPERM, SEED)
    try:
        tables = perms.read().astype(np.int64)
    finally:
        perms.close()
    assert (labels[tables] == labels[None, :]).all()
    want = _from_counts(be, *wr.counts(indptr, indices, w, values, tables), NPERM, 'both')
    for name in RESULTS:
        same_bits(getattr(sf, name), want[name], 'strata: ' + name)
    # custom weights, sparse and dense, members W does not store get 0
    rng = np.random.default_rng(8)
    custom = np.where(rng.uniform(size=len(indices)) < 0.2, 0.0, 1.0 - rng.uniform(size=len(indices)))
    W = sparse.csr_array((custom.copy(), indices.copy(), indptr.copy()), shape=(N_FLOW, N_FLOW))
    W.eliminate_zeros()
    for given in (W, W.toarray()):
        sf = _weighted(amd, world, values, kind='none')
        assert sf.neighborhood_weights is None
        sf.set_neighborhood_weights(given)
        assert sf.neighborhood_weighting == 'custom'
        got = sf.neighborhood_weights
        assert np.array_equal(got.indices, indices) and np.array_equal(got.indptr, indptr)
        same_bits(got.data, custom, 'custom weights')
        sf.compute_pvalues(how='analytic')
        same_bits(sf.ns, wr.score(indptr, indices, custom, values), 'ns under custom weights')
    # eager outputs: the same bytes as lazy ones
    eager = _weighted(amd, world, values, kind='none', lazy_outputs=False)
    eager.set_neighborhood_weights(W)
    eager.compute_pvalues(how='analytic')
    assert isinstance(eager.__dict__['_r_ns'], np.ndarray)    # already on the host
    for name in RESULTS:
        same_bits(getattr(eager, name), getattr(sf, name), 'eager: ' + name)
    # assigning neighborhoods drops the weights; 'custom' goes back to 'none'
    eager.neighborhoods = eager.neighborhoods.copy()
    assert eager.neighborhood_weighting == 'none' and eager.neighborhood_weights is None


def test_none_is_the_default_and_gives_its_bytes(amd, world, values):
    out = []
    for kwargs in ({}, {'neighborhood_weighting': 'none'}):
        sf = _safe(amd, world[0], random_seed=SEED)
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.15, **kwargs)
        assert sf.neighborhood_weights is None and not sf._nbr.has_weights
        sf.load_attributes(attribute_file=values.copy())
        res = []
        for how in ('analytic', 'randomization'):
            sf.compute_pvalues(how=how, num_permutations=NPERM)
            res.append(_results(sf))
        out.append((sf.neighborhoods.copy(), res))
    assert np.array_equal(out[0][0], out[1][0])
    for r0, r1 in zip(out[0][1], out[1][1]):
        for name in RESULTS:
            same_bits(r0[name], r1[name], name)
    # and unit weights give the flat analytic bytes on integer-valued data
    ints = np.random.default_rng(4).integers(0, 5, size=(N_FLOW, 4)).astype(np.float64)
    res = []
    for kind in ('none', 'uniform'):
        sf = _weighted(amd, world, ints, kind=kind)
        sf.compute_pvalues(how='analytic')
        res.append(_results(sf))
    for name in RESULTS:
        same_bits(res[0][name], res[1][name], 'uniform weights: ' + name)


def test_pickle_round_trip(amd, world, values):
    sf = _weighted(amd, world, values, kind='gaussian', neighborhood_weight_bandwidth=0.25)
    sf.compute_pvalues(how='analytic')
    before, w = _results(sf), sf.neighborhood_weights
    back = pickle.loads(pickle.dumps(sf))
    assert back._nbr is None and (back.neighborhood_weighting, back.neighborhood_weight_bandwidth) == ('gaussian', 0.25)
    same_bits(back.neighborhood_weights.data, w.data, 'weights')
    assert np.array_equal(back.neighborhood_weights.indices, w.indices)
    back.graph = world[0]
    back.compute_pvalues(how='analytic')                        # the rebuilt handle gets the weights back
    for name in RESULTS:
        same_bits(_results(back)[name], before[name], 'after unpickling: ' + name)


def test_refusals_leave_the_results(amd, world, values):
    sf = _weighted(amd, world, values)
    sf.compute_pvalues(how='analytic')
    before, w = _results(sf), sf.neighborhood_weights.data
    binary = _weighted(amd, world, (np.nan_to_num(values) > 2).astype(np.float64))
    binary.compute_pvalues(how='analytic')
    kept = _results(binary)
    with pytest.raises(ValueError, match="'analytic' or how = 'randomization'"):
        binary.compute_pvalues(how='auto')                      # 'auto' on 0/1 data is a hypergeometric route
    for name in RESULTS:
        same_bits(_results(binary)[name], kept[name], name)
    for kwargs, match in (({'how': 'hypergeometric'}, 'hypergeometric'),
                          ({'how': 'randomization', 'neighborhood_score_type': 'z-score'}, 'z-score')):
        with pytest.raises(ValueError, match=match):
            sf.compute_pvalues(**kwargs)
        sf.neighborhood_score_type, sf.enrichment_type = 'sum', 'analytic'
        for name in RESULTS:
            same_bits(_results(sf)[name], before[name], name)
    with pytest.raises(ValueError, match='set_neighborhood_weights'):
        sf.define_neighborhoods(neighborhood_weighting='custom')
    sf.neighborhood_weighting = 'triangular'
    member = sf.neighborhoods
    for bad in (np.ones((N_FLOW, N_FLOW)), -1.0 * member, np.where(member, np.nan, 0.0), np.ones((3, 3)), np.ones(N_FLOW)):
        with pytest.raises(ValueError):
            sf.set_neighborhood_weights(bad)
        assert sf.neighborhood_weighting == 'triangular'
        same_bits(sf.neighborhood_weights.data, w, 'a refused call changed the weights')
        same_bits(sf._nbr.weights(), w, 'a refused call changed the weights on the device')


def test_device_memory_is_steady(amd, be, world, values):
    sf = _weighted(amd, world, values, random_seed=SEED)
    for how in ('analytic', 'randomization'):
        sf.compute_pvalues(how=how, num_permutations=NPERM)
        _results(sf)
    sf.ns = sf.pvalues_neg = sf.pvalues_pos = sf.nes = sf.nes_binary = None
    live = be.device_live_alloc_count()
    for _ in range(3):
        for how in ('analytic', 'randomization'):
            sf.compute_pvalues(how=how, num_permutations=NPERM)
            _results(sf)
        sf.ns = sf.pvalues_neg = sf.pvalues_pos = sf.nes = sf.nes_binary = None
    assert be.device_live_alloc_count() == live
