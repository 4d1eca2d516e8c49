"""node_distance_metric = 'diffusion' through SAFE on a 300-node graph: define_neighborhoods under the three radius types, the
enrichment routes, the distance weights, the 'radius' unimodality metric, compute_node_distances, node_distance_percentile,
pickling and the refusals, all against the NumPy restatement of the contract (tests/diffusion_ref.py).  Needs an MI355X."""
import pickle

import numpy as np
import pytest

import diffusion_ref as dr
import nearest_ref as nr
import pair_counts_ref as pc
import radius_ref as rr
import weights_ref as wr

pytestmark = pytest.mark.gpu

N = 300
OUTPUTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def world():
    """The graph (edges carry 'length' and no 'weight': unit weights), its edge arrays and the restated distance matrix at the
    default parameters; nothing changes it."""
    G, xy = pc.flow_graph(n=N)
    eu = np.array([u for u, _ in G.edges()])
    ev = np.array([v for _, v in G.edges()])
    d = dr.distance(dr.kernel(N, eu, ev, None, 0.5, 32))
    d.setflags(write=False)
    assert np.isposinf(d[0, N - 1])                                     # the lonely path is cut off
    return G, xy, eu, ev, d


def _safe(amd, graph, **settings):
    sf = amd.SAFE(verbose=False)
    sf.graph = graph
    for key, value in settings.items():
        setattr(sf, key, value)
    return sf


def _finite_upper(d):
    v = d[np.triu_indices(d.shape[0], 1)]
    return v[np.isfinite(v)]


def _want(d, kind, radius):
    """(membership, radius resolved, radii or None) of a radius type from the restated matrix."""
    if kind == 'nearest':
        r = nr.radii(d, radius, True)
        return nr.membership(d, r, True), float(np.median(r)), r
    resolved = float(np.percentile(_finite_upper(d), radius)) if kind == 'percentile' else float(radius)
    return dr.members(d, resolved), resolved, None


CASES = [('percentile', 2.0), ('percentile', 0.5), ('nearest', 10), ('absolute', 0.85)]


@pytest.mark.parametrize('kind,radius', CASES)
def test_define_neighborhoods(amd, world, kind, radius):
    G, _, _, _, d = world
    a, resolved, radii = _want(d, kind, radius)
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type=kind, neighborhood_radius=radius)
    assert np.array_equal(sf.neighborhoods, a)
    assert a.diagonal().all() and 0 < a.sum() - N < N * N - N           # a real neighborhood structure
    assert nr.bits(sf.neighborhood_radius_resolved)[0] == nr.bits(resolved)[0]
    if radii is None:
        assert sf.neighborhood_radii is None
    else:
        assert np.array_equal(nr.bits(sf.neighborhood_radii), nr.bits(radii))
    assert np.array_equal(nr.bits(rr.dense_of(sf.node_distances, N)), nr.bits(nr.masked(d, a)))
    other = _safe(amd, G)
    other.compute_node_distances(node_distance_metric='diffusion', neighborhood_radius_type=kind, neighborhood_radius=radius)
    assert other.neighborhoods is None
    assert np.array_equal(nr.bits(rr.dense_of(other.node_distances, N)), nr.bits(nr.masked(d, a)))


def test_node_distance_percentile(amd, world):
    G, _, _, _, d = world
    sf = _safe(amd, G, node_distance_metric='diffusion')
    qs = [0, 0.5, 2.0, 50, 99.9, 100]
    got = sf.node_distance_percentile(qs)
    assert np.array_equal(nr.bits(got), nr.bits(np.percentile(_finite_upper(d), qs)))
    assert sf.node_distance_percentile(2.0) == float(np.percentile(_finite_upper(d), 2.0))
    assert sf.neighborhoods is None and sf.node_distances is None


def test_other_parameters_and_the_weight_attribute(amd, world):
    """diffusion_restart / diffusion_steps as keywords; the 'weight' edge attribute is the walk's weight, 'length' never."""
    G, _, eu, ev, _ = world
    H = G.copy()
    rng = np.random.default_rng(4)
    for u, v in H.edges():
        H[u][v]['weight'] = float(rng.uniform(0.2, 2.5))
    w = np.array([H[u][v]['weight'] for u, v in H.edges()])
    heu = np.array([u for u, _ in H.edges()])
    hev = np.array([v for _, v in H.edges()])
    d = dr.distance(dr.kernel(N, heu, hev, w, 0.2, 6))
    sf = _safe(amd, H)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='absolute', neighborhood_radius=0.9,
                            diffusion_restart=0.2, diffusion_steps=6)
    assert (sf.diffusion_restart, sf.diffusion_steps) == (0.2, 6)
    assert np.array_equal(sf.neighborhoods, dr.members(d, 0.9))
    assert np.array_equal(nr.bits(rr.dense_of(sf.node_distances, N)), nr.bits(dr.kept(d, 0.9)))


def _attributes(kind, n, m, seed):
    rng = np.random.default_rng(seed)
    if kind == 'binary':
        b = (rng.uniform(size=(n, m)) < rng.uniform(0.03, 0.3, size=m)).astype(np.float64)
    else:
        b = rng.normal(size=(n, m))
    b[rng.choice(n, 12, replace=False)] = np.nan
    return b


ROUTES = [('binary', dict(how='hypergeometric')),
          ('binary', dict(how='randomization', num_permutations=25, verbose=False)),
          ('quantitative', dict(how='randomization', num_permutations=25, verbose=False)),
          ('quantitative', dict(how='randomization', neighborhood_score_type='z-score', num_permutations=25, verbose=False)),
          ('quantitative', dict(how='analytic'))]


@pytest.mark.parametrize('data,call', ROUTES, ids=lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values()))
@pytest.mark.parametrize('kind,radius', [('percentile', 5.0), ('nearest', 10)])
def test_compute_pvalues_equals_an_instance_with_the_restated_membership(amd, world, kind, radius, data, call):
    G, _, _, _, d = world
    a, _, _ = _want(d, kind, radius)
    b = _attributes(data, N, 30, 2)
    got = _safe(amd, G, random_seed=7)
    got.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type=kind, neighborhood_radius=radius)
    want = _safe(amd, G, random_seed=7)
    want.neighborhoods = a.copy()
    for sf in (got, want):
        sf.load_attributes(attribute_file=b.copy())
        sf.compute_pvalues(**call)
    for key in OUTPUTS:
        x, y = getattr(got, key), getattr(want, key)
        assert (x is None) == (y is None), key
        if x is not None:
            assert np.array_equal(nr.bits(x), nr.bits(y)), key
    assert np.array_equal(got.attributes['num_neighborhoods_enriched'].values, want.attributes['num_neighborhoods_enriched'].values)
    assert np.isfinite(got.nes).any()


@pytest.mark.parametrize('kind,radius', [('percentile', 2.0), ('nearest', 10), ('absolute', 0.85)])
def test_triangular_weights_come_from_the_kept_distances(amd, world, kind, radius):
    G, _, _, _, d = world
    a, resolved, radii = _want(d, kind, radius)
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type=kind, neighborhood_radius=radius,
                            neighborhood_weighting='triangular')
    indptr, indices = wr.csr_of(a)
    want = wr.member_weights('triangular', wr.matrix_member_distances(d, indptr, indices), indptr, resolved if radii is None else radii)
    w = sf.neighborhood_weights
    assert np.array_equal(w.indptr, indptr) and np.array_equal(w.indices, indices)
    assert np.array_equal(nr.bits(w.data), nr.bits(want))
    assert (want == 1.0).sum() >= N and ((want > 0) & (want < 1)).any()


def test_radius_unimodality_uses_the_diffusion_reach(amd, world):
    import pandas as pd
    G, xy, _, _, d = world
    b = pc.flow_attributes(xy)
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='percentile', neighborhood_radius=2.0)
    sf.load_attributes(attribute_file=b.copy())
    sf.attributes = pd.DataFrame({'id': np.arange(b.shape[1]), 'name': ['a%d' % i for i in range(b.shape[1])]})
    sf.compute_pvalues()
    sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_enrichment_min_size=10,
                             attribute_unimodality_radius_multiple=1.15, attribute_unimodality_min_fraction=0.4)
    resolved = float(np.percentile(_finite_upper(d), 2.0))
    assert sf.neighborhood_radius_resolved == resolved
    cand = sf.attributes['num_neighborhoods_enriched'].values >= 10
    assert cand.sum() >= 3
    t = pc.table(sf.nes_binary, np.flatnonzero(cand), dr.members(d, 1.15 * resolved), 0.4)      # `<=`, the diagonal, reached pairs
    top = cand.copy()
    top[cand] = ~t['fails']
    assert t['fails'].any() and not t['fails'].all()                    # the relation splits the candidates
    assert np.array_equal(sf.attributes['top'].values, top)
    assert np.array_equal(sf.attributes['num_enriched_pairs'].values[cand], t['pairs'])
    assert np.array_equal(sf.attributes['num_enriched_pairs_within'].values[cand], t['within'])


def test_pickle_round_trip(amd, world):
    G, _, _, _, d = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='nearest', neighborhood_radius=10,
                            diffusion_restart=0.5, diffusion_steps=32)
    clone = pickle.loads(pickle.dumps(sf))
    a, resolved, radii = _want(d, 'nearest', 10)
    assert (clone.node_distance_metric, clone.diffusion_restart, clone.diffusion_steps) == ('diffusion', 0.5, 32)
    assert np.array_equal(clone.neighborhoods, a) and clone.neighborhood_radius_resolved == resolved
    assert np.array_equal(nr.bits(clone.neighborhood_radii), nr.bits(radii))
    assert np.array_equal(nr.bits(rr.dense_of(clone.node_distances, N)), nr.bits(nr.masked(d, a)))
    assert np.array_equal(nr.bits(rr.dense_of(sf.node_distances, N)), nr.bits(nr.masked(d, a)))


def test_refusals_leave_everything_as_it_was(amd, world):
    G, _, _, _, d = world
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='absolute', neighborhood_radius=0.85)
    sf.load_attributes(attribute_file=_attributes('binary', N, 12, 3))
    sf.compute_pvalues(how='hypergeometric')
    before = (sf.neighborhoods.copy(), rr.dense_of(sf.node_distances, N), sf.nes.copy(), sf.neighborhood_radius_resolved)

    def unchanged():
        assert np.array_equal(sf.neighborhoods, before[0]) and np.array_equal(rr.dense_of(sf.node_distances, N), before[1])
        assert np.array_equal(nr.bits(sf.nes), nr.bits(before[2])) and sf.neighborhood_radius_resolved == before[3]

    for kind in ('diameter', None):
        with pytest.raises(ValueError, match="'diameter' is not defined"):
            sf.define_neighborhoods(neighborhood_radius_type=kind, neighborhood_radius=0.1)
        unchanged()
        with pytest.raises(ValueError, match="'diameter' is not defined"):
            sf.compute_node_distances()
        unchanged()
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'absolute', 0.85
    for bad in (dict(diffusion_restart=0.0), dict(diffusion_restart=1), dict(diffusion_steps=0), dict(diffusion_steps=2.5),
                dict(node_distance_metric='manhattan')):
        with pytest.raises(ValueError):
            sf.define_neighborhoods(**bad)
        unchanged()
    assert (sf.diffusion_restart, sf.diffusion_steps) == (0.5, 32)
    assert sf.node_distance_metric == 'shortpath_weighted_layout'       # 'manhattan' restored the default


@pytest.mark.parametrize('metric', ['euclidean', 'shortpath', 'shortpath_weighted_layout'])
def test_other_metrics_give_the_same_bytes_after_diffusion_was_used(amd, world, metric):
    G, _, _, _, _ = world
    radius = 2 if metric == 'shortpath' else 0.15

    def run(sf):
        sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius_type='diameter', neighborhood_radius=radius)
        nd = sf.node_distances
        return sf.neighborhoods.copy(), None if nd is None else rr.dense_of(nd, N), sf.neighborhood_radius_resolved

    fresh = run(_safe(amd, G))
    sf = _safe(amd, G)
    sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='nearest', neighborhood_radius=10)
    again = run(sf)
    assert np.array_equal(fresh[0], again[0]) and fresh[2] == again[2]
    if metric != 'euclidean':                                           # ('euclidean' leaves node_distances as they were, as before)
        assert np.array_equal(nr.bits(fresh[1]), nr.bits(again[1]))
    assert sf.neighborhood_radii is None


def test_an_edge_list_without_coordinates_needs_no_layout(amd, world):
    """'diffusion' reads no coordinate: a graph whose nodes have no x / y gives the same neighborhoods and the same results (the
    layout hint, which only orders the nodes on the device, is then left out)."""
    import networkx as nx
    G, _, _, _, d = world
    bare = nx.Graph()
    bare.add_nodes_from(range(N))
    bare.add_edges_from(G.edges())
    a, resolved, _ = _want(d, 'percentile', 5.0)
    b = _attributes('quantitative', N, 20, 5)
    got, want = _safe(amd, bare, random_seed=3), _safe(amd, G, random_seed=3)
    for sf in (got, want):
        sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='percentile', neighborhood_radius=5.0)
        assert np.array_equal(sf.neighborhoods, a) and sf.neighborhood_radius_resolved == resolved
        sf.load_attributes(attribute_file=b.copy())
        sf.compute_pvalues(how='randomization', num_permutations=25, verbose=False)
    for key in OUTPUTS:
        assert np.array_equal(nr.bits(getattr(got, key)), nr.bits(getattr(want, key))), key
