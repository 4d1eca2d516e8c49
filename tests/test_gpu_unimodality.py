"""SAFE.define_top_attributes with attribute_unimodality_metric = 'radius': an attribute stays top when at least
attribute_unimodality_min_fraction of the pairs of its enriched nodes lie within attribute_unimodality_radius_multiple x the
resolved neighborhood radius of each other, under the current node_distance_metric.

Reference: tests/pair_counts_ref.py on the host copy of nes_binary, with the within-reach matrix from scipy's pdist
('euclidean') or networkx's bounded Dijkstra (the shortest-path metrics).  Every comparison is exact.  Needs an MI355X."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

import pair_counts_ref as pc

pytestmark = pytest.mark.gpu

RADIUS_COLUMNS = ['num_enriched_pairs', 'num_enriched_pairs_within', 'fraction_enriched_pairs_within']
CONNECTIVITY_COLUMNS = ['num_connected_components', 'size_connected_components', 'num_large_connected_components']


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


def is_resident(sf):
    from safepy_amd.safe import _DeviceResult
    return isinstance(sf.__dict__.get('_r_nes_binary'), _DeviceResult)


def same_column(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if want.dtype.kind != 'f':
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def expected(nes_binary, num_enriched, w, min_size, min_fraction):
    """The four columns 'radius' writes, from the restatement."""
    cand = np.asarray(num_enriched) >= min_size
    m = cand.size
    t = pc.table(nes_binary, np.flatnonzero(cand), w, min_fraction)
    pairs, within, frac = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.full(m, np.nan)
    pairs[cand], within[cand], frac[cand] = t['pairs'], t['within'], t['fraction']
    top = cand.copy()
    top[cand] = ~t['fails']
    return dict(top=top, num_enriched_pairs=pairs, num_enriched_pairs_within=within, fraction_enriched_pairs_within=frac)


def check_table(attrs, want):
    for name, col in want.items():
        assert same_column(attrs[name].values, col), (name, attrs[name].values, col)


# ------------------------------------------------------------------------------------------------------ designed case ----

def test_designed_attributes(amd):
    import pandas as pd
    xy = pc.two_clusters()
    nb, num = pc.designed_attributes()
    sf = amd.SAFE(verbose=False)
    sf.graph = pc.cluster_graph(xy)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=pc.CLUSTER_RADIUS)
    sf.attributes = pd.DataFrame({'id': np.arange(3), 'name': ['A', 'B', 'C'], 'num_neighborhoods_enriched': num})
    sf.nes_binary = nb
    sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_enrichment_min_size=10)
    assert sf.attributes['top'].tolist() == [True, False, True]
    t = pc.DEFAULT_MULTIPLE * (pc.CLUSTER_RADIUS * pc.x_range(xy))
    assert sf.neighborhood_radius_resolved == pc.CLUSTER_RADIUS * pc.x_range(xy)
    check_table(sf.attributes, expected(nb, num, pc.within_euclidean(xy, t), 10, pc.DEFAULT_MIN_FRACTION))
    assert np.array_equal(sf.attributes['num_enriched_pairs'].values, pc.DESIGNED_PAIRS)
    assert np.array_equal(sf.attributes['num_enriched_pairs_within'].values, pc.DESIGNED_WITHIN)
    assert sf.attributes['fraction_enriched_pairs_within'].tolist() == [1.0, 132 / 276, 66 / 78]
    assert sf.attributes['num_enriched_pairs'].dtype == np.int64 and sf.attributes['fraction_enriched_pairs_within'].dtype == np.float64
    assert not set(CONNECTIVITY_COLUMNS) & set(sf.attributes.columns)      # the connectivity columns are not written
    # a stricter fraction drops C too; a smaller multiple is a smaller reach
    sf.define_top_attributes(attribute_unimodality_min_fraction=0.9)
    assert sf.attributes['top'].tolist() == [True, False, False]
    sf.define_top_attributes(attribute_unimodality_min_fraction=0.65, attribute_unimodality_radius_multiple=0.25)
    check_table(sf.attributes, expected(nb, num, pc.within_euclidean(xy, 0.25 * (pc.CLUSTER_RADIUS * pc.x_range(xy))), 10, 0.65))
    assert sf.attributes['num_enriched_pairs_within'].values[0] < 66
    # the one stray node of C makes two components: 'connectivity' drops it
    sf.define_top_attributes(attribute_unimodality_metric='connectivity', attribute_unimodality_radius_multiple=2.0)
    assert not sf.attributes['top'].values[2] and not sf.attributes['top'].values[1]
    assert sf.attributes['num_connected_components'].values[2] >= 2
    # any other value skips requirement 2
    sf.define_top_attributes(attribute_unimodality_metric='none')
    assert sf.attributes['top'].tolist() == [True, True, True]


# -------------------------------------------------------------------------------------------------------- whole flows ----

@pytest.fixture(scope='module')
def flow():
    G, xy = pc.flow_graph()
    return G, xy, pc.flow_attributes(xy)


def run_flow(amd, flow, metric, radius, radius_type=None, read_first=False):
    import pandas as pd
    G, xy, b = flow
    sf = amd.SAFE(verbose=False)
    sf.graph = G
    kwargs = {} if radius_type is None else {'neighborhood_radius_type': radius_type}
    sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius=radius, **kwargs)
    sf.load_attributes(attribute_file=b.copy())
    sf.attributes = pd.DataFrame({'id': np.arange(b.shape[1]), 'name': ['a%d' % i for i in range(b.shape[1])]})
    sf.compute_pvalues()
    if read_first:
        assert sf.nes_binary.shape == b.shape and not is_resident(sf)
    else:
        assert is_resident(sf)
    return sf


def within_of(flow, metric, t):
    G, xy, _ = flow
    if metric == 'euclidean':
        return pc.within_euclidean(xy, t)
    return pc.within_shortpath(G, t, 'length' if metric == 'shortpath_weighted_layout' else 'weight')


@pytest.mark.parametrize('metric, radius', [('euclidean', 0.1), ('shortpath_weighted_layout', 0.15), ('shortpath', 2)])
def test_flow_resident_equals_host_equals_restatement(amd, flow, metric, radius):
    G, xy, b = flow
    dev, host = run_flow(amd, flow, metric, radius), run_flow(amd, flow, metric, radius, read_first=True)
    r = float(radius) if metric == 'shortpath' else radius * pc.x_range(xy)
    min_size = 10
    for multiple, min_fraction in ((2.0, 0.65), (1.0, 0.65), (2.0, 1.0), (3.5, 0.2)):
        for sf in (dev, host):
            sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_enrichment_min_size=min_size,
                                     attribute_unimodality_radius_multiple=multiple, attribute_unimodality_min_fraction=min_fraction)
            assert sf.neighborhood_radius_resolved == r
        assert is_resident(dev), 'define_top_attributes downloaded nes_binary'
        assert list(dev.attributes.columns) == list(host.attributes.columns)
        for col in dev.attributes.columns:
            assert dev.attributes[col].equals(host.attributes[col]), col
        num = host.attributes['num_neighborhoods_enriched'].values
        want = expected(host.nes_binary, num, within_of(flow, metric, multiple * r), min_size, min_fraction)
        check_table(dev.attributes, want)
        if (multiple, min_fraction) == (2.0, 0.65):                        # the default rule keeps some candidates and drops others
            assert want['top'].any() and ((num >= min_size) & ~want['top']).any()
        assert not set(CONNECTIVITY_COLUMNS) & set(dev.attributes.columns)
    assert (num >= min_size).sum() >= 5                                   # the flow has candidates to judge
    assert np.array_equal(dev.nes_binary, host.nes_binary)                # and the matrix is still what compute_pvalues made


def test_percentile_radius_is_resolved_before_the_multiple(amd, flow):
    G, xy, b = flow
    sf = run_flow(amd, flow, 'euclidean', 2.0, radius_type='percentile')
    sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_unimodality_radius_multiple=1.5)
    r = float(np.percentile(pdist(xy), 2.0))
    assert sf.neighborhood_radius_resolved == r
    assert is_resident(sf)
    num = sf.attributes['num_neighborhoods_enriched'].values
    nb = sf.nes_binary
    check_table(sf.attributes, expected(nb, num, pc.within_euclidean(xy, 1.5 * r), 10, pc.DEFAULT_MIN_FRACTION))
    assert (num >= 10).any()


def test_graph_without_coordinates_raises_and_leaves_the_table_alone(amd):
    import networkx as nx
    import pandas as pd
    n = 40
    G = nx.path_graph(n)                                                  # no x, no y
    nb = np.zeros((n, 2))
    nb[:15, 0] = 1
    nb[20:, 1] = 1
    for metric in ('euclidean', 'shortpath_weighted_layout'):
        sf = amd.SAFE(verbose=False)
        sf.graph = G
        sf.node_distance_metric = metric
        sf.attributes = pd.DataFrame({'name': ['a', 'b'], 'num_neighborhoods_enriched': [15, 20]})
        sf.nes_binary = nb
        before = sf.attributes.copy()
        with pytest.raises(ValueError, match='radius'):
            sf.define_top_attributes(attribute_unimodality_metric='radius')
        assert list(sf.attributes.columns) == list(before.columns) and sf.attributes.equals(before)
        # with a table that already has `top`, the old column stays whole
        sf.define_top_attributes(attribute_unimodality_metric='none')
        assert sf.attributes['top'].tolist() == [True, True]
        sf.attributes.loc[1, 'num_neighborhoods_enriched'] = 3
        with pytest.raises(ValueError, match='radius'):
            sf.define_top_attributes(attribute_unimodality_metric='radius')
        assert sf.attributes['top'].tolist() == [True, True]
    # hop counts need no coordinates: the same graph works under 'shortpath'
    sf = amd.SAFE(verbose=False)
    sf.graph = G
    sf.attributes = pd.DataFrame({'name': ['a', 'b'], 'num_neighborhoods_enriched': [15, 20]})
    sf.nes_binary = nb
    sf.node_distance_metric, sf.neighborhood_radius = 'shortpath', 3
    sf.define_top_attributes(attribute_unimodality_metric='radius')
    w = pc.within_shortpath(G, 6.0, 'weight')
    check_table(sf.attributes, expected(nb, np.array([15, 20]), w, 10, pc.DEFAULT_MIN_FRACTION))
