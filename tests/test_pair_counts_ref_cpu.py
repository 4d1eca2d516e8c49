"""The NumPy restatement of the enriched-pair counts (tests/pair_counts_ref.py) held to the per-attribute loops the reference
would write -- scipy's pdist and networkx's bounded Dijkstra on each attribute's enriched nodes -- and the host side of
attribute_unimodality_metric = 'radius': the two new settings, pickling, and the two new symbols.  No device needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
from scipy.spatial.distance import pdist

import pair_counts_ref as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clustered_values(n, m, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(size=(n, m)) < rng.uniform(0.02, 0.4, size=m)).astype(np.float64)
    v[:, 0] = 0                                                           # nothing enriched
    v[:, 1] = pc.ODD_VALUES[np.arange(n) % pc.ODD_VALUES.size]            # only 1, 2.5 and +inf are
    v[n // 3, 2] = np.nan
    return v


def test_restatement_equals_the_pdist_loop_on_a_clustered_layout():
    xy = pc.two_clusters(per=60, seed=1)
    xy[60:, 0] -= 0.93                                                    # the clusters now overlap at their edges
    n, m = xy.shape[0], 9
    v = clustered_values(n, m, seed=2)
    for t in (0.01, 0.03, 0.08, 5.0):
        w = pc.within_euclidean(xy, t)
        q, e = pc.pair_counts(v, np.arange(m), w)
        pairs, within = pc.pairs_within(q, e)
        for a in range(m):
            idx = np.flatnonzero(v[:, a] > 0)
            assert e[a] == idx.size
            assert pairs[a] == idx.size * (idx.size - 1) // 2
            assert within[a] == int((pdist(xy[idx]) < t).sum()), (t, a)
    assert within[3] == pairs[3] and e[0] == 0 and q[0] == 0              # t = 5: everything within reach
    assert e[1] == int(pc.ODD_ENRICHED[np.arange(n) % 8].sum())


@pytest.mark.parametrize('weight', ['length', 'weight'])
def test_restatement_equals_bounded_dijkstra_on_each_enriched_set(weight):
    """'length' is what shortpath_weighted_layout searches on, 'weight' (absent here: hops) what shortpath does."""
    import networkx as nx
    G, xy = pc.flow_graph(n=90, seed=4, lonely=10)                        # two components
    assert nx.number_connected_components(G) >= 2
    n, m = 90, 8
    v = clustered_values(n, m, seed=5)
    for t in ((0.15, 0.4) if weight == 'length' else (1, 2, 3.5)):
        w = pc.within_shortpath(G, t, weight)
        assert np.array_equal(w, w.T) and (np.diag(w) == 1).all()
        q, e = pc.pair_counts(v, np.arange(m), w)
        pairs, within = pc.pairs_within(q, e)
        dist = dict(nx.all_pairs_dijkstra_path_length(G, cutoff=t, weight=weight))
        for a in range(m):
            idx = np.flatnonzero(v[:, a] > 0).tolist()
            want = sum(1 for k, i in enumerate(idx) for j in idx[k + 1:] if j in dist[i])
            assert within[a] == want and pairs[a] == len(idx) * (len(idx) - 1) // 2, (t, a)
        assert (within < pairs).any()                                     # unreached pairs exist


def test_q_is_e_plus_twice_within_for_symmetric_w_only():
    rng = np.random.default_rng(6)
    n, m = 70, 6
    v = clustered_values(n, m, seed=7)
    w = pc.within_euclidean(rng.uniform(size=(n, 2)), 0.3)
    q, e = pc.pair_counts(v, np.arange(m), w)
    for a in range(m):
        idx = np.flatnonzero(v[:, a] > 0)
        within = sum(int(w[i, j]) for k, i in enumerate(idx) for j in idx[k + 1:])
        assert q[a] == e[a] + 2 * within
    # the raw form for any matrix: asymmetric, no diagonal
    asym = (rng.uniform(size=(n, n)) < 0.2).astype(np.int64)
    q, e = pc.pair_counts(v, [3, 3, 5], asym)
    for k, a in enumerate([3, 3, 5]):
        idx = np.flatnonzero(v[:, a] > 0)
        assert q[k] == asym[np.ix_(idx, idx)].sum() and e[k] == idx.size


def test_designed_attributes_keep_drop_keep():
    xy = pc.two_clusters()
    nb, num = pc.designed_attributes()
    assert num.tolist() == [12, 24, 13]
    r = pc.CLUSTER_RADIUS * pc.x_range(xy)
    t = pc.DEFAULT_MULTIPLE * r
    d0 = pdist(xy[:150]).max()
    assert d0 < t and pdist(xy[150:]).max() < t and t < 0.5               # a cluster's diameter < 2 r << the gap
    got = pc.table(nb, [0, 1, 2], pc.within_euclidean(xy, t))
    assert np.array_equal(got['pairs'], pc.DESIGNED_PAIRS) and np.array_equal(got['within'], pc.DESIGNED_WITHIN)
    assert got['fraction'].tolist() == [1.0, 132 / 276, 66 / 78]
    assert np.array_equal(got['fails'], pc.DESIGNED_FAILS)
    # the bound itself: within == min_fraction * pairs is kept (strict <)
    assert not pc.fails(np.array([100]), np.array([50]), 0.5)[0]
    assert pc.fails(np.array([100]), np.array([49]), 0.5)[0]
    assert not pc.fails(np.array([0]), np.array([0]), 1.0)[0]             # no pair: nothing to fail


def test_pattern_columns_are_what_their_names_say():
    v, names = pc.pattern_columns(200, seed=1)
    e = (v > 0).sum(0)
    by = dict(zip(names, e.tolist()))
    assert by['empty'] == 0 and by['full'] == 200 and by['one_node'] == 1 and by['last_row'] == 1 and v[199, names.index('last_row')] == 1
    assert by['bit63'] == 3 and by['alternating'] == 100
    assert by['odd_values_cycle'] == int(pc.ODD_ENRICHED[np.arange(200) % 8].sum())


# ---- the host side ----------------------------------------------------------------------------------------------------------

def test_new_settings_have_their_defaults_and_are_validated():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.attribute_unimodality_metric == 'connectivity'
    assert sf.attribute_unimodality_radius_multiple == 2.0 and sf.attribute_unimodality_min_fraction == 0.65
    for bad in (0, -1.0, np.inf, np.nan, 'two', None, True):
        sf.attribute_unimodality_radius_multiple = bad
        with pytest.raises(ValueError, match='attribute_unimodality_radius_multiple'):
            sf.validate_config()
        assert sf.attribute_unimodality_radius_multiple == 2.0
    for bad in (0, 0.0, -0.5, 1.0000001, 2, np.nan, '0.5', None, True):
        sf.attribute_unimodality_min_fraction = bad
        with pytest.raises(ValueError, match='attribute_unimodality_min_fraction'):
            sf.validate_config()
        assert sf.attribute_unimodality_min_fraction == 0.65
    for good_multiple, good_fraction in ((1, 1), (0.5, 1.0), (3.0, 1e-9), (np.float64(2.5), np.float32(0.5))):
        sf.attribute_unimodality_radius_multiple, sf.attribute_unimodality_min_fraction = good_multiple, good_fraction
        sf.validate_config()
    sf.attribute_unimodality_metric = 'anything'                          # the metric itself stays unvalidated
    sf.validate_config()


def test_kwargs_of_define_top_attributes_are_validated_before_anything_is_written():
    import pandas as pd
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.attributes = pd.DataFrame({'name': ['a', 'b'], 'num_neighborhoods_enriched': [20, 3]})
    with pytest.raises(ValueError, match='attribute_unimodality_min_fraction'):
        sf.define_top_attributes(attribute_unimodality_metric='radius', attribute_unimodality_min_fraction=1.5)
    assert 'top' not in sf.attributes.columns and sf.attribute_unimodality_min_fraction == 0.65
    # any other value of the metric skips requirement 2 and needs no device
    sf.define_top_attributes(attribute_unimodality_metric='none')
    assert sf.attributes['top'].tolist() == [True, False]
    assert list(sf.attributes.columns) == ['name', 'num_neighborhoods_enriched', 'top']


def test_pickle_round_trip_and_old_state(tmp_path):
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.attribute_unimodality_metric = 'radius'
    sf.attribute_unimodality_radius_multiple = 1.5
    sf.attribute_unimodality_min_fraction = 0.9
    path = str(tmp_path / 'safe_output.p')
    sf.save(output_file=path)
    with open(path, 'rb') as handle:
        back = pickle.load(handle)
    assert back.attribute_unimodality_metric == 'radius'
    assert back.attribute_unimodality_radius_multiple == 1.5 and back.attribute_unimodality_min_fraction == 0.9
    back.validate_config()
    # an object pickled before the settings existed
    state = sf.__getstate__()
    del state['attribute_unimodality_radius_multiple'], state['attribute_unimodality_min_fraction']
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.attribute_unimodality_radius_multiple == 2.0 and old.attribute_unimodality_min_fraction == 0.65
    old.validate_config()


def test_header_binding_and_library_agree_on_the_new_symbols():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in {'safe_enriched_pair_counts': 6, 'safe_enriched_pair_counts_dev': 10}.items():
        m = re.search(r'\bint %s\s*\(([^;]*)\);' % name, code)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        assert hasattr(raw, name), name
    dev = _lib.PROTOTYPES['safe_enriched_pair_counts_dev'][1]
    assert dev[3] is ctypes.c_int64 and dev[4] is ctypes.c_int64 and dev[6] is ctypes.c_int64
    assert hasattr(backend, 'enriched_pair_counts') and hasattr(backend, 'enriched_pair_counts_dev')
    assert hasattr(backend.Context, 'enriched_pair_counts_dev')
    # NULL arguments are refused before a device is touched
    assert _lib.lib.safe_enriched_pair_counts(None, None, None, 1, None, None) == _lib.E_INVALID
    assert _lib.lib.safe_enriched_pair_counts_dev(None, None, None, 1, 1, None, 1, None, None, None) == _lib.E_INVALID
    # the symbols are additive: header, binding and library agree on the unchanged ABI version
    assert '#define SAFE_HIP_ABI_VERSION 9' in header
    assert _lib.ABI_VERSION == raw.safe_abi_version() == 9
