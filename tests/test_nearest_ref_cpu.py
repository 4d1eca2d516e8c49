"""neighborhood_radius_type = 'nearest' without a device: the NumPy restatement of the rule against a per-row sorted() loop
and a lattice worked out by hand, the square-root tie, validate_config, the INI file, pickling, and the four new symbols."""
import os
import pickle
import re

import numpy as np
import pytest

import nearest_ref as nr
import radius_ref as rr
import shortpath_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'safe_row_distance_select_xy': 5, 'safe_nbr_row_distance_select': 3, 'safe_nbr_euclidean_rows': 5,
               'safe_nbr_from_distances_rows': 4}


@pytest.mark.parametrize('kind', rr.KINDS)
@pytest.mark.parametrize('n', [1, 2, 3, 17, 65])
def test_restatement_equals_the_sorted_loop_on_coordinates(kind, n):
    d = nr.euclid(rr.xy_input(kind, n))
    sc = nr.sorted_candidates(d, False)
    assert np.array_equal(sc[1], np.full(n, n - 1))
    for k in nr.ks_for(n):
        assert np.array_equal(nr.bits(nr.radii_from_sorted(sc, k)), nr.bits(nr.radii_brute(d, k, False))), (kind, n, k)


@pytest.mark.parametrize('name', sorted(sp.edge_cases()))
def test_restatement_equals_the_sorted_loop_on_designed_graphs(name):
    g = sp.edge_cases()[name][0]
    d = sp.oracle_reference(g, np.inf)[1]
    for k in (1, 2, 3, g.n, g.n + 5):
        r = nr.radii(d, k, True)
        assert np.array_equal(nr.bits(r), nr.bits(nr.radii_brute(d, k, True))), (name, k)
        assert np.isfinite(r).all()                                    # an unreached node is no candidate
        a = nr.membership(d, r, True)
        assert (np.diag(a) == 1).all() and not a[np.isinf(d)].any()
        assert (a.sum(axis=1) >= np.minimum(k, np.isfinite(d).sum(axis=1) - 1) + 1).all()


def test_component_graph_has_components_ties_and_isolated_nodes():
    for n in (2, 3, 17, 129):
        g = nr.component_graph(n)
        assert sp.scipy_allowed(g)
        d = sp.scipy_reference(g, np.inf)[1]
        assert np.array_equal(nr.bits(nr.radii(d, 3, True)), nr.bits(nr.radii_brute(d, 3, True)))
        if n >= 3:
            assert np.isinf(d[n - 1, :n - 1]).all() and nr.radii(d, 3, True)[n - 1] == 0.0          # isolated: no candidate
            assert np.isinf(d[0, (n - max(1, n // 16)) - 1])                                          # two components
    d = sp.scipy_reference(nr.component_graph(129), np.inf)[1]
    big = nr.radii(d, 1000, True)                                      # k larger than a component: its largest distance
    assert np.array_equal(nr.bits(big), nr.bits(np.where(np.isfinite(d), d, 0.0).max(axis=1)))


def test_three_by_three_lattice_by_hand():
    """Nodes (a, b), a, b in 0..2, index 3 a + b.  From the corner (0, 0) the other eight lie at 1, 1, sqrt 2, 2, 2, sqrt 5,
    sqrt 5, sqrt 8; from the edge node (0, 1) at 1, 1, 1, sqrt 2, sqrt 2, 2, sqrt 5, sqrt 5; from the centre at 1 x 4, sqrt 2 x 4."""
    g = np.arange(3, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(9, 2)
    d = nr.euclid(xy)
    s2, s5, s8 = np.sqrt(2.0), np.sqrt(5.0), np.sqrt(8.0)
    corner = {1: (1.0, 3), 2: (1.0, 3), 3: (s2, 4), 4: (2.0, 6), 5: (2.0, 6), 6: (s5, 8), 7: (s5, 8), 8: (s8, 9), 9: (s8, 9)}
    edge = {1: (1.0, 4), 2: (1.0, 4), 3: (1.0, 4), 4: (s2, 6), 5: (s2, 6), 6: (2.0, 7), 7: (s5, 9), 8: (s5, 9), 20: (s5, 9)}
    centre = {1: (1.0, 5), 4: (1.0, 5), 5: (s2, 9), 8: (s2, 9), 9: (s2, 9)}
    for node, table in ((0, corner), (1, edge), (4, centre)):
        for k, (radius, members) in table.items():
            r = nr.radii(d, k, False)
            assert nr.bits(r[node])[0] == nr.bits(radius)[0], (node, k)
            assert nr.membership(d, r, False)[node].sum() == members, (node, k)
    a = nr.membership(d, nr.radii(d, 3, False), False)
    assert a[0, 4] == 1 and a[4, 0] == 0                               # the centre is the corner's third nearest, not the reverse


def test_square_root_tie_takes_both_nodes():
    from scipy.spatial.distance import pdist
    xy = nr.TIE_XY
    dx, dy = xy[2] - xy[0]
    assert dx * dx + dy * dy == 1.0 + 2.0 ** -52 and np.nextafter(1.0, 2.0) == 1.0 + 2.0 ** -52
    v = pdist(xy)
    assert nr.bits(v[0])[0] == nr.bits(v[1])[0] == nr.bits(1.0)[0]      # pairs (0, 1) and (0, 2)
    d = nr.euclid(xy)
    r = nr.radii(d, 1, False)
    assert r[0] == 1.0
    assert np.array_equal(nr.membership(d, r, False)[0], [1, 1, 1, 0, 0])


def test_a_coincident_node_is_a_neighbour_and_the_node_itself_is_not():
    xy = np.array([(0.0, 0.0), (0.0, 0.0), (3.0, 4.0)])
    d = nr.euclid(xy)
    assert np.array_equal(nr.radii(d, 1, False), [0.0, 0.0, 5.0])
    assert np.array_equal(nr.radii(d, 2, False), [5.0, 5.0, 5.0])
    assert np.array_equal(nr.membership(d, nr.radii(d, 1, False), False), [[1, 1, 0], [1, 1, 0], [1, 1, 1]])
    assert np.array_equal(nr.radii(np.zeros((1, 1)), 4, False), [0.0])


# ------------------------------------------------------------------ settings ----

@pytest.mark.parametrize('k', [1, 50, 50.0, np.int64(7), np.float64(3.0)])
def test_validate_config_accepts_nearest_with_a_whole_number(k):
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'nearest', k
    sf.validate_config()
    assert sf.neighborhood_radius_type == 'nearest' and sf.neighborhood_radius == k


@pytest.mark.parametrize('k', [0, 2.5, -3, float('nan'), float('inf'), True, '5', None])
def test_validate_config_refuses_nearest_with_anything_else(k):
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'nearest', k
    with pytest.raises(ValueError) as err:
        sf.validate_config()
    assert 'nearest' in str(err.value)
    assert sf.neighborhood_radius_type == 'diameter' and sf.neighborhood_radius == 0.1
    sf.validate_config()


def test_unknown_type_message_names_the_four_options():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.neighborhood_radius_type = 'radius'
    with pytest.raises(ValueError) as err:
        sf.validate_config()
    assert sf.neighborhood_radius_type == 'diameter'
    assert all(word in str(err.value) for word in ('diameter', 'absolute', 'percentile', 'nearest'))
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'absolute', 2.5       # only 'nearest' asks for a whole number
    sf.validate_config()


def test_ini_with_nearest_loads(tmp_path):
    import safepy_amd
    ini = tmp_path / 'user.ini'
    ini.write_text('[Analysis parameters]\nneighborhoodRadiusType = nearest\nneighborhoodRadius = 50\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert sf.neighborhood_radius_type == 'nearest' and sf.neighborhood_radius == 50
    assert sf.neighborhood_radii is None and sf.neighborhood_radius_resolved is None
    bad = tmp_path / 'bad.ini'
    bad.write_text('[Analysis parameters]\nneighborhoodRadiusType = nearest\nneighborhoodRadius = 0.1\n')
    with pytest.raises(ValueError):
        safepy_amd.SAFE(path_to_ini_file=str(bad), verbose=False)


def test_neighborhood_radii_pickles_and_defaults():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.neighborhood_radii is None
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'nearest', 3
    sf.neighborhood_radii = np.array([0.25, 0.0, 1.5])
    sf.neighborhood_radius_resolved = 0.25
    clone = pickle.loads(pickle.dumps(sf))
    assert np.array_equal(nr.bits(clone.neighborhood_radii), nr.bits(sf.neighborhood_radii))
    assert clone.neighborhood_radius_type == 'nearest' and clone.neighborhood_radius_resolved == 0.25
    state = sf.__getstate__()
    del state['neighborhood_radii']                                    # an object pickled before the attribute existed
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.neighborhood_radii is None and old.neighborhood_radius == 3


# ------------------------------------------------------------------ the C ABI ----

def test_new_entry_points_are_declared_bound_and_exported():
    from safepy_amd import _lib
    with open(os.path.join(ROOT, 'include', 'safe_hip.h')) as f:
        header = f.read()
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert decl is not None and len(decl.group(1).split(',')) == n_args, name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(_lib.lib, name), name
        assert '%s (safepy/safe.py:369-430)' % name in header, name     # each export cites the reference lines it extends
    version = int(re.search(r'#define SAFE_HIP_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == _lib.lib.safe_abi_version()


def test_backend_wrappers_exist_and_check_shapes_before_the_library():
    from safepy_amd import backend as be
    for owner, name in ((be.Context, 'row_distance_select'), (be.Neighborhoods, 'row_distance_select'),
                        (be.Neighborhoods, 'euclidean_rows'), (be.Neighborhoods, 'from_distances_rows')):
        assert callable(getattr(owner, name)), name
    with pytest.raises(ValueError):
        be.Neighborhoods.euclidean_rows(None, np.zeros((4, 2)), np.zeros(3))      # a radii length other than n
    with pytest.raises(ValueError):
        be.Neighborhoods.euclidean_rows(None, np.zeros((4, 3)), np.zeros(4))
