"""neighborhood_radius_type without a device: the rank arithmetic and interpolation behind 'percentile' against np.percentile
on the bits, and validate_config's handling of the setting."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

import radius_ref as rr


def _same(got, want):
    return rr.bits(got)[0] == rr.bits(want)[0]


@pytest.mark.parametrize('scale', [1.0, 37.5, 1e-3])
@pytest.mark.parametrize('n', [2, 3, 4, 5, 17, 64, 65, 129, 300, 1000])
def test_rank_function_and_lerp_reproduce_np_percentile(n, scale):
    from safepy_amd import safe as S
    v = pdist(np.random.default_rng(n).uniform(size=(n, 2)) * scale)
    sv = np.sort(v)
    for q in rr.QS:
        assert _same(rr.percentile_by_ranks(sv, q, S._percentile_ranks, S._lerp), np.percentile(v, q)), (n, scale, q)


def test_rank_function_with_coincident_nodes_and_hop_counts():
    from safepy_amd import safe as S
    rng = np.random.default_rng(7)
    xy = rng.uniform(size=(40, 2))
    xy[10:20] = xy[3]                                                   # ten coincident nodes: 55 zero distances and many ties
    hops = rng.integers(1, 9, size=5000).astype(np.float64)             # integer-valued v: the 'shortpath' metric
    for v in (pdist(xy), hops, np.array([3.0]), np.zeros(6)):
        sv = np.sort(v)
        for q in rr.QS:
            assert _same(rr.percentile_by_ranks(sv, q, S._percentile_ranks, S._lerp), np.percentile(v, q)), (v.shape, q)


def test_rank_function_limits():
    from safepy_amd import safe as S
    assert S._percentile_ranks(10, 0)[:2] == (0, 1) and S._percentile_ranks(10, 0)[2] == 0.0
    assert S._percentile_ranks(10, 100)[:2] == (9, 9)
    assert S._percentile_ranks(1, 50)[:2] == (0, 0)
    k, k1, _ = S._percentile_ranks(2147450880, 99.9)                    # 65 536 nodes: ranks beyond f32 / int32 habits stay exact
    assert k1 == k + 1 and k == 2145303428
    with pytest.raises(ValueError):
        S._percentile_ranks(0, 50)
    ranks, use = S._percentile_plan(11, [50, 0, 100, 55])
    assert ranks == [0, 1, 5, 6, 10] and [u[:2] for u in use] == [(2, 3), (0, 1), (4, 4), (2, 3)]


def test_validate_config_accepts_the_three_types_and_none():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    for kind in (None, 'diameter', 'absolute', 'percentile'):
        sf.neighborhood_radius_type = kind
        sf.validate_config()
        assert sf.neighborhood_radius_type == kind


def test_validate_config_rejects_other_types_and_bad_percentiles():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.neighborhood_radius_type = 'radius'
    with pytest.raises(ValueError) as err:
        sf.validate_config()
    assert sf.neighborhood_radius_type == 'diameter'
    assert all(word in str(err.value) for word in ('diameter', 'absolute', 'percentile'))
    for q in (-1, 100.5):
        sf.neighborhood_radius_type, sf.neighborhood_radius = 'percentile', q
        with pytest.raises(ValueError):
            sf.validate_config()
        assert sf.neighborhood_radius_type == 'diameter' and sf.neighborhood_radius == 0.1
    sf.neighborhood_radius_type, sf.neighborhood_radius = 'absolute', 100.5       # only a percentile is bounded
    sf.validate_config()
    for q in (0, 100, 2.5):
        sf.neighborhood_radius_type, sf.neighborhood_radius = 'percentile', q
        sf.validate_config()


def test_ini_with_a_percentile_radius_loads(tmp_path):
    import safepy_amd
    ini = tmp_path / 'user.ini'
    ini.write_text('[Analysis parameters]\nneighborhoodRadiusType = percentile\nneighborhoodRadius = 2.5\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert sf.neighborhood_radius_type == 'percentile' and sf.neighborhood_radius == 2.5
    assert sf.neighborhood_radius_resolved is None
    bad = tmp_path / 'bad.ini'
    bad.write_text('[Analysis parameters]\nneighborhoodRadiusType = radius\n')
    with pytest.raises(ValueError):
        safepy_amd.SAFE(path_to_ini_file=str(bad), verbose=False)


def test_new_entry_points_are_declared_and_bound():
    from safepy_amd import _lib
    assert len(_lib.PROTOTYPES['safe_pair_distance_select_xy'][1]) == 7
    assert len(_lib.PROTOTYPES['safe_nbr_distance_select'][1]) == 5
    assert hasattr(_lib.lib, 'safe_pair_distance_select_xy') and hasattr(_lib.lib, 'safe_nbr_distance_select')
