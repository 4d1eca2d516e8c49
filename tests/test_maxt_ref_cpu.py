"""familywise_adjustment = 'maxT' without a GPU: the NumPy restatement of the contract (tests/maxt_ref.py) against an enumeration
of all permutations, a hand-worked lattice, the degenerate cells, the monotonicity of the adjustment and the null example of
the design; and the settings, INI keys, pickling, refusals and symbols of the feature."""
import ctypes
import itertools
import os
import pickle
import re

import numpy as np
import pytest

import maxt_ref as mx
import weights_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_case(a, b, tables, w=None):
    indptr, indices = wr.csr_of(a)
    flags = (~np.isnan(b)).any(axis=1)
    n_v = int(flags.sum())
    loc, scale = mx.row_factors(indptr, indices, flags, n_v, w)
    mu, q = mx.column_moments(b, flags)
    return mx.extremes(indptr, indices, w, b, tables, loc, scale, mu, q)


@pytest.mark.parametrize('n_v,seed', [(4, 0), (5, 1), (6, 2)])
def test_enumeration_of_all_permutations(n_v, seed):
    """With all n_v! permutations the adjusted p-value of the cell that holds the family maximum is the exact share of
    permutations whose maximum reaches it -- computed here a second time, cell by cell in plain Python."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n_v, n_v)) < 0.5
    a[np.arange(n_v), np.arange(n_v)] = True
    a[0] = [True] * (n_v - 1) + [False]                                     # (no row holds the whole population by accident)
    b = np.round(rng.normal(size=(n_v, 2)), 2)
    tables = np.array(list(itertools.permutations(range(n_v))))
    z_obs, live, tmax, tmin, _ = _flat_case(a, b, tables)
    neg, pos, least_neg, least_pos = mx.counts(z_obs, live, tmax, tmin, mx.COLUMN)
    for j in range(2):
        vals = b[:, j].tolist()
        mu = sum(vals) / n_v
        q = sum((v - mu) ** 2 for v in vals)
        rows = []
        for i in range(n_v):
            members = [k for k in range(n_v) if a[i, k]]
            f = len(members) * (n_v - len(members)) / (n_v * (n_v - 1.0))
            if f > 0:
                rows.append((i, members, len(members) * mu, (f * q) ** 0.5))

        def family_max(t):
            return max((sum(vals[t[k]] for k in members) - c) / sd for _, members, c, sd in rows)

        top = family_max(list(range(n_v)))
        reached = sum(family_max(t) >= top - 1e-12 for t in tables.tolist())
        i_top = int(np.argmax(np.where(live[:, j], z_obs[:, j], -np.inf)))
        assert abs(z_obs[i_top, j] - top) < 1e-12
        assert pos[i_top, j] == reached and least_pos[j] == reached
        assert pos[i_top, j] / len(tables) == reached / len(tables)


def test_three_by_three_lattice_by_hand():
    """3 x 3 lattice, members within distance 1 (corners 3, edges 4, the centre 5 members), one column with a single 1 at corner
    node 0; n_v = 9, mu = 1/9, Q = 8/9, f = 1/4 (corners) and 5/18 (edges, centre).  A neighborhood scores 1 where it holds the
    1: z = sqrt(2) (corner), 5/sqrt(20) (edge), 4/sqrt(20) (centre), else -1/sqrt(2), -4/sqrt(20), -5/sqrt(20).  Nine tables move
    the 1 to each node r: the maximum is sqrt(2) unless r is the centre (5/sqrt(20)); the minimum is -5/sqrt(20) for a corner,
    -4/sqrt(20) for an edge, -1/sqrt(2) for the centre."""
    _, a = mx.lattice(3, 1.0)
    assert a.sum(axis=1).tolist() == [3, 4, 3, 4, 5, 4, 3, 4, 3]
    b = np.zeros((9, 1))
    b[0, 0] = 1.0
    tables = np.tile(np.arange(9), (9, 1))
    for r in range(9):
        tables[r, r], tables[r, 0] = 0, r
    z_obs, live, tmax, tmin, _ = _flat_case(a, b, tables)
    s2, s20 = np.sqrt(2.0), np.sqrt(20.0)
    np.testing.assert_allclose(z_obs[:, 0], [s2, 5 / s20, -1 / s2, 5 / s20, -5 / s20, -4 / s20, -1 / s2, -4 / s20, -1 / s2], rtol=1e-14)
    assert live.all()
    np.testing.assert_allclose(tmax[:, 0], [s2, s2, s2, s2, 5 / s20, s2, s2, s2, s2], rtol=1e-14)
    np.testing.assert_allclose(tmin[:, 0], [-5 / s20, -4 / s20, -5 / s20, -4 / s20, -1 / s2, -4 / s20, -5 / s20, -4 / s20, -5 / s20], rtol=1e-14)
    for scope in (mx.COLUMN, mx.MATRIX):                                      # one column: the two families coincide
        neg, pos, least_neg, least_pos = mx.counts(z_obs, live, tmax, tmin, scope)
        assert pos[:, 0].tolist() == [8, 9, 9, 9, 9, 9, 9, 9, 9]
        assert neg[:, 0].tolist() == [9, 9, 9, 9, 4, 8, 9, 8, 9]
        assert least_pos.tolist() == [8] and least_neg.tolist() == [4]


def test_degenerate_cells_leave_the_extremes_and_get_p_one():
    rng = np.random.default_rng(3)
    n = 12
    a = rng.uniform(size=(n, n)) < 0.4
    a[np.arange(n), np.arange(n)] = True
    b = np.round(rng.normal(size=(n, 4)), 2)
    b[10:] = np.nan                                                           # rows 10, 11 hold no value: n_v = 10
    a[0] = False                                                              # k_0 = 0 ...
    a[0, 11] = True                                                           # ... its only member holds no value
    a[1] = True                                                               # k_1 = n_v
    b[:10, 2] = 7.0                                                           # a constant column
    flags = (~np.isnan(b)).any(axis=1)
    tables = mx.random_tables(n, flags, 40, rng)
    z_obs, live, tmax, tmin, z_all = _flat_case(a, b, tables)
    assert not live[0].any() and not live[1].any() and not live[:, 2].any() and live[2:, [0, 1, 3]].all()
    assert (z_obs[~live] == 0).all()
    assert np.isneginf(tmax[:, 2]).all() and np.isposinf(tmin[:, 2]).all()
    np.testing.assert_array_equal(tmax[:, [0, 1, 3]], z_all[:, 2:][:, :, [0, 1, 3]].max(axis=1))
    for scope in (mx.COLUMN, mx.MATRIX):
        neg, pos, least_neg, least_pos = mx.counts(z_obs, live, tmax, tmin, scope)
        assert (neg[~live] == 40).all() and (pos[~live] == 40).all()
        assert least_neg[2] == 40 and least_pos[2] == 40
    # the whole population at one weight: W1 mu is every permuted score
    indptr, indices = wr.csr_of(a)
    w = wr.designed_weights(indptr, indices)
    w[indptr[1]:indptr[2]] = 0.375
    loc, scale = mx.row_factors(indptr, indices, flags, 10, w)
    assert scale[0] == 0 and scale[1] == 0 and (scale[2:] > 0).all()
    mu, q = mx.column_moments(b, flags)
    z_w, live_w, tmax_w, _, z_all_w = mx.extremes(indptr, indices, w, b, tables, loc, scale, mu, q)
    assert not live_w[:2].any() and (z_w[:2] == 0).all()
    np.testing.assert_array_equal(tmax_w[:, 0], z_all_w[:, 2:, 0].max(axis=1))


def test_adjusted_counts_dominate():
    """adjusted >= raw in every cell, and the whole-matrix family >= the column family."""
    a, b, indptr, indices, w = wr.order_sensitive(40, 6, 11)
    flags = np.ones(40, dtype=bool)
    tables = mx.random_tables(40, flags, 60, np.random.default_rng(4))
    for weights in (None, w):
        z_obs, live, tmax, tmin, z_all = _flat_case(a, b, tables, weights)
        raw_neg, raw_pos = mx.raw_counts(z_obs, z_all)
        col = mx.counts(z_obs, live, tmax, tmin, mx.COLUMN)
        mat = mx.counts(z_obs, live, tmax, tmin, mx.MATRIX)
        assert (col[0] >= raw_neg).all() and (col[1] >= raw_pos).all()
        assert (mat[0] >= col[0]).all() and (mat[1] >= col[1]).all()
        assert (mat[2] >= col[2]).all() and (mat[3] >= col[3]).all()
        assert (col[1] > raw_pos).any() and (mat[1] > col[1]).any()


def test_null_example_keeps_its_family_wise_error_rate():
    """18 x 18 lattice, 13-member discs, 400 standard-normal columns, +1.5 planted on the radius-3 disc around node 40 of column
    0, P = 200.  At most 0.05 * 399 + 5 sigma = 41 null columns may have a smallest adjusted p-value <= 0.05 (sigma =
    sqrt(399 * 0.05 * 0.95) = 4.35); the raw p-values must flag at least 390 of them; the planted column must be found."""
    P = 200
    xy, a, b, planted = mx.planted_lattice()
    assert a.sum(axis=1).max() == 13
    flags = np.ones(len(a), dtype=bool)
    tables = mx.random_tables(len(a), flags, P, np.random.default_rng(5))
    z_obs, live, tmax, tmin, z_all = _flat_case(a, b, tables)
    neg, pos, least_neg, least_pos = mx.counts(z_obs, live, tmax, tmin, mx.COLUMN)
    _, raw_pos = mx.raw_counts(z_obs, z_all)
    adjusted_null = int(np.count_nonzero(least_pos[1:] / P <= 0.05))
    raw_null = int(np.count_nonzero(raw_pos[:, 1:].min(axis=0) / P <= 0.05))
    found = int(np.count_nonzero(pos[planted, 0] / P <= 0.05))
    print('null columns flagged: adjusted %d, raw %d of 399; planted cells found %d of %d, smallest adjusted p %.3f'
          % (adjusted_null, raw_null, found, len(planted), least_pos[0] / P))
    assert adjusted_null <= 41
    assert raw_null >= 390
    assert least_pos[0] / P <= 0.05
    assert (pos >= raw_pos).all()


def test_settings_ini_and_pickle(tmp_path):
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.familywise_adjustment == 'none' and sf.familywise_scope == 'neighborhoods' and sf.familywise_statistic is None
    for bad in ('maxt', 'bonferroni', 1, None, ['maxT']):
        sf.familywise_adjustment = bad
        with pytest.raises(ValueError, match='familywise_adjustment'):
            sf.validate_config()
        assert sf.familywise_adjustment == 'none'                             # restored
    for bad in ('attributes', 'rows', 0, None):
        sf.familywise_scope = bad
        with pytest.raises(ValueError, match='familywise_scope'):
            sf.validate_config()
        assert sf.familywise_scope == 'neighborhoods'
    sf.familywise_adjustment, sf.familywise_scope = 'maxT', 'all'
    sf.validate_config()

    ini = tmp_path / 'maxt.ini'
    ini.write_text('[Analysis parameters]\nfamilywiseAdjustment = maxT\nfamilywiseScope = all\n')
    got = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert got.familywise_adjustment == 'maxT' and got.familywise_scope == 'all'
    ini.write_text('[Analysis parameters]\nfamilywiseAdjustment =\nfamilywiseScope =\n')
    got = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert got.familywise_adjustment == 'none' and got.familywise_scope == 'neighborhoods'
    for text, name in (('familywiseAdjustment = holm\n', 'familywise_adjustment'), ('familywiseScope = nodes\n', 'familywise_scope')):
        ini.write_text('[Analysis parameters]\n' + text)
        with pytest.raises(ValueError, match=name):
            safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)

    sf.familywise_statistic = np.arange(6.0).reshape(3, 2)
    back = pickle.loads(pickle.dumps(sf))
    assert back.familywise_adjustment == 'maxT' and back.familywise_scope == 'all'
    np.testing.assert_array_equal(back.familywise_statistic, np.arange(6.0).reshape(3, 2))
    state = sf.__getstate__()
    for name in ('familywise_adjustment', 'familywise_scope', '_r_familywise_statistic'):
        del state[name]                                                       # an object pickled before the settings existed
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.familywise_adjustment == 'none' and old.familywise_scope == 'neighborhoods' and old.familywise_statistic is None
    old.validate_config()


def test_refusals_before_any_device_work():
    """how = 'analytic', how = 'hypergeometric', 'z-score' scores and multiple_testing with 'maxT', and bad values of the two
    settings, are refused before a device is touched (this test has none) and leave the results as they were."""
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.node2attribute = np.zeros((5, 2))
    marks = {name: object() for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'familywise_statistic')}
    for name, mark in marks.items():
        setattr(sf, name, mark)
    for kwargs, message in [(dict(how='analytic', familywise_adjustment='maxT'), "how = 'randomization'"),
                            (dict(how='hypergeometric', familywise_adjustment='maxT'), "how = 'randomization'"),
                            (dict(how='randomization', familywise_adjustment='maxT', neighborhood_score_type='z-score'), 'z-score'),
                            (dict(how='randomization', familywise_adjustment='maxT', multiple_testing=True), 'multiple_testing'),
                            (dict(how='randomization', familywise_adjustment='minP'), 'not a valid setting'),
                            (dict(how='randomization', familywise_adjustment='maxT', familywise_scope='attributes'), 'familywise_scope')]:
        with pytest.raises(ValueError, match=message):
            sf.compute_pvalues(**kwargs)
        for name, mark in marks.items():
            assert getattr(sf, name) is mark, (kwargs, name)
        sf.familywise_adjustment, sf.familywise_scope = 'none', 'neighborhoods'
        sf.neighborhood_score_type, sf.multiple_testing, sf.enrichment_type = 'sum', False, 'auto'
    sf.neighborhood_score_type = 'z-score'
    with pytest.raises(ValueError, match='z-score'):                          # the randomization entry point called directly
        sf.compute_pvalues_by_randomization(familywise_adjustment='maxT')
    sf.neighborhood_score_type, sf.multiple_testing = 'sum', True
    with pytest.raises(ValueError, match='multiple_testing'):
        sf.compute_pvalues_by_randomization(familywise_adjustment='maxT')
    assert all(getattr(sf, name) is mark for name, mark in marks.items())


def test_symbols_are_declared_bound_and_exported():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    assert re.search(r'#define SAFE_HIP_ABI_VERSION 9\b', header)             # additive: the version stays
    assert re.search(r'#define SAFE_FAMILY_COLUMN 0\b', header) and re.search(r'#define SAFE_FAMILY_MATRIX 1\b', header)
    assert (_lib.FAMILY_COLUMN, _lib.FAMILY_MATRIX) == (0, 1) == (mx.COLUMN, mx.MATRIX)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, n_args in (('safe_permtest_extremes', 10), ('safe_counts_from_extremes', 13)):
        found = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, code)
        assert found and len(found.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert hasattr(backend, 'permtest_extremes') and hasattr(backend, 'counts_from_extremes')
    assert backend.FAMILY_SCOPES == {'neighborhoods': 0, 'all': 1}
    # NULL arguments are refused before a device is touched
    assert _lib.lib.safe_permtest_extremes(None, None, None, None, 0, 1, None, None, None, None) == _lib.E_INVALID
    assert b'NULL argument' in _lib.lib.safe_last_error()
    assert _lib.lib.safe_counts_from_extremes(None, 1, 1, 1, 0, None, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert b'NULL argument' in _lib.lib.safe_last_error()
