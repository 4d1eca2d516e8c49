"""multiple_testing_scope without a GPU: the NumPy restatements of the column and whole-matrix count forms of safepy_amd/csrc/fdr.hip against
oracle.safe_oracle.fdrcorrection (along axis 0, and on the ravelled matrix) on the GPU tests' own case lists, a hand-worked 3 x 4
example with three different answers, the forms safepy_amd/csrc/fdr_plan.h chooses (built for the host and run as a program:
tests/fdr_plan_driver.py), the setting's validation and pickling, and the new symbols in header, binding and library."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import fdr_cases as fc
import fdr_plan_driver as fp
import fdr_scope_ref as fs
from oracle import safe_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the constants ----

@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    return fp.build(tmp_path_factory.mktemp('fdr_plan'))


def test_the_constants_are_the_ones_in_the_source(plan):
    c, _ = fp.constants(plan)
    assert (c['COL_LDS_BYTES'], c['COL_TILE_MAX'], c['COL_TILE_MIN']) == (fs.COL_LDS_BYTES, fs.COL_TILE_MAX, fs.COL_TILE_MIN) == (128 * 1024, 16, 4)
    assert (c['COL_HIST_MAX_P'], c['ALL_HIST_MAX_P'], c['ALL_BLOCK']) == (fs.COL_HIST_MAX_P, fs.ALL_HIST_MAX_P, fs.ALL_BLOCK) == (4095, 16383, 2048)
    assert (c['TR_TILE'], c['ALL_IPT'], c['COL_BIN_BYTES']) == (fs.TR_TILE, fs.ALL_IPT, 8) and c['ALL_BLOCK'] == c['THREADS'] * c['ALL_IPT']
    assert fs.col_tile(1000) == 16 and fs.col_tile(fs.COL_HIST_MAX_P) == fs.COL_TILE_MIN
    assert fs.col_tile(fs.COL_HIST_MAX_P) * 8 * (fs.COL_HIST_MAX_P + 1) <= fs.COL_LDS_BYTES
    assert 4 * (fs.ALL_HIST_MAX_P + 1) <= 64 * 1024 < 4 * (fs.ALL_HIST_MAX_P + 2)


def test_the_column_forms_are_the_ones_the_header_chooses(plan):
    """The column count form serves exactly P <= COL_HIST_MAX_P, with the tile of fdr_scope_ref.col_tile and its tables inside
    128 KiB; the sort form is the row form of the [m, n] transpose."""
    span = list(range(0, fs.COL_HIST_MAX_P + 300))
    assert fp.exists(plan, [(fp.COLS, P, None) for P in span]) == [1 <= P <= fs.COL_HIST_MAX_P for P in span]
    for P, f in zip(fs.COLS_COUNT_P, fp.forms(plan, [(fp.COLS, 257, 70, P, None) for P in fs.COLS_COUNT_P])):
        if P <= fs.COL_HIST_MAX_P:
            assert f['kind'] == fp.COL_COUNTS and f['tile'] == fs.col_tile(P) >= fs.COL_TILE_MIN, P
            assert f['lds'] == f['tile'] * 8 * (P + 1) <= fs.COL_LDS_BYTES, P
        else:
            assert f['kind'] == fp.COL_SORT and (f['row_kind'], f['ipt']) == (fp.ROW_BLOCK_SORT, fc.ipt_for(257)), P
    m = 70
    cols = fp.forms(plan, [(fp.COLS, n, m, 0, None) for n in fs.COLS_SORT_N])
    rows = fp.forms(plan, [(fp.ROWS, m, n, 0, None) for n in fs.COLS_SORT_N])
    for n, c, r in zip(fs.COLS_SORT_N, cols, rows):
        assert c['kind'] == fp.COL_SORT and (c['row_kind'], c['ipt'], c['batch_rows']) == (r['kind'], r['ipt'], r['batch_rows']), n
        assert c['ipt'] == (fc.ipt_for(n) or 0) and c['row_kind'] == (fp.ROW_BLOCK_SORT if n <= fc.BLOCK_SORT_MAX else fp.ROW_LIBRARY_SORT), n


def test_the_matrix_forms_are_the_ones_the_header_chooses(plan):
    """The whole-matrix count form serves exactly P <= ALL_HIST_MAX_P; the sort form ends below 2^31 items -- refused at
    n m = 2^31 and at n = 2^31 with m = 1 unless the count form serves, allowed at 2^31 - 1."""
    span = [0, 1, 2, 4096, fs.ALL_HIST_MAX_P - 1, fs.ALL_HIST_MAX_P, fs.ALL_HIST_MAX_P + 1, fs.ALL_HIST_MAX_P + 2, 1 << 20]
    assert fp.exists(plan, [(fp.ALL, P, None) for P in span]) == [1 <= P <= fs.ALL_HIST_MAX_P for P in span]
    big = 1 << 31
    cases = [(fp.ALL, 1 << 16, 1 << 15, 0, None), (fp.ALL, big, 1, 0, None), (fp.ALL, 1, big, 0, None), (fp.ALL, 1 << 40, 1 << 40, 0, None),
             (fp.ALL, 1 << 16, 1 << 15, fs.ALL_HIST_MAX_P + 1, None), (fp.ALL, 1 << 16, 1 << 15, 100, 'sort'),
             (fp.ALL, big - 1, 1, 0, None), (fp.ALL, 1, big - 1, 0, None), (fp.ALL, 46341, 46340, 0, None),
             (fp.ALL, 1 << 16, 1 << 15, 100, None), (fp.ALL, big, 1, fs.ALL_HIST_MAX_P, None)]
    kinds = [f['kind'] for f in fp.forms(plan, cases)]
    assert kinds == [fp.UNSUPPORTED] * 6 + [fp.ALL_SORT] * 3 + [fp.ALL_COUNTS] * 2
    assert 46341 * 46340 < big
    f = fp.forms(plan, [(fp.ALL, 255, 257, P, None) for P in fs.ALL_COUNT_P])
    assert [x['kind'] for x in f] == [fp.ALL_COUNTS] * 4 + [fp.ALL_SORT] and [x['lds'] for x in f[:4]] == [4 * (P + 1) for P in fs.ALL_COUNT_P[:4]]


def test_chain_positions_reach_every_kind_of_chunk():
    assert len(fs.all_chain_positions(2049 * 2051)) == 7          # the last workgroup holds three ranks: one chunk
    total = 1000 * 1031
    pos = fs.all_chain_positions(total)
    blocks = -(-total // fs.ALL_BLOCK)
    assert len(pos) == 9
    assert {at // fs.ALL_BLOCK for at in pos.values()} == {0, blocks // 2, blocks - 1}
    assert max(pos.values()) >= total - fs.ALL_IPT and min(pos.values()) < fs.ALL_IPT
    assert fs.all_chain_positions(1) and len(fs.all_chain_positions(257)) == 3          # one workgroup: three chunks
    for shape in fs.ALL_SHAPES[:7]:
        for name in fs.all_sort_names(shape[0] * shape[1]):
            p = fs.all_sort_family(shape, name)
            assert p.shape == shape
            if name.startswith('chain_min'):
                w = fs.want(p, 'all').ravel()
                at = fs.all_chain_positions(p.size)[name]
                order = np.argsort(p.ravel())
                assert np.unique(w[order[:at + 1]]).size == 1 and (np.diff(w[order[at:]]) > 0).all()   # the minimum travels left only


# ---------------------------------------------------------------------------------------- the NumPy restatements ----

@pytest.mark.parametrize('P', fs.COLS_COUNT_P)
def test_column_count_form_restated_equals_the_oracle(P):
    for n in (1, 2, 257):
        for m in fs.cols_count_m(P)[-1:] + (10,):
            names, p = fs.cols_count_matrix(P, n, m)
            got, want = fs.counts_cols(p, P), fs.want(p, 'neighborhoods')
            assert fc.same(got, want), (P, n, m, fc.failing(names, got.T, want.T))
            if n >= 3:                                           # a column with a NaN becomes NaN, its neighbours stay numbers
                nan_cols = np.array(['nan' in name for name in names])
                assert np.isnan(want[:, nan_cols]).all() and not np.isnan(want[:, ~nan_cols]).any() and nan_cols.any()


@pytest.mark.parametrize('P', fs.ALL_COUNT_P)
def test_matrix_count_form_restated_equals_the_oracle(P):
    for shape in fs.ALL_SHAPES[:7]:
        for name in fs.ALL_COUNT_NAMES:
            p = fs.all_count_family(shape, P, name)
            assert fc.same(fs.counts_all(p, P), fs.want(p, 'all')), (P, shape, name)
    names, p = fs.cols_count_matrix(P, 257, 10)                  # the column cases as one family: NaN everywhere
    assert np.isnan(fs.want(p, 'all')).all() and np.isnan(fs.counts_all(p, P)).all()
    q = np.stack([row for name, row in zip(*fc.count_matrix(P, 300, 0)) if 'nan' not in name])
    assert fc.same(fs.counts_all(q, P), fs.want(q, 'all'))


def test_heavy_ties_zeros_and_one_value():
    for p, P in ((np.zeros((7, 5)), 10), (np.ones((7, 5)), 10), (np.full((7, 5), 0.3), 10),
                 (np.random.default_rng(3).integers(0, 2, size=(50, 9)) / 1.0, 1)):
        assert fc.same(fs.counts_cols(p, P), fs.want(p, 'neighborhoods'))
        assert fc.same(fs.counts_all(p, P), fs.want(p, 'all'))


# --------------------------------------------------------------------------------------------------- by hand ----

def test_hand_worked_example_has_three_answers():
    p = fs.HAND_P
    for scope, hand in (('attributes', fs.HAND_ROWS), ('neighborhoods', fs.HAND_COLS), ('all', fs.HAND_ALL)):
        np.testing.assert_allclose(fs.want(p, scope), hand, rtol=1e-14, atol=0)
    assert fc.same(fs.want(p, 'neighborhoods'), np.stack([orc.fdrcorrection(p[:, j]) for j in range(4)], axis=1))
    assert fc.same(fs.want(p, 'all'), orc.fdrcorrection(p.ravel()).reshape(3, 4))
    a, b, c = (fs.want(p, s) for s in ('attributes', 'neighborhoods', 'all'))
    assert not np.allclose(a, b) and not np.allclose(a, c) and not np.allclose(b, c)
    assert [(x < 0.05).sum() for x in (a, b, c)] == [4, 3, 0]     # the three scopes call different cells significant


# -------------------------------------------------------------------------------------- the setting of the class ----

def fresh():
    import safepy_amd
    return safepy_amd.SAFE(verbose=False)


@pytest.mark.parametrize('value', ['attributes', 'neighborhoods', 'all'])
def test_validate_config_accepts_the_three_scopes(value):
    sf = fresh()
    assert sf.multiple_testing_scope == 'attributes'
    sf.multiple_testing_scope = value
    sf.validate_config()
    assert sf.multiple_testing_scope == value


@pytest.mark.parametrize('value', ['rows', None, 1, ['all']])
def test_validate_config_refuses_anything_else_and_restores_the_default(value):
    sf = fresh()
    sf.multiple_testing_scope = value
    with pytest.raises(ValueError, match='multiple_testing_scope'):
        sf.validate_config()
    assert sf.multiple_testing_scope == 'attributes'
    sf.validate_config()


def test_compute_pvalues_refuses_a_bad_scope_before_any_device_work():
    sf = fresh()
    with pytest.raises(ValueError, match='multiple_testing_scope'):
        sf.compute_pvalues(multiple_testing=True, multiple_testing_scope='rows')
    assert sf.multiple_testing_scope == 'attributes'


def test_pickle_round_trip_keeps_the_setting(tmp_path):
    sf = fresh()
    sf.multiple_testing_scope = 'all'
    back = pickle.loads(pickle.dumps(sf))
    assert back.multiple_testing_scope == 'all'
    sf.multiple_testing_scope = 'neighborhoods'
    sf.save(output_file=str(tmp_path / 'safe.p'))
    with open(str(tmp_path / 'safe.p'), 'rb') as f:
        assert pickle.load(f).multiple_testing_scope == 'neighborhoods'


def test_an_object_pickled_before_the_setting_existed_gets_the_default():
    sf = fresh()
    state = sf.__getstate__()
    del state['multiple_testing_scope']
    old = type(sf).__new__(type(sf))
    old.__setstate__(state)
    assert old.multiple_testing_scope == 'attributes'
    old.validate_config()


# ------------------------------------------------------------------------------------------------------ symbols ----

def test_the_new_symbols_are_in_header_binding_and_library():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    for name, value in (('SAFE_FDR_SCOPE_ROWS', 0), ('SAFE_FDR_SCOPE_COLS', 1), ('SAFE_FDR_SCOPE_ALL', 2)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
        assert getattr(_lib, name[len('SAFE_'):]) == value
    assert backend.FDR_SCOPES == fs.SCOPES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, n_args in (('safe_fdr_adjust_scope', 12), ('safe_fdr_adjust_matrix', 6)):
        assert re.search(r'\bint %s\s*\(' % name, code), name
        assert len(_lib.PROTOTYPES[name][1]) == n_args and hasattr(raw, name)
        assert name in header[:header.index('#ifndef SAFE_HIP_H')]              # the list of calls that wait for the stream
    assert callable(backend.fdr_adjust_scope) and callable(backend.fdr_adjust_matrix)
