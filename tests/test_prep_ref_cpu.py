"""Self-tests of tests/prep_ref.py: the references have known answers on hand-written inputs, the launch arithmetic is pinned,
every builder produces its designed rows and columns at every listed shape, and the two host-side claims the GPU tests lean
on hold -- SciPy's pdist is the separately rounded sqrt(dx*dx + dy*dy) on every point set, and the squared-threshold rule
equals sqrt(s) < nr for every radius of the edge test.  No device."""
import os
import re

import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform

import prep_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.nan, np.inf


# ------------------------------------------------------------------------------------------------ 1. attribute facts ----

def test_attr_facts_on_hand_written_matrices():
    b = np.array([[NAN, NAN, NAN],
                  [0.0, 1.0, NAN],
                  [-0.0, 2.0, 0.5],
                  [INF, -INF, NAN],
                  [1e30, -1.0, 1.0]])
    f = pr.attr_facts(b)
    assert f['n_other'] == 6                                            # 2, 0.5, inf, -inf, 1e30, -1 -- and not -0.0
    assert f['n_non_integer'] == 1                                      # 0.5 alone: +-inf and 1e30 are integers
    assert f['max_nan_col'] == 3                                        # the last column
    assert f['row_flags'].tolist() == [0, 1, 1, 1, 1] and f['row_flags'].dtype == np.uint8
    assert f['n_rows_with_value'] == 4
    assert f['value_counts'] == (5, 2, 6, 2)                            # NaN, zeros (-0.0 is one), positives, negatives
    assert sum(f['value_counts']) == b.size
    assert f['col_sum'][2] == 1.5 and f['col_sum'][0] == INF and f['col_sum'][1] == -INF

    binary = np.array([[1, 0], [NAN, 1], [1, NAN], [NAN, NAN]], dtype=np.float32)
    f = pr.attr_facts(binary)
    assert (f['n_other'], f['n_non_integer'], f['max_nan_col'], f['n_rows_with_value']) == (0, 0, 2, 3)
    assert f['col_sum'].tolist() == [2.0, 1.0] and f['col_sum'].dtype == np.float64
    assert f['value_counts'] == (4, 1, 3, 0)

    f = pr.attr_facts(np.array([[True, False], [False, False]]))        # the byte form: no NaN
    assert f['row_flags'].tolist() == [1, 1] and f['max_nan_col'] == 0 and f['value_counts'] == (0, 3, 1, 0)
    f = pr.attr_facts(np.full((3, 2), NAN))
    assert f['max_nan_col'] == 3 and f['n_rows_with_value'] == 0 and f['col_sum'].tolist() == [0.0, 0.0]


@pytest.mark.parametrize('n,m', pr.F_SHAPES + pr.C_SHAPES)
def test_attr_input_has_its_designed_rows_and_columns(n, m):
    for dtype in (np.float32, np.float64):
        for flavour in ('binary', 'mixed'):
            b = pr.attr_input(n, m, dtype, flavour, seed=1)
            assert b.shape == (n, m) and b.dtype == dtype and b.flags.c_contiguous
            nan = np.isnan(b)
            nan_rows, only_last, only_first = pr.attr_design(n, m)
            assert set(nan_rows) == {r for r in (0, 31, 32, 63, 64, n - 1) if r < n}
            assert nan[nan_rows].all()
            if only_last is not None:
                assert not nan[only_last, m - 1] and nan[only_last, :m - 1].all()
            if only_first is not None:
                assert not nan[only_first, 0] and nan[only_first, 1:].all() and only_first != only_last
            assert (only_last is None) == (n <= 2) and (only_first is None) == (n <= 3 or m == 1)
            counts = nan.sum(axis=0)
            if m > 1 and n >= 16:
                assert counts[m - 1] > counts[:m - 1].max()             # strictly the largest wherever rows are left
            values = b[~nan]
            if flavour == 'binary':
                assert np.isin(values, (0.0, 1.0)).all()
            elif n * m >= 1000:
                assert set(np.unique(values).tolist()) == set(np.float64(dtype(v)) for v in pr.MIXED_VALUES)
                assert np.signbit(values[values == 0]).any()            # -0.0 is there
            full = pr.attr_input(n, m, dtype, flavour, seed=1, nan_column=True)
            assert np.isnan(full[:, m - 1]).all() and pr.attr_facts(full)['max_nan_col'] == n
            assert np.array_equal(np.isnan(full[:, :m - 1]), nan[:, :m - 1])


def test_attr_input_at_one_row_and_in_byte_form():
    assert np.isnan(pr.attr_input(1, 1, np.float64, 'binary', 0)).all()         # row 0 is row n - 1: all NaN
    assert np.isnan(pr.attr_input(1, 3, np.float32, 'mixed', 0)).all()
    assert not np.isnan(pr.attr_input(1, 3, np.float32, 'mixed', 0, designed=False)).all()
    for n, m in pr.U8_SHAPES:
        for dtype in (np.uint8, np.bool_):
            b = pr.attr_input(n, m, dtype, 'binary', 0)
            assert b.dtype == dtype and b.shape == (n, m) and np.isin(b.astype(np.int64), (0, 1)).all()
    assert sorted({n * m for n, m in pr.U8_SHAPES}) == sorted(set(pr.U8_COUNTS))
    assert set(pr.U8_COUNTS) >= {1, 15, 16, 17, 4095, 4096, 4097}


def test_large_row_counts_stay_small_and_sit_on_the_lds_edges():
    for n in pr.LARGE_ROWS:
        for m, _ in pr.LARGE_LAYOUTS:
            assert n * m * 4 <= 10_000_000
    assert -(-262144 // 32) * 4 == 32 * 1024                            # the last size on the static limit ...
    assert -(-262209 // 32) * 4 > 32 * 1024                             # ... and the first trips past it
    assert -(-pr.ROW_LIMIT // 32) * 4 == 150 * 1024 and -(-(pr.ROW_LIMIT + 1) // 32) * 4 > 150 * 1024
    b = pr.attr_input(pr.ROW_LIMIT, 2, np.float32, 'binary', 0)
    f = pr.attr_facts(b)
    assert f['row_flags'][[0, 31, 32, 63, 64, pr.ROW_LIMIT - 1]].sum() == 0 and f['row_flags'][[1, 2, 65]].all()
    assert np.isnan(b).sum(axis=0).argmax() == 1


# ------------------------------------------------------------------------------- 2. the fused dense Euclidean kernel ----

def test_dense_geometry_is_pinned_at_256_compute_units():
    assert pr.dense_geometry(1793, 256) == (4, 256, True)
    assert pr.dense_geometry(1792, 256) == (4, 256, False)
    assert pr.dense_geometry(2049, 256) == (5, 204, True)
    assert pr.dense_geometry(1, 256) == (1, 1, False) and pr.dense_geometry(513, 256) == (2, 512, False)
    assert pr.first_batched_n(256) == 1793
    assert not any(pr.dense_geometry(n, 256)[2] for n in (257, 300, 301, 513, 1000, 1001))   # the sizes tested before
    nb, sizes = pr.dense_sizes(256)
    assert nb == 1793 and tuple(sizes) == pr.DENSE_SLOTS
    sizes = list(sizes.values())
    assert sizes == [1, 2, 3, 511, 512, 513, 1024, 1025, 1792, 1793, 1794, 2049, 2050]
    assert any(pr.dense_geometry(n, 256)[2] for n in sizes) and any(pr.last_lane_has_one_column(n) for n in sizes)
    assert {n % 2 for n in sizes if pr.dense_geometry(n, 256)[2]} == {0, 1}              # whole batches in VEC and scalar form
    for cus in (64, 104, 120, 228, 304):                                # other devices: the rule still finds its sizes
        nb, sizes = pr.dense_sizes(cus)
        assert pr.dense_geometry(nb, cus)[2] and not pr.dense_geometry(nb - 1, cus)[2]
        assert pr.dense_geometry(sizes['next_chunk_odd'], cus)[0] == pr.dense_geometry(nb + 1, cus)[0] + 1
        assert sizes['next_chunk_odd'] % 2 == 1 and pr.dense_geometry(sizes['next_chunk_odd'] - 1, cus)[0] == pr.dense_geometry(nb + 1, cus)[0]


@pytest.mark.parametrize('kind', pr.XY_KINDS)
@pytest.mark.parametrize('n', [1, 2, 3, 11, 300, 513])
def test_xy_input_and_pdist_is_the_separately_rounded_root(kind, n):
    xy = pr.xy_input(kind, n)
    assert xy.shape == (n, 2) and xy.dtype == np.float64 and np.isfinite(xy).all()
    d = squareform(pdist(xy)) if n > 1 else np.zeros((1, 1))
    assert np.array_equal(pr.bits(d), pr.bits(pr.separately_rounded_distances(xy)))
    nr = pr.XY_RADIUS[kind]
    if n > 10:
        assert d[0, 1] == 0.0 and d[2, 3] == nr                         # coincident pair; a pair exactly on the threshold
        assert not (d[2, 3] < nr)
        member = d < nr
        assert member[0, 1] and not member[2, 3]
        if kind == 'huge':
            off = d[~np.eye(n, dtype=bool)]
            assert np.isinf(off).sum() >= off.size - 4 * n              # (the four designed nodes aside)
        if kind == 'tiny':
            s = d[d > 0] ** 2
            assert s.max() < 2.3e-308                                   # every square is subnormal
        if kind == 'lattice' and n >= 300:
            assert np.unique(d).size < d.size // 20                     # many exact ties
    assert np.array_equal(xy, pr.xy_input(kind, n))                     # a builder, not a generator: same call, same points


@pytest.mark.parametrize('kind', ['uniform', 'tiny', 'huge'])
def test_squared_threshold_rule_equals_the_rooted_comparison(kind):
    """s < T  <=>  sqrt(s) < nr, on every squared distance of the point set and on the doubles around T."""
    xy = pr.xy_input(kind, 300)
    x, y = xy[:, 0], xy[:, 1]
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    with np.errstate(over='ignore', under='ignore'):
        s_all = np.unique(dx * dx + dy * dy)
    assert np.array_equal(pr.bits(pr.separately_rounded_distances(xy)), pr.bits(squareform(pdist(xy))))
    for nr in pr.radius_edges(xy) + (pr.XY_RADIUS[kind],):
        t = pr.squared_threshold(nr)
        around = [t]
        for _ in range(3):
            around = [np.nextafter(around[0], 0.0)] + around + [np.nextafter(around[-1], np.inf)]
        s = np.concatenate([s_all, np.array([v for v in around if v >= 0.0])])
        assert np.array_equal(s < t, np.sqrt(s) < nr), (kind, nr, t)
    assert pr.squared_threshold(5e-324) == 5e-324 and pr.squared_threshold(1e-200) == 5e-324   # only s == 0 is below
    assert pr.squared_threshold(0.0) == 0.0 and pr.squared_threshold(-1.0) == 0.0 and pr.squared_threshold(NAN) == 0.0
    assert pr.squared_threshold(INF) == INF and pr.squared_threshold(1e200) == INF
    assert pr.squared_threshold(2.0 ** -530) == 2.0 ** -1060            # a subnormal threshold, exact


def test_edge_input():
    for n_edges in (0, 1, 255, 256, 257):
        eu, ev = pr.edge_input(300, n_edges)
        assert eu.shape == ev.shape == (n_edges,) and eu.dtype == ev.dtype == np.int32
        assert n_edges == 0 or (eu.min() >= 0 and max(eu.max(), ev.max()) < 300)
        if n_edges >= 1:
            assert eu[0] == ev[0]                                       # a self edge
        if n_edges >= 3:
            assert (eu[-1], ev[-1]) == (eu[1], ev[1])                   # a repeated edge


# ------------------------------------------------------------------------------------------------ 3. membership forms ----

@pytest.mark.parametrize('n', pr.MEMBERSHIP_SIZES)
def test_membership_has_its_designed_rows(n):
    a = pr.membership(n)
    assert a.shape == (n, n) and a.dtype == np.int64 and np.isin(a, (0, 1)).all()
    rows = pr.membership_design(n)
    assert a[rows['full']].all()
    assert ('empty' in rows) == (n >= 2) and ('only_last' in rows) == (n >= 3)
    assert ('beyond_group' in rows) == ('straddle' in rows) == (n > 4096)
    if 'empty' in rows:
        assert not a[rows['empty']].any()
    if 'only_last' in rows:
        assert np.nonzero(a[rows['only_last']])[0].tolist() == [n - 1]
    if n > 4096:
        cols = np.nonzero(a[rows['beyond_group']])[0]
        assert cols.min() == 4096 and cols.max() == n - 1
        assert np.nonzero(a[rows['straddle']])[0].tolist() == [4095, 4096]
    if n >= 4095:
        density = a[8:].mean()
        assert 0.008 < density < 0.012                                  # about 1 %
    row_ptr, col = pr.csr_of(a)
    assert row_ptr[-1] == a.sum() == col.size and row_ptr.dtype == col.dtype == np.int32
    for i in sorted(set(rows.values()) | {n - 1}):
        assert np.array_equal(col[row_ptr[i]:row_ptr[i + 1]], np.nonzero(a[i])[0])


# ----------------------------------------------------------------------------------------------------- 4. the accessor ----

def test_column_sums_is_declared_and_bound():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    assert re.search(r'\bint safe_attr_column_sums\(safe_attr \*attr, double \*out_host\);', header)
    res, args = _lib.PROTOTYPES['safe_attr_column_sums']
    assert len(args) == 2
    assert hasattr(_lib.lib, 'safe_attr_column_sums') and hasattr(backend.Attributes, 'column_sums')
    assert _lib.lib.safe_attr_column_sums(None, None) == _lib.E_INVALID           # refuses NULL before it touches a device
    assert b'NULL argument' in _lib.lib.safe_last_error()
