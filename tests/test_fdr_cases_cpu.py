"""tests/fdr_cases.py on the host: the constants it mirrors are still the ones safepy_amd/csrc/fdr_plan.h dispatches on -- asked of
the header itself, built for the host and run as a program (tests/fdr_plan_driver.py); a change of the dispatch fails here until
the shapes are revisited -- every designed length reaches the kernel it is meant for, and the designed rows have the properties
they claim when pushed through oracle.safe_oracle.fdrcorrection.  No GPU."""
import numpy as np
import pytest

import fdr_cases as fc
import fdr_plan_driver as fp
from oracle import safe_oracle as orc


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    return fp.build(tmp_path_factory.mktemp('fdr_plan'))


# ----------------------------------------------------------------------------------------------- the constants ----

def test_the_constants_are_the_ones_of_the_header(plan):
    c, ladder = fp.constants(plan)
    assert ladder == fc.IPT_LADDER and c['THREADS'] == fc.THREADS and c['BLOCK_SORT_MAX'] == fc.BLOCK_SORT_MAX
    assert fc.BLOCK_SORT_MAX == fc.THREADS * fc.IPT_LADDER[-1]
    assert fc.BLOCK_SORT_MAX <= 1 << 16                          # column ids travel as unsigned short
    assert (c['ROW_HIST_BIN_BYTES'], c['ROW_HIST_LDS_BYTES'], c['ROW_HIST_MAX_P']) == (fc.HIST_BYTES_PER_BIN, fc.HIST_LDS_BYTES, fc.HIST_MAX_P)
    assert fc.HIST_LDS_BYTES == 60 * 1024 and fc.HIST_MAX_P == 5119
    assert (fc.HIST_MAX_P + 1) * fc.HIST_BYTES_PER_BIN <= fc.HIST_LDS_BYTES < (fc.HIST_MAX_P + 2) * fc.HIST_BYTES_PER_BIN
    assert fc.HIST_MAX_P in fc.HIST_P and fc.HIST_MAX_P + 1 in fc.HIST_P
    assert (c['SEG_BATCH_KEYS'], c['SORT_MAX_ITEMS']) == (1 << 27, 1 << 31)


def test_the_ipt_ladder_is_the_one_in_the_source(plan):
    """Rows, default switch: every length up to 8193 goes to the rung fdr_cases.ipt_for names; 8192 is the last row of the block
    sort, 8193 the first of the library sort."""
    lengths = sorted(set(fc.sort_lengths()) | set(range(1, fc.BLOCK_SORT_MAX + 2)))
    got = fp.forms(plan, [(fp.ROWS, 10, m, 0, None) for m in lengths])
    for m, f in zip(lengths, got):
        want = fc.ipt_for(m)
        assert f['kind'] == f['row_kind'] == (fp.ROW_LIBRARY_SORT if want is None else fp.ROW_BLOCK_SORT), m
        assert f['ipt'] == (want or 0), m
    assert tuple(sorted({f['ipt'] for f in got} - {0})) == fc.IPT_LADDER
    by_m = dict(zip(lengths, got))
    assert by_m[fc.BLOCK_SORT_MAX]['kind'] == fp.ROW_BLOCK_SORT and by_m[fc.BLOCK_SORT_MAX + 1]['kind'] == fp.ROW_LIBRARY_SORT
    assert by_m[fc.BLOCK_SORT_MAX + 1]['batch_rows'] == 10       # all ten rows in one call of the library sort


def test_the_hand_over_to_the_library_sort_is_the_one_in_the_source(plan):
    """SAFE_HIP_FDR_SORT: under 'cub' every row length goes to the library sort, under any other value the hand-over stays at
    8192 / 8193; no count form exists under either."""
    for f in fp.forms(plan, [(fp.ROWS, 3, m, P, 'cub') for m in fc.library_lengths() for P in (0, 100)]):
        assert f['kind'] == fp.ROW_LIBRARY_SORT and f['batch_rows'] == 3
    block = fp.forms(plan, [(fp.ROWS, 3, m, P, 'block') for m in (fc.BLOCK_SORT_MAX, fc.BLOCK_SORT_MAX + 1) for P in (0, 100)])
    assert [f['kind'] for f in block] == [fp.ROW_BLOCK_SORT] * 2 + [fp.ROW_LIBRARY_SORT] * 2 and block[0]['ipt'] == fc.IPT_LADDER[-1]
    assert not any(fp.exists(plan, [(scope, P, sw) for scope in (fp.ROWS, fp.COLS, fp.ALL) for P in (1, 100, 4095) for sw in ('cub', 'block', 'sort')]))
    assert all(fp.exists(plan, [(scope, P, None) for scope in (fp.ROWS, fp.COLS, fp.ALL) for P in (1, 100, 4095)]))


def test_the_lds_rule_of_the_histogram_form_is_the_one_in_the_source(plan):
    """The row count form serves exactly P <= HIST_MAX_P, with (P + 1) * 12 bytes of LDS."""
    span = list(range(0, fc.HIST_MAX_P + 300))
    assert fp.exists(plan, [(fp.ROWS, P, None) for P in span]) == [1 <= P <= fc.HIST_MAX_P for P in span]
    for P, f in zip(fc.HIST_P, fp.forms(plan, [(fp.ROWS, 9, 300, P, None) for P in fc.HIST_P])):
        if P <= fc.HIST_MAX_P:
            assert f['kind'] == fp.ROW_HIST and f['lds'] == (P + 1) * fc.HIST_BYTES_PER_BIN <= fc.HIST_LDS_BYTES, P
        else:
            assert f['kind'] == fp.ROW_BLOCK_SORT and f['ipt'] == fc.ipt_for(300), P


def test_the_span_helper_is_the_one_the_cases_mirror(plan):
    """fdr_span equals fdr_cases.hist_bins for every thread of every designed P, and gives the library sort's chunk."""
    cases = [(P, t) for P in fc.HIST_P for t in range(fc.THREADS)]
    got = plan('span %d %d %d' % (P + 1, fc.THREADS, t) for P, t in cases)
    assert [tuple(int(x) for x in r) for r in got] == [fc.hist_bins(P, t) for P, t in cases]
    for m in fc.library_lengths():
        got = plan('span %d %d %d' % (m, fc.THREADS, t) for t in range(fc.THREADS))
        c = fc.chunk(m, 'library')
        assert [tuple(int(x) for x in r) for r in got] == [(min(t * c, m), min(t * c + c, m)) for t in range(fc.THREADS)], m


def test_the_key_transform_orders_like_argsort(plan):
    """On the bit patterns of the designed rows -- NaN of both signs and all ones, -0.0, the subnormals -- sorting by fdr_key is
    np.argsort; every NaN has the one key behind every number and below the padding key, both zeros the key 0."""
    for name, row in fc.rows(1024):
        k = fp.keys(plan, row)
        assert np.array_equal(np.argsort(k, kind='stable'), np.argsort(row, kind='stable')), name
        nan = np.isnan(row)
        assert (k[nan] == 0x7FF8000000000000).all() and (k[~nan] < 0x7FF8000000000000).all(), name
        assert np.array_equal(k[~nan], fc.bits(row[~nan] + 0.0)) and (k < fc.ALL_ONES_BITS).all(), name
    zeros = fp.keys(plan, np.array([0.0, -0.0]))
    assert zeros.tolist() == [0, 0]


def test_the_ratio_rule_is_numpys(plan):
    """fdr_ratio_bin on a designed count matrix, and on it with one entry that is no count ratio: a bin exactly where
    np.rint(p P) / P == p, the bin np.rint(p P); NaN of either sign is told apart from an entry that is no ratio."""
    P = 257
    p = fc.count_matrix(P, 300)[1]
    q = p.copy()
    q[3, 7] = 0.123456
    for mat, n_bad in ((p, 0), (q, 1)):
        got = fp.ratio_bins(plan, mat, P).reshape(mat.shape)
        nan = np.isnan(mat)
        with np.errstate(invalid='ignore'):
            ratio = ~nan & (np.rint(mat * P) / P == mat)
        assert nan.sum() == 2 and (got[nan] == fp.BIN_NAN).all()
        assert np.array_equal(got >= 0, ratio) and (got[~nan & ~ratio] == fp.BIN_NOT_RATIO).all() and (~nan & ~ratio).sum() == n_bad
        assert np.array_equal(got[ratio], np.rint(mat[ratio] * P).astype(np.int64))
    assert fp.ratio_bins(plan, np.array([-1.0 / P, (P + 1.0) / P, 1.0, 0.0, -0.0]), P).tolist() == [fp.BIN_NOT_RATIO, fp.BIN_NOT_RATIO, P, 0, 0]


# ------------------------------------------------------------------------------------------------- the lengths ----

def test_every_sort_length_reaches_the_kernel_it_is_meant_for():
    lengths = fc.sort_lengths()
    assert len(set(lengths)) == len(lengths) == 3 * len(fc.IPT_LADDER) + 1
    it = iter(lengths)
    for ipt in fc.IPT_LADDER:
        first, below, full = next(it), next(it), next(it)
        assert [fc.ipt_for(v) for v in (first, below, full)] == [ipt] * 3
        assert first == 1 or fc.ipt_for(first - 1) == ipt - 4    # the first length this rung serves
        assert full == fc.THREADS * ipt == below + 1             # no padding keys / one
    assert next(it) == fc.BLOCK_SORT_MAX + 1 and fc.ipt_for(fc.BLOCK_SORT_MAX + 1) is None
    assert {fc.ipt_for(v) for v in lengths} == set(fc.IPT_LADDER) | {None}
    ids = [fc.sort_id(v) for v in lengths]
    for ipt in fc.IPT_LADDER:
        assert sum(i.startswith('ipt%d-' % ipt) for i in ids) == 3
    assert 'ipt32-m8192' in ids and 'library-m8193' in ids


def test_library_lengths_leave_threads_without_a_chunk():
    lengths = fc.library_lengths()
    assert lengths == [1, 2, 255, 256, 257, 8193, 65537]
    idle = {m: fc.THREADS - -(-m // fc.chunk(m, 'library')) for m in lengths}
    assert idle == {1: 255, 2: 254, 255: 1, 256: 0, 257: 127, 8193: 7, 65537: 0}
    assert 65537 - 255 * fc.chunk(65537, 'library') == 2          # the last thread's chunk is a short one
    assert [m for m in lengths if fc.ipt_for(m) is None] == [8193, 65537]


def test_histogram_sizes_leave_threads_without_bins():
    assert fc.HIST_P == (1, 2, 255, 256, 257, 5119, 5120)
    assert [fc.hist_id(P) for P in fc.HIST_P][-2:] == ['P5119-hist', 'P5120-sort']
    owners = {P: sum(b0 < b1 for b0, b1 in (fc.hist_bins(P, t) for t in range(fc.THREADS))) for P in fc.HIST_P}
    assert owners == {1: 2, 2: 3, 255: 256, 256: 129, 257: 129, 5119: 256, 5120: 244}
    for P in fc.HIST_P:
        spans = [fc.hist_bins(P, t) for t in range(fc.THREADS)]
        assert spans[0][0] == 0 and max(b1 for _, b1 in spans) == P + 1
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


# ---------------------------------------------------------------------------------------------------- the rows ----

EVERY_KIND = {'uniform', 'ascending', 'descending', 'ties40', 'ones', 'one_value', 'nan_first', 'nan_last', 'nan_middle', 'all_nan',
              'sign_nan_middle', 'ones_bits_nan_middle', 'neg_zero', 'both_zeros', 'subnormal', 'above_one', 'chain_up',
              'chain_down'} | {'chain_min_t%d' % t for t in fc.CHAIN_THREADS}


def test_rows_are_named_deterministic_and_complete():
    assert [name for name, _ in fc.rows(1)] == ['uniform', 'ties40', 'ones', 'one_value', 'nan_first', 'all_nan', 'sign_nan_middle',
                                                'ones_bits_nan_middle', 'subnormal']
    assert {name for name, _ in fc.rows(2)} == EVERY_KIND - {'nan_middle', 'both_zeros', 'chain_min_t1', 'chain_min_t127',
                                                             'chain_min_t254', 'chain_min_t255'}
    for m in (1021, 1024, 8192, 8193 + 33 * 7):
        assert {name for name, _ in fc.rows(m)} == EVERY_KIND, m
    assert {name for name, _ in fc.rows(8193)} == EVERY_KIND - {'chain_min_t254', 'chain_min_t255'}      # 249 chunks of 33
    assert {name for name, _ in fc.rows(257, 0, 'library')} == EVERY_KIND - {'chain_min_t254', 'chain_min_t255'}
    for (na, a), (nb, b) in zip(fc.rows(300, 1), fc.rows.__wrapped__(300, 1)):
        assert na == nb and np.array_equal(fc.bits(a), fc.bits(b))
    assert not np.array_equal(fc.rows(300, 1)[0][1], fc.rows(300, 2)[0][1])
    names, p = fc.matrix(70, None, 60)
    assert p.shape == (60, 70) and len(names) == 60 and names[0] == 'uniform/0' and names[-1].endswith('/2')
    assert not p.flags.writeable


@pytest.mark.parametrize('m', [2, 255, 1024, 2049, 8192, 8193])
def test_plain_rows_are_what_they_say(m):
    r = dict(fc.rows(m))
    assert np.unique(r['uniform']).size == m and (r['uniform'] > 0).all() and (r['uniform'] < 1).all()
    assert np.array_equal(np.argsort(r['ascending'], kind='stable'), np.arange(m))
    assert np.array_equal(np.argsort(r['descending'], kind='stable'), np.arange(m)[::-1])
    assert np.array_equal(r['ties40'] * 40, np.round(r['ties40'] * 40)) and np.unique(r['ties40']).size <= 41
    assert (r['ones'] == 1).all() and np.unique(r['one_value']).size == 1
    assert np.array_equal(orc.fdrcorrection(r['one_value']), r['one_value'])           # a one-value row adjusts to itself
    for name, col in (('nan_first', 0), ('nan_last', m - 1), ('nan_middle', m // 2)):
        if name in r:
            assert np.flatnonzero(np.isnan(r[name])).tolist() == [col]
            assert fc.bits(r[name])[col] >> 63 == 0                                       # the positive NaN
            assert np.isnan(orc.fdrcorrection(r[name])).all()
    assert np.isnan(r['all_nan']).all()
    assert (r['subnormal'] == 5e-324).sum() == 1 and (np.abs(r['subnormal']) < 2.2250738585072014e-308).sum() == min(m, 5)
    adj = orc.fdrcorrection(r['subnormal'])
    assert (adj > 0).all() and adj.min() == 5e-324 * m                                   # the smallest value has rank 1
    assert np.isinf(r['above_one']).sum() == 1 and (r['above_one'] > 1).any()
    adj = orc.fdrcorrection(r['above_one'])
    assert adj.max() == 1.0 and adj[np.isinf(r['above_one'])] == 1.0 and (adj[r['above_one'] > 1] == 1.0).all()


@pytest.mark.parametrize('m', [1, 2, 3, 1024, 8193])
def test_a_nan_of_either_sign_makes_the_row_nan(m):
    """np.argsort puts every NaN last, whatever its sign bit, and np.minimum.accumulate carries it through the row."""
    r = dict(fc.rows(m))
    for name, pattern in (('sign_nan_middle', fc.SIGN_NAN_BITS), ('ones_bits_nan_middle', fc.ALL_ONES_BITS)):
        assert fc.bits(r[name])[m // 2] == pattern and np.isnan(r[name]).sum() == 1
        assert np.isnan(orc.fdrcorrection(r[name])).all()
        assert np.argsort(r[name])[-1] == m // 2


@pytest.mark.parametrize('m', [2, 3, 1024, 8193])
def test_a_negative_zero_is_a_zero(m):
    """NumPy sorts -0.0 as 0.0: the entry comes out as a (signed) zero and the rest of the row as if it had been +0.0."""
    r = dict(fc.rows(m))
    for name in ('neg_zero', 'both_zeros'):
        if name not in r:
            continue
        row = r[name]
        neg = np.flatnonzero(fc.bits(row) == 1 << 63)
        assert neg.size == 1 and (np.delete(row, neg) >= 0).all() and (row > 0).sum() == m - (1 if name == 'neg_zero' else 2)
        plus = row.copy()
        plus[neg] = 0.0
        assert (fc.bits(plus) >> 63 == 0).all()
        adj = orc.fdrcorrection(row)
        assert np.array_equal(adj, orc.fdrcorrection(plus))
        assert (adj[row == 0] == 0).all() and (adj[row > 0] > 0).all()


@pytest.mark.parametrize('form,m', [('block', 2), ('block', 255), ('block', 1024), ('block', 1025), ('block', 8191), ('block', 8192),
                                    ('library', 2), ('library', 257), ('library', 8193), ('library', 65537)])
def test_chain_rows_have_the_property_they_claim(form, m):
    r = dict(fc.rows(m, 0, form))
    x = np.arange(1, m + 1) / float(m)

    def sorted_raw_and_adjusted(row):
        order = np.argsort(row, kind='stable')
        assert (np.diff(row[order]) > 0).all()                   # distinct: the ranks are unambiguous
        return row[order] / x, orc.fdrcorrection(row)[order]

    raw, adj = sorted_raw_and_adjusted(r['chain_up'])
    assert (np.diff(raw) > 0).all() and raw.max() <= 1 and np.array_equal(adj, raw)          # every entry keeps its own value
    raw, adj = sorted_raw_and_adjusted(r['chain_down'])
    assert (np.diff(raw) < 0).all() and raw[-1] == 0.75 and (adj == 0.75).all()             # every entry takes the last one's
    c = fc.chunk(m, form)
    for t in fc.CHAIN_THREADS:
        name = 'chain_min_t%d' % t
        assert (name in r) == (t * c < m), (name, c)
        if name not in r:
            continue
        raw, adj = sorted_raw_and_adjusted(r[name])
        at = int(np.argmin(raw))
        assert at == fc.chain_rank(m, form, t) and at // c == t and (raw > raw[at]).sum() == m - 1
        assert raw.max() <= 1
        assert (adj[:at + 1] == raw[at]).all() and np.array_equal(adj[at:], raw[at:])     # the minimum travels left only
        assert (np.diff(raw[at:]) > 0).all()
    if m > 2:
        shuffled = [name for name in r if name.startswith('chain_')]
        assert all(not np.array_equal(np.argsort(r[name]), np.arange(m)) for name in shuffled)


@pytest.mark.parametrize('P,m', [(P, 300) for P in fc.HIST_P] + [(5119, 5120)])
def test_count_rows_are_what_they_say(P, m):
    r = dict(fc.count_rows(P, m))
    want = {'zeros', 'all_P', 'middle', 'last_thread', 'ties012', 'uniform', 'one_nan', 'sign_nan', 'neg_zero'} | ({'every_count'} if m >= P + 1 else set())
    assert set(r) == want
    assert ('every_count' in r) == ((P, m) in ((1, 300), (2, 300), (255, 300), (256, 300), (257, 300), (5119, 5120)))
    for name, row in r.items():
        ok = row[~np.isnan(row)]
        assert np.array_equal(ok, np.round(ok)) and ok.min() >= 0 and ok.max() <= P, name
    assert (r['zeros'] == 0).all() and (r['all_P'] == P).all() and np.unique(r['middle']).size == 1 and 0 < r['middle'][0] <= P
    owners = [t for t in range(fc.THREADS) if fc.hist_bins(P, t)[0] < fc.hist_bins(P, t)[1]]
    b0, b1 = fc.hist_bins(P, owners[-1])
    assert b1 == P + 1 and ((r['last_thread'] >= b0) & (r['last_thread'] < b1)).all()
    assert set(np.unique(r['ties012'])) <= {0.0, 1.0, 2.0}
    if 'every_count' in r:
        assert np.array_equal(np.unique(r['every_count']), np.arange(P + 1))
    assert np.isnan(r['one_nan']).sum() == 1 and np.isnan(r['sign_nan']).sum() == 1
    assert (fc.bits(r['neg_zero']) == 1 << 63).sum() == 1 and (r['neg_zero'] > 0).sum() == m - 1
    names, p = fc.count_matrix(P, m)
    assert (fc.bits(p[names.index('sign_nan')]) == fc.SIGN_NAN_BITS).sum() == 1
    assert (fc.bits(p[names.index('neg_zero')]) == 1 << 63).sum() == 1
    assert names == tuple(r) and p.shape == (len(r), m)
    ok = ~np.isnan(p)
    assert np.array_equal(np.rint(p[ok] * P) / P, p[ok])          # what k_fdr_check_ratio asks of a count ratio
    w = fc.count_want(P, m)
    nan_rows = [names.index('one_nan'), names.index('sign_nan')]
    assert np.isnan(w[nan_rows]).all() and not np.isnan(np.delete(w, nan_rows, axis=0)).any()
    plus = np.abs(p[names.index('neg_zero')])
    assert np.array_equal(w[names.index('neg_zero')], orc.fdrcorrection(plus)) and (w[names.index('neg_zero')] == 0).sum() == 1
    assert (w[names.index('zeros')] == 0).all() and (w[names.index('all_P')] == 1).all()
    assert not np.array_equal(fc.count_matrix(P, m, 1)[1], p, equal_nan=True)
