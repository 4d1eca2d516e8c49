"""safe_fdr_adjust_scope and safe_fdr_adjust_matrix (safepy_amd/csrc/fdr.hip) on the device: Benjamini-Hochberg along the
columns and over the whole matrix, in the count and the sort form, against oracle.safe_oracle.fdrcorrection applied along axis 0
(orc.fdr_rows(p.T).T) and to the ravelled matrix.  Every comparison is exact (fdr_cases.same: NaN equals NaN, -0.0 equals 0.0):
the device does statsmodels' divisions on the same doubles.  Shapes, designed families and references come from
tests/fdr_scope_ref.py and tests/fdr_cases.py.  Needs an MI355X."""
import numpy as np
import pytest

import fdr_cases as fc
import fdr_scope_ref as fs

pytestmark = pytest.mark.gpu

COLS, ALL = 'neighborhoods', 'all'


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)


def adjust_matrix(be, ctx, p, scope, P=0):
    """safe_fdr_adjust_matrix on a copy of p, downloaded."""
    n, m = p.shape
    buf = ctx.alloc_f64(n, m)
    try:
        buf.upload(np.ascontiguousarray(p))
        be.fdr_adjust_matrix(ctx, n, m, scope, buf.ptr, count_denominator=P)
        return buf.download((n, m))
    finally:
        buf.free()


def adjust_scope(be, ctx, p_neg, p_pos, P, sign, scope, threshold=fc.THRESHOLD, entry=None):
    """safe_fdr_adjust_scope (or `entry`, called like backend.fdr_adjust) on copies: dict(pvalues_neg, pvalues_pos, nes, nes_binary,
    num_enriched)."""
    n, m = p_pos.shape
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    try:
        if p_neg is not None:
            bufs[0].upload(np.ascontiguousarray(p_neg))
        bufs[1].upload(np.ascontiguousarray(p_pos))
        ptrs = [bufs[0].ptr if p_neg is not None else None] + [b.ptr for b in bufs[1:]]
        if entry is None:
            be.fdr_adjust_scope(ctx, n, m, P, sign, threshold, scope, ptrs)
        else:
            entry(ctx, n, m, P, sign, threshold, ptrs)
        return {'pvalues_neg': bufs[0].download((n, m)) if p_neg is not None else None, 'pvalues_pos': bufs[1].download((n, m)),
                'nes': bufs[2].download((n, m)), 'nes_binary': bufs[3].download((n, m)), 'num_enriched': bufs[4].download((m,))}
    finally:
        for b in bufs:
            b.free()


def check_columns(got, names, want, what):
    bad = fc.failing(names, got.T, want.T)
    assert not bad and fc.same(got, want), (what, bad[:8])


# ------------------------------------------------------------------------------------------------ columns, sort form ----

@pytest.mark.parametrize('n', fs.COLS_SORT_N, ids=lambda n: 'n%d' % n)
def test_columns_sort_form(be, ctx, n):
    """Designed rows of fdr_cases.rows(n) as columns, every m around the 32 x 32 transpose tile and the 64-wide ones of the issue;
    n = 8193 is a row of the library sort after the transpose."""
    for m in fs.COLS_SORT_M:
        names, p = fs.cols_sort_matrix(n, m)
        check_columns(adjust_matrix(be, ctx, p, COLS), names, fs.want(p, COLS), (n, m))


# ----------------------------------------------------------------------------------------------- columns, count form ----

@pytest.mark.parametrize('P', fs.COLS_COUNT_P, ids=lambda P: 'P%d-%s' % (P, 'hist' if P <= fs.COL_HIST_MAX_P else 'sort'))
def test_columns_count_form(be, ctx, P):
    """k_fdr_col_counts with lanes that own no bin (P + 1 < 64), at the largest P whose tile of four columns fits the LDS, and
    P = 4096, which the sort takes over; m on both sides of the column tile of that P; a column with a NaN becomes NaN and its
    neighbours stay untouched (the designed columns hold NaN of both signs and a -0.0)."""
    for n in fs.COLS_COUNT_N:
        for m in fs.cols_count_m(P) + (10,):
            names, p = fs.cols_count_matrix(P, n, m)
            want = fs.want(p, COLS)
            got = adjust_matrix(be, ctx, p, COLS, P)
            check_columns(got, names, want, (P, n, m))
            nan_cols = np.array(['nan' in name for name in names])
            assert np.isnan(got[:, nan_cols]).all() and not np.isnan(got[:, ~nan_cols]).any()


@pytest.mark.parametrize('P', [255, fs.COL_HIST_MAX_P])
def test_columns_one_value_that_is_no_count_ratio(be, ctx, P):
    """count_denominator = P with one entry that is not c / P: the sort form's bytes."""
    names, p = fs.cols_count_matrix(P, 257, 2 * fs.col_tile(P) + 1)
    p = p.copy()
    p[7, names.index('uniform/0')] = 0.123456
    assert np.rint(0.123456 * P) / P != 0.123456
    got, sort = adjust_matrix(be, ctx, p, COLS, P), adjust_matrix(be, ctx, p, COLS, 0)
    assert np.array_equal(fc.bits(got), fc.bits(sort))
    check_columns(got, names, fs.want(p, COLS), P)


def test_columns_both_forms_agree_on_the_bits(be, ctx):
    names, p = fs.cols_count_matrix(257, 4099, 33)
    count, sort = adjust_matrix(be, ctx, p, COLS, 257), adjust_matrix(be, ctx, p, COLS, 0)
    assert np.array_equal(fc.bits(count), fc.bits(sort))


# ------------------------------------------------------------------------------------------- whole matrix, sort form ----

ALL_SORT_CASES = [(shape, name) for shape in fs.ALL_SHAPES for name in fs.all_sort_names(shape[0] * shape[1])]


@pytest.mark.parametrize('shape,name', ALL_SORT_CASES, ids=['%dx%d-%s' % (s[0], s[1], name) for s, name in ALL_SORT_CASES])
def test_matrix_sort_form(be, ctx, shape, name):
    """One family of n m values: the single minimum of a chain in the first, a middle and the last thread chunk of the first, a
    middle and the last workgroup of the suffix-minimum kernels (it has to cross every chunk, workgroup and carry boundary to
    its left), a NaN at cell 0 / in the middle / at the last cell (everything becomes NaN), values above 1 with +inf, one value,
    heavy ties with a -0.0."""
    p = fs.all_sort_family(shape, name)
    got = adjust_matrix(be, ctx, p, ALL)
    assert fc.same(got, fs.want(p, ALL)), (shape, name)
    if name.startswith('nan_'):
        assert (fc.bits(got) == 0x7FF8000000000000).all()


# ------------------------------------------------------------------------------------------ whole matrix, count form ----

@pytest.mark.parametrize('P', fs.ALL_COUNT_P, ids=lambda P: 'P%d-%s' % (P, 'hist' if P <= fs.ALL_HIST_MAX_P else 'sort'))
@pytest.mark.parametrize('shape', fs.ALL_SHAPES, ids=lambda s: '%dx%d' % s)
def test_matrix_count_form(be, ctx, shape, P):
    for name in fs.ALL_COUNT_NAMES:
        p = fs.all_count_family(shape, P, name)
        got = adjust_matrix(be, ctx, p, ALL, P)
        assert fc.same(got, fs.want(p, ALL)), (shape, P, name)
        if name == 'one_nan':
            assert (fc.bits(got) == 0x7FF8000000000000).all()


def test_matrix_one_value_that_is_no_count_ratio(be, ctx):
    P, shape = 257, (255, 257)
    p = fs.all_count_family(shape, P, 'uniform').copy()
    p[100, 100] = 0.123456
    got, sort = adjust_matrix(be, ctx, p, ALL, P), adjust_matrix(be, ctx, p, ALL, 0)
    assert np.array_equal(fc.bits(got), fc.bits(sort)) and fc.same(got, fs.want(p, ALL))
    q = fs.all_count_family(shape, P, 'uniform')
    assert np.array_equal(fc.bits(adjust_matrix(be, ctx, q, ALL, P)), fc.bits(adjust_matrix(be, ctx, q, ALL, 0)))   # both forms, the same bits


# ------------------------------------------------------------------------------------------------------- row scope ----

@pytest.mark.parametrize('m', [1, 257, 1025])
def test_row_scope_gives_the_bytes_of_the_row_entry_points(be, ctx, m):
    names, p = fc.matrix(m)
    n = p.shape[0]
    buf = ctx.alloc_f64(n, m)
    try:
        buf.upload(p)
        be.fdr_adjust_rows(ctx, n, m, buf.ptr)
        rows = buf.download((n, m))
    finally:
        buf.free()
    assert np.array_equal(fc.bits(adjust_matrix(be, ctx, p, 'attributes')), fc.bits(rows))
    assert np.array_equal(fc.bits(adjust_matrix(be, ctx, p, 0)), fc.bits(rows))
    cases = [(None, p, 0, 'both'), (fc.count_matrix(100, m, 0)[1], fc.count_matrix(100, m, 1)[1], 100, 'both'),
             (fc.count_matrix(100, m, 0)[1], fc.count_matrix(100, m, 1)[1], 100, 'lowest')]
    for p_neg, p_pos, P, sign in cases:
        got = adjust_scope(be, ctx, p_neg, p_pos, P, sign, 'attributes')
        want = adjust_scope(be, ctx, p_neg, p_pos, P, sign, None, entry=be.fdr_adjust)
        for key, w in want.items():
            assert (w is None and got[key] is None) or np.array_equal(fc.bits(got[key]), fc.bits(w)), (m, P, sign, key)
    # the count form of the rows through safe_fdr_adjust_matrix; at m = 257 also at and past its LDS limit (5120: no count form,
    # so no ratio check either, and the rows are sorted)
    for P in (100,) + ((fc.HIST_MAX_P, fc.HIST_MAX_P + 1) if m == 257 else ()):
        q = fc.count_matrix(P, m, 0)[1]
        assert fc.same(adjust_matrix(be, ctx, q, 'attributes', P), fc.count_want(P, m, 0)), P


# --------------------------------------------------------------------------------------------------------- epilogue ----

def epilogue_inputs(form, n, m):
    rng = np.random.default_rng([23, n, m])
    if form == 'hypergeometric':
        return None, 10.0 ** -rng.uniform(0.0, 8.0, size=(n, m)), 0
    counts = np.floor(100 * rng.uniform(size=(2, n, m)) ** 6)
    counts[rng.uniform(size=counts.shape) < 0.02] = 100
    return counts[0] / 100.0, counts[1] / 100.0, 100


@pytest.mark.parametrize('scope', [COLS, ALL])
@pytest.mark.parametrize('form', fc.NES_FORMS)
def test_epilogue_is_the_pinned_one(be, ctx, form, scope):
    """nes and nes_binary of safe_fdr_adjust_scope equal, byte for byte, what safe_fdr_adjust returns for the expected adjusted
    matrices reshaped to [n m, 1]: a family of one is left as it is, so that call is the pinned epilogue applied cell by cell.
    num_enriched = the column sums of that nes_binary."""
    n, m = 129, 70
    p_neg, p_pos, P = epilogue_inputs(form, n, m)
    sign = 'both' if form == 'hypergeometric' else form
    got = adjust_scope(be, ctx, p_neg, p_pos, P, sign, scope)
    q_pos = fs.want(p_pos, scope)
    q_neg = fs.want(p_neg, scope) if p_neg is not None else None
    assert fc.same(got['pvalues_pos'], q_pos) and (q_neg is None or fc.same(got['pvalues_neg'], q_neg))
    cells = adjust_scope(be, ctx, q_neg.reshape(-1, 1) if q_neg is not None else None, q_pos.reshape(-1, 1), P, sign, None, entry=be.fdr_adjust)
    assert fc.same(cells['pvalues_pos'].reshape(n, m), q_pos)      # (left as they were)
    assert np.array_equal(fc.bits(got['nes']), fc.bits(cells['nes'].reshape(n, m)))
    assert np.array_equal(fc.bits(got['nes_binary']), fc.bits(cells['nes_binary'].reshape(n, m)))
    assert np.array_equal(got['num_enriched'], cells['nes_binary'].reshape(n, m).sum(axis=0))
    assert 0 < got['nes_binary'].sum() < n * m                      # both decisions occur


# --------------------------------------------------------------------------------------------------------- refusals ----

def test_refusals_write_nothing(be, ctx):
    n, m = 20, 10
    E = be._lib
    marker = np.full((n, m), -3.0)
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    ptrs = [b.ptr for b in bufs]

    def code(fn):
        with pytest.raises(E.SafeHipError) as err:
            fn()
        return err.value.code

    try:
        for b in bufs[:4]:
            b.upload(marker)
        bufs[4].upload(marker[0])
        for scope in (1, 2):
            assert code(lambda: be.fdr_adjust_matrix(ctx, n, m, scope, None)) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_matrix(ctx, 0, m, scope, ptrs[0])) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_matrix(ctx, n, 0, scope, ptrs[0])) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_matrix(ctx, n, m, scope, ptrs[0], count_denominator=-1)) == E.E_VALUE
            for k in range(1, 5):                                   # every output is needed, and pvalues_neg with P > 0
                assert code(lambda: be.fdr_adjust_scope(ctx, n, m, 0, 'both', 0.05, scope, ptrs[:k] + [None] + ptrs[k + 1:])) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_scope(ctx, n, m, 100, 'both', 0.05, scope, [None] + ptrs[1:])) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_scope(ctx, 0, m, 0, 'both', 0.05, scope, ptrs)) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_scope(ctx, n, 0, 0, 'both', 0.05, scope, ptrs)) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_scope(ctx, n, m, -1, 'both', 0.05, scope, ptrs)) == E.E_VALUE
            for thr in (0.0, 1.0, -0.5, float('nan')):
                assert code(lambda: be.fdr_adjust_scope(ctx, n, m, 0, 'both', thr, scope, ptrs)) == E.E_VALUE
        for scope in (-1, 3):
            assert code(lambda: be.fdr_adjust_matrix(ctx, n, m, scope, ptrs[0])) == E.E_VALUE
            assert code(lambda: be.fdr_adjust_scope(ctx, n, m, 0, 'both', 0.05, scope, ptrs)) == E.E_VALUE
        with pytest.raises(KeyError):
            be.fdr_adjust_matrix(ctx, n, m, 'rows', ptrs[0])
        for b in bufs[:4]:
            assert np.array_equal(b.download((n, m)), marker)       # nothing was written
        assert np.array_equal(bufs[4].download((m,)), marker[0])
        p = fs.all_count_family((n, m), 10, 'uniform')               # the context still works
        assert fc.same(adjust_matrix(be, ctx, p, ALL, 10), fs.want(p, ALL))
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------ the four forms ----

FORMS = [(COLS, 100), (COLS, 0), (ALL, 100), (ALL, 0)]
FORM_IDS = ['%s-%s' % (scope, 'count' if P else 'sort') for scope, P in FORMS]


def form_inputs(P, n=257, m=70):
    rng = np.random.default_rng([29, P, n, m])
    if P:
        p_neg, p_pos = np.floor(P * rng.uniform(size=(2, n, m)) ** 3) / float(P)
    else:                                                           # ties, and no multiples of 1 / 1000: the sort forms
        p_neg, p_pos = np.round(rng.uniform(size=(2, n, m)) ** 3, 4)
        p_neg[0, 0] = p_pos[0, 0] = 0.12345
    return p_neg, p_pos


@pytest.mark.parametrize('scope,P', FORMS, ids=FORM_IDS)
def test_three_identical_calls_give_identical_bytes(be, ctx, scope, P):
    p_neg, p_pos = form_inputs(P)
    runs = [adjust_scope(be, ctx, p_neg, p_pos, P if P else 1000, 'both', scope) for _ in range(3)]
    for other in runs[1:]:
        for key, first in runs[0].items():
            assert np.array_equal(fc.bits(first), fc.bits(other[key])), key
    assert fc.same(runs[0]['pvalues_pos'], fs.want(p_pos, scope)) and fc.same(runs[0]['pvalues_neg'], fs.want(p_neg, scope))


@pytest.mark.parametrize('scope,P', FORMS, ids=FORM_IDS)
def test_no_growth_of_live_allocations_over_20_calls(be, ctx, scope, P):
    n, m = 70, 130
    p_neg, p_pos = form_inputs(P, n, m)
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    ptrs = [b.ptr for b in bufs]
    try:
        def one(k):
            bufs[0].upload(p_neg)
            bufs[1].upload(p_pos)
            be.fdr_adjust_scope(ctx, n, m, P if P else 1000, 'both', 0.05, scope, ptrs)
            be.fdr_adjust_matrix(ctx, n, m, scope, ptrs[0], count_denominator=0 if k % 2 else P)
            if k % 5 == 0:
                with pytest.raises(be._lib.SafeHipError):
                    be.fdr_adjust_matrix(ctx, n, m, 3, ptrs[0])
        for k in range(3):                                          # the scratch slots grow to their sizes
            one(k)
        before = be.device_live_alloc_count()
        for k in range(20):
            one(k)
        assert be.device_live_alloc_count() == before
    finally:
        for b in bufs:
            b.free()


# -------------------------------------------------------------------------------------------- a busy caller's stream ----

def test_entry_points_on_a_busy_caller_stream(be, ctx):
    """Both entry points, every form, on a caller's stream that is still busy producing their (poisoned) inputs: the same bits as
    a quiet run, and the oracle's values (the harness of tests/test_gpu_stream_order.py)."""
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    n, m = 257, 70
    try:
        for (scope, P), case in zip(FORMS, FORM_IDS):
            host = form_inputs(P)
            st = [torch.from_numpy(x).to('cuda') for x in host]
            dev = [torch.empty_like(x) for x in st] + [torch.empty_like(st[0])]
            st.append(st[1])                                         # a third matrix for safe_fdr_adjust_matrix
            outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(2)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]

            def fn(scope=scope, P=P, dev=dev, outs=outs):
                be.fdr_adjust_scope(ctx, n, m, P if P else 1000, 'both', 0.05, scope, [d.data_ptr() for d in dev[:2]] + [o.data_ptr() for o in outs])
                be.fdr_adjust_matrix(ctx, n, m, scope, dev[2].data_ptr(), count_denominator=P)

            def check(got, scope=scope, host=host):
                assert fc.same(got[0], fs.want(host[0], scope)) and fc.same(got[1], fs.want(host[1], scope))
                assert fc.same(got[2], fs.want(host[1], scope))
                assert np.array_equal(got[5], got[4].sum(axis=0))

            call = so.Call(['safe_fdr_adjust_scope', 'safe_fdr_adjust_matrix'], list(zip(dev, st)), dev + outs, fn, check)
            quiet, t_call_ms = so.run_quiet(lab, call)
            call.check(quiet)
            busy, _ = so.run_busy(lab, call, t_call_ms)
            for i, (q, v) in enumerate(zip(quiet, busy)):
                assert np.array_equal(so.bits(v), so.bits(q)), '%s: output %d of the busy run differs from the quiet run' % (case, i)
            call.check(busy)
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        lab.close()
