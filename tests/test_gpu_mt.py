"""safe_mt_adjust_matrix and safe_mt_adjust_scope (safepy_amd/csrc/fdr.hip) on the device: Benjamini-Yekutieli, Holm, Hochberg and
Bonferroni -- and Benjamini-Hochberg through the new entry points -- in every form and scope, bit for bit against the NumPy
restatement tests/mt_ref.py.  No tolerance anywhere: the device does multipletests' operations on the same doubles.  Shapes come
from tests/fdr_cases.py and tests/fdr_scope_ref.py (every rung of the block sort, the library sort, the LDS limits of the count
forms, the workgroup edges of the whole-matrix scan); the designed families from mt_ref (a procedure's running extreme in a
chosen chunk, tie groups across chunk and workgroup edges, clamps, NaN of both signs, -0.0, subnormals).  Every call runs on a
buffer with poisoned padding behind the matrix, which must stay as it was.  Needs an MI355X."""
import numpy as np
import pytest

import fdr_cases as fc
import fdr_scope_ref as fs
import mt_ref as mt

pytestmark = pytest.mark.gpu

ROWS, COLS, ALL = 'attributes', 'neighborhoods', 'all'
PAD, POISON = 64, -7.25


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


def adjust(be, ctx, p, scope, method, P=0, old=False):
    """safe_mt_adjust_matrix (old: safe_fdr_adjust_matrix) on a copy of p with PAD poisoned doubles behind it, downloaded."""
    n, m = p.shape
    host = np.concatenate([np.ascontiguousarray(p, dtype=np.float64).ravel(), np.full(PAD, POISON)])
    buf = ctx.alloc_f64(n * m + PAD)
    try:
        buf.upload(host)
        if old:
            be.fdr_adjust_matrix(ctx, n, m, scope, buf.ptr, count_denominator=P)
        else:
            be.mt_adjust_matrix(ctx, n, m, scope, method, buf.ptr, count_denominator=P)
        out = buf.download((n * m + PAD,))
    finally:
        buf.free()
    assert (out[n * m:] == POISON).all(), 'the padding behind the matrix was written'
    return out[:n * m].reshape(n, m)


def check(be, ctx, p, scope, method, P=0, names=None, what=None, sort_too=None):
    """The device against the restatement on the bits; under 'fdr_bh' also against the old entry point's bytes; sort_too: a
    monkeypatch -- the same call with the count forms switched off must give the same bytes."""
    want = mt.adjust(p, scope, method)
    got = adjust(be, ctx, p, scope, method, P)
    if not mt.same_bits(got, want):
        rows = (got, want) if scope == ROWS else (got.T, want.T)
        bad = mt.differing(names, *rows) if names is not None and scope != ALL else int((fc.bits(got) != fc.bits(want)).sum())
        raise AssertionError((method, scope, p.shape, P, what, bad if isinstance(bad, int) else bad[:8]))
    if method == 'fdr_bh':
        assert mt.same_bits(got, adjust(be, ctx, p, scope, method, P, old=True)), (scope, p.shape, P, what)
    if sort_too is not None:
        sort_too.setenv('SAFE_HIP_FDR_SORT', '1')
        assert mt.same_bits(adjust(be, ctx, p, scope, method, P), got), (method, scope, p.shape, P, what)
        sort_too.delenv('SAFE_HIP_FDR_SORT')
    return got


# ------------------------------------------------------------------------------------------------ rows, sort forms ----

@pytest.mark.parametrize('method', mt.METHODS)
def test_rows_block_sort_every_rung(be, ctx, method):
    """m = 1, 2, 255 and, for every rung of k_fdr_row_sort<IPT>, its first length, 256 IPT - 1 and 256 IPT; 8193 is the first row
    of the library sort.  The procedure's extreme sits in the chunks of threads 0, 1, 127, 254, 255 and has to be carried."""
    for m in [1, 2, 255] + fc.sort_lengths():
        names, p = mt.matrix(method, m)
        check(be, ctx, p, ROWS, method, names=names, what=fc.sort_id(m))


@pytest.mark.parametrize('method', mt.METHODS)
def test_rows_library_sort(be, ctx, method, monkeypatch):
    """SAFE_HIP_FDR_SORT=cub: every length through the segmented sort and k_fdr_row; 8191 / 8192 / 8193 and 65 537 among them.  A
    NaN whose sign bit is set sorts in FRONT of the numbers there: Holm's ranks must not count it."""
    monkeypatch.setenv('SAFE_HIP_FDR_SORT', 'cub')
    for m in fc.library_lengths() + [8191, 8192]:
        names, p = mt.matrix(method, m, 'library')
        if m > 8193:
            keep = [i for i, name in enumerate(names) if name.startswith(('mt_', 'small', 'clamp', 'ties_at', 'nans_', 'nan_', 'sign_nan', 'neg_zero'))]
            names, p = [names[i] for i in keep], p[keep]
        want = mt.adjust(p, ROWS, method)
        got = adjust(be, ctx, p, ROWS, method)
        assert not mt.differing(names, got, want), (method, m, mt.differing(names, got, want)[:8])
        if method == 'fdr_bh':
            assert mt.same_bits(got, adjust(be, ctx, p, ROWS, method, old=True)), m


# ---------------------------------------------------------------------------------------------------- count forms ----

def count_rows(P, m):
    names0, p0 = fc.count_matrix(P, m, 0)
    names1, p1 = fc.count_matrix(P, m, 1)
    return names0 + names1, np.concatenate([p0, p1])


@pytest.mark.parametrize('method', mt.METHODS)
def test_rows_count_form(be, ctx, method, monkeypatch):
    """k_fdr_row_counts at P = 1, 2, 10, 1000, 5119 and the hand-over to the sort at 5120: the restatement's bits, and the bytes
    of the sort form (the count form's table holds the same doubles: first position for Holm, last for the others)."""
    for P in (1, 2, 10, 1000, fc.HIST_MAX_P, fc.HIST_MAX_P + 1):
        for m in (257, 1031):
            names, p = count_rows(P, m)
            check(be, ctx, p, ROWS, method, P, names, fc.hist_id(P), sort_too=monkeypatch)


@pytest.mark.parametrize('method', mt.METHODS)
def test_columns_count_form(be, ctx, method, monkeypatch):
    """k_fdr_col_counts at tiles of 16 columns (P = 255, 1023) and of 4 (P = 4095), and P = 4096, which the sort takes; m on
    both sides of the tile; columns with NaN of both signs and -0.0."""
    for P in (255, 1023, fs.COL_HIST_MAX_P, fs.COL_HIST_MAX_P + 1):
        assert fs.col_tile(min(P, fs.COL_HIST_MAX_P)) == (16 if P <= 1023 else 4)
        for n in (2, 257, 4099):
            for m in fs.cols_count_m(P)[1:]:
                names, p = fs.cols_count_matrix(P, n, m)
                check(be, ctx, p, COLS, method, P, names, (P, n, m), sort_too=monkeypatch if n == 257 else None)


@pytest.mark.parametrize('method', mt.METHODS)
def test_matrix_count_form(be, ctx, method, monkeypatch):
    """k_fdr_all_hist / _table / _map at P = 1000, 16 383 and the hand-over at 16 384."""
    for P in (1000, fs.ALL_HIST_MAX_P, fs.ALL_HIST_MAX_P + 1):
        for shape in ((1, 257), (16, 16), (255, 257)):
            for name in fs.ALL_COUNT_NAMES:
                p = fs.all_count_family(shape, P, name)
                got = check(be, ctx, p, ALL, method, P, what=(P, shape, name), sort_too=monkeypatch)
                if name == 'one_nan':
                    assert np.isnan(got).sum() == (got.size if method in mt.POISONED else 1)


# ------------------------------------------------------------------------------------------------ columns, sort form ----

@pytest.mark.parametrize('method', mt.METHODS)
def test_columns_sort_form(be, ctx, method):
    """The transpose around the row forms: designed rows as columns, n through the block sort and (8193) the library sort, m around
    the 32 x 32 transpose tile."""
    for n in (1, 2, 257, 1025, 8193):
        names, rows = mt.matrix(method, n)
        for m in (1, 31, 33):
            p = np.ascontiguousarray(rows[:m].T)
            check(be, ctx, p, COLS, method, names=names[:m], what=(n, m))


# ------------------------------------------------------------------------------------------------ matrix, sort form ----

ALL_SORT_SHAPES = ((1, 1), (23, 89), (8, 256), (3, 683), (11, 559))        # totals 1, 2047, 2048, 2049, 3 2048 + 5


def all_sort_families(method, shape):
    total = shape[0] * shape[1]
    assert total in (1, fs.ALL_BLOCK - 1, fs.ALL_BLOCK, fs.ALL_BLOCK + 1, 3 * fs.ALL_BLOCK + 5)
    rng = np.random.default_rng([59, total])
    shuffle = rng.permutation(total)
    out = []
    if total >= 2:
        for name, at in fs.all_chain_positions(total).items():      # first / middle / last chunk of the first / middle / last workgroup
            v = np.empty(total)
            v[shuffle] = mt.chain(method, total, at)
            assert mt.extreme_rank(v, method) == at or method == 'bonferroni'
            out.append(('mt_' + name, v))
    edges = [fs.ALL_IPT, 255 * fs.ALL_IPT, fs.ALL_BLOCK, 2 * fs.ALL_BLOCK, 3 * fs.ALL_BLOCK]
    out += [('small', mt.small(total)), ('clamp', mt.clamp_family(total)), ('ties_at_edges', mt.tie_family(total, edges)),
            ('ones', np.ones(total)), ('ties40', rng.integers(0, 41, size=total) / 40.0 / total)]
    for name, cells in (('nan_first', [0]), ('nan_middle', [total // 2]), ('nan_last', [total - 1]), ('nan_three', [0, total // 2, total - 1])):
        v = mt.small(total, 1)
        for i, cell in enumerate(cells):
            v = mt.with_bits(v, cell, fc.SIGN_NAN_BITS if i % 2 == 0 else mt.QNAN_BITS)
        out.append((name, v))
    v = mt.small(total, 2)
    v[total // 3] = -0.0
    if total >= 8:
        v[[1, 5, 7]] = [5e-324, 1e-310, 0.0]
    out.append(('zeros_subnormals', v))
    return [(name, v.reshape(shape)) for name, v in out]


@pytest.mark.parametrize('method', mt.METHODS)
def test_matrix_sort_form(be, ctx, method):
    """One family of n m values on shapes that are not square: the extreme of the procedure's scan in the first, a middle and
    the last chunk of the first, a middle and the last workgroup -- Holm's maximum travels right from the first workgroup, the
    others' minimum left from the last -- tie groups across chunk and workgroup edges, clamps, NaN at both ends and the middle."""
    for shape in ALL_SORT_SHAPES:
        for name, p in all_sort_families(method, shape):
            got = check(be, ctx, p, ALL, method, what=(shape, name))
            if name.startswith('nan_'):
                nans = 3 if name == 'nan_three' else 1
                assert np.isnan(got).sum() == (got.size if method in mt.POISONED else min(nans, got.size)), (shape, name)


def test_holm_and_hochberg_differ_in_most_cells(be, ctx):
    """The two procedures share the products and differ in the scan: on the small families the device's results differ in most
    cells, so a swapped direction cannot pass the tests above."""
    for scope, p in ((ROWS, np.stack([mt.small(1025, s) for s in range(8)])), (ALL, mt.small(6149).reshape(11, 559)),
                     (COLS, np.stack([mt.small(1025, s) for s in range(8)], axis=1))):
        holm, hochberg = adjust(be, ctx, p, scope, 'holm'), adjust(be, ctx, p, scope, 'hochberg')
        assert (holm >= hochberg).all() and (holm != hochberg).sum() > p.size // 2, scope


# ------------------------------------------------------------------------------------------------------ Bonferroni ----

def test_bonferroni_is_element_wise_in_every_scope(be, ctx, monkeypatch):
    """p times the size of the scope's family, clamped, NaN cells alone NaN: no form, so SAFE_HIP_FDR_SORT and a count
    denominator change nothing."""
    names, rows = mt.matrix('bonferroni', 257)
    p = np.ascontiguousarray(rows[:33])
    for scope in (ROWS, COLS, ALL):
        count = mt.family_size(p.shape, scope)
        with np.errstate(invalid='ignore'):
            want = np.where(p == 0, 0.0, p) * float(count)
            want[want > 1] = 1
        want[np.isnan(want)] = np.nan
        got = check(be, ctx, p, scope, 'bonferroni', what=scope, sort_too=monkeypatch)
        assert mt.same_bits(got, want)
        assert mt.same_bits(adjust(be, ctx, p, scope, 'bonferroni', P=1000), got)


# -------------------------------------------------------------------------------------------------------- epilogue ----

def scope_call(be, ctx, p_neg, p_pos, P, sign, scope, method=None, threshold=fc.THRESHOLD):
    """safe_mt_adjust_scope (method None: safe_fdr_adjust_scope) on copies: dict(pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched)."""
    n, m = p_pos.shape
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    try:
        if p_neg is not None:
            bufs[0].upload(np.ascontiguousarray(p_neg))
        bufs[1].upload(np.ascontiguousarray(p_pos))
        ptrs = [bufs[0].ptr if p_neg is not None else None] + [b.ptr for b in bufs[1:]]
        if method is None:
            be.fdr_adjust_scope(ctx, n, m, P, sign, threshold, scope, ptrs)
        else:
            be.mt_adjust_scope(ctx, n, m, P, sign, threshold, scope, method, ptrs)
        return {'pvalues_neg': bufs[0].download((n, m)) if p_neg is not None else None, 'pvalues_pos': bufs[1].download((n, m)),
                'nes': bufs[2].download((n, m)), 'nes_binary': bufs[3].download((n, m)), 'num_enriched': bufs[4].download((m,))}
    finally:
        for b in bufs:
            b.free()


def epilogue_inputs(form, n, m):
    """Small p-values, so that cells stay enriched after a family-wise adjustment over up to n m tests."""
    rng = np.random.default_rng([61, n, m])
    if form == 'hypergeometric':
        return None, 10.0 ** -rng.uniform(0.0, 9.0, size=(n, m)), 0
    counts = np.floor(100 * rng.uniform(size=(2, n, m)) ** 8)
    counts[rng.uniform(size=counts.shape) < 0.02] = 100
    return counts[0] / 100.0, counts[1] / 100.0, 100


@pytest.mark.parametrize('method', mt.METHODS)
@pytest.mark.parametrize('form', fc.NES_FORMS)
def test_scope_entry_point_and_its_epilogue(be, ctx, form, method):
    """safe_mt_adjust_scope: both matrices against the restatement; nes / nes_binary equal, byte for byte, what safe_fdr_adjust
    returns for the expected adjusted matrices reshaped to [n m, 1] (a family of one is left as it is: the pinned epilogue cell
    by cell), num_enriched its column sums.  'fdr_bh' also gives the bytes of safe_fdr_adjust_scope."""
    n, m = 129, 70
    p_neg, p_pos, P = epilogue_inputs(form, n, m)
    sign = 'both' if form == 'hypergeometric' else form
    hits = 0
    for scope in (ROWS, COLS, ALL):
        got = scope_call(be, ctx, p_neg, p_pos, P, sign, scope, method)
        q_pos = mt.adjust(p_pos, scope, method)
        q_neg = mt.adjust(p_neg, scope, method) if p_neg is not None else None
        assert mt.same_bits(got['pvalues_pos'], q_pos) and (q_neg is None or mt.same_bits(got['pvalues_neg'], q_neg)), scope
        cells = scope_call(be, ctx, q_neg.reshape(-1, 1) if q_neg is not None else None, q_pos.reshape(-1, 1), P, sign, ROWS)
        assert mt.same_bits(cells['pvalues_pos'].reshape(n, m), q_pos)          # (left as they were)
        assert mt.same_bits(got['nes'], cells['nes'].reshape(n, m)), scope
        assert mt.same_bits(got['nes_binary'], cells['nes_binary'].reshape(n, m)), scope
        assert np.array_equal(got['num_enriched'], cells['nes_binary'].reshape(n, m).sum(axis=0)), scope
        hits += got['nes_binary'].sum()
        if method == 'fdr_bh':
            old = scope_call(be, ctx, p_neg, p_pos, P, sign, scope)
            for key, value in old.items():
                assert (value is None and got[key] is None) or mt.same_bits(got[key], value), (scope, key)
    assert 0 < hits < 3 * n * m                                       # both decisions occur


# ------------------------------------------------------------------------------- repeatability, memory, refusals ----

FORMS = [(ROWS, 100), (ROWS, 0), (COLS, 100), (COLS, 0), (ALL, 100), (ALL, 0)]


def form_inputs(P, n=257, m=70):
    rng = np.random.default_rng([67, P, n, m])
    if P:
        return np.floor(P * rng.uniform(size=(2, n, m)) ** 3) / float(P)
    p = np.round(rng.uniform(size=(2, n, m)) ** 3, 4)                 # ties, and no multiples of 1 / 1000: the sort forms
    p[:, 0, 0] = 0.12345
    return p


@pytest.mark.parametrize('method', mt.METHODS[1:])
def test_identical_calls_give_identical_bytes_and_memory_stays_steady(be, ctx, method):
    n, m = 70, 130
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    ptrs = [b.ptr for b in bufs]
    try:
        for scope, P in FORMS:
            p_neg, p_pos = form_inputs(P, n, m)
            runs = [scope_call(be, ctx, p_neg, p_pos, P if P else 1000, 'both', scope, method) for _ in range(3)]
            for other in runs[1:]:
                for key, first in runs[0].items():
                    assert mt.same_bits(first, other[key]), (scope, P, key)
            assert mt.same_bits(runs[0]['pvalues_neg'], mt.adjust(p_neg, scope, method))

            def one(k):
                bufs[0].upload(p_neg)
                bufs[1].upload(p_pos)
                be.mt_adjust_scope(ctx, n, m, P if P else 1000, 'both', 0.05, scope, method, ptrs)
                be.mt_adjust_matrix(ctx, n, m, scope, method, ptrs[0], count_denominator=0 if k % 2 else P)
                if k % 4 == 0:
                    with pytest.raises(be._lib.SafeHipError):
                        be.mt_adjust_matrix(ctx, n, m, scope, 7, ptrs[0])
            for k in range(2):                                        # the scratch slots grow to their sizes
                one(k)
            before = be.device_live_alloc_count()
            for k in range(8):
                one(k)
            assert be.device_live_alloc_count() == before, (scope, P)
    finally:
        for b in bufs:
            b.free()


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
        for method in mt.METHODS:
            for scope in (0, 1, 2):
                assert code(lambda: be.mt_adjust_matrix(ctx, n, m, scope, method, None)) == E.E_VALUE
                assert code(lambda: be.mt_adjust_matrix(ctx, 0, m, scope, method, ptrs[0])) == E.E_VALUE
                assert code(lambda: be.mt_adjust_matrix(ctx, n, 0, scope, method, ptrs[0])) == E.E_VALUE
                assert code(lambda: be.mt_adjust_matrix(ctx, n, m, scope, method, ptrs[0], count_denominator=-1)) == E.E_VALUE
                for k in range(1, 5):                                 # every output is needed, and pvalues_neg with P > 0
                    assert code(lambda: be.mt_adjust_scope(ctx, n, m, 0, 'both', 0.05, scope, method, ptrs[:k] + [None] + ptrs[k + 1:])) == E.E_VALUE
                assert code(lambda: be.mt_adjust_scope(ctx, n, m, 100, 'both', 0.05, scope, method, [None] + ptrs[1:])) == E.E_VALUE
                assert code(lambda: be.mt_adjust_scope(ctx, n, m, -1, 'both', 0.05, scope, method, ptrs)) == E.E_VALUE
                for thr in (0.0, 1.0, float('nan')):
                    assert code(lambda: be.mt_adjust_scope(ctx, n, m, 0, 'both', thr, scope, method, ptrs)) == E.E_VALUE
            for scope in (-1, 3):
                assert code(lambda: be.mt_adjust_matrix(ctx, n, m, scope, method, ptrs[0])) == E.E_VALUE
                assert code(lambda: be.mt_adjust_scope(ctx, n, m, 0, 'both', 0.05, scope, method, ptrs)) == E.E_VALUE
        for number in (-1, 5, 99):                                    # a method outside 0 ... 4
            assert code(lambda: be.mt_adjust_matrix(ctx, n, m, 0, number, ptrs[0])) == E.E_VALUE
            assert code(lambda: be.mt_adjust_scope(ctx, n, m, 0, 'both', 0.05, 2, number, ptrs)) == E.E_VALUE
        for c in (0.0, 0.5, -1.0, float('inf'), float('nan')):        # Benjamini-Yekutieli's constant: finite and at least 1
            assert code(lambda: be.mt_adjust_matrix(ctx, n, m, 0, 'fdr_by', ptrs[0], by_const=c)) == E.E_VALUE
            assert code(lambda: be.mt_adjust_scope(ctx, n, m, 0, 'both', 0.05, 1, 'fdr_by', ptrs, by_const=c)) == E.E_VALUE
        with pytest.raises(KeyError):
            be.mt_adjust_matrix(ctx, n, m, 'all', 'sidak', ptrs[0])
        for b in bufs[:4]:
            assert np.array_equal(b.download((n, m)), marker)         # nothing was written
        assert np.array_equal(bufs[4].download((m,)), marker[0])
        # ... and the constant is ignored by the other procedures; the context still works
        p = mt.small(n * m).reshape(n, m)
        bufs[0].upload(p)
        be.mt_adjust_matrix(ctx, n, m, 'all', 'holm', bufs[0].ptr, by_const=float('nan'))
        assert mt.same_bits(bufs[0].download((n, m)), mt.adjust(p, 'all', 'holm'))
    finally:
        for b in bufs:
            b.free()


def test_by_constant_crosses_the_abi_as_given(be, ctx):
    """The library sums nothing: a constant that is not the family's harmonic sum gives the restatement's bits with that constant."""
    names, p = mt.matrix('fdr_bh', 257)
    for c in (1.0, 2.5, be.by_constant(257)):
        buf = ctx.alloc_f64(*p.shape)
        try:
            buf.upload(p)
            be.mt_adjust_matrix(ctx, p.shape[0], 257, ROWS, 'fdr_by', buf.ptr, by_const=c)
            assert mt.same_bits(buf.download(p.shape), mt.rows(p, 'fdr_by', c)), c
        finally:
            buf.free()
