"""safe_fdr_adjust and safe_fdr_adjust_rows (safepy_amd/csrc/fdr.hip) against oracle.safe_oracle.fdr_rows at every sort width and
key edge: the eight instantiations of k_fdr_row_sort on both sides of every 256 IPT, the library sort at the lengths that
reach it by default, the histogram form around its thread and LDS limits, and the epilogue k_nes_from_pvalues around its
64 x 64 tile.  Lengths, rows and references come from tests/fdr_cases.py (computed once, read-only).  The adjusted p-values are
the same divisions in the same order as NumPy's, so they are compared without a tolerance (NaN equal to NaN, -0.0 to 0.0).
Needs an MI355X."""
import numpy as np
import pytest

import fdr_cases as fc
from oracle import safe_oracle as orc

pytestmark = pytest.mark.gpu

MANY_ROWS = 300                              # more workgroups per launch than the device has compute units


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


def adjust_rows(be, ctx, p):
    """safe_fdr_adjust_rows on a copy of p, downloaded."""
    n, m = p.shape
    buf = ctx.alloc_f64(n, m)
    try:
        buf.upload(p)
        be.fdr_adjust_rows(ctx, n, m, buf.ptr)
        return buf.download((n, m))
    finally:
        buf.free()


def adjust(be, ctx, p_neg, p_pos, num_permutations, sign='both', threshold=fc.THRESHOLD):
    """safe_fdr_adjust on copies: dict(pvalues_neg, pvalues_pos, nes, nes_binary, num_enriched)."""
    n, m = p_pos.shape
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    try:
        if p_neg is not None:
            bufs[0].upload(p_neg)
        bufs[1].upload(p_pos)
        be.fdr_adjust(ctx, n, m, num_permutations, sign, threshold, [bufs[0].ptr if p_neg is not None else None] + [b.ptr for b in bufs[1:]])
        out = {'pvalues_neg': bufs[0].download((n, m)) if p_neg is not None else None, 'pvalues_pos': bufs[1].download((n, m)),
               'nes': bufs[2].download((n, m)), 'nes_binary': bufs[3].download((n, m)), 'num_enriched': bufs[4].download((m,))}
    finally:
        for b in bufs:
            b.free()
    return out


def check_rows(got, names, want, what):
    bad = fc.failing(names, got, want)
    assert not bad and fc.same(got, want), (what, bad)


# ------------------------------------------------------------------------------------------------- the block sort ----

@pytest.mark.parametrize('m', fc.sort_lengths(), ids=fc.sort_id)
def test_designed_rows_at_every_sort_width(be, ctx, monkeypatch, m):
    """The first length of every k_fdr_row_sort<IPT>, 256 IPT - 1 and 256 IPT (no padding keys; column ids up to 8191), and
    8193, the first row of the library sort."""
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    names, p = fc.matrix(m)
    check_rows(adjust_rows(be, ctx, p), names, fc.want(m), fc.sort_id(m))


@pytest.mark.parametrize('m', [fc.BLOCK_SORT_MAX, fc.BLOCK_SORT_MAX + 1], ids=fc.sort_id)
def test_many_workgroups_on_both_sides_of_the_hand_over(be, ctx, monkeypatch, m):
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    names, p = fc.matrix(m, None, MANY_ROWS)
    assert p.shape == (MANY_ROWS, m)
    check_rows(adjust_rows(be, ctx, p), names, fc.want(m, None, MANY_ROWS), fc.sort_id(m))


# ----------------------------------------------------------------------------------------------- the library sort ----

@pytest.mark.parametrize('m', fc.library_lengths(), ids=lambda m: 'cub-m%d' % m)
def test_designed_rows_through_the_library_sort(be, ctx, monkeypatch, m):
    """SAFE_HIP_FDR_SORT=cub: k_fdr_row with one busy thread, with len = 1, and with trailing threads that have no chunk."""
    monkeypatch.setenv('SAFE_HIP_FDR_SORT', 'cub')
    names, p = fc.matrix(m, 'library')
    check_rows(adjust_rows(be, ctx, p), names, fc.want(m, 'library'), 'cub, m = %d' % m)


@pytest.mark.parametrize('m', [v for v in fc.library_lengths() if fc.ipt_for(v) is None], ids=fc.sort_id)
def test_library_sort_where_it_is_the_default(be, ctx, monkeypatch, m):
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    names, p = fc.matrix(m, 'library')
    got = adjust_rows(be, ctx, p)
    check_rows(got, names, fc.want(m, 'library'), fc.sort_id(m))
    monkeypatch.setenv('SAFE_HIP_FDR_SORT', 'cub')              # the switch changes nothing up here
    assert np.array_equal(fc.bits(adjust_rows(be, ctx, p)), fc.bits(got))


@pytest.mark.parametrize('form', ['block', 'library'])
def test_both_sorts_agree_on_the_bits_at_8192(be, ctx, monkeypatch, form):
    """The longest row of the block sort through both forms (rows aimed at the chunks of either): the same bits, the sign of
    a zero and the payload of a NaN included."""
    m = fc.BLOCK_SORT_MAX
    names, p = fc.matrix(m, form)
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    block = adjust_rows(be, ctx, p)
    monkeypatch.setenv('SAFE_HIP_FDR_SORT', 'cub')
    library = adjust_rows(be, ctx, p)
    check_rows(block, names, fc.want(m, form), 'block')
    check_rows(library, names, fc.want(m, form), 'cub')
    differ = [name for name, a, b in zip(names, block, library) if not np.array_equal(fc.bits(a), fc.bits(b))]
    assert not differ, differ


# ---------------------------------------------------------------------------------------------- the histogram form ----

HIST_SHAPES = [(P, 300) for P in fc.HIST_P] + [(fc.HIST_MAX_P, fc.HIST_MAX_P + 1)]


@pytest.mark.parametrize('P,m', HIST_SHAPES, ids=['%s-m%d' % (fc.hist_id(P), m) for P, m in HIST_SHAPES])
def test_count_ratios_around_the_thread_and_lds_limits(be, ctx, monkeypatch, P, m):
    """k_fdr_row_counts with threads that own no bin (P + 1 < 256, and per = 2 from P = 256 on), at the largest P whose
    table fits the LDS, and P = 5120, which the sort takes over."""
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    got = adjust(be, ctx, fc.count_matrix(P, m, 0)[1], fc.count_matrix(P, m, 1)[1], P)
    for key, seed in (('pvalues_neg', 0), ('pvalues_pos', 1)):
        check_rows(got[key], fc.count_matrix(P, m, seed)[0], fc.count_want(P, m, seed), (fc.hist_id(P), key))


@pytest.mark.parametrize('sort', ['block', 'cub'])
def test_count_ratios_through_the_sorts(be, ctx, monkeypatch, sort):
    """The same matrices with the histogram form switched off: all three forms give one answer."""
    monkeypatch.setenv('SAFE_HIP_FDR_SORT', sort)
    P, m = 257, 300
    got = adjust(be, ctx, fc.count_matrix(P, m, 0)[1], fc.count_matrix(P, m, 1)[1], P)
    for key, seed in (('pvalues_neg', 0), ('pvalues_pos', 1)):
        check_rows(got[key], fc.count_matrix(P, m, seed)[0], fc.count_want(P, m, seed), (sort, key))


@pytest.mark.parametrize('P', [255, fc.HIST_MAX_P], ids=fc.hist_id)
def test_one_value_that_is_no_count_ratio(be, ctx, monkeypatch, P):
    """One entry of one matrix is not c / P: both matrices go through the sort, and nothing is adjusted twice."""
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    m = 300
    names, p = fc.count_matrix(P, m, 0)
    p = p.copy()
    p[names.index('uniform'), 7] = 0.123456
    assert np.rint(0.123456 * P) / P != 0.123456
    q = fc.count_matrix(P, m, 1)[1]
    got = adjust(be, ctx, p, q, P)
    check_rows(got['pvalues_neg'], names, orc.fdr_rows(p), 'the matrix with the odd value')
    check_rows(got['pvalues_pos'], names, fc.count_want(P, m, 1), 'the other matrix')


# ------------------------------------------------------------------------------------------ k_nes_from_pvalues ----

@pytest.mark.parametrize('m', fc.NES_M)
@pytest.mark.parametrize('n', fc.NES_N)
@pytest.mark.parametrize('form', fc.NES_FORMS)
def test_epilogue_around_the_tile(be, ctx, monkeypatch, form, n, m):
    """nes_binary and num_enriched exactly, nes at the tolerance tests/test_gpu_parity.py::test_fdr_randomization_vs_oracle
    grants the device's log10."""
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    p_neg, p_pos, nperm, ref = fc.nes_case(form, n, m)
    if form == 'both':
        assert fc.nes_margin(ref) > fc.NES_MARGIN                # a condition on the input, checked before the device is asked
    got = adjust(be, ctx, p_neg, p_pos, nperm, 'both' if form == 'hypergeometric' else form)
    for key in ('pvalues_neg', 'pvalues_pos'):
        if ref[key] is not None:
            assert fc.same(got[key], ref[key]), key
    assert np.array_equal(got['nes_binary'], ref['nes_binary']), np.argwhere(got['nes_binary'] != ref['nes_binary'])[:5]
    assert np.array_equal(got['num_enriched'], ref['num_enriched'])
    np.testing.assert_allclose(got['nes'], ref['nes'], rtol=1e-12, atol=1e-12)
    if n * m >= 63 * 63:
        assert 0 < ref['nes_binary'].sum() < n * m               # both decisions occur


@pytest.mark.parametrize('m', [1, 65])
@pytest.mark.parametrize('form', ['hypergeometric', 'highest', 'lowest'])
def test_binarisation_at_the_boundary_after_adjustment(be, ctx, monkeypatch, form, m):
    """One-value rows adjust to themselves, so the epilogue sees the threshold, its neighbours and the pair of doubles
    between which the host's -log10(p) > -log10(threshold) changes its answer: nes_p_cut must put the cut there."""
    monkeypatch.delenv('SAFE_HIP_FDR_SORT', raising=False)
    values = fc.boundary_values()
    p = np.repeat(values[:, None], m, axis=1)
    other = np.full(p.shape, 0.5)
    want = (-np.log10(p) > -np.log10(fc.THRESHOLD)).astype(np.float64)
    assert want.sum(axis=1).tolist() == [float(w) * m for w in want[:, 0]] and want[3, 0] == 1 and want[4, 0] == 0
    if form == 'hypergeometric':
        got = adjust(be, ctx, None, p, 0)
    elif form == 'highest':
        got = adjust(be, ctx, other, p, fc.NES_PERM, 'highest')
    else:
        got = adjust(be, ctx, p, other, fc.NES_PERM, 'lowest')
    side = 'pvalues_neg' if form == 'lowest' else 'pvalues_pos'
    assert np.array_equal(fc.bits(got[side]), fc.bits(p))         # a one-value row adjusts to itself
    assert np.array_equal(got['nes_binary'], want), (got['nes_binary'][:, 0], want[:, 0])
    assert np.array_equal(got['num_enriched'], want.sum(axis=0))
    np.testing.assert_allclose(got['nes'], -np.log10(p), rtol=1e-12, atol=1e-12)
