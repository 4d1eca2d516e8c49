"""The decision margins of the filtered matrix-core permutation tests (k_permtest_mfma_g, k_permtest_mfma_gz, the general
kernel's filtered form), on the designed near-ties of tests/filter_margin_cases.py: a large share of ALL compares sits within a
factor four of each margin with the low digits at their extremes, so a window one unit too narrow changes a counter.  Every
case runs the default form, the general filtered form and the classic six- / seven-slice form and asks for bit-equal
outputs; 'sum' counters also equal the exact integer reference.  No tolerance anywhere.  Needs an MI355X."""
import numpy as np
import pytest

import filter_margin_cases as fm

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(autouse=True)
def narrow_blocks_stay_on_the_matrix_cores(monkeypatch):
    """(As in test_gpu_mfma.py: the product sends blocks this narrow to the LDS-resident f64 kernel.)"""
    monkeypatch.setenv('SAFE_HIP_NARROW_LDS', '0')
    for knob in ('SAFE_HIP_MFMA_FORM', 'SAFE_HIP_MFMA_FILTER', 'SAFE_HIP_MFMA_FILTER_CAP', 'SAFE_HIP_FORCE_PATH'):
        monkeypatch.delenv(knob, raising=False)


def _run(amd, ctx, nbr, case, nperm, col0=0, col1=None):
    """One permtest_counts call -> {ns, neg, pos, name, slices, core, undecided, tables}."""
    from safepy_amd import backend as be
    b = case.b
    n, m = b.shape
    col1 = m if col1 is None else col1
    attr = be.Attributes.from_host(ctx, b)
    perms = be.Permutations(ctx, n, attr.row_flags(), nperm, case.seed)
    ns, neg, pos = (ctx.alloc_f64(n, col1 - col0) for _ in range(3))
    be.permtest_counts(ctx, nbr, attr, perms, case.score, ns.ptr, neg.ptr, pos.ptr, col0, col1)
    core, undecided = be.last_mfma_filter(ctx)
    out = dict(ns=ns.download((n, col1 - col0)), neg=neg.download((n, col1 - col0)), pos=pos.download((n, col1 - col0)),
               name=ctx.last_kernel()[0], slices=be.last_mfma_slices(ctx), core=core, undecided=undecided,
               tables=perms.read().astype(np.int64))
    perms.close()
    attr.close()
    return out


def _three_forms(amd, ctx, monkeypatch, case, nperm, col0=0, col1=None):
    """The default form (checked to be the filtered one), the general filtered form, the classic form; the three must leave
    bit-equal outputs.  Returns (default, classic, report)."""
    z = case.score == 'z-score'
    nbr = amd.Neighborhoods.euclidean(ctx, case.xy, case.nr)
    try:
        first = _run(amd, ctx, nbr, case, nperm, col0, col1)
        assert first['name'] == 'k_permtest_mfma'
        if not z:
            assert first['slices'] == 6
        assert first['core'] == (4 if z else 3) and first['undecided'] >= 0, (first['core'], first['undecided'])
        compares = first['neg'].size * nperm
        report = '%s, %d permutations: %d of %d compares (%.2f %%) left to the resolve kernel by the default form' % (
            case.name, nperm, first['undecided'], compares, 100.0 * first['undecided'] / compares)
        monkeypatch.setenv('SAFE_HIP_MFMA_FORM', 'general')
        general = _run(amd, ctx, nbr, case, nperm, col0, col1)
        assert general['name'] == 'k_permtest_mfma' and general['core'] == (4 if z else 3) and general['undecided'] >= 0
        monkeypatch.delenv('SAFE_HIP_MFMA_FORM')
        monkeypatch.setenv('SAFE_HIP_MFMA_FILTER', '0')
        classic = _run(amd, ctx, nbr, case, nperm, col0, col1)
        assert classic['name'] == 'k_permtest_mfma' and classic['core'] == (7 if z else 6)
        monkeypatch.delenv('SAFE_HIP_MFMA_FILTER')
    finally:
        nbr.close()
    np.testing.assert_array_equal(first['tables'], classic['tables'])
    for form, got in (('default', first), ('general filtered', general)):
        for key in ('neg', 'pos', 'ns'):
            np.testing.assert_array_equal(got[key], classic[key], err_msg='%s form, %s vs the classic form; %s' % (form, key, report))
    return first, classic, report


def _check_sum(case, first, report, col0=0, col1=None):
    col1 = case.b.shape[1] if col1 is None else col1
    sub = case.b[:, col0:col1]
    neg_w, pos_w = fm.exact_counts(case.a, sub, first['tables'])
    np.testing.assert_array_equal(first['neg'], neg_w, err_msg=report)
    np.testing.assert_array_equal(first['pos'], pos_w, err_msg=report)
    np.testing.assert_array_equal(first['ns'], fm.exact_sums(case.a, sub).astype(np.float64), err_msg=report)


CASES = [(name, fm.NPERM) for name in fm.CASES] + [(name, p) for name in ('S-offset', 'Z-near') for p in fm.NPERM_FLUSH]


@pytest.mark.parametrize('name,nperm', CASES, ids=['%s-%d' % c for c in CASES])
def test_near_ties_at_the_margins_every_form(amd, ctx, monkeypatch, name, nperm):
    """(Z-var is also the regression case of identical values under rounded squares: the neighborhood of row 226 holds identical values, five columns
    hold their squares rounded, and EXX - mean^2 was the rounding of those squares -- in column 9 positive, an observed score
    of 18418071.61 where the variance is zero and the reference says NaN; mf_identical_values recognises the neighborhood from
    its sums.  Z-near and Z-count hold the other side: real variances of the same size, scores of 4.4e6 ... 8.9e6, stay.)"""
    case = fm.CASES[name]()
    assert nperm in case.nperms
    first, classic, report = _three_forms(amd, ctx, monkeypatch, case, nperm)
    if case.score == 'sum':
        # S-top-2047 is the largest neighborhood k_permtest_mfma_g takes; S-top-2048 runs the general filtered form by default
        _check_sum(case, first, report)
    else:
        ns_w = orc.compute_neighborhood_score(case.a, case.b, 'z-score')
        differ = np.argwhere(np.isnan(first['ns']) != np.isnan(ns_w))
        assert differ.size == 0, '%s; NaN pattern of the observed scores differs from the oracle at (row, column) %s: %s, oracle %s' % (
            report, differ.tolist(), first['ns'][tuple(differ.T)], ns_w[tuple(differ.T)])
        if name == 'Z-exact':                                           # values AND squares exact: the oracle's f64 sums are exact
            neg_w, pos_w = orc.run_permutations(case.a, case.b, 'z-score', nperm, case.seed)
            np.testing.assert_array_equal(first['ns'], ns_w, err_msg=report)
            np.testing.assert_array_equal(first['neg'], neg_w, err_msg=report)
            np.testing.assert_array_equal(first['pos'], pos_w, err_msg=report)


def test_near_ties_in_a_column_shard_that_starts_inside_a_tile(amd, ctx, monkeypatch):
    case = fm.s_offset()
    first, _, report = _three_forms(amd, ctx, monkeypatch, case, fm.NPERM, col0=5)
    _check_sum(case, first, report, col0=5)


def test_near_ties_over_two_launch_spans(amd, ctx, monkeypatch):
    case = fm.s_offset()
    first, _, report = _three_forms(amd, ctx, monkeypatch, case, 300)
    _check_sum(case, first, report)
