"""Hypergeometric p-values of every evaluator against the EXACT rational tail (tests/hyp_exact.py) on designed inputs
(tests/hyp_cases.py): every cell's (pop, K, n, x) is chosen -- deep tails down to the subnormals, supports that start above 0,
K and n at 0, 1 and the population, populations cut by all-NaN rows, 20 000 nodes, calls whose largest count cuts the table far
below / at the top of a support.  Needs an MI355X.

Evaluators (selected as test_midsize_hypergeometric_vs_oracle does, the kernel name asserted):

    bits         k_hyp_table read by k_counts_bits<hypergeom>                 SAFE_HIP_COUNTS=bits
    mfma         ... by k_hyp_emit, table slab in LDS                         SAFE_HIP_COUNTS=mfma
    mfma-nolds   ... by k_hyp_emit, gathered from memory                      + SAFE_HIP_EMIT_LDS_KB=0
    mfma-fused   ... by the epilogue of k_permtest_mfma<counts>               + SAFE_HIP_HYP_SPLIT=0
    per-element  hyp_sf in k_hypergeom_tail                                   SAFE_HIP_HYPER_TABLE=0

(family, form) pairs that cannot be reached, by the routes in enrich.hip (counts_route, hypergeom_fused):

  * table forms x any call with a neighborhood of 1024 or more members (row sum of A): the count route of the table forms is the
    bit-sliced one, which ends there -- such a call goes to k_hypergeom_tail whatever the switches say.  So
    'deep-N2003-large-neighborhoods' (n = pop - 3, pop at 2003 nodes) and 'full-N20000-hub' run per-element only, the 20 000-node
    table case stops at n = 1023 (not "just below 2048": that is the permutation kernel's limit, not this route's), and n = pop - 3,
    pop reach the table forms at 1000 nodes ('deep-N1000') and in families 1 and 3.
  * matrix-core forms x networks below 257 nodes: no test of the project runs them there and the issue does not ask for it; the
    small populations reach them inside a 320-node network whose other rows are all NaN ('padded320-*': pop stays 1 .. 40).

Bounds.  Table forms: <= 1 ulp of the exact value wherever it is a normal double (the kernel's own claim), the same bits from all
four readers.  Per-element form: relative error <= 1e-6 for exact p >= 1e-290 (the project's tolerance for this path).  All
forms: p == 1 at the bottom of the support, 0 <= p <= 1, never NaN, non-increasing in x; exact p subnormal or 0 -> p <= 1e-300 and
NES inf or >= 300; NES against -log10 of the exact value (rtol 1e-6, atol 1e-9); nes_binary decided on the exact rational at
thresholds 0.05 and 1e-100 (cells within 1e-6 relative of the threshold are left out, except p == threshold exactly: not
enriched in the table forms); num_neighborhoods_enriched = the column sums of that matrix."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hyp_cases as hc
import hyp_exact as hx

pytestmark = pytest.mark.gpu

FORMS = {
    'bits': ({'SAFE_HIP_COUNTS': 'bits'}, 'k_counts_bits<hypergeom>'),
    'mfma': ({'SAFE_HIP_COUNTS': 'mfma'}, 'k_hyp_emit'),
    'mfma-nolds': ({'SAFE_HIP_COUNTS': 'mfma', 'SAFE_HIP_EMIT_LDS_KB': '0'}, 'k_hyp_emit'),
    'mfma-fused': ({'SAFE_HIP_COUNTS': 'mfma', 'SAFE_HIP_HYP_SPLIT': '0'}, 'k_permtest_mfma<counts>'),
    'per-element': ({'SAFE_HIP_HYPER_TABLE': '0'}, 'k_hypergeom_tail'),
}
SWITCHES = ('SAFE_HIP_COUNTS', 'SAFE_HIP_EMIT_LDS_KB', 'SAFE_HIP_HYP_SPLIT', 'SAFE_HIP_HYPER_TABLE', 'SAFE_HIP_FORCE_PATH')
THRESHOLDS = {0.05: Fraction(1, 20), 1e-100: Fraction(1, 10 ** 100)}
WORST = {}                                                      # (family, form) -> worst ulp error seen (printed)


def forms_of(case):
    if not case.table_ok:
        return ['per-element']
    if case.n_total < 257:
        return ['bits', 'per-element']
    return list(FORMS)


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


class Cells:
    """The checked cells of a case grouped by their (K, n, x): index arrays and the exact values, built once per case."""

    def __init__(self, case, a, b):
        pop, K, n, x = case.recomputed(a, b)
        dK, dn, dx = case.designed()
        assert pop == case.pop and np.array_equal(K, dK) and np.array_equal(n, dn) and np.array_equal(x, dx), \
            'the arrays do not hold the designed parameters'
        assert int(a.sum(axis=1).max()) == case.max_row_count
        self.triples = case.triples()
        index = {t: i for i, t in enumerate(self.triples)}
        kk = np.broadcast_to(K[None, :], x.shape)
        nn = np.broadcast_to(n[:, None], x.shape)
        self.idx = np.array([index[t] for t in zip(kk.ravel().tolist(), nn.ravel().tolist(), x.ravel().tolist())]).reshape(x.shape)
        flat = self.idx.ravel()
        self.order = np.argsort(flat, kind='stable')
        self.starts = np.searchsorted(flat[self.order], np.arange(len(self.triples)))
        self.exact = [hx.exact_tail(pop, *t) for t in self.triples]
        self.want_nes = [hx.neg_log10(e) for e in self.exact]

    def per_triple(self, rows_matrix):
        """One value per (K, n, x) from a [checked rows, M] matrix; all cells of a triple must hold the same bits."""
        v = rows_matrix.ravel()[self.order]
        low, high = np.minimum.reduceat(v, self.starts), np.maximum.reduceat(v, self.starts)
        same = (low == high) | (np.isnan(low) & np.isnan(high))
        assert same.all(), 'cells with the same (K, n, x) differ: %s' % [self.triples[i] for i in np.nonzero(~same)[0][:5]]
        return low


def check_form(case, cells, form, p_full, nes_full, nb_full, enriched, thr, errors):
    table = form != 'per-element'
    rows = case.checked_rows
    say = lambda msg: errors.append('%s / %s / threshold %g: %s' % (case.name, form, thr, msg))   # noqa: E731
    if np.isnan(p_full).any() or not ((p_full >= 0) & (p_full <= 1)).all():
        say('p outside [0, 1] or NaN')
    # every row of a size group is the same neighborhood: the same output row
    groups = {}
    for i, r in enumerate(case.rows):
        groups.setdefault(r, []).append(i)
    for r, members in groups.items():
        for full in (p_full, nes_full, nb_full):
            if not (full[members] == full[members[0]]).all():
                say('rows of neighborhood size %s differ from each other' % (r,))
                break
    p = cells.per_triple(p_full[rows])
    nes = cells.per_triple(nes_full[rows])
    nb = cells.per_triple(nb_full[rows])
    thr_q = THRESHOLDS[thr]
    worst, excluded = 0.0, False
    want_nb = np.zeros(len(cells.triples))
    prev = None
    for i, (t, e) in enumerate(zip(cells.triples, cells.exact)):
        K, n, x = t
        lo, hi = hx.support(case.pop, K, n)
        got = float(p[i])
        cell = '(pop=%d K=%d n=%d x=%d) exact %.17g got %.17g' % (case.pop, K, n, x, float(e), got)
        if prev is not None and prev[0][:2] == (K, n) and got > prev[1]:
            say('p rises with x at ' + cell)
        prev = (t, got)
        if x <= lo and got != 1.0:
            say('p != 1 at the bottom of the support ' + cell)
        normal = float(e) >= 2.2250738585072014e-308
        checked_value = normal if table else e >= Fraction(1, 10 ** 290)
        if normal:
            err = hx.ulp_error(got, e)
            worst = max(worst, err) if checked_value else worst
            if table and err > 1.0:
                say('%.3g ulp off at %s' % (err, cell))
            if not table and checked_value and abs(Fraction(got) - e) > e / 10 ** 6:
                say('relative error %.3g at %s' % (float(abs(Fraction(got) - e) / e), cell))
            if not table and not checked_value and got > 1.0000011e-290:
                say('p above 1e-290 at ' + cell)
        else:
            if not 0.0 <= got <= 1e-300:
                say('exact p subnormal or 0, got above 1e-300 at ' + cell)
            if not (nes[i] == math.inf or nes[i] >= 300.0):
                say('NES %r for a subnormal p at %s' % (nes[i], cell))
        if checked_value and abs(nes[i] - cells.want_nes[i]) > 1e-9 + 1e-6 * abs(cells.want_nes[i]):
            say('NES %r, exact %r at %s' % (nes[i], cells.want_nes[i], cell))
        if abs(e - thr_q) <= thr_q / 10 ** 6:
            if e == thr_q and table:
                if nb[i] != 0.0:
                    say('p exactly on the threshold is enriched at ' + cell)
            else:
                excluded = True
                want_nb[i] = nb[i]
        else:
            want_nb[i] = 1.0 if e < thr_q else 0.0
            if nb[i] != want_nb[i]:
                say('nes_binary %r, exact decision %r at %s' % (nb[i], want_nb[i], cell))
    if not np.array_equal(enriched, nb_full.sum(axis=0)):
        say('num_neighborhoods_enriched is not the column sum of nes_binary')
    if not excluded:
        first_checked = {case.rows[i]: k for k, i in reversed(list(enumerate(rows)))}
        want = np.zeros(nb_full.shape[1])
        for r, members in groups.items():
            want += len(members) * want_nb[cells.idx[first_checked[r]]]
        if not np.array_equal(enriched, want):
            say('num_neighborhoods_enriched differs from the exact decisions in %d columns' % int((enriched != want).sum()))
    return worst, p


@pytest.mark.parametrize('case', hc.all_cases(), ids=repr)
def test_hypergeometric_p_against_exact_tails(amd, ctx, monkeypatch, case):
    a, b = case.arrays()
    cells = Cells(case, a, b)
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(np.random.default_rng(1).uniform(size=(case.n_total, 2)))
    sf.neighborhoods = a
    sf.load_attributes(attribute_file=b)
    errors, table_bits = [], {}
    thresholds = [0.05, 1e-100] if case.family in (2, 5) else [0.05]
    try:
        for form in forms_of(case):
            env, kernel = FORMS[form]
            for name in SWITCHES:
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            for thr in thresholds:
                sf.enrichment_threshold = thr
                sf.compute_pvalues()
                assert ctx.last_kernel()[0] == kernel, (case.name, form, ctx.last_kernel()[0])
                p_full, nes_full, nb_full = np.array(sf.pvalues_pos), np.array(sf.nes), np.array(sf.nes_binary)
                enriched = np.asarray(sf.attributes['num_neighborhoods_enriched'].values, dtype=np.float64)
                worst, p = check_form(case, cells, form, p_full, nes_full, nb_full, enriched, thr, errors)
                WORST[(case.family, form)] = max(WORST.get((case.family, form), 0.0), worst)
                if form != 'per-element':
                    table_bits[(form, thr)] = p_full
            print('%s / %s: worst ulp error %.3g over %d distinct (K, n, x)' % (case.name, form, worst, len(cells.triples)))
    finally:
        sf.enrichment_threshold = 0.05
        sf.neighborhoods = None                                 # gives the device copy of the membership back
    keys = list(table_bits)
    for k in keys[1:]:                                          # one table, four readers (and the threshold does not enter p)
        if not np.array_equal(table_bits[keys[0]], table_bits[k]):
            errors.append('%s: p of %s and %s differ in %d cells' % (case.name, keys[0], k, int((table_bits[keys[0]] != table_bits[k]).sum())))
    assert not errors, '%d findings, first ones:\n%s' % (len(errors), '\n'.join(errors[:25]))


def test_zz_worst_errors_per_family_and_form():
    """Prints the figures DESIGN.md quotes (run with -s); SciPy's own, on the same cells, come from tests/test_hyp_exact_cpu.py."""
    for (family, form), worst in sorted(WORST.items()):
        print('family %d / %-11s worst ulp error %.3g' % (family, form, worst))
