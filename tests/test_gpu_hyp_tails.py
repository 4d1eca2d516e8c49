"""safe_hypergeom_tails, safe_hypergeom_outputs and safe_fdr_adjust_rows (include/safe_hip.h; safepy_amd/csrc/hyptails.hip,
fdr.hip) on the device: both hypergeometric tails of every designed cell of tests/hyp_cases.py against the EXACT rationals
(tests/hyp_exact.py, tests/hyp_tails_ref.py), through both evaluators.  Needs an MI355X.

Inputs.  Every case runs twice: its own (a, b), and its mirror (a, 1 - b) with NaN kept -- K -> pop - K, x -> n - x -- which puts
the designed deep upper tails, down to the subnormals, on the LOWER side.  The mirror's exact tails are the case's own with the
sides swapped (P[H <= x | K] = P[H' >= n - x | pop - K]; tests/test_hyp_tails_ref_cpu.py proves the identity on every triple).

Bounds.  Table evaluator: both tails <= 1 ulp of the exact value wherever it is a normal double (the bound k_hyp_table is held
to; the arithmetic is the same).  Per-element evaluator: relative error <= 1e-6 for exact p >= 1e-290 (the project's bound for
hyp_sf).  Both: 0 <= p <= 1, never NaN; pvalues_pos non-increasing and pvalues_neg non-decreasing in x; p_neg == 1 at the top
of the support, p_pos == 1 at its bottom; p_pos + p_neg >= 1; an exact tail that is subnormal or 0 gives p <= 1e-300; rows of
one neighborhood are bit-equal.  NES against -log10 of the exact values (rtol 1e-6, atol 1e-9, infinities equal; for 'both',
cells whose two tails are both within 1e-12 of 1 are skipped).  nes_binary decided on the exact rationals at thresholds 0.05 and
1e-100 -- all three signs on families 1, 3, 4 and 'deep-N1000', 'both' on everything else -- leaving out cells within 1e-6
(relative) of a threshold (for 'both': of thr and 1 / thr as ratios p_neg / p_pos) except p == threshold exactly, which is kept
and not enriched for the table evaluator.  (The per-element evaluator is held to 1e-6 relative on p, which cannot decide a cell
that sits ON the threshold: at pop = 6, K = 3, n = 3, x = 3, exact p = 1 / 20, hyp_sf returns 0.049999999999999961 and the
cell comes out enriched (measured on an MI355X; 0.050000000000000031 at pop = 20, K = n = x = 1).  For that evaluator such cells are left out like the rest of the band and what it returned is printed
-- the rule tests/test_gpu_hypergeom_exact.py applies to k_hypergeom_tail.)  The left-out cells are counted per (input, sign, threshold) and may be at most 0.5 % of the distinct triples
(test_zz_left_out_cells_stay_rare).  num_neighborhoods_enriched = the column sums of the returned nes_binary."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import hyp_cases as hc
import hyp_exact as hx
import hyp_tails_ref as ht

pytestmark = pytest.mark.gpu

THRESHOLDS = {0.05: Fraction(1, 20), 1e-100: Fraction(1, 10 ** 100)}
EVALUATORS = {'table': 'k_hyp_tails_emit<table>', 'element': 'k_hyp_tails_emit<element>'}
SMALLEST_NORMAL = 2.2250738585072014e-308
ROW_TILE = 16                                                   # TAILS_ROW_TILE of hyptails.hip
LEFT_OUT = {}                                                   # (input, sign, threshold) -> [left-out triples, triples]
WORST = {}                                                      # (evaluator, side) -> worst error seen (ulp / relative)


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


def run_tails(be, ctx, nbr, attr, sign, thr, evaluator, col0=0, col1=None, guard=0):
    """One safe_hypergeom_tails call: ({name: array}, kernel name).  guard > 0: every output buffer is `guard` doubles longer,
    filled with a pattern the call must leave alone."""
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    names = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'num_enriched')
    sizes = [n * m] * 5 + [m]
    bufs = [ctx.alloc_f64(s + guard) for s in sizes]
    poison = np.full(max(sizes) + guard, -12345.678)
    try:
        for b, s in zip(bufs, sizes):
            b.upload(poison[:s + guard])
        be.hypergeom_tails(ctx, nbr, attr, sign, thr, [b.ptr for b in bufs], col0, col1, evaluator)
        kernel = ctx.last_kernel()[0]
        out = {}
        for name, b, s in zip(names, bufs, sizes):
            flat = b.download((s + guard,))
            assert (flat[s:] == -12345.678).all(), '%s: the call wrote past the end of its output' % name
            out[name] = flat[:s].reshape((m,) if name == 'num_enriched' else (n, m)).copy()
    finally:
        for b in bufs:
            b.free()
    return out, kernel


class Cells:
    """The checked cells of one input of a case grouped by their (K, n, x), with the exact tails of each triple."""

    def __init__(self, case, mirrored):
        K, n, x = case.designed()
        own = sorted(set(zip(np.broadcast_to(K[None, :], x.shape).ravel().tolist(), np.broadcast_to(n[:, None], x.shape).ravel().tolist(),
                             x.ravel().tolist())))
        e_up = {t: hx.exact_tail(case.pop, *t) for t in own}
        e_low = {t: ht.exact_lower_tail(case.pop, *t) for t in own}
        if mirrored:                                            # (K, n, x) -> (pop - K, n, n - x): the tails swap sides
            K, x = case.pop - K, n[:, None] - x
            e_up, e_low = ({(case.pop - k, nn, nn - xx): v for (k, nn, xx), v in d.items()} for d in (e_low, e_up))
        self.K, self.n, self.x = K, n, x
        self.triples = sorted(e_up)
        index = {t: i for i, t in enumerate(self.triples)}
        kk, nn = np.broadcast_to(K[None, :], x.shape), np.broadcast_to(n[:, None], x.shape)
        flat = np.array([index[t] for t in zip(kk.ravel().tolist(), nn.ravel().tolist(), x.ravel().tolist())])
        self.order = np.argsort(flat, kind='stable')
        self.starts = np.searchsorted(flat[self.order], np.arange(len(self.triples)))
        self.e_pos = [e_up[t] for t in self.triples]
        self.e_neg = [e_low[t] for t in self.triples]
        self.f_pos = np.array([float(e) for e in self.e_pos])    # the exact values correctly rounded
        self.f_neg = np.array([float(e) for e in self.e_neg])
        self.nes_pos = np.array([hx.neg_log10(e) for e in self.e_pos])
        self.nes_neg = np.array([hx.neg_log10(e) for e in self.e_neg])
        tk, tn, tx = (np.array(v, dtype=np.int64) for v in zip(*self.triples))
        self.same_kn = (tk[1:] == tk[:-1]) & (tn[1:] == tn[:-1])            # consecutive triples of one (K, n): x rises
        self.at_bottom = tx <= np.maximum(0, tn + tk - case.pop)
        self.at_top = tx >= np.minimum(tk, tn)
        self.decisions = {}

    def per_triple(self, rows_matrix, what):
        v = rows_matrix.ravel()[self.order]
        low, high = np.minimum.reduceat(v, self.starts), np.maximum.reduceat(v, self.starts)
        same = (low == high) | (np.isnan(low) & np.isnan(high))
        assert same.all(), '%s: cells with the same (K, n, x) differ: %s' % (what, [self.triples[i] for i in np.nonzero(~same)[0][:5]])
        return low

    def decision(self, sign, thr):
        """(wanted nes_binary, left out, exact p == threshold) per triple, decided on the exact rationals."""
        if (sign, thr) not in self.decisions:
            got = [ht.exact_decision(ep, en, sign, THRESHOLDS[thr]) for ep, en in zip(self.e_pos, self.e_neg)]
            side = {'highest': self.e_pos, 'lowest': self.e_neg, 'both': []}[sign]
            on_thr = np.array([e == THRESHOLDS[thr] for e in side] or [False] * len(got))
            self.decisions[(sign, thr)] = (np.array([float(g[0]) for g in got]), np.array([g[1] for g in got]), on_thr)
        return self.decisions[(sign, thr)]


def check_values(case, cells, evaluator, out, say):
    """The p matrices of one call against the exact tails; returns (p_pos, p_neg) per triple."""
    rows = case.checked_rows
    pp_full, pn_full = out['pvalues_pos'], out['pvalues_neg']
    for name, full in (('pvalues_pos', pp_full), ('pvalues_neg', pn_full)):
        if np.isnan(full).any() or not ((full >= 0) & (full <= 1)).all():
            say('%s outside [0, 1] or NaN' % name)
    if not (pp_full + pn_full >= 1.0).all():
        say('p_pos + p_neg < 1 in %d cells' % int((pp_full + pn_full < 1.0).sum()))
    if not np.array_equal(out['ns'][rows], cells.x.astype(np.float64)):
        say('ns is not the designed x')
    groups = {}
    for i, r in enumerate(case.rows):
        groups.setdefault(r, []).append(i)
    for r, members in groups.items():
        for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
            if not (out[name][members] == out[name][members[0]]).all():
                say('%s: rows of neighborhood size %s differ from each other' % (name, r))
    pp = cells.per_triple(pp_full[rows], 'pvalues_pos')
    pn = cells.per_triple(pn_full[rows], 'pvalues_neg')
    if (pp[1:][cells.same_kn] > pp[:-1][cells.same_kn]).any():
        say('pvalues_pos rises with x')
    if (pn[1:][cells.same_kn] < pn[:-1][cells.same_kn]).any():
        say('pvalues_neg falls with x')
    if not (pp[cells.at_bottom] == 1.0).all():
        say('p_pos != 1 at the bottom of a support')
    if not (pn[cells.at_top] == 1.0).all():
        say('p_neg != 1 at the top of a support')
    for side, got, exact, rounded in (('pos', pp, cells.e_pos, cells.f_pos), ('neg', pn, cells.e_neg, cells.f_neg)):
        tiny = rounded < SMALLEST_NORMAL
        if not (got[tiny] <= 1e-300).all():
            say('p_%s above 1e-300 where the exact tail is subnormal or 0' % side)
        if evaluator == 'table':
            suspects = np.nonzero(~tiny & (got != rounded))[0]              # (got == the correctly rounded value: <= 0.5 ulp)
            worst = 0.5 if (~tiny).any() else 0.0
            for i in suspects:
                err = hx.ulp_error(got[i], exact[i])
                worst = max(worst, err)
                if err > 1.0:
                    say('p_%s %.3g ulp off at (pop=%d K=%d n=%d x=%d): exact %.17g got %.17g'
                        % ((side, err, case.pop) + cells.triples[i] + (rounded[i], got[i])))
        else:
            checked = rounded >= 0.99e-290
            with np.errstate(divide='ignore', invalid='ignore'):
                rel = np.where(checked, np.abs(got - rounded) / rounded, 0.0)
            worst = float(rel.max()) if len(rel) else 0.0
            for i in np.nonzero(rel > 0.9e-6)[0]:                           # (the exact comparison only where it can matter)
                if exact[i] >= Fraction(1, 10 ** 290) and abs(Fraction(float(got[i])) - exact[i]) > exact[i] / 10 ** 6:
                    say('p_%s relative error %.3g at (pop=%d K=%d n=%d x=%d)' % ((side, rel[i], case.pop) + cells.triples[i]))
        WORST[(evaluator, side)] = max(WORST.get((evaluator, side), 0.0), worst)
    return pp, pn


def check_nes(case, cells, evaluator, sign, thr, out, tag, say):
    rows = case.checked_rows
    nes = cells.per_triple(out['nes'][rows], 'nes')
    nb = cells.per_triple(out['nes_binary'][rows], 'nes_binary')
    floor = SMALLEST_NORMAL if evaluator == 'table' else 1e-290              # where the p-value itself is held to a bound
    ok_pos, ok_neg = cells.f_pos >= floor, cells.f_neg >= floor
    with np.errstate(invalid='ignore'):
        want = {'highest': cells.nes_pos, 'lowest': cells.nes_neg, 'both': cells.nes_pos - cells.nes_neg}[sign]
    checked = {'highest': ok_pos, 'lowest': ok_neg, 'both': ok_pos & ok_neg}[sign]
    if sign == 'both':
        checked = checked & ~((np.abs(cells.f_pos - 1.0) <= 1e-12) & (np.abs(cells.f_neg - 1.0) <= 1e-12))
    bad = checked & ~(np.abs(nes - want) <= 1e-9 + 1e-6 * np.abs(want))
    for i in np.nonzero(bad)[0][:3]:
        say('NES %r, exact %r at (K=%d n=%d x=%d)' % ((nes[i], want[i]) + cells.triples[i]))
    zero_pos, zero_neg = cells.f_pos == 0.0, cells.f_neg == 0.0             # an exact tail of 0: the infinities are equal
    for mask, value in {'highest': [(zero_pos, np.inf)], 'lowest': [(zero_neg, np.inf)],
                        'both': [(zero_pos & ~zero_neg, np.inf), (zero_neg & ~zero_pos, -np.inf)]}[sign]:
        exact_zero = mask & np.array([e == 0 for e in (cells.e_pos if value > 0 else cells.e_neg)])
        if not (nes[exact_zero] == value).all():
            say('NES is not %r where the exact tail is 0' % value)
    if sign != 'both':                                                       # a subnormal tail: NES inf or >= 300
        tiny = (cells.f_pos if sign == 'highest' else cells.f_neg) < SMALLEST_NORMAL
        if not ((nes[tiny] == np.inf) | (nes[tiny] >= 300.0)).all():
            say('NES below 300 for a subnormal tail')
    want_nb, left_out, on_thr = cells.decision(sign, thr)
    if evaluator == 'element' and on_thr.any():
        # Exact p == threshold is decided by the table evaluator alone (module docstring): hyp_sf is held to 1e-6 relative, and
        # a value a few ulp below 1 / 20 is enriched.  What it returned is printed for the record.
        p_side = cells.per_triple(out['pvalues_pos' if sign == 'highest' else 'pvalues_neg'][rows], 'p')
        for i in np.nonzero(on_thr)[0]:
            print('%s / element / %s: exact p == %g at (K=%d n=%d x=%d), returned %.17g, nes_binary %g'
                  % ((case.name, sign, thr) + cells.triples[i] + (p_side[i], nb[i])))
        left_out = left_out | on_thr
    count = LEFT_OUT.setdefault((tag, sign, thr), {})
    count[case.name] = (int(left_out.sum()), len(left_out))
    wrong = ~left_out & (nb != want_nb)
    for i in np.nonzero(wrong)[0][:3]:
        say('nes_binary %r, exact decision %r at (K=%d n=%d x=%d), exact p_pos %.17g p_neg %.17g'
            % ((nb[i], want_nb[i]) + cells.triples[i] + (cells.f_pos[i], cells.f_neg[i])))
    if not np.array_equal(out['num_enriched'], out['nes_binary'].sum(axis=0)):
        say('num_neighborhoods_enriched is not the column sum of nes_binary')


def signs_of(case):
    return ht.SIGNS if case.family in (1, 3, 4) or case.name == 'deep-N1000' else ('both',)


@pytest.mark.parametrize('case', hc.all_cases(), ids=repr)
def test_both_tails_against_exact_rationals(be, ctx, case):
    a, b = case.arrays()
    errors = []
    nbr = be.Neighborhoods.from_dense(ctx, a)
    del a
    try:
        for tag, values in (('own', b), ('mirrored', ht.mirror(b))):
            cells = Cells(case, tag == 'mirrored')
            attr = be.Attributes.from_host(ctx, values)
            try:
                p_seen = {}
                for evaluator, kernel in EVALUATORS.items():
                    first = True
                    for sign in signs_of(case):
                        for thr in THRESHOLDS:
                            say = lambda msg: errors.append('%s / %s / %s / %s / %g: %s' % (case.name, tag, evaluator, sign, thr, msg))   # noqa: E731
                            try:
                                out, name = run_tails(be, ctx, nbr, attr, sign, thr, evaluator)
                            except be._lib.SafeHipError as err:
                                assert evaluator == 'table' and err.code == be._lib.E_UNSUPPORTED, err
                                break                                      # the size rule declines the table for this call
                            assert name == kernel, (case.name, evaluator, name)
                            if first:
                                p_seen[evaluator] = check_values(case, cells, evaluator, out, say)
                                first = False
                                p_first = (out['pvalues_pos'], out['pvalues_neg'], out['ns'])
                            else:                                          # neither the sign nor the threshold enters p
                                for x, y in zip(p_first, (out['pvalues_pos'], out['pvalues_neg'], out['ns'])):
                                    if not np.array_equal(x, y):
                                        say('p or ns changes with the sign or the threshold')
                            check_nes(case, cells, evaluator, sign, thr, out, tag, say)
                        else:
                            continue
                        break
                print('%s / %s: evaluators run %s, %d distinct (K, n, x)' % (case.name, tag, sorted(p_seen), len(cells.triples)))
                assert 'element' in p_seen
            finally:
                attr.close()
    finally:
        nbr.close()
    assert not errors, '%d findings, first ones:\n%s' % (len(errors), '\n'.join(errors[:25]))


def test_zz_left_out_cells_stay_rare():
    """At most 0.5 % of the distinct triples per (input, sign, threshold) sit so close to a threshold that nes_binary is not
    checked there (counted over the cases that ran; figures printed with -s)."""
    for key, per_case in sorted(LEFT_OUT.items(), key=repr):
        left, total = (sum(v[i] for v in per_case.values()) for i in (0, 1))
        print('%-9s %-8s %-7g left out %d of %d distinct (K, n, x)' % (key + (left, total)))
        if len(per_case) == len(hc.all_cases()) or total > 5000:
            assert left <= 0.005 * total, key
    for key, worst in sorted(WORST.items()):
        print('worst %s error, evaluator %s, p_%s: %.3g' % (('ulp' if key[0] == 'table' else 'relative',) + key + (worst,)))


# ------------------------------------------------------------------------------------------ shapes of the emit kernel ----

def shaped_input(n_rows, m, sizes=None):
    """A designed input of n_rows nodes (the last one all NaN, a member of every second neighborhood) and m columns: rows cycle
    through two neighborhood sizes, columns through three annotation counts at moving offsets.  (a, b, pop, K, n, x)."""
    pop = n_rows - 1
    sizes = sizes or [(min(3, pop), 0), (max(pop - 2, 0), 1)]
    Ks = [min(1, pop), min(4, pop), pop // 2]
    a = np.zeros((n_rows, n_rows), dtype=np.int64)
    nn = np.zeros(n_rows, dtype=np.int64)
    for i in range(n_rows):
        ni, gi = sizes[i % len(sizes)]
        a[i, :ni] = 1
        a[i, pop:pop + gi] = 1
        nn[i] = ni
    b = np.zeros((n_rows, m))
    K = np.array([Ks[j % 3] for j in range(m)], dtype=np.int64)
    s = np.array([(5 * j) % (pop - K[j] + 1) for j in range(m)], dtype=np.int64)
    for j in range(m):
        b[s[j]:s[j] + K[j], j] = 1.0
    b[pop:] = np.nan
    x = np.clip(nn[:, None] - s[None, :], 0, K[None, :])
    return a, b, pop, K, nn, x


def exact_matrices(pop, K, n, x):
    up = np.array([[float(hx.exact_tail(pop, int(K[j]), int(n[i]), int(x[i, j]))) for j in range(len(K))] for i in range(len(n))])
    low = np.array([[float(ht.exact_lower_tail(pop, int(K[j]), int(n[i]), int(x[i, j]))) for j in range(len(K))] for i in range(len(n))])
    return up, low


def check_against_floats(out, up, low, x, evaluator, sign, thr, what):
    """A small call against the correctly rounded exact tails: the evaluator's bound on p, then NES / nes_binary / counts from
    the RETURNED p through the NumPy restatement (away from the threshold band)."""
    assert np.array_equal(out['ns'], x.astype(np.float64)), what
    for got, want in ((out['pvalues_pos'], up), (out['pvalues_neg'], low)):
        if evaluator == 'table':
            assert (np.abs(got - want) <= np.spacing(want)).all(), what
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=what)
    nes, nb, counts = ht.outputs(out['pvalues_pos'], out['pvalues_neg'], sign, thr)
    np.testing.assert_allclose(out['nes'], nes, rtol=1e-6, atol=1e-9, err_msg=what)
    edge = np.abs(np.abs(nes) + np.log10(thr)) <= 1e-6
    assert np.array_equal(out['nes_binary'][~edge], nb[~edge]), what
    assert np.array_equal(out['num_enriched'], out['nes_binary'].sum(axis=0)), what


@pytest.mark.parametrize('n_rows', [ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE + 1])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 129])
def test_shapes_and_column_ranges(be, ctx, n_rows, m):
    """Column counts around the 64 lanes, row counts around the row tile, whole matrices and [col0, col1) sub-ranges of a wider
    matrix whose other columns hold other data; every output buffer has a guard band behind it."""
    wide = m + 3
    a, b, pop, K, n, x = shaped_input(n_rows, wide)
    b[:pop, 0] = 1.0                                            # the neighbours of the sub-range [2, 2 + m): all ones, and a
    b[:pop, wide - 1] = (np.arange(pop) % 2).astype(np.float64)    # column of its own
    nbr = be.Neighborhoods.from_dense(ctx, a)
    whole = be.Attributes.from_host(ctx, np.ascontiguousarray(b[:, 2:2 + m]))
    part = be.Attributes.from_host(ctx, b)
    up, low = exact_matrices(pop, K[2:2 + m], n, x[:, 2:2 + m])
    try:
        for evaluator, kernel in EVALUATORS.items():
            for k, sign in enumerate(ht.SIGNS):
                thr = (0.05, 0.3, 0.05)[k]
                ref, name = run_tails(be, ctx, nbr, whole, sign, thr, evaluator, guard=64)
                assert name == kernel
                check_against_floats(ref, up, low, x[:, 2:2 + m], evaluator, sign, thr, (n_rows, m, evaluator, sign, 'whole'))
                got, name = run_tails(be, ctx, nbr, part, sign, thr, evaluator, col0=2, col1=2 + m, guard=64)
                assert name == kernel
                for key in ref:
                    assert np.array_equal(got[key], ref[key]), (n_rows, m, evaluator, sign, key, 'sub-range differs from the whole matrix')
    finally:
        whole.close()
        part.close()
        nbr.close()


def test_one_node_and_empty_rows_and_columns(be, ctx):
    """pop = 1; K = 0 columns, n = 0 rows (a neighborhood of all-NaN nodes only), K = pop columns."""
    for a, b in [(np.ones((1, 1), dtype=np.int64), np.ones((1, 1))), (np.ones((1, 1), dtype=np.int64), np.zeros((1, 1)))]:
        nbr, attr = be.Neighborhoods.from_dense(ctx, a), be.Attributes.from_host(ctx, b)
        try:
            with pytest.raises(be._lib.SafeHipError):           # (one cell: the size rule declines the table)
                run_tails(be, ctx, nbr, attr, 'both', 0.05, 'table')
            for evaluator in (None, 'element'):
                out, name = run_tails(be, ctx, nbr, attr, 'both', 0.05, evaluator, guard=8)
                assert name == EVALUATORS['element']
                for key, want in (('ns', b[0, 0]), ('pvalues_pos', 1.0), ('pvalues_neg', 1.0), ('nes', 0.0), ('nes_binary', 0.0)):
                    assert out[key][0, 0] == want, (evaluator, key)
                assert out['num_enriched'][0] == 0.0
        finally:
            attr.close()
            nbr.close()
    n_rows, m = 20, 8
    a, b, pop, K, n, x = shaped_input(n_rows, m, sizes=[(0, 1), (5, 0), (n_rows - 1, 1), (0, 0)])
    b[:pop, 0], b[:pop, 1] = 0.0, 1.0                           # K = 0 and K = pop
    K[0], K[1] = 0, pop
    x[:, 0], x[:, 1] = 0, n
    up, low = exact_matrices(pop, K, n, x)
    assert (up[:, 0] == 1).all() and (low[:, 0] == 1).all() and (up[n == 0] == 1).all() and (low[n == 0] == 1).all()
    nbr, attr = be.Neighborhoods.from_dense(ctx, a), be.Attributes.from_host(ctx, b)
    try:
        for evaluator in EVALUATORS:
            for sign in ht.SIGNS:
                out, _ = run_tails(be, ctx, nbr, attr, sign, 0.05, evaluator, guard=8)
                check_against_floats(out, up, low, x, evaluator, sign, 0.05, (evaluator, sign))
    finally:
        attr.close()
        nbr.close()


def test_table_declined_for_48_sizes_times_48_counts(be, ctx):
    """48 nodes, 48 distinct neighborhood sizes x 48 distinct annotation counts: 4 * 2304 pairs > 2304 cells, so the rule
    declines the table: evaluator 0 runs per element, evaluator 1 says SAFE_E_UNSUPPORTED."""
    pop = 48
    a = np.tril(np.ones((pop, pop), dtype=np.int64))            # row i: the first i + 1 nodes
    b = np.triu(np.ones((pop, pop)))                            # column j: ones on the first j + 1 nodes
    n, K = np.arange(1, pop + 1), np.arange(1, pop + 1)
    x = np.minimum(n[:, None], K[None, :])
    nbr, attr = be.Neighborhoods.from_dense(ctx, a), be.Attributes.from_host(ctx, b)
    try:
        with pytest.raises(be._lib.SafeHipError) as err:
            run_tails(be, ctx, nbr, attr, 'both', 0.05, 'table')
        assert err.value.code == be._lib.E_UNSUPPORTED
        out, name = run_tails(be, ctx, nbr, attr, 'both', 0.05, None, guard=8)
        assert name == EVALUATORS['element']
        up, low = exact_matrices(pop, K, n, x)
        check_against_floats(out, up, low, x, 'element', 'both', 0.05, 'declined table')
        assert (out['pvalues_neg'] == 1.0).all()                # every cell sits at the top of its support
    finally:
        attr.close()
        nbr.close()


# ----------------------------------------------------------------------------- safe_hypergeom_outputs on designed p ----

def p_cut(thr):
    """nes_p_cut of common.h: the smallest double whose -log10 does not exceed -log10(thr)."""
    bound = -np.log10(thr)
    p = np.float64(thr)
    while -np.log10(p) > bound:
        p = np.nextafter(p, 1.0)
    while not -np.log10(np.nextafter(p, 0.0)) > bound:
        p = np.nextafter(p, 0.0)
    return p


def designed_pairs(thr):
    cut = p_cut(thr)
    singles = [0.0, 1.0, np.nan, 5e-324, 1e-310, SMALLEST_NORMAL, cut, np.nextafter(cut, 0.0), np.nextafter(cut, 1.0), thr, 0.5, 1e-300, 0.999]
    # the other side is never 1 next to a value at the cut: 'both' would then decide on the device's own log10 of that value,
    # one rounding away from NumPy's; the one-sided decisions at the cut do not depend on the other side
    pairs = [(p, q) for p in singles for q in (0.5, 0.0, np.nan)] + [(0.5, p) for p in singles]
    pairs += [(0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.5, 1.0), (1.0, 0.5), (1e-300, 1.0), (1.0, 1e-300), (5e-324, 1.0)]
    for base in (1.0, 0.37, 1e-5, 1e-200):                      # p_neg / p_pos on both sides of thr and of 1 / thr
        for ratio in (thr * (1 - 1e-7), thr * (1 + 1e-7)):
            pairs += [(base, base * ratio), (base * ratio, base)]
    return pairs


@pytest.mark.parametrize('shape', [(63, 65), (64, 64), (65, 63), (1, 1), (130, 129)])
def test_outputs_from_designed_p_matrices(be, ctx, shape):
    n, m = shape
    for thr in (0.05, 1e-100):
        pairs = designed_pairs(thr)
        idx = (np.arange(n * m) * 7 + 3) % len(pairs)
        p_pos = np.array([pairs[i][0] for i in idx]).reshape(n, m)
        p_neg = np.array([pairs[i][1] for i in idx]).reshape(n, m)
        bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
        try:
            bufs[0].upload(p_neg)
            bufs[1].upload(p_pos)
            for sign in ht.SIGNS:
                for b in bufs[2:4]:
                    b.upload(np.full((n, m), -7.0))
                be.hypergeom_outputs(ctx, n, m, sign, thr, bufs[0].ptr, bufs[1].ptr, [b.ptr for b in bufs[2:]])
                nes, nb = bufs[2].download((n, m)), bufs[3].download((n, m))
                counts = bufs[4].download((m,))
                want_nes, want_nb, want_counts = ht.outputs(p_pos, p_neg, sign, thr)
                np.testing.assert_allclose(nes, want_nes, rtol=1e-6, atol=1e-9, equal_nan=True, err_msg=str((shape, thr, sign)))
                assert np.array_equal(np.isnan(nes), np.isnan(want_nes)) and np.array_equal(np.isinf(nes), np.isinf(want_nes))
                assert np.array_equal(nb, want_nb), (shape, thr, sign, np.argwhere(nb != want_nb)[:5])
                assert np.array_equal(counts, want_counts), (shape, thr, sign)
                assert np.array_equal(bufs[0].download((n, m)), p_neg, equal_nan=True) and np.array_equal(bufs[1].download((n, m)), p_pos, equal_nan=True)
        finally:
            for b in bufs:
                b.free()


# ----------------------------------------------------------------------------------------------- safe_fdr_adjust_rows ----

@pytest.mark.parametrize('m', [1, 2, 257, 4373])
def test_fdr_adjust_rows_gives_the_bits_of_fdr_adjust(be, ctx, m):
    n = 5
    rng = np.random.default_rng(m)
    p = np.round(rng.uniform(size=(n, m)), 3)                   # (ties)
    p[1, ::3] = 0.0
    p[2, :] = 1.0
    p[3, m // 2] = 1e-300
    bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
    try:
        bufs[0].upload(p)
        bufs[1].upload(p)
        be.fdr_adjust_rows(ctx, n, m, bufs[0].ptr)
        be.fdr_adjust(ctx, n, m, 0, 'highest', 0.05, [None] + [b.ptr for b in bufs[1:]])
        got, want = bufs[0].download((n, m)), bufs[1].download((n, m))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert (got >= p).all() and (got <= 1).all()
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_refusals(be, ctx):
    a, b, pop, K, n, x = shaped_input(20, 10)
    nbr, attr = be.Neighborhoods.from_dense(ctx, a), be.Attributes.from_host(ctx, b)
    half = b.copy()
    half[3, 4] = 0.5
    bad = be.Attributes.from_host(ctx, half)
    lib, E = be._lib.lib, be._lib
    bufs = [ctx.alloc_f64(20, 10) for _ in range(5)] + [ctx.alloc_f64(10)]
    ptrs = [buf.ptr for buf in bufs]
    marker = np.full((20, 10), -3.0)

    def code(fn):
        with pytest.raises(be._lib.SafeHipError) as err:
            fn()
        return err.value.code

    def raw(sign, evaluator, thr=0.05):
        be.check(lib.safe_hypergeom_tails(ctx.handle, nbr.handle, attr.handle, sign, thr, evaluator, 0, 10, *[C.c_void_p(p) for p in ptrs]))

    try:
        for k in range(6):                                      # every output is needed
            assert code(lambda: be.hypergeom_tails(ctx, nbr, attr, 'both', 0.05, ptrs[:k] + [None] + ptrs[k + 1:])) == E.E_INVALID
        assert code(lambda: be.hypergeom_tails(ctx, nbr, attr, 'both', 0.05, ptrs, 0, 11)) == E.E_INVALID
        assert code(lambda: be.hypergeom_tails(ctx, nbr, attr, 'both', 0.05, ptrs, 5, 5)) == E.E_INVALID
        for thr in (0.0, 1.0, -0.5, float('nan')):
            assert code(lambda: raw(2, 0, thr)) == E.E_INVALID
        assert code(lambda: raw(3, 0)) == E.E_INVALID and code(lambda: raw(-1, 0)) == E.E_INVALID
        assert code(lambda: raw(2, 3)) == E.E_INVALID and code(lambda: raw(2, -1)) == E.E_INVALID
        for buf in bufs[:5]:
            buf.upload(marker)
        assert code(lambda: be.hypergeom_tails(ctx, nbr, bad, 'both', 0.05, ptrs)) == E.E_VALUE       # non-0/1 data ...
        for buf in bufs[:5]:
            assert np.array_equal(buf.download((20, 10)), marker)                                  # ... and nothing was written
        for k in range(3):
            assert code(lambda: be.hypergeom_outputs(ctx, 20, 10, 'both', 0.05, ptrs[1], ptrs[2], ptrs[3:3 + k] + [None] + ptrs[4 + k:])) == E.E_INVALID
        assert code(lambda: be.hypergeom_outputs(ctx, 20, 10, 'both', 0.05, None, ptrs[2], ptrs[3:])) == E.E_INVALID
        assert code(lambda: be.hypergeom_outputs(ctx, 0, 10, 'both', 0.05, ptrs[1], ptrs[2], ptrs[3:])) == E.E_INVALID
        assert code(lambda: be.hypergeom_outputs(ctx, 20, 10, 'both', 1.0, ptrs[1], ptrs[2], ptrs[3:])) == E.E_INVALID
        assert code(lambda: be.fdr_adjust_rows(ctx, 20, 10, None)) == E.E_INVALID
        assert code(lambda: be.fdr_adjust_rows(ctx, 20, 0, ptrs[0])) == E.E_INVALID
        run_tails(be, ctx, nbr, attr, 'both', 0.05, None)       # the context still works
    finally:
        for buf in bufs:
            buf.free()
        for h in (bad, attr, nbr):
            h.close()


# -------------------------------------------------------------------------------------------- a busy caller's stream ----

def test_entry_points_on_a_busy_caller_stream(be, ctx):
    """safe_hypergeom_tails and safe_hypergeom_outputs (+ safe_fdr_adjust_rows) on a caller's stream that is still busy
    producing their inputs, outputs poisoned: the same bits as a quiet run (the harness of tests/test_gpu_stream_order.py)."""
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    nbr = None
    try:
        a, b64, _, _, _, _ = shaped_input(301, 70)               # (two neighborhood sizes: the table rule accepts the call)
        n, m = b64.shape
        nbr = be.Neighborhoods.from_dense(ctx, a)
        a = a.astype(np.float64)

        def tails_call(evaluator):
            bor = so.Borrowed(lab, b64)
            attr = bor.handle(lab)
            outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(5)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]
            fn = lambda: be.hypergeom_tails(ctx, nbr, attr, 'both', 0.05, [o.data_ptr() for o in outs], evaluator=evaluator)   # noqa: E731

            def check(got):
                valid = (~np.isnan(b64)).any(axis=1)
                assert np.array_equal(got[0], a @ np.nan_to_num(b64))
                from scipy.stats import hypergeom
                N, K, nn = int(valid.sum()), np.nansum(b64, axis=0), a @ valid.astype(np.float64)
                np.testing.assert_allclose(got[2], hypergeom.sf(got[0] - 1, N, K[None, :], nn[:, None]), rtol=1e-6, atol=1e-300)
                np.testing.assert_allclose(got[1], hypergeom.cdf(got[0], N, K[None, :], nn[:, None]), rtol=1e-6, atol=1e-300)
                assert np.array_equal(got[5], got[4].sum(axis=0))
            return so.Call(['safe_hypergeom_tails'], [(bor.tensor, bor.staging)], outs, fn, check, done=attr.close)

        def outputs_call():
            rng = np.random.default_rng(5)
            host = [np.round(rng.uniform(size=(257, 70)), 2) for _ in range(2)]
            st = [torch.from_numpy(x).to('cuda') for x in host]
            dev = [torch.empty_like(x) for x in st]
            outs = [torch.empty((257, 70), dtype=torch.float64, device='cuda') for _ in range(2)] + [torch.empty((70,), dtype=torch.float64, device='cuda')]

            def fn():
                be.fdr_adjust_rows(ctx, 257, 70, dev[0].data_ptr())
                be.fdr_adjust_rows(ctx, 257, 70, dev[1].data_ptr())
                be.hypergeom_outputs(ctx, 257, 70, 'both', 0.05, dev[0].data_ptr(), dev[1].data_ptr(), [o.data_ptr() for o in outs])

            def check(got):
                from oracle import safe_oracle as orc
                qn, qp = orc.fdr_rows(host[0]), orc.fdr_rows(host[1])
                assert np.array_equal(got[0], qn) and np.array_equal(got[1], qp)
                nes, nb, counts = ht.outputs(qp, qn, 'both', 0.05)
                np.testing.assert_allclose(got[2], nes, rtol=1e-6, atol=1e-9)
                assert np.array_equal(got[4], got[3].sum(axis=0))
            return so.Call(['safe_fdr_adjust_rows', 'safe_hypergeom_outputs'], list(zip(dev, st)), dev + outs, fn, check)

        for case, call in (('table', tails_call('table')), ('element', tails_call('element')), ('outputs', outputs_call())):
            try:
                quiet, t_call_ms = so.run_quiet(lab, call)
                call.check(quiet)
                busy, _ = so.run_busy(lab, call, t_call_ms)
            finally:
                call.done()
            for i, (q, v) in enumerate(zip(quiet, busy)):
                assert np.array_equal(so.bits(v), so.bits(q)), '%s: output %d of the busy run differs from the quiet run' % (case, i)
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        if nbr is not None:
            nbr.close()


# ------------------------------------------------------------------------------------------- live device allocations ----

def test_no_growth_of_live_allocations_over_20_calls(be, ctx):
    a, b, pop, K, n, x = shaped_input(70, 130)
    nbr, attr = be.Neighborhoods.from_dense(ctx, a), be.Attributes.from_host(ctx, b)
    half = b.copy()
    half[0, 0] = 0.5
    bad = be.Attributes.from_host(ctx, half)
    bufs = [ctx.alloc_f64(70, 130) for _ in range(5)] + [ctx.alloc_f64(130)]
    ptrs = [buf.ptr for buf in bufs]
    try:
        def one(k):
            evaluator = ('table', 'element', None)[k % 3]
            be.hypergeom_tails(ctx, nbr, attr, ht.SIGNS[k % 3], 0.05, ptrs, evaluator=evaluator)
            be.fdr_adjust_rows(ctx, 70, 130, ptrs[1])
            be.hypergeom_outputs(ctx, 70, 130, ht.SIGNS[k % 3], 0.05, ptrs[1], ptrs[2], ptrs[3:])
            if k % 5 == 0:
                with pytest.raises(be._lib.SafeHipError):
                    be.hypergeom_tails(ctx, nbr, bad, 'both', 0.05, ptrs)
        for k in range(3):                                      # the scratch slots grow to their sizes
            one(k)
        before = be.device_live_alloc_count()
        for k in range(20):
            one(k)
        assert be.device_live_alloc_count() == before
    finally:
        for buf in bufs:
            buf.free()
        for h in (bad, attr, nbr):
            h.close()
