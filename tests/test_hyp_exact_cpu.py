"""The exact hypergeometric reference (tests/hyp_exact.py) and the designed case list (tests/hyp_cases.py) checked where no GPU
exists: against brute-force binomial sums, against SciPy on the very cells the GPU test uses, and the cost of building them."""
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import hyp_cases as hc
import hyp_exact as hx


def test_exact_tail_equals_brute_force_binomial_sums():
    for pop in range(0, 15):
        for K in range(pop + 1):
            for n in range(pop + 1):
                den = math.comb(pop, n)
                lo, hi = hx.support(pop, K, n)
                tails = hx.exact_tails(pop, K, n)
                assert sorted(tails) == list(range(lo, hi + 1))
                for x in range(-1, pop + 2):
                    if x <= lo:
                        want = Fraction(1)                      # scipy's sf below the support
                    elif x > hi:
                        want = Fraction(0)
                    else:
                        want = Fraction(sum(math.comb(K, t) * math.comb(pop - K, n - t) for t in range(x, hi + 1)), den)
                    assert hx.exact_tail(pop, K, n, x) == want, (pop, K, n, x)
                    if lo <= x <= hi:
                        assert tails[x] == (want if x > lo else 1)


def test_exact_tail_rejects_impossible_parameters():
    with pytest.raises(ValueError):
        hx.exact_tail(5, 6, 1, 0)
    with pytest.raises(ValueError):
        hx.exact_tail(5, 1, 6, 0)


def test_ulp_error_and_neg_log10():
    third = Fraction(1, 3)
    assert hx.ulp_error(float(third), third) <= 0.5
    assert 0.5 <= hx.ulp_error(np.nextafter(float(third), 1.0), third) <= 1.5
    assert hx.ulp_error(0.05, Fraction(1, 20)) < 0.5 and hx.ulp_error(0.0, Fraction(0)) == 0.0
    assert hx.neg_log10(Fraction(1, 10 ** 300)) == 300.0 and hx.neg_log10(Fraction(0)) == math.inf
    assert hx.neg_log10(Fraction(1, 20)) == pytest.approx(-math.log10(0.05), rel=1e-15)
    assert hx.first_x_below(100, 50, 50, Fraction(1, 2)) == min(x for x, e in hx.exact_tails(100, 50, 50).items() if e < Fraction(1, 2))
    assert hx.first_x_below(10, 5, 5, Fraction(1, 10 ** 9)) is None


@pytest.mark.parametrize('case', [c for c in hc.all_cases() if c.family != 5], ids=repr)
def test_designed_parameters_are_what_the_arrays_hold(case):
    """(pop, K, n, x) recomputed from the membership and attribute matrices the way the reference counts them are the designed
    ones (the 20 000-node cases do this on the GPU machine only: their membership matrix is 3.2 GB)."""
    a, b = case.arrays()
    pop, K, n, x = case.recomputed(a, b)
    dK, dn, dx = case.designed()
    assert pop == case.pop and np.array_equal(K, dK) and np.array_equal(n, dn) and np.array_equal(x, dx)
    assert int(a.sum(axis=1).max()) == case.max_row_count
    lo = np.maximum(0, n[:, None] + K[None, :] - pop)
    assert np.all((x >= lo) & (x <= np.minimum(n[:, None], K[None, :])))


def test_family_1_reaches_every_parameter_of_its_populations():
    for pop in range(1, 13):
        seen = set()
        for c in hc.family1():
            if c.pop == pop and c.n_nan == 0:
                seen |= set(c.triples())
        want = {(K, n, x) for K in range(pop + 1) for n in range(pop + 1) for x in range(max(0, n + K - pop), min(K, n) + 1)}
        assert seen == want
        padded = [c for c in hc.family1_padded() if c.pop == pop]
        assert len(padded) == 1 and set(padded[0].triples()) == want
    assert hx.exact_tail(20, 1, 1, 1) == Fraction(1, 20) and (1, 1, 1) in hc.family1()[-2].triples()
    assert hx.exact_tail(40, 1, 2, 1) == Fraction(1, 20) and (1, 2, 1) in hc.family1()[-1].triples()


def test_family_2_populates_every_decade_band():
    for c in hc.family2():
        if not c.table_ok:
            continue
        counts = dict.fromkeys(hc.BANDS, 0)
        for e in c.expected().values():
            band = hc.band_of(e)
            if band:
                counts[band] += 1
        print('%s: cells per band %s' % (c.name, counts))
        # (1000 nodes cannot go below 1 / C(1000, 500) = 3.7e-300: that case is there for n = pop on the table forms)
        assert all(v >= 3 for k, v in counts.items() if c.pop >= 2000 or k in ('1e-10', '1e-50', '1e-100', '1e-200')), (c.name, counts)


def test_family_4_is_the_pair_of_calls_it_says():
    """Counts <= 2 under supports of hundreds in one call; the same columns, a cell at the top of a support of 300 and an all-zero
    column next to it in the other."""
    tiny, top, mid = hc.family4()
    hx_lo = [hx.support(tiny.pop, K, n) for K, n, _ in tiny.triples()]
    assert max(hi for _, hi in hx_lo) >= 300
    K, n, x = tiny.designed()
    assert x.max() == 2 and min(K.max(), n.max()) >= 300
    K2, n2, x2 = top.designed()
    assert x2.max() == 300 and (300, 300, 300) in top.triples() and set(tiny.cols) < set(top.cols)
    assert (x2[:, top.cols.index((50, 900))] == 0).all()
    assert mid.designed()[2].max() == 237 and 1e-16 < float(hx.exact_tail(1000, 300, 602, 237)) < 1e-10


def test_reference_against_scipy_on_the_gpu_case_list():
    """SciPy agrees with the exact tails at the project's rtol = 1e-6 wherever exact p >= 1e-290: the reference stays inside
    every bound the GPU test uses.  Prints SciPy's worst ulp error per family (the yardstick for the per-element kernel) and the
    time of building all expected values."""
    from scipy.stats import hypergeom
    hx.tail_numerators.cache_clear()                            # (warm from the tests above)
    t0 = time.perf_counter()
    cases = hc.all_cases()
    build = time.perf_counter() - t0
    worst = {}
    cells = 0
    for c in cases:
        t0 = time.perf_counter()
        exp = c.expected()
        build += time.perf_counter() - t0
        cells += len(exp)
        keys = list(exp)
        K, n, x = (np.array(v, dtype=np.int64) for v in zip(*keys))
        got = hypergeom.sf(x - 1, c.pop, K, n)
        for t, g in zip(keys, got):
            e = exp[t]
            assert 0.0 <= g <= 1.0
            if e >= Fraction(1, 10 ** 290):
                assert abs(Fraction(float(g)) - e) <= e / 10 ** 6, (c.name, t, g, float(e))
                worst[c.family] = max(worst.get(c.family, 0.0), hx.ulp_error(g, e))
            else:
                assert g <= 1e-289, (c.name, t, g)
    print('case list and expected values of the GPU test: %d distinct (K, n, x) in %.1f s' % (cells, build))
    print('worst ulp error of scipy.stats.hypergeom.sf (exact p >= 1e-290) per family: %s'
          % {k: float('%.3g' % v) for k, v in sorted(worst.items())})
    assert build < 60.0
