"""Exact hypergeometric upper tails in Python integers: the reference the GPU evaluators are held to.

P[H >= x] for H ~ Hypergeom(pop, K, n) (pop nodes with a value, K of them annotated, n drawn) with the
support rules of scipy's rv_discrete.sf as safe.py:596 calls it: x <= lo -> 1, x > hi -> 0, where
lo = max(0, n + K - pop) and hi = min(K, n).  One sweep of the term recurrence

    C(K, t+1) C(pop-K, n-t-1) = C(K, t) C(pop-K, n-t) (K-t)(n-t) / ((t+1)(pop-K-n+t+1))      (exact division)

gives the numerators of every tail of one (pop, K, n); the denominator is their sum, C(pop, n)."""
import math
from fractions import Fraction
from functools import lru_cache


def support(pop, K, n):
    return max(0, n + K - pop), min(K, n)


@lru_cache(maxsize=4096)
def tail_numerators(pop, K, n):
    """(lo, hi, num, den): num[x - lo] / den = P[H >= x] for lo <= x <= hi, integers."""
    if not (0 <= K <= pop and 0 <= n <= pop):
        raise ValueError('need 0 <= K, n <= pop, got pop=%d K=%d n=%d' % (pop, K, n))
    lo, hi = support(pop, K, n)
    term = math.comb(K, lo) * math.comb(pop - K, n - lo)
    terms = [term]
    for t in range(lo, hi):
        term = term * ((K - t) * (n - t)) // ((t + 1) * (pop - K - n + t + 1))
        terms.append(term)
    num = [0] * len(terms)
    run = 0
    for i in range(len(terms) - 1, -1, -1):                   # tails from the top down
        run += terms[i]
        num[i] = run
    return lo, hi, tuple(num), run


def exact_tails(pop, K, n):
    """{x: P[H >= x]} for every x of the support, as Fractions (one sweep)."""
    lo, hi, num, den = tail_numerators(pop, K, n)
    return {lo + i: Fraction(v, den) for i, v in enumerate(num)}


def exact_tail(pop, K, n, x):
    """P[H >= x] as a Fraction; 1 at or below the bottom of the support, 0 above its top."""
    lo, hi, num, den = tail_numerators(pop, K, n)
    if x <= lo:
        return Fraction(1)
    if x > hi:
        return Fraction(0)
    return Fraction(num[x - lo], den)


def ulp_error(got, exact):
    """|got - exact| in units of the spacing of doubles at `exact` (the exact value rounded to a double)."""
    got = Fraction(float(got))
    return float(abs(got - exact) / Fraction(math.ulp(float(exact))))


def neg_log10(exact):
    """-log10 of an exact tail in 120-bit arithmetic, rounded to a double (inf for 0)."""
    import mpmath
    if exact == 0:
        return math.inf
    with mpmath.workprec(120):
        return float(-(mpmath.log10(mpmath.mpf(exact.numerator)) - mpmath.log10(mpmath.mpf(exact.denominator))))


def first_x_below(pop, K, n, bound):
    """Smallest x of the support with P[H >= x] < bound (a Fraction), or None."""
    lo, hi, num, den = tail_numerators(pop, K, n)
    a, b = 0, len(num)                                        # the tails fall with x: bisection
    while a < b:
        mid = (a + b) // 2
        if num[mid] * bound.denominator < bound.numerator * den:
            b = mid
        else:
            a = mid + 1
    return lo + a if a < len(num) else None
