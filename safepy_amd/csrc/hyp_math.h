// The hypergeometric arithmetic shared by enrich.hip (safe_hypergeom) and hyptails.hip (safe_hypergeom_tails): the
// log-factorial pmf, the reciprocal of the term ratios, the double-double helpers of the table kernels and the
// per-element upper tail.  Device code only; every translation unit that includes it is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// helpers of the hypergeometric kernels (K4, further down)
__device__ __forceinline__ double hyp_logpmf(const double *__restrict__ lf, int64_t t, int64_t pop, int64_t good,
                                             int64_t draws) {
    return (lf[good] - lf[t] - lf[good - t]) + (lf[pop - good] - lf[draws - t] - lf[pop - good - draws + t]) -
           (lf[pop] - lf[draws] - lf[pop - draws]);
}

// 1 / x for the term ratios of the tail recurrence: hardware reciprocal estimate + two Newton
// steps (a couple of ulp, far inside the 1e-6 relative parity bound) instead of the ~30-instruction
// IEEE division; no table loads inside the serial loop (they left the waves waiting 80 % of the time)
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// double-double helpers of the table kernel (error-free transformations; the TU is built with
// -ffp-contract=off, every fma below is explicit)
struct dd_t {
    double hi, lo;
};
__device__ __forceinline__ dd_t dd_fast_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd_t dd_add(dd_t x, dd_t y) {
    const double s = x.hi + y.hi, bb = s - x.hi;
    const double e = ((x.hi - (s - bb)) + (y.hi - bb)) + (x.lo + y.lo);
    return dd_fast_two_sum(s, e);
}
__device__ __forceinline__ dd_t dd_mul_d(dd_t x, double d) {
    const double p = x.hi * d;
    const double e = fma(x.lo, d, fma(x.hi, d, -p));
    return dd_fast_two_sum(p, e);
}
__device__ __forceinline__ dd_t dd_div_d(dd_t x, double d) {
    const double r = fast_rcp(d), q1 = x.hi * r, p = q1 * d;
    const double rem = ((x.hi - p) - fma(q1, d, -p)) + x.lo;            // x - q1 * d, exactly enough
    return dd_fast_two_sum(q1, rem * r);
}
__device__ __forceinline__ double dd_ratio(dd_t a, dd_t b) {            // a / b rounded to double
    const double r = fast_rcp(b.hi), q1 = a.hi * r;
    const dd_t prod = dd_mul_d(b, q1);
    const double rem = ((a.hi - prod.hi) - prod.lo) + a.lo;
    return q1 + rem * r;
}

// --------------------------------------------------------------------------------------
// K4: hypergeometric upper tail P[H >= X] = sf(X - 1) with the semantics of
// scipy.stats.hypergeom.sf as called at safe.py:596 (rv_discrete.sf wrapper: argument
// check -> NaN, below support -> 1, at/after the top of the support -> 0, result clipped
// to [0,1]).  pmf from a host-built log-factorial table, tail by the term recurrence,
// summed on the side of the mode that keeps the sum short (complemented when needed).
// --------------------------------------------------------------------------------------
__device__ double hyp_sf(const double *__restrict__ lf, double x_hits, double pop_d, double good_d, double draws_d) {
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    // _argcheck of scipy's hypergeom: integers, 0 <= good <= pop, 0 <= draws <= pop
    if (!(pop_d >= 0.0) || !(good_d >= 0.0) || !(draws_d >= 0.0) || good_d > pop_d || draws_d > pop_d ||
        pop_d != floor(pop_d) || good_d != floor(good_d) || draws_d != floor(draws_d))
        return qnan;
    const double k_d = x_hits - 1.0;
    if (k_d != k_d) return qnan;
    const int64_t pop = static_cast<int64_t>(pop_d), good = static_cast<int64_t>(good_d),
                  draws = static_cast<int64_t>(draws_d);
    const int64_t lo = draws - (pop - good) > 0 ? draws - (pop - good) : 0;
    const int64_t hi = good < draws ? good : draws;
    if (k_d < static_cast<double>(lo)) return 1.0;
    if (k_d >= static_cast<double>(hi)) return 0.0;
    // inside the support a non-integer k is NaN (SciPy 1.15's Boost tail, pinned by tests/golden/fdr.npz `hyp_nan`:
    // half-integer hit counts of a forced-hypergeometric call on non-0/1 data); outside it the rules above win
    if (k_d != floor(k_d)) return qnan;
    const int64_t k = static_cast<int64_t>(k_d);
    const double eps = 2.220446049250313e-16;
    const double mode = floor(static_cast<double>(good + 1) * static_cast<double>(draws + 1) / static_cast<double>(pop + 2));
    // the loops count in doubles (exact: integers below 2^53): 64-bit integer -> double
    // conversions would cost more than the recurrence itself
    const int lo_i = static_cast<int>(lo), hi_i = static_cast<int>(hi);
    const double rest_d = pop_d - good_d - draws_d;                     // may be negative; rest + t >= 0 inside the support
    double result;
    if (static_cast<double>(k) < mode) {
        // lower tail cdf(k) downwards from k, then complement
        int t = static_cast<int>(k);
        double td = static_cast<double>(t);
        double term = exp(hyp_logpmf(lf, t, pop, good, draws));
        double sum = term;
        while (t > lo_i && term > eps) {
            // pmf(t-1) / pmf(t)
            term = term * (td * (rest_d + td)) * fast_rcp((good_d - td + 1.0) * (draws_d - td + 1.0));
            sum += term;
            --t;
            td -= 1.0;
        }
        result = 1.0 - sum;
    } else {
        int t = static_cast<int>(k) + 1;
        double td = static_cast<double>(t);
        double term = exp(hyp_logpmf(lf, t, pop, good, draws));
        double sum = term;
        while (t < hi_i && term > eps * sum) {
            // pmf(t+1) / pmf(t)
            term = term * ((good_d - td) * (draws_d - td)) * fast_rcp((td + 1.0) * (rest_d + td + 1.0));
            sum += term;
            ++t;
            td += 1.0;
        }
        result = sum;
    }
    return result < 0.0 ? 0.0 : (result > 1.0 ? 1.0 : result);
}
