// Shortest round-trip text of an IEEE double, as NumPy writes it (np.array([v]).astype(str), which pandas' to_csv uses for
// float blocks) -- equal to CPython's repr(float):
//   * the shortest digit string that reads back as v; among several of that length the one closest to v, ties to even
//   * positional notation when the decimal exponent e of d.ddd x 10^e satisfies -4 <= e < 16 ("0.0001", "1.0",
//     "9999999999999998.0"), otherwise d[.ddd]e+XX with at least two exponent digits ("1e+16", "5e-324")
//   * "-0.0" keeps its sign, "inf" / "-inf"; NaN is written as nothing (pandas' default na_rep)
//
// Digit generation is Ryu (Ulf Adams, "Ryu: fast float-to-string conversion", PLDI 2018): the interval of reals that round
// to v is scaled by a 125-bit power of five (obj/pow5_table.h, written by gen_pow5.py) so that the decimal digits of its
// two ends and of v come out of 64x64->128-bit products; digits are then removed while the ends still differ, tracking
// whether the removed digits were all zero (exact ties).  No division by anything but constants, no big integers.
//
// __host__ __device__: the device formatter (format.hip) runs it; a host build of the same header is what the CPU test
// compares with NumPy on millions of values (tests/test_format_cpu.py).  The caller's output pointer may be LDS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SAFE_HD __host__ __device__ inline
#define SAFE_FMT_TABLE __device__ constexpr
#else
#define SAFE_HD inline
#define SAFE_FMT_TABLE constexpr
#endif

#include "pow5_table.h"

// longest text of one value: "-0.00012345678901234567" / "-1.2345678901234567e-308" (24 bytes)
#define F64_TEXT_MAX 24

SAFE_HD uint64_t f64_umulh(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (m * mul) >> j for a 128-bit mul = {lo, hi} and 64 < j < 128 (the result fits 64 bits)
SAFE_HD uint64_t f64_mul_shift(uint64_t m, const uint64_t *mul, int j) {
    const uint64_t lo_hi = f64_umulh(m, mul[0]);
    const uint64_t b_lo = m * mul[1];
    const uint64_t b_hi = f64_umulh(m, mul[1]);
    const uint64_t s_lo = b_lo + lo_hi;
    const uint64_t s_hi = b_hi + (s_lo < b_lo);
    const int s = j - 64;
    return (s_lo >> s) | (s_hi << (64 - s));
}

SAFE_HD int f64_pow5bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }
SAFE_HD int f64_log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }
SAFE_HD int f64_log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }

SAFE_HD bool f64_multiple_of_pow5(uint64_t v, int p) {
    int count = 0;
    while (v % 5 == 0 && count < p) {
        v /= 5;
        ++count;
    }
    return count >= p;
}

SAFE_HD bool f64_multiple_of_pow2(uint64_t v, int p) { return (v & ((1ull << p) - 1)) == 0; }

// Shortest digits of a finite, non-zero |v| given by its exponent field and mantissa: |v| = *digits * 10^*e10.
SAFE_HD void f64_shortest(uint32_t ieee_exp, uint64_t ieee_mant, uint64_t *digits, int *e10_out) {
    int e2;
    uint64_t m2;
    if (ieee_exp == 0) {
        e2 = 1 - 1023 - 52 - 2;
        m2 = ieee_mant;
    } else {
        e2 = (int)ieee_exp - 1023 - 52 - 2;
        m2 = (1ull << 52) | ieee_mant;
    }
    const bool accept_bounds = (m2 & 1) == 0;
    const uint64_t mv = 4 * m2;
    const uint32_t mm_shift = (ieee_mant != 0 || ieee_exp <= 1) ? 1 : 0;    // the interval below is half as wide at a power of two

    uint64_t vr, vp, vm;
    int e10;
    bool vm_tz = false, vr_tz = false;
    if (e2 >= 0) {
        const int q = f64_log10_pow2(e2) - (e2 > 3);
        e10 = q;
        const int k = F64_POW5_INV_BITCOUNT + f64_pow5bits(q) - 1;
        const int i = -e2 + q + k;
        vr = f64_mul_shift(4 * m2, F64_POW5_INV[q], i);
        vp = f64_mul_shift(4 * m2 + 2, F64_POW5_INV[q], i);
        vm = f64_mul_shift(4 * m2 - 1 - mm_shift, F64_POW5_INV[q], i);
        if (q <= 21) {
            if (mv % 5 == 0) vr_tz = f64_multiple_of_pow5(mv, q);
            else if (accept_bounds) vm_tz = f64_multiple_of_pow5(mv - 1 - mm_shift, q);
            else vp -= f64_multiple_of_pow5(mv + 2, q);
        }
    } else {
        const int q = f64_log10_pow5(-e2) - (-e2 > 1);
        e10 = q + e2;
        const int i = -e2 - q;
        const int k = f64_pow5bits(i) - F64_POW5_BITCOUNT;
        const int j = q - k;
        vr = f64_mul_shift(4 * m2, F64_POW5[i], j);
        vp = f64_mul_shift(4 * m2 + 2, F64_POW5[i], j);
        vm = f64_mul_shift(4 * m2 - 1 - mm_shift, F64_POW5[i], j);
        if (q <= 1) {
            vr_tz = true;
            if (accept_bounds) vm_tz = mm_shift == 1;
            else --vp;
        } else if (q < 63) {
            vr_tz = f64_multiple_of_pow2(mv, q);
        }
    }

    int removed = 0;
    uint32_t last = 0;
    uint64_t out;
    if (vm_tz || vr_tz) {
        // rare: an end of the interval or the value itself is exact in the removed digits
        while (vp / 10 > vm / 10) {
            vm_tz &= vm % 10 == 0;
            vr_tz &= last == 0;
            last = (uint32_t)(vr % 10);
            vr /= 10;
            vp /= 10;
            vm /= 10;
            ++removed;
        }
        if (vm_tz) {
            while (vm % 10 == 0) {
                vr_tz &= last == 0;
                last = (uint32_t)(vr % 10);
                vr /= 10;
                vp /= 10;
                vm /= 10;
                ++removed;
            }
        }
        if (vr_tz && last == 5 && vr % 2 == 0) last = 4;          // exact tie: round half to even
        out = vr + ((vr == vm && (!accept_bounds || !vm_tz)) || last >= 5);
    } else {
        bool round_up = false;
        if (vp / 100 > vm / 100) {
            round_up = vr % 100 >= 50;
            vr /= 100;
            vp /= 100;
            vm /= 100;
            removed += 2;
        }
        while (vp / 10 > vm / 10) {
            round_up = vr % 10 >= 5;
            vr /= 10;
            vp /= 10;
            vm /= 10;
            ++removed;
        }
        out = vr + (vr == vm || round_up);
    }
    *digits = out;
    *e10_out = e10 + removed;
}

SAFE_HD int f64_decimal_length(uint64_t v) {
    int n = 1;
    uint64_t p = 10;
    while (n < 17 && v >= p) {
        ++n;
        p *= 10;
    }
    return n;
}

// Text of the value with bit pattern `bits`: writes it to out (unless out is NULL) and returns its length (0 for NaN).
SAFE_HD int f64_text(uint64_t bits, char *out) {
    const int sign = (int)(bits >> 63);
    const uint32_t ieee_exp = (uint32_t)((bits >> 52) & 0x7ff);
    const uint64_t ieee_mant = bits & ((1ull << 52) - 1);
    if (ieee_exp == 0x7ff) {
        if (ieee_mant) return 0;
        if (out) {
            if (sign) out[0] = '-';
            out[sign] = 'i';
            out[sign + 1] = 'n';
            out[sign + 2] = 'f';
        }
        return sign + 3;
    }
    if (sign && out) out[0] = '-';
    if (ieee_exp == 0 && ieee_mant == 0) {
        if (out) {
            out[sign] = '0';
            out[sign + 1] = '.';
            out[sign + 2] = '0';
        }
        return sign + 3;
    }
    uint64_t d;
    int e10;
    f64_shortest(ieee_exp, ieee_mant, &d, &e10);
    const int n = f64_decimal_length(d);
    const int e = e10 + n - 1;                    // v = d.ddd x 10^e
    char *o = out ? out + sign : nullptr;
    int len;
    if (e >= -4 && e < 16) {
        if (e >= 0) {
            if (n <= e + 1) {                     // integral: digits, zeros, ".0"
                len = e + 3;
                if (o) {
                    for (int i = n; i <= e; ++i) o[i] = '0';
                    o[e + 1] = '.';
                    o[e + 2] = '0';
                    for (int i = n - 1; i >= 0; --i, d /= 10) o[i] = (char)('0' + d % 10);
                }
            } else {                              // digits with the point after digit e
                len = n + 1;
                if (o) {
                    o[e + 1] = '.';
                    for (int i = n - 1; i >= 0; --i, d /= 10) o[i <= e ? i : i + 1] = (char)('0' + d % 10);
                }
            }
        } else {                                  // "0." then -e-1 zeros then the digits
            const int z = -e - 1;
            len = 2 + z + n;
            if (o) {
                o[0] = '0';
                o[1] = '.';
                for (int i = 0; i < z; ++i) o[2 + i] = '0';
                for (int i = n - 1; i >= 0; --i, d /= 10) o[2 + z + i] = (char)('0' + d % 10);
            }
        }
    } else {
        const int ae = e < 0 ? -e : e;
        const int mant_len = n > 1 ? n + 1 : 1;
        const int exp_digits = ae >= 100 ? 3 : 2;
        len = mant_len + 2 + exp_digits;
        if (o) {
            for (int i = n - 1; i >= 1; --i, d /= 10) o[i + 1] = (char)('0' + d % 10);
            o[0] = (char)('0' + d);
            if (n > 1) o[1] = '.';
            o[mant_len] = 'e';
            o[mant_len + 1] = e < 0 ? '-' : '+';
            int x = ae;
            for (int i = exp_digits - 1; i >= 0; --i, x /= 10) o[mant_len + 2 + i] = (char)('0' + x % 10);
        }
    }
    return sign + len;
}
