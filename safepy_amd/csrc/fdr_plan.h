// The planning arithmetic of the Benjamini-Hochberg adjustment (fdr.hip): which form adjusts a family -- histogram, block sort or
// library sort -- with its geometry, chosen here and nowhere else; the span of a thread's share of a family; and the per-entry
// arithmetic every form does.  Host code over plain numbers -- no HIP runtime, no context, no environment: the host compiler
// alone builds it (tests/test_fdr_cases_cpu.py, tests/test_fdr_scope_cpu.py).  What the kernels call as well is FDR_HD.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define FDR_HD __host__ __device__ __forceinline__
#else
#define FDR_HD inline
#endif

// ------------------------------------------------------------------------------------------------------ constants ----

constexpr int FDR_THREADS = 256;                       // threads of every workgroup but the column count form's
// k_fdr_row_sort<IPT>: items per thread, the sort pads the row to FDR_THREADS * IPT keys; a row takes the smallest rung that holds it
constexpr int FDR_IPT_LADDER[] = {4, 8, 12, 16, 20, 24, 28, 32};
constexpr int FDR_IPT_RUNGS = sizeof(FDR_IPT_LADDER) / sizeof(FDR_IPT_LADDER[0]);
constexpr int64_t FDR_BLOCK_SORT_MAX = 8192;           // longer rows go to the library sort (column ids travel as unsigned short)
static_assert(FDR_BLOCK_SORT_MAX == FDR_THREADS * FDR_IPT_LADDER[FDR_IPT_RUNGS - 1] && FDR_BLOCK_SORT_MAX <= 65536, "the last rung");
// k_fdr_row_counts: f64 table + u32 histogram per bin; both must fit the LDS
constexpr int FDR_ROW_HIST_BIN_BYTES = 12;
constexpr int FDR_ROW_HIST_LDS_BYTES = 60 * 1024;
constexpr int64_t FDR_ROW_HIST_MAX_P = FDR_ROW_HIST_LDS_BYTES / FDR_ROW_HIST_BIN_BYTES - 1;          // 5119
constexpr int FDR_COL_BIN_BYTES = 8;                   // k_fdr_col_counts: one slot per bin and column, histogram then table
constexpr int FDR_COL_LDS_BYTES = 128 * 1024;          // of the CU's 160 KiB: the tile's tables
constexpr int FDR_COL_TILE_MAX = 16;                   // columns of a tile: 128-byte row segments
constexpr int FDR_COL_THREADS = 1024;                  // a tile of 16 tables takes a CU's LDS alone: the one workgroup brings 16 waves
                                                       // (256 threads: 0.55 ms per 3971 x 4373 matrix at P = 1000, 1024: 0.28 ms)
constexpr int FDR_COL_TILE_MIN = 4;                    // below that the column reads fall apart: the sort form takes over
constexpr int64_t FDR_COL_HIST_MAX_P = FDR_COL_LDS_BYTES / (FDR_COL_BIN_BYTES * FDR_COL_TILE_MIN) - 1;   // 4095
constexpr int FDR_ALL_HIST_LDS_BYTES = 64 * 1024;      // k_fdr_all_hist: a u32 histogram per workgroup
constexpr int64_t FDR_ALL_HIST_MAX_P = FDR_ALL_HIST_LDS_BYTES / 4 - 1;                               // 16383
constexpr int FDR_TR_TILE = 32;                        // transpose tile, 32 x 32 doubles
constexpr int FDR_ALL_IPT = 8;                         // sorted ranks per thread of the whole-matrix suffix minimum
constexpr int FDR_ALL_BLOCK = FDR_THREADS * FDR_ALL_IPT;   // ... per workgroup
constexpr int64_t FDR_SEG_BATCH_KEYS = int64_t(1) << 27;   // keys per call of the segmented library sort (temporaries ~ 3 GB)
constexpr int64_t FDR_SORT_MAX_ITEMS = int64_t(1) << 31;   // the library sorts count their items in an int

// -------------------------------------------------------------------------------------------------------- the form ----

enum FdrScope { FDR_SCOPE_ROWS = 0, FDR_SCOPE_COLS = 1, FDR_SCOPE_ALL = 2 };          // SAFE_FDR_SCOPE_* of safe_hip.h

// SAFE_HIP_FDR_SORT, read by the entry point once per call: any value switches every count form off (the tests use the sorts as
// references for the count forms), "cub" also sends every row length to the library sort
enum FdrSwitch { FDR_SWITCH_UNSET = 0, FDR_SWITCH_CUB, FDR_SWITCH_OTHER };
static inline FdrSwitch fdr_switch(const char *value) {
    return !value ? FDR_SWITCH_UNSET : !std::strcmp(value, "cub") ? FDR_SWITCH_CUB : FDR_SWITCH_OTHER;
}

// Whether families of `scope` whose entries are counts / P have a count form: the tables of P + 1 bins fit the LDS.  The
// read-only ratio check (k_fdr_check_ratio) runs only where this says yes.
static inline bool fdr_count_form_exists(int scope, int64_t P, FdrSwitch sw) {
    const int64_t max_p = scope == FDR_SCOPE_ROWS ? FDR_ROW_HIST_MAX_P : scope == FDR_SCOPE_COLS ? FDR_COL_HIST_MAX_P : FDR_ALL_HIST_MAX_P;
    return sw == FDR_SWITCH_UNSET && P > 0 && P <= max_p;
}

// columns per workgroup of k_fdr_col_counts
static inline int fdr_col_tile(int64_t P) {
    const int64_t fit = FDR_COL_LDS_BYTES / (FDR_COL_BIN_BYTES * (P + 1));
    return static_cast<int>(fit < FDR_COL_TILE_MAX ? fit : FDR_COL_TILE_MAX);
}

enum FdrKind {
    FDR_UNSUPPORTED = 0,     // the whole-matrix sort would pass FDR_SORT_MAX_ITEMS
    FDR_ROW_HIST,            // k_fdr_row_counts, lds_bytes
    FDR_ROW_BLOCK_SORT,      // k_fdr_row_sort<ipt>
    FDR_ROW_LIBRARY_SORT,    // segmented library sort of batch_rows rows per call + k_fdr_row
    FDR_ROW_TOO_LONG,        // ... whose single row would pass FDR_SORT_MAX_ITEMS
    FDR_COL_COUNTS,          // k_fdr_col_counts, tile columns per workgroup, lds_bytes
    FDR_COL_SORT,            // transpose, row_kind: the row form of the [m, n] transpose, transpose back
    FDR_ALL_COUNTS,          // k_fdr_all_hist (lds_bytes) / _table / _map
    FDR_ALL_SORT             // one device-wide sort + the three suffix-minimum kernels
};
struct FdrForm {
    FdrKind kind;
    int ipt, tile;
    size_t lds_bytes;
    int64_t batch_rows;
    FdrKind row_kind;        // FDR_COL_SORT: the row form of the transpose, with its ipt / batch_rows
};

// P: the count denominator when every entry is known to be a count ratio c / P (checked), else 0
static inline FdrForm fdr_row_form(int64_t n, int64_t m, int64_t P, FdrSwitch sw) {
    if (fdr_count_form_exists(FDR_SCOPE_ROWS, P, sw))
        return {FDR_ROW_HIST, 0, 0, static_cast<size_t>(P + 1) * FDR_ROW_HIST_BIN_BYTES, 0, FDR_ROW_HIST};
    if (m <= FDR_BLOCK_SORT_MAX && sw != FDR_SWITCH_CUB) {
        int k = 0;
        while (FDR_THREADS * FDR_IPT_LADDER[k] < m) ++k;
        return {FDR_ROW_BLOCK_SORT, FDR_IPT_LADDER[k], 0, 0, 0, FDR_ROW_BLOCK_SORT};
    }
    const int64_t fit = FDR_SEG_BATCH_KEYS / (m > 1 ? m : 1), batch_rows = fit < 1 ? 1 : fit < n ? fit : n;
    if (!(m < FDR_SORT_MAX_ITEMS - 1 && batch_rows * m < FDR_SORT_MAX_ITEMS)) return {FDR_ROW_TOO_LONG, 0, 0, 0, 0, FDR_ROW_TOO_LONG};
    return {FDR_ROW_LIBRARY_SORT, 0, 0, 0, batch_rows, FDR_ROW_LIBRARY_SORT};
}

// The form that adjusts a [n, m] matrix along `scope`; P as for fdr_row_form.
static inline FdrForm fdr_form(int scope, int64_t n, int64_t m, int64_t P, FdrSwitch sw) {
    const bool counts = fdr_count_form_exists(scope, P, sw);
    if (scope == FDR_SCOPE_ROWS) return fdr_row_form(n, m, P, sw);
    if (scope == FDR_SCOPE_COLS && !counts) {
        FdrForm f = fdr_row_form(m, n, 0, sw);
        f.kind = FDR_COL_SORT;
        return f;
    }
    if (scope == FDR_SCOPE_COLS) {
        const int tile = fdr_col_tile(P);
        return {FDR_COL_COUNTS, 0, tile, static_cast<size_t>(tile) * (P + 1) * FDR_COL_BIN_BYTES, 0, FDR_UNSUPPORTED};
    }
    if (counts) return {FDR_ALL_COUNTS, 0, 0, static_cast<size_t>(P + 1) * 4, 0, FDR_UNSUPPORTED};
    // (n and m before n * m: the product of two large sizes may wrap)
    const bool fits = n < FDR_SORT_MAX_ITEMS && m < FDR_SORT_MAX_ITEMS && n * m < FDR_SORT_MAX_ITEMS;
    return {fits ? FDR_ALL_SORT : FDR_UNSUPPORTED, 0, 0, 0, 0, FDR_UNSUPPORTED};
}

// ------------------------------------------------------------------------------------------- a thread's share, entries ----

// [b0, b1): the share of part t of `parts` over `count` items, ceil(count / parts) each while they last
template <typename I>
FDR_HD void fdr_span(I count, I parts, I t, I &b0, I &b1) {
    const I per = (count + parts - 1) / parts;
    b0 = t * per < count ? t * per : count;
    b1 = b0 + per < count ? b0 + per : count;
}

// -0.0 -> +0.0, every other value as it is: NumPy sorts and compares the two zeros as one value, and the rows of all three
// forms come out with the same bits
FDR_HD double fdr_plus_zero(double v) { return v == 0.0 ? 0.0 : v; }

// The sort key of a p-value: its bit pattern after two substitutions.  -0.0 becomes +0.0 (key 0; left as 0x8000... it would sort
// last, and -0.0 / (m / m) would be the running minimum of the whole row) and every NaN, of either sign and any payload, becomes
// 0x7FF8....  Then positive doubles order like their bits, both zeros sort first as one value and every NaN sorts behind every
// number, as np.argsort puts them.  (Negative p-values other than -0.0 are a caller's error: not defined.)
constexpr unsigned long long FDR_KEY_NAN = 0x7FF8000000000000ull;
FDR_HD unsigned long long fdr_key(double v) { return v != v ? FDR_KEY_NAN : __builtin_bit_cast(unsigned long long, fdr_plus_zero(v)); }

// The count c of an entry v = c / P: the bin of the count forms, exact in f64
FDR_HD double fdr_count_of(double v, double P) { return rint(v * P); }
// ... as a bin, or why the entry has none: a NaN (poisons its family), or not exactly c / P with c in [0, P] (the family is sorted)
constexpr int FDR_BIN_NAN = -1, FDR_BIN_NOT_RATIO = -2;
FDR_HD int fdr_ratio_bin(double v, double P) {
    if (v != v) return FDR_BIN_NAN;
    const double cf = fdr_count_of(v, P);
    if (!(cf >= 0.0 && cf <= P) || cf / P != v) return FDR_BIN_NOT_RATIO;
    return static_cast<int>(cf);
}

// statsmodels' raw value of the entry p at sorted position `rank1` (from 1) of a family of `count`: the same two divisions on
// the same doubles; then the running minimum from the right, and values above 1 become 1
FDR_HD double fdr_raw(double p, double rank1, double count) { return p / (rank1 / count); }
FDR_HD double fdr_clamp(double v) { return v > 1.0 ? 1.0 : v; }

// ----------------------------------------------------------------------------------------------- the other procedures ----

// multiple_testing_method (SAFE_MT_* of safe_hip.h): statsmodels' multipletests restated.  The form of a call (fdr_form) does
// not depend on the procedure; Bonferroni alone takes no form at all (element-wise).
enum FdrProcedure { FDR_PROC_BH = 0, FDR_PROC_BY = 1, FDR_PROC_HOLM = 2, FDR_PROC_HOCHBERG = 3, FDR_PROC_BONFERRONI = 4 };
constexpr int FDR_PROC_COUNT = 5;

// Hochberg's and Holm's raw value at sorted position `rank1` (from 1): the integer count - rank1 + 1 is exact in f64, one
// rounded product
FDR_HD double fdr_step_raw(double p, double rank1, double count) { return (count - rank1 + 1.0) * p; }
// Benjamini-Yekutieli's: statsmodels divides the rank fractions by c = sum 1 / i first, then the p-values by the result --
// three divisions in this order; c comes from the caller (backend.by_constant)
FDR_HD double fdr_by_raw(double p, double rank1, double count, double c_by) { return p / ((rank1 / count) / c_by); }
// Bonferroni's: one rounded product (then the clamp)
FDR_HD double fdr_bonferroni_raw(double p, double count) { return p * count; }

// The raw value of a sorted procedure.  `proc` is a compile-time constant in every kernel, so one branch is left.
FDR_HD double fdr_proc_raw(int proc, double p, double rank1, double count, double c_by) {
    return proc == FDR_PROC_BH ? fdr_raw(p, rank1, count)
           : proc == FDR_PROC_BY ? fdr_by_raw(p, rank1, count, c_by)
                                 : fdr_step_raw(p, rank1, count);
}
// Holm is step-down: the running MAXIMUM from the LEFT (a tie group takes the value of its FIRST sorted position); the others
// take the running minimum from the right (a tie group takes the value of its LAST position)
constexpr bool fdr_proc_from_left(int proc) { return proc == FDR_PROC_HOLM; }
// np.minimum.accumulate from the right carries a NaN (sorted last) through the whole family; np.maximum.accumulate from the left
// and the element-wise product leave it where it is: the NaN entries become 0x7FF8... and the numbers are adjusted as members
// of a family of `count` entries, NaNs counted
constexpr bool fdr_proc_nan_poisons(int proc) { return proc == FDR_PROC_BH || proc == FDR_PROC_BY || proc == FDR_PROC_HOCHBERG; }
constexpr bool fdr_proc_sorts(int proc) { return proc != FDR_PROC_BONFERRONI; }
