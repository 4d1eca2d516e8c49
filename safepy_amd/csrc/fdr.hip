// multiple_testing=True: Benjamini-Hochberg (and, further down, multiple_testing_method's other procedures) adjustment of the p-value matrices along multiple_testing_scope, followed by the NES /
// binarisation steps that depend on the adjusted values (safe.py:546-554, 608, 468-472).  The family of one adjustment is every
// ROW (one node's neighborhood across its m attributes), i.e. np.apply_along_axis(fdrcorrection, 1, pvalues)[:, 1, :] of
// safepy/safe.py:536-542 (randomization) and 599-605 (hypergeometric); or every COLUMN (one attribute across the n neighborhoods:
// np.apply_along_axis(lambda c: fdrcorrection(c)[1], 0, p)); or the WHOLE matrix (fdrcorrection(p.ravel())[1].reshape(p.shape)).
//
// statsmodels' fdrcorrection(pvals) (method 'indep'), operation by operation:
//     order = argsort(pvals); ps = pvals[order]
//     raw = ps / (arange(1, n+1) / float(n))
//     corrected = minimum.accumulate(raw[::-1])[::-1];  corrected[corrected > 1] = 1
//     out[order] = corrected
// Ties need no care: tied entries end up with the same value whatever their order (the running minimum from the right passes
// through the group's last member).  NaN p-values sort last and np.minimum propagates them through the whole family, so a family
// with any NaN, of either sign and any payload, becomes all 0x7FF8... -- for the whole-matrix scope that is the whole matrix --
// and -0.0 is the value 0.0.  Every form does the same two divisions on the same doubles (fdr_raw; the count is n for a column, n m
// for the whole matrix, exact in f64); all counting is in integers and fmin of numbers does not depend on the order, so identical
// calls give identical bytes.
//
// The form of a call is chosen in fdr_plan.h (fdr_form) and nowhere else:
//   rows, count form      p = counts / num_permutations: no sort, the row's histogram over the counts (k_fdr_row_counts).
//   rows, block sort      rows of up to 8192 attributes are adjusted by ONE kernel, one workgroup per row: block-wide radix sort of
//                         the row's p-values with their column ids, then the Benjamini-Hochberg pass on the registers that hold the
//                         sorted row (k_fdr_row_sort, instead of the library's segmented radix sort of the whole matrix + its
//                         temporaries).
//   rows, library sort    longer rows: hipCUB segmented radix sort, rows batched so a call stays below 2^31 keys, then the same BH
//                         pass (k_fdr_row).
//   columns, count form   k_fdr_col_counts: p = c / P with P <= FDR_COL_HIST_MAX_P.  A workgroup owns a tile of adjacent columns
//                         (its row reads are contiguous), one LDS histogram of P + 1 bins per column; a wave turns a column's
//                         histogram into the table of adjusted values (the same bin rule, fdr_ratio_bin); one table look-up per
//                         entry.
//   columns, sort form    tiled LDS transpose into per-call memory, the row sort forms on the [m, n] transpose, transpose back.
//   matrix, count form    P <= FDR_ALL_HIST_MAX_P: k_fdr_all_hist (per-workgroup LDS histograms flushed with integer atomics
//                         into 64-bit counters), k_fdr_all_table (one workgroup: the P + 1 adjusted values), k_fdr_all_map.
//                         Two reads and one write of the matrix.
//   matrix, sort form     one device-wide radix sort of the n m keys (fdr_key) with the cell index as payload; the running minimum
//                         from the right as per-block minima (k_fdr_all_blockmin), a carry pass (k_fdr_all_carry) and the apply
//                         pass, which scatters back (k_fdr_all_apply).  The keys-only sort with a binary search per cell was not
//                         built.  n m >= 2^31 is beyond the library sort: SAFE_E_UNSUPPORTED.
//
// multiple_testing_method (safe_mt_adjust_scope / safe_mt_adjust_matrix): the same passes with another per-entry value, statsmodels'
// multipletests operation by operation (fdr_plan.h: fdr_proc_raw).  Every kernel that scans takes the procedure as a template
// parameter M -- no switch inside the unrolled loops of the block sort -- and the M = Benjamini-Hochberg instantiation is the code
// above, operation for operation.
//     fdr_by      raw = ps / ((k / count) / c), c = sum 1 / i from the caller: the running minimum from the right
//     hochberg    raw = (count - k + 1) ps: the running minimum from the right
//     holm        the same raw: the running MAXIMUM from the LEFT -- prefix_max beside suffix_min; k_fdr_all_blockmin keeps block
//                 maxima, k_fdr_all_carry carries from the left, k_fdr_all_apply scans upwards
//     bonferroni  ps count: k_fdr_bonferroni, element-wise, no form at all
// A tie group gets one value whatever its order: the minimum from the right passes through the group's LAST sorted position, the
// maximum from the left through its FIRST, so the count forms evaluate Holm at rank before[c] + 1 = cum[c] - hist[c] + 1 and the
// others at rank cum[c], on the same doubles as the sort forms.  NaN: the minimum from the right carries it through the family;
// np.maximum.accumulate from the left reaches the NaNs (sorted last) only after every number, and the element-wise product never
// mixes entries, so under Holm and Bonferroni a NaN entry becomes 0x7FF8... on its own and the numbers are adjusted as members
// of a family of `count` entries, NaNs counted.  fmax skips a NaN, so the Holm kernels write those entries explicitly; the
// library sort puts NaNs whose sign bit is set in FRONT of the numbers, which k_fdr_row counts and takes off Holm's ranks.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "fdr_plan.h"

static_assert(FDR_SCOPE_ROWS == SAFE_FDR_SCOPE_ROWS && FDR_SCOPE_COLS == SAFE_FDR_SCOPE_COLS && FDR_SCOPE_ALL == SAFE_FDR_SCOPE_ALL,
              "fdr_plan.h numbers the scopes as safe_hip.h does");
static_assert(FDR_PROC_BH == SAFE_MT_FDR_BH && FDR_PROC_BY == SAFE_MT_FDR_BY && FDR_PROC_HOLM == SAFE_MT_HOLM &&
                  FDR_PROC_HOCHBERG == SAFE_MT_HOCHBERG && FDR_PROC_BONFERRONI == SAFE_MT_BONFERRONI,
              "fdr_plan.h numbers the procedures as safe_hip.h does");

namespace {

__device__ __forceinline__ double fdr_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double fdr_key_value(unsigned long long k) { return __longlong_as_double(static_cast<long long>(k)); }
__device__ __forceinline__ double fdr_qnan() { return fdr_key_value(FDR_KEY_NAN); }

// one entry into an LDS histogram over the counts; what keeps it out goes to `bad`: 1 = a NaN, 2 = not a count ratio
__device__ __forceinline__ void hist_add(unsigned int *hist, double v, double P, unsigned int &bad) {
    const int bin = fdr_ratio_bin(v, P);
    if (bin >= 0) atomicAdd(&hist[bin], 1u);
    else bad |= bin == FDR_BIN_NAN ? 1u : 2u;
}

// part[u]: the minimum of thread u's share of the sorted family; `carry` joined with the shares right of thread t's
__device__ __forceinline__ double suffix_min(const double *part, int t, double carry) {
    for (int u = t + 1; u < FDR_THREADS; ++u) carry = fmin(carry, part[u]);
    return carry;
}

// Holm's counterpart: part[u]: the maximum of thread u's share; `carry` joined with the shares left of thread t's
__device__ __forceinline__ double prefix_max(const double *part, int t, double carry) {
    for (int u = 0; u < t; ++u) carry = fmax(carry, part[u]);
    return carry;
}

// A family's histogram over the counts -> table[c] = the adjusted value of every entry with count c, by one workgroup.  All
// members of a tie end up with the value of the tie's LAST sorted position (header above), so cum[c] = #entries with count <= c
// is that position, raw[c] = (c / P) / (cum[c] / count) the value statsmodels computes there, and table[c] = min over the occupied
// c' >= c: block scan (thread t owns the bins fdr_span gives it), reverse running minimum.  H: the counters (u32 in LDS, u64 in
// memory); unoccupied bins count as +inf.  M: the procedure (fdr_proc_raw at the same position).  Holm runs the other way:
// the tie takes the value of its FIRST position before[c] + 1 = cum[c] - hist[c] + 1, table[c] = max over the occupied c' <= c,
// unoccupied bins count as -inf; count_d counts the NaN entries the histogram leaves out.
template <int M, typename H>
__device__ __forceinline__ void hist_to_table(const H *__restrict__ hist, int bins, double P, double count_d, double c_by,
                                              double *__restrict__ table) {
    __shared__ H part_u[FDR_THREADS];
    __shared__ double part_d[FDR_THREADS];
    const int t = threadIdx.x;
    int b0, b1;
    fdr_span(bins, FDR_THREADS, t, b0, b1);
    H local = 0;
    for (int c = b0; c < b1; ++c) local += hist[c];
    part_u[t] = local;
    __syncthreads();
    H cum = 0;
    for (int u = 0; u < t; ++u) cum += part_u[u];
    if constexpr (fdr_proc_from_left(M)) {
        double mx = -fdr_inf();
        for (int c = b0; c < b1; ++c) {
            const H h = hist[c];
            const double raw = h ? fdr_step_raw(static_cast<double>(c) / P, static_cast<double>(cum + 1), count_d) : -fdr_inf();
            cum += h;
            table[c] = raw;
            mx = fmax(mx, raw);
        }
        part_d[t] = mx;
        __syncthreads();
        double carry = prefix_max(part_d, t, -fdr_inf());
        for (int c = b0; c < b1; ++c) {
            carry = fmax(carry, table[c]);
            table[c] = fdr_clamp(carry);
        }
    } else {
        double mn = fdr_inf();
        for (int c = b0; c < b1; ++c) {
            const H h = hist[c];
            cum += h;
            const double raw = h ? fdr_proc_raw(M, static_cast<double>(c) / P, static_cast<double>(cum), count_d, c_by) : fdr_inf();
            table[c] = raw;
            mn = fmin(mn, raw);
        }
        part_d[t] = mn;
        __syncthreads();
        double carry = suffix_min(part_d, t, fdr_inf());
        for (int c = b1 - 1; c >= b0; --c) {
            carry = fmin(carry, table[c]);
            table[c] = fdr_clamp(carry);
        }
    }
}

// ----------------------------------------------------------------------------------------------------- rows, sort forms ----

__global__ void k_fdr_cols(int32_t *__restrict__ idx, int64_t count, int64_t m) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x;
    if (i < count) idx[i] = static_cast<int32_t>(i % m);
}

__global__ void k_fdr_offsets(int64_t *__restrict__ off, int64_t rows, int64_t m) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x;
    if (i <= rows) off[i] = i * m;
}

// one workgroup per row of the batch; ps / cols: the row sorted ascending with its column ids.  M: the procedure
template <int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_row(const double *__restrict__ ps, const int32_t *__restrict__ cols, int64_t m,
                                                         double c_by, double *__restrict__ out) {
    __shared__ double part[FDR_THREADS];
    const int64_t row = blockIdx.x;
    const double *p = ps + row * m;
    const int32_t *c = cols + row * m;
    double *o = out + row * m;
    const int t = threadIdx.x;
    const double n_d = static_cast<double>(m);
    int64_t r0, r1;
    fdr_span<int64_t>(m, FDR_THREADS, t, r0, r1);
    // The library's float key puts a NaN whose sign bit is set (0xFFF8...: what x86 makes of 0 / 0) BEFORE every number and
    // the others behind them (it treats -0.0 as +0.0): a row has a NaN iff one of its two ends is one.
    if constexpr (fdr_proc_from_left(M)) {
        // Holm: the numbers keep their ranks among the numbers (np.argsort puts every NaN last): position r minus the NaNs in
        // front of the numbers, which are the NaNs whose sign bit is set
        __shared__ unsigned int lead_nans;
        if (t == 0) lead_nans = 0u;
        __syncthreads();
        unsigned int here = 0;
        for (int64_t r = r0; r < r1; ++r) here += (p[r] != p[r]) && __double_as_longlong(p[r]) < 0;
        if (here) atomicAdd(&lead_nans, here);
        __syncthreads();
        const int64_t lead = lead_nans;
        double mine = -fdr_inf();
        for (int64_t r = r0; r < r1; ++r) {
            const double v = p[r];
            if (v == v) mine = fmax(mine, fdr_step_raw(fdr_plus_zero(v), static_cast<double>(r - lead + 1), n_d));
        }
        part[t] = mine;
        __syncthreads();
        double carry = prefix_max(part, t, -fdr_inf());             // maximum over everything left of this thread's chunk
        for (int64_t r = r0; r < r1; ++r) {
            const double v = p[r];
            if (v != v) {                                           // (fmax would skip it: written explicitly)
                o[c[r]] = fdr_qnan();
                continue;
            }
            carry = fmax(carry, fdr_step_raw(fdr_plus_zero(v), static_cast<double>(r - lead + 1), n_d));
            o[c[r]] = fdr_clamp(carry);
        }
    } else {
        const double first = p[0], last = p[m - 1];
        if (first != first || last != last) {                       // a NaN anywhere poisons the whole row
            for (int64_t r = t; r < m; r += FDR_THREADS) o[r] = fdr_qnan();
            return;
        }
        double mine = fdr_inf();
        for (int64_t r = r1 - 1; r >= r0; --r) mine = fmin(mine, fdr_proc_raw(M, fdr_plus_zero(p[r]), static_cast<double>(r + 1), n_d, c_by));
        part[t] = mine;
        __syncthreads();
        double carry = suffix_min(part, t, fdr_inf());              // minimum over everything right of this thread's chunk
        for (int64_t r = r1 - 1; r >= r0; --r) {
            carry = fmin(carry, fdr_proc_raw(M, fdr_plus_zero(p[r]), static_cast<double>(r + 1), n_d, c_by));
            o[c[r]] = fdr_clamp(carry);
        }
    }
}

// One workgroup = one row: a block-wide radix sort (hipcub::BlockRadixSort: keys and column ids in registers, LDS
// for the exchanges) leaves thread t with ranks [t IPT, (t + 1) IPT) of the sorted row -- exactly the chunks the
// Benjamini-Hochberg pass wants.  Keys: fdr_key of the p-values; padding keys are all ones, behind the NaN key, so
// the ranks below m hold the row and nothing else.
// (A bitonic network on an LDS copy of the row was tried first: 91 stages x 20 bytes per element = 15 MB of LDS
// traffic per row, 3.2 ms per 3971 x 4373 matrix.)
#ifndef FDR_RADIX_BITS
#define FDR_RADIX_BITS 8
#endif
// M: the procedure, a template parameter so that the unrolled loops over the registers hold one arithmetic and no switch.
template <int IPT, int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_row_sort(double *__restrict__ pvals, int64_t m, double c_by) {
    using BlockSort = hipcub::BlockRadixSort<unsigned long long, FDR_THREADS, IPT, unsigned short, FDR_RADIX_BITS>;
    __shared__ typename BlockSort::TempStorage temp;
    __shared__ double part[FDR_THREADS];
    __shared__ int has_nan;
    const int t = threadIdx.x;
    double *p = pvals + static_cast<int64_t>(blockIdx.x) * m;
    unsigned long long key[IPT];
    unsigned short idx[IPT];
    if (t == 0) has_nan = 0;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const int e = t * IPT + i;
        key[i] = e < m ? fdr_key(p[e]) : ~0ull;
        idx[i] = static_cast<unsigned short>(e);
    }
    __syncthreads();
    BlockSort(temp).Sort(key, idx, 0, 64);
    // the same arithmetic, in the same order, as k_fdr_row, on the registers that hold the sorted row; rank of key[i] = t * IPT + i
    const double n_d = static_cast<double>(m);
    const int r0 = t * IPT;
    if constexpr (fdr_proc_from_left(M)) {
        // Holm: the running maximum from the left; the NaN keys sit behind the numbers and keep the numbers' ranks
        double mine = -fdr_inf();
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            if (r0 + i >= m) continue;
            const double v = fdr_key_value(key[i]);
            if (v == v) mine = fmax(mine, fdr_step_raw(v, static_cast<double>(r0 + i + 1), n_d));
        }
        part[t] = mine;
        __syncthreads();
        double carry = prefix_max(part, t, -fdr_inf());             // maximum over everything left of this thread's chunk
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            if (r0 + i >= m) continue;
            const double v = fdr_key_value(key[i]);
            if (v != v) {                                           // (fmax would skip it: written explicitly)
                p[idx[i]] = fdr_qnan();
                continue;
            }
            carry = fmax(carry, fdr_step_raw(v, static_cast<double>(r0 + i + 1), n_d));
            p[idx[i]] = fdr_clamp(carry);
        }
    } else {
        double mine = fdr_inf();
        bool nan_here = false;
#pragma unroll
        for (int i = IPT - 1; i >= 0; --i) {
            if (r0 + i >= m) continue;
            const double v = fdr_key_value(key[i]);
            nan_here |= v != v;
            mine = fmin(mine, fdr_proc_raw(M, v, static_cast<double>(r0 + i + 1), n_d, c_by));
        }
        part[t] = mine;
        if (nan_here) has_nan = 1;
        __syncthreads();
        if (has_nan) {                                              // a NaN anywhere poisons the whole row
            for (int64_t r = t; r < m; r += FDR_THREADS) p[r] = fdr_qnan();
            return;
        }
        double carry = suffix_min(part, t, fdr_inf());              // minimum over everything right of this thread's chunk
#pragma unroll
        for (int i = IPT - 1; i >= 0; --i) {
            if (r0 + i >= m) continue;
            carry = fmin(carry, fdr_proc_raw(M, fdr_key_value(key[i]), static_cast<double>(r0 + i + 1), n_d, c_by));
            p[idx[i]] = fdr_clamp(carry);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the count forms ----

// The same adjustment WITHOUT a sort, for p-values that are counts / num_permutations (the randomization form: every entry is one of
// P + 1 values): a row needs only its histogram over the counts (hist_to_table).  One workgroup per row: LDS histogram, the table,
// one table look-up per entry.  0.9 ms -> HBM speed per matrix at 3971 x 4373.  An entry that is not exactly c / P raises `flag`
// (the caller then sorts instead).
// M: the procedure.  Under Holm a NaN stays out of the histogram, stays in the count m and becomes 0x7FF8... on its own.
template <int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_row_counts(double *__restrict__ pvals, int64_t m, int64_t n_perm, double c_by,
                                                                unsigned int *__restrict__ flag) {
    extern __shared__ unsigned char fdr_lds[];
    const int bins = static_cast<int>(n_perm) + 1;
    double *adj = reinterpret_cast<double *>(fdr_lds);                    // [bins]
    unsigned int *hist = reinterpret_cast<unsigned int *>(adj + bins);   // [bins]
    __shared__ unsigned int bad;
    const int t = threadIdx.x;
    double *p = pvals + static_cast<int64_t>(blockIdx.x) * m;
    const double P = static_cast<double>(n_perm);
    for (int c = t; c < bins; c += FDR_THREADS) hist[c] = 0u;
    if (t == 0) bad = 0;
    __syncthreads();
    unsigned int mine_bad = 0;                                            // 1: a NaN (poisons the row), 2: not a count ratio
    for (int64_t e = t; e < m; e += FDR_THREADS) hist_add(hist, p[e], P, mine_bad);
    if (mine_bad) atomicOr(&bad, mine_bad);
    __syncthreads();
    if (bad & 2) {
        if (t == 0) atomicOr(flag, 1u);
        return;
    }
    if (fdr_proc_nan_poisons(M) && (bad & 1)) {                           // np.minimum propagates the NaN through the whole row
        for (int64_t e = t; e < m; e += FDR_THREADS) p[e] = fdr_qnan();
        return;
    }
    hist_to_table<M>(hist, bins, P, static_cast<double>(m), c_by, adj);
    __syncthreads();
    if constexpr (fdr_proc_nan_poisons(M)) {
        for (int64_t e = t; e < m; e += FDR_THREADS) p[e] = adj[static_cast<int>(fdr_count_of(p[e], P))];
    } else {
        for (int64_t e = t; e < m; e += FDR_THREADS) {
            const double v = p[e];
            p[e] = v != v ? fdr_qnan() : adj[static_cast<int>(fdr_count_of(v, P))];
        }
    }
}

// read-only: is every non-NaN entry a count ratio c / P, c in [0, P]?  (what the count forms need; anything else is sorted)
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_check_ratio(const double *__restrict__ p, int64_t total, double P, unsigned int *__restrict__ flag) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x;
    const bool bad = i < total && fdr_ratio_bin(p[i], P) == FDR_BIN_NOT_RATIO;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// slot[col][bin]: first the histogram (low word), then -- written by the lane that owns the bin -- the adjusted value
// M: the procedure (Holm: the first position of a tie and the running maximum over the lanes from the left; a NaN stays out of
// its column's histogram and becomes 0x7FF8... on its own)
template <int M>
__global__ __launch_bounds__(FDR_COL_THREADS) void k_fdr_col_counts(double *__restrict__ pvals, int64_t n, int64_t m, int64_t n_perm, int tile,
                                                        double c_by, unsigned int *__restrict__ flag) {
    extern __shared__ unsigned long long col_slot[];
    __shared__ int col_nan[FDR_COL_TILE_MAX];
    const int bins = static_cast<int>(n_perm) + 1;
    const int t = threadIdx.x;
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * tile;
    const int w = static_cast<int>(m - c0 < tile ? m - c0 : tile);
    // thread t walks column t % w, from row t / w on in steps of FDR_COL_THREADS / w rows: a wave reads whole row segments of the tile
    const int col = t % w, step = FDR_COL_THREADS / w;
    const int64_t row0 = t / w < step ? t / w : n;
    const double P = static_cast<double>(n_perm), n_d = static_cast<double>(n);
    for (int i = t; i < w * bins; i += FDR_COL_THREADS) col_slot[i] = 0ull;
    if (t < FDR_COL_TILE_MAX) col_nan[t] = 0;
    __syncthreads();
    for (int64_t row = row0; row < n; row += step) {
        const int bin = fdr_ratio_bin(pvals[row * m + c0 + col], P);
        if (bin >= 0) atomicAdd(reinterpret_cast<unsigned int *>(&col_slot[col * bins + bin]), 1u);
        else if (bin == FDR_BIN_NAN) atomicOr(&col_nan[col], 1);
        else atomicOr(flag, 1u);                                        // (cannot happen: the caller checked the matrix)
    }
    __syncthreads();
    // one wave per column: lane l owns the bins [b0, b1); hist_to_table's scan with wave shuffles in place of the LDS partials
    const int lane = t & 63;
    int b0, b1;
    fdr_span(bins, 64, lane, b0, b1);
    for (int wc = t >> 6; wc < w; wc += FDR_COL_THREADS / 64) {
        if (fdr_proc_nan_poisons(M) && col_nan[wc]) continue;
        unsigned long long *slot = col_slot + wc * bins;
        unsigned int local = 0;
        for (int c = b0; c < b1; ++c) local += static_cast<unsigned int>(slot[c]);
        unsigned int upto = local;                                      // inclusive sum over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int o = __shfl_up(upto, d);
            if (lane >= d) upto += o;
        }
        unsigned int cum = upto - local;
        if constexpr (fdr_proc_from_left(M)) {
            double mx = -fdr_inf();
            for (int c = b0; c < b1; ++c) {
                const unsigned int h = static_cast<unsigned int>(slot[c]);
                const double raw = h ? fdr_step_raw(static_cast<double>(c) / P, static_cast<double>(cum + 1u), n_d) : -fdr_inf();
                cum += h;
                slot[c] = static_cast<unsigned long long>(__double_as_longlong(raw));
                mx = fmax(mx, raw);
            }
            double left = mx;                                           // inclusive maximum over the lanes from the left
            for (int d = 1; d < 64; d <<= 1) {
                const double o = __shfl_up(left, d);
                if (lane >= d) left = fmax(left, o);
            }
            double carry = __shfl_up(left, 1);
            if (lane == 0) carry = -fdr_inf();
            for (int c = b0; c < b1; ++c) {
                carry = fmax(carry, fdr_key_value(slot[c]));
                slot[c] = static_cast<unsigned long long>(__double_as_longlong(fdr_clamp(carry)));
            }
            continue;
        }
        double mn = fdr_inf();
        for (int c = b0; c < b1; ++c) {
            const unsigned int h = static_cast<unsigned int>(slot[c]);
            cum += h;
            const double raw = h ? fdr_proc_raw(M, static_cast<double>(c) / P, static_cast<double>(cum), n_d, c_by) : fdr_inf();
            slot[c] = static_cast<unsigned long long>(__double_as_longlong(raw));
            mn = fmin(mn, raw);
        }
        double right = mn;                                              // inclusive minimum over the lanes from the right
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_down(right, d);
            if (lane + d < 64) right = fmin(right, o);
        }
        double carry = __shfl_down(right, 1);
        if (lane == 63) carry = fdr_inf();
        for (int c = b1 - 1; c >= b0; --c) {
            carry = fmin(carry, fdr_key_value(slot[c]));
            slot[c] = static_cast<unsigned long long>(__double_as_longlong(fdr_clamp(carry)));
        }
    }
    __syncthreads();
    for (int64_t row = row0; row < n; row += step) {
        double *cell = pvals + row * m + c0 + col;
        if (fdr_proc_nan_poisons(M) ? col_nan[col] != 0 : *cell != *cell) {   // np.minimum carries the NaN through the whole column
            *cell = fdr_qnan();
            continue;
        }
        const double cf = fdr_count_of(*cell, P);
        if (!(cf >= 0.0 && cf <= P)) continue;
        *cell = fdr_key_value(col_slot[col * bins + static_cast<int>(cf)]);
    }
}

// flags: 1 = a NaN, 2 = an entry that is no count ratio
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_hist(const double *__restrict__ p, int64_t total, int64_t n_perm,
                                                              unsigned long long *__restrict__ hist, unsigned int *__restrict__ flags) {
    extern __shared__ unsigned int all_hist[];
    const int bins = static_cast<int>(n_perm) + 1;
    const int t = threadIdx.x;
    const double P = static_cast<double>(n_perm);
    for (int c = t; c < bins; c += FDR_THREADS) all_hist[c] = 0u;
    __syncthreads();
    unsigned int bad = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + t; i < total; i += static_cast<int64_t>(gridDim.x) * FDR_THREADS)
        hist_add(all_hist, p[i], P, bad);
    if (bad) atomicOr(flags, bad);
    __syncthreads();
    for (int c = t; c < bins; c += FDR_THREADS)
        if (all_hist[c]) atomicAdd(&hist[c], static_cast<unsigned long long>(all_hist[c]));
}

// one workgroup: table[c] = the adjusted value of every entry with count c, from the one histogram in memory
template <int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_table(const unsigned long long *__restrict__ hist, int64_t n_perm, double total_d,
                                                               double c_by, double *__restrict__ table) {
    hist_to_table<M>(hist, static_cast<int>(n_perm) + 1, static_cast<double>(n_perm), total_d, c_by, table);
}

// POISON: a NaN anywhere turns the whole matrix into NaN (the procedures of the running minimum); else every NaN on its own
template <bool POISON>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_map(double *__restrict__ p, int64_t total, int64_t n_perm, const double *__restrict__ table,
                                                             const unsigned int *__restrict__ flags) {
    const unsigned int f = *flags;
    if (f & 2u) return;                                                 // (cannot happen: the caller checked the matrix)
    const double P = static_cast<double>(n_perm);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * FDR_THREADS) {
        if constexpr (POISON) {
            p[i] = (f & 1u) ? fdr_qnan() : table[static_cast<int>(fdr_count_of(p[i], P))];
        } else {
            const double v = p[i];
            p[i] = v != v ? fdr_qnan() : table[static_cast<int>(fdr_count_of(v, P))];
        }
    }
}

// Bonferroni, every scope: p count, clamped; a NaN becomes 0x7FF8... on its own, -0.0 is the value 0.0.  No sort, no histogram,
// no limit on n m.
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_bonferroni(double *__restrict__ p, int64_t total, double count_d) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * FDR_THREADS) {
        const double v = p[i];
        p[i] = v != v ? fdr_qnan() : fdr_clamp(fdr_bonferroni_raw(fdr_plus_zero(v), count_d));
    }
}

// -------------------------------------------------------------------------------------------------- columns, sort form ----

// out[c][r] = in[r][c]; one 32 x 32 tile per workgroup, tiles numbered along the columns of `in` first
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_transpose(const double *__restrict__ in, int64_t rows, int64_t cols, double *__restrict__ out) {
    __shared__ double tile[FDR_TR_TILE][FDR_TR_TILE + 1];
    const int64_t tiles_c = (cols + FDR_TR_TILE - 1) / FDR_TR_TILE;
    const int64_t tr = static_cast<int64_t>(blockIdx.x) / tiles_c, tc = static_cast<int64_t>(blockIdx.x) - tr * tiles_c;
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (int k = y; k < FDR_TR_TILE; k += 8) {
        const int64_t r = tr * FDR_TR_TILE + k, c = tc * FDR_TR_TILE + x;
        if (r < rows && c < cols) tile[k][x] = in[r * cols + c];
    }
    __syncthreads();
    for (int k = y; k < FDR_TR_TILE; k += 8) {
        const int64_t c = tc * FDR_TR_TILE + k, r = tr * FDR_TR_TILE + x;
        if (r < rows && c < cols) out[c * rows + r] = tile[x][k];
    }
}

// --------------------------------------------------------------------------------------------------- matrix, sort form ----

__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_keys(const double *__restrict__ p, int64_t total, unsigned long long *__restrict__ keys,
                                                              unsigned int *__restrict__ cells) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x;
    if (i >= total) return;
    keys[i] = fdr_key(p[i]);
    cells[i] = static_cast<unsigned int>(i);
}

template <int M>
__device__ __forceinline__ double all_raw(const unsigned long long *__restrict__ keys, int64_t r, double total_d, double c_by) {
    return fdr_proc_raw(M, fdr_key_value(keys[r]), static_cast<double>(r + 1), total_d, c_by);
}
// the identity and the join of a procedure's running extreme: -inf / fmax from the left (Holm), +inf / fmin from the right
template <bool LEFT>
__device__ __forceinline__ double scan_identity() { return LEFT ? -fdr_inf() : fdr_inf(); }
template <bool LEFT>
__device__ __forceinline__ double scan_join(double a, double b) { return LEFT ? fmax(a, b) : fmin(a, b); }

// workgroup b: the minimum (Holm: the maximum, over the numbers) of the raw values of the sorted ranks
// [b FDR_ALL_BLOCK, (b + 1) FDR_ALL_BLOCK)
template <int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_blockmin(const unsigned long long *__restrict__ keys, int64_t total, double c_by,
                                                                  double *__restrict__ blockmin) {
    constexpr bool LEFT = fdr_proc_from_left(M);
    __shared__ double part[FDR_THREADS];
    const int t = threadIdx.x;
    const double total_d = static_cast<double>(total);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * FDR_ALL_BLOCK + t * FDR_ALL_IPT;
    double mine = scan_identity<LEFT>();
    for (int i = 0; i < FDR_ALL_IPT; ++i)
        if (r0 + i < total && !(LEFT && keys[r0 + i] == FDR_KEY_NAN)) mine = scan_join<LEFT>(mine, all_raw<M>(keys, r0 + i, total_d, c_by));
    part[t] = mine;
    __syncthreads();
    for (int s = FDR_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = scan_join<LEFT>(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) blockmin[blockIdx.x] = part[0];
}

// one workgroup: carry[b] = the minimum over every workgroup right of b; LEFT (Holm): the maximum over every workgroup left of b
template <bool LEFT>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_carry(const double *__restrict__ blockmin, int64_t blocks, double *__restrict__ carry) {
    __shared__ double part[FDR_THREADS];
    const int t = threadIdx.x;
    int64_t b0, b1;
    fdr_span<int64_t>(blocks, FDR_THREADS, t, b0, b1);
    double mine = scan_identity<LEFT>();
    for (int64_t b = b0; b < b1; ++b) mine = scan_join<LEFT>(mine, blockmin[b]);
    part[t] = mine;
    __syncthreads();
    if constexpr (LEFT) {
        double run = prefix_max(part, t, -fdr_inf());
        for (int64_t b = b0; b < b1; ++b) {
            carry[b] = run;
            run = fmax(run, blockmin[b]);
        }
    } else {
        double run = suffix_min(part, t, fdr_inf());
        for (int64_t b = b1 - 1; b >= b0; --b) {
            carry[b] = run;
            run = fmin(run, blockmin[b]);
        }
    }
}

// the running minimum from the right inside the workgroup's ranks, joined with carry[b], written to the cells the ranks came from;
// Holm: the running maximum from the left, and every NaN key (they sit behind the numbers) written as NaN on its own
template <int M>
__global__ __launch_bounds__(FDR_THREADS) void k_fdr_all_apply(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ cells,
                                                               int64_t total, double c_by, const double *__restrict__ carry,
                                                               double *__restrict__ out) {
    __shared__ double part[FDR_THREADS];
    const int t = threadIdx.x;
    const double total_d = static_cast<double>(total);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * FDR_ALL_BLOCK + t * FDR_ALL_IPT;
    if constexpr (fdr_proc_from_left(M)) {
        double mine = -fdr_inf();
        for (int i = 0; i < FDR_ALL_IPT; ++i)
            if (r0 + i < total && keys[r0 + i] != FDR_KEY_NAN) mine = fmax(mine, all_raw<M>(keys, r0 + i, total_d, c_by));
        part[t] = mine;
        __syncthreads();
        double run = prefix_max(part, t, carry[blockIdx.x]);
        for (int i = 0; i < FDR_ALL_IPT; ++i) {
            if (r0 + i >= total) continue;
            if (keys[r0 + i] == FDR_KEY_NAN) {
                out[cells[r0 + i]] = fdr_qnan();
                continue;
            }
            run = fmax(run, all_raw<M>(keys, r0 + i, total_d, c_by));
            out[cells[r0 + i]] = fdr_clamp(run);
        }
    } else {
        // every NaN carries the largest key: the matrix has one iff the last sorted key is one, and then all of it becomes NaN
        if (keys[total - 1] == FDR_KEY_NAN) {
            for (int i = 0; i < FDR_ALL_IPT; ++i)
                if (r0 + i < total) out[cells[r0 + i]] = fdr_qnan();
            return;
        }
        double mine = fdr_inf();
        for (int i = 0; i < FDR_ALL_IPT; ++i)
            if (r0 + i < total) mine = fmin(mine, all_raw<M>(keys, r0 + i, total_d, c_by));
        part[t] = mine;
        __syncthreads();
        double run = suffix_min(part, t, carry[blockIdx.x]);
        for (int i = FDR_ALL_IPT - 1; i >= 0; --i) {
            if (r0 + i >= total) continue;
            run = fmin(run, all_raw<M>(keys, r0 + i, total_d, c_by));
            out[cells[r0 + i]] = fdr_clamp(run);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- the epilogue ----

// NES / binarisation from (adjusted) p-values; n_perm == 0: hypergeometric form nes = -log10(p_pos)
__global__ __launch_bounds__(256) void k_nes_from_pvalues(const double *__restrict__ p_neg, const double *__restrict__ p_pos,
                                                          int64_t n, int64_t m, double inv_perm, int sign_mode,
                                                          double nes_threshold, double p_cut, double *__restrict__ nes_out,
                                                          double *__restrict__ nes_binary, unsigned int *__restrict__ enriched) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x & 63);
    const int64_t i0 = static_cast<int64_t>(blockIdx.y) * 64 + (threadIdx.x >> 6);
    if (c >= m) return;
    unsigned int hits = 0;
    for (int64_t i = i0; i < n && i < (static_cast<int64_t>(blockIdx.y) + 1) * 64; i += 4) {
        const int64_t o = i * m + c;
        double nes;
        bool hit;
        // where the NES is one logarithm, the binarisation is decided on p itself (nes_p_cut, common.h):
        // the device's log10 may round differently from the host libm the reference calls
        if (inv_perm == 0.0) {
            nes = -log10(p_pos[o]);                                  // safe.py:608
            hit = p_pos[o] < p_cut;                                  // safe.py:468-470
        } else {                                                     // safe.py:546-554
            const double pp = p_pos[o] == 0.0 ? inv_perm : p_pos[o], pn = p_neg[o] == 0.0 ? inv_perm : p_neg[o];
            const double ep = -log10(pp), en = -log10(pn);
            nes = sign_mode == SAFE_SIGN_HIGHEST ? ep : sign_mode == SAFE_SIGN_LOWEST ? en : ep - en;
            hit = sign_mode == SAFE_SIGN_HIGHEST ? pp < p_cut
                  : sign_mode == SAFE_SIGN_LOWEST ? pn < p_cut
                                                  : (nes == nes) && (fabs(nes) > nes_threshold);
        }
        nes_out[o] = nes;
        nes_binary[o] = hit ? 1.0 : 0.0;
        hits += hit;
    }
    if (hits) atomicAdd(&enriched[c], hits);
}

__global__ void k_fdr_u32_to_f64(const unsigned int *__restrict__ in, double *__restrict__ out, int64_t count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * FDR_THREADS + threadIdx.x;
    if (i < count) out[i] = static_cast<double>(in[i]);
}

// ------------------------------------------------------------------------------------------------------------- host ----

// the end of every form: its launches are checked and the stream has drained
int drained(safe_ctx *ctx, const char *who) {
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

// the u32 at d_flag, read once the launches before it are checked and the stream has drained
int read_flag(safe_ctx *ctx, const char *who, const unsigned int *d_flag, unsigned int *value) {
    void *pinned = nullptr;
    SAFE_TRY(ctx_pinned(ctx, sizeof(unsigned int), &pinned));
    SAFE_HIP_CHECK(hipMemcpyAsync(pinned, d_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_TRY(drained(ctx, who));
    *value = *static_cast<unsigned int *>(pinned);
    return SAFE_OK;
}

// ... of the context's flag, zeroed for the kernels `launch(flag)` starts
template <typename Launch>
int with_flag(safe_ctx *ctx, const char *who, Launch launch, unsigned int *value) {
    unsigned int *d_flag = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_FDR_FLAG, sizeof(unsigned int), reinterpret_cast<void **>(&d_flag)));
    SAFE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(unsigned int), ctx->stream));
    launch(d_flag);
    return read_flag(ctx, who, d_flag, value);
}

// the end of a count form: `bad` is what its kernels left in the flag (cannot happen: the entry point validated the matrix before
// it chose the form)
int count_form_done(const char *who, unsigned int bad, int64_t n_perm) {
    if (!bad) return SAFE_OK;
    safe_set_error("%s: a p-value is not a multiple of 1 / %lld", who, (long long)n_perm);
    return SAFE_E_VALUE;
}

// The procedure of a call: `proc` (FdrProcedure, one of the four that sort) and Benjamini-Yekutieli's constant
struct FdrProc {
    int proc;
    double c_by;
};

// f(std::integral_constant<int, M>) for the sorted procedure `proc`: the kernels take it as a template parameter
template <typename F>
auto with_proc(int proc, F f) {
    switch (proc) {
    case FDR_PROC_BY: return f(std::integral_constant<int, FDR_PROC_BY>{});
    case FDR_PROC_HOLM: return f(std::integral_constant<int, FDR_PROC_HOLM>{});
    case FDR_PROC_HOCHBERG: return f(std::integral_constant<int, FDR_PROC_HOCHBERG>{});
    default: return f(std::integral_constant<int, FDR_PROC_BH>{});
    }
}

template <int M, int K = 0>
void launch_row_sort(int ipt, hipStream_t stream, double *p_dev, int64_t n, int64_t m, double c_by) {
    if constexpr (K < FDR_IPT_RUNGS) {
        if (ipt == FDR_IPT_LADDER[K])
            hipLaunchKernelGGL((k_fdr_row_sort<FDR_IPT_LADDER[K], M>), dim3(n), dim3(FDR_THREADS), 0, stream, p_dev, m, c_by);
        else launch_row_sort<M, K + 1>(ipt, stream, p_dev, n, m, c_by);
    }
}

// The procedure pr on every row of p_dev (f64 [n, m] row-major) in place, in the row form `kind` of f.  n_perm: the count
// denominator of the histogram form.  The stream has drained when it returns.
int adjust_rows(safe_ctx *ctx, const char *who, FdrProc pr, FdrKind kind, const FdrForm &f, double *p_dev, int64_t n, int64_t m,
                int64_t n_perm) {
    if (kind == FDR_ROW_HIST) {
        unsigned int bad = 0;
        SAFE_HIP_CHECK(with_proc(pr.proc, [&](auto M) {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdr_row_counts<decltype(M)::value>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(f.lds_bytes));
        }));
        SAFE_TRY(with_flag(ctx, who, [&](unsigned int *flag) {
            with_proc(pr.proc, [&](auto M) {
                hipLaunchKernelGGL(k_fdr_row_counts<decltype(M)::value>, dim3(n), dim3(FDR_THREADS), f.lds_bytes, ctx->stream, p_dev, m, n_perm,
                                   pr.c_by, flag);
            });
        }, &bad));
        return count_form_done(who, bad, n_perm);
    }
    if (kind == FDR_ROW_BLOCK_SORT) {
        with_proc(pr.proc, [&](auto M) { launch_row_sort<decltype(M)::value>(f.ipt, ctx->stream, p_dev, n, m, pr.c_by); });
        return drained(ctx, who);
    }
    SAFE_REQUIRE(kind == FDR_ROW_LIBRARY_SORT, "%s: %lld attributes per row are too many", who, (long long)m);
    const int64_t batch_rows = f.batch_rows, batch_items = batch_rows * m;
    double *keys_out = nullptr;
    int32_t *vals_in = nullptr, *vals_out = nullptr;
    int64_t *offsets = nullptr;
    uint8_t *temp = nullptr;
    size_t temp_bytes = 0;
    CallBufs b;
    SAFE_TRY(b.alloc(&keys_out, batch_items));
    SAFE_TRY(b.alloc(&vals_in, batch_items));
    SAFE_TRY(b.alloc(&vals_out, batch_items));
    SAFE_TRY(b.alloc(&offsets, batch_rows + 1));
    hipLaunchKernelGGL(k_fdr_cols, dim3(ceil_div(batch_items, FDR_THREADS)), dim3(FDR_THREADS), 0, ctx->stream, vals_in, batch_items, m);
    hipLaunchKernelGGL(k_fdr_offsets, dim3(ceil_div(batch_rows + 1, FDR_THREADS)), dim3(FDR_THREADS), 0, ctx->stream, offsets, batch_rows, m);
    SAFE_HIP_CHECK_AS(who, hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, temp_bytes, p_dev, keys_out, vals_in, vals_out,
                                                                       static_cast<int>(batch_items), static_cast<int>(batch_rows),
                                                                       offsets, offsets + 1, 0, 64, ctx->stream));
    SAFE_TRY(b.alloc(&temp, std::max<size_t>(temp_bytes, 16)));
    for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
        const int64_t rows = std::min<int64_t>(batch_rows, n - r0);
        double *block = p_dev + r0 * m;
        SAFE_HIP_CHECK_AS(who, hipcub::DeviceSegmentedRadixSort::SortPairs(temp, temp_bytes, block, keys_out, vals_in, vals_out,
                                                                           static_cast<int>(rows * m), static_cast<int>(rows), offsets,
                                                                           offsets + 1, 0, 64, ctx->stream));
        with_proc(pr.proc, [&](auto M) {
            hipLaunchKernelGGL(k_fdr_row<decltype(M)::value>, dim3(rows), dim3(FDR_THREADS), 0, ctx->stream, keys_out, vals_out, m, pr.c_by, block);
        });
        SAFE_HIP_CHECK_AS(who, hipGetLastError());
    }
    return drained(ctx, who);
}

int adjust_cols_counts(safe_ctx *ctx, const char *who, FdrProc pr, const FdrForm &f, double *p_dev, int64_t n, int64_t m, int64_t n_perm) {
    unsigned int bad = 0;
    SAFE_HIP_CHECK(with_proc(pr.proc, [&](auto M) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdr_col_counts<decltype(M)::value>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(f.lds_bytes));
    }));
    SAFE_TRY(with_flag(ctx, who, [&](unsigned int *flag) {
        with_proc(pr.proc, [&](auto M) {
            hipLaunchKernelGGL(k_fdr_col_counts<decltype(M)::value>, dim3(ceil_div(m, f.tile)), dim3(FDR_COL_THREADS), f.lds_bytes, ctx->stream,
                               p_dev, n, m, n_perm, f.tile, pr.c_by, flag);
        });
    }, &bad));
    return count_form_done(who, bad, n_perm);
}

int adjust_cols_sort(safe_ctx *ctx, const char *who, FdrProc pr, const FdrForm &f, double *p_dev, int64_t n, int64_t m) {
    CallBufs b;
    double *t_dev = nullptr;
    SAFE_TRY(b.alloc(&t_dev, n * m));
    const int64_t tiles = ceil_div(n, FDR_TR_TILE) * ceil_div(m, FDR_TR_TILE);
    hipLaunchKernelGGL(k_fdr_transpose, dim3(tiles), dim3(FDR_THREADS), 0, ctx->stream, p_dev, n, m, t_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_TRY(adjust_rows(ctx, who, pr, f.row_kind, f, t_dev, m, n, 0));
    hipLaunchKernelGGL(k_fdr_transpose, dim3(tiles), dim3(FDR_THREADS), 0, ctx->stream, t_dev, m, n, p_dev);
    return drained(ctx, who);
}

int adjust_all_counts(safe_ctx *ctx, const char *who, FdrProc pr, const FdrForm &f, double *p_dev, int64_t total, int64_t n_perm) {
    const int64_t bins = n_perm + 1;
    unsigned long long *hist = nullptr;                              // [bins], then the table f64 [bins], then the u32 flags
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_FDR_SCOPE, static_cast<size_t>(bins) * 16 + 16, reinterpret_cast<void **>(&hist)));
    double *table = reinterpret_cast<double *>(hist + bins);
    unsigned int *flags = reinterpret_cast<unsigned int *>(table + bins), bad = 0;
    SAFE_HIP_CHECK(hipMemsetAsync(hist, 0, static_cast<size_t>(bins) * 16 + 16, ctx->stream));       // (one fill for all three)
    const int64_t grid = std::min<int64_t>(ceil_div(total, FDR_THREADS), 2048);
    SAFE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdr_all_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(f.lds_bytes)));
    hipLaunchKernelGGL(k_fdr_all_hist, dim3(grid), dim3(FDR_THREADS), f.lds_bytes, ctx->stream, p_dev, total, n_perm, hist, flags);
    with_proc(pr.proc, [&](auto M) {
        constexpr int proc = decltype(M)::value;
        hipLaunchKernelGGL(k_fdr_all_table<proc>, dim3(1), dim3(FDR_THREADS), 0, ctx->stream, hist, n_perm, static_cast<double>(total), pr.c_by,
                           table);
        hipLaunchKernelGGL(k_fdr_all_map<fdr_proc_nan_poisons(proc)>, dim3(grid), dim3(FDR_THREADS), 0, ctx->stream, p_dev, total, n_perm, table,
                           flags);
    });
    SAFE_TRY(read_flag(ctx, who, flags, &bad));
    return count_form_done(who, bad & 2u, n_perm);
}

int adjust_all_sort(safe_ctx *ctx, const char *who, FdrProc pr, double *p_dev, int64_t total) {
    CallBufs b;
    unsigned long long *keys_in = nullptr, *keys_out = nullptr;
    unsigned int *cells_in = nullptr, *cells_out = nullptr;
    double *blockmin = nullptr, *carry = nullptr;
    uint8_t *temp = nullptr;
    size_t temp_bytes = 0;
    const int64_t blocks = ceil_div(total, FDR_ALL_BLOCK);
    SAFE_TRY(b.alloc(&keys_in, total));
    SAFE_TRY(b.alloc(&keys_out, total));
    SAFE_TRY(b.alloc(&cells_in, total));
    SAFE_TRY(b.alloc(&cells_out, total));
    SAFE_TRY(b.alloc(&blockmin, blocks));
    SAFE_TRY(b.alloc(&carry, blocks));
    SAFE_HIP_CHECK_AS(who, hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, keys_in, keys_out, cells_in, cells_out,
                                                              static_cast<int>(total), 0, 64, ctx->stream));
    SAFE_TRY(b.alloc(&temp, std::max<size_t>(temp_bytes, 16)));
    hipLaunchKernelGGL(k_fdr_all_keys, dim3(ceil_div(total, FDR_THREADS)), dim3(FDR_THREADS), 0, ctx->stream, p_dev, total, keys_in, cells_in);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, cells_in, cells_out,
                                                              static_cast<int>(total), 0, 64, ctx->stream));
    with_proc(pr.proc, [&](auto M) {
        constexpr int proc = decltype(M)::value;
        hipLaunchKernelGGL(k_fdr_all_blockmin<proc>, dim3(blocks), dim3(FDR_THREADS), 0, ctx->stream, keys_out, total, pr.c_by, blockmin);
        hipLaunchKernelGGL(k_fdr_all_carry<fdr_proc_from_left(proc)>, dim3(1), dim3(FDR_THREADS), 0, ctx->stream, blockmin, blocks, carry);
        hipLaunchKernelGGL(k_fdr_all_apply<proc>, dim3(blocks), dim3(FDR_THREADS), 0, ctx->stream, keys_out, cells_out, total, pr.c_by, carry,
                           p_dev);
    });
    return drained(ctx, who);
}

// One matrix along `scope`, in place: the form from fdr_plan.h, then its launches.  hist_perm > 0: every entry is a count ratio
// c / hist_perm (checked).  Bonferroni takes no form: one element-wise pass with the size of the family.  The stream has drained
// when it returns.
int adjust_matrix(safe_ctx *ctx, const char *who, FdrProc pr, FdrSwitch sw, int scope, double *p_dev, int64_t n, int64_t m,
                  int64_t hist_perm) {
    if (!fdr_proc_sorts(pr.proc)) {
        const int64_t total = n * m, grid = std::min<int64_t>(ceil_div(total, FDR_THREADS), 8192);
        const int64_t count = scope == FDR_SCOPE_ROWS ? m : scope == FDR_SCOPE_COLS ? n : total;
        hipLaunchKernelGGL(k_fdr_bonferroni, dim3(grid), dim3(FDR_THREADS), 0, ctx->stream, p_dev, total, static_cast<double>(count));
        return drained(ctx, who);
    }
    const FdrForm f = fdr_form(scope, n, m, hist_perm, sw);
    switch (f.kind) {
    case FDR_UNSUPPORTED:
        safe_set_error("%s: %lld x %lld p-values as one family are beyond the library sort (2^31 items)", who, (long long)n, (long long)m);
        return SAFE_E_UNSUPPORTED;
    case FDR_COL_COUNTS: return adjust_cols_counts(ctx, who, pr, f, p_dev, n, m, hist_perm);
    case FDR_COL_SORT: return adjust_cols_sort(ctx, who, pr, f, p_dev, n, m);
    case FDR_ALL_COUNTS: return adjust_all_counts(ctx, who, pr, f, p_dev, n * m, hist_perm);
    case FDR_ALL_SORT: return adjust_all_sort(ctx, who, pr, p_dev, n * m);
    default: return adjust_rows(ctx, who, pr, f.kind, f, p_dev, n, m, hist_perm);
    }
}

// What an entry point asks for: the matrices pos (and neg, in the randomization form of the entry points with an epilogue) of
// f64 [n, m] adjusted in place along `scope`; nes != NULL: then nes, nes_binary and the per-attribute counts from the adjusted values.
struct FdrCall {
    const char *who;               // the entry point, for error texts
    int bad_arguments;             // its code for them: SAFE_E_INVALID (safe_fdr_adjust, _rows) or SAFE_E_VALUE (_scope, _matrix)
    bool epilogue;
    int64_t n, m, n_perm;
    int scope, sign_mode;
    double enrichment_threshold;
    double *neg, *pos, *nes, *nes_binary, *num_enriched;
    int method = SAFE_MT_FDR_BH;   // SAFE_MT_*: the safe_fdr_* entry points are Benjamini-Hochberg
    double by_constant = 0.0;      // SAFE_MT_FDR_BY only
};

// (SAFE_REQUIRE: SAFE_E_INVALID, which run turns into the entry point's own code)
int validate(const safe_ctx *ctx, const FdrCall &c) {
    SAFE_REQUIRE(ctx && c.pos && (!c.epilogue || (c.nes && c.nes_binary && c.num_enriched)), "%s: NULL argument", c.who);
    SAFE_REQUIRE(c.n >= 1 && c.m >= 1 && c.n_perm >= 0, "%s: bad sizes", c.who);
    if (c.epilogue) {
        SAFE_REQUIRE(c.n_perm == 0 || c.neg, "%s: the randomization form needs pvalues_neg", c.who);
        SAFE_REQUIRE(c.sign_mode >= SAFE_SIGN_HIGHEST && c.sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", c.who, c.sign_mode);
        SAFE_REQUIRE(c.enrichment_threshold > 0.0 && c.enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", c.who);
    }
    SAFE_REQUIRE(c.scope >= SAFE_FDR_SCOPE_ROWS && c.scope <= SAFE_FDR_SCOPE_ALL, "%s: bad scope %d", c.who, c.scope);
    SAFE_REQUIRE(c.method >= SAFE_MT_FDR_BH && c.method <= SAFE_MT_BONFERRONI, "%s: bad method %d", c.who, c.method);
    SAFE_REQUIRE(c.method != SAFE_MT_FDR_BY || (std::isfinite(c.by_constant) && c.by_constant >= 1.0),
                 "%s: by_constant %g is not the harmonic sum of a family (finite, at least 1)", c.who, c.by_constant);
    return SAFE_OK;
}

// The body of the four entry points.  The library's own empirical p-values are count ratios c / num_permutations and need no
// sort.  A caller may hand over other values with num_permutations > 0 (only the 0 -> 1 / P rule of the NES depends on it): where
// a count form exists the matrices are checked READ-ONLY first (k_fdr_check_ratio), and one entry of either that is not a count
// ratio sends both through the sort, like the hypergeometric form.  A refusal writes nothing.
int run(safe_ctx *ctx, const FdrCall &c) {
    if (validate(ctx, c) != SAFE_OK) return c.bad_arguments;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const FdrSwitch sw = fdr_switch(getenv("SAFE_HIP_FDR_SORT"));
    const int n_mats = c.epilogue && c.n_perm > 0 ? 2 : 1;             // the randomization form: pvalues_neg, then pvalues_pos
    double *mats[2] = {n_mats == 2 ? c.neg : c.pos, c.pos};
    const FdrProc pr = {c.method, c.method == SAFE_MT_FDR_BY ? c.by_constant : 0.0};
    int64_t hist_perm = 0;
    if (fdr_proc_sorts(pr.proc) && fdr_count_form_exists(c.scope, c.n_perm, sw)) {
        unsigned int bad = 0;
        SAFE_TRY(with_flag(ctx, c.who, [&](unsigned int *flag) {
            for (int k = 0; k < n_mats; ++k)
                hipLaunchKernelGGL(k_fdr_check_ratio, dim3(ceil_div(c.n * c.m, FDR_THREADS)), dim3(FDR_THREADS), 0, ctx->stream, mats[k],
                                   c.n * c.m, static_cast<double>(c.n_perm), flag);
        }, &bad));
        if (!bad) hist_perm = c.n_perm;
    }
    for (int k = 0; k < n_mats; ++k) SAFE_TRY(adjust_matrix(ctx, c.who, pr, sw, c.scope, mats[k], c.n, c.m, hist_perm));
    if (!c.epilogue) return SAFE_OK;
    CallBufs b;
    unsigned int *d_enr = nullptr;
    SAFE_TRY(b.alloc(&d_enr, c.m));
    SAFE_HIP_CHECK(hipMemsetAsync(d_enr, 0, c.m * sizeof(unsigned int), ctx->stream));
    hipLaunchKernelGGL(k_nes_from_pvalues, dim3(ceil_div(c.m, 64), ceil_div(c.n, 64)), dim3(256), 0, ctx->stream, c.neg, c.pos, c.n, c.m,
                       c.n_perm > 0 ? 1.0 / static_cast<double>(c.n_perm) : 0.0, c.sign_mode, -std::log10(c.enrichment_threshold),
                       nes_p_cut(c.enrichment_threshold), c.nes, c.nes_binary, d_enr);
    hipLaunchKernelGGL(k_fdr_u32_to_f64, dim3(ceil_div(c.m, FDR_THREADS)), dim3(FDR_THREADS), 0, ctx->stream, d_enr, c.num_enriched, c.m);
    return drained(ctx, c.who);
}

}  // namespace

extern "C" int safe_fdr_adjust(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                               double enrichment_threshold, double *pvalues_neg_dev, double *pvalues_pos_dev, double *nes_dev,
                               double *nes_binary_dev, double *num_enriched_dev) {
    return run(ctx, {"safe_fdr_adjust", SAFE_E_INVALID, true, n, m, num_permutations, SAFE_FDR_SCOPE_ROWS, sign_mode, enrichment_threshold,
                     pvalues_neg_dev, pvalues_pos_dev, nes_dev, nes_binary_dev, num_enriched_dev});
}

// Benjamini-Hochberg on every row of one matrix, in place: the sort form (what safe_fdr_adjust with num_permutations = 0 does to
// pvalues_pos), without the NES epilogue
extern "C" int safe_fdr_adjust_rows(safe_ctx *ctx, int64_t n, int64_t m, double *p_dev) {
    return run(ctx, {"safe_fdr_adjust_rows", SAFE_E_INVALID, false, n, m, 0, SAFE_FDR_SCOPE_ROWS, 0, 0.0, nullptr, p_dev, nullptr, nullptr, nullptr});
}

extern "C" int safe_fdr_adjust_scope(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                                     double enrichment_threshold, int scope, double *pvalues_neg_dev, double *pvalues_pos_dev,
                                     double *nes_dev, double *nes_binary_dev, double *num_enriched_dev) {
    return run(ctx, {"safe_fdr_adjust_scope", SAFE_E_VALUE, true, n, m, num_permutations, scope, sign_mode, enrichment_threshold,
                     pvalues_neg_dev, pvalues_pos_dev, nes_dev, nes_binary_dev, num_enriched_dev});
}

extern "C" int safe_fdr_adjust_matrix(safe_ctx *ctx, int64_t n, int64_t m, int scope, int64_t count_denominator, double *p_dev) {
    return run(ctx, {"safe_fdr_adjust_matrix", SAFE_E_VALUE, false, n, m, count_denominator, scope, 0, 0.0, nullptr, p_dev, nullptr, nullptr,
                     nullptr});
}

// safe_fdr_adjust_scope with the procedure named by `method` (SAFE_MT_*); SAFE_MT_FDR_BH gives its bytes
extern "C" int safe_mt_adjust_scope(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                                    double enrichment_threshold, int scope, int method, double by_constant, double *pvalues_neg_dev,
                                    double *pvalues_pos_dev, double *nes_dev, double *nes_binary_dev, double *num_enriched_dev) {
    return run(ctx, {"safe_mt_adjust_scope", SAFE_E_VALUE, true, n, m, num_permutations, scope, sign_mode, enrichment_threshold,
                     pvalues_neg_dev, pvalues_pos_dev, nes_dev, nes_binary_dev, num_enriched_dev, method, by_constant});
}

// safe_fdr_adjust_matrix with the procedure named by `method`
extern "C" int safe_mt_adjust_matrix(safe_ctx *ctx, int64_t n, int64_t m, int scope, int method, double by_constant,
                                     int64_t count_denominator, double *p_dev) {
    return run(ctx, {"safe_mt_adjust_matrix", SAFE_E_VALUE, false, n, m, count_denominator, scope, 0, 0.0, nullptr, p_dev, nullptr, nullptr,
                     nullptr, method, by_constant});
}
