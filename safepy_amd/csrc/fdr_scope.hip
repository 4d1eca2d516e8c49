// multiple_testing_scope: Benjamini-Hochberg along another family than the reference's.  fdr.hip adjusts every ROW of a p-value
// matrix (one node's neighborhood across its m attributes: safepy/safe.py:536-542, 599-605); here the family is every COLUMN
// (one attribute across the n neighborhoods: np.apply_along_axis(lambda c: fdrcorrection(c)[1], 0, p)) or the WHOLE matrix
// (fdrcorrection(p.ravel())[1].reshape(p.shape)).  The arithmetic is statsmodels', operation by operation, as fdr.hip's header
// spells it out: raw = p_(r) / ((r + 1) / count), both divisions on the same doubles, a running minimum from the right, values
// above 1 become 1; count = n for a column, n m for the whole matrix, exact in f64.  A NaN of either sign and any payload
// anywhere in a family turns the whole family into 0x7FF8... -- for the whole-matrix scope that is the whole matrix -- and -0.0
// is the value 0.0.  All counting is in integers and fmin of numbers does not depend on the order, so identical calls give
// identical bytes.
//
//   columns, count form   k_fdr_col_counts: p = c / P with P <= FDR_COL_HIST_MAX_P.  A workgroup owns a tile of adjacent columns
//                         (its row reads are contiguous), one LDS histogram of P + 1 bins per column; a wave turns a column's
//                         histogram into the table of adjusted values (the column twin of k_fdr_row_counts, the same rint(p P)
//                         bin rule); one table look-up per entry.
//   columns, sort form    tiled LDS transpose into per-call memory, fdr_matrix (fdr.hip: block sort up to 8192 per family, the
//                         library sort beyond) on the [m, n] transpose, transpose back.
//   matrix, count form    P <= FDR_ALL_HIST_MAX_P: k_fdr_all_hist (per-workgroup LDS histograms flushed with integer atomics
//                         into 64-bit counters), k_fdr_all_table (one workgroup: the P + 1 adjusted values), k_fdr_all_map.
//                         Two reads and one write of the matrix.
//   matrix, sort form     one device-wide radix sort of the n m keys (the key transform of k_fdr_row_sort) with the cell index as
//                         payload; the running minimum from the right as per-block minima (k_fdr_all_blockmin), a carry pass
//                         (k_fdr_all_carry) and the apply pass, which scatters back (k_fdr_all_apply).  The keys-only sort with
//                         a binary search per cell was not built.  n m >= 2^31 is beyond the library sort: SAFE_E_UNSUPPORTED.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "fdr_shared.h"

namespace {

constexpr int FDR_COL_LDS_BYTES = 128 * 1024;          // of the CU's 160 KiB: the tile's tables (8 bytes per bin and column)
constexpr int FDR_COL_TILE_MAX = 16;                   // columns of a tile: 128-byte row segments
constexpr int FDR_COL_THREADS = 1024;                  // a tile of 16 tables takes a CU's LDS alone: the one workgroup brings 16 waves
                                                       // (256 threads: 0.55 ms per 3971 x 4373 matrix at P = 1000, 1024: 0.28 ms)
constexpr int FDR_COL_TILE_MIN = 4;                    // below that the column reads fall apart: the sort form takes over
constexpr int64_t FDR_COL_HIST_MAX_P = FDR_COL_LDS_BYTES / (8 * FDR_COL_TILE_MIN) - 1;   // 4095
constexpr int64_t FDR_ALL_HIST_MAX_P = 64 * 1024 / 4 - 1;                                // 16383: a u32 histogram in 64 KiB
constexpr int FDR_TR_TILE = 32;                        // transpose tile, 32 x 32 doubles
constexpr int FDR_ALL_IPT = 8;                         // sorted ranks per thread of the whole-matrix suffix minimum
constexpr int FDR_ALL_BLOCK = 256 * FDR_ALL_IPT;       // ... per workgroup
constexpr int64_t FDR_SORT_MAX_ITEMS = int64_t(1) << 31;

__device__ __forceinline__ double scope_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double scope_qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

// ------------------------------------------------------------------------------------------------ columns, count form ----

// slot[col][bin]: first the histogram (low word), then -- written by the lane that owns the bin -- the adjusted value
__global__ __launch_bounds__(FDR_COL_THREADS) void k_fdr_col_counts(double *__restrict__ pvals, int64_t n, int64_t m, int64_t n_perm, int tile,
                                                        unsigned int *__restrict__ flag) {
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
        const double v = pvals[row * m + c0 + col];
        if (v != v) {
            atomicOr(&col_nan[col], 1);
            continue;
        }
        const double cf = rint(v * P);
        if (!(cf >= 0.0 && cf <= P) || cf / P != v) {                  // (cannot happen: the caller checked the matrix)
            atomicOr(flag, 1u);
            continue;
        }
        atomicAdd(reinterpret_cast<unsigned int *>(&col_slot[col * bins + static_cast<int>(cf)]), 1u);
    }
    __syncthreads();
    // one wave per column: lane l owns the bins [b0, b1)
    const int lane = t & 63;
    const int per = (bins + 63) / 64, b0 = lane * per < bins ? lane * per : bins, b1 = b0 + per < bins ? b0 + per : bins;
    for (int wc = t >> 6; wc < w; wc += FDR_COL_THREADS / 64) {
        if (col_nan[wc]) continue;
        unsigned long long *slot = col_slot + wc * bins;
        unsigned int local = 0;
        for (int c = b0; c < b1; ++c) local += static_cast<unsigned int>(slot[c]);
        unsigned int upto = local;                                      // inclusive sum over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int o = __shfl_up(upto, d);
            if (lane >= d) upto += o;
        }
        double mn = scope_inf();
        unsigned int cum = upto - local;
        for (int c = b0; c < b1; ++c) {
            const unsigned int h = static_cast<unsigned int>(slot[c]);
            cum += h;
            const double raw = h ? (static_cast<double>(c) / P) / (static_cast<double>(cum) / n_d) : scope_inf();
            slot[c] = static_cast<unsigned long long>(__double_as_longlong(raw));
            mn = fmin(mn, raw);
        }
        double right = mn;                                              // inclusive minimum over the lanes from the right
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_down(right, d);
            if (lane + d < 64) right = fmin(right, o);
        }
        double carry = __shfl_down(right, 1);
        if (lane == 63) carry = scope_inf();
        for (int c = b1 - 1; c >= b0; --c) {
            carry = fmin(carry, __longlong_as_double(static_cast<long long>(slot[c])));
            slot[c] = static_cast<unsigned long long>(__double_as_longlong(carry > 1.0 ? 1.0 : carry));
        }
    }
    __syncthreads();
    for (int64_t row = row0; row < n; row += step) {
        double *cell = pvals + row * m + c0 + col;
        if (col_nan[col]) {                                             // np.minimum carries the NaN through the whole column
            *cell = scope_qnan();
            continue;
        }
        const double cf = rint(*cell * P);
        if (!(cf >= 0.0 && cf <= P)) continue;
        *cell = __longlong_as_double(static_cast<long long>(col_slot[col * bins + static_cast<int>(cf)]));
    }
}

// ------------------------------------------------------------------------------------------------- columns, sort form ----

// out[c][r] = in[r][c]; one 32 x 32 tile per workgroup, tiles numbered along the columns of `in` first
__global__ __launch_bounds__(256) void k_fdr_transpose(const double *__restrict__ in, int64_t rows, int64_t cols, double *__restrict__ out) {
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

// -------------------------------------------------------------------------------------------------- matrix, count form ----

// flags: 1 = a NaN, 2 = an entry that is no count ratio
__global__ __launch_bounds__(256) void k_fdr_all_hist(const double *__restrict__ p, int64_t total, int64_t n_perm,
                                                      unsigned long long *__restrict__ hist, unsigned int *__restrict__ flags) {
    extern __shared__ unsigned int all_hist[];
    const int bins = static_cast<int>(n_perm) + 1;
    const int t = threadIdx.x;
    const double P = static_cast<double>(n_perm);
    for (int c = t; c < bins; c += 256) all_hist[c] = 0u;
    __syncthreads();
    unsigned int bad = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + t; i < total; i += static_cast<int64_t>(gridDim.x) * 256) {
        const double v = p[i];
        if (v != v) {
            bad |= 1u;
            continue;
        }
        const double cf = rint(v * P);
        if (!(cf >= 0.0 && cf <= P) || cf / P != v) {
            bad |= 2u;
            continue;
        }
        atomicAdd(&all_hist[static_cast<int>(cf)], 1u);
    }
    if (bad) atomicOr(flags, bad);
    __syncthreads();
    for (int c = t; c < bins; c += 256)
        if (all_hist[c]) atomicAdd(&hist[c], static_cast<unsigned long long>(all_hist[c]));
}

// one workgroup: table[c] = the adjusted value of every entry with count c (k_fdr_row_counts' scan over one histogram in memory)
__global__ __launch_bounds__(256) void k_fdr_all_table(const unsigned long long *__restrict__ hist, int64_t n_perm, double total_d,
                                                       double *__restrict__ table) {
    __shared__ unsigned long long part_u[256];
    __shared__ double part_d[256];
    const int bins = static_cast<int>(n_perm) + 1;
    const int t = threadIdx.x;
    const double P = static_cast<double>(n_perm);
    const int per = (bins + 255) / 256, b0 = t * per < bins ? t * per : bins, b1 = b0 + per < bins ? b0 + per : bins;
    unsigned long long local = 0;
    for (int c = b0; c < b1; ++c) local += hist[c];
    part_u[t] = local;
    __syncthreads();
    unsigned long long cum = 0;
    for (int u = 0; u < t; ++u) cum += part_u[u];
    double mn = scope_inf();
    for (int c = b0; c < b1; ++c) {
        const unsigned long long h = hist[c];
        cum += h;
        const double raw = h ? (static_cast<double>(c) / P) / (static_cast<double>(cum) / total_d) : scope_inf();
        table[c] = raw;
        mn = fmin(mn, raw);
    }
    part_d[t] = mn;
    __syncthreads();
    double carry = scope_inf();
    for (int u = t + 1; u < 256; ++u) carry = fmin(carry, part_d[u]);
    for (int c = b1 - 1; c >= b0; --c) {
        carry = fmin(carry, table[c]);
        table[c] = carry > 1.0 ? 1.0 : carry;
    }
}

__global__ __launch_bounds__(256) void k_fdr_all_map(double *__restrict__ p, int64_t total, int64_t n_perm, const double *__restrict__ table,
                                                     const unsigned int *__restrict__ flags) {
    const unsigned int f = *flags;
    if (f & 2u) return;                                                 // (cannot happen: the caller checked the matrix)
    const double P = static_cast<double>(n_perm);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * 256)
        p[i] = (f & 1u) ? scope_qnan() : table[static_cast<int>(rint(p[i] * P))];
}

// --------------------------------------------------------------------------------------------------- matrix, sort form ----

// the keys of k_fdr_row_sort: -0.0 -> +0.0, every NaN -> 0x7FF8..., then positive doubles order like their bits
__global__ __launch_bounds__(256) void k_fdr_all_keys(const double *__restrict__ p, int64_t total, unsigned long long *__restrict__ keys,
                                                      unsigned int *__restrict__ cells) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const double v = p[i];
    keys[i] = v != v ? 0x7FF8000000000000ull : static_cast<unsigned long long>(__double_as_longlong(v == 0.0 ? 0.0 : v));
    cells[i] = static_cast<unsigned int>(i);
}

__device__ __forceinline__ double all_raw(const unsigned long long *__restrict__ keys, int64_t r, double total_d) {
    return __longlong_as_double(static_cast<long long>(keys[r])) / (static_cast<double>(r + 1) / total_d);
}

// workgroup b: the minimum of the raw values of the sorted ranks [b FDR_ALL_BLOCK, (b + 1) FDR_ALL_BLOCK)
__global__ __launch_bounds__(256) void k_fdr_all_blockmin(const unsigned long long *__restrict__ keys, int64_t total, double *__restrict__ blockmin) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const double total_d = static_cast<double>(total);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * FDR_ALL_BLOCK + t * FDR_ALL_IPT;
    double mine = scope_inf();
    for (int i = 0; i < FDR_ALL_IPT; ++i)
        if (r0 + i < total) mine = fmin(mine, all_raw(keys, r0 + i, total_d));
    part[t] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) part[t] = fmin(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) blockmin[blockIdx.x] = part[0];
}

// one workgroup: carry[b] = the minimum over every workgroup right of b
__global__ __launch_bounds__(256) void k_fdr_all_carry(const double *__restrict__ blockmin, int64_t blocks, double *__restrict__ carry) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const int64_t len = (blocks + 255) / 256, b0 = t * len < blocks ? t * len : blocks, b1 = b0 + len < blocks ? b0 + len : blocks;
    double mine = scope_inf();
    for (int64_t b = b0; b < b1; ++b) mine = fmin(mine, blockmin[b]);
    part[t] = mine;
    __syncthreads();
    double run = scope_inf();
    for (int u = t + 1; u < 256; ++u) run = fmin(run, part[u]);
    for (int64_t b = b1 - 1; b >= b0; --b) {
        carry[b] = run;
        run = fmin(run, blockmin[b]);
    }
}

// the running minimum from the right inside the workgroup's ranks, joined with carry[b], written to the cells the ranks came from
__global__ __launch_bounds__(256) void k_fdr_all_apply(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ cells,
                                                       int64_t total, const double *__restrict__ carry, double *__restrict__ out) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const double total_d = static_cast<double>(total);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * FDR_ALL_BLOCK + t * FDR_ALL_IPT;
    // every NaN carries the largest key: the matrix has one iff the last sorted key is one, and then all of it becomes NaN
    if (keys[total - 1] == 0x7FF8000000000000ull) {
        for (int i = 0; i < FDR_ALL_IPT; ++i)
            if (r0 + i < total) out[cells[r0 + i]] = scope_qnan();
        return;
    }
    double mine = scope_inf();
    for (int i = 0; i < FDR_ALL_IPT; ++i)
        if (r0 + i < total) mine = fmin(mine, all_raw(keys, r0 + i, total_d));
    part[t] = mine;
    __syncthreads();
    double run = carry[blockIdx.x];
    for (int u = t + 1; u < 256; ++u) run = fmin(run, part[u]);
    for (int i = FDR_ALL_IPT - 1; i >= 0; --i) {
        if (r0 + i >= total) continue;
        run = fmin(run, all_raw(keys, r0 + i, total_d));
        out[cells[r0 + i]] = run > 1.0 ? 1.0 : run;
    }
}

// ------------------------------------------------------------------------------------------------------------- host ----

int scope_cols_counts(safe_ctx *ctx, const char *who, double *p_dev, int64_t n, int64_t m, int64_t n_perm) {
    const int64_t bins = n_perm + 1;
    const int tile = static_cast<int>(std::min<int64_t>(FDR_COL_TILE_MAX, FDR_COL_LDS_BYTES / (8 * bins)));
    const size_t lds = static_cast<size_t>(tile) * bins * 8;
    unsigned int *d_flag = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_FDR_SCOPE, sizeof(unsigned int), reinterpret_cast<void **>(&d_flag)));
    SAFE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(unsigned int), ctx->stream));
    SAFE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdr_col_counts), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds)));
    hipLaunchKernelGGL(k_fdr_col_counts, dim3(ceil_div(m, tile)), dim3(FDR_COL_THREADS), lds, ctx->stream, p_dev, n, m, n_perm, tile, d_flag);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    void *pinned = nullptr;
    SAFE_TRY(ctx_pinned(ctx, sizeof(unsigned int), &pinned));
    SAFE_HIP_CHECK(hipMemcpyAsync(pinned, d_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    if (*static_cast<unsigned int *>(pinned) == 0u) return SAFE_OK;
    safe_set_error("%s: a p-value is not a multiple of 1 / %lld", who, (long long)n_perm);   // (cannot happen: checked before)
    return SAFE_E_VALUE;
}

int scope_cols_sort(safe_ctx *ctx, const char *who, double *p_dev, int64_t n, int64_t m) {
    CallBufs b;
    double *t_dev = nullptr;
    SAFE_TRY(b.alloc(&t_dev, n * m));
    const int64_t tiles = ceil_div(n, FDR_TR_TILE) * ceil_div(m, FDR_TR_TILE);
    hipLaunchKernelGGL(k_fdr_transpose, dim3(tiles), dim3(256), 0, ctx->stream, p_dev, n, m, t_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_TRY(fdr_matrix(ctx, t_dev, m, n));
    hipLaunchKernelGGL(k_fdr_transpose, dim3(tiles), dim3(256), 0, ctx->stream, t_dev, m, n, p_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int scope_all_counts(safe_ctx *ctx, const char *who, double *p_dev, int64_t total, int64_t n_perm) {
    const int64_t bins = n_perm + 1;
    uint8_t *base = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_FDR_SCOPE, static_cast<size_t>(bins) * 16 + 16, reinterpret_cast<void **>(&base)));
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(base);
    double *table = reinterpret_cast<double *>(base + bins * 8);
    unsigned int *flags = reinterpret_cast<unsigned int *>(base + bins * 16);
    SAFE_HIP_CHECK(hipMemsetAsync(base, 0, static_cast<size_t>(bins) * 16 + 16, ctx->stream));
    const size_t lds = static_cast<size_t>(bins) * 4;
    const int64_t grid = std::min<int64_t>(ceil_div(total, 256), 2048);
    SAFE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fdr_all_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds)));
    hipLaunchKernelGGL(k_fdr_all_hist, dim3(grid), dim3(256), lds, ctx->stream, p_dev, total, n_perm, hist, flags);
    hipLaunchKernelGGL(k_fdr_all_table, dim3(1), dim3(256), 0, ctx->stream, hist, n_perm, static_cast<double>(total), table);
    hipLaunchKernelGGL(k_fdr_all_map, dim3(grid), dim3(256), 0, ctx->stream, p_dev, total, n_perm, table, flags);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    void *pinned = nullptr;
    SAFE_TRY(ctx_pinned(ctx, sizeof(unsigned int), &pinned));
    SAFE_HIP_CHECK(hipMemcpyAsync(pinned, flags, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    if (!(*static_cast<unsigned int *>(pinned) & 2u)) return SAFE_OK;
    safe_set_error("%s: a p-value is not a multiple of 1 / %lld", who, (long long)n_perm);   // (cannot happen: checked before)
    return SAFE_E_VALUE;
}

int scope_all_sort(safe_ctx *ctx, const char *who, double *p_dev, int64_t total) {
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
    hipLaunchKernelGGL(k_fdr_all_keys, dim3(ceil_div(total, 256)), dim3(256), 0, ctx->stream, p_dev, total, keys_in, cells_in);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, cells_in, cells_out,
                                                              static_cast<int>(total), 0, 64, ctx->stream));
    hipLaunchKernelGGL(k_fdr_all_blockmin, dim3(blocks), dim3(256), 0, ctx->stream, keys_out, total, blockmin);
    hipLaunchKernelGGL(k_fdr_all_carry, dim3(1), dim3(256), 0, ctx->stream, blockmin, blocks, carry);
    hipLaunchKernelGGL(k_fdr_all_apply, dim3(blocks), dim3(256), 0, ctx->stream, keys_out, cells_out, total, carry, p_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

// the largest count denominator whose count form `scope` has (rows: fdr_matrix decides for itself)
int64_t scope_hist_max_p(int scope) {
    return scope == SAFE_FDR_SCOPE_COLS ? FDR_COL_HIST_MAX_P : scope == SAFE_FDR_SCOPE_ALL ? FDR_ALL_HIST_MAX_P : INT64_MAX;
}

bool scope_may_count(int scope, int64_t n_perm) {
    return n_perm > 0 && n_perm <= scope_hist_max_p(scope) && !getenv("SAFE_HIP_FDR_SORT");
}

// hist_perm > 0: every entry is a count ratio c / hist_perm (checked) and scope_may_count(scope, hist_perm)
int scope_matrix(safe_ctx *ctx, const char *who, double *p_dev, int64_t n, int64_t m, int scope, int64_t hist_perm) {
    if (scope == SAFE_FDR_SCOPE_ROWS) return fdr_matrix(ctx, p_dev, n, m, hist_perm);
    if (scope == SAFE_FDR_SCOPE_COLS)
        return hist_perm > 0 ? scope_cols_counts(ctx, who, p_dev, n, m, hist_perm) : scope_cols_sort(ctx, who, p_dev, n, m);
    return hist_perm > 0 ? scope_all_counts(ctx, who, p_dev, n * m, hist_perm) : scope_all_sort(ctx, who, p_dev, n * m);
}

// bad arguments of the two entry points below are SAFE_E_VALUE
#define SCOPE_REQUIRE(cond, ...)                                                               \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            safe_set_error(__VA_ARGS__);                                                       \
            return SAFE_E_VALUE;                                                               \
        }                                                                                      \
    } while (0)

// chooses the form of a call over `n_mats` matrices: *hist_perm = n_perm when the count form serves, else 0 (the sort form);
// SAFE_E_UNSUPPORTED where the whole-matrix sort would pass the library sort's item count.  Reads only.
int scope_choose(safe_ctx *ctx, const char *who, int scope, int64_t n, int64_t m, int64_t n_perm, const double *const *mats,
                 int n_mats, int64_t *hist_perm) {
    *hist_perm = 0;
    const bool too_long = scope == SAFE_FDR_SCOPE_ALL && (n >= FDR_SORT_MAX_ITEMS || m >= FDR_SORT_MAX_ITEMS || n * m >= FDR_SORT_MAX_ITEMS);
    const bool may = scope_may_count(scope, n_perm);
    if (may) {
        bool all = false;
        SAFE_TRY(fdr_all_count_ratios(ctx, mats, n_mats, n * m, n_perm, &all));
        if (all) *hist_perm = n_perm;
    }
    if (too_long && *hist_perm == 0) {
        safe_set_error("%s: %lld x %lld p-values as one family are beyond the library sort (2^31 items)", who, (long long)n, (long long)m);
        return SAFE_E_UNSUPPORTED;
    }
    return SAFE_OK;
}

}  // namespace

extern "C" int safe_fdr_adjust_scope(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                                     double enrichment_threshold, int scope, double *pvalues_neg_dev, double *pvalues_pos_dev,
                                     double *nes_dev, double *nes_binary_dev, double *num_enriched_dev) {
    const char *who = "safe_fdr_adjust_scope";
    SCOPE_REQUIRE(ctx && pvalues_pos_dev && nes_dev && nes_binary_dev && num_enriched_dev, "%s: NULL argument", who);
    SCOPE_REQUIRE(n >= 1 && m >= 1 && num_permutations >= 0, "%s: bad sizes", who);
    SCOPE_REQUIRE(num_permutations == 0 || pvalues_neg_dev, "%s: the randomization form needs pvalues_neg", who);
    SCOPE_REQUIRE(sign_mode >= SAFE_SIGN_HIGHEST && sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", who, sign_mode);
    SCOPE_REQUIRE(enrichment_threshold > 0.0 && enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", who);
    SCOPE_REQUIRE(scope >= SAFE_FDR_SCOPE_ROWS && scope <= SAFE_FDR_SCOPE_ALL, "%s: bad scope %d", who, scope);
    if (scope == SAFE_FDR_SCOPE_ROWS)
        return safe_fdr_adjust(ctx, n, m, num_permutations, sign_mode, enrichment_threshold, pvalues_neg_dev, pvalues_pos_dev, nes_dev,
                               nes_binary_dev, num_enriched_dev);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const double *mats[2] = {pvalues_pos_dev, pvalues_neg_dev};
    int64_t hist_perm = 0;
    SAFE_TRY(scope_choose(ctx, who, scope, n, m, num_permutations, mats, num_permutations > 0 ? 2 : 1, &hist_perm));
    if (num_permutations > 0) SAFE_TRY(scope_matrix(ctx, who, pvalues_neg_dev, n, m, scope, hist_perm));
    SAFE_TRY(scope_matrix(ctx, who, pvalues_pos_dev, n, m, scope, hist_perm));
    return fdr_nes_epilogue(ctx, who, n, m, num_permutations, sign_mode, enrichment_threshold, pvalues_neg_dev, pvalues_pos_dev, nes_dev,
                            nes_binary_dev, num_enriched_dev);
}

extern "C" int safe_fdr_adjust_matrix(safe_ctx *ctx, int64_t n, int64_t m, int scope, int64_t count_denominator, double *p_dev) {
    const char *who = "safe_fdr_adjust_matrix";
    SCOPE_REQUIRE(ctx && p_dev, "%s: NULL argument", who);
    SCOPE_REQUIRE(n >= 1 && m >= 1 && count_denominator >= 0, "%s: bad sizes", who);
    SCOPE_REQUIRE(scope >= SAFE_FDR_SCOPE_ROWS && scope <= SAFE_FDR_SCOPE_ALL, "%s: bad scope %d", who, scope);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const double *mats[1] = {p_dev};
    int64_t hist_perm = 0;
    SAFE_TRY(scope_choose(ctx, who, scope, n, m, count_denominator, mats, 1, &hist_perm));
    return scope_matrix(ctx, who, p_dev, n, m, scope, hist_perm);
}
