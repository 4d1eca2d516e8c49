// The Westfall-Young single-step max-statistic adjustment on gfx950: per permutation and column, the extremes over the rows of
// the standardised permuted 'sum' scores, and the counts of the observed statistics against them.
//
// The contract (include/safe_hip.h): all arithmetic f64, every operation rounded, in the order written; the
// library is built with -ffp-contract=off.  Columns j in [col0, col1), rows i, permutations p in [0, P), T_p = row p of the table.
//
//   S_p[i,j]  = (((0.0 + w_i,k1 v_T_p[k1],j) + w_i,k2 v_T_p[k2],j) + ...)   members in ascending k, one accumulator per cell, NaN -> 0;
//               w = the handle's weights, 1.0 on a flat handle (1.0 v is v: the plain ascending sum)
//   loc_i, scale_i = k_i, f_i of safe_moments_test on a flat handle; W1_i, g_i of safe_moments_test_weighted on a weighted one
//   var       = scale_i Q_j;  z_p[i,j] = (S_p[i,j] - loc_i mu_j) / sqrt(var) where var > 0, else the cell is degenerate (for every p)
//   z_obs     = the same with the observed score: the z_dev of the matching moments entry point, 0 at a degenerate cell
//   tmax[p,j] = max of z_p[i,j] over the non-degenerate i (-inf without one);  tmin[p,j] = their min (+inf without one)
//
//   k_maxt_tile_prep   column tiles Bt[tile][row][16] f64, NaN -> 0 (the operand of k_permtest_weighted without its padding row)
//   k_maxt_transpose   the table [P][n + 1] as [n][P]: a member's source rows of 64 permutations are one coalesced read
//   k_maxt_observed    z_obs and the live flags, lanes along columns
//   k_maxt_extremes    THE HOT KERNEL.  One lane = one permutation, one wave = 64 of them, a workgroup = 256 permutations x one
//                      16-column tile x every n_groups-th chunk of 16 rows.  The members and weights of a row are wave-uniform
//                      (scalar loads), the table read coalesces, the gather is one 128-byte tile row per lane as in
//                      k_permtest_weighted; the running max / min of the 16 columns stay in registers over all the rows the
//                      workgroup walks and leave once, as 64-bit atomics on order-preserving integer keys (max and min do not
//                      depend on arrival order: two calls give the same bits)
//   k_maxt_decode      keys [column][P] -> tmax / tmin f64 [P][columns]
//   k_maxt_family      SAFE_FAMILY_MATRIX: the extremes of a permutation over all columns
//   k_maxt_counts      counts_pos = #{p : E+ >= z_obs}, counts_neg = #{p : E- <= z_obs}: lanes along columns, 16 rows per lane in
//                      registers, the extremes staged in LDS 32 permutations at a time (any P: the passes repeat)
#include <cmath>

#include "common.h"

namespace {

constexpr int MX_BN = 16;                   // columns of a tile: a lane's gather is one 128-byte row
constexpr int MX_RB = 16;                   // rows whose centre and deviation a workgroup stages at a time (256 threads = 16 x 16)
constexpr int MX_PB = 256;                  // permutations of a workgroup (64 per wave)
constexpr int CT_PC = 32;                   // permutations staged per pass of k_maxt_counts
constexpr int CT_RT = 16;                   // rows a lane of k_maxt_counts holds
constexpr int CT_ROWS = 4 * CT_RT;          // rows of a k_maxt_counts block

using u64 = unsigned long long;

// doubles (no NaN) <-> unsigned keys in the same order: -inf < ... < -0.0 < +0.0 < ... < +inf
__device__ __forceinline__ u64 key_of(double x) {
    const u64 u = static_cast<u64>(__double_as_longlong(x));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double of_key(u64 k) {
    const u64 u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double(static_cast<long long>(u));
}

template <typename T>
__global__ __launch_bounds__(256) void k_maxt_tile_prep(const void *__restrict__ raw, int64_t n, int64_t rs, int64_t cs, int64_t col0,
                                                        int64_t mloc, int64_t n_tiles, double *__restrict__ bt) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t total = n_tiles * n * MX_BN;
    if (idx >= total) return;
    const int c = static_cast<int>(idx % MX_BN);
    const int64_t row = (idx / MX_BN) % n;
    const int64_t tile = idx / (static_cast<int64_t>(MX_BN) * n);
    const int64_t j = tile * MX_BN + c;
    double v = 0.0;
    if (j < mloc) {
        const T x = reinterpret_cast<const T *>(raw)[row * rs + (col0 + j) * cs];
        if (x == x) v = static_cast<double>(x);
    }
    bt[idx] = v;
}

// tt[k][p] = table[p][k], k < n (the table's padding entry n stays behind).  32 x 32 tiles through LDS, 256 threads.
__global__ __launch_bounds__(256) void k_maxt_transpose(const int32_t *__restrict__ table, int64_t n, int64_t P, int32_t *__restrict__ tt) {
    __shared__ int32_t s[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // ty 0..7
    const int64_t k0 = static_cast<int64_t>(blockIdx.x) * 32, p0 = static_cast<int64_t>(blockIdx.y) * 32;
    for (int r = ty; r < 32; r += 8) {
        const int64_t p = p0 + r, k = k0 + tx;
        s[r][tx] = (p < P && k < n) ? table[p * (n + 1) + k] : 0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t k = k0 + r, p = p0 + tx;
        if (k < n && p < P) tt[k * P + p] = s[tx][r];
    }
}

__global__ __launch_bounds__(256) void k_maxt_fill_keys(u64 *__restrict__ keys, int64_t count, u64 value) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < count) keys[i] = value;
}

// z_obs[i][j] and live[i][j] (either may be NULL): block = (row, 256 columns), a row's member list is block-uniform
template <bool W>
__global__ __launch_bounds__(256) void k_maxt_observed(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ w, int64_t n, const double *__restrict__ bt,
                                                       const double *__restrict__ loc, const double *__restrict__ scale,
                                                       const double *__restrict__ mean, const double *__restrict__ css, int64_t mloc,
                                                       double *__restrict__ z_out, uint8_t *__restrict__ live_out) {
    const int64_t i = blockIdx.x;
    const int64_t j = static_cast<int64_t>(blockIdx.y) * 256 + threadIdx.x;
    if (j >= mloc) return;
    const double *tb = bt + (j / MX_BN) * n * MX_BN + (j % MX_BN);
    const int32_t beg = row_ptr[i], end = row_ptr[i + 1];
    double acc = 0.0;
    for (int32_t e = beg; e < end; ++e) {
        const double v = tb[static_cast<int64_t>(col[e]) * MX_BN];
        if (W) acc += w[e] * v;
        else acc += v;
    }
    const double var = scale[i] * css[j];
    double z = 0.0;
    if (var > 0.0) z = (acc - loc[i] * mean[j]) / sqrt(var);
    if (z_out) z_out[i * mloc + j] = z;
    if (live_out) live_out[i * mloc + j] = var > 0.0 ? 1 : 0;
}

// Workgroups of one tile are placed on one XCD (blockIdx % 8), as k_permtest_weighted places them: the tile is fetched into a
// single L2.  per_tile = (blocks of 256 permutations) x n_groups workgroups share a tile.
template <bool W>
__global__ __launch_bounds__(256) void k_maxt_extremes(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ w, int64_t n, const double *__restrict__ bt,
                                                       int64_t n_tiles, int64_t per_tile, int n_groups, const int32_t *__restrict__ tt,
                                                       int64_t P, const double *__restrict__ loc, const double *__restrict__ scale,
                                                       const double *__restrict__ mean, const double *__restrict__ css, int64_t mloc,
                                                       u64 *__restrict__ kmax, u64 *__restrict__ kmin) {
    __shared__ double s_center[MX_RB * MX_BN], s_sd[MX_RB * MX_BN];
    const int64_t b = blockIdx.x;
    const int64_t xcd = b & 7, q = b >> 3;
    const int64_t tile = (q / per_tile) * 8 + xcd;
    if (tile >= n_tiles) return;                                    // (the whole workgroup: no barrier is left waiting)
    const int64_t rem = q % per_tile;
    const int64_t pblock = rem / n_groups;
    const int group = static_cast<int>(rem % n_groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t p0 = pblock * MX_PB + wave * 64;
    const bool wave_live = p0 < P;
    const bool lane_live = p0 + lane < P;
    const int64_t p = lane_live ? p0 + lane : P - 1;                // a lane behind the table's end reads its last row and writes nothing
    const double *tb = bt + tile * n * MX_BN;
    const int64_t jbase = tile * MX_BN;
    const int32_t *tp = tt + p;

    double mx[MX_BN], mn[MX_BN];
#pragma unroll
    for (int c = 0; c < MX_BN; ++c) {
        mx[c] = -INFINITY;
        mn[c] = INFINITY;
    }

    const int64_t n_chunks = (n + MX_RB - 1) / MX_RB;
    for (int64_t chunk = group; chunk < n_chunks; chunk += n_groups) {
        const int64_t r0 = chunk * MX_RB;
        __syncthreads();                                            // the chunk before has been read
        {
            const int64_t row = r0 + (threadIdx.x >> 4);
            const int c = threadIdx.x & 15;
            double ce = 0.0, sd = 0.0;
            if (row < n) {
                const double var = scale[row] * css[jbase + c];   // (css and mean are padded to whole tiles with 0)
                if (var > 0.0) {
                    sd = sqrt(var);
                    ce = loc[row] * mean[jbase + c];
                }
            }
            s_center[threadIdx.x] = ce;
            s_sd[threadIdx.x] = sd;
        }
        __syncthreads();
        if (!wave_live) continue;
        const int64_t r1 = r0 + MX_RB < n ? r0 + MX_RB : n;
        for (int64_t row = r0; row < r1; ++row) {
            if (!(scale[row] > 0.0)) continue;                      // every cell of the row is degenerate
            const int32_t beg = __builtin_amdgcn_readfirstlane(row_ptr[row]), end = __builtin_amdgcn_readfirstlane(row_ptr[row + 1]);
            double acc[MX_BN];
#pragma unroll
            for (int c = 0; c < MX_BN; ++c) acc[c] = 0.0;
#pragma unroll 2
            for (int32_t e = beg; e < end; ++e) {
                const int64_t k = col[e];
                const double2 *r = reinterpret_cast<const double2 *>(tb + static_cast<int64_t>(tp[k * P]) * MX_BN);
                const double wt = W ? w[e] : 1.0;
#pragma unroll
                for (int h = 0; h < MX_BN / 2; ++h) {
                    const double2 v = r[h];
                    if (W) {
                        acc[2 * h] += wt * v.x;
                        acc[2 * h + 1] += wt * v.y;
                    } else {
                        acc[2 * h] += v.x;
                        acc[2 * h + 1] += v.y;
                    }
                }
            }
            const int so = static_cast<int>(row - r0) * MX_BN;
#pragma unroll
            for (int c = 0; c < MX_BN; ++c) {
                const double sd = s_sd[so + c];
                if (sd > 0.0) {
                    const double z = (acc[c] - s_center[so + c]) / sd;
                    mx[c] = z > mx[c] ? z : mx[c];
                    mn[c] = z < mn[c] ? z : mn[c];
                }
            }
        }
    }
    if (!lane_live) return;
#pragma unroll
    for (int c = 0; c < MX_BN; ++c) {
        const int64_t j = jbase + c;
        if (j >= mloc) continue;
        if (mx[c] != -INFINITY) atomicMax(&kmax[j * P + p], key_of(mx[c]));
        if (mn[c] != INFINITY) atomicMin(&kmin[j * P + p], key_of(mn[c]));
    }
}

__global__ __launch_bounds__(256) void k_maxt_decode(const u64 *__restrict__ kmax, const u64 *__restrict__ kmin, int64_t P, int64_t mloc,
                                                     double *__restrict__ tmax, double *__restrict__ tmin) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= P * mloc) return;
    const int64_t p = idx / mloc, j = idx % mloc;
    tmax[idx] = of_key(kmax[j * P + p]);
    tmin[idx] = of_key(kmin[j * P + p]);
}

// fam[p] = max over the m columns of tmax[p][.], fam[P + p] = min of tmin[p][.]: one wave per permutation
__global__ __launch_bounds__(256) void k_maxt_family(const double *__restrict__ tmax, const double *__restrict__ tmin, int64_t P, int64_t m,
                                                     double *__restrict__ fam) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    double hi = -INFINITY, lo = INFINITY;
    for (int64_t j = lane; j < m; j += 64) {
        const double a = tmax[p * m + j], b = tmin[p * m + j];
        hi = a > hi ? a : hi;
        lo = b < lo ? b : lo;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(hi, d), b = __shfl_xor(lo, d);
        hi = a > hi ? a : hi;
        lo = b < lo ? b : lo;
    }
    if (lane == 0) {
        fam[p] = hi;
        fam[P + p] = lo;
    }
}

// Block = 64 columns x CT_ROWS rows; lane = column, wave w holds rows r0 + w CT_RT ... of it in registers.  fam != NULL: every
// column compares with the family's extremes.  A degenerate cell gets P and stays out of the column minima (u32 [2][m], neg | pos).
__global__ __launch_bounds__(256) void k_maxt_counts(const double *__restrict__ z, const uint8_t *__restrict__ live, int64_t n, int64_t m,
                                                     int64_t P, const double *__restrict__ tmax, const double *__restrict__ tmin,
                                                     const double *__restrict__ fam, double *__restrict__ counts_neg,
                                                     double *__restrict__ counts_pos, unsigned int *__restrict__ col_min) {
    __shared__ double s_hi[CT_PC][64], s_lo[CT_PC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * CT_ROWS + wave * CT_RT;
    const bool col_ok = j < m;
    double zv[CT_RT];
    unsigned int cp[CT_RT], cn[CT_RT];
    bool on[CT_RT];
#pragma unroll
    for (int t = 0; t < CT_RT; ++t) {
        const int64_t row = r0 + t;
        const bool cell = col_ok && row < n;
        zv[t] = cell ? z[row * m + j] : 0.0;
        on[t] = cell && live[row * m + j] != 0;
        cp[t] = cn[t] = 0;
    }
    for (int64_t pb = 0; pb < P; pb += CT_PC) {
        const int cnt = static_cast<int>(P - pb < CT_PC ? P - pb : CT_PC);
        __syncthreads();                                            // the pass before has been read
        for (int t = wave; t < cnt; t += 4) {
            const int64_t p = pb + t;
            s_hi[t][lane] = fam ? fam[p] : (col_ok ? tmax[p * m + j] : 0.0);
            s_lo[t][lane] = fam ? fam[P + p] : (col_ok ? tmin[p * m + j] : 0.0);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double hi = s_hi[t][lane], lo = s_lo[t][lane];
#pragma unroll
            for (int u = 0; u < CT_RT; ++u) {
                cp[u] += hi >= zv[u];
                cn[u] += lo <= zv[u];
            }
        }
    }
    if (!col_ok) return;
    unsigned int best_n = static_cast<unsigned int>(P), best_p = static_cast<unsigned int>(P);
#pragma unroll
    for (int t = 0; t < CT_RT; ++t) {
        const int64_t row = r0 + t;
        if (row >= n) continue;
        const unsigned int a = on[t] ? cn[t] : static_cast<unsigned int>(P), b = on[t] ? cp[t] : static_cast<unsigned int>(P);
        counts_neg[row * m + j] = static_cast<double>(a);
        counts_pos[row * m + j] = static_cast<double>(b);
        best_n = a < best_n ? a : best_n;
        best_p = b < best_p ? b : best_p;
    }
    if (col_min) {
        atomicMin(&col_min[j], best_n);
        atomicMin(&col_min[m + j], best_p);
    }
}

__global__ __launch_bounds__(256) void k_maxt_fill_u32(unsigned int *__restrict__ out, int64_t count, unsigned int value) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < count) out[i] = value;
}

__global__ __launch_bounds__(256) void k_maxt_u32_to_f64(const unsigned int *__restrict__ in, double *__restrict__ out, int64_t count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < count) out[i] = static_cast<double>(in[i]);
}

unsigned int grid1(int64_t count) { return static_cast<unsigned int>(ceil_div(count, 256)); }

}  // namespace

extern "C" {

int safe_permtest_extremes(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms, int64_t col0, int64_t col1, double *z_dev,
                           uint8_t *live_dev, double *tmax_dev, double *tmin_dev) {
    const char *who = "safe_permtest_extremes";
    SAFE_REQUIRE(ctx && nbr && attr && perms && tmax_dev && tmin_dev, "%s: NULL argument", who);
    SAFE_REQUIRE(nbr->n == attr->n, "%s: membership is %lld x %lld but the attribute matrix has %lld rows", who, (long long)nbr->n,
                 (long long)nbr->n, (long long)attr->n);
    SAFE_REQUIRE(0 <= col0 && col0 < col1 && col1 <= attr->m, "%s: column range [%lld,%lld) outside [0,%lld)", who, (long long)col0,
                 (long long)col1, (long long)attr->m);
    SAFE_REQUIRE(perms->n == nbr->n, "%s: permutation tables are for %lld rows, membership has %lld", who, (long long)perms->n,
                 (long long)nbr->n);
    SAFE_REQUIRE(perms->count >= 1, "%s: no permutations", who);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_attr_prepare(attr));
    const int64_t n = nbr->n, mloc = col1 - col0, P = perms->count, n_tiles = ceil_div(mloc, MX_BN), mpad = n_tiles * MX_BN;
    const bool weighted = nbr->w_csr != nullptr;
    // enough workgroups to fill the chip several times over: every n_groups-th chunk of MX_RB rows per workgroup
    const int64_t n_pblocks = ceil_div(P, MX_PB), n_chunks = ceil_div(n, MX_RB);
    const int n_groups = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(n_chunks, ceil_div(ctx->num_cu * 8, n_tiles * n_pblocks))));
    const int64_t per_tile = n_pblocks * n_groups;
    const int64_t blocks = ceil_div(n_tiles, 8) * 8 * per_tile;
    SAFE_REQUIRE(blocks <= 0x7FFFFFFF, "%s: %lld workgroups exceed a launch", who, (long long)blocks);
    hipStream_t s = ctx->stream;

    double *rows = nullptr, *bt = nullptr;                                // loc [n] | scale [n] | mu [mpad] | Q [mpad]
    int32_t *tt = nullptr;
    u64 *keys = nullptr;                                                  // max keys [mloc][P] | min keys [mloc][P]
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MAXT_ROWS, static_cast<size_t>(2 * n + 2 * mpad) * sizeof(double), reinterpret_cast<void **>(&rows)));
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MAXT_TILES, static_cast<size_t>(n_tiles * n * MX_BN) * sizeof(double), reinterpret_cast<void **>(&bt)));
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MAXT_TABLE, static_cast<size_t>(n * P) * sizeof(int32_t), reinterpret_cast<void **>(&tt)));
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MAXT_KEYS, static_cast<size_t>(2 * mloc * P) * sizeof(u64), reinterpret_cast<void **>(&keys)));
    double *d_loc = rows, *d_scale = rows + n, *d_mean = d_scale + n, *d_css = d_mean + mpad;
    u64 *kmax = keys, *kmin = keys + mloc * P;

    SAFE_TRY(perms_wait(perms, P, s));
    SAFE_HIP_CHECK_AS(who, hipMemsetAsync(d_mean, 0, static_cast<size_t>(2 * mpad) * sizeof(double), s));
    if (weighted) SAFE_TRY(weights_row_factors_dev(ctx, nbr, attr, who, d_loc, d_scale));
    else SAFE_TRY(moments_row_factors_dev(ctx, nbr, attr, who, d_loc, d_scale));
    {
        double *d_tmp_mean = nullptr;                                     // column_moments_dev writes two dense [mloc] arrays
        SAFE_TRY(ctx_scratch(ctx, SCRATCH_MOMENTS_SMALL, static_cast<size_t>(2 * mloc) * sizeof(double), reinterpret_cast<void **>(&d_tmp_mean)));
        SAFE_TRY(column_moments_dev(ctx, attr, col0, col1, who, d_tmp_mean, d_tmp_mean + mloc));
        SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_mean, d_tmp_mean, mloc * sizeof(double), hipMemcpyDeviceToDevice, s));
        SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_css, d_tmp_mean + mloc, mloc * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    const int64_t tile_total = n_tiles * n * MX_BN;
    if (attr->dtype == SAFE_DTYPE_F32)
        hipLaunchKernelGGL(k_maxt_tile_prep<float>, dim3(grid1(tile_total)), dim3(256), 0, s, attr->raw, n, attr->row_stride, attr->col_stride,
                           col0, mloc, n_tiles, bt);
    else
        hipLaunchKernelGGL(k_maxt_tile_prep<double>, dim3(grid1(tile_total)), dim3(256), 0, s, attr->raw, n, attr->row_stride, attr->col_stride,
                           col0, mloc, n_tiles, bt);
    hipLaunchKernelGGL(k_maxt_transpose, dim3(static_cast<unsigned int>(ceil_div(n, 32)), static_cast<unsigned int>(ceil_div(P, 32))), dim3(256),
                       0, s, perms->table, n, P, tt);
    hipLaunchKernelGGL(k_maxt_fill_keys, dim3(grid1(mloc * P)), dim3(256), 0, s, kmax, mloc * P, 0x000FFFFFFFFFFFFFull);   // key_of(-inf)
    hipLaunchKernelGGL(k_maxt_fill_keys, dim3(grid1(mloc * P)), dim3(256), 0, s, kmin, mloc * P, 0xFFF0000000000000ull);   // key_of(+inf)
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    if (z_dev || live_dev) {
        const dim3 grid(static_cast<unsigned int>(n), static_cast<unsigned int>(ceil_div(mloc, 256)));
        if (weighted)
            hipLaunchKernelGGL(k_maxt_observed<true>, grid, dim3(256), 0, s, nbr->row_ptr, nbr->col, nbr->w_csr, n, bt, d_loc, d_scale, d_mean,
                               d_css, mloc, z_dev, live_dev);
        else
            hipLaunchKernelGGL(k_maxt_observed<false>, grid, dim3(256), 0, s, nbr->row_ptr, nbr->col, nbr->w_csr, n, bt, d_loc, d_scale, d_mean,
                               d_css, mloc, z_dev, live_dev);
        SAFE_HIP_CHECK_AS(who, hipGetLastError());
    }
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));
    if (weighted)
        hipLaunchKernelGGL(k_maxt_extremes<true>, dim3(static_cast<unsigned int>(blocks)), dim3(256), 0, s, nbr->row_ptr, nbr->col, nbr->w_csr, n,
                           bt, n_tiles, per_tile, n_groups, tt, P, d_loc, d_scale, d_mean, d_css, mloc, kmax, kmin);
    else
        hipLaunchKernelGGL(k_maxt_extremes<false>, dim3(static_cast<unsigned int>(blocks)), dim3(256), 0, s, nbr->row_ptr, nbr->col, nbr->w_csr, n,
                           bt, n_tiles, per_tile, n_groups, tt, P, d_loc, d_scale, d_mean, d_css, mloc, kmax, kmin);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    hipLaunchKernelGGL(k_maxt_decode, dim3(grid1(P * mloc)), dim3(256), 0, s, kmax, kmin, P, mloc, tmax_dev, tmin_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));                          // the timing events are read back: the call has finished when it returns
    float ms = 0.f;
    SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ctx->k0, ctx->k1));
    ctx->last_kernel.name = "k_maxt_extremes";
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = ms;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = false;
    return SAFE_OK;
}

int safe_counts_from_extremes(safe_ctx *ctx, int64_t n, int64_t m, int64_t P, int scope, const double *z_dev, const uint8_t *live_dev,
                              const double *tmax_dev, const double *tmin_dev, double *counts_neg_dev, double *counts_pos_dev,
                              double *min_counts_neg_dev, double *min_counts_pos_dev) {
    const char *who = "safe_counts_from_extremes";
    SAFE_REQUIRE(ctx && z_dev && live_dev && tmax_dev && tmin_dev && counts_neg_dev && counts_pos_dev, "%s: NULL argument", who);
    SAFE_REQUIRE(n >= 1 && m >= 1, "%s: bad sizes %lld x %lld", who, (long long)n, (long long)m);
    SAFE_REQUIRE(P >= 1 && P <= 0x7FFFFFFF, "%s: %lld permutations", who, (long long)P);
    SAFE_REQUIRE(scope == SAFE_FAMILY_COLUMN || scope == SAFE_FAMILY_MATRIX, "%s: unknown scope %d", who, scope);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *block = nullptr;                                                // family extremes f64 [2][P] | column minima u32 [2][m]
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MAXT_FAMILY, static_cast<size_t>(2 * P) * sizeof(double) + static_cast<size_t>(2 * m) * sizeof(unsigned int), &block));
    double *fam = static_cast<double *>(block);
    unsigned int *col_min = reinterpret_cast<unsigned int *>(fam + 2 * P);
    const bool want_min = min_counts_neg_dev || min_counts_pos_dev;
    if (want_min) hipLaunchKernelGGL(k_maxt_fill_u32, dim3(grid1(2 * m)), dim3(256), 0, s, col_min, 2 * m, static_cast<unsigned int>(P));
    if (scope == SAFE_FAMILY_MATRIX)
        hipLaunchKernelGGL(k_maxt_family, dim3(static_cast<unsigned int>(ceil_div(P, 4))), dim3(256), 0, s, tmax_dev, tmin_dev, P, m, fam);
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));
    hipLaunchKernelGGL(k_maxt_counts, dim3(static_cast<unsigned int>(ceil_div(m, 64)), static_cast<unsigned int>(ceil_div(n, CT_ROWS))), dim3(256),
                       0, s, z_dev, live_dev, n, m, P, tmax_dev, tmin_dev, scope == SAFE_FAMILY_MATRIX ? fam : nullptr, counts_neg_dev,
                       counts_pos_dev, want_min ? col_min : nullptr);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    if (min_counts_neg_dev) hipLaunchKernelGGL(k_maxt_u32_to_f64, dim3(grid1(m)), dim3(256), 0, s, col_min, min_counts_neg_dev, m);
    if (min_counts_pos_dev) hipLaunchKernelGGL(k_maxt_u32_to_f64, dim3(grid1(m)), dim3(256), 0, s, col_min + m, min_counts_pos_dev, m);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));
    float ms = 0.f;
    SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ctx->k0, ctx->k1));
    ctx->last_kernel.name = "k_maxt_counts";
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = ms;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = false;
    return SAFE_OK;
}

}  // extern "C"
