// The analytic test on gfx950: exact moments of the permutation null, normal tails, no permutation drawn.
//
// The randomization route (safepy/safe.py:496-554) shuffles the rows that hold a value (indx_vals, safe_extras.py:51) and
// compares a neighborhood's 'sum' score with its scores under the shuffles.  Under that null a score is a sum of k draws
// without replacement from a column's n_v values, so its mean and variance are closed-form.  safe_moments_test evaluates them
// and a normal tail per cell -- the SAFE paper's own significance for quantitative attributes, on the exact moments instead of
// sampled ones.
//
// The contract.  Population of column j: the rows r with row_flags[r] = 1; a NaN cell inside them counts as 0
// (safe_extras.py:10); n_v = the handle's n_rows_with_value.
//
//   mu_j   = col_sum_j / n_v                          (col_sum: the handle's nansum)
//   Q_j    = sum over flagged r of (b_rj - mu_j)^2    (second pass, centred; NaN -> 0); Q_j := 0 when the column's min over
//                                                     the population equals its max (decided on min / max, not on Q_j == 0)
//   k_i    = members of neighborhood i with row_flags = 1
//   x_ij   = ns = A . nan_to_num(B)                   (safe_score 'sum')
//   f_i    = k_i (n_v - k_i) / (n_v (n_v - 1))        (both products exact, one rounded division)
//   var_ij = f_i * Q_j
//   z_ij   = (x_ij - k_i * mu_j) / sqrt(var_ij)
//   small  = erfc(|z| * sqrt(1/2)) / 2                (one erfc per cell); large = 1 - small
//   p_pos  = P[Z >= z] = small for z >= 0, large otherwise; p_neg = P[Z <= z] the other one
//
// Degenerate cells -- n_v < 2, k_i = 0, k_i = n_v (f_i = 0) or a constant column (Q_j = 0), i.e. var_ij is not positive: every
// permuted score equals the observed one, so p_pos = p_neg = 1 and z = 0, the permutation test's own limit.
// NES, nes_binary and the per-attribute counts follow safe_hypergeom_tails (tails_nes, tails_shared.h).
//
// Built with -ffp-contract=off like the rest of the library: the operation order above is the rounding order.
//
//   k_col_moments       partial Q / min / max of MOM_ROW_CHUNK rows of a column, lanes along the matrix's contiguous axis
//   k_col_moments_fold  the chunks of a column added in ascending order; the constant-column rule; mu_j
//                       (no floating-point atomic anywhere: two calls give the same bits)
//   k_moments_emit      streaming, lanes along columns: 8 B read, 32 B (40 B with z) written per cell
#include <cmath>

#include "common.h"
#include "tails_shared.h"

namespace {

constexpr int MOM_ROW_CHUNK = 2048;         // rows of a k_col_moments block
constexpr int MOM_ROW_TILE = 16;            // rows of an emit block (4 per wave)
constexpr int MOM_COL_CHUNK = 1024;         // columns of an emit block (16 groups of 64 lanes)

__device__ __forceinline__ double col_mean(double col_sum, double nv) { return nv > 0.0 ? col_sum / nv : 0.0; }

// parts = three planes [chunks][mloc]: sum of squares | min | max of the chunk's flagged rows.
// CC (columns contiguous, C order): 64 columns x 4 row lanes per block, a wave reads 64 adjacent columns of one row.
// otherwise (Fortran order, or one column): one column per block, 256 threads along its rows.
// Either way a thread adds its rows in ascending order and the threads of a block meet in a fixed order.
template <typename T, bool CC>
__global__ __launch_bounds__(256) void k_col_moments(const void *__restrict__ raw, int64_t n, int64_t rs, int64_t cs,
                                                     const uint8_t *__restrict__ row_flags, const double *__restrict__ col_sum, double nv,
                                                     int64_t col0, int64_t mloc, int64_t chunks, double *__restrict__ parts) {
    __shared__ double s_q[256], s_mn[256], s_mx[256];
    const int64_t chunk = blockIdx.y;
    const int64_t r0 = chunk * MOM_ROW_CHUNK;
    const int64_t r1 = r0 + MOM_ROW_CHUNK < n ? r0 + MOM_ROW_CHUNK : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t jl = CC ? static_cast<int64_t>(blockIdx.x) * 64 + lane : static_cast<int64_t>(blockIdx.x);
    const bool live = jl < mloc;
    const double mu = live ? col_mean(col_sum[col0 + jl], nv) : 0.0;
    const T *src = static_cast<const T *>(raw) + (live ? (col0 + jl) * cs : 0);
    double q = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t r = r0 + (CC ? wave : static_cast<int>(threadIdx.x)); r < r1; r += CC ? 4 : 256) {
        if (!live || !row_flags[r]) continue;
        double v = static_cast<double>(src[r * rs]);           // widened before any arithmetic
        v = v != v ? 0.0 : v;
        const double d = v - mu;
        q += d * d;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    if (!CC) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            q += __shfl_down(q, off);
            const double a = __shfl_down(mn, off), b = __shfl_down(mx, off);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
    }
    if (CC || lane == 0) {
        const int slot = CC ? static_cast<int>(threadIdx.x) : wave;
        s_q[slot] = q;
        s_mn[slot] = mn;
        s_mx[slot] = mx;
    }
    __syncthreads();
    if ((CC ? wave == 0 : threadIdx.x == 0) && live) {
        const int stride = CC ? 64 : 1, first = CC ? lane : 0;
        q = s_q[first];
        mn = s_mn[first];
        mx = s_mx[first];
        for (int w = 1; w < 4; ++w) {
            q += s_q[first + w * stride];
            mn = s_mn[first + w * stride] < mn ? s_mn[first + w * stride] : mn;
            mx = s_mx[first + w * stride] > mx ? s_mx[first + w * stride] : mx;
        }
        const int64_t plane = chunks * mloc, o = chunk * mloc + jl;
        parts[o] = q;
        parts[plane + o] = mn;
        parts[2 * plane + o] = mx;
    }
}

__global__ __launch_bounds__(256) void k_col_moments_fold(const double *__restrict__ parts, int64_t chunks, int64_t mloc,
                                                          const double *__restrict__ col_sum, double nv, int64_t col0,
                                                          double *__restrict__ mean, double *__restrict__ css) {
    const int64_t jl = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (jl >= mloc) return;
    const int64_t plane = chunks * mloc;
    double q = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t o = c * mloc + jl;
        q += parts[o];
        mn = parts[plane + o] < mn ? parts[plane + o] : mn;
        mx = parts[2 * plane + o] > mx ? parts[2 * plane + o] : mx;
    }
    mean[jl] = col_mean(col_sum[col0 + jl], nv);
    css[jl] = mn == mx ? 0.0 : q;                            // a constant column: a rounded mean leaves dust in q
}

// f_i = k_i (n_v - k_i) / (n_v (n_v - 1)); 0 where the neighborhood cannot vary (n_v < 2, k_i = 0, k_i = n_v)
__global__ __launch_bounds__(256) void k_moments_row_factor(const double *__restrict__ size, int64_t n, double nv, double *__restrict__ factor) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double k = size[i];
    factor[i] = (nv >= 2.0 && k > 0.0 && k < nv) ? (k * (nv - k)) / (nv * (nv - 1.0)) : 0.0;
}

struct MomentsEmit {
    const double *ns;           // [n][mloc] observed 'sum' scores
    int64_t n, mloc;
    const double *size;         // [n] k_i
    const double *factor;       // [n] f_i
    const double *mean;         // [mloc] mu_j
    const double *css;          // [mloc] Q_j
    int sign_mode;
    double p_cut, nes_threshold;
    double *pvalues_neg, *pvalues_pos, *nes, *nes_binary;
    double *z;                  // or NULL
    unsigned int *enriched;     // [mloc]
};

// A block = MOM_ROW_TILE rows x MOM_COL_CHUNK columns; a wave takes every fourth row of the tile, its lanes 64 adjacent
// columns (the layout of k_hyp_tails_emit<false>).  Per-column enriched counts: one atomic per wave and column group.
__global__ __launch_bounds__(256) void k_moments_emit(const MomentsEmit e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * MOM_ROW_TILE;
    const int64_t r1 = r0 + MOM_ROW_TILE < e.n ? r0 + MOM_ROW_TILE : e.n;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * MOM_COL_CHUNK;
    const int64_t c1 = c0 + MOM_COL_CHUNK < e.mloc ? c0 + MOM_COL_CHUNK : e.mloc;
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int64_t c = cb + lane;
        if (c >= c1) continue;
        const double mu = e.mean[c], q = e.css[c];
        unsigned int hits = 0;
        for (int64_t row = r0 + wave; row < r1; row += 4) {
            const int64_t o = row * e.mloc + c;
            const double x = e.ns[o];
            const double k = e.size[row], var = e.factor[row] * q;
            double z = 0.0, pp = 1.0, pn = 1.0;
            if (var > 0.0) {
                z = (x - k * mu) / sqrt(var);
                const double small = 0.5 * erfc(fabs(z) * 0.70710678118654752440);
                const double large = 1.0 - small;
                const bool upper = z >= 0.0;
                pp = upper ? small : large;
                pn = upper ? large : small;
            }
            double nes;
            const bool hit = tails_nes(pp, pn, e.sign_mode, e.p_cut, e.nes_threshold, &nes);
            e.pvalues_pos[o] = pp;
            e.pvalues_neg[o] = pn;
            e.nes[o] = nes;
            e.nes_binary[o] = hit ? 1.0 : 0.0;
            if (e.z) e.z[o] = z;
            hits += hit;
        }
        if (hits) atomicAdd(&e.enriched[c], hits);
    }
}

}  // namespace

// mu_j and Q_j of columns [col0, col1) into d_mean / d_css [col1 - col0], enqueued on the context's stream (also weights.hip)
int column_moments_dev(safe_ctx *ctx, safe_attr *attr, int64_t col0, int64_t col1, const char *who, double *d_mean, double *d_css) {
    const int64_t n = attr->n, mloc = col1 - col0, chunks = ceil_div(n, MOM_ROW_CHUNK);
    const double nv = static_cast<double>(attr->n_rows_with_value);
    double *parts = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MOMENTS_PARTS, static_cast<size_t>(3 * chunks * mloc) * sizeof(double), reinterpret_cast<void **>(&parts)));
    const bool cc = attr->col_stride == 1 && attr->m > 1;
    const dim3 grid(static_cast<unsigned int>(cc ? ceil_div(mloc, 64) : mloc), static_cast<unsigned int>(chunks));
#define MOMENTS(T, CC)                                                                                                          \
    hipLaunchKernelGGL((k_col_moments<T, CC>), grid, dim3(256), 0, ctx->stream, attr->raw, n, attr->row_stride, attr->col_stride, \
                       attr->row_flags, attr->col_sum, nv, col0, mloc, chunks, parts)
    if (attr->dtype == SAFE_DTYPE_F32) {
        if (cc) MOMENTS(float, true);
        else MOMENTS(float, false);
    } else {
        if (cc) MOMENTS(double, true);
        else MOMENTS(double, false);
    }
#undef MOMENTS
    hipLaunchKernelGGL(k_col_moments_fold, dim3(ceil_div(mloc, 256)), dim3(256), 0, ctx->stream, parts, chunks, mloc, attr->col_sum, nv, col0,
                       d_mean, d_css);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return SAFE_OK;
}

// k_i and f_i of every row into d_size / d_factor [n], enqueued on the context's stream (also maxt.hip); the attribute handle is prepared
int moments_row_factors_dev(safe_ctx *ctx, const safe_nbr *nbr, const safe_attr *attr, const char *who, double *d_size, double *d_factor) {
    const int64_t n = nbr->n;
    const double nv = static_cast<double>(attr->n_rows_with_value);
    hipLaunchKernelGGL(k_hyp_tails_nbr_size, dim3(ceil_div(n, 4)), dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col, attr->row_flags, n, d_size);
    hipLaunchKernelGGL(k_moments_row_factor, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, d_size, n, nv, d_factor);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return SAFE_OK;
}

extern "C" {

int safe_attr_column_moments(safe_attr *attr, int64_t col0, int64_t col1, double *mean_host, double *css_host) {
    const char *who = "safe_attr_column_moments";
    SAFE_REQUIRE(attr && mean_host && css_host, "%s: NULL argument", who);
    SAFE_REQUIRE(0 <= col0 && col0 < col1 && col1 <= attr->m, "%s: column range [%lld,%lld) outside [0,%lld)", who, (long long)col0,
                 (long long)col1, (long long)attr->m);
    safe_ctx *ctx = attr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_attr_prepare(attr));
    const int64_t mloc = col1 - col0;
    double *d_mean = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MOMENTS_SMALL, static_cast<size_t>(2 * mloc) * sizeof(double), reinterpret_cast<void **>(&d_mean)));
    SAFE_TRY(column_moments_dev(ctx, attr, col0, col1, who, d_mean, d_mean + mloc));
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(mean_host, d_mean, mloc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(css_host, d_mean + mloc, mloc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_moments_test(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold, int64_t col0, int64_t col1,
                      double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev, double *nes_dev, double *nes_binary_dev,
                      double *num_enriched_dev, double *z_dev) {
    const char *who = "safe_moments_test";
    SAFE_REQUIRE(ctx && ns_dev && pvalues_neg_dev && pvalues_pos_dev && nes_dev && nes_binary_dev && num_enriched_dev, "%s: NULL argument", who);
    SAFE_REQUIRE(nbr && attr, "%s: NULL handle", who);
    SAFE_REQUIRE(nbr->n == attr->n, "%s: membership is %lld x %lld but the attribute matrix has %lld rows", who, (long long)nbr->n,
                 (long long)nbr->n, (long long)attr->n);
    SAFE_REQUIRE(0 <= col0 && col0 < col1 && col1 <= attr->m, "%s: column range [%lld,%lld) outside [0,%lld)", who, (long long)col0,
                 (long long)col1, (long long)attr->m);
    SAFE_REQUIRE(sign_mode >= SAFE_SIGN_HIGHEST && sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", who, sign_mode);
    SAFE_REQUIRE(enrichment_threshold > 0.0 && enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", who);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_attr_prepare(attr));
    const int64_t n = nbr->n, mloc = col1 - col0;
    const double nv = static_cast<double>(attr->n_rows_with_value);
    hipStream_t s = ctx->stream;

    // x = A . nan_to_num(B) through the 'sum' score; it returns once its kernels have ended
    SAFE_TRY(safe_score(ctx, nbr, attr, SAFE_SCORE_SUM, col0, col1, ns_dev));

    void *small = nullptr;                                                // k f64 [n] | f f64 [n] | mu f64 [mloc] | Q f64 [mloc] | enriched u32 [mloc + 16]
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_MOMENTS_SMALL, static_cast<size_t>(2 * n + 2 * mloc) * sizeof(double) + static_cast<size_t>(mloc + 16) * sizeof(unsigned int), &small));
    double *d_size = static_cast<double *>(small), *d_factor = d_size + n, *d_mean = d_factor + n, *d_css = d_mean + mloc;
    unsigned int *d_enr = reinterpret_cast<unsigned int *>(d_css + mloc);
    SAFE_HIP_CHECK_AS(who, hipMemsetAsync(d_enr, 0, (mloc + 16) * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_hyp_tails_nbr_size, dim3(ceil_div(n, 4)), dim3(256), 0, s, nbr->row_ptr, nbr->col, attr->row_flags, n, d_size);
    hipLaunchKernelGGL(k_moments_row_factor, dim3(ceil_div(n, 256)), dim3(256), 0, s, d_size, n, nv, d_factor);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_TRY(column_moments_dev(ctx, attr, col0, col1, who, d_mean, d_css));

    MomentsEmit e{};
    e.ns = ns_dev;
    e.n = n;
    e.mloc = mloc;
    e.size = d_size;
    e.factor = d_factor;
    e.mean = d_mean;
    e.css = d_css;
    e.sign_mode = sign_mode;
    e.p_cut = nes_p_cut(enrichment_threshold);
    e.nes_threshold = -std::log10(enrichment_threshold);
    e.pvalues_neg = pvalues_neg_dev;
    e.pvalues_pos = pvalues_pos_dev;
    e.nes = nes_dev;
    e.nes_binary = nes_binary_dev;
    e.z = z_dev;
    e.enriched = d_enr;
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));
    hipLaunchKernelGGL(k_moments_emit, dim3(ceil_div(n, MOM_ROW_TILE), ceil_div(mloc, MOM_COL_CHUNK)), dim3(256), 0, s, e);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    ctx->last_kernel.name = "k_moments_emit";
    hipLaunchKernelGGL(k_hyp_tails_u32_to_f64, dim3(ceil_div(mloc, 256)), dim3(256), 0, s, d_enr, num_enriched_dev, mloc);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));                          // the timing events are read back: the call has finished when it returns
    float ms = 0.f;
    SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ctx->k0, ctx->k1));
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = ms;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = false;
    return SAFE_OK;
}

}  // extern "C"
