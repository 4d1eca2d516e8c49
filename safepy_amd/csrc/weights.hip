// Distance-weighted neighborhoods on gfx950: one f64 weight per member, the weighted 'sum' score, and the analytic and the
// randomization test of that score.
//
// Every other route scores a neighborhood as if it were flat: a node just inside the radius counts as much as the node itself.
// Here member k of row i carries a weight w_ik >= 0, built from the node distance D[i,k] and the row's radius r_i, or given by
// the caller.  The contract (include/safe_hip.h): all arithmetic f64, every operation rounded, in the order written;
// the library is built with -ffp-contract=off.
//
//   u = D[i,k] / r_i, u = 0 when r_i == 0 (0 / 0 is never evaluated); h = the bandwidth
//   uniform 1.0 | triangular max(0, 1 - u) | epanechnikov max(0, 1 - u u) | gaussian exp(-0.5 (t t)), t = u / h
//   D: sqrt(dx dx + dy dy) (the bits of pdist, as k_euclid_* compute them), or the matrix a shortest-path handle kept
//   A member whose weight is 0 stays a member: the stored pattern is the membership's CSR, with explicit zeros.
//
//   x_ij = (((0.0 + w_i,k1 v_k1,j) + w_i,k2 v_k2,j) + ...)   members in ascending k, v = the value widened to f64, NaN -> 0;
//          one accumulator per cell: no split of a row's sum across lanes, no atomic
//
//   analytic: over the members of row i with row_flags = 1, ascending: W1_i = sum w, W2_i = sum w w, c_i their number, and
//          the smallest and the largest w;  g_i = (n_v W2_i - W1_i W1_i) / (n_v (n_v - 1)), 0 when n_v < 2, c_i = 0, c_i = n_v
//          with smallest == largest (the whole population at one weight), or the value is not positive;
//          var = g_i Q_j, z = (x_ij - W1_i mu_j) / sqrt(var); tails, NES and counts as safe_moments_test
//   randomization: S_p[i,j] = the score with v taken at row T_p[k]; counts_pos = #{p: S_p >= x}, counts_neg = #{p: S_p <= x}
//
//   k_weights_build       one wave per row, lanes along its members: D, u, w of every CSR entry
//   k_weights_fill_sell   the same weights in SELL-64 order beside sell_col, padding entries at weight 0
//   k_score_weighted      one workgroup per (row, 1024 columns): the row's (k, w) list staged in LDS 256 members at a time,
//                         lanes along columns, four columns per lane
//   k_weights_row_sums    one wave per row: 64 members loaded coalesced, added in member order
//   k_weights_emit        the layout and the cell arithmetic of k_moments_emit, W1_i for k_i and g_i for f_i
//   k_permtest_weighted   the shape of k_permtest_gather<16,false> with a weight stream beside the member ids; without
//                         permutations it is also the score of row-contiguous (Fortran-order) storage
#include <cmath>

#include "common.h"
#include "tails_shared.h"

namespace {

constexpr int WS_STAGE = 256;               // members of a row staged per pass of k_score_weighted
constexpr int WS_CPT = 4;                   // columns per lane of k_score_weighted
constexpr int WS_COLS = 256 * WS_CPT;       // columns of a k_score_weighted block
constexpr int WM_ROW_TILE = 16;             // rows of an emit block (4 per wave), as MOM_ROW_TILE
constexpr int WM_COL_CHUNK = 1024;          // columns of an emit block, as MOM_COL_CHUNK
constexpr int WP_BN = 16;                   // columns a lane of k_permtest_weighted keeps in registers

__device__ __forceinline__ double weight_of(int kind, double d, double r, double h) {
    const double u = r == 0.0 ? 0.0 : d / r;
    if (kind == SAFE_WEIGHT_TRIANGULAR) {
        const double t = 1.0 - u;
        return t > 0.0 ? t : 0.0;
    }
    if (kind == SAFE_WEIGHT_EPANECHNIKOV) {
        const double t = 1.0 - u * u;
        return t > 0.0 ? t : 0.0;
    }
    if (kind == SAFE_WEIGHT_GAUSSIAN) {
        const double t = u / h;
        return exp(-0.5 * (t * t));
    }
    return 1.0;
}

// xy != NULL: D from the coordinates; else from the kept matrix dist [n][n].  Four rows per block.
__global__ __launch_bounds__(256) void k_weights_build(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col, int64_t n,
                                                       const double *__restrict__ xy, const double *__restrict__ dist,
                                                       const double *__restrict__ radii, int kind, double h, double *__restrict__ w) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const double r = radii[i];
    const double xi = xy ? xy[2 * i] : 0.0, yi = xy ? xy[2 * i + 1] : 0.0;
    for (int32_t e = row_ptr[i] + lane; e < row_ptr[i + 1]; e += 64) {
        const int64_t k = col[e];
        double d;
        if (xy) {
            const double dx = xi - xy[2 * k];
            const double dy = yi - xy[2 * k + 1];
            d = sqrt(dx * dx + dy * dy);                            // no FMA (-ffp-contract=off)
        } else {
            d = dist[i * n + k];
        }
        w[e] = weight_of(kind, d, r, h);
    }
}

// the twin of k_fill_sell (nbr.hip) for the weights: entry t of lane l of a slice = weight of the row's t-th member, 0 behind it
__global__ void k_weights_fill_sell(const int32_t *__restrict__ row_ptr, const double *__restrict__ w, const int32_t *__restrict__ sell_row,
                                    const int64_t *__restrict__ slice_off, const int32_t *__restrict__ slice_width, int64_t n_slices,
                                    double *__restrict__ sell_w) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;     // 64 threads
    if (s >= n_slices) return;
    const int32_t r = sell_row[s * 64 + lane];
    const int32_t beg = r >= 0 ? row_ptr[r] : 0;
    const int32_t cnt = r >= 0 ? row_ptr[r + 1] - beg : 0;
    const int64_t off = slice_off[s];
    const int32_t wdt = slice_width[s];
    for (int32_t t = 0; t < wdt; ++t) sell_w[off + static_cast<int64_t>(t) * 64 + lane] = t < cnt ? w[beg + t] : 0.0;
}

// out[i][c] = sum over the members of row i, ascending, of w * nan_to_num(B[k][col0 + c]).  Block = (row, WS_COLS columns);
// lane l owns columns c0 + l + 256 u: a member's attribute row is one coalesced read per u when columns are contiguous.
template <typename T>
__global__ __launch_bounds__(256) void k_score_weighted(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const double *__restrict__ w, const void *__restrict__ raw, int64_t rs, int64_t cs,
                                                        int64_t col0, int64_t mloc, double *__restrict__ out) {
    __shared__ int32_t s_k[WS_STAGE];
    __shared__ double s_w[WS_STAGE];
    const int64_t i = blockIdx.x;
    const int32_t beg = row_ptr[i], end = row_ptr[i + 1];
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * WS_COLS + threadIdx.x;
    const T *src[WS_CPT];
    bool live[WS_CPT];
    double acc[WS_CPT];
#pragma unroll
    for (int u = 0; u < WS_CPT; ++u) {
        const int64_t c = c0 + 256 * u;
        live[u] = c < mloc;
        src[u] = static_cast<const T *>(raw) + (live[u] ? (col0 + c) * cs : 0);
        acc[u] = 0.0;
    }
    for (int32_t base = beg; base < end; base += WS_STAGE) {
        __syncthreads();                                            // the pass before has read its stage
        const int32_t e = base + static_cast<int32_t>(threadIdx.x);
        if (e < end) {
            s_k[threadIdx.x] = col[e];
            s_w[threadIdx.x] = w[e];
        }
        __syncthreads();
        const int cnt = end - base < WS_STAGE ? end - base : WS_STAGE;
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {
            const int64_t k = s_k[t];
            const double wt = s_w[t];
#pragma unroll
            for (int u = 0; u < WS_CPT; ++u) {
                if (!live[u]) continue;
                double v = static_cast<double>(src[u][k * rs]);   // widened before any arithmetic
                v = v != v ? 0.0 : v;
                acc[u] += wt * v;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < WS_CPT; ++u)
        if (live[u]) out[i * mloc + c0 + 256 * u] = acc[u];
}

// W1_i and g_i of every row.  A wave loads 64 members at a time (coalesced) and every lane adds them in member order from the
// lanes' registers, so the two sums run in ascending k; an unflagged member and a lane behind the row's end add +0.0, which
// leaves a sum of non-negative terms as it is.  min / max / count are order-free.
__global__ __launch_bounds__(256) void k_weights_row_sums(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                          const double *__restrict__ w, const uint8_t *__restrict__ row_flags, int64_t n,
                                                          double nv, double *__restrict__ w1_out, double *__restrict__ g_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int32_t beg = row_ptr[i], end = row_ptr[i + 1];
    double w1 = 0.0, w2 = 0.0, mn = INFINITY, mx = -INFINITY;
    int c = 0;
    for (int32_t base = beg; base < end; base += 64) {
        const int32_t e = base + lane;
        const bool on = e < end && row_flags[col[e]] != 0;
        const double mine = on ? w[e] : 0.0;
        c += on;
        mn = on && mine < mn ? mine : mn;
        mx = on && mine > mx ? mine : mx;
        const int cnt = end - base < 64 ? end - base : 64;
        for (int t = 0; t < cnt; ++t) {
            const double wt = __shfl(mine, t);
            w1 += wt;
            w2 += wt * wt;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c += __shfl_xor(c, d);
        const double a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane != 0) return;
    const double cd = static_cast<double>(c);
    double g = 0.0;
    if (nv >= 2.0 && c > 0 && !(cd == nv && mn == mx)) {
        g = (nv * w2 - w1 * w1) / (nv * (nv - 1.0));
        g = g > 0.0 ? g : 0.0;
    }
    w1_out[i] = w1;
    g_out[i] = g;
}

struct WeightsEmit {
    const double *ns;           // [n][mloc] observed weighted scores
    int64_t n, mloc;
    const double *w1;           // [n] W1_i
    const double *factor;       // [n] g_i
    const double *mean;         // [mloc] mu_j
    const double *css;          // [mloc] Q_j
    int sign_mode;
    double p_cut, nes_threshold;
    double *pvalues_neg, *pvalues_pos, *nes, *nes_binary;
    double *z;                  // or NULL
    unsigned int *enriched;     // [mloc]
};

// k_moments_emit (moments.hip) restated, W1_i where it reads k_i and g_i where it reads f_i: 8 B read, 32 B (40 B with z)
// written per cell
__global__ __launch_bounds__(256) void k_weights_emit(const WeightsEmit e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * WM_ROW_TILE;
    const int64_t r1 = r0 + WM_ROW_TILE < e.n ? r0 + WM_ROW_TILE : e.n;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * WM_COL_CHUNK;
    const int64_t c1 = c0 + WM_COL_CHUNK < e.mloc ? c0 + WM_COL_CHUNK : e.mloc;
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int64_t c = cb + lane;
        if (c >= c1) continue;
        const double mu = e.mean[c], q = e.css[c];
        unsigned int hits = 0;
        for (int64_t row = r0 + wave; row < r1; row += 4) {
            const int64_t o = row * e.mloc + c;
            const double x = e.ns[o];
            const double k = e.w1[row], var = e.factor[row] * q;
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

// Column tiles Bt[tile][row 0..n][WP_BN] f64, NaN -> 0; row n is the all-zero row the SELL padding entries point at
// (k_tile_prep<T, 16, 1> of enrich.hip restated)
template <typename T>
__global__ __launch_bounds__(256) void k_weights_tile_prep(const void *__restrict__ raw, int64_t n, int64_t rs, int64_t cs, int64_t col0,
                                                           int64_t mloc, int64_t n_tiles, double *__restrict__ bt) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t total = n_tiles * (n + 1) * WP_BN;
    if (idx >= total) return;
    const int c = static_cast<int>(idx % WP_BN);
    const int64_t row = (idx / WP_BN) % (n + 1);
    const int64_t tile = idx / (static_cast<int64_t>(WP_BN) * (n + 1));
    const int64_t j = tile * WP_BN + c;
    double v = 0.0;
    if (row < n && j < mloc) {
        const T x = reinterpret_cast<const T *>(raw)[row * rs + (col0 + j) * cs];
        if (x == x) v = static_cast<double>(x);
    }
    bt[idx] = v;
}

// One workgroup = (column tile, slice group); its 4 waves walk 64-row slices; inside a slice every lane owns one neighborhood
// and WP_BN columns.  Workgroups of one tile are placed on one XCD (blockIdx % 8) so the tile is fetched into a single L2.
// A padding entry is (member n, weight 0): 0 x 0 added to a sum that started at +0.0 changes nothing.  n_perm = 0 and
// counts_neg = counts_pos = NULL: the observed scores alone (the score of row-contiguous storage).
__global__ __launch_bounds__(256) void k_permtest_weighted(const int32_t *__restrict__ sell_row, const int64_t *__restrict__ slice_off,
                                                           const int32_t *__restrict__ slice_width, const int32_t *__restrict__ sell_col,
                                                           const double *__restrict__ sell_w, int64_t n_slices, int64_t n,
                                                           const double *__restrict__ bt, int64_t n_tiles, int n_groups,
                                                           const int32_t *__restrict__ table, int64_t n_perm, int64_t mloc,
                                                           double *__restrict__ ns, double *__restrict__ counts_neg,
                                                           double *__restrict__ counts_pos) {
    const int64_t b = blockIdx.x;
    const int64_t xcd = b & 7, q = b >> 3;
    const int64_t tile = (q / n_groups) * 8 + xcd;
    const int group = static_cast<int>(q % n_groups);
    if (tile >= n_tiles) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double *tb = bt + tile * (n + 1) * WP_BN;
    const int64_t stride = n + 1;
    const int64_t jbase = tile * WP_BN;

    for (int64_t s = group + static_cast<int64_t>(n_groups) * wave; s < n_slices; s += static_cast<int64_t>(n_groups) * 4) {
        const int32_t row = sell_row[s * 64 + lane];
        const int32_t *cols = sell_col + slice_off[s] + lane;
        const double *wts = sell_w + slice_off[s] + lane;
        const int wdt = slice_width[s];

        double acc[WP_BN], obs[WP_BN];
#pragma unroll
        for (int c = 0; c < WP_BN; ++c) acc[c] = 0.0;
        for (int t = 0; t < wdt; ++t) {
            const double *r = tb + static_cast<int64_t>(cols[t * 64]) * WP_BN;
            const double wt = wts[t * 64];
#pragma unroll
            for (int c = 0; c < WP_BN; ++c) acc[c] += wt * r[c];
        }
#pragma unroll
        for (int c = 0; c < WP_BN; ++c) obs[c] = acc[c];

        unsigned int cneg[WP_BN], cpos[WP_BN];
#pragma unroll
        for (int c = 0; c < WP_BN; ++c) cneg[c] = cpos[c] = 0;

        for (int64_t p = 0; p < n_perm; ++p) {
            const int32_t *cur = table + p * stride;
#pragma unroll
            for (int c = 0; c < WP_BN; ++c) acc[c] = 0.0;
#pragma unroll 2
            for (int t = 0; t < wdt; ++t) {
                const double *r = tb + static_cast<int64_t>(cur[cols[t * 64]]) * WP_BN;
                const double wt = wts[t * 64];
#pragma unroll
                for (int c = 0; c < WP_BN; ++c) acc[c] += wt * r[c];
            }
#pragma unroll
            for (int c = 0; c < WP_BN; ++c) {
                cneg[c] += acc[c] <= obs[c];
                cpos[c] += acc[c] >= obs[c];
            }
        }

        if (row < 0) continue;
        const int64_t o = static_cast<int64_t>(row) * mloc + jbase;
#pragma unroll
        for (int c = 0; c < WP_BN; ++c) {
            if (jbase + c >= mloc) continue;
            if (ns) ns[o + c] = obs[c];
            if (counts_neg) {
                counts_neg[o + c] = static_cast<double>(cneg[c]);
                counts_pos[o + c] = static_cast<double>(cpos[c]);
            }
        }
    }
}

int check_weighted(const char *who, const safe_nbr *nbr, const safe_attr *attr, int64_t col0, int64_t col1) {
    SAFE_REQUIRE(nbr && attr, "%s: NULL handle", who);
    SAFE_REQUIRE(nbr->n == attr->n, "%s: membership is %lld x %lld but the attribute matrix has %lld rows", who, (long long)nbr->n,
                 (long long)nbr->n, (long long)attr->n);
    SAFE_REQUIRE(0 <= col0 && col0 < col1 && col1 <= attr->m, "%s: column range [%lld,%lld) outside [0,%lld)", who, (long long)col0,
                 (long long)col1, (long long)attr->m);
    SAFE_REQUIRE(nbr->w_csr != nullptr, "%s: the membership handle has no weights (safe_nbr_weights_from_xy, "
                 "safe_nbr_weights_from_distances, safe_nbr_set_weights)", who);
    return SAFE_OK;
}

// Enqueues k_permtest_weighted over columns [col0, col1) on the context's stream: the attribute tiles go into their scratch slot,
// then one launch covers the n_perm rows of `table` (n_perm = 0, no table and no counts: the observed scores alone).
// mark_kernel: the context's k0 event is recorded between the two.
int gather_weighted_dev(safe_ctx *ctx, const char *who, const safe_nbr *nbr, const safe_attr *attr, const int32_t *table, int64_t n_perm,
                        int64_t col0, int64_t col1, double *ns_dev, double *counts_neg_dev, double *counts_pos_dev, bool mark_kernel) {
    const int64_t n = nbr->n, mloc = col1 - col0, n_tiles = ceil_div(mloc, WP_BN);
    const int64_t total = n_tiles * (n + 1) * WP_BN;
    hipStream_t s = ctx->stream;
    double *bt = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_WEIGHT_TILES, static_cast<size_t>(total) * sizeof(double), reinterpret_cast<void **>(&bt)));
    if (attr->dtype == SAFE_DTYPE_F32)
        hipLaunchKernelGGL(k_weights_tile_prep<float>, dim3(static_cast<unsigned int>(ceil_div(total, 256))), dim3(256), 0, s, attr->raw, n,
                           attr->row_stride, attr->col_stride, col0, mloc, n_tiles, bt);
    else
        hipLaunchKernelGGL(k_weights_tile_prep<double>, dim3(static_cast<unsigned int>(ceil_div(total, 256))), dim3(256), 0, s, attr->raw, n,
                           attr->row_stride, attr->col_stride, col0, mloc, n_tiles, bt);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    if (mark_kernel) SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));       // (the timed kernel starts behind the tile pass)
    // slice groups: enough workgroups to fill the chip several times over (launch_gather, enrich.hip)
    const int n_groups = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nbr->n_slices, 4), ceil_div(ctx->num_cu * 8, n_tiles))));
    const int64_t blocks = ceil_div(n_tiles, 8) * 8 * n_groups;
    hipLaunchKernelGGL(k_permtest_weighted, dim3(static_cast<unsigned int>(blocks)), dim3(256), 0, s, nbr->sell_row, nbr->slice_off,
                       nbr->slice_width, nbr->sell_col, nbr->w_sell, nbr->n_slices, n, bt, n_tiles, n_groups, table, n_perm, mloc, ns_dev,
                       counts_neg_dev, counts_pos_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return SAFE_OK;
}

// Rows contiguous (Fortran order): lanes along columns would read one cache line per lane, so the score takes the tiles and the
// lane-per-neighborhood shape of the permutation kernel instead -- the same member order, one accumulator per cell.
bool score_by_tiles(const safe_attr *attr) { return attr->row_stride == 1 && attr->m > 1; }
const char *score_kernel_name(const safe_attr *attr) { return score_by_tiles(attr) ? "k_permtest_weighted" : "k_score_weighted"; }

// enqueues the weighted score of columns [col0, col1) into out_dev [n][col1 - col0] on the context's stream
int score_weighted_dev(safe_ctx *ctx, const char *who, const safe_nbr *nbr, const safe_attr *attr, int64_t col0, int64_t col1, double *out_dev) {
    if (score_by_tiles(attr)) return gather_weighted_dev(ctx, who, nbr, attr, nullptr, 0, col0, col1, out_dev, nullptr, nullptr, false);
    const int64_t mloc = col1 - col0;
    const dim3 grid(static_cast<unsigned int>(nbr->n), static_cast<unsigned int>(ceil_div(mloc, WS_COLS)));
    if (attr->dtype == SAFE_DTYPE_F32)
        hipLaunchKernelGGL(k_score_weighted<float>, grid, dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col, nbr->w_csr, attr->raw,
                           attr->row_stride, attr->col_stride, col0, mloc, out_dev);
    else
        hipLaunchKernelGGL(k_score_weighted<double>, grid, dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col, nbr->w_csr, attr->raw,
                           attr->row_stride, attr->col_stride, col0, mloc, out_dev);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return SAFE_OK;
}

// the time between the context's k0 / k1 events as its last kernel, after the stream has been synchronised
int record_last_kernel(safe_ctx *ctx, const char *who, const char *kernel) {
    float ms = 0.f;
    SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ctx->k0, ctx->k1));
    ctx->last_kernel.name = kernel;
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = ms;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = false;
    return SAFE_OK;
}

// The handle takes the CSR-order weights in d_w (a block of `bufs`): their SELL-order copy is made, then both replace what the
// handle had.  Nothing of the handle changes on a failure.
int weights_install(safe_nbr *nbr, const char *who, CallBufs *bufs, double *d_w) {
    safe_ctx *ctx = nbr->ctx;
    double *d_sell = nullptr;
    SAFE_TRY(bufs->alloc(&d_sell, static_cast<size_t>(nbr->sell_entries)));
    hipLaunchKernelGGL(k_weights_fill_sell, dim3(static_cast<unsigned int>(nbr->n_slices)), dim3(64), 0, ctx->stream, nbr->row_ptr, d_w,
                       nbr->sell_row, nbr->slice_off, nbr->slice_width, nbr->n_slices, d_sell);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    (void)dev_free(nbr->w_csr);
    (void)dev_free(nbr->w_sell);
    nbr->w_csr = bufs->release(d_w);
    nbr->w_sell = bufs->release(d_sell);
    return SAFE_OK;
}

int check_kind(const char *who, int kind, const double *radii_host, int64_t n, double bandwidth) {
    SAFE_REQUIRE(kind >= SAFE_WEIGHT_UNIFORM && kind <= SAFE_WEIGHT_GAUSSIAN, "%s: unknown weight kind %d", who, kind);
    SAFE_TRY(check_radii(who, radii_host, n));
    if (!(std::isfinite(bandwidth) && bandwidth > 0.0)) {
        safe_set_error("%s: bandwidth %g must be finite and > 0", who, bandwidth);
        return SAFE_E_VALUE;
    }
    return SAFE_OK;
}

int weights_build(safe_nbr *nbr, const char *who, const double *xy_host, int kind, const double *radii_host, double bandwidth) {
    safe_ctx *ctx = nbr->ctx;
    const int64_t n = nbr->n;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    double *d_in = nullptr;                                                // radii f64 [n] | xy f64 [n][2]
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_WEIGHT_INPUTS, static_cast<size_t>(3 * n) * sizeof(double), reinterpret_cast<void **>(&d_in)));
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_in, radii_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (xy_host) SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_in + n, xy_host, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const DistSource src = xy_host ? DistSource{d_in + n, nullptr, n} : DistSource{nullptr, nbr->dist, n};
    CallBufs bufs;
    double *d_w = nullptr;
    SAFE_TRY(bufs.alloc(&d_w, static_cast<size_t>(nbr->nnz)));
    hipLaunchKernelGGL(k_weights_build, dim3(static_cast<unsigned int>(ceil_div(n, 4))), dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col, n,
                       src.xy, src.dist, d_in, kind, bandwidth, d_w);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return weights_install(nbr, who, &bufs, d_w);
}

}  // namespace

// W1_i and g_i of every row of a handle that carries weights into d_w1 / d_g [n], enqueued on the context's stream (also maxt.hip);
// the attribute handle is prepared
int weights_row_factors_dev(safe_ctx *ctx, const safe_nbr *nbr, const safe_attr *attr, const char *who, double *d_w1, double *d_g) {
    const int64_t n = nbr->n;
    hipLaunchKernelGGL(k_weights_row_sums, dim3(static_cast<unsigned int>(ceil_div(n, 4))), dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col,
                       nbr->w_csr, attr->row_flags, n, static_cast<double>(attr->n_rows_with_value), d_w1, d_g);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    return SAFE_OK;
}

extern "C" {

int safe_nbr_weights_from_xy(safe_nbr *nbr, const double *xy_host, int kind, const double *radii_host, double bandwidth) {
    const char *who = "safe_nbr_weights_from_xy";
    SAFE_REQUIRE(nbr && xy_host && radii_host, "%s: NULL argument", who);
    SAFE_TRY(check_kind(who, kind, radii_host, nbr->n, bandwidth));
    SAFE_TRY(check_layout_finite(who, xy_host, nbr->n));
    return weights_build(nbr, who, xy_host, kind, radii_host, bandwidth);
}

int safe_nbr_weights_from_distances(safe_nbr *nbr, int kind, const double *radii_host, double bandwidth) {
    const char *who = "safe_nbr_weights_from_distances";
    SAFE_REQUIRE(nbr && radii_host, "%s: NULL argument", who);
    SAFE_REQUIRE(nbr->dist != nullptr, "%s: handle was built without keep_distances", who);
    SAFE_TRY(check_kind(who, kind, radii_host, nbr->n, bandwidth));
    return weights_build(nbr, who, nullptr, kind, radii_host, bandwidth);
}

int safe_nbr_set_weights(safe_nbr *nbr, const double *w_host) {
    const char *who = "safe_nbr_set_weights";
    SAFE_REQUIRE(nbr && (w_host || nbr->nnz == 0), "%s: NULL argument", who);
    for (int64_t e = 0; e < nbr->nnz; ++e)
        if (!(std::isfinite(w_host[e]) && w_host[e] >= 0.0)) {
            safe_set_error("%s: weight %lld is %g: every weight must be finite and >= 0", who, (long long)e, w_host[e]);
            return SAFE_E_VALUE;
        }
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs bufs;
    double *d_w = nullptr;
    SAFE_TRY(bufs.alloc(&d_w, static_cast<size_t>(nbr->nnz)));
    if (nbr->nnz) SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_w, w_host, nbr->nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return weights_install(nbr, who, &bufs, d_w);
}

int safe_nbr_weights(safe_nbr *nbr, double *out_host) {
    const char *who = "safe_nbr_weights";
    SAFE_REQUIRE(nbr && (out_host || nbr->nnz == 0), "%s: NULL argument", who);
    SAFE_REQUIRE(nbr->w_csr != nullptr, "%s: the handle has no weights", who);
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    if (nbr->nnz) SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(out_host, nbr->w_csr, nbr->nnz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_nbr_clear_weights(safe_nbr *nbr) {
    const char *who = "safe_nbr_clear_weights";
    SAFE_REQUIRE(nbr != nullptr, "%s: NULL argument", who);
    if (!nbr->w_csr) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(nbr->ctx->device));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(nbr->ctx->stream));
    (void)dev_free(nbr->w_csr);
    (void)dev_free(nbr->w_sell);
    nbr->w_csr = nbr->w_sell = nullptr;
    return SAFE_OK;
}

int safe_score_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int64_t col0, int64_t col1, double *ns_dev) {
    const char *who = "safe_score_weighted";
    SAFE_REQUIRE(ctx && ns_dev, "%s: NULL argument", who);
    SAFE_TRY(check_weighted(who, nbr, attr, col0, col1));
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, ctx->stream));
    SAFE_TRY(score_weighted_dev(ctx, who, nbr, attr, col0, col1, ns_dev));
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, ctx->stream));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));
    return record_last_kernel(ctx, who, score_kernel_name(attr));
}

int safe_moments_test_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold, int64_t col0,
                               int64_t col1, double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev, double *nes_dev,
                               double *nes_binary_dev, double *num_enriched_dev, double *z_dev) {
    const char *who = "safe_moments_test_weighted";
    SAFE_REQUIRE(ctx && ns_dev && pvalues_neg_dev && pvalues_pos_dev && nes_dev && nes_binary_dev && num_enriched_dev, "%s: NULL argument", who);
    SAFE_TRY(check_weighted(who, nbr, attr, col0, col1));
    SAFE_REQUIRE(sign_mode >= SAFE_SIGN_HIGHEST && sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", who, sign_mode);
    SAFE_REQUIRE(enrichment_threshold > 0.0 && enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", who);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_attr_prepare(attr));
    const int64_t n = nbr->n, mloc = col1 - col0;
    const double nv = static_cast<double>(attr->n_rows_with_value);
    hipStream_t s = ctx->stream;

    void *small = nullptr;                                                // W1 f64 [n] | g f64 [n] | mu f64 [mloc] | Q f64 [mloc] | enriched u32 [mloc + 16]
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_WEIGHT_ROWS, static_cast<size_t>(2 * n + 2 * mloc) * sizeof(double) + static_cast<size_t>(mloc + 16) * sizeof(unsigned int), &small));
    double *d_w1 = static_cast<double *>(small), *d_factor = d_w1 + n, *d_mean = d_factor + n, *d_css = d_mean + mloc;
    unsigned int *d_enr = reinterpret_cast<unsigned int *>(d_css + mloc);
    SAFE_HIP_CHECK_AS(who, hipMemsetAsync(d_enr, 0, (mloc + 16) * sizeof(unsigned int), s));
    SAFE_TRY(score_weighted_dev(ctx, who, nbr, attr, col0, col1, ns_dev));
    hipLaunchKernelGGL(k_weights_row_sums, dim3(static_cast<unsigned int>(ceil_div(n, 4))), dim3(256), 0, s, nbr->row_ptr, nbr->col, nbr->w_csr,
                       attr->row_flags, n, nv, d_w1, d_factor);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_TRY(column_moments_dev(ctx, attr, col0, col1, who, d_mean, d_css));

    WeightsEmit e{};
    e.ns = ns_dev;
    e.n = n;
    e.mloc = mloc;
    e.w1 = d_w1;
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
    hipLaunchKernelGGL(k_weights_emit, dim3(static_cast<unsigned int>(ceil_div(n, WM_ROW_TILE)), static_cast<unsigned int>(ceil_div(mloc, WM_COL_CHUNK))),
                       dim3(256), 0, s, e);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    hipLaunchKernelGGL(k_hyp_tails_u32_to_f64, dim3(static_cast<unsigned int>(ceil_div(mloc, 256))), dim3(256), 0, s, d_enr, num_enriched_dev, mloc);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));                          // the timing events are read back: the call has finished when it returns
    return record_last_kernel(ctx, who, "k_weights_emit");
}

int safe_permtest_counts_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms, int64_t col0, int64_t col1,
                                  double *ns_dev, double *counts_neg_dev, double *counts_pos_dev) {
    const char *who = "safe_permtest_counts_weighted";
    SAFE_REQUIRE(ctx && perms && counts_neg_dev && counts_pos_dev, "%s: NULL argument", who);
    SAFE_TRY(check_weighted(who, nbr, attr, col0, col1));
    SAFE_REQUIRE(perms->n == nbr->n, "%s: permutation tables are for %lld rows, membership has %lld", who, (long long)perms->n,
                 (long long)nbr->n);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->packed_layout = -1;
    hipStream_t s = ctx->stream;
    SAFE_TRY(perms_wait(perms, perms->count, s));
    SAFE_TRY(gather_weighted_dev(ctx, who, nbr, attr, perms->table, perms->count, col0, col1, ns_dev, counts_neg_dev, counts_pos_dev, true));
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));
    return record_last_kernel(ctx, who, "k_permtest_weighted");
}

}  // extern "C"
