// node_distance_metric = 'diffusion' on gfx950: the truncated random-walk-with-restart (regularised Laplacian) kernel of an
// edge-list network and the cosine-normalised distance derived from it, as a membership handle that keeps the distances.
//
// Additive: the reference (safepy/safe.py:369-430) measures node distance by hops or along a 2-D layout only.  The contract
// (include/safe_hip.h, safe_nbr_diffusion) fixes every rounding: f64 throughout, one operation at a time (-ffp-contract=off),
// every sum in the order of the row's CSR entries.  No floating-point atomics: identical calls give identical bytes.
//
//   k_diffusion_scale / k_diffusion_entries   d_i, r_i = 1 / sqrt(d_i), s_ik = (w_ik r_i) r_k
//   k_diffusion_identity                      X_0 = I
//   k_diffusion_step                          Y = alpha I + beta (S X): the hot kernel, launched `steps` times, ping-pong
//   k_diffusion_transform                     K -> D, the membership bits and the kept matrix, upper triangle read once
#include <algorithm>
#include <cmath>
#include <numeric>

#include "common.h"

// --------------------------------------------------------------------------------------
// Degree and scale.  One thread per row adds the row's entry weights in entry order (the order is the contract; a hub row of a
// few thousand entries is microseconds); then one wave per row scales its entries.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_diffusion_scale(int64_t n, const int32_t *__restrict__ ptr, const double *__restrict__ w,
                                                         double *__restrict__ r) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) d = d + w[e];
    r[i] = d == 0.0 ? 0.0 : 1.0 / sqrt(d);
}

__global__ __launch_bounds__(256) void k_diffusion_entries(int64_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ w, const double *__restrict__ r,
                                                           double *__restrict__ s) {
    const int64_t i = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const double ri = r[i];
    for (int32_t e = ptr[i] + lane; e < ptr[i + 1]; e += 64) s[e] = (w[e] * ri) * r[col[e]];
}

__global__ __launch_bounds__(256) void k_diffusion_identity(int64_t n, int64_t ld, double *__restrict__ x) {
    const int64_t total = n * ld;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
         t += static_cast<int64_t>(gridDim.x) * blockDim.x)
        x[t] = (t / ld == t % ld) ? 1.0 : 0.0;
}

// --------------------------------------------------------------------------------------
// The step  Y[i][j] = (i == j ? alpha : 0) + beta * sum_e s_e X[col_e][j],  e over row i's entries in order.
//
// X and Y are row-major with pitch ld (n rounded up to 8: every row starts on a 64-byte line, the padding columns are zero and
// stay zero).  Lanes run along the columns, two adjacent columns per lane, so a wave reads 1 KiB of a neighbor's row with one
// 16-byte load per lane.  A wave owns DIFF_ROWS rows x DIFF_COLS columns; the four waves of a workgroup take four such row tiles of
// the same column chunk.  The entry list of a row is the same for every lane: it is read through the scalar unit.
//
// Rows are taken in descending order of their entry count (order[]): the waves of a workgroup then carry like work, and the long
// rows of a column chunk start first.  The sum of a row cannot be split -- its order is the contract -- but nothing orders the
// columns: a hub row is cut into ld / DIFF_COLS independent wave tasks that run side by side, and inside a task eight neighbor
// rows are in flight before the first is added.
//
// The grid is one-dimensional and dealt to the eight XCDs in turn (workgroup id mod 8), each with a private 4 MiB L2.  Workgroup id
// -> (column chunk, row tile) is chosen so that an XCD walks the row tiles of ONE column chunk before it moves to its next chunk
// (chunk = 8 x pass + XCD): what its workgroups re-read is then one n x 1 KiB slab of X, not eight.  Chunks are rounded up to a
// multiple of 8; the workgroups of the chunks that do not exist leave at once.
// --------------------------------------------------------------------------------------
#define DIFF_ROWS 4
#define DIFF_COLS 128
#define DIFF_WAVES 4
#define DIFF_UNROLL 8
#define DIFF_XCDS 8

__global__ __launch_bounds__(64 * DIFF_WAVES) void k_diffusion_step(int64_t n, int64_t ld, const int32_t *__restrict__ ptr,
                                                                    const int32_t *__restrict__ col, const double *__restrict__ s,
                                                                    const int32_t *__restrict__ order, double alpha, double beta,
                                                                    int64_t row_tiles, const double *__restrict__ x,
                                                                    double *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t slot = blockIdx.x / DIFF_XCDS;                                    // position in this XCD's own sequence
    const int64_t chunk = (slot / row_tiles) * DIFF_XCDS + blockIdx.x % DIFF_XCDS;
    const int64_t c = chunk * DIFF_COLS + 2 * lane;                                 // this lane's columns c, c + 1 (ld is even)
    if (c >= ld) return;
    const int64_t t0 = ((slot % row_tiles) * DIFF_WAVES + wave) * DIFF_ROWS;
    const double *xc = x + c;
    for (int64_t t = t0; t < t0 + DIFF_ROWS && t < n; ++t) {
        const int64_t i = order[t];
        const int32_t p1 = ptr[i + 1];
        int32_t e = ptr[i];
        double a0 = 0.0, a1 = 0.0;
        for (; e + DIFF_UNROLL <= p1; e += DIFF_UNROLL) {
            double2 v[DIFF_UNROLL];
#pragma unroll
            for (int u = 0; u < DIFF_UNROLL; ++u)
                v[u] = *reinterpret_cast<const double2 *>(xc + static_cast<int64_t>(col[e + u]) * ld);
#pragma unroll
            for (int u = 0; u < DIFF_UNROLL; ++u) {
                const double su = s[e + u];
                a0 = a0 + su * v[u].x;
                a1 = a1 + su * v[u].y;
            }
        }
        for (; e < p1; ++e) {
            const double2 v = *reinterpret_cast<const double2 *>(xc + static_cast<int64_t>(col[e]) * ld);
            const double su = s[e];
            a0 = a0 + su * v.x;
            a1 = a1 + su * v.y;
        }
        double2 out;
        out.x = beta * a0;
        out.y = beta * a1;
        if (c == i) out.x = alpha + out.x;
        if (c + 1 == i) out.y = alpha + out.y;
        *reinterpret_cast<double2 *>(y + i * ld + c) = out;
    }
}

// --------------------------------------------------------------------------------------
// K -> distances, membership bits and the kept matrix.  One workgroup per 64 x 64 tile (ti <= tj) of the upper triangle: the tile
// of K is read once, row by row, D = 1 - K[a][b] / sqrt(K[a][a] K[b][b]) (clamped at 0; +inf where K[a][b] == 0) goes to LDS, and
// the workgroup writes the tile and, from the transposed LDS image, its mirror -- so D is exactly symmetric and every store is a
// run of 64 adjacent columns, which is also exactly one word of the bit matrix (the wave's ballot).  Every (row, word) and every
// element of the kept matrix is written by exactly one workgroup: no fill pass in front, no atomics.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void diffusion_emit(int64_t row, int64_t word, int64_t column, double d, int64_t n, double cutoff,
                                               uint64_t *__restrict__ bits, int64_t words, double *__restrict__ dist) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const bool member = column < n && ((d <= cutoff && d < inf) || column == row);
    const unsigned long long w = __ballot(member);
    if ((threadIdx.x & 63) == 0) bits[row * words + word] = w;
    if (column < n) dist[row * n + column] = member ? d : inf;
}

__global__ __launch_bounds__(256) void k_diffusion_transform(const double *__restrict__ k, int64_t n, int64_t ld, double cutoff,
                                                             uint64_t *__restrict__ bits, int64_t words, double *__restrict__ dist) {
    const int64_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ double tile[64][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t i0 = ti * 64, j0 = tj * 64;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const int64_t gj = j0 + lane;
    const double kbb = gj < n ? k[gj * ld + gj] : 1.0;
    for (int r = wave; r < 64; r += 4) {
        const int64_t gi = i0 + r;
        double d = inf;
        if (gi < n && gj < n && gi < gj) {
            const double kab = k[gi * ld + gj];
            if (kab != 0.0) {
                d = 1.0 - kab / sqrt(k[gi * ld + gi] * kbb);
                if (d < 0.0) d = 0.0;
            }
        }
        tile[r][lane] = d;
    }
    __syncthreads();
    for (int r = wave; r < 64; r += 4) {
        const int64_t gi = i0 + r;
        if (gi >= n) break;
        double d = tile[r][lane];
        if (ti == tj) d = lane > r ? d : (lane == r ? 0.0 : tile[lane][r]);
        diffusion_emit(gi, tj, gj, d, n, cutoff, bits, words, dist);
    }
    if (ti != tj) {
        for (int r = wave; r < 64; r += 4) {
            const int64_t row = j0 + r;
            if (row >= n) break;
            diffusion_emit(row, ti, i0 + lane, tile[lane][r], n, cutoff, bits, words, dist);
        }
    }
}

// --------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------
static inline size_t diffusion_carve(size_t *cursor, size_t bytes) {
    const size_t at = *cursor;
    *cursor = at + ((bytes + 255) & ~size_t(255));
    return at;
}

extern "C" {

int safe_nbr_diffusion(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v,
                       const double *edge_w, double restart, int steps, double cutoff, double *kernel_out_host, safe_nbr **out) {
    const char *fn = "safe_nbr_diffusion";
    SAFE_REQUIRE(ctx && out && n >= 1 && n_edges >= 0, "%s: bad argument", fn);
    SAFE_REQUIRE(n_edges == 0 || (edge_u && edge_v), "%s: NULL edge arrays", fn);
    SAFE_REQUIRE(restart > 0.0 && restart < 1.0, "%s: restart = %g is outside (0, 1)", fn, restart);
    SAFE_REQUIRE(steps >= 1, "%s: steps = %d is less than 1", fn, steps);
    SAFE_REQUIRE(!(cutoff != cutoff), "%s: the cutoff is NaN", fn);
    if (n > SAFE_SELECT_MAX_NODES) {
        safe_set_error("%s: n = %lld exceeds SAFE_SELECT_MAX_NODES = %d", fn, (long long)n, SAFE_SELECT_MAX_NODES);
        return SAFE_E_UNSUPPORTED;
    }
    // the undirected CSR, a row's entries by (neighbor id, input order): filled in input order, then sorted stably by neighbor id
    std::vector<int32_t> ptr, h_col;
    std::vector<double> h_w;
    SAFE_TRY(build_undirected_csr(fn, n, n_edges, edge_u, edge_v, edge_w, &ptr, &h_col, &h_w));
    const int64_t n_adj = ptr[n];
    {
        std::vector<std::pair<int32_t, double>> ent;
        for (int64_t i = 0; i < n; ++i) {
            ent.clear();
            for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) ent.emplace_back(h_col[e], h_w[e]);
            std::stable_sort(ent.begin(), ent.end(),
                             [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) { return a.first < b.first; });
            for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) {
                h_col[e] = ent[e - ptr[i]].first;
                h_w[e] = ent[e - ptr[i]].second;
            }
        }
    }
    std::vector<int32_t> h_order(n);
    std::iota(h_order.begin(), h_order.end(), 0);
    std::stable_sort(h_order.begin(), h_order.end(),
                     [&](int32_t a, int32_t b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });

    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t ld = (n + 7) & ~int64_t(7);
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    SAFE_TRY(dev_alloc(&nbr->dist, n * n));
    CallBufs b;                                         // (behind the host vectors: the uploads read them)
    CallTimer t_steps, t_transform;
    double *xa = nullptr, *xb = nullptr;
    SAFE_TRY(b.alloc(&xa, n * ld));
    SAFE_TRY(b.alloc(&xb, n * ld));
    size_t bytes = 0;
    const size_t o_ptr = diffusion_carve(&bytes, (n + 1) * sizeof(int32_t));
    const size_t o_col = diffusion_carve(&bytes, std::max<int64_t>(n_adj, 1) * sizeof(int32_t));
    const size_t o_w = diffusion_carve(&bytes, std::max<int64_t>(n_adj, 1) * sizeof(double));
    const size_t o_s = diffusion_carve(&bytes, std::max<int64_t>(n_adj, 1) * sizeof(double));
    const size_t o_r = diffusion_carve(&bytes, n * sizeof(double));
    const size_t o_order = diffusion_carve(&bytes, n * sizeof(int32_t));
    void *graph = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_DIFFUSION_GRAPH, bytes, &graph));
    char *g = static_cast<char *>(graph);
    int32_t *d_ptr = reinterpret_cast<int32_t *>(g + o_ptr), *d_col = reinterpret_cast<int32_t *>(g + o_col);
    int32_t *d_order = reinterpret_cast<int32_t *>(g + o_order);
    double *d_w = reinterpret_cast<double *>(g + o_w), *d_s = reinterpret_cast<double *>(g + o_s);
    double *d_r = reinterpret_cast<double *>(g + o_r);
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_ptr, ptr.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_order, h_order.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_adj) {
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_col, h_col.data(), n_adj * sizeof(int32_t), hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_w, h_w.data(), n_adj * sizeof(double), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_diffusion_scale, dim3(ceil_div(n, 256)), dim3(256), 0, s, n, d_ptr, d_w, d_r);
    hipLaunchKernelGGL(k_diffusion_entries, dim3(ceil_div(n * 64, 256)), dim3(256), 0, s, n, d_ptr, d_col, d_w, d_r, d_s);
    hipLaunchKernelGGL(k_diffusion_identity, dim3(std::min<int64_t>(ceil_div(n * ld, 256), 4096)), dim3(256), 0, s, n, ld, xa);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    const double alpha = restart, beta = 1.0 - alpha;
    const int64_t row_tiles = ceil_div(n, DIFF_ROWS * DIFF_WAVES);
    const dim3 step_grid(row_tiles * DIFF_XCDS * ceil_div(ceil_div(ld, DIFF_COLS), DIFF_XCDS));
    SAFE_HIP_CHECK_AS(fn, t_steps.start(s));
    double *cur = xa, *nxt = xb;
    for (int t = 0; t < steps; ++t) {
        hipLaunchKernelGGL(k_diffusion_step, step_grid, dim3(64 * DIFF_WAVES), 0, s, n, ld, d_ptr, d_col, d_s, d_order, alpha, beta,
                           row_tiles, cur, nxt);
        std::swap(cur, nxt);
    }
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, t_steps.stop(s));
    const int64_t tiles = ceil_div(n, 64);
    SAFE_HIP_CHECK_AS(fn, t_transform.start(s));
    hipLaunchKernelGGL(k_diffusion_transform, dim3(tiles, tiles), dim3(256), 0, s, cur, n, ld, cutoff, nbr->bits, nbr->words,
                       nbr->dist);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, t_transform.stop(s));
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));        // (waits for the stream: the uploads have read the host vectors)
    if (kernel_out_host) {
        SAFE_HIP_CHECK_AS(fn, hipMemcpy2DAsync(kernel_out_host, n * sizeof(double), cur, ld * sizeof(double), n * sizeof(double), n,
                                               hipMemcpyDeviceToHost, s));
        SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    }
    SAFE_HIP_CHECK_AS(fn, t_transform.ms(&ctx->diffusion_ms[1]));
    SAFE_HIP_CHECK_AS(fn, t_steps.finish(ctx, "k_diffusion_step", steps, &ctx->diffusion_ms[0]));
    ctx->diffusion_steps = steps;
    *out = nbr.release();
    return SAFE_OK;
}

int safe_last_diffusion_stats(safe_ctx *ctx, double *steps_ms, int *steps, double *transform_ms) {
    SAFE_REQUIRE(ctx != nullptr, "safe_last_diffusion_stats: ctx is NULL");
    if (steps_ms) *steps_ms = ctx->diffusion_ms[0];
    if (steps) *steps = ctx->diffusion_steps;
    if (transform_ms) *transform_ms = ctx->diffusion_ms[1];
    return SAFE_OK;
}

}  // extern "C"
