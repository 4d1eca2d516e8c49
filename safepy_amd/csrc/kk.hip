// Kamada-Kawai layout on gfx950: the cost and gradient networkx 3.4.2 hands to SciPy's L-BFGS-B, bit for bit.
//
// Replaces the nx.kamada_kawai_layout(G) of apply_network_layout (safepy/safe_io.py:288-308): networkx's
// _kamada_kawai_solve minimises _kamada_kawai_costfn, which builds a handful of [N, N, 2] f64 temporaries per call.
// Here one call is two kernels over the N^2 pairs and nothing of that size is stored besides the two matrices the
// handle keeps: invdist = 1 / (dist_mtx + eye * 1e-3) and its transpose.  The optimiser stays SciPy's, on the host.
//
// The pair (i, j), delta = pos_i - pos_j, all f64, every operation rounded (-ffp-contract=off, correctly rounded
// quotient and square root):
//   sep = sqrt(dx*dx + dy*dy)                     np.linalg.norm(delta, axis=-1)
//   inv = 1 / (sep + (i == j ? 1e-3 : 0))         1 / (nodesep + eye * 1e-3)
//   dir = delta * inv                             einsum("ijk,ij->ijk")
//   off = sep * invdist[i][j] - 1, 0 on the diagonal
//   t(i, j) = (invdist[i][j] * off[i][j]) * dir[i][j]
//   g[i] = ((0 + t(i, 0)) + t(i, 1)) + ...        einsum("ij,ij,ijk->ik"): a chain over j in node order
//   h[j] = ((0 + t(0, j)) + t(1, j)) + ...        einsum("ij,ij,ijk->jk"): a chain over i in node order
//   grad = (g - h) + 1e-3 * sumpos,  cost = 0.5 * sum(off^2) + 0.5e-3 * |sumpos|^2
//
// Gradient (k_kk_grad).  Row i's h chain runs over t(., i): sep is bitwise symmetric, dir[j][i] = -dir[i][j] exactly,
// and invdist[j][i] is read from the transpose, so both chains of a row read row i of a matrix.  Only the four chains of
// a row (gx, gy, hx, hy) are serial: a workgroup owns 16 rows, its four waves compute the terms of a 64-column chunk
// (a wave: 4 rows x 64 consecutive columns, so the matrix loads are whole 512-byte row segments) into LDS, and the 64
// lanes of wave 0 -- one per (row, chain) -- add them in column order while the other waves compute the next chunk
// (double-buffered LDS, 64 KB, one barrier per chunk).  The next chunk's matrix entries are in registers before the current
// chunk's arithmetic starts.
//
// Cost (k_kk_cost).  np.sum(offset**2) is not one pairwise sum: numpy cuts the row-major flat array into buffers of
// 8192 elements (they cross row ends), sums each with its pairwise routine and adds the buffer sums in order.  The
// routine: below 8 elements a sequential sum from 0; up to 128 eight strided accumulators, combined
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder sequentially; above 128 split at n/2 rounded down to a
// multiple of 8.  A full buffer is 64 blocks of 128 under a balanced tree: one wave, a lane per block, then six
// exchange-and-add steps between partner lanes (an add's two operands commute, so both partners hold the same sum).
// The ragged last buffer's blocks (listed by the host from its length) are summed a lane each; the host adds the buffer
// sums in order and walks the ragged buffer's tree over at most 128 block sums.  off is recomputed from pos by flat
// index; nothing of size N^2 is written.  No atomics anywhere: every run gives the same bits.
#include "common.h"

namespace {

constexpr int KK_ROWS = 16;                                  // rows i per workgroup
constexpr int KK_THREADS = 256;
constexpr int KK_WAVES = KK_THREADS / SAFE_WAVE;
constexpr int KK_ROWS_PER_WAVE = KK_ROWS / KK_WAVES;         // terms per thread per chunk
constexpr int KK_CHUNK = SAFE_WAVE;                          // 64 columns j per chunk: a lane per column
constexpr int KK_BUF = 8192;                                 // numpy's reduction buffer, in elements
constexpr int KK_BLOCK = 128;                                // numpy's PW_BLOCKSIZE
constexpr double KK_EPS = 1e-3;                              // eye * 1e-3, and meanweight
static_assert(KK_ROWS * 4 == SAFE_WAVE, "one chain lane per (row, gx / gy / hx / hy)");
static_assert(KK_BUF == SAFE_WAVE * KK_BLOCK, "a full buffer is one block per lane");

__device__ inline double kk_div(double a, double b) { return a / b; }
__device__ inline double kk_sqrt(double a) { return __builtin_sqrt(a); }

// dist -> invdist = 1 / (dist_mtx + eye * 1e-3) in place or from another matrix; inf (unreached) counts as 1e6.
// flag[0] = 1 when a distance is NaN or negative.
__global__ __launch_bounds__(256) void k_kk_invdist(const double *__restrict__ dist, int64_t n, double *__restrict__ inv,
                                                    int *__restrict__ flag) {
    const int64_t total = n * n;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        double d = dist[e];
        if (!(d >= 0.0)) flag[0] = 1;
        if (d == HUGE_VAL) d = 1e6;
        inv[e] = kk_div(1.0, d + (e / n == e % n ? KK_EPS : 0.0));
    }
}

// out = in^T, 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_kk_transpose(const double *__restrict__ in, int64_t n, double *__restrict__ out) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * 32, r0 = static_cast<int64_t>(blockIdx.y) * 32;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < n && c0 + tx < n) tile[k][tx] = in[(r0 + k) * n + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < n && r0 + tx < n) out[(c0 + k) * n + r0 + tx] = tile[tx][k];
}

// One chunk's operands of a thread: the column's position and, per row of the wave, invdist[i][j] and invdist[j][i].
struct KkOperands {
    double xj, yj, a[KK_ROWS_PER_WAVE], b[KK_ROWS_PER_WAVE];
};

__device__ inline void kk_load(KkOperands &o, const double *__restrict__ pos, const double *__restrict__ invd,
                               const double *__restrict__ invd_t, int n, int row0, int j) {
    const bool col_ok = j < n;
    o.xj = col_ok ? pos[2 * j] : 0.0;
    o.yj = col_ok ? pos[2 * j + 1] : 0.0;
#pragma unroll
    for (int q = 0; q < KK_ROWS_PER_WAVE; ++q) {
        const int i = row0 + q;
        const bool ok = col_ok && i < n;
        const int64_t e = static_cast<int64_t>(i) * n + j;
        o.a[q] = ok ? invd[e] : 0.0;
        o.b[q] = ok ? invd_t[e] : 0.0;
    }
}

// grad[i] = (g[i] - h[i]) + (msx, msy), with msx / msy = 1e-3 * sumpos from the host.
__global__ __launch_bounds__(KK_THREADS) void k_kk_grad(const double *__restrict__ pos, int n, const double *__restrict__ invd,
                                                        const double *__restrict__ invd_t, double msx, double msy,
                                                        double *__restrict__ grad) {
    // [buffer][chain row = (gx / gy / hx / hy) * 16 + row][slot]: column jl of chain row R lies in slot (jl + R) % 64, so that the
    // 64 chain lanes, each walking its own row, read 64 different banks (and a wave's 64 writes to one row stay consecutive);
    // 64 KB exactly
    __shared__ double s_term[2][4 * KK_ROWS][KK_CHUNK];

    const int tid = threadIdx.x, lane = tid % SAFE_WAVE, wave = tid / SAFE_WAVE;
    const int rl0 = wave * KK_ROWS_PER_WAVE;                  // the wave's first row inside the tile
    const int row0 = blockIdx.x * KK_ROWS + rl0;
    const int chunks = (n + KK_CHUNK - 1) / KK_CHUNK;
    double xi[KK_ROWS_PER_WAVE], yi[KK_ROWS_PER_WAVE];
#pragma unroll
    for (int q = 0; q < KK_ROWS_PER_WAVE; ++q) {
        const int i = row0 + q;
        xi[q] = i < n ? pos[2 * i] : 0.0;
        yi[q] = i < n ? pos[2 * i + 1] : 0.0;
    }

    KkOperands cur, nxt;
    kk_load(cur, pos, invd, invd_t, n, row0, lane);
    nxt = cur;
    double acc = 0.0;                                         // wave 0: row tid % 16, chain tid / 16
    for (int c = 0; c < chunks; ++c) {
        const int b = c & 1;
        const int j = c * KK_CHUNK + lane;
        if (c + 1 < chunks) kk_load(nxt, pos, invd, invd_t, n, row0, j + KK_CHUNK);   // in flight behind the terms below

#pragma unroll
        for (int q = 0; q < KK_ROWS_PER_WAVE; ++q) {
            const bool diag = row0 + q == j;
            const double dx = xi[q] - cur.xj, dy = yi[q] - cur.yj;
            const double sep = kk_sqrt(dx * dx + dy * dy);
            const double inv = kk_div(1.0, sep + (diag ? KK_EPS : 0.0));
            const double dirx = dx * inv, diry = dy * inv;
            const double off_a = diag ? 0.0 : sep * cur.a[q] - 1.0;
            const double off_b = diag ? 0.0 : sep * cur.b[q] - 1.0;
            const double ca = cur.a[q] * off_a, cb = cur.b[q] * off_b;
            const int r = rl0 + q;
            s_term[b][r][(lane + r) % KK_CHUNK] = ca * dirx;
            s_term[b][KK_ROWS + r][(lane + KK_ROWS + r) % KK_CHUNK] = ca * diry;
            s_term[b][2 * KK_ROWS + r][(lane + 2 * KK_ROWS + r) % KK_CHUNK] = cb * -dirx;   // t(j, i): dir[j][i] = -dir[i][j]
            s_term[b][3 * KK_ROWS + r][(lane + 3 * KK_ROWS + r) % KK_CHUNK] = cb * -diry;
        }
        cur = nxt;
        __syncthreads();

        if (tid < SAFE_WAVE) {                                // the serial part: in column order
            const double *src = &s_term[b][tid][0];           // chain row tid = chain * 16 + row
            const int cnt = min(KK_CHUNK, n - c * KK_CHUNK);
            for (int jl = 0; jl < cnt; ++jl) acc = acc + src[(jl + tid) % KK_CHUNK];
        }
    }

    if (tid < SAFE_WAVE) {
        const double h = __shfl(acc, (tid + 2 * KK_ROWS) % SAFE_WAVE);
        const int i = blockIdx.x * KK_ROWS + tid % KK_ROWS;
        if (tid < 2 * KK_ROWS && i < n) grad[2 * i + tid / KK_ROWS] = (acc - h) + (tid < KK_ROWS ? msx : msy);
    }
}

// numpy's pairwise_sum over the `len` <= 128 values off^2 at flat indices first, first + 1, ...
__device__ inline double kk_block_sum(const double *__restrict__ pos, const double *__restrict__ invd, int64_t n, int64_t first,
                                      int len) {
    int64_t i = first / n, j = first % n;
    double xi = pos[2 * i], yi = pos[2 * i + 1];
    auto next = [&]() {                                       // off[i][j]^2, then one step along the flat array
        const double dx = xi - pos[2 * j], dy = yi - pos[2 * j + 1];
        const double off = i == j ? 0.0 : kk_sqrt(dx * dx + dy * dy) * invd[i * n + j] - 1.0;
        if (++j == n) {
            j = 0;
            if (++i < n) xi = pos[2 * i], yi = pos[2 * i + 1];
        }
        return off * off;
    };
    if (len < 8) {
        double res = 0.0;
        for (int k = 0; k < len; ++k) res = res + next();
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = next();
    int k = 8;
    for (; k < len - len % 8; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = r[u] + next();
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; k < len; ++k) res = res + next();
    return res;
}

// Wave w < n_full: sums[w] = pairwise sum of buffer w.  The waves behind them: sums[n_full + l] = block sum of block l of
// the ragged last buffer, blocks[l] = (offset inside the buffer, length).
__global__ __launch_bounds__(KK_THREADS) void k_kk_cost(const double *__restrict__ pos, const double *__restrict__ invd, int64_t n,
                                                        int64_t n_full, const int2 *__restrict__ blocks, int n_blocks,
                                                        double *__restrict__ sums) {
    const int lane = threadIdx.x % SAFE_WAVE;
    const int64_t w = static_cast<int64_t>(blockIdx.x) * KK_WAVES + threadIdx.x / SAFE_WAVE;
    if (w < n_full) {
        double v = kk_block_sum(pos, invd, n, w * KK_BUF + static_cast<int64_t>(lane) * KK_BLOCK, KK_BLOCK);
        for (int o = 1; o < SAFE_WAVE; o <<= 1) v = v + __shfl_xor(v, o);
        if (lane == 0) sums[w] = v;
    } else {
        const int64_t l = (w - n_full) * SAFE_WAVE + lane;
        if (l < n_blocks) sums[n_full + l] = kk_block_sum(pos, invd, n, n_full * KK_BUF + blocks[l].x, blocks[l].y);
    }
}

// the blocks of numpy's pairwise_sum over `len` elements, in the order its recursion reaches them
void kk_list_blocks(int off, int len, std::vector<int2> &out) {
    if (len <= KK_BLOCK) {
        out.push_back(make_int2(off, len));
        return;
    }
    int half = len / 2;
    half -= half % 8;
    kk_list_blocks(off, half, out);
    kk_list_blocks(off + half, len - half, out);
}

// ... and the sum over them: the same recursion over the block sums
double kk_combine(const double *block_sum, int &next, int len) {
    if (len <= KK_BLOCK) return block_sum[next++];
    int half = len / 2;
    half -= half % 8;
    const double lo = kk_combine(block_sum, next, half);
    const double hi = kk_combine(block_sum, next, len - half);
    return lo + hi;
}

}  // namespace

struct safe_kk {
    safe_ctx *ctx = nullptr;
    int64_t n = 0;
    double *inv = nullptr, *inv_t = nullptr;    // [n][n] invdist and its transpose
    double *d_pos = nullptr, *d_grad = nullptr; // [2n]
    double *d_sums = nullptr;                   // [n_full + blocks.size()]
    int2 *d_blocks = nullptr;
    double *h_stage = nullptr;                  // pinned: pos [2n] | grad [2n] | sums
    int64_t n_full = 0;                         // full 8192-element buffers of the flat [n][n] array
    int ragged = 0;                             // elements of the last, shorter buffer (0: none)
    std::vector<int2> blocks;                   // its blocks
};

static void kk_free(safe_kk *kk) {
    if (!kk) return;
    for (const void *q : {(const void *)kk->inv, (const void *)kk->inv_t, (const void *)kk->d_pos, (const void *)kk->d_grad,
                          (const void *)kk->d_sums, (const void *)kk->d_blocks})
        (void)dev_free(q);
    if (kk->h_stage) (void)hipHostFree(kk->h_stage);
    delete kk;
}

// dist_dev: [n][n] on the device (the handle's own inv buffer when dist_host is uploaded into it first)
static int kk_create(safe_ctx *ctx, int64_t n, const double *dist_host, const double *dist_dev, safe_kk **out) {
    *out = nullptr;
    if (n > SAFE_KK_MAX_NODES) {
        safe_set_error("safe_kk_create: %lld nodes exceed the limit of %lld", (long long)n, (long long)SAFE_KK_MAX_NODES);
        return SAFE_E_UNSUPPORTED;
    }
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<safe_kk, void (*)(safe_kk *)> kk(new safe_kk, kk_free);   // (half built until it is released into *out)
    kk->ctx = ctx;
    kk->n = n;
    kk->n_full = n * n / KK_BUF;
    kk->ragged = static_cast<int>(n * n % KK_BUF);
    if (kk->ragged) kk_list_blocks(0, kk->ragged, kk->blocks);
    const size_t n_sums = static_cast<size_t>(kk->n_full) + kk->blocks.size();
    const char *fn = "safe_kk_create";
    hipStream_t s = ctx->stream;
    CallBufs b;
    int *d_flag = nullptr;
    int flag = 0;
    SAFE_TRY(dev_alloc(&kk->inv, n * n));
    SAFE_TRY(dev_alloc(&kk->inv_t, n * n));
    SAFE_TRY(dev_alloc(&kk->d_pos, 2 * n));
    SAFE_TRY(dev_alloc(&kk->d_grad, 2 * n));
    SAFE_TRY(dev_alloc(&kk->d_sums, n_sums));
    SAFE_TRY(dev_alloc(&kk->d_blocks, kk->blocks.size()));
    SAFE_TRY(b.alloc(&d_flag, 1));
    g_alloc_calls.fetch_add(1, std::memory_order_relaxed);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&kk->h_stage), (4 * n + n_sums) * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        safe_set_error("hipHostMalloc(%zu bytes) failed: %s", (4 * n + n_sums) * sizeof(double), hipGetErrorString(e));
        return SAFE_E_NOMEM;
    }
    if (dist_host) {
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(kk->inv, dist_host, n * n * sizeof(double), hipMemcpyHostToDevice, s));
        dist_dev = kk->inv;
    }
    if (!kk->blocks.empty())
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(kk->d_blocks, kk->blocks.data(), kk->blocks.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_flag, 0, sizeof(int), s));
    const int grid = static_cast<int>(std::min<int64_t>(ceil_div(n * n, 256), 65536));
    hipLaunchKernelGGL(k_kk_invdist, dim3(grid), dim3(256), 0, s, dist_dev, n, kk->inv, d_flag);
    const unsigned tiles = static_cast<unsigned>(ceil_div(n, 32));
    hipLaunchKernelGGL(k_kk_transpose, dim3(tiles, tiles), dim3(256), 0, s, kk->inv, n, kk->inv_t);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    if (flag) {
        safe_set_error("safe_kk_create: the distance matrix holds a NaN or a negative distance");
        return SAFE_E_VALUE;
    }
    *out = kk.release();
    return SAFE_OK;
}

int safe_kk_create_host(safe_ctx *ctx, const double *dist_host, int64_t n, safe_kk **out) {
    SAFE_REQUIRE(ctx && dist_host && out && n >= 1, "safe_kk_create_host: bad argument");
    return kk_create(ctx, n, dist_host, nullptr, out);
}

int safe_kk_create_nbr(safe_ctx *ctx, safe_nbr *nbr, safe_kk **out) {
    SAFE_REQUIRE(ctx && nbr && out, "safe_kk_create_nbr: NULL argument");
    SAFE_REQUIRE(nbr->ctx == ctx, "safe_kk_create_nbr: the membership handle belongs to another context");
    SAFE_REQUIRE(nbr->dist != nullptr, "safe_kk_create_nbr: handle was built without keep_distances");
    return kk_create(ctx, nbr->n, nullptr, nbr->dist, out);
}

int safe_kk_eval(safe_kk *kk, const double *pos_host, double *cost, double *grad_host) {
    SAFE_REQUIRE(kk && pos_host && cost && grad_host, "safe_kk_eval: NULL argument");
    safe_ctx *ctx = kk->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t n = kk->n;
    const size_t n_sums = static_cast<size_t>(kk->n_full) + kk->blocks.size();
    double *h_pos = kk->h_stage, *h_grad = kk->h_stage + 2 * n, *h_sums = kk->h_stage + 4 * n;
    // np.sum(pos_arr, axis=0): the rows added in node order
    double sx = 0.0, sy = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        h_pos[2 * i] = pos_host[2 * i];
        h_pos[2 * i + 1] = pos_host[2 * i + 1];
        sx = sx + pos_host[2 * i];
        sy = sy + pos_host[2 * i + 1];
    }
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(kk->d_pos, h_pos, 2 * n * sizeof(double), hipMemcpyHostToDevice, s));
    const int64_t waves = kk->n_full + ceil_div(static_cast<int64_t>(kk->blocks.size()), SAFE_WAVE);
    hipLaunchKernelGGL(k_kk_cost, dim3(static_cast<unsigned>(ceil_div(waves, KK_WAVES))), dim3(KK_THREADS), 0, s, kk->d_pos, kk->inv,
                       n, kk->n_full, kk->d_blocks, static_cast<int>(kk->blocks.size()), kk->d_sums);
    hipLaunchKernelGGL(k_kk_grad, dim3(static_cast<unsigned>(ceil_div(n, KK_ROWS))), dim3(KK_THREADS), 0, s, kk->d_pos,
                       static_cast<int>(n), kk->inv, kk->inv_t, KK_EPS * sx, KK_EPS * sy, kk->d_grad);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(hipMemcpyAsync(h_grad, kk->d_grad, 2 * n * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(h_sums, kk->d_sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    std::memcpy(grad_host, h_grad, 2 * n * sizeof(double));
    // the buffer sums in order, from 0; the ragged buffer last
    double total = 0.0;
    for (int64_t c = 0; c < kk->n_full; ++c) total = total + h_sums[c];
    if (kk->ragged) {
        int next = 0;
        total = total + kk_combine(h_sums + kk->n_full, next, kk->ragged);
    }
    double c = 0.5 * total;
    c = c + (0.5 * KK_EPS) * (sx * sx + sy * sy);
    *cost = c;
    return SAFE_OK;
}

int safe_kk_destroy(safe_kk *kk) {
    if (!kk) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(kk->ctx->device));
    SAFE_HIP_CHECK(safe_stream_sync(kk->ctx->stream));
    kk_free(kk);
    return SAFE_OK;
}
