// Spring-embedded layout on gfx950: networkx 3.4.2's Fruchterman-Reingold iteration, bit for bit.
//
// Replaces the layout step of load_network_from_txt (safepy/safe_io.py:288-308,
// nx.spring_layout(G, k=0.2, iterations=100, seed=...)).  networkx runs one of two restatements of
// the same iteration:
//   N <  500  _fruchterman_reingold         f64 throughout; displacement = einsum over j, then
//                                           delta_pos = displacement * (t / length)
//   N >= 500  _sparse_fruchterman_reingold  f32 positions, weights, k, t; each row's force is an f32
//                                           sum over j (numpy adds the F-ordered (2, N) product
//                                           sequentially in j), widened into an f64 displacement;
//                                           delta_pos = displacement * t / length in f64, and
//                                           pos = f32(f64(pos) + delta_pos)
// The term of the pair (i, j), dx = pos_i - pos_j, d = max(sqrt(dx*dx + dy*dy), 0.01):
//   (dx, dy) * (kk / (d*d) - (A_ij * d) / k)
// and for A_ij == 0 the subtracted quotient is +0, so a non-neighbour's term is (dx, dy) * kk / (d*d)
// exactly.  Compiled with -ffp-contract=off: every operation is rounded as numpy rounds it.  The f32
// quotients and square roots are the correctly rounded ones (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt: v_div_scale / v_div_fmas / v_div_fixup, and v_sqrt_f32
// followed by its correction), f64 likewise.
//
// Order.  A row's force must be ((0 + term_0) + term_1) + ... + term_{N-1}, in node order.  Only that
// add chain is serial: a workgroup owns 16 rows, its 256 threads compute the terms of a 128-column
// chunk (16 rows x 8 columns each) into LDS, and 32 lanes of wave 0 -- one per (row, component) --
// add them in order while the other waves compute the next chunk (double-buffered LDS, one barrier
// per chunk).  Neighbour weights come from a per-(row tile, chunk) list built on the host from the
// CSR, scattered into an LDS row of weights that the compute threads read (and reset to 0).
//
// Iterations.  One launch per iteration, positions double-buffered.  Each launch adds its
// sum of delta_pos^2 into sumsq[it] (f64 atomics: the order of that sum is not numpy's BLAS ddot, so
// the early-stop decision norm(delta_pos) / N < threshold can differ from networkx's only when the
// ratio lies within rounding of the threshold); launch it + 1 reads it and returns at once once the
// ratio is below the threshold, so the host enqueues every iteration without waiting.
#include <type_traits>

#include "common.h"

namespace {

constexpr int LT_ROWS = 16;                                  // rows i per workgroup
constexpr int LT_THREADS = 256;
constexpr int LT_COLS_PER_THREAD = 8;                        // terms per thread per chunk
constexpr int LT_CHUNK = LT_THREADS / LT_ROWS * LT_COLS_PER_THREAD;   // 128 columns j per chunk
constexpr int LT_STRIDE = LT_CHUNK + 4;                      // LDS row stride: writers and the b128 readers avoid bank conflicts
constexpr int64_t LT_MAX_N = 65536;                          // host-built neighbour lists: (N/16) x (N/128) offsets

__device__ inline float div_rn(float a, float b) { return a / b; }
__device__ inline double div_rn(double a, double b) { return a / b; }
__device__ inline float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ inline double sqrt_rn(double a) { return __builtin_sqrt(a); }

// One iteration.  state[0] = stopped, state[1] = iterations run; sumsq[it] = sum of delta_pos^2 of iteration it.
template <typename T>
__global__ __launch_bounds__(LT_THREADS) void k_spring_step(const T *__restrict__ pos_in, T *__restrict__ pos_out, int n,
                                                            const int *__restrict__ nb_off, const int *__restrict__ nb_slot,
                                                            const T *__restrict__ nb_w, T kk, T k, T dmin, T t, int it,
                                                            double threshold, double *__restrict__ sumsq,
                                                            int *__restrict__ state) {
    if (it > 0 && (state[0] != 0 || sqrt(sumsq[it - 1]) / static_cast<double>(n) < threshold)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) state[0] = 1;   // every block of this launch decides the same
        return;
    }
    __shared__ T s_term[2][2][LT_ROWS][LT_STRIDE];           // [buffer][x / y][row][column in chunk]
    __shared__ T s_w[2][LT_ROWS][LT_STRIDE];                 // A_ij of the chunk's columns, 0 = not a neighbour
    __shared__ T s_pos[2][LT_CHUNK * 2];                     // the chunk's positions, x y interleaved

    const int tid = threadIdx.x;
    const int r = tid % LT_ROWS, jq = tid / LT_ROWS;
    const int i = blockIdx.x * LT_ROWS + r;
    const int chunks = (n + LT_CHUNK - 1) / LT_CHUNK;
    const int *off = nb_off + static_cast<int64_t>(blockIdx.x) * chunks;
    const T xi = i < n ? pos_in[2 * i] : T(0);
    const T yi = i < n ? pos_in[2 * i + 1] : T(0);

    for (int e = tid; e < 2 * LT_ROWS * LT_STRIDE; e += LT_THREADS) (&s_w[0][0][0])[e] = T(0);
    __syncthreads();
    {   // chunk 0 into buffer 0
        if (tid < 2 * n) s_pos[0][tid] = pos_in[tid];
        for (int e = off[0] + tid; e < off[1]; e += LT_THREADS) (&s_w[0][0][0])[nb_slot[e]] = nb_w[e];
    }
    __syncthreads();

    T acc = T(0);                                             // wave 0, lanes < 32: row tid % 16, component tid / 16
    for (int c = 0; c < chunks; ++c) {
        const int b = c & 1;
        // the next chunk's positions and first neighbour entry, loaded before the terms so their latency hides behind them
        const bool more = c + 1 < chunks;
        const int jn = (c + 1) * LT_CHUNK * 2 + tid;
        T p_next = T(0);
        if (more && jn < 2 * n) p_next = pos_in[jn];
        const int e0 = more ? off[c + 1] + tid : 0, e1 = more ? off[c + 2] : 0;
        int slot0 = 0;
        T w0 = T(0);
        if (e0 < e1) {
            slot0 = nb_slot[e0];
            w0 = nb_w[e0];
        }

#pragma unroll
        for (int q = 0; q < LT_COLS_PER_THREAD; ++q) {
            const int jl = jq + q * (LT_THREADS / LT_ROWS);
            const T dx = xi - s_pos[b][2 * jl], dy = yi - s_pos[b][2 * jl + 1];
            T d = sqrt_rn(dx * dx + dy * dy);
            d = d < dmin ? dmin : d;
            T w = div_rn(kk, d * d);
            const T a = s_w[b][r][jl];
            if (a != T(0)) {
                s_w[b][r][jl] = T(0);
                w = w - div_rn(a * d, k);
            }
            s_term[b][0][r][jl] = dx * w;
            s_term[b][1][r][jl] = dy * w;
        }

        if (more) {
            const int nb = b ^ 1;
            s_pos[nb][tid] = p_next;
            if (e0 < e1) (&s_w[nb][0][0])[slot0] = w0;
            for (int e = e0 + LT_THREADS; e < e1; e += LT_THREADS) (&s_w[nb][0][0])[nb_slot[e]] = nb_w[e];
        }
        __syncthreads();

        if (tid < 2 * LT_ROWS) {                              // the serial part: in column order
            const T *src = &s_term[b][tid / LT_ROWS][tid % LT_ROWS][0];
            const int cnt = min(LT_CHUNK, n - c * LT_CHUNK);
            for (int jl = 0; jl < cnt; ++jl) acc = acc + src[jl];
        }
    }

    if (tid < SAFE_WAVE) {
        const T acc_y = __shfl(acc, (tid + LT_ROWS) % SAFE_WAVE);
        double dp2 = 0.0;
        if (tid < LT_ROWS && i < n) {
            const double fx = static_cast<double>(acc), fy = static_cast<double>(acc_y);
            double len = sqrt(fx * fx + fy * fy);
            if (len < 0.01) len = 0.1;
            double px, py;
            if constexpr (std::is_same<T, float>::value) {       // (displacement * t / length).T
                px = (fx * static_cast<double>(t)) / len;
                py = (fy * static_cast<double>(t)) / len;
            } else {                                              // einsum("ij,i->ij", displacement, t / length)
                const double s = static_cast<double>(t) / len;
                px = fx * s;
                py = fy * s;
            }
            pos_out[2 * i] = static_cast<T>(static_cast<double>(xi) + px);
            pos_out[2 * i + 1] = static_cast<T>(static_cast<double>(yi) + py);
            dp2 = px * px + py * py;
        }
        for (int o = LT_ROWS / 2; o >= 1; o >>= 1) dp2 += __shfl_down(dp2, o);
        if (tid == 0) {
            atomicAdd(&sumsq[it], dp2);
            if (blockIdx.x == 0) state[1] = it + 1;
        }
    }
}

template <typename T>
int layout_run(safe_ctx *ctx, int n, const int32_t *row_ptr, const int32_t *col, const double *weight, const double *pos0,
               double k, int iterations, double threshold, double *pos_out, int *iterations_run) {
    const int tiles = (n + LT_ROWS - 1) / LT_ROWS, chunks = (n + LT_CHUNK - 1) / LT_CHUNK;
    const int64_t nnz = row_ptr[n];
    // neighbour entries grouped by (row tile, chunk): slot = row-in-tile * LT_STRIDE + column-in-chunk
    std::vector<int> off(static_cast<size_t>(tiles) * chunks + 1, 0);
    for (int i = 0; i < n; ++i)
        for (int32_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p) off[static_cast<size_t>(i / LT_ROWS) * chunks + col[p] / LT_CHUNK + 1]++;
    for (size_t q = 1; q < off.size(); ++q) off[q] += off[q - 1];
    std::vector<int> fill(off.begin(), off.end() - 1), slot(std::max<int64_t>(nnz, 1));
    std::vector<T> w(std::max<int64_t>(nnz, 1));
    for (int i = 0; i < n; ++i)
        for (int32_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p) {
            const int e = fill[static_cast<size_t>(i / LT_ROWS) * chunks + col[p] / LT_CHUNK]++;
            slot[e] = (i % LT_ROWS) * LT_STRIDE + col[p] % LT_CHUNK;
            w[e] = static_cast<T>(weight ? weight[p] : 1.0);      // to_scipy_sparse_array(dtype='f') rounds the weights to f32
        }

    // positions in the branch's dtype and the cooling schedule, as networkx computes them in that dtype
    std::vector<T> pos(2 * static_cast<size_t>(n));
    for (size_t q = 0; q < pos.size(); ++q) pos[q] = static_cast<T>(pos0[q]);
    T xmin = pos[0], xmax = pos[0], ymin = pos[1], ymax = pos[1];
    for (int i = 1; i < n; ++i) {
        xmin = std::min(xmin, pos[2 * i]), xmax = std::max(xmax, pos[2 * i]);
        ymin = std::min(ymin, pos[2 * i + 1]), ymax = std::max(ymax, pos[2 * i + 1]);
    }
    const T xr = xmax - xmin, yr = ymax - ymin;
    T t = (yr > xr ? yr : xr) * static_cast<T>(0.1);
    const T dt = t / static_cast<T>(iterations + 1);
    const T kk = static_cast<T>(k * k), kt = static_cast<T>(k), dmin = static_cast<T>(0.01);

    CallBufs bufs;
    T *d_pos = nullptr, *d_w = nullptr;
    int *d_off = nullptr, *d_slot = nullptr, *d_state = nullptr;
    double *d_sumsq = nullptr;
    SAFE_TRY(bufs.alloc(&d_pos, 4 * static_cast<size_t>(n)));
    SAFE_TRY(bufs.alloc(&d_off, off.size()));
    SAFE_TRY(bufs.alloc(&d_slot, slot.size()));
    SAFE_TRY(bufs.alloc(&d_w, w.size()));
    SAFE_TRY(bufs.alloc(&d_sumsq, std::max(iterations, 1)));
    SAFE_TRY(bufs.alloc(&d_state, 2));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(d_pos, pos.data(), pos.size() * sizeof(T), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_slot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_w, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemsetAsync(d_sumsq, 0, std::max(iterations, 1) * sizeof(double), s));
    SAFE_HIP_CHECK(hipMemsetAsync(d_state, 0, 2 * sizeof(int), s));
    for (int it = 0; it < iterations; ++it) {
        const T *src = d_pos + (it & 1) * 2 * static_cast<size_t>(n);
        T *dst = d_pos + ((it + 1) & 1) * 2 * static_cast<size_t>(n);
        hipLaunchKernelGGL(k_spring_step<T>, dim3(tiles), dim3(LT_THREADS), 0, s, src, dst, n, d_off, d_slot, d_w, kk, kt,
                           dmin, t, it, threshold, d_sumsq, d_state);
        SAFE_HIP_CHECK(hipGetLastError());
        t = t - dt;
    }
    int state[2] = {0, 0};
    SAFE_HIP_CHECK(hipMemcpyAsync(state, d_state, sizeof(state), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(pos.data(), d_pos + (state[1] & 1) * 2 * static_cast<size_t>(n), pos.size() * sizeof(T),
                                  hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    for (size_t q = 0; q < pos.size(); ++q) pos_out[q] = static_cast<double>(pos[q]);
    if (iterations_run) *iterations_run = state[1];
    return SAFE_OK;
}

}  // namespace

int safe_layout_spring(safe_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const double *weight, int dtype,
                       const double *pos0, double k, int iterations, double threshold, double *pos_out,
                       int *iterations_run) {
    SAFE_REQUIRE(ctx && row_ptr && pos0 && pos_out && n >= 1 && iterations >= 0, "safe_layout_spring: bad argument");
    SAFE_REQUIRE(dtype == SAFE_DTYPE_F32 || dtype == SAFE_DTYPE_F64, "safe_layout_spring: dtype must be F32 or F64");
    if (n > LT_MAX_N) {
        safe_set_error("safe_layout_spring: %lld nodes exceed the kernel's limit of %lld", (long long)n, (long long)LT_MAX_N);
        return SAFE_E_UNSUPPORTED;
    }
    SAFE_REQUIRE(row_ptr[0] == 0 && (row_ptr[n] == 0 || col), "safe_layout_spring: bad CSR");
    for (int64_t i = 0; i < n; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) {
            safe_set_error("safe_layout_spring: row_ptr decreases at row %lld", (long long)i);
            return SAFE_E_VALUE;
        }
        for (int32_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p)
            if (col[p] < 0 || col[p] >= n || (p > row_ptr[i] && col[p] <= col[p - 1])) {
                safe_set_error("safe_layout_spring: row %lld: columns must be in [0,%lld) and strictly increasing", (long long)i,
                               (long long)n);
                return SAFE_E_VALUE;
            }
    }
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    if (iterations_run) *iterations_run = 0;
    return dtype == SAFE_DTYPE_F32
               ? layout_run<float>(ctx, static_cast<int>(n), row_ptr, col, weight, pos0, k, iterations, threshold, pos_out,
                                   iterations_run)
               : layout_run<double>(ctx, static_cast<int>(n), row_ptr, col, weight, pos0, k, iterations, threshold, pos_out,
                                    iterations_run);
}
