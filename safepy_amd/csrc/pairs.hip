// The enriched (node, attribute) pairs of a device-resident result matrix as CSR or CSC, compacted on the device.
//
// Replaces the np.nonzero(nes_binary) / nes[r, c] a caller runs on the host after reading the whole f64 [n, m] matrices
// (the selection of safepy/safe.py:468-472: nes_binary > 0, or |nes| > t): the selector matrix is read where it lies,
// twice -- once to count (safe_pairs_create), once to emit (safe_pairs_read) -- and only the pointer array, the indices
// and the values at the selected cells cross the link.  Nothing of size n * m is written, no host loop touches n * m cells.
//
// By row (CSR).  A row is cut into chunks of PAIRS_ROW_CHUNK columns; a wave owns one (row, chunk) and walks it in steps
// of 64 columns, one 512-byte read per step, PAIRS_UNROLL steps in flight.  The 64-bit ballot of the predicate is the step's
// selection: create adds its population count, read places lane l's entry at base + running + mbcnt(ballot), so the entries
// of a row come out in column order without a sort.  The per-(row, chunk) counts lie row-major, so ONE flat exclusive scan
// gives every chunk's base, and every row's pointer is the base of its first chunk.
//
// By column (CSC).  The matrix is cut into blocks of PAIRS_COL_ROWS rows; a wave owns 64 adjacent columns of one block and
// every lane walks its column down the block (a row step is one coalesced 512-byte read).  create writes the int32 count table
// [blocks][m]; k_pairs_colscan turns every column of the table into its running offsets and leaves the column totals,
// whose flat scan is the pointer array.  In read a lane stores at pointer[column] + table[block][column] + its running
// count: row order inside every column.
//
// The scan (k_pairs_scan) is one workgroup walking the counts in tiles -- they are 1/2048 (rows) or 1/n (columns) of the
// cells.  Offsets are 64-bit on the device, so an nnz of 2^31 or more is seen (and refused) rather than wrapped; the
// int32 pointer array SciPy wants is written once nnz is known to fit.
//
// The selector is the caller's memory and may have changed between the two calls.  read never trusts it: every store is
// clamped to the range [base, limit) the scan gave the wave (row chunk) or the lane (column block), and a wave whose
// selection does not fill exactly that range raises a flag -- the call then fails with SAFE_E_VALUE and copies nothing out.
#include "common.h"

namespace {

constexpr int PAIRS_THREADS = 256;
constexpr int PAIRS_WAVES = PAIRS_THREADS / SAFE_WAVE;
constexpr int PAIRS_ROW_CHUNK = 2048;                        // columns of a row one wave walks (by row)
constexpr int PAIRS_UNROLL = 4;                              // 64-column steps whose loads are issued together
constexpr int PAIRS_COL_ROWS = 64;                           // rows of a block (by column)
constexpr int PAIRS_SCAN_THREADS = 1024;
constexpr int PAIRS_SCAN_ITEMS = 4;                          // consecutive counts per thread and tile
constexpr int PAIRS_SCAN_TILE = PAIRS_SCAN_THREADS * PAIRS_SCAN_ITEMS;
static_assert(PAIRS_ROW_CHUNK % (SAFE_WAVE * PAIRS_UNROLL) == 0, "a chunk is whole unrolled steps");

// mode 0: x > 0   1: |x| > t   2: x > t   3: x < -t.  Strict; NaN compares false everywhere.
__device__ inline bool pairs_selected(double x, int mode, double t) {
    switch (mode) {
        case 0: return x > 0.0;
        case 1: return fabs(x) > t;
        case 2: return x > t;
        default: return x < -t;
    }
}

__device__ inline int pairs_lanes_below(unsigned long long ballot) {
    return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(ballot >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(ballot), 0u)));
}

// EMIT = false: counts[task] = selected cells of the (row, chunk).  EMIT = true: their column indices (and values) at
// offs[task] .. offs[task + 1].  task = row * chunks + chunk.
template <bool EMIT>
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_rows(const double *__restrict__ sel, const unsigned long long *__restrict__ values,
                                                              int64_t m, int64_t chunks, int64_t tasks, int mode, double t,
                                                              int32_t *__restrict__ counts, const int64_t *__restrict__ offs,
                                                              int32_t *__restrict__ indices, unsigned long long *__restrict__ data,
                                                              int *__restrict__ flag) {
    const int lane = threadIdx.x % SAFE_WAVE;
    const int64_t task = static_cast<int64_t>(blockIdx.x) * PAIRS_WAVES + threadIdx.x / SAFE_WAVE;
    if (task >= tasks) return;                               // (the whole wave)
    const int64_t row = task / chunks, c0 = (task % chunks) * PAIRS_ROW_CHUNK;
    const int64_t c1 = min(m, c0 + PAIRS_ROW_CHUNK);
    const int64_t cell0 = row * m;
    const bool same = EMIT && values == reinterpret_cast<const unsigned long long *>(sel);
    int64_t base = 0, limit = 0;
    if (EMIT) base = offs[task], limit = offs[task + 1];
    int running = 0;
    bool spilled = false;
    for (int64_t c = c0; c < c1; c += SAFE_WAVE * PAIRS_UNROLL) {
        double x[PAIRS_UNROLL];
#pragma unroll
        for (int u = 0; u < PAIRS_UNROLL; ++u) {
            const int64_t col = c + u * SAFE_WAVE + lane;
            x[u] = col < c1 ? sel[cell0 + col] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PAIRS_UNROLL; ++u) {
            const int64_t col = c + u * SAFE_WAVE + lane;
            const bool hit = col < c1 && pairs_selected(x[u], mode, t);
            const unsigned long long ballot = __ballot(hit);
            if (EMIT && hit) {
                const int64_t at = base + running + pairs_lanes_below(ballot);
                if (at < limit) {
                    indices[at] = static_cast<int32_t>(col);
                    if (data) data[at] = same ? static_cast<unsigned long long>(__double_as_longlong(x[u])) : values[cell0 + col];
                } else {
                    spilled = true;
                }
            }
            running += __popcll(ballot);
        }
    }
    if (!EMIT) {
        if (lane == 0) counts[task] = running;
    } else if (spilled || (lane == 0 && base + running != limit)) {
        flag[0] = 1;
    }
}

// A wave: columns g * 64 .. + 63 of row block b.  EMIT = false: table[b][column] = selected cells of the column inside the
// block.  EMIT = true: table holds the column's running offsets (k_pairs_colscan); row indices (and values) at
// offs[column] + table[b][column] ...
template <bool EMIT>
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_cols(const double *__restrict__ sel, const unsigned long long *__restrict__ values,
                                                              int64_t n, int64_t m, int64_t groups, int64_t blocks, int mode, double t,
                                                              int32_t *__restrict__ table, const int64_t *__restrict__ offs,
                                                              int32_t *__restrict__ indices, unsigned long long *__restrict__ data,
                                                              int *__restrict__ flag) {
    const int lane = threadIdx.x % SAFE_WAVE;
    const int64_t task = static_cast<int64_t>(blockIdx.x) * PAIRS_WAVES + threadIdx.x / SAFE_WAVE;
    if (task >= groups * blocks) return;
    const int64_t b = task / groups, col = (task % groups) * SAFE_WAVE + lane;
    if (col >= m) return;
    const int64_t r0 = b * PAIRS_COL_ROWS, r1 = min(n, r0 + PAIRS_COL_ROWS);
    const bool same = EMIT && values == reinterpret_cast<const unsigned long long *>(sel);
    int64_t at = 0, limit = 0;
    if (EMIT) {
        const int64_t col0 = offs[col];
        at = col0 + table[b * m + col];
        limit = b + 1 < blocks ? col0 + table[(b + 1) * m + col] : offs[col + 1];
    }
    int count = 0;
    bool spilled = false;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
        const double x = sel[r * m + col];
        if (pairs_selected(x, mode, t)) {
            if (!EMIT) {
                ++count;
            } else if (at < limit) {
                indices[at] = static_cast<int32_t>(r);
                if (data) data[at] = same ? static_cast<unsigned long long>(__double_as_longlong(x)) : values[r * m + col];
                ++at;
            } else {
                spilled = true;
            }
        }
    }
    if (!EMIT) {
        table[b * m + col] = count;
    } else if (spilled || at != limit) {
        flag[0] = 1;
    }
}

// table[.][c] -> its exclusive running sums down the column; totals[c] = the column's sum
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_colscan(int32_t *__restrict__ table, int64_t m, int64_t blocks,
                                                                 int32_t *__restrict__ totals) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * PAIRS_THREADS + threadIdx.x;
    if (c >= m) return;
    int32_t run = 0;
#pragma unroll 8
    for (int64_t b = 0; b < blocks; ++b) {
        const int32_t v = table[b * m + c];
        table[b * m + c] = run;
        run += v;
    }
    totals[c] = run;
}

// offs[i] = counts[0] + ... + counts[i - 1] for i = 0 .. len (64-bit), one workgroup
__global__ __launch_bounds__(PAIRS_SCAN_THREADS) void k_pairs_scan(const int32_t *__restrict__ counts, int64_t len, int64_t *__restrict__ offs) {
    __shared__ int64_t s_wave[PAIRS_SCAN_THREADS / SAFE_WAVE];
    __shared__ int64_t s_carry;
    const int tid = threadIdx.x, lane = tid % SAFE_WAVE, wave = tid / SAFE_WAVE;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t tile = 0; tile < len; tile += PAIRS_SCAN_TILE) {
        const int64_t i0 = tile + static_cast<int64_t>(tid) * PAIRS_SCAN_ITEMS;
        int64_t v[PAIRS_SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int k = 0; k < PAIRS_SCAN_ITEMS; ++k) {
            v[k] = i0 + k < len ? counts[i0 + k] : 0;
            mine += v[k];
        }
        int64_t incl = mine;                                  // inclusive scan of the threads' sums inside the wave
        for (int o = 1; o < SAFE_WAVE; o <<= 1) {
            const int64_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == SAFE_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        int64_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        int64_t run = before + incl - mine;
#pragma unroll
        for (int k = 0; k < PAIRS_SCAN_ITEMS; ++k) {
            if (i0 + k < len) offs[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();                                      // everybody has read s_carry and s_wave
        if (tid == PAIRS_SCAN_THREADS - 1) s_carry = run;
        __syncthreads();
    }
    if (tid == 0) offs[len] = s_carry;
}

// indptr[i] = offs[i * stride], i = 0 .. dim (nnz < 2^31 is known)
__global__ __launch_bounds__(PAIRS_THREADS) void k_pairs_indptr(const int64_t *__restrict__ offs, int64_t stride, int64_t dim,
                                                                int32_t *__restrict__ indptr) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * PAIRS_THREADS + threadIdx.x;
    if (i <= dim) indptr[i] = static_cast<int32_t>(offs[i * stride]);
}

constexpr int64_t PAIRS_INT32_END = int64_t(1) << 31;

}  // namespace

hipError_t pairs_scan_launch(hipStream_t s, const int32_t *counts, int64_t len, int64_t *offs) {
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(PAIRS_SCAN_THREADS), 0, s, counts, len, offs);
    return hipGetLastError();
}

struct safe_pairs {
    safe_ctx *ctx = nullptr;
    int64_t n = 0, m = 0, nnz = 0;
    int mode = 0, axis = 0;
    double threshold = 0.0;
    int64_t chunks = 0;             // by row: chunks of a row
    int64_t blocks = 0, groups = 0; // by column: row blocks, 64-column groups
    int64_t scan_len = 0;           // entries of offs, - 1
    int64_t *offs = nullptr;        // [scan_len + 1] by row: base of every (row, chunk); by column: first entry of every column
    int32_t *indptr = nullptr;      // [n + 1] or [m + 1]
    int32_t *table = nullptr;       // by column: [blocks][m] running offsets inside the column
};

static void pairs_free(safe_pairs *p) {
    if (!p) return;
    (void)dev_free(p->offs);
    (void)dev_free(p->indptr);
    (void)dev_free(p->table);
    delete p;
}

extern "C" {

int safe_pairs_create(safe_ctx *ctx, const double *selector_dev, int64_t n, int64_t m, int mode, double threshold, int axis,
                      safe_pairs **out, int64_t *nnz, double *kernel_ms) {
    SAFE_REQUIRE(ctx && out && nnz && n >= 0 && m >= 0, "safe_pairs_create: bad argument");
    *out = nullptr;
    SAFE_REQUIRE(mode >= 0 && mode <= 3, "safe_pairs_create: mode %d is not 0 (> 0), 1 (|x| > t), 2 (x > t) or 3 (x < -t)", mode);
    SAFE_REQUIRE(axis == 0 || axis == 1, "safe_pairs_create: axis %d is not 0 (by row) or 1 (by column)", axis);
    if (mode != 0 && !(threshold >= 0.0)) {
        safe_set_error("safe_pairs_create: the threshold must be a number >= 0 (inf allowed), got %g", threshold);
        return SAFE_E_VALUE;
    }
    if (n >= PAIRS_INT32_END || m >= PAIRS_INT32_END) {
        safe_set_error("safe_pairs_create: a [%lld, %lld] matrix does not fit 32-bit indices (each side must be below 2^31)",
                       (long long)n, (long long)m);
        return SAFE_E_UNSUPPORTED;
    }
    if (kernel_ms) *kernel_ms = 0;
    std::unique_ptr<safe_pairs, void (*)(safe_pairs *)> p(new safe_pairs, pairs_free);
    p->ctx = ctx;
    p->n = n, p->m = m, p->mode = mode, p->axis = axis, p->threshold = mode ? threshold : 0.0;
    if (n == 0 || m == 0) {                                   // nothing to read: an all-zero pointer array, made by safe_pairs_read
        *nnz = 0;
        *out = p.release();
        return SAFE_OK;
    }
    SAFE_REQUIRE(selector_dev, "safe_pairs_create: selector_dev is NULL");
    const int64_t dim = axis == 0 ? n : m;
    int64_t tasks;
    if (axis == 0) {
        p->chunks = ceil_div(m, PAIRS_ROW_CHUNK);
        p->scan_len = tasks = n * p->chunks;
    } else {
        p->blocks = ceil_div(n, PAIRS_COL_ROWS);
        p->groups = ceil_div(m, SAFE_WAVE);
        p->scan_len = m;
        tasks = p->blocks * p->groups;
    }
    SAFE_REQUIRE(ceil_div(tasks, PAIRS_WAVES) < PAIRS_INT32_END, "safe_pairs_create: too many cells for one launch");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const char *fn = "safe_pairs_create";
    hipStream_t s = ctx->stream;
    CallBufs b;
    int32_t *d_counts = nullptr;                              // by row: [tasks]; by column: the column totals [m]
    SAFE_TRY(dev_alloc(&p->offs, static_cast<size_t>(p->scan_len + 1)));
    SAFE_TRY(dev_alloc(&p->indptr, static_cast<size_t>(dim + 1)));
    if (axis == 1) SAFE_TRY(dev_alloc(&p->table, static_cast<size_t>(p->blocks * m)));
    SAFE_TRY(b.alloc(&d_counts, static_cast<size_t>(p->scan_len)));
    const unsigned grid = static_cast<unsigned>(ceil_div(tasks, PAIRS_WAVES));
    CallTimer tm;
    SAFE_HIP_CHECK_AS(fn, tm.start(s));
    if (axis == 0) {
        hipLaunchKernelGGL(k_pairs_rows<false>, dim3(grid), dim3(PAIRS_THREADS), 0, s, selector_dev,
                           static_cast<const unsigned long long *>(nullptr), m, p->chunks, tasks, mode, p->threshold, d_counts,
                           static_cast<const int64_t *>(nullptr), static_cast<int32_t *>(nullptr),
                           static_cast<unsigned long long *>(nullptr), static_cast<int *>(nullptr));
    } else {
        hipLaunchKernelGGL(k_pairs_cols<false>, dim3(grid), dim3(PAIRS_THREADS), 0, s, selector_dev,
                           static_cast<const unsigned long long *>(nullptr), n, m, p->groups, p->blocks, mode, p->threshold, p->table,
                           static_cast<const int64_t *>(nullptr), static_cast<int32_t *>(nullptr),
                           static_cast<unsigned long long *>(nullptr), static_cast<int *>(nullptr));
        SAFE_HIP_CHECK_AS(fn, hipGetLastError());
        hipLaunchKernelGGL(k_pairs_colscan, dim3(static_cast<unsigned>(ceil_div(m, PAIRS_THREADS))), dim3(PAIRS_THREADS), 0, s, p->table, m,
                           p->blocks, d_counts);
    }
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(PAIRS_SCAN_THREADS), 0, s, d_counts, p->scan_len, p->offs);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, tm.stop(s));
    int64_t total = 0;
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(&total, p->offs + p->scan_len, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    SAFE_HIP_CHECK_AS(fn, tm.finish(ctx, axis == 0 ? "k_pairs_rows<count>" : "k_pairs_cols<count>", 1, kernel_ms));
    if (total >= PAIRS_INT32_END) {
        safe_set_error("safe_pairs_create: %lld selected cells do not fit 32-bit indices (nnz must be below 2^31)", (long long)total);
        return SAFE_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_pairs_indptr, dim3(static_cast<unsigned>(ceil_div(dim + 1, PAIRS_THREADS))), dim3(PAIRS_THREADS), 0, s, p->offs,
                       axis == 0 ? p->chunks : int64_t(1), dim, p->indptr);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    p->nnz = total;
    *nnz = total;
    *out = p.release();
    return SAFE_OK;
}

int safe_pairs_read(safe_pairs *pairs, const double *selector_dev, const double *values_dev, int32_t *indptr_host, int32_t *indices_host,
                    double *data_host, double *kernel_ms) {
    SAFE_REQUIRE(pairs && indptr_host, "safe_pairs_read: NULL argument");
    safe_pairs *p = pairs;
    const int64_t dim = p->axis == 0 ? p->n : p->m;
    if (kernel_ms) *kernel_ms = 0;
    if (p->n == 0 || p->m == 0) {
        std::memset(indptr_host, 0, static_cast<size_t>(dim + 1) * sizeof(int32_t));
        return SAFE_OK;
    }
    SAFE_REQUIRE(selector_dev, "safe_pairs_read: selector_dev is NULL");
    SAFE_REQUIRE(p->nnz == 0 || indices_host, "safe_pairs_read: indices_host is NULL");
    SAFE_REQUIRE(!values_dev || p->nnz == 0 || data_host, "safe_pairs_read: values_dev without data_host");
    safe_ctx *ctx = p->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const char *fn = "safe_pairs_read";
    hipStream_t s = ctx->stream;
    CallBufs b;
    int32_t *d_indices = nullptr;
    unsigned long long *d_data = nullptr;
    int *d_flag = nullptr;
    SAFE_TRY(b.alloc(&d_indices, static_cast<size_t>(p->nnz)));
    if (values_dev) SAFE_TRY(b.alloc(&d_data, static_cast<size_t>(p->nnz)));
    SAFE_TRY(b.alloc(&d_flag, 1));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_flag, 0, sizeof(int), s));
    const unsigned long long *values = reinterpret_cast<const unsigned long long *>(values_dev);
    const int64_t tasks = p->axis == 0 ? p->scan_len : p->blocks * p->groups;
    const unsigned grid = static_cast<unsigned>(ceil_div(tasks, PAIRS_WAVES));
    CallTimer tm;
    SAFE_HIP_CHECK_AS(fn, tm.start(s));
    if (p->axis == 0)
        hipLaunchKernelGGL(k_pairs_rows<true>, dim3(grid), dim3(PAIRS_THREADS), 0, s, selector_dev, values, p->m, p->chunks, tasks, p->mode,
                           p->threshold, static_cast<int32_t *>(nullptr), p->offs, d_indices, d_data, d_flag);
    else
        hipLaunchKernelGGL(k_pairs_cols<true>, dim3(grid), dim3(PAIRS_THREADS), 0, s, selector_dev, values, p->n, p->m, p->groups,
                           p->blocks, p->mode, p->threshold, p->table, p->offs, d_indices, d_data, d_flag);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, tm.stop(s));
    int flag = 0;
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    SAFE_HIP_CHECK_AS(fn, tm.finish(ctx, p->axis == 0 ? "k_pairs_rows<emit>" : "k_pairs_cols<emit>", 1, kernel_ms));
    if (flag) {                                               // (nothing has been copied out)
        safe_set_error("safe_pairs_read: selection changed between create and read");
        return SAFE_E_VALUE;
    }
    SAFE_TRY(safe_memcpy_d2h(ctx, indptr_host, p->indptr, static_cast<size_t>(dim + 1) * sizeof(int32_t)));
    SAFE_TRY(safe_memcpy_d2h(ctx, indices_host, d_indices, static_cast<size_t>(p->nnz) * sizeof(int32_t)));
    if (values_dev) SAFE_TRY(safe_memcpy_d2h(ctx, data_host, d_data, static_cast<size_t>(p->nnz) * sizeof(double)));
    return SAFE_OK;
}

int safe_pairs_destroy(safe_pairs *pairs) {
    if (!pairs) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(pairs->ctx->device));
    SAFE_HIP_CHECK(safe_stream_sync(pairs->ctx->stream));
    pairs_free(pairs);
    return SAFE_OK;
}

}  // extern "C"
