// attribute_transform = 'rank': the midrank of every value among the non-NaN values of its column, on gfx950.
//
// safe_attr_rank makes, from any attribute handle, a new handle that owns R f64 [n, m] in Fortran order:
//   R[i, j] = NaN where the source is NaN, else scipy.stats.rankdata(col_j, method='average', nan_policy='omit') -- bit for bit.
// The sum of midranks over a neighborhood is the Wilcoxon / Mann-Whitney statistic, so the analytic test on R is the tie-corrected
// rank-sum test and the randomization test on R its permutation form; both run unchanged on the new handle.
//
// Exact by construction: a value is turned into a 64-bit key whose unsigned order is the IEEE order of the value widened to f64
// (-0.0 == +0.0, NaN = the all-ones key, above +inf), every comparison after that is an integer one, and
//   less = #keys of the column <  the cell's key        leq = #keys of the column <= the cell's key
//   R    = (less + leq + 1) * 0.5                        (the mean of the ranks less + 1 .. leq; an integer below 2 n + 2 halved)
// A non-NaN key is below the all-ones key, so NaN cells and the padding of a sorted chunk are never counted.
//
//   k_rank_keys  source (f32 / f64, either element order) -> keys u64, column-major, written where R will be; a C-order source
//                goes through a 64 x 64 LDS tile so that both the read and the write run along a contiguous axis
//   k_rank_sort  one workgroup per (column, chunk of SAFE_RANK_CHUNK rows): the chunk's keys sorted in LDS by a bitonic network
//                (keys only), padded with all-ones keys, written to scratch [m][chunks][SAFE_RANK_CHUNK]
//   k_rank_emit  one workgroup per (column, chunk of cells): the cells' keys wait in registers (16 per thread) while every sorted
//                chunk of the column passes through LDS; two binary searches per cell and chunk, their results added; the
//                rank replaces the key in place.  No merge pass: the counts of the chunks add up.
//
// SAFE_RANK_CHUNK = 4096 keys = 32 KiB of LDS: five workgroups (20 waves) share a CU's 160 KiB, against one at 16384 keys; the
// network has 78 steps instead of 105 and the emit kernel's searches 13 probes instead of 15, at twice .. four times as many
// chunks per column to search.
//
// LDS banks in the compare-exchange steps (an 8-byte access is served per 32-lane half, 64 banks of 4 bytes): a half's 32 lanes
// take the keys with bit log2(stride) clear -- or set -- of a 64-key span, so for strides <= 16 keys p and p + 32 of the span meet
// on one bank pair (2-way conflict in 50 of the 78 steps).  The keys are therefore kept at position p ^ (bit 5 of p ? 31 : 0): the
// upper 32 keys of a span land on the bank pairs the lower 32 leave free, for every stride <= 16 at once, and strides >= 32 (32
// consecutive keys per half) stay a permutation of one bank row.
#include "common.h"

namespace {

constexpr int RANK_T = SAFE_RANK_CHUNK;
constexpr int RANK_PER = RANK_T / 256;                // cells of an emit thread
constexpr uint64_t RANK_NAN_KEY = ~0ull;
static_assert((RANK_T & (RANK_T - 1)) == 0 && RANK_T >= 512 && RANK_T * 8 <= 64 * 1024, "chunk: a power of two that fits static LDS");

__device__ __forceinline__ uint64_t rank_key(double v) {
    if (v != v) return RANK_NAN_KEY;
    if (v == 0.0) return 0x8000000000000000ull;         // -0.0 ties with +0.0
    const uint64_t b = static_cast<uint64_t>(__double_as_longlong(v));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ int rank_slot(int p) { return p ^ (-((p >> 5) & 1) & 31); }

// rows contiguous (Fortran order, one column, or one row): the key of element e goes to position e
template <typename T>
__global__ __launch_bounds__(256) void k_rank_keys(const T *__restrict__ src, int64_t count, uint64_t *__restrict__ keys) {
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < count; e += static_cast<int64_t>(gridDim.x) * 256)
        keys[e] = rank_key(static_cast<double>(src[e]));
}

// columns contiguous (C order): 64 x 64 tiles turned around through LDS (the layout of k_reindex_rows)
template <typename T>
__global__ __launch_bounds__(256) void k_rank_keys_tile(const T *__restrict__ src, int64_t n, int64_t m, int64_t tiles_m,
                                                        uint64_t *__restrict__ keys) {
    __shared__ uint64_t tile[64][65];
    const int64_t i0 = static_cast<int64_t>(blockIdx.x / tiles_m) * 64, j0 = static_cast<int64_t>(blockIdx.x % tiles_m) * 64;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int t = threadIdx.x + 256 * k;
        const int r = t >> 6, c = t & 63;
        const int64_t i = i0 + r, j = j0 + c;
        if (i < n && j < m) tile[r][c] = rank_key(static_cast<double>(src[i * m + j]));
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int t = threadIdx.x + 256 * k;
        const int r = t & 63, c = t >> 6;
        const int64_t i = i0 + r, j = j0 + c;
        if (i < n && j < m) keys[j * n + i] = tile[r][c];
    }
}

__global__ __launch_bounds__(256) void k_rank_sort(const uint64_t *__restrict__ keys, int64_t n, int64_t chunks,
                                                   uint64_t *__restrict__ sorted) {
    __shared__ uint64_t s[RANK_T];
    const int64_t j = blockIdx.x / chunks, r0 = static_cast<int64_t>(blockIdx.x % chunks) * RANK_T;
    const uint64_t *col = keys + j * n;
    for (int p = threadIdx.x; p < RANK_T; p += 256) s[rank_slot(p)] = r0 + p < n ? col[r0 + p] : RANK_NAN_KEY;
    __syncthreads();
    for (int k = 2; k <= RANK_T; k <<= 1) {
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int t = threadIdx.x; t < RANK_T / 2; t += 256) {
                const int lo = ((t & ~(d - 1)) << 1) | (t & (d - 1)), hi = lo | d;
                const bool ascending = (lo & k) == 0;       // (always, in the last stage)
                const uint64_t a = s[rank_slot(lo)], b = s[rank_slot(hi)];
                if ((a > b) == ascending) {
                    s[rank_slot(lo)] = b;
                    s[rank_slot(hi)] = a;
                }
            }
            __syncthreads();
        }
    }
    uint64_t *dst = sorted + static_cast<int64_t>(blockIdx.x) * RANK_T;
    for (int p = threadIdx.x; p < RANK_T; p += 256) dst[p] = s[rank_slot(p)];
}

// #keys of the sorted chunk s below key (STRICT) or not above it
template <bool STRICT>
__device__ __forceinline__ unsigned int rank_bound(const uint64_t *s, uint64_t key) {
    int pos = 0;
#pragma unroll
    for (int step = RANK_T / 2; step > 0; step >>= 1) {
        const uint64_t probe = s[pos + step - 1];
        if (STRICT ? probe < key : probe <= key) pos += step;
    }
    const uint64_t last = s[pos];                       // pos <= RANK_T - 1
    return static_cast<unsigned int>(pos) + ((STRICT ? last < key : last <= key) ? 1u : 0u);
}

__global__ __launch_bounds__(256) void k_rank_emit(uint64_t *__restrict__ cells, int64_t n, int64_t chunks,
                                                   const uint64_t *__restrict__ sorted) {
    __shared__ uint64_t s[RANK_T];
    const int64_t j = blockIdx.x / chunks, r0 = static_cast<int64_t>(blockIdx.x % chunks) * RANK_T;
    uint64_t *col = cells + j * n;
    uint64_t key[RANK_PER];
    unsigned int both[RANK_PER];                        // less + leq
#pragma unroll
    for (int u = 0; u < RANK_PER; ++u) {
        const int64_t r = r0 + u * 256 + threadIdx.x;
        key[u] = r < n ? col[r] : RANK_NAN_KEY;
        both[u] = 0;
    }
    const uint64_t *src = sorted + j * chunks * RANK_T;
    for (int64_t c = 0; c < chunks; ++c, src += RANK_T) {
        __syncthreads();                                // the searches of the chunk before have ended
        for (int p = threadIdx.x; p < RANK_T; p += 256) s[p] = src[p];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RANK_PER; ++u)
            if (key[u] != RANK_NAN_KEY) both[u] += rank_bound<true>(s, key[u]) + rank_bound<false>(s, key[u]);
    }
#pragma unroll
    for (int u = 0; u < RANK_PER; ++u) {
        const int64_t r = r0 + u * 256 + threadIdx.x;
        if (r >= n) continue;
        const double rank = key[u] == RANK_NAN_KEY ? __builtin_nan("") : static_cast<double>(both[u] + 1u) * 0.5;
        col[r] = static_cast<uint64_t>(__double_as_longlong(rank));
    }
}

}  // namespace

extern "C" {

int safe_attr_rank(safe_attr *src, safe_attr **out) {
    const char *who = "safe_attr_rank";
    SAFE_REQUIRE(src && out, "%s: NULL argument", who);
    *out = nullptr;
    safe_ctx *ctx = src->ctx;
    const int64_t n = src->n, m = src->m, chunks = ceil_div(n, RANK_T);
    SAFE_REQUIRE(n >= 1 && m >= 1, "%s: empty matrix (%lld x %lld)", who, (long long)n, (long long)m);
    SAFE_REQUIRE(n < (1ll << 30), "%s: %lld rows, must be below 2^30 (32-bit counts of less + leq)", who, (long long)n);
    const int64_t tiles_m = ceil_div(m, 64), tiles = ceil_div(n, 64) * tiles_m;
    SAFE_REQUIRE(m * chunks < (1ll << 31) && tiles < (1ll << 31), "%s: %lld x %lld is more than one launch covers", who, (long long)n,
                 (long long)m);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t count = n * m;
    CallBufs b;
    uint64_t *cells = nullptr, *sorted = nullptr;        // cells: keys, then R
    SAFE_TRY(b.alloc(&cells, static_cast<size_t>(count)));
    SAFE_TRY(b.alloc(&sorted, static_cast<size_t>(m * chunks) * RANK_T));
    hipEvent_t *ev = nullptr;
    SAFE_TRY(ctx_events(ctx, true, 4, &ev));

    const bool f32 = src->dtype == SAFE_DTYPE_F32;
    // element e of the source is element e of a Fortran-order [n, m]: Fortran order itself, one column, one row
    const bool linear = src->row_stride == 1 || n == 1;
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ev[0], s));
    if (linear) {
        const dim3 grid(static_cast<unsigned int>(std::min<int64_t>(ceil_div(count, 256), 1 << 20)));
        if (f32) hipLaunchKernelGGL(k_rank_keys<float>, grid, dim3(256), 0, s, static_cast<const float *>(src->raw), count, cells);
        else hipLaunchKernelGGL(k_rank_keys<double>, grid, dim3(256), 0, s, static_cast<const double *>(src->raw), count, cells);
    } else {
        const dim3 grid(static_cast<unsigned int>(tiles));
        if (f32) hipLaunchKernelGGL(k_rank_keys_tile<float>, grid, dim3(256), 0, s, static_cast<const float *>(src->raw), n, m, tiles_m, cells);
        else hipLaunchKernelGGL(k_rank_keys_tile<double>, grid, dim3(256), 0, s, static_cast<const double *>(src->raw), n, m, tiles_m, cells);
    }
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ev[1], s));
    const dim3 grid(static_cast<unsigned int>(m * chunks));
    hipLaunchKernelGGL(k_rank_sort, grid, dim3(256), 0, s, cells, n, chunks, sorted);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(k_rank_emit, grid, dim3(256), 0, s, cells, n, chunks, sorted);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ev[3], s));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));
    double total = 0.0;
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        ctx->rank_ms[k] = ms;
        total += ms;
    }
    ctx->last_kernel.name = "k_rank_keys+k_rank_sort+k_rank_emit";
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = total;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = true;

    safe_attr *made = nullptr;
    SAFE_TRY(attr_new(ctx, SAFE_DTYPE_F64, n, m, 1, n, &made));
    std::unique_ptr<safe_attr> a(made);                   // (owns nothing on the device yet)
    SAFE_TRY(attr_inherit_flags(made, src));
    a->raw = b.release(cells);
    a->owns_raw = true;
    *out = a.release();
    return SAFE_OK;
}

int safe_last_rank_stats(safe_ctx *ctx, double *keys_ms, double *sort_ms, double *emit_ms) {
    SAFE_REQUIRE(ctx != nullptr, "safe_last_rank_stats: ctx is NULL");
    if (keys_ms) *keys_ms = ctx->rank_ms[0];
    if (sort_ms) *sort_ms = ctx->rank_ms[1];
    if (emit_ms) *emit_ms = ctx->rank_ms[2];
    return SAFE_OK;
}

}  // extern "C"
