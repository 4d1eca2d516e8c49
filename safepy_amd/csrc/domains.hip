// The two data-parallel pieces of the consumers of nes_binary:
//
//  * define_top_attributes (safepy/safe.py:631-656): for every candidate attribute, the connected
//    components of the subgraph induced by its enriched nodes (nx.subgraph + nx.connected_components,
//    one Python call per attribute in the reference).  Here: all attributes at once, min-label
//    hooking + pointer jumping over the edge list (Shiloach-Vishkin style); the final label of a
//    node is the smallest node id of its component.
//  * define_domains (safepy/safe.py:672-673): the condensed Jaccard distance vector between the
//    binarised enrichment profiles of the top attributes -- scipy's pdist(m, 'jaccard') inside
//    linkage(): d = #(x != y and (x != 0 or y != 0)) / #(x != 0 or y != 0), 0 when the denominator
//    is 0 -- from bit-packed columns with popcounts; the linkage itself stays SciPy's.
//
// Both exist in two forms.  The host forms (safe_enriched_components, safe_jaccard_condensed) take a dense host copy of the
// chosen columns.  The device forms (safe_enriched_components_dev, safe_profile_distances) read the chosen columns in place
// from the row-major [n, m] matrix compute_pvalues left on the device, so the matrix is never copied:
//  * k_cc_init_cols: a 64 x 64 tile per workgroup, read with the lanes along the column list (one row's chosen columns: one
//    or a few cache lines per wave), transposed through LDS and written with the lanes along the nodes (parent is [n_cols][n]);
//    the hook and compress kernels are the host form's.
//  * k_profile_pack: one wave per (64 rows, 64 chosen columns); lane a walks the 64 rows of its column and builds the word
//    itself -- every load of the wave is one row's 64 chosen columns -- and writes bits[word][column], so the pair kernel's
//    lanes (consecutive second profiles j) read consecutive words.  No transposed [m_top, n] copy exists at any point.
//  * k_profile_pairs: ntt, ntf, nft from popcounts (nff = n - the rest: the padding bits of the last word are zero in every
//    profile and count for none of the three), then metric_distance, one or two f64 operations on exact integers restating
//    SciPy 1.15's pdist for the boolean metrics (tests/domain_metrics_ref.py has the table, held to SciPy on the CPU).
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

__global__ __launch_bounds__(256) void k_cc_init(const double *__restrict__ member, int64_t n, int64_t n_cols,
                                                 int32_t *__restrict__ parent) {
    // member: [n][n_cols] row-major (nes_binary[:, cols]); parent: [n_cols][n]
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= n * n_cols) return;
    const int64_t a = idx / n, v = idx % n;
    parent[idx] = member[v * n_cols + a] > 0.0 ? static_cast<int32_t>(v) : -1;
}

__global__ __launch_bounds__(256) void k_cc_hook(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, int64_t n_edges,
                                                 int64_t n, int32_t *__restrict__ parent, int *__restrict__ changed) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int32_t *p = parent + static_cast<int64_t>(blockIdx.y) * n;
    const int32_t pu = p[eu[e]], pv = p[ev[e]];
    if (pu < 0 || pv < 0 || pu == pv) return;
    // hang the larger root under the smaller label (labels only ever decrease)
    if (pu < pv) atomicMin(&p[pv], pu);
    else atomicMin(&p[pu], pv);
    *changed = 1;
}

__global__ __launch_bounds__(256) void k_cc_compress(int64_t n, int64_t n_cols, int32_t *__restrict__ parent) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= n * n_cols) return;
    int32_t *p = parent + (idx / n) * n;
    int32_t l = parent[idx];
    if (l < 0) return;
    while (p[l] != l) l = p[l];                                          // roots are fixed points
    parent[idx] = l;
}

// parent[a][v] = v if values[v][cols[a]] > 0 else -1, straight from the row-major [n, m] matrix
__global__ __launch_bounds__(256) void k_cc_init_cols(const double *__restrict__ values, int64_t n, int64_t m,
                                                      const int64_t *__restrict__ cols, int64_t n_cols,
                                                      int32_t *__restrict__ parent) {
    __shared__ int32_t tile[64][65];
    const int64_t v0 = static_cast<int64_t>(blockIdx.x) * 64, a0 = static_cast<int64_t>(blockIdx.y) * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t a = a0 + lane;
    const int64_t col = a < n_cols ? cols[a] : 0;
    for (int r = wave; r < 64; r += 4) {
        const int64_t v = v0 + r;
        tile[r][lane] = (a < n_cols && v < n && values[v * m + col] > 0.0) ? static_cast<int32_t>(v) : -1;
    }
    __syncthreads();
    const int64_t v = v0 + lane;
    for (int c = wave; c < 64; c += 4)
        if (a0 + c < n_cols && v < n) parent[(a0 + c) * n + v] = tile[lane][c];
}

__global__ __launch_bounds__(256) void k_jaccard_pack(const double *__restrict__ x, int64_t m_top, int64_t n, int64_t words,
                                                      unsigned long long *__restrict__ bits) {
    // x: [m_top][n] row-major; one wave per 64 consecutive values of one row
    const int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), a = blockIdx.y;
    if (w >= words) return;
    const int64_t i = w * 64 + (threadIdx.x & 63);
    const bool on = i < n && x[a * n + i] != 0.0;
    const unsigned long long v = __builtin_amdgcn_ballot_w64(on);
    if ((threadIdx.x & 63) == 0) bits[a * words + w] = v;
}

__global__ __launch_bounds__(256) void k_jaccard_pairs(const unsigned long long *__restrict__ bits, int64_t m_top, int64_t words,
                                                       double *__restrict__ out) {
    const int64_t i = blockIdx.y, j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j <= i || j >= m_top) return;
    const unsigned long long *a = bits + i * words, *b = bits + j * words;
    long long neq = 0, any = 0;
    for (int64_t w = 0; w < words; ++w) {
        const unsigned long long x = a[w], y = b[w];
        neq += __popcll(x ^ y);
        any += __popcll(x | y);
    }
    const int64_t k = i * (2 * m_top - i - 1) / 2 + (j - i - 1);       // scipy's condensed index
    out[k] = any == 0 ? 0.0 : static_cast<double>(neq) / static_cast<double>(any);
}

// bits[w][a] = rows 64 w .. 64 w + 63 of column cols[a] of the row-major [n, m] matrix (non-zero = set; rows >= n: 0)
__global__ __launch_bounds__(256) void k_profile_pack(const double *__restrict__ values, int64_t n, int64_t m,
                                                      const int64_t *__restrict__ cols, int64_t m_top, int64_t words,
                                                      unsigned long long *__restrict__ bits) {
    const int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int64_t a = static_cast<int64_t>(blockIdx.y) * 64 + (threadIdx.x & 63);
    if (w >= words || a >= m_top) return;
    const double *p = values + cols[a];
    const int64_t r0 = w * 64;
    const int cnt = static_cast<int>(n - r0 < 64 ? n - r0 : 64);
    unsigned long long word = 0;
#pragma unroll 8
    for (int r = 0; r < cnt; ++r) word |= static_cast<unsigned long long>(p[(r0 + r) * m] != 0.0) << r;
    bits[w * m_top + a] = word;
}

// SciPy 1.15's pdist for 0/1 profiles from the contingency counts (all exact in f64: one rounding, in the division)
__device__ inline double metric_distance(int metric, long long ntt, long long ntf, long long nft, long long n) {
    const double tt = static_cast<double>(ntt), nn = static_cast<double>(n);
    const double ndiff = static_cast<double>(ntf + nft);
    switch (metric) {
    case SAFE_METRIC_JACCARD: {
        const double den = tt + ndiff;
        return den == 0.0 ? 0.0 : ndiff / den;
    }
    case SAFE_METRIC_HAMMING: return ndiff / nn;
    case SAFE_METRIC_DICE: return ndiff / (2.0 * tt + ndiff);                       // 0 / 0 = NaN, as SciPy
    case SAFE_METRIC_ROGERSTANIMOTO:
    case SAFE_METRIC_SOKALMICHENER: return (2.0 * ndiff) / (nn + ndiff);
    case SAFE_METRIC_RUSSELLRAO: return (nn - tt) / nn;
    case SAFE_METRIC_SOKALSNEATH: return (2.0 * ndiff) / (2.0 * ndiff + tt);        // 0 / 0 = NaN, as SciPy
    default: {                                                                      // SAFE_METRIC_YULE
        const double half_r = static_cast<double>(ntf) * static_cast<double>(nft);
        const double nff = static_cast<double>(n - ntt - ntf - nft);
        return half_r == 0.0 ? 0.0 : (2.0 * half_r) / (tt * nff + half_r);
    }
    }
}

__global__ __launch_bounds__(256) void k_profile_pairs(const unsigned long long *__restrict__ bits, int64_t m_top, int64_t words,
                                                       int64_t n, int metric, double *__restrict__ out) {
    const int64_t i = blockIdx.y, j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j <= i || j >= m_top) return;
    long long ntt = 0, ntf = 0, nft = 0;
    for (int64_t w = 0; w < words; ++w) {
        const unsigned long long x = bits[w * m_top + i], y = bits[w * m_top + j];
        ntt += __popcll(x & y);
        ntf += __popcll(x & ~y);
        nft += __popcll(~x & y);
    }
    const int64_t k = i * (2 * m_top - i - 1) / 2 + (j - i - 1);       // scipy's condensed index
    out[k] = metric_distance(metric, ntt, ntf, nft, n);
}

// Device buffers and timing events of one call, released on every return path.
struct DomBufs {
    std::vector<void *> p;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~DomBufs() {
        for (void *q : p) (void)hipFree(q);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <typename T>
    int alloc(T **q, size_t count) {
        const int rc = dev_alloc(q, count);
        if (rc == SAFE_OK) p.push_back(*q);
        return rc;
    }
    hipError_t start(hipStream_t s) {
        for (hipEvent_t &e : ev) {
            const hipError_t err = hipEventCreateWithFlags(&e, safe_event_flags(hipEventDefault));
            if (err != hipSuccess) return err;
        }
        return hipEventRecord(ev[0], s);
    }
    hipError_t stop(hipStream_t s) { return hipEventRecord(ev[1], s); }
    // after the stream has been synchronised: the kernels' time, also recorded as the context's last kernel
    hipError_t finish(safe_ctx *ctx, const char *name, int64_t launches, double *kernel_ms) {
        float f = 0;
        const hipError_t err = hipEventElapsedTime(&f, ev[0], ev[1]);
        if (err != hipSuccess) return err;
        ctx->last_kernel.name = name;
        ctx->last_kernel.total_ms = f;
        ctx->last_kernel.launches = launches;
        ctx->last_kernel.busy_ms = f;
        ctx->last_kernel.summed = true;
        if (kernel_ms) *kernel_ms = f;
        return hipSuccess;
    }
};

// Hook + compress rounds over parent [n_cols][n] until no edge joins two labels (both forms of safe_enriched_components).
// Synchronises the stream once per round (the changed flag).
hipError_t cc_rounds(hipStream_t s, const int32_t *d_eu, const int32_t *d_ev, int64_t n_edges, int64_t n, int64_t n_cols,
                     int32_t *d_parent, int *d_changed, int64_t *launches) {
    const int64_t total = n * n_cols;
    hipError_t e = hipSuccess;
    for (int round = 0; n_edges > 0 && round < 64; ++round) {             // O(log n) rounds in practice
        int changed = 0;
        e = hipMemsetAsync(d_changed, 0, sizeof(int), s);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_cc_hook, dim3(ceil_div(n_edges, 256), n_cols), dim3(256), 0, s, d_eu, d_ev, n_edges, n, d_parent, d_changed);
        hipLaunchKernelGGL(k_cc_compress, dim3(ceil_div(total, 256)), dim3(256), 0, s, n, n_cols, d_parent);
        if (launches) *launches += 2;
        e = hipMemcpyAsync(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = safe_stream_sync(s);
        if (e != hipSuccess || !changed) break;
    }
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}

}  // namespace

extern "C" {

int safe_enriched_components(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v,
                             const double *member_host, int64_t n_cols, int32_t *labels_host) {
    SAFE_REQUIRE(ctx && labels_host && (n_cols == 0 || member_host), "safe_enriched_components: NULL argument");
    SAFE_REQUIRE(n >= 1 && n < (1ll << 31) && n_edges >= 0 && n_cols >= 0, "safe_enriched_components: bad sizes");
    SAFE_REQUIRE(n_edges == 0 || (edge_u && edge_v), "safe_enriched_components: NULL edge list");
    if (n_cols == 0) return SAFE_OK;
    for (int64_t e = 0; e < n_edges; ++e)
        SAFE_REQUIRE(edge_u[e] >= 0 && edge_u[e] < n && edge_v[e] >= 0 && edge_v[e] < n, "safe_enriched_components: edge %lld out of range",
                     (long long)e);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    double *d_member = nullptr;
    int32_t *d_parent = nullptr, *d_eu = nullptr, *d_ev = nullptr;
    int *d_changed = nullptr;
    int rc = dev_alloc(&d_member, static_cast<size_t>(n) * n_cols);
    if (rc == SAFE_OK) rc = dev_alloc(&d_parent, static_cast<size_t>(n) * n_cols);
    if (rc == SAFE_OK) rc = dev_alloc(&d_eu, std::max<int64_t>(n_edges, 1));
    if (rc == SAFE_OK) rc = dev_alloc(&d_ev, std::max<int64_t>(n_edges, 1));
    if (rc == SAFE_OK) rc = dev_alloc(&d_changed, 1);
    hipError_t e = hipSuccess;
    if (rc == SAFE_OK) {
        e = hipMemcpyAsync(d_member, member_host, static_cast<size_t>(n) * n_cols * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n_edges)
            e = hipMemcpyAsync(d_eu, edge_u, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n_edges)
            e = hipMemcpyAsync(d_ev, edge_v, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    }
    if (rc == SAFE_OK && e == hipSuccess) {
        const int64_t total = n * n_cols;
        hipLaunchKernelGGL(k_cc_init, dim3(ceil_div(total, 256)), dim3(256), 0, ctx->stream, d_member, n, n_cols, d_parent);
        e = cc_rounds(ctx->stream, d_eu, d_ev, n_edges, n, n_cols, d_parent, d_changed, nullptr);
        if (e == hipSuccess)
            e = hipMemcpyAsync(labels_host, d_parent, static_cast<size_t>(total) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = safe_stream_sync(ctx->stream);
    }
    if (rc == SAFE_OK && e != hipSuccess) {
        safe_set_error("safe_enriched_components: %s", hipGetErrorString(e));
        rc = SAFE_E_HIP;
    }
    (void)hipFree(d_member);
    (void)hipFree(d_parent);
    (void)hipFree(d_eu);
    (void)hipFree(d_ev);
    (void)hipFree(d_changed);
    return rc;
}

int safe_jaccard_condensed(safe_ctx *ctx, int64_t m_top, int64_t n, const double *x_host, double *out_host) {
    SAFE_REQUIRE(ctx && (m_top < 2 || (x_host && out_host)), "safe_jaccard_condensed: NULL argument");
    SAFE_REQUIRE(m_top >= 0 && n >= 1, "safe_jaccard_condensed: bad sizes");
    if (m_top < 2) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t words = ceil_div(n, 64), pairs = m_top * (m_top - 1) / 2;
    double *d_x = nullptr, *d_out = nullptr;
    unsigned long long *d_bits = nullptr;
    int rc = dev_alloc(&d_x, static_cast<size_t>(m_top) * n);
    if (rc == SAFE_OK) rc = dev_alloc(&d_bits, static_cast<size_t>(m_top) * words);
    if (rc == SAFE_OK) rc = dev_alloc(&d_out, pairs);
    hipError_t e = hipSuccess;
    if (rc == SAFE_OK) {
        e = hipMemcpyAsync(d_x, x_host, static_cast<size_t>(m_top) * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_jaccard_pack, dim3(ceil_div(words, 4), m_top), dim3(256), 0, ctx->stream, d_x, m_top, n, words, d_bits);
            hipLaunchKernelGGL(k_jaccard_pairs, dim3(ceil_div(m_top, 256), m_top), dim3(256), 0, ctx->stream, d_bits, m_top, words, d_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_out, pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = safe_stream_sync(ctx->stream);
        if (e != hipSuccess) {
            safe_set_error("safe_jaccard_condensed: %s", hipGetErrorString(e));
            rc = SAFE_E_HIP;
        }
    }
    (void)hipFree(d_x);
    (void)hipFree(d_bits);
    (void)hipFree(d_out);
    return rc;
}

int safe_enriched_components_dev(safe_ctx *ctx, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v, const double *values_dev,
                                 int64_t n, int64_t m, const int64_t *cols_host, int64_t n_cols, int32_t *labels_host,
                                 double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 1 && n < (1ll << 31) && m >= 0 && n_edges >= 0 && n_cols >= 0, "safe_enriched_components_dev: bad argument");
    if (kernel_ms) *kernel_ms = 0;
    if (n_cols == 0) return SAFE_OK;
    SAFE_REQUIRE(values_dev && cols_host && labels_host, "safe_enriched_components_dev: NULL argument");
    SAFE_REQUIRE(n_edges == 0 || (edge_u && edge_v), "safe_enriched_components_dev: NULL edge list");
    for (int64_t c = 0; c < n_cols; ++c)
        SAFE_REQUIRE(cols_host[c] >= 0 && cols_host[c] < m, "safe_enriched_components_dev: column %lld out of [0, %lld)",
                     (long long)cols_host[c], (long long)m);
    for (int64_t e = 0; e < n_edges; ++e)
        SAFE_REQUIRE(edge_u[e] >= 0 && edge_u[e] < n && edge_v[e] >= 0 && edge_v[e] < n,
                     "safe_enriched_components_dev: edge %lld out of range", (long long)e);
    SAFE_REQUIRE(n_cols < 65536 && ceil_div(n * n_cols, 256) < (1ll << 31), "safe_enriched_components_dev: too many labels for one launch");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    DomBufs b;
    int64_t *d_cols = nullptr;
    int32_t *d_parent = nullptr, *d_eu = nullptr, *d_ev = nullptr;
    int *d_changed = nullptr;
    SAFE_TRY(b.alloc(&d_cols, static_cast<size_t>(n_cols)));
    SAFE_TRY(b.alloc(&d_parent, static_cast<size_t>(n) * n_cols));
    SAFE_TRY(b.alloc(&d_eu, static_cast<size_t>(std::max<int64_t>(n_edges, 1))));
    SAFE_TRY(b.alloc(&d_ev, static_cast<size_t>(std::max<int64_t>(n_edges, 1))));
    SAFE_TRY(b.alloc(&d_changed, 1));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(d_cols, cols_host, n_cols * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (n_edges) {
        SAFE_HIP_CHECK(hipMemcpyAsync(d_eu, edge_u, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK(hipMemcpyAsync(d_ev, edge_v, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    SAFE_HIP_CHECK(b.start(s));
    int64_t launches = 1;
    hipLaunchKernelGGL(k_cc_init_cols, dim3(static_cast<unsigned>(ceil_div(n, 64)), static_cast<unsigned>(ceil_div(n_cols, 64))), dim3(256),
                       0, s, values_dev, n, m, d_cols, n_cols, d_parent);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(cc_rounds(s, d_eu, d_ev, n_edges, n, n_cols, d_parent, d_changed, &launches));
    SAFE_HIP_CHECK(b.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(labels_host, d_parent, static_cast<size_t>(n) * n_cols * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(b.finish(ctx, "k_cc_init_cols+k_cc_hook+k_cc_compress", launches, kernel_ms));
    return SAFE_OK;
}

int safe_profile_distances(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top,
                           int metric, double *out_host, double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 1 && m >= 0 && m_top >= 0, "safe_profile_distances: bad argument");
    SAFE_REQUIRE(metric >= SAFE_METRIC_JACCARD && metric <= SAFE_METRIC_YULE, "safe_profile_distances: unknown metric id %d", metric);
    if (kernel_ms) *kernel_ms = 0;
    SAFE_REQUIRE(m_top == 0 || cols_host, "safe_profile_distances: NULL argument");
    for (int64_t c = 0; c < m_top; ++c)
        SAFE_REQUIRE(cols_host[c] >= 0 && cols_host[c] < m, "safe_profile_distances: column %lld out of [0, %lld)",
                     (long long)cols_host[c], (long long)m);
    if (m_top < 2) return SAFE_OK;
    SAFE_REQUIRE(values_dev && out_host, "safe_profile_distances: NULL argument");
    const int64_t words = ceil_div(n, 64), pairs = m_top * (m_top - 1) / 2;
    SAFE_REQUIRE(m_top < 65536 && ceil_div(words, 4) < (1ll << 31), "safe_profile_distances: too many profiles or rows for one launch");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    DomBufs b;
    int64_t *d_cols = nullptr;
    unsigned long long *d_bits = nullptr;
    double *d_out = nullptr;
    SAFE_TRY(b.alloc(&d_cols, static_cast<size_t>(m_top)));
    SAFE_TRY(b.alloc(&d_bits, static_cast<size_t>(m_top) * words));
    SAFE_TRY(b.alloc(&d_out, static_cast<size_t>(pairs)));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(d_cols, cols_host, m_top * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(b.start(s));
    hipLaunchKernelGGL(k_profile_pack, dim3(static_cast<unsigned>(ceil_div(words, 4)), static_cast<unsigned>(ceil_div(m_top, 64))), dim3(256),
                       0, s, values_dev, n, m, d_cols, m_top, words, d_bits);
    SAFE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_profile_pairs, dim3(static_cast<unsigned>(ceil_div(m_top, 256)), static_cast<unsigned>(m_top)), dim3(256), 0, s,
                       d_bits, m_top, words, n, metric, d_out);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(b.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(b.finish(ctx, "k_profile_pack+k_profile_pairs", 2, kernel_ms));
    return SAFE_OK;
}

}  // extern "C"
