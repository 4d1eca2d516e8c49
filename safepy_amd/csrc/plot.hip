// The data-parallel parts of the reference's plot methods (safepy/safe.py:786-1003):
//   k_kde_grid         domain contours (plot_composite_network_contours, safe.py:822-829): SciPy's gaussian_kde of each
//                      domain's nodes evaluated on its 100 x 100 grid, every domain in one launch
//   k_domain_counts    composite colours (plot_composite_network, safe.py:883-886): nes_binary [N, M] summed over each
//                      domain's attribute columns (the reference's groupby(level='domain', axis=1).sum()); its second
//                      form is the node-to-domain table of define_domains (below)
//   k_gather_columns   a few columns of a device-resident [N, M] matrix (plot_sample_attributes' nes / nes_binary columns)
//
// k_kde_grid restates SciPy 1.15's gaussian_kernel_estimate (scipy/stats/_stats.pyx) operation for operation, for d = 2
// and one weight column, on points and grid already whitened by the host (solve_triangular with SciPy's cho_cov):
//   for each grid point j, for points i in ascending order:
//     a = 0; r = p[i,0] - x[j,0]; a += r*r; r = p[i,1] - x[j,1]; a += r*r
//     e = exp(-a / 2) * norm
//     z[j] += w[i] * e
// in f64 with the device library's exp (within an ulp of the host's, not always equal to it); -ffp-contract=off keeps every
// product and sum rounded on its own.  One thread owns one grid point; a workgroup's 256 threads share tiles of 256 points
// staged in LDS.  A set whose grid alone cannot fill the device (one 10^4-point grid is 157 waves for 1024 SIMDs) is cut
// into contiguous point chunks: each chunk's sum is written to its own row of a partial buffer and a second kernel adds the
// rows in chunk order.  A set of one chunk gives exactly the serial sum (0 + s = s).  No atomics: every run gives the same z.
//
// k_domain_counts: one workgroup per row, one f64 LDS bin per domain (LDS atomics), bins written out once the row is read.
// Only non-zero, non-NaN values are added (pandas' sum skips NaN).  For whole-number inputs -- nes_binary is 0/1 -- every
// partial sum is exact, so the order of the adds does not matter and the counts are the same on every run; other inputs
// are added in an unspecified order.
//
// k_domain_counts<true> (safe_node_domains) is the same pass with the row of nes read beside the row of nes_binary: it also
// keeps each domain's largest non-NaN NES in LDS and ends with the node's primary domain and primary NES (define_domains,
// safepy/safe.py:693-705), so the node table needs one pass over the two matrices and neither leaves the device.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int KDE_THREADS = 256;                       // grid points per workgroup; also points per LDS tile
constexpr int64_t KDE_TARGET_BLOCKS = 2048;            // split sets into chunks while the launch has fewer workgroups than this
constexpr int64_t KDE_MIN_CHUNK = 1024;                // points; a chunk is never cut shorter
constexpr int DC_THREADS = 256;
constexpr int64_t DC_MAX_DOMAINS = 4096;               // f64 LDS bins: at most 32 KB per workgroup
constexpr int64_t ND_MAX_DOMAINS = 2048;               // safe_node_domains: a sum bin and a maximum key per domain, 32 KB
constexpr int GC_THREADS = 256;

// One workgroup = one (work item, tile of 256 grid points).  Work item t covers points [p0[t], p1[t]) of set set[t] and
// writes its sums to row t of part [items, g].
__global__ __launch_bounds__(KDE_THREADS) void k_kde_grid(const double *__restrict__ pts, const double *__restrict__ w,
                                                         const double *__restrict__ norm, const double *__restrict__ xi,
                                                         const int64_t *__restrict__ item_set, const int64_t *__restrict__ item_p0,
                                                         const int64_t *__restrict__ item_p1, int64_t g, int64_t tiles,
                                                         double *__restrict__ part) {
    __shared__ double sx[KDE_THREADS], sy[KDE_THREADS], sw[KDE_THREADS];
    const int64_t item = blockIdx.x / tiles;
    const int64_t j = (blockIdx.x % tiles) * KDE_THREADS + threadIdx.x;
    const int64_t d = item_set[item], p0 = item_p0[item], p1 = item_p1[item];
    const bool live = j < g;
    double x0 = 0, x1 = 0;
    if (live) {
        x0 = xi[(d * g + j) * 2];
        x1 = xi[(d * g + j) * 2 + 1];
    }
    const double nm = norm[d];
    double z = 0;
    for (int64_t base = p0; base < p1; base += KDE_THREADS) {
        const int cnt = static_cast<int>(p1 - base < KDE_THREADS ? p1 - base : KDE_THREADS);
        __syncthreads();
        if (threadIdx.x < cnt) {
            const int64_t i = base + threadIdx.x;
            sx[threadIdx.x] = pts[2 * i];
            sy[threadIdx.x] = pts[2 * i + 1];
            sw[threadIdx.x] = w[i];
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            double a = 0;
            double r = sx[t] - x0;
            a += r * r;
            r = sy[t] - x1;
            a += r * r;
            const double e = exp(-a / 2.0) * nm;
            z += sw[t] * e;
        }
    }
    if (live) part[item * g + j] = z;
}

// z[d, j] = partial sums of set d's items added in chunk order.
__global__ __launch_bounds__(KDE_THREADS) void k_kde_sum_chunks(const double *__restrict__ part, const int64_t *__restrict__ set_item0,
                                                               int64_t n_sets, int64_t g, double *__restrict__ z) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * KDE_THREADS + threadIdx.x;
    if (t >= n_sets * g) return;
    const int64_t d = t / g, j = t % g;
    double s = 0;
    for (int64_t item = set_item0[d]; item < set_item0[d + 1]; ++item) s += part[item * g + j];
    z[t] = s;
}

// f64 -> u64 key that orders like the value (-inf < ... < -0.0 < +0.0 < ... < +inf); no non-NaN value has key 0
__device__ inline unsigned long long nd_key(double v) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double nd_value(unsigned long long k) {
    return __longlong_as_double(static_cast<long long>((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// One workgroup per row r.  bins[d] = sum of values[r, c] over the columns with domain[c] == d (domain holds bin indices).
// NODE form (safe_node_domains) in the same pass over the row: keys[d] = the largest non-NaN nes[r, c] of bin d as an
// ordered integer key (0 = none seen; LDS integer max), then wave 0 picks the row's primary bin -- the first maximum of the
// bins from first_real on, or bin 0's role "no domain" (zero_bin, -1 when no column has domain id 0) when that maximum is 0
// -- and writes the bin index and the primary NES (NaN: no non-NaN value, or no such bin).
template <bool NODE>
__global__ __launch_bounds__(DC_THREADS) void k_domain_counts(const double *__restrict__ values, const double *__restrict__ nes,
                                                             int64_t m, const int32_t *__restrict__ domain, int64_t n_domains,
                                                             int first_real, int zero_bin, double *__restrict__ counts,
                                                             int32_t *__restrict__ primary, double *__restrict__ primary_nes) {
    extern __shared__ double bins[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(bins + n_domains);      // NODE form only
    const int64_t r = blockIdx.x;
    for (int64_t d = threadIdx.x; d < n_domains; d += DC_THREADS) {
        bins[d] = 0;
        if (NODE) keys[d] = 0;
    }
    __syncthreads();
    const double *row = values + r * m;
    const double *nrow = NODE ? nes + r * m : nullptr;
    for (int64_t c = threadIdx.x; c < m; c += DC_THREADS) {
        const double v = row[c];
        const int32_t d = domain[c];
        if (v != 0 && v == v) atomicAdd(&bins[d], v);
        if (NODE) {
            const double x = nrow[c];
            if (x == x) {
                const unsigned long long k = nd_key(x);
                // the bin only grows: a stale read can cost an atomic that changes nothing, never skip one that would
                if (k > *reinterpret_cast<volatile unsigned long long *>(&keys[d])) atomicMax(&keys[d], k);
            }
        }
    }
    __syncthreads();
    for (int64_t d = threadIdx.x; d < n_domains; d += DC_THREADS) counts[r * n_domains + d] = bins[d];
    if (!NODE || threadIdx.x >= 64) return;
    // first maximum over the real domains: per lane over its strided bins (ascending, strict >), then across the wave
    double best = -1;                                                    // sums of 0/1 values are >= 0
    int best_d = 0x7fffffff;
    for (int d = first_real + static_cast<int>(threadIdx.x); d < n_domains; d += 64)
        if (bins[d] > best) {
            best = bins[d];
            best_d = d;
        }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int od = __shfl_xor(best_d, off, 64);
        if (ob > best || (ob == best && od < best_d)) {
            best = ob;
            best_d = od;
        }
    }
    if (threadIdx.x == 0) {
        const int p = (best_d == 0x7fffffff || best == 0) ? zero_bin : best_d;
        primary[r] = p;
        const unsigned long long k = p >= 0 ? keys[p] : 0;
        primary_nes[r] = k ? nd_value(k) : __longlong_as_double(0x7ff8000000000000ll);
    }
}

__global__ __launch_bounds__(GC_THREADS) void k_gather_columns(const double *__restrict__ values, int64_t n, int64_t m,
                                                              const int64_t *__restrict__ cols, int64_t k, double *__restrict__ out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GC_THREADS + threadIdx.x;
    if (t >= n * k) return;
    const int64_t r = t / k, c = t % k;
    out[t] = values[r * m + cols[c]];
}

}  // namespace

extern "C" {

int safe_kde_grid(safe_ctx *ctx, int64_t n_sets, const int64_t *offsets_host, const double *pts_host, const double *weights_host,
                  const double *norm_host, int64_t g, const double *xi_host, double *z_host, double *kernel_ms) {
    SAFE_REQUIRE(ctx && n_sets >= 0 && g >= 0, "safe_kde_grid: bad argument");
    if (kernel_ms) *kernel_ms = 0;
    if (n_sets == 0 || g == 0) return SAFE_OK;
    SAFE_REQUIRE(offsets_host && norm_host && xi_host && z_host, "safe_kde_grid: NULL argument");
    SAFE_REQUIRE(offsets_host[0] == 0, "safe_kde_grid: offsets[0] must be 0");
    for (int64_t d = 0; d < n_sets; ++d)
        SAFE_REQUIRE(offsets_host[d + 1] >= offsets_host[d], "safe_kde_grid: offsets decrease at set %lld", (long long)d);
    const int64_t total = offsets_host[n_sets];
    SAFE_REQUIRE(total == 0 || (pts_host && weights_host), "safe_kde_grid: NULL points or weights");
    const int64_t tiles = ceil_div(g, KDE_THREADS);

    // work items: one per set, or contiguous chunks of at least KDE_MIN_CHUNK points when the sets' grids are too few
    int64_t chunk = INT64_MAX;
    if (n_sets * tiles < KDE_TARGET_BLOCKS) {
        const int64_t items_wanted = ceil_div(KDE_TARGET_BLOCKS, tiles);
        chunk = std::max(KDE_MIN_CHUNK, ceil_div(total, items_wanted));
    }
    std::vector<int64_t> item_set, item_p0, item_p1, set_item0(n_sets + 1, 0);
    for (int64_t d = 0; d < n_sets; ++d) {
        const int64_t a = offsets_host[d], b = offsets_host[d + 1];
        set_item0[d] = static_cast<int64_t>(item_set.size());
        int64_t p = a;
        do {
            const int64_t e = (b - p > chunk) ? p + chunk : b;
            item_set.push_back(d);
            item_p0.push_back(p);
            item_p1.push_back(e);
            p = e;
        } while (p < b);
    }
    const int64_t items = static_cast<int64_t>(item_set.size());
    set_item0[n_sets] = items;
    SAFE_REQUIRE(items * tiles < (int64_t(1) << 31) && n_sets * g < (int64_t(1) << 31) * KDE_THREADS,
                 "safe_kde_grid: too many sets or grid points for one launch");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));

    CallBufs b;
    double *d_pts = nullptr, *d_w = nullptr, *d_norm = nullptr, *d_xi = nullptr, *d_part = nullptr, *d_z = nullptr;
    int64_t *d_item = nullptr, *d_set_item0 = nullptr;
    SAFE_TRY(b.alloc(&d_pts, static_cast<size_t>(2 * total)));
    SAFE_TRY(b.alloc(&d_w, static_cast<size_t>(total)));
    SAFE_TRY(b.alloc(&d_norm, static_cast<size_t>(n_sets)));
    SAFE_TRY(b.alloc(&d_xi, static_cast<size_t>(2 * n_sets * g)));
    SAFE_TRY(b.alloc(&d_part, static_cast<size_t>(items * g)));
    SAFE_TRY(b.alloc(&d_z, static_cast<size_t>(n_sets * g)));
    SAFE_TRY(b.alloc(&d_item, static_cast<size_t>(3 * items)));
    SAFE_TRY(b.alloc(&d_set_item0, static_cast<size_t>(n_sets + 1)));
    hipStream_t s = ctx->stream;
    if (total) {
        SAFE_HIP_CHECK(hipMemcpyAsync(d_pts, pts_host, 2 * total * sizeof(double), hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK(hipMemcpyAsync(d_w, weights_host, total * sizeof(double), hipMemcpyHostToDevice, s));
    }
    SAFE_HIP_CHECK(hipMemcpyAsync(d_norm, norm_host, n_sets * sizeof(double), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_xi, xi_host, 2 * n_sets * g * sizeof(double), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_item, item_set.data(), items * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_item + items, item_p0.data(), items * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_item + 2 * items, item_p1.data(), items * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_set_item0, set_item0.data(), (n_sets + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    CallTimer tm;
    SAFE_HIP_CHECK(tm.start(s));
    hipLaunchKernelGGL(k_kde_grid, dim3(static_cast<unsigned>(items * tiles)), dim3(KDE_THREADS), 0, s, d_pts, d_w, d_norm, d_xi,
                       d_item, d_item + items, d_item + 2 * items, g, tiles, d_part);
    SAFE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_kde_sum_chunks, dim3(static_cast<unsigned>(ceil_div(n_sets * g, KDE_THREADS))), dim3(KDE_THREADS), 0, s,
                       d_part, d_set_item0, n_sets, g, d_z);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(z_host, d_z, n_sets * g * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    if (kernel_ms) SAFE_HIP_CHECK(tm.ms(kernel_ms));
    return SAFE_OK;
}

int safe_domain_counts(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int32_t *domain_host, int64_t n_domains,
                       double *counts_host, double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 0 && m >= 0 && n_domains >= 1, "safe_domain_counts: bad argument");
    if (n_domains > DC_MAX_DOMAINS) {
        safe_set_error("safe_domain_counts: %lld domains exceed the kernel's limit of %lld (one f64 LDS bin each)",
                       (long long)n_domains, (long long)DC_MAX_DOMAINS);
        return SAFE_E_UNSUPPORTED;
    }
    if (kernel_ms) *kernel_ms = 0;
    if (n == 0) return SAFE_OK;
    SAFE_REQUIRE(counts_host && (m == 0 || (values_dev && domain_host)), "safe_domain_counts: NULL argument");
    for (int64_t c = 0; c < m; ++c)
        if (domain_host[c] < 0 || domain_host[c] >= n_domains) {
            safe_set_error("safe_domain_counts: column %lld: domain %d not in [0, %lld)", (long long)c, domain_host[c],
                           (long long)n_domains);
            return SAFE_E_VALUE;
        }
    SAFE_REQUIRE(n < (int64_t(1) << 31), "safe_domain_counts: too many rows");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    int32_t *d_dom = nullptr;
    double *d_counts = nullptr;
    SAFE_TRY(b.alloc(&d_dom, static_cast<size_t>(m)));
    SAFE_TRY(b.alloc(&d_counts, static_cast<size_t>(n * n_domains)));
    hipStream_t s = ctx->stream;
    if (m) SAFE_HIP_CHECK(hipMemcpyAsync(d_dom, domain_host, m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    CallTimer tm;
    SAFE_HIP_CHECK(tm.start(s));
    hipLaunchKernelGGL(k_domain_counts<false>, dim3(static_cast<unsigned>(n)), dim3(DC_THREADS), n_domains * sizeof(double), s, values_dev,
                       static_cast<const double *>(nullptr), m, d_dom, n_domains, 0, 0, d_counts, static_cast<int32_t *>(nullptr),
                       static_cast<double *>(nullptr));
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(counts_host, d_counts, n * n_domains * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    if (kernel_ms) SAFE_HIP_CHECK(tm.ms(kernel_ms));
    return SAFE_OK;
}

int safe_node_domains(safe_ctx *ctx, const double *nes_binary_dev, const double *nes_dev, int64_t n, int64_t m,
                      const int32_t *domain_host, const int32_t *ids_host, int64_t n_ids, double *sums_host, int32_t *primary_host,
                      double *primary_nes_host, double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 0 && m >= 0 && n_ids >= 1, "safe_node_domains: bad argument");
    if (n_ids > ND_MAX_DOMAINS) {
        safe_set_error("safe_node_domains: %lld domains exceed the kernel's limit of %lld (two 8-byte LDS slots each)", (long long)n_ids,
                       (long long)ND_MAX_DOMAINS);
        return SAFE_E_UNSUPPORTED;
    }
    if (kernel_ms) *kernel_ms = 0;
    SAFE_REQUIRE(ids_host, "safe_node_domains: NULL argument");
    for (int64_t d = 1; d < n_ids; ++d)
        if (ids_host[d] <= ids_host[d - 1]) {
            safe_set_error("safe_node_domains: domain ids must be sorted and distinct (position %lld)", (long long)d);
            return SAFE_E_VALUE;
        }
    if (n == 0) return SAFE_OK;
    SAFE_REQUIRE(sums_host && primary_host && primary_nes_host && (m == 0 || (nes_binary_dev && nes_dev && domain_host)),
                 "safe_node_domains: NULL argument");
    std::vector<int32_t> bin(static_cast<size_t>(m));
    for (int64_t c = 0; c < m; ++c) {
        const int32_t *at = std::lower_bound(ids_host, ids_host + n_ids, domain_host[c]);
        if (at == ids_host + n_ids || *at != domain_host[c]) {
            safe_set_error("safe_node_domains: column %lld: domain %d is not one of the %lld ids", (long long)c, domain_host[c],
                           (long long)n_ids);
            return SAFE_E_VALUE;
        }
        bin[c] = static_cast<int32_t>(at - ids_host);
    }
    // ids >= 1 are the real domains; a node none of them holds an attribute of gets id 0
    const int first_real = static_cast<int>(std::lower_bound(ids_host, ids_host + n_ids, 1) - ids_host);
    const int32_t *zero = std::lower_bound(ids_host, ids_host + n_ids, 0);
    const int zero_bin = (zero != ids_host + n_ids && *zero == 0) ? static_cast<int>(zero - ids_host) : -1;
    SAFE_REQUIRE(n < (int64_t(1) << 31), "safe_node_domains: too many rows");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    int32_t *d_dom = nullptr, *d_primary = nullptr;
    double *d_counts = nullptr, *d_pnes = nullptr;
    SAFE_TRY(b.alloc(&d_dom, static_cast<size_t>(m)));
    SAFE_TRY(b.alloc(&d_counts, static_cast<size_t>(n * n_ids)));
    SAFE_TRY(b.alloc(&d_primary, static_cast<size_t>(n)));
    SAFE_TRY(b.alloc(&d_pnes, static_cast<size_t>(n)));
    hipStream_t s = ctx->stream;
    if (m) SAFE_HIP_CHECK(hipMemcpyAsync(d_dom, bin.data(), m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    CallTimer tm;
    SAFE_HIP_CHECK(tm.start(s));
    hipLaunchKernelGGL(k_domain_counts<true>, dim3(static_cast<unsigned>(n)), dim3(DC_THREADS), 2 * n_ids * sizeof(double), s,
                       nes_binary_dev, nes_dev, m, d_dom, n_ids, first_real, zero_bin, d_counts, d_primary, d_pnes);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(sums_host, d_counts, n * n_ids * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(primary_host, d_primary, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(primary_nes_host, d_pnes, n * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));      // (bin is read by the upload until here)
    SAFE_HIP_CHECK(tm.finish(ctx, "k_domain_counts<node>", 1, kernel_ms));
    // bin indices -> ids; a node without a primary bin (no real domain holds an attribute of it and no column has id 0) gets id 0
    for (int64_t r = 0; r < n; ++r) primary_host[r] = primary_host[r] >= 0 ? ids_host[primary_host[r]] : 0;
    return SAFE_OK;
}

int safe_gather_columns(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t k,
                        double *out_host, double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 0 && m >= 0 && k >= 0, "safe_gather_columns: bad argument");
    if (kernel_ms) *kernel_ms = 0;
    if (n == 0 || k == 0) return SAFE_OK;
    SAFE_REQUIRE(values_dev && cols_host && out_host, "safe_gather_columns: NULL argument");
    for (int64_t c = 0; c < k; ++c)
        SAFE_REQUIRE(cols_host[c] >= 0 && cols_host[c] < m, "safe_gather_columns: column %lld out of [0, %lld)",
                     (long long)cols_host[c], (long long)m);
    SAFE_REQUIRE(ceil_div(n * k, GC_THREADS) < (int64_t(1) << 31), "safe_gather_columns: too many values");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    int64_t *d_cols = nullptr;
    double *d_out = nullptr;
    SAFE_TRY(b.alloc(&d_cols, static_cast<size_t>(k)));
    SAFE_TRY(b.alloc(&d_out, static_cast<size_t>(n * k)));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(d_cols, cols_host, k * sizeof(int64_t), hipMemcpyHostToDevice, s));
    CallTimer tm;
    SAFE_HIP_CHECK(tm.start(s));
    hipLaunchKernelGGL(k_gather_columns, dim3(static_cast<unsigned>(ceil_div(n * k, GC_THREADS))), dim3(GC_THREADS), 0, s, values_dev,
                       n, m, d_cols, k, d_out);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, n * k * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    if (kernel_ms) SAFE_HIP_CHECK(tm.ms(kernel_ms));
    return SAFE_OK;
}

}  // extern "C"
