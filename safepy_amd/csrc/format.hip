// Text of a row-major [N, M] f64 matrix as pandas writes it with DataFrame.to_csv(sep='\t') (safepy/safe.py:1300-1306, the
// node table of print_output_files without domains): each row is its host-made prefix (index, key and label fields,
// already quoted), then '\t' + text(v) for each of the M values, then '\n'.  text() is fmt_f64.h: NumPy's astype(str),
// which pandas uses for float blocks with float_format=None and decimal='.'; NaN is written as nothing (na_rep='').
//
// Rows go in chunks under a byte budget: a field is at most 1 + F64_TEXT_MAX bytes, so a chunk's size is bounded before
// it is formatted.  Per chunk:
//   k_fmt_row_len   one workgroup per row: the row's length (prefix + fields + newline)
//   hipcub scan     inclusive sum over the chunk's rows: where each row ends
//   k_fmt_write     one workgroup per row: the prefix, then tiles of 256 values -- each lane formats its value into LDS
//                   at its place in the tile (block scan of the lengths), and the tile leaves in aligned 16-byte stores;
//                   the bytes of a tile's last partial word wait in LDS for the next tile, and the partial words at the
//                   row's two ends (shared with the neighbour rows) are written byte by byte
// then one device-to-host copy into a pinned buffer; the host writes chunk c to the file while the device formats and
// copies chunk c + 1 (two device and two pinned buffers).
#include <hipcub/hipcub.hpp>

#include <cerrno>
#include <chrono>
#include <unistd.h>

#include "common.h"
#include "fmt_f64.h"

namespace {

constexpr int FMT_THREADS = 256;
constexpr int FMT_FIELD_MAX = 1 + F64_TEXT_MAX;                         // '\t' + text
constexpr int FMT_PREFIX_PIECE = 4096;                                  // prefix bytes staged at a time
constexpr int FMT_STAGE_BYTES = 16 + (FMT_THREADS * FMT_FIELD_MAX > FMT_PREFIX_PIECE ? FMT_THREADS * FMT_FIELD_MAX : FMT_PREFIX_PIECE);
constexpr int FMT_STAGE_WORDS = (FMT_STAGE_BYTES + 15) / 16;

__device__ inline int fmt_field_len(double v) { return 1 + f64_text(static_cast<uint64_t>(__double_as_longlong(v)), nullptr); }

__global__ __launch_bounds__(FMT_THREADS) void k_fmt_row_len(const double *__restrict__ values, int64_t m, int64_t r0,
                                                            const int64_t *__restrict__ prefix_off, int64_t *__restrict__ row_len) {
    using Reduce = hipcub::BlockReduce<int64_t, FMT_THREADS>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t r = blockIdx.x;
    const double *row = values + (r0 + r) * m;
    int64_t sum = 0;
    for (int64_t j = threadIdx.x; j < m; j += FMT_THREADS) sum += fmt_field_len(row[j]);
    sum = Reduce(tmp).Sum(sum);
    if (threadIdx.x == 0) row_len[r] = (prefix_off[r + 1] - prefix_off[r]) + sum + 1;
}

// Bytes stage[0, fill) stand for out[base, base + fill): every complete 16-byte word leaves (byte-wise where it reaches below
// `lo`, the row's first byte), the rest moves to the front of the stage.  Returns the bytes left (< 16); base advances.
__device__ inline int fmt_flush(uint4 *stage4, int fill, int64_t &base, int64_t lo, char *__restrict__ out) {
    const int words = fill >> 4;
    char *stage = reinterpret_cast<char *>(stage4);
    for (int w = threadIdx.x; w < words; w += FMT_THREADS) {
        const int64_t addr = base + 16 * static_cast<int64_t>(w);
        if (addr >= lo) {
            *reinterpret_cast<uint4 *>(out + addr) = stage4[w];
        } else {
            for (int b = 0; b < 16; ++b)
                if (addr + b >= lo) out[addr + b] = stage[16 * w + b];
        }
    }
    const int tail = fill & 15;
    char c = 0;
    if (threadIdx.x < tail) c = stage[16 * words + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < tail) stage[threadIdx.x] = c;
    __syncthreads();
    base += 16 * static_cast<int64_t>(words);
    return tail;
}

__global__ __launch_bounds__(FMT_THREADS) void k_fmt_write(const double *__restrict__ values, int64_t m, int64_t r0,
                                                          const char *__restrict__ prefix, const int64_t *__restrict__ prefix_off,
                                                          const int64_t *__restrict__ row_end, char *__restrict__ out) {
    using Scan = hipcub::BlockScan<int, FMT_THREADS>;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ uint4 stage4[FMT_STAGE_WORDS];
    char *stage = reinterpret_cast<char *>(stage4);
    const int64_t r = blockIdx.x;
    const int64_t lo = r ? row_end[r - 1] : 0;
    const int64_t hi = row_end[r];
    int64_t base = lo & ~static_cast<int64_t>(15);
    int fill = static_cast<int>(lo - base);

    // the prefix, in pieces
    const int64_t p0 = prefix_off[r], plen = prefix_off[r + 1] - p0;
    for (int64_t q = 0; q < plen; q += FMT_PREFIX_PIECE) {
        const int cnt = static_cast<int>(plen - q < FMT_PREFIX_PIECE ? plen - q : FMT_PREFIX_PIECE);
        for (int i = threadIdx.x; i < cnt; i += FMT_THREADS) stage[fill + i] = prefix[p0 + q + i];
        __syncthreads();
        fill = fmt_flush(stage4, fill + cnt, base, lo, out);
    }

    // the values, one tile of FMT_THREADS at a time
    const double *row = values + (r0 + r) * m;
    for (int64_t t = 0; t < m; t += FMT_THREADS) {
        const int64_t j = t + threadIdx.x;
        uint64_t bits = 0;
        int len = 0;
        if (j < m) {
            bits = static_cast<uint64_t>(__double_as_longlong(row[j]));
            len = 1 + f64_text(bits, nullptr);
        }
        int off, total;
        Scan(scan_tmp).ExclusiveSum(len, off, total);
        if (len) {
            char *dst = stage + fill + off;
            dst[0] = '\t';
            f64_text(bits, dst + 1);
        }
        __syncthreads();
        fill = fmt_flush(stage4, fill + total, base, lo, out);
    }

    // the newline, then the last partial word, byte by byte
    if (threadIdx.x == 0) stage[fill] = '\n';
    __syncthreads();
    ++fill;
    for (int b = threadIdx.x; b < fill; b += FMT_THREADS)
        if (base + b >= lo && base + b < hi) out[base + b] = stage[b];
}

struct FmtState {
    safe_ctx *ctx;
    char *d_prefix = nullptr;
    int64_t *d_prefix_off = nullptr, *d_len = nullptr, *d_end = nullptr;
    void *d_tmp = nullptr;
    char *d_out[2] = {nullptr, nullptr};
    char *h_out[2] = {nullptr, nullptr};
    int64_t *h_total = nullptr;
    hipEvent_t ev[10] = {};       // per slot k: [5k] kernels start, [5k+1] kernels end, [5k+2] copy start, [5k+3] copy end, [5k+4] length known
    ~FmtState() {
        (void)safe_stream_sync(ctx->stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (void *p : {(void *)d_prefix, (void *)d_prefix_off, (void *)d_len, (void *)d_end, d_tmp, (void *)d_out[0], (void *)d_out[1]})
            (void)dev_free(p);
        for (void *p : {(void *)h_out[0], (void *)h_out[1], (void *)h_total})
            if (p) (void)hipHostFree(p);
    }
};

int fmt_write_all(int fd, const char *p, size_t bytes) {
    while (bytes) {
        const ssize_t w = ::write(fd, p, bytes);
        if (w < 0) {
            if (errno == EINTR) continue;
            safe_set_error("safe_format_tsv: write failed: %s", std::strerror(errno));
            return SAFE_E_INVALID;
        }
        p += w;
        bytes -= static_cast<size_t>(w);
    }
    return SAFE_OK;
}

template <typename T>
int fmt_alloc(T **p, size_t bytes) {
    const int rc = dev_alloc_bytes(reinterpret_cast<void **>(p), std::max<size_t>(bytes, 16));
    if (rc != SAFE_OK) {
        const std::string why = safe_last_error();              // (the entry point names itself in its messages)
        safe_set_error("safe_format_tsv: %s", why.c_str());
    }
    return rc;
}

template <typename T>
int fmt_host_alloc(T **p, size_t bytes) {
    g_alloc_calls.fetch_add(1, std::memory_order_relaxed);
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(p), std::max<size_t>(bytes, 16), hipHostMallocDefault);
    if (e != hipSuccess) {
        safe_set_error("safe_format_tsv: hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return SAFE_E_NOMEM;
    }
    return SAFE_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int safe_format_tsv(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, int64_t r0, int64_t r1, const char *prefix_host,
                    const int64_t *prefix_off_host, int fd, int64_t budget_bytes, double *stats_out) {
    const auto t_call = std::chrono::steady_clock::now();
    SAFE_REQUIRE(ctx && prefix_off_host && n >= 0 && m >= 0 && 0 <= r0 && r0 <= r1 && r1 <= n && fd >= 0 && budget_bytes > 0,
                 "safe_format_tsv: bad argument");
    SAFE_REQUIRE(values_dev || r1 == r0 || m == 0, "safe_format_tsv: NULL values");
    const int64_t rows = r1 - r0;
    const int64_t pbase = prefix_off_host[0];
    for (int64_t i = 0; i < rows; ++i)
        SAFE_REQUIRE(prefix_off_host[i + 1] >= prefix_off_host[i], "safe_format_tsv: prefix offsets decrease at row %lld", (long long)i);
    const int64_t prefix_bytes = prefix_off_host[rows] - pbase;
    SAFE_REQUIRE(prefix_bytes == 0 || prefix_host, "safe_format_tsv: NULL prefixes");
    double stats[5] = {0, 0, 0, 0, 0};
    if (rows == 0) {
        if (stats_out) std::memcpy(stats_out, stats, sizeof(stats));
        return SAFE_OK;
    }
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));

    // chunks: consecutive rows whose bound stays within the budget (at least one row each)
    std::vector<int64_t> rel_off(rows + 1), chunk_start{0};
    int64_t cap = 0, acc = 0, max_rows = 0;
    for (int64_t i = 0; i < rows; ++i) {
        rel_off[i] = prefix_off_host[i] - pbase;
        const int64_t bound = (prefix_off_host[i + 1] - prefix_off_host[i]) + FMT_FIELD_MAX * m + 1;
        if (i > chunk_start.back() && acc + bound > budget_bytes) {
            cap = std::max(cap, acc);
            max_rows = std::max(max_rows, i - chunk_start.back());
            chunk_start.push_back(i);
            acc = 0;
        }
        acc += bound;
    }
    rel_off[rows] = prefix_bytes;
    cap = std::max(cap, acc);
    max_rows = std::max(max_rows, rows - chunk_start.back());
    chunk_start.push_back(rows);
    const int n_chunks = static_cast<int>(chunk_start.size()) - 1;
    SAFE_REQUIRE(max_rows < (int64_t(1) << 31), "safe_format_tsv: too many rows per chunk");

    FmtState st{ctx};
    hipStream_t s = ctx->stream;
    size_t tmp_bytes = 0;
    SAFE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, st.d_len, st.d_end, static_cast<int>(max_rows), s));
    SAFE_TRY(fmt_alloc(&st.d_prefix, prefix_bytes));
    SAFE_TRY(fmt_alloc(&st.d_prefix_off, (rows + 1) * sizeof(int64_t)));
    SAFE_TRY(fmt_alloc(&st.d_len, max_rows * sizeof(int64_t)));
    SAFE_TRY(fmt_alloc(&st.d_end, max_rows * sizeof(int64_t)));
    SAFE_TRY(fmt_alloc(&st.d_tmp, tmp_bytes));
    SAFE_TRY(fmt_host_alloc(&st.h_total, 2 * sizeof(int64_t)));
    const int slots = n_chunks > 1 ? 2 : 1;
    for (int k = 0; k < slots; ++k) {
        SAFE_TRY(fmt_alloc(&st.d_out[k], static_cast<size_t>(cap)));
        SAFE_TRY(fmt_host_alloc(&st.h_out[k], static_cast<size_t>(cap)));
    }
    for (hipEvent_t &e : st.ev) SAFE_HIP_CHECK(hipEventCreateWithFlags(&e, safe_event_flags(hipEventDefault)));
    if (prefix_bytes) SAFE_HIP_CHECK(hipMemcpyAsync(st.d_prefix, prefix_host + pbase, prefix_bytes, hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(st.d_prefix_off, rel_off.data(), (rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));

    int64_t chunk_bytes[2] = {0, 0};
    auto finish = [&](int c) -> int {           // chunk c's copy is done: time it and write it out
        const int k = c & 1;
        SAFE_HIP_CHECK(hipEventSynchronize(st.ev[5 * k + 3]));
        float ms = 0;
        SAFE_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[5 * k], st.ev[5 * k + 1]));
        stats[0] += ms;
        SAFE_HIP_CHECK(hipEventElapsedTime(&ms, st.ev[5 * k + 2], st.ev[5 * k + 3]));
        stats[1] += ms;
        const auto tw = std::chrono::steady_clock::now();
        SAFE_TRY(fmt_write_all(fd, st.h_out[k], static_cast<size_t>(chunk_bytes[k])));
        stats[2] += ms_since(tw);
        stats[4] += static_cast<double>(chunk_bytes[k]);
        return SAFE_OK;
    };
    for (int c = 0; c < n_chunks; ++c) {
        const int k = c & 1;
        const int64_t a = chunk_start[c], cnt = chunk_start[c + 1] - a;
        SAFE_HIP_CHECK(hipEventRecord(st.ev[5 * k], s));
        hipLaunchKernelGGL(k_fmt_row_len, dim3(static_cast<unsigned>(cnt)), dim3(FMT_THREADS), 0, s, values_dev, m, r0 + a,
                           st.d_prefix_off + a, st.d_len);
        SAFE_HIP_CHECK(hipGetLastError());
        SAFE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(st.d_tmp, tmp_bytes, st.d_len, st.d_end, static_cast<int>(cnt), s));
        SAFE_HIP_CHECK(hipMemcpyAsync(st.h_total + k, st.d_end + cnt - 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        SAFE_HIP_CHECK(hipEventRecord(st.ev[5 * k + 4], s));
        // chunk c - 2's copy out of d_out[k] precedes this launch on the stream
        hipLaunchKernelGGL(k_fmt_write, dim3(static_cast<unsigned>(cnt)), dim3(FMT_THREADS), 0, s, values_dev, m, r0 + a,
                           st.d_prefix, st.d_prefix_off + a, st.d_end, st.d_out[k]);
        SAFE_HIP_CHECK(hipGetLastError());
        SAFE_HIP_CHECK(hipEventRecord(st.ev[5 * k + 1], s));
        SAFE_HIP_CHECK(hipEventSynchronize(st.ev[5 * k + 4]));   // the chunk's length (k_fmt_write may still run)
        chunk_bytes[k] = st.h_total[k];
        if (chunk_bytes[k] > cap) {
            safe_set_error("safe_format_tsv: chunk of %lld bytes exceeds its bound %lld", (long long)chunk_bytes[k], (long long)cap);
            return SAFE_E_VALUE;
        }
        // h_out[k] was written to the file by finish(c - 2) in the previous iteration; the copy follows k_fmt_write on the stream
        SAFE_HIP_CHECK(hipEventRecord(st.ev[5 * k + 2], s));
        SAFE_HIP_CHECK(hipMemcpyAsync(st.h_out[k], st.d_out[k], static_cast<size_t>(chunk_bytes[k]), hipMemcpyDeviceToHost, s));
        SAFE_HIP_CHECK(hipEventRecord(st.ev[5 * k + 3], s));
        if (c > 0) SAFE_TRY(finish(c - 1));     // the host writes chunk c - 1 while chunk c is formatted and copied
    }
    SAFE_TRY(finish(n_chunks - 1));
    stats[3] = ms_since(t_call);
    if (stats_out) std::memcpy(stats_out, stats, sizeof(stats));
    return SAFE_OK;
}
