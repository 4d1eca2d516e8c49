// What the per-row selection kernel (K3b, k_row_select of nbr.hip) spends its time on, and two variants that were tried:
//   MODE 0  all six digit passes for every row, one 2048-bin LDS histogram, wave-aggregated atomics
//   MODE 1  the same sweeps WITHOUT the histogram atomics (wrong results by construction): what the distance arithmetic, or the
//           reads of the matrix row, cost on their own -- the difference to MODE 0 is the share of the atomics
//   MODE 2  matrix source only: MODE 0 with the row staged in LDS once (8 n bytes beside the histogram; n <= 19 000)
//   MODE 3  early exit, the kernel as shipped: once the chosen bin holds a single key, one last sweep fetches that key and the
//           later passes are skipped
// Measured on an MI355X: staging is flat (0.131 against 0.123 ms at 3971 nodes, and the row does not fit at 20 000), the early
// exit is not (2.32 -> 0.94 ms from coordinates, 3.47 -> 1.80 ms from the matrix at 20 000 nodes): the first went, the second stayed.
// sel_count, row_key and k_row_select are copies of nbr.hip's: they follow every change there.
// Inputs: n uniform points (coordinates), and for the matrix source their Manhattan distances with every tenth entry +inf.
// MODE 0, 2 and 3 must agree on every row; MODE 0 is checked against std::nth_element on 16 rows.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off row_select.hip -o row_select ; run: ./row_select [n ...]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define SEL_BINS 2048
#define CHECK(e)                                                                             \
    do {                                                                                     \
        hipError_t _e = (e);                                                                 \
        if (_e != hipSuccess) {                                                              \
            std::fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(_e), __LINE__); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

__device__ __forceinline__ void sel_count(uint32_t *hist, int bin, int lane) {
    unsigned long long todo = __ballot(bin >= 0);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (!todo) return;
        const int leader = __ffsll(todo) - 1;
        const int b = __shfl(bin, leader);
        const unsigned long long same = __ballot(bin == b);
        if (lane == leader) atomicAdd(&hist[b], static_cast<uint32_t>(__popcll(same)));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&hist[bin], 1u);
}

template <bool XY>
__device__ __forceinline__ unsigned long long row_key(const double *__restrict__ src, const unsigned long long *__restrict__ row,
                                                      double xi, double yi, int64_t j, bool in) {
    if (XY) {
        const double dx = xi - (in ? src[2 * j] : 0.0);
        const double dy = yi - (in ? src[2 * j + 1] : 0.0);
        const double s = dx * dx + dy * dy;
        return static_cast<unsigned long long>(__double_as_longlong(s));
    }
    return in ? row[j] : 0x7FF0000000000000ull;
}

template <bool XY, int MODE>
__global__ __launch_bounds__(256) void k_row_select(const double *__restrict__ src, int64_t n, int64_t k,
                                                    unsigned long long *__restrict__ keys_out) {
    __shared__ __align__(16) uint32_t hist[SEL_BINS];
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t s_digit, s_rem, s_binsize;
    __shared__ unsigned long long s_key;
    extern __shared__ __align__(16) unsigned long long staged[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const unsigned long long INF_BITS = 0x7FF0000000000000ull;
    const double xi = XY ? src[2 * i] : 0.0, yi = XY ? src[2 * i + 1] : 0.0;
    const unsigned long long *row = reinterpret_cast<const unsigned long long *>(src) + (XY ? 0 : i * n);
    if (MODE == 2) {
        for (int64_t j = tid; j < n; j += 256) staged[j] = row[j];
        __syncthreads();
        row = staged;
    }
    unsigned long long prefix = 0, fold = 0;
    uint32_t rem = 0;
    for (int pass = 0; pass < 6; ++pass) {
        const int nbits = pass < 3 ? 11 : 10;
        const int shift = pass < 3 ? 52 - 11 * pass : 20 - 10 * (pass - 3);
        const int hshift = shift + nbits;
        const unsigned int mask = (1u << nbits) - 1;
        for (int b = tid; b < SEL_BINS; b += 256) hist[b] = 0;
        __syncthreads();
        for (int64_t jb = 0; jb < n; jb += 256) {
            const int64_t j = jb + tid;
            const bool in = j < n && j != i;
            const unsigned long long key = row_key<XY>(src, row, xi, yi, j, in);
            const bool counts = in && (XY || key < INF_BITS) && (key >> hshift) == prefix;
            const int bin = counts ? static_cast<int>((key >> shift) & mask) : -1;
            if (MODE == 1) fold += static_cast<unsigned long long>(bin);
            else sel_count(hist, bin, lane);
        }
        if (MODE == 1) {                                         // no counts to scan: keep the sweeps, take any digit
            prefix = (prefix << nbits) | (fold & mask);
            continue;
        }
        __syncthreads();
        const uint4 lo = reinterpret_cast<const uint4 *>(hist)[2 * tid], hi = reinterpret_cast<const uint4 *>(hist)[2 * tid + 1];
        const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) mine += c[q];
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            base += w < wave ? wave_sum[w] : 0u;
            total += wave_sum[w];
        }
        if (pass == 0) {
            if (total == 0) {
                if (tid == 0) keys_out[i] = 0ull;
                return;
            }
            rem = static_cast<uint32_t>((k < static_cast<int64_t>(total) ? k : static_cast<int64_t>(total)) - 1);
        }
        const uint32_t excl = base + incl - mine;
        if (rem >= excl && rem - excl < mine) {
            uint32_t r = rem - excl;
            int q = 0;
            bool found = false;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (!found && r < c[t]) {
                    q = t;
                    found = true;
                }
                if (!found) r -= c[t];
            }
            s_digit = static_cast<uint32_t>(8 * tid + q);
            s_rem = r;
            s_binsize = c[q];
        }
        __syncthreads();
        prefix = (prefix << nbits) | s_digit;
        rem = s_rem;
        if (MODE == 3 && s_binsize == 1 && pass < 5) {           // one key left under the prefix: fetch it
            for (int64_t j = tid; j < n; j += 256) {
                if (j == i) continue;
                const unsigned long long key = row_key<XY>(src, row, xi, yi, j, true);
                if ((XY || key < INF_BITS) && (key >> shift) == prefix) s_key = key;
            }
            __syncthreads();
            if (tid == 0) keys_out[i] = s_key;
            return;
        }
    }
    if (tid == 0) keys_out[i] = MODE == 1 ? prefix ^ fold : prefix;
}

template <bool XY, int MODE>
static float run(const double *d_src, int64_t n, int64_t k, unsigned long long *d_keys, std::vector<unsigned long long> *out) {
    const size_t lds = MODE == 2 ? static_cast<size_t>(n) * 8 : 0;
    if (lds) CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_row_select<XY, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds)));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float ms[6];
    for (int it = 0; it < 6; ++it) {                             // the first is the warm-up
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((k_row_select<XY, MODE>), dim3(n), dim3(256), lds, 0, d_src, n, k, d_keys);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms[it], e0, e1));
    }
    out->resize(n);
    CHECK(hipMemcpy(out->data(), d_keys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    std::sort(ms + 1, ms + 6);
    return ms[3];                                                // median of the five timed launches
}

int main(int argc, char **argv) {
    std::vector<int64_t> sizes;
    for (int a = 1; a < argc; ++a) sizes.push_back(std::atoll(argv[a]));
    if (sizes.empty()) sizes = {3971, 20000};
    for (int64_t n : sizes) {
        std::vector<double> xy(2 * n), dist(static_cast<size_t>(n) * n);
        srand48(n);
        for (double &v : xy) v = drand48();
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j)
                dist[i * n + j] = (i + j) % 10 == 3 && i != j ? INFINITY : std::fabs(xy[2 * i] - xy[2 * j]) + std::fabs(xy[2 * i + 1] - xy[2 * j + 1]);
        double *d_xy, *d_dist;
        unsigned long long *d_keys;
        CHECK(hipMalloc(&d_xy, xy.size() * sizeof(double)));
        CHECK(hipMalloc(&d_dist, dist.size() * sizeof(double)));
        CHECK(hipMalloc(&d_keys, n * sizeof(unsigned long long)));
        CHECK(hipMemcpy(d_xy, xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_dist, dist.data(), dist.size() * sizeof(double), hipMemcpyHostToDevice));
        for (int64_t k : {int64_t(50), int64_t(500)}) {
            std::vector<unsigned long long> k0, k1, k2, k3;
            const float xy0 = run<true, 0>(d_xy, n, k, d_keys, &k0);
            const float xy1 = run<true, 1>(d_xy, n, k, d_keys, &k1);
            const float xy3 = run<true, 3>(d_xy, n, k, d_keys, &k3);
            int bad = k0 != k3;
            for (int64_t i = 0; i < n; i += std::max<int64_t>(1, n / 16)) {
                std::vector<double> s;
                for (int64_t j = 0; j < n; ++j)
                    if (j != i) {
                        const double dx = xy[2 * i] - xy[2 * j], dy = xy[2 * i + 1] - xy[2 * j + 1];
                        s.push_back(dx * dx + dy * dy);
                    }
                const int64_t rank = std::min<int64_t>(k, static_cast<int64_t>(s.size())) - 1;   // (n below k + 1: the farthest)
                if (rank < 0) continue;
                std::nth_element(s.begin(), s.begin() + rank, s.end());
                unsigned long long want;
                std::memcpy(&want, &s[rank], 8);
                bad += want != k0[i];
            }
            std::printf("coordinates N=%6lld k=%3lld  six passes %.3f ms  no atomics %.3f ms (atomics' share %.0f %%)  early exit, shipped %.3f ms  "
                        "bound 6 N^2 = %.2e distance evaluations  %s\n", (long long)n, (long long)k, xy0, xy1, 100.0 * (xy0 - xy1) / xy0, xy3,
                        6.0 * n * n, bad ? "MISMATCH" : "rows agree");
            const float d0 = run<false, 0>(d_dist, n, k, d_keys, &k0);
            const float d1 = run<false, 1>(d_dist, n, k, d_keys, &k1);
            const float d3 = run<false, 3>(d_dist, n, k, d_keys, &k3);
            bad = k0 != k3;
            float d2 = -1.0f;
            if (n <= 19000) {
                d2 = run<false, 2>(d_dist, n, k, d_keys, &k2);
                bad += k0 != k2;
            }
            std::printf("matrix      N=%6lld k=%3lld  six passes %.3f ms (%.0f GB/s of 6 x 8 N^2 bytes)  no atomics %.3f ms  row in LDS %.3f ms  "
                        "early exit, shipped %.3f ms  %s\n", (long long)n, (long long)k, d0, 48.0 * n * n / (d0 * 1e6), d1, d2, d3,
                        bad ? "MISMATCH" : "rows agree");
        }
        CHECK(hipFree(d_xy));
        CHECK(hipFree(d_dist));
        CHECK(hipFree(d_keys));
    }
    return 0;
}
