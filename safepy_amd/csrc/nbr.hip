// Neighborhood definition on gfx950: all-pairs Euclidean distance + threshold, bounded
// all-pairs shortest paths, and the derived CSR / SELL-64 membership forms.
//
// Replaces SAFE.define_neighborhoods (safepy/safe.py:369-430) and
// calculate_edge_lengths (safepy/safe_io.py:311-333).  Compiled with -ffp-contract=off:
// the reference arithmetic is scipy pdist's sqrt(dx*dx + dy*dy) with every operation
// rounded separately, and bit-exact masks need the same roundings.
//
// Where the distances come from -- coordinates, recomputed with pdist's roundings, or an N x N matrix a handle kept -- is one
// DistSource (common.h) from the exports down to the kernel launch: the two pair selections and the two row selections are thin
// wrappers over one function each, and k_euclid_bits<ROWS> is the one Euclidean bit kernel (one strict threshold, or one `<=`
// threshold per row).  The host pieces every entry point shares live here too: check_layout_finite, check_radii, upload_layout
// and build_undirected_csr (the adjacency of safe_nbr_shortpath and, sorted afterwards, of safe_nbr_diffusion).
#include <algorithm>
#include <cmath>
#include <numeric>
#include <type_traits>

#include "common.h"

// --------------------------------------------------------------------------------------
// Thresholds without a square root.  sqrt is correctly rounded and monotone, so
//   sqrt(s) <  nr  <=>  s <  T,   T = min{ s : sqrt(s) >= nr }   (squared_threshold: the reference's strict rule)
//   sqrt(s) <= r   <=>  s <= C,   C = max{ s : sqrt(s) <= r }    (squared_threshold_le: one radius per row, r >= 0)
// Both are found on the host by stepping from the square of the radius to the exact boundary.
// --------------------------------------------------------------------------------------
static double squared_threshold(double nr) {
    if (!(nr > 0.0)) return 0.0;                 // D >= 0 is never < nr
    if (std::isinf(nr)) return nr;
    double c = nr * nr;
    if (std::isinf(c)) return c;
    while (c > 0.0 && std::sqrt(c) >= nr) c = std::nextafter(c, 0.0);
    while (std::sqrt(c) < nr) c = std::nextafter(c, INFINITY);
    return c;
}

static double squared_threshold_le(double r) {
    if (std::isinf(r)) return r;
    double c = r * r;
    while (c > 0.0 && std::sqrt(c) > r) c = std::nextafter(c, 0.0);
    for (;;) {
        const double up = std::nextafter(c, INFINITY);
        if (std::isinf(up) || std::sqrt(up) > r) return c;
        c = up;
    }
}

// --------------------------------------------------------------------------------------
// K1a: distance + threshold -> bit matrix.  One lane owns one (row, 64-column word):
// the 64 lanes of a wave share the word index, so x[j], y[j] are LDS broadcasts.
// ROWS = false: bit (i, j) = (s_ij < thr), one squared_threshold for the matrix.  ROWS = true: bit (i, j) = (s_ij <= thr[i]),
// one squared_threshold_le per row, so the rule is sqrt(s) <= r_i without a root per pair.
// --------------------------------------------------------------------------------------
template <bool ROWS>
using EuclidThreshold = std::conditional_t<ROWS, const double *__restrict__, double>;

template <bool ROWS>
__global__ __launch_bounds__(256) void k_euclid_bits(const double *__restrict__ xy, int64_t n, EuclidThreshold<ROWS> thr,
                                                     uint64_t *__restrict__ bits, int64_t words) {
    __shared__ double sx[64], sy[64];
    const int64_t w = blockIdx.x;                                   // word (column block)
    const int64_t i = static_cast<int64_t>(blockIdx.y) * 256 + threadIdx.x;
    const int64_t j0 = w * 64;
    if (threadIdx.x < 64) {
        const int64_t j = j0 + threadIdx.x;
        sx[threadIdx.x] = j < n ? xy[2 * j] : 0.0;
        sy[threadIdx.x] = j < n ? xy[2 * j + 1] : 0.0;
    }
    __syncthreads();
    if (i >= n) return;
    const double xi = xy[2 * i], yi = xy[2 * i + 1];
    double c;
    if constexpr (ROWS) c = thr[i];
    else c = thr;
    const int jn = static_cast<int>(n - j0 < 64 ? n - j0 : 64);
    uint64_t word = 0;
#pragma unroll 8
    for (int t = 0; t < 64; ++t) {
        const double dx = xi - sx[t];
        const double dy = yi - sy[t];
        const double s = dx * dx + dy * dy;                          // no FMA (-ffp-contract=off)
        word |= static_cast<uint64_t>((ROWS ? s <= c : s < c) & (t < jn)) << t;
    }
    bits[i * words + w] = word;
}

// --------------------------------------------------------------------------------------
// K1b: the fused all-pairs kernel in the reference's own output layout: int64 [n,n]
// membership and/or f64 [n,n] distances.  HBM-write bound, so the kernel is shaped by what
// the memory system likes for pure stores (tools/ubench/store_ceiling.hip: 5.5 TB/s for
// independent 512 x 32 tiles, up to 6.5 TB/s when few waves per CU sweep one compact window --
// which a kernel with twelve f64 operations per store cannot keep fed): persistent workgroups,
// four per CU; workgroup b owns the 512-column chunk b % chunks_per_row of the rows
// b / chunks_per_row, + R, + 2R, ... -- at any moment they write R whole consecutive rows.  A lane keeps its two columns'
// coordinates in registers for all its rows (16 B per lane and row, 1 KiB per wave); the row's
// coordinates are wave-uniform (scalar loads).
// --------------------------------------------------------------------------------------
#define K1B_BATCH 8
// MODE bit 0: membership out, bit 1: distances out; VEC: 16-byte pair stores (even n)
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void k_euclid_dense(const double *__restrict__ xy, int64_t n, double thr_sq, int chunks_per_row,
                                                      int rows_per_sweep, int64_t *__restrict__ mask, double *__restrict__ dist) {
    const int chunk = blockIdx.x % chunks_per_row;
    const int64_t j = (static_cast<int64_t>(chunk) * 256 + threadIdx.x) * 2;
    if (j >= n) return;
    const bool two = (j + 1 < n);
    const double xa = xy[2 * j], ya = xy[2 * j + 1];
    const double xb = two ? xy[2 * j + 2] : 0.0, yb = two ? xy[2 * j + 3] : 0.0;
    auto row = [&](int64_t i, double xi, double yi) __attribute__((always_inline)) {
        const double dxa = xi - xa, dya = yi - ya;
        const double dxb = xi - xb, dyb = yi - yb;
        const double sa = dxa * dxa + dya * dya;          // no FMA (-ffp-contract=off)
        const double sb = dxb * dxb + dyb * dyb;
        const int64_t o = i * n + j;
        if (MODE & 1) {
            const int64_t ma = sa < thr_sq, mb = sb < thr_sq;
            if (VEC) {
                *reinterpret_cast<longlong2 *>(mask + o) = make_longlong2(ma, mb);
            } else {
                mask[o] = ma;
                if (two) mask[o + 1] = mb;
            }
        }
        if (MODE & 2) {
            const double da = sqrt(sa), db = sqrt(sb);
            if (VEC) {
                *reinterpret_cast<double2 *>(dist + o) = make_double2(da, db);
            } else {
                dist[o] = da;
                if (two) dist[o + 1] = db;
            }
        }
    };
    // rows in batches of K1B_BATCH: all their (wave-uniform) coordinates are requested before the first is used, so the
    // scalar-load latency is paid once per batch and the stores of a batch go out back to back
    const int64_t step = static_cast<int64_t>(K1B_BATCH) * rows_per_sweep;
    int64_t i0 = blockIdx.x / chunks_per_row;
    for (; i0 + step - rows_per_sweep < n; i0 += step) {   // whole batches
        double xi[K1B_BATCH], yi[K1B_BATCH];
#pragma unroll
        for (int u = 0; u < K1B_BATCH; ++u) {
            const int64_t i = i0 + static_cast<int64_t>(u) * rows_per_sweep;
            xi[u] = xy[2 * i];
            yi[u] = xy[2 * i + 1];
        }
#pragma unroll
        for (int u = 0; u < K1B_BATCH; ++u) row(i0 + static_cast<int64_t>(u) * rows_per_sweep, xi[u], yi[u]);
    }
    for (; i0 < n; i0 += rows_per_sweep) row(i0, xy[2 * i0], xy[2 * i0 + 1]);
}

__global__ void k_edge_lengths(const double *__restrict__ xy, int64_t n_edges, const int32_t *__restrict__ eu,
                               const int32_t *__restrict__ ev, double *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t u = eu[e], v = ev[e];
    const double dx = xy[2 * u] - xy[2 * v];
    const double dy = xy[2 * u + 1] - xy[2 * v + 1];
    out[e] = sqrt(dx * dx + dy * dy);
}

// --------------------------------------------------------------------------------------
// dense int64 <-> bit matrix
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_to_bits(const int64_t *__restrict__ a, int64_t n, int64_t words,
                                                       uint64_t *__restrict__ bits, int *__restrict__ bad) {
    // one wave per (row, word): lane t tests column 64*w + t, ballot packs the word
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= n * words) return;
    const int64_t i = wave / words, w = wave % words;
    const int64_t j = w * 64 + lane;
    int64_t v = 0;
    if (j < n) v = a[i * n + j];
    if (v != 0 && v != 1) atomicOr(bad, 1);
    const uint64_t word = __ballot(v != 0);
    if (lane == 0) bits[wave] = word;
}

__global__ __launch_bounds__(256) void k_bits_to_dense(const uint64_t *__restrict__ bits, int64_t n, int64_t words,
                                                       int64_t *__restrict__ out) {
    // lane writes two adjacent int64 (16 B); a wave covers 128 columns = two words
    const int64_t j = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 2;
    const int64_t i = blockIdx.y;
    if (j >= n) return;
    const uint64_t word = bits[i * words + (j >> 6)];
    const int64_t a = (word >> (j & 63)) & 1, b = (word >> ((j + 1) & 63)) & 1;   // j even => same word
    const int64_t o = i * n + j;
    if (j + 1 < n && (n & 1) == 0) {
        *reinterpret_cast<longlong2 *>(out + o) = make_longlong2(a, b);
    } else {
        out[o] = a;
        if (j + 1 < n) out[o + 1] = b;
    }
}

__global__ void k_row_popcount(const uint64_t *__restrict__ bits, int64_t n, int64_t words,
                               int32_t *__restrict__ count) {
    // one wave per row
    const int64_t row = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    int c = 0;
    for (int64_t w = lane; w < words; w += 64) c += __popcll(bits[row * words + w]);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) count[row] = c;
}

__global__ void k_fill_csr(const uint64_t *__restrict__ bits, int64_t n, int64_t words,
                           const int32_t *__restrict__ row_ptr, int32_t *__restrict__ col) {
    // one wave per row; lanes take words round-robin, an exclusive wave scan orders the output
    const int64_t row = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    int base = row_ptr[row];
    for (int64_t w0 = 0; w0 < words; w0 += 64) {
        const int64_t w = w0 + lane;
        uint64_t word = w < words ? bits[row * words + w] : 0;
        const int c = __popcll(word);
        int incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        int pos = base + incl - c;
        while (word) {
            const int b = __ffsll(static_cast<unsigned long long>(word)) - 1;
            col[pos++] = static_cast<int32_t>(w * 64 + b);
            word &= word - 1;
        }
        base += __shfl(incl, 63);
    }
}

__global__ void k_fill_sell(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                            const int32_t *__restrict__ sell_row, const int64_t *__restrict__ slice_off,
                            const int32_t *__restrict__ slice_width, int64_t n_slices, int32_t pad,
                            int32_t *__restrict__ sell_col) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;     // 64 threads
    if (s >= n_slices) return;
    const int32_t r = sell_row[s * 64 + lane];
    const int32_t beg = r >= 0 ? row_ptr[r] : 0;
    const int32_t cnt = r >= 0 ? row_ptr[r + 1] - beg : 0;
    const int64_t off = slice_off[s];
    const int32_t wdt = slice_width[s];
    for (int32_t t = 0; t < wdt; ++t) sell_col[off + static_cast<int64_t>(t) * 64 + lane] = t < cnt ? col[beg + t] : pad;
}

__global__ void k_sell_scale16(const int32_t *__restrict__ sell_col, int64_t entries, int64_t total, uint32_t pad2,
                               uint16_t *__restrict__ out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < total) out[i] = i < entries ? static_cast<uint16_t>(2 * sell_col[i]) : static_cast<uint16_t>(pad2);
}

// The same 2*id list in BLOCKED order: inside a slice, block b (8 members) of lane l is the 16 bytes at
// entry offset (b * 64 + l) * 8 -- a lane fetches a block with ONE 16-byte load (64 lanes: 1 KiB contiguous)
// instead of eight 2-byte loads (k_permtest_bits_blk).  The order of a lane's members is free: sums commute.
__global__ void k_sell_blocked16(const int32_t *__restrict__ sell_col, const int64_t *__restrict__ slice_off,
                                 const int32_t *__restrict__ slice_width, int64_t n_slices, int64_t entries, int64_t total,
                                 uint32_t pad2, uint16_t *__restrict__ out) {
    const int64_t s = blockIdx.x;
    if (s == n_slices) {                                       // the tail one prefetched block may touch
        for (int64_t i = entries + threadIdx.x; i < total; i += blockDim.x) out[i] = static_cast<uint16_t>(pad2);
        return;
    }
    const int64_t off = slice_off[s];
    const int64_t cnt = static_cast<int64_t>(slice_width[s]) * 64;
    for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int64_t t = i >> 6, lane = i & 63;
        out[off + ((t >> 3) * 64 + lane) * 8 + (t & 7)] = static_cast<uint16_t>(2 * sell_col[off + i]);
    }
}

// --------------------------------------------------------------------------------------
// K2: bounded all-pairs shortest paths.  One wave per source, label-correcting frontier
// relaxation to a fixpoint over the CSR adjacency.  cand = dist[v] + w is an f64 add in
// the same order Dijkstra performs it, a candidate is dropped iff cand > cutoff, and the
// kept minimum is independent of relaxation order (f64 add is monotone), so distances and
// the reached set equal networkx's bounded Dijkstra bit for bit.
// Non-negative doubles order like their bit patterns, so the per-wave distance array is
// updated with a 64-bit integer atomicMin.
// --------------------------------------------------------------------------------------
struct SpScratch {
    unsigned long long *dist;   // [workers][n]  f64 bits, init +inf
    int32_t *qa, *qb;           // [workers][n]  frontier queues
    int32_t *reached;           // [workers][n]
    int32_t *flag;              // [workers][n]  0 = not queued for next round
};

__global__ __launch_bounds__(64) void k_shortpath(int64_t n, const int32_t *__restrict__ adj_ptr,
                                                  const int32_t *__restrict__ adj_col,
                                                  const double *__restrict__ adj_w, double cutoff, SpScratch sc,
                                                  int64_t n_workers, uint64_t *__restrict__ bits, int64_t words,
                                                  double *__restrict__ dist_out) {
    const int64_t worker = blockIdx.x;
    const int lane = threadIdx.x;
    unsigned long long *dist = sc.dist + worker * n;
    int32_t *qcur = sc.qa + worker * n;
    int32_t *qnext = sc.qb + worker * n;
    int32_t *reached = sc.reached + worker * n;
    int32_t *flag = sc.flag + worker * n;
    __shared__ int s_nnext, s_nreached;
    const unsigned long long INF_BITS = 0x7FF0000000000000ull;

    for (int64_t src = worker; src < n; src += n_workers) {
        if (lane == 0) {
            atomicExch(&dist[src], 0ull);
            qcur[0] = static_cast<int32_t>(src);
            reached[0] = static_cast<int32_t>(src);
            s_nreached = 1;
            s_nnext = 0;
        }
        __syncthreads();
        int ncur = 1;
        while (ncur > 0) {
            for (int q = lane; q < ncur; q += 64) {
                const int32_t v = qcur[q];
                atomicExch(&flag[v], 0);     // dist/flag are only ever touched by L2 atomics (no stale L1 reads)
            }
            __syncthreads();
            for (int q = lane; q < ncur; q += 64) {
                const int32_t v = qcur[q];
                const double dv = __longlong_as_double(static_cast<long long>(
                    __hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
                const int32_t e1 = adj_ptr[v + 1];
                for (int32_t e = adj_ptr[v]; e < e1; ++e) {
                    const int32_t u = adj_col[e];
                    const double cand = dv + (adj_w ? adj_w[e] : 1.0);
                    if (cand > cutoff) continue;
                    const unsigned long long cb = static_cast<unsigned long long>(__double_as_longlong(cand));
                    const unsigned long long old = atomicMin(&dist[u], cb);
                    if (cb < old) {
                        if (old == INF_BITS) reached[atomicAdd(&s_nreached, 1)] = u;
                        if (atomicExch(&flag[u], 1) == 0) qnext[atomicAdd(&s_nnext, 1)] = u;
                    }
                }
            }
            __syncthreads();
            ncur = s_nnext;
            __syncthreads();
            if (lane == 0) s_nnext = 0;
            int32_t *t = qcur;
            qcur = qnext;
            qnext = t;
            __syncthreads();
        }
        const int nr = s_nreached;
        for (int q = lane; q < nr; q += 64) {
            const int32_t u = reached[q];
            atomicOr(reinterpret_cast<unsigned long long *>(&bits[src * words + (u >> 6)]), 1ull << (u & 63));
            const unsigned long long du = atomicExch(&dist[u], INF_BITS);
            if (dist_out) dist_out[src * n + u] = __longlong_as_double(static_cast<long long>(du));
            atomicExch(&flag[u], 0);
        }
        __syncthreads();
    }
}

__global__ void k_count_cols(const int32_t *__restrict__ col, int64_t nnz, int32_t *__restrict__ cnt) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e < nnz) atomicAdd(&cnt[col[e]], 1);
}

__global__ void k_fill_transpose(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col, int64_t n,
                                 const int32_t *__restrict__ at_ptr, int32_t *__restrict__ cursor,
                                 int32_t *__restrict__ at_col) {
    // one wave per row
    const int64_t row = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    for (int32_t e = row_ptr[row] + lane; e < row_ptr[row + 1]; e += 64) {
        const int32_t k = col[e];
        at_col[at_ptr[k] + atomicAdd(&cursor[k], 1)] = static_cast<int32_t>(row);
    }
}

__global__ void k_fill_u64(unsigned long long *p, unsigned long long v, int64_t count) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        p[i] = v;
}

// --------------------------------------------------------------------------------------
// K3: exact order statistics of the pairwise node distances (neighborhood_radius_type
// 'percentile': the radius is np.percentile of the distances of all pairs i < j), without
// ever holding the N (N - 1) / 2 distances.
//
// Keys are the f64 bit patterns of non-negative values, which order like unsigned integers
// (as in K2).  Bit 63 is never set; the other 63 bits are taken most significant digit first
// in six digits of 11, 11, 11, 10, 10, 10 bits -- the first is exactly the exponent field.  A
// pass sweeps every key once: a key whose bits above the digit equal one of up to SEL_SLOTS
// prefixes adds one to that prefix's histogram of the digit.  The host then finds, for every
// requested rank, the bin that holds it and appends the bin's digit to the rank's prefix; after
// the sixth pass the prefix is the key.  All counts are integers, so the result does not depend
// on the order of the atomics.
//
// Histograms are private to a workgroup (u32 in LDS: a call sees fewer than 2^32 keys, see
// SAFE_SELECT_MAX_NODES) and go to the 64-bit global counters once, when the workgroup ends.
// Real inputs put most keys of a pass into a few bins (one exponent; whole runs of tied
// distances), so a wave first settles the bins of its two leading lanes with one LDS atomic each,
// carrying the number of lanes that share the bin; only the lanes left over add singly.
// --------------------------------------------------------------------------------------
#define SEL_SLOTS SAFE_SELECT_SLOTS   // 4 x 2048 u32 = 32 KiB of LDS per workgroup
#define SEL_BINS 2048
static const int kSelPasses = 6;
static const int kSelShift[kSelPasses] = {52, 41, 30, 20, 10, 0};
static const int kSelBits[kSelPasses] = {11, 11, 11, 10, 10, 10};

struct SelPass {
    unsigned long long pre[SEL_SLOTS];   // bits above the digit that select slot q; ~0 = slot unused (bit 63 of a key is 0)
    int shift, hshift;                   // digit = (key >> shift) & mask; prefix = key >> hshift
    unsigned int mask;
};

// bin (slot * SEL_BINS + digit) the key counts in, -1 = none
__device__ __forceinline__ int sel_bin(unsigned long long key, bool valid, const SelPass &ps) {
    const unsigned long long hi = key >> ps.hshift;
    int slot = -1;
#pragma unroll
    for (int q = 0; q < SEL_SLOTS; ++q) slot = (hi == ps.pre[q]) ? q : slot;
    const int digit = static_cast<int>((key >> ps.shift) & ps.mask);
    return (valid && slot >= 0) ? slot * SEL_BINS + digit : -1;
}

// every lane of the wave calls this together
__device__ __forceinline__ void sel_count(uint32_t *hist, int bin, int lane) {
    unsigned long long todo = __ballot(bin >= 0);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (!todo) return;                                           // wave-uniform
        const int leader = __ffsll(todo) - 1;
        const int b = __shfl(bin, leader);                           // >= 0: lanes without a key never match
        const unsigned long long same = __ballot(bin == b);
        if (lane == leader) atomicAdd(&hist[b], static_cast<uint32_t>(__popcll(same)));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&hist[bin], 1u);
}

__device__ __forceinline__ void sel_flush(const uint32_t *hist, unsigned long long *__restrict__ ghist) {
    for (int b = threadIdx.x; b < SEL_SLOTS * SEL_BINS; b += 256)
        if (hist[b]) atomicAdd(&ghist[b], static_cast<unsigned long long>(hist[b]));
}

// Keys from coordinates: the SQUARED distance dx*dx + dy*dy of every pair i < j, recomputed in each pass with the operand
// order of k_euclid_dense (each operation rounded, no FMA: -ffp-contract=off).  Selecting on the square is valid because sqrt
// is correctly rounded and monotone: the sorted distances are the square roots of the sorted squares, element by element, so
// the r-th smallest distance is sqrt of the r-th smallest square (the caller takes that one root per rank on the host).
// A workgroup takes tiles of 64 rows x 256 columns: a lane keeps its column's coordinates in registers, the rows' are LDS
// broadcasts.  Tiles without a pair i < j are skipped.
__global__ __launch_bounds__(256) void k_select_xy(const double *__restrict__ xy, int64_t n, int64_t tiles_j, int64_t tiles,
                                                   SelPass ps, unsigned long long *__restrict__ ghist) {
    __shared__ uint32_t hist[SEL_SLOTS * SEL_BINS];
    __shared__ double sx[64], sy[64];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int b = tid; b < SEL_SLOTS * SEL_BINS; b += 256) hist[b] = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i0 = (t / tiles_j) * 64, j0 = (t % tiles_j) * 256;
        if (i0 >= j0 + 255) continue;                                // (same for the whole workgroup)
        __syncthreads();                                             // the tile before is done with sx, sy (first tile: hist is zero)
        if (tid < 64) {
            const int64_t i = i0 + tid;
            sx[tid] = i < n ? xy[2 * i] : 0.0;
            sy[tid] = i < n ? xy[2 * i + 1] : 0.0;
        }
        __syncthreads();
        const int64_t j = j0 + tid;
        const bool jin = j < n;
        const double xj = jin ? xy[2 * j] : 0.0, yj = jin ? xy[2 * j + 1] : 0.0;
        const int tn = static_cast<int>(n - i0 < 64 ? n - i0 : 64);
        for (int u = 0; u < tn; ++u) {
            const double dx = sx[u] - xj;
            const double dy = sy[u] - yj;
            const double s = dx * dx + dy * dy;                      // no FMA (-ffp-contract=off)
            sel_count(hist, sel_bin(static_cast<unsigned long long>(__double_as_longlong(s)), jin && i0 + u < j, ps), lane);
        }
    }
    __syncthreads();
    sel_flush(hist, ghist);
}

// Keys from the distance matrix a shortest-path handle kept (f64 [n][n], +inf where unreached), read in place: the entries
// above the diagonal, row i = the search from source i; +inf is no key.  Workgroups take rows round-robin.
__global__ __launch_bounds__(256) void k_select_dist(const double *__restrict__ dist, int64_t n, SelPass ps,
                                                     unsigned long long *__restrict__ ghist) {
    __shared__ uint32_t hist[SEL_SLOTS * SEL_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long INF_BITS = 0x7FF0000000000000ull;
    for (int b = tid; b < SEL_SLOTS * SEL_BINS; b += 256) hist[b] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x; i < n - 1; i += gridDim.x) {
        const unsigned long long *row = reinterpret_cast<const unsigned long long *>(dist) + i * n;
        for (int64_t jb = i + 1; jb < n; jb += 256) {
            const int64_t j = jb + tid;
            const unsigned long long key = j < n ? row[j] : INF_BITS;
            sel_count(hist, sel_bin(key, key < INF_BITS, ps), lane);
        }
    }
    __syncthreads();
    sel_flush(hist, ghist);
}

// --------------------------------------------------------------------------------------
// K3b: the k-th smallest distance of every ROW (neighborhood_radius_type 'nearest': node i's radius is the distance to its
// k-th nearest other node).  K3's digit plan, one workgroup per row, all six passes inside one launch: a pass sweeps the row's
// keys once, counts those whose bits above the digit equal the prefix found so far into one 2048-bin u32 histogram in LDS
// (8 KiB), a workgroup scan finds the bin that holds the wanted rank, and the bin's digit joins the prefix.  The first pass
// also counts the row's candidates, cnt, and the rank is min(k, cnt) - 1; a row without candidates gives key 0.  Counts are
// integers, so the result does not depend on the order of the atomics, nor on any order among equal keys.  Once the chosen bin
// holds a single key, one more sweep fetches it and the row is done (tools/ubench/row_select.hip: 2.32 -> 0.94 ms at 20 000 nodes).
// That microbenchmark carries a copy of sel_count, row_key and k_row_select with its variants: a change here goes there too, or
// the figures DESIGN.md quotes stop describing this kernel.
//
// XY = true: keys are the squares dx*dx + dy*dy in the operand order of k_euclid_bits, recomputed in every pass (xy is 16 B per
// node); the caller takes the one root per row.  XY = false: row i of a kept f64 [n][n] distance matrix read in place, +inf is no
// key.  Node i itself is left out by index in both.
// --------------------------------------------------------------------------------------
// key of candidate j of the row (xi, yi) / `row`; `in` = false (j past the end, or the node itself) reads nothing and is no key
template <bool XY>
__device__ __forceinline__ unsigned long long row_key(const double *__restrict__ src, const unsigned long long *__restrict__ row,
                                                      double xi, double yi, int64_t j, bool in) {
    if (XY) {
        const double dx = xi - (in ? src[2 * j] : 0.0);
        const double dy = yi - (in ? src[2 * j + 1] : 0.0);
        const double s = dx * dx + dy * dy;                                    // no FMA (-ffp-contract=off)
        return static_cast<unsigned long long>(__double_as_longlong(s));
    }
    return in ? row[j] : 0x7FF0000000000000ull;
}

template <bool XY>
__global__ __launch_bounds__(256) void k_row_select(const double *__restrict__ src, int64_t n, int64_t k,
                                                    unsigned long long *__restrict__ keys_out) {
    __shared__ __align__(16) uint32_t hist[SEL_BINS];
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t s_digit, s_rem, s_alone;
    __shared__ unsigned long long s_key;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const unsigned long long INF_BITS = 0x7FF0000000000000ull;
    const double xi = XY ? src[2 * i] : 0.0, yi = XY ? src[2 * i + 1] : 0.0;
    const unsigned long long *row = reinterpret_cast<const unsigned long long *>(src) + (XY ? 0 : i * n);
    unsigned long long prefix = 0;
    uint32_t rem = 0;
    for (int pass = 0; pass < 6; ++pass) {
        const int nbits = pass < 3 ? 11 : 10;
        const int shift = pass < 3 ? 52 - 11 * pass : 20 - 10 * (pass - 3);   // 52, 41, 30, 20, 10, 0
        const int hshift = shift + nbits;                                      // (63 in the first pass: bit 63 of a key is 0)
        const unsigned int mask = (1u << nbits) - 1;
        for (int b = tid; b < SEL_BINS; b += 256) hist[b] = 0;
        __syncthreads();
        for (int64_t jb = 0; jb < n; jb += 256) {                              // (the same trip count for every lane: sel_count)
            const int64_t j = jb + tid;
            const bool in = j < n && j != i;
            const unsigned long long key = row_key<XY>(src, row, xi, yi, j, in);
            const bool counts = in && (XY || key < INF_BITS) && (key >> hshift) == prefix;
            sel_count(hist, counts ? static_cast<int>((key >> shift) & mask) : -1, lane);
        }
        __syncthreads();
        // workgroup scan: a thread owns eight consecutive bins
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
            if (total == 0) {                                                  // no candidate (the same for the whole workgroup)
                if (tid == 0) keys_out[i] = 0ull;
                return;
            }
            rem = static_cast<uint32_t>((k < static_cast<int64_t>(total) ? k : static_cast<int64_t>(total)) - 1);
        }
        const uint32_t excl = base + incl - mine;
        if (rem >= excl && rem - excl < mine) {                                // one thread: the bins before its own hold excl keys
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
            s_alone = c[q] == 1;
        }
        __syncthreads();
        prefix = (prefix << nbits) | s_digit;
        rem = s_rem;
        if (s_alone && pass < 5) {                                             // (the same for the whole workgroup)
            // the chosen bin holds ONE key, the wanted one: a last sweep fetches it and the later passes are skipped (untied
            // distances of a row part after two or three digits; tied ones -- a bin of two or more -- run all six)
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
    if (tid == 0) keys_out[i] = prefix;
}

// Membership from a kept distance matrix and one radius per row: bit (i, j) = (D[i][j] <= r[i]) and D[i][j] reached.  One
// workgroup per row, a wave per 64-column word (the ballot is the word).  masked_out, when given, receives D[i][j] where the bit
// is set and +inf elsewhere: the matrix a handle built with a cutoff keeps.
__global__ __launch_bounds__(256) void k_dist_bits_rows(const double *__restrict__ dist, int64_t n, const double *__restrict__ radii,
                                                        uint64_t *__restrict__ bits, int64_t words, double *__restrict__ masked_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const double r = radii[i], inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int64_t w = wave; w < words; w += 4) {
        const int64_t j = w * 64 + lane;
        const double d = j < n ? dist[i * n + j] : inf;
        const bool member = d <= r && d < inf;
        const unsigned long long word = __ballot(member);
        if (lane == 0) bits[i * words + w] = word;
        if (masked_out && j < n) masked_out[i * n + j] = member ? d : inf;
    }
}

// --------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------
int check_layout_finite(const char *fn, const double *xy_host, int64_t n) {
    for (int64_t i = 0; i < 2 * n; ++i)
        if (!std::isfinite(xy_host[i])) {
            safe_set_error("%s: node %lld has a coordinate that is not finite", fn, (long long)(i / 2));
            return SAFE_E_VALUE;
        }
    return SAFE_OK;
}

int check_radii(const char *fn, const double *radii, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(radii[i] >= 0.0)) {
            safe_set_error("%s: the radius of row %lld is negative or NaN", fn, (long long)i);
            return SAFE_E_VALUE;
        }
    return SAFE_OK;
}

int upload_layout(safe_ctx *ctx, CallBufs *b, const char *fn, const double *xy_host, int64_t n, const double **d_xy_out) {
    double *d_xy = nullptr;
    SAFE_TRY(b->alloc(&d_xy, 2 * n));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_xy, xy_host, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    *d_xy_out = d_xy;
    return SAFE_OK;
}

int build_undirected_csr(const char *fn, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v, const double *edge_w,
                         std::vector<int32_t> *ptr, std::vector<int32_t> *col, std::vector<double> *w) {
    ptr->assign(n + 1, 0);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int32_t u = edge_u[e], v = edge_v[e];
        SAFE_REQUIRE(u >= 0 && u < n && v >= 0 && v < n, "%s: edge %lld has an end point outside [0,%lld)", fn, (long long)e,
                     (long long)n);
        // +inf is refused too: the shortest-path kernel's +inf means "unreached", networkx's "reached over a path of length +inf"
        if (edge_w)
            SAFE_REQUIRE(edge_w[e] >= 0.0 && std::isfinite(edge_w[e]), "%s: edge %lld has a negative, infinite or NaN weight", fn,
                         (long long)e);
        (*ptr)[u + 1]++;
        if (u != v) (*ptr)[v + 1]++;
    }
    for (int64_t i = 0; i < n; ++i) {
        SAFE_REQUIRE(static_cast<int64_t>((*ptr)[i]) + (*ptr)[i + 1] < (1ll << 31), "%s: too many entries for int32 CSR offsets", fn);
        (*ptr)[i + 1] += (*ptr)[i];
    }
    const int64_t n_adj = (*ptr)[n];
    col->assign(std::max<int64_t>(n_adj, 1), 0);
    w->assign(std::max<int64_t>(n_adj, 1), 0.0);
    std::vector<int32_t> fill(ptr->begin(), ptr->end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int32_t u = edge_u[e], v = edge_v[e];
        const double we = edge_w ? edge_w[e] : 1.0;
        (*col)[fill[u]] = v;
        (*w)[fill[u]++] = we;
        if (u != v) {
            (*col)[fill[v]] = u;
            (*w)[fill[v]++] = we;
        }
    }
    return SAFE_OK;
}

// one pass for up to SEL_SLOTS prefixes: the histograms, on the host
static int sel_pass(safe_ctx *ctx, const DistSource &src, const SelPass &ps, unsigned long long *d_hist,
                    std::vector<unsigned long long> &h_hist) {
    hipStream_t s = ctx->stream;
    const size_t bytes = static_cast<size_t>(SEL_SLOTS) * SEL_BINS * sizeof(unsigned long long);
    const int64_t n = src.n, wgs = 4 * static_cast<int64_t>(ctx->num_cu);   // 33 KiB of LDS each: four fit a CU
    SAFE_HIP_CHECK(hipMemsetAsync(d_hist, 0, bytes, s));
    if (src.xy) {
        const int64_t tiles_j = ceil_div(n, 256), tiles = ceil_div(n, 64) * tiles_j;
        hipLaunchKernelGGL(k_select_xy, dim3(std::min(tiles, wgs)), dim3(256), 0, s, src.xy, n, tiles_j, tiles, ps, d_hist);
    } else {
        hipLaunchKernelGGL(k_select_dist, dim3(std::min(n - 1, wgs)), dim3(256), 0, s, src.dist, n, ps, d_hist);
    }
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(hipMemcpyAsync(h_hist.data(), d_hist, bytes, hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    return SAFE_OK;
}

// keys[t] = the key of rank ranks[t] (0-based, ascending multiset) among the source's keys; *count = how many keys there are.
// Ranks are checked against the count, which the first pass delivers.
static int sel_keys(safe_ctx *ctx, const DistSource &src, const char *who, const int64_t *ranks, int64_t n_ranks,
                    std::vector<unsigned long long> *keys, int64_t *count) {
    *count = 0;
    keys->assign(n_ranks, 0);
    std::vector<unsigned long long> h_hist(static_cast<size_t>(SEL_SLOTS) * SEL_BINS), pre(n_ranks, 0), next(n_ranks, 0), distinct;
    std::vector<int64_t> rem(ranks, ranks + n_ranks);
    CallBufs b;                                         // (behind h_hist: the read-backs write it)
    unsigned long long *d_hist = nullptr;
    SAFE_TRY(b.alloc(&d_hist, h_hist.size()));
    for (int pass = 0; pass < kSelPasses && src.n >= 2; ++pass) {
        distinct.assign(pre.begin(), pre.end());
        if (pass == 0) distinct.assign(1, 0ull);        // one empty prefix: every key, whether or not a rank was asked for
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        const int bins = 1 << kSelBits[pass];
        for (size_t g = 0; g < distinct.size(); g += SEL_SLOTS) {
            const int used = static_cast<int>(std::min<size_t>(SEL_SLOTS, distinct.size() - g));
            SelPass ps;
            for (int q = 0; q < SEL_SLOTS; ++q) ps.pre[q] = q < used ? distinct[g + q] : ~0ull;
            ps.shift = kSelShift[pass];
            ps.hshift = kSelShift[pass] + kSelBits[pass];
            ps.mask = static_cast<unsigned int>(bins - 1);
            SAFE_TRY(sel_pass(ctx, src, ps, d_hist, h_hist));
            if (pass == 0) {
                unsigned long long total = 0;
                for (int d = 0; d < bins; ++d) total += h_hist[d];
                *count = static_cast<int64_t>(total);
                break;                                  // (the ranks are resolved below, once they are known to be inside)
            }
            for (int64_t t = 0; t < n_ranks; ++t) {
                int q = 0;
                while (q < used && ps.pre[q] != pre[t]) ++q;
                if (q == used) continue;                // this rank's prefix is in another group
                const unsigned long long *h = &h_hist[static_cast<size_t>(q) * SEL_BINS];
                int d = 0;
                while (d < bins && static_cast<unsigned long long>(rem[t]) >= h[d]) rem[t] -= static_cast<int64_t>(h[d++]);
                if (d == bins) {
                    safe_set_error("%s: the histograms of pass %d do not hold rank %lld", who, pass, (long long)ranks[t]);
                    return SAFE_E_HIP;
                }
                next[t] = (pre[t] << kSelBits[pass]) | static_cast<unsigned long long>(d);
            }
        }
        if (pass == 0) {
            for (int64_t t = 0; t < n_ranks; ++t) {
                SAFE_REQUIRE(ranks[t] >= 0 && ranks[t] < *count, "%s: rank %lld is outside [0, %lld)", who, (long long)ranks[t],
                             (long long)*count);
                int d = 0;
                while (static_cast<unsigned long long>(rem[t]) >= h_hist[d]) rem[t] -= static_cast<int64_t>(h_hist[d++]);
                next[t] = static_cast<unsigned long long>(d);
            }
            if (n_ranks == 0) return SAFE_OK;
        }
        pre.swap(next);
    }
    SAFE_REQUIRE(src.n >= 2 || n_ranks == 0, "%s: rank %lld is outside [0, 0): one node has no pair", who, (long long)ranks[0]);
    *keys = pre;
    return SAFE_OK;
}

void nbr_free(safe_nbr *nbr) {
    if (!nbr) return;
    for (const void *q : {(const void *)nbr->bits, (const void *)nbr->row_ptr, (const void *)nbr->col, (const void *)nbr->sell_row,
                          (const void *)nbr->sell_pos, (const void *)nbr->slice_off, (const void *)nbr->slice_width,
                          (const void *)nbr->sell_col, (const void *)nbr->sell_col2, (const void *)nbr->sell_col2b,
                          (const void *)nbr->dist, (const void *)nbr->at_ptr, (const void *)nbr->at_col, (const void *)nbr->w_csr,
                          (const void *)nbr->w_sell})
        (void)dev_free(q);
    nbr_free_blocks(nbr);
    if (nbr->bits_plan_pinned) (void)hipHostFree(nbr->bits_plan_pinned);
    delete nbr;
}

int nbr_new(safe_ctx *ctx, int64_t n, NbrPtr *out) {
    SAFE_REQUIRE(n >= 1 && n < (1ll << 31) - 64, "neighborhood size n=%lld out of range", (long long)n);
    NbrPtr nbr(new safe_nbr(), nbr_free);
    nbr->ctx = ctx;
    nbr->n = n;
    nbr->words = ceil_div(n, 64);
    SAFE_TRY(dev_alloc(&nbr->bits, static_cast<size_t>(n) * nbr->words));
    *out = std::move(nbr);
    return SAFE_OK;
}

// per-row member counts of the bit matrix into nbr->h_row_count
static int nbr_row_counts(safe_nbr *nbr) {
    safe_ctx *ctx = nbr->ctx;
    const int64_t n = nbr->n;
    CallBufs b;
    int32_t *d_count = nullptr;
    SAFE_TRY(b.alloc(&d_count, n));
    hipLaunchKernelGGL(k_row_popcount, dim3(ceil_div(n * 64, 256)), dim3(256), 0, ctx->stream, nbr->bits, n,
                       nbr->words, d_count);
    nbr->h_row_count.resize(n);
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->h_row_count.data(), d_count, n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                  ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int nbr_finalize_from_bits(safe_nbr *nbr) {
    safe_ctx *ctx = nbr->ctx;
    const int64_t n = nbr->n;
    SAFE_TRY(nbr_row_counts(nbr));

    std::vector<int32_t> row_ptr(n + 1, 0);
    int64_t nnz = 0, max_count = 0;
    for (int64_t i = 0; i < n; ++i) {
        nnz += nbr->h_row_count[i];
        max_count = std::max<int64_t>(max_count, nbr->h_row_count[i]);
        SAFE_REQUIRE(nnz < (1ll << 31), "membership has too many entries for int32 CSR offsets");
        row_ptr[i + 1] = static_cast<int32_t>(nnz);
    }
    nbr->nnz = nnz;
    nbr->max_count = max_count;

    // SELL-64: rows sorted by descending count (stable: ties keep node order)
    std::vector<int32_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return nbr->h_row_count[a] > nbr->h_row_count[b];
    });
    nbr->n_slices = ceil_div(n, 64);
    std::vector<int32_t> sell_row(nbr->n_slices * 64, -1);
    std::copy(order.begin(), order.end(), sell_row.begin());
    std::vector<int32_t> sell_pos(n);
    for (int64_t t = 0; t < n; ++t) sell_pos[order[t]] = static_cast<int32_t>(t);
    nbr->h_slice_width.assign(nbr->n_slices, 0);
    nbr->h_slice_off.assign(nbr->n_slices + 1, 0);
    for (int64_t s = 0; s < nbr->n_slices; ++s) {
        int32_t wdt = nbr->h_row_count[order[s * 64]];              // first row of the slice is its largest
        wdt = (wdt + 7) & ~7;                                       // unroll granule of the gather loops (8-input carry-save blocks)
        nbr->h_slice_width[s] = wdt;
        nbr->h_slice_off[s + 1] = nbr->h_slice_off[s] + static_cast<int64_t>(wdt) * 64;
    }
    nbr->sell_entries = nbr->h_slice_off[nbr->n_slices];

    SAFE_TRY(dev_alloc(&nbr->row_ptr, n + 1));
    SAFE_TRY(dev_alloc(&nbr->col, nnz));
    SAFE_TRY(dev_alloc(&nbr->sell_row, nbr->n_slices * 64));
    SAFE_TRY(dev_alloc(&nbr->sell_pos, n));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->sell_pos, sell_pos.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SAFE_TRY(dev_alloc(&nbr->slice_off, nbr->n_slices + 1));
    SAFE_TRY(dev_alloc(&nbr->slice_width, nbr->n_slices));
    SAFE_TRY(dev_alloc(&nbr->sell_col, nbr->sell_entries));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->row_ptr, row_ptr.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                                  ctx->stream));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->sell_row, sell_row.data(), sell_row.size() * sizeof(int32_t),
                                  hipMemcpyHostToDevice, ctx->stream));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->slice_off, nbr->h_slice_off.data(), (nbr->n_slices + 1) * sizeof(int64_t),
                                  hipMemcpyHostToDevice, ctx->stream));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->slice_width, nbr->h_slice_width.data(), nbr->n_slices * sizeof(int32_t),
                                  hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_fill_csr, dim3(ceil_div(n * 64, 256)), dim3(256), 0, ctx->stream, nbr->bits, n, nbr->words,
                       nbr->row_ptr, nbr->col);
    hipLaunchKernelGGL(k_fill_sell, dim3(nbr->n_slices), dim3(64), 0, ctx->stream, nbr->row_ptr, nbr->col,
                       nbr->sell_row, nbr->slice_off, nbr->slice_width, nbr->n_slices, static_cast<int32_t>(n),
                       nbr->sell_col);
    if (n < 32768) {
        const int64_t total = nbr->sell_entries + 1024;         // tail: two blocks of 8 x 64 may be prefetched past the end
        SAFE_TRY(dev_alloc(&nbr->sell_col2, total));
        hipLaunchKernelGGL(k_sell_scale16, dim3(ceil_div(total, 256)), dim3(256), 0, ctx->stream, nbr->sell_col,
                           nbr->sell_entries, total, static_cast<uint32_t>(2 * n), nbr->sell_col2);
        SAFE_TRY(dev_alloc(&nbr->sell_col2b, total));
        hipLaunchKernelGGL(k_sell_blocked16, dim3(nbr->n_slices + 1), dim3(256), 0, ctx->stream, nbr->sell_col, nbr->slice_off,
                           nbr->slice_width, nbr->n_slices, nbr->sell_entries, total, static_cast<uint32_t>(2 * n),
                           nbr->sell_col2b);
    }
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));   // host vectors above go out of scope
    return SAFE_OK;
}

int nbr_build_transpose(safe_nbr *nbr) {
    if (nbr->at_ptr) return SAFE_OK;
    safe_ctx *ctx = nbr->ctx;
    const int64_t n = nbr->n, nnz = nbr->nnz;
    std::vector<int32_t> cnt(n), ptr(n + 1, 0);
    CallBufs b;
    int32_t *d_cnt = nullptr;
    SAFE_TRY(b.alloc(&d_cnt, n));
    SAFE_HIP_CHECK(hipMemsetAsync(d_cnt, 0, n * sizeof(int32_t), ctx->stream));
    if (nnz) hipLaunchKernelGGL(k_count_cols, dim3(ceil_div(nnz, 256)), dim3(256), 0, ctx->stream, nbr->col, nnz, d_cnt);
    SAFE_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    for (int64_t k = 0; k < n; ++k) ptr[k + 1] = ptr[k] + cnt[k];
    SAFE_TRY(dev_alloc(&nbr->at_ptr, n + 1));
    SAFE_TRY(dev_alloc(&nbr->at_col, nnz));
    SAFE_HIP_CHECK(hipMemcpyAsync(nbr->at_ptr, ptr.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SAFE_HIP_CHECK(hipMemsetAsync(d_cnt, 0, n * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_fill_transpose, dim3(ceil_div(n * 64, 256)), dim3(256), 0, ctx->stream, nbr->row_ptr, nbr->col, n,
                       nbr->at_ptr, d_cnt, nbr->at_col);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

// K3b on the context's stream: keys[i] of every row into a host vector
static int row_select_keys(safe_ctx *ctx, const char *fn, const DistSource &src, int64_t k, std::vector<unsigned long long> *keys) {
    const int64_t n = src.n;
    keys->assign(n, 0);
    CallBufs b;                                         // (behind *keys: the read-back writes it)
    unsigned long long *d_keys = nullptr;
    SAFE_TRY(b.alloc(&d_keys, n));
    if (src.xy) hipLaunchKernelGGL(k_row_select<true>, dim3(n), dim3(256), 0, ctx->stream, src.xy, n, k, d_keys);
    else hipLaunchKernelGGL(k_row_select<false>, dim3(n), dim3(256), 0, ctx->stream, src.dist, n, k, d_keys);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(keys->data(), d_keys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

// The selections behind the exports, over either source.  xy_host given: the source is that layout -- checked, uploaded into src.xy,
// keys are squared distances and the caller's values the one root per key (k_select_xy, k_row_select); else src.dist is read in place.
static void keys_to_distances(const std::vector<unsigned long long> &keys, bool squared, double *out_host) {
    if (keys.empty()) return;
    std::memcpy(out_host, keys.data(), keys.size() * sizeof(double));
    if (squared)
        for (size_t t = 0; t < keys.size(); ++t) out_host[t] = std::sqrt(out_host[t]);
}

static int pair_distance_select(safe_ctx *ctx, DistSource src, const double *xy_host, const char *fn, const int64_t *ranks, int64_t n_ranks,
                                double *out_host, int64_t *count_out) {
    SAFE_REQUIRE(n_ranks == 0 || (ranks && out_host), "%s: NULL rank or output array", fn);
    if (count_out) *count_out = 0;
    if (src.n > SAFE_SELECT_MAX_NODES) {
        safe_set_error("%s: n=%lld is above the %d nodes the selection takes", fn, (long long)src.n, SAFE_SELECT_MAX_NODES);
        return SAFE_E_UNSUPPORTED;
    }
    if (xy_host) SAFE_TRY(check_layout_finite(fn, xy_host, src.n));
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<unsigned long long> keys;
    CallBufs b;
    if (xy_host) SAFE_TRY(upload_layout(ctx, &b, fn, xy_host, src.n, &src.xy));
    int64_t count = 0;
    const int rc = sel_keys(ctx, src, fn, ranks, n_ranks, &keys, &count);
    if (count_out) *count_out = count;                                // (known even where a rank is refused)
    SAFE_TRY(rc);
    if (xy_host) SAFE_HIP_CHECK_AS(fn, safe_stream_sync(ctx->stream));   // (n = 1 launches nothing: the upload still reads xy_host)
    keys_to_distances(keys, xy_host != nullptr, out_host);
    return SAFE_OK;
}

static int row_distance_select(safe_ctx *ctx, DistSource src, const double *xy_host, const char *fn, int64_t k, double *radii_out_host) {
    SAFE_REQUIRE(k >= 1, "%s: k=%lld, the number of nearest nodes must be at least 1", fn, (long long)k);
    if (xy_host) SAFE_TRY(check_layout_finite(fn, xy_host, src.n));
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<unsigned long long> keys;
    CallBufs b;
    if (xy_host) SAFE_TRY(upload_layout(ctx, &b, fn, xy_host, src.n, &src.xy));
    SAFE_TRY(row_select_keys(ctx, fn, src, k, &keys));
    keys_to_distances(keys, xy_host != nullptr, radii_out_host);
    return SAFE_OK;
}

extern "C" {

int safe_nbr_euclidean(safe_ctx *ctx, const double *xy_host, int64_t n, double nr, safe_nbr **out) {
    SAFE_REQUIRE(ctx && xy_host && out, "safe_nbr_euclidean: NULL argument");
    *out = nullptr;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    CallBufs b;
    const double *d_xy = nullptr;
    SAFE_TRY(upload_layout(ctx, &b, "safe_nbr_euclidean", xy_host, n, &d_xy));
    hipLaunchKernelGGL(k_euclid_bits<false>, dim3(nbr->words, ceil_div(n, 256)), dim3(256), 0, ctx->stream, d_xy, n,
                       squared_threshold(nr), nbr->bits, nbr->words);
    SAFE_HIP_CHECK_AS("safe_nbr_euclidean", hipGetLastError());
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));
    nbr->h_xy.assign(xy_host, xy_host + 2 * n);       // node order of the block-sparse form (mfma.hip)
    *out = nbr.release();
    return SAFE_OK;
}

int safe_nbr_block_count(const safe_nbr *nbr, int64_t *blocks) {
    SAFE_REQUIRE(nbr && blocks, "safe_nbr_block_count: NULL argument");
    *blocks = nbr->blocks_ready ? nbr->bs_blocks : 0;
    return SAFE_OK;
}

int safe_nbr_piece_count(const safe_nbr *nbr, int64_t *pieces) {
    SAFE_REQUIRE(nbr && pieces, "safe_nbr_piece_count: NULL argument");
    *pieces = nbr->blocks_ready ? nbr->bs_pieces : 0;
    return SAFE_OK;
}

int safe_nbr_set_layout(safe_nbr *nbr, const double *xy_host) {
    SAFE_REQUIRE(nbr && xy_host, "safe_nbr_set_layout: NULL argument");
    nbr->h_xy.assign(xy_host, xy_host + 2 * nbr->n);
    if (nbr->blocks_ready) nbr_free_blocks(nbr);      // rebuilt in the new order on next use
    return SAFE_OK;
}

int safe_euclidean_dense_dev(safe_ctx *ctx, const double *xy_dev, int64_t n, double nr, int64_t *mask_out_dev,
                             double *dist_out_dev) {
    SAFE_REQUIRE(ctx && xy_dev && n >= 1, "safe_euclidean_dense_dev: bad argument");
    SAFE_REQUIRE(mask_out_dev || dist_out_dev, "safe_euclidean_dense_dev: no output requested");
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t wgs = 4 * static_cast<int64_t>(ctx->num_cu);   // resident workgroups (16 waves per CU hide the scalar-load and f64 latency); they sweep whole rows together
    const int64_t chunks_per_row = ceil_div(n, 512);
    const int64_t rows_per_sweep = std::max<int64_t>(1, std::min<int64_t>(n, wgs / chunks_per_row));
    const int mode = (mask_out_dev ? 1 : 0) | (dist_out_dev ? 2 : 0);
    const bool vec = (n & 1) == 0;                         // 16-byte pair stores need even n (row starts stay 16-byte aligned)
    const dim3 grid(chunks_per_row * rows_per_sweep), block(256);
    const double thr_sq = squared_threshold(nr);
    const int cpr = static_cast<int>(chunks_per_row), rps = static_cast<int>(rows_per_sweep);
#define LAUNCH_K1B(M, V) hipLaunchKernelGGL((k_euclid_dense<M, V>), grid, block, 0, ctx->stream, xy_dev, n, thr_sq, cpr, rps, mask_out_dev, dist_out_dev)
    if (vec) {
        if (mode == 1) LAUNCH_K1B(1, true);
        else if (mode == 2) LAUNCH_K1B(2, true);
        else LAUNCH_K1B(3, true);
    } else {
        if (mode == 1) LAUNCH_K1B(1, false);
        else if (mode == 2) LAUNCH_K1B(2, false);
        else LAUNCH_K1B(3, false);
    }
#undef LAUNCH_K1B
    SAFE_HIP_CHECK(hipGetLastError());
    return SAFE_OK;
}

int safe_edge_lengths(safe_ctx *ctx, const double *xy_host, int64_t n, int64_t n_edges, const int32_t *edge_u,
                      const int32_t *edge_v, double *out_host) {
    SAFE_REQUIRE(ctx && xy_host && n >= 1 && n_edges >= 0, "safe_edge_lengths: bad argument");
    if (n_edges == 0) return SAFE_OK;
    SAFE_REQUIRE(edge_u && edge_v && out_host, "safe_edge_lengths: NULL argument");
    for (int64_t e = 0; e < n_edges; ++e)
        SAFE_REQUIRE(edge_u[e] >= 0 && edge_u[e] < n && edge_v[e] >= 0 && edge_v[e] < n,
                     "safe_edge_lengths: edge %lld has an end point outside [0,%lld)", (long long)e, (long long)n);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const double *d_xy = nullptr;
    double *d_out = nullptr;
    int32_t *d_u = nullptr, *d_v = nullptr;
    CallBufs b;
    SAFE_TRY(upload_layout(ctx, &b, "safe_edge_lengths", xy_host, n, &d_xy));
    SAFE_TRY(b.alloc(&d_out, n_edges));
    SAFE_TRY(b.alloc(&d_u, n_edges));
    SAFE_TRY(b.alloc(&d_v, n_edges));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_u, edge_u, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SAFE_HIP_CHECK(hipMemcpyAsync(d_v, edge_v, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_edge_lengths, dim3(ceil_div(n_edges, 256)), dim3(256), 0, ctx->stream, d_xy, n_edges, d_u,
                       d_v, d_out);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, n_edges * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_nbr_shortpath(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v,
                       const double *edge_w, double cutoff, int keep_distances, safe_nbr **out) {
    SAFE_REQUIRE(ctx && out && n >= 1 && n_edges >= 0, "safe_nbr_shortpath: bad argument");
    SAFE_REQUIRE(n_edges == 0 || (edge_u && edge_v), "safe_nbr_shortpath: NULL edge arrays");
    *out = nullptr;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const char *fn = "safe_nbr_shortpath";
    // two edges between one pair are both kept, so the lighter one counts -- nx.Graph would keep the weight added last:
    // de-duplicating is the caller's job
    std::vector<int32_t> deg, adj_col;
    std::vector<double> adj_w;
    SAFE_TRY(build_undirected_csr(fn, n, n_edges, edge_u, edge_v, edge_w, &deg, &adj_col, &adj_w));
    const int64_t n_adj = deg[n];
    hipStream_t s = ctx->stream;
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    const int64_t n_workers = std::min<int64_t>(n, static_cast<int64_t>(ctx->num_cu) * 8);
    CallBufs b;                                         // (behind deg, adj_col, adj_w: the uploads read them)
    int32_t *d_ptr = nullptr, *d_col = nullptr;
    double *d_w = nullptr;
    SpScratch sc{};
    SAFE_TRY(b.alloc(&d_ptr, n + 1));
    SAFE_TRY(b.alloc(&d_col, n_adj));
    if (edge_w) SAFE_TRY(b.alloc(&d_w, n_adj));
    SAFE_TRY(b.alloc(&sc.dist, n_workers * n));
    SAFE_TRY(b.alloc(&sc.qa, n_workers * n));
    SAFE_TRY(b.alloc(&sc.qb, n_workers * n));
    SAFE_TRY(b.alloc(&sc.reached, n_workers * n));
    SAFE_TRY(b.alloc(&sc.flag, n_workers * n));
    if (keep_distances) SAFE_TRY(dev_alloc(&nbr->dist, n * n));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_ptr, deg.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_adj) SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_col, adj_col.data(), n_adj * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (d_w && n_adj) SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_w, adj_w.data(), n_adj * sizeof(double), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(nbr->bits, 0, n * nbr->words * sizeof(uint64_t), s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(sc.flag, 0, n_workers * n * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_fill_u64, dim3(1024), dim3(256), 0, s, sc.dist, 0x7FF0000000000000ull, n_workers * n);
    if (nbr->dist)
        hipLaunchKernelGGL(k_fill_u64, dim3(2048), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(nbr->dist),
                           0x7FF0000000000000ull, n * n);
    hipLaunchKernelGGL(k_shortpath, dim3(n_workers), dim3(64), 0, s, n, d_ptr, d_col, d_w, cutoff, sc, n_workers, nbr->bits,
                       nbr->words, nbr->dist);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));
    *out = nbr.release();
    return SAFE_OK;
}

int safe_nbr_from_dense_i64(safe_ctx *ctx, const int64_t *a_host, int64_t n, safe_nbr **out) {
    SAFE_REQUIRE(ctx && a_host && out, "safe_nbr_from_dense_i64: NULL argument");
    *out = nullptr;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const char *fn = "safe_nbr_from_dense_i64";
    hipStream_t s = ctx->stream;
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    int bad = 0;
    {
        CallBufs b;                                     // (the 8 n^2 byte copy of the matrix goes before the derived forms are built)
        int64_t *d_a = nullptr;
        int *d_bad = nullptr;
        SAFE_TRY(b.alloc(&d_a, n * n));
        SAFE_TRY(b.alloc(&d_bad, 1));
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_a, a_host, n * n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_bad, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_dense_to_bits, dim3(ceil_div(n * nbr->words * 64, 256)), dim3(256), 0, s, d_a, n, nbr->words, nbr->bits,
                           d_bad);
        SAFE_HIP_CHECK_AS(fn, hipGetLastError());
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
        SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    }
    if (bad) {
        safe_set_error("safe_nbr_from_dense_i64: membership matrix has entries outside {0,1}");
        return SAFE_E_VALUE;
    }
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));
    *out = nbr.release();
    return SAFE_OK;
}

int safe_nbr_destroy(safe_nbr *nbr) {
    if (!nbr) return SAFE_OK;
    (void)hipSetDevice(nbr->ctx->device);
    (void)safe_stream_sync(nbr->ctx->stream);
    nbr_free(nbr);
    return SAFE_OK;
}

int safe_nbr_info(const safe_nbr *nbr, int64_t *n, int64_t *nnz, int64_t *max_row_count) {
    SAFE_REQUIRE(nbr != nullptr, "safe_nbr_info: nbr is NULL");
    if (n) *n = nbr->n;
    if (nnz) *nnz = nbr->nnz;
    if (max_row_count) *max_row_count = nbr->max_count;
    return SAFE_OK;
}

int safe_nbr_to_dense_i64_dev(safe_nbr *nbr, int64_t *out_dev) {
    SAFE_REQUIRE(nbr && out_dev, "safe_nbr_to_dense_i64_dev: NULL argument");
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_bits_to_dense, dim3(ceil_div(nbr->n, 512), nbr->n), dim3(256), 0, ctx->stream, nbr->bits,
                       nbr->n, nbr->words, out_dev);
    SAFE_HIP_CHECK(hipGetLastError());
    return SAFE_OK;
}

int safe_nbr_to_dense_i64(safe_nbr *nbr, int64_t *out_host) {
    SAFE_REQUIRE(nbr && out_host, "safe_nbr_to_dense_i64: NULL argument");
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    int64_t *d = nullptr;
    SAFE_TRY(b.alloc(&d, nbr->n * nbr->n));
    SAFE_TRY(safe_nbr_to_dense_i64_dev(nbr, d));
    SAFE_HIP_CHECK_AS("safe_nbr_to_dense_i64", hipMemcpyAsync(out_host, d, nbr->n * nbr->n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK_AS("safe_nbr_to_dense_i64", safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_nbr_row_counts(safe_nbr *nbr, int64_t *out_host) {
    SAFE_REQUIRE(nbr && out_host, "safe_nbr_row_counts: NULL argument");
    for (int64_t i = 0; i < nbr->n; ++i) out_host[i] = nbr->h_row_count[i];
    return SAFE_OK;
}

int safe_nbr_csr(safe_nbr *nbr, int32_t *row_ptr_host, int32_t *col_host) {
    SAFE_REQUIRE(nbr && row_ptr_host && col_host, "safe_nbr_csr: NULL argument");
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_HIP_CHECK(hipMemcpyAsync(row_ptr_host, nbr->row_ptr, (nbr->n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                                  ctx->stream));
    if (nbr->nnz)
        SAFE_HIP_CHECK(hipMemcpyAsync(col_host, nbr->col, nbr->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_nbr_distances(safe_nbr *nbr, double *out_host) {
    SAFE_REQUIRE(nbr && out_host, "safe_nbr_distances: NULL argument");
    SAFE_REQUIRE(nbr->dist != nullptr, "safe_nbr_distances: handle was built without keep_distances");
    safe_ctx *ctx = nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_HIP_CHECK(hipMemcpyAsync(out_host, nbr->dist, nbr->n * nbr->n * sizeof(double), hipMemcpyDeviceToHost,
                                  ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return SAFE_OK;
}

int safe_pair_distance_select_xy(safe_ctx *ctx, const double *xy_host, int64_t n, const int64_t *ranks, int64_t n_ranks,
                                 double *out_host, int64_t *n_pairs) {
    const char *fn = "safe_pair_distance_select_xy";
    SAFE_REQUIRE(ctx && xy_host && n >= 1 && n_ranks >= 0, "%s: bad argument", fn);
    return pair_distance_select(ctx, DistSource{nullptr, nullptr, n}, xy_host, fn, ranks, n_ranks, out_host, n_pairs);
}

int safe_nbr_distance_select(safe_nbr *nbr, const int64_t *ranks, int64_t n_ranks, double *out_host, int64_t *n_finite_pairs) {
    const char *fn = "safe_nbr_distance_select";
    SAFE_REQUIRE(nbr && n_ranks >= 0, "%s: bad argument", fn);
    SAFE_REQUIRE(nbr->dist != nullptr, "%s: handle was built without keep_distances", fn);
    return pair_distance_select(nbr->ctx, DistSource{nullptr, nbr->dist, nbr->n}, nullptr, fn, ranks, n_ranks, out_host, n_finite_pairs);
}

int safe_row_distance_select_xy(safe_ctx *ctx, const double *xy_host, int64_t n, int64_t k, double *radii_out_host) {
    const char *fn = "safe_row_distance_select_xy";
    SAFE_REQUIRE(ctx && xy_host && radii_out_host, "%s: NULL argument", fn);
    SAFE_REQUIRE(n >= 1 && n < (1ll << 31) - 64, "%s: n=%lld out of range", fn, (long long)n);
    return row_distance_select(ctx, DistSource{nullptr, nullptr, n}, xy_host, fn, k, radii_out_host);
}

int safe_nbr_row_distance_select(safe_nbr *nbr, int64_t k, double *radii_out_host) {
    const char *fn = "safe_nbr_row_distance_select";
    SAFE_REQUIRE(nbr && radii_out_host, "%s: NULL argument", fn);
    SAFE_REQUIRE(nbr->dist != nullptr, "%s: handle was built without keep_distances", fn);
    return row_distance_select(nbr->ctx, DistSource{nullptr, nbr->dist, nbr->n}, nullptr, fn, k, radii_out_host);
}

int safe_nbr_euclidean_rows(safe_ctx *ctx, const double *xy_host, int64_t n, const double *radii_host, safe_nbr **out) {
    const char *fn = "safe_nbr_euclidean_rows";
    SAFE_REQUIRE(ctx && xy_host && radii_host && out, "%s: NULL argument", fn);
    *out = nullptr;
    SAFE_REQUIRE(n >= 1 && n < (1ll << 31) - 64, "%s: n=%lld out of range", fn, (long long)n);
    SAFE_TRY(check_radii(fn, radii_host, n));
    std::vector<double> c(n);
    for (int64_t i = 0; i < n; ++i) c[i] = squared_threshold_le(radii_host[i]);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    CallBufs b;                                         // (behind c: the upload reads it)
    const double *d_xy = nullptr;
    double *d_c = nullptr;
    SAFE_TRY(upload_layout(ctx, &b, fn, xy_host, n, &d_xy));
    SAFE_TRY(b.alloc(&d_c, n));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_c, c.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_euclid_bits<true>, dim3(nbr->words, ceil_div(n, 256)), dim3(256), 0, ctx->stream, d_xy, n,
                       static_cast<const double *>(d_c), nbr->bits, nbr->words);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));        // (waits for the stream: the uploads have read xy_host and c)
    nbr->h_xy.assign(xy_host, xy_host + 2 * n);         // node order of the block-sparse form (mfma.hip)
    *out = nbr.release();
    return SAFE_OK;
}

int safe_nbr_from_distances_rows(safe_nbr *src_nbr, const double *radii_host, int keep_distances, safe_nbr **out) {
    const char *fn = "safe_nbr_from_distances_rows";
    SAFE_REQUIRE(src_nbr && radii_host && out, "%s: NULL argument", fn);
    *out = nullptr;
    SAFE_REQUIRE(src_nbr->dist != nullptr, "%s: the source handle was built without keep_distances", fn);
    const int64_t n = src_nbr->n;
    SAFE_TRY(check_radii(fn, radii_host, n));
    safe_ctx *ctx = src_nbr->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    NbrPtr nbr(nullptr, nbr_free);
    SAFE_TRY(nbr_new(ctx, n, &nbr));
    if (keep_distances) SAFE_TRY(dev_alloc(&nbr->dist, n * n));
    CallBufs b;
    double *d_r = nullptr;
    SAFE_TRY(b.alloc(&d_r, n));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_r, radii_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_dist_bits_rows, dim3(n), dim3(256), 0, ctx->stream, src_nbr->dist, n, d_r, nbr->bits, nbr->words,
                       nbr->dist);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_TRY(nbr_finalize_from_bits(nbr.get()));        // (waits for the stream: the upload has read radii_host)
    nbr->h_xy = src_nbr->h_xy;
    *out = nbr.release();
    return SAFE_OK;
}

}  // extern "C"
