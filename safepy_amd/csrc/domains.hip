// The two data-parallel pieces of the consumers of nes_binary:
//
//  * define_top_attributes (safepy/safe.py:631-656): for every candidate attribute, the connected
//    components of the subgraph induced by its enriched nodes (nx.subgraph + nx.connected_components,
//    one Python call per attribute in the reference).  Here: all attributes at once, min-label
//    hooking + pointer jumping over the edge list (Shiloach-Vishkin style); the final label of a
//    node is the smallest node id of its component.
//  * define_top_attributes with attribute_unimodality_metric = 'radius' (additive; safepy/safe.py:632 reads the setting and
//    ignores every value but 'connectivity'): for every candidate attribute the number of its enriched nodes and the number of
//    ordered pairs of them that a membership handle W -- the within-reach relation -- joins: diag(E^T W E) on bit matrices
//    (k_profile_pack<true> + k_pair_count below).
//  * define_domains (safepy/safe.py:672-673): the condensed Jaccard distance vector between the
//    binarised enrichment profiles of the top attributes -- scipy's pdist(m, 'jaccard') inside
//    linkage(): d = #(x != y and (x != 0 or y != 0)) / #(x != 0 or y != 0), 0 when the denominator
//    is 0 -- from bit-packed columns with popcounts.
//  * the linkage of those distances (safepy/safe.py:672: linkage(m, method='average', metric=...)): SciPy's nn_chain restated
//    step for step -- k_linkage_expand + k_linkage_nn_chain below -- so that Z equals SciPy 1.15's bit for bit, ties included.
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
#include <climits>
#include <cmath>
#include <numeric>
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

// bits[w][a] = rows 64 w .. 64 w + 63 of column cols[a] of the row-major [n, m] matrix (non-zero = set; rows >= n: 0).
// ENRICHED: the test is > 0 (NaN, 0, -0.0 and negatives are not set: safepy/safe.py:641) and the words of a column lie
// together, bits[a][w] -- the form k_pair_count walks.
template <bool ENRICHED>
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
    for (int r = 0; r < cnt; ++r) {
        const double v = p[(r0 + r) * m];
        word |= static_cast<unsigned long long>(ENRICHED ? v > 0.0 : v != 0.0) << r;
    }
    bits[ENRICHED ? a * words + w : w * m_top + a] = word;
}

// ---- enriched-pair counts (attribute_unimodality_metric = 'radius') ----
// q[a] += sum over the rows i set in column a of popcount(W[i][:] & column a), e[a] += the number of those rows.
//  * A wave owns one (column a, chunk of PC_CHUNK_WORDS x 64 rows, block of 64 KW words).  Its slice of the column -- KW words
//    per lane, KW = ceil(words / 64) up to PC_MAX_KW, chosen by the host: one block covers the rows of up to 32 768 nodes --
//    stays in registers; the rows of the chunk are walked through the column's own words (wave-uniform: scalar loads, ctz):
//    a row that is not enriched costs nothing beyond finding the next set bit, an enriched one costs KW coalesced 512-byte
//    reads of the row's word block, issued together, and an AND and a popcount per word.  A lane past the last word keeps 0
//    for its slice and reads the row's last word instead of its own (in bounds, no divergence).  Nothing is decided in
//    floating point.
//  * Partial sums are 32-bit per lane (q[a] <= nnz(W) < 2^31: row_ptr is int32), folded with wave shuffles and added to the
//    64-bit q[a] with one atomic per wave: integer adds commute, so the sums are exact in any order.
//  * W may be any bit matrix (asymmetric, empty): this is the raw quadratic form diag(E^T W E).
//  Bound: the stream of W rows, nnz(E) x words x 8 bytes through L2 / the memory-side cache (the bit matrix, 50 MB at 20 000
//  nodes, does not fit an XCD's L2); the integer work -- two ANDs and two 32-bit popcounts per word -- is ~4 lane-operations
//  per 8 bytes and stays below it ("Enriched-pair counts").
constexpr int PC_MAX_KW = 8;                             // most 64-bit words of the column a lane keeps
constexpr int64_t PC_CHUNK_WORDS = 16;                   // words of the column whose rows a wave walks = 1024 rows
template <int KW>
__global__ __launch_bounds__(256) void k_pair_count(const uint64_t *__restrict__ w_bits, int64_t words,
                                                    const unsigned long long *__restrict__ e_bits, int64_t n_cols,
                                                    unsigned long long *__restrict__ q, unsigned long long *__restrict__ e) {
    const int lane = threadIdx.x & 63;
    const int64_t a = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    if (a >= n_cols) return;                                             // (wave-uniform)
    const unsigned long long *col = e_bits + a * words;
    const int64_t wb0 = static_cast<int64_t>(blockIdx.z) * (64 * KW);
    unsigned long long mine[KW];
    int64_t at[KW];
    bool any = false;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int64_t w = wb0 + k * 64 + lane;
        at[k] = w < words ? w : words - 1;
        mine[k] = w < words ? col[w] : 0ull;
        any |= mine[k] != 0ull;
    }
    const bool count_rows = blockIdx.z == 0;                             // e[a] is counted once, by the first word block
    if (!count_rows && __builtin_amdgcn_ballot_w64(any) == 0ull) return; // no enriched node in this block: nothing to add
    const int64_t rw0 = static_cast<int64_t>(blockIdx.y) * PC_CHUNK_WORDS;
    const int64_t rw1 = rw0 + PC_CHUNK_WORDS < words ? rw0 + PC_CHUNK_WORDS : words;
    unsigned int acc = 0, n_rows = 0;
    for (int64_t rw = rw0; rw < rw1; ++rw) {
        unsigned long long rows = col[rw];                               // the same address in every lane
        n_rows += __popcll(rows);
        while (rows) {                                                   // bits of rows >= n are never set (k_profile_pack)
            const int64_t i = rw * 64 + __builtin_ctzll(rows);
            rows &= rows - 1;
            const uint64_t *wr = w_bits + i * words;
            uint64_t v[KW];
#pragma unroll
            for (int k = 0; k < KW; ++k) v[k] = wr[at[k]];
#pragma unroll
            for (int k = 0; k < KW; ++k) acc += __popcll(v[k] & mine[k]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        if (acc) atomicAdd(&q[a], static_cast<unsigned long long>(acc));
        if (count_rows && n_rows) atomicAdd(&e[a], static_cast<unsigned long long>(n_rows));
    }
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

// ---- average linkage (scipy.cluster.hierarchy.linkage(d, 'average') = _hierarchy.nn_chain + a stable sort + a relabel) ----
//
//  * k_linkage_expand: the condensed vector (never modified) becomes a square symmetric f64 working matrix [n, n], so that
//    every nearest-neighbour scan reads one contiguous row.  A workgroup owns a 32 x 32 tile of the upper triangle: it reads
//    its rows' segments of the condensed vector, writes them as they are and, through LDS, transposed.  The same pass raises
//    a flag when a distance is not finite (SciPy refuses such input; `dist < cur` is never true for a NaN).
//  * k_linkage_nn_chain: all n - 1 merges in ONE workgroup of up to 1024 lanes -- no grid-wide synchronisation and no
//    assumption about co-residency.  Uniform state (chain length, chain top x and its predecessor p, merge count) lives in
//    registers of every lane; the chain (16-bit ids) and the live bits are in LDS, the cluster sizes in a small global array.
//    A scan is a strided read of row x with the dead columns masked, a (value, index) minimum that prefers the smaller index
//    (wave shuffles, then one LDS slot per wave; the slots alternate between two sets so that one barrier per scan is enough),
//    and the predecessor compared LAST under SciPy's strict rule: y = p unless the row minimum is < D[x, p].  A merge rewrites
//    row y and column y with the Lance-Williams average (nx * D[i, x] + ny * D[i, y]) / (nx + ny), every operation rounded on
//    its own (-ffp-contract=off), and ends in the one barrier that orders its stores before the next scan.  The sizes of x
//    and p are read with the scan (before its barrier), so the merge that follows may overwrite them without another one.
//    The scans are bounded by 4 n + 64 (the algorithm needs fewer than 3 n): a kernel that cannot hang.
//  Roofline: latency.  A scan is one dependent global read of 8 n bytes spread over the workgroup plus a two-level reduction;
//  the ~3 n scans and n merges run back to back on one CU, the other 255 idle -- the work per step (n values) is too small to
//  pay for a grid-wide barrier ("Domain stage").
constexpr int64_t LINKAGE_MAX_POINTS = SAFE_LINKAGE_MAX_POINTS;
constexpr int LK_THREADS = 1024, LK_UNROLL = 8;
constexpr int LK_BAD_INPUT = 1, LK_OVERFLOW = 2, LK_INTERNAL = 4;
static_assert(LINKAGE_MAX_POINTS <= 65536 / 4 && LINKAGE_MAX_POINTS % 32 == 0, "chain ids are 16-bit, the chain is 32 KB of LDS");

__global__ __launch_bounds__(256) void k_linkage_expand(const double *__restrict__ cond, int64_t n, double *__restrict__ sq,
                                                        int *__restrict__ flag) {
    __shared__ double tile[32][33];
    const int64_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    bool bad = false;
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = bi * 32 + r, j = bj * 32 + tx;
        double v = 0.0;                                                  // the diagonal is never read
        if (i < n && j < n) {
            if (i != j) {
                const int64_t a = i < j ? i : j, b = i < j ? j : i;
                v = cond[a * (2 * n - a - 1) / 2 + (b - a - 1)];       // scipy's condensed index
                bad |= !std::isfinite(v);
            }
            sq[i * n + j] = v;
        }
        tile[r][tx] = v;
    }
    if (bi != bj) {                                                      // (a diagonal tile has read both of its halves itself)
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int64_t j = bj * 32 + r, i = bi * 32 + tx;
            if (i < n && j < n) sq[j * n + i] = tile[tx][r];
        }
    }
    if (bad) atomicOr(flag, LK_BAD_INPUT);
}

__device__ inline void lk_take_smaller(double &v, int &i, double ov, int oi) {
    if (ov < v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// (minimum value, smallest index that attains it) over the workgroup, in every lane; `set` alternates between the two LDS sets
__device__ inline void lk_block_min(double &v, int &i, double (*part_v)[16], int (*part_i)[16], int &set, int waves) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        lk_take_smaller(v, i, ov, oi);
    }
    if (waves == 1) return;
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        part_v[set][threadIdx.x >> 6] = v;
        part_i[set][threadIdx.x >> 6] = i;
    }
    __syncthreads();
    const int slot = lane & 15;
    v = slot < waves ? part_v[set][slot] : INFINITY;
    i = slot < waves ? part_i[set][slot] : INT_MAX;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        lk_take_smaller(v, i, ov, oi);
    }
    set ^= 1;
}

// sq: the working matrix of k_linkage_expand (modified); size: int32 [n] scratch; merges: f64 [n - 1][3] = (x, y, height) in
// merge order, x < y; flag: LK_* bits (a flag that is already set ends the kernel at once)
__global__ __launch_bounds__(LK_THREADS) void k_linkage_nn_chain(double *sq, int n, int *size, double *merges, int *flag) {
    __shared__ unsigned short chain[LINKAGE_MAX_POINTS];
    __shared__ unsigned int live[LINKAGE_MAX_POINTS / 32];
    __shared__ double part_v[2][16];
    __shared__ int part_i[2][16];
    __shared__ int stop;
    const int tid = threadIdx.x, threads = blockDim.x, waves = threads >> 6;
    const int words = (n + 31) >> 5;
    if (*flag) return;
    for (int w = tid; w < words; w += threads) live[w] = (w + 1) * 32 <= n ? 0xffffffffu : (1u << (n & 31)) - 1u;
    for (int i = tid; i < n; i += threads) size[i] = 1;
    if (tid == 0) stop = 0;
    __syncthreads();
    auto is_live = [&](int i) { return (live[i >> 5] >> (i & 31)) & 1u; };

    int len = 0, x = 0, p = -1, first_word = 0, set = 0;
    int64_t scans_left = 4ll * n + 64;
    for (int k = 0; k < n - 1;) {
        if (len == 0) {                                                  // the chain starts at the smallest live index
            while (first_word < words && live[first_word] == 0) ++first_word;
            if (first_word >= words) {
                if (tid == 0) atomicOr(flag, LK_INTERNAL);
                return;
            }
            x = first_word * 32 + __ffs(live[first_word]) - 1;
            p = -1;
            len = 1;
            if (tid == 0) chain[0] = static_cast<unsigned short>(x);
        }
        if (--scans_left < 0) {
            if (tid == 0) atomicOr(flag, LK_INTERNAL);
            return;
        }
        // ---- nearest neighbour of x: the row minimum over the live columns, smallest index first
        const double *row = sq + static_cast<int64_t>(x) * n;
        const double d_xp = p >= 0 ? row[p] : INFINITY;
        const int size_x = size[x], size_p = p >= 0 ? size[p] : 0;
        double best = INFINITY;
        int best_i = INT_MAX;
        for (int base = tid; base < n; base += threads * LK_UNROLL) {
            double v[LK_UNROLL];
#pragma unroll
            for (int u = 0; u < LK_UNROLL; ++u) {
                const int i = base + u * threads;
                v[u] = i < n ? row[i] : INFINITY;
            }
#pragma unroll
            for (int u = 0; u < LK_UNROLL; ++u) {
                const int i = base + u * threads;
                if (i < n && i != x && is_live(i) && v[u] < best) {      // ascending i per lane: strict < keeps the smallest
                    best = v[u];
                    best_i = i;
                }
            }
        }
        lk_block_min(best, best_i, part_v, part_i, set, waves);
        if (best_i == INT_MAX) {                                         // no finite distance left in the row
            if (tid == 0) atomicOr(flag, LK_OVERFLOW);
            return;
        }
        if (p < 0 || best < d_xp) {                                      // someone is strictly closer than the predecessor: push
            if (tid == 0) chain[len] = static_cast<unsigned short>(best_i);
            ++len;
            p = x;
            x = best_i;
            continue;
        }
        // ---- x and p are mutual nearest neighbours at height d_xp: merge the smaller index into the larger
        const int a = x < p ? x : p, b = x < p ? p : x;
        const int na = x < p ? size_x : size_p, nb = x < p ? size_p : size_x;
        const double fa = static_cast<double>(na), fb = static_cast<double>(nb), ft = static_cast<double>(na + nb);
        const double *row_a = sq + static_cast<int64_t>(a) * n;
        double *row_b = sq + static_cast<int64_t>(b) * n;
        bool overflow = false;
        for (int base = tid; base < n; base += threads * LK_UNROLL) {
            double va[LK_UNROLL], vb[LK_UNROLL];
#pragma unroll
            for (int u = 0; u < LK_UNROLL; ++u) {
                const int i = base + u * threads;
                va[u] = i < n ? row_a[i] : 0.0;
                vb[u] = i < n ? row_b[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < LK_UNROLL; ++u) {
                const int i = base + u * threads;
                if (i < n && i != a && i != b && is_live(i)) {
                    const double d = (fa * va[u] + fb * vb[u]) / ft;
                    overflow |= !std::isfinite(d);
                    row_b[i] = d;
                    sq[static_cast<int64_t>(i) * n + b] = d;
                }
            }
        }
        if (overflow) stop = 1;
        if (tid == 0) {
            merges[3 * static_cast<int64_t>(k)] = static_cast<double>(a);
            merges[3 * static_cast<int64_t>(k) + 1] = static_cast<double>(b);
            merges[3 * static_cast<int64_t>(k) + 2] = d_xp;
            size[b] = na + nb;
            live[a >> 5] &= ~(1u << (a & 31));
        }
        __syncthreads();                                                 // row b, column b, size, live bit and chain: visible
        if (stop) {
            if (tid == 0) atomicOr(flag, LK_OVERFLOW);
            return;
        }
        ++k;
        len -= 2;
        x = len >= 1 ? chain[len - 1] : 0;
        p = len >= 2 ? chain[len - 2] : -1;
    }
}

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

// Argument checks shared by safe_profile_distances and safe_profile_linkage (fn names the caller in the messages).
int profile_check(const char *fn, safe_ctx *ctx, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top, int metric,
                  double *kernel_ms) {
    SAFE_REQUIRE(ctx && n >= 1 && m >= 0 && m_top >= 0, "%s: bad argument", fn);
    SAFE_REQUIRE(metric >= SAFE_METRIC_JACCARD && metric <= SAFE_METRIC_YULE, "%s: unknown metric id %d", fn, metric);
    if (kernel_ms) *kernel_ms = 0;
    SAFE_REQUIRE(m_top == 0 || cols_host, "%s: NULL argument", fn);
    for (int64_t c = 0; c < m_top; ++c)
        SAFE_REQUIRE(cols_host[c] >= 0 && cols_host[c] < m, "%s: column %lld out of [0, %lld)", fn, (long long)cols_host[c], (long long)m);
    return SAFE_OK;
}

// Pack + pair kernels of the checked arguments on the context's stream: *d_out (owned by b) receives the condensed distances.
// Starts the timer; the caller stops it behind whatever it enqueues next.
int profile_condensed(const char *fn, safe_ctx *ctx, CallBufs &b, CallTimer &tm, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host,
                      int64_t m_top, int metric, double **d_out) {
    const int64_t words = ceil_div(n, 64), pairs = m_top * (m_top - 1) / 2;
    SAFE_REQUIRE(m_top < 65536 && ceil_div(words, 4) < (1ll << 31), "%s: too many profiles or rows for one launch", fn);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    int64_t *d_cols = nullptr;
    unsigned long long *d_bits = nullptr;
    SAFE_TRY(b.alloc(&d_cols, static_cast<size_t>(m_top)));
    SAFE_TRY(b.alloc(&d_bits, static_cast<size_t>(m_top) * words));
    SAFE_TRY(b.alloc(d_out, static_cast<size_t>(pairs)));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemcpyAsync(d_cols, cols_host, m_top * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK(tm.start(s));
    hipLaunchKernelGGL(k_profile_pack<false>, dim3(static_cast<unsigned>(ceil_div(words, 4)), static_cast<unsigned>(ceil_div(m_top, 64))), dim3(256),
                       0, s, values_dev, n, m, d_cols, m_top, words, d_bits);
    SAFE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_profile_pairs, dim3(static_cast<unsigned>(ceil_div(m_top, 256)), static_cast<unsigned>(m_top)), dim3(256), 0, s,
                       d_bits, m_top, words, n, metric, *d_out);
    SAFE_HIP_CHECK(hipGetLastError());
    return SAFE_OK;
}

int linkage_check_size(const char *fn, int64_t n) {
    if (n > LINKAGE_MAX_POINTS) {
        safe_set_error("%s: %lld points exceed the limit of %lld (an 8 n^2 byte working matrix; 16-bit chain ids in LDS)", fn, (long long)n,
                       (long long)LINKAGE_MAX_POINTS);
        return SAFE_E_UNSUPPORTED;
    }
    return SAFE_OK;
}

// Average linkage of the condensed distances d_cond (device, n >= 2 points, read only) into z_host f64 [n - 1, 4]: expand and
// NN-chain kernels behind what the stream holds (the timer is running: started by the caller, stopped here), then SciPy's
// epilogue on the host -- a stable sort of the merges by height and the union-find relabel (linkage() -> label()).  Synchronises.
// z_host is written only on success.
int linkage_run(const char *fn, safe_ctx *ctx, CallBufs &b, CallTimer &tm, const double *d_cond, int64_t n, const char *kernels, int64_t launches,
                double *z_host, double *kernel_ms) {
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    double *d_sq = nullptr, *d_merges = nullptr;
    int *d_size = nullptr, *d_flag = nullptr;
    SAFE_TRY(b.alloc(&d_sq, static_cast<size_t>(n) * n));
    SAFE_TRY(b.alloc(&d_size, static_cast<size_t>(n)));
    SAFE_TRY(b.alloc(&d_merges, static_cast<size_t>(3 * (n - 1))));
    SAFE_TRY(b.alloc(&d_flag, 1));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), s));
    const unsigned tiles = static_cast<unsigned>(ceil_div(n, 32));
    hipLaunchKernelGGL(k_linkage_expand, dim3(tiles, tiles), dim3(256), 0, s, d_cond, n, d_sq, d_flag);
    SAFE_HIP_CHECK(hipGetLastError());
    const unsigned threads = static_cast<unsigned>(std::min<int64_t>(LK_THREADS, ceil_div(n, 64) * 64));
    hipLaunchKernelGGL(k_linkage_nn_chain, dim3(1), dim3(threads), 0, s, d_sq, static_cast<int>(n), d_size, d_merges, d_flag);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(tm.stop(s));
    int flag = 0;
    std::vector<double> merges(static_cast<size_t>(3 * (n - 1)));
    SAFE_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(hipMemcpyAsync(merges.data(), d_merges, merges.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(tm.finish(ctx, kernels, launches, kernel_ms));
    if (flag) {
        safe_set_error(flag & LK_BAD_INPUT  ? "%s: the distances are not all finite (SciPy's linkage refuses them too)"
                       : flag & LK_OVERFLOW ? "%s: an averaged distance overflowed"
                                            : "%s: the chain did not end (internal error)",
                       fn);
        return SAFE_E_VALUE;
    }
    // np.argsort(Z[:, 2], kind='mergesort'), then label(): row i joins the current clusters of its two points as cluster n + i
    std::vector<int64_t> order(static_cast<size_t>(n - 1));
    std::iota(order.begin(), order.end(), int64_t(0));
    std::stable_sort(order.begin(), order.end(), [&](int64_t u, int64_t v) { return merges[3 * u + 2] < merges[3 * v + 2]; });
    std::vector<int64_t> parent(static_cast<size_t>(2 * n - 1)), count(static_cast<size_t>(2 * n - 1), 1);
    std::iota(parent.begin(), parent.end(), int64_t(0));
    auto find = [&](int64_t v) {
        int64_t root = v;
        while (parent[root] != root) root = parent[root];
        while (parent[v] != root) {
            const int64_t next = parent[v];
            parent[v] = root;
            v = next;
        }
        return root;
    };
    for (int64_t i = 0; i < n - 1; ++i) {
        const double *mg = &merges[3 * order[i]];
        const int64_t u = find(static_cast<int64_t>(mg[0])), v = find(static_cast<int64_t>(mg[1]));
        parent[u] = parent[v] = n + i;
        count[n + i] = count[u] + count[v];
        z_host[4 * i] = static_cast<double>(std::min(u, v));
        z_host[4 * i + 1] = static_cast<double>(std::max(u, v));
        z_host[4 * i + 2] = mg[2];
        z_host[4 * i + 3] = static_cast<double>(count[n + i]);
    }
    return SAFE_OK;
}

// Pack + count kernels of checked arguments on the context's stream into q_host / e_host int64 [n_cols].
// d_values: f64 [n][m] row-major on the device.  Synchronises.
int pair_counts_run(const char *fn, safe_ctx *ctx, CallBufs &b, const safe_nbr *within, const double *d_values, int64_t m,
                    const int64_t *cols_host, int64_t n_cols, int64_t *q_host, int64_t *e_host, double *kernel_ms) {
    const int64_t n = within->n, words = within->words;
    const int kw = static_cast<int>(std::min<int64_t>(ceil_div(words, 64), PC_MAX_KW));      // words of a column per lane
    const int64_t chunks = ceil_div(words, PC_CHUNK_WORDS), blocks = ceil_div(words, 64 * kw);
    SAFE_REQUIRE(ceil_div(n_cols, 4) < (1ll << 31) && ceil_div(n_cols, 64) < 65536 && ceil_div(words, 4) < (1ll << 31) && chunks < 65536 &&
                     blocks < 65536,
                 "%s: too many columns or rows for one launch", fn);
    int64_t *d_cols = nullptr;
    unsigned long long *d_bits = nullptr, *d_qe = nullptr;
    CallTimer tm;
    SAFE_TRY(b.alloc(&d_cols, static_cast<size_t>(n_cols)));
    SAFE_TRY(b.alloc(&d_bits, static_cast<size_t>(n_cols) * words));
    SAFE_TRY(b.alloc(&d_qe, static_cast<size_t>(2 * n_cols)));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_cols, cols_host, n_cols * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_qe, 0, 2 * n_cols * sizeof(unsigned long long), s));
    SAFE_HIP_CHECK_AS(fn, tm.start(s));
    hipLaunchKernelGGL(k_profile_pack<true>, dim3(static_cast<unsigned>(ceil_div(words, 4)), static_cast<unsigned>(ceil_div(n_cols, 64))),
                       dim3(256), 0, s, d_values, n, m, d_cols, n_cols, words, d_bits);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    const dim3 grid(static_cast<unsigned>(ceil_div(n_cols, 4)), static_cast<unsigned>(chunks), static_cast<unsigned>(blocks));
    unsigned long long *d_q = d_qe, *d_e = d_qe + n_cols;
#define PC_LAUNCH(K) \
    case K: hipLaunchKernelGGL(k_pair_count<K>, grid, dim3(256), 0, s, within->bits, words, d_bits, n_cols, d_q, d_e); break
    switch (kw) {
        PC_LAUNCH(1);
        PC_LAUNCH(2);
        PC_LAUNCH(3);
        PC_LAUNCH(4);
        PC_LAUNCH(5);
        PC_LAUNCH(6);
        PC_LAUNCH(7);
    default:
        static_assert(PC_MAX_KW == 8, "one case per KW");
        hipLaunchKernelGGL(k_pair_count<8>, grid, dim3(256), 0, s, within->bits, words, d_bits, n_cols, d_q, d_e);
    }
#undef PC_LAUNCH
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, tm.stop(s));
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied out as int64");
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(q_host, d_q, n_cols * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(e_host, d_e, n_cols * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    SAFE_HIP_CHECK_AS(fn, tm.finish(ctx, "k_profile_pack+k_pair_count", 2, kernel_ms));
    return SAFE_OK;
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
    const char *fn = "safe_enriched_components";
    const int64_t total = n * n_cols;
    hipStream_t s = ctx->stream;
    CallBufs b;
    SAFE_TRY(b.alloc(&d_member, static_cast<size_t>(total)));
    SAFE_TRY(b.alloc(&d_parent, static_cast<size_t>(total)));
    SAFE_TRY(b.alloc(&d_eu, std::max<int64_t>(n_edges, 1)));
    SAFE_TRY(b.alloc(&d_ev, std::max<int64_t>(n_edges, 1)));
    SAFE_TRY(b.alloc(&d_changed, 1));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_member, member_host, static_cast<size_t>(total) * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_edges) {
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_eu, edge_u, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_ev, edge_v, n_edges * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_cc_init, dim3(ceil_div(total, 256)), dim3(256), 0, s, d_member, n, n_cols, d_parent);
    SAFE_HIP_CHECK_AS(fn, cc_rounds(s, d_eu, d_ev, n_edges, n, n_cols, d_parent, d_changed, nullptr));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(labels_host, d_parent, static_cast<size_t>(total) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    return SAFE_OK;
}

int safe_jaccard_condensed(safe_ctx *ctx, int64_t m_top, int64_t n, const double *x_host, double *out_host) {
    SAFE_REQUIRE(ctx && (m_top < 2 || (x_host && out_host)), "safe_jaccard_condensed: NULL argument");
    SAFE_REQUIRE(m_top >= 0 && n >= 1, "safe_jaccard_condensed: bad sizes");
    if (m_top < 2) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t words = ceil_div(n, 64), pairs = m_top * (m_top - 1) / 2;
    double *d_x = nullptr, *d_out = nullptr;
    unsigned long long *d_bits = nullptr;
    const char *fn = "safe_jaccard_condensed";
    hipStream_t s = ctx->stream;
    CallBufs b;
    SAFE_TRY(b.alloc(&d_x, static_cast<size_t>(m_top) * n));
    SAFE_TRY(b.alloc(&d_bits, static_cast<size_t>(m_top) * words));
    SAFE_TRY(b.alloc(&d_out, pairs));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_x, x_host, static_cast<size_t>(m_top) * n * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_jaccard_pack, dim3(ceil_div(words, 4), m_top), dim3(256), 0, s, d_x, m_top, n, words, d_bits);
    hipLaunchKernelGGL(k_jaccard_pairs, dim3(ceil_div(m_top, 256), m_top), dim3(256), 0, s, d_bits, m_top, words, d_out);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(out_host, d_out, pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    return SAFE_OK;
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
    CallBufs b;
    CallTimer tm;
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
    SAFE_HIP_CHECK(tm.start(s));
    int64_t launches = 1;
    hipLaunchKernelGGL(k_cc_init_cols, dim3(static_cast<unsigned>(ceil_div(n, 64)), static_cast<unsigned>(ceil_div(n_cols, 64))), dim3(256),
                       0, s, values_dev, n, m, d_cols, n_cols, d_parent);
    SAFE_HIP_CHECK(hipGetLastError());
    SAFE_HIP_CHECK(cc_rounds(s, d_eu, d_ev, n_edges, n, n_cols, d_parent, d_changed, &launches));
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(labels_host, d_parent, static_cast<size_t>(n) * n_cols * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(tm.finish(ctx, "k_cc_init_cols+k_cc_hook+k_cc_compress", launches, kernel_ms));
    return SAFE_OK;
}

int safe_profile_distances(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top,
                           int metric, double *out_host, double *kernel_ms) {
    const char *fn = "safe_profile_distances";
    SAFE_TRY(profile_check(fn, ctx, n, m, cols_host, m_top, metric, kernel_ms));
    if (m_top < 2) return SAFE_OK;
    SAFE_REQUIRE(values_dev && out_host, "%s: NULL argument", fn);
    CallBufs b;
    CallTimer tm;
    double *d_out = nullptr;
    SAFE_TRY(profile_condensed(fn, ctx, b, tm, values_dev, n, m, cols_host, m_top, metric, &d_out));
    hipStream_t s = ctx->stream;
    SAFE_HIP_CHECK(tm.stop(s));
    SAFE_HIP_CHECK(hipMemcpyAsync(out_host, d_out, m_top * (m_top - 1) / 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK(safe_stream_sync(s));
    SAFE_HIP_CHECK(tm.finish(ctx, "k_profile_pack+k_profile_pairs", 2, kernel_ms));
    return SAFE_OK;
}

int safe_linkage_average(safe_ctx *ctx, const double *cond_dev, int64_t m_top, double *z_host, double *kernel_ms) {
    const char *fn = "safe_linkage_average";
    SAFE_REQUIRE(ctx && m_top >= 0, "%s: bad argument", fn);
    if (kernel_ms) *kernel_ms = 0;
    if (m_top < 2) return SAFE_OK;
    SAFE_REQUIRE(cond_dev && z_host, "%s: NULL argument", fn);
    SAFE_TRY(linkage_check_size(fn, m_top));
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    CallTimer tm;
    SAFE_HIP_CHECK(tm.start(ctx->stream));
    return linkage_run(fn, ctx, b, tm, cond_dev, m_top, "k_linkage_expand+k_linkage_nn_chain", 2, z_host, kernel_ms);
}

int safe_profile_linkage(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top,
                         int metric, double *z_host, double *kernel_ms) {
    const char *fn = "safe_profile_linkage";
    SAFE_TRY(profile_check(fn, ctx, n, m, cols_host, m_top, metric, kernel_ms));
    if (m_top < 2) return SAFE_OK;
    SAFE_REQUIRE(values_dev && z_host, "%s: NULL argument", fn);
    SAFE_TRY(linkage_check_size(fn, m_top));
    CallBufs b;
    CallTimer tm;
    double *d_cond = nullptr;
    SAFE_TRY(profile_condensed(fn, ctx, b, tm, values_dev, n, m, cols_host, m_top, metric, &d_cond));
    return linkage_run(fn, ctx, b, tm, d_cond, m_top, "k_profile_pack+k_profile_pairs+k_linkage_expand+k_linkage_nn_chain", 4, z_host, kernel_ms);
}

int safe_enriched_pair_counts(safe_ctx *ctx, safe_nbr *within, const double *member_host, int64_t n_cols, int64_t *q_host,
                              int64_t *e_host) {
    const char *fn = "safe_enriched_pair_counts";
    SAFE_REQUIRE(ctx && within && n_cols >= 0, "%s: bad argument", fn);
    if (n_cols == 0) return SAFE_OK;
    SAFE_REQUIRE(member_host && q_host && e_host, "%s: NULL argument", fn);
    SAFE_REQUIRE(within->n >= 1 && within->bits, "%s: the membership handle holds no bit matrix", fn);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t total = within->n * n_cols;
    std::vector<int64_t> cols(static_cast<size_t>(n_cols));
    std::iota(cols.begin(), cols.end(), int64_t(0));
    CallBufs b;                                                          // (after cols: see CallBufs)
    double *d_member = nullptr;
    SAFE_TRY(b.alloc(&d_member, static_cast<size_t>(total)));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_member, member_host, static_cast<size_t>(total) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return pair_counts_run(fn, ctx, b, within, d_member, n_cols, cols.data(), n_cols, q_host, e_host, nullptr);
}

int safe_enriched_pair_counts_dev(safe_ctx *ctx, safe_nbr *within, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host,
                                  int64_t n_cols, int64_t *q_host, int64_t *e_host, double *kernel_ms) {
    const char *fn = "safe_enriched_pair_counts_dev";
    SAFE_REQUIRE(ctx && within && n >= 1 && m >= 0 && n_cols >= 0, "%s: bad argument", fn);
    if (kernel_ms) *kernel_ms = 0;
    SAFE_REQUIRE(within->n == n && within->bits, "%s: the matrix has %lld rows, the membership handle %lld", fn, (long long)n,
                 (long long)within->n);
    if (n_cols == 0) return SAFE_OK;
    SAFE_REQUIRE(values_dev && cols_host && q_host && e_host, "%s: NULL argument", fn);
    for (int64_t c = 0; c < n_cols; ++c)
        SAFE_REQUIRE(cols_host[c] >= 0 && cols_host[c] < m, "%s: column %lld out of [0, %lld)", fn, (long long)cols_host[c], (long long)m);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    CallBufs b;
    return pair_counts_run(fn, ctx, b, within, values_dev, m, cols_host, n_cols, q_host, e_host, kernel_ms);
}

}  // extern "C"
