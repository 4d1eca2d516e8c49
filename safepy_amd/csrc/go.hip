// Gene-to-term annotations propagated up an is_a DAG, on the device: direct (locus, term) pairs in, the CSC of the
// propagated 0/1 matrix out (safe_go_create / safe_go_read), or that matrix itself as a safe_attr (safe_go_as_attr).
//
// Restates the contract of safepy/utils/make_go.py ("a matrix of gene-to-term annotations (propagated)", :18-26, built by
// :247-289): cell (locus, term) = 1 iff the locus is annotated to the term or to any DESCENDANT of it; terms without a locus
// are dropped (:273-275); loci without a term go to the root (:277-280).  On a DAG the reference's store_predecessors_all
// (:206-229) keeps only the ancestors along the path of its last visit; this file computes the full ancestor set.
//
// The state is a bit matrix [n_terms][W] of 32-bit words: row t holds the loci of term t, bit (r & 31) of word (r >> 5) is
// locus r.  W = ceil(n_rows / 32) rounded up to a multiple of 4, so that every row starts on a 16-byte boundary and the level
// kernel moves four words per lane and load; bits at and beyond n_rows (the padding words included) are never set.
//
//   k_go_scatter   one lane per annotation pair, atomicOr of its bit (duplicates are harmless)
//   k_go_level     one launch per level from 1 upwards (leaves are level 0, a term is 1 + the maximum over its children,
//                  Kahn's algorithm on the host).  A workgroup is GO_LEVEL_WAVES = 8 waves (512 threads, 8 KB of LDS) over
//                  the SAME GO_CHUNK_WORDS adjacent words of one term's row; a lane owns four of them (one 16-byte load), so a
//                  child row is read in coalesced 1 KiB pieces, GO_UNROLL loads in flight, and every output word has one owner:
//                  nothing needs an atomic.  Up to GO_SPLIT_FROM = 16 children wave 0 ORs them into the term's row alone and
//                  the other seven waves leave at once; beyond, wave v takes children v, v + 8, ... and wave 0 ORs the eight
//                  partial rows together through LDS before it stores.  The choice is uniform per workgroup (it depends on
//                  the term alone): a hub with thousands of children is a loop an eighth as long, a 200-level chain is 200
//                  short launches, same kernel, no list of special terms from the host.
//   k_go_count     one wave per term, lanes along the words: population count of the row
//   k_go_any       OR over all rows per word (a workgroup: GO_CHUNK_WORDS words x GO_ANY_TERMS terms, then atomicOr)
//   k_go_root      per word: loci in no row and not missing get the root's bit; their number is counted
//   k_pairs_scan   (pairs.hip) exclusive scans of the column lengths (the pointer array) and of the kept flags
//   k_go_compact   kept term k -> its index and indptr[k]
//   k_go_emit      one wave per kept term: the set bits of its row as ascending int32 locus indices; a lane's place is the
//                  column's base + the words before its step + the prefix of the population counts inside the wave, so the
//                  output is the same bytes for the same input.
#include "common.h"

namespace {

constexpr int GO_THREADS = 256;
constexpr int GO_WAVES = GO_THREADS / SAFE_WAVE;
constexpr int GO_LEVEL_WAVES = 8;                            // k_go_level: waves of a workgroup, all over the same words
constexpr int GO_LEVEL_THREADS = GO_LEVEL_WAVES * SAFE_WAVE;
constexpr int GO_CHUNK_WORDS = 4 * SAFE_WAVE;                // words of a row one workgroup of k_go_level / k_go_any covers (8192 loci): four per lane
constexpr int GO_SPLIT_FROM = 16;                            // more children than this: the waves of the workgroup share them
static_assert(GO_CHUNK_WORDS == GO_THREADS, "k_go_any: one word per thread of a GO_THREADS workgroup covers the same chunk");
constexpr int GO_UNROLL = 8;                                 // child rows whose loads are issued together
constexpr int GO_ANY_TERMS = 64;                             // rows a workgroup of k_go_any folds before its atomicOr
constexpr int64_t GO_INT32_END = int64_t(1) << 31;

__global__ __launch_bounds__(GO_THREADS) void k_go_scatter(const int32_t *__restrict__ row, const int32_t *__restrict__ term, int64_t n_ann,
                                                           int64_t n_rows, int64_t n_terms, int64_t W, uint32_t *__restrict__ bits) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * GO_THREADS + threadIdx.x;
    if (i >= n_ann) return;
    const int64_t r = row[i], t = term[i];
    if (r < 0 || r >= n_rows || t < 0 || t >= n_terms) return;   // (checked on the host; guarded all the same)
    atomicOr(&bits[t * W + (r >> 5)], 1u << (r & 31));
}

// level[i], i = 0 .. n_level - 1: the terms of this level; workgroup b: term level[b / chunks], words (b % chunks) * GO_CHUNK_WORDS ...
// W is a multiple of 4 and bits is 16-byte aligned: rows are addressed as uint4.
__global__ __launch_bounds__(GO_LEVEL_THREADS) void k_go_level(const int32_t *__restrict__ level, int64_t chunks,
                                                               const int32_t *__restrict__ child_ptr, const int32_t *__restrict__ child_idx,
                                                               int64_t n_terms, int64_t W, uint32_t *__restrict__ bits) {
    __shared__ uint4 s_part[GO_LEVEL_WAVES][SAFE_WAVE];
    const int lane = threadIdx.x % SAFE_WAVE, wave = threadIdx.x / SAFE_WAVE;
    const int64_t b = blockIdx.x;
    const int64_t t = level[b / chunks];
    if (t < 0 || t >= n_terms) return;                        // (the whole workgroup)
    const int64_t W4 = W >> 2, q = (b % chunks) * SAFE_WAVE + lane;                    // quad q = words 4 q .. 4 q + 3
    const int32_t c0 = child_ptr[t], c1 = child_ptr[t + 1];
    const bool split = c1 - c0 > GO_SPLIT_FROM;               // (the same for every wave of the workgroup)
    if (!split && wave != 0) return;
    const bool active = q < W4;
    uint4 *rows = reinterpret_cast<uint4 *>(bits);
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    if (active) {
        if (wave == 0) acc = rows[t * W4 + q];
        const int32_t step = split ? GO_LEVEL_WAVES : 1;
        int32_t c = c0 + (split ? wave : 0);
        for (; c < c1 - (GO_UNROLL - 1) * step; c += GO_UNROLL * step) {
            uint4 v[GO_UNROLL];
#pragma unroll
            for (int u = 0; u < GO_UNROLL; ++u) {
                const int64_t k = child_idx[c + u * step];
                v[u] = (k >= 0 && k < n_terms) ? rows[k * W4 + q] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < GO_UNROLL; ++u) acc.x |= v[u].x, acc.y |= v[u].y, acc.z |= v[u].z, acc.w |= v[u].w;
        }
        for (; c < c1; c += step) {
            const int64_t k = child_idx[c];
            if (k >= 0 && k < n_terms) {
                const uint4 v = rows[k * W4 + q];
                acc.x |= v.x, acc.y |= v.y, acc.z |= v.z, acc.w |= v.w;
            }
        }
    }
    if (split) {
        s_part[wave][lane] = acc;
        __syncthreads();                                      // (every wave of the workgroup is here: split is uniform)
        if (wave != 0) return;
#pragma unroll
        for (int v = 1; v < GO_LEVEL_WAVES; ++v) {
            const uint4 p = s_part[v][lane];
            acc.x |= p.x, acc.y |= p.y, acc.z |= p.z, acc.w |= p.w;
        }
    }
    if (active) rows[t * W4 + q] = acc;
}

// count[first + i] = set bits of row first + i, i = 0 .. n - 1 (one wave each)
__global__ __launch_bounds__(GO_THREADS) void k_go_count(const uint32_t *__restrict__ bits, int64_t first, int64_t n, int64_t W,
                                                         int32_t *__restrict__ count) {
    const int lane = threadIdx.x % SAFE_WAVE;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * GO_WAVES + threadIdx.x / SAFE_WAVE;
    if (i >= n) return;                                       // (the whole wave)
    const uint32_t *row = bits + (first + i) * W;
    int sum = 0;
    for (int64_t w = lane; w < W; w += SAFE_WAVE) sum += __popc(row[w]);
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) count[first + i] = sum;
}

// any[w] |= OR of bits[t][w] over the workgroup's GO_ANY_TERMS terms (any is zero before the launch)
__global__ __launch_bounds__(GO_THREADS) void k_go_any(const uint32_t *__restrict__ bits, int64_t chunks, int64_t n_terms, int64_t W,
                                                       uint32_t *__restrict__ any) {
    const int64_t b = blockIdx.x;
    const int64_t t0 = (b / chunks) * GO_ANY_TERMS, t1 = min(n_terms, t0 + GO_ANY_TERMS);
    const int64_t w = (b % chunks) * GO_CHUNK_WORDS + threadIdx.x;
    if (w >= W) return;
    uint32_t acc = 0;
#pragma unroll 8
    for (int64_t t = t0; t < t1; ++t) acc |= bits[t * W + w];
    if (acc) atomicOr(&any[w], acc);
}

// loci of word w that no row holds and that are not missing: set in the root's row; assigned += their number
__global__ __launch_bounds__(GO_THREADS) void k_go_root(const uint32_t *__restrict__ any, const uint8_t *__restrict__ missing, int64_t n_rows,
                                                        int64_t W, int64_t root, uint32_t *__restrict__ bits, int32_t *__restrict__ assigned) {
    const int64_t w = static_cast<int64_t>(blockIdx.x) * GO_THREADS + threadIdx.x;
    if (w >= W) return;
    const int64_t r0 = w * 32, left = n_rows - r0;
    uint32_t open = left >= 32 ? 0xFFFFFFFFu : left > 0 ? ((1u << left) - 1u) : 0u;      // (left <= 0: a padding word)
    open &= ~any[w];
    if (missing && open) {
        for (int b = 0; b < 32 && r0 + b < n_rows; ++b)
            if (missing[r0 + b]) open &= ~(1u << b);
    }
    if (open) {
        bits[root * W + w] |= open;
        atomicAdd(assigned, __popc(open));
    }
}

__global__ __launch_bounds__(GO_THREADS) void k_go_flags(const int32_t *__restrict__ count, int64_t n_terms, int32_t *__restrict__ kept) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GO_THREADS + threadIdx.x;
    if (t < n_terms) kept[t] = count[t] > 0;
}

// pos / offs: exclusive scans of kept / count over the terms.  Kept term t is column pos[t]: kept_idx, indptr; the totals
// (columns, entries, loci given to the root) go to totals[0 .. 2].
__global__ __launch_bounds__(GO_THREADS) void k_go_compact(const int32_t *__restrict__ kept, const int64_t *__restrict__ pos,
                                                           const int64_t *__restrict__ offs, const int32_t *__restrict__ assigned, int64_t n_terms,
                                                           int32_t *__restrict__ kept_idx, int64_t *__restrict__ indptr,
                                                           int64_t *__restrict__ totals) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GO_THREADS + threadIdx.x;
    if (t < n_terms && kept[t]) {
        const int64_t k = pos[t];
        if (k >= 0 && k < n_terms) {
            kept_idx[k] = static_cast<int32_t>(t);
            indptr[k] = offs[t];
        }
    }
    if (t == 0) {
        const int64_t n_kept = pos[n_terms];
        if (n_kept >= 0 && n_kept <= n_terms) indptr[n_kept] = offs[n_terms];
        totals[0] = n_kept;
        totals[1] = offs[n_terms];
        totals[2] = assigned[0];
    }
}

// one wave per term with a locus: indices[offs[t] .. offs[t + 1]) = the set bits of its row, ascending
__global__ __launch_bounds__(GO_THREADS) void k_go_emit(const uint32_t *__restrict__ bits, const int32_t *__restrict__ count,
                                                        const int64_t *__restrict__ offs, int64_t n_terms, int64_t W, int64_t nnz,
                                                        int32_t *__restrict__ indices) {
    const int lane = threadIdx.x % SAFE_WAVE;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GO_WAVES + threadIdx.x / SAFE_WAVE;
    if (t >= n_terms || count[t] <= 0) return;                // (the whole wave)
    const uint32_t *row = bits + t * W;
    const int64_t base = offs[t], limit = min(offs[t + 1], nnz);
    int64_t running = 0;
    for (int64_t w0 = 0; w0 < W; w0 += SAFE_WAVE) {
        const int64_t w = w0 + lane;
        uint32_t word = w < W ? row[w] : 0u;
        const int mine = __popc(word);
        int incl = mine;
        for (int o = 1; o < SAFE_WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        int64_t at = base + running + (incl - mine);
        while (word) {
            const int b = __ffs(word) - 1;
            word &= word - 1u;
            if (at >= 0 && at < limit) indices[at] = static_cast<int32_t>(w * 32 + b);
            ++at;
        }
        running += __shfl(incl, SAFE_WAVE - 1);
    }
}

// waits for the stream when the scope ends: host vectors that asynchronous copies read are declared in front of it
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)safe_stream_sync(s); }
};

inline size_t go_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace

struct safe_go {
    safe_ctx *ctx = nullptr;
    int64_t n_rows = 0, n_terms = 0, n_kept = 0, nnz = 0, n_root_assigned = 0, n_levels = 0;
    int64_t *indptr = nullptr;      // [n_terms + 1], the first n_kept + 1 in use
    int32_t *kept = nullptr;        // [n_terms], the first n_kept in use: indices of the kept terms, ascending
    int32_t *indices = nullptr;     // [nnz]
    uint8_t *missing = nullptr;     // [n_rows] or NULL
    double pass_ms[SAFE_GO_PASSES] = {};
};

static void go_free(safe_go *g) {
    if (!g) return;
    (void)dev_free(g->indptr);
    (void)dev_free(g->kept);
    (void)dev_free(g->indices);
    (void)dev_free(g->missing);
    delete g;
}

extern "C" {

int safe_go_create(safe_ctx *ctx, int64_t n_rows, int64_t n_terms, const int32_t *child_ptr, const int32_t *child_idx, int64_t n_ann,
                   const int32_t *ann_row, const int32_t *ann_term, int64_t root, const uint8_t *missing_rows, safe_go **out,
                   int64_t *n_kept, int64_t *nnz, int64_t *num_root_assigned, double *kernel_ms) {
    SAFE_REQUIRE(ctx && out && n_kept && nnz && num_root_assigned && child_ptr, "safe_go_create: NULL argument");
    SAFE_REQUIRE(n_ann == 0 || (ann_row && ann_term), "safe_go_create: %lld annotation pairs without arrays", (long long)n_ann);
    const char *fn = "safe_go_create";
    // ---- every refusal, before anything is allocated or launched --------------------------------------------------
    if (n_rows < 1 || n_terms < 1 || n_ann < 0 || n_rows >= GO_INT32_END || n_terms >= GO_INT32_END || n_ann >= GO_INT32_END) {
        safe_set_error("%s: n_rows = %lld, n_terms = %lld, %lld annotation pairs: each must be below 2^31, rows and terms at least 1", fn,
                       (long long)n_rows, (long long)n_terms, (long long)n_ann);
        return SAFE_E_VALUE;
    }
    if (root < 0 || root >= n_terms) {
        safe_set_error("%s: root index %lld outside [0, %lld)", fn, (long long)root, (long long)n_terms);
        return SAFE_E_VALUE;
    }
    if (child_ptr[0] != 0) {
        safe_set_error("%s: child_ptr[0] is not 0", fn);
        return SAFE_E_VALUE;
    }
    for (int64_t t = 0; t < n_terms; ++t)
        if (child_ptr[t + 1] < child_ptr[t]) {
            safe_set_error("%s: child_ptr decreases at term %lld", fn, (long long)t);
            return SAFE_E_VALUE;
        }
    const int64_t n_edges = child_ptr[n_terms];
    SAFE_REQUIRE(n_edges == 0 || child_idx, "safe_go_create: %lld edges without child_idx", (long long)n_edges);
    for (int64_t e = 0; e < n_edges; ++e)
        if (child_idx[e] < 0 || child_idx[e] >= n_terms) {
            safe_set_error("%s: child index %d (edge %lld) outside [0, %lld)", fn, child_idx[e], (long long)e, (long long)n_terms);
            return SAFE_E_VALUE;
        }
    for (int64_t i = 0; i < n_ann; ++i) {
        if (ann_row[i] < 0 || ann_row[i] >= n_rows || ann_term[i] < 0 || ann_term[i] >= n_terms) {
            safe_set_error("%s: annotation %lld = (row %d, term %d) outside [0, %lld) x [0, %lld)", fn, (long long)i, ann_row[i], ann_term[i],
                           (long long)n_rows, (long long)n_terms);
            return SAFE_E_VALUE;
        }
        if (missing_rows && missing_rows[ann_row[i]]) {
            safe_set_error("%s: annotation %lld lies on row %d, which missing_rows marks as absent from the annotations", fn, (long long)i,
                           ann_row[i]);
            return SAFE_E_VALUE;
        }
    }
    // Kahn's algorithm from the leaves: pending[t] = children of t not yet levelled; a term is ready once it reaches 0, and its
    // level is 1 + the largest level among its children.  order = the terms by level, level_off = where each level starts.
    std::vector<int32_t> pending(static_cast<size_t>(n_terms)), level(static_cast<size_t>(n_terms), 0), order;
    std::vector<int32_t> par_ptr(static_cast<size_t>(n_terms) + 1, 0), par_idx(static_cast<size_t>(n_edges));
    for (int64_t e = 0; e < n_edges; ++e) ++par_ptr[static_cast<size_t>(child_idx[e]) + 1];
    for (int64_t t = 0; t < n_terms; ++t) par_ptr[t + 1] += par_ptr[t];
    {
        std::vector<int32_t> fill(par_ptr.begin(), par_ptr.end() - 1);
        for (int64_t t = 0; t < n_terms; ++t)
            for (int32_t e = child_ptr[t]; e < child_ptr[t + 1]; ++e) par_idx[fill[child_idx[e]]++] = static_cast<int32_t>(t);
    }
    order.reserve(static_cast<size_t>(n_terms));
    for (int64_t t = 0; t < n_terms; ++t) {
        pending[t] = child_ptr[t + 1] - child_ptr[t];
        if (pending[t] == 0) order.push_back(static_cast<int32_t>(t));
    }
    for (size_t head = 0; head < order.size(); ++head) {
        const int32_t c = order[head];
        for (int32_t e = par_ptr[c]; e < par_ptr[c + 1]; ++e) {
            const int32_t p = par_idx[e];
            level[p] = std::max(level[p], level[c] + 1);
            if (--pending[p] == 0) order.push_back(p);
        }
    }
    if (static_cast<int64_t>(order.size()) != n_terms) {
        safe_set_error("%s: the is_a edges hold a cycle (%lld of %lld terms could be ordered)", fn, (long long)order.size(), (long long)n_terms);
        return SAFE_E_VALUE;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return level[a] < level[b]; });
    std::vector<int64_t> level_off;
    for (int64_t i = 0; i < n_terms; ++i)
        if (i == 0 || level[order[i]] != level[order[i - 1]]) level_off.push_back(i);
    level_off.push_back(n_terms);
    const int64_t n_levels = static_cast<int64_t>(level_off.size()) - 1;
    const int64_t W = ceil_div(n_rows, 128) * 4, chunks = ceil_div(W, GO_CHUNK_WORDS);   // words per row: whole 16-byte quads
    int64_t widest = 0;
    for (int64_t l = 1; l < n_levels; ++l) widest = std::max(widest, level_off[l + 1] - level_off[l]);
    if (widest * chunks >= GO_INT32_END || ceil_div(n_terms, GO_ANY_TERMS) * chunks >= GO_INT32_END) {
        safe_set_error("%s: %lld terms x %lld rows are too many cells for one launch", fn, (long long)n_terms, (long long)n_rows);
        return SAFE_E_UNSUPPORTED;
    }

    // ---- device ---------------------------------------------------------------------------------------------------
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::unique_ptr<safe_go, void (*)(safe_go *)> g(new safe_go, go_free);
    g->ctx = ctx, g->n_rows = n_rows, g->n_terms = n_terms, g->n_levels = n_levels;
    const size_t nt = static_cast<size_t>(n_terms);
    // SCRATCH_GO_WORK, carved: ann_row | ann_term | child_ptr | child_idx | order | count | kept flags | offs | pos | any | assigned | totals
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t at = off;
        off += go_align(bytes);
        return at;
    };
    const size_t o_row = carve(static_cast<size_t>(n_ann) * 4), o_term = carve(static_cast<size_t>(n_ann) * 4), o_cptr = carve((nt + 1) * 4),
                 o_cidx = carve(static_cast<size_t>(n_edges) * 4), o_order = carve(nt * 4), o_count = carve(nt * 4), o_flag = carve(nt * 4),
                 o_offs = carve((nt + 1) * 8), o_pos = carve((nt + 1) * 8), o_any = carve(static_cast<size_t>(W) * 4), o_asg = carve(4),
                 o_tot = carve(3 * 8);
    void *work_v = nullptr, *bits_v = nullptr, *pinned = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_GO_WORK, off, &work_v));
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_GO_BITS, nt * static_cast<size_t>(W) * 4, &bits_v));
    SAFE_TRY(ctx_pinned(ctx, 64, &pinned));
    SAFE_TRY(dev_alloc(&g->indptr, nt + 1));
    SAFE_TRY(dev_alloc(&g->kept, nt));
    if (missing_rows) SAFE_TRY(dev_alloc(&g->missing, static_cast<size_t>(n_rows)));
    hipEvent_t *ev = nullptr;
    SAFE_TRY(ctx_events(ctx, true, SAFE_GO_PASSES + 2, &ev));   // ev[p], ev[p + 1] bracket pass p < 5; ev[6], ev[7] the emit pass
    uint8_t *work = static_cast<uint8_t *>(work_v);
    uint32_t *bits = static_cast<uint32_t *>(bits_v);
    int32_t *d_row = reinterpret_cast<int32_t *>(work + o_row), *d_term = reinterpret_cast<int32_t *>(work + o_term);
    int32_t *d_cptr = reinterpret_cast<int32_t *>(work + o_cptr), *d_cidx = reinterpret_cast<int32_t *>(work + o_cidx);
    int32_t *d_order = reinterpret_cast<int32_t *>(work + o_order), *d_count = reinterpret_cast<int32_t *>(work + o_count);
    int32_t *d_flag = reinterpret_cast<int32_t *>(work + o_flag), *d_asg = reinterpret_cast<int32_t *>(work + o_asg);
    int64_t *d_offs = reinterpret_cast<int64_t *>(work + o_offs), *d_pos = reinterpret_cast<int64_t *>(work + o_pos);
    int64_t *d_tot = reinterpret_cast<int64_t *>(work + o_tot);
    uint32_t *d_any = reinterpret_cast<uint32_t *>(work + o_any);
    auto blocks = [](int64_t items, int64_t per) { return dim3(static_cast<unsigned>(std::max<int64_t>(ceil_div(items, per), 1))); };

    StreamDrain drain{s};                                     // (behind the host vectors above: they outlive the copies)
    if (n_ann) {
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_row, ann_row, static_cast<size_t>(n_ann) * 4, hipMemcpyHostToDevice, s));
        SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_term, ann_term, static_cast<size_t>(n_ann) * 4, hipMemcpyHostToDevice, s));
    }
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_cptr, child_ptr, (nt + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_edges) SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_cidx, child_idx, static_cast<size_t>(n_edges) * 4, hipMemcpyHostToDevice, s));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(d_order, order.data(), nt * 4, hipMemcpyHostToDevice, s));
    if (missing_rows) SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(g->missing, missing_rows, static_cast<size_t>(n_rows), hipMemcpyHostToDevice, s));
    // pass 0: zero + scatter
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[0], s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(bits, 0, nt * static_cast<size_t>(W) * 4, s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_any, 0, static_cast<size_t>(W) * 4, s));
    SAFE_HIP_CHECK_AS(fn, hipMemsetAsync(d_asg, 0, 4, s));
    if (n_ann) {
        hipLaunchKernelGGL(k_go_scatter, blocks(n_ann, GO_THREADS), dim3(GO_THREADS), 0, s, d_row, d_term, n_ann, n_rows, n_terms, W, bits);
        SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    }
    // pass 1: the closure, level by level
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[1], s));
    for (int64_t l = 1; l < n_levels; ++l) {
        const int64_t n_level = level_off[l + 1] - level_off[l];
        hipLaunchKernelGGL(k_go_level, dim3(static_cast<unsigned>(n_level * chunks)), dim3(GO_LEVEL_THREADS), 0, s, d_order + level_off[l], chunks,
                           d_cptr, d_cidx, n_terms, W, bits);
        SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    }
    // pass 2: loci per term
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(k_go_count, blocks(n_terms, GO_WAVES), dim3(GO_THREADS), 0, s, bits, int64_t(0), n_terms, W, d_count);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    // pass 3: loci without a term -> the root
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(k_go_any, dim3(static_cast<unsigned>(ceil_div(n_terms, GO_ANY_TERMS) * chunks)), dim3(GO_THREADS), 0, s, bits, chunks,
                       n_terms, W, d_any);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    hipLaunchKernelGGL(k_go_root, blocks(W, GO_THREADS), dim3(GO_THREADS), 0, s, d_any, g->missing, n_rows, W, root, bits, d_asg);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    hipLaunchKernelGGL(k_go_count, dim3(1), dim3(GO_THREADS), 0, s, bits, root, int64_t(1), W, d_count);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    // pass 4: kept flags, the two scans, the pointer array
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[4], s));
    hipLaunchKernelGGL(k_go_flags, blocks(n_terms, GO_THREADS), dim3(GO_THREADS), 0, s, d_count, n_terms, d_flag);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, pairs_scan_launch(s, d_count, n_terms, d_offs));
    SAFE_HIP_CHECK_AS(fn, pairs_scan_launch(s, d_flag, n_terms, d_pos));
    hipLaunchKernelGGL(k_go_compact, blocks(n_terms, GO_THREADS), dim3(GO_THREADS), 0, s, d_flag, d_pos, d_offs, d_asg, n_terms, g->kept,
                       g->indptr, d_tot);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[5], s));
    SAFE_HIP_CHECK_AS(fn, hipMemcpyAsync(pinned, d_tot, 3 * 8, hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    int64_t tot[3];
    std::memcpy(tot, pinned, sizeof(tot));
    if (tot[0] < 0 || tot[0] > n_terms || tot[1] < 0) {
        safe_set_error("%s: inconsistent totals from the device (%lld columns, %lld entries)", fn, (long long)tot[0], (long long)tot[1]);
        return SAFE_E_HIP;
    }
    if (tot[1] >= GO_INT32_END) {
        safe_set_error("%s: %lld stored entries do not fit 32-bit indices (nnz must be below 2^31)", fn, (long long)tot[1]);
        return SAFE_E_UNSUPPORTED;
    }
    g->n_kept = tot[0], g->nnz = tot[1], g->n_root_assigned = tot[2];
    // pass 5: the row indices of every kept column
    SAFE_TRY(dev_alloc(&g->indices, static_cast<size_t>(g->nnz)));
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[6], s));
    hipLaunchKernelGGL(k_go_emit, blocks(n_terms, GO_WAVES), dim3(GO_THREADS), 0, s, bits, d_count, d_offs, n_terms, W, g->nnz, g->indices);
    SAFE_HIP_CHECK_AS(fn, hipGetLastError());
    SAFE_HIP_CHECK_AS(fn, hipEventRecord(ev[7], s));
    SAFE_HIP_CHECK_AS(fn, safe_stream_sync(s));
    double total_ms = 0;
    for (int p = 0; p < SAFE_GO_PASSES; ++p) {
        float f = 0;
        SAFE_HIP_CHECK_AS(fn, hipEventElapsedTime(&f, ev[p < 5 ? p : 6], ev[p < 5 ? p + 1 : 7]));
        g->pass_ms[p] = f;
        total_ms += f;
    }
    ctx->last_kernel.name = "k_go_level";
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = g->pass_ms[1];
    ctx->last_kernel.launches = std::max<int64_t>(n_levels - 1, 0);
    ctx->last_kernel.summed = true;
    if (kernel_ms) *kernel_ms = total_ms;
    *n_kept = g->n_kept;
    *nnz = g->nnz;
    *num_root_assigned = g->n_root_assigned;
    *out = g.release();
    return SAFE_OK;
}

int safe_go_read(safe_go *go, int64_t *indptr_host, int32_t *indices_host, int32_t *kept_host, int64_t *num_root_assigned) {
    SAFE_REQUIRE(go && indptr_host, "safe_go_read: NULL argument");
    SAFE_REQUIRE(go->nnz == 0 || indices_host, "safe_go_read: indices_host is NULL");
    SAFE_REQUIRE(go->n_kept == 0 || kept_host, "safe_go_read: kept_host is NULL");
    safe_ctx *ctx = go->ctx;
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_memcpy_d2h(ctx, indptr_host, go->indptr, static_cast<size_t>(go->n_kept + 1) * sizeof(int64_t)));
    if (go->nnz) SAFE_TRY(safe_memcpy_d2h(ctx, indices_host, go->indices, static_cast<size_t>(go->nnz) * sizeof(int32_t)));
    if (go->n_kept) SAFE_TRY(safe_memcpy_d2h(ctx, kept_host, go->kept, static_cast<size_t>(go->n_kept) * sizeof(int32_t)));
    if (num_root_assigned) *num_root_assigned = go->n_root_assigned;
    return SAFE_OK;
}

int safe_go_as_attr(safe_go *go, safe_attr **out) {
    SAFE_REQUIRE(go && out, "safe_go_as_attr: NULL argument");
    SAFE_REQUIRE(go->n_kept >= 1, "safe_go_as_attr: no term is left (every row is missing): there is no matrix to make");
    return attr_create_csc(go->ctx, go->n_rows, go->n_kept, go->nnz, go->indptr, go->indices, nullptr, SAFE_DTYPE_F32, go->missing, true, out);
}

int safe_go_pass_ms(safe_go *go, double *ms, int64_t *n_levels) {
    SAFE_REQUIRE(go && ms, "safe_go_pass_ms: NULL argument");
    for (int p = 0; p < SAFE_GO_PASSES; ++p) ms[p] = go->pass_ms[p];
    if (n_levels) *n_levels = go->n_levels;
    return SAFE_OK;
}

int safe_go_destroy(safe_go *go) {
    if (!go) return SAFE_OK;
    SAFE_HIP_CHECK(hipSetDevice(go->ctx->device));
    SAFE_HIP_CHECK(safe_stream_sync(go->ctx->stream));
    go_free(go);
    return SAFE_OK;
}

}  // extern "C"
