// Hypergeometric test with both tails on gfx950: depletion and two-sided scores for 0/1 attributes.
//
// safe_hypergeom (enrich.hip) computes what the reference computes: pvalues_pos = P[H >= x] and nothing else
// (safepy/safe.py:556-608), whatever attribute_sign says.  safe_hypergeom_tails follows attribute_sign the way the
// randomization route does (safe.py:546-554): per cell the count x = A . nan_to_num(B) (safe.py:593-594), the upper tail
// P[H >= x] = hypergeom.sf(x - 1, N, K, n), the lower tail P[H <= x] = hypergeom.cdf(x, N, K, n) (N, K, n as at
// safe.py:574-590), NES = -log10 of the side the sign names (their difference for 'both'), the binarisation and the
// per-attribute counts (safe.py:468-472).
//
//   counts      safe_score 'sum' (enrich.hip), written into ns
//   evaluators  table: k_hyp_tails_table, one thread per distinct (n, K) pair, pmf relative to the mode in double-double,
//               both tails divided by the total (k_hyp_table's arithmetic, hyp_math.h); cut at the call's largest count
//               per-element: hyp_sf twice per cell, the lower tail by symmetry P[H <= x | N, K, n] = P[H' >= n - x | N, N - K, n]
//   emit        k_hyp_tails_emit: streaming, lanes along columns, 8 B read and 32 B written per cell
//
// Built with -ffp-contract=off like the rest of the library: every fma of the double-double helpers is explicit.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "hyp_math.h"
#include "tails_shared.h"   // k_hyp_tails_nbr_size, tails_nes, k_hyp_tails_u32_to_f64 (also moments.hip)

namespace {

constexpr int TAILS_ROW_TILE = 16;          // rows of an emit block (4 per wave)
constexpr int TAILS_COL_CHUNK = 1024;       // columns of an emit block (16 groups of 64 lanes)
constexpr size_t TAILS_LDS_BYTES = 48 * 1024;   // a size's table slab goes to LDS up to here

// the call's largest count (whole numbers >= 0 as f64): the table stops there
__global__ __launch_bounds__(256) void k_hyp_tails_max(const double *__restrict__ ns, int64_t total, unsigned int *__restrict__ xmax) {
    unsigned int v = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * 256) {
        const double x = ns[i];
        const unsigned int u = x >= 1.0 ? (x < 4294967295.0 ? static_cast<unsigned int>(x) : 4294967295u) : 0u;
        v = u > v ? u : v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned int o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(xmax, v);
}

// tab[nid][x][kid] = (P[H >= x], P[H <= x]) for H ~ Hypergeom(pop, K = kvals[kid], n = nvals[nid]), x = 0 .. xs-1, with the
// support rules of scipy's rv_discrete: upper tail 1 at or below the bottom of the support and 0 above its top, lower tail 0
// below the support and 1 at or above its top.  One thread per (n, K) pair; the arithmetic is k_hyp_table's (enrich.hip): the
// pmf RELATIVE to its value at the mode in double-double, every tail divided by the sum over the whole support.  The upper
// tail is summed from the top down, the lower tail from the bottom up (smallest terms first on either side).  Unlike
// k_hyp_table the downward recurrence goes on until a term underflows to 0: a deep lower tail consists of exactly the terms
// that are negligible beside the total.  `terms` [same shape] holds the relative pmf between the passes.
__global__ __launch_bounds__(64) void k_hyp_tails_table(const int32_t *__restrict__ nvals, int64_t n_nid,
                                                        const int32_t *__restrict__ kvals, int64_t n_kid, int64_t xs, int64_t pop,
                                                        double2 *__restrict__ terms, double2 *__restrict__ tab) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (idx >= n_nid * n_kid) return;
    const int64_t draws = nvals[idx / n_kid], good = kvals[idx % n_kid];
    const int64_t base = (idx / n_kid) * xs * n_kid + idx % n_kid;       // layout [size id][x][count id], as k_hyp_table
    double2 *t_base = terms + base, *o_base = tab + base;
#define t_term(t) t_base[(t) * n_kid]
#define t_out(t) o_base[(t) * n_kid]
    const int64_t lo = draws - (pop - good) > 0 ? draws - (pop - good) : 0;
    const int64_t hi = good < draws ? good : draws;
    const double good_d = static_cast<double>(good), draws_d = static_cast<double>(draws);
    const double rest_d = static_cast<double>(pop) - good_d - draws_d;
    int64_t mode = static_cast<int64_t>(floor(static_cast<double>(good + 1) * static_cast<double>(draws + 1) / static_cast<double>(pop + 2)));
    mode = mode < lo ? lo : (mode > hi ? hi : mode);
    // terms at or beyond xs are only summed (`beyond`); once such a term is below 1e-40 of `beyond` the rest of the upper side
    // adds nothing to any quantity at double-double precision (k_hyp_table)
    dd_t beyond{0.0, 0.0}, total{0.0, 0.0}, term{1.0, 0.0};
    double td = static_cast<double>(mode);
    for (int64_t t = mode; t <= hi; ++t) {                              // upwards from the mode
        if (t < xs) t_term(t) = make_double2(term.hi, term.lo);
        else beyond = dd_add(beyond, term);
        total = dd_add(total, term);
        if (t >= xs && (term.hi == 0.0 || term.hi < beyond.hi * 1e-40)) break;
        term = dd_mul_d(dd_mul_d(term, good_d - td), draws_d - td);
        term = dd_div_d(dd_div_d(term, td + 1.0), rest_d + td + 1.0);
        td += 1.0;
    }
    term = dd_t{1.0, 0.0};
    td = static_cast<double>(mode);
    int64_t t_stop = lo;                                                // terms below t_stop have underflowed to 0
    for (int64_t t = mode - 1; t >= lo; --t) {                          // downwards from the mode
        term = dd_mul_d(dd_mul_d(term, td), rest_d + td);
        term = dd_div_d(dd_div_d(term, good_d - td + 1.0), draws_d - td + 1.0);
        td -= 1.0;
        if (!(term.hi > 0.0)) {
            t_stop = t + 1;
            break;
        }
        if (t < xs) t_term(t) = make_double2(term.hi, term.lo);
        else beyond = dd_add(beyond, term);
        total = dd_add(total, term);
    }
    dd_t running = beyond;
    for (int64_t t = xs - 1; t >= 0; --t) {                             // upper tails, from the top down
        double p;
        if (t > hi) {
            p = 0.0;                                                    // sf(x - 1) with x - 1 >= top of the support
        } else if (t <= lo) {
            p = 1.0;                                                    // x - 1 below the support
        } else {
            if (t >= t_stop) running = dd_add(running, dd_t{t_term(t).x, t_term(t).y});
            p = dd_ratio(running, total);
            p = p > 1.0 ? 1.0 : p;
        }
        t_out(t).x = p;
    }
    running = dd_t{0.0, 0.0};
    for (int64_t t = 0; t < xs; ++t) {                                  // lower tails, from the bottom up
        double p;
        if (t < lo) {
            p = 0.0;                                                    // cdf below the support
        } else if (t >= hi) {
            p = 1.0;                                                    // at or above its top
        } else {
            if (t >= t_stop) running = dd_add(running, dd_t{t_term(t).x, t_term(t).y});
            p = dd_ratio(running, total);
            p = p > 1.0 ? 1.0 : p;
        }
        t_out(t).y = p;
    }
#undef t_term
#undef t_out
}

struct TailsEmit {
    const double *ns;           // [n][mloc] counts
    int64_t n, mloc;
    // table evaluator
    const int32_t *order;       // [n] rows sorted by size id (a tile of one size shares an LDS slab)
    const int32_t *nid;         // [n]
    const int32_t *kid;         // [mloc]
    const double2 *tab;         // [n_nid][xs][n_kid] of (p_pos, p_neg)
    int64_t n_kid, xs;
    int slab_lds;               // 1: a size's slab (xs * n_kid entries) fits the block's LDS
    // per-element evaluator
    const double *size;         // [n] neighborhood sizes
    const double *col_sum;      // [mloc] annotation counts of the call's columns
    const double *lf;           // log-factorial table [pop + 2]
    double pop;
    // NES and binarisation
    int sign_mode;
    double p_cut, nes_threshold;
    double *pvalues_neg, *pvalues_pos, *nes, *nes_binary;
    unsigned int *enriched;     // [mloc]
};

// A block = TAILS_ROW_TILE rows (positions of `order` for the table evaluator) x TAILS_COL_CHUNK columns; a wave takes every
// fourth row of the tile, its lanes 64 adjacent columns.  Per-column enriched counts: one atomic per wave and column group.
template <bool TABLE>
__global__ __launch_bounds__(256) void k_hyp_tails_emit(const TailsEmit e) {
    extern __shared__ double2 tails_slab[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * TAILS_ROW_TILE;
    const int64_t r1 = r0 + TAILS_ROW_TILE < e.n ? r0 + TAILS_ROW_TILE : e.n;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * TAILS_COL_CHUNK;
    const int64_t c1 = c0 + TAILS_COL_CHUNK < e.mloc ? c0 + TAILS_COL_CHUNK : e.mloc;
    bool lds = false;
    if (TABLE) {
        const int32_t nid_first = e.nid[e.order[r0]], nid_last = e.nid[e.order[r1 - 1]];
        lds = e.slab_lds && nid_first == nid_last;                       // (block-uniform: rows are sorted by size id)
        if (lds) {
            const double2 *src = e.tab + static_cast<int64_t>(nid_first) * e.xs * e.n_kid;
            for (int64_t k = threadIdx.x; k < e.xs * e.n_kid; k += 256) tails_slab[k] = src[k];
            __syncthreads();
        }
    }
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int64_t c = cb + lane;
        const bool live = c < c1;
        unsigned int hits = 0;
        int32_t kid = 0;
        double good = 0.0;
        if (live) {
            if (TABLE) kid = e.kid[c];
            else good = e.col_sum[c];
        }
        for (int64_t pos = r0 + wave; pos < r1; pos += 4) {
            const int64_t row = TABLE ? static_cast<int64_t>(e.order[pos]) : pos;
            if (!live) continue;
            const int64_t o = row * e.mloc + c;
            const double x = e.ns[o];
            double pp, pn;
            if (TABLE) {
                int64_t xi = x >= 0.0 ? static_cast<int64_t>(x) : 0;        // (always 0 <= x <= the call's largest count < xs)
                xi = xi < e.xs ? xi : e.xs - 1;
                const double2 v = lds ? tails_slab[xi * e.n_kid + kid]
                                      : e.tab[(static_cast<int64_t>(e.nid[row]) * e.xs + xi) * e.n_kid + kid];
                pp = v.x;
                pn = v.y;
            } else {
                const double draws = e.size[row];
                pp = hyp_sf(e.lf, x, e.pop, good, draws);                               // P[H >= x]
                pn = hyp_sf(e.lf, draws - x, e.pop, e.pop - good, draws);               // P[H <= x] = P[H' >= n - x], H' the zeros drawn
            }
            double nes;
            const bool hit = tails_nes(pp, pn, e.sign_mode, e.p_cut, e.nes_threshold, &nes);
            e.pvalues_pos[o] = pp;
            e.pvalues_neg[o] = pn;
            e.nes[o] = nes;
            e.nes_binary[o] = hit ? 1.0 : 0.0;
            hits += hit;
        }
        if (hits) atomicAdd(&e.enriched[c], hits);
    }
}

// NES / binarisation / counts from two p matrices (after the FDR adjustment): 64 columns x 64 rows per block
__global__ __launch_bounds__(256) void k_hyp_tails_outputs(const double *__restrict__ p_neg, const double *__restrict__ p_pos,
                                                           int64_t n, int64_t m, int sign_mode, double p_cut, double nes_threshold,
                                                           double *__restrict__ nes_out, double *__restrict__ nes_binary,
                                                           unsigned int *__restrict__ enriched) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x & 63);
    const int64_t i0 = static_cast<int64_t>(blockIdx.y) * 64 + (threadIdx.x >> 6);
    if (c >= m) return;
    unsigned int hits = 0;
    for (int64_t i = i0; i < n && i < (static_cast<int64_t>(blockIdx.y) + 1) * 64; i += 4) {
        const int64_t o = i * m + c;
        double nes;
        const bool hit = tails_nes(p_pos[o], p_neg[o], sign_mode, p_cut, nes_threshold, &nes);
        nes_out[o] = nes;
        nes_binary[o] = hit ? 1.0 : 0.0;
        hits += hit;
    }
    if (hits) atomicAdd(&enriched[c], hits);
}

// distinct whole values of v[0 .. count) in [0, pop] -> dense ids in order of first appearance; false if a value is not one
bool dense_ids(const double *v, int64_t count, int64_t pop, std::vector<int32_t> &id_of, std::vector<int32_t> &vals,
               std::vector<int32_t> &ids, int64_t *max_val) {
    std::fill(id_of.begin(), id_of.end(), -1);
    *max_val = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (!(v[i] >= 0.0) || v[i] > static_cast<double>(pop) || v[i] != std::floor(v[i])) return false;
        const int32_t iv = static_cast<int32_t>(v[i]);
        if (id_of[iv] < 0) {
            id_of[iv] = static_cast<int32_t>(vals.size());
            vals.push_back(iv);
        }
        ids[i] = id_of[iv];
        *max_val = std::max<int64_t>(*max_val, iv);
    }
    return true;
}

}  // namespace

extern "C" {

int safe_hypergeom_tails(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold, int evaluator,
                         int64_t col0, int64_t col1, double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev,
                         double *nes_dev, double *nes_binary_dev, double *num_enriched_dev) {
    const char *who = "safe_hypergeom_tails";
    SAFE_REQUIRE(ctx && ns_dev && pvalues_neg_dev && pvalues_pos_dev && nes_dev && nes_binary_dev && num_enriched_dev, "%s: NULL argument", who);
    SAFE_REQUIRE(nbr && attr, "%s: NULL handle", who);
    SAFE_REQUIRE(nbr->n == attr->n, "%s: membership is %lld x %lld but the attribute matrix has %lld rows", who, (long long)nbr->n,
                 (long long)nbr->n, (long long)attr->n);
    SAFE_REQUIRE(0 <= col0 && col0 < col1 && col1 <= attr->m, "%s: column range [%lld,%lld) outside [0,%lld)", who, (long long)col0,
                 (long long)col1, (long long)attr->m);
    SAFE_REQUIRE(sign_mode >= SAFE_SIGN_HIGHEST && sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", who, sign_mode);
    SAFE_REQUIRE(enrichment_threshold > 0.0 && enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", who);
    SAFE_REQUIRE(evaluator >= 0 && evaluator <= 2, "%s: bad evaluator %d (0 = choose, 1 = table, 2 = per-element)", who, evaluator);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    SAFE_TRY(safe_attr_prepare(attr));
    if (attr->n_other != 0) {                                             // before anything is launched
        safe_set_error("%s: the attribute matrix holds %lld values other than 0, 1 and NaN (both tails are defined for 0/1 data)", who,
                       (long long)attr->n_other);
        return SAFE_E_VALUE;
    }
    const int64_t n = nbr->n, mloc = col1 - col0, pop = attr->n_rows_with_value;
    hipStream_t s = ctx->stream;
    std::vector<double> lf;                                               // (host memory an upload reads: declared before the CallBufs)
    CallBufs bufs;

    // counts x = A . nan_to_num(B) (safe.py:593-594) through the 'sum' score; it returns once its kernels have ended
    SAFE_TRY(safe_score(ctx, nbr, attr, SAFE_SCORE_SUM, col0, col1, ns_dev));

    void *small = nullptr;                                                // d_size f64 [n] | d_enr u32 [mloc] | xmax u32 (+ padding)
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_TAILS_SMALL, static_cast<size_t>(n) * sizeof(double) + static_cast<size_t>(mloc + 16) * sizeof(unsigned int), &small));
    double *d_size = static_cast<double *>(small);
    unsigned int *d_enr = reinterpret_cast<unsigned int *>(d_size + n), *d_xmax = d_enr + mloc;
    SAFE_HIP_CHECK_AS(who, hipMemsetAsync(d_enr, 0, (mloc + 16) * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_hyp_tails_nbr_size, dim3(ceil_div(n, 4)), dim3(256), 0, s, nbr->row_ptr, nbr->col, attr->row_flags, n, d_size);
    hipLaunchKernelGGL(k_hyp_tails_max, dim3(std::min<int64_t>(ceil_div(n * mloc, 256), 4096)), dim3(256), 0, s, ns_dev, n * mloc, d_xmax);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    // pinned staging: [neighborhood sizes | column sums | largest count] coming back, then the ids going up
    void *pinned = nullptr;
    const size_t down_bytes = static_cast<size_t>(n + mloc + 1) * sizeof(double);
    const size_t up_bytes = static_cast<size_t>(3 * n + 2 * mloc + 8) * sizeof(int32_t);
    SAFE_TRY(ctx_pinned(ctx, down_bytes + up_bytes, &pinned));
    double *h_size = static_cast<double *>(pinned), *h_k = h_size + n;
    unsigned int *h_xmax = reinterpret_cast<unsigned int *>(h_k + mloc);
    int32_t *up = reinterpret_cast<int32_t *>(static_cast<char *>(pinned) + down_bytes);
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(h_size, d_size, n * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(h_k, attr->col_sum + col0, mloc * sizeof(double), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(h_xmax, d_xmax, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));

    // distinct sizes and annotation counts -> dense ids (whole numbers in [0, pop] for 0/1 data)
    std::vector<int32_t> id_of(std::max<int64_t>(pop, n) + 2, -1), nvals, kvals, nid(n), kid(mloc);
    int64_t max_n = 0, max_k = 0;
    if (!dense_ids(h_size, n, pop, id_of, nvals, nid, &max_n) || !dense_ids(h_k, mloc, pop, id_of, kvals, kid, &max_k)) {
        safe_set_error("%s: a neighborhood size or an annotation count is not a whole number in [0, %lld]", who, (long long)pop);
        return SAFE_E_VALUE;
    }
    const int64_t xs = std::min<int64_t>(std::min(max_n, max_k), static_cast<int64_t>(*h_xmax)) + 1;   // x <= min(K, n), cut at the largest count
    const int64_t n_nid = static_cast<int64_t>(nvals.size()), n_kid = static_cast<int64_t>(kvals.size());
    // the acceptance rule of hypergeom_fused (enrich.hip): the table <= 512 MB, and at least 4 cells per distinct (n, K) pair
    const double table_bytes = static_cast<double>(n_nid) * n_kid * xs * sizeof(double2);
    const bool table_ok = table_bytes <= 512e6 && static_cast<double>(n_nid) * n_kid * 4.0 <= static_cast<double>(n) * mloc;
    if (evaluator == 1 && !table_ok) {
        safe_set_error("%s: the table evaluator declines this call (%lld sizes x %lld counts x %lld values of x for %lld cells)", who,
                       (long long)n_nid, (long long)n_kid, (long long)xs, (long long)(n * mloc));
        return SAFE_E_UNSUPPORTED;
    }
    const bool table = evaluator == 1 || (evaluator == 0 && table_ok);

    TailsEmit e{};
    e.ns = ns_dev;
    e.n = n;
    e.mloc = mloc;
    e.sign_mode = sign_mode;
    e.p_cut = nes_p_cut(enrichment_threshold);
    e.nes_threshold = -std::log10(enrichment_threshold);
    e.pvalues_neg = pvalues_neg_dev;
    e.pvalues_pos = pvalues_pos_dev;
    e.nes = nes_dev;
    e.nes_binary = nes_binary_dev;
    e.enriched = d_enr;
    const dim3 grid(ceil_div(n, TAILS_ROW_TILE), ceil_div(mloc, TAILS_COL_CHUNK));
    if (table) {
        const size_t entries = static_cast<size_t>(n_nid) * n_kid * xs;
        double2 *d_tab = nullptr, *d_terms = nullptr;
        int32_t *d_ids = nullptr;
        SAFE_TRY(ctx_scratch(ctx, SCRATCH_TAILS_TABLE, entries * sizeof(double2), reinterpret_cast<void **>(&d_tab)));
        SAFE_TRY(ctx_scratch(ctx, SCRATCH_TAILS_TERMS, entries * sizeof(double2), reinterpret_cast<void **>(&d_terms)));
        SAFE_TRY(ctx_scratch(ctx, SCRATCH_TAILS_IDS, static_cast<size_t>(n_nid + n_kid + 2 * n + mloc) * sizeof(int32_t), reinterpret_cast<void **>(&d_ids)));
        // d_ids = [nvals | kvals | nid | kid | order]: one copy out of the pinned block; order = rows sorted by size id
        int32_t *h_order = up + n_nid + n_kid + n + mloc;
        for (int64_t i = 0; i < n; ++i) h_order[i] = static_cast<int32_t>(i);
        std::stable_sort(h_order, h_order + n, [&](int32_t a, int32_t b) { return nid[a] < nid[b]; });
        memcpy(up, nvals.data(), n_nid * sizeof(int32_t));
        memcpy(up + n_nid, kvals.data(), n_kid * sizeof(int32_t));
        memcpy(up + n_nid + n_kid, nid.data(), n * sizeof(int32_t));
        memcpy(up + n_nid + n_kid + n, kid.data(), mloc * sizeof(int32_t));
        SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_ids, up, static_cast<size_t>(n_nid + n_kid + 2 * n + mloc) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_hyp_tails_table, dim3(ceil_div(n_nid * n_kid, 64)), dim3(64), 0, s, d_ids, n_nid, d_ids + n_nid, n_kid, xs, pop,
                           d_terms, d_tab);
        SAFE_HIP_CHECK_AS(who, hipGetLastError());
        e.nid = d_ids + n_nid + n_kid;
        e.kid = e.nid + n;
        e.order = e.kid + mloc;
        e.tab = d_tab;
        e.n_kid = n_kid;
        e.xs = xs;
        const size_t slab_bytes = static_cast<size_t>(xs) * n_kid * sizeof(double2);
        // the slab pays when a block reads it less often than it looks up: at most half as many entries as the block has cells
        e.slab_lds = slab_bytes <= TAILS_LDS_BYTES &&
                     static_cast<size_t>(xs) * n_kid * 2 <= static_cast<size_t>(TAILS_ROW_TILE) * std::min<int64_t>(mloc, TAILS_COL_CHUNK);
        if (e.slab_lds)
            SAFE_HIP_CHECK_AS(who, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hyp_tails_emit<true>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(TAILS_LDS_BYTES)));
        SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));
        hipLaunchKernelGGL(k_hyp_tails_emit<true>, grid, dim3(256), e.slab_lds ? slab_bytes : 0, s, e);
        ctx->last_kernel.name = "k_hyp_tails_emit<table>";
    } else {
        // pmf from a log-factorial table lf[k] = log(k!), k = 0 .. pop + 1 (safe_hypergeom's per-element form)
        lf.resize(std::max<int64_t>(pop, n) + 2);
        for (size_t k = 0; k < lf.size(); ++k) lf[k] = std::lgamma(static_cast<double>(k) + 1.0);
        double *d_lf = nullptr;
        SAFE_TRY(bufs.alloc(&d_lf, lf.size()));
        SAFE_HIP_CHECK_AS(who, hipMemcpyAsync(d_lf, lf.data(), lf.size() * sizeof(double), hipMemcpyHostToDevice, s));
        e.size = d_size;
        e.col_sum = attr->col_sum + col0;
        e.lf = d_lf;
        e.pop = static_cast<double>(pop);
        SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k0, s));
        hipLaunchKernelGGL(k_hyp_tails_emit<false>, grid, dim3(256), 0, s, e);
        ctx->last_kernel.name = "k_hyp_tails_emit<element>";
    }
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, hipEventRecord(ctx->k1, s));
    hipLaunchKernelGGL(k_hyp_tails_u32_to_f64, dim3(ceil_div(mloc, 256)), dim3(256), 0, s, d_enr, num_enriched_dev, mloc);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(s));                          // the id vectors and lf are host memory; the call has finished when it returns
    float ms = 0.f;
    SAFE_HIP_CHECK_AS(who, hipEventElapsedTime(&ms, ctx->k0, ctx->k1));
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = ms;
    ctx->last_kernel.launches = 1;
    ctx->last_kernel.summed = false;
    return SAFE_OK;
}

int safe_hypergeom_outputs(safe_ctx *ctx, int64_t n, int64_t m, int sign_mode, double enrichment_threshold, const double *pvalues_neg_dev,
                           const double *pvalues_pos_dev, double *nes_dev, double *nes_binary_dev, double *num_enriched_dev) {
    const char *who = "safe_hypergeom_outputs";
    SAFE_REQUIRE(ctx && pvalues_neg_dev && pvalues_pos_dev && nes_dev && nes_binary_dev && num_enriched_dev, "%s: NULL argument", who);
    SAFE_REQUIRE(n >= 1 && m >= 1, "%s: bad sizes", who);
    SAFE_REQUIRE(sign_mode >= SAFE_SIGN_HIGHEST && sign_mode <= SAFE_SIGN_BOTH, "%s: bad sign_mode %d", who, sign_mode);
    SAFE_REQUIRE(enrichment_threshold > 0.0 && enrichment_threshold < 1.0, "%s: enrichment_threshold must be in (0,1)", who);
    SAFE_HIP_CHECK(hipSetDevice(ctx->device));
    void *small = nullptr;
    SAFE_TRY(ctx_scratch(ctx, SCRATCH_TAILS_SMALL, static_cast<size_t>(m + 16) * sizeof(unsigned int), &small));
    unsigned int *d_enr = static_cast<unsigned int *>(small);
    SAFE_HIP_CHECK_AS(who, hipMemsetAsync(d_enr, 0, (m + 16) * sizeof(unsigned int), ctx->stream));
    hipLaunchKernelGGL(k_hyp_tails_outputs, dim3(ceil_div(m, 64), ceil_div(n, 64)), dim3(256), 0, ctx->stream, pvalues_neg_dev, pvalues_pos_dev,
                       n, m, sign_mode, nes_p_cut(enrichment_threshold), -std::log10(enrichment_threshold), nes_dev, nes_binary_dev, d_enr);
    hipLaunchKernelGGL(k_hyp_tails_u32_to_f64, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream, d_enr, num_enriched_dev, m);
    SAFE_HIP_CHECK_AS(who, hipGetLastError());
    SAFE_HIP_CHECK_AS(who, safe_stream_sync(ctx->stream));                // the call has finished when it returns, like safe_fdr_adjust
    return SAFE_OK;
}

}  // extern "C"
