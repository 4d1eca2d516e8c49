// Internal declarations shared by the translation units of libsafe_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "safe_hip.h"
#include "bits_plan.h"   // BitsQueues, BitsTaskPlan, ceil_div: the host-only planning arithmetic of the bit-sliced launch

#define SAFE_WAVE 64
#define SAFE_PAD_U16 0xFFFFu

void safe_set_error(const char *fmt, ...);
// SAFE_HIP_TRACE=1: host-side time stamps (ms since the first call) on stderr
void safe_trace(const char *what);

// hipStreamSynchronize, or a sleeping wait on a blocking event when blocking waits are on (ctx.hip)
hipError_t safe_stream_sync(hipStream_t s);
// flags for events the host may wait on: adds hipEventBlockingSync while blocking waits are on
unsigned safe_event_flags(unsigned base);
bool safe_blocking_sync_selected();
// A diagnostic switch that makes a kernel skip work (timing experiments: SAFE_HIP_BITS_DBG, SAFE_HIP_MFMA_DBG*) is in effect: says so
// on stderr, once per switch -- results of such a run are WRONG by construction and must not be mistaken for the product's.
void safe_warn_diagnostic(const char *name);
bool safe_hidden_regs_checked();                // buildinfo.cpp: the build's disassembly check of the id-stream registers passed   // blocking (sleeping) host waits are on: do not spin

#define SAFE_HIP_CHECK(expr)                                                                   \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            safe_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                           __LINE__);                                                          \
            return SAFE_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

#define SAFE_REQUIRE(cond, ...)                                                                \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            safe_set_error(__VA_ARGS__);                                                       \
            return SAFE_E_INVALID;                                                             \
        }                                                                                      \
    } while (0)

#define SAFE_TRY(expr)                                                                         \
    do {                                                                                       \
        int _rc = (expr);                                                                      \
        if (_rc != SAFE_OK) return _rc;                                                        \
    } while (0)

struct safe_perms;

struct KernelStat {
    std::string name;
    double total_ms = 0.0;
    int64_t launches = 0;
    double busy_ms = 0.0;           // union of the launches' intervals (consecutive launches overlap on two streams); 0 = not measured
    bool summed = false;            // the launches' own events were summed (kernel_stat_from_events): k0 / k1 do not apply
};

struct safe_perms;
// The context's draw thread (rng.cpp): one persistent host thread runs the sequential part of every seeded stream of the
// context (np.random.seed / np.random.permutation, safepy/safe_extras.py:46,58).  A thread created per call started on whatever
// idle core the scheduler found -- clock and caches cold -- and one step in twenty drew 1.5-2 x slower; the persistent thread
// spins briefly for its next job before it sleeps, so back-to-back calls never pay a wake-up either.
struct DrawWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;                 // job posted / worker idle again
    std::atomic<safe_perms *> job{nullptr};     // posted, not yet taken
    bool busy = false;                          // (under mu) a job is running
    bool quit = false;
};
void draw_worker_shutdown(safe_ctx *ctx);

// The context's grow-only scratch buffers (ctx_scratch): one line per slot -- what lives there | who takes it | how long the
// contents must survive.  A slot with several users holds one ROLE: those users never run at the same time, and sharing keeps a
// single allocation of the largest size.  A new buffer gets a new enumerator in front of N_SCRATCH, not a free-looking old one.
enum ScratchSlot {
    SCRATCH_COUNTERS,       // packed u32 counters [mloc][n_pad] | every integer-counter route: bits_call_buffers, launch_lds_f64 (enrich.hip),
                            //   mfma_make_plan (mfma.hip) | until the next integer-counter call: ctx->packed_counts points here
    SCRATCH_OPERANDS,       // the attribute operand: bit planes (uint2), f64 tiles, block-sparse i8 planes (d_bs) | launch_bits,
                            //   launch_counts_bits, launch_lds_f64, hypergeom_fused (enrich.hip), counts_setup, mfma_prepare_columns
                            //   (mfma.hip) | within the call
    SCRATCH_F64_MATRIX,     // one f64 [n][mloc] matrix -- observed scores nobody asked for (launch_lds_f64, launch_mfma_run), the hits of
                            //   safe_hypergeom's per-element form -- or hypergeom_fused's (p, -log10 p) table | within the call
    SCRATCH_TASKS,          // task lists + queue offsets and counters | bits_call_buffers (enrich.hip), counts_setup, mfma_make_plan (mfma.hip) |
                            //   within the call
    SCRATCH_STREAM_A,       // double buffer, even launches: permuted member ids (bits_call_buffers), permuted source rows (mfma_make_plan);
                            //   or counts_setup's one source-row list | within the call
    SCRATCH_STREAM_B,       // ... odd launches; or the split count form's u16 counts (mfma_counts_split_begin) | within the call
    SCRATCH_COLUMN_META,    // per-column side data: hypergeom_fused's distinct (n, K) values and ids (enrich.hip), mfma_prepare_columns'
                            //   column statistics (mfma.hip) | within the call
    SCRATCH_BITS_OBSERVED,  // observed sums of every (word group, slice) of the blocked bit-sliced kernel | bits_observe | within the call
    SCRATCH_SPLIT_ROWS,     // row lists + tasks of the split count form's second half | mfma_counts_split_rows | within the call
    SCRATCH_HYP_SMALL,      // neighborhood sizes f64 [n] | enriched counters u32 [mloc + 64] | safe_hypergeom | within the call
    SCRATCH_ENRICHED,       // enriched counters u32 [m + 16] | safe_randomization, safe_outputs_from_counts | within the call
    SCRATCH_ATTR_STATS,     // accumulators | row bitmap | column counts of the statistics sweep | safe_attr_prepare (attr.hip) | within the call
    SCRATCH_MFMA_OBS64,     // filtered 'sum' form: exact fixed-point observed scores i64 [n_pad][mloc] | mfma_make_plan | within the call
    SCRATCH_MFMA_AMB_A,     // double buffer, even launches: the filtered form's undecided compares | mfma_make_plan | within the call
    SCRATCH_MFMA_AMB_B,     // ... odd launches
    SCRATCH_MFMA_FILTER,    // source-row ids | per-launch counts of undecided compares | mfma_make_plan | within the call
    SCRATCH_MFMA_Q64,       // filtered 'sum' form: the fixed-point values as i64 [n + 1][mloc] | mfma_prepare_columns | within the call
    SCRATCH_MFMA_Z64,       // filtered z form: value | square + not-NaN flag [n + 1][mloc] | mfma_prepare_columns | within the call
    SCRATCH_BITS_TAIL_IDS,  // permuted member ids of the column-chunked exchange tail | bits_call_buffers | within the call
    SCRATCH_NES_TABLE,      // the NES table f64 [P + 1] | ctx_nes_table alone, for safe_randomization and every safe_outputs_from_* entry
                            //   point | ACROSS calls: the device copy of ctx->nes_tab_host, uploaded again only when the table changes
    SCRATCH_ATTR_STAGED,    // the bytes of a u8 attribute matrix as they came | safe_attr_create_host (attr.hip) | within the call
    SCRATCH_HYP_DUMMY,      // 64 write-only f64 for the padding rows / columns of branch-free epilogues (HypLookup::dummy) |
                            //   hypergeom_fused | within the call
    SCRATCH_FDR_FLAG,       // one u32 flag | the count-ratio check and the count forms of the safe_fdr_adjust* entry points (with_flag, fdr.hip) | within the call
    SCRATCH_TAILS_SMALL,    // neighborhood sizes f64 [n] | enriched counters u32 [mloc] | largest count u32 | safe_hypergeom_tails,
                            //   safe_hypergeom_outputs (hyptails.hip) | within the call
    SCRATCH_TAILS_TABLE,    // the (p_pos, p_neg) table [sizes][x][counts] | safe_hypergeom_tails | within the call
    SCRATCH_TAILS_TERMS,    // the relative pmf (hi, lo) of the same shape between the passes of k_hyp_tails_table | within the call
    SCRATCH_TAILS_IDS,      // distinct (n, K) values, row / column ids, rows sorted by size id | safe_hypergeom_tails | within the call
    SCRATCH_MOMENTS_SMALL,  // neighborhood sizes f64 [n] | row factors f64 [n] | column means f64 [mloc] | centred sums of squares f64
                            //   [mloc] | enriched counters u32 [mloc + 16] | safe_moments_test, safe_attr_column_moments (moments.hip) |
                            //   within the call
    SCRATCH_MOMENTS_PARTS,  // per (row chunk, column) partial sum of squares | min | max, f64 [3][chunks][mloc] | k_col_moments ->
                            //   k_col_moments_fold (moments.hip) | within the call
    SCRATCH_GO_BITS,        // the (term x locus) bit matrix u32 [n_terms][W] | safe_go_create (go.hip) | within the call
    SCRATCH_GO_WORK,        // annotation pairs | children CSR | level order | per-term counts, flags, offsets | per-word OR |
                            //   readback words | safe_go_create | within the call
    SCRATCH_FDR_SCOPE,      // 64-bit histogram [P + 1] | adjusted values f64 [P + 1] | u32 flags of the whole-matrix count form |
                            //   safe_fdr_adjust_scope, safe_fdr_adjust_matrix (fdr.hip) | within the call
    SCRATCH_WEIGHT_INPUTS,  // radii f64 [n] | layout f64 [n][2] | safe_nbr_weights_from_xy, safe_nbr_weights_from_distances (weights.hip) |
                            //   within the call
    SCRATCH_WEIGHT_ROWS,    // weight sums W1 f64 [n] | row factors g f64 [n] | column means f64 [mloc] | centred sums of squares f64
                            //   [mloc] | enriched counters u32 [mloc + 16] | safe_moments_test_weighted (weights.hip) | within the call
    SCRATCH_WEIGHT_TILES,   // the attribute operand of the weighted permutation kernel: f64 tiles [tile][n + 1][16] |
                            //   safe_permtest_counts_weighted, and the weighted score of row-contiguous storage (weights.hip) |
                            //   within the call
    SCRATCH_DIFFUSION_GRAPH,// CSR of the network: row starts i32 [n + 1] | neighbor ids i32 [entries] | entry weights, then the scaled entries
                            //   s_ik, f64 [entries] | row scales r f64 [n] | rows by descending entry count i32 [n] | safe_nbr_diffusion
                            //   (diffusion.hip) | within the call
    SCRATCH_MAXT_ROWS,      // loc f64 [n] | scale f64 [n] | column means f64 [tiles * 16] | centred sums of squares f64 [tiles * 16] |
                            //   safe_permtest_extremes (maxt.hip) | within the call
    SCRATCH_MAXT_TILES,     // the attribute operand of k_maxt_extremes: f64 tiles [tile][n][16] | safe_permtest_extremes | within the call
    SCRATCH_MAXT_TABLE,     // the permutation table transposed, i32 [n][P] | safe_permtest_extremes | within the call
    SCRATCH_MAXT_KEYS,      // ordered 64-bit keys of the running maxima | minima, u64 [2][columns][P] | safe_permtest_extremes | within the call
    SCRATCH_MAXT_FAMILY,    // whole-matrix extremes f64 [2][P] | smallest counts per column u32 [2][m] | safe_counts_from_extremes (maxt.hip) |
                            //   within the call
    N_SCRATCH
};
static_assert(SCRATCH_STREAM_B == SCRATCH_STREAM_A + 1 && SCRATCH_MFMA_AMB_B == SCRATCH_MFMA_AMB_A + 1,
              "the two halves of a double buffer are adjacent slots (scratch_pair)");
// half b (0 / 1) of the double buffer whose first slot is `first`
static inline ScratchSlot scratch_pair(ScratchSlot first, int b) { return static_cast<ScratchSlot>(first + b); }

struct safe_ctx {
    int device = 0;
    DrawWorker *draw_worker = nullptr, *draw_worker2 = nullptr;    // (the second one runs the twin chain: safe_perms::twin)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;           // permutation-table generation (overlaps the enrichment kernels)
    hipStream_t side_stream = nullptr;          // second enrichment stream: consecutive spans overlap their tails
    hipStream_t more_streams[2] = {nullptr, nullptr};   // third and fourth (bit-sliced kernel: deeper overlap of consecutive launches)
    int num_cu = 0;
    int64_t hbm_bytes = 0;
    char arch[64] = {0};
    hipEvent_t t0 = nullptr, t1 = nullptr;      // safe_timer_*
    hipEvent_t k0 = nullptr, k1 = nullptr;      // dominant-kernel timing
    hipEvent_t switch_ev = nullptr;             // safe_ctx_set_stream: end of the work on the stream being left (created on first use)
    KernelStat last_kernel;
    int last_slices = 0;                        // i8 slices of the last matrix-core permutation test (2 / 4 / 6)
    void *diag_prof = nullptr;                  // (diagnostic builds) per-phase cycle counters of the matrix-core kernel
    int last_core_slices = 0;                   // slices its matrix-core kernel multiplied (3 of 6 in the filtered form)
    int64_t last_undecided = 0;                 // filtered form: compares decided by k_mfma_resolve (negative: list overflow, six-slice rerun)
    double diffusion_ms[2] = {0.0, 0.0};        // all k_diffusion_step launches, k_diffusion_transform of the last safe_nbr_diffusion
    int diffusion_steps = 0;                    //   and the number of step launches (safe_last_diffusion_stats)
    double rank_ms[3] = {0.0, 0.0, 0.0};        // k_rank_keys, k_rank_sort, k_rank_emit of the last safe_attr_rank (safe_last_rank_stats)
    // grow-only scratch buffers reused across calls (hipMalloc of >100 MB costs milliseconds)
    struct safe_perms *perm_cache = nullptr;    // buffers of the last destroyed permutation handle, reused by the next
    struct PermRing *ring = nullptr;            // node-shared permutation stream (safe_ctx_share_stream), or NULL
    // packed <= / >= counters of the last integer-counter permutation kernel (SCRATCH_COUNTERS):
    // u32 [packed_m][packed_n_pad] = (#less << 16 | #greater); layout 0 = SELL positions,
    // 1 = block order of the MFMA kernel, -1 = none (safe_export_packed_counts)
    const unsigned int *packed_counts = nullptr;
    int64_t packed_n_pad = 0, packed_m = 0, packed_perms = 0;
    int packed_layout = -1;
    // Exchange overlap of the sharded step (safe_set_exchange_chunks; sharding.py): the bit-sliced launches run the LAST part of
    // the permutations column chunk by column chunk, so that a chunk's counters are final -- and can travel -- while the later
    // chunks still compute.  xc_want / xc_cols: what the caller armed; xc_made / xc_bounds / xc_events: what the last call did.
    static constexpr int XC_MAX = 8;
    int xc_want = 0;
    int64_t xc_cols = 0;
    void (*xc_callback)(void *) = nullptr;      // called once every launch of the call is enqueued (before the call's own sync)
    void *xc_user = nullptr;
    int xc_made = 0;
    int64_t xc_bounds[XC_MAX + 1] = {};         // column boundaries of the chunks (this rank's columns: clipped to packed_m)
    int64_t xc_tail_perms = 0;                  // permutations the column-chunked launches covered
    hipEvent_t xc_events[XC_MAX] = {};          // chunk k's counters are final
    std::vector<double> nes_tab_host;           // ctx_nes_table: the table SCRATCH_NES_TABLE holds (empty: none)
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    // large device-to-host copies into pageable memory (safe_memcpy_d2h): a ring of pinned slots the DMA engine fills while host
    // threads copy finished slots into the destination (and take its first-touch page faults in parallel)
    static constexpr int D2H_SLOTS = 8;
    static constexpr size_t D2H_SLOT_BYTES = size_t(4) << 20;
    void *d2h_ring = nullptr;
    std::mutex d2h_mu;                          // the ring serves one read-back at a time
    hipEvent_t d2h_events[D2H_SLOTS] = {};
    std::vector<hipEvent_t> ev_timing, ev_plain;   // reused per-launch events (creating 20 per call costs ~0.1 ms)
    std::vector<std::pair<size_t, void *>> block_cache;   // small device blocks of destroyed handles (ctx_block_alloc)
    void *scratch[N_SCRATCH] = {};
    size_t scratch_bytes[N_SCRATCH] = {};
};

// Returns a device buffer of at least `bytes` from slot `slot`; its contents are undefined.  The buffer is valid until the next
// request for the same slot: a larger request frees it and allocates anew.  Before it frees, ctx_scratch synchronises the
// context's two enrichment streams (ctx->stream, ctx->side_stream) and NO other: a caller that uses the buffer on any other
// stream -- the aux stream, a stream of the application's -- must itself have synchronised that stream before it asks again.
int ctx_scratch(safe_ctx *ctx, ScratchSlot slot, size_t bytes, void **out);
// The NES look-up table tab[k] = -log10(k / P), k = 0 .. P (k = 0 as k = 1) -- `host_or_null` [P + 1], or computed here -- on the
// device, for work on stream s (enrich.hip).  The table stays resident in SCRATCH_NES_TABLE: a call with the table of the call
// before costs no upload and no synchronisation; another table synchronises s before the old one is released or overwritten
// (whatever still reads it on s finishes first), is uploaded on s, and s is synchronised again (the source is host memory).
// As with ctx_scratch, work that reads the table on yet another stream is the caller's to finish before the table changes.
int ctx_nes_table(safe_ctx *ctx, const double *host_or_null, int64_t P, hipStream_t s, const double **d_tab);
// grow-only pinned host buffer (device-to-host copies into it go through the DMA engines: no copy kernel
// that would have to wait for a CU while a persistent kernel holds all of them)
int ctx_pinned(safe_ctx *ctx, size_t bytes, void **out);
// `count` reusable events of the context (timing-enabled, or hipEventDisableTiming); valid until the next request of the same kind
int ctx_events(safe_ctx *ctx, bool timing, size_t count, hipEvent_t **out);
void perms_cache_drop(safe_ctx *ctx);   // frees ctx->perm_cache (rng.cpp)
int kernel_stat_from_events(safe_ctx *ctx, hipEvent_t *ev, int64_t n_launch);   // enrich.hip
// The frame of a launcher whose spans alternate between ctx->stream and ctx->side_stream (launch_bits, launch_lds_f64,
// launch_mfma_run).  open: the call's last_kernel record starts at zero under `name`; 2 * n_launch timing events (ev[2 c],
// ev[2 c + 1] bracket launch c) and n_plain plain ones come from the context's pool; plain[0] says "inputs ready" on ctx->stream
// and the side stream waits for it.  join, behind the last launch: ctx->stream waits for the side stream (plain[1]).  close,
// behind the finalize pass: k0 / k1, the call's host wait, kernel_stat_from_events.
struct SpanFrame {
    hipEvent_t *ev = nullptr, *plain = nullptr;
    int64_t n_launch = 0;
};
static inline int span_frame_open(safe_ctx *ctx, const char *name, int64_t n_launch, size_t n_plain, SpanFrame *f) {
    ctx->last_kernel.name = name;
    ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = 0.0;
    ctx->last_kernel.launches = 0;
    f->n_launch = n_launch;
    SAFE_TRY(ctx_events(ctx, true, 2 * n_launch, &f->ev));
    SAFE_TRY(ctx_events(ctx, false, n_plain, &f->plain));
    SAFE_HIP_CHECK(hipEventRecord(f->plain[0], ctx->stream));
    SAFE_HIP_CHECK(hipStreamWaitEvent(ctx->side_stream, f->plain[0], 0));
    return SAFE_OK;
}
static inline int span_frame_join(safe_ctx *ctx, const SpanFrame &f) {
    SAFE_HIP_CHECK(hipEventRecord(f.plain[1], ctx->side_stream));
    SAFE_HIP_CHECK(hipStreamWaitEvent(ctx->stream, f.plain[1], 0));
    return SAFE_OK;
}
static inline int span_frame_close(safe_ctx *ctx, const SpanFrame &f) {
    SAFE_HIP_CHECK(hipEventRecord(ctx->k0, ctx->stream));
    SAFE_HIP_CHECK(hipEventRecord(ctx->k1, ctx->stream));
    SAFE_HIP_CHECK(safe_stream_sync(ctx->stream));
    return kernel_stat_from_events(ctx, f.ev, f.n_launch);
}
// small per-handle device blocks (row flags, column sums): hipMalloc + hipFree cost tens of microseconds each and a handle
// is made per compute_pvalues pass, so freed blocks wait in the context for the next handle of the same shape
int ctx_block_alloc(safe_ctx *ctx, size_t bytes, void **out);
void ctx_block_free(safe_ctx *ctx, void *p, size_t bytes);

// as SAFE_HIP_CHECK, with the message "<who>: <hip error string>" of the entry points that name themselves
#define SAFE_HIP_CHECK_AS(who, expr)                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            safe_set_error("%s: %s", who, hipGetErrorString(_e));                              \
            return SAFE_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

// Device memory of the library: every block comes from dev_alloc and goes back through dev_free.  Who owns a block:
//   * the context: its scratch slots (ctx_scratch) and pooled small blocks (ctx_block_alloc), until safe_ctx_destroy;
//   * a handle (safe_nbr, safe_attr, safe_perms, safe_kk, safe_pairs, safe_go): its members, plain pointers, until the handle's destroy;
//   * a call: a CallBufs (below) on the stack of the entry point, until it returns -- on whatever path.
// calls of hipMalloc / hipHostMalloc made by the library so far (safe_alloc_count): a timed step is expected to make none
extern std::atomic<long long> g_alloc_calls;
// device blocks from dev_alloc that dev_free has not seen yet (safe_live_alloc_count): the same before and after any call
// that returns no handle
extern std::atomic<long long> g_live_blocks;

static inline int dev_alloc_bytes(void **p, size_t bytes) {
    *p = nullptr;
    g_alloc_calls.fetch_add(1, std::memory_order_relaxed);
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        safe_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return SAFE_E_NOMEM;
    }
    g_live_blocks.fetch_add(1, std::memory_order_relaxed);
    return SAFE_OK;
}

template <typename T>
static inline int dev_alloc(T **p, size_t count) {
    return dev_alloc_bytes(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
}

// NULL is fine.  hipFree waits until the device is idle: work that still uses the block has ended before it is released.
static inline hipError_t dev_free(const void *p) {
    if (!p) return hipSuccess;
    g_live_blocks.fetch_sub(1, std::memory_order_relaxed);
    return hipFree(const_cast<void *>(p));
}

// The device buffers of one call, released when the call returns on any path.  The destructor may run while work of the call
// is still enqueued (an early return behind a launch): dev_free waits for the device, so the kernels and copies that use the
// buffers have ended before they go.  Host memory has no such wait -- declare a CallBufs AFTER every host std::vector an
// asynchronous copy of the call reads, so that it is destroyed (and the device idle) before the vector is.
struct CallBufs {
    std::vector<void *> p;
    CallBufs() = default;
    CallBufs(const CallBufs &) = delete;
    CallBufs &operator=(const CallBufs &) = delete;
    ~CallBufs() {
        for (void *q : p) (void)dev_free(q);
    }
    template <typename T>
    int alloc(T **q, size_t count) {
        const int rc = dev_alloc(q, count);
        if (rc == SAFE_OK) p.push_back(*q);
        return rc;
    }
    // the block now belongs to a handle: it stays when the call ends
    template <typename T>
    T *release(T *q) {
        p.erase(std::remove(p.begin(), p.end(), static_cast<void *>(q)), p.end());
        return q;
    }
};

// Kernel time of a call between two events on a stream; the events are destroyed on every return path.
struct CallTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    CallTimer() = default;
    CallTimer(const CallTimer &) = delete;
    CallTimer &operator=(const CallTimer &) = delete;
    ~CallTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t start(hipStream_t s) {
        for (hipEvent_t &e : ev) {
            const hipError_t err = hipEventCreateWithFlags(&e, safe_event_flags(hipEventDefault));
            if (err != hipSuccess) return err;
        }
        return hipEventRecord(ev[0], s);
    }
    hipError_t stop(hipStream_t s) { return hipEventRecord(ev[1], s); }
    // after the stream has been synchronised
    hipError_t ms(double *out) {
        float f = 0;
        const hipError_t err = hipEventElapsedTime(&f, ev[0], ev[1]);
        *out = f;
        return err;
    }
    // ... the time also recorded as the context's last kernel
    hipError_t finish(safe_ctx *ctx, const char *name, int64_t launches, double *kernel_ms) {
        double t = 0;
        const hipError_t err = ms(&t);
        if (err != hipSuccess) return err;
        ctx->last_kernel.name = name;
        ctx->last_kernel.total_ms = ctx->last_kernel.busy_ms = t;
        ctx->last_kernel.launches = launches;
        ctx->last_kernel.summed = true;
        if (kernel_ms) *kernel_ms = t;
        return hipSuccess;
    }
};

// Membership structure.  Canonical form: bit matrix; derived: CSR and SELL-64 (sliced
// ELLPACK with rows sorted by descending count so each 64-row slice is nearly uniform).
struct safe_nbr {
    safe_ctx *ctx = nullptr;
    int64_t n = 0;
    int64_t nnz = 0;
    int64_t max_count = 0;
    int64_t words = 0;              // 64-bit words per bit-matrix row
    uint64_t *bits = nullptr;       // [n][words]
    int32_t *row_ptr = nullptr;     // [n+1]
    int32_t *col = nullptr;         // [nnz]
    // SELL-64
    int64_t n_slices = 0;
    int32_t *sell_row = nullptr;    // [n_slices*64] original row id, -1 = padding lane
    int32_t *sell_pos = nullptr;    // [n] position of row i in sell_row (inverse map)
    int64_t *slice_off = nullptr;   // [n_slices+1] offset into sell_col (entries)
    int32_t *slice_width = nullptr; // [n_slices]
    int32_t *sell_col = nullptr;    // [slice_off[n_slices]] column id, n = padding (zero row)
    int64_t sell_entries = 0;
    uint16_t *sell_col2 = nullptr;  // [sell_entries + 1024] 2*column id as u16 (n < 32768 only): LDS byte offsets of a u16 table
    uint16_t *sell_col2b = nullptr; // the same list in blocked order: 8 members of a lane adjacent (one 16-byte load per lane and block)
    std::vector<int32_t> h_slice_width;
    BitsTaskPlan bits_plan;         // (bits_task_plan's cache, enrich.hip)
    void *bits_plan_pinned = nullptr;              // the plan's task lists in pinned host memory (grow-only): uploaded from there every
    size_t bits_plan_pinned_bytes = 0;             // pass -- an async copy from pageable memory pins the pages first (an ioctl that
                                                   // was seen to take milliseconds once in a few hundred passes)
    std::vector<int64_t> h_slice_off;
    std::vector<int32_t> h_row_count;   // host copy of per-row counts
    double *dist = nullptr;         // optional [n][n]
    // distance weights (weights.hip), or NULL: one f64 per member.  No entry point outside weights.hip reads them.
    double *w_csr = nullptr;        // [nnz] in CSR order
    double *w_sell = nullptr;       // [sell_entries] beside sell_col, padding entries 0.0
    // CSR of the transpose (column k -> rows i with A[i,k] = 1), built on first use
    int32_t *at_ptr = nullptr;      // [n+1]
    int32_t *at_col = nullptr;      // [nnz], unordered inside a column
    // Block-sparse form for the MFMA permutation kernel (mfma.hip), built on first use:
    // nodes in a locality-preserving order (Hilbert curve over the layout when one is known,
    // Cuthill-McKee over the membership graph otherwise); 256-row groups x 32-column blocks,
    // only blocks holding at least one member are stored, as 256 32-bit row words each.
    std::vector<double> h_xy;       // [n][2] layout, if known (safe_nbr_euclidean / safe_nbr_set_layout)
    bool blocks_ready = false;
    int64_t bs_groups = 0;          // number of 256-row groups
    int64_t bs_blocks = 0;          // stored blocks (every group padded to a multiple of 4)
    int64_t bs_pieces = 0;          // 32-row x 32-column pieces of the stored blocks that hold at least one member (the only ones multiplied)
    int64_t bs_src = 0;             // length of a source-row map: (ceil(n/32)+1)*32, the last block is padding
    int32_t *bs_order = nullptr;    // [bs_src] node at ordered position u (n = padding -> zero attribute row)
    int32_t *bs_rowmap = nullptr;   // [bs_groups*256] node at ordered row u, -1 = padding
    int32_t *bs_rowcnt = nullptr;   // [bs_groups*256] members of that node's neighborhood (-1 = padding row)
    int32_t *bs_grpmax = nullptr;   // [bs_groups] largest neighborhood of the group's rows
    uint4 *bs_bits4p = nullptr;     // the membership bits again, [super-step of 4 blocks][256 rows][4] (one 16-byte load per row and super-step),
                                    // the bits of every word in operand order: bit 8 b + 4 h + j = member 16 h + 4 j + b of the block
                                    // (k_permtest_mfma_g: register j of lane half h is (word >> (4 h + j)) & 0x01010101)
    int64_t bs_max_group_blocks = 0;   // blocks of the longest group
    int32_t *bs_ptr = nullptr;      // [bs_groups+1] first block of a group
    int32_t *bs_kb = nullptr;       // [bs_blocks] ordered column block of a stored block
    uint32_t *bs_bits = nullptr;    // [bs_blocks][256] membership bits of the block's 256 rows
    std::vector<int32_t> h_bs_ptr;
    std::vector<int32_t> h_bs_rowmap;   // host copy of bs_rowmap
    // task list of the matrix-core COUNT kernel (one i8 plane per tile): (row group, column group) pairs in eight per-XCD queues;
    // a function of the block structure and the number of column groups only, kept for the next call (counts_setup)
    std::vector<int2> counts_tasks;
    int32_t counts_qoff[9] = {0};
    int64_t counts_tasks_grp = -1;
};

// Hypergeometric epilogue by table lookup (enrich.hip: k_hyp_table builds tab): instead of a count X
// a kernel writes p = tab[(nid[row] * n_kid + kid[col]) * xs + X], -log10 p, the binarised value and
// the per-attribute enriched counts (safe.py:596-608, 468-472).  tab == NULL: plain counts as f64
// into pvalues_pos (compute_neighborhood_score 'sum' of 0/1 data).
struct HypLookup {
    const int32_t *nid;        // [n] index of the row's neighborhood size among the distinct sizes
    const int32_t *kid;        // [mloc] index of the column's annotation count among the distinct counts
    const double2 *tab;        // [n_nid][n_kid][xs] of (p, -log10 p)
    int64_t n_kid, xs;
    double p_cut;              // binarisation as a bound on p (nes_p_cut)
    double *dummy;             // [64] write-only slots for the padding rows / columns of branch-free epilogues
    double *pvalues_pos, *nes, *nes_binary;
    unsigned int *enriched;
    unsigned int *cnt16;       // split form of the matrix-core counts: packed u16 counts [group][position][32][6], else NULL
    unsigned int *xmax;        // split form: largest count of the call (written by the count kernel, read by the emit kernel)
    int dbg = 0;               // diagnostic builds of the matrix-core permutation kernel (SAFE_HIP_MFMA_DBG; wrong results)
};

// |nes| > -log10(enrichment_threshold) (safe.py:468-470) for nes = -log10(p), p in [0, 1], restated as a
// bound on p itself: hit <=> p < p_cut with p_cut = the smallest double whose -log10 (host libm, the one
// NumPy calls) does NOT exceed the threshold.  log10 is monotone, so the decision for a given p is the
// reference's whatever the device's own log10 rounds to.
static inline double nes_p_cut(double enrichment_threshold) {
    const double thr = -std::log10(enrichment_threshold);
    auto hit = [&](double p) { return -std::log10(p) > thr; };
    double p = enrichment_threshold;
    for (int it = 0; it < 4096 && hit(p); ++it) p = std::nextafter(p, 1.0);
    for (int it = 0; it < 4096 && !hit(std::nextafter(p, 0.0)); ++it) p = std::nextafter(p, 0.0);
    return p;
}

// what a permutation-test kernel writes (PermOut::mode)
enum PermMode {
    PERM_SCORE = 0,    // the observed score only
    PERM_COUNTS = 1,   // raw counts
    PERM_FULL = 2,     // full post-processing: p-values, NES, nes_binary, enriched counters
    PERM_SUBSET = 4,   // any subset of p-values / NES / nes_binary (NULL = not wanted) from 'sum' counters (k_counts_finalize)
};

// outputs of the permutation-test kernels (enrich.hip, mfma.hip)
struct PermOut {
    double *ns;            // [n][mloc] or NULL
    double *counts_neg;    // raw-count mode
    double *counts_pos;
    double *pvalues_neg;   // full mode
    double *pvalues_pos;
    double *nes;
    double *nes_binary;
    unsigned int *enriched;   // [mloc] u32 column counters
    const double *nes_table;  // [P+1]
    double nes_threshold;     // -log10(enrichment_threshold)
    int sign_mode;
    int mode;                 // PermMode
    int64_t ld;               // row pitch of the output matrices in elements (0 = the column count of the call)
};

struct safe_attr {
    safe_ctx *ctx = nullptr;
    int64_t n = 0, m = 0;
    int dtype = SAFE_DTYPE_F64;
    int64_t row_stride = 0, col_stride = 0;
    const void *raw = nullptr;      // device
    bool owns_raw = false;
    size_t raw_pool_bytes = 0;      // owns_raw and > 0: raw is a block of the context's pool (ctx_block_alloc) of that size
    uint8_t *row_flags = nullptr;   // [n] device, 1 = row has >= 1 non-NaN value
    std::vector<uint8_t> h_row_flags;   // host copy of row_flags (kept in step: safe_attr_row_flags answers without a device sync)
    bool flags_ready = false;
    bool stats_ready = false;
    int64_t n_other = 0, max_nan_col = 0, n_rows_with_value = 0, n_non_integer = 0;
    double *col_sum = nullptr;      // [m] nansum per column (device)
    double max_abs = 0.0;           // max |value| over non-NaN entries
    // binary matrices only: support lists (CSC of the ones), built on first use
    int32_t *sup_ptr = nullptr;     // [m+1]
    int32_t *sup_row = nullptr;     // [n_ones]
    int64_t n_ones = 0;
    std::vector<int32_t> h_sup_ptr; // host copy
    size_t sup_ptr_pool_bytes = 0, sup_row_pool_bytes = 0;   // > 0: the lists are blocks of the context's pool (installed from a CSC input)
};

struct DrawStream;   // host MT19937 draw stream (rng.cpp)

struct safe_perms {
    safe_ctx *ctx = nullptr;
    int64_t n = 0;
    int64_t count = 0;
    int64_t k = 0;                  // number of movable rows (indx_vals)
    std::vector<int32_t> h_movable;
    DrawStream *stream = nullptr;
    // pipeline positions (in permutations): drawn >= enqueued on the GPU
    int64_t generated = 0, enqueued = 0;
    std::vector<int64_t> stages;                   // pipeline stage boundaries of this handle (perms_stage_plan(count))
    std::vector<hipEvent_t> chunk_done;            // recorded on ctx->aux_stream after each enqueued chunk
    std::vector<uint32_t> h_local;                 // the draw thread's private buffer: the targets of one shuffle (L1-resident)
    // the draw thread: runs the sequential MT19937 / rejection stream chunk by chunk into the pinned staging buffers, at most
    // kStage chunks ahead of the uploads, independent of the thread that launches kernels
    std::thread drawer;                            // a thread of its own (only when the context's draw worker is busy with another handle)
    bool on_worker = false;                        // this handle's draws run (or ran) on ctx->draw_worker
    bool worker_done = false;                      // (under the worker's mutex) ... and have ended
    // The TWIN: a second draw thread runs the very same chain (same seed, same words) on another core into buffers of its own,
    // and whichever thread finishes a chunk first publishes it.  The chain is sequential and cannot be sped up, but on a shared
    // host one thread runs 1.5-2 x slower for a millisecond or two now and then (a neighbour on its sibling hardware thread, a
    // pre-emption) -- the idea was that both threads stumbling in the same chunk is rare.  Measured: no better than one thread
    // (rng.cpp, perms_create_impl), so it is opt-in (SAFE_HIP_DRAW_TWIN=1).
    bool twin = false;
    bool on_worker2 = false, worker_done2 = false;
    DrawStream *stream2 = nullptr;
    void *h_stage2[3] = {nullptr, nullptr, nullptr};
    hipEvent_t staged2[3] = {nullptr, nullptr, nullptr};
    std::vector<uint32_t> h_local2;
    std::vector<uint8_t> chunk_src;                // (under draw_mu) which thread's staging buffer holds chunk c
    int64_t twin_wins = 0;                         // chunks the twin published first (diagnostics)
    std::mutex draw_mu;
    std::condition_variable draw_cv;
    int64_t drawn_chunks = 0;                      // chunks whose targets are complete in h_stage[c % kStage]
    std::atomic<int64_t> drawn_chunks_pub{0};      // the same, readable without the mutex (the launcher spins on it)
    int64_t enqueued_chunks = 0;                   // chunks whose upload has been queued (staged[c % kStage] recorded)
    bool draw_stop = false;
    bool draw_failed = false;        // the draw thread gave up (under draw_mu): waiters return an error instead of waiting for ever
    static constexpr int kStage = 3;
    void *h_stage[kStage] = {nullptr, nullptr, nullptr};   // pinned: accepted swap targets of a chunk, [chunk][target_width] u16 (k <= 65535) or u32
    hipEvent_t staged[kStage] = {nullptr, nullptr, nullptr};
    size_t stage_bytes = 0;                        // capacity of each staging buffer (sized for k = n)
    int target_bytes = 2;                          // bytes per swap target on the wire (2 when k <= 65535)
    int64_t target_width = 0;                      // targets per permutation row: k - 1 rounded up to 8
    void *d_targets = nullptr;                     // device copy of the chunk being replayed (even chunks)
    void *d_targets_odd = nullptr;                 // ... odd chunks: a chunk's upload and replay run beside its predecessor's scan
    int32_t *d_maps_odd[2] = {nullptr, nullptr};   // row maps / scan ping-pong of the odd chunks
    hipEvent_t replayed[2] = {nullptr, nullptr};   // by chunk parity: the replay has written its row maps (recorded on the replay stream)
    hipEvent_t movpos_ready = nullptr;             // d_movpos uploaded (aux stream) -- the replay stream waits for it once per handle
    int32_t *d_big = nullptr;                      // k > 65535 only: [chunk][k] position arrays of the global-memory replay
    int32_t *h_movpos = nullptr;                   // pinned [2n]: staging of d_movpos
    int32_t *d_maps[2] = {nullptr, nullptr};       // [chunk][n+1] row maps / scan ping-pong
    int32_t *d_cur = nullptr;       // [n+1] running composition (last emitted row)
    int32_t *table = nullptr;       // [count][n+1] device; entry n is the padding row (== n)
    // 16-bit copy of the table, rows padded to a multiple of 8 entries (n < 65535 only)
    uint16_t *table16 = nullptr;
    int64_t stride16 = 0;
    // transposed inverse permutations, built on first use (n < 65535 only):
    // inverse_t[r * inv_stride + p] = position k with table[p][k] == r; inv_stride = padded count
    uint16_t *inverse_t = nullptr;
    int64_t inv_stride = 0;
    bool from_table = false;        // rows supplied by the caller (safe_perms_create_from_table): no stream, complete from the start
    // node-shared stream (ring.h; safe_perms_create_shared): local rank 0 of a node publishes every chunk's row maps,
    // the other ranks fetch them instead of drawing (no draw thread, no swap workers on those ranks)
    bool device_gen = false;        // tables generated on the device (safe_perms_create_device): no host stream at all
    int32_t *d_movpos = nullptr;    // [n] movable rows (first k used) | [n] position of a row in that list (-1: fixed)
    // restricted permutations (safe_perms_create_device_strata) only, allocated on first use and kept with the handle:
    // [S + 1] starts of the strata in the stratum-ordered list of movable rows | [n_big] strata the whole wave shuffles
    int32_t *d_strata = nullptr;
    int32_t *h_strata = nullptr;    // pinned staging of d_strata (2n + 8 entries each)
    struct PermRing *ring = nullptr;               // the context's ring while this handle takes part in a shared call, else NULL
    bool ring_consumer = false;
    // Identity of the composed table while the handle is parked in ctx->perm_cache (rng.cpp, perms_create_impl): the stream is a
    // pure function of (seed, n, count, movable rows), so the next seeded create with the same inputs takes the finished table
    // as it lies in HBM.  tables_valid is only ever set by safe_perms_destroy and cleared the moment the handle is taken back.
    bool has_seed = false;          // the caller named the seed (an entropy-seeded stream is never kept)
    uint32_t seed = 0;
    bool tables_valid = false;      // parked: table / table16 hold the complete stream of (seed, n, count, h_movable)
    bool resident = false;          // live: this handle took a parked table instead of drawing (role 4 of safe_perms_timing)
    // host-side timing of the stream (safe_perms_timing), ms since the handle was created
    double t_created_s = 0.0, draw_busy_ms = 0.0, drawn_all_ms = 0.0, enqueued_all_ms = 0.0, ring_wait_ms = 0.0;
};

int safe_attr_prepare(safe_attr *attr);   // row flags + stats (attr.hip)
// mu_j and Q_j of columns [col0, col1) into d_mean / d_css [col1 - col0], enqueued on the context's stream (moments.hip)
int column_moments_dev(safe_ctx *ctx, safe_attr *attr, int64_t col0, int64_t col1, const char *who, double *d_mean, double *d_css);
// the row side of the permutation moments into two f64 [n] arrays, enqueued on the context's stream; the attribute handle is
// prepared.  Flat: k_i and f_i of safe_moments_test (moments.hip); a handle with weights: W1_i and g_i of
// safe_moments_test_weighted (weights.hip)
int moments_row_factors_dev(safe_ctx *ctx, const safe_nbr *nbr, const safe_attr *attr, const char *who, double *d_size, double *d_factor);
int weights_row_factors_dev(safe_ctx *ctx, const safe_nbr *nbr, const safe_attr *attr, const char *who, double *d_w1, double *d_g);
int nbr_finalize_from_bits(safe_nbr *nbr);   // bits -> CSR + SELL (nbr.hip)
// a handle under construction (nbr.hip; diffusion.hip builds one too): nbr_new allocates the bit matrix, and the handle is freed
// on every return path until it is released into the caller's *out
void nbr_free(safe_nbr *nbr);
using NbrPtr = std::unique_ptr<safe_nbr, void (*)(safe_nbr *)>;
int nbr_new(safe_ctx *ctx, int64_t n, NbrPtr *out);
int nbr_build_transpose(safe_nbr *nbr);      // at_ptr / at_col (nbr.hip)
// Where node distances are read from on the device: the layout xy [n][2] (recomputed with pdist's roundings wherever they are
// needed) or the matrix dist [n][n] a handle kept (+inf = unreached), read in place.  Exactly one of the two is set.
struct DistSource {
    const double *xy;
    const double *dist;
    int64_t n;
};
// Host checks and uploads the neighborhood entry points share (nbr.hip); `fn` prefixes the message.
// every coordinate of xy_host [n][2] is finite, else SAFE_E_VALUE
int check_layout_finite(const char *fn, const double *xy_host, int64_t n);
// radii of the per-row builders and of the weights: none NaN, none negative (+inf is a radius), else SAFE_E_VALUE
int check_radii(const char *fn, const double *radii, int64_t n);
// xy_host [n][2] into a block of the call's `b`, copied on the context's stream: xy_host is read until the stream has been waited for
int upload_layout(safe_ctx *ctx, CallBufs *b, const char *fn, const double *xy_host, int64_t n, const double **d_xy_out);
// Undirected CSR adjacency of an edge list, on the host: one entry per direction, a self-loop once, duplicates kept, a row's
// entries in input order; edge_w NULL = 1 per edge.  ptr [n + 1], col and w [max(entries, 1)].  SAFE_E_INVALID for an end point
// outside [0, n), a negative, infinite or NaN weight, or more entries than int32 offsets hold.
int build_undirected_csr(const char *fn, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v, const double *edge_w,
                         std::vector<int32_t> *ptr, std::vector<int32_t> *col, std::vector<double> *w);
int attr_build_support(safe_attr *attr);     // sup_ptr / sup_row of a binary matrix (attr.hip)
// an attribute handle that owns nothing on the device yet (the checks of safe_attr_create_*; attr.hip)
int attr_new(safe_ctx *ctx, int dtype, int64_t n, int64_t m, int64_t rs, int64_t cs, safe_attr **out);
// dst (same n, no flags yet) takes a copy of src's row flags if src has any -- computed or installed; else nothing happens (attr.hip)
int attr_inherit_flags(safe_attr *dst, const safe_attr *src);
// the expansion behind safe_attr_create_csc_host; on_device: the four input arrays are device memory, complete on ctx->stream (attr.hip)
int attr_create_csc(safe_ctx *ctx, int64_t n, int64_t m, int64_t nnz, const int64_t *indptr, const int32_t *indices, const void *values,
                    int dtype, const uint8_t *missing_rows, bool on_device, safe_attr **out);
// offs[i] = counts[0] + ... + counts[i - 1], i = 0 .. len, 64-bit, one workgroup on stream s (k_pairs_scan, pairs.hip)
hipError_t pairs_scan_launch(hipStream_t s, const int32_t *counts, int64_t len, int64_t *offs);
int perms_build_inverse(safe_perms *perms);  // inverse tables (rng.cpp)
int perms_generate_until(safe_perms *perms, int64_t upto);   // enqueue table rows [generated, upto) on aux_stream (rng.cpp)
// host/GPU pipeline stages of the permutation stream for `count` permutations: boundaries b[0] = 0 < b[1] < ... < b.back() = count
// (a short first stage, 128 each, short last stages -- rng.cpp)
std::vector<int64_t> perms_stage_plan(int64_t count);
// launch boundaries of the permutation kernels: starts[c] .. starts[c+1]; the default follows the
// stream's pipeline stages (so the first launch can start after 32 permutations have been drawn),
// SAFE_HIP_BITS_SPAN=<n> forces uniform spans.  *span = the longest launch.
// merge > 1: after the three start-up stages (32, 96, 128 permutations) a launch covers `merge` stages -- fewer,
// longer launches once the stream is ahead of the kernels.
// drawn_spans: a resident table (safe_perms::resident: complete before the first launch, stages = even spans) is consumed in
// the launches of the drawn stream all the same -- any boundaries are valid for it, every stage event is complete.  For callers
// whose launch logic is sized by those stages: the matrix-core path (its list of undecided compares holds what a launch of
// <= 128 permutations leaves) and the column-chunked exchange tail (it needs three launches in front of the tail).
static inline std::vector<int64_t> perm_launch_starts(const safe_perms *perms, int64_t *span, int merge = 1, bool drawn_spans = false) {
    const int64_t P = perms->count;
    std::vector<int64_t> starts;
    int64_t uniform = 0;
    if (const char *e = getenv("SAFE_HIP_BITS_SPAN")) uniform = std::max<int64_t>(16, atoll(e));
    if (uniform > 0) {
        for (int64_t p = 0; p < P; p += uniform) starts.push_back(p);
    } else {
        // the handle's own stages (host pipeline, or even spans for device tables and resident tables)
        const std::vector<int64_t> plan = (drawn_spans && perms->resident) ? perms_stage_plan(P) : perms->stages;
        const int64_t nc = static_cast<int64_t>(plan.size()) - 1;
        for (int64_t c = 0; c < nc; ++c)
            if (c < 3 || merge <= 1 || (c - 3) % merge == 0) starts.push_back(plan[c]);
    }
    if (starts.empty()) starts.push_back(0);
    starts.push_back(std::max<int64_t>(P, 0));
    *span = 1;
    for (size_t c = 0; c + 1 < starts.size(); ++c) *span = std::max<int64_t>(*span, starts[c + 1] - starts[c]);
    return starts;
}
int perms_wait(safe_perms *perms, int64_t upto, hipStream_t s);   // make stream s wait until rows [0, upto) exist (rng.cpp)
// counters [column][position] (#less << 16 | #greater) -> outputs; rowmap[position] = row or -1 (enrich.hip)
int enrich_finalize_counts(safe_ctx *ctx, const unsigned int *counts, int64_t n_pad, const int32_t *rowmap, int64_t mloc,
                           int64_t n_perm, const PermOut &out, const double *ns_direct, hipStream_t on = nullptr, bool pk20 = false);
// MFMA (i8, exact fixed point) form of the permutation test for quantitative attributes (mfma.hip); force_mfma =
// SAFE_HIP_FORCE_PATH=mfma (parsed by the caller, enrich.hip route_switches)
bool mfma_applicable(const safe_nbr *nbr, const safe_perms *perms, bool z, bool force_mfma);
int launch_mfma(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms, int64_t col0, int64_t col1, bool z,
                const PermOut &out, bool force_mfma, bool *declined);
// X = A . B0 for 0/1 attributes on the matrix cores (block-sparse, one i8 plane per 32-column tile),
// written through `hl` (mfma.hip); sets ctx->last_kernel and the k0/k1 timing events
int launch_mfma_counts(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int64_t col0, int64_t col1, const HypLookup &hl);
struct MfmaCountsSplit;
bool mfma_counts_split_applicable(const safe_nbr *nbr);
int mfma_counts_split_begin(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int64_t col0, int64_t col1, MfmaCountsSplit **out);
int mfma_counts_split_rows(safe_ctx *ctx, safe_nbr *nbr, MfmaCountsSplit *st, const int32_t *h_nid, hipStream_t hs, void *pinned_stage);
int mfma_counts_split_emit(safe_ctx *ctx, safe_nbr *nbr, MfmaCountsSplit *st, const HypLookup &hl);
void mfma_counts_split_free(MfmaCountsSplit *st);
const unsigned int *mfma_counts_split_xmax(const MfmaCountsSplit *st);   // device: largest count of the call
void nbr_free_blocks(safe_nbr *nbr);
