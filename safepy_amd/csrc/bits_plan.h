// The planning arithmetic of the bit-sliced permutation launch (enrich.hip: launch_bits and its steps): the form and its geometry,
// the cut of the column-chunked exchange tail, the task lists and queues of every launch.  Host code over plain numbers -- no HIP
// runtime, no context, no environment: the host compiler alone builds it (tests/test_bits_plan_cpu.py).
#pragma once
#include <hip/hip_vector_types.h>   // int4

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// launch-geometry helpers
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// levels of a neighborhood sum of the bit-sliced kernels: max row count < 1024 (enrich.hip pins its BT_LV to this)
constexpr int BITS_PLAN_LV = 10;

struct BitsQueues {
    int off[9];                                                           // tasks [off[q], off[q+1]) belong to queue q
};
// Task lists of the bit-sliced permutation kernel for one launch plan (bits_task_plan, enrich.hip): a function of the membership structure and of
// `key` only, so the handle keeps the last one (building them took 90 us of every compute_pvalues pass)
struct BitsTaskPlan {
    std::vector<int64_t> key;
    std::vector<int4> tasks;                                              // the lists back to back
    std::vector<int64_t> list_span, list_first, list_count, launch_list;
    std::vector<BitsQueues> list_queues;
    // the blocked form's per-wave lists (plan_bits_wave_tasks), list k beside list k of the members above: a task is FOUR records,
    // one per wave, wave_first / wave_count in tasks
    std::vector<int4> wave_recs;
    std::vector<int64_t> wave_first, wave_count;
    std::vector<BitsQueues> wave_queues;
};

// LDS of a word column plus the permutation rows, the layout of the row-in-LDS kernel of rounds 1-5 (removed): it still sets the
// number of workgroup slots per CU that the bit-sliced forms' task sizes are cut for (launch_bits)
static inline size_t bits_lds_bytes(int64_t n, int64_t stride16) {
    const size_t t_words = 2 * ((static_cast<size_t>(n) + 2) & ~size_t(1));
    return (t_words + static_cast<size_t>(stride16) + 4) * sizeof(unsigned int);
}
// the word column T of the full-word forms (8 bytes per node) and of the half-word form (4 bytes per node), with the queue slot
static inline size_t bits_pre_lds_bytes(int64_t n) { return (2 * ((static_cast<size_t>(n) + 2) & ~size_t(1)) + 4) * sizeof(unsigned int); }
static inline size_t bits_half_lds_bytes(int64_t n) { return (((static_cast<size_t>(n) + 4) & ~size_t(3)) + 4) * sizeof(unsigned int); }

// The bit-sliced forms, chosen here and nowhere else:
//   BITS_BLK    k_permtest_bits_blk: four waves per workgroup, blocked member lists of 8 * id (the LDS byte offsets fit 16 bits:
//               8 (N + 1) < 65536), neighborhoods below 1024 members;
//   BITS_PRE16  k_permtest_bits_pre: sixteen waves share one word column (N <= 20 470), lists of 2 * id; also the form of
//               neighborhoods of 1024 .. 2047 members on the small networks;
//   BITS_PRE32  k_permtest_bits_pre32: the same over 32-attribute half words (4 bytes per node), lists of ids, up to N = 32 767
//               (the resident 2 * id lists are u16: sell_col2 exists below N = 32 768 only).
// levels: of the vertical sums, eleven when a neighborhood has 1024 .. 2047 members (the PRE forms only), else ten.
// With the form its geometry, derived here once: waves (= adjacent slices of a task) per workgroup and threads per block; the
// permuted member lists hold id << id_shift; half: the tasks' column units are the halves of the word groups; lds_bytes: the
// kernel's word column and queue slot (its dynamic LDS); wgs_per_cu: workgroups per CU of the grid -- blocked form: four (the
// register file holds 16 waves) where the LDS allows, sixteen-wave forms: one.
enum BitsKind { BITS_NONE = 0, BITS_BLK, BITS_PRE16, BITS_PRE32 };
struct BitsForm {
    BitsKind kind;
    int levels, waves, block, id_shift;
    bool half;
    size_t lds_bytes;
    int wgs_per_cu;
};
static inline BitsForm bits_form(int64_t n, int64_t max_count, bool has_col2, size_t lds_limit) {
    const BitsForm none = {BITS_NONE, 0, 0, 0, 0, false, 0, 0};
    if (!has_col2 || n >= 32768 || max_count >= (2 << BITS_PLAN_LV)) return none;
    const int levels = max_count >= (1 << BITS_PLAN_LV) ? BITS_PLAN_LV + 1 : BITS_PLAN_LV;
    const size_t lds_full = bits_pre_lds_bytes(n), lds_half = bits_half_lds_bytes(n);
    if ((n + 1) * 8 < 65536 && levels == BITS_PLAN_LV)
        return {BITS_BLK, levels, 4, 256, 3, false, lds_full, static_cast<int>(std::max<size_t>(1, std::min<size_t>(4, lds_limit / lds_full)))};
    if (lds_full <= lds_limit) return {BITS_PRE16, levels, 16, 1024, 1, false, lds_full, 1};
    if (lds_half <= lds_limit) return {BITS_PRE32, levels, 16, 1024, 0, true, lds_half, 1};
    return none;
}

// The column-chunked exchange tail (enrich.hip, bits_tail_lists): the launches [0, n_major) run stage by stage over all columns,
// the permutations [p_split, P) as n_chunks launches over column chunks of wpc word groups each.  No tail (n_chunks = 0,
// n_major = every launch, p_split = P) unless at least two chunks of whole word groups are wanted (xc_want, xc_cols), they
// cover the call's mloc columns, the form is the blocked one, the stream has at least three launches and frac -- the wanted
// share of the permutations -- is positive; then the tail begins at the first launch boundary at or behind (1 - frac) P, with at
// least one launch in front of it and the last launch inside it.
struct BitsTail {
    int64_t n_major, p_split;
    int n_chunks;
    int64_t wpc;
};
static inline BitsTail bits_tail_split(int xc_want, int64_t xc_cols, int xc_max, bool blocked, const std::vector<int64_t> &starts,
                                       int64_t P, int64_t mloc, double frac) {
    BitsTail t = {static_cast<int64_t>(starts.size()) - 1, P, 0, 0};
    if (xc_want >= 2 && xc_cols >= 64 && xc_cols % 64 == 0 && blocked && t.n_major >= 3 &&
        static_cast<int64_t>(std::min<int>(xc_want, xc_max)) * xc_cols >= mloc && frac > 0.0) {
        int64_t c_split = 1;
        while (c_split < t.n_major - 1 && static_cast<double>(starts[c_split]) < (1.0 - frac) * static_cast<double>(P)) ++c_split;
        t = {c_split, starts[c_split], std::min<int>(xc_want, xc_max), xc_cols / 64};
    }
    return t;
}

// The 8-member blocks of the widest slice of each group of `wv` adjacent slices (at least one): what a permutation costs the wave
// group of a task
static inline std::vector<int64_t> slice_group_blocks(const std::vector<int32_t> &slice_width, int64_t n_slices, int wv) {
    std::vector<int64_t> blocks(ceil_div(n_slices, wv), 0);
    for (int64_t s = 0; s < n_slices; ++s) blocks[s / wv] = std::max<int64_t>(blocks[s / wv], slice_width[s] / 8);
    for (int64_t &b : blocks) b = std::max<int64_t>(b, 1);
    return blocks;
}

// Tasks (column unit w in [w_lo, w_hi), slice group g, permutations [p0, p1) of a launch of `span`) cut to about equal cost:
// tasks_per_unit tasks per column unit, each at least 256 block-permutations and 16 permutations and at most ppt_cap
// permutations; stably sorted heaviest first for the kernels' dynamic queues.  half_words: a unit is one half (32 columns) of a
// word group, and a last half without columns has no task.
static inline std::vector<int4> cost_sorted_tasks(const std::vector<int64_t> &sg_blocks, int64_t span, int64_t w_lo, int64_t w_hi,
                                           int64_t tasks_per_unit, int64_t ppt_cap, bool half_words, int64_t mloc) {
    int64_t blocks_per_perm = 0;
    for (const int64_t bl : sg_blocks) blocks_per_perm += bl;
    const int64_t target = std::max<int64_t>(256, blocks_per_perm * span / tasks_per_unit);      // block-permutations per task
    struct TaskCost { int4 t; int64_t cost; };
    std::vector<TaskCost> tc;
    for (size_t g = 0; g < sg_blocks.size(); ++g) {
        const int64_t bl = sg_blocks[g];
        int64_t ppt = std::min<int64_t>(std::min<int64_t>(span, ppt_cap), std::max<int64_t>(16, target / bl));
        const int64_t chunks = ceil_div(span, ppt);
        ppt = ceil_div(span, chunks);
        for (int64_t c = 0; c < chunks; ++c) {
            const int64_t p0 = c * ppt, p1 = std::min<int64_t>(span, p0 + ppt);
            for (int64_t w = w_lo; w < w_hi; ++w)
                if (!half_words || (w >> 1) * 64 + (w & 1) * 32 < mloc)
                    tc.push_back({make_int4(static_cast<int>(w), static_cast<int>(g), static_cast<int>(p0), static_cast<int>(p1)),
                                  bl * (p1 - p0)});
        }
    }
    std::stable_sort(tc.begin(), tc.end(), [](const TaskCost &a, const TaskCost &b) { return a.cost > b.cost; });
    std::vector<int4> out(tc.size());
    for (size_t i = 0; i < tc.size(); ++i) out[i] = tc[i].t;
    return out;
}

// The blocked kernel's per-XCD queues: the tasks of one (slice group, permutation range) -- one per word group, adjacent after the
// stable sort -- go to one queue, (group, range) pairs dealt round-robin in heaviest-first order.  Returns the list queue by queue.
static inline std::vector<int4> split_xcd_queues(const std::vector<int4> &list, BitsQueues &bq) {
    std::vector<std::vector<int4>> q(8);
    int64_t pair = -1;
    int last_g = -1, last_p0 = -1;
    for (const int4 &t : list) {
        if (t.y != last_g || t.z != last_p0) {
            ++pair;
            last_g = t.y;
            last_p0 = t.z;
        }
        q[pair & 7].push_back(t);
    }
    std::vector<int4> out;
    out.reserve(list.size());
    bq.off[0] = 0;
    for (int k = 0; k < 8; ++k) {
        out.insert(out.end(), q[k].begin(), q[k].end());
        bq.off[k + 1] = static_cast<int>(out.size());
    }
    return out;
}

// The task lists of one launch plan of the bit-sliced forms (all but plan.key): one list per DISTINCT stage-launch size over all
// n_units column units (word groups, or their halves), then -- the exchange tail -- one per column chunk of xc_wpc word groups
// over the tail's permutations (starts[n_major] .. the end).  slots: workgroup slots of the chip; one task per slot and unit set.
// One list per launch size: the stream's stages are 32, 96, 128 ... and short last ones, and a list cut for 128 permutations
// leaves a 32-permutation launch with half-empty and empty tasks (each still reloads T): a 32-permutation launch took 207 us,
// 6.5 us per permutation against 3.2 in the long launches.
static inline void plan_bits_tasks(BitsTaskPlan &plan, const std::vector<int32_t> &slice_width, int64_t n_slices, int wv, int64_t slots,
                            const std::vector<int64_t> &starts, int64_t n_units, int64_t mloc, bool half_words, int64_t n_major,
                            int64_t n_tail, int64_t xc_wpc) {
    // queue depth per workgroup slot: every task reloads T and flushes its counters (64 wave-atomics + two 32 x 32 bit transposes
    // per wave: 11 % of the kernel at depth 2, tools/bits_ablate.py dbg=2), so as few tasks as fill the chip once -- depth 1 vs 2:
    // seeded step 3.52 -> 3.41 ms, 10 000 unseeded permutations 25.8 -> 24.4 ms (tools/exp_ab.sh; round 3 had chosen 2 while the
    // host stream bound the step)
    constexpr int64_t tasks_per_slot = 1;
    // SHORT launches (the ramp at the head of the stream, the stage behind the last draw: nothing else runs beside them) cost
    // ~150 us + 2 us per permutation alone on the chip (10 / 16 / 32 / 64 / 128 permutations: 160 / 200 / 186 / 266 / 413 us,
    // tools/r6/short_launch.sh): their heaviest slice group's tasks are the critical path (16 permutations x 40-49 blocks x
    // 420-700 clocks) and every wave-task carries 13 + 30 + 30-60 kclk of table load, start-up and counter flush.  Cutting
    // their tasks finer (4 or 8 permutations per task at least) shortened a lone 16-permutation launch to 170 / 145 us but the
    // seeded step got LONGER (3.16-3.34 -> 3.30-3.38 ms: twice the wave-tasks, each with its fixed part) -- not kept.
    const std::vector<int64_t> sg_blocks = slice_group_blocks(slice_width, n_slices, wv);
    // (a column chunk of the tail has fewer word groups: its tasks are cut so that ITS launch fills the slots once too -- with the
    // stage launches' task size a chunk of the last stage had 288 tasks for 960 slots and lasted as long as a whole stage)
    auto one_list = [&](int64_t span, int64_t w_lo, int64_t w_hi, int64_t list_span) {
        BitsQueues bq{};
        const int64_t tpu = std::max<int64_t>(1, ceil_div(tasks_per_slot * slots, std::max<int64_t>(1, w_hi - w_lo)));
        // (a task counts at most 255 permutations: eight counter levels)
        const std::vector<int4> one =
            w_hi > w_lo ? split_xcd_queues(cost_sorted_tasks(sg_blocks, span, w_lo, w_hi, tpu, 255, half_words, mloc), bq)
                        : std::vector<int4>();
        plan.list_queues.push_back(bq);
        plan.list_span.push_back(list_span);
        plan.list_first.push_back(static_cast<int64_t>(plan.tasks.size()));
        plan.list_count.push_back(static_cast<int64_t>(one.size()));
        plan.tasks.insert(plan.tasks.end(), one.begin(), one.end());
    };
    plan = BitsTaskPlan{};
    plan.launch_list.assign(std::max<int64_t>(n_major + n_tail, 1), 0);
    for (int64_t k = 0; k < n_tail; ++k) {             // one list per column chunk (possibly empty on a rank with fewer columns)
        const int64_t w_lo = std::min<int64_t>(k * xc_wpc, n_units);
        const int64_t w_hi = k + 1 == n_tail ? n_units : std::min<int64_t>((k + 1) * xc_wpc, n_units);
        plan.launch_list[n_major + k] = static_cast<int64_t>(plan.list_span.size());
        one_list(starts.back() - starts[n_major], w_lo, w_hi, -1 - k);          // (a list span that never matches a stage's)
    }
    for (int64_t c = 0; c < n_major; ++c) {
        const int64_t span_c = starts[c + 1] - starts[c];
        size_t k = 0;
        while (k < plan.list_span.size() && plan.list_span[k] != span_c) ++k;
        if (k == plan.list_span.size()) one_list(span_c, 0, n_units, span_c);
        plan.launch_list[c] = static_cast<int64_t>(k);
    }
}

// ---- Per-wave tasks of the blocked form.  A task of plan_bits_tasks gives its four waves four ADJACENT slices over one permutation
// range, and the waves meet at the barrier at the task's end: the slices are sorted by width, so the wave of the narrowest one
// waits for the widest (the headline network's first group: 34 / 30 / 26 / 23 blocks per permutation; over all groups 404
// wave-blocks occupied for 341 used).  Here every wave gets an item of its own -- (slice, permutation range) -- and four items
// of about equal cost make a task.

// The items of one column unit over a launch of `span`: (slice, p0, p1) and the cost (blocks of the slice + 1) x permutations
// (the one: what a permutation costs beside its blocks -- compare and count).  Every slice with blocks is cut into ranges of
// about total cost / (4 tasks_per_unit), at least 16 and at most 255 permutations (eight counter levels), equal to within one
// permutation; a slice without blocks has no item (its sums and counters are zero either way).  At most max_items items where
// one range of 255 permutations per slice allows it: the ranges grow until they fit.  Stably sorted heaviest first.
struct BitsWaveItem {
    int slice, p0, p1;
    int64_t cost;
};
static inline std::vector<BitsWaveItem> wave_items(const std::vector<int32_t> &slice_width, int64_t n_slices, int64_t span,
                                                   int64_t tasks_per_unit, int64_t max_items) {
    constexpr int64_t per_perm = 1;
    int64_t cost_per_perm = 0;
    for (int64_t s = 0; s < n_slices; ++s)
        if (slice_width[s] / 8 > 0) cost_per_perm += slice_width[s] / 8 + per_perm;
    std::vector<BitsWaveItem> items;
    if (cost_per_perm == 0 || span <= 0) return items;
    const int64_t ppt_max = std::min<int64_t>(span, 255);
    int64_t target = std::max<int64_t>(1, cost_per_perm * span / (4 * tasks_per_unit));
    for (;;) {
        items.clear();
        bool cut = false;                                                   // a slice has more ranges than the 255 permutations force
        for (int64_t s = 0; s < n_slices; ++s) {
            const int64_t cps = slice_width[s] / 8 + per_perm;
            if (cps == per_perm) continue;
            const int64_t ppt = std::min<int64_t>(ppt_max, std::max<int64_t>(16, target / cps));
            const int64_t chunks = ceil_div(span, ppt);
            cut = cut || ppt < ppt_max;
            for (int64_t c = 0; c < chunks; ++c) {
                const int64_t p0 = c * span / chunks, p1 = (c + 1) * span / chunks;
                items.push_back({static_cast<int>(s), static_cast<int>(p0), static_cast<int>(p1), cps * (p1 - p0)});
            }
        }
        if (static_cast<int64_t>(items.size()) <= max_items || !cut) break;
        target += target / 8 + 1;
    }
    std::stable_sort(items.begin(), items.end(), [](const BitsWaveItem &a, const BitsWaveItem &b) { return a.cost > b.cost; });
    return items;
}

// The per-wave lists of the blocked form, beside the lists of plan_bits_tasks (which it calls first: the list bookkeeping --
// list_span, launch_list, one list per distinct launch size and per column chunk of the tail -- is that function's, and so is
// everything else it writes).  List k: wave_count[k] tasks from task wave_first[k], task t = the records wave_recs[4 t .. 4 t + 3],
// wave i's {column unit, slice, p0, p1}; slice -1: no item for this wave.  Four consecutive items of wave_items make a QUAD, and
// a quad's tasks -- one per column unit, all four records naming that unit: the waves share the word column -- go to one queue
// (the quad's id lists are then fetched into one XCD's L2 only, as with split_xcd_queues), quads dealt round-robin in
// heaviest-first order.  Items per unit: at most four times the tasks per unit of the list's tasks of plan_bits_tasks.
static inline void plan_bits_wave_tasks(BitsTaskPlan &plan, const std::vector<int32_t> &slice_width, int64_t n_slices, int64_t slots,
                                        const std::vector<int64_t> &starts, int64_t n_units, int64_t mloc, int64_t n_major,
                                        int64_t n_tail, int64_t xc_wpc) {
    plan_bits_tasks(plan, slice_width, n_slices, 4, slots, starts, n_units, mloc, false, n_major, n_tail, xc_wpc);
    for (size_t k = 0; k < plan.list_span.size(); ++k) {
        int64_t span = plan.list_span[k], w_lo = 0, w_hi = n_units;
        if (span < 0) {                                                     // the list of column chunk -1 - span of the tail
            const int64_t chunk = -1 - span;
            span = starts.back() - starts[n_major];
            w_lo = std::min<int64_t>(chunk * xc_wpc, n_units);
            w_hi = chunk + 1 == n_tail ? n_units : std::min<int64_t>((chunk + 1) * xc_wpc, n_units);
        }
        const int64_t units = std::max<int64_t>(0, w_hi - w_lo);
        std::vector<std::vector<int4>> q(8);
        if (units > 0) {
            const int64_t tpu = std::max<int64_t>(1, ceil_div(slots, units));
            const std::vector<BitsWaveItem> items = wave_items(slice_width, n_slices, span, tpu, 4 * (plan.list_count[k] / units));
            for (size_t i = 0; i < items.size(); i += 4)
                for (int64_t w = w_lo; w < w_hi; ++w)
                    for (size_t j = i; j < i + 4; ++j)
                        q[(i / 4) & 7].push_back(j < items.size() ? make_int4(static_cast<int>(w), items[j].slice, items[j].p0, items[j].p1)
                                                                  : make_int4(static_cast<int>(w), -1, 0, 0));
        }
        BitsQueues bq{};
        plan.wave_first.push_back(static_cast<int64_t>(plan.wave_recs.size() / 4));
        for (int i = 0; i < 8; ++i) {
            plan.wave_recs.insert(plan.wave_recs.end(), q[i].begin(), q[i].end());
            bq.off[i + 1] = static_cast<int>(plan.wave_recs.size() / 4 - plan.wave_first.back());
        }
        plan.wave_count.push_back(bq.off[8]);
        plan.wave_queues.push_back(bq);
    }
}
