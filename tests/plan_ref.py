"""The launch plans that are sized from the chip's CU count, restated in plain Python as functions of (shape, CU count), and
the shapes of tests/test_gpu_plan_cus.py.  Nothing here touches the library: tests/test_plan_ref_cpu.py checks on the CPU that
every shape reaches a second pass on a small planning CU count (SAFE_HIP_PLAN_CUS) and makes a single one on the whole chip.

Two kinds of plan:
  strided   a workgroup (or one of its waves) takes the units first, first + stride, ...: the functions return the passes of
            every workgroup or wave, so the largest, the smallest and a partly filled last stride can be read off;
  queue     `slots` persistent workgroups fetch tasks from a dynamic queue: the functions return the slot count and the task
            count (or bounds on it).  With more tasks than slots some workgroup takes a second one whatever the timing; with
            at most as many tasks as slots the launch has a workgroup per task.

The formulas ("Launch plans sized from the CU count"):
  k_permtest_weighted, k_permtest_gather   n_groups = max(1, min(ceil(n_slices / 4), ceil(8 CU / n_tiles))); wave w of group g
                                           takes slices g + n_groups w, + 4 n_groups, ...
  k_maxt_extremes                          n_groups = max(1, min(n_chunks, ceil(8 CU / (n_tiles n_pblocks)))); group g takes
                                           chunks g, g + n_groups, ...
  k_permtest_scatter                       min(m, CU per_cu) workgroups, one attribute per task
  k_permtest_lds                           min(tasks, CU per_cu) workgroups; cost_sorted_tasks emits, per (group of 16 slices,
                                           column tile), ceil(span / ppt) tasks with ppt >= min(span, 16) and span <= P
  k_select_xy, k_select_dist               min(units, 4 CU) workgroups stride over the 64 x 256 tiles / over the rows
  k_shortpath                              min(n, 8 CU) one-wave workers stride over the sources
  k_euclid_dense                           prep_ref.dense_geometry"""
import collections

import numpy as np

FULL_CUS = 256                                  # an MI355X
SLICE_ROWS = 64                                 # rows of a SELL slice
LDS_BUDGET = 160 * 1024                         # bytes of LDS the per-CU slot counts are cut for


def ceil_div(a, b):
    return -(-int(a) // int(b))


def strided(units, workers):
    """Passes of workers 0 .. workers - 1 over units 0 .. units - 1, worker w taking w, w + workers, ..."""
    return np.array([max(0, ceil_div(units - w, workers)) for w in range(workers)], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------ strided plans ----

def slice_tiles(m, score='sum'):
    """Column tiles of k_permtest_gather (16 columns for 'sum', 8 for 'z-score') and of k_permtest_weighted (16)."""
    return ceil_div(m, 8 if score == 'z-score' else 16)


def slice_plan(n, n_tiles, num_cu):
    """(n_groups, passes [n_groups, 4]) of k_permtest_weighted / k_permtest_gather: passes[g, w] slices for wave w of a
    workgroup of slice group g (the same for every column tile)."""
    n_slices = ceil_div(n, SLICE_ROWS)
    n_groups = max(1, min(ceil_div(n_slices, 4), ceil_div(8 * num_cu, n_tiles)))
    passes = np.array([[len(range(g + n_groups * w, n_slices, 4 * n_groups)) for w in range(4)] for g in range(n_groups)], dtype=np.int64)
    assert passes.sum() == n_slices
    return n_groups, passes


def maxt_plan(n, m, n_perm, num_cu):
    """(n_groups, passes [n_groups]) of k_maxt_extremes: chunks of 16 rows a workgroup of group g walks (the same for every
    column tile and block of 256 permutations)."""
    n_tiles, n_pblocks, n_chunks = ceil_div(m, 16), ceil_div(n_perm, 256), ceil_div(n, 16)
    n_groups = max(1, min(n_chunks, ceil_div(8 * num_cu, n_tiles * n_pblocks)))
    return n_groups, strided(n_chunks, n_groups)


def select_xy_plan(n, num_cu):
    """Passes of the workgroups of k_select_xy over the ceil(n / 64) x ceil(n / 256) tiles."""
    tiles = ceil_div(n, 64) * ceil_div(n, 256)
    return strided(tiles, min(tiles, 4 * num_cu))


def select_dist_plan(n, num_cu):
    """Passes of the workgroups of k_select_dist over rows 0 .. n - 2."""
    return strided(n - 1, min(n - 1, 4 * num_cu))


def shortpath_plan(n, num_cu):
    """Sources per worker of k_shortpath."""
    return strided(n, min(n, 8 * num_cu))


# -------------------------------------------------------------------------------------------------------- queue plans ----

Queue = collections.namedtuple('Queue', 'slots tasks_lo tasks_hi')


def per_cu(lds_bytes):
    return max(1, min(8, LDS_BUDGET // lds_bytes))


def scatter_plan(n, m, num_cu):
    """k_permtest_scatter: one task per attribute; EP, CT (u32 [n]), the queue slot and SO (u16 [n]) in LDS."""
    lds = (2 * n + 4) * 4 + ((n + 1) & ~1) * 2
    return Queue(num_cu * per_cu(lds), m, m)


def lds_plan(n, m, score, n_perm, num_cu):
    """k_permtest_lds: column tiles of 4 ('sum') or 1 ('z-score') columns; bounds on the task count of one launch."""
    n_tiles = m if score == 'z-score' else ceil_div(m, 4)
    stride16 = ceil_div(n + 1, 8) * 8
    lds = (8 * (n + 1) + stride16 + 4) * 4
    units = ceil_div(ceil_div(n, SLICE_ROWS), 16) * n_tiles
    return Queue(num_cu * per_cu(lds), units, units * ceil_div(n_perm, 16))


# -------------------------------------------------------------------------------------------------------- summaries ----

Passes = collections.namedtuple('Passes', 'most least')         # of the busiest and of the idlest worker; least None: not known


def of_strided(passes):
    return Passes(int(np.max(passes)), int(np.min(passes)))


def of_queue(q):
    """most: what some workgroup takes at least (pigeonhole on the lower bound); a launch whose tasks all find a slot of their
    own counts as one pass.  least is known only where the task count is."""
    most = 1 if q.tasks_hi <= q.slots else ceil_div(q.tasks_lo, q.slots)
    least = q.tasks_lo // min(q.slots, q.tasks_lo) if q.tasks_lo == q.tasks_hi else None
    return Passes(most, least)


# ------------------------------------------------------------------------------------- the shapes of the GPU tests ----

SMALL_CUS = (1, 2)

WEIGHTED = {'n': 600, 'm': 130, 'n_perm': 12}
GATHER = {'sum': {'n': 600, 'm': 130, 'n_perm': 24}, 'z-score': {'n': 600, 'm': 70, 'n_perm': 24}}   # (24: a cell can pass the 0.05 threshold)
MAXT = {'n': 100, 'm': 20, 'n_perm': 300}
SCATTER = {'n': 300, 'm': 40, 'n_perm': 24}
SCATTER_HUB = {'n': 2100, 'm': 24, 'n_perm': 24}
LDS = {'sum': {'n': 600, 'm': 60, 'n_perm': 40}, 'z-score': {'n': 600, 'm': 40, 'n_perm': 40}}
SELECT = {'n': 300}
SHORTPATH = {'workers': 40, 'n': 101}                      # shortpath_ref.rung_graph(40, 1): n = 101


def gpu_cases():
    """{case name: (kernel, CU counts the case runs at besides the whole chip, CU count -> Passes)}"""
    w, mx, sc, hub, sel = WEIGHTED, MAXT, SCATTER, SCATTER_HUB, SELECT
    cases = {
        'weighted': ('k_permtest_weighted', SMALL_CUS, lambda k: of_strided(slice_plan(w['n'], slice_tiles(w['m']), k)[1])),
        'maxt': ('k_maxt_extremes', SMALL_CUS, lambda k: of_strided(maxt_plan(mx['n'], mx['m'], mx['n_perm'], k)[1])),
        'scatter': ('k_permtest_scatter', SMALL_CUS, lambda k: of_queue(scatter_plan(sc['n'], sc['m'], k))),
        'scatter_hub': ('k_permtest_scatter', SMALL_CUS, lambda k: of_queue(scatter_plan(hub['n'], hub['m'], k))),
        'select_xy': ('k_select_xy', SMALL_CUS, lambda k: of_strided(select_xy_plan(sel['n'], k))),
        'select_dist': ('k_select_dist', SMALL_CUS, lambda k: of_strided(select_dist_plan(sel['n'], k))),
        'shortpath': ('k_shortpath', SMALL_CUS, lambda k: of_strided(shortpath_plan(SHORTPATH['n'], k))),
    }
    for score, g in GATHER.items():
        cases['gather_' + score] = ('k_permtest_gather', SMALL_CUS,
                                    lambda k, g=g, score=score: of_strided(slice_plan(g['n'], slice_tiles(g['m'], score), k)[1]))
    for score, g in LDS.items():
        cases['lds_' + score] = ('k_permtest_lds', SMALL_CUS,
                                 lambda k, g=g, score=score: of_queue(lds_plan(g['n'], g['m'], score, g['n_perm'], k)))
    return cases
