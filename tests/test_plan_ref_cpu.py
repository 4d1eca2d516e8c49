"""The shapes of tests/test_gpu_plan_cus.py against the launch formulas of tests/plan_ref.py, on the CPU: (a) at the case's
small planning CU counts some workgroup or wave makes a second pass; (b) for at least one of them per kernel the passes are
uneven, so the last stride (or the last round of a queue) is partly filled; (c) on the whole chip, 256 CUs, the same shape
makes exactly one pass -- which is why the case needs SAFE_HIP_PLAN_CUS.

(b) is not claimed for k_permtest_lds: its task count depends on the slice widths and the launch spans, plan_ref bounds it
from both sides only."""
import numpy as np
import pytest

import plan_ref as pl
import prep_ref as pr

CASES = pl.gpu_cases()
UNEVEN_EXEMPT = {'k_permtest_lds'}


@pytest.mark.parametrize('name', sorted(CASES))
def test_small_plans_make_a_second_pass_and_the_whole_chip_makes_one(name):
    kernel, cus, passes = CASES[name]
    for k in cus:
        p = passes(k)
        print('%s (%s) at %d CUs: busiest %d, idlest %s' % (name, kernel, k, p.most, p.least))
        assert p.most >= 2, (name, k, p)                                                            # (a)
    full = passes(pl.FULL_CUS)
    print('%s (%s) at %d CUs: busiest %d' % (name, kernel, pl.FULL_CUS, full.most))
    assert full.most == 1, (name, full)                                                             # (c)


@pytest.mark.parametrize('kernel', sorted({c[0] for c in CASES.values()} - UNEVEN_EXEMPT))
def test_every_kernel_has_a_partly_filled_last_stride(kernel):
    uneven = [(name, k) for name, (kern, cus, passes) in CASES.items() if kern == kernel
              for k in cus if passes(k).least is not None and passes(k).least < passes(k).most]
    print('%s: uneven at %s' % (kernel, uneven))
    assert uneven, kernel                                                                           # (b)


def test_the_figures_of_the_weighted_and_the_extremes_plan():
    """The passes by hand, once: 10 slices on one group are 3, 3, 2, 2 per wave; on two groups only wave 0 comes back.
    7 chunks on two groups are 4 and 3, on four groups 2, 2, 2, 1."""
    w = pl.WEIGHTED
    assert pl.slice_tiles(w['m']) == 9 > 8                                                          # more tiles than XCD queues
    n_groups, passes = pl.slice_plan(w['n'], 9, 1)
    assert n_groups == 1 and passes.tolist() == [[3, 3, 2, 2]]
    n_groups, passes = pl.slice_plan(w['n'], 9, 2)
    assert n_groups == 2 and passes.tolist() == [[2, 1, 1, 1], [2, 1, 1, 1]]
    assert pl.slice_plan(w['n'], 9, pl.FULL_CUS)[1].tolist() == [[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 0]]
    assert pl.slice_tiles(70, 'z-score') == 9
    mx = pl.MAXT
    assert [pl.maxt_plan(mx['n'], mx['m'], mx['n_perm'], k)[1].tolist() for k in (1, 2)] == [[4, 3], [2, 2, 2, 1]]
    assert pl.maxt_plan(mx['n'], mx['m'], mx['n_perm'], pl.FULL_CUS)[0] == 7
    assert mx['n_perm'] - 256 == 44                                     # live lanes of wave 0 of the second permutation block


def test_the_figures_of_the_queues_and_the_selection():
    assert pl.scatter_plan(300, 40, 1) == pl.Queue(8, 40, 40) and pl.scatter_plan(300, 40, 2).slots == 16
    assert pl.scatter_plan(2100, 24, 1).slots == 7                      # 21 016 bytes of LDS: seven workgroups a CU
    for score, tiles in (('sum', 15), ('z-score', 40)):                 # 21 680 bytes of LDS: seven workgroups a CU
        g = pl.LDS[score]
        assert [pl.lds_plan(g['n'], g['m'], score, g['n_perm'], k).slots for k in (1, 2)] == [7, 14]
        assert pl.lds_plan(g['n'], g['m'], score, g['n_perm'], 2).tasks_lo == tiles > 14
        assert g['n'] * g['m'] <= 204800                                # a narrow block: the route's own choice
    assert pl.select_xy_plan(300, 1).tolist() == [3, 3, 2, 2] and pl.select_xy_plan(300, 2).tolist() == [2, 2, 1, 1, 1, 1, 1, 1]
    assert sorted(set(pl.shortpath_plan(101, 1).tolist())) == [12, 13] and len(pl.shortpath_plan(101, 1)) == 8


def test_the_strided_passes_cover_every_unit_once():
    for units in (0, 1, 7, 8, 9, 101):
        for workers in (1, 2, 8, 100):
            taken = np.zeros(units, dtype=np.int64)
            for w in range(workers):
                taken[w::workers] += 1
                assert pl.strided(units, workers)[w] == len(range(w, units, workers))
            assert (taken == 1).all()


def test_the_dense_sweep_runs_whole_batches_on_one_cu_only():
    """prep_ref.dense_sizes(1): whole batches from n = 29 on, in both store forms; none of those sizes on 256 CUs."""
    nb, sizes = pr.dense_sizes(1)
    assert nb == 29
    batched = [n for n in sizes.values() if pr.dense_geometry(n, 1)[2]]
    assert batched and {n % 2 for n in batched} == {0, 1} and max(sizes.values()) <= 1025
    assert any(not pr.dense_geometry(n, 1)[2] for n in sizes.values())
    assert not any(pr.dense_geometry(n, pl.FULL_CUS)[2] for n in sizes.values())
