"""The per-wave task lists of the blocked bit-sliced kernel (safepy_amd/csrc/bits_plan.h: plan_bits_wave_tasks) built for the host
with the system C++ compiler and run as a program, as tests/test_bits_plan_cpu.py does for the lists of plan_bits_tasks -- with
the address and undefined-behaviour sanitizers where the compiler links them.  Part one: the invariants every list must hold, on
seeded random inputs.  Part two: the balance of the four waves of a task on the headline network's slice widths.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_bits_plan_cpu import BLK, XC_MAX, case_text, plan_case, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')

# One line of integers per result and plan case: "tail", "list_span", "list_count" (the tasks of plan_bits_tasks' list),
# "launch_list", "wave_first", "wave_count", "wave_queues", "wave_recs".  Input: the "plan" lines of tests/test_bits_plan_cpu.py.
DRIVER = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "bits_plan.h"
static void put(const char *name, const std::vector<long long> &v) {
    std::printf("%s", name);
    for (long long x : v) std::printf(" %lld", x);
    std::printf("\n");
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char what[16];
    while (std::fscanf(f, "%15s", what) == 1) {
        if (std::strcmp(what, "plan")) return 4;
        int kind, xc_want;
        long long slots, mloc, xc_cols, n_slices, n_starts;
        double frac;
        if (std::fscanf(f, "%d %lld %lld %d %lld %lf %lld", &kind, &slots, &mloc, &xc_want, &xc_cols, &frac, &n_slices) != 7) return 3;
        if (kind != BITS_BLK) return 5;
        std::vector<int32_t> widths(n_slices);
        for (auto &w : widths)
            if (std::fscanf(f, "%d", &w) != 1) return 3;
        if (std::fscanf(f, "%lld", &n_starts) != 1) return 3;
        std::vector<int64_t> starts(n_starts);
        for (auto &s : starts) {
            long long v;
            if (std::fscanf(f, "%lld", &v) != 1) return 3;
            s = v;
        }
        const int64_t n_units = ceil_div(mloc, 64);
        const BitsTail t = bits_tail_split(xc_want, xc_cols, XC_MAX_, true, starts, starts.back(), mloc, frac);
        BitsTaskPlan plan, old;
        plan_bits_wave_tasks(plan, widths, n_slices, slots, starts, n_units, mloc, t.n_major, t.n_chunks, t.wpc);
        // what plan_bits_tasks writes stays what it writes on its own
        plan_bits_tasks(old, widths, n_slices, 4, slots, starts, n_units, mloc, false, t.n_major, t.n_chunks, t.wpc);
        if (old.tasks.size() != plan.tasks.size() || old.list_span != plan.list_span || old.list_first != plan.list_first ||
            old.list_count != plan.list_count || old.launch_list != plan.launch_list)
            return 6;
        for (size_t i = 0; i < old.tasks.size(); ++i)
            if (std::memcmp(&old.tasks[i], &plan.tasks[i], sizeof(int4))) return 6;
        for (size_t i = 0; i < old.list_queues.size(); ++i)
            if (std::memcmp(&old.list_queues[i], &plan.list_queues[i], sizeof(BitsQueues))) return 6;
        put("tail", {t.n_major, t.p_split, t.n_chunks, t.wpc});
        std::vector<long long> rc, q;
        for (const int4 &k : plan.wave_recs) { rc.push_back(k.x); rc.push_back(k.y); rc.push_back(k.z); rc.push_back(k.w); }
        for (const BitsQueues &b : plan.wave_queues)
            for (int i = 0; i < 9; ++i) q.push_back(b.off[i]);
        put("list_span", std::vector<long long>(plan.list_span.begin(), plan.list_span.end()));
        put("list_count", std::vector<long long>(plan.list_count.begin(), plan.list_count.end()));
        put("launch_list", std::vector<long long>(plan.launch_list.begin(), plan.launch_list.end()));
        put("wave_first", std::vector<long long>(plan.wave_first.begin(), plan.wave_first.end()));
        put("wave_count", std::vector<long long>(plan.wave_count.begin(), plan.wave_count.end()));
        put("wave_queues", q);
        put("wave_recs", rc);
    }
    std::fclose(f);
    return 0;
}
'''.replace('XC_MAX_', str(XC_MAX))

KEYS = ('tail', 'list_span', 'list_count', 'launch_list', 'wave_first', 'wave_count', 'wave_queues', 'wave_recs')

# the slice widths of the headline network (workloads.costanzo_surrogate(seed=0), shortest-path neighborhoods: 63 slices,
# 341 blocks), 69 word groups of attributes
HEADLINE_WIDTHS = [272, 240, 208, 184, 168, 144, 128, 104, 96, 80, 72, 64, 64, 56, 48, 40, 40, 32, 32, 32, 32, 24, 24, 24,
                   24, 24, 24, 24] + [16] * 18 + [8] * 17
HEADLINE_UNITS = 69


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed to build the planning header for the CPU'
    d = tmp_path_factory.mktemp('bits_wave_plan')
    (d / 'drv.cpp').write_text(DRIVER)
    hip_inc = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include')
    base = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-D__HIP_PLATFORM_AMD__', '-I' + hip_inc, '-I' + CSRC, str(d / 'drv.cpp'),
            '-o', str(d / 'drv')]
    # a stand-alone program: the sanitizers are linked into it where the compiler has them and their runtime starts (an empty
    # input runs none of the code under test), else it is built plain
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    (d / 'in.txt').write_text('')
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0 or \
            subprocess.run([str(d / 'drv'), str(d / 'in.txt')], capture_output=True, env=env).returncode != 0:
        subprocess.run(base, check=True)

    def run(cases):
        (d / 'in.txt').write_text(''.join(case_text(c) for c in cases))
        out = subprocess.run([str(d / 'drv'), str(d / 'in.txt')], check=True, capture_output=True, text=True, env=env).stdout
        rows = [ln.split() for ln in out.splitlines()]
        assert len(rows) == len(KEYS) * len(cases)
        plans = []
        for i in range(len(cases)):
            one = {}
            for k, r in zip(KEYS, rows[len(KEYS) * i:len(KEYS) * (i + 1)]):
                assert r[0] == k
                one[k] = np.array([int(x) for x in r[1:]], dtype=np.int64)
            one['wave_queues'] = one['wave_queues'].reshape(-1, 9)
            one['wave_recs'] = one['wave_recs'].reshape(-1, 4, 4)               # [task][wave][unit, slice, p0, p1]
            plans.append(one)
        return plans
    return run


def launch_ranges(c, p):
    """(list, span, first unit, end unit) of every launch of a plan case, as launch_bits cuts them."""
    starts, n_units = c['starts'], -(-c['mloc'] // 64)
    n_major, p_split, n_chunks, wpc = (int(x) for x in p['tail'])
    for ln, li in enumerate(p['launch_list']):
        if ln < n_major:
            yield int(li), starts[ln + 1] - starts[ln], 0, n_units, False
        else:
            k = ln - n_major
            yield int(li), starts[-1] - p_split, min(k * wpc, n_units), n_units if k + 1 == n_chunks else min((k + 1) * wpc, n_units), True


def test_every_wave_list_covers_its_launch_exactly_once(planner):
    """On 200 seeded random inputs of the blocked form, for every launch's list: each (column unit of the launch's range, slice
    with blocks, permutation of the launch's span) is in exactly one item and a slice without blocks in none; no item counts more
    than 255 permutations; the four records of a task name one column unit; the queue offsets start at 0, never decrease and end
    at the list's count; the tasks of one item quad -- one per column unit -- sit in one queue; stage launches of equal span
    share one list; a tail chunk's list names its own units only; a unit has at most four times as many items as tasks of
    plan_bits_tasks."""
    r = np.random.default_rng(20240607)
    cases = []
    while len(cases) < 200:
        c = random_case(r)
        c['kind'] = BLK
        cases.append(c)
    plans = planner(cases)
    n_tails = n_empty_waves = n_same_slice = 0
    for c, p in zip(cases, plans):
        w8 = np.array(c['widths']) // 8
        n_tails += int(p['tail'][2]) > 0
        assert len(p['wave_first']) == len(p['wave_count']) == len(p['wave_queues']) == len(p['list_span'])
        assert p['wave_count'].sum() == len(p['wave_recs'])
        for q, cnt in zip(p['wave_queues'], p['wave_count']):
            assert q[0] == 0 and np.all(np.diff(q) >= 0) and q[8] == cnt
        span_list = {}
        for li, span, w_lo, w_hi, in_tail in launch_ranges(c, p):
            if not in_tail:
                assert span_list.setdefault(span, li) == li and p['list_span'][li] == span
                assert len(set(span_list.values())) == len(span_list)
            t = p['wave_recs'][p['wave_first'][li]:p['wave_first'][li] + p['wave_count'][li]]
            units = max(w_hi - w_lo, 0)
            cover = np.zeros((units, len(w8), span), dtype=np.int32)
            items = np.zeros(units, dtype=np.int64)
            quad_queue = {}
            for ti, task in enumerate(t):
                assert len({int(w) for w in task[:, 0]}) == 1 and w_lo <= task[0, 0] < w_hi, (c, li, task)
                queue = int(np.searchsorted(p['wave_queues'][li], ti, side='right')) - 1
                quad = tuple(int(x) for x in task[:, 1:].ravel())
                assert quad_queue.setdefault(quad, queue) == queue
                slices = [int(s) for s in task[:, 1] if s >= 0]
                n_same_slice += len(set(slices)) < len(slices)
                for w, s, p0, p1 in task:
                    if s < 0:
                        n_empty_waves += 1
                        continue
                    assert s < len(w8) and w8[s] > 0 and 0 <= p0 < p1 <= span and p1 - p0 <= 255
                    cover[w - w_lo, s, p0:p1] += 1
                    items[w - w_lo] += 1
            assert np.all(cover == (w8 > 0).astype(np.int32)[None, :, None]), (c, li)
            if units:
                assert p['list_count'][li] % units == 0 and np.all(items <= 4 * (p['list_count'][li] // units)), (c, li)
                assert len(t) == len(quad_queue) * units                       # every quad has one task per unit
    assert n_tails >= 5 and n_empty_waves > 0 and n_same_slice > 0            # the cases hit what the checks are for


@pytest.mark.parametrize('span', [200, 128])
@pytest.mark.parametrize('slots', [768, 1024])
def test_waves_of_a_task_are_balanced_on_the_headline_shape(planner, span, slots):
    """The headline network's 63 slice widths, 69 column units, launches of 200 (resident table) and 128 (drawn stream)
    permutations, 768 and 1024 workgroup slots: a task occupies its four waves for as long as its heaviest item, cost (blocks
    + 1) x permutations; summed over the tasks, 4 x the heaviest item's cost is at most 1.05 of the items' cost (adjacent
    slices over one range: 1.158); a unit has at most four times as many items as tasks of plan_bits_tasks."""
    c = plan_case(BLK, slots, HEADLINE_UNITS * 64, [0, span], HEADLINE_WIDTHS)
    p = planner([c])[0]
    assert len(HEADLINE_WIDTHS) == 63 and sum(HEADLINE_WIDTHS) // 8 == 341
    assert list(p['launch_list']) == [0] and p['list_count'][0] % HEADLINE_UNITS == 0
    t = p['wave_recs']
    w8 = np.array(HEADLINE_WIDTHS + [0]) // 8                                 # (slice -1: no item, cost 0)
    cost = np.where(t[:, :, 1] >= 0, (w8[t[:, :, 1]] + 1) * (t[:, :, 3] - t[:, :, 2]), 0)
    occupied, used = 4 * cost.max(axis=1).sum(), cost.sum()
    assert used == HEADLINE_UNITS * (341 + 63) * span
    items_per_unit = int((t[:, :, 1] >= 0).sum()) // HEADLINE_UNITS
    print('span %d slots %d: occupied / used = %.4f, %d items per unit, %d tasks per unit of plan_bits_tasks'
          % (span, slots, occupied / used, items_per_unit, p['list_count'][0] // HEADLINE_UNITS))
    assert occupied <= 1.05 * used, occupied / used
    assert items_per_unit <= 4 * (p['list_count'][0] // HEADLINE_UNITS)
