"""The planning arithmetic of the bit-sliced permutation launch (safepy_amd/csrc/bits_plan.h: form and geometry, tail split,
task lists, queue split) built for the host with the system C++ compiler and run as a program -- with the address and
undefined-behaviour sanitizers where the compiler links them.  Part one: exact equality with the record of the code before it
moved into the header (tests/golden/bits_plan.npz).  Part two: the invariants every task list must hold, on seeded random
inputs.  No GPU needed; the launches themselves are pinned by the tests/test_gpu_*.py parity tests."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bits_plan.npz')
BLK, PRE16, PRE32 = 1, 2, 3                       # BitsKind
XC_MAX = 8                                        # safe_ctx::XC_MAX, passed to the tail split as a plain number

# One line of integers per result: "form ..." per form case; "tail", "tasks", "list_span", "list_first", "list_count",
# "launch_list", "queues" per plan case.  A plan case runs what launch_bits runs: the tail split, then plan_bits_tasks.
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
        if (!std::strcmp(what, "form")) {
            long long n, mc;
            int col2;
            if (std::fscanf(f, "%lld %lld %d", &n, &mc, &col2) != 3) return 3;
            const BitsForm fm = bits_form(n, mc, col2 != 0, 160 * 1024);
            put("form", {fm.kind, fm.levels, fm.waves, fm.block, fm.id_shift, fm.half ? 1 : 0, static_cast<long long>(fm.lds_bytes),
                         fm.wgs_per_cu});
        } else if (!std::strcmp(what, "plan")) {
            int kind, xc_want;
            long long slots, mloc, xc_cols, n_slices, n_starts;
            double frac;
            if (std::fscanf(f, "%d %lld %lld %d %lld %lf %lld", &kind, &slots, &mloc, &xc_want, &xc_cols, &frac, &n_slices) != 7) return 3;
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
            const bool blk = kind == BITS_BLK, half = kind == BITS_PRE32;
            const int64_t n_wg = ceil_div(mloc, 64), n_units = half ? 2 * n_wg : n_wg;
            const BitsTail t = bits_tail_split(xc_want, xc_cols, XC_MAX_, blk, starts, starts.back(), mloc, frac);
            BitsTaskPlan plan;
            plan_bits_tasks(plan, widths, n_slices, blk ? 4 : 16, slots, starts, n_units, mloc, half, t.n_major, t.n_chunks, t.wpc);
            put("tail", {t.n_major, t.p_split, t.n_chunks, t.wpc});
            std::vector<long long> tk, q;
            for (const int4 &k : plan.tasks) { tk.push_back(k.x); tk.push_back(k.y); tk.push_back(k.z); tk.push_back(k.w); }
            for (const BitsQueues &b : plan.list_queues)
                for (int i = 0; i < 9; ++i) q.push_back(b.off[i]);
            put("tasks", tk);
            put("list_span", std::vector<long long>(plan.list_span.begin(), plan.list_span.end()));
            put("list_first", std::vector<long long>(plan.list_first.begin(), plan.list_first.end()));
            put("list_count", std::vector<long long>(plan.list_count.begin(), plan.list_count.end()));
            put("launch_list", std::vector<long long>(plan.launch_list.begin(), plan.launch_list.end()));
            put("queues", q);
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
'''.replace('XC_MAX_', str(XC_MAX))

PLAN_KEYS = ('tail', 'tasks', 'list_span', 'list_first', 'list_count', 'launch_list', 'queues')


def ramp(p):
    """Launch boundaries shaped like the permutation stream's stages: 32, 96, then 128 each, a short last one."""
    b = [0] + [q for q in (32, 128) if q < p] + list(range(256, p, 128))
    if p - b[-1] > 48 and p > 128:
        b.append(p - 32)
    return b + [p]


def widths(n_slices, top, seed):
    """Slice widths as the SELL structure has them: multiples of 8, widest first."""
    r = np.random.default_rng(seed)
    return sorted((int(w) // 8 * 8 for w in r.integers(0, top + 1, n_slices)), reverse=True)


def plan_case(kind, slots, mloc, starts, w, xc_want=0, xc_cols=0, frac=0.0):
    return dict(kind=kind, slots=slots, mloc=mloc, starts=list(starts), widths=list(w), xc_want=xc_want, xc_cols=xc_cols, frac=frac)


# (n, max_count, has_col2): the boundaries of bits_form -- the 16-bit LDS offsets of the blocked form (8 (N + 1) < 65536), the
# word column of the sixteen-wave form against 160 KB (20 477 / 20 478), the u16 lists (32 767 / 32 768), ten / eleven / too many
# levels, and no resident 2 * id lists
FORMS = [(300, 200, 1), (8190, 100, 1), (8191, 100, 1), (20470, 100, 1), (20471, 100, 1), (20477, 100, 1), (20478, 100, 1),
         (32767, 100, 1), (32768, 100, 1), (2600, 1023, 1), (2600, 1024, 1), (2600, 2047, 1), (2600, 2048, 1), (25000, 1023, 1),
         (25000, 1024, 1), (25000, 2047, 1), (25000, 2048, 1), (8190, 1024, 1), (300, 200, 0), (25000, 100, 0)]

PLANS = [
    plan_case(BLK, 960, 1, [0, 1], [8]),                                               # one column, one slice, one permutation
    plan_case(BLK, 960, 64, [0, 32, 60], widths(3, 200, 1)),                           # two launches
    plan_case(BLK, 960, 65, ramp(1000), widths(10, 400, 2)),                           # more slices than a group of four
    plan_case(BLK, 8, 700, ramp(1000), widths(7, 120, 3)),                             # fewer slots than column units
    plan_case(BLK, 1024, 300, ramp(500), widths(5, 1000, 4)),
    plan_case(PRE16, 240, 64, [0, 1], [1024]),                                         # sixteen waves, one slice
    plan_case(PRE16, 240, 65, ramp(500), widths(40, 2000, 5)),                         # more slices than a group of sixteen
    plan_case(PRE16, 16, 1, [0, 32, 60], widths(17, 64, 6)),
    plan_case(PRE32, 240, 1, [0, 1], [16]),
    plan_case(PRE32, 240, 33, ramp(300), widths(20, 300, 7)),                          # half words: 2, 4, 3 and 2 halves with columns
    plan_case(PRE32, 256, 97, ramp(300), widths(20, 300, 8)),
    plan_case(PRE32, 3, 65, [0, 32, 60], widths(33, 900, 9)),                          # (the fourth half has no columns: no task)
    plan_case(PRE32, 240, 64, ramp(1000), widths(2, 40, 10)),
    plan_case(BLK, 960, 100, ramp(300), widths(6, 200, 11), 2, 64, 0.4),               # a tail of two chunks, the second ragged
    plan_case(BLK, 960, 100, ramp(300), widths(6, 200, 11), 2, 64, 1e-9),              # ... of the last stage only
    plan_case(BLK, 960, 40, ramp(300), widths(6, 200, 12), 2, 64, 1e-9),               # ... whose last chunk has no word groups
    plan_case(BLK, 960, 500, ramp(1000), widths(12, 300, 13), 8, 64, 0.4),             # eight chunks
    plan_case(BLK, 64, 500, ramp(1000), widths(12, 300, 13), 12, 64, 1.0),             # more chunks wanted than XC_MAX, all in the tail
    plan_case(BLK, 960, 200, ramp(1000), widths(4, 80, 14), 3, 128, 0.2),              # three chunks of two word groups: 2 + 2 + 0
    plan_case(BLK, 960, 100, ramp(300), widths(6, 200, 11), 2, 100, 0.4),              # no tail: chunk not a multiple of 64 columns,
    plan_case(BLK, 960, 100, ramp(300), widths(6, 200, 11), 1, 64, 0.4),               # one chunk wanted,
    plan_case(BLK, 960, 100, [0, 32, 60], widths(6, 200, 11), 2, 64, 0.4),             # fewer than three launches,
    plan_case(BLK, 960, 200, ramp(300), widths(6, 200, 11), 2, 64, 0.4),               # chunks that do not cover the columns,
    plan_case(BLK, 960, 100, ramp(300), widths(6, 200, 11), 2, 64, 0.0),               # fraction zero,
    plan_case(PRE16, 240, 100, ramp(300), widths(6, 200, 11), 2, 64, 0.4),             # not the blocked form
]


def case_text(c):
    return 'plan %d %d %d %d %d %r %d %s %d %s\n' % (c['kind'], c['slots'], c['mloc'], c['xc_want'], c['xc_cols'], float(c['frac']),
                                                     len(c['widths']), ' '.join(map(str, c['widths'])), len(c['starts']),
                                                     ' '.join(map(str, c['starts'])))


def input_text(forms, plans):
    return ''.join('form %d %d %d\n' % f for f in forms) + ''.join(case_text(c) for c in plans)


def parse_output(out, n_forms, n_plans):
    rows = [ln.split() for ln in out.splitlines()]
    got_forms = np.array([[int(x) for x in r[1:]] for r in rows if r[0] == 'form'], dtype=np.int64).reshape(-1, 8)
    rest = [r for r in rows if r[0] != 'form']
    assert len(got_forms) == n_forms and len(rest) == len(PLAN_KEYS) * n_plans
    got_plans = []
    for i in range(n_plans):
        one = {}
        for k, r in zip(PLAN_KEYS, rest[len(PLAN_KEYS) * i:len(PLAN_KEYS) * (i + 1)]):
            assert r[0] == k
            one[k] = np.array([int(x) for x in r[1:]], dtype=np.int64)
        one['tasks'] = one['tasks'].reshape(-1, 4)
        one['queues'] = one['queues'].reshape(-1, 9)
        got_plans.append(one)
    return got_forms, got_plans


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed to build the planning header for the CPU'
    d = tmp_path_factory.mktemp('bits_plan')
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

    def run(forms, plans):
        (d / 'in.txt').write_text(input_text(forms, plans))
        out = subprocess.run([str(d / 'drv'), str(d / 'in.txt')], check=True, capture_output=True, text=True, env=env).stdout
        return parse_output(out, len(forms), len(plans))
    return run


def test_forms_and_plans_equal_the_record(planner):
    """Every number equal to what the functions gave before they moved: form and geometry (kind, levels, waves, threads,
    id shift, half words, LDS bytes, workgroups per CU), tail split (stage launches, first tail permutation, chunks, word
    groups per chunk), tasks, list_span / list_first / list_count, launch_list, queue offsets."""
    want = np.load(GOLDEN)
    forms, plans = planner(FORMS, PLANS)
    assert np.array_equal(forms, want['form']), (forms, want['form'])
    assert {int(k) for k in forms[:, 0]} == {0, BLK, PRE16, PRE32} and {int(k) for k in forms[:, 1]} == {0, 10, 11}
    for i, p in enumerate(plans):
        for k in PLAN_KEYS:
            assert np.array_equal(p[k], want['%02d_%s' % (i, k)].reshape(p[k].shape)), (i, k)
    chunks = [int(p['tail'][2]) for p in plans]
    assert 2 in chunks and 8 in chunks and 3 in chunks and chunks.count(0) >= 6            # the cases hit what they are named for
    assert any(p['tail'][2] and p['list_count'][p['launch_list'][-1]] == 0 for p in plans)  # a last chunk without word groups


def random_case(r):
    kind = int(r.choice([BLK, PRE16, PRE32]))
    p = int(r.choice([1, 20, 60, 100, 300, 700, 1500])) + int(r.integers(0, 30))
    if r.random() < 0.25:
        span = int(r.integers(16, 200))
        starts = list(range(0, p, span)) + [p]
    else:
        starts = ramp(p)
    return plan_case(kind, int(r.choice([1, 8, 64, 256, 960, 1024, 2048])), int(r.choice([1, 33, 64, 65, 97, 128, int(r.integers(1, 700))])),
                     starts, widths(int(r.integers(1, 41)), int(r.choice([8, 64, 400, 2000])), int(r.integers(1 << 30))),
                     int(r.choice([0, 2, 3, 8, 12])), int(r.choice([64, 128, 256, 100])), float(r.choice([0.0, 1e-9, 0.2, 0.4, 1.0])))


def test_every_list_covers_its_launch_exactly_once(planner):
    """On 200 seeded random inputs, for every launch's list: each (column unit of the launch's range, slice group, permutation of
    the launch's span) is in exactly one task and a half-word unit without columns in none; no task counts more than 255
    permutations; the queue offsets start at 0, never decrease and end at the list's count; stage launches of equal span share
    one list."""
    r = np.random.default_rng(20240607)
    cases = [random_case(r) for _ in range(200)]
    _, plans = planner([], cases)
    n_tails = 0
    for c, p in zip(cases, plans):
        starts, mloc, half = c['starts'], c['mloc'], c['kind'] == PRE32
        n_wg = -(-mloc // 64)
        n_units = 2 * n_wg if half else n_wg
        n_groups = -(-len(c['widths']) // (4 if c['kind'] == BLK else 16))
        n_major, p_split, n_chunks, wpc = (int(x) for x in p['tail'])
        n_tails += n_chunks > 0
        assert len(p['launch_list']) == n_major + n_chunks and n_major + (1 if n_chunks else 0) <= len(starts) - 1
        assert p_split == starts[n_major] if n_chunks else n_major == len(starts) - 1
        for q, cnt in zip(p['queues'], p['list_count']):
            assert q[0] == 0 and np.all(np.diff(q) >= 0) and q[8] == cnt
        span_list = {}
        for ln, li in enumerate(p['launch_list']):
            if ln < n_major:
                span, w_lo, w_hi = starts[ln + 1] - starts[ln], 0, n_units
                assert span_list.setdefault(span, li) == li and p['list_span'][li] == span
            else:
                k = ln - n_major
                span, w_lo = starts[-1] - p_split, min(k * wpc, n_units)
                w_hi = n_units if k + 1 == n_chunks else min((k + 1) * wpc, n_units)
            assert len(set(span_list.values())) == len(span_list)
            t = p['tasks'][p['list_first'][li]:p['list_first'][li] + p['list_count'][li]]
            cover = np.zeros((max(w_hi - w_lo, 0), n_groups, span), dtype=np.int32)
            for w, g, p0, p1 in t:
                assert w_lo <= w < w_hi and 0 <= g < n_groups and 0 <= p0 < p1 <= span and p1 - p0 <= 255
                cover[w - w_lo, g, p0:p1] += 1
            for w in range(w_lo, w_hi):
                has_columns = (w >> 1) * 64 + (w & 1) * 32 < mloc if half else True
                assert np.all(cover[w - w_lo] == (1 if has_columns else 0)), (c, ln, w)
    assert n_tails >= 5
