"""safepy_amd/csrc/fdr_plan.h -- the form choice, the span helper and the per-entry arithmetic of the Benjamini-Hochberg code --
built for the host with the system C++ compiler and run as a program, as tests/test_bits_plan_cpu.py does with bits_plan.h:
with the address and undefined-behaviour sanitizers where the compiler links them.  Shared by tests/test_fdr_cases_cpu.py and
tests/test_fdr_scope_cpu.py.  Nothing is loaded into Python; no GPU."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')

ROWS, COLS, ALL = 0, 1, 2                                         # FdrScope
# FdrKind
UNSUPPORTED, ROW_HIST, ROW_BLOCK_SORT, ROW_LIBRARY_SORT, ROW_TOO_LONG, COL_COUNTS, COL_SORT, ALL_COUNTS, ALL_SORT = range(9)
BIN_NAN, BIN_NOT_RATIO = -1, -2
CONSTANTS = ('THREADS', 'BLOCK_SORT_MAX', 'ROW_HIST_BIN_BYTES', 'ROW_HIST_LDS_BYTES', 'ROW_HIST_MAX_P', 'COL_BIN_BYTES', 'COL_LDS_BYTES',
             'COL_TILE_MAX', 'COL_TILE_MIN', 'COL_HIST_MAX_P', 'ALL_HIST_MAX_P', 'TR_TILE', 'ALL_IPT', 'ALL_BLOCK', 'SEG_BATCH_KEYS',
             'SORT_MAX_ITEMS')

# One line of integers per command.  The switch travels as the text of SAFE_HIP_FDR_SORT ("-": unset) through fdr_switch.
#   const                     -> the constants in the order of CONSTANTS, then the IPT ladder
#   exists scope P sw         -> fdr_count_form_exists
#   form scope n m P sw       -> kind tile lds_bytes row_kind ipt batch_rows
#   span count parts t        -> b0 b1
#   key bits                  -> fdr_key of the double with these bits (hex)
#   ratio bits P              -> fdr_ratio_bin
DRIVER = r'''
#include <cstdio>
#include <cstring>
#include "fdr_plan.h"
static FdrSwitch sw_of(const char *s) { return fdr_switch(std::strcmp(s, "-") ? s : nullptr); }
static double from_bits(unsigned long long b) {
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char what[16], sw[32];
    long long a, b, c, d;
    unsigned long long bits;
    while (std::fscanf(f, "%15s", what) == 1) {
        if (!std::strcmp(what, "const")) {
            std::printf("%d %lld %d %d %lld %d %d %d %d %lld %lld %d %d %d %lld %lld", FDR_THREADS, (long long)FDR_BLOCK_SORT_MAX,
                        FDR_ROW_HIST_BIN_BYTES, FDR_ROW_HIST_LDS_BYTES, (long long)FDR_ROW_HIST_MAX_P, FDR_COL_BIN_BYTES, FDR_COL_LDS_BYTES,
                        FDR_COL_TILE_MAX, FDR_COL_TILE_MIN, (long long)FDR_COL_HIST_MAX_P, (long long)FDR_ALL_HIST_MAX_P, FDR_TR_TILE,
                        FDR_ALL_IPT, FDR_ALL_BLOCK, (long long)FDR_SEG_BATCH_KEYS, (long long)FDR_SORT_MAX_ITEMS);
            for (int k = 0; k < FDR_IPT_RUNGS; ++k) std::printf(" %d", FDR_IPT_LADDER[k]);
            std::printf("\n");
        } else if (!std::strcmp(what, "exists")) {
            if (std::fscanf(f, "%lld %lld %31s", &a, &b, sw) != 3) return 3;
            std::printf("%d\n", fdr_count_form_exists(static_cast<int>(a), b, sw_of(sw)) ? 1 : 0);
        } else if (!std::strcmp(what, "form")) {
            if (std::fscanf(f, "%lld %lld %lld %lld %31s", &a, &b, &c, &d, sw) != 5) return 3;
            const FdrForm fm = fdr_form(static_cast<int>(a), b, c, d, sw_of(sw));
            std::printf("%d %d %lld %d %d %lld\n", fm.kind, fm.tile, (long long)fm.lds_bytes, fm.row_kind, fm.ipt, (long long)fm.batch_rows);
        } else if (!std::strcmp(what, "span")) {
            if (std::fscanf(f, "%lld %lld %lld", &a, &b, &c) != 3) return 3;
            long long b0, b1;
            fdr_span<long long>(a, b, c, b0, b1);
            std::printf("%lld %lld\n", b0, b1);
        } else if (!std::strcmp(what, "key")) {
            if (std::fscanf(f, "%llx", &bits) != 1) return 3;
            std::printf("%llu\n", fdr_key(from_bits(bits)));
        } else if (!std::strcmp(what, "ratio")) {
            if (std::fscanf(f, "%llx %lld", &bits, &a) != 2) return 3;
            std::printf("%d\n", fdr_ratio_bin(from_bits(bits), static_cast<double>(a)));
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
'''


def build(d):
    """Builds the driver in the directory d (a pathlib path) and returns run(lines) -> uint64 / int64 array [len(lines), ...]:
    one row of integers per command line."""
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed to build the planning header for the CPU'
    (d / 'drv.cpp').write_text(DRIVER)
    base = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-I' + CSRC, str(d / 'drv.cpp'), '-o', str(d / 'drv')]
    # a stand-alone program: the sanitizers are linked into it where the compiler has them and their runtime starts (an empty
    # input runs none of the code under test), else it is built plain
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    (d / 'in.txt').write_text('')
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0 or \
            subprocess.run([str(d / 'drv'), str(d / 'in.txt')], capture_output=True, env=env).returncode != 0:
        subprocess.run(base, check=True)

    def run(lines, dtype=np.int64):
        lines = list(lines)
        (d / 'in.txt').write_text('\n'.join(lines) + '\n')
        out = subprocess.run([str(d / 'drv'), str(d / 'in.txt')], check=True, capture_output=True, text=True, env=env).stdout
        rows = [[int(x) for x in ln.split()] for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return np.array(rows, dtype=dtype)
    return run


def constants(run):
    """({name: value}, ladder)"""
    row = [int(x) for x in run(['const'])[0]]
    return dict(zip(CONSTANTS, row)), tuple(row[len(CONSTANTS):])


def forms(run, cases):
    """cases: (scope, n, m, P, switch text or None) -> list of dicts(kind, tile, lds, row_kind, ipt, batch_rows)"""
    out = run('form %d %d %d %d %s' % (s, n, m, P, sw or '-') for s, n, m, P, sw in cases)
    return [dict(zip(('kind', 'tile', 'lds', 'row_kind', 'ipt', 'batch_rows'), (int(x) for x in r))) for r in out]


def exists(run, cases):
    """cases: (scope, P, switch text or None) -> list of bool"""
    return [bool(r[0]) for r in run('exists %d %d %s' % (s, P, sw or '-') for s, P, sw in cases)]


def keys(run, values):
    """fdr_key of every double of `values`, as uint64"""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).ravel()
    return run(('key %x' % int(b) for b in bits), dtype=np.uint64)[:, 0]


def ratio_bins(run, values, P):
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).ravel()
    return run('ratio %x %d' % (int(b), P) for b in bits)[:, 0]
