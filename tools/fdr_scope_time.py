"""Time of the Benjamini-Hochberg adjustment of one p-value matrix along the three multiple_testing_scope families
(safe_fdr_adjust_matrix), in the count and the sort form where both apply, next to today's row scope in the same process, on
device-resident matrices.

  configs[1]  3971 x 4373, p = counts / 1000 (what the randomization test leaves): count and sort forms
  configs[3]  20 000 x 10 000, continuous p (what the hypergeometric test leaves): sort forms only

Per form, the median (min .. max) of --passes passes after one discarded warm-up pass, between the context's event pair
(safe_timer_start / safe_timer_stop_ms around the one call; the matrix is restored from a device copy before the clock starts).
The floor is the bytes the form's kernels move by construction, per cell of the matrix, summed over the kernels listed beside
it, and the time that traffic would take at 8 TB/s; `of peak` is that time over the measured one.  The event pair times the whole
call, host waits between its kernels included, not single kernels.

There is no pass / fail time here.

usage: python tools/fdr_scope_time.py [--configs 1,3] [--passes 5] [--json FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12
RADIX_PASSES = 8                            # the library's radix sort of 64-bit keys, 8 bits per pass

# bytes per matrix cell each kernel moves by construction
CHECK = ('k_fdr_check_ratio', 8)                                  # reads the matrix
COUNTS = ('histogram + look-up', 8 + 8 + 8)                       # reads it for the histogram, again for the look-up, writes it
BLOCK_SORT = ('k_fdr_row_sort', 8 + 8)                            # reads and writes it; the sort stays in registers and LDS
TRANSPOSE = ('k_fdr_transpose x 2', 2 * (8 + 8))
ALL_HIST = ('k_fdr_all_hist + k_fdr_all_map', 8 + 8 + 8)
PAIR_SORT = ('keys + radix sort of (u64, u32) pairs', (8 + 12) + 8 + RADIX_PASSES * (12 + 12))
SUFFIX_MIN = ('k_fdr_all_blockmin + k_fdr_all_apply', 8 + (12 + 8))
SEGMENTED = ('segmented radix sort of (f64, i32) pairs + k_fdr_row', 4 + 8 + RADIX_PASSES * (12 + 12) + (12 + 8))


def forms(n, m, P):
    """[(label, scope, count_denominator, kernels)]; rows longer than 8192 go through the library's segmented sort."""
    row_sort = BLOCK_SORT if m <= 8192 else SEGMENTED
    col_sort = BLOCK_SORT if n <= 8192 else SEGMENTED
    out = []
    if P:
        out.append(('rows, count form (today)', 'attributes', P, [CHECK, COUNTS]))
    out.append(('rows, sort form (today)', 'attributes', 0, [row_sort]))
    if P:
        out.append(('columns, count form', 'neighborhoods', P, [CHECK, COUNTS]))
    out.append(('columns, sort form', 'neighborhoods', 0, [TRANSPOSE, col_sort]))
    if P:
        out.append(('matrix, count form', 'all', P, [CHECK, ALL_HIST]))
    out.append(('matrix, sort form', 'all', 0, [PAIR_SORT, SUFFIX_MIN]))
    return out


def make_matrix(config):
    """(host p [n, m], P): seeded, with the ties and zeros of the real thing."""
    rng = np.random.default_rng(config)
    if config == 1:
        n, m, P = 3971, 4373, 1000
        return np.floor(P * rng.random((n, m)) ** 3) / float(P), P
    n, m = 20000, 10000
    p = rng.random((n, m))
    p *= p
    p *= p                                                       # u^4: small p-values in most families
    return p, 0


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='1,3')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    import torch
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    report = {}
    for config in [int(c) for c in args.configs.split(',')]:
        host, P = make_matrix(config)
        n, m = host.shape
        source = torch.from_numpy(host).to('cuda')
        work = torch.empty_like(source)
        del host
        times = {label: [] for label, *_ in forms(n, m, P)}
        for k in range(args.passes + 1):
            for label, scope, denominator, _ in forms(n, m, P):
                work.copy_(source)
                torch.cuda.synchronize()
                ctx.timer_start()
                be.fdr_adjust_matrix(ctx, n, m, scope, work.data_ptr(), count_denominator=denominator)
                ms = ctx.timer_stop_ms()
                if k:
                    times[label].append(ms)
        print('configs[%d]: %d x %d, %s' % (config, n, m, 'p = counts / %d' % P if P else 'continuous p'))
        for label, scope, denominator, kernels in forms(n, m, P):
            per_cell = sum(b for _, b in kernels)
            floor_bytes = float(per_cell) * n * m
            floor_ms = 1e3 * floor_bytes / PEAK_BYTES_PER_S
            med = float(np.median(times[label]))
            print('  %-26s ms %s   floor %.2f GB (%d B per cell: %s) = %.3f ms at 8 TB/s, %.3f of peak'
                  % (label, spread(times[label]), floor_bytes / 1e9, per_cell, ' + '.join('%s %d' % kb for kb in kernels), floor_ms,
                     floor_ms / med))
            report['configs[%d] %s' % (config, label)] = {'ms': times[label], 'floor_bytes': floor_bytes, 'floor_ms': floor_ms,
                                                          'kernels': kernels}
        del source, work
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
