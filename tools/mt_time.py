"""Time of every multiple_testing_method procedure (safe_mt_adjust_matrix) on one p-value matrix, per scope and form, with
Benjamini-Hochberg through the old entry point (safe_fdr_adjust_matrix) timed beside each one in the same process, on
device-resident matrices.

  configs[1]  3971 x 4373, p = counts / 1000 (what the randomization test leaves): count and sort forms
  configs[3]  20 000 x 10 000, continuous p (what the hypergeometric test leaves): sort forms only

Per form and procedure, the median (min .. max) of --passes passes after one discarded warm-up pass, between the context's event
pair around the one call (the matrix is restored from a device copy before the clock starts), and its ratio to the old entry
point's median.  The sorted procedures run the kernels of Benjamini-Hochberg with another per-entry value, so they move the bytes
tools/fdr_scope_time.py lists for the form; Bonferroni takes no form: one read and one write of the matrix, 16 bytes per cell.

There is no pass / fail time here.

usage: python tools/mt_time.py [--configs 1,3] [--passes 5] [--json FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fdr_scope_time import PEAK_BYTES_PER_S, forms, make_matrix, spread      # noqa: E402

METHODS = ('fdr_bh', 'fdr_by', 'holm', 'hochberg', 'bonferroni')
BONFERRONI_BYTES = 16


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
        for scope in ('attributes', 'neighborhoods', 'all'):         # (the harmonic sums are host work: outside the clock)
            be._mt_method('fdr_by', n, m, scope)
        cases = [(label, scope, den, kernels, method) for label, scope, den, kernels in forms(n, m, P) for method in ('old',) + METHODS]
        times = {(label, method): [] for label, _, _, _, method in cases}
        # one case at a time, its passes back to back: the per-call blocks of a form (gigabytes at configs[3]) then come from the
        # context's pool from the second pass on, as they do in an application that repeats one call
        for label, scope, den, _, method in cases:
            for k in range(args.passes + 1):
                work.copy_(source)
                torch.cuda.synchronize()
                ctx.timer_start()
                if method == 'old':
                    be.fdr_adjust_matrix(ctx, n, m, scope, work.data_ptr(), count_denominator=den)
                else:
                    be.mt_adjust_matrix(ctx, n, m, scope, method, work.data_ptr(), count_denominator=den)
                ms = ctx.timer_stop_ms()
                if k:
                    times[label, method].append(ms)
        print('configs[%d]: %d x %d, %s' % (config, n, m, 'p = counts / %d' % P if P else 'continuous p'))
        for label, scope, den, kernels in forms(n, m, P):
            old = float(np.median(times[label, 'old']))
            per_cell = sum(b for _, b in kernels)
            print('  %s: %d B per cell by construction; safe_fdr_adjust_matrix ms %s' % (label.replace(' (today)', ''), per_cell, spread(times[label, 'old'])))
            for method in METHODS:
                med = float(np.median(times[label, method]))
                note = ''
                if method == 'bonferroni':
                    floor_ms = 1e3 * BONFERRONI_BYTES * n * m / PEAK_BYTES_PER_S
                    note = '   (element-wise: %d B per cell = %.3f ms at 8 TB/s, %.3f of peak)' % (BONFERRONI_BYTES, floor_ms, floor_ms / med)
                print('    %-11s ms %s   x %.3f of the old entry point%s' % (method, spread(times[label, method]), med / old, note))
                report['configs[%d] %s %s' % (config, label, method)] = {'ms': times[label, method], 'old_ms': times[label, 'old']}
        del source, work
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
