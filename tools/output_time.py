"""Time of the node table of print_output_files without domains (safe_format_tsv: DataFrame(nes).to_csv(sep='\\t'),
safepy/safe.py:1297-1306) at BASELINE configs[1] (3971 x 4373) and configs[3] (20 000 x 10 000), one line per shape.
The matrix is NES-like -- -log10(k / 1000) for random k, 5 % NaN rows, as compute_pvalues leaves it on the device.

  kernel ms   HIP events around the format kernels (row lengths, scan, text), summed over the chunks
  copy ms     HIP events around the device-to-host copies into the pinned buffers
  write ms    host clock around the write() calls (overlaps the next chunk's kernels and copy)
  call ms     host clock around the whole call (uploads of the row prefixes, allocations, the pipeline)
  pandas      DataFrame.to_csv(sep='\\t') of the first --pandas-rows rows on this host's CPU, scaled to all rows

usage: python tools/output_time.py [--shapes 3971x4373,20000x10000] [--out DIR] [--repeats 2] [--pandas-rows 200]
--out: directory for the files (default: a temporary directory, removed afterwards); 'null' writes to /dev/null."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='3971x4373,20000x10000')
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--pandas-rows', type=int, default=200)
    ap.add_argument('--budget-mb', type=int, default=0, help='chunk budget (default: the library default)')
    args = ap.parse_args()
    import pandas as pd
    from safepy_amd import backend as be
    from safepy_amd.safe import _row_prefixes
    ctx = be.Context.default(0)
    tmpdir = None
    out = args.out
    if not out:
        tmpdir = tempfile.TemporaryDirectory()
        out = tmpdir.name
    for shape in args.shapes.split(','):
        n, m = (int(v) for v in shape.split('x'))
        rng = np.random.default_rng(n)
        nes = -np.log10(rng.integers(1, 1001, size=(n, m)) / 1000.0)
        nes[rng.uniform(size=n) < 0.05] = np.nan
        keys = ['ORF%d' % i for i in range(n)]
        t0 = time.perf_counter()
        prefixes, offsets = _row_prefixes(keys, keys, n)
        prefix_ms = 1e3 * (time.perf_counter() - t0)
        buf = ctx.alloc_f64(n, m)
        buf.upload(nes)
        path = os.devnull if out == 'null' else os.path.join(out, 'node_properties_annotation.txt')
        runs = []
        for _ in range(args.repeats + 1):                    # the first call warms up
            with open(path, 'wb') as f:
                runs.append(ctx.format_tsv(buf.ptr, n, m, prefixes, offsets, f.fileno(),
                                           budget_bytes=(args.budget_mb << 20) or None))
        buf.free()
        if out != 'null':
            os.remove(path)
        best = min(runs[1:], key=lambda r: r['call_ms'])
        k = min(args.pandas_rows, n)
        frame = pd.DataFrame(nes[:k])
        frame.insert(0, 'key', keys[:k])
        frame.insert(1, 'label', keys[:k])
        t0 = time.perf_counter()
        frame.to_csv(os.devnull, sep='\t')
        pandas_s = (time.perf_counter() - t0) * n / k
        print('%5d x %5d  %7.1f MB  kernel ms %7.2f  copy ms %7.2f  write ms %8.2f  call ms %8.2f  (prefixes %.1f ms)  '
              'GB/s %.2f  pandas s %.1f (%d rows, scaled)'
              % (n, m, best['bytes'] / 1e6, best['kernel_ms'], best['copy_ms'], best['write_ms'], best['call_ms'], prefix_ms,
                 best['bytes'] / best['call_ms'] / 1e6, pandas_s, k), flush=True)
    if tmpdir is not None:
        tmpdir.cleanup()


if __name__ == '__main__':
    main()
