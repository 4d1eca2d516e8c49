"""Time of the gene-to-term closure (safe_go_create / safe_go_read, csrc/go.hip) at Gene-Ontology size, against the host
restatement of tests/go_ref.py on the same machine.

  input     a synthetic ontology -- 30 000 terms on 15 levels, every term but the root with 1-3 (about 2) parents on
            shallower levels -- and 300 000 annotation rows over 20 000 and over 6 000 loci (seeded; nothing is read from disk)
  device    backend.GoClosure(...) + read(): median (min .. max) of --passes passes after one discarded warm-up pass
              call ms    the whole route: index arrays in, indptr / indices / kept terms on the host out
              per pass   ms between the events that bracket it, and the bytes the pass cannot avoid moving (its floor, below)
                         over that time, as GB/s and as a share of 8 TB/s
  host      go_ref.closure_ref (networkx ancestors per annotated term, a dense 0/1 matrix, NumPy), --host-passes times
            (default 1: it takes seconds); the two results are compared, and must be equal

Floors, with W = ceil(loci / 32) rounded up to a multiple of 4, words of 4 bytes per term row, E = is_a edges, T = terms, T' = terms with a child:
  scatter   4 T W (the zero fill) + 8 per annotation row (its two indices)
  closure   4 W (E + 2 T')      every child row read once per parent edge, every parent row read and written once
  count     4 T W
  root      4 T W               (the OR over all rows; the root's row and the per-word work are W-sized)
  scan      not a bandwidth pass: two single-workgroup scans over T counts -- ms only
  emit      4 T W + 4 nnz

usage: python tools/go_time.py [--loci 20000,6000] [--passes 5] [--host-passes 1] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_BYTES_PER_S = 8e12
N_TERMS, N_LEVELS, N_ANNOTATIONS = 30000, 15, 300000


def make_ontology(seed):
    """(parent, child) pairs: term 0 the root, levels 1 .. 14 about equally filled, 1-3 parents per term (mean 2), one of them on
    the level right above."""
    rng = np.random.default_rng(seed)
    depth = np.zeros(N_TERMS, dtype=np.int64)
    depth[1:] = 1 + np.arange(N_TERMS - 1) % (N_LEVELS - 1)
    starts = np.searchsorted(np.sort(depth), np.arange(N_LEVELS + 1))
    order = np.argsort(depth, kind='stable')                   # terms by depth; order[starts[d] : starts[d + 1]] is level d
    parents, children = [], []
    for extra in range(3):
        for d in range(1, N_LEVELS):
            kids = order[starts[d]:starts[d + 1]]
            if extra == 0:
                pool = order[starts[d - 1]:starts[d]]
                take = np.ones(kids.shape[0], dtype=bool)
            else:
                pool = order[:starts[d]]
                take = rng.uniform(size=kids.shape[0]) < 0.5
            parents.append(pool[rng.integers(0, pool.shape[0], kids.shape[0])][take])
            children.append(kids[take])
    e = np.unique(np.stack([np.concatenate(parents), np.concatenate(children)], axis=1), axis=0)
    relabel = np.concatenate([[0], 1 + rng.permutation(N_TERMS - 1)])
    return relabel[e]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loci', default='20000,6000')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--host-passes', type=int, default=1)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    import go_ref
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    edges = make_ontology(0)
    ptr, idx = go_ref.children_csr(N_TERMS, edges)
    with_child = int((np.diff(ptr) > 0).sum())
    rows = []
    for n_loci in [int(x) for x in args.loci.split(',')]:
        rng = np.random.default_rng(n_loci)
        ann_row = rng.integers(0, n_loci - n_loci // 50, N_ANNOTATIONS).astype(np.int32)        # the last 2 % of the loci have no term
        ann_term = rng.integers(0, N_TERMS, N_ANNOTATIONS).astype(np.int32)
        W = (n_loci + 127) // 128 * 4                         # words per term row: ceil(loci / 32), whole 16-byte quads
        call, per_pass, got, levels = [], {p: [] for p in be.GoClosure.PASSES}, None, 0
        for p in range(args.passes + 1):                       # pass 0 warms up and is discarded
            ctx.sync()
            t0 = time.perf_counter()
            g = be.GoClosure(ctx, n_loci, N_TERMS, ptr, idx, ann_row, ann_term, 0)
            out = g.read()
            ms = 1e3 * (time.perf_counter() - t0)
            passes, levels = g.pass_ms()
            g.close()
            if p:
                call.append(ms)
                for k, v in passes.items():
                    per_pass[k].append(v)
            else:
                got = out
        host = []
        for _ in range(args.host_passes):
            t0 = time.perf_counter()
            want = go_ref.closure_ref(n_loci, N_TERMS, edges, ann_row, ann_term, 0)
            host.append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(got[0], want['indptr']) and np.array_equal(got[1], want['indices'])
            assert np.array_equal(got[2], want['kept']) and got[3] == want['assigned']
            del want
        nnz = int(got[1].shape[0])
        floors = {'scatter': 4 * N_TERMS * W + 8 * N_ANNOTATIONS, 'closure': 4 * W * (edges.shape[0] + 2 * with_child),
                  'count': 4 * N_TERMS * W, 'root': 4 * N_TERMS * W, 'scan': None, 'emit': 4 * N_TERMS * W + 4 * nnz}

        def stat(v):
            return '%9.3f (%8.3f .. %8.3f)' % (float(np.median(v)), min(v), max(v))
        print('%d terms, %d edges, %d levels, %d loci, %d annotation rows -> %d kept terms, nnz %d, %d loci to the root'
              % (N_TERMS, edges.shape[0], levels, n_loci, N_ANNOTATIONS, got[2].shape[0], nnz, got[3]), flush=True)
        print('  call ms      %s' % stat(call))
        row = {'loci': n_loci, 'terms': N_TERMS, 'edges': int(edges.shape[0]), 'levels': int(levels), 'nnz': nnz, 'kept': int(got[2].shape[0]),
               'root_assigned': int(got[3]), 'passes': args.passes, 'call_ms': call, 'host_ms': host, 'pass_ms': per_pass, 'floor_bytes': floors}
        for k in be.GoClosure.PASSES:
            line = '  %-8s ms  %s' % (k, stat(per_pass[k]))
            if floors[k]:
                rate = floors[k] / (float(np.median(per_pass[k])) * 1e-3)
                line += '  floor %8.1f MB  %7.1f GB/s = %4.1f %% of 8 TB/s' % (floors[k] / 1e6, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S)
            print(line)
        print('  kernels ms   %9.3f (sum of the medians)' % sum(float(np.median(per_pass[k])) for k in be.GoClosure.PASSES))
        if host:
            print('  host ms      %s  (go_ref.closure_ref, %d pass%s; results equal)' % (stat(host), len(host), '' if len(host) == 1 else 'es'))
            print('  call / host  %.4f' % (float(np.median(call)) / float(np.median(host))), flush=True)
        rows.append(row)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
