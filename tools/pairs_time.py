"""Time of getting the enriched (node, attribute) pairs out of a finished compute_pvalues(), two routes alternating in one
process on one device, at configs[1] and configs[3] alternating too:

  dense   what a caller did before SAFE.enriched_pairs: read nes_binary and nes through the lazy attributes (both whole
          matrices cross the link as f64), then np.nonzero, nes[rows, cols] and scipy.sparse.csr_array on the host
  csr     SAFE.enriched_pairs(values='nes', format='csr'): compacted on the device, the matrices stay there
  csc     SAFE.enriched_pairs(values='nes', format='csc')

  configs[3]  20 000 x 10 000 binary, 1 % ones, euclidean r = 0.1, hypergeometric (bench.py's dropin_extras inputs)
  configs[1]  3971 x 4373 Costanzo surrogate, shortest-path network, randomization, 1000 permutations, seeded

Every pass runs compute_pvalues() again first (not timed: the dense route leaves the matrices on the host).  Per route, the
median (min .. max) of --passes passes after one discarded warm-up pass:
  call ms     the whole route, results of compute_pvalues on the device in, scipy.sparse array out
  count ms    safe_pairs_create's kernels (count, scans); emit ms: safe_pairs_read's kernel; behind each the share of
              8 TB/s that the 8 n m bytes of the selector over that time come to
  link bytes  dense: 16 n m; csr / csc: 12 nnz + 4 (rows or columns + 1) -- arithmetic, not a measurement

usage: python tools/pairs_time.py [--configs 3,1] [--passes 5] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12


def make_instance(config):
    import safepy_amd
    from safepy_amd import workloads
    sf = safepy_amd.SAFE(verbose=False)
    sf.random_seed = 0
    if config == 3:
        n, m = 20000, 10000
        sf.graph = safepy_amd.LayoutGraph(workloads.uniform_layout(4, n))
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1)
        sf.node2attribute = (np.random.default_rng(5).uniform(size=(n, m)) < 0.01).astype(np.float32)
        return sf, {}
    data = workloads.costanzo_surrogate(seed=0)
    sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.1)
    sf.node2attribute = data['attributes']
    return sf, dict(how='randomization', num_permutations=1000)


def dense_route(sf):
    import scipy.sparse as sp
    nes_binary, nes = sf.nes_binary, sf.nes
    rows, cols = np.nonzero(nes_binary)
    return sp.csr_array((nes[rows, cols], (rows, cols)), shape=nes.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='3,1')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)

    kernel_ms = [(0.0, 0.0)]
    real = be.Context.enriched_pairs

    def recording(self, *a):
        out = real(self, *a)
        kernel_ms[0] = out[3]
        return out
    be.Context.enriched_pairs = recording

    configs = [int(c) for c in args.configs.split(',')]
    made = {c: make_instance(c) for c in configs}
    routes = ('dense', 'csr', 'csc')
    t = {c: {r: {'call': [], 'count': [], 'emit': []} for r in routes} for c in configs}
    shape, nnz = {}, {}
    for p in range(args.passes + 1):                           # pass 0 warms up and is discarded
        for c in configs:
            sf, kw = made[c]
            sf.compute_pvalues(**kw)
            ctx.sync()
            results = {}
            for route in ('csr', 'csc', 'dense'):              # (dense last: it takes the matrices off the device)
                t0 = time.perf_counter()
                results[route] = dense_route(sf) if route == 'dense' else sf.enriched_pairs(values='nes', format=route)
                call = 1e3 * (time.perf_counter() - t0)
                if p:
                    t[c][route]['call'].append(call)
                    if route != 'dense':
                        t[c][route]['count'].append(kernel_ms[0][0])
                        t[c][route]['emit'].append(kernel_ms[0][1])
            if p == 0:                                          # the three routes give one matrix
                shape[c], nnz[c] = results['csr'].shape, int(results['csr'].nnz)
                want = results['dense']
                want.sort_indices()
                for route in ('csr', 'csc'):
                    got = results[route].tocsr()
                    got.sort_indices()
                    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
                    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))
            del results

    rows = []
    for c in configs:
        n, m = shape[c]
        for route in routes:
            def stat(key):
                v = t[c][route][key]
                return '%8.3f (%7.3f .. %7.3f)' % (float(np.median(v)), min(v), max(v))
            link = 16 * n * m if route == 'dense' else 12 * nnz[c] + 4 * ((m if route == 'csc' else n) + 1)
            line = 'configs[%d] %5d x %5d  nnz %8d (%.2f %%)  %-5s  call ms %s  link MB %8.1f' % (
                c, n, m, nnz[c], 100.0 * nnz[c] / (n * m), route, stat('call'), link / 1e6)
            row = {'config': c, 'shape': [int(n), int(m)], 'nnz': nnz[c], 'route': route, 'passes': args.passes, 'link_bytes': int(link),
                   'call_ms': [float(x) for x in t[c][route]['call']]}
            if route != 'dense':
                for key in ('count', 'emit'):
                    med = float(np.median(t[c][route][key]))
                    share = 8.0 * n * m / (med * 1e-3) / HBM_BYTES_PER_S
                    line += '  %s ms %s = %4.1f %% of 8 TB/s' % (key, stat(key), 100.0 * share)
                    row[key + '_ms'] = [float(x) for x in t[c][route][key]]
                    row[key + '_share_of_8TBps'] = share
            print(line, flush=True)
            rows.append(row)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
