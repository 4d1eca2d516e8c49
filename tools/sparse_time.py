"""Time of the drop-in SAFE.compute_pvalues() call by the form the attribute matrix is handed over in: the reference's
float32 dense matrix, a uint8 dense matrix (SAFE_DTYPE_U8) and a scipy.sparse CSC matrix (safe_attr_create_csc_host), the
three alternating in one process on one device.

  configs[3]  20 000 x 10 000 binary, 1 % ones, euclidean r = 0.1, hypergeometric (bench.py's dropin_extras inputs)
  configs[1]  3971 x 4373 Costanzo surrogate, shortest-path network, randomization, 1000 permutations, seeded.  Its matrix
              has 182 all-NaN rows: the float32 and the CSC form (missing_rows) carry them; uint8 has no missing value, so
              the uint8 line runs on the matrix with those rows as zeros (another result, the same amount of work).

Per form, the median (min .. max) of --passes passes after one discarded warm-up pass:
  upload ms   backend.Attributes.from_host / from_sparse up to a device synchronise (host-side preparation included)
  create ms   the C entry point alone (safe_attr_create_host / safe_attr_create_csc_host), inside that
  call ms     the whole compute_pvalues() call, NumPy / SciPy object in, results left on the device
  link bytes  what the create call copies to the device; device bytes: the dense matrix plus the staging of the call

usage: python tools/sparse_time.py [--configs 3,1] [--passes 5] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_config(config):
    import safepy_amd
    from safepy_amd import workloads
    if config == 3:
        n, m = 20000, 10000
        b = (np.random.default_rng(5).uniform(size=(n, m)) < 0.01).astype(np.float32)
        return safepy_amd.LayoutGraph(workloads.uniform_layout(4, n)), 'euclidean', b, {}
    data = workloads.costanzo_surrogate(seed=0)
    graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
    return graph, 'shortpath_weighted_layout', data['attributes'], dict(how='randomization', num_permutations=1000)


def forms_of(b):
    """name -> (attribute_file, missing_rows, link bytes, device bytes)"""
    import scipy.sparse as sp
    n, m = b.shape
    missing = np.isnan(b).all(axis=1)
    zeroed = np.where(np.isnan(b), 0, b)
    a = sp.csc_matrix(zeroed)
    a.sort_indices()
    assert a.has_canonical_format
    if not np.array_equal(np.isnan(b), np.broadcast_to(missing[:, None], b.shape)):
        raise SystemExit('the workload has NaNs outside whole rows: not the case this tool times')
    ones = bool((a.data == 1).all())
    link = 8 * (m + 1) + 4 * a.nnz + (0 if ones else a.data.itemsize * a.nnz) + (n if missing.any() else 0)
    return {
        'f32': (b, None, b.nbytes, 4 * n * m),
        'uint8': (zeroed.astype(np.uint8), None, n * m, 5 * n * m),
        'csc': (a, missing.astype(np.uint8) if missing.any() else None, link, 4 * n * m + link + 4 * (m + 1)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='3,1')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    import safepy_amd
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    logging.disable(logging.WARNING)
    create_ms = [0.0]

    def timed(name):
        real = getattr(be.lib, name)

        def call(*a):
            t0 = time.perf_counter()
            rc = real(*a)
            create_ms[0] = 1e3 * (time.perf_counter() - t0)
            return rc
        setattr(be.lib, name, call)
    timed('safe_attr_create_host')
    timed('safe_attr_create_csc_host')

    rows = []
    for config in (int(c) for c in args.configs.split(',')):
        graph, metric, b, kw = make_config(config)
        forms = forms_of(b)
        del b
        sfs = {}
        for name, (src, missing, _, _) in forms.items():
            sf = safepy_amd.SAFE(verbose=False)
            sf.random_seed = 0
            sf.graph = graph
            sf.define_neighborhoods(node_distance_metric=metric, neighborhood_radius=0.1)
            if missing is not None:
                sf.load_attributes(attribute_file=src, missing_rows=missing)
            else:
                sf.node2attribute = src
            sfs[name] = sf
        t = {name: {'upload': [], 'create': [], 'call': []} for name in forms}
        for p in range(args.passes + 1):                       # pass 0 warms up and is discarded
            for name, (src, missing, _, _) in forms.items():
                t0 = time.perf_counter()
                attr = be.Attributes.from_sparse(ctx, src, missing) if name == 'csc' else be.Attributes.from_host(ctx, src)
                ctx.sync()
                up = 1e3 * (time.perf_counter() - t0)
                cr = create_ms[0]
                attr.close()
                t0 = time.perf_counter()
                sfs[name].compute_pvalues(**kw)
                call = 1e3 * (time.perf_counter() - t0)
                if p:
                    t[name]['upload'].append(up)
                    t[name]['create'].append(cr)
                    t[name]['call'].append(call)
        n, m = forms['f32'][0].shape
        for name, (src, _, link, dev) in forms.items():
            def stat(key):
                v = t[name][key]
                return '%7.2f (%6.2f .. %6.2f)' % (float(np.median(v)), min(v), max(v))
            extra = ''
            if name == 'csc':
                extra = '  nnz %d' % src.nnz
            print('configs[%d] %5d x %5d  %-5s  upload ms %s  create ms %s  call ms %s  link MB %7.1f  device MB %7.1f%s'
                  % (config, n, m, name, stat('upload'), stat('create'), stat('call'), link / 1e6, dev / 1e6, extra), flush=True)
            rows.append({'config': config, 'shape': [n, m], 'form': name, 'passes': args.passes, 'link_bytes': int(link), 'device_bytes': int(dev),
                         **{key + '_ms': [float(x) for x in t[name][key]] for key in ('upload', 'create', 'call')}})
        del sfs, forms
        ctx.trim()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
