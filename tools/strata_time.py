"""Time of the restricted permutations (permutation_strata) on one MI355X, one process, at configs[1]'s shape -- 3971 nodes,
4373 0/1 attributes, 1000 permutations -- on the seeded surrogate of bench.py (safepy_amd.workloads.costanzo_surrogate).

  generator   backend.Permutations.stratified alone for S = 1, 10, 30, 100 and k / 2 strata (pairs) of equal size, node order
              interleaved, next to backend.Permutations(seed=None) (safe_perms_create_device) on the same rows: host clock
              from the call to a device-wide synchronise, so the partition's host work (sort, two uploads) is inside.  With
              --wave-min a,b,c the same figures with SAFE_HIP_STRATA_WAVE_MIN set to each value: the size at which a stratum
              moves from one lane to the whole wave (a performance constant; the tables do not change).
  call        SAFE.compute_pvalues(how='randomization', permutation_strata='neighborhood_size') next to the unseeded call
              without strata: host clock around the call (results stay on the device; the call ends in a synchronise).

Medians (min .. max) of --passes passes after one discarded warm-up pass; the variants alternate inside a pass.  There is no
pass / fail time here.

usage: python tools/strata_time.py [--passes 5] [--wave-min 16,64,128,512] [--json FILE]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NPERM = 1000


def spread(values):
    return '%.3f (%.3f .. %.3f)' % (float(np.median(values)), min(values), max(values))


def partitions(movable):
    """{label: int32 [n] strata}: S strata of equal size over the movable rows, interleaved in node order."""
    n, k = len(movable), int(movable.sum())
    out = {}
    for label, count in (('S = 1', 1), ('S = 10', 10), ('S = 30', 30), ('S = 100', 100), ('S = k / 2 (pairs)', (k + 1) // 2)):
        strata = np.zeros(n, dtype=np.int32)
        strata[movable != 0] = np.arange(k) % count
        out[label] = strata
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--wave-min', default='')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    import torch
    import safepy_amd
    from safepy_amd import backend as be, workloads
    logging.disable(logging.WARNING)
    ctx = be.Context.default(0)
    data = workloads.costanzo_surrogate(seed=0)
    b = data['attributes']
    n = b.shape[0]
    movable = (~np.isnan(b)).any(axis=1).astype(np.uint8) if np.issubdtype(b.dtype, np.floating) else np.ones(n, dtype=np.uint8)
    report = {'shape': [int(n), int(b.shape[1])], 'movable_rows': int(movable.sum()), 'permutations': NPERM}

    def timed_create(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        perms = make()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        perms.close()
        return ms

    parts = partitions(movable)
    settings = [None] + [v for v in args.wave_min.split(',') if v]
    variants = [('safe_perms_create_device', None, None)]
    variants += [('%s%s' % (label, '' if w is None else ', wave_min = %s' % w), label, w) for w in settings for label in parts]
    times = {name: [] for name, _, _ in variants}
    for k in range(args.passes + 1):
        for name, label, wave_min in variants:
            if wave_min is None:
                os.environ.pop('SAFE_HIP_STRATA_WAVE_MIN', None)
            else:
                os.environ['SAFE_HIP_STRATA_WAVE_MIN'] = wave_min
            if label is None:
                ms = timed_create(lambda: be.Permutations(ctx, n, movable, NPERM, None, device_key=k))
            else:
                ms = timed_create(lambda: be.Permutations.stratified(ctx, n, movable, parts[label], NPERM, k))
            if k:
                times[name].append(ms)
    os.environ.pop('SAFE_HIP_STRATA_WAVE_MIN', None)
    print('generator alone, %d movable rows of %d, %d permutations: ms, call to device-wide synchronise' % (movable.sum(), n, NPERM))
    for name, _, _ in variants:
        print('  %-44s %s' % (name, spread(times[name])))
    report['generator_ms'] = times

    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.1)
    sf.node2attribute = b
    calls = {'unseeded, no strata': dict(permutation_strata=None), "permutation_strata = 'neighborhood_size'": dict(permutation_strata='neighborhood_size')}
    call_ms = {name: [] for name in calls}
    for k in range(args.passes + 1):
        for name, kw in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sf.compute_pvalues(how='randomization', num_permutations=NPERM, **kw)
            torch.cuda.synchronize()
            if k:
                call_ms[name].append(1e3 * (time.perf_counter() - t0))
    print('whole compute_pvalues call (%s): ms' % ctx.last_kernel()[0])
    for name in calls:
        print('  %-44s %s' % (name, spread(call_ms[name])))
    print('  strata sizes: %s' % sf.permutation_strata_sizes.tolist())
    report['compute_pvalues_ms'] = call_ms
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
