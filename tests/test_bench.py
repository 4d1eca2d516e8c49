"""bench.py itself: the options of a plain run, --dump-outputs (CPU: what a dump holds; GPU: a plain run's dump equals what the
drop-in API returns for the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    return bench.parse()


def test_a_plain_run_leaves_out_the_full_legs(monkeypatch):
    args = _parse(monkeypatch, ['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    assert _parse(monkeypatch, ['--full']).full
    with pytest.raises(SystemExit):
        _parse(monkeypatch, ['--steps', '0'])


def test_dump_outputs_writes_small_arrays_whole_and_a_fixed_sample_of_large_ones(tmp_path, monkeypatch):
    import torch
    import bench
    # a step leaves at most seven arrays (five output blocks, the enriched counts, N > 1 the gathered NES): under 64 MB in all
    assert 7 * bench.DUMP_ELEMENTS * 8 <= 64 << 20
    monkeypatch.setattr(bench, 'DUMP_ELEMENTS', 1000)
    big = torch.from_numpy(np.random.default_rng(3).standard_normal((50, 100)))
    small = torch.arange(10, dtype=torch.float64)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small}, np, torch)
    assert sorted(os.listdir(tmp_path / 'a')) == ['big.npy', 'small.npy']
    a_big, b_big = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'b' / 'big.npy')
    want = np.sort(np.random.default_rng(0).choice(5000, 1000, replace=False))
    assert a_big.dtype == np.float64 and a_big.shape == (1000,)
    np.testing.assert_array_equal(a_big, big.numpy().reshape(-1)[want])
    np.testing.assert_array_equal(a_big, b_big)
    a_small = np.load(tmp_path / 'a' / 'small.npy')
    assert a_small.dtype == np.float64 and a_small.shape == (10,)
    np.testing.assert_array_equal(a_small, np.arange(10.0))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_the_call_returns(tmp_path):
    """A plain run times exactly --steps steps, runs none of the --full legs, and its dump equals what SAFE.compute_pvalues
    returns for the same seeded workload (the surrogate recipe of bench.Workload, random_seed 0)."""
    import safepy_amd
    from safepy_amd import workloads
    n, m, perms = 1200, 640, 200
    dump = tmp_path / 'dump'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1',
                          '--nodes', str(n), '--attrs', str(m), '--perms', str(perms), '--dump-outputs', str(dump)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['steps'] == 4 and len(line['step_ms_slowest3']) == 3 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(float(n) * m * perms / (1e-3 * line['ms_per_step']))
    full_only = {'unseeded_device_stream', 'cpu_baseline', 'hbm_bound_kernels', 'mfma_bound_kernels', 'dropin_compute_pvalues',
                 'example3_published_shape', 'off_fast_path_shapes', 'exchange', 'multi_gpu_configs'}
    assert not full_only & set(line), sorted(full_only & set(line))
    names = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')
    assert sorted(os.listdir(dump)) == sorted(k + '.npy' for k in names + ('num_neighborhoods_enriched',))

    data = workloads.costanzo_surrogate(seed=0, n=n, m=m, target_edges=int(28202 * n / 3971))
    sf = safepy_amd.SAFE(verbose=False)
    sf.random_seed = 0
    sf.graph = safepy_amd.LayoutGraph(data['xy'], data['edge_u'], data['edge_v'], length=data['length'])
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.1)
    sf.load_attributes(attribute_file=data['attributes'])
    sf.compute_pvalues(how='randomization', num_permutations=perms)
    for k in names:
        got = np.load(dump / (k + '.npy'))
        assert got.dtype == np.float64 and got.shape == (n, m), (k, got.dtype, got.shape)
        np.testing.assert_array_equal(got, np.asarray(getattr(sf, k), dtype=np.float64), err_msg=k)
    np.testing.assert_array_equal(np.load(dump / 'num_neighborhoods_enriched.npy'),
                                  sf.attributes['num_neighborhoods_enriched'].to_numpy(dtype=np.float64))
