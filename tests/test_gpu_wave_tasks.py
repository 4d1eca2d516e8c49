"""The per-wave tasks of the blocked bit-sliced kernel (bits_plan.h: plan_bits_wave_tasks; enrich.hip: bits_blk_body): every wave
of a workgroup reads a record of its own -- (word group, slice, permutation range) -- instead of taking the slice next to its
neighbour's.  Counts and neighborhood scores against the oracle, exactly (integers), on memberships small enough for a few
seconds and shaped so that

  * a task has a wave without an item (three slices: fewer items than a multiple of four),
  * the widest slices are cut into several permutation ranges while the narrow ones are not, and ranges of ONE slice meet in one
    task (each wave flushes its own counters through atomics),
  * the second word group is ragged and some rows are all NaN,
  * one, a few and more than 255 permutations run, on the drawn stream's launches and -- the second identical call -- on the
    resident table's launches of 200,
  * the build without the id stream (SAFE_HIP_BITS_DBG=256) runs the same body,
  * a membership without any member leaves no task at all.

Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402

SEED = 13


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


def membership(rng, n, sizes):
    a = np.zeros((n, n), dtype=np.int64)
    for i, k in enumerate(sizes):
        a[i, rng.choice(n, int(k), replace=False)] = 1
    return a


def attributes(rng, n, m, nan_rows):
    b = (rng.uniform(size=(n, m)) < np.linspace(0.01, 0.9, m)).astype(np.float64)
    b[rng.choice(n, nan_rows, replace=False)] = np.nan
    return b


def small_network():
    """N = 130: three SELL slices -- one of hubs (100 .. 128 members), two of rows of 0 .. 8; m = 70: a second word group of six
    columns."""
    rng = np.random.default_rng(130)
    n, m = 130, 70
    sizes = np.r_[rng.integers(100, 129, 5), rng.integers(0, 9, n - 5)]
    rng.shuffle(sizes)
    return membership(rng, n, sizes), attributes(rng, n, m, 6)


def split_network():
    """N = 600: ten rows of 250 .. 500 members, the rest below 30 (ten slices, the first some twenty times the cost of the last);
    m = 131: three word groups, the last of three columns."""
    rng = np.random.default_rng(600)
    n, m = 600, 131
    sizes = np.r_[rng.integers(250, 501, 10), rng.integers(0, 30, n - 10)]
    rng.shuffle(sizes)
    return membership(rng, n, sizes), attributes(rng, n, m, 17)


_cases = {}


def case(name, nperm):
    """Membership, attributes and the oracle's counts and scores: computed once per (network, P), shared, never written to."""
    if name not in _cases:
        _cases[name] = small_network() if name == 'small' else split_network()
    a, b = _cases[name]
    if (name, nperm) not in _cases:
        _cases[name, nperm] = orc.run_permutations(a, b, 'sum', nperm, SEED) + (orc.compute_neighborhood_score(a, b, 'sum'),)
    return (a, b) + _cases[name, nperm]


def gpu_counts(amd, a, b, nperm):
    cn, cp = amd.run_permutations((a, b, 'sum', nperm, SEED), verbose=False)
    name, _, launches = amd.Context.default(0).last_kernel()
    assert name == 'k_permtest_bits_blk', name
    return cn, cp, launches


@pytest.mark.parametrize('nperm', [1, 40, 300])
def test_small_network_with_an_empty_wave(amd, monkeypatch, nperm):
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'bits')
    monkeypatch.delenv('SAFE_HIP_BITS_DBG', raising=False)
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    a, b, cn_want, cp_want, ns_want = case('small', nperm)
    assert a.sum(axis=1).max() >= 100 and np.isnan(b).all(axis=1).sum() == 6
    runs = [gpu_counts(amd, a, b, nperm) for _ in range(2)]                 # the drawn stream, then its resident table
    for cn, cp, _ in runs:
        assert np.array_equal(cn, cn_want) and np.array_equal(cp, cp_want)
    if nperm == 300:
        assert runs[1][2] == 2 and runs[0][2] > 2, (runs[0][2], runs[1][2])  # resident: launches of 200 | 100
    assert np.array_equal(amd.compute_neighborhood_score(a, b, 'sum'), ns_want)


def test_membership_without_members_has_no_task(amd, monkeypatch):
    """No slice has a block: the per-wave lists are empty and the launches are skipped; every permuted score equals the observed 0."""
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'bits')
    monkeypatch.delenv('SAFE_HIP_BITS_DBG', raising=False)
    rng = np.random.default_rng(3)
    a, b = np.zeros((70, 70), dtype=np.int64), attributes(rng, 70, 70, 4)
    cn_want, cp_want = orc.run_permutations(a, b, 'sum', 5, SEED)
    cn, cp, _ = gpu_counts(amd, a, b, 5)
    assert np.array_equal(cn, cn_want) and np.array_equal(cp, cp_want) and np.all(cn == 5) and np.all(cp == 5)


@pytest.mark.parametrize('dbg', [None, '256'])
def test_split_slices_meet_in_one_task(amd, monkeypatch, dbg):
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'bits')
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    if dbg is None:
        monkeypatch.delenv('SAFE_HIP_BITS_DBG', raising=False)
    else:
        monkeypatch.setenv('SAFE_HIP_BITS_DBG', dbg)                        # the plain build of the same body
    a, b, cn_want, cp_want, ns_want = case('split', 257)
    assert (a.sum(axis=1) >= 250).sum() == 10 and a.sum(axis=1).max() <= 500
    cn, cp, _ = gpu_counts(amd, a, b, 257)
    assert np.array_equal(cn, cn_want) and np.array_equal(cp, cp_want)
    assert np.array_equal(amd.compute_neighborhood_score(a, b, 'sum'), ns_want)
