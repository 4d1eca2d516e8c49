"""Restricted permutations generated on the device (safe_perms_create_device_strata, backend.Permutations.stratified): the
tables bit for bit against the NumPy restatement (tests/strata_ref.py) over the partitions that exercise both forms of the
kernel -- strata shuffled by one lane, strata shuffled by the whole wave -- and everything a handle has to do (the handle on a
busy caller stream: tests/test_gpu_stream_strata.py).  A table row
depends on (key, movable rows, partition, permutation index) only, so the restatement is made once per (k, partition) at the
largest P and its leading rows serve the smaller ones.  Needs an MI355X."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)
import strata_ref as sr                           # noqa: E402
from safepy_amd._lib import E_INVALID, E_UNSUPPORTED, E_VALUE      # noqa: E402

KEY = 0x5AFE0C0DE0000 + 0xB0C7
COUNTS = (1, 3, 130)
SIZES = (1, 2, 63, 64, 65, 257, 4097)
PARTITIONS = ('singletons', 'pairs', 'halves', 'large_and_small', 'strata64', 'strata65')


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module', autouse=True)
def nothing_left_for_later_modules():
    """Objects of this module that still own device memory are released when it ends, not by a garbage collection inside a
    later module's busy-stream case (a release waits for the device and would drain that case's stream)."""
    yield
    gc.collect()


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


def stratum_sizes(kind, k, rng):
    if kind == 'singletons':
        return [1] * k
    if kind == 'pairs':
        return [2] * (k // 2) + [1] * (k % 2)
    if kind == 'halves':
        return [s for s in (k // 2, k - k // 2) if s]
    if kind == 'large_and_small':                     # one stratum of half the rows, the others of 1 - 3
        sizes, left = [max(1, k // 2)], k - max(1, k // 2)
        while left:
            sizes.append(int(min(left, rng.integers(1, 4))))
            left -= sizes[-1]
        return sizes
    count = {'strata64': 64, 'strata65': 65}[kind]    # (callers ask for these at k >= count only)
    return [len(part) for part in np.array_split(np.arange(k), count)]


def layout(sizes, rng, fixed_every=5):
    """(n, movable, labels) for strata of the given sizes: the strata interleaved in node order, a row that does not move after
    every few that do, labels neither contiguous nor sorted by rank order of appearance, garbage (negative values included) on
    the rows that do not move."""
    k = int(sum(sizes))
    n = k + k // fixed_every + 3
    movable = np.zeros(n, dtype=np.uint8)
    movable[rng.choice(n, k, replace=False)] = 1
    names = rng.choice(2 ** 31 - 1, len(sizes), replace=False)               # distinct labels >= 0 in no order
    of_row = np.repeat(names, sizes)
    rng.shuffle(of_row)
    labels = rng.integers(-2 ** 31, 2 ** 31 - 1, size=n)                      # garbage where nothing moves
    labels[movable == 1] = of_row
    return n, movable, labels.astype(np.int32)


def check_structure(tables, n, movable, labels):
    assert (np.sort(tables, axis=1) == np.arange(n)).all()                    # every row a permutation
    fixed = movable == 0
    assert (tables[:, fixed] == np.flatnonzero(fixed)).all()                  # rows without a value never move
    assert (labels[tables][:, ~fixed] == labels[~fixed]).all()                # a row only ever takes a row of its own stratum


CASES = [(k, kind) for k in SIZES for kind in PARTITIONS if not (kind.startswith('strata6') and k < int(kind[6:]))]


@pytest.mark.parametrize('k,kind', CASES)
def test_tables_equal_the_restatement(be, ctx, k, kind):
    rng = np.random.default_rng(k * 131 + PARTITIONS.index(kind))
    n, movable, labels = layout(stratum_sizes(kind, k, rng), rng)
    want = sr.strata_tables(n, movable, labels, max(COUNTS), KEY)
    check_structure(want, n, movable, labels)
    for count in COUNTS:
        perms = be.Permutations.stratified(ctx, n, movable, labels, count, KEY)
        got = perms.read().astype(np.int64)
        assert perms.timing()['role'] == 'device' and perms.device_key == KEY
        perms.close()
        np.testing.assert_array_equal(got, want[:count], err_msg='P = %d' % count)


def test_every_stratum_size_up_to_300(be, ctx, monkeypatch):
    """One stratum of every size 1 .. 300 (45150 movable rows): whatever the size at which a stratum moves from the lane form
    to the wave form, the sweep straddles it; and the tables are the same bytes with that size set to 2 (every stratum of two
    or more rows by the wave), to 17 and far above every stratum (every stratum by one lane)."""
    rng = np.random.default_rng(300)
    n, movable, labels = layout(list(range(1, 301)), rng, fixed_every=50)
    want = sr.strata_tables(n, movable, labels, 2, KEY)
    check_structure(want, n, movable, labels)
    for wave_min in (None, '2', '17', '100000'):
        if wave_min is None:
            monkeypatch.delenv('SAFE_HIP_STRATA_WAVE_MIN', raising=False)
        else:
            monkeypatch.setenv('SAFE_HIP_STRATA_WAVE_MIN', wave_min)
        perms = be.Permutations.stratified(ctx, n, movable, labels, 2, KEY)
        got = perms.read().astype(np.int64)
        perms.close()
        np.testing.assert_array_equal(got, want, err_msg='SAFE_HIP_STRATA_WAVE_MIN=%s' % wave_min)


@pytest.mark.parametrize('wave_min', ['2', '100000'])
def test_both_forms_give_the_same_tables(be, ctx, monkeypatch, wave_min):
    """The lane form and the wave form are one algorithm: the partitions of the main test at k = 257, every stratum forced
    through one form."""
    monkeypatch.setenv('SAFE_HIP_STRATA_WAVE_MIN', wave_min)
    for kind in ('pairs', 'halves', 'large_and_small', 'strata65'):
        rng = np.random.default_rng(257 * 131 + PARTITIONS.index(kind))
        n, movable, labels = layout(stratum_sizes(kind, 257, rng), rng)
        perms = be.Permutations.stratified(ctx, n, movable, labels, 3, KEY)
        got = perms.read().astype(np.int64)
        perms.close()
        np.testing.assert_array_equal(got, sr.strata_tables(n, movable, labels, 3, KEY), err_msg=kind)


@pytest.mark.parametrize('k', SIZES)
def test_one_stratum_is_the_device_stream(be, ctx, k):
    rng = np.random.default_rng(k)
    n, movable, labels = layout([k], rng)
    for count in COUNTS:
        plain = be.Permutations(ctx, n, movable, count, None, device_key=KEY)
        want = plain.read()
        plain.close()
        perms = be.Permutations.stratified(ctx, n, movable, labels, count, KEY)
        got = perms.read()
        perms.close()
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:3].astype(np.int64), orc.device_stream_tables(n, movable, 3, KEY))


def test_limit_of_movable_rows(be, ctx):
    """65535 movable rows in two strata are generated; 65536 are refused, nothing allocated."""
    k, n = 65535, 65600
    rng = np.random.default_rng(65535)
    movable = np.zeros(n, dtype=np.uint8)
    movable[rng.choice(n, k, replace=False)] = 1
    labels = rng.integers(0, 2, size=n).astype(np.int32) * 9 + 4
    perms = be.Permutations.stratified(ctx, n, movable, labels, 2, KEY)
    got = perms.read().astype(np.int64)
    perms.close()
    check_structure(got, n, movable, labels)
    np.testing.assert_array_equal(got, sr.strata_tables(n, movable, labels, 2, KEY))
    movable[np.flatnonzero(movable == 0)[0]] = 1
    live = be.device_live_alloc_count()
    h = C.c_void_p(12345)
    rc = be.lib.safe_perms_create_device_strata(ctx.handle, n, movable.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p), 2,
                                                C.c_uint64(KEY), C.byref(h))
    assert rc == E_UNSUPPORTED
    assert h.value is None and be.device_live_alloc_count() == live
    with pytest.raises(Exception, match='65536 movable rows'):
        be.Permutations.stratified(ctx, n, movable, labels, 2, KEY)


def test_refusals_write_nothing(be, ctx):
    n = 40
    movable = np.ones(n, dtype=np.uint8)
    labels = (np.arange(n) % 3).astype(np.int32)
    mp, lp = movable.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p)
    create = be.lib.safe_perms_create_device_strata
    bad = labels.copy()
    bad[7] = -1
    live = be.device_live_alloc_count()
    for want, args in [(E_INVALID, (None, n, mp, lp, 5)), (E_INVALID, (ctx.handle, n, None, lp, 5)), (E_INVALID, (ctx.handle, n, mp, None, 5)),
                       (E_INVALID, (ctx.handle, 0, mp, lp, 5)), (E_INVALID, (ctx.handle, 2 ** 31 - 1, mp, lp, 5)),
                       (E_INVALID, (ctx.handle, n, mp, lp, -1)), (E_VALUE, (ctx.handle, n, mp, bad.ctypes.data_as(C.c_void_p), 5))]:
        h = C.c_void_p(12345)
        assert create(*args, C.c_uint64(KEY), C.byref(h)) == want, args
        assert h.value is None, args
        assert be.device_live_alloc_count() == live, args
    assert create(ctx.handle, n, mp, lp, 5, C.c_uint64(KEY), None) == E_INVALID
    movable[7] = 0                                    # the negative label sits on a row that does not move: not read
    perms = be.Permutations.stratified(ctx, n, movable, bad, 5, KEY)
    np.testing.assert_array_equal(perms.read().astype(np.int64), sr.strata_tables(n, movable, bad, 5, KEY))
    perms.close()


def test_empty_calls(be, ctx):
    """P = 0 and no movable row at all are valid, as for safe_perms_create_device."""
    n = 17
    labels = np.arange(n, dtype=np.int32) % 4
    perms = be.Permutations.stratified(ctx, n, np.ones(n, dtype=np.uint8), labels, 0, KEY)
    assert perms.read().shape == (0, n) and perms.timing()['role'] == 'device'
    perms.close()
    perms = be.Permutations.stratified(ctx, n, np.zeros(n, dtype=np.uint8), labels, 4, KEY)
    np.testing.assert_array_equal(perms.read(), np.tile(np.arange(n), (4, 1)))
    perms.close()


def test_handle_slice_read_repeat_and_keys(be, ctx):
    rng = np.random.default_rng(77)
    n, movable, labels = layout([40, 3, 1, 200, 2, 2, 17], rng)
    want = sr.strata_tables(n, movable, labels, 12, KEY)
    perms = be.Permutations.stratified(ctx, n, movable, labels, 12, KEY)
    assert perms.timing()['role'] == 'device'
    np.testing.assert_array_equal(perms.read(4, 9).astype(np.int64), want[4:9])
    part = perms.slice(2, 7)
    np.testing.assert_array_equal(part.read().astype(np.int64), want[2:7])
    part.close()
    first = perms.read()
    perms.close()
    again = be.Permutations.stratified(ctx, n, movable, labels, 12, KEY)      # (the buffers of the last handle are reused)
    assert again.read().tobytes() == first.tobytes()
    again.close()
    other = be.Permutations.stratified(ctx, n, movable, labels, 12, KEY + 1)
    assert not np.array_equal(other.read(), first)
    other.close()
    fresh = be.Permutations.stratified(ctx, n, movable, labels, 12, None)     # OS entropy
    assert fresh.device_key != KEY and not np.array_equal(fresh.read(), first)
    fresh.close()
    # a seeded handle of the same shape afterwards draws its own NumPy-compatible stream: the stratified table was not kept
    seeded = be.Permutations(ctx, n, movable, 12, 5)
    assert seeded.timing()['role'] == 'own'
    b = np.where(movable[:, None] == 1, 0.0, np.nan)                          # (a matrix whose rows with a value are `movable`)
    np.testing.assert_array_equal(seeded.read(), orc.permutation_index_table(b, 12, 5))
    seeded.close()
