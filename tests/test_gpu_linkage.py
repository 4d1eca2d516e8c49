"""Average linkage on the device: safe_linkage_average and safe_profile_linkage (include/safe_hip.h; k_linkage_expand and
k_linkage_nn_chain in domains.hip) and SAFE.define_domains on device-resident results, which now clusters there.

Reference.  Every comparison is with live scipy.cluster.hierarchy.linkage(cond, method='average') on the same condensed
vector: the bits of Z (uint64 views), and equal fcluster output at 0.75 of the largest height.  tests/linkage_ref.py
documents the algorithm and is held to SciPy on the CPU (tests/test_linkage_ref_cpu.py); it is not the reference here.

Sizes.  m_top in 2, 3, 4 (the smallest chains), 63 / 64 / 65 (one wave and the first two-wave workgroup), 130, 257 and 1025
(more points than the 1024 lanes of the workgroup: a lane scans more than one column).  Inputs: the eight boolean metrics on
profiles of 10 .. 16 rows (small rationals: heavy ties), all distances equal (every step a tie), distinct random distances
(no tie), points on a line with strictly decreasing gaps (the chain grows through all m_top points before the first merge:
the longest chain), profiles with exact duplicates (zero distances, clusters larger than one from the first merge on).
Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore:The sokalmichener metric:DeprecationWarning')]

from domain_metrics_ref import METRICS            # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'domains.npz')
SIZES = (2, 3, 4, 63, 64, 65, 130, 257, 1025)
KERNEL = 'k_linkage_nn_chain'


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(scope='module')
def be():
    from safepy_amd import backend
    return backend


def on_device(ctx, host):
    host = np.ascontiguousarray(host, dtype=np.float64)
    buf = ctx.alloc_f64(max(host.size, 1))
    if host.size:
        buf.upload(host)
    return buf


def assert_same_linkage(got, cond, what):
    from scipy.cluster.hierarchy import fcluster, linkage
    want = linkage(cond, method='average')
    assert got.shape == want.shape and got.dtype == np.float64, what
    same = got.view(np.uint64) == want.view(np.uint64)
    if not same.all():
        row = int(np.flatnonzero(~same.all(axis=1))[0])
        raise AssertionError('%s: Z differs from SciPy first at row %d of %d: got %r, want %r'
                             % (what, row, want.shape[0], got[row].tolist(), want[row].tolist()))
    max_d = np.max(want[:, 2] * 0.75)
    assert np.array_equal(fcluster(got, max_d, criterion='distance'), fcluster(want, max_d, criterion='distance')), what


def run_vector(ctx, be, cond, n, what):
    """safe_linkage_average on a device copy of cond (which it must leave as it was) against SciPy."""
    cond = np.ascontiguousarray(cond, dtype=np.float64)
    assert cond.shape == (n * (n - 1) // 2,) and np.isfinite(cond).all()
    buf = on_device(ctx, cond)
    try:
        got, ms = be.linkage_average(ctx, buf.ptr, n)
        assert ms > 0 and ctx.last_kernel()[0] == 'k_linkage_expand+' + KERNEL
        assert np.array_equal(buf.download(cond.shape).view(np.uint64), cond.view(np.uint64)), 'the input vector was modified'
    finally:
        buf.free()
    assert_same_linkage(got, cond, what)


# ---------------------------------------------------------------------------------------------- the vector entry point ----

@pytest.mark.parametrize('n', SIZES)
def test_boolean_metric_distances_with_heavy_ties(ctx, be, n):
    """Each of the eight boolean metrics on random profiles of 10 .. 16 rows; a vector that is not finite (dice / sokalsneath
    of two empty profiles) is drawn again with the next seed."""
    from scipy.spatial.distance import pdist
    tied = 0
    for k, metric in enumerate(METRICS):
        for seed in range(8):
            rng = np.random.default_rng(1000 * n + 10 * k + seed)
            x = rng.random((n, int(rng.integers(10, 17)))) < rng.uniform(0.3, 0.7)
            cond = pdist(x, metric)
            if np.isfinite(cond).all():
                break
        else:
            raise AssertionError('no finite %s vector for %d profiles' % (metric, n))
        tied += len(np.unique(cond)) < len(cond)
        run_vector(ctx, be, cond, n, (metric, n))
    assert n < 63 or tied == len(METRICS)                         # (from 63 profiles on every vector has tied distances)


@pytest.mark.parametrize('n', SIZES)
def test_all_distances_equal(ctx, be, n):
    """Every scan and every merge is a tie: the smallest live index, the chain predecessor and the stable sort decide."""
    for value in (0.5, 0.0, 1.0 / 3.0):
        run_vector(ctx, be, np.full(n * (n - 1) // 2, value), n, ('equal', value, n))


@pytest.mark.parametrize('n', SIZES)
def test_distinct_random_distances(ctx, be, n):
    cond = np.random.default_rng(n).random(n * (n - 1) // 2)
    assert len(np.unique(cond)) == len(cond)
    run_vector(ctx, be, cond, n, ('distinct', n))


@pytest.mark.parametrize('n', SIZES)
def test_points_on_a_line_with_decreasing_gaps(ctx, be, n):
    """The nearest neighbour of point i is i + 1 for every i: starting from point 0 the chain holds all n points before the
    first merge (the last two), the longest chain there is."""
    from scipy.spatial.distance import pdist
    gaps = np.linspace(2.0, 1.0, n - 1) if n > 2 else np.array([1.0])
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    assert np.all(np.diff(gaps) < 0) and np.all(np.diff(np.diff(pos)) < 0)
    run_vector(ctx, be, pdist(pos[:, None]), n, ('line', n))


@pytest.mark.parametrize('n', SIZES)
def test_profiles_with_exact_duplicates(ctx, be, n):
    """About three copies of every profile: zero distances, and merged clusters (size > 1) take part from the start."""
    from scipy.spatial.distance import pdist
    rng = np.random.default_rng(7 * n)
    base = rng.random((max(n // 3, 1), 12)) < 0.5
    base[:, 0] = True
    x = base[rng.integers(0, base.shape[0], size=n)]
    for metric in ('jaccard', 'hamming'):
        cond = pdist(x, metric)
        assert n < 4 or (cond == 0).any()
        run_vector(ctx, be, cond, n, ('duplicates', metric, n))


def test_a_host_vector_is_uploaded(ctx, be):
    from scipy.spatial.distance import pdist
    x = np.random.default_rng(3).random((65, 12)) < 0.5
    cond = pdist(x, 'hamming')
    got, ms = be.linkage_average(ctx, cond)
    assert ms > 0
    assert_same_linkage(got, cond, 'host vector')
    with pytest.raises(ValueError):
        be.linkage_average(ctx, cond[:-1])
    with pytest.raises(ValueError):
        be.linkage_average(ctx, 12345)                               # a device pointer without m_top


# ----------------------------------------------------------------------------------------------------- the fused call ----

M_WIDE = 150


def resident_matrix(n, seed):
    """f64 0/1 [n, M_WIDE]: random columns of several densities; columns 10 and 11 empty, 20 and 21 full, 31 a copy of 30."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(size=(n, M_WIDE)) < rng.choice([0.05, 0.2, 0.5, 0.9], size=M_WIDE)).astype(np.float64)
    x[:, [10, 11]] = 0
    x[:, [20, 21]] = 1
    x[:, 31] = x[:, 30]
    return x


@pytest.mark.parametrize('n', [63, 65, 200])
def test_fused_call_from_a_resident_matrix(ctx, be, n):
    """safe_profile_linkage on a [n, 150] matrix wider than its column list, the list unsorted and with repeats: Z of SciPy's
    linkage on SciPy's pdist of those columns, and of the two separate calls."""
    from scipy.spatial.distance import pdist
    x = resident_matrix(n, seed=n)
    rng = np.random.default_rng(n + 1)
    buf = on_device(ctx, x)
    try:
        for m_top in (2, 3, 70, 131):
            cols = rng.integers(0, M_WIDE, size=m_top)
            cols[-1] = cols[0]                                       # at least one repeat, far apart
            if m_top > 3:
                cols[:6] = [30, 11, 31, 10, 20, 21]                  # the designed columns, unsorted
            for metric in ('jaccard', 'hamming', 'yule'):
                cond = pdist(np.ascontiguousarray(x[:, cols].T), metric)
                got, ms = be.profile_linkage(ctx, buf.ptr, n, M_WIDE, cols, metric)
                assert ms > 0 and ctx.last_kernel()[0] == 'k_profile_pack+k_profile_pairs+k_linkage_expand+' + KERNEL
                assert_same_linkage(got, cond, (metric, n, m_top))
                dist, _ = be.profile_distances(ctx, buf.ptr, n, M_WIDE, cols, metric)
                assert np.array_equal(dist, cond)
                assert np.array_equal(be.linkage_average(ctx, dist)[0].view(np.uint64), got.view(np.uint64))
        assert np.array_equal(buf.download(x.shape), x)
    finally:
        buf.free()


# ----------------------------------------------------------------------------------------------------------- refusals ----

def test_refusals_write_nothing(amd, ctx, be):
    from safepy_amd import _lib
    lib, h = _lib.lib, ctx.handle
    vp = C.c_void_p
    ptr = lambda a: vp(a.ctypes.data)
    n, k = 65, 40
    x = resident_matrix(n, seed=5)
    mat = on_device(ctx, x)
    good = np.random.default_rng(0).random(k * (k - 1) // 2)
    cap = be.Context.LINKAGE_MAX_POINTS
    assert cap >= 8192 and cap == _lib.LINKAGE_MAX_POINTS
    try:
        # a distance that is not finite: first, in the middle, last; +inf, -inf and NaN
        for pos in (0, good.size // 2, good.size - 1):
            for value in (np.nan, np.inf, -np.inf):
                cond = good.copy()
                cond[pos] = value
                buf = on_device(ctx, cond)
                try:
                    z = np.full((k - 1, 4), 4.5)
                    assert lib.safe_linkage_average(h, vp(buf.ptr), k, ptr(z), None) == _lib.E_VALUE, (pos, value)
                    assert 'finite' in lib.safe_last_error().decode()
                    assert (z == 4.5).all()
                    with pytest.raises(amd.SafeHipError) as err:
                        be.linkage_average(ctx, cond)
                    assert err.value.code == _lib.E_VALUE
                finally:
                    buf.free()
        # dice and sokalsneath of the two empty columns: 0 / 0
        cols = np.array([3, 10, 40, 11, 7], dtype=np.int64)
        for metric in ('dice', 'sokalsneath'):
            z = np.full((cols.size - 1, 4), 4.5)
            assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(cols), cols.size, _lib.METRIC_IDS[metric], ptr(z),
                                            None) == _lib.E_VALUE
            assert (z == 4.5).all()
            with pytest.raises(amd.SafeHipError) as err:
                be.profile_linkage(ctx, mat.ptr, n, M_WIDE, cols, metric)
            assert err.value.code == _lib.E_VALUE
        assert be.profile_linkage(ctx, mat.ptr, n, M_WIDE, cols, 'jaccard')[0].shape == (4, 4)       # (finite for jaccard)
        # more points than the working matrix is built for: refused before anything is read or allocated
        z = np.full((3, 4), 4.5)
        small = on_device(ctx, good)
        try:
            assert lib.safe_linkage_average(h, vp(small.ptr), cap + 1, ptr(z), None) == _lib.E_UNSUPPORTED
            assert str(cap) in lib.safe_last_error().decode()
        finally:
            small.free()
        many = np.zeros(cap + 1, dtype=np.int64)
        assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(many), many.size, 0, ptr(z), None) == _lib.E_UNSUPPORTED
        with pytest.raises(amd.SafeHipError) as err:
            be.profile_linkage(ctx, mat.ptr, n, M_WIDE, many, 'jaccard')
        assert err.value.code == _lib.E_UNSUPPORTED
        # fewer than two points: nothing to do, nothing written
        for m_top in (0, 1):
            ms = C.c_double(-1.0)
            assert lib.safe_linkage_average(h, vp(mat.ptr), m_top, ptr(z), C.byref(ms)) == 0 and ms.value == 0
            assert lib.safe_linkage_average(h, None, m_top, None, None) == 0
            assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(cols), m_top, 0, ptr(z), None) == 0
            assert be.profile_linkage(ctx, mat.ptr, n, M_WIDE, cols[:m_top], 'dice')[0].shape == (0, 4)
            assert be.linkage_average(ctx, np.empty(0))[0].shape == (0, 4)
        assert be.linkage_average(ctx, mat.ptr, 1)[0].shape == (0, 4)
        # the checks of safe_profile_distances: columns, metric ids, NULL pointers
        for bad in ([0, M_WIDE], [-1, 2], [3, 1 << 40]):
            cols2 = np.array(bad, dtype=np.int64)
            assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(cols2), 2, 0, ptr(z), None) == _lib.E_INVALID
            assert 'column' in lib.safe_last_error().decode()
        for metric in (-1, 8, 1000):
            assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(cols), 2, metric, ptr(z), None) == _lib.E_INVALID
            assert 'metric' in lib.safe_last_error().decode()
        with pytest.raises(ValueError):
            be.profile_linkage(ctx, mat.ptr, n, M_WIDE, [0, 1], 'euclidean')
        assert lib.safe_profile_linkage(None, vp(mat.ptr), n, M_WIDE, ptr(cols), 2, 0, ptr(z), None) == _lib.E_INVALID
        assert lib.safe_profile_linkage(h, None, n, M_WIDE, ptr(cols), 2, 0, ptr(z), None) == _lib.E_INVALID
        assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, None, 2, 0, ptr(z), None) == _lib.E_INVALID
        assert lib.safe_profile_linkage(h, vp(mat.ptr), n, M_WIDE, ptr(cols), 2, 0, None, None) == _lib.E_INVALID
        assert lib.safe_linkage_average(None, vp(mat.ptr), 3, ptr(z), None) == _lib.E_INVALID
        assert lib.safe_linkage_average(h, None, 3, ptr(z), None) == _lib.E_INVALID
        assert lib.safe_linkage_average(h, vp(mat.ptr), 3, None, None) == _lib.E_INVALID
        assert lib.safe_linkage_average(h, vp(mat.ptr), -1, ptr(z), None) == _lib.E_INVALID
        assert (z == 4.5).all()
    finally:
        mat.free()


# ------------------------------------------------------------------------------------------------------- stream order ----

class Busy:
    """A caller's stream kept busy (the fixture of tests/test_gpu_domain_stage.py, restated): the device inputs are poisoned
    with NaN, a chain of f32 4096 x 4096 matmuls of at least 30 ms is enqueued on the stream, the true inputs are copied in
    behind it on the same stream, and the entry point is called while the chain still runs (asserted).  A call that read its
    input ahead of the stream would see NaN and refuse it."""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx = torch, ctx
        self.s = torch.cuda.Stream()
        self.a = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device='cuda')
        self.c = torch.empty_like(self.a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            for _ in range(3):
                torch.mm(self.a, self.a, out=self.c)
            e0.record(self.s)
            for _ in range(4):
                torch.mm(self.a, self.a, out=self.c)
            e1.record(self.s)
        e1.synchronize()
        self.links = int(np.ceil(30.0 / max(e0.elapsed_time(e1) / 4.0, 0.02)))

    def run(self, inputs, call):
        """inputs: [(device tensor, staging tensor)]; returns call()'s result from the busy stream."""
        torch = self.torch
        torch.cuda.synchronize()
        self.ctx.set_stream(self.s.cuda_stream)
        try:
            with torch.cuda.stream(self.s):
                for t, _ in inputs:
                    t.fill_(float('nan'))
                for _ in range(self.links):
                    torch.mm(self.a, self.a, out=self.c)
                done = torch.cuda.Event()
                done.record(self.s)
                for t, staging in inputs:
                    t.copy_(staging)
            assert not done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
            out = call()
            with torch.cuda.stream(self.s):
                for t, _ in inputs:
                    t.fill_(float('nan'))
            self.s.synchronize()
        finally:
            self.ctx.set_stream(None)
            torch.cuda.synchronize()
        return out


@pytest.fixture(scope='module')
def busy(ctx):
    import torch
    assert torch.cuda.is_available()
    return Busy(ctx)


def staged(busy, host):
    torch = busy.torch
    staging = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)).cuda()
    return torch.empty_like(staging), staging


def test_linkage_on_a_busy_stream(ctx, be, busy):
    from scipy.spatial.distance import pdist
    n = 130
    x = np.random.default_rng(11).random((n, 14)) < 0.4
    cond = pdist(x, 'jaccard')
    t, staging = staged(busy, cond)
    got = busy.run([(t, staging)], lambda: be.linkage_average(ctx, t.data_ptr(), n)[0])
    assert_same_linkage(got, cond, 'busy stream')


def test_fused_call_on_a_busy_stream(ctx, be, busy):
    from scipy.spatial.distance import pdist
    n = 200
    x = resident_matrix(n, seed=8)
    t, staging = staged(busy, x)
    cols = list(range(M_WIDE - 1, 0, -2))
    for metric in ('jaccard', 'yule'):
        got = busy.run([(t, staging)], lambda: be.profile_linkage(ctx, t.data_ptr(), n, M_WIDE, cols, metric)[0])
        assert_same_linkage(got, pdist(np.ascontiguousarray(x[:, cols].T), metric), ('busy stream', metric))


# -------------------------------------------------------------------------------------------------------- whole stage ----

def pipeline(amd, g):
    import pandas as pd
    sf = amd.SAFE(verbose=False)
    xy, eu, ev = g['xy'], g['edge_u'], g['edge_v']
    length = np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1))
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length)
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
    sf.load_attributes(attribute_file=g['attributes'].copy())
    sf.attributes = pd.DataFrame({'id': np.arange(len(g['names'])), 'name': list(g['names'])})
    sf.compute_pvalues()
    return sf


def resident(sf):
    from safepy_amd.safe import _DeviceResult
    return [isinstance(sf.__dict__.get(slot), _DeviceResult) for slot in ('_r_nes', '_r_nes_binary')]


class Spy:
    """Records what Context.profile_linkage / profile_distances did inside define_domains: the kernel the context named right
    after each call (define_domains goes on to safe_node_domains, which records its own kernel, so the name is read here and
    not after define_domains returns), or the error code."""

    def __init__(self, monkeypatch, be):
        self.calls = []
        for name in ('profile_linkage', 'profile_distances'):
            real = getattr(be.Context, name)                          # AttributeError without the linkage entry point
            monkeypatch.setattr(be.Context, name, self.wrap(name, real))

    def wrap(self, name, real):
        from safepy_amd import SafeHipError

        def f(ctx, *a):
            try:
                got = real(ctx, *a)
            except SafeHipError as err:
                self.calls.append((name, err.code))
                raise
            self.calls.append((name, ctx.last_kernel()[0]))
            return got
        return f


@pytest.mark.parametrize('metric', ['jaccard', 'dice', 'hamming'])
def test_whole_stage_clusters_on_the_device(amd, be, monkeypatch, metric):
    """A SAFE instance whose results stay resident against one that works on host arrays (SciPy's linkage): the same domains
    and node table, from the linkage kernel, with nes / nes_binary still on the device."""
    g = dict(np.load(GOLDEN))
    dev, host = pipeline(amd, g), pipeline(amd, g)
    dev.attribute_distance_metric = host.attribute_distance_metric = metric
    assert host.nes.shape == host.nes_binary.shape == (300, 40)                  # read: this instance works on host arrays
    assert resident(dev) == [True, True] and resident(host) == [False, False]
    for sf in (dev, host):
        sf.define_top_attributes()
        assert sf.attributes['top'].sum() >= 2
    host.define_domains(attribute_distance_threshold=0.75)
    spy = Spy(monkeypatch, be)
    dev.define_domains(attribute_distance_threshold=0.75)
    assert [name for name, _ in spy.calls] == ['profile_linkage'] and KERNEL in spy.calls[0][1], spy.calls
    assert resident(dev) == [True, True], 'define_domains downloaded a result matrix'
    assert dev.attributes['domain'].equals(host.attributes['domain'])
    assert dev.node2domain.equals(host.node2domain)
    assert len(np.unique(dev.attributes['domain'])) >= 2


def test_whole_stage_falls_back_where_scipy_refuses(amd, be, monkeypatch):
    """dice with two top attributes that no node is enriched for: the distances hold NaN, the linkage entry point refuses them
    and define_domains takes the earlier path, which ends in SciPy's own ValueError -- on the resident instance as on the host
    one -- and leaves the matrices resident."""
    g = dict(np.load(GOLDEN))
    g['attributes'] = g['attributes'].copy()
    g['attributes'][:, [4, 9]] = 0
    dev, host = pipeline(amd, g), pipeline(amd, g)
    dev.attribute_distance_metric = host.attribute_distance_metric = 'dice'
    assert not host.nes_binary[:, [4, 9]].any()
    messages = []
    for sf in (host, dev):
        sf.define_top_attributes()
        sf.attributes.loc[[4, 9], 'top'] = True
        spy = Spy(monkeypatch, be) if sf is dev else None
        with pytest.raises(ValueError) as err:
            sf.define_domains()
        messages.append(str(err.value))
    from safepy_amd import _lib
    assert spy.calls[0] == ('profile_linkage', _lib.E_VALUE) and spy.calls[1][0] == 'profile_distances', spy.calls
    assert messages[0] == messages[1] and 'finite' in messages[0]
    assert resident(dev) == [True, True]
