"""The domain stage on the device-resident results of compute_pvalues: safe_enriched_components_dev, safe_profile_distances
and safe_node_domains (include/safe_hip.h) read nes_binary / nes in place, and SAFE.define_top_attributes / define_domains /
trim_domains use them while nobody has read the matrices -- which then stay on the device.

References.  Components: backend.enriched_components on the host slice, and networkx.connected_components per column.
Distances: live scipy.spatial.distance.pdist on the same f64 0/1 matrix, np.array_equal, NaN only where SciPy has NaN (the
count-to-distance table is tests/domain_metrics_ref.py, held to SciPy by tests/test_domain_metrics_cpu.py); Jaccard also
against backend.jaccard_condensed.  Node table: node_table_ref below, a NumPy restatement of define_domains' host path
(the reference's safe.py:693-705), bit for bit with NaN positions.  Whole stage: a SAFE instance whose results stay
resident against one whose nes / nes_binary were read to the host first.

Shapes are the smallest that reach every path: n on both sides of a 64-bit word and of the 64-row tiles (63, 64, 65, 130,
200, 300), column lists on both sides of the 64-column tiles (2, 3, 65, 130), and domain counts below and above the 64
lanes that pick a row's primary domain (2, 6, 34 and 100 ids).  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore:The sokalmichener metric:DeprecationWarning')]

from domain_metrics_ref import METRICS            # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'domains.npz')


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
    buf = ctx.alloc_f64(*host.shape)
    buf.upload(np.ascontiguousarray(host, dtype=np.float64))
    return buf


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


# ------------------------------------------------------------------------------------------------------ components ----

def component_case(n, m, seed, edges=True):
    """(edge_u, edge_v, nes_binary-like [n, m]): column 0 nothing enriched, column 1 everything, column 2 only nodes
    without any edge (isolated enriched nodes); the other columns random with densities 0.1 .. 0.9."""
    rng = np.random.default_rng(seed)
    lonely = rng.choice(n, 5, replace=False)
    pool = np.setdiff1d(np.arange(n), lonely)
    k = int(1.2 * n) if edges else 0
    eu, ev = rng.choice(pool, k), rng.choice(pool, k)
    x = (rng.uniform(size=(n, m)) < rng.uniform(0.1, 0.9, size=m)).astype(np.float64)
    x[:, 0] = 0
    x[:, 1] = 1
    x[:, 2] = 0
    x[lonely, 2] = 1
    return eu, ev, x


def networkx_labels(n, eu, ev, member):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(eu.tolist(), ev.tolist()))
    lab = np.full(n, -1, dtype=np.int32)
    for comp in nx.connected_components(g.subgraph(np.flatnonzero(member > 0).tolist())):
        lab[list(comp)] = min(comp)
    return lab


@pytest.mark.parametrize('n', [63, 64, 65, 130])
@pytest.mark.parametrize('m', [7, 70])
def test_components_from_the_resident_matrix(ctx, be, n, m):
    eu, ev, x = component_case(n, m, seed=100 * n + m)
    buf = on_device(ctx, x)
    try:
        lists = [[], [3], [1], [0], [2], [6, 0, 4, 2], [5, 5, 1, 5], list(range(m)), list(range(m - 1, -1, -2))]
        for cols in lists:
            got, ms = be.enriched_components_dev(ctx, buf.ptr, n, m, cols, eu, ev)
            assert got.shape == (len(cols), n) and got.dtype == np.int32
            if not cols:
                continue
            assert np.array_equal(got, be.enriched_components(ctx, n, eu, ev, x[:, cols])), cols
            for row, c in enumerate(cols):
                assert np.array_equal(got[row], networkx_labels(n, eu, ev, x[:, c])), (cols, c)
            assert ms > 0 and ctx.last_kernel()[0].startswith('k_cc_init_cols')
        assert np.all(be.enriched_components_dev(ctx, buf.ptr, n, m, [0], eu, ev)[0] == -1)
        iso = be.enriched_components_dev(ctx, buf.ptr, n, m, [2], eu, ev)[0][0]
        assert np.array_equal(iso[iso >= 0], np.flatnonzero(x[:, 2]))            # every isolated node is its own component
    finally:
        buf.free()


def test_components_of_a_graph_without_edges(ctx, be):
    n, m = 65, 7
    eu, ev, x = component_case(n, m, seed=5, edges=False)
    buf = on_device(ctx, x)
    try:
        got, _ = be.enriched_components_dev(ctx, buf.ptr, n, m, np.arange(m), eu, ev)
        assert np.array_equal(got, np.where(x.T > 0, np.arange(n)[None, :], -1))
        assert np.array_equal(got, be.enriched_components(ctx, n, eu, ev, x))
    finally:
        buf.free()


# -------------------------------------------------------------------------------------------------------- distances ----

M_WIDE = 150
SPECIAL = {'empty': (10, 11), 'full': (20, 21), 'same': (30, 31), 'complement': (40, 41)}


def profile_matrix(n, seed):
    """f64 0/1 [n, M_WIDE]: random columns of densities 0 .. 1 and the designed pairs of SPECIAL."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(size=(n, M_WIDE)) < rng.choice([0.02, 0.2, 0.5, 0.9], size=M_WIDE)).astype(np.float64)
    x[:, SPECIAL['empty']] = 0
    x[:, SPECIAL['full']] = 1
    x[:, SPECIAL['same'][1]] = x[:, SPECIAL['same'][0]]
    x[:, SPECIAL['complement'][1]] = 1 - x[:, SPECIAL['complement'][0]]
    return x


def column_lists(m_top, rng):
    special = [c for pair in SPECIAL.values() for c in pair]
    if m_top == 2:
        return [list(pair) for pair in SPECIAL.values()] + [[77, 3]]
    if m_top == 3:
        return [[10, 11, 20], [20, 40, 41], [30, 21, 31], [99, 5, 140]]
    rest = np.setdiff1d(np.arange(M_WIDE), special)
    return [list(rng.permutation(np.concatenate([special, rng.choice(rest, m_top - len(special), replace=False)])))]


@pytest.mark.parametrize('n', [63, 64, 65, 200])
@pytest.mark.parametrize('m_top', [2, 3, 65, 130])
def test_distances_equal_scipy_for_every_metric(ctx, be, n, m_top):
    from scipy.spatial.distance import pdist
    x = profile_matrix(n, seed=n)
    buf = on_device(ctx, x)
    try:
        for cols in column_lists(m_top, np.random.default_rng(m_top)):
            assert len(cols) == m_top
            sub = np.ascontiguousarray(x[:, cols].T)
            for metric in METRICS:
                got, ms = be.profile_distances(ctx, buf.ptr, n, M_WIDE, cols, metric)
                want = pdist(sub, metric)
                assert same_bits(got, want), (metric, cols[:4], got[:4], want[:4])
                assert ms > 0 and ctx.last_kernel()[0] == 'k_profile_pack+k_profile_pairs'
            assert np.array_equal(be.profile_distances(ctx, buf.ptr, n, M_WIDE, cols, 'jaccard')[0], be.jaccard_condensed(ctx, sub))
    finally:
        buf.free()


def test_distances_of_fewer_than_two_profiles(ctx, be):
    x = profile_matrix(64, seed=1)
    buf = on_device(ctx, x)
    try:
        for cols in ([], [7]):
            got, _ = be.profile_distances(ctx, buf.ptr, 64, M_WIDE, cols, 'dice')
            assert got.shape == (0,)
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------------------- assignment ----

def node_table_ref(nes_binary, nes, dom, ids):
    """sums, primary, primary_nes as define_domains' host path computes them (None: that path raises KeyError(0))."""
    onehot = (dom[:, None] == ids[None, :]).astype(np.float64)
    sums = nes_binary @ onehot
    real = ids >= 1
    t = sums[:, real]
    primary = np.where(t.max(axis=1) == 0, 0, ids[real][np.argmax(t, axis=1)])
    if np.any(~np.isin(primary, ids)):
        return sums, primary, None
    primary_nes = np.full(primary.shape[0], np.nan)
    with np.errstate(invalid='ignore'):
        for d in ids:
            rows = np.nonzero(primary == d)[0]
            if rows.size == 0:
                continue
            block = nes[np.ix_(rows, np.nonzero(dom == d)[0])]
            nan = np.isnan(block)
            primary_nes[rows] = np.where(nan.all(axis=1), np.nan, np.where(nan, -np.inf, block).max(axis=1))
    return sums, primary, primary_nes


def assignment_case(n, m, n_real, seed, with_zero=True):
    """Domains 0 .. n_real (every id present; ids 1 .. n_real only when not with_zero), signed NES without zeros, and the
    designed rows: 0 enriched for nothing, 1 and 2 ties between domain sums, 3 a primary domain whose NES are all NaN, 4 one
    whose NES are partly NaN, 5 all NES of the row NaN, 6 only negative NES in the primary domain."""
    rng = np.random.default_rng(seed)
    lo = 0 if with_zero else 1
    dom = np.concatenate([np.arange(lo, n_real + 1), [n_real, n_real],                       # (three attributes in the last domain)
                          rng.integers(lo, n_real + 1, size=m - (n_real + 1 - lo) - 2)]).astype(np.int64)
    dom = rng.permutation(dom)
    nb = (rng.uniform(size=(n, m)) < 0.3).astype(np.float64)
    nes = rng.normal(size=(n, m)) * 3
    nes[rng.uniform(size=(n, m)) < 0.1] = np.nan
    nb[0] = 0
    if n_real >= 2:
        for row, (a, b) in ((1, (1, 2)), (2, (n_real, n_real - 1))):          # one attribute of each of two domains: a tie
            nb[row] = 0
            nb[row, np.flatnonzero(dom == a)[0]] = 1
            nb[row, np.flatnonzero(dom == b)[0]] = 1
    for row in (3, 4, 6):
        nb[row] = 0
        nb[row, np.flatnonzero(dom == n_real)[0]] = 1                        # primary domain n_real
    of_last = np.flatnonzero(dom == n_real)
    nes[3, of_last] = np.nan
    nes[4, of_last[0]] = np.nan
    if of_last.size > 1:
        nes[4, of_last[1]] = -1.25
    nes[5] = np.nan
    nes[6, of_last] = -np.abs(nes[6, of_last])
    nes[6, of_last[-1]] = -0.5
    return nb, nes, dom, np.unique(dom)


@pytest.mark.parametrize('n', [65, 300])
@pytest.mark.parametrize('n_real', [1, 5, 33])
def test_node_domains_equal_the_host_path(ctx, be, n, n_real):
    m = 40
    nb, nes, dom, ids = assignment_case(n, m, n_real, seed=n + n_real)
    want_sums, want_primary, want_nes = node_table_ref(nb, nes, dom, ids)
    assert want_primary[0] == 0 and np.isnan(want_nes[3]) and not np.isnan(want_nes[4]) and want_nes[6] < 0
    if n_real >= 2:
        assert want_primary[1] == 1 and want_primary[2] == n_real - 1                 # first id wins a tie
    b_nb, b_nes = on_device(ctx, nb), on_device(ctx, nes)
    try:
        sums, primary, pnes, ms = be.node_domains(ctx, b_nb.ptr, b_nes.ptr, n, m, dom, ids)
        assert np.array_equal(sums, want_sums)
        assert np.array_equal(primary, want_primary) and primary.dtype == np.int32
        assert same_bits(pnes, want_nes)
        assert ms > 0 and ctx.last_kernel_busy_ms() == ms
        # the sums are safe_domain_counts' (one kernel, two forms)
        counts, _ = be.domain_counts(ctx, b_nb.ptr, np.searchsorted(ids, dom), len(ids), n, m)
        assert np.array_equal(sums, counts)
    finally:
        b_nb.free()
        b_nes.free()


def test_node_domains_with_more_ids_than_lanes_and_sparse_ids(ctx, be):
    """100 distinct ids that are not 0 .. D (the kernel works on positions in `ids`), more than a wave's 64 lanes."""
    n, m = 65, 130
    rng = np.random.default_rng(3)
    ids = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 1000), 99, replace=False))])
    dom = rng.permutation(np.concatenate([ids, rng.choice(ids, m - ids.size)]))
    nb = (rng.uniform(size=(n, m)) < 0.2).astype(np.float64)
    nb[0] = 0
    nes = rng.normal(size=(n, m))
    nes[rng.uniform(size=(n, m)) < 0.3] = np.nan
    want = node_table_ref(nb, nes, dom, ids)
    b_nb, b_nes = on_device(ctx, nb), on_device(ctx, nes)
    try:
        sums, primary, pnes, _ = be.node_domains(ctx, b_nb.ptr, b_nes.ptr, n, m, dom, ids)
        assert np.array_equal(sums, want[0]) and np.array_equal(primary, want[1]) and same_bits(pnes, want[2])
    finally:
        b_nb.free()
        b_nes.free()


def test_node_without_domain_when_every_attribute_has_one(ctx, be):
    """No attribute has domain 0: a node enriched for nothing still gets primary 0 (define_domains then raises KeyError(0),
    test_whole_stage_keyerror) with NaN as its NES; the other nodes are as on the host."""
    n, m = 65, 40
    nb, nes, dom, ids = assignment_case(n, m, 5, seed=9, with_zero=False)
    assert ids[0] == 1
    want_sums, want_primary, want_nes = node_table_ref(nb, nes, dom, ids)
    assert want_nes is None and want_primary[0] == 0
    b_nb, b_nes = on_device(ctx, nb), on_device(ctx, nes)
    try:
        sums, primary, pnes, _ = be.node_domains(ctx, b_nb.ptr, b_nes.ptr, n, m, dom, ids)
        assert np.array_equal(sums, want_sums) and np.array_equal(primary, want_primary)
        assert np.all(np.isnan(pnes[primary == 0]))
    finally:
        b_nb.free()
        b_nes.free()


# ------------------------------------------------------------------------------------------------------ whole stage ----

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


def frames_equal(a, b):
    assert list(a.columns) == list(b.columns)
    for col in a.columns:
        if col == 'size_connected_components':
            for x, y in zip(a[col], b[col]):
                assert (x is None and y is None) or np.array_equal(x, y)
        else:
            assert a[col].equals(b[col]), col


@pytest.mark.parametrize('metric', ['jaccard', 'dice', 'hamming'])
def test_whole_stage_resident_equals_host(amd, metric):
    g = dict(np.load(GOLDEN))
    dev, host = pipeline(amd, g), pipeline(amd, g)
    dev.attribute_distance_metric = host.attribute_distance_metric = metric
    assert resident(dev) == [True, True]
    assert host.nes.shape == host.nes_binary.shape == (300, 40)                  # read: this instance works on host arrays
    assert resident(host) == [False, False]
    for sf in (dev, host):
        sf.define_top_attributes()
        assert sf.attributes['top'].sum() >= 2
        sf.define_domains(attribute_distance_threshold=0.75)
    assert resident(dev) == [True, True], 'define_top_attributes / define_domains downloaded a result matrix'
    frames_equal(dev.attributes, host.attributes)
    assert dev.node2domain.equals(host.node2domain)
    assert len(np.unique(dev.attributes['domain'])) >= 2
    for sf in (dev, host):
        sf.trim_domains()
    assert resident(dev) == [True, True], 'trim_domains downloaded a result matrix'
    frames_equal(dev.attributes, host.attributes)
    assert dev.node2domain.equals(host.node2domain)
    assert dev.domains.equals(host.domains)
    # and the matrices are still what compute_pvalues made
    assert np.array_equal(dev.nes_binary, host.nes_binary) and same_bits(dev.nes, host.nes)


def test_whole_stage_keyerror(amd):
    """Every attribute in a domain and a node enriched for nothing: KeyError(0) on both paths, as in the reference."""
    g = dict(np.load(GOLDEN))
    dev, host = pipeline(amd, g), pipeline(amd, g)
    assert (host.nes_binary.sum(axis=1) == 0).any() and host.nes is not None
    for sf in (dev, host):
        sf.attributes['top'] = True
        with pytest.raises(KeyError) as err:
            sf.define_domains()
        assert err.value.args == (0,)
    assert resident(dev) == [True, True]


# ----------------------------------------------------------------------------------------------------- stream order ----

class Busy:
    """A caller's stream kept busy (tests/test_gpu_stream_order.py): the device inputs are poisoned, a chain of f32
    4096 x 4096 matmuls of at least 30 ms is enqueued on the stream, the true inputs are copied in behind it on the same
    stream, and the entry point is called while the chain still runs (asserted)."""

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


def test_components_on_a_busy_stream(ctx, be, busy):
    n, m = 130, 70
    eu, ev, x = component_case(n, m, seed=77)
    t, staging = staged(busy, x)
    cols = [1, 3, 69, 3, 40]
    got = busy.run([(t, staging)], lambda: be.enriched_components_dev(ctx, t.data_ptr(), n, m, cols, eu, ev)[0])
    assert np.array_equal(got, be.enriched_components(ctx, n, eu, ev, x[:, cols]))
    assert (got[0] >= 0).all()                     # a NaN-poisoned column 1 would have no enriched node


def test_distances_on_a_busy_stream(ctx, be, busy):
    from scipy.spatial.distance import pdist
    n = 200
    x = profile_matrix(n, seed=8)
    t, staging = staged(busy, x)
    cols = list(range(0, M_WIDE, 2))
    for metric in ('jaccard', 'yule'):
        got = busy.run([(t, staging)], lambda: be.profile_distances(ctx, t.data_ptr(), n, M_WIDE, cols, metric)[0])
        assert same_bits(got, pdist(np.ascontiguousarray(x[:, cols].T), metric)), metric


def test_node_domains_on_a_busy_stream(ctx, be, busy):
    n, m = 300, 40
    nb, nes, dom, ids = assignment_case(n, m, 5, seed=21)
    want = node_table_ref(nb, nes, dom, ids)
    t_nb, s_nb = staged(busy, nb)
    t_nes, s_nes = staged(busy, nes)
    sums, primary, pnes, _ = busy.run([(t_nb, s_nb), (t_nes, s_nes)],
                                      lambda: be.node_domains(ctx, t_nb.data_ptr(), t_nes.data_ptr(), n, m, dom, ids))
    assert np.array_equal(sums, want[0]) and np.array_equal(primary, want[1]) and same_bits(pnes, want[2])


# --------------------------------------------------------------------------------------------------------- refusals ----

def test_refusals_write_nothing(amd, ctx, be):
    from safepy_amd import _lib
    lib, h = _lib.lib, ctx.handle
    n, m = 65, 7
    eu, ev, x = component_case(n, m, seed=2)
    buf = on_device(ctx, x)
    vp = C.c_void_p
    ptr = lambda a: vp(a.ctypes.data)
    eu32, ev32 = eu.astype(np.int32), ev.astype(np.int32)
    try:
        for bad in ([0, m], [-1, 2], [3, 1 << 40]):
            cols = np.array(bad, dtype=np.int64)
            labels = np.full((2, n), 12345, dtype=np.int32)
            assert lib.safe_enriched_components_dev(h, eu32.size, ptr(eu32), ptr(ev32), vp(buf.ptr), n, m, ptr(cols), 2, ptr(labels),
                                                    None) == _lib.E_INVALID
            assert (labels == 12345).all()
            out = np.full(1, 4.5)
            assert lib.safe_profile_distances(h, vp(buf.ptr), n, m, ptr(cols), 2, 0, ptr(out), None) == _lib.E_INVALID
            assert out[0] == 4.5
            with pytest.raises(amd.SafeHipError) as err:
                be.profile_distances(ctx, buf.ptr, n, m, bad, 'jaccard')
            assert err.value.code == _lib.E_INVALID and 'column' in str(err.value)
        cols = np.array([0, 1], dtype=np.int64)
        out = np.full(1, 4.5)
        for metric in (-1, 8, 1000):
            assert lib.safe_profile_distances(h, vp(buf.ptr), n, m, ptr(cols), 2, metric, ptr(out), None) == _lib.E_INVALID
            assert 'metric' in lib.safe_last_error().decode()
        with pytest.raises(ValueError):
            be.profile_distances(ctx, buf.ptr, n, m, [0, 1], 'euclidean')
        labels = np.full((2, n), 12345, dtype=np.int32)
        # NULL pointers: context, matrix, column list, outputs, one edge array
        assert lib.safe_profile_distances(None, vp(buf.ptr), n, m, ptr(cols), 2, 0, ptr(out), None) == _lib.E_INVALID
        assert lib.safe_profile_distances(h, None, n, m, ptr(cols), 2, 0, ptr(out), None) == _lib.E_INVALID
        assert lib.safe_profile_distances(h, vp(buf.ptr), n, m, None, 2, 0, ptr(out), None) == _lib.E_INVALID
        assert lib.safe_profile_distances(h, vp(buf.ptr), n, m, ptr(cols), 2, 0, None, None) == _lib.E_INVALID
        assert lib.safe_enriched_components_dev(None, 0, None, None, vp(buf.ptr), n, m, ptr(cols), 2, ptr(labels), None) == _lib.E_INVALID
        assert lib.safe_enriched_components_dev(h, 0, None, None, None, n, m, ptr(cols), 2, ptr(labels), None) == _lib.E_INVALID
        assert lib.safe_enriched_components_dev(h, 0, None, None, vp(buf.ptr), n, m, None, 2, ptr(labels), None) == _lib.E_INVALID
        assert lib.safe_enriched_components_dev(h, 0, None, None, vp(buf.ptr), n, m, ptr(cols), 2, None, None) == _lib.E_INVALID
        assert lib.safe_enriched_components_dev(h, eu32.size, ptr(eu32), None, vp(buf.ptr), n, m, ptr(cols), 2, ptr(labels),
                                                None) == _lib.E_INVALID
        edge_out = np.array([n], dtype=np.int32)
        assert lib.safe_enriched_components_dev(h, 1, ptr(edge_out), ptr(edge_out), vp(buf.ptr), n, m, ptr(cols), 2, ptr(labels),
                                                None) == _lib.E_INVALID
        assert (labels == 12345).all() and out[0] == 4.5

        dom = np.array([0, 1, 1, 2, 0, 2, 1], dtype=np.int32)
        ids = np.array([0, 1, 2], dtype=np.int32)
        sums, primary, pnes = np.full((n, 3), 4.5), np.full(n, 12345, dtype=np.int32), np.full(n, 4.5)

        def node(hh=h, a=vp(buf.ptr), b=vp(buf.ptr), d=dom, i=ids, k=3, s=sums, p=primary, q=pnes):
            return lib.safe_node_domains(hh, a, b, n, m, ptr(d) if d is not None else None, ptr(i) if i is not None else None, k,
                                         ptr(s) if s is not None else None, ptr(p) if p is not None else None,
                                         ptr(q) if q is not None else None, None)
        assert node(hh=None) == _lib.E_INVALID and node(a=None) == _lib.E_INVALID and node(b=None) == _lib.E_INVALID
        assert node(d=None) == _lib.E_INVALID and node(i=None) == _lib.E_INVALID and node(s=None) == _lib.E_INVALID
        assert node(p=None) == _lib.E_INVALID and node(q=None) == _lib.E_INVALID and node(k=0) == _lib.E_INVALID
        assert node(d=np.array([0, 1, 1, 3, 0, 2, 1], dtype=np.int32)) == _lib.E_VALUE            # an id that is not listed
        assert node(i=np.array([0, 2, 1], dtype=np.int32)) == _lib.E_VALUE                       # ids not sorted
        assert node(i=np.array([0, 1, 1], dtype=np.int32)) == _lib.E_VALUE                       # ids not distinct
        many = np.arange(be.Context.NODE_DOMAINS_MAX + 1, dtype=np.int32)
        assert node(i=many, k=many.size) == _lib.E_UNSUPPORTED
        assert (sums == 4.5).all() and (primary == 12345).all() and (pnes == 4.5).all()
        assert node() == 0 and (primary != 12345).all()
    finally:
        buf.free()
