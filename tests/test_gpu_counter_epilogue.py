"""The counter-to-output epilogue (enrich.hip: k_counts_finalize behind enrich_finalize_counts, k_counts_to_outputs) and the
20-bit exchange form (k_pack_counts20, the PK20 read) on DESIGNED counters: the consumers take counters from the caller, so
a plain NumPy restatement of safepy/safe.py:532-554, 468-472 (tests/counter_ref.py, itself checked against the oracle on the
CPU) pins them at permutation counts, counter values and column geometries that real permutation runs of test size never
leave behind -- every bit of both fields, both sides of each table variant's limit (NES and k / P tables in LDS up to
P = 1279, the NES table alone up to 2559, global memory above), full 16-bit fields at P = 65 535, 512-column tile tails,
ragged slabs inside a wider matrix.  With the NES table handed over (nes_table_host) every output is bit-equal.

The consumers scatter position `pos` of a counter column to row rowmap[pos]; the map is not exported, so the fixture
recovers it from one real call per layout (exported counters against safe_permtest_counts of the same handles) and every
designed slab poisons the padding positions.  Needs an MI355X; every test well under a second."""
import ctypes as C
import itertools

import numpy as np
import pytest

import counter_ref as cr
from oracle import safe_oracle as orc

pytestmark = pytest.mark.gpu

N = 200                                     # one 256-position group in both layouts: 56 padding positions
P_U32 = (1, 2, 255, 256, 1023, 1024, 1279, 1280, 2559, 2560, 65535)
P_NARROW = (1, 2, 511, 512, 1023)
P_COUNTS = (1, 255, 256, 1279, 1280, 2559, 2560, 65535, 65536, 100000)
M_TOTALS = (1, 511, 512, 513, 1030)         # around the 512-column tile of k_counts_finalize
THRESHOLDS = (0.05, 0.1)
# four ragged slabs in a matrix of 1037 columns: not in slab order, columns 518-520 and 1033-1036 covered by nobody
SLAB_COLS, OUT_COL0, M_SLABS = (0, 1, 511, 518), (1037, 521, 522, 0), 1037
SLAB_SRC0 = (0, 0, 1, 512)                  # the slab's columns of the designed [N, 1030] matrices
SLACK_COLS = 2                              # poisoned columns behind every slab (slab_stride is larger than the slab)
SENTINEL = -7.0
SWITCHES = ('SAFE_HIP_FORCE_PATH', 'SAFE_HIP_NARROW_LDS', 'SAFE_HIP_COUNTS', 'SAFE_HIP_HYPER_TABLE', 'SAFE_HIP_MFMA_Z',
            'SAFE_HIP_HYP_SPLIT', 'SAFE_HIP_XCHG_TAIL')
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(cr.NAMES, k)]


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


def _data(kind, m, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(N, m)) < 0.3).astype(np.float64) if kind == 'binary' else rng.normal(size=(N, m))


def _membership():
    """A random membership with every node in its own neighborhood: no two neighborhoods are the same set (two rows with
    one neighborhood have the same counters in every column and could not be told apart)."""
    a = ((np.random.default_rng(2024).uniform(size=(N, N)) < 0.05) | np.eye(N, dtype=bool)).astype(np.int64)
    assert len({tuple(r) for r in a.tolist()}) == N
    return a


def _randomization(be, ctx, nbr, b, nperm, seed, sign='both', thr=0.05):
    """One real safe_randomization; returns its five matrices and the enriched counts."""
    n, m = b.shape
    attr = be.Attributes.from_host(ctx, b)
    perms = be.Permutations(ctx, n, attr.row_flags(), nperm, seed)
    outs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
    try:
        be.randomization(ctx, nbr, attr, perms, 'sum', sign, thr, [o.ptr for o in outs])
        ctx.sync()
        return [o.download((n, m)) for o in outs[:5]] + [outs[5].download((m,))]
    finally:
        for o in outs:
            o.free()
        perms.close()
        attr.close()


def _exported(be, ctx):
    """The u32 counters [m, n_pad] the last call left, with (n_pad, layout)."""
    n_pad, m, layout = be.packed_counts_info(ctx)
    buf = ctx.alloc(4 * n_pad * m)
    try:
        be.export_packed_counts(ctx, buf.ptr, n_pad * m)
        ctx.sync()
        return buf.download((m, n_pad), np.uint32), n_pad, layout
    finally:
        buf.free()


def _recover_map(be, ctx, nbr, kind, layout):
    """pos_of_row [N] of a layout, independent of the consumers: the counters safe_randomization left, position by position,
    against the counts safe_permtest_counts gives row by row for the same handles -- all columns of a row together are the
    key (seeds fixed so that the keys are distinct and no padding position repeats one)."""
    nperm, seed, m = 20, 31, 40
    b = _data(kind, m, 77)
    _randomization(be, ctx, nbr, b, nperm, seed)
    slab, n_pad, got_layout = _exported(be, ctx)
    assert got_layout == layout and slab.shape == (m, n_pad)
    attr = be.Attributes.from_host(ctx, b)
    perms = be.Permutations(ctx, N, attr.row_flags(), nperm, seed)
    bufs = [ctx.alloc_f64(N, m) for _ in range(3)]
    be.permtest_counts(ctx, nbr, attr, perms, 'sum', *[x.ptr for x in bufs])
    ctx.sync()
    cn, cp = bufs[1].download((N, m)), bufs[2].download((N, m))
    for x in bufs:
        x.free()
    perms.close()
    attr.close()
    keys = ((nperm - cp).astype(np.uint32) << np.uint32(16)) | (nperm - cn).astype(np.uint32)      # #less << 16 | #greater
    row_of_key = {tuple(k): r for r, k in enumerate(keys.tolist())}
    assert len(row_of_key) == N, 'the rows of this seed are not distinguishable by their counters'
    pos_of_row = np.full(N, -1, dtype=np.int64)
    padding = 0
    for pos in range(n_pad):
        r = row_of_key.get(tuple(slab[:, pos].tolist()))
        if r is None:
            padding += 1
        else:
            assert pos_of_row[r] < 0, 'two positions hold the counters of row %d' % r
            pos_of_row[r] = pos
    # an injection of the N rows into n_pad positions, every other position padding
    assert (pos_of_row >= 0).all() and len(set(pos_of_row.tolist())) == N and padding == n_pad - N
    return n_pad, pos_of_row


@pytest.fixture(scope='module')
def world(amd, ctx):
    """The membership handle with both counter layouts built, their recovered row maps and the output buffers."""
    from safepy_amd import backend as be
    nbr = be.Neighborhoods.from_dense(ctx, _membership())
    mp = pytest.MonkeyPatch()
    maps = {}
    try:
        for var in SWITCHES:
            mp.delenv(var, raising=False)
        for layout, kind, force in ((0, 'binary', 'bits'), (1, 'quantitative', 'mfma')):      # (tests/test_gpu_routes.py)
            mp.setenv('SAFE_HIP_FORCE_PATH', force)
            maps[layout] = _recover_map(be, ctx, nbr, kind, layout)
    finally:
        mp.undo()
    w = World(be, amd, ctx, nbr, maps)
    yield w
    for b in w.out + [w.slab]:
        b.free()
    nbr.close()


class World:
    def __init__(self, be, amd, ctx, nbr, maps):
        self.be, self.lib, self.E_INVALID, self.ctx, self.nbr, self.maps = be, amd._lib.lib, amd._lib.E_INVALID, ctx, nbr, maps
        self.sign = {'highest': amd._lib.SIGN_HIGHEST, 'lowest': amd._lib.SIGN_LOWEST, 'both': amd._lib.SIGN_BOTH}
        self.out = [ctx.alloc_f64(N, M_SLABS) for _ in range(4)]
        self.slab_words = len(SLAB_COLS) * (max(SLAB_COLS) + SLACK_COLS) * 256
        self.slab = ctx.alloc(4 * self.slab_words)
        self.designs = {}

    def design(self, P):
        """less, greater [N, 1030] of a permutation count, with the reference outputs of every sign and threshold: computed
        once, shared, never modified (the parity of a row's position differs between the layouts: one design per layout)."""
        if P not in self.designs:
            self.designs.clear()                                           # (one at a time: 40 MB each)
            d = {}
            for layout, (n_pad, pos) in self.maps.items():
                less, greater = cr.designed_matrix(P, N, max(M_TOTALS), pos & 1, np.random.default_rng(1000 * P + layout))
                for a in (less, greater):
                    a.flags.writeable = False
                want = {(s, t): cr.outputs_from_pairs(less, greater, P, s, t) for s in cr.SIGNS for t in THRESHOLDS}
                d[layout] = (less, greater, want)
            self.designs[P] = d
        return self.designs[P]

    def prefill(self, m):
        sentinel = np.full((N, m), SENTINEL)
        for b in self.out:
            b.upload(sentinel)

    def ptrs(self, subset):
        return [C.c_void_p(b.ptr) if k in subset else None for k, b in zip(cr.NAMES, self.out)]

    def results(self, m):
        self.ctx.sync()
        return {k: b.download((N, m)) for k, b in zip(cr.NAMES, self.out)}

    @staticmethod
    def table_ptr(table):
        return C.c_void_p(table.ctypes.data) if table is not None else None

    # the three consumers, called through the ABI itself (return code, and NULL for the NES table where a case wants it)
    def packed_counts(self, layout, n_pad, m, P, sign, thr, subset, table):
        return self.lib.safe_outputs_from_packed_counts(self.ctx.handle, self.nbr.handle, C.c_void_p(self.slab.ptr), layout, n_pad, m, P,
                                                        self.sign[sign], thr, self.table_ptr(table), *self.ptrs(subset))

    def nes_from_packed(self, layout, n_pad, m, P, sign, table, want_nes=True):
        return self.lib.safe_nes_from_packed_counts(self.ctx.handle, self.nbr.handle, C.c_void_p(self.slab.ptr), layout, n_pad, m, P,
                                                    self.sign[sign], self.table_ptr(table), self.ptrs(('nes',) if want_nes else ())[2])

    def packed_slabs(self, layout, n_pad, stride, cols, col0, m_total, P, sign, thr, subset, table):
        k = len(cols)
        return self.lib.safe_outputs_from_packed_slabs(self.ctx.handle, self.nbr.handle, C.c_void_p(self.slab.ptr), layout, n_pad, k, stride,
                                                       (C.c_int64 * k)(*cols), (C.c_int64 * k)(*col0), m_total, P, self.sign[sign], thr,
                                                       self.table_ptr(table), *self.ptrs(subset), None)


def _check(got, want, m, subset, what):
    for k in cr.NAMES:
        if k in subset:
            np.testing.assert_array_equal(got[k], want[k][:, :m], err_msg='%s %s' % (what, k))
        else:
            assert (got[k] == SENTINEL).all(), '%s: %s was not requested' % (what, k)


# ---- the lists themselves -----------------------------------------------------------------------------------------------------

def test_case_lists_reach_every_variant():
    """enrich_finalize_counts keeps the NES table [P + 1] f64 in LDS while it fits 20 KiB and a k / P table behind it while
    both fit: the lists hold the last P of each variant and the first of the next, and the packed forms' largest P."""
    lds = 20 * 1024
    assert 2 * (1279 + 1) * 8 <= lds < 2 * (1280 + 1) * 8 and (2559 + 1) * 8 <= lds < (2560 + 1) * 8
    assert {1279, 1280, 2559, 2560, 65535} <= set(P_U32) and {1279, 1280, 2559, 2560, 65535} <= set(P_COUNTS)
    assert {511, 512, 1023} <= set(P_NARROW) and max(P_NARROW) == 1023 and 1024 in P_U32
    assert {511, 512, 513} <= set(M_TOTALS) and max(M_TOTALS) > 2 * 512
    assert sum(SLAB_COLS) == max(M_TOTALS) and 0 in SLAB_COLS and list(OUT_COL0) != sorted(OUT_COL0)
    covered = np.zeros(M_SLABS, dtype=int)
    for c, c0 in zip(SLAB_COLS, OUT_COL0):
        covered[c0:c0 + c] += 1
    assert covered.max() == 1 and (covered == 0).sum() == M_SLABS - sum(SLAB_COLS) > 0


@pytest.mark.parametrize('layout', [0, 1])
def test_row_map_is_an_injection_with_poisonable_padding(world, layout):
    n_pad, pos = world.maps[layout]
    assert n_pad == 256 and n_pad - N == 56
    assert pos.shape == (N,) and len(np.unique(pos)) == N and pos.min() >= 0 and pos.max() < n_pad
    slab = cr.slab_u32(np.zeros((N, 2), dtype=np.int64), np.zeros((N, 2), dtype=np.int64), pos, n_pad).reshape(2, n_pad)
    assert (slab == 0xFFFFFFFF).sum() == 2 * 56 and (slab[:, pos] == 0).all()
    assert 0 < (pos & 1).sum() < N                                           # rows at even and at odd positions


# ---- designed counters, u32 form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', P_U32)
def test_outputs_and_nes_from_packed_counts(world, P):
    """safe_outputs_from_packed_counts and safe_nes_from_packed_counts: both layouts x five widths x three signs x two
    thresholds, bit-equal to the restated reference; padding positions hold 0xFFFFFFFF."""
    w = world
    table = cr.nes_table(P)
    for layout, (n_pad, pos) in w.maps.items():
        less, greater, want = w.design(P)[layout]
        dl, dg = cr.designed_pairs(P)
        assert set(zip(dl.tolist(), dg.tolist())) <= set(zip(less[:, :4].ravel().tolist(), greater[:, :4].ravel().tolist()))
        w.slab.upload(cr.slab_u32(less, greater, pos, n_pad))              # a narrower matrix is a prefix of the slab
        for m in M_TOTALS:
            for sign, thr in itertools.product(cr.SIGNS, THRESHOLDS):
                what = 'P=%d layout=%d m=%d %s %g' % (P, layout, m, sign, thr)
                w.prefill(m)
                assert w.packed_counts(layout, n_pad, m, P, sign, thr, cr.NAMES, table) == 0, what
                _check(w.results(m), want[sign, thr], m, cr.NAMES, what)
            for sign in cr.SIGNS:
                w.prefill(m)
                assert w.nes_from_packed(layout, n_pad, m, P, sign, table) == 0
                _check(w.results(m), want[sign, 0.05], m, ('nes',), 'nes P=%d layout=%d m=%d %s' % (P, layout, m, sign))


def _fill_slabs(w, less, greater, pos, n_pad, narrow):
    """The four slabs of SLAB_COLS in one buffer whose every other word -- slack behind each slab, padding positions --
    is 0xFFFFFFFF (all-ones pairs in the narrow form); returns (stride, the packed words of the real columns)."""
    stride = (max(SLAB_COLS) + SLACK_COLS) * n_pad
    host = np.full(len(SLAB_COLS) * stride, 0xFFFFFFFF, dtype=np.uint32)
    packed = []
    for r, (c, s0) in enumerate(zip(SLAB_COLS, SLAB_SRC0)):
        words = cr.slab_u32(less[:, s0:s0 + c], greater[:, s0:s0 + c], pos, n_pad, poison=0x03FF03FF if narrow else 0xFFFFFFFF)
        if narrow:
            words = cr.pack20(words, n_pad, c)
            np.testing.assert_array_equal(cr.unpack20(words, n_pad, c).reshape(c, n_pad)[:, pos] >> 16, less[:, s0:s0 + c].T)
            packed.append(words)
        assert len(words) + n_pad <= stride                                # at least one whole poisoned column behind it
        host[r * stride:r * stride + len(words)] = words
    assert host.nbytes <= w.slab.nbytes
    w.slab.upload(host)
    return stride, packed


def _slab_want(want):
    full = {k: np.full((N, M_SLABS), SENTINEL) for k in cr.NAMES}
    for c, c0, s0 in zip(SLAB_COLS, OUT_COL0, SLAB_SRC0):
        for k in cr.NAMES:
            full[k][:, c0:c0 + c] = want[k][:, s0:s0 + c]
    return full


@pytest.mark.parametrize('P', P_U32)
def test_outputs_from_packed_slabs_u32(world, P):
    """Four ragged slabs (0, 1, 511 and 518 columns) written out of slab order into a [N, 1037] matrix: the covered columns
    equal the reference, the seven uncovered ones keep the sentinel, the poisoned slack behind each slab is never used."""
    w = world
    table = cr.nes_table(P)
    for layout, (n_pad, pos) in w.maps.items():
        less, greater, want = w.design(P)[layout]
        stride, _ = _fill_slabs(w, less, greater, pos, n_pad, False)
        for sign, thr in itertools.product(cr.SIGNS, THRESHOLDS):
            what = 'slabs P=%d layout=%d %s %g' % (P, layout, sign, thr)
            w.prefill(M_SLABS)
            assert w.packed_slabs(layout, n_pad, stride, SLAB_COLS, OUT_COL0, M_SLABS, P, sign, thr, cr.NAMES, table) == 0, what
            _check(w.results(M_SLABS), _slab_want(want[sign, thr]), M_SLABS, cr.NAMES, what)


# ---- designed counters, 20-bit form ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', P_NARROW)
def test_outputs_from_packed_slabs_narrow(world, P):
    """The same slabs as 20-bit pairs (SAFE_PACKED_NARROW).  From P = 512 on bit 9 of both fields -- bit 39 of a 40-bit
    group, the top bit of the side byte, for #less at an odd position -- is set at even and at odd positions, and every
    bit of the side byte is 1 in one group of two real rows and 0 in another (asserted here, on the words uploaded)."""
    w = world
    table = cr.nes_table(P)
    for layout, (n_pad, pos) in w.maps.items():
        less, greater, want = w.design(P)[layout]
        stride, packed = _fill_slabs(w, less, greater, pos, n_pad, True)
        if P >= 512:
            for field in (less, greater):
                for parity in (0, 1):
                    assert (field[(pos & 1) == parity] & 512).any(), 'bit 9 never set at parity %d' % parity
            real = np.zeros(n_pad, dtype=bool)
            real[pos] = True
            both_real = real[0::2] & real[1::2]
            side = np.concatenate([np.ascontiguousarray(words.reshape(c, -1)[:, n_pad // 2:]).astype('<u4').view(np.uint8)
                                   .reshape(c, n_pad // 2)[:, both_real].ravel() for words, c in zip(packed, SLAB_COLS) if c])
            for bit in range(8):
                assert ((side >> bit) & 1).any() and not ((side >> bit) & 1).all(), 'side byte bit %d' % bit
        for sign, thr in itertools.product(cr.SIGNS, THRESHOLDS):
            what = 'narrow slabs P=%d layout=%d %s %g' % (P, layout, sign, thr)
            w.prefill(M_SLABS)
            rc = w.packed_slabs(layout | w.be.PACKED_NARROW, n_pad, stride, SLAB_COLS, OUT_COL0, M_SLABS, P, sign, thr, cr.NAMES, table)
            assert rc == 0, what
            _check(w.results(M_SLABS), _slab_want(want[sign, thr]), M_SLABS, cr.NAMES, what)


def test_narrow_form_ends_at_1023_permutations(world):
    """P = 1024 with the narrow flag: SAFE_E_INVALID, nothing written, and the context goes on working."""
    w = world
    n_pad, pos = w.maps[0]
    less, greater, want = w.design(1023)[0]
    stride, _ = _fill_slabs(w, less, greater, pos, n_pad, True)
    w.prefill(M_SLABS)
    args = (n_pad, stride, SLAB_COLS, OUT_COL0, M_SLABS)
    assert w.packed_slabs(w.be.PACKED_NARROW, *args, 1024, 'both', 0.05, cr.NAMES, cr.nes_table(1024)) == w.E_INVALID
    _check(w.results(M_SLABS), None, M_SLABS, (), 'refused')
    assert w.packed_slabs(w.be.PACKED_NARROW, *args, 1023, 'both', 0.05, cr.NAMES, cr.nes_table(1023)) == 0
    _check(w.results(M_SLABS), _slab_want(want['both', 0.05]), M_SLABS, cr.NAMES, 'after the refusal')


# ---- subsets of the outputs, the library's own table, refusals ------------------------------------------------------------------

@pytest.mark.parametrize('entry', ['counts', 'slabs', 'slabs-narrow'])
def test_every_subset_of_the_outputs(world, entry):
    """Each of the fifteen non-empty subsets: the requested matrices equal the reference, a NULL output is skipped."""
    w = world
    P, layout, sign, thr = (1023, 1, 'both', 0.1) if entry == 'slabs-narrow' else (1280, 0, 'lowest', 0.05)
    n_pad, pos = w.maps[layout]
    less, greater, want = w.design(P)[layout]
    table = cr.nes_table(P)
    if entry == 'counts':
        m = 513
        w.slab.upload(cr.slab_u32(less, greater, pos, n_pad))
        full = want[sign, thr]
    else:
        m = M_SLABS
        stride, _ = _fill_slabs(w, less, greater, pos, n_pad, entry == 'slabs-narrow')
        full = _slab_want(want[sign, thr])
    assert len(SUBSETS) == 15
    for subset in SUBSETS:
        w.prefill(m)
        if entry == 'counts':
            rc = w.packed_counts(layout, n_pad, m, P, sign, thr, subset, table)
        else:
            flag = w.be.PACKED_NARROW if entry == 'slabs-narrow' else 0
            rc = w.packed_slabs(layout | flag, n_pad, stride, SLAB_COLS, OUT_COL0, m, P, sign, thr, subset, table)
        assert rc == 0, subset
        _check(w.results(m), full, m, subset, '%s %s' % (entry, '+'.join(subset)))


@pytest.mark.parametrize('entry', ['counts', 'nes', 'slabs', 'slabs-narrow'])
def test_library_table_when_none_is_given(world, entry):
    """nes_table_host = NULL: the library evaluates -log10(k / P) with its own libm.  P-values do not depend on it and are
    exact.  A libm log10 is good to an ulp, 2^-53 ~ 1.1e-16 relative, in the library's table and in NumPy's alike, so a
    table entry -- the NES of 'highest' and 'lowest' -- differs by at most 2.2e-16 relative: rtol = 1e-12 leaves almost
    four orders of magnitude.  'both' subtracts two entries; equal counts give exactly 0 on both sides, and the closest
    unequal ones at these P (k and k + 1 around P / 2) differ by 0.434 / 640 = 6.8e-4 with an absolute error of at most
    2 * 2.2e-16 * 0.3: 2e-13 relative, still inside.  (At P = 65 535 that cancellation could reach 5e-12, which is why
    this case runs at P = 1279 and 1023.)  nes_binary can differ from the reference only where |NES| is within that error
    of -log10(threshold), i.e. k / P == threshold: P = 1279 is prime, 1023 = 3 * 11 * 31, neither has such a count
    (asserted), so nes_binary is exact too."""
    w = world
    P, layout, sign, thr = (1023, 0, 'both', 0.05) if entry == 'slabs-narrow' else (1279, 1, 'both', 0.1)
    assert all(abs(k / P - t) > 1e-6 for k in range(P + 1) for t in THRESHOLDS)
    n_pad, pos = w.maps[layout]
    less, greater, want = w.design(P)[layout]
    if entry in ('counts', 'nes'):
        m, subset = 1030, cr.NAMES if entry == 'counts' else ('nes',)
        w.slab.upload(cr.slab_u32(less, greater, pos, n_pad))
        w.prefill(m)
        rc = w.packed_counts(layout, n_pad, m, P, sign, thr, subset, None) if entry == 'counts' else w.nes_from_packed(layout, n_pad, m, P, sign, None)
        full = want[sign, thr]
    else:
        m, subset = M_SLABS, cr.NAMES
        stride, _ = _fill_slabs(w, less, greater, pos, n_pad, entry == 'slabs-narrow')
        w.prefill(m)
        flag = w.be.PACKED_NARROW if entry == 'slabs-narrow' else 0
        rc = w.packed_slabs(layout | flag, n_pad, stride, SLAB_COLS, OUT_COL0, m, P, sign, thr, subset, None)
        full = _slab_want(want[sign, thr])
    assert rc == 0
    got = w.results(m)
    for k in subset:
        if k == 'nes':
            np.testing.assert_allclose(got[k], full[k][:, :m], rtol=1e-12, err_msg=entry)
        else:
            np.testing.assert_array_equal(got[k], full[k][:, :m], err_msg='%s %s' % (entry, k))
    if entry == 'slabs':                               # the table the context keeps between slab calls follows the argument
        w.prefill(m)
        assert w.packed_slabs(layout, n_pad, stride, SLAB_COLS, OUT_COL0, m, P, sign, thr, subset, cr.nes_table(P)) == 0
        _check(w.results(m), full, m, subset, 'the caller\'s table after the library\'s')


def test_refusals_leave_the_outputs_alone(world):
    """Every argument check of the three packed entry points: SAFE_E_INVALID, the outputs keep their sentinel."""
    w = world
    P, m = 20, 3
    n_pad, pos = w.maps[0]
    less, greater, want = w.design(P)[0]
    w.slab.upload(cr.slab_u32(less[:, :m], greater[:, :m], pos, n_pad))
    table = cr.nes_table(65536)                       # (long enough for whatever count a call names)
    narrow = w.be.PACKED_NARROW
    slabs = (n_pad, m * n_pad, (m,), (0,), m)         # n_pad, stride, cols, col0, m_total of one slab that fits exactly
    bad = [
        ('counts: no output', lambda: w.packed_counts(0, n_pad, m, P, 'both', 0.05, (), table)),
        ('nes: no output', lambda: w.nes_from_packed(0, n_pad, m, P, 'both', table, want_nes=False)),
        ('slabs: no output', lambda: w.packed_slabs(0, *slabs, P, 'both', 0.05, (), table)),
        ('counts: layout 2', lambda: w.packed_counts(2, n_pad, m, P, 'both', 0.05, cr.NAMES, table)),
        ('counts: layout -1', lambda: w.packed_counts(-1, n_pad, m, P, 'both', 0.05, cr.NAMES, table)),
        ('counts: the narrow flag', lambda: w.packed_counts(narrow, n_pad, m, P, 'both', 0.05, cr.NAMES, table)),
        ('nes: layout 2', lambda: w.nes_from_packed(2, n_pad, m, P, 'both', table)),
        ('slabs: layout 2', lambda: w.packed_slabs(2, *slabs, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: layout 2, narrow', lambda: w.packed_slabs(2 | narrow, *slabs, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: layout -1', lambda: w.packed_slabs(-1, *slabs, P, 'both', 0.05, cr.NAMES, table)),
    ]
    for wrong in (n_pad - 16, n_pad + 16, n_pad // 2, 0):
        bad += [('counts: n_pad %d' % wrong, lambda v=wrong: w.packed_counts(0, v, m, P, 'both', 0.05, cr.NAMES, table)),
                ('nes: n_pad %d' % wrong, lambda v=wrong: w.nes_from_packed(0, v, m, P, 'both', table)),
                ('slabs: n_pad %d' % wrong, lambda v=wrong: w.packed_slabs(0, v, *slabs[1:], P, 'both', 0.05, cr.NAMES, table))]
    for count in (0, 65536):
        bad += [('counts: P = %d' % count, lambda v=count: w.packed_counts(0, n_pad, m, v, 'both', 0.05, cr.NAMES, table)),
                ('nes: P = %d' % count, lambda v=count: w.nes_from_packed(0, n_pad, m, v, 'both', table)),
                ('slabs: P = %d' % count, lambda v=count: w.packed_slabs(0, *slabs, v, 'both', 0.05, cr.NAMES, table))]
    bad += [
        ('slabs: stride one word short', lambda: w.packed_slabs(0, n_pad, m * n_pad - 1, (m,), (0,), m, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: second slab wider than the stride', lambda: w.packed_slabs(0, n_pad, n_pad, (1, 2), (0, 1), m, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: narrow stride one word short',
         lambda: w.packed_slabs(narrow, n_pad, m * (n_pad // 8 * 5) - 1, (m,), (0,), m, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: past the last column', lambda: w.packed_slabs(0, n_pad, m * n_pad, (m,), (1,), m, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: second slab past the last column', lambda: w.packed_slabs(0, n_pad, 2 * n_pad, (1, 2), (0, 2), m, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: negative column', lambda: w.packed_slabs(0, n_pad, m * n_pad, (m,), (-1,), m + 1, P, 'both', 0.05, cr.NAMES, table)),
        ('slabs: negative width', lambda: w.packed_slabs(0, n_pad, m * n_pad, (-1,), (0,), m, P, 'both', 0.05, cr.NAMES, table)),
    ]
    w.prefill(m + 1)
    for what, call in bad:
        assert call() == w.E_INVALID, what
        _check(w.results(m + 1), None, m + 1, (), what)
    # the calls the refusals were variations of are accepted, and the context has taken no harm
    w.prefill(m)
    assert w.packed_counts(0, n_pad, m, P, 'both', 0.05, cr.NAMES, cr.nes_table(P)) == 0
    _check(w.results(m), want['both', 0.05], m, cr.NAMES, 'counts after the refusals')
    w.prefill(m)
    assert w.packed_slabs(0, *slabs, P, 'both', 0.05, cr.NAMES, cr.nes_table(P)) == 0
    _check(w.results(m), want['both', 0.05], m, cr.NAMES, 'slabs after the refusals')
    w.prefill(m)
    assert w.nes_from_packed(0, n_pad, m, P, 'both', cr.nes_table(P)) == 0
    _check(w.results(m), want['both', 0.05], m, ('nes',), 'nes after the refusals')


def _want_from_table(less, greater, P, sign, thr, table):
    """outputs_from_pairs with the NES looked up in `table` (the nes_table_host of a call) instead of evaluated: what the
    consumers do with a table that is not -log10(k / P)."""
    want = dict(cr.outputs_from_pairs(less, greater, P, sign, thr))
    ep, en = table[P - less], table[P - greater]
    want['nes'] = {'highest': ep, 'lowest': en, 'both': ep - en}[sign]
    want['nes_binary'] = (np.abs(want['nes']) > -np.log10(thr)).astype(np.float64)
    return want


def test_the_nes_table_follows_the_call_across_entry_points(world, monkeypatch):
    """One context keeps ONE NES table on the device for all its entry points and uploads it only when a call names another.
    Six calls in a row, each with another permutation count or table than the call before it -- slabs P = 37, packed counts
    P = 1000, f64 counts P = 37, a real safe_randomization P = 1000, slabs P = 37 again, slabs P = 37 with a table that
    differs in one entry -- each bit-equal to the reference for ITS count and table: the table of the call before never
    shows through.  70 columns: more than one 64-column word group; the membership spans more than one 64-row slice."""
    w, be, ctx = world, world.be, world.ctx
    layout, sign, thr, m = 0, 'both', 0.05, 70
    n_pad, pos = w.maps[layout]
    assert n_pad > 64 and m > 64
    tables = {P: cr.nes_table(P) for P in (37, 1000)}
    design = {}
    for P in (37, 1000):
        less, greater = cr.designed_matrix(P, N, m, pos & 1, np.random.default_rng(50 + P))
        design[P] = (less, greater, cr.outputs_from_pairs(less, greater, P, sign, thr))
        lookup = _want_from_table(less, greater, P, sign, thr, tables[P])     # (the look-up restatement is the evaluated one)
        for k in cr.NAMES:
            np.testing.assert_array_equal(lookup[k], design[P][2][k], err_msg='table look-up, P=%d %s' % (P, k))
    one_slab = (n_pad, m * n_pad, (m,), (0,), m)

    def slabs(P, table, want, what):
        less, greater, _ = design[P]
        w.slab.upload(cr.slab_u32(less, greater, pos, n_pad))
        w.prefill(m)
        assert w.packed_slabs(layout, *one_slab, P, sign, thr, cr.NAMES, table) == 0, what
        _check(w.results(m), want, m, cr.NAMES, what)

    # 1. slabs, P = 37
    slabs(37, tables[37], design[37][2], '1: slabs P=37')
    # 2. packed counts, P = 1000
    less, greater, want = design[1000]
    w.slab.upload(cr.slab_u32(less, greater, pos, n_pad))
    w.prefill(m)
    assert w.packed_counts(layout, n_pad, m, 1000, sign, thr, cr.NAMES, tables[1000]) == 0
    _check(w.results(m), want, m, cr.NAMES, '2: packed counts P=1000')
    # 3. f64 counts, P = 37 (no NaN scores: the same four matrices, and the column sums of nes_binary)
    less, greater, want = design[37]
    d = [ctx.alloc_f64(N, m) for _ in range(3)] + [ctx.alloc_f64(m)]
    try:
        for x, host in zip(d, ((37 - greater).astype(np.float64), (37 - less).astype(np.float64), np.zeros((N, m)))):
            x.upload(host)
        d[3].upload(np.full(m, SENTINEL))
        w.prefill(m)
        rc = w.lib.safe_outputs_from_counts(ctx.handle, N, m, 37, w.sign[sign], thr, w.table_ptr(tables[37]),
                                            *[C.c_void_p(x.ptr) for x in d[:3]], *w.ptrs(cr.NAMES), C.c_void_p(d[3].ptr))
        assert rc == 0
        _check(w.results(m), want, m, cr.NAMES, '3: f64 counts P=37')
        np.testing.assert_array_equal(d[3].download((m,)), want['nes_binary'].sum(axis=0), err_msg='3: num_enriched')
    finally:
        for x in d:
            x.free()
    # 4. a real safe_randomization on the bit-sliced kernel, P = 1000: its matrices against the counters it leaves
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'bits')
    ns, pn, pp, nes, nb, ne = _randomization(be, ctx, w.nbr, _data('binary', 40, 5), 1000, 3, sign, thr)
    left, left_pad, left_layout = _exported(be, ctx)
    assert (left_layout, left_pad) == (layout, n_pad) and not np.isnan(ns).any()
    less, greater = (left[:, pos] >> 16).T.astype(np.int64), (left[:, pos] & 0xFFFF).T.astype(np.int64)
    assert (less + greater <= 1000).all() and (less + greater).max() > 37          # (counts a table of 38 entries cannot serve)
    want = cr.outputs_from_pairs(less, greater, 1000, sign, thr)
    for k, got in zip(cr.NAMES, (pn, pp, nes, nb)):
        np.testing.assert_array_equal(got, want[k], err_msg='4: randomization P=1000 %s' % k)
    np.testing.assert_array_equal(ne, want['nes_binary'].sum(axis=0), err_msg='4: num_enriched')
    # 5. slabs again, P = 37
    slabs(37, tables[37], design[37][2], '5: slabs P=37 after P=1000')
    # 6. ... and once more with a table of the same length that differs in ONE entry, one the counters use
    less, greater, want5 = design[37]
    other = tables[37].copy()
    other[37] = 0.25                                                           # (count 37 of 37: the pair (0, 0) is designed in)
    assert ((37 - less) == 37).any() and (other != tables[37]).sum() == 1
    want6 = _want_from_table(less, greater, 37, sign, thr, other)
    assert not np.array_equal(want6['nes'], want5['nes'])
    slabs(37, other, want6, '6: slabs P=37, another table')


# ---- f64 counts (k_counts_to_outputs) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', P_COUNTS)
def test_outputs_from_f64_counts(world, P):
    """safe_outputs_from_counts on the designed pairs as f64 counts, [37, 513], up to P = 100 000 (no 16-bit limit here):
    bit-equal; NaN observed scores (one row, isolated cells) give NaN p-values and NES and nes_binary 0; num_enriched is
    the column sum of nes_binary.  At P = 1279 one more call takes the library's own table (nes_table_host = NULL;
    tolerance and the choice of P: test_library_table_when_none_is_given)."""
    w, be, ctx = world, world.be, world.ctx
    n, m = 37, 513
    less, greater = cr.designed_matrix(P, n, m, np.arange(n) & 1, np.random.default_rng(P))
    ns = np.zeros((n, m))
    ns[5, :] = np.nan
    for cell in ((0, 0), (36, 512), (17, 256), (4, 100), (6, 100)):
        ns[cell] = np.nan
    nan = np.isnan(ns)
    counts_neg = np.where(nan, np.nan, (P - greater).astype(np.float64))
    counts_pos = np.where(nan, np.nan, (P - less).astype(np.float64))
    d = [ctx.alloc_f64(n, m) for _ in range(7)] + [ctx.alloc_f64(m)]
    try:
        for x, host in zip(d, (counts_neg, counts_pos, ns)):
            x.upload(host)
        for sign, thr in itertools.product(cr.SIGNS, THRESHOLDS):
            want = cr.outputs_from_pairs(less, greater, P, sign, thr)
            for k in ('pvalues_neg', 'pvalues_pos', 'nes'):
                want[k][nan] = np.nan
            want['nes_binary'][nan] = 0.0
            tables = [cr.nes_table(P)]
            if P == 1279 and (sign, thr) == ('both', 0.05):
                tables.append(None)
            for table in tables:
                for x in d[3:7]:
                    x.upload(np.full((n, m), SENTINEL))
                d[7].upload(np.full(m, SENTINEL))
                rc = w.lib.safe_outputs_from_counts(ctx.handle, n, m, P, w.sign[sign], thr, w.table_ptr(table), *[C.c_void_p(x.ptr) for x in d])
                assert rc == 0
                ctx.sync()
                got = {k: x.download((n, m)) for k, x in zip(cr.NAMES, d[3:7])}
                what = 'P=%d %s %g table=%s' % (P, sign, thr, 'given' if table is not None else 'NULL')
                for k in cr.NAMES:
                    if k == 'nes' and table is None:
                        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=what)
                    else:
                        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (what, k))
                assert np.isnan(got['nes'][5]).all() and (got['nes_binary'][5] == 0).all()
                np.testing.assert_array_equal(d[7].download((m,)), got['nes_binary'].sum(axis=0), err_msg=what)
                np.testing.assert_array_equal(d[7].download((m,)), want['nes_binary'].sum(axis=0), err_msg=what)
    finally:
        for x in d:
            x.free()


# ---- the export side (k_pack_counts20, chunked export) ----------------------------------------------------------------------------

def test_exported_counters_narrow_and_chunked(world, monkeypatch):
    """One real binary run at P = 1023 whose counters pass 511 in both fields: safe_export_packed_chunk_narrow == pack20 of
    safe_export_packed_counts bit for bit, whole and in two chunks of 64 + 36 columns with the rest of `capacity` zeroed
    (the u32 chunks likewise); the narrow slabs fed back through safe_outputs_from_packed_slabs give the call's matrices."""
    w, be, ctx = world, world.be, world.ctx
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    m, P, seed, sign, thr = 100, 1023, 9, 'both', 0.05
    b = _data('binary', m, 5)
    n_pad, pos = w.maps[0]
    cap_u32, cap_narrow = 128 * n_pad + 64, be.packed_slab_words(128, n_pad, True) + 64
    chunk = ctx.alloc(4 * cap_u32)
    try:
        for chunks, cols in ((1, 128), (2, 64)):
            be.set_exchange_chunks(ctx, chunks, cols)
            ran = _randomization(be, ctx, w.nbr, b, P, seed, sign, thr)
            whole, got_pad, layout = _exported(be, ctx)
            assert (got_pad, layout, whole.shape) == (n_pad, 0, (m, n_pad))
            real = whole[:, pos]
            assert (real >> 16).max() >= 512 and (real & 0xFFFF).max() >= 512 and max((real >> 16).max(), (real & 0xFFFF).max()) <= P
            assert ((whole >> 16) <= 1023).all() and ((whole & 0xFFFF) <= 1023).all()             # padding included: it is packed too
            bounds = [min(k * cols, m) for k in range(chunks)] + [m]
            assert [b1 - b0 for b0, b1 in zip(bounds, bounds[1:])] == ([100] if chunks == 1 else [64, 36])
            narrow = []
            for k, (c0, c1) in enumerate(zip(bounds, bounds[1:])):
                chunk.upload(np.full(cap_u32, 0xA5A5A5A5, dtype=np.uint32))
                be.export_packed_chunk(ctx, k, chunk.ptr, cap_u32)
                ctx.sync()
                got = chunk.download((cap_u32,), np.uint32)
                np.testing.assert_array_equal(got[:(c1 - c0) * n_pad], whole[c0:c1].ravel())
                assert not got[(c1 - c0) * n_pad:].any()
                chunk.upload(np.full(cap_u32, 0xA5A5A5A5, dtype=np.uint32))
                be.export_packed_chunk(ctx, k, chunk.ptr, cap_narrow, narrow=True)
                ctx.sync()
                got = chunk.download((cap_u32,), np.uint32)
                words = be.packed_slab_words(c1 - c0, n_pad, True)
                np.testing.assert_array_equal(got[:words], cr.pack20(whole[c0:c1].ravel(), n_pad, c1 - c0))
                assert not got[words:cap_narrow].any() and (got[cap_narrow:] == 0xA5A5A5A5).all()
                narrow.append(got[:cap_narrow])
            # the chunks as the slabs of an exchange: stride = the capacity, the zeroed rest is the slack
            w.slab.upload(np.concatenate(narrow))
            w.prefill(m)
            widths = [b1 - b0 for b0, b1 in zip(bounds, bounds[1:])]
            rc = w.packed_slabs(be.PACKED_NARROW, n_pad, cap_narrow, widths, bounds[:-1], m, P, sign, thr, cr.NAMES, cr.nes_table(P))
            assert rc == 0
            _check(w.results(m), dict(zip(cr.NAMES, ran[1:5])), m, cr.NAMES, '%d chunks' % chunks)
            # ... and the call's matrices are the reference's for its own counters
            ref = cr.outputs_from_pairs((real >> 16).T, (real & 0xFFFF).T, P, sign, thr)
            for k, x in zip(cr.NAMES, ran[1:5]):
                np.testing.assert_array_equal(x, ref[k], err_msg=k)
            np.testing.assert_array_equal(ran[5], ref['nes_binary'].sum(axis=0))
    finally:
        be.set_exchange_chunks(ctx, 0)
        chunk.free()
    assert be.packed_chunk_info(ctx)[0] == 0


# ---- the fused call at the table edges ----------------------------------------------------------------------------------------

def _fused(amd, xy, a, b, P, seed):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, np.arange(len(xy) - 1), np.arange(1, len(xy)))
    sf.random_seed = seed
    sf.neighborhoods = a.astype(np.int64)
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='randomization', neighborhood_score_type='sum', num_permutations=P, verbose=False)
    return sf


def _assert_fused_equals_oracle(sf, want, P):
    got = {k: np.asarray(getattr(sf, k)) for k in cr.NAMES}
    for side in ('pvalues_neg', 'pvalues_pos'):
        counts, counts_want = np.rint(got[side] * P), np.rint(want[side] * P)
        np.testing.assert_array_equal(counts / P, got[side])                     # p-values ARE counts / P ...
        np.testing.assert_array_equal(counts, counts_want, err_msg='counts ' + side)  # ... of the reference's counts
    for k in cr.NAMES:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(sf.attributes['num_neighborhoods_enriched'].values, want['num_neighborhoods_enriched'])


@pytest.mark.parametrize('P', [1279, 1280, 2559, 2560])
def test_fused_binary_call_at_the_table_edges(amd, monkeypatch, P):
    """SAFE.compute_pvalues(how='randomization') on binary columns (the bit-sliced kernel: counters #less / #greater, the
    whole epilogue in one pass) == the oracle, exactly, on both sides of each table variant's limit."""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(P)
    n, m, seed = 150, 70, 3
    xy = rng.uniform(size=(n, 2))
    a = orc.neighborhoods_euclidean(xy, 0.12)
    b = (rng.uniform(size=(n, m)) < np.linspace(0.02, 0.5, m)).astype(np.float64)
    b[rng.choice(n, 6, replace=False)] = np.nan
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', num_permutations=P, random_seed=seed)
    sf = _fused(amd, xy, a, b, P, seed)
    assert amd.Context.default(0).last_kernel()[0].startswith('k_permtest_bits')
    _assert_fused_equals_oracle(sf, want, P)


def test_fused_quantitative_call_at_1280(amd, monkeypatch):
    """The same for quantitative columns on the LDS-resident f64 kernel (tests/test_gpu_parity.py, test_gpu_golden2.py hold
    it to the oracle exactly): its counters are #>= / #<= and NaN observed scores matter -- the direct form of the epilogue,
    here with the NES table in LDS and the divisions in the kernel."""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'lds')
    P, n, m, seed = 1280, 150, 70, 4
    rng = np.random.default_rng(P + 1)
    xy = rng.uniform(size=(n, 2))
    a = orc.neighborhoods_euclidean(xy, 0.12)
    b = rng.normal(size=(n, m))
    b[rng.choice(n, 6, replace=False)] = np.nan
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', num_permutations=P, random_seed=seed)
    sf = _fused(amd, xy, a, b, P, seed)
    assert amd.Context.default(0).last_kernel()[0] == 'k_permtest_lds'
    _assert_fused_equals_oracle(sf, want, P)
