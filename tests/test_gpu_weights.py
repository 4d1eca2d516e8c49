"""The distance-weighted entry points of the library (include/safe_hip.h; safepy_amd/csrc/weights.hip) against
tests/weights_ref.py.  Needs an MI355X.

Constants of weights.hip the shapes are chosen around (both sides of each):
  wave = 64 lanes            k_weights_build, k_weights_row_sums: one wave per row, 64 members per pass; 4 rows per block
  WS_STAGE = 256             members of a row that k_score_weighted stages in LDS per pass
  WS_COLS = 1024 (4 x 256)   columns of a k_score_weighted block: lane l owns columns l, l + 256, l + 512, l + 768
                             (row-contiguous storage takes the tiles and the shape of k_permtest_weighted instead)
  WM_ROW_TILE = 16, WM_COL_CHUNK = 1024   rows and columns of a k_weights_emit block (the layout of k_moments_emit)
  WP_BN = 16                 columns of a k_permtest_weighted tile; SELL-64 slices of 64 rows, widths padded to 8 members;
                             tiles are dealt to 8 queues (blockIdx % 8); one launch covers every permutation (no span constant)

W1  builders: 'uniform', 'triangular', 'epanechnikov' bit-equal to the restatement from coordinates and from kept matrices;
    'gaussian': the argument -0.5 (t t) is restated bit for bit in NumPy, the device's value is compared with mpmath's
    correctly rounded exp of it; allowed error K_exp_ref + 1 ulp (K_exp_ref: np.exp's own worst error on such arguments,
    tests/test_weights_ref_cpu.py; the one ulp is the room a different faithfully rounded exp needs).
W2  safe_score_weighted bit-equal to the ascending-order restatement.
W3  safe_moments_test_weighted.  Designed case (dyadic weights: x, W1, W2 and n_v W2 - W1 W1 are exact): the device rounds
        g = (n_v W2 - W1 W1) / (n_v (n_v - 1))   [one division]
        var = g Q;  sd = sqrt(var);  t = W1 mu;  d = x - t;  z = d / sd
    the same six operations as safe_moments_test, so |dz| <= 2^-53 (6 |z| + 2 |W1 mu| / sd) (tests/test_gpu_moments.py T2).
    Real weights: z against the exact z of the device's own ns, weights, mean and css.  With c members, sequential sums of
    non-negative terms carry (c - 1) 2^-53 (W1) and c 2^-53 (W2: a rounded square each) relative error, so A = n_v W2 carries
    (c + 1), B = W1 W1 carries (2 c - 1), and A - B is off by at most 2 c (A + B) 2^-53 plus its own rounding: with the
    condition number kappa = (A + B) / (A - B), computed exactly per row, g is off by (2 c kappa + 2) 2^-53 relative (its
    division included), sd by half of that plus var's product and the root, (c kappa + 2.5) 2^-53.  d = x - W1 mu is off by
    2^-53 |d| + c 2^-53 |W1 mu| (W1's error times mu, the product's rounding).  With the last division,
        |dz| <= 2^-53 ((c kappa + 4.5) |z| + c |W1 mu| / sd)
    to first order; the test allows twice that for the second-order terms.  No measured constant.
    p-values against mpmath at the device's z bits within 2 K_ref (moments_ref.designed_k_ref), the large side 1 - small.
W4  safe_permtest_counts_weighted: counts bit-equal to the restatement on the tables read back from the handle."""
import numpy as np
import pytest

import moments_ref as mr
import weights_ref as wr

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049)
OUTPUTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'num_enriched')
POISON = -12345.678
WORST = {'exp_ulps': 0.0, 'z_designed': 0.0, 'z_real': 0.0}


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(scope='module')
def k_exp_ref():
    return wr.k_exp_ref()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    assert np.array_equal(bits(got), bits(want)), what


def layout(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'lattice':
        side = int(np.ceil(np.sqrt(n)))
        return np.array([(i % side, i // side) for i in range(n)], dtype=np.float64)
    if kind == 'coincident':
        return rng.integers(0, max(2, int(np.ceil(np.sqrt(n / 3.0)))), size=(n, 2)).astype(np.float64)   # ~3 nodes share a place
    if kind == 'clustered':
        return rng.normal(size=(n, 2)) * 0.05 + rng.integers(0, 3, size=(n, 1))
    return rng.uniform(size=(n, 2))


def one_radius(kind, n):
    """A radius that gives the layout neighborhoods of a handful to a few hundred members."""
    return {'lattice': 1.5, 'coincident': 1.0, 'clustered': 0.05}.get(kind, float(np.sqrt(12.0 / (np.pi * max(n, 2)))))


def csr_of_handle(nbr):
    rp, col = nbr.csr()
    return rp.astype(np.int64), col.astype(np.int64)


def check_gaussian(got, arg, k_exp_ref, what):
    """The device's exp against mpmath on the distinct arguments (at most 400 of them; equal arguments must give equal bits)."""
    ua, first, inv = np.unique(arg, return_index=True, return_inverse=True)
    assert np.array_equal(bits(got), bits(got[first][inv.ravel()])), what + ': equal arguments, different weights'
    pick = np.arange(len(ua)) if len(ua) <= 400 else np.random.default_rng(len(ua)).choice(len(ua), 400, replace=False)
    worst = wr.exp_error_ulps(ua[pick], got[first][pick])
    WORST['exp_ulps'] = max(WORST['exp_ulps'], worst)
    assert worst <= k_exp_ref + 1.0, '%s: exp off by %.3f ulp, allowed %.3f' % (what, worst, k_exp_ref + 1.0)


def check_builder(nbr, d, radii, k_exp_ref, set_kind, what):
    indptr, indices = csr_of_handle(nbr)
    dist = d(indptr, indices)
    for kind in ('uniform', 'triangular', 'epanechnikov'):
        set_kind(kind, 0.5)
        same_bits(nbr.weights(), wr.member_weights(kind, dist, indptr, radii), '%s %s' % (what, kind))
    for h in (0.25, 0.5, 2.0):
        set_kind('gaussian', h)
        r = np.broadcast_to(np.asarray(radii, dtype=np.float64), (nbr.n,))[wr.rows_of(indptr)]
        check_gaussian(nbr.weights(), wr.gaussian_argument(dist, r, h), k_exp_ref, '%s gaussian h=%g' % (what, h))


# ----------------------------------------------------------------------------------------------------------------- W1 ----

@pytest.mark.parametrize('n', SIZES)
def test_weights_from_coordinates(be, ctx, k_exp_ref, n):
    kinds = ('lattice', 'random', 'coincident', 'clustered')
    for t, mode in enumerate(('one', 1, 10, n + 5)):
        if mode == n + 5 and n > 1100:
            continue                                            # (every node a member of every row: 4.2 M entries at 2049)
        xy = layout(kinds[(t + n) % 4], n, seed=n + t)
        if mode == 'one':
            radii = one_radius(kinds[(t + n) % 4], n)
            nbr = be.Neighborhoods.euclidean(ctx, xy, radii)
        else:
            radii = ctx.row_distance_select(xy, mode)
            nbr = be.Neighborhoods.euclidean_rows(ctx, xy, radii)
            if kinds[(t + n) % 4] == 'coincident' and n >= 63 and mode == 1:
                assert (radii == 0).any()                       # rows with r_i = 0: u = 0
        try:
            check_builder(nbr, lambda ip, ix: wr.euclidean_member_distances(xy, ip, ix), radii, k_exp_ref,
                          lambda kind, h: nbr.set_weights_from_xy(xy, kind, radii, h), 'n=%d mode=%s' % (n, mode))
        finally:
            nbr.close()


def graph(n, seed):
    """A ring with chords (unit hops: tied path lengths), a second component, isolated nodes."""
    rng = np.random.default_rng(seed)
    main = max(1, (2 * n) // 3)
    eu = list(range(main - 1)) + ([main - 1] if main > 2 else [])
    ev = list(range(1, main)) + ([0] if main > 2 else [])
    for _ in range(main // 8):
        u, v = rng.integers(0, main, size=2)
        if u != v:
            eu.append(int(u)), ev.append(int(v))
    second = list(range(main, min(n, main + max(0, n // 4))))
    eu += second[:-1]
    ev += second[1:]
    return np.array(eu, dtype=np.int32), np.array(ev, dtype=np.int32)


@pytest.mark.parametrize('n', SIZES)
def test_weights_from_kept_distances(be, ctx, k_exp_ref, n):
    eu, ev = graph(n, n)
    for cutoff, weighted in ((3.0, False), (2.5, True)):
        w = None if not weighted else 0.5 + (np.arange(len(eu)) % 3) * 0.5
        nbr = be.Neighborhoods.shortpath(ctx, n, eu, ev, w, cutoff, keep_distances=True)
        try:
            dist = nbr.distances()
            check_builder(nbr, lambda ip, ix: wr.matrix_member_distances(dist, ip, ix), cutoff, k_exp_ref,
                          lambda kind, h: nbr.set_weights_from_distances(kind, cutoff, h), 'graph n=%d cutoff=%g' % (n, cutoff))
            if n >= 63:                                         # per-row radii, some of them 0
                radii = np.where(np.arange(n) % 5 == 0, 0.0, cutoff * (1 + np.arange(n) % 3))
                nbr.set_weights_from_distances('triangular', radii)
                indptr, indices = csr_of_handle(nbr)
                same_bits(nbr.weights(), wr.member_weights('triangular', wr.matrix_member_distances(dist, indptr, indices), indptr, radii), n)
        finally:
            nbr.close()


def test_set_weights_round_trip_refusals_and_untouched_entry_points(amd, be, ctx):
    rng = np.random.default_rng(3)
    n, m = 300, 9
    xy = rng.uniform(size=(n, 2))
    b = np.round(rng.normal(size=(n, m)) * 3, 3)
    nbr = be.Neighborhoods.euclidean(ctx, xy, 0.12)
    attr = be.Attributes.from_host(ctx, b)
    out = ctx.alloc_f64(n, m)
    try:
        def facts():
            be.score(ctx, nbr, attr, 'sum', out.ptr)
            return [nbr.to_dense(), nbr.csr()[0], nbr.csr()[1], nbr.row_counts(), out.download((n, m))]
        before = facts()
        for call in (nbr.weights, lambda: be.score_weighted(ctx, nbr, attr, out.ptr)):
            with pytest.raises(amd.SafeHipError) as err:        # no weights yet
                call()
            assert err.value.code == be._lib.E_INVALID
        with pytest.raises(amd.SafeHipError) as err:            # an euclidean handle keeps no distances
            nbr.set_weights_from_distances('uniform', 1.0)
        assert err.value.code == be._lib.E_INVALID and not nbr.has_weights
        w = 1.0 - rng.uniform(size=nbr.nnz)
        w[::7] = 0.0
        nbr.set_weights(w)
        same_bits(nbr.weights(), w, 'round trip')
        bad_xy = xy.copy()
        bad_xy[5, 1] = np.inf
        refusals = [(lambda v=v: nbr.set_weights(np.where(np.arange(nbr.nnz) == 4, v, w)), be._lib.E_VALUE) for v in (np.nan, np.inf, -1e-300)]
        tenth = np.full(n, 0.1)
        refusals += [(lambda: nbr.set_weights_from_xy(bad_xy, 'uniform', 0.1), be._lib.E_VALUE),
                     (lambda: nbr.set_weights_from_xy(xy, 'uniform', np.nan), be._lib.E_VALUE),
                     (lambda: nbr.set_weights_from_xy(xy, 'uniform', -0.1), be._lib.E_VALUE),
                     (lambda: nbr.set_weights_from_xy(xy, 'gaussian', 0.1, 0.0), be._lib.E_VALUE),
                     (lambda: nbr.set_weights_from_xy(xy, 'gaussian', 0.1, np.inf), be._lib.E_VALUE),
                     (lambda: be._lib.check(be._lib.lib.safe_nbr_weights_from_xy(nbr.handle, be._ptr(xy), 7, be._ptr(tenth), 0.5)),
                      be._lib.E_INVALID)]
        for call, code in refusals:
            with pytest.raises(amd.SafeHipError) as err:
                call()
            assert err.value.code == code
            same_bits(nbr.weights(), w, 'a refused call changed the weights')
        with pytest.raises(ValueError):
            nbr.set_weights_from_xy(xy, 'cosine', 0.1)
        after = facts()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), 'weights changed what an existing entry point computes'
        nbr.set_weights_from_xy(xy, 'triangular', 0.12)         # (warm: the builder's scratch slot has its size)
        live = be.device_live_alloc_count()
        for _ in range(3):
            nbr.set_weights_from_xy(xy, 'triangular', 0.12)
            be.score_weighted(ctx, nbr, attr, out.ptr)
        assert be.device_live_alloc_count() == live
        nbr.clear_weights()
        assert be.device_live_alloc_count() == live - 2
        with pytest.raises(amd.SafeHipError):
            nbr.weights()
        nbr.clear_weights()                                     # twice is fine
    finally:
        out.free()
        attr.close()
        nbr.close()


# ----------------------------------------------------------------------------------------------------------------- W2 ----

def run_score(be, ctx, nbr, attr, col0=0, col1=None, guard=64, kernels=('k_score_weighted',)):
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    buf = ctx.alloc_f64(n * m + guard)
    try:
        buf.upload(np.full(n * m + guard, POISON))
        be.score_weighted(ctx, nbr, attr, buf.ptr, col0, col1)
        assert ctx.last_kernel()[0] in kernels, ctx.last_kernel()[0]
        flat = buf.download((n * m + guard,))
        assert (flat[n * m:] == POISON).all(), 'the call wrote past the end of its output'
        return flat[:n * m].reshape(n, m).copy()
    finally:
        buf.free()


def membership(n, seed, dense_row=False):
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, n)) < min(1.0, 12.0 / n)
    a[np.arange(n), np.arange(n)] = True
    if n >= 3:
        a[1] = False                                            # an empty row (a dense membership may have one)
    if dense_row:
        a[0] = True                                             # every node: n members, more than WS_STAGE when n > 256
    return a.astype(np.int64)


def attributes(n, m, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 4, size=(n, m)).astype(np.uint8)
    b = np.round(rng.normal(size=(n, m)) * 3, 3)
    if n >= 4:
        b[rng.uniform(size=b.shape) < 0.05] = np.nan           # NaN cells
        b[rng.choice(n, max(1, n // 8), replace=False)] = np.nan   # members without a value
    return b.astype(dtype)


SCORE_SHAPES = [(1, 1), (2, 7), (63, 63), (64, 64), (65, 65), (255, 1025), (256, 1), (257, 7), (1025, 65), (2049, 63)]


@pytest.mark.parametrize('n,m', SCORE_SHAPES)
def test_score_weighted(be, ctx, n, m):
    a = membership(n, n + m, dense_row=True)
    indptr, indices = wr.csr_of(a)
    w = 1.0 - np.random.default_rng(n).uniform(size=len(indices))
    w[::5] = 0.0                                                # zero weights stay members
    nbr = be.Neighborhoods.from_dense(ctx, a)
    try:
        nbr.set_weights(w)
        for t, (dtype, order) in enumerate(((np.float64, 'C'), (np.float32, 'F'), (np.uint8, 'C'), (np.float64, 'F'), (np.float32, 'C'))):
            if n * m > 70000 and t >= 2:
                continue                                        # (the large shapes take two storage forms)
            b = attributes(n, m, n * 31 + t, dtype)
            attr = be.Attributes.from_host(ctx, np.asarray(b, order=order))
            # columns contiguous: lanes along columns; rows contiguous (Fortran order, more than one row and column): the tiles
            # and the lane-per-neighborhood shape of the permutation kernel
            ks = ('k_score_weighted',) if order == 'C' else ('k_permtest_weighted',) if min(n, m) > 1 else ('k_score_weighted', 'k_permtest_weighted')
            try:
                want = wr.score(indptr, indices, w, b.astype(np.float64))
                same_bits(run_score(be, ctx, nbr, attr, kernels=ks), want, 'n=%d m=%d %s %s' % (n, m, np.dtype(dtype).name, order))
                if m >= 7:                                      # a sub-range that starts inside a tile
                    c0, c1 = 3, m - 1
                    same_bits(run_score(be, ctx, nbr, attr, c0, c1, kernels=ks), want[:, c0:c1], 'columns %d:%d' % (c0, c1))
                if m == 1025:
                    same_bits(run_score(be, ctx, nbr, attr, 1023, 1025, kernels=ks), want[:, 1023:], 'columns across a block')
            finally:
                attr.close()
    finally:
        nbr.close()


def test_score_weighted_on_csc_input_and_the_order_sensitive_input(be, ctx):
    from scipy import sparse
    a, b, indptr, indices, w = wr.order_sensitive(2100, 7, seed=9, big_row=2049)      # a 2049-member row
    assert np.diff(indptr).max() >= 2049
    nbr = be.Neighborhoods.from_dense(ctx, a)
    dense = be.Attributes.from_host(ctx, b)
    sp = np.where(np.abs(b) > 4, b, 0.0)
    csc = be.Attributes.from_sparse(ctx, sparse.csc_array(sp))
    try:
        nbr.set_weights(w)
        want = wr.score(indptr, indices, w, b)
        got = run_score(be, ctx, nbr, dense)
        same_bits(got, want, 'order-sensitive input')
        same_bits(run_score(be, ctx, nbr, dense), got, 'identical calls, identical bytes')
        down = wr.score(indptr, indices, w, b, descending=True)
        assert (got[0] != down[0]).mean() >= 0.5                # what makes the equality above a test of the order
        same_bits(run_score(be, ctx, nbr, csc, kernels=('k_score_weighted', 'k_permtest_weighted')), wr.score(indptr, indices, w, sp),
                  'a handle from CSC input')
    finally:
        csc.close()
        dense.close()
        nbr.close()


# ----------------------------------------------------------------------------------------------------------------- W3 ----

def run_moments(be, ctx, nbr, attr, weighted=True, sign='both', thr=0.05, col0=0, col1=None, want_z=True, guard=64):
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    names = OUTPUTS + (('z',) if want_z else ())
    sizes = [n * m] * 5 + [m] + ([n * m] if want_z else [])
    bufs = [ctx.alloc_f64(s + guard) for s in sizes]
    poison = np.full(max(sizes) + guard, POISON)
    try:
        for b, s in zip(bufs, sizes):
            b.upload(poison[:s + guard])
        call = be.moments_test_weighted if weighted else be.moments_test
        call(ctx, nbr, attr, sign, thr, [b.ptr for b in bufs[:6]], col0, col1, z_ptr=bufs[6].ptr if want_z else None)
        assert ctx.last_kernel()[0] == ('k_weights_emit' if weighted else 'k_moments_emit')
        out = {}
        for name, b, s in zip(names, bufs, sizes):
            flat = b.download((s + guard,))
            assert (flat[s:] == POISON).all(), '%s: the call wrote past the end of its output' % name
            out[name] = flat[:s].reshape((m,) if name == 'num_enriched' else (n, m)).copy()
            assert not (out[name] == POISON).any(), '%s: a cell was left unwritten' % name
        return out
    finally:
        for b in bufs:
            b.free()


def check_tails(out, live, k_ref, what):
    """p-values against mpmath at the device's z bits; the large side 1 - small; degenerate cells (1, 1, 0)."""
    z, pp, pn = out['z'], out['pvalues_pos'], out['pvalues_neg']
    dead = ~live
    assert (z[dead] == 0).all() and (pp[dead] == 1).all() and (pn[dead] == 1).all(), what + ': degenerate cells'
    upper = z >= 0
    small, large = np.where(upper, pp, pn), np.where(upper, pn, pp)
    assert np.array_equal(bits(large)[live], bits(1.0 - small)[live]), what + ': the large side is not 1 - the small side'
    zs, where = np.unique(bits(z)[live], return_index=True)
    same = np.unique(np.stack([bits(z)[live], bits(small)[live]], axis=1), axis=0)
    assert len(same) == len(zs), what + ': one z, two p-values'
    pick = np.arange(len(zs)) if len(zs) <= 3000 else np.random.default_rng(1).choice(len(zs), 3000, replace=False)
    for zb, p in zip(zs.view(np.float64)[pick], small[live][where][pick]):
        zf, p = float(zb), float(p)
        if abs(zf) > mr.Z_EDGE:
            assert 0.0 <= p <= mr.SMALL_MAX, (what, zf, p)
            continue
        want = mr.small_side(zf)
        err = float(abs(mr.MP.mpf(p) - want) / want / ((1 + mr.MP.mpf(zf) ** 2) * mr.U))
        assert err <= 2 * k_ref, '%s: p(z = %r) = %r: %.2f (1 + z^2) 2^-53, bound %.2f' % (what, zf, p, err, 2 * k_ref)


def check_outputs(out, sign, thr, what):
    pp, pn, nes = out['pvalues_pos'], out['pvalues_neg'], out['nes']
    want = mr.nes_of(pp, pn, sign)
    assert not np.isnan(nes).any() and np.array_equal(np.isinf(nes), np.isinf(want)), what
    np.testing.assert_allclose(nes, want, rtol=1e-6, atol=1e-9, err_msg=what)
    assert np.array_equal(out['nes_binary'], mr.decisions(pp, pn, nes, sign, thr)), what
    assert np.array_equal(out['num_enriched'], out['nes_binary'].sum(axis=0)), what


def test_moments_weighted_designed_case(be, ctx):
    case, indptr, indices, w = wr.designed()
    x, rows, zmap = wr.designed_cells()
    k_ref = mr.designed_k_ref()
    nbr = be.Neighborhoods.from_dense(ctx, case.a.astype(np.int64))
    attr = be.Attributes.from_host(ctx, case.b)
    try:
        nbr.set_weights(w)
        out = run_moments(be, ctx, nbr, attr)
        same_bits(out['ns'], x, 'designed ns')
        z = out['z']
        live = np.ones(z.shape, dtype=bool)
        seen = {}
        for j in range(z.shape[1]):
            for i in range(z.shape[0]):
                key = (rows[i][0], rows[i][2], j, x[i, j])
                want, sd, w1mu = zmap[key]
                if want is None:
                    live[i, j] = False
                    continue
                if key in seen:                                 # equal cells, equal bits: one of them is checked exactly
                    assert z[i, j] == seen[key]
                    continue
                seen[key] = z[i, j]
                bound = mr.U * (6 * abs(want) + 2 * abs(w1mu) / sd)
                dz = abs(mr.MP.mpf(float(z[i, j])) - want)
                WORST['z_designed'] = max(WORST['z_designed'], float(dz / bound))
                assert dz <= bound, 'z(%d, %d) = %r, exact %s' % (i, j, z[i, j], mr.MP.nstr(want, 20))
        check_tails(out, live, k_ref, 'designed')
        for sign, thr in (('highest', 0.05), ('lowest', 1e-9), ('both', 0.05)):
            o = run_moments(be, ctx, nbr, attr, sign=sign, thr=thr, want_z=(sign == 'both'))
            check_outputs(o, sign, thr, 'designed %s' % sign)
            for name in ('ns', 'pvalues_pos', 'pvalues_neg'):
                same_bits(o[name], out[name], 'identical calls, identical bytes: ' + name)
    finally:
        attr.close()
        nbr.close()


def test_moments_weighted_degenerate_kinds(be, ctx):
    n = 40
    rng = np.random.default_rng(2)
    b = np.round(rng.normal(size=(n, 3)) * 3, 3)
    b[:, 2] = 1.5                                               # a constant column
    b[36:] = np.nan                                             # four rows without a value: n_v = 36
    a = (rng.uniform(size=(n, n)) < 0.3).astype(np.int64)
    a[0] = 0
    a[0, :36] = 1                                               # the whole population ...
    a[1] = a[0]
    a[2] = 0
    a[2, 36:] = 1                                               # only members without a value: c = 0
    a[3] = 0                                                    # an empty row
    indptr, indices = wr.csr_of(a)
    w = 1.0 - rng.uniform(size=len(indices))
    w[indptr[0]:indptr[1]] = 0.1                                # ... at weight 0.1: degenerate (decided on min / max)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, b)
    try:
        nbr.set_weights(w)
        out = run_moments(be, ctx, nbr, attr)
        flags = mr.row_flags(b)
        g = wr.row_sums(indptr, indices, w, flags, 36)[3]
        assert g[0] == 0 and g[1] > 0 and g[2] == 0 and g[3] == 0 and (g[4:] > 0).all()
        live = (g > 0)[:, None] & np.array([True, True, False])[None, :]
        check_tails(out, live, mr.designed_k_ref(), 'degenerate kinds')
        assert (out['z'][live] != 0).any()
        lonely = np.full((n, 2), np.nan)
        lonely[7] = (1.0, 2.0)                                  # n_v = 1
        attr1 = be.Attributes.from_host(ctx, lonely)
        try:
            o = run_moments(be, ctx, nbr, attr1)
            assert (o['z'] == 0).all() and (o['pvalues_pos'] == 1).all() and (o['pvalues_neg'] == 1).all()
        finally:
            attr1.close()
    finally:
        attr.close()
        nbr.close()


@pytest.mark.parametrize('n,m', [(1, 1), (15, 63), (16, 64), (17, 65), (33, 1023), (16, 1024), (17, 1025)])
def test_unit_weights_give_the_bytes_of_the_unweighted_test(be, ctx, n, m):
    case = mr.periodic_case(n, m, seed=n + m, integers=True)
    nbr = be.Neighborhoods.from_dense(ctx, case.a.astype(np.int64))
    attr = be.Attributes.from_host(ctx, case.b)
    try:
        nbr.set_weights(np.ones(nbr.nnz))
        for sign in mr.SIGNS:
            want = run_moments(be, ctx, nbr, attr, weighted=False, sign=sign)
            got = run_moments(be, ctx, nbr, attr, weighted=True, sign=sign)
            for name in want:
                same_bits(got[name], want[name], '%s %s' % (sign, name))
    finally:
        attr.close()
        nbr.close()


def test_moments_weighted_triangular_weights(be, ctx):
    rng = np.random.default_rng(17)
    n, m = 300, 5
    xy = rng.uniform(size=(n, 2))
    b = np.round(rng.normal(size=(n, m)) * 3, 3)
    b[rng.choice(n, 30, replace=False)] = np.nan
    nbr = be.Neighborhoods.euclidean(ctx, xy, 0.15)
    attr = be.Attributes.from_host(ctx, b)
    try:
        nbr.set_weights_from_xy(xy, 'triangular', 0.15)
        out = run_moments(be, ctx, nbr, attr)
        indptr, indices = csr_of_handle(nbr)
        w = nbr.weights()
        mean, css = attr.column_moments()
        flags = mr.row_flags(b)
        n_v = int(flags.sum())
        same_bits(out['ns'], wr.score(indptr, indices, w, b), 'ns')
        live = np.zeros(out['z'].shape, dtype=bool)
        for i in range(0, n, 3):
            sel = [e for e in range(indptr[i], indptr[i + 1]) if flags[indices[e]]]
            w1, w2, g = wr.exact_row(w[sel], n_v)
            if g == 0:
                continue
            c, big_a, big_b = len(sel), n_v * w2, w1 * w1
            kappa = float((big_a + big_b) / (big_a - big_b))
            for j in range(m):
                want, sd, w1mu = wr.exact_z(out['ns'][i, j], w1, g, mean[j], css[j])
                bound = 2 * mr.U * ((c * kappa + 4.5) * abs(want) + c * abs(w1mu) / sd)
                dz = abs(mr.MP.mpf(float(out['z'][i, j])) - want)
                WORST['z_real'] = max(WORST['z_real'], float(dz / bound))
                assert dz <= bound, 'z(%d, %d) = %r, exact %s, kappa %.3g' % (i, j, out['z'][i, j], mr.MP.nstr(want, 20), kappa)
                live[i, j] = True
        g_all = wr.row_sums(indptr, indices, w, flags, n_v)[3]
        check_tails(out, (g_all > 0)[:, None] & (css > 0)[None, :], mr.designed_k_ref(), 'triangular')
        check_outputs(out, 'both', 0.05, 'triangular')
        assert live.sum() > 300
        fortran = be.Attributes.from_host(ctx, np.asfortranarray(b))      # the score through the tiles: the same bytes
        try:
            other = run_moments(be, ctx, nbr, fortran)
            same_bits(other['ns'], out['ns'], 'Fortran order: ns')
            # (the column moments add their rows in another order there: css, hence z, may differ in the last bits)
            np.testing.assert_allclose(other['z'], out['z'], rtol=1e-12, atol=1e-12)
        finally:
            fortran.close()
    finally:
        attr.close()
        nbr.close()


# ----------------------------------------------------------------------------------------------------------------- W4 ----

def run_counts(be, ctx, nbr, attr, perms, weighted=True, col0=0, col1=None, guard=64):
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    bufs = [ctx.alloc_f64(n * m + guard) for _ in range(3)]
    try:
        for b in bufs:
            b.upload(np.full(n * m + guard, POISON))
        if weighted:
            be.permtest_counts_weighted(ctx, nbr, attr, perms, *[b.ptr for b in bufs], col0, col1)
            assert ctx.last_kernel()[0] == 'k_permtest_weighted'
        else:
            be.permtest_counts(ctx, nbr, attr, perms, 'sum', *[b.ptr for b in bufs], col0, col1)
        out = []
        for b in bufs:
            flat = b.download((n * m + guard,))
            assert (flat[n * m:] == POISON).all(), 'the call wrote past the end of its output'
            out.append(flat[:n * m].reshape(n, m).copy())
        return out
    finally:
        for b in bufs:
            b.free()


def make_perms(be, ctx, how, n, flags, count, seed):
    if how == 'seeded':
        return be.Permutations(ctx, n, flags, count, seed)
    if how == 'device':
        return be.Permutations(ctx, n, flags, count, None, device_key=0xC0FFEE + seed)
    if how == 'stratified':
        return be.Permutations.stratified(ctx, n, flags, (np.arange(n) % 3).astype(np.int32), count, 0xBEEF + seed)
    rng = np.random.default_rng(seed)
    table = np.tile(np.arange(n), (count, 1))
    mov = np.nonzero(flags)[0]
    for p in range(count):
        table[p, mov] = rng.permutation(mov)
    return be.Permutations.from_table(ctx, table)


# n: one slice, two slices with a short second one, five slices, 17 slices; m: below a tile, 9 (one column short of ...),
# 65 = four tiles and one column (more tiles than the 8 queues hold needs m > 128: the 130-permutation case takes m = 130)
COUNT_CASES = [('seeded', 2, 1, 10), ('device', 65, 9, 1), ('stratified', 300, 65, 10), ('table', 1025, 9, 10),
               ('device', 300, 130, 130), ('seeded', 65, 1, 130), ('table', 2, 9, 1)]


@pytest.mark.parametrize('how,n,m,count', COUNT_CASES)
def test_permtest_counts_weighted(be, ctx, how, n, m, count):
    a = membership(n, n * 7 + m)
    indptr, indices = wr.csr_of(a)
    w = 1.0 - np.random.default_rng(n + m).uniform(size=len(indices))
    w[::4] = 0.0
    b = attributes(n, m, n + count)
    flags = mr.row_flags(b).astype(np.uint8)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, np.asarray(b, order='F' if n % 2 else 'C'))
    perms = make_perms(be, ctx, how, n, flags, count, seed=n + m)
    try:
        nbr.set_weights(w)
        got = run_counts(be, ctx, nbr, attr, perms)
        tables = perms.read().astype(np.int64)
        x, neg, pos = wr.counts(indptr, indices, w, b, tables)
        same_bits(got[0], x, 'ns')
        assert np.array_equal(got[1], neg) and np.array_equal(got[2], pos), (how, n, m, count)
        again = run_counts(be, ctx, nbr, attr, perms)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(got, again)), 'identical calls, identical bytes'
        if m >= 9:
            sub = run_counts(be, ctx, nbr, attr, perms, col0=3, col1=m - 1)
            assert np.array_equal(sub[1], neg[:, 3:m - 1]) and np.array_equal(sub[2], pos[:, 3:m - 1])
    finally:
        perms.close()
        attr.close()
        nbr.close()


def test_counts_on_designed_inputs(be, ctx):
    rng = np.random.default_rng(23)
    n, m, count = 300, 9, 10
    a = membership(n, 5)
    indptr, indices = wr.csr_of(a)
    ints = rng.integers(0, 6, size=(n, m)).astype(np.float64)
    ints[:, 4] = 3.0                                            # a constant column: every permuted score equals the observed
    binary = (rng.uniform(size=(n, m)) < 0.2).astype(np.float64)
    flags = np.ones(n, dtype=np.uint8)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    perms = make_perms(be, ctx, 'seeded', n, flags, count, seed=4)
    try:
        for values in (ints, binary):
            attr = be.Attributes.from_host(ctx, values)
            try:
                nbr.set_weights(np.ones(nbr.nnz))               # unit weights: the bytes of safe_permtest_counts
                want = run_counts(be, ctx, nbr, attr, perms, weighted=False)
                got = run_counts(be, ctx, nbr, attr, perms)
                for p, q, name in zip(got, want, ('ns', 'counts_neg', 'counts_pos')):
                    same_bits(p, q, 'unit weights: ' + name)
                nbr.set_weights(wr.designed_weights(indptr, indices))      # dyadic weights: exact sums
                got = run_counts(be, ctx, nbr, attr, perms)
                if values is ints:
                    assert (got[1][:, 4] == count).all() and (got[2][:, 4] == count).all()
            finally:
                attr.close()
        # the order-sensitive input
        a2, b, ip, ix, w = wr.order_sensitive(n, 5, seed=31)
        nbr2 = be.Neighborhoods.from_dense(ctx, a2)
        attr = be.Attributes.from_host(ctx, b)
        try:
            nbr2.set_weights(w)
            got = run_counts(be, ctx, nbr2, attr, perms)
            x, neg, pos = wr.counts(ip, ix, w, b, perms.read().astype(np.int64))
            same_bits(got[0], x, 'ns')
            assert np.array_equal(got[1], neg) and np.array_equal(got[2], pos)
        finally:
            attr.close()
            nbr2.close()
    finally:
        perms.close()
        nbr.close()


def test_refusals_and_live_allocations(amd, be, ctx):
    n, m = 65, 9
    a = membership(n, 1)
    b = attributes(n, m, 2)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, b)
    small = be.Attributes.from_host(ctx, b[:64])
    perms = make_perms(be, ctx, 'device', n, mr.row_flags(b).astype(np.uint8), 10, 1)
    bufs = [ctx.alloc_f64(n, m) for _ in range(7)]
    ptrs = [x.ptr for x in bufs]
    try:
        calls = [lambda: be.score_weighted(ctx, nbr, attr, ptrs[0]),
                 lambda: be.moments_test_weighted(ctx, nbr, attr, 'both', 0.05, ptrs[:6]),
                 lambda: be.permtest_counts_weighted(ctx, nbr, attr, perms, *ptrs[:3])]
        for call in calls:                                      # no weights
            with pytest.raises(amd.SafeHipError) as err:
                call()
            assert err.value.code == be._lib.E_INVALID
        nbr.set_weights(np.ones(nbr.nnz))
        refused = [lambda: be.score_weighted(ctx, nbr, small, ptrs[0]),
                   lambda: be.score_weighted(ctx, nbr, attr, ptrs[0], 3, 3),
                   lambda: be.score_weighted(ctx, nbr, attr, ptrs[0], 0, m + 1),
                   lambda: be.moments_test_weighted(ctx, nbr, attr, 'both', 1.5, ptrs[:6]),
                   lambda: be.moments_test_weighted(ctx, nbr, attr, 'both', 0.05, [0] + ptrs[1:6]),
                   lambda: be.permtest_counts_weighted(ctx, nbr, attr, perms, ptrs[0], 0, ptrs[2]),
                   lambda: be.permtest_counts_weighted(ctx, nbr, small, perms, *ptrs[:3])]
        for call in refused:
            with pytest.raises(amd.SafeHipError) as err:
                call()
            assert err.value.code == be._lib.E_INVALID
        for call in calls:                                      # warm: the scratch slots have their sizes
            call()
        live = be.device_live_alloc_count()
        for _ in range(3):
            for call in calls:
                call()
        assert be.device_live_alloc_count() == live
    finally:
        for x in bufs:
            x.free()
        perms.close()
        small.close()
        attr.close()
        nbr.close()


def test_print_the_worst_errors():
    print('worst exp error %.3f ulp; worst |dz| / bound: designed %.3f, real weights %.3f'
          % (WORST['exp_ulps'], WORST['z_designed'], WORST['z_real']))
