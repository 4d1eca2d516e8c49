"""Stream order of every entry point that takes device pointers (include/safe_hip.h, "Conventions"): work is enqueued on the
context's stream, a caller may substitute a stream of their own (safe_ctx_set_stream), and behind that stream a context runs
four more (side, aux, two further enrichment streams) that every permutation and count entry point forks onto and joins
back from with event pairs.  A missing wait gives silent, timing-dependent wrong p-values; nothing else in the suite can see
one, because every other test hands over complete inputs and reads outputs after a full synchronisation.

The busy-stream harness (run_busy) makes the caller's stream `s` (a non-default torch stream the context is switched to) busy:
  1. every device INPUT of the call is poisoned (NaN for f32 / f64, 0xFF bytes for integers), the true values wait in staging
     tensors;
  2. a delay -- a chain of f32 4096 x 4096 matmuls -- is enqueued on `s`, an event `delay_done` recorded behind it;
  3. still on `s`, the staging tensors are copied into the inputs: they become valid only once the delay has drained;
  4. the entry point is called; nothing synchronises; `pending = not delay_done.query()` says whether it returned early;
  5. on `s`, every output is copied into a snapshot, then all outputs AND all inputs are poisoned again;
  6. `s.synchronize()`, and the snapshots are compared.
A library stream that starts before the producer of step 3, or that has not been joined when the call returns, reads or
leaves poison.  Before the busy run each case runs once the quiet way (complete inputs, the context on its own stream, a sync):
that fills the lazy caches (statistics of safe_attr_prepare, row flags, routes, cached buffers) exactly as the repeated calls
of bench.py and the drop-in class find them, gives the call's host-side wall time T_call, and gives the quiet outputs.

What is compared: the quiet outputs against the oracle (oracle/safe_oracle.py) at the tolerances the suite uses for the same
quantities -- counts, p-values that are count ratios, FDR-adjusted p-values and binarised outputs exact; observed scores rtol
1e-9 / atol 1e-12; hypergeometric p rtol 1e-6 / atol 1e-300; NES rtol 1e-6 / atol 1e-9; masks and distances bit-equal -- and
the busy snapshots BIT FOR BIT against the quiet outputs of the same handles (tests/test_gpu_routes.py already relies on these
outputs being reproducible), hence against the oracle at the same tolerances.

Sizing of the delay (harness sizing, not a tolerance): one link of the chain is timed with events when the module starts; the
chain is repeated until it lasts max(30 ms, 3 x T_call), capped at 300 ms.  30 ms is three orders of magnitude above a kernel
launch, so a call that returns without waiting does so while the delay runs; 3 x T_call keeps the delay longer than everything
the call itself enqueues; the cap bounds the worst case of a test.  There is no spin kernel: nothing here can hang.

Limits.  The library's streams map onto few hardware queues (four by default), several of them share a queue with the caller's
stream, and a shared queue serialises work: that can MASK a missing wait.  The check is one-sided -- a failure is real, a pass
is weaker evidence than on a device with more queues; queue settings are left alone.  The entry points of SYNCHRONISES drain the
context's stream before they return: for them the consumer's snapshot can see a missing final join only if the unjoined stream
outlives that wait, so what the busy run checks there is the START of the call (every library stream behind the producer of the
inputs) and the results, not the join.  run_busy asserts, right before the call, that the delay is still running: a step of the
harness that drained the stream (a handle destroyed, a hipFree) fails the case instead of turning it into a quiet run; permutation
handles are therefore never destroyed between the delay and the call.  One process, the fixture's context, no retries; the delay
cap and the small shapes keep every test at a fraction of a second.

Asynchrony.  The header promises that functions with only device outputs return without waiting.  SYNCHRONISES lists the
entry points that do wait, each with the readback or host-memory lifetime that makes them (the header names the same ones);
for every other entry point the test asserts `pending`.  The table of `pending` per case is printed when the module ends
(pytest shows it with -s: `pytest tests/test_gpu_stream_order.py -m gpu -s`).
Needs an MI355X."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)
import test_gpu_routes as routes                 # noqa: E402  (DATA, make_data, the switch table, the expected kernel names)

NPERM, SEED = routes.NPERM, routes.SEED
KEY = 0x5AFE0007                                 # key of the device-generated tables
THRESHOLD = 0.05

# entry point -> why it returns only after the context's stream has drained (safepy_amd/csrc, file:line of the wait)
SYNCHRONISES = {
    'safe_score': 'enrich.hip:3210 finish_kernel_timing reads the dominant kernel\'s event pair (hipEventSynchronize)',
    'safe_permtest_counts': 'enrich.hip:3210 finish_kernel_timing; the launchers also wait for their host task lists (enrich.hip:2436, 2946, 3045)',
    'safe_randomization': 'enrich.hip:3523 temporaries of the call; its callers rely on the call having finished when it returns',
    'safe_hypergeom': 'enrich.hip:3614 host id vectors and temporaries of the call (and enrich.hip:3174, 3607)',
    'safe_fdr_adjust': 'fdr.hip: read_flag reads back the count-ratio flag; run frees the enriched counters when it returns',
    'safe_outputs_from_counts': 'enrich.hip:3649 reads back the out-of-range flag (SAFE_E_VALUE)',
    'safe_outputs_from_packed_counts': 'enrich.hip:3684 the slab epilogue followed by a wait: the call has finished when it returns',
    'safe_nes_from_packed_counts': 'enrich.hip:3684 (it is safe_outputs_from_packed_counts with one output)',
    'safe_attr_nan_to_zero': 'attr.hip:592 frees the support lists derived from the old values',
}

PENDING = {}                                     # case -> (entry points, pending)


# --------------------------------------------------------------------------------------------------------- fixtures ----

@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


class Lab:
    """The caller's side of the harness: torch, the busy stream, the operands of the delay chain and the data kinds."""

    def __init__(self, be, ctx, torch):
        self.be, self.ctx, self.torch = be, ctx, torch
        self.s = torch.cuda.Stream()
        self.s2 = torch.cuda.Stream()
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
        self.link_ms = max(e0.elapsed_time(e1) / 4.0, 0.02)
        self.kinds = {}
        self.refs = {}

    def delay(self, stream, t_call_ms):
        """Enqueues the chain on `stream`; returns the event recorded behind it."""
        want_ms = min(max(30.0, 3.0 * t_call_ms), 300.0)
        with self.torch.cuda.stream(stream):
            for _ in range(int(np.ceil(want_ms / self.link_ms))):
                self.torch.mm(self.a, self.a, out=self.c)
            done = self.torch.cuda.Event()
            done.record(stream)
        return done

    def kind(self, name):
        """(membership handle, dense 0/1 membership as f64, f64 C-order attribute values, n, m) of a data kind of test_gpu_routes.py."""
        if name not in self.kinds:
            nbr, attr, n, m = routes.make_data(self.be, self.ctx, name)
            b = attr.download(np.float64, 'C')
            attr.close()
            self.kinds[name] = (nbr, nbr.to_dense().astype(np.float64), b, n, m)     # (f64: the oracle's np.dot goes through BLAS)
        return self.kinds[name]

    def ref(self, key, make):
        if key not in self.refs:
            self.refs[key] = make()
        return self.refs[key]

    def close(self):
        for nbr, *_ in self.kinds.values():
            nbr.close()


@pytest.fixture(scope='module')
def lab(amd, ctx):
    import torch
    from safepy_amd import backend as be
    assert torch.cuda.is_available()
    lab = Lab(be, ctx, torch)
    yield lab
    ctx.set_stream(None)
    torch.cuda.synchronize()
    lab.close()
    lines = ['', 'returned while the caller\'s stream was still busy (pending), per case:']
    lines += ['  %-7s %-72s %s' % ('yes' if pend else 'no', case, ' + '.join(entries)) for case, (entries, pend) in PENDING.items()]
    print('\n'.join(lines))                      # (shown with -s, and in the teardown section of a failing test)


@pytest.fixture
def switches(monkeypatch):
    """Sets the routing switches of a case and clears the others (tests/test_gpu_routes.py run_case)."""
    def apply(env):
        for key, var in routes.SWITCHES.items():
            if key in env:
                monkeypatch.setenv(var, env[key])
            else:
                monkeypatch.delenv(var, raising=False)
    apply({})
    return apply


# ---------------------------------------------------------------------------------------------------------- harness ----

def poison(t):
    """NaN into f32 / f64 tensors, 0xFF bytes into integer ones."""
    if t.is_floating_point():
        t.fill_(float('nan'))
    else:
        import torch
        t.view(-1).view(torch.uint8).fill_(255)


class Call:
    """One case: `inputs` [(device tensor, staging tensor with its true values)], `outputs` [device tensors], fn() makes the
    library call(s); early() creates what the case creates before the delay, late() what it creates behind the producer,
    post() runs straight after the call (before the consumer), done() closes what is left; check(outputs as NumPy arrays)
    compares with the oracle; entries: the entry points fn() goes through."""

    def __init__(self, entries, inputs, outputs, fn, check, early=None, late=None, post=None, done=None):
        self.entries = tuple(entries)
        self.inputs, self.outputs, self.fn, self.check = list(inputs), list(outputs), fn, check
        noop = lambda: None
        self.early, self.late, self.post, self.done = early or noop, late or noop, post or noop, done or noop


def seq(calls):
    """Several calls issued back to back as one case: separate inputs and outputs, no synchronisation in between."""
    def each(name):
        def run():
            for c in calls:
                getattr(c, name)()
        return run

    def check(outs):
        at = 0
        for c in calls:
            c.check(outs[at:at + len(c.outputs)])
            at += len(c.outputs)
    return Call([e for c in calls for e in c.entries], [i for c in calls for i in c.inputs], [o for c in calls for o in c.outputs],
                each('fn'), check, each('early'), each('late'), each('post'), each('done'))


def numpy_of(t):
    return t.cpu().numpy()


def run_quiet(lab, call):
    """Complete inputs, the context on its own stream, a sync: (outputs, host wall time of the call in ms)."""
    torch, ctx = lab.torch, lab.ctx
    ctx.set_stream(None)
    for o in call.outputs:
        poison(o)
    for t, staging in call.inputs:                # (after the poison: an in-place call's inputs are outputs too)
        t.copy_(staging)
    torch.cuda.synchronize()
    call.early()
    call.late()
    t0 = time.perf_counter()
    call.fn()
    ctx.sync()
    t_call_ms = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    return [numpy_of(o) for o in call.outputs], t_call_ms


def run_busy(lab, call, t_call_ms, stream=None):
    """The call on the busy caller's stream (module docstring): (snapshots of the outputs, pending)."""
    torch, ctx = lab.torch, lab.ctx
    s = stream or lab.s
    snaps = [torch.empty_like(o) for o in call.outputs]
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        call.early()
        with torch.cuda.stream(s):
            for o in call.outputs:
                poison(o)
            for t, _ in call.inputs:
                poison(t)
        delay_done = lab.delay(s, t_call_ms)
        with torch.cuda.stream(s):
            for t, staging in call.inputs:
                t.copy_(staging)
        call.late()
        lab.delay_done = delay_done                   # (for a case that samples `pending` at a second point)
        # the guard of the harness itself: nothing between the delay and the call may have drained the caller's stream
        assert not delay_done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
        call.fn()
        pending = not delay_done.query()
        call.post()
        with torch.cuda.stream(s):
            for snap, o in zip(snaps, call.outputs):
                snap.copy_(o)
            for o in call.outputs:
                poison(o)
            for t, _ in call.inputs:
                poison(t)
        s.synchronize()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
    return [numpy_of(x) for x in snaps], pending


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_case(lab, case, call, kernel=None):
    """Quiet run against the oracle, busy run bit for bit against the quiet run, `pending` recorded (and asserted for the entry
    points the header calls asynchronous)."""
    try:
        quiet, t_call_ms = run_quiet(lab, call)
        if kernel is not None:
            assert lab.ctx.last_kernel()[0] == kernel
        call.check(quiet)
        busy, pending = run_busy(lab, call, t_call_ms)
    finally:
        call.done()
    PENDING[case] = (call.entries, pending)
    for i, (q, b) in enumerate(zip(quiet, busy)):
        assert np.array_equal(bits(b), bits(q)), '%s: output %d of the busy run differs from the quiet run' % (case, i)
    call.check(busy)
    if not any(e in SYNCHRONISES for e in call.entries):
        assert pending, '%s returned only after the caller\'s stream had drained; the header calls it asynchronous' % case
    return quiet


# ---------------------------------------------------------------------------------------------- oracle comparisons ----

def same(got, want, what=''):
    np.testing.assert_array_equal(got, want, err_msg=what)


def close(got, want, rtol, atol, what=''):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, equal_nan=True, err_msg=what)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what


def outputs_of_counts(ns, counts_neg, counts_pos, sign='both'):
    """safe.py:528-554 and 468-472 from counts (oracle/safe_oracle.py pvalues_by_randomization + binarize)."""
    cn, cp = counts_neg.copy(), counts_pos.copy()
    if ns is not None:
        cn[np.isnan(ns)] = np.nan
        cp[np.isnan(ns)] = np.nan
    pn, pp = cn / NPERM, cp / NPERM
    with np.errstate(invalid='ignore', divide='ignore'):
        nes_pos = -np.log10(np.where(pp == 0, 1 / NPERM, pp))
        nes_neg = -np.log10(np.where(pn == 0, 1 / NPERM, pn))
    nes = {'highest': nes_pos, 'lowest': nes_neg, 'both': nes_pos - nes_neg}[sign]
    nb, ne = orc.binarize(nes, THRESHOLD)
    return {'pvalues_neg': pn, 'pvalues_pos': pp, 'nes': nes, 'nes_binary': nb, 'num_neighborhoods_enriched': ne}


def perm_reference(lab, kind, tag, a, b, score, device):
    """ns, counts and the outputs of compute_pvalues for one data kind, seeded (the oracle's own run) or on the oracle's
    restatement of the device-generated tables."""
    def make():
        ns = orc.compute_neighborhood_score(a, b, score)
        if not device:
            cn, cp = orc.run_permutations(a, b, score, NPERM, SEED)
            out = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type=score,
                                      num_permutations=NPERM, random_seed=SEED, attribute_sign='both', enrichment_threshold=THRESHOLD)
        else:
            tables = orc.device_stream_tables(a.shape[0], (~np.isnan(b)).any(axis=1), NPERM, KEY)
            cn, cp = np.zeros(ns.shape), np.zeros(ns.shape)
            with np.errstate(invalid='ignore'):
                for row in tables:
                    sc = orc.compute_neighborhood_score(a, b[row], score)
                    cn += sc <= ns
                    cp += sc >= ns
            out = outputs_of_counts(ns, cn, cp)
        out = dict(out, ns=ns, counts_neg=cn, counts_pos=cp)
        return out
    return lab.ref((kind, tag, score, bool(device)), make)


def check_randomization(want, ns, pn, pp, nes, nb, ne):
    close(ns, want['ns'], 1e-9, 1e-12, 'ns')
    same(pn, want['pvalues_neg'], 'pvalues_neg')
    same(pp, want['pvalues_pos'], 'pvalues_pos')
    close(nes, want['nes'], 1e-6, 1e-9, 'nes')
    same(nb, want['nes_binary'], 'nes_binary')
    same(ne, want['num_neighborhoods_enriched'], 'num_enriched')


# ------------------------------------------------------------------------------------------- enrichment call cases ----

LAYOUTS = [(np.float64, 'C'), (np.float32, 'F'), (np.float64, 'F'), (np.float32, 'C')]


class Borrowed:
    """An attribute matrix in a torch tensor the library borrows (Attributes.from_device), its staging copy and the values
    the oracle gets (the f32 form rounds them)."""

    def __init__(self, lab, b64, dtype=np.float64, order='C'):
        torch = lab.torch
        host = b64.astype(dtype)
        self.values = host.astype(np.float64)
        self.n, self.m = host.shape
        self.dtype, self.order = dtype, order
        flat = np.ascontiguousarray(host if order == 'C' else host.T)
        self.staging = torch.from_numpy(flat).to('cuda')
        self.tensor = torch.empty_like(self.staging)
        self.flags = (~np.isnan(self.values)).any(axis=1).astype(np.uint8)       # movable rows, from the host values

    def handle(self, lab):
        return lab.be.Attributes.from_device(lab.ctx, self.tensor.data_ptr(), self.dtype, self.n, self.m, self.order,
                                             keepalive=self.tensor)


def enrich_call(lab, entry, kind, score, perms_how=('seeded', 'before'), layout=(np.float64, 'C'), own_nbr=False,
                destroy_after=False):
    """A Call for safe_score / safe_permtest_counts / safe_randomization / safe_hypergeom on a data kind with a borrowed
    attribute matrix.  perms_how: ('seeded' | 'device', 'before' | 'after' the delay).  own_nbr: a membership handle of the
    case's own (from the dense matrix); destroy_after: attr, perms (and the case's own nbr) are destroyed straight after the call."""
    be, ctx, torch = lab.be, lab.ctx, lab.torch
    nbr, a, b64, n, m = lab.kind(kind)
    bor = Borrowed(lab, b64, *layout)
    tag = np.dtype(layout[0]).name
    b = bor.values
    state = {'attr': bor.handle(lab), 'perms': None, 'old': [], 'nbr': be.Neighborhoods.from_dense(ctx, a.astype(np.int64)) if own_nbr else nbr}
    device = perms_how[0] == 'device'
    shapes = {'permtest_counts': [(n, m)] * 3, 'randomization': [(n, m)] * 5 + [(m,)], 'score': [(n, m)],
              'hypergeom': [(n, m)] * 3 + [(m,)]}[entry]
    outs = [torch.empty(shape, dtype=torch.float64, device='cuda') for shape in shapes]
    ptrs = [o.data_ptr() for o in outs]
    needs_perms = entry in ('permtest_counts', 'randomization')

    def new_perms():
        # The handle before it stays open until done(): safe_perms_destroy waits for the context's stream, and a destroyed
        # handle of another shape in the context's cache is freed by the next create (hipFree waits for the device) -- either
        # would drain the caller's stream before the call.  With every earlier handle still open the cache is empty here.
        if state['perms'] is not None:
            state['old'].append(state['perms'])
        state['perms'] = be.Permutations(ctx, n, bor.flags, NPERM, None if device else SEED, device_key=KEY if device else None)

    def early():
        if needs_perms and state['perms'] is None:    # (the busy run keeps the quiet run's handle: the repeated-call state)
            new_perms()

    def late():
        if needs_perms and perms_how[1] == 'after' and state.get('ran'):
            new_perms()                               # its tables are still being generated when the call is made

    def fn():
        state['ran'] = True
        if entry == 'permtest_counts':
            be.permtest_counts(ctx, state['nbr'], state['attr'], state['perms'], score, *ptrs)
        elif entry == 'randomization':
            be.randomization(ctx, state['nbr'], state['attr'], state['perms'], score, 'both', THRESHOLD, ptrs)
        elif entry == 'score':
            be.score(ctx, state['nbr'], state['attr'], score, ptrs[0])
        else:
            be.hypergeom(ctx, state['nbr'], state['attr'], THRESHOLD, ptrs)

    def close_all():
        for key in ('attr', 'perms') + (('nbr',) if own_nbr else ()):
            if state[key] is not None:
                state[key].close()                    # (the borrowed tensor stays the caller's: nothing of it is freed)
        for old in state['old']:
            old.close()

    def check(got):
        if entry == 'score':
            want = lab.ref((kind, tag, score, 'score'), lambda: orc.compute_neighborhood_score(a, b, score))
            close(got[0], want, 1e-9, 1e-12, 'ns')
        elif entry == 'hypergeom':
            want = lab.ref((kind, tag, 'hypergeom'), lambda: orc.compute_pvalues(a, b.copy(), enrichment_type='hypergeometric',
                                                                                 enrichment_threshold=THRESHOLD))
            close(got[0], want['pvalues_pos'], 1e-6, 1e-300, 'pvalues_pos')
            close(got[1], want['nes'], 1e-6, 1e-9, 'nes')
            same(got[2], want['nes_binary'], 'nes_binary')
            same(got[3], want['num_neighborhoods_enriched'], 'num_enriched')
        else:
            want = perm_reference(lab, kind, tag, a, b, score, device)
            if entry == 'permtest_counts':
                close(got[0], want['ns'], 1e-9, 1e-12, 'ns')
                same(got[1], want['counts_neg'], 'counts_neg')
                same(got[2], want['counts_pos'], 'counts_pos')
            else:
                check_randomization(want, *got)

    return Call(['safe_' + entry], [(bor.tensor, bor.staging)], outs, fn, check, early=early, late=late,
                post=close_all if destroy_after else None, done=close_all)


# ------------------------------------------------------------------------------------------------------- case 1 ----

@pytest.mark.parametrize('n,mode', [(301, 'mask'), (300, 'distances'), (513, 'both')])
def test_euclidean_dense_dev(lab, n, mode):
    torch, ctx = lab.torch, lab.ctx
    xy = np.random.default_rng(n).uniform(-2, 3, size=(n, 2))
    nr = orc.layout_radius(xy[:, 0], 0.15)
    staging = torch.from_numpy(xy).to('cuda')
    t_xy = torch.empty_like(staging)
    mask = torch.empty((n, n), dtype=torch.int64, device='cuda') if mode != 'distances' else None
    dist = torch.empty((n, n), dtype=torch.float64, device='cuda') if mode != 'mask' else None
    outs = [t for t in (mask, dist) if t is not None]
    want_d = orc.euclidean_distances(xy)

    def check(got):
        if mask is not None:
            same(got[0], (want_d < nr).astype(np.int64), 'mask')
        if dist is not None:
            assert np.array_equal(bits(got[-1]), bits(want_d)), 'distances'

    call = Call(['safe_euclidean_dense_dev'], [(t_xy, staging)], outs,
                lambda: ctx.euclidean_dense(t_xy.data_ptr(), n, nr, mask.data_ptr() if mask is not None else None,
                                            dist.data_ptr() if dist is not None else None), check)
    run_case(lab, 'euclidean_dense_dev-%s-%d' % (mode, n), call)


def test_nbr_to_dense_dev(lab):
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    n = 517
    a = (np.random.default_rng(4).uniform(size=(n, n)) < 0.03).astype(np.int64)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    out = torch.empty((n, n), dtype=torch.int64, device='cuda')
    call = Call(['safe_nbr_to_dense_i64_dev'], [], [out], lambda: nbr.to_dense_dev(out.data_ptr()), lambda got: same(got[0], a),
                done=nbr.close)
    run_case(lab, 'nbr_to_dense_i64_dev', call)


def test_dev_memset(lab):
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    out = torch.empty(100003, dtype=torch.uint8, device='cuda')
    call = Call(['safe_dev_memset'], [], [out],
                lambda: be.check(be.lib.safe_dev_memset(ctx.handle, C.c_void_p(out.data_ptr()), 0x5A, out.numel())),
                lambda got: same(got[0], np.full(100003, 0x5A, dtype=np.uint8)))
    run_case(lab, 'dev_memset', call)


@pytest.mark.parametrize('dtype,order', LAYOUTS, ids=lambda v: getattr(v, '__name__', v))
def test_attr_create_dev_then_nan_to_zero(lab, dtype, order):
    """safe_attr_create_dev borrows a buffer whose producer is still queued; safe_attr_nan_to_zero rewrites it in place."""
    be, ctx = lab.be, lab.ctx
    b = np.random.default_rng(11).normal(size=(333, 7))
    b[np.random.default_rng(12).uniform(size=b.shape) < 0.2] = np.nan
    bor = Borrowed(lab, b, dtype, order)
    want = np.where(np.isnan(bor.values), 0.0, bor.values).astype(dtype)
    want = np.ascontiguousarray(want if order == 'C' else want.T)

    tag = '%s-%s' % (np.dtype(dtype).name, order)
    made = []

    def fn():                                          # the call whose `pending` is asserted: safe_attr_create_dev alone
        made.append(bor.handle(lab))

    def consume():                                     # its consumer, straight behind it; `pending` sampled a second time
        attr = made.pop()
        attr.nan_to_zero()
        if getattr(lab, 'delay_done', None) is not None:
            PENDING['attr_nan_to_zero-' + tag] = (('safe_attr_nan_to_zero',), not lab.delay_done.query())
        attr.close()

    def quiet_too():                                   # (the quiet run has no post(): the consumer runs in done())
        while made:
            consume()

    lab.delay_done = None
    call = Call(['safe_attr_create_dev'], [(bor.tensor, bor.staging)], [bor.tensor], fn, lambda got: same(got[0], want), post=consume)
    inner_fn = call.fn
    state = {'quiet': True}

    def fn_quiet_aware():
        inner_fn()
        if state['quiet']:                             # the quiet run: create and consume in one go
            state['quiet'] = False
            consume()
    call.fn = fn_quiet_aware
    call.done = quiet_too
    run_case(lab, 'attr_create_dev-%s (then nan_to_zero)' % tag, call)


@pytest.mark.parametrize('entry', ['score', 'permtest_counts', 'randomization', 'hypergeom'])
@pytest.mark.parametrize('dtype,order', LAYOUTS, ids=lambda v: getattr(v, '__name__', v))
def test_default_route_borrowed_layouts(lab, switches, entry, dtype, order):
    """The four enrichment entry points on their default route, the attribute matrix borrowed in f32 / f64, C / Fortran order."""
    call = enrich_call(lab, entry, 'bin', 'sum', layout=(dtype, order))
    run_case(lab, '%s-bin-default-%s-%s' % (entry, np.dtype(dtype).name, order), call,
             kernel=routes.EXPECTED[routes._case_id(entry, 'bin', 'sum', {})])


def _p_matrices(lab, form, n=257, m=70):
    """(pvalues_neg or None, pvalues_pos, num_permutations) of a safe_fdr_adjust form, with NaN rows and ties."""
    rng = np.random.default_rng(len(form))
    if form == 'histogram':
        pn, pp = (rng.integers(0, NPERM + 1, size=(n, m)) / NPERM for _ in range(2))
    else:
        pn, pp = (np.round(rng.uniform(size=(n, m)), 2) for _ in range(2))
    pn[3], pp[3] = np.nan, np.nan
    pp[7, 5] = pn[7, 5] = np.nan
    return (None if form == 'hypergeometric' else pn), pp, (0 if form == 'hypergeometric' else NPERM)


def fdr_call(lab, form):
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    pn, pp, nperm = _p_matrices(lab, form)
    n, m = pp.shape
    st = [torch.from_numpy(x).to('cuda') if x is not None else None for x in (pn, pp)]
    dev = [torch.empty_like(x) if x is not None else None for x in st]
    nes, nb = (torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(2))
    ne = torch.empty((m,), dtype=torch.float64, device='cuda')
    ins = [(d, s) for d, s in zip(dev, st) if d is not None]
    outs = [d for d in dev if d is not None] + [nes, nb, ne]

    def check(got):
        with np.errstate(invalid='ignore', divide='ignore'):
            if nperm:
                qn, qp = orc.fdr_rows(pn), orc.fdr_rows(pp)
                want_nes = -np.log10(np.where(qp == 0, 1 / nperm, qp)) + np.log10(np.where(qn == 0, 1 / nperm, qn))
                same(got[0], qn, 'pvalues_neg')
            else:
                qp = orc.fdr_rows(pp)
                want_nes = -np.log10(qp)
        want_nb, want_ne = orc.binarize(want_nes, THRESHOLD)
        same(got[-4], qp, 'pvalues_pos')
        close(got[-3], want_nes, 1e-6, 1e-9, 'nes')
        same(got[-2], want_nb, 'nes_binary')
        same(got[-1], want_ne, 'num_enriched')

    fn = lambda: be.fdr_adjust(ctx, n, m, nperm, 'both', THRESHOLD, [dev[0].data_ptr() if dev[0] is not None else None, dev[1].data_ptr(),
                                                                    nes.data_ptr(), nb.data_ptr(), ne.data_ptr()])
    return Call(['safe_fdr_adjust'], ins, outs, fn, check)


@pytest.mark.parametrize('form', ['histogram', 'sorted', 'hypergeometric'])
def test_fdr_adjust(lab, form):
    """The p-value matrices are adjusted in place: they are inputs produced behind the delay and outputs."""
    run_case(lab, 'fdr_adjust-' + form, fdr_call(lab, form))


def test_outputs_from_counts(lab):
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    rng = np.random.default_rng(2)
    n, m = 301, 37
    cn, cp = (rng.integers(0, NPERM + 1, size=(n, m)).astype(np.float64) for _ in range(2))
    ns = rng.normal(size=(n, m))
    ns[rng.uniform(size=(n, m)) < 0.05] = np.nan
    st = [torch.from_numpy(x).to('cuda') for x in (cn, cp, ns)]
    dev = [torch.empty_like(x) for x in st]
    outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(4)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]
    want = outputs_of_counts(ns, cn, cp)

    def check(got):
        same(got[0], want['pvalues_neg'])
        same(got[1], want['pvalues_pos'])
        close(got[2], want['nes'], 1e-6, 1e-9)
        same(got[3], want['nes_binary'])
        same(got[4], want['num_neighborhoods_enriched'])

    call = Call(['safe_outputs_from_counts'], list(zip(dev, st)), outs,
                lambda: be.outputs_from_counts(ctx, n, m, NPERM, 'both', THRESHOLD, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                               [o.data_ptr() for o in outs]), check)
    run_case(lab, 'outputs_from_counts', call)


@pytest.fixture
def exchange_chunk(lab):
    """One armed exchange chunk (safe_set_exchange_chunks) for the chunk exports; switched off afterwards."""
    lab.be.set_exchange_chunks(lab.ctx, 1, 64)
    yield
    lab.be.set_exchange_chunks(lab.ctx, 0)


def test_packed_counter_exports_and_their_consumers(lab, switches, exchange_chunk):
    """safe_randomization on the bit-sliced kernel, then the three exports of its counters (whole, chunk, narrow chunk) straight
    behind it; then, with the exported slabs as inputs produced behind the delay, every consumer of packed counters."""
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    nbr, a, b64, n, m = lab.kind('bin')
    rnd = enrich_call(lab, 'randomization', 'bin', 'sum')
    run_quiet(lab, rnd)                                                     # (the sizes of the counters)
    n_pad, m_loc, layout = be.packed_counts_info(ctx)
    assert layout == 0 and m_loc == m
    narrow_words = be.packed_slab_words(m, n_pad, True)
    whole, chunk = (torch.empty(m * n_pad + 64, dtype=torch.int32, device='cuda') for _ in range(2))
    narrow = torch.empty(narrow_words + 64, dtype=torch.int32, device='cuda')

    def exports():
        rnd.fn()
        be.export_packed_counts(ctx, whole.data_ptr(), m * n_pad)
        be.export_packed_chunk(ctx, 0, chunk.data_ptr(), chunk.numel(), None)
        be.export_packed_chunk(ctx, 0, narrow.data_ptr(), narrow.numel(), None, narrow=True)

    def check_exports(got):
        rnd.check(got[:6])
        same(got[7][:m * n_pad], got[6][:m * n_pad], 'chunk 0 is the whole block')
        assert not got[7][m * n_pad:].any() and not got[8][narrow_words:].any()          # the rest of the capacity is zeroed

    both = Call(rnd.entries + ('safe_export_packed_counts', 'safe_export_packed_chunk', 'safe_export_packed_chunk_narrow'),
                rnd.inputs, rnd.outputs + [whole, chunk, narrow], exports, check_exports, early=rnd.early, late=rnd.late, done=rnd.done)
    quiet = run_case(lab, 'randomization+export_packed_*', both)
    # the exports on their own behind the delay (their source, the context's counters, is complete): asynchronous
    alone = Call(['safe_export_packed_counts', 'safe_export_packed_chunk', 'safe_export_packed_chunk_narrow'], [], [whole, chunk, narrow],
                 lambda: (be.export_packed_counts(ctx, whole.data_ptr(), m * n_pad),
                          be.export_packed_chunk(ctx, 0, chunk.data_ptr(), chunk.numel(), None),
                          be.export_packed_chunk(ctx, 0, narrow.data_ptr(), narrow.numel(), None, narrow=True)),
                 lambda got: [same(g, q) for g, q in zip(got, quiet[6:])])
    run_case(lab, 'export_packed_* alone', alone)

    want = perm_reference(lab, 'bin', 'float64', a, b64, 'sum', False)
    slab_u32 = torch.from_numpy(quiet[7]).to('cuda')
    slab_narrow = torch.from_numpy(quiet[8]).to('cuda')

    def consumer(entry, staging, lay, explicit_stream=False):
        dev = torch.empty_like(staging)
        outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(1 if entry == 'nes' else 4)]
        ptrs = [o.data_ptr() for o in outs]

        def fn():
            if entry == 'nes':
                be.nes_from_packed_counts(ctx, nbr, dev.data_ptr(), lay, n_pad, m, NPERM, 'both', ptrs[0])
            elif entry == 'counts':
                be.outputs_from_packed_counts(ctx, nbr, dev.data_ptr(), lay, n_pad, m, NPERM, 'both', THRESHOLD, ptrs)
            else:
                be.outputs_from_packed_slabs(ctx, nbr, dev.data_ptr(), lay, n_pad, dev.numel(), [m], [0], m, NPERM, 'both', THRESHOLD, ptrs,
                                             stream=lab.s.cuda_stream if explicit_stream else None)

        def check(got):
            if entry == 'nes':
                close(got[0], want['nes'], 1e-6, 1e-9, 'nes')
                return
            same(got[0], want['pvalues_neg'], 'pvalues_neg')
            same(got[1], want['pvalues_pos'], 'pvalues_pos')
            close(got[2], want['nes'], 1e-6, 1e-9, 'nes')
            same(got[3], want['nes_binary'], 'nes_binary')
        name = {'nes': 'safe_nes_from_packed_counts', 'counts': 'safe_outputs_from_packed_counts', 'slabs': 'safe_outputs_from_packed_slabs'}[entry]
        return Call([name], [(dev, staging)], outs, fn, check)

    run_case(lab, 'nes_from_packed_counts', consumer('nes', slab_u32, layout))
    run_case(lab, 'outputs_from_packed_counts', consumer('counts', slab_u32, layout))
    run_case(lab, 'outputs_from_packed_slabs-u32', consumer('slabs', slab_u32, layout, explicit_stream=True))
    run_case(lab, 'outputs_from_packed_slabs-narrow', consumer('slabs', slab_narrow, layout | be.PACKED_NARROW, explicit_stream=True))


# ------------------------------------------------------------------------------------------------------- case 2 ----

# one case per kernel family tests/test_gpu_routes.py names: (data kind, score, switches)
PERM_FAMILIES = [
    ('bin', 'sum', {}),                                            # bit-sliced
    ('bin', 'sum', {'F': 'scatter'}),                              # scatter
    ('bin', 'sum', {'F': 'gather'}),                               # f64 gather
    ('q_narrow', 'sum', {'F': 'gather'}),
    ('q_narrow', 'sum', {}),                                       # LDS-resident f64
    ('q_narrow', 'sum', {'F': 'mfma'}),                            # matrix-core sum
    ('q_narrow', 'z-score', {'NARROW': '0'}),                      # matrix-core z-score
    ('q_narrow', 'z-score', {'NARROW': '0', 'MFMA_Z': '0'}),       # ... and its f64 counterpart
    ('q_decline', 'sum', {'NARROW': '0'}),                         # the column the matrix cores decline
    ('q_big_n', 'sum', {}),                                        # N too large for the LDS-resident kernel
    ('q_big_n', 'z-score', {'MFMA_Z': '0'}),
    ('dense', 'sum', {}),
    ('bin_hub', 'sum', {}),
]
COUNT_FAMILIES = [
    ('bin', 'sum', {}),                                            # bit-sliced counts
    ('bin', 'sum', {'F': 'gather'}),                               # f64 gather / per-element hypergeometric kernel
    ('bin', 'sum', {'COUNTS': 'mfma'}),                            # matrix-core counts: split + table
    ('bin', 'sum', {'COUNTS': 'mfma', 'SPLIT': '0'}),
    ('bin', 'sum', {'TABLE': '0', 'COUNTS': 'mfma'}),
    ('dense', 'sum', {}),                                          # matrix-core counts by the dense-network rule
    ('dense', 'sum', {'SPLIT': '0'}),
    ('dense', 'sum', {'TABLE': '0'}),
    ('bin_hub', 'sum', {}),
    ('q_narrow', 'sum', {}),                                       # (score only: the hypergeometric test is for 0/1 data)
    ('q_narrow', 'z-score', {}),
]
PERMS_HOW = [('seeded', 'before'), ('device', 'after')]
# the other two combinations where the tables are cheapest and where the launches fork widest
PERMS_SWAPPED = [('seeded', 'after'), ('device', 'before')]

ROUTE_CASES = ([(e, *f, how) for e in ('permtest_counts', 'randomization') for f in PERM_FAMILIES for how in PERMS_HOW] +
               [(e, *f, how) for e in ('permtest_counts', 'randomization') for f in (PERM_FAMILIES[0], PERM_FAMILIES[5]) for how in PERMS_SWAPPED] +
               [(e, *f, None) for e in ('score', 'hypergeom') for f in COUNT_FAMILIES
                if not (e == 'hypergeom' and (f[1] != 'sum' or f[0] == 'q_narrow'))])


def _route_id(entry, kind, score, env, how):
    return routes._case_id(entry, kind, score, env) + ('' if how is None else '-%s-%s' % how)


@pytest.mark.parametrize('case', ROUTE_CASES, ids=[_route_id(*c) for c in ROUTE_CASES])
def test_forked_routes(lab, switches, case):
    entry, kind, score, env, how = case
    switches(env)
    call = enrich_call(lab, entry, kind, score, perms_how=how or ('seeded', 'before'))
    run_case(lab, _route_id(*case), call, kernel=routes.EXPECTED[routes._case_id(entry, kind, score, env)])


# ------------------------------------------------------------------------------------------------------- case 3 ----

def _with_switches(call, switches, env):
    """The call with its routing switches set right before it (consecutive calls of a sequence take different routes)."""
    inner = call.fn

    def fn():
        switches(env)
        inner()
    call.fn = fn
    return call


def test_back_to_back_permutation_tests(lab, switches):
    """bits -> matrix cores -> gather -> bits on one context into separate outputs, one sync at the end.  These entry points wait
    for the context's stream themselves (SYNCHRONISES), so only the first call of a sequence meets the busy stream; the later ones
    check that nothing a call leaves behind -- scratch slots, cached buffers, the table pipeline of a handle made behind the
    delay -- disturbs a call of another route and shape issued straight after it."""
    steps = [('bin', {}), ('q_narrow', {'F': 'mfma'}), ('q_narrow', {'F': 'gather'}), ('bin', {})]
    calls = [_with_switches(enrich_call(lab, 'permtest_counts', kind, 'sum', perms_how=('seeded', 'before' if i % 2 else 'after')), switches, env)
             for i, (kind, env) in enumerate(steps)]
    run_case(lab, 'sequence: bits -> mfma -> gather -> bits', seq(calls))


def test_back_to_back_hypergeom_randomization_fdr(lab, switches):
    calls = [_with_switches(enrich_call(lab, 'hypergeom', 'dense', 'sum'), switches, {}),
             _with_switches(enrich_call(lab, 'randomization', 'q_narrow', 'sum', perms_how=('device', 'after')), switches, {}),
             fdr_call(lab, 'histogram'),
             _with_switches(enrich_call(lab, 'score', 'bin', 'sum'), switches, {'COUNTS': 'mfma'})]
    run_case(lab, 'sequence: hypergeom -> randomization -> fdr_adjust -> score', seq(calls))


# ------------------------------------------------------------------------------------------------------- case 4 ----

@pytest.mark.parametrize('entry,kind,env', [('randomization', 'bin', {}), ('permtest_counts', 'q_narrow', {'F': 'mfma'}),
                                            ('hypergeom', 'dense', {}), ('score', 'bin', {})],
                         ids=['randomization-bits', 'permtest_counts-mfma', 'hypergeom-split', 'score-bits'])
def test_destroy_right_after_the_call(lab, switches, entry, kind, env):
    """attr, perms and nbr handles destroyed as soon as the call has returned, before the consumer reads: the outputs are
    final and nothing of the borrowed tensor is freed."""
    switches(env)
    call = enrich_call(lab, entry, kind, 'sum', own_nbr=True, destroy_after=True)
    run_case(lab, 'destroy after %s-%s' % (entry, kind), call)
    bor_tensor, staging = call.inputs[0]
    bor_tensor.copy_(staging)                                   # the borrowed buffer is still the caller's to use
    lab.torch.cuda.synchronize()
    assert np.array_equal(bits(numpy_of(bor_tensor)), bits(numpy_of(staging)))


# ------------------------------------------------------------------------------------------------------- case 5 ----

def test_handles_made_on_one_stream_used_on_another(lab, switches):
    """Handles created while the context is on the delayed stream s1 -- nbr from dense, attr from device (its producer still
    queued on s1), perms -- then safe_ctx_set_stream(s2) and an enrichment call on s2: safe_ctx_set_stream orders the new
    stream behind the one it leaves."""
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    _, a, b64, n, m = lab.kind('bin')
    bor = Borrowed(lab, b64)
    want = perm_reference(lab, 'bin', 'float64', a, b64, 'sum', False)
    outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(5)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]
    snaps = [torch.empty_like(o) for o in outs]
    s1, s2 = lab.s, lab.s2
    torch.cuda.synchronize()
    handles = []
    try:
        ctx.set_stream(s1.cuda_stream)
        nbr = be.Neighborhoods.from_dense(ctx, a.astype(np.int64))               # (uploads from the host: synchronous)
        handles.append(nbr)
        # a handle kept open: creating it empties the context's cache of a destroyed handle, which the create behind the delay
        # would otherwise free (hipFree waits for the device and would drain s1)
        handles.append(be.Permutations(ctx, n, bor.flags, 1, SEED))
        with torch.cuda.stream(s1):
            poison(bor.tensor)
        delay_done = lab.delay(s1, 10.0)
        with torch.cuda.stream(s1):
            bor.tensor.copy_(bor.staging)
        attr = bor.handle(lab)
        handles.append(attr)
        perms = be.Permutations(ctx, n, bor.flags, NPERM, SEED)
        handles.append(perms)
        assert not delay_done.query(), 'the harness drained s1 before the switch: nothing would be tested'
        ctx.set_stream(s2.cuda_stream)
        switch_pending = not delay_done.query()
        PENDING['stream switch s1 -> s2: set_stream'] = (('safe_ctx_set_stream',), switch_pending)
        assert switch_pending, 'safe_ctx_set_stream waited for the stream it left'
        be.randomization(ctx, nbr, attr, perms, 'sum', 'both', THRESHOLD, [o.data_ptr() for o in outs])
        PENDING['stream switch s1 -> s2: randomization'] = (('safe_randomization',), not delay_done.query())
        with torch.cuda.stream(s2):
            for snap, o in zip(snaps, outs):
                snap.copy_(o)
            for o in outs:
                poison(o)
        s2.synchronize()
        s1.synchronize()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        for h in reversed(handles):
            h.close()
    check_randomization(want, *[numpy_of(x) for x in snaps])


def test_call_on_one_stream_read_on_the_contexts_own(lab):
    """An asynchronous call on the delayed stream s1, then back to the context's own stream and a host-output function
    (safe_memcpy_d2h): it reads the finished result."""
    torch, be, ctx = lab.torch, lab.be, lab.ctx
    n = 400
    xy = np.random.default_rng(6).uniform(size=(n, 2))
    staging = torch.from_numpy(xy).to('cuda')
    t_xy = torch.empty_like(staging)
    dist = torch.empty((n, n), dtype=torch.float64, device='cuda')
    got = np.empty((n, n), dtype=np.float64)
    s1 = lab.s
    torch.cuda.synchronize()
    try:
        ctx.set_stream(s1.cuda_stream)
        with torch.cuda.stream(s1):
            poison(t_xy)
            poison(dist)
        delay_done = lab.delay(s1, 10.0)
        with torch.cuda.stream(s1):
            t_xy.copy_(staging)
        assert not delay_done.query(), 'the harness drained s1 before the call'
        ctx.euclidean_dense(t_xy.data_ptr(), n, 0.1, None, dist.data_ptr())
        pending = not delay_done.query()
        ctx.set_stream(None)
        be.check(be.lib.safe_memcpy_d2h(ctx.handle, C.c_void_p(got.ctypes.data), C.c_void_p(dist.data_ptr()), got.nbytes))
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
    PENDING['stream switch s1 -> own: euclidean_dense_dev, memcpy_d2h'] = (('safe_euclidean_dense_dev', 'safe_ctx_set_stream'), pending)
    assert pending, 'safe_euclidean_dense_dev returned only after the caller\'s stream had drained'
    assert np.array_equal(bits(got), bits(orc.euclidean_distances(xy)))


# ------------------------------------------------------------------------------------------------------- case 6 ----

def test_nes_table_grows_behind_a_call_still_queued_on_the_callers_stream(lab, switches):
    """safe_outputs_from_packed_slabs on a stream the caller passes in while the context stays on its own: the call at
    P = 37 finds its table resident and returns at once, its kernel queued behind the delay; the call straight after it at
    P = 65535 needs a table 1700 times as large, so the context's table buffer is released and allocated anew.  The first
    call's kernel must have read the old table before that happens: both calls' outputs equal the reference bit for bit.
    (The wait for growth of a scratch buffer covers the context's streams only; the caller's stream is the table helper's to
    wait for.)  A context of the test's own: in the shared one an earlier module may have left a table buffer that is
    large enough already.  The counters are those a real run of NPERM = 20 permutations leaves (both fields <= 20, valid
    for either count); the reference is tests/counter_ref.py on the oracle's counts of that run."""
    import counter_ref as cr
    torch, be = lab.torch, lab.be
    _, a, b64, n, m = lab.kind('bin')
    ref = perm_reference(lab, 'bin', 'float64', a, b64, 'sum', False)
    assert not (np.isnan(ref['counts_pos']).any() or np.isnan(ref['counts_neg']).any())
    less, greater = (NPERM - ref['counts_pos']).astype(np.int64), (NPERM - ref['counts_neg']).astype(np.int64)
    counts = (37, 65535)
    want = {P: cr.outputs_from_pairs(less, greater, P, 'both', THRESHOLD) for P in counts}
    tables = {P: cr.nes_table(P) for P in counts}
    ctx = be.Context(0)
    nbr = be.Neighborhoods.from_dense(ctx, a.astype(np.int64))
    attr = be.Attributes.from_host(ctx, b64)
    perms = be.Permutations(ctx, n, (~np.isnan(b64)).any(axis=1).astype(np.uint8), NPERM, SEED)
    s = lab.s
    try:
        scratch = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(5)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]
        be.randomization(ctx, nbr, attr, perms, 'sum', 'both', THRESHOLD, [t.data_ptr() for t in scratch])
        n_pad, m_loc, layout = be.packed_counts_info(ctx)
        assert (layout, m_loc) == (0, m)
        staging = torch.empty(m * n_pad, dtype=torch.int32, device='cuda')
        be.export_packed_counts(ctx, staging.data_ptr(), m * n_pad)
        ctx.sync()
        slab = torch.empty_like(staging)
        outs = {P: [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(4)] for P in counts}
        snaps = {P: [torch.empty_like(o) for o in outs[P]] for P in counts}

        def call(P):
            be.outputs_from_packed_slabs(ctx, nbr, slab.data_ptr(), layout, n_pad, m * n_pad, [m], [0], m, P, 'both', THRESHOLD,
                                         [o.data_ptr() for o in outs[P]], table=tables[P], stream=s.cuda_stream)

        slab.copy_(staging)
        torch.cuda.synchronize()
        call(37)                                       # the quiet way first: the table of P = 37 is resident from here on
        s.synchronize()
        for k, o in zip(cr.NAMES, outs[37]):
            same(numpy_of(o), want[37][k], 'quiet P=37 ' + k)
        with torch.cuda.stream(s):
            for P in counts:
                for o in outs[P]:
                    poison(o)
            poison(slab)
        delay_done = lab.delay(s, 1.0)
        with torch.cuda.stream(s):
            slab.copy_(staging)
        assert not delay_done.query(), 'the harness drained the busy stream before the calls'
        call(37)
        pending = not delay_done.query()
        call(65535)                                    # the table buffer grows here
        with torch.cuda.stream(s):
            for P in counts:
                for snap, o in zip(snaps[P], outs[P]):
                    snap.copy_(o)
                for o in outs[P]:
                    poison(o)
            poison(slab)
        s.synchronize()
    finally:
        torch.cuda.synchronize()
        perms.close()
        attr.close()
        nbr.close()
    PENDING['outputs_from_packed_slabs P=37 then P=65535 (table grows)'] = (('safe_outputs_from_packed_slabs',), pending)
    assert pending, 'safe_outputs_from_packed_slabs with its table resident returned only after the caller\'s stream had drained'
    for P in counts:
        for k, snap in zip(cr.NAMES, snaps[P]):
            same(numpy_of(snap), want[P][k], 'busy P=%d %s' % (P, k))
