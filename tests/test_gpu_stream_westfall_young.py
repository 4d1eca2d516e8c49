"""The two entry points of the max-statistic adjustment that take device pointers (safe_permtest_extremes,
safe_counts_from_extremes) on a busy caller stream with poisoned inputs, with the harness of tests/test_gpu_stream_order.py.
The file sorts behind that one on purpose: the harness takes two more streams from torch's pool and its delay operands, and the
stream-order cases themselves keep the process state they have always run in.

Both entry points read a timing event back, so they return only once the context's stream has drained (the header lists them
with safe_permtest_counts_weighted): what the busy run checks is the START of every call -- each kernel behind the producer of
the inputs -- and the results.  Quiet outputs against tests/maxt_ref.py, busy snapshots bit for bit against the quiet ones.
Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import maxt_ref as mx                             # noqa: E402
import weights_ref as wr                          # noqa: E402

KEY = 0x5AFE0C0DE0000 + 0x3A87


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


@pytest.mark.parametrize('weighted', [False, True])
def test_busy_caller_stream(be, ctx, weighted):
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    nbr = None
    try:
        _, a, b64, n, m = lab.kind('q_small')
        nbr = be.Neighborhoods.from_dense(ctx, a.astype(np.int64))
        indptr, indices = wr.csr_of(a)
        w = None
        if weighted:
            w = 1.0 - np.random.default_rng(11).uniform(size=len(indices))
            nbr.set_weights(w)
        bor = so.Borrowed(lab, b64)
        P = so.NPERM
        # the restatement, once: on the device's own column moments (the contract) and the tables of the key
        quiet_attr = be.Attributes.from_host(ctx, bor.values)
        perms = be.Permutations(ctx, n, bor.flags, P, None, device_key=KEY)
        try:
            mu, q = quiet_attr.column_moments()
            tables = perms.read().astype(np.int64)
        finally:
            perms.close()
            quiet_attr.close()
        loc, scale = mx.row_factors(indptr, indices, bor.flags != 0, int(bor.flags.sum()), w)
        z, live, tmax, tmin, _ = mx.extremes(indptr, indices, w, bor.values, tables, loc, scale, mu, q)

        # ---- safe_permtest_extremes: the borrowed attribute matrix is the poisoned input
        outs = [torch.empty((n, m), dtype=torch.float64, device='cuda'), torch.empty((n, m), dtype=torch.uint8, device='cuda'),
                torch.empty((P, m), dtype=torch.float64, device='cuda'), torch.empty((P, m), dtype=torch.float64, device='cuda')]
        ptrs = [o.data_ptr() for o in outs]
        state = {'attr': bor.handle(lab), 'perms': None, 'old': []}

        def late():
            if state['perms'] is None or state.get('ran'):
                if state['perms'] is not None:
                    state['old'].append(state['perms'])           # (stays open until done(): see so.enrich_call)
                state['perms'] = be.Permutations(ctx, n, bor.flags, P, None, device_key=KEY)

        def fn():
            state['ran'] = True
            be.permtest_extremes(ctx, nbr, state['attr'], state['perms'], *ptrs)

        def done():
            for h in [state['attr'], state['perms']] + state['old']:
                if h is not None:
                    h.close()

        def check(got):
            assert np.array_equal(so.bits(got[0]), so.bits(z)), 'z'
            assert np.array_equal(got[1], live.astype(np.uint8)), 'live'
            assert np.array_equal(so.bits(got[2]), so.bits(tmax)) and np.array_equal(so.bits(got[3]), so.bits(tmin)), 'extremes'

        call = so.Call(['safe_permtest_extremes'], [(bor.tensor, bor.staging)], outs, fn, check, late=late, done=done)
        try:
            quiet, t_call_ms = so.run_quiet(lab, call)
            check(quiet)
            busy, _ = so.run_busy(lab, call, t_call_ms)
            for i, (x, y) in enumerate(zip(quiet, busy)):
                assert np.array_equal(so.bits(y), so.bits(x)), 'extremes: output %d of the busy run differs from the quiet run' % i
            check(busy)
        finally:
            done()

        # ---- safe_counts_from_extremes: z, the flags and the extremes are the poisoned inputs
        for scope, code in (('neighborhoods', mx.COLUMN), ('all', mx.MATRIX)):
            staged = [torch.from_numpy(np.ascontiguousarray(x)).to('cuda') for x in (z, live.astype(np.uint8), tmax, tmin)]
            inputs = [(torch.empty_like(s), s) for s in staged]
            outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(2)] + \
                   [torch.empty((m,), dtype=torch.float64, device='cuda') for _ in range(2)]
            want = mx.counts(z, live, tmax, tmin, code)

            def fn_counts(scope=scope, inputs=inputs, outs=outs):
                be.counts_from_extremes(ctx, n, m, P, scope, *[t.data_ptr() for t, _ in inputs], *[o.data_ptr() for o in outs])

            def check_counts(got, want=want):
                for g, x in zip(got, want):
                    assert np.array_equal(g, x), scope

            call = so.Call(['safe_counts_from_extremes'], inputs, outs, fn_counts, check_counts)
            quiet, t_call_ms = so.run_quiet(lab, call)
            check_counts(quiet)
            busy, _ = so.run_busy(lab, call, t_call_ms)
            for i, (x, y) in enumerate(zip(quiet, busy)):
                assert np.array_equal(so.bits(y), so.bits(x)), 'counts: output %d of the busy run differs from the quiet run' % i
            check_counts(busy)
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        if nbr is not None:
            nbr.close()
        lab.close()
