"""The weighted entry points that take device pointers (safe_score_weighted, safe_moments_test_weighted,
safe_permtest_counts_weighted) on a busy caller stream with poisoned inputs, with the harness of
tests/test_gpu_stream_order.py.  The file sorts behind that one on purpose: the harness takes two more streams from torch's
pool and its delay operands, and the stream-order cases themselves keep the process state they have always run in.

The three entry points read a timing event back, so they return only once the context's stream has drained (the header lists
them with safe_score and safe_moments_test): what the busy run checks is the START of every call -- each kernel behind the
producer of the inputs -- and the results.  Quiet outputs against tests/weights_ref.py, busy snapshots bit for bit against the
quiet ones.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import moments_ref as mr                          # noqa: E402
import weights_ref as wr                          # noqa: E402

KEY = 0x5AFE0C0DE0000 + 0xD157


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


def test_busy_caller_stream(be, ctx):
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    nbr = None
    try:
        _, a, b64, n, m = lab.kind('q_small')
        nbr = be.Neighborhoods.from_dense(ctx, a.astype(np.int64))
        indptr, indices = wr.csr_of(a)
        w = 1.0 - np.random.default_rng(11).uniform(size=len(indices))
        nbr.set_weights(w)
        for entry in ('score', 'moments', 'counts'):
            bor = so.Borrowed(lab, b64)
            shapes = {'score': [(n, m)], 'moments': [(n, m)] * 5 + [(m,), (n, m)], 'counts': [(n, m)] * 3}[entry]
            outs = [torch.empty(shape, dtype=torch.float64, device='cuda') for shape in shapes]
            ptrs = [o.data_ptr() for o in outs]
            state = {'attr': bor.handle(lab), 'perms': None, 'old': []}

            def late(state=state, entry=entry, bor=bor):
                if entry == 'counts' and (state['perms'] is None or state.get('ran')):
                    if state['perms'] is not None:
                        state['old'].append(state['perms'])   # (stays open until done(): see so.enrich_call)
                    state['perms'] = be.Permutations(ctx, n, bor.flags, so.NPERM, None, device_key=KEY)

            def fn(state=state, entry=entry, ptrs=ptrs):
                state['ran'] = True
                if entry == 'score':
                    be.score_weighted(ctx, nbr, state['attr'], ptrs[0])
                elif entry == 'moments':
                    be.moments_test_weighted(ctx, nbr, state['attr'], 'both', so.THRESHOLD, ptrs[:6], z_ptr=ptrs[6])
                else:
                    be.permtest_counts_weighted(ctx, nbr, state['attr'], state['perms'], *ptrs)

            def done(state=state):
                for h in [state['attr'], state['perms']] + state['old']:
                    if h is not None:
                        h.close()

            def check(got, state=state, entry=entry, bor=bor):
                x = wr.score(indptr, indices, w, bor.values)
                assert np.array_equal(got[0], x), entry + ': ns'
                if entry == 'moments':
                    pp, pn, nes = got[2], got[1], got[3]
                    assert np.array_equal(got[4], mr.decisions(pp, pn, nes, 'both', so.THRESHOLD))
                    assert np.array_equal(got[5], got[4].sum(axis=0)) and not np.isnan(got[6]).any()
                if entry == 'counts':
                    tables = state['perms'].read().astype(np.int64)
                    _, neg, pos = wr.counts(indptr, indices, w, bor.values, tables)
                    assert np.array_equal(got[1], neg) and np.array_equal(got[2], pos)

            call = so.Call(['safe_%s_weighted' % entry], [(bor.tensor, bor.staging)], outs, fn, check, late=late, done=done)
            try:
                quiet, t_call_ms = so.run_quiet(lab, call)
                check(quiet)
                busy, _ = so.run_busy(lab, call, t_call_ms)
                for i, (q, b) in enumerate(zip(quiet, busy)):
                    assert np.array_equal(so.bits(b), so.bits(q)), '%s: output %d of the busy run differs from the quiet run' % (entry, i)
                check(busy)                               # ('counts': the busy run's new handle has the same key, the same tables)
            finally:
                done()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        if nbr is not None:
            nbr.close()
        lab.close()
