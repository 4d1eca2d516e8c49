"""A stratified permutation handle (safe_perms_create_device_strata) on a busy caller stream, with the harness of
tests/test_gpu_stream_order.py.  The file sorts behind that one on purpose: the harness takes two more streams from torch's
pool and its delay operands, and the stream-order cases themselves keep the process state they have always run in.
Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)
import strata_ref as sr                           # noqa: E402

KEY = 0x5AFE0C0DE0000 + 0xB0C7


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
    """The pattern of tests/test_gpu_stream_order.py: the permutation test on the caller's busy stream with poisoned inputs,
    the stratified tables created behind the delay (their generation is still queued when the call is made); the busy run's
    outputs bit for bit against the quiet run's, the quiet run's against a NumPy evaluation of the restated tables."""
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    try:
        nbr, a, b64, n, m = lab.kind('q_small')
        bor = so.Borrowed(lab, b64)
        labels = (np.random.default_rng(5).integers(0, 6, size=n) * 11).astype(np.int32)
        state = {'attr': bor.handle(lab), 'perms': None, 'old': []}
        outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(3)]

        def new_perms():                              # (earlier handles stay open until done(): see so.enrich_call)
            if state['perms'] is not None:
                state['old'].append(state['perms'])
            state['perms'] = be.Permutations.stratified(ctx, n, bor.flags, labels, so.NPERM, KEY)

        def late():
            if state['perms'] is None or state.get('ran'):
                new_perms()

        def fn():
            state['ran'] = True
            be.permtest_counts(ctx, nbr, state['attr'], state['perms'], 'sum', *[o.data_ptr() for o in outs])

        def done():
            for h in [state['attr'], state['perms']] + state['old']:
                if h is not None:
                    h.close()

        def check(got):
            b = bor.values
            ns = orc.compute_neighborhood_score(a, b, 'sum')
            cn, cp = np.zeros(ns.shape), np.zeros(ns.shape)
            with np.errstate(invalid='ignore'):
                for row in sr.strata_tables(n, bor.flags, labels, so.NPERM, KEY):
                    sc = orc.compute_neighborhood_score(a, b[row], 'sum')
                    cn += sc <= ns
                    cp += sc >= ns
            so.close(got[0], ns, 1e-9, 1e-12, 'ns')
            so.same(got[1], cn, 'counts_neg')
            so.same(got[2], cp, 'counts_pos')

        call = so.Call(['safe_permtest_counts'], [(bor.tensor, bor.staging)], outs, fn, check, late=late, done=done)
        so.run_case(lab, 'permtest_counts-strata-after', call)
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        lab.close()
