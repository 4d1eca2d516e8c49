"""safe_nbr_diffusion on a busy caller stream, with the harness of tests/test_gpu_stream_order.py.  The file sorts behind that one
and its siblings on purpose: the harness takes two more streams from torch's pool and its delay operands, and the stream-order
cases themselves keep the process state they have always run in.

The entry point takes host arrays and returns a handle, so there is no device input to poison; what the busy run checks is that
every kernel of the call runs on the caller's stream behind the delay, that the call is synchronous on that stream (the header
says so: it returns K and a finished handle), and that the membership a consumer then reads on the same stream -- the one device
output, safe_nbr_to_dense_i64_dev into a poisoned tensor -- and the host results equal the quiet run's bit for bit and the NumPy
restatement (tests/diffusion_ref.py).  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import diffusion_ref as dr                        # noqa: E402


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
    n, restart, steps, cutoff = 257, 0.5, 8, 0.9
    eu, ev, w = dr.awkward_graph(n, 9)
    k = dr.kernel(n, eu, ev, w, restart, steps)
    d = dr.distance(k)
    lab = so.Lab(be, ctx, torch)
    mask = torch.empty((n, n), dtype=torch.int64, device='cuda')
    state = {'handles': [], 'host': []}

    def fn():
        nbr, got = be.Neighborhoods.diffusion(ctx, n, eu, ev, w, restart, steps, cutoff, want_kernel=True)
        state['handles'].append(nbr)                                  # (closed in the end: a hipFree would drain the stream)
        state['drained'] = lab.delay_done.query() if state.get('busy') else None
        nbr.to_dense_dev(mask.data_ptr())
        state['host'].append((got, nbr.distances()))

    def check(outs):
        assert np.array_equal(outs[0], dr.members(d, cutoff))
        got, dist = state['host'][-1]
        assert np.array_equal(so.bits(got), so.bits(k)) and np.array_equal(so.bits(dist), so.bits(dr.kept(d, cutoff)))

    call = so.Call(['safe_nbr_diffusion', 'safe_nbr_to_dense_i64_dev'], [], [mask], fn, check)
    try:
        quiet, t_call_ms = so.run_quiet(lab, call)
        check(quiet)
        state['busy'] = True
        busy, _ = so.run_busy(lab, call, t_call_ms)
        assert state['drained'] is True, 'safe_nbr_diffusion returned before the caller\'s stream had drained'
        assert np.array_equal(so.bits(busy[0]), so.bits(quiet[0]))
        check(busy)
        for (k0, d0), (k1, d1) in zip(state['host'][:-1], state['host'][1:]):
            assert np.array_equal(so.bits(k0), so.bits(k1)) and np.array_equal(so.bits(d0), so.bits(d1))
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        for nbr in state['handles']:
            nbr.close()
        lab.close()
