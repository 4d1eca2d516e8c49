"""safe_mt_adjust_scope and safe_mt_adjust_matrix on a busy caller stream, with the harness of tests/test_gpu_stream_order.py:
every procedure, every scope, the count and the sort form, on a stream that is still busy producing the (poisoned) inputs.  The
file sorts behind that one on purpose, as tests/test_gpu_stream_strata.py does: the harness takes two more streams from torch's
pool and its delay operands, and the stream-order cases themselves keep the process state they have always run in.
Needs an MI355X."""
import numpy as np
import pytest

import mt_ref as mt

pytestmark = pytest.mark.gpu

FORMS = [('attributes', 100), ('attributes', 0), ('neighborhoods', 100), ('neighborhoods', 0), ('all', 100), ('all', 0)]


def form_inputs(P, n, m):
    rng = np.random.default_rng([71, P, n, m])
    if P:
        return np.floor(P * rng.uniform(size=(2, n, m)) ** 3) / float(P)
    p = np.round(rng.uniform(size=(2, n, m)) ** 3, 4)                 # ties, and no multiples of 1 / 1000: the sort forms
    p[:, 0, 0] = 0.12345
    return p


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


@pytest.mark.parametrize('method', mt.METHODS)
def test_busy_caller_stream(be, ctx, method):
    """The same bits as a quiet run, and the restatement's values."""
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    n, m = 257, 70
    try:
        for scope, P in FORMS:
            host = form_inputs(P, n, m)
            st = [torch.from_numpy(x).to('cuda') for x in host]
            dev = [torch.empty_like(x) for x in st] + [torch.empty_like(st[0])]
            st.append(st[1])                                         # a third matrix for safe_mt_adjust_matrix
            outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(2)] + [torch.empty((m,), dtype=torch.float64, device='cuda')]

            def fn(scope=scope, P=P, dev=dev, outs=outs):
                be.mt_adjust_scope(ctx, n, m, P if P else 1000, 'both', 0.05, scope, method,
                                   [d.data_ptr() for d in dev[:2]] + [o.data_ptr() for o in outs])
                be.mt_adjust_matrix(ctx, n, m, scope, method, dev[2].data_ptr(), count_denominator=P)

            def check(got, scope=scope, host=host):
                assert mt.same_bits(got[0], mt.adjust(host[0], scope, method)) and mt.same_bits(got[1], mt.adjust(host[1], scope, method))
                assert mt.same_bits(got[2], mt.adjust(host[1], scope, method))
                assert np.array_equal(got[5], got[4].sum(axis=0))

            call = so.Call(['safe_mt_adjust_scope', 'safe_mt_adjust_matrix'], list(zip(dev, st)), dev + outs, fn, check)
            quiet, t_call_ms = so.run_quiet(lab, call)
            call.check(quiet)
            busy, _ = so.run_busy(lab, call, t_call_ms)
            for i, (q, v) in enumerate(zip(quiet, busy)):
                assert np.array_equal(so.bits(v), so.bits(q)), '%s %s P=%d: output %d of the busy run differs from the quiet run' % (method, scope, P, i)
            call.check(busy)
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        lab.close()
