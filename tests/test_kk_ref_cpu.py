"""tests/kk_ref.py against the real thing: networkx 3.4.2's _kamada_kawai_costfn on the bits of cost and gradient, and
nx.kamada_kawai_layout's L-BFGS-B run reproduced with the restatement as the cost function.  No device."""
import numpy as np
import pytest

import kk_ref

nx = pytest.importorskip('networkx')
from networkx.drawing import layout as nxl   # noqa: E402


def _check(n, eu, ev, ew, tag):
    invdist = kk_ref.invdist_of(kk_ref.nx_dist_mtx(kk_ref.nx_graph(n, eu, ev, ew)))
    for kind in ('circle', 'random'):
        pos = kk_ref.positions(n, kind, seed=n)
        with np.errstate(all='ignore'):
            want_cost, want_grad = nxl._kamada_kawai_costfn(pos.ravel(), np, invdist, 1e-3, 2)
        cost, grad = kk_ref.kk_costfn_ref(pos.ravel(), invdist)
        assert kk_ref.same_bits(np.array([cost]), np.array([want_cost])), (tag, n, kind, cost, want_cost)
        assert kk_ref.same_bits(grad, want_grad), (tag, n, kind)


@pytest.mark.parametrize('n', kk_ref.SIZES)
def test_restatement_equals_networkx_on_a_sparse_graph_with_a_disconnected_part(n):
    eu, ev, ew = kk_ref.sparse_edges(n, seed=100 + n)
    if n >= 3:
        assert (kk_ref.nx_dist_mtx(kk_ref.nx_graph(n, eu, ev)) == kk_ref.UNREACHED).any()
    _check(n, eu, ev, ew, 'sparse')


@pytest.mark.parametrize('n', kk_ref.SIZES)
def test_restatement_equals_networkx_with_non_dyadic_weights(n):
    eu, ev, ew = kk_ref.sparse_edges(n, seed=200 + n, weighted=True)
    _check(n, eu, ev, ew, 'weighted')


def test_restatement_puts_nan_where_networkx_does_for_coincident_nodes():
    n = 9
    eu, ev, ew = kk_ref.sparse_edges(n, seed=5)
    invdist = kk_ref.invdist_of(kk_ref.nx_dist_mtx(kk_ref.nx_graph(n, eu, ev, ew)))
    pos = kk_ref.positions(n, 'random', seed=1)
    pos[4] = pos[2]
    with np.errstate(all='ignore'):
        want_cost, want_grad = nxl._kamada_kawai_costfn(pos.ravel(), np, invdist, 1e-3, 2)
    cost, grad = kk_ref.kk_costfn_ref(pos.ravel(), invdist)
    assert np.isnan(want_grad).any() and not np.isnan(want_grad).all()
    assert kk_ref.same_bits(grad, want_grad) and kk_ref.same_bits(np.array([cost]), np.array([want_cost]))


@pytest.mark.parametrize('n', (130, 300))
def test_minimize_with_the_restatement_gives_networkx_positions(n):
    import scipy.optimize
    eu, ev, ew = kk_ref.sparse_edges(n, seed=300 + n)
    dist_mtx = kk_ref.nx_dist_mtx(kk_ref.nx_graph(n, eu, ev, ew))
    pos0 = kk_ref.positions(n, 'circle')
    want = nxl._kamada_kawai_solve(dist_mtx, pos0.copy(), 2)
    invdist = kk_ref.invdist_of(dist_mtx)
    calls = [0]

    def fun(x):
        calls[0] += 1
        return kk_ref.kk_costfn_ref(x, invdist)

    got = scipy.optimize.minimize(fun, pos0.ravel(), method='L-BFGS-B', jac=True)
    assert calls[0] > 20
    assert np.array_equal(kk_ref.bits(got.x.reshape(-1, 2)), kk_ref.bits(want))
