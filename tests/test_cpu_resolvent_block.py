"""CPU suite of the block resolvent: the new entry point refuses loudly, the least-squares core of the block GMRES solves dense
problems with dependent and zero right-hand sides, and the randomised SVD is exact on a matrix of rank k."""
import ctypes as C

import numpy as np
import pytest

from resolvent_block_ref import DenseResolvent, ZVec, block_arnoldi


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_forced_block_refuses_null(lib):
    from neklab_amd import _lib
    assert len(_lib.SIGNATURES["nlg_linop_integrate_forced_block"][1]) == 8
    rc = lib.nlg_linop_integrate_forced_block(None, 1, None, None, None, 8.0, 0, None)
    assert rc != 0 and b"integrate_forced" in lib.nlg_last_error()


@pytest.mark.parametrize("kind", ["dependent", "zero"])
def test_block_gmres_least_squares(kind):
    """(A - I) X = B through block Arnoldi of A (numpy, with the device's deflation convention) and host._block_gmres_ls: one
    right-hand side a combination of the other two / one zero.  The block Krylov space is run to exhaustion (n = 40), so the
    bound is dense algebra at rounding: 1e-10 relative per column (the zero column: relative to the largest one)."""
    from neklab_amd.host import _block_gmres_ls
    rng = np.random.default_rng(7)
    n, s = 40, 3
    G = rng.standard_normal((n, n))
    A = 0.6 * G / np.linalg.norm(G, 2)                     # non-symmetric contraction: A - I is safely invertible
    B = rng.standard_normal((n, s))
    if kind == "dependent":
        B[:, 2] = 0.7 * B[:, 0] - 1.3 * B[:, 1]
    else:
        B[:, 1] = 0.0
    nsteps = 22                                            # rank-2 blocks fill R^40 after 20 steps
    Q, H, R0 = block_arnoldi(A, B, nsteps)
    assert np.count_nonzero(np.diag(R0)) == 2              # the third direction of the residual block is deflated
    Y, res = _block_gmres_ls(H, R0, s, nsteps, -1.0)
    X = Q[:, :nsteps * s] @ Y
    true = np.linalg.norm((A - np.eye(n)) @ X - B, axis=0)
    bn = np.linalg.norm(B, axis=0)
    for v in range(s):
        ref = bn[v] if bn[v] > 0 else bn.max()
        assert true[v] <= 1e-10 * ref, (v, true[v], ref)
        assert abs(res[v] - true[v]) <= 1e-10 * ref        # the reported residual is the true one
    if kind == "zero":
        assert np.linalg.norm(X[:, 1]) <= 1e-10 * np.linalg.norm(X)
    # and on the way there the reported norms are those of the iterate (orthonormal basis), and they do not grow
    last = np.full(s, np.inf)
    for j in (1, 3, 6):
        Yj, rj = _block_gmres_ls(H, R0, s, j, -1.0)
        tj = np.linalg.norm((A - np.eye(n)) @ (Q[:, :j * s] @ Yj) - B, axis=0)
        assert np.all(np.abs(rj - tj) <= 1e-10 * bn.max()) and np.all(rj <= last + 1e-12)
        last = rj


@pytest.mark.parametrize("q", [0, 1])
def test_resolvent_analysis_exact_at_rank_k(q):
    """A randomised SVD of a rank-k matrix with k samples is exact: sigma to 1e-10 relative, U and V orthonormal to 1e-12,
    R^H U = V Sigma to 1e-10 -- through the duck-typed interface (apply_linear_block, nek_zvector's methods)."""
    from neklab_amd.host import resolvent_analysis
    rng = np.random.default_rng(3)
    n, k = 30, 3
    U0 = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))[0]
    V0 = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))[0]
    s0 = np.array([5.0, 2.0, 0.5])
    M = (U0 * s0) @ V0.conj().T
    R = DenseResolvent(M)
    Omega = [ZVec(rng.standard_normal(n) + 1j * rng.standard_normal(n)) for _ in range(k)]
    keep = [o.a.copy() for o in Omega]
    sigma, U, V = resolvent_analysis(R, k, power_iters=q, Omega=Omega)
    assert R.napply == 2 * q + 2
    assert all(np.array_equal(o.a, a) for o, a in zip(Omega, keep))
    assert np.max(np.abs(sigma - s0) / s0) < 1e-10
    Um, Vm = np.stack([u.a for u in U], 1), np.stack([v.a for v in V], 1)
    assert np.max(np.abs(Um.conj().T @ Um - np.eye(k))) < 1e-12
    assert np.max(np.abs(Vm.conj().T @ Vm - np.eye(k))) < 1e-12
    assert np.max(np.abs(M.conj().T @ Um - Vm * sigma)) < 1e-10 * s0[0]
    # the triplets are those of M: R v_j = sigma_j u_j
    assert np.max(np.abs(M @ Vm - Um * sigma)) < 1e-10 * s0[0]
    with pytest.raises(ValueError):
        resolvent_analysis(R, 5, Omega=Omega)
