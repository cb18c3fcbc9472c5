"""CPU suite: the entry points of the wavenumber sweep are declared, bound and exported, fail loudly on NULL arguments without a
device, and the Ritz helper of the sweep driver follows the rule of `ritz_pairs` in csrc/krylov.hip."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nlg_linop_set_projection_lanes": 7, "nlg_linop_project_block": 3, "nlg_basis_cgs2_batch": 7, "nlg_sweep_arnoldi_step": 8}


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_sweep_symbols_are_declared_bound_and_exported(lib):
    from neklab_amd import _lib
    header = open(os.path.join(ROOT, "include", "neklab_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    capi = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    for nm, nargs in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % nm, header), "header lacks %s" % nm
        assert nm in _lib.SIGNATURES, "ctypes table lacks %s" % nm
        assert hasattr(lib, nm), "library lacks %s" % nm
        assert len(_lib.SIGNATURES[nm][1]) == nargs, nm
        assert 'name="%s"' % nm in capi, "Fortran capi lacks %s" % nm


def test_sweep_entry_points_refuse_null_arguments(lib):
    from neklab_amd import host
    assert issubclass(host.exptA_sweep_linop, host.exptA_proj_linop)
    assert callable(host.linear_stability_analysis_wavenumbers) and callable(host.sweep_arnoldi_step)
    assert lib.nlg_linop_set_projection_lanes(None, 2, None, 1, None, None, None) != 0
    assert b"nlg_linop_set_projection_lanes" in lib.nlg_last_error()
    assert lib.nlg_linop_project_block(None, 1, None) != 0 and b"nlg_linop_project_block" in lib.nlg_last_error()
    assert lib.nlg_basis_cgs2_batch(1, None, 0, None, None, 0, None) != 0 and b"nlg_basis_cgs2_batch" in lib.nlg_last_error()
    assert lib.nlg_sweep_arnoldi_step(None, 1, None, 0, None, 2, 0, 0) != 0 and b"nlg_sweep_arnoldi_step" in lib.nlg_last_error()
    with pytest.raises(host.NlgError, match="nlg_sweep_arnoldi_step"):
        host.check(lib.nlg_sweep_arnoldi_step(None, 1, None, 0, None, 2, 0, 0))


def test_ritz_from_hessenberg_on_a_dense_arnoldi_run():
    from neklab_amd.host import _ritz_from_hessenberg
    rng = np.random.default_rng(7)
    n, m = 30, 30
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    V = np.zeros((n, m + 1))
    H = np.zeros((m + 1, m))
    v = rng.standard_normal(n)
    V[:, 0] = v / np.linalg.norm(v)
    for k in range(m):
        w = A @ V[:, k]
        for _ in range(2):                                    # CGS2
            h = V[:, :k + 1].T @ w
            w -= V[:, :k + 1] @ h
            H[:k + 1, k] += h
        H[k + 1, k] = np.linalg.norm(w)
        if k + 1 < n:
            V[:, k + 1] = w / H[k + 1, k]
    for k in (1, 2, 9, 20, 30):
        lam, Y, res = _ritz_from_hessenberg(H, k)
        ref = np.linalg.eigvals(H[:k, :k])
        assert lam.shape == (k,) and Y.shape == (k, k) and res.shape == (k,)
        assert np.all(np.diff(np.abs(lam)) <= 1e-13)                                      # decreasing modulus (pairs: equal to rounding)
        assert max(np.min(np.abs(ref - l)) for l in lam) < 1e-12 and max(np.min(np.abs(lam - l)) for l in ref) < 1e-12
        assert np.max(np.abs(np.linalg.norm(Y, axis=0) - 1.0)) < 1e-13                     # unit Ritz vectors
        assert np.max(np.abs(H[:k, :k] @ Y - Y * lam)) < 1e-11
        assert np.allclose(res, abs(H[k, k - 1]) * np.abs(Y[k - 1, :]), rtol=0, atol=1e-15)
        # the residual formula is the norm of the true residual of the Ritz pair (A V_k y - lam V_k y = h_{k+1,k} y_k v_{k+1})
        if k < n:
            for j in range(min(k, 3)):
                x = V[:, :k] @ Y[:, j]
                assert abs(np.linalg.norm(A @ x - lam[j] * x) - res[j]) < 1e-10
    # the whole space: the Ritz values are the eigenvalues of A and the residuals vanish with h_{31,30}
    lam, Y, res = _ritz_from_hessenberg(H, 30)
    ref = np.linalg.eigvals(A)
    assert max(np.min(np.abs(ref - l)) for l in lam) < 1e-9
    assert np.max(res) < 1e-9
