"""CPU suite: the properties of the OTD twin (tests/otd_ref.py) that tests/test_gpu_otd.py leans on, shown on the oracle first.
Case A of tests/floquet_ref.py: 2-D walled box, 3 x 3 elements, lx1 = 6, Re = 50, dt = 0.01, solves converged to 1e-13."""
import numpy as np
import pytest

import floquet_ref as fr
import otd_ref
from oracle import krylov
from oracle.lns import ExptA, LNSConfig

KA, leading = otd_ref.KA, otd_ref.leading


def ka_setup():
    hm, sem = fr.case_mesh("A")
    cfg = LNSConfig(**fr.case_cfg("A", re=KA["re"], dt=KA["dt"], tau=KA["tau"]))
    return sem, cfg, fr.orbit_state("A", KA["amp"])


def test_transform_orthonormalises_to_rounding():
    hm, sem = fr.case_mesh("A")
    cfg = LNSConfig(**fr.case_cfg("A"))
    rng = np.random.default_rng(5)
    B = otd_ref.orthonormal_basis(sem, 3)
    M = np.eye(3) + 0.4 * rng.standard_normal((3, 3))        # far from orthonormal
    B2 = []
    for j in range(3):
        v = B[0].copy()
        v.scal(M[0, j])
        for i in (1, 2):
            v.axpby(M[i, j], B[i], 1.0)
        B2.append(v)
    R = otd_ref.OTDRef(sem, cfg, fr.orbit_state("A"), B2, orthostep=2)
    assert np.abs(R.G0 - M.T @ M).max() < 1e-13
    assert np.abs(R.gram() - np.eye(3)).max() <= 1e-13
    R.advance(3)
    Lr, G = R.reduced()
    assert np.abs(R.gram() - np.eye(3)).max() <= 1e-13
    # the forcing keeps C + C^T = Lr + Lr^T: orthonormality drifts only at the order of the time scheme
    C = R.forcing_matrix(Lr)
    assert np.abs((C + C.T) - (Lr + Lr.T)).max() < 1e-12 * np.abs(Lr).max() and np.allclose(np.tril(C, -1), 0.0)


def test_modes_are_nested():
    """the first mode of an r = 3 run is the r = 1 run, the first two the r = 2 run (6 steps, orthostep = 2)"""
    hm, sem = fr.case_mesh("A")
    cfg = LNSConfig(**fr.case_cfg("A"))
    X0, B = fr.orbit_state("A"), otd_ref.orthonormal_basis(sem, 3)
    runs = {}
    for r in (1, 2, 3):
        runs[r] = otd_ref.OTDRef(sem, cfg, X0, B[:r], orthostep=2)
        runs[r].advance(6)
    e = [fr.vec_err(runs[3].basis(0), runs[1].basis(0)), fr.vec_err(runs[3].basis(0), runs[2].basis(0)),
         fr.vec_err(runs[3].basis(1), runs[2].basis(1))]
    print("nestedness on the twin:", e)
    assert max(e) <= 1e-13
    assert fr.vec_err(runs[3].basis(1), runs[3].basis(0)) > 0.1          # (the modes are not all the same vector)


@pytest.mark.slow
def test_leading_eigenvalue_of_Lr_converges_to_the_propagators():
    """The leading eigenvalue of Lr against log(mu_1) / tau of oracle.krylov.eigs on the frozen propagator of the same configuration.
    Measured (twin): step 0: 1.15e+2; 80 steps: 9.05e-3; 81: 8.20e-3; 82: 7.43e-3; 90: 3.31e-3; 100: 9.8e-4; 150: 7.83e-4, where it stays: the O(dt^3) gap
    between a Rayleigh quotient of L and the discrete eigenvalue of the bdf3 propagator (|lambda| (|lambda| dt)^3 = 7.5e-4 at
    lambda = -5.2459).  Tolerance 10 x that floor = 7.8e-3; 82 is the smallest step count at which the twin is inside it."""
    sem, cfg, X0 = ka_setup()
    mu = krylov.eigs(ExptA(sem, X0.v, cfg).matvec, fr.start_vector(sem), 2, 24, tol=1e-10)[0]
    lam_ref = np.log(complex(mu[0])) / cfg.tau
    R = otd_ref.OTDRef(sem, cfg, X0, otd_ref.orthonormal_basis(sem, KA["r"]), orthostep=10)
    d0 = abs(leading(R.reduced()[0]) - lam_ref)
    R.advance(KA["nsteps"])
    d = abs(leading(R.reduced()[0]) - lam_ref)
    print("lambda_ref %s, |lambda_1(Lr) - lambda_ref|: step 0 %.3e, step %d %.3e" % (lam_ref, d0, KA["nsteps"], d))
    assert d <= KA["tol"]
    assert d0 > 100.0 * KA["tol"]
