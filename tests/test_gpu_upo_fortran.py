"""The periodic-orbit Newton through the Fortran 2008 shim (neklab_amd/fortran: nek_ext_dvector, nek_system_upo / nek_jacobian_upo,
gmres_upo; driver and Makefile: tests/fortran_upo), on the manufactured root of tests/test_gpu_upo.py, against the Python driver: the
same C calls in the same order."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import floquet_ref as fr
import upo_ref as ur
from neklab_amd import host
from test_gpu_upo import NEWTON_REF_ITERATIONS, manufactured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "tests", "fortran_upo")

pytestmark = pytest.mark.gpu

OFFSET_TOL = 1e-12


def test_fortran_newton_periodic_orbit_matches_python_driver(gpu_ctx):
    """tests/fortran_upo/upo_driver.f90 runs newton_periodic_orbit's loop on class(abstract_vector_rdp): residuals and periods of
    every iteration agree with the Python driver's to 1e-12 relative; the field file carries the period as its time.
    Residuals of 1e-9 are differences of O(1) fields, so 1e-12 relative needs the same arithmetic operation by operation: the two
    GMRES loops use the same sequential sums and sqrt(a a + b b) on the host, and the driver is built with -ffp-contract=off; the two
    runs are then bitwise equal."""
    subprocess.run(["make", "-s", "-C", FDIR], check=True)
    exe = os.path.join(FDIR, "_build", "upo_driver")
    hm, sem = fr.case_mesh("A")
    kw = fr.tangent_cfg()
    ref, Xs, start = ur.manufactured()
    kdim, maxiter = 60, NEWTON_REF_ITERATIONS + 2
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "case.bin"), "wb") as f:
        np.array([2, hm.n, hm.E, 6, kdim, maxiter], dtype=np.int32).tofile(f)
        np.array([kw["re"], kw["dt"], kw["vtol"], kw["ptol"], ur.NEWTON_TOL, Xs.T, start.T, OFFSET_TOL], dtype=np.float64).tofile(f)
        for a in (hm.x, hm.y):
            a.astype(np.float64).tofile(f)
        hm.glo_num.astype(np.int64).tofile(f)
        for a in (hm.mask[0], hm.mask[1], Xs.vec.v[0], Xs.vec.v[1], Xs.vec.pr, start.vec.v[0], start.vec.v[1], start.vec.pr):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("NEWTON")]
    fres, fper = np.array([float(p[2]) for p in rows]), np.array([float(p[3]) for p in rows])
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.split()}
    # the Python driver on the same inputs
    gm = host.Mesh(gpu_ctx, hm)
    S, _, _, _, X, gXs = manufactured(gm)
    S.set_tolerance(OFFSET_TOL)                                       # the offset with the solves at 0.1 OFFSET_TOL, as the driver's response() does
    off = host.nek_ext_dvector(gm)
    S.eval(gXs, off)
    py = host.newton_periodic_orbit(S, X, ur.NEWTON_TOL, maxiter=maxiter, kdim=kdim, offset=off, fixed_nsteps=6)
    pres, pper = np.array(py["residuals"]), np.array(py["periods"])
    print("Fortran residuals %s periods %s\nPython  residuals %s periods %s" % (fres, fper, pres, pper))
    assert py["converged"] and "CONVERGED" in out and int(out["CONVERGED"][0]) == py["iterations"]
    assert len(fres) == len(pres)
    print("largest relative difference: residuals %.3e, periods %.3e" % (np.max(np.abs(fres - pres) / pres), np.max(np.abs(fper - pper) / pper)))
    assert np.max(np.abs(fres - pres) / pres) <= 1e-12 and np.max(np.abs(fper - pper) / pper) <= 1e-12
    assert int(out["MATVECS"][0]) == py["gmres_matvecs"]
    assert abs(float(out["OFFNORM"][0]) - off.norm()) <= 1e-12 * off.norm()
    assert abs(float(out["PERIOD"][0]) - X.T) <= 1e-12 * X.T
    from neklab_amd import nekio
    fld = nekio.read_fld(os.path.join(tmp, "uponeklab0.f00001"))
    assert abs(fld["time"] - X.T) <= 1e-12 * X.T
    assert np.max(np.abs(fld["ux"].ravel() - X.vec.get_field(0))) <= 1e-12 * np.max(np.abs(X.vec.get_field(0)))
