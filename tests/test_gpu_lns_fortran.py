"""The strong-form operator L through the Fortran 2008 shim (neklab_amd/fortran: apply_L, apply_Lv, compute_LNS_conv,
compute_LNS_laplacian, compute_LNS_gradp, set_lns_baseflow, lns_linop, nek_otd%matvec / rmatvec, apply_exptA; driver and Makefile:
tests/fortran_lns) against the Python calls on the same inputs: the same C calls are behind both, so 1e-12 x scale is a loose bound
and the largest difference seen is printed."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import floquet_ref as fr
import otd_ref
from neklab_amd import host
from oracle.vectors import NekDVector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "tests", "fortran_lns")
EXE = os.path.join(FDIR, "_build", "lns_driver")

pytestmark = pytest.mark.gpu

R, NSTEPS = 2, 3


def inputs():
    hm, sem = fr.case_mesh("A")
    rng = np.random.default_rng(11)
    vin = NekDVector(sem)
    for k in range(2):
        vin.v[k][...] = rng.standard_normal(sem.shape1)
    vin.pr[...] = rng.standard_normal(sem.shape2)
    return hm, sem, fr.orbit_state("A"), vin, otd_ref.orthonormal_basis(sem, R)


def write_case(tmp, hm, kw, base, vin, basis):
    with open(os.path.join(tmp, "case.bin"), "wb") as f:
        np.array([2, hm.n, hm.E, R, NSTEPS], dtype=np.int32).tofile(f)
        np.array([kw["re"], kw["dt"], kw["vtol"], kw["ptol"], kw["tau"]], dtype=np.float64).tofile(f)
        for a in (hm.x, hm.y):
            a.astype(np.float64).tofile(f)
        hm.glo_num.astype(np.int64).tofile(f)
        for v in [None, base, vin] + list(basis):
            for a in ((hm.mask[0], hm.mask[1]) if v is None else (v.v[0], v.v[1], v.pr)):
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def test_fortran_names_match_the_python_calls(gpu_ctx):
    subprocess.run(["make", "-s", "-C", FDIR], check=True)
    hm, sem, base, vin, basis = inputs()
    kw = fr.case_cfg("A")
    tmp = tempfile.mkdtemp()
    write_case(tmp, hm, kw, base, vin, basis)
    r = subprocess.run([EXE], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    got = np.fromfile(os.path.join(tmp, "out.bin")).reshape(14, 2, -1)

    gm = host.Mesh(gpu_ctx, hm)

    def up(ov):
        gv = host.nek_dvector(gm)
        for k in range(2):
            gv.set_field(k, ov.v[k])
        gv.set_field(host.PR, ov.pr)
        return gv

    gbase, gin, out = up(base), up(vin), host.nek_dvector(gm)
    ref = []
    L = host.lns_linop(gbase, kw["re"])
    for fn, trans in ((host.apply_L, (False, True)), (host.apply_Lv, (False, True)), (host.compute_LNS_conv, (False, True))):
        for t in trans:
            fn(L, gin, out, t)
            ref.append([out.get_field(k) for k in range(2)])
    for fn in (host.compute_LNS_laplacian, host.compute_LNS_gradp):
        fn(L, gin, out)
        ref.append([out.get_field(k) for k in range(2)])
    for mv in (L.matvec, L.rmatvec):
        mv(gin, out)
        ref.append([out.get_field(k) for k in range(2)])
    L.close()
    O = host.nek_otd(gbase, R, pprecond=1, pproj=0, **kw)
    O.init(host.otd_opts(solve_baseflow=True, orthostep=2), basis0=[up(b) for b in basis])
    O.advance(NSTEPS)
    for mv in (O.matvec, O.rmatvec):
        mv(gin, out)
        ref.append([out.get_field(k) for k in range(2)])
    O.close()
    cfg = dict(kw, pprecond=1, pproj=0)
    cfg.pop("tau")
    A = host.exptA_linop(1.0, gbase, **cfg)
    A.init()
    A.tau = kw["tau"]
    for mv in (A.matvec, A.rmatvec):
        mv(gin, out)
        ref.append([out.get_field(k) for k in range(2)])
    A.close()
    names = ["apply_L", "apply_L trans", "apply_Lv", "apply_Lv trans", "compute_LNS_conv", "compute_LNS_conv trans", "compute_LNS_laplacian",
             "compute_LNS_gradp", "lns_linop%matvec", "lns_linop%rmatvec", "nek_otd%matvec", "nek_otd%rmatvec", "apply_exptA", "apply_exptA trans"]
    assert len(ref) == 14
    worst = 0.0
    for name, g, rf in zip(names, got, ref):
        scale = max(np.abs(a).max() for a in rf)
        err = max(np.abs(a - b).max() for a, b in zip(g, rf))
        print("%-24s scale %.3e, difference / scale %.3e" % (name, scale, err / scale))
        worst = max(worst, err / scale)
        assert scale > 0 and err <= 1e-12 * scale, name
    print("largest difference / scale: %.3e" % worst)
    # the pieces are different fields: no record is a copy of another
    # (lns_linop%matvec / rmatvec repeat apply_L; nek_otd's are about the base flow its run has moved)
    assert len({a[0].tobytes() for a in got}) == 12
    # an array routine before set_lns_baseflow stops with a message that names it
    r = subprocess.run([EXE, "nobase"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "set_lns_baseflow" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
