"""Wall forces through the Fortran 2008 shim (neklab_amd/fortran: nek_wall_forces, nek_dns%set_wall_forces; driver and Makefile:
tests/fortran_forces) on case A, against the Python driver host.wall_forces: both make the same C calls, so the sample of the initial
state, the areas and a 3-step force series agree to 1e-12 relative."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import floquet_ref as fr
import forces_ref as fo
from neklab_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "tests", "fortran_forces")

pytestmark = pytest.mark.gpu

NSTEPS = 3
NU = 0.37


def test_fortran_forces_match_python_driver(gpu_ctx):
    subprocess.run(["make", "-s", "-C", FDIR], check=True)
    exe = os.path.join(FDIR, "_build", "forces_driver")
    hm, sem = fr.case_mesh("A")
    kw = fr.case_cfg("A")
    X0 = fr.orbit_state("A")
    X0.pr[...] = np.random.default_rng(5).standard_normal(sem.shape2)      # the pressure part of the sample is not trivially 0
    objects = fo.case_objects("A", hm)
    centres = np.array([[0.5, 0.5], [0.0, 1.0], [-1.0, 0.25]])
    flat = [(e, f, o) for o, faces in enumerate(objects) for e, f in faces]
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "case.bin"), "wb") as f:
        np.array([2, hm.n, hm.E, NSTEPS, len(flat), len(objects)], dtype=np.int32).tofile(f)
        np.array([kw["re"], kw["dt"], kw["vtol"], kw["ptol"], NU], dtype=np.float64).tofile(f)
        for a in (hm.x, hm.y):
            a.astype(np.float64).tofile(f)
        hm.glo_num.astype(np.int64).tofile(f)
        for a in (hm.mask[0], hm.mask[1], X0.v[0], X0.v[1], X0.pr):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        for k, shift in ((0, 1), (1, 0), (2, 1)):                          # elements and objects 1-based, as the shim takes them
            np.array([t[k] + shift for t in flat], dtype=np.int32).tofile(f)
        np.ascontiguousarray(centres, dtype=np.float64).tofile(f)          # centres(ldim, nobj) column-major = [nobj][dim] row-major
    r = subprocess.run([exe], cwd=tmp, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.split()}
    nobj, nq = len(objects), fo.nq(2)
    assert [int(a) for a in out["SHAPE"]] == [NSTEPS + 1, nobj, nq]
    raw = np.fromfile(os.path.join(tmp, "forces.bin"), dtype=np.float64)
    farea, fsample, fseries = raw[:nobj], raw[nobj: nobj + nobj * nq].reshape(nobj, nq), raw[nobj + nobj * nq:].reshape(NSTEPS + 1, nobj, nq)
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = host.nek_dvector(gm)
    for i in range(2):
        gX0.set_field(i, X0.v[i])
    gX0.set_field(host.PR, X0.pr)
    wf = host.wall_forces(gm, objects, centres)
    sample = wf.sample(gX0, NU)
    dns = host.nek_dns(gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    dns.set_wall_forces(wf)
    dns.advance(NSTEPS)
    series = dns.series()["force"]
    es = np.abs(fsample - sample).max() / np.abs(sample).max()
    ef = np.abs(fseries - series).max() / np.abs(series).max()
    print("Fortran against Python: sample %.3e, force series %.3e (relative), areas %s; bit-equal: %s"
          % (es, ef, farea, np.array_equal(fsample, sample) and np.array_equal(fseries, series)))
    assert np.array_equal(farea, wf.area)
    assert es <= 1e-12 and ef <= 1e-12
    dns.close()
    wf.close()
