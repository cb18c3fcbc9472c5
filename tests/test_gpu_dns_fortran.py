"""A DNS run with history points through the Fortran 2008 shim (neklab_amd/fortran: nek_dns; driver and Makefile: tests/fortran_dns) on
case A, against the Python driver host.nek_dns: both make the same C calls in the same order, so the series agree to 1e-12 relative."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dns_ref
import floquet_ref as fr
from neklab_amd import host, nekio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "tests", "fortran_dns")

pytestmark = pytest.mark.gpu

NSTEPS = 5


def test_fortran_dns_matches_python_driver(gpu_ctx):
    subprocess.run(["make", "-s", "-C", FDIR], check=True)
    exe = os.path.join(FDIR, "_build", "dns_driver")
    hm, sem = fr.case_mesh("A")
    kw = fr.case_cfg("A")
    X0 = fr.orbit_state("A")
    xyz = np.array([p[1] for p in dns_ref.case_points("A", hm) if p[2] == 0])
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "case.bin"), "wb") as f:
        np.array([2, hm.n, hm.E, NSTEPS, len(xyz)], dtype=np.int32).tofile(f)
        np.array([kw["re"], kw["dt"], kw["vtol"], kw["ptol"]], dtype=np.float64).tofile(f)
        for a in (hm.x, hm.y):
            a.astype(np.float64).tofile(f)
        hm.glo_num.astype(np.int64).tofile(f)
        for a in (hm.mask[0], hm.mask[1], X0.v[0], X0.v[1], X0.pr, xyz):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe], cwd=tmp, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.split()}
    n, npts, nf = (int(a) for a in out["SHAPE"])
    assert (n, npts, nf) == (NSTEPS + 1, len(xyz), 3)
    raw = np.fromfile(os.path.join(tmp, "series.bin"), dtype=np.float64)
    ftime, fprobe, fdist = raw[:n], raw[n: n + n * npts * nf].reshape(n, npts, nf), raw[n + n * npts * nf:]
    # the Python driver on the same inputs
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = host.nek_dvector(gm)
    for i in range(2):
        gX0.set_field(i, X0.v[i])
    gX0.set_field(host.PR, X0.pr)
    dns = host.nek_dns(gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    hp = host.history_points(gm, xyz)
    dns.set_history_points(hp)
    dns.set_reference()
    dns.advance(NSTEPS)
    s = dns.series()
    sc = np.abs(s["probe"]).max()
    ep, ed = np.abs(fprobe - s["probe"]).max() / sc, np.abs(fdist - s["dist"]).max() / s["dist"].max()
    print("Fortran against Python: history points %.3e, d(t) %.3e (relative); bit-equal: %s"
          % (ep, ed, np.array_equal(fprobe, s["probe"]) and np.array_equal(fdist, s["dist"])))
    assert np.array_equal(ftime, s["time"])
    assert ep <= 1e-12 and ed <= 1e-12
    assert int(out["INFO"][0]) == NSTEPS and abs(float(out["INFO"][2]) - dns.info()["dt"]) <= 1e-15
    assert abs(float(out["NORM"][0]) - dns.state().norm()) <= 1e-12 * dns.state().norm()
    # the text file the driver wrote is the layout nekio reads
    his = nekio.read_his(os.path.join(tmp, "run.his"))
    assert np.allclose(his["xyz"], xyz, rtol=5e-8, atol=1e-300) and np.allclose(his["time"], s["time"], rtol=5e-8, atol=0)
    assert his["probe"].shape == s["probe"].shape and np.allclose(his["probe"], s["probe"], rtol=5e-8, atol=1e-7 * sc)
    dns.close()
    hp.close()
