"""eigenvalue_sensitivity through the Fortran 2008 shim (neklab_amd/fortran/neklab_analysis.f90; driver and Makefile:
tests/fortran_sens) against the Python call on the same two mode pairs, a complex and a real one: d and the largest modulus of every
field returned agree to 1e-12 relative (the same C calls are behind both)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import floquet_ref as fr
from neklab_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "tests", "fortran_sens")
EXE = os.path.join(FDIR, "_build", "sens_driver")

pytestmark = pytest.mark.gpu


def test_fortran_call_matches_the_python_call(gpu_ctx):
    subprocess.run(["make", "-s", "-C", FDIR], check=True)
    hm, sem = fr.case_mesh("A")
    rng = np.random.default_rng(23)
    fields = [[rng.standard_normal(sem.shape1) for _ in range(2)] for _ in range(6)]
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "case.bin"), "wb") as f:
        np.array([2, hm.n, hm.E], dtype=np.int32).tofile(f)
        for a in (hm.x, hm.y):
            a.astype(np.float64).tofile(f)
        hm.glo_num.astype(np.int64).tofile(f)
        for a in [hm.mask[0], hm.mask[1]] + [c for v in fields for c in v]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([EXE], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    got = {ln.split()[0]: [float(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln[:1] in "DGTW" and ln != "DONE"}

    gm = host.Mesh(gpu_ctx, hm)

    def up(v):
        gv = host.nek_dvector(gm)
        gv.zero()
        for k in range(2):
            gv.set_field(k, v[k])
        return gv

    g = [up(v) for v in fields]
    mx = lambda v: [np.abs(v.get_field(k)).max() for k in range(2)]
    d1, grad1, tr1, w1 = host.eigenvalue_sensitivity((g[0], g[1]), (g[2], g[3]), parts=True)
    d2, grad2, _, _ = host.eigenvalue_sensitivity((g[4], None), (g[5], None), wavemaker=False)
    want = {"D1": [d1.real, d1.imag], "GRE1": mx(grad1[0]), "GIM1": mx(grad1[1]), "TRE1": mx(tr1[0]), "TIM1": mx(tr1[1]), "WMK1": mx(w1),
            "D2": [d2.real, d2.imag], "GRE2": mx(grad2[0]), "GIM2": mx(grad2[1])}
    assert set(got) == set(want), r.stdout
    for key, w in want.items():
        print("%-5s fortran %s python %s" % (key, got[key], w))
        scale = max(abs(x) for x in w)
        assert scale > 0 or key in ("GIM2",)
        for a, b in zip(got[key], w):
            assert abs(a - b) <= 1e-12 * max(scale, 1e-300), key
    assert got["WMK1"][1] == 0.0 and got["D2"][1] == 0.0
