"""The pressure operator at lx1 = 8 on the matrix pipe (csrc/sem.hip k_opgradt3m8 / k_opdiv3m8): single-vector launches on meshes of at least
NLG_SMALL_E elements.  NLG_POP_MFMA=0 keeps the vector kernels k_opgradt3n / k_opdiv3n; the switches are read once, hence one fresh process
per setting.  Every child sets NLG_SMALL_E=0, so that a handful of elements reach the kernels of the headline size.  The kernels have no
element-count tail (one block per element); the meshes cover the slot tables, the mask bytes and faces without neighbours.
k_opdiv3m8 exists for the face-grouped layout with the compact weights only (the natural-layout launches of nlg_op_opdiv keep k_opdiv3n, which
measured faster there): nlg_op_cdabdtp and the pressure solves of a matvec are the calls that reach it."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MESHES = {
    "walls": ((2, 2, 2), dict(periodic=(True, False, False))),   # every face orientation has a neighbour, the masks are not trivial
    "self": ((3, 1, 2), dict(periodic=(False, True, False))),    # an element is its own neighbour
    "outflow": ((3, 2, 1), dict(outflow_xmax=True)),
    "one": ((1, 1, 1), dict()),
}
SWITCHES = ("NLG_POP_MFMA", "NLG_OPDIV_MASKB", "NLG_SMALL_E", "NLG_PCG_STORE_Z", "NLG_PCG_DEFER_X", "NLG_PCG_DEFER_XP", "NLG_PCG_SINGLE_RED")


def make_mesh(kind, n=8):
    nel, kw = MESHES[kind]
    return box_mesh(nel, n, deform=0.05, **kw)


def inputs(hm):
    rng = np.random.default_rng(77)
    n2 = hm.n - 2
    return [rng.standard_normal(hm.x.shape) for _ in range(hm.dim)], rng.standard_normal(hm.E * n2 ** hm.dim)


CHILD = r'''
import json, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
from neklab_amd.mesh import box_mesh
import test_gpu_pop_mfma as T
mode, path = sys.argv[1], sys.argv[2]
ctx = host.Context(0); lib = ctx.lib
out = {}
if mode == "ops":       # D u and D^T p on every mesh
    for kind in T.MESHES:
        hm = T.make_mesh(kind); gm = host.Mesh(ctx, hm)
        out["pop_" + kind] = gm.pop_mfma()
        u, p = T.inputs(hm)
        vin, vout = host.nek_dvector(gm), host.nek_dvector(gm)
        for i in range(3): vin.set_field(i, u[i])
        vin.set_field(host.PR, p)
        host.check(lib.nlg_op_opdiv(gm.h, vin.h, vout.h)); out["opdiv_" + kind] = vout.get_field(host.PR).copy()
        host.check(lib.nlg_op_opgradt(gm.h, vin.h, vout.h)); out["opgradt_" + kind] = np.stack([vout.get_field(i) for i in range(3)])
        host.check(lib.nlg_op_cdabdtp(gm.h, vin.h, vout.h)); out["cdabdtp_" + kind] = vout.get_field(host.PR).copy()
elif mode == "mv":      # one matvec of the time stepper in tolerance mode
    hm = T.make_mesh("walls"); gm = host.Mesh(ctx, hm)
    out["pop"] = gm.pop_mfma()
    gb = host.nek_dvector(gm)
    gb.set_field(0, hm.mask[0] * (1.0 + 0.5 * np.sin(hm.x) * np.cos(hm.y))); gb.set_field(1, hm.mask[1] * 0.3 * np.sin(2 * hm.x))
    A = host.exptA_linop(0.02, gb, re=40.0, dt=0.01, torder=3, vtol=1e-12, ptol=1e-11, maxit_v=400, maxit_p=4000); A.init()
    x = host.nek_dvector(gm); x.rand(True, seed=40)
    y = host.nek_dvector(gm)
    A.matvec(x, y)
    st = A.stats()
    out["stats"] = np.array([st["steps"], st["v_iters"], st["p_iters"]])
    out["nrst"] = y.nrst
    for irst in range(y.nrst + 1):
        for f in (0, 1, 2, host.PR):
            out["f%%d_%%d" %% (irst, f)] = np.array(y.get_field(f, irst))
elif mode == "path":    # which meshes take the matrix-pipe kernels
    for tag, nel, n, kw in (("n8", (2, 2, 2), 8, dict(periodic=(True, False, False))), ("n10", (2, 2, 1), 10, dict(periodic=(True, False, False))),
                            ("2d", (3, 2), 8, dict(periodic=(True, False)))):
        out["pop_" + tag] = host.Mesh(ctx, box_mesh(nel, n, deform=0.05, **kw)).pop_mfma()
np.savez(path, **out)
print("CHILD OK")
''' % dict(root=ROOT, here=os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def run_child(mode, env_extra):
    key = (mode, tuple(sorted(env_extra.items())))
    if key not in _cache:
        env = dict(os.environ)
        for k in SWITCHES:
            env.pop(k, None)
        env.update(env_extra)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "out.npz")
            r = subprocess.run([sys.executable, "-c", CHILD, mode, path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
            assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            _cache[key] = dict(np.load(path))
    return _cache[key]


MFMA = {"NLG_SMALL_E": "0"}
VECTOR = {"NLG_SMALL_E": "0", "NLG_POP_MFMA": "0"}


def relerr(a, b):
    return float(np.max(np.abs(np.ravel(a) - np.ravel(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("kind", list(MESHES))
def test_against_oracle(kind):
    got = run_child("ops", MFMA)
    assert int(got["pop_" + kind]) == 1
    hm = make_mesh(kind)
    sem = SEM(hm)
    u, p = inputs(hm)
    e_div = relerr(got["opdiv_" + kind], sem.opdiv(u))
    e_grad = relerr(got["opgradt_" + kind], np.stack([a.reshape(hm.E, -1) for a in sem.opgradt(p)]))
    e_e = relerr(got["cdabdtp_" + kind], sem.cdabdtp(p))      # face-grouped gradient, gather-scatter, face-grouped weighted divergence
    print(kind, "opdiv %.2e opgradt %.2e cdabdtp %.2e" % (e_div, e_grad, e_e))
    assert e_div <= 1e-13 and e_grad <= 1e-13
    assert e_e <= 1e-12       # the bound test_gpu_pprec_oracle.py holds the composed operator of the vector kernels to


@pytest.mark.parametrize("kind", list(MESHES))
def test_against_vector_kernels(kind):
    a, b = run_child("ops", MFMA), run_child("ops", VECTOR)
    assert (int(a["pop_" + kind]), int(b["pop_" + kind])) == (1, 0), "the two runs took the same path"
    e_div, e_grad = relerr(a["opdiv_" + kind], b["opdiv_" + kind]), relerr(a["opgradt_" + kind], b["opgradt_" + kind])
    e_e = relerr(a["cdabdtp_" + kind], b["cdabdtp_" + kind])
    print(kind, "opdiv %.2e opgradt %.2e cdabdtp %.2e" % (e_div, e_grad, e_e))
    assert e_div <= 1e-13 and e_grad <= 1e-13 and e_e <= 1e-12


def test_adjoint_on_the_device():
    got = run_child("ops", MFMA)
    hm = make_mesh("walls")
    u, p = inputs(hm)
    du, dtp = got["opdiv_walls"].ravel(), got["opgradt_walls"]
    lhs = float(p @ du)
    rhs = float(sum(dtp[i].ravel() @ u[i].ravel() for i in range(3)))
    bound = 1e-13 * np.linalg.norm(p) * np.linalg.norm(du)
    print("(p, D u) %.15e (D^T p, u) %.15e difference %.2e bound %.2e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


# the fused direction update, the face-grouped layout and the (p, E p) sums: the pressure solves of a matvec
@pytest.mark.parametrize("other", [VECTOR, {"NLG_SMALL_E": "0", "NLG_OPDIV_MASKB": "0"}], ids=["vector", "maskb0"])
def test_inside_the_solver(other):
    a, b = run_child("mv", MFMA), run_child("mv", other)
    assert int(a["pop"]) == 1
    if "NLG_POP_MFMA" in other:
        assert int(b["pop"]) == 0, "the two runs took the same path"
    sa, sb = a["stats"], b["stats"]
    print("steps / v_iters / p_iters", sa, sb, "path", int(a["pop"]), int(b["pop"]))
    assert sa[0] == sb[0] and sa[1] == sb[1], (sa, sb)
    assert abs(int(sa[2]) - int(sb[2])) <= 2, (sa, sb)
    nrst = int(a["nrst"])
    assert nrst == 2 and int(b["nrst"]) == 2      # the output and its two history blocks
    worst = 0.0
    for irst in range(nrst + 1):
        for f in (0, 1, 2, host.PR):
            k = "f%d_%d" % (irst, f)
            x, y = a[k], b[k]
            sc = np.abs(y).max()
            if sc == 0.0:
                assert np.abs(x).max() == 0.0, k
                continue
            e = float(np.abs(x - y).max() / sc)
            worst = max(worst, e)
            assert e <= 1e-10, (k, e)
    print("largest relative difference %.2e" % worst)


def test_path_taken():
    big = run_child("path", MFMA)
    assert (int(big["pop_n8"]), int(big["pop_n10"]), int(big["pop_2d"])) == (1, 0, 0)
    assert int(run_child("path", {})["pop_n8"]) == 0                  # eight elements are a small mesh by default
    assert int(run_child("ops", VECTOR)["pop_walls"]) == 0
