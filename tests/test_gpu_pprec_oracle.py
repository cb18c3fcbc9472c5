"""The two-level Schwarz pressure preconditioner and the 3-D operators against float64 references, on meshes whose elements
are rotated (tests/rotmesh.py) as well as aligned.

(a) nlg_op_pprec against oracle/pprec.py (a restatement from the definition that shares no table with the device): overlap
    0 / 1 x coarse level 0 / 1; 3-D lx1 = 6, 7, 8, 9, 10, 12 (k_q1_restrict_local3s<6/8/10>, the generic restriction,
    k_fdm_ext<N, ...>, k_fdm_ext_mfma8, k_sch_finish<N>), 2-D lx1 = 6, 8 (10 without overlap); walls, fully periodic,
    periodic one element wide (an element is its own neighbour), an outflow face, E not a multiple of 4; the aggregated
    coarse mode in a child process with a small NLG_COARSE_EXACT_MAX.
(b) equivariance on the GPU itself: on a rotated mesh with the re-indexed input every operator gives the aligned mesh's
    result, re-indexed -- in this process and in a child with NLG_SMALL_E=0 (the one-wave pressure kernels).
(c) the headline instantiations (NLG_SMALL_E=0: k_opgradt3n / k_opdiv3n<8>) against oracle/sem.py, and the fixed-iteration
    matvec of test_gpu_n8.py against the oracle.
(d) pressure iteration counts in tolerance mode with the Schwarz preconditioner against the oracle's PCG with
    oracle/pprec.py: a wrong ghost layer, neighbour length or hat weight leaves M symmetric positive and the answer right,
    and only moves this count.  One lane and a block of four.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.lns import ExptA, LNSConfig
from oracle.pprec import SchwarzPrec
from oracle.sem import SEM
from oracle.vectors import NekDVector

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from rotmesh import Rotated  # noqa: E402

pytestmark = pytest.mark.gpu

# mesh kinds: (nel 3-D, nel 2-D, keyword arguments of box_mesh)
KINDS = {
    "walls": ((3, 2, 2), (4, 3), dict()),
    "periodic": ((3, 3, 2), (3, 3), dict(periodic=(True, True, True))),
    "self": ((3, 1, 2), (3, 1), dict(periodic=(False, True, False))),      # one element wide and periodic in y
    "outflow": ((3, 2, 1), (3, 2), dict(outflow_xmax=True)),
}
CASES3 = [(6, "walls"), (6, "self"), (7, "periodic"), (7, "outflow"), (8, "walls"), (8, "periodic"), (8, "self"), (8, "outflow"),
          (9, "self"), (9, "walls"), (10, "outflow"), (10, "periodic"), (10, "walls"), (12, "walls"), (12, "periodic")]
CASES2 = [(6, "walls"), (6, "self"), (8, "periodic"), (8, "outflow"), (10, "walls"), (10, "periodic")]


def make_mesh(dim, n, kind, rotated, seed=7):
    nel3, nel2, kw = KINDS[kind]
    kw = dict(kw)
    if "periodic" in kw:
        kw["periodic"] = kw["periodic"][:dim]
    hm = box_mesh(nel3 if dim == 3 else nel2, n, deform=0.05, **kw)
    return Rotated(hm, seed=seed).mesh if rotated else hm


def gpu_pprec(ctx, gm, r, overlap, with_coarse):
    vin, vout = host.nek_dvector(gm), host.nek_dvector(gm)
    vin.set_field(host.PR, r)
    host.check(ctx.lib.nlg_op_pprec(gm.h, vin.h, vout.h, overlap, with_coarse))
    return vout.get_field(host.PR).copy()


def relerr(a, b):
    return float(np.max(np.abs(np.ravel(a) - np.ravel(b))) / np.max(np.abs(b)))


def check_against_oracle(ctx, hm, overlaps, tol=1e-12):
    sem = SEM(hm)
    gm = host.Mesh(ctx, hm)
    r = np.random.default_rng(3).standard_normal(gm.lpn)
    worst = 0.0
    for ov in overlaps:
        for wc in (0, 1):
            z = gpu_pprec(ctx, gm, r, ov, wc)
            zo = SchwarzPrec(sem, overlap=ov, with_coarse=wc).apply(r)
            err = relerr(z, zo)
            worst = max(worst, err)
            assert err <= tol, "overlap %d coarse %d: relative error %.3e" % (ov, wc, err)
    return worst


@pytest.mark.parametrize("rotated", [False, True], ids=["aligned", "rotated"])
@pytest.mark.parametrize("n,kind", CASES3, ids=["n%d_%s" % c for c in CASES3])
def test_pprec_3d_matches_oracle(gpu_ctx, n, kind, rotated):
    err = check_against_oracle(gpu_ctx, make_mesh(3, n, kind, rotated), (0, 1))
    print("pprec 3-D n%d %s %s: %.2e" % (n, kind, "rotated" if rotated else "aligned", err))


@pytest.mark.parametrize("rotated", [False, True], ids=["aligned", "rotated"])
@pytest.mark.parametrize("n,kind", CASES2, ids=["n%d_%s" % c for c in CASES2])
def test_pprec_2d_matches_oracle(gpu_ctx, n, kind, rotated):
    err = check_against_oracle(gpu_ctx, make_mesh(2, n, kind, rotated), (0, 1) if n <= 8 else (0,))
    print("pprec 2-D n%d %s %s: %.2e" % (n, kind, "rotated" if rotated else "aligned", err))


def test_pprec_overlap_not_set_up_raises(gpu_ctx):
    """The overlapping variant exists in 3-D for every supported lx1 (4..10, 12; lx1 = 11 is refused at mesh creation) and in
    2-D up to lx1 = 8, and only where some face is shared."""
    with pytest.raises(host.NlgError):
        host.Mesh(gpu_ctx, make_mesh(3, 11, "walls", False))
    for hm in (make_mesh(2, 10, "walls", False), box_mesh((1, 1, 1), 8), box_mesh((1, 1), 6)):
        gm = host.Mesh(gpu_ctx, hm)
        r = np.random.default_rng(1).standard_normal(gm.lpn)
        with pytest.raises(host.NlgError):
            gpu_pprec(gpu_ctx, gm, r, 1, 1)
        z = gpu_pprec(gpu_ctx, gm, r, 0, 1)   # the variant without overlap exists
        assert relerr(z, SchwarzPrec(SEM(hm), overlap=False).apply(r)) <= 1e-12


# ---- aggregated coarse mode: NLG_COARSE_EXACT_MAX is read at mesh set-up, so it runs in a fresh process
AGG_MAX = 16
AGG_CASES = [((4, 4, 3), 8, dict(), True), ((4, 4, 4), 6, dict(periodic=(True, True, True)), False),
             ((4, 3, 3), 10, dict(outflow_xmax=True), True), ((6, 5), 8, dict(), True)]


def agg_mesh(nel, n, kw, rot):
    hm = box_mesh(nel, n, deform=0.05, **kw)
    return Rotated(hm, seed=5).mesh if rot else hm

_CHILD_AGG = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
from test_gpu_pprec_oracle import AGG_CASES, agg_mesh, gpu_pprec
ctx = host.Context(0)
out = {}
for i, case in enumerate(AGG_CASES):
    gm = host.Mesh(ctx, agg_mesh(*case))
    r = np.random.default_rng(3).standard_normal(gm.lpn)
    for ov in (0, 1):
        out["c%%d_o%%d" %% (i, ov)] = gpu_pprec(ctx, gm, r, ov, 1)
np.savez(%(out)r, **out)
print("CHILD OK")
'''


def run_child(code, env_extra, timeout):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_pprec_aggregated_coarse_matches_oracle():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "agg.npz")
        run_child(_CHILD_AGG % dict(root=ROOT, here=HERE, out=path), {"NLG_COARSE_EXACT_MAX": str(AGG_MAX)}, 300)
        got = dict(np.load(path))
    for i, case in enumerate(AGG_CASES):
        sem = SEM(agg_mesh(*case))
        r = np.random.default_rng(3).standard_normal(sem.lpn)
        for ov in (0, 1):
            P = SchwarzPrec(sem, overlap=ov, with_coarse=True, exact_max=AGG_MAX)
            assert P.na < P.nvert and not P.ambiguous, "case %d does not test the aggregated mode" % i
            err = relerr(got["c%d_o%d" % (i, ov)], P.apply(r))
            print("pprec aggregated case %d overlap %d: %.2e" % (i, ov, err))
            assert err <= 1e-12, "case %d overlap %d: relative error %.3e" % (i, ov, err)


# ---- (b) equivariance under element rotation, GPU against GPU
def _base_vec(gm, hm, f1):
    X = [hm.x, hm.y, hm.z]
    b = host.nek_dvector(gm)
    b.set_field(0, f1(hm.mask[0] * (1.0 + 0.5 * np.sin(X[0]) * np.cos(X[1]))))
    b.set_field(1, f1(hm.mask[1] * 0.3 * np.sin(2 * X[2])))
    b.set_field(2, f1(hm.mask[2] * 0.2 * np.cos(X[0] + X[1])))
    return b


def equivariance_errors(ctx, n):
    """max relative differences between the rotated mesh's results and the aligned mesh's, re-indexed"""
    hm = box_mesh((4, 3, 3), n, periodic=(True, False, False), deform=0.05)
    R = Rotated(hm, seed=11)
    lib = ctx.lib
    rng = np.random.default_rng(2)
    u = [hm.mask[i] * rng.standard_normal(hm.x.shape) for i in range(3)]
    p = rng.standard_normal((hm.E, (n - 2) ** 3))
    res = {}
    for tag, mesh, f1, f2 in (("a", hm, lambda a: a, lambda a: a), ("r", R.mesh, R.fwd1, R.fwd2)):
        gm = host.Mesh(ctx, mesh)
        vin, out = host.nek_dvector(gm), host.nek_dvector(gm)
        for i in range(3):
            vin.set_field(i, f1(u[i]))
        vin.set_field(host.PR, f2(p))
        base = _base_vec(gm, hm, f1)
        got = {}

        def vel(name):
            got[name] = [out.get_field(i).reshape(hm.E, -1) for i in range(3)]
        for ov in (0, 1):
            host.check(lib.nlg_op_pprec(gm.h, vin.h, out.h, ov, 1))
            got["pprec%d" % ov] = out.get_field(host.PR).reshape(hm.E, -1)
        host.check(lib.nlg_op_helmholtz(gm.h, vin.h, out.h, 0.7, 3.0, 1))
        vel("helmholtz")
        tmp = vin.copy()
        host.check(lib.nlg_op_dssum(gm.h, tmp.h))
        got["dssum"] = [tmp.get_field(i).reshape(hm.E, -1) for i in range(3)]
        host.check(lib.nlg_op_opdiv(gm.h, vin.h, out.h))
        got["opdiv"] = out.get_field(host.PR).reshape(hm.E, -1)
        host.check(lib.nlg_op_opgradt(gm.h, vin.h, out.h))
        vel("opgradt")
        host.check(lib.nlg_op_cdabdtp(gm.h, vin.h, out.h))
        got["cdabdtp"] = out.get_field(host.PR).reshape(hm.E, -1)
        for adj in (0, 1):
            host.check(lib.nlg_op_conv(gm.h, base.h, vin.h, out.h, adj))
            vel("conv%d" % adj)
        A = host.exptA_linop(0.02, base, re=50.0, dt=0.01, torder=3, vtol=1e-13, ptol=1e-13, fixed_iters_v=60, fixed_iters_p=200, pprecond=0)
        A.init()
        A.matvec(vin, out)
        vel("matvec")
        got["matvec_p"] = out.get_field(host.PR).reshape(hm.E, -1)
        res[tag] = got
    errs = {}
    for k, a in res["a"].items():
        b = res["r"][k]
        if isinstance(a, list):
            sc = max(np.abs(x).max() for x in a)
            errs[k] = max(float(np.abs(R.fwd1(x) - y).max()) for x, y in zip(a, b)) / sc
        else:
            errs[k] = float(np.abs(R.fwd2(a) - b).max() / np.abs(a).max())
    return errs


EQUIV_TOL = {"matvec_p": 1e-10}


@pytest.mark.parametrize("n", [8, 10])
def test_operators_equivariant_under_rotation(gpu_ctx, n):
    errs = equivariance_errors(gpu_ctx, n)
    print("equivariance n%d:" % n, " ".join("%s %.1e" % kv for kv in sorted(errs.items())))
    for k, e in errs.items():
        assert e <= EQUIV_TOL.get(k, 1e-12), "%s: %.3e" % (k, e)


_CHILD_EQUIV = r'''
import sys, json
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
from test_gpu_pprec_oracle import equivariance_errors
ctx = host.Context(0)
print("RESULT " + json.dumps({n: equivariance_errors(ctx, n) for n in (8, 10)}))
print("CHILD OK")
'''


def test_operators_equivariant_under_rotation_one_wave_kernels():
    env = dict(os.environ, NLG_SMALL_E="0")
    r = subprocess.run([sys.executable, "-c", _CHILD_EQUIV % dict(root=ROOT, here=HERE)], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for n, errs in res.items():
        print("equivariance (NLG_SMALL_E=0) n%s:" % n, " ".join("%s %.1e" % kv for kv in sorted(errs.items())))
        for k, e in errs.items():
            assert e <= EQUIV_TOL.get(k, 1e-12), "n%s %s: %.3e" % (n, k, e)


# ---- (c) the headline instantiations (one-wave pressure kernels at lx1 = 8) against the oracle
_CHILD_HEADLINE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
from test_gpu_pprec_oracle import headline_mesh, headline_inputs
import test_gpu_n8 as t8
ctx = host.Context(0)
out = {}
lib = ctx.lib
for rot in (0, 1):
    hm = headline_mesh(rot)
    gm = host.Mesh(ctx, hm)
    u, p = headline_inputs(hm)
    vin, vout = host.nek_dvector(gm), host.nek_dvector(gm)
    for i in range(3):
        vin.set_field(i, u[i])
    vin.set_field(host.PR, p)
    host.check(lib.nlg_op_opdiv(gm.h, vin.h, vout.h)); out["opdiv%%d" %% rot] = vout.get_field(host.PR)
    host.check(lib.nlg_op_opgradt(gm.h, vin.h, vout.h)); out["opgradt%%d" %% rot] = np.stack([vout.get_field(i) for i in range(3)])
    host.check(lib.nlg_op_cdabdtp(gm.h, vin.h, vout.h)); out["cdabdtp%%d" %% rot] = vout.get_field(host.PR)
kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000, fixed_iters_v=40, fixed_iters_p=600)
hm, sem = t8.mesh()
for adj in (0, 1):
    gm, gA = t8.gpu_case(ctx, kw, pprecond=1, pproj=0)
    gv, g1, g2 = t8.upload(gm, t8.start_vector(sem)), host.nek_dvector(gm), host.nek_dvector(gm)
    mv = gA.rmatvec if adj else gA.matvec
    mv(gv, g1)
    mv(g1, g2)
    for k, g in ((1, g1), (2, g2)):
        out["mv%%d_%%d" %% (adj, k)] = np.stack([g.get_field(i) for i in range(3)])
        out["mvp%%d_%%d" %% (adj, k)] = g.get_field(host.PR)
np.savez(%(out)r, **out)
print("CHILD OK")
'''


def headline_mesh(rot):
    hm = box_mesh((3, 3, 2), 8, periodic=(True, False, False), deform=0.05)
    return Rotated(hm, seed=13).mesh if rot else hm


def headline_inputs(hm):
    rng = np.random.default_rng(21)
    return [hm.mask[i] * rng.standard_normal(hm.x.shape) for i in range(3)], rng.standard_normal(hm.E * 6 ** 3)


def test_headline_pressure_kernels_and_matvec_match_oracle():
    import test_gpu_n8 as t8
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "headline.npz")
        run_child(_CHILD_HEADLINE % dict(root=ROOT, here=HERE, out=path), {"NLG_SMALL_E": "0"}, 300)
        got = dict(np.load(path))
    worst = {}
    for rot in (0, 1):
        hm = headline_mesh(rot)
        sem = SEM(hm)
        u, p = headline_inputs(hm)
        e = relerr(got["opdiv%d" % rot], sem.opdiv(u))
        assert e <= 1e-13, ("opdiv", rot, e)
        ref = np.stack([a.reshape(hm.E, -1) for a in sem.opgradt(p)])
        e2 = relerr(got["opgradt%d" % rot], ref)
        assert e2 <= 1e-13, ("opgradt", rot, e2)
        e3 = relerr(got["cdabdtp%d" % rot], sem.cdabdtp(p))
        assert e3 <= 1e-12, ("cdabdtp", rot, e3)
        worst[rot] = (e, e2, e3)
    print("headline operators (aligned, rotated):", worst)
    for adj in (0, 1):
        oA, kw, ov, o1, o2 = t8.oracle_case(True, bool(adj))
        for k, o in ((1, o1), (2, o2)):
            sc = max(np.abs(a).max() for a in o.v)
            err = max(np.abs(got["mv%d_%d" % (adj, k)][i] - o.v[i].ravel()).max() for i in range(3)) / sc
            errp = np.abs(got["mvp%d_%d" % (adj, k)] - o.pr.ravel()).max() / max(np.abs(o.pr).max(), sc)
            print("headline matvec adjoint %d #%d: velocity %.2e pressure %.2e" % (adj, k, err, errp))
            assert err <= 1e-10 and errp <= 1e-9, (adj, k, err, errp)


# ---- (d) pressure iteration counts with the Schwarz preconditioner against the oracle's PCG with oracle/pprec.py
def _iter_case(n):
    hm = box_mesh((3, 2, 2), n, periodic=(True, False, False), deform=0.05)
    sem = SEM(hm)
    U = [sem.mask[i] * sem.dsavg(np.sin(sem.X[0] * (i + 1)) * np.cos(sem.X[1])) for i in range(3)]
    U[0] = U[0] + sem.mask[0]
    kw = dict(re=50.0, torder=3, tau=0.02, dt=0.01, vtol=1e-11, ptol=1e-9, maxit_v=400, maxit_p=4000)
    return hm, sem, U, kw


def _lane_input(sem, v):
    ov = NekDVector(sem)
    ov.rand(ifnorm=True, seed=60 + v)
    for a in ov.v:
        a *= 10.0 ** (-v)                 # different magnitudes: different iteration counts per lane
    return ov


@pytest.mark.parametrize("n", [8, 10])
def test_pressure_iterations_match_oracle(gpu_ctx, n):
    hm, sem, U, kw = _iter_case(n)
    gm = host.Mesh(gpu_ctx, hm)
    gb = host.nek_dvector(gm)
    for i in range(3):
        gb.set_field(i, U[i])
    for pprecond in (0, 2):
        oA = ExptA(sem, U, LNSConfig(pprecond=pprecond, **kw))
        gA = host.exptA_linop(kw["tau"], gb, pprecond=pprecond, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
        gA.init()
        nl = 4 if pprecond == 0 else 1
        ins = [_lane_input(sem, v) for v in range(nl)]
        ref = []
        for ov in ins:
            p0 = oA.stats["p_iters"]
            oA.matvec(ov)
            ref.append(oA.stats["p_iters"] - p0)
        gins, gouts = [], []
        for ov in ins:
            g = host.nek_dvector(gm)
            for i in range(3):
                g.set_field(i, ov.v[i])
            gins.append(g)
            gouts.append(host.nek_dvector(gm))
        s0 = gA.stats()["p_iters"]
        gA.matvec(gins[0], gouts[0])
        one = gA.stats()["p_iters"] - s0
        print("n%d pprecond %d: p_iters one lane %d, oracle %d" % (n, pprecond, one, ref[0]))
        assert one >= 10 and abs(one - ref[0]) <= 0.02 * ref[0] + 2, (pprecond, one, ref[0])
        if nl > 1:
            s0 = gA.stats()["p_iters"]
            gA.matvec_block(gins, [host.nek_dvector(gm) for _ in range(nl)])
            blk = gA.stats()["p_iters"] - s0
            print("n%d pprecond %d: p_iters block of %d %d, oracle %s" % (n, pprecond, nl, blk, ref))
            assert abs(blk - sum(ref)) <= 0.02 * sum(ref) + 2 * nl, (pprecond, blk, ref)
