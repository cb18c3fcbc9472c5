"""Explicit modal filter on the GPU (nlg_exptA_config.filter_weight / filter_modes; Nek5000 `filtering = explicit`).

The kernel on its own (nlg_op_filter) against the numpy definition at the operator tolerance of DESIGN 2e (1e-13), and the filter
inside the time stepper -- direct, adjoint, with the temperature, nonlinear map, forced integration -- against the oracle subclass
tests/filter_ref.py FilteredExptA, whose advance() filters what the parent's advance() left.

Tolerances.  Velocity-only matvec with the oracle's own iteration (Jacobi, solves converged to 1e-13): 1e-10, the project's matvec
tolerance.  The coupled, nonlinear and forced integrations are held to what their unfiltered twins are held to (1e-9:
tests/test_gpu_heat.py, test_gpu_newton.py, test_gpu_resolvent.py): the filter adds rounding and nothing else.
"""
import numpy as np
import pytest

from filter_ref import FilteredExptA, apply_filter, filter_matrix, modal_basis
from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.lns import LNSConfig
from oracle.sem import SEM
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

MATVEC_TOL = 1e-10


def small_mesh(dim, n):
    if dim == 2:
        return box_mesh((3, 2), n, lengths=(2.0, 1.0), periodic=(True, False), deform=0.03)
    return box_mesh((2, 2, 2), n, lengths=(2.0, 1.0, 1.0), periodic=(True, False, True), deform=0.03)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncut", [1, 3])
@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("dim,n", [(2, 6), (2, 8), (3, 6), (3, 8), (3, 10), (3, 12)])
def test_filter_kernel_matches_definition(gpu_ctx, dim, n, lanes, ncut):
    hm = small_mesh(dim, n)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    w = 0.3
    F = filter_matrix(n, ncut, w, sem.z1)
    nscal = 1 if lanes == 4 else 0              # the four-lane case carries the scalar as a fourth field
    rng = np.random.default_rng(100 * n + 10 * lanes + ncut)
    vecs, fields = [], []
    for v in range(lanes):
        gv = host.nek_dvector(gm, nscal)
        fl = [10.0 ** (-v) * rng.standard_normal(sem.shape1) for _ in range(dim + nscal)]
        for c in range(dim):
            gv.set_field(c, fl[c])
        if nscal:
            gv.set_field(host.THETA, fl[dim])
        pr = rng.standard_normal(sem.shape2)
        gv.set_field(host.PR, pr)
        vecs.append(gv)
        fields.append((fl, pr))
    arr = (host.vp * lanes)(*[x.h for x in vecs])
    host.check(gpu_ctx.lib.nlg_op_filter(gm.h, lanes, arr, w, ncut))
    worst = 0.0
    for v in range(lanes):
        fl, pr = fields[v]
        for c in range(dim + nscal):
            ref = apply_filter(sem, fl[c], F)
            got = vecs[v].get_field(c if c < dim else host.THETA).reshape(sem.shape1)
            err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
            worst = max(worst, err)
        assert np.array_equal(vecs[v].get_field(host.PR).reshape(sem.shape2), pr)      # the pressure is never filtered
    print("filter kernel dim=%d n=%d lanes=%d ncut=%d: max rel err %.3e" % (dim, n, lanes, ncut, worst))
    assert worst <= 1e-13


def test_filter_kernel_leaves_element_vertices_untouched(gpu_ctx):
    """Rows 1 and n of F are unit vectors: in 1-D terms the end points stay.  In an element the vertices stay, bit for bit; the
    other points of a face are filtered along the face (by F x F of the face's own values, the same from either side)."""
    hm = small_mesh(3, 8)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    gv = host.nek_dvector(gm)
    rng = np.random.default_rng(4)
    u = rng.standard_normal(sem.shape1)
    gv.set_field(0, u)
    host.check(gpu_ctx.lib.nlg_op_filter(gm.h, 1, (host.vp * 1)(gv.h), 0.5, 2))
    got = gv.get_field(0).reshape(sem.shape1)
    assert np.array_equal(got[:, ::7, ::7, ::7], u[:, ::7, ::7, ::7])
    assert np.max(np.abs(got - u)) > 1e-3
    F = filter_matrix(8, 2, 0.5)
    face = np.einsum("ai,bj,eij->eab", F, F, u[:, 0])            # the face z = -1 of every element from its own values alone
    assert np.max(np.abs(got[:, 0] - face)) <= 1e-13 * np.max(np.abs(face))
    assert np.max(np.abs(got[:, 0] - u[:, 0])) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# inside the time stepper
# ---------------------------------------------------------------------------------------------------------------------
def base_flow(sem):
    dim = sem.dim
    if dim == 2:
        U = [sem.mask[i] * sem.dsavg(np.sin(sem.X[0] * (i + 1) * np.pi) * np.cos(sem.X[1])) for i in range(2)]
    else:
        U = [sem.mask[i] * sem.dsavg(np.sin(sem.X[0] * (i + 1) * np.pi) * np.cos(sem.X[1]) * np.cos(np.pi * sem.X[2] + i)) for i in range(3)]
    U[0] = U[0] + sem.mask[0]
    return U


def start_vector(sem, seed=3):
    ov = NekDVector(sem)
    ov.rand(ifnorm=True, seed=seed)
    ov.pr[...] = 0.01 * np.random.default_rng(5).standard_normal(sem.shape2)
    return ov


def upload(gm, ov, nscal=0):
    gv = host.nek_dvector(gm, nscal)
    for i in range(gm.dim):
        gv.set_field(i, ov.v[i])
    gv.set_field(host.PR, ov.pr)
    if nscal:
        gv.set_field(host.THETA, ov.theta[0])
    return gv


def gpu_operator(gm, sem, kw, **extra):
    gb = host.nek_dvector(gm)
    for i, u in enumerate(base_flow(sem)):
        gb.set_field(i, u)
    A = host.exptA_linop(kw["tau"], gb, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"}, **extra)
    A.init()
    return A


def max_err(gv, ov, sem, irst=0):
    src = ov.v if irst == 0 else ov.v_rst[irst - 1]
    return max(np.max(np.abs(gv.get_field(i, irst).reshape(sem.shape1) - src[i])) for i in range(sem.dim))


# dim, lx1, filter_modes, torder, adjoint.  lx1 = 10, 12: the direct case covers the kernel instantiation inside the step (the adjoint
# differs in the convective term only)
MATVEC_CASES = [(2, 6, 1, 3, False), (2, 6, 1, 3, True), (3, 8, 2, 3, False), (3, 8, 2, 3, True), (3, 10, 2, 2, False), (3, 12, 3, 2, False)]


@pytest.mark.parametrize("dim,n,ncut,torder,adjoint", MATVEC_CASES)
def test_filtered_matvec_matches_filtered_oracle(gpu_ctx, dim, n, ncut, torder, adjoint):
    """Direct and adjoint, with history slots: two chained applications, the second replays the history of the first (stored after
    the filter, loaded as it is).  And the filter is not a no-op: the unfiltered GPU result is far away."""
    check_filtered_matvec(gpu_ctx, dim, n, ncut, torder, adjoint)


@pytest.mark.parametrize("dim,n,ncut,torder,adjoint", [(2, 6, 1, 3, True), (3, 8, 2, 3, False), (3, 8, 2, 3, True)])
def test_separate_filter_pass_matches_filtered_oracle(gpu_ctx, monkeypatch, dim, n, ncut, torder, adjoint):
    """NLG_FILTER_FUSED=0 (read when the operator is created): the velocity update in its own kernel, then the filter alone, as
    two launches.  The same check against the same reference as the default, which does both in one kernel."""
    monkeypatch.setenv("NLG_FILTER_FUSED", "0")
    check_filtered_matvec(gpu_ctx, dim, n, ncut, torder, adjoint)


def test_fused_and_separate_filter_agree(gpu_ctx, monkeypatch):
    """The two variants do the same arithmetic in the same order up to the contraction of s * (w * x) into the sum: 4 lanes,
    3-D, lx1 = 8, to 1e-11 like a block against single matvecs."""
    hm = small_mesh(3, 8)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
    vin = []
    for v in range(4):
        x = host.nek_dvector(gm)
        x.rand(True, seed=60 + v)
        vin.append(x)
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("NLG_FILTER_FUSED", fused)
        A = gpu_operator(gm, sem, kw, filter_weight=0.05, filter_modes=2)
        out[fused] = [host.nek_dvector(gm) for _ in range(4)]
        A.matvec_block(vin, out[fused])
    worst = 0.0
    for a, b in zip(out["1"], out["0"]):
        sc = max(np.abs(a.get_field(i)).max() for i in range(3))
        worst = max(worst, max(np.max(np.abs(a.get_field(i, r) - b.get_field(i, r))) for r in range(3) for i in range(3)) / sc)
    print("fused against separate filter, block of 4: rel diff %.3e" % worst)
    assert worst <= 1e-11
    # the switch does switch: with fixed iteration counts the separate variant is exactly one launch per time step more
    import ctypes as C
    one = dict(kw, tau=0.01, dt=0.01, fixed_iters_v=20, fixed_iters_p=200)
    launches = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("NLG_FILTER_FUSED", fused)
        A = gpu_operator(gm, sem, one, filter_weight=0.05, filter_modes=2)
        y = host.nek_dvector(gm)
        A.matvec(vin[0], y)                       # work buffers and one-off set-up launches
        n0, n1 = C.c_int64(0), C.c_int64(0)
        s0 = A.stats()["steps"]
        host.check(gpu_ctx.lib.nlg_counters(C.byref(n0), None))
        A.matvec(vin[0], y)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(n1), None))
        steps = A.stats()["steps"] - s0           # the step of tau = dt and the torder - 1 steps that fill the history slots
        launches[fused] = n1.value - n0.value
    print("launches of a matvec of %d time steps: fused %d, separate %d" % (steps, launches["1"], launches["0"]))
    assert steps >= 1 and launches["0"] == launches["1"] + steps


def check_filtered_matvec(gpu_ctx, dim, n, ncut, torder, adjoint):
    hm = small_mesh(dim, n)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    w = 0.05
    kw = dict(re=50.0, torder=torder, tau=0.03 if n <= 8 else 0.01, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
    if n > 8:
        kw["dt"] = 0.005
    oA = FilteredExptA(sem, base_flow(sem), LNSConfig(**kw), filter_weight=w, filter_modes=ncut)
    ov = start_vector(sem)
    o1 = oA.matvec(ov, adjoint=adjoint)
    o2 = oA.matvec(o1, adjoint=adjoint)
    gA = gpu_operator(gm, sem, kw, filter_weight=w, filter_modes=ncut)
    assert gA.info()["nsteps"] == oA.nsteps
    mv = gA.rmatvec if adjoint else gA.matvec
    gv, g1, g2 = upload(gm, ov), host.nek_dvector(gm), host.nek_dvector(gm)
    mv(gv, g1)
    sc = max(np.abs(a).max() for a in o1.v)
    errs = [max_err(g1, o1, sem, r) / sc for r in range(torder)]
    mv(g1, g2)
    sc2 = max(np.abs(a).max() for a in o2.v)
    err2 = max_err(g2, o2, sem) / sc2
    print("filtered matvec dim=%d n=%d adjoint=%s: rel err main/history %s, chained %.3e" % (dim, n, adjoint, ["%.3e" % e for e in errs], err2))
    assert g1.nrst == o1.nrst == torder - 1
    assert max(errs) <= MATVEC_TOL
    assert err2 <= MATVEC_TOL
    errp = np.max(np.abs(g1.get_field(host.PR).reshape(sem.shape2) - o1.pr))
    assert errp <= 10 * MATVEC_TOL * max(np.abs(o1.pr).max(), sc)
    # not a no-op
    gU = gpu_operator(gm, sem, kw)
    u1 = host.nek_dvector(gm)
    (gU.rmatvec if adjoint else gU.matvec)(gv, u1)
    diff = max(np.max(np.abs(u1.get_field(i) - g1.get_field(i))) for i in range(dim)) / sc
    print("filtered against unfiltered: %.3e" % diff)
    assert diff > 100 * MATVEC_TOL


@pytest.mark.parametrize("dim,n,ncut", [(2, 6, 1), (3, 8, 2)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_filtered_block_equals_single_matvecs(gpu_ctx, dim, n, ncut, adjoint):
    """Four lanes through the filtered step together give what four single matvecs give: the set-up of
    tests/test_gpu_block.py::test_matvec_block_equals_single_matvecs (mesh, base flow, solver settings, lanes of very different
    magnitude, a restart history on the odd lanes) with the filter on."""
    nel = (4, 3) if dim == 2 else (3, 2, 2)
    hm = box_mesh(nel, n, periodic=(True,) + (False,) * (dim - 1), deform=0.04)
    gm = host.Mesh(gpu_ctx, hm)
    X = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
    gb = host.nek_dvector(gm)
    gb.set_field(0, hm.mask[0] * (1.0 + 0.5 * np.sin(X[0]) * np.cos(X[1])))
    gb.set_field(1, hm.mask[1] * 0.3 * np.sin(2 * X[0]))
    A = host.exptA_linop(0.05, gb, re=40.0, dt=0.01, torder=3, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000,
                         filter_weight=0.05, filter_modes=ncut)
    A.init()
    mv = A.rmatvec if adjoint else A.matvec
    s = 4
    vin = []
    for v in range(s):
        x = host.nek_dvector(gm)
        x.rand(True, seed=40 + v)
        x.scal(10.0 ** (-2 * v))
        if v % 2 == 1:
            y = host.nek_dvector(gm)
            mv(x, y)
            x = y
        vin.append(x)
    single = [host.nek_dvector(gm) for _ in range(s)]
    for v in range(s):
        mv(vin[v], single[v])
    blk = [host.nek_dvector(gm) for _ in range(s)]
    A.matvec_block(vin, blk, transpose=adjoint)
    worst = []
    for v in range(s):
        sc = max(np.abs(single[v].get_field(i)).max() for i in range(dim))
        worst.append(max(np.max(np.abs(blk[v].get_field(i, r) - single[v].get_field(i, r))) for r in range(3) for i in range(dim)) / sc)
        assert blk[v].nrst == 2
    print("filtered block against single, dim=%d n=%d adjoint=%s: rel diff per lane %s" % (dim, n, adjoint, ["%.3e" % e for e in worst]))
    assert max(worst) <= 1e-11


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 8)])
def test_filtered_boussinesq_matvec_matches_filtered_oracle(gpu_ctx, dim, n):
    """ifheat: the temperature is filtered with the velocity at the end of the step; the fluid sees the unfiltered new temperature."""
    hm = small_mesh(dim, n)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    U = [sem.mask[0] * (4 * sem.X[1] * (1 - sem.X[1]))] + [np.zeros(sem.shape1) for _ in range(dim - 1)]
    Theta = 1.0 - sem.X[1] + 0.1 * np.sin(np.pi * sem.X[0]) * np.sin(np.pi * sem.X[1])
    gb = host.nek_dvector(gm, 1)
    gb.set_field(0, U[0])
    gb.set_field(host.THETA, Theta)
    kw = dict(re=5.0, torder=3, vtol=1e-13, ptol=1e-13, maxit_v=600, maxit_p=4000, dt=0.01)
    heat = dict(ifheat=True, conductivity=0.3, rhocp=1.5, buoy=(0.0, 50.0, 0.0))
    w, ncut = 0.05, 2
    oA = FilteredExptA(sem, U, LNSConfig(tau=0.05, **kw, **heat), Theta, filter_weight=w, filter_modes=ncut)
    gA = host.exptA_linop(0.05, gb, pprecond=1, pproj=0, filter_weight=w, filter_modes=ncut, **kw, **{**heat, "ifheat": 1})
    gA.init()
    gU = host.exptA_linop(0.05, gb, pprecond=1, pproj=0, **kw, **{**heat, "ifheat": 1})
    gU.init()
    rng = np.random.default_rng(0)
    ov = NekDVector(sem, 1)
    for i in range(dim):
        ov.v[i][...] = sem.mask[i] * sem.dsavg(rng.standard_normal(sem.shape1))
    ov.theta[0][...] = sem.tmask * sem.dsavg(rng.standard_normal(sem.shape1))
    gv = upload(gm, ov, 1)
    for adjoint in (False, True):
        gout, uout = host.nek_dvector(gm, 1), host.nek_dvector(gm, 1)
        (gA.rmatvec if adjoint else gA.matvec)(gv, gout)
        (gU.rmatvec if adjoint else gU.matvec)(gv, uout)
        oout = oA.matvec(ov, adjoint=adjoint)
        sc = max(np.abs(a).max() for a in oout.v)
        st = np.abs(oout.theta[0]).max()
        ev = max_err(gout, oout, sem) / sc
        et = np.max(np.abs(gout.get_field(host.THETA).reshape(sem.shape1) - oout.theta[0])) / st
        eh = np.max(np.abs(gout.get_field(host.THETA, 2).reshape(sem.shape1) - oout.theta_rst[1][0])) / st
        dt_ = np.max(np.abs(gout.get_field(host.THETA) - uout.get_field(host.THETA))) / st
        print("filtered Boussinesq dim=%d n=%d adjoint=%s: velocity %.3e temperature %.3e (history %.3e); temperature against unfiltered %.3e"
              % (dim, n, adjoint, ev, et, eh, dt_))
        assert ev <= 1e-9 and et <= 1e-9 and eh <= 1e-9
        assert dt_ > 100 * 1e-9                       # the temperature is filtered, not only the velocity


@pytest.mark.parametrize("dim", [2, 3])
def test_filtered_nonlinear_map_matches_filtered_oracle(gpu_ctx, dim):
    if dim == 2:
        hm = box_mesh((3, 3), 6, lengths=(1.0, 1.0), deform=0.02)
    else:
        hm = box_mesh((3, 3, 2), 6, lengths=(1.0, 1.0, 0.6), periodic=(False, False, True), deform=0.02)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    x, y = sem.X[0], sem.X[1]
    oX = NekDVector(sem)
    oX.v[0][...] = (16 * x ** 2 * (1 - x) ** 2) * (y > 1 - 1e-9)
    for i in range(dim):
        oX.v[i][...] += 0.2 * sem.mask[i] * sem.dsavg(np.sin(3 * sem.X[0] + i) * np.cos(2 * sem.X[1]))
    gX = upload(gm, oX)
    tau, re, w, ncut = 0.1, 30.0, 0.05, 1
    cfg = LNSConfig(re=re, torder=3, tau=tau, cfl_limit=0.4, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
    oF = FilteredExptA(sem, oX.v, cfg, filter_weight=w, filter_modes=ncut).nonlinear_map(oX)
    kw = dict(re=re, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000, pprecond=1, pproj=0)
    sysf = host.nek_system(tau, gX, filter_weight=w, filter_modes=ncut, **kw)
    # the options arrive in both operators of the system
    assert sysf.nl.cfg.filter_weight == w and sysf.jac.cfg.filter_weight == w
    assert sysf.nl.cfg.filter_modes == ncut and sysf.jac.cfg.filter_modes == ncut
    gF, uF = host.nek_dvector(gm), host.nek_dvector(gm)
    sysf.eval(gX, gF)
    host.nek_system(tau, gX, **kw).eval(gX, uF)
    sc = max(np.abs(a).max() for a in oF.v)
    err = max_err(gF, oF, sem) / sc
    diff = max(np.max(np.abs(gF.get_field(i) - uF.get_field(i))) for i in range(dim)) / sc
    print("filtered nonlinear map dim=%d: rel err %.3e, against unfiltered %.3e" % (dim, err, diff))
    assert err <= 1e-9
    assert diff > 100 * 1e-9
    # the Jacobian operator of the system carries the filter too: its matvec is the filtered oracle's about the same state
    oJ = FilteredExptA(sem, oX.v, LNSConfig(re=re, torder=3, tau=tau, cfl_limit=0.5, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000),
                       filter_weight=w, filter_modes=ncut)
    ov = start_vector(sem)
    oj = oJ.matvec(ov)
    gj = host.nek_dvector(gm)
    sysf.jac.matvec(upload(gm, ov), gj)
    assert max_err(gj, oj, sem) <= 1e-9 * max(np.abs(a).max() for a in oj.v)


@pytest.mark.parametrize("dim,adjoint", [(2, False), (2, True), (3, False)])
def test_filtered_forced_integration_matches_filtered_oracle(gpu_ctx, dim, adjoint):
    hm = box_mesh((3, 3), 6, lengths=(2.0, 1.0), periodic=(True, False), deform=0.03) if dim == 2 else small_mesh(3, 6)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    U = [sem.mask[0] * (4 * sem.X[1] * (1 - sem.X[1]))] + [np.zeros(sem.shape1) for _ in range(dim - 1)]
    gb = host.nek_dvector(gm)
    gb.set_field(0, U[0])
    rng = np.random.default_rng(1)
    fz = host.nek_zvector(gm)
    fre, fim = [], []
    for i in range(dim):
        a = sem.mask[i] * sem.dsavg(np.sin(np.pi * sem.X[0] + i) * np.sin(np.pi * sem.X[1]) + 0.1 * rng.standard_normal(sem.shape1))
        b = sem.mask[i] * sem.dsavg(np.cos(np.pi * sem.X[0]) * np.sin(2 * np.pi * sem.X[1]))
        fre.append(a)
        fim.append(b)
        fz.re.set_field(i, a)
        fz.im.set_field(i, b)
    omega, w, ncut = 8.0, 0.05, 1
    tau = 2 * np.pi / omega
    kw = dict(re=20.0, torder=3, vtol=1e-12, ptol=1e-12, maxit_v=400, maxit_p=4000)
    ob = FilteredExptA(sem, U, LNSConfig(tau=tau, **kw), filter_weight=w, filter_modes=ncut).integrate_forced(None, fre, fim, omega, adjoint)
    gA = host.exptA_linop(tau, gb, pprecond=1, pproj=0, filter_weight=w, filter_modes=ncut, **kw)
    gA.init()
    gU = host.exptA_linop(tau, gb, pprecond=1, pproj=0, **kw)
    gU.init()
    gout, uout = host.nek_dvector(gm), host.nek_dvector(gm)
    host.integrate_forced(gA, None, fz.re, fz.im, omega, adjoint, gout)
    host.integrate_forced(gU, None, fz.re, fz.im, omega, adjoint, uout)
    sc = max(np.abs(a).max() for a in ob.v)
    err = max_err(gout, ob, sem) / sc
    diff = max(np.max(np.abs(gout.get_field(i) - uout.get_field(i))) for i in range(dim)) / sc
    print("filtered forced integration dim=%d adjoint=%s: rel err %.3e, against unfiltered %.3e" % (dim, adjoint, err, diff))
    assert err <= 1e-9
    assert diff > 100 * 1e-9


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 8)])
def test_full_weight_filter_removes_the_top_mode(gpu_ctx, dim, n):
    """Independent of the oracle: with weight 1 on one mode F is a projector, so the top modal coefficient (row n of Phi^-1 along a
    direction) of the velocity a matvec returns vanishes along every direction of every element."""
    hm = small_mesh(dim, n)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
    gA = gpu_operator(gm, sem, kw, filter_weight=1.0, filter_modes=1)
    gU = gpu_operator(gm, sem, kw)
    gv, g1, u1 = upload(gm, start_vector(sem)), host.nek_dvector(gm), host.nek_dvector(gm)
    gA.matvec(gv, g1)
    gU.matvec(gv, u1)
    top = np.linalg.inv(modal_basis(sem.z1))[-1]
    worst, plain = 0.0, 0.0
    for i in range(dim):
        a, b = g1.get_field(i).reshape(sem.shape1), u1.get_field(i).reshape(sem.shape1)
        for ax in range(1, dim + 1):
            worst = max(worst, np.max(np.abs(np.tensordot(top, a, axes=([0], [ax])))) / np.max(np.abs(a)))
            plain = max(plain, np.max(np.abs(np.tensordot(top, b, axes=([0], [ax])))) / np.max(np.abs(b)))
    print("top-mode coefficient / |u|_inf: filtered %.3e, unfiltered %.3e" % (worst, plain))
    assert worst <= 1e-12
    assert plain > 1e-6                      # ... and it was there to be removed


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 8)])
def test_zero_weight_is_the_unfiltered_operator_bit_for_bit(gpu_ctx, dim, n):
    hm = small_mesh(dim, n)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
    gv = upload(gm, start_vector(sem))
    outs = []
    for extra in ({}, dict(filter_weight=0.0, filter_modes=3), dict(filter_weight=0.0, filter_modes=-5)):
        A = gpu_operator(gm, sem, kw, **extra)
        y = host.nek_dvector(gm)
        A.matvec(gv, y)
        outs.append([y.get_field(f, r) for r in range(3) for f in list(range(dim)) + [host.PR]])
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_filter_options_are_validated(gpu_ctx):
    hm = small_mesh(2, 6)
    sem = SEM(hm)
    gm = host.Mesh(gpu_ctx, hm)
    gb = host.nek_dvector(gm)
    for bad in (dict(filter_weight=-0.1, filter_modes=1), dict(filter_weight=1.5, filter_modes=1),
                dict(filter_weight=0.01, filter_modes=0), dict(filter_weight=0.01, filter_modes=5)):     # lx1 - 1 = 5
        with pytest.raises(host.NlgError, match="filter"):
            host.exptA_linop(0.1, gb, **bad)
    host.exptA_linop(0.1, gb, filter_weight=1.0, filter_modes=4)        # the ends of both ranges are accepted
    # lx1 without a kernel: an error, not a fall-back
    gm7 = host.Mesh(gpu_ctx, small_mesh(2, 7))
    with pytest.raises(host.NlgError, match="filter"):
        host.exptA_linop(0.1, host.nek_dvector(gm7), filter_weight=0.01, filter_modes=1)
