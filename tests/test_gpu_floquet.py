"""Coupled (orbit) mode of the propagator on the GPU (nlg_linop_set_orbit; host.exptA_orbit_linop): the base flow advanced by the
nonlinear step as one more lane of the launches that advance 1 to 3 perturbations about its current state.

Reference: tests/floquet_ref.py (two oracle propagators in lockstep), which tests/test_cpu_floquet.py checks on the same inputs.
Case A: 2-D walled box, 3 x 3 elements, lx1 = 6, bdf3 with history, 5 + 2 steps.  Case B: 3-D, 2 x 2 x 2 deformed elements, periodic
in x, lx1 = 8 (the k_conv3m / MFMA instantiation), 3 + 2 steps.  Re = 50, dt = 0.01.

Tolerances: a whole matvec against the oracle in the oracle's own iteration (Jacobi, tolerance mode, solves converged to 1e-13):
1e-10, the bound of tests/test_gpu_n8.py; a block against single matvecs: 1e-11, the bound of tests/test_gpu_block.py.
"""
import ctypes as C

import numpy as np
import pytest

import floquet_ref as fr
from neklab_amd import host
from oracle.krylov import arnoldi_step as o_arnoldi_step
from oracle.lns import LNSConfig
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

MATVEC_TOL = 1e-10
_ref = {}


def upload(gm, ov):
    """oracle vector -> device vector, history slots included"""
    def main(dst, fields, pr):
        for i in range(gm.dim):
            dst.set_field(i, fields[i])
        dst.set_field(host.PR, pr)
    gv = host.nek_dvector(gm)
    main(gv, ov.v, ov.pr)
    for r in range(ov.nrst):
        tmp = host.nek_dvector(gm)
        main(tmp, ov.v_rst[r], ov.pr_rst[r])
        gv.save_rst(tmp, r + 1)
    return gv


def gpu_orbit(gm, gX0, kw, **extra):
    return host.exptA_orbit_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"}, **extra)


def gpu_frozen(gm, gX0, kw, **extra):
    A = host.exptA_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"}, **extra)
    A.init()
    return A


def rel_err(gv, ov, sem, irst=0):
    """max error of the velocity of level irst over the max of the main velocity"""
    sc = max(np.abs(a).max() for a in ov.v)
    src = ov.v if irst == 0 else ov.v_rst[irst - 1]
    return max(np.max(np.abs(gv.get_field(i, irst).reshape(sem.shape1) - src[i])) for i in range(sem.dim)) / sc


def gpu_diff(a, b, dim, levels=1):
    sc = max(np.abs(b.get_field(i)).max() for i in range(dim))
    return max(np.max(np.abs(a.get_field(i, r) - b.get_field(i, r))) for r in range(levels) for i in range(dim)) / sc


def reference(name, filt=False):
    """two chained coupled matvecs of the oracle, computed once: (X0, v, o1, end, o2, iterations of the first)"""
    key = (name, filt)
    if key not in _ref:
        hm, sem = fr.case_mesh(name)
        ref = fr.FloquetRef(sem, LNSConfig(**fr.case_cfg(name)), filter_weight=0.05 if filt else 0.0, filter_modes=2)
        X0, v = fr.orbit_state(name), fr.start_vector(sem)
        o1, end = ref.coupled_matvec(X0, v)
        it1 = ref.step_iters
        o2, end2 = ref.coupled_matvec(X0, o1)
        assert all(np.array_equal(a, b) for a, b in zip(end.v, end2.v))
        _ref[key] = (ref, X0, v, o1, end, o2, it1)
    return _ref[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with floquet_ref
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,filt", [("A", False), ("B", False), ("A", True)])
def test_coupled_matvec_matches_reference(gpu_ctx, name, filt):
    """Main fields, both history slots and orbit_end; a second matvec from the reference's first result replays its history.
    Iteration counts of every lane in every time step within one of the reference's."""
    hm, sem = fr.case_mesh(name)
    ref, X0, v, o1, end, o2, it1 = reference(name, filt)
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg(name)
    extra = dict(filter_weight=0.05, filter_modes=2) if filt else {}
    A = gpu_orbit(gm, upload(gm, X0), kw, **extra)
    info = A.info()
    assert info["nsteps"] == ref.nsteps and abs(info["dt"] - ref.dt) < 1e-15 and abs(info["tau"] - kw["tau"]) < 1e-15
    g1, g2 = host.nek_dvector(gm), host.nek_dvector(gm)
    A.matvec(upload(gm, v), g1)
    errs = [rel_err(g1, o1, sem, r) for r in range(3)]
    e_end = rel_err(A.orbit_end(), end, sem)
    errp = np.max(np.abs(g1.get_field(host.PR).reshape(sem.shape2) - o1.pr)) / max(np.abs(o1.pr).max(), max(np.abs(a).max() for a in o1.v))
    nst = ref.nsteps + 2
    got = {"pert": [A.lane_iters(0, k) for k in range(1, nst + 1)], "base": [A.lane_iters(1, k) for k in range(1, nst + 1)]}
    A.matvec(upload(gm, o1), g2)
    err2 = [rel_err(g2, o2, sem, r) for r in range(3)]
    print("coupled matvec case %s filter=%s: main/history %s, orbit_end %.3e, pressure %.3e, with replayed history %s"
          % (name, filt, ["%.3e" % e for e in errs], e_end, errp, ["%.3e" % e for e in err2]))
    worst_it = 0
    for lane in ("pert", "base"):
        for k in range(nst):
            worst_it = max(worst_it, abs(got[lane][k]["v_iters"] - it1[lane][k][0]), abs(got[lane][k]["p_iters"] - it1[lane][k][1]))
    print("iterations per lane and step, device: %s; reference: %s; largest difference %d"
          % ({k: [(d["v_iters"], d["p_iters"]) for d in x] for k, x in got.items()}, it1, worst_it))
    assert g1.nrst == o1.nrst == 2 and g2.nrst == 2
    assert max(errs) <= MATVEC_TOL and e_end <= MATVEC_TOL and errp <= 10 * MATVEC_TOL
    assert max(err2) <= MATVEC_TOL
    assert worst_it <= 1
    assert A.closure() == pytest.approx(fr.vec_err(end, X0), rel=1e-6)      # (the wrapper, not the fields: those are checked above)


# ---------------------------------------------------------------------------------------------------------------------
# 2. block = singles
# ---------------------------------------------------------------------------------------------------------------------
def test_coupled_block_equals_single_matvecs(gpu_ctx):
    hm, sem = fr.case_mesh("B")
    gm = host.Mesh(gpu_ctx, hm)
    A = gpu_orbit(gm, upload(gm, fr.orbit_state("B")), fr.case_cfg("B"))
    vin = []
    for v in range(3):
        x = host.nek_dvector(gm)
        x.rand(True, seed=40 + v)
        x.scal(10.0 ** (-2 * v))
        if v == 1:                                   # one lane with a restart history to replay
            y = host.nek_dvector(gm)
            A.matvec(x, y)
            x = y
        vin.append(x)
    single, ends = [host.nek_dvector(gm) for _ in range(3)], []
    for v in range(3):
        A.matvec(vin[v], single[v])
        ends.append(A.orbit_end())
    blk = [host.nek_dvector(gm) for _ in range(3)]
    A.matvec_block(vin, blk)
    ends.append(A.orbit_end())
    worst = [gpu_diff(blk[v], single[v], 3, levels=3) for v in range(3)]
    e_end = max(gpu_diff(e, ends[0], 3) for e in ends[1:])
    print("coupled block against singles: per lane %s, orbit_end across the four runs %.3e" % (["%.3e" % e for e in worst], e_end))
    assert all(b.nrst == 2 for b in blk)
    assert max(worst) <= 1e-11
    assert e_end <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 3. the base-flow lane is the nonlinear map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_base_flow_lane_is_the_nonlinear_map(gpu_ctx, name):
    hm, sem = fr.case_mesh(name)
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg(name)
    gX0 = upload(gm, fr.orbit_state(name))
    A = gpu_orbit(gm, gX0, kw)
    y = host.nek_dvector(gm)
    A.matvec(upload(gm, fr.start_vector(sem)), y)
    d = A.orbit_end()
    d.axpby(-1.0, gX0, 1.0)
    N = gpu_frozen(gm, gX0, kw)
    F = host.nek_dvector(gm)
    host.check(gpu_ctx.lib.nlg_linop_nonlinear_map(N.h, gX0.h, F.h))
    err = gpu_diff(d, F, sem.dim)
    print("orbit_end - X0 against nonlinear_map(X0), case %s: %.3e (|F|max %.3e)" % (name, err, max(np.abs(F.get_field(i)).max() for i in range(sem.dim))))
    assert err <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 4. zero base flow
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_base_flow_is_the_frozen_operator_about_zero(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    gX0 = host.nek_dvector(gm)
    A, Fz = gpu_orbit(gm, gX0, kw), gpu_frozen(gm, gX0, kw)
    gv, a, b = upload(gm, fr.start_vector(sem)), host.nek_dvector(gm), host.nek_dvector(gm)
    A.matvec(gv, a)
    Fz.matvec(gv, b)
    err = gpu_diff(a, b, 2, levels=3)
    print("zero base flow, coupled against frozen: %.3e" % err)
    assert err <= 1e-13
    assert all(np.array_equal(A.orbit_end().get_field(i), np.zeros(sem.lvn)) for i in range(2))


# ---------------------------------------------------------------------------------------------------------------------
# 5. tangent property without the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_coupled_matvec_is_the_tangent_of_the_nonlinear_map(gpu_ctx):
    """The inputs and the three conditions of tests/test_cpu_floquet.py, with Phi evaluated by nlg_linop_nonlinear_map."""
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.tangent_cfg()
    gX0, gv = upload(gm, fr.orbit_state("A")), upload(gm, fr.start_vector(sem))
    A, N = gpu_orbit(gm, gX0, kw), gpu_frozen(gm, gX0, kw)
    assert A.info()["nsteps"] == 6
    Mv, Fv = host.nek_dvector(gm), host.nek_dvector(gm)
    A.matvec(gv, Mv)
    N.matvec(gv, Fv)                                   # the frozen operator about X0 (before nonlinear_map moves its base flow)

    def flow(X):
        out = host.nek_dvector(gm)
        host.check(gpu_ctx.lib.nlg_linop_nonlinear_map(N.h, X.h, out.h))
        out.axpby(1.0, X, 1.0)
        return out

    e = [fr.tangent_errors(flow, Mv, gX0, gv, eps) for eps in fr.EPS]
    e_frozen = fr.tangent_errors(flow, Fv, gX0, gv, fr.EPS[1])
    print("tangent test (device): e(%g) = %.3e, e(%g) = %.3e, ratio %.1f, frozen operator %.3e" % (fr.EPS[0], e[0], fr.EPS[1], e[1], e[0] / e[1], e_frozen))
    fr.check_tangent(e[0], e[1], e_frozen)


# ---------------------------------------------------------------------------------------------------------------------
# 6. Arnoldi and the Floquet driver
# ---------------------------------------------------------------------------------------------------------------------
def test_arnoldi_and_floquet_driver(gpu_ctx, tmp_path):
    hm, sem = fr.case_mesh("A")
    ref, X0, v, *_ = reference("A")
    gm = host.Mesh(gpu_ctx, hm)
    A = gpu_orbit(gm, upload(gm, X0), fr.case_cfg("A"))
    m = 3
    B = host.KrylovBasis(gm, m + 1)
    B[0].assign(upload(gm, v))
    H, oH = np.zeros((m + 1, m), order="F"), np.zeros((m + 1, m))
    oV = [v.copy()] + [None] * m
    for k in range(m):
        host.arnoldi_step(A, B, k, H)
        o_arnoldi_step(lambda x: ref.coupled_matvec(X0, x)[0], oV, oH, k)
    err = np.max(np.abs(H - oH)) / np.max(np.abs(oH))
    print("Hessenberg of 3 Arnoldi steps on the coupled operator: rel err %.3e" % err)
    assert err <= 1e-10
    mu, expo, res, vecs, info = host.linear_stability_analysis_periodic_orbit(A, kdim=8, nev=2, outdir=str(tmp_path), seed=1, max_restarts=2)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(expo)) and np.all(np.abs(mu) > 0)
    assert np.allclose(expo, np.log(mu.astype(complex)) / A.info()["tau"])
    mu2, res2, info2 = host.eigs(A, [host.nek_dvector(gm) for _ in range(2)], kdim=8, seed=1, max_restarts=2, logfile=str(tmp_path / "eigs2.txt"))
    print("Floquet multipliers %s, residuals %s (nlg_eigs: %s)" % (mu, res, res2))
    assert np.allclose(mu, mu2, rtol=1e-9, atol=0) and np.allclose(res, res2, rtol=1e-6, atol=1e-14) and info == info2


# ---------------------------------------------------------------------------------------------------------------------
# 7. one set of launches
# ---------------------------------------------------------------------------------------------------------------------
def launches_per_step(gpu_ctx, make, run):
    """kernel launches of one time step: the difference between a run of 6 and a run of 3 time steps (what a run launches
    outside its time steps cancels), fixed iteration counts"""
    n = []
    for nsteps in (3, 6):
        op = make(fr.case_cfg("B", tau=nsteps * fr.DT, no_history=True, fixed_iters_v=10, fixed_iters_p=30))
        run(op)                                       # work buffers, one-off set-up
        a, b = C.c_int64(0), C.c_int64(0)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(a), None))
        run(op)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(b), None))
        n.append(b.value - a.value)
    assert (n[1] - n[0]) % 3 == 0, n
    return (n[1] - n[0]) // 3


def test_coupled_step_is_one_set_of_launches(gpu_ctx):
    """coupled(s) <= frozen_block(s + 1) + [nonlinear_step - linear_step(1)] in launches per time step, s = 2: the bracket is the
    per-step set-up of the fine-mesh factors that nonlinear mode already pays.  Two operators stepped alternately would launch
    frozen_block(s) + nonlinear_step."""
    hm, sem = fr.case_mesh("B")
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, fr.orbit_state("B"))
    vin = []
    for v in range(3):
        x = host.nek_dvector(gm)
        x.rand(True, seed=70 + v)
        vin.append(x)
    out = [host.nek_dvector(gm) for _ in range(3)]
    coupled = launches_per_step(gpu_ctx, lambda kw: gpu_orbit(gm, gX0, kw), lambda op: op.matvec_block(vin[:2], out[:2]))
    frozen3 = launches_per_step(gpu_ctx, lambda kw: gpu_frozen(gm, gX0, kw), lambda op: op.matvec_block(vin, out))
    frozen2 = launches_per_step(gpu_ctx, lambda kw: gpu_frozen(gm, gX0, kw), lambda op: op.matvec_block(vin[:2], out[:2]))
    linear1 = launches_per_step(gpu_ctx, lambda kw: gpu_frozen(gm, gX0, kw), lambda op: op.matvec(vin[0], out[0]))
    nonlin = launches_per_step(gpu_ctx, lambda kw: gpu_frozen(gm, gX0, kw),
                               lambda op: host.check(gpu_ctx.lib.nlg_linop_nonlinear_map(op.h, gX0.h, out[0].h)))
    print("launches per time step: coupled(2) %d, frozen block(3) %d, frozen block(2) %d, linear(1) %d, nonlinear %d"
          % (coupled, frozen3, frozen2, linear1, nonlin))
    assert nonlin > linear1
    assert coupled <= frozen3 + (nonlin - linear1)
    assert coupled < frozen2 + nonlin                  # ... which alternating two operators could not meet


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_orbit_mode_refusals_and_leaving_the_mode(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    lib = gpu_ctx.lib
    gX0, gv = upload(gm, fr.orbit_state("A")), upload(gm, fr.start_vector(sem))
    A = gpu_orbit(gm, gX0, kw)
    y = [host.nek_dvector(gm) for _ in range(4)]
    x4 = []
    for v in range(4):
        x = host.nek_dvector(gm)
        x.rand(True, seed=v)
        x4.append(x)
    with pytest.raises(host.NlgError, match="orbit"):
        A.orbit_end()                                  # no matvec yet
    with pytest.raises(host.NlgError, match="orbit mode"):
        A.rmatvec(gv, y[0])
    with pytest.raises(host.NlgError, match="orbit mode"):
        A.matvec_block(x4[:1], y[:1], transpose=True)
    with pytest.raises(host.NlgError, match="orbit mode"):
        A.matvec_block(x4, y)                          # s = 4: the base flow needs the fourth lane
    with pytest.raises(host.NlgError, match="orbit mode"):
        lab = host.line_labels(gm, 1)
        host.check(lib.nlg_linop_set_projection(A.h, 1.0, 1, lab.ctypes.data_as(host._lib.c_int64_p), None, None))
    with pytest.raises(host.NlgError, match="orbit mode"):
        host.integrate_forced(A, None, gv, None, 1.0, False, y[0])
    with pytest.raises(host.NlgError, match="orbit mode"):
        A.tau = 2 * kw["tau"]
    gXt = host.nek_dvector(gm, 1)
    with pytest.raises(host.NlgError, match="orbit mode"):
        gpu_orbit(gm, gXt, kw, ifheat=1)
    # nothing above has disturbed the operator
    A.matvec(gv, y[0])
    B = gpu_orbit(gm, gX0, kw)
    B.matvec(gv, y[1])
    assert all(np.array_equal(y[0].get_field(f, r), y[1].get_field(f, r)) for r in range(3) for f in (0, 1, host.PR))
    # leaving the mode: the frozen operator about X0, bit for bit a fresh one's
    host.check(lib.nlg_linop_set_orbit(A.h, None, 0.0))
    A.matvec(gv, y[2])
    gpu_frozen(gm, gX0, kw).matvec(gv, y[3])
    assert all(np.array_equal(y[2].get_field(f, r), y[3].get_field(f, r)) for r in range(3) for f in (0, 1, host.PR))
    assert not np.array_equal(y[2].get_field(0), y[0].get_field(0))
    with pytest.raises(host.NlgError, match="orbit"):
        A.orbit_end()
