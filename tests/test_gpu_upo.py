"""Periodic-orbit Newton on the GPU (nlg_upo_*; host.nek_ext_dvector, nek_upo_system, gmres_upo, newton_periodic_orbit).

Reference: tests/upo_ref.py (the oracle's coupled step with the border written out), which tests/test_cpu_upo.py checks on the same
inputs.  Cases of tests/floquet_ref.py: A: 2-D walled box, 3 x 3 elements, lx1 = 6; B: 3-D, 2 x 2 x 2 deformed elements, periodic in
x, lx1 = 8.  Re = 50, dt = 0.01, solves converged to 1e-13, pprecond = 1, pproj = 0.

Tolerances.  A matvec against the oracle: 1e-10 of max|U| (tests/test_gpu_floquet.py); a difference of two such states over dt:
1e-10 / dt = 1e-8; the pressure is held to the same bounds on the same scale as the velocity.  The bordered matvec: 1e-10 from M v plus t_in 1e-8 from fT,
under 2e-10.  Device against device: rounding.
"""
import ctypes as C

import numpy as np
import pytest

import floquet_ref as fr
import upo_ref as ur
from neklab_amd import host
from neklab_amd._lib import NlgError

pytestmark = pytest.mark.gpu

MATVEC_TOL = 1e-10
DDT_TOL = MATVEC_TOL / fr.DT
DELTA_T, FT_FD_BOUND = ur.DELTA_T, ur.FT_FD_BOUND
_ref = {}


def upload(gm, ov):
    gv = host.nek_dvector(gm)
    for i in range(gm.dim):
        gv.set_field(i, ov.v[i])
    gv.set_field(host.PR, ov.pr)
    return gv


def make_sys(gm, gX0, T, kw, **extra):
    """an operator in orbit mode about (X0, T) with the solver settings of the Floquet tests; kw: a case_cfg (its tau is ignored)"""
    X = host.nek_ext_dvector(gm, T=T, _vec=gX0)
    cfg = {k: v for k, v in kw.items() if k not in ("tau", "re", "torder")}
    cfg.setdefault("no_history", 0)
    return host.nek_upo_system(X, re=kw["re"], torder=kw["torder"], pprecond=1, pproj=0, **cfg, **extra), X


def fields(gv, dim):
    return [gv.get_field(i) for i in range(dim)], gv.get_field(host.PR)


def err_vs_oracle(gv, ov, sem, sc):
    """(velocity, pressure) max errors over the scale sc"""
    v, p = fields(gv, sem.dim)
    ev = max(np.max(np.abs(v[i].reshape(sem.shape1) - ov.v[i])) for i in range(sem.dim)) / sc
    return ev, np.max(np.abs(p.reshape(sem.shape2) - ov.pr)) / sc


def dev_diff(a, b, dim, sc=None):
    """max difference of all main fields of two device vectors over the largest velocity of b (or sc)"""
    (va, pa), (vb, pb) = fields(a, dim), fields(b, dim)
    sc = sc if sc is not None else max(np.abs(x).max() for x in vb)
    return max(max(np.max(np.abs(x - y)) for x, y in zip(va, vb)), np.max(np.abs(pa - pb))) / sc


def umax(ov):
    return max(np.abs(a).max() for a in ov.v)


def case(name, history):
    """inputs and one reference run, computed once: (sem, hm, kw, UpoRef, X0, v, run with v riding along)"""
    key = (name, history)
    if key not in _ref:
        hm, sem = fr.case_mesh(name)
        if history:
            kw, nst = fr.case_cfg(name), None
        else:
            kw, nst = (fr.tangent_cfg(), 6) if name == "A" else (fr.case_cfg("B", no_history=True), 3)
        ref = ur.UpoRef(sem, kw, nsteps=nst)
        X0, v = fr.orbit_state(name), fr.start_vector(sem)
        _ref[key] = (sem, hm, kw, ref, X0, v, ref.run(X0, kw["tau"], v))
    return _ref[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. residual and the two time derivatives
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_residual_and_time_derivatives_match_reference(gpu_ctx, name):
    """With history (A: 5 + 2 steps, B: 3 + 2): f0, fT and orbit_end from a coupled matvec, then residual, f0, fT from
    nlg_upo_residual, against upo_ref; nlg_upo_residual against orbit_end - X0 of the coupled matvec."""
    sem, hm, kw, ref, X0, v, r = case(name, True)
    gm = host.Mesh(gpu_ctx, hm)
    S, X = make_sys(gm, upload(gm, X0), kw["tau"], kw)
    info = S.info()
    assert info["nsteps"] == r["nsteps"] and abs(info["dt"] - r["dt"]) < 1e-15
    sc = umax(X0)
    out = host.nek_dvector(gm)
    S.op.matvec(upload(gm, v), out)
    assert out.nrst == 2
    e_mv = [err_vs_oracle(S.fdot(w), r[nm], sem, sc) for w, nm in ((0, "f0"), (1, "fT"))]
    closing = S.op.orbit_end()
    closing.axpby(-1.0, X.vec, 1.0)
    res = host.nek_ext_dvector(gm)
    S.eval(X, res)
    e_res = err_vs_oracle(res.vec, r["res"], sem, sc)
    e_ev = [err_vs_oracle(S.fdot(w), r[nm], sem, sc) for w, nm in ((0, "f0"), (1, "fT"))]
    e_close = dev_diff(res.vec, closing, sem.dim, sc)
    print("case %s: residual (vel, pr) %.3e %.3e; f0 / fT from the matvec %s, from the residual run %s; residual against orbit_end - X0 %.3e"
          % (name, e_res[0], e_res[1], ["%.3e %.3e" % e for e in e_mv], ["%.3e %.3e" % e for e in e_ev], e_close))
    assert res.T == 0.0 and res.vec.nrst == 0
    assert e_res[0] <= MATVEC_TOL and e_res[1] <= MATVEC_TOL
    for ev, ep in e_mv + e_ev:
        assert ev <= DDT_TOL and ep <= DDT_TOL
    assert e_close <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the bordered matvec, and the fused border against the composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_bordered_matvec_matches_reference(gpu_ctx, name):
    """No history.  t_in = 0.5 dt against upo_ref: field part 2e-10 of max(|M v|, |U|), phase row 1e-9 of |f0| |v|.  t_in = 0: the
    field part is M v - v from the existing matvec and axpby, to 1e-13."""
    sem, hm, kw, ref, X0, v, r = case(name, False)
    gm = host.Mesh(gpu_ctx, hm)
    S, X = make_sys(gm, upload(gm, X0), kw["tau"], kw, fixed_nsteps=r["nsteps"])
    assert S.info()["nsteps"] == r["nsteps"]
    t_in = 0.5 * fr.DT
    J = ref.jacobian(ur.Ext(X0, kw["tau"]), ur.Ext(v, t_in))
    gv = host.nek_ext_dvector(gm, T=t_in, _vec=upload(gm, v))
    out = host.nek_ext_dvector(gm)
    S.jac_matvec(gv, out)
    sc = max(umax(r["Mv"]), umax(X0))
    ev, ep = err_vs_oracle(out.vec, J.vec, sem, sc)
    e_phase = abs(out.T - J.T) / (r["f0"].norm() * v.norm())
    gv.T = 0.0
    out0 = host.nek_ext_dvector(gm)
    S.jac_matvec(gv, out0)
    Mv = host.nek_dvector(gm)
    S.op.matvec(gv.vec, Mv)
    Mv.axpby(-1.0, gv.vec, 1.0)
    e0 = dev_diff(out0.vec, Mv, sem.dim)
    print("case %s bordered matvec: field %.3e, pressure %.3e, phase row %.3e (value %.6e); t_in = 0 against M v - v %.3e"
          % (name, ev, ep, e_phase, out.T, e0))
    assert out.vec.nrst == 0
    assert ev <= 2e-10 and ep <= 2e-10
    assert e_phase <= 1e-9 and abs(J.T) > 1e-3 * r["f0"].norm() * v.norm()
    assert out0.T == out.T and e0 <= 1e-13


@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_border_equals_composition(gpu_ctx, name):
    """k_upo_border against sub + axpby + dot issued from here, and against the library's composed path, on w = M v for the random
    v of test 2 and for v = f0, whose phase row is |f0|^2: fields 1e-14, phase row 1e-13, relative."""
    sem, hm, kw, ref, X0, v, r = case(name, False)
    gm = host.Mesh(gpu_ctx, hm)
    S, X = make_sys(gm, upload(gm, X0), kw["tau"], kw, fixed_nsteps=r["nsteps"])
    lib, t_in = S.lib, 0.5 * fr.DT
    S.eval(X, host.nek_ext_dvector(gm))
    f0 = S.fdot(0)
    for label, gv in (("random v", upload(gm, v)), ("v = f0", f0.copy())):
        Mv = host.nek_dvector(gm)
        S.op.matvec(gv, Mv)
        Mv.clear_rst_fields()
        fT, f0 = S.fdot(1), S.fdot(0)
        w = [Mv.copy() for _ in range(3)]
        t = [C.c_double(), C.c_double()]
        host.check(lib.nlg_upo_border(S.h, gv.h, t_in, w[0].h, C.byref(t[0]), 0))
        host.check(lib.nlg_upo_border(S.h, gv.h, t_in, w[1].h, C.byref(t[1]), 1))
        w[2].axpby(-1.0, gv, 1.0)
        w[2].axpby(t_in, fT, 1.0)
        phase = gv.dot(f0)
        e = [dev_diff(w[0], w[k], sem.dim) for k in (1, 2)]
        ep = [abs(t[0].value - x) / abs(phase) for x in (t[1].value, phase)]
        print("case %s, %s: fused against composed (library, here) fields %s, phase row %s (value %.6e)"
              % (name, label, ["%.3e" % x for x in e], ["%.3e" % x for x in ep], phase))
        assert max(e) <= 1e-14 and max(ep) <= 1e-13
        assert dev_diff(w[0], Mv, sem.dim) > 1e-6                        # (the border did something)
        if label == "v = f0":
            assert phase == pytest.approx(f0.norm() ** 2, rel=1e-13) and phase > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the extended Arnoldi step
# ---------------------------------------------------------------------------------------------------------------------
def test_upo_arnoldi_step(gpu_ctx):
    """Four steps from a start vector with T = 0.6 of its unit norm: orthonormal in the extended inner product to 1e-12 (and NOT in
    the plain one: > 1e-6), J V_k = V_{k+1} H against independent nlg_upo_jac_matvec calls to 1e-11."""
    sem, hm, kw, ref, X0, v, r = case("A", False)
    gm = host.Mesh(gpu_ctx, hm)
    S, X = make_sys(gm, upload(gm, X0), kw["tau"], kw, fixed_nsteps=6)
    m = 4
    B = host.KrylovBasis(gm, m + 1)
    tcol = np.zeros(m + 2)
    g0 = upload(gm, v)
    g0.scal(0.8 / g0.norm())
    B[0].assign(g0)
    tcol[0] = 0.6
    H = np.zeros((m + 2, m + 1), order="F")
    for k in range(m):
        host.upo_arnoldi_step(S, B, tcol, k, H)
    G = np.array([[B[i].dot(B[j]) for j in range(m + 1)] for i in range(m + 1)])
    e_ext = np.max(np.abs(G + np.outer(tcol[: m + 1], tcol[: m + 1]) - np.eye(m + 1)))
    e_plain = np.max(np.abs(G - np.eye(m + 1)))
    worst = 0.0
    for k in range(m):
        Jv = host.nek_ext_dvector(gm)
        S.jac_matvec(host.nek_ext_dvector(gm, T=tcol[k], _vec=B[k]), Jv)
        comb = host.nek_dvector(gm)
        B.combine(k + 2, np.ascontiguousarray(H[: k + 2, k]), comb)
        sc = max(np.abs(a).max() for a in fields(Jv.vec, 2)[0])
        worst = max(worst, dev_diff(comb, Jv.vec, 2, sc), abs(float(tcol[: k + 2] @ H[: k + 2, k]) - Jv.T) / max(abs(Jv.T), sc))
    print("extended Arnoldi: orthonormality %.3e (plain inner product: %.3e), Arnoldi relation %.3e, tcol %s" % (e_ext, e_plain, worst, tcol[: m + 1]))
    assert e_ext <= 1e-12
    assert e_plain > 1e-6
    assert worst <= 1e-11


# ---------------------------------------------------------------------------------------------------------------------
# 5. finite differences on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_jacobian_is_the_derivative_of_the_residual_on_the_device(gpu_ctx):
    """The two checks of tests/test_cpu_upo.py with the device's residual and Jacobian, same bounds."""
    sem, hm, kw, ref, X0, v, r = case("A", False)
    gm = host.Mesh(gpu_ctx, hm)
    T = kw["tau"]
    S, X = make_sys(gm, upload(gm, X0), T, kw, fixed_nsteps=6)
    gv = upload(gm, v)
    Jv = host.nek_ext_dvector(gm)
    S.jac_matvec(host.nek_ext_dvector(gm, T=0.0, _vec=gv), Jv)
    fT = S.fdot(1)
    frozen = host.exptA_linop(T, X.vec, pprecond=1, pproj=0, **{k: a for k, a in kw.items() if k != "tau"})
    frozen.init()
    Fv = host.nek_dvector(gm)
    frozen.matvec(gv, Fv)
    Fv.axpby(-1.0, gv, 1.0)

    def R(x, period=T):
        out = host.nek_ext_dvector(gm)
        S.eval(host.nek_ext_dvector(gm, T=period, _vec=x), out)
        return out.vec

    e = [fr.tangent_errors(R, Jv.vec, X.vec, gv, eps) for eps in fr.EPS]
    e_frozen = fr.tangent_errors(R, Fv, X.vec, gv, fr.EPS[1])
    d = DELTA_T * T
    q = R(X.vec, T + d)
    q.axpby(-1.0, R(X.vec, T - d), 1.0)
    q.scal(0.5 / d)
    q.axpby(-1.0, fT, 1.0)
    err = q.norm() / fT.norm()
    print("device: x-block e(%g) = %.3e, e(%g) = %.3e, ratio %.1f, frozen operator %.3e; T-column %.4e (bound %.3e)"
          % (fr.EPS[0], e[0], fr.EPS[1], e[1], e[0] / e[1], e_frozen, err, FT_FD_BOUND))
    fr.check_tangent(e[0], e[1], e_frozen)
    assert err <= FT_FD_BOUND               # twice the 7.11e-3 measured on the CPU (tests/upo_ref.py); measured here: the same 7.11e-3


# ---------------------------------------------------------------------------------------------------------------------
# 6. GMRES on the bordered system
# ---------------------------------------------------------------------------------------------------------------------
def test_gmres_upo_true_residual(gpu_ctx):
    sem, hm, kw, ref, X0, v, r = case("A", False)
    gm = host.Mesh(gpu_ctx, hm)
    S, X = make_sys(gm, upload(gm, X0), kw["tau"], kw, fixed_nsteps=6)
    b = host.nek_ext_dvector(gm)
    b.rand(True, seed=17)
    assert b.T != 0.0
    atol = 1e-9 * b.norm()
    x = host.nek_ext_dvector(gm)
    hist = []
    res, nmv = host.gmres_upo(S, b, x, atol=atol, kdim=60, history=hist)
    Jx = host.nek_ext_dvector(gm)
    S.jac_matvec(x, Jx)
    Jx.axpby(-1.0, b, 1.0)
    true = Jx.norm()
    print("gmres_upo: %d matvecs, recurrence residual %.3e, true residual %.3e, atol %.3e" % (nmv, res, true, atol))
    assert res <= atol and true <= 1.01 * atol


# ---------------------------------------------------------------------------------------------------------------------
# 7. Newton on a manufactured root
# ---------------------------------------------------------------------------------------------------------------------
# tests/upo_ref.py's plain Newton needs 3 iterations on these inputs (residuals 9.6e-4, 4.3e-6, 4.9e-9, 7.0e-10; run on the CPU with
# `python tests/upo_ref.py`); the cap is that plus 2.
NEWTON_REF_ITERATIONS = 3


def manufactured(gm):
    ref, Xs, start = ur.manufactured()
    kw = fr.tangent_cfg()
    S, gXs = make_sys(gm, upload(gm, Xs.vec), Xs.T, kw, fixed_nsteps=6)
    off = host.nek_ext_dvector(gm)
    S.eval(gXs, off)                                                  # R(X*, T*) on the device, solves at 1e-13
    X = host.nek_ext_dvector(gm, T=start.T, _vec=upload(gm, start.vec))
    return S, kw, Xs, off, X, gXs


def test_newton_periodic_orbit_on_a_manufactured_root(gpu_ctx, tmp_path):
    """X* = orbit_state("A"), T* = 6 dt, 6 steps fixed, no history, offset = R(X*, T*); from X* + 1e-3 v and 1.01 T*.  Converges to
    1e-9 within the reference's count + 2; the residual recomputed on a fresh operator (solves at 1e-13) is below 1e-9; the period
    stays within 5 % of T*."""
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    S, kw, Xs, off, X, _ = manufactured(gm)
    log = []
    out = host.newton_periodic_orbit(S, X, ur.NEWTON_TOL, maxiter=NEWTON_REF_ITERATIONS + 2, kdim=60, offset=off, fixed_nsteps=6, log=log.append,
                                     outdir=str(tmp_path))
    print("\n".join(log))
    S2, _ = make_sys(gm, X.vec.copy(), X.T, kw, fixed_nsteps=6)
    r = host.nek_ext_dvector(gm)
    S2.eval(X, r)
    r.axpby(-1.0, off, 1.0)
    fresh = r.norm()
    print("Newton: %d iterations, %d GMRES matvecs, residuals %s, periods %s; recomputed residual %.3e; |T - T*| / T* = %.3e"
          % (out["iterations"], out["gmres_matvecs"], ["%.3e" % x for x in out["residuals"]], ["%.8f" % x for x in out["periods"]],
             fresh, abs(X.T - Xs.T) / Xs.T))
    assert out["converged"] and out["iterations"] <= NEWTON_REF_ITERATIONS + 2
    assert len(out["periods"]) == len(out["residuals"]) == out["iterations"] + 1 and out["periods"][-1] == X.T
    assert out["residuals"][-1] < ur.NEWTON_TOL and fresh < ur.NEWTON_TOL
    assert abs(X.T - Xs.T) < 0.05 * Xs.T
    # the converged orbit is written with the period as the header's time; a list goes through the writer once: coordinates in its
    # first file only, every file with its own period
    from neklab_amd import nekio
    f = nekio.read_fld(str(tmp_path / "uponeklab0.f00001"))
    assert abs(f["time"] - X.T) <= 1e-12 * X.T and "x" in f
    assert np.array_equal(f["ux"].ravel(), X.vec.get_field(0)) and np.array_equal(f["uy"].ravel(), X.vec.get_field(1))
    Y = X.copy()
    Y.scal(2.0)
    paths = host.outpost_ext_dnek([X, Y], "tst", outdir=str(tmp_path))
    g = [nekio.read_fld(q) for q in paths]
    assert len(paths) == 2 and "x" in g[0] and "x" not in g[1]
    assert abs(g[0]["time"] - X.T) <= 1e-12 * X.T and abs(g[1]["time"] - 2.0 * X.T) <= 1e-12 * X.T
    assert np.array_equal(g[1]["ux"].ravel(), Y.vec.get_field(0))


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals, and leaving no trace
# ---------------------------------------------------------------------------------------------------------------------
def test_upo_refusals_and_a_clean_operator_afterwards(gpu_ctx):
    sem, hm, kw, ref, X0, v, r = case("A", False)
    gm = host.Mesh(gpu_ctx, hm)
    gX0, gv = upload(gm, X0), upload(gm, v)
    cfg = {k: a for k, a in kw.items() if k != "tau"}
    frozen = host.exptA_linop(kw["tau"], gX0, pprecond=1, pproj=0, **cfg)
    frozen.init()
    lib, t, o = frozen.lib, C.c_double(), host.nek_dvector(gm)
    B = host.KrylovBasis(gm, 3)
    tcol, H = np.zeros(3), np.zeros((3, 2), order="F")
    calls = {
        "nlg_linop_set_orbit_steps": lambda h: lib.nlg_linop_set_orbit_steps(h, gX0.h, kw["tau"], 6),
        "nlg_upo_residual": lambda h: lib.nlg_upo_residual(h, o.h),
        "nlg_upo_fdot": lambda h: lib.nlg_upo_fdot(h, 0, o.h),
        "nlg_upo_jac_matvec": lambda h: lib.nlg_upo_jac_matvec(h, gv.h, 0.0, o.h, C.byref(t)),
        "nlg_upo_border": lambda h: lib.nlg_upo_border(h, gv.h, 0.0, o.h, C.byref(t), 0),
        "nlg_upo_arnoldi_step": lambda h: lib.nlg_upo_arnoldi_step(h, B.h, host.dptr(tcol), 0, host.dptr(H), 3),
    }
    for nm, call in calls.items():                                       # an operator that is not in orbit mode
        with pytest.raises(NlgError, match="not in orbit mode.*nlg_linop_set_orbit"):
            host.check(call(frozen.h))
    S, X = make_sys(gm, gX0, kw["tau"], kw, fixed_nsteps=6)
    for which in (0, 1):                                                 # before the first run
        with pytest.raises(NlgError, match="nlg_upo_fdot: no run yet"):
            S.fdot(which)
    with pytest.raises(NlgError, match="nlg_upo_border: no run yet"):
        host.check(lib.nlg_upo_border(S.h, gv.h, 0.0, o.h, C.byref(t), 0))
    # a UPO session: residual, Jacobian, a step-count change and back, two Arnoldi steps
    S.eval(X, host.nek_ext_dvector(gm))
    S.jac_matvec(host.nek_ext_dvector(gm, T=0.1, _vec=gv), host.nek_ext_dvector(gm))
    S.fixed_nsteps = 4
    S.eval(X, host.nek_ext_dvector(gm))
    assert S.info()["nsteps"] == 4
    B[0].assign(gv)
    host.upo_arnoldi_step(S, B, tcol, 0, H)
    # ... then back to the rule (cfg.dt): a plain coupled matvec is bit for bit the one of a fresh exptA_orbit_linop
    host.check(lib.nlg_linop_set_orbit_steps(S.h, gX0.h, kw["tau"], 0))
    fresh = host.exptA_orbit_linop(kw["tau"], gX0, pprecond=1, pproj=0, **cfg)
    assert S.info() == fresh.info()
    a, b = host.nek_dvector(gm), host.nek_dvector(gm)
    S.op.matvec(gv, a)
    fresh.matvec(gv, b)
    for f in (0, 1, host.PR):
        assert np.array_equal(a.get_field(f), b.get_field(f))
    ea, eb = S.op.orbit_end(), fresh.orbit_end()
    for f in (0, 1, host.PR):
        assert np.array_equal(ea.get_field(f), eb.get_field(f))
