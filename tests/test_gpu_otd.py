"""OTD modes on the GPU (nlg_otd_*; host.nek_otd): r lanes of the block stepper with the reduced operator, the forcing and the
re-orthonormalisation computed on the device from what the time step holds in memory.

Reference: tests/otd_ref.py (r oracle propagators in lockstep), which tests/test_cpu_otd.py checks on the same inputs.  Cases of
tests/floquet_ref.py: A: 2-D walled box, 3 x 3 elements, lx1 = 6; B: 3-D, 2 x 2 x 2 deformed elements, periodic in x, lx1 = 8; Re = 50,
dt = 0.01, solves converged to 1e-13.

Tolerances: Lr against sums formed on the host from the public operators: 1e-12 max|Lr| (summation orders of the same products);
six steps against the twin: 1e-10 (MATVEC_TOL of tests/test_gpu_floquet.py: same cases, solver tolerances and step counts; OTD adds
O(1) linear combinations of the lanes); nestedness 1e-11 (the same operations per lane, only the block reductions differ); plain
steps against matvec_block 1e-12; |G - I| after a transform 1e-13.
"""
import ctypes as C

import numpy as np
import pytest

import floquet_ref as fr
import otd_ref
from otd_ref import KA, leading
from neklab_amd import host
from oracle.lns import LNSConfig

pytestmark = pytest.mark.gpu

TOL = 1e-10
_ref = {}


def upload(gm, ov):
    gv = host.nek_dvector(gm)
    for i in range(gm.dim):
        gv.set_field(i, ov.v[i])
    gv.set_field(host.PR, ov.pr)
    return gv


def gpu_otd(gm, gX0, kw, basis, **opts):
    """nek_otd in the oracle's iteration (Jacobi pressure preconditioner, no residual projection), created from `basis`"""
    opts.setdefault("solve_baseflow", False)
    O = host.nek_otd(gX0, len(basis), pprecond=1, pproj=0, **kw)
    O.init(host.otd_opts(**opts), basis0=basis)
    return O


def field_err(gv, ov, sem):
    sc = max(np.abs(a).max() for a in ov.v)
    ev = max(np.max(np.abs(gv.get_field(i).reshape(sem.shape1) - ov.v[i])) for i in range(sem.dim)) / sc
    ep = np.max(np.abs(gv.get_field(host.PR).reshape(sem.shape2) - ov.pr)) / max(np.abs(ov.pr).max(), sc)
    return ev, ep


def gpu_diff(a, b, dim):
    sc = max(np.abs(b.get_field(i)).max() for i in range(dim))
    return max(np.max(np.abs(a.get_field(i) - b.get_field(i))) for i in range(dim)) / sc


def twin(name, r, coupled=False, filt=False):
    """six steps of the twin with orthostep = 2, computed once"""
    key = (name, r, coupled, filt)
    if key not in _ref:
        hm, sem = fr.case_mesh(name)
        B = otd_ref.orthonormal_basis(sem, r)
        R = otd_ref.OTDRef(sem, LNSConfig(**fr.case_cfg(name)), fr.orbit_state(name), B, orthostep=2, solve_baseflow=coupled,
                           filter_weight=0.05 if filt else 0.0, filter_modes=2)
        R.advance(6)
        Lr, G = R.reduced()
        _ref[key] = (B, R, Lr, G)
    return _ref[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. Lr against the public operators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r,trans", [("A", 1, 0), ("A", 2, 0), ("A", 3, 0), ("A", 4, 0), ("B", 4, 0), ("A", 2, 1), ("A", 4, 1)])
def test_reduced_operator_against_public_operators(gpu_ctx, name, r, trans):
    hm, sem = fr.case_mesh(name)
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg(name)
    gX0 = upload(gm, fr.orbit_state(name))
    O = gpu_otd(gm, gX0, kw, [upload(gm, b) for b in otd_ref.orthonormal_basis(sem, r)], trans=bool(trans))
    Lr, G = O.reduced()
    lib, dim = gm.lib, gm.dim
    U, W = [], []
    for j in range(r):
        b = O.basis(j)
        h, c, g = host.nek_dvector(gm), host.nek_dvector(gm), host.nek_dvector(gm)
        host.check(lib.nlg_op_helmholtz(gm.h, b.h, h.h, 1.0 / kw["re"], 0.0, 0))
        host.check(lib.nlg_op_conv(gm.h, gX0.h, b.h, c.h, trans))
        host.check(lib.nlg_op_opgradt(gm.h, b.h, g.h))
        U.append([b.get_field(i) for i in range(dim)])
        W.append([g.get_field(i) - h.get_field(i) - c.get_field(i) for i in range(dim)])
    ref = np.array([[sum(np.sum(U[i][c] * W[j][c]) for c in range(dim)) for j in range(r)] for i in range(r)])
    err = np.abs(Lr - ref).max() / np.abs(ref).max()
    print("Lr case %s r=%d trans=%d: max|Lr| %.3e, relative difference %.3e, |G - I| before %.3e" % (name, r, trans, np.abs(ref).max(), err,
                                                                                                 np.abs(G - np.eye(r)).max()))
    O.close()
    assert err <= 1e-12
    assert np.abs(G - np.eye(r)).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# 2. six steps against the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r,coupled,filt", [("A", 2, False, False), ("A", 3, False, False), ("A", 2, False, True), ("A", 2, True, False),
                                                 ("B", 4, False, False), ("B", 3, True, False)])
def test_six_steps_match_the_twin(gpu_ctx, name, r, coupled, filt):
    hm, sem = fr.case_mesh(name)
    B, R, Lr_ref, G_ref = twin(name, r, coupled, filt)
    gm = host.Mesh(gpu_ctx, hm)
    extra = dict(filter_weight=0.05, filter_modes=2) if filt else {}
    O = gpu_otd(gm, upload(gm, fr.orbit_state(name)), dict(fr.case_cfg(name), **extra), [upload(gm, b) for b in B], orthostep=2,
                solve_baseflow=coupled)
    O.advance(6)
    Lr, G = O.reduced()
    info = O.info()
    errs = [field_err(O.basis(j), R.basis(j), sem) for j in range(r)]
    ev, ep = max(e[0] for e in errs), max(e[1] for e in errs)
    eb = field_err(O.current_baseflow(), R.baseflow(), sem) if coupled else field_err(O.current_baseflow(), fr.orbit_state(name), sem)
    eL = np.abs(Lr - Lr_ref).max() / np.abs(Lr_ref).max()
    print("OTD case %s r=%d coupled=%s filter=%s: velocities %.3e, pressures %.3e, base flow %.3e / %.3e, Lr %.3e, G before the last transform: "
          "device %.3e twin %.3e" % (name, r, coupled, filt, ev, ep, eb[0], eb[1], eL, np.abs(G - np.eye(r)).max(), np.abs(G_ref - np.eye(r)).max()))
    O.close()
    assert info["istep"] == 6 and abs(info["time"] - 6 * fr.DT) < 1e-14 and abs(info["dt"] - R.dt) < 1e-15
    assert ev <= TOL and ep <= TOL and max(eb) <= TOL and eL <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact structure
# ---------------------------------------------------------------------------------------------------------------------
def test_orthonormal_after_reduced_and_nested(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    gX0 = upload(gm, fr.orbit_state("A"))
    B = otd_ref.orthonormal_basis(sem, 3)
    runs = {}
    for r in (1, 2, 3):
        runs[r] = gpu_otd(gm, gX0, kw, [upload(gm, b) for b in B[:r]], orthostep=2)
        runs[r].advance(6)
    e = [gpu_diff(runs[3].basis(0), runs[1].basis(0), 2), gpu_diff(runs[3].basis(0), runs[2].basis(0), 2), gpu_diff(runs[3].basis(1), runs[2].basis(1), 2)]
    print("nestedness: mode 1 of r=3 against r=1 %.3e, against r=2 %.3e, mode 2 of r=3 against r=2 %.3e" % tuple(e))
    runs[3].reduced()
    G_after = runs[3].reduced()[1]                     # the Gram matrix before the second transform = after the first
    vec = [runs[3].basis(j) for j in range(3)]
    G_dot = np.array([[vec[i].dot(vec[j]) for j in range(3)] for i in range(3)])
    print("|G - I| after reduced(): %.3e (from nlg_vec_dot: %.3e)" % (np.abs(G_after - np.eye(3)).max(), np.abs(G_dot - np.eye(3)).max()))
    assert np.abs(G_after - np.eye(3)).max() <= 1e-13 and np.abs(G_dot - np.eye(3)).max() <= 1e-13
    for r in (1, 2, 3):
        runs[r].close()
    assert max(e) <= 1e-11


def test_steps_before_startstep_are_block_steps(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, fr.orbit_state("A"))
    O = gpu_otd(gm, gX0, fr.case_cfg("A"), [upload(gm, b) for b in otd_ref.orthonormal_basis(sem, 3)], startstep=4)
    vin = [O.basis(j) for j in range(3)]
    O.advance(3)
    got = [O.basis(j) for j in range(3)]
    O.close()
    kw = fr.case_cfg("A", tau=3 * fr.DT, no_history=True)
    A = host.exptA_linop(kw.pop("tau"), gX0, pprecond=1, pproj=0, **kw)
    A.init()
    out = [host.nek_dvector(gm) for _ in range(3)]
    A.matvec_block(vin, out)
    e = [gpu_diff(got[j], out[j], 2) for j in range(3)]
    ep = max(np.max(np.abs(got[j].get_field(host.PR) - out[j].get_field(host.PR))) / max(np.abs(out[j].get_field(host.PR)).max(), 1e-300) for j in range(3))
    print("three steps before startstep against matvec_block: velocities %s, pressure %.3e" % (["%.3e" % x for x in e], ep))
    A.close()
    assert max(e) <= 1e-12 and ep <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 4. batched lanes
# ---------------------------------------------------------------------------------------------------------------------
def test_otd_step_is_one_set_of_launches(gpu_ctx):
    """A step past the start-up (no transform): launches and reduction sites by nlg_counters, fixed iteration counts.  The step with
    OTD against the same step without it (startstep out of reach): one reduction site more."""
    hm, sem = fr.case_mesh("B")
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, fr.orbit_state("B"))
    kw = fr.case_cfg("B", fixed_iters_v=10, fixed_iters_p=30)
    B = otd_ref.orthonormal_basis(sem, 3)

    def per_step(r, startstep):
        O = gpu_otd(gm, gX0, kw, [upload(gm, b) for b in B[:r]], startstep=startstep, orthostep=1000)
        O.advance(startstep + 11 if startstep == 1 else 12)
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
        O.advance(2)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(c), C.byref(d)))
        O.close()
        assert (c.value - a.value) % 2 == 0 and (d.value - b.value) % 2 == 0
        return (c.value - a.value) // 2, (d.value - b.value) // 2

    l1, c1 = per_step(1, 1)
    l3, c3 = per_step(3, 1)
    l3p, c3p = per_step(3, 10 ** 6)
    print("per OTD step on B: launches r=1 %d, r=3 %d (block step without OTD, r=3: %d); reduction sites r=1 %d, r=3 %d (without OTD %d)"
          % (l1, l3, l3p, c1, c3, c3p))
    assert l1 == l3
    assert c3 == c3p + 1 and c1 == c3


# ---------------------------------------------------------------------------------------------------------------------
# 5. known answer on the code's own operator
# ---------------------------------------------------------------------------------------------------------------------
def test_leading_eigenvalue_of_Lr_is_the_propagators(gpu_ctx, tmp_path):
    """Case A at Re = 10 about the frozen orbit_state("A", 1.0), dt = 0.01, r = 2: after 82 steps the leading eigenvalue of Lr agrees
    with log(mu_1) / tau of host.eigs on the frozen propagator (tau = 0.2) to 7.8e-3.  From tests/test_cpu_otd.py: the twin's difference
    to oracle.krylov.eigs settles at 7.83e-4 (150 steps: the O(dt^3) gap between a Rayleigh quotient of L and the discrete eigenvalue of
    the bdf3 propagator); the tolerance is 10 x that, and 82 is the smallest step count at which the twin is inside it (7.43e-3;
    81 steps: 8.20e-3).  At step 0 the same quantity misses by 1.15e+2."""
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A", re=KA["re"], dt=KA["dt"], tau=KA["tau"])
    gX0 = upload(gm, fr.orbit_state("A", KA["amp"]))
    A = host.exptA_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    A.init()
    mu, res, info = host.eigs(A, [host.nek_dvector(gm) for _ in range(2)], kdim=24, tol=1e-10, x0=upload(gm, fr.start_vector(sem)),
                              logfile=str(tmp_path / "eigs.txt"))
    lam_ref = np.log(complex(mu[0])) / kw["tau"]
    A.close()
    O = gpu_otd(gm, gX0, kw, [upload(gm, b) for b in otd_ref.orthonormal_basis(sem, KA["r"])], orthostep=10)
    d0 = abs(leading(O.reduced()[0]) - lam_ref)
    O.advance(KA["nsteps"])
    d = abs(leading(O.reduced()[0]) - lam_ref)
    O.close()
    print("lambda_ref %s (residual %.1e), |lambda_1(Lr) - lambda_ref|: step 0 %.3e, step %d %.3e" % (lam_ref, res[0], d0, KA["nsteps"], d))
    assert d <= KA["tol"]
    assert d0 > 100.0 * KA["tol"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    gX0 = upload(gm, fr.orbit_state("A"))
    lib = gm.lib

    def create(op, **o):
        oo = host._lib.OtdOpts()
        host.check(lib.nlg_otd_opts_default(C.byref(oo)))
        for k, v in o.items():
            setattr(oo, k, v)
        h = host.vp()
        host.check(lib.nlg_otd_create(op.h, C.byref(oo), None, C.byref(h)))
        return h

    def linop(**over):
        k2 = dict(kw, **over)
        return host.exptA_linop(k2.pop("tau"), gX0, pprecond=1, pproj=0, **k2)

    A = linop()
    for o, word in ((dict(trans=1, solve_baseflow=1), "trans with solve_baseflow"), (dict(r=0), "out of range"), (dict(r=5), "out of range"),
                    (dict(r=4, solve_baseflow=1), "out of range")):
        with pytest.raises(host.NlgError, match=word):
            create(A, **o)
    # cfg.ifheat
    bT = host.nek_dvector(gm, 1, 3)
    H = host.exptA_linop(kw["tau"], bT, pprecond=1, pproj=0, ifheat=1, **{k: v for k, v in kw.items() if k != "tau"})
    with pytest.raises(host.NlgError, match="ifheat"):
        create(H)
    H.close()
    # wavenumber projection
    from neklab_amd.mesh import box_mesh
    gm2 = host.Mesh(gpu_ctx, box_mesh((3, 3), 6, lengths=(1.0, 1.0)))          # (lines along x need a mesh that is not deformed)
    b2 = host.nek_dvector(gm2)
    b2.set_field(0, 1.0 - (2.0 * np.asarray(gm2.host.y).ravel() - 1.0) ** 2)
    P = host.exptA_proj_linop(kw["tau"], b2, 2.0, idir=1, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    P.init()
    with pytest.raises(host.NlgError, match="wavenumber projection"):
        create(P)
    P.close()
    # orbit mode
    Ob = host.exptA_orbit_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    with pytest.raises(host.NlgError, match="orbit mode"):
        create(Ob)
    Ob.close()
    # while an nlg_otd lives on the operator
    h = create(A, r=2)                                   # basis0 = NULL: random lanes, seeds 1, 2
    lab = host.line_labels(gm, 1)
    x, y = host.nek_dvector(gm), host.nek_dvector(gm)
    x.rand(True, seed=3)
    calls = [lambda: A.matvec(x, y), lambda: A.rmatvec(x, y), lambda: A.matvec_block([x], [y]),
             lambda: host.integrate_forced(A, None, x, None, 1.0, False, y),
             lambda: host.check(lib.nlg_linop_set_baseflow(A.h, gX0.h)), lambda: host.check(lib.nlg_linop_set_tolerances(A.h, 1e-8, 1e-8)),
             lambda: host.check(lib.nlg_linop_set_tau(A.h, 0.1)), lambda: host.check(lib.nlg_linop_set_orbit(A.h, gX0.h, 0.1)),
             lambda: host.check(lib.nlg_linop_nonlinear_map(A.h, x.h, y.h)), lambda: create(A),
             lambda: host.check(lib.nlg_linop_set_projection(A.h, 2.0, 1, lab.ctypes.data_as(host._lib.c_int64_p), None, None)),
             lambda: A.init(), lambda: host.check(lib.nlg_linop_destroy(A.h))]
    for call in calls:
        with pytest.raises(host.NlgError, match="nlg_otd"):
            call()
    host.check(lib.nlg_otd_advance(h, 2))                # ... and the run itself is unharmed
    Lr = np.zeros((2, 2), order="F")
    host.check(lib.nlg_otd_reduced(h, host.dptr(Lr), None))
    assert np.all(np.isfinite(Lr))
    host.check(lib.nlg_otd_destroy(h))
    A.matvec(x, y)                                       # after destroy the operator does matvecs again
    assert np.isfinite(y.norm()) and y.norm() > 0
    A.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the operator after a run, a dependent basis, the analysis loop
# ---------------------------------------------------------------------------------------------------------------------
def test_operator_is_its_own_again_after_a_coupled_run(gpu_ctx):
    """a run with solve_baseflow rebuilds the convective factors from the moving base flow in every step; after destroy a matvec
    on the caller's operator is bit for bit the matvec before the run, and a frozen OTD run on it equals one on a fresh operator"""
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    gX0 = upload(gm, fr.orbit_state("A"))
    lib = gm.lib
    A = host.exptA_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    A.init()
    x, y0, y1 = host.nek_dvector(gm), host.nek_dvector(gm), host.nek_dvector(gm)
    x.rand(True, seed=5)
    A.matvec(x, y0)
    B = [upload(gm, b) for b in otd_ref.orthonormal_basis(sem, 2)]

    def run(op, coupled, nsteps):
        o = host._lib.OtdOpts()
        host.check(lib.nlg_otd_opts_default(C.byref(o)))
        o.r, o.solve_baseflow = 2, int(coupled)
        h = host.vp()
        host.check(lib.nlg_otd_create(op.h, C.byref(o), (host.vp * 2)(*[b.h for b in B]), C.byref(h)))
        host.check(lib.nlg_otd_advance(h, nsteps))
        Lr = np.zeros((2, 2), order="F")
        host.check(lib.nlg_otd_reduced(h, host.dptr(Lr), None))
        host.check(lib.nlg_otd_destroy(h))
        return Lr

    Lc = run(A, True, 4)
    A.matvec(x, y1)
    d = max(np.max(np.abs(y1.get_field(i, r) - y0.get_field(i, r))) for i in range(2) for r in range(3))
    Lf = run(A, False, 4)
    F = host.exptA_linop(kw["tau"], gX0, pprecond=1, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    Lf_fresh = run(F, False, 4)
    print("matvec after a coupled OTD run against before: %.3e; frozen Lr on the used operator against a fresh one: %.3e; coupled against "
          "frozen Lr: %.3e" % (d, np.abs(Lf - Lf_fresh).max(), np.abs(Lc - Lf).max()))
    A.close()
    F.close()
    assert d == 0.0
    assert np.array_equal(Lf, Lf_fresh)
    assert np.abs(Lc - Lf).max() > 1e-6 * np.abs(Lf).max()        # (the coupled run did move the base flow)


def test_dependent_basis_is_an_error_not_a_silent_run(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    b = upload(gm, otd_ref.orthonormal_basis(sem, 1)[0])
    O = host.nek_otd(upload(gm, fr.orbit_state("A")), 2, pprecond=1, pproj=0, **fr.case_cfg("A"))
    with pytest.raises(host.NlgError, match="not positive definite"):
        O.init(host.otd_opts(solve_baseflow=False), basis0=[b, host.nek_dvector(gm)])      # the second mode is the zero vector
    O.close()


def test_otd_analysis_loop_files_and_rows(gpu_ctx, tmp_path):
    """six steps of case A with printstep 2, iostep 4, iorststep 3, the first mode read from OTDIC_01.fld: rows, Ls.dat / Lr.dat lines,
    mode and restart files, and the same numbers as stepping by hand"""
    from neklab_amd import nekio
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")
    gX0 = upload(gm, fr.orbit_state("A"))
    ic = upload(gm, otd_ref.orthonormal_basis(sem, 1)[0])
    ic.set_field(host.PR, np.zeros(gm.lpn))
    E = hm.E
    nekio.write_fld(str(tmp_path / "OTDIC_01.fld"), hm.n, 2, coords=[np.asarray(hm.x).reshape(E, -1), np.asarray(hm.y).reshape(E, -1)],
                    vel=[ic.get_field(i).reshape(E, -1) for i in range(2)], p=np.zeros((E, hm.n ** 2)))
    opts = host.otd_opts(printstep=2, iostep=4, iorststep=3, orthostep=10, n_usrIC=1, solve_baseflow=False)
    O = host.nek_otd(gX0, 2, pprecond=1, pproj=0, **kw)
    rows = host.otd_analysis(O, opts, nsteps=6, outdir=str(tmp_path))
    assert O.info()["istep"] == 6 and abs(O.info()["dt"] - fr.DT) < 1e-15
    assert [r["istep"] for r in rows] == [2, 4, 6] and np.allclose([r["time"] for r in rows], [0.02, 0.04, 0.06], atol=1e-14)
    ls = open(tmp_path / "Ls.dat").read().splitlines()
    lr = open(tmp_path / "Lr.dat").read().splitlines()
    assert len(ls) == 3 and len(lr) == 3
    for k, row in enumerate(rows):
        assert ls[k] == host.otd_log_line(row["istep"], row["time"], (" Ls ", row["sigma"]))
        assert lr[k] == host.otd_log_line(row["istep"], row["time"], (" Lr%Re ", row["lambda"].real), (" Lr%Im ", row["lambda"].imag))
        assert np.all(np.diff(row["sigma"]) <= 0) and np.all(np.diff(row["lambda"].real) <= 1e-14)
    for name in ("m01neklab0.f00001", "m02neklab0.f00001", "rstneklab0.f00001", "rstneklab0.f00002", "rstneklab0.f00003", "rstneklab0.f00004"):
        assert (tmp_path / name).exists(), name
    # the restart files of step 6 hold the basis as it stands
    f = nekio.read_fld(str(tmp_path / "rstneklab0.f00004"))
    assert np.max(np.abs(f["ux"].ravel() - O.basis(1).get_field(0))) <= 1e-15
    # the same run by hand: the same read-outs at the same steps
    v2 = host.nek_dvector(gm)
    v2.rand(True, seed=2)
    P = host.nek_otd(gX0, 2, pprecond=1, pproj=0, **kw)
    P.init(opts, basis0=[ic, v2])
    hand = []
    for n in (2, 1, 1, 2):                               # read-outs at 2, (3: restart files only), 4, 6
        P.advance(n)
        if P.info()["istep"] != 3:
            hand.append(P.spectral_analysis(P.reduced()[0])[0])
    e = max(np.abs(hand[k] - rows[k]["sigma"]).max() for k in range(3))
    print("otd_analysis against the same steps by hand: sigma differs by %.3e; sigma at step 6: %s" % (e, rows[2]["sigma"]))
    O.close()
    P.close()
    assert e <= 1e-12 * np.abs(rows[2]["sigma"]).max()
