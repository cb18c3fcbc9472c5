"""Block resolvent: forced integration of s <= 4 lanes (nlg_linop_integrate_forced_block) against the oracle and against the single
call, one forcing launch per time step, refusals; the conjugate convention of resolvent_matvec and the linear pair built on it;
block applications (block GMRES) against single ones; the randomised SVD on the block path."""
import ctypes as C

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.lns import ExptA, LNSConfig
from test_gpu_resolvent import case

pytestmark = pytest.mark.gpu

OMEGA, RE = 8.0, 20.0
TAU = 2 * np.pi / OMEGA
KW = dict(re=RE, torder=3, vtol=1e-12, ptol=1e-12, maxit_v=400, maxit_p=4000)


def box8(ctx):
    """The 3-D 2 x 2 x 2 box at lx1 = 8 (the lx1 = 8 kernels), a base flow and two complex forcings."""
    hm = box_mesh((2, 2, 2), 8, lengths=(2.0, 1.0, 1.0), periodic=(True, False, True), deform=0.03)
    gm = host.Mesh(ctx, hm)
    X = [hm.x, hm.y, hm.z]
    gb = host.nek_dvector(gm)
    gb.set_field(0, hm.mask[0] * (4 * X[1] * (1 - X[1])))
    fz = []
    for k in range(3):
        z = host.nek_zvector(gm)
        for i in range(3):
            z.re.set_field(i, hm.mask[i] * np.sin(np.pi * X[0] + i + k) * np.sin(np.pi * X[1]) * np.cos(2 * np.pi * X[2] * k))
            z.im.set_field(i, hm.mask[i] * np.cos(np.pi * X[0] * (1 + k)) * np.sin(2 * np.pi * X[1]))
        fz.append(z)
    return hm, gm, gb, fz


def lanes_of_case(gm, fz):
    """Three lanes from the forcing of test_gpu_resolvent.case: (re, im), (im, -) real-forced, (im, re)."""
    return [fz.re, fz.im, fz.im], [fz.im, None, fz.re]


def upload(gm, ov):
    g = host.nek_dvector(gm)
    for i in range(gm.dim):
        g.set_field(i, ov.v[i])
    g.set_field(host.PR, ov.pr)
    return g


def fields(v, dim):
    return [v.get_field(i) for i in range(dim)] + [v.get_field(host.PR)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the forced block run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,adjoint", [(2, False), (2, True), (3, False), (3, True)])
def test_forced_block_matches_oracle_lane_by_lane(gpu_ctx, dim, adjoint):
    """Lane 0 complex-forced from rest, lane 1 real-forced from rest (no f_im), lane 2 complex-forced from a state with velocity and
    pressure (lane 1's result): each within 1e-9 scale of the oracle's run, the bound of test_gpu_resolvent.py."""
    hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, dim)
    oA = ExptA(sem, U, LNSConfig(tau=TAU, **KW))
    nsteps = oA.nsteps
    o0 = oA.integrate_forced(None, fre, fim, OMEGA, adjoint)
    o1 = oA.integrate_forced(None, fim, None, OMEGA, adjoint)
    ob = (o0, o1, oA.integrate_forced(o1.copy(), fim, fre, OMEGA, adjoint))
    A = host.exptA_linop(TAU, gb, **KW)
    A.init()
    assert A.info()["nsteps"] == nsteps
    f_re, f_im = lanes_of_case(gm, fz)
    outs = [host.nek_dvector(gm) for _ in range(3)]
    host.integrate_forced_block(A, [None, None, upload(gm, ob[1])], f_re, f_im, OMEGA, adjoint, outs)
    for v in range(3):
        sc = max(np.abs(a).max() for a in ob[v].v)
        for i in range(dim):
            err = np.max(np.abs(outs[v].get_field(i).reshape(sem.shape1) - ob[v].v[i]))
            assert err < 1e-9 * sc, (v, i, err, sc)
        assert outs[v].nrst == 0


@pytest.mark.parametrize("which,adjoint,pprecond", [("2d", False, 0), ("2d", True, 1), ("3d", False, 1), ("3d", True, 1), ("box8", False, 0), ("box8", True, 0)])
def test_forced_block_equals_single_calls(gpu_ctx, which, adjoint, pprecond):
    """Every lane of a block of three is the single call with the same arguments: 1e-11 relative on the velocity and 1e-9 on the
    pressure (the block-against-single bounds of tests/test_gpu_block.py), with the iteration counts of the single run at every
    time step -- equal under the Jacobi preconditioner (pprecond = 1, tolerance mode: a lane that read another lane's data would
    converge differently), within one otherwise (the Schwarz kernels sum in a lane-dependent order, and a residual that lands on
    the tolerance may take one iteration more or less).  The block of one IS the single call: bit for bit.
    The lx1 = 8 box runs under the Schwarz preconditioner only: on a small mesh at lx1 = 8 the SINGLE call's pressure operator is
    another kernel (k_opgradt3w / k_opdiv3w, three waves per element) than the lane path's (k_opgradt3n / k_opdiv3n), so equal counts
    are not a property of the code there (measured under Jacobi: 254 against 255 pressure iterations in the first step of lane 0)."""
    if which != "box8":
        hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, int(which[0]))
        f_re, f_im = lanes_of_case(gm, fz)
    else:
        hm, gm, gb, z = box8(gpu_ctx)
        f_re, f_im = [z[0].re, z[1].re, z[2].re], [z[0].im, None, z[2].im]
    dim = gm.dim
    A = host.exptA_linop(TAU, gb, pprecond=pprecond, **KW)
    A.init()
    ns = A.info()["nsteps"]
    ic2 = host.nek_dvector(gm)
    host.integrate_forced(A, None, f_re[1], None, OMEGA, adjoint, ic2)           # a state with velocity and pressure
    ics = [None, None, ic2]
    single, iters = [], []
    for v in range(3):
        o = host.nek_dvector(gm)
        host.integrate_forced(A, ics[v], f_re[v], f_im[v], OMEGA, adjoint, o)
        single.append(o)
        iters.append([A.lane_iters(0, k) for k in range(1, ns + 1)])
    blk = [host.nek_dvector(gm) for _ in range(3)]
    host.integrate_forced_block(A, ics, f_re, f_im, OMEGA, adjoint, blk)
    slack = 0 if pprecond == 1 else 1
    for v in range(3):
        sc = max(np.abs(single[v].get_field(i)).max() for i in range(dim))
        for i in range(dim):
            assert np.max(np.abs(blk[v].get_field(i) - single[v].get_field(i))) < 1e-11 * sc, (v, i)
        ps = single[v].get_field(host.PR)
        assert np.max(np.abs(blk[v].get_field(host.PR) - ps)) < 1e-9 * max(sc, np.abs(ps).max()), v
        for k in range(1, ns + 1):
            b, a = A.lane_iters(v, k), iters[v][k - 1]
            assert abs(b["v_iters"] - a["v_iters"]) <= slack and abs(b["p_iters"] - a["p_iters"]) <= slack, (v, k, a, b)
    one = host.nek_dvector(gm)
    host.integrate_forced_block(A, [ics[2]], [f_re[2]], [f_im[2]], OMEGA, adjoint, [one])
    assert all(np.array_equal(a, b) for a, b in zip(fields(one, dim), fields(single[2], dim)))
    for k in range(1, ns + 1):
        assert A.lane_iters(0, k) == iters[2][k - 1]


def test_forcing_is_one_launch_per_step_whatever_s(gpu_ctx):
    """By nlg_counters, history-free operator, fixed iteration counts, every lane with an initial condition: a forced run costs the
    launches of the matvec from the same states plus ONE per time step, for one lane and for three -- so going from one lane to three
    costs a forced run exactly what it costs a matvec.  The forcings are zero vectors: a PCG whose residual reaches the rounding
    floor before its fixed count stops launching, which depends on the data (measured with the forcings of `case`: the unforced
    matvecs run 30 and 28 launches short of 20 full steps, the forced runs none), and with a zero forcing every solve of the
    forced run is bit for bit the matvec's."""
    hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, 2)
    A = host.exptA_linop(TAU, gb, no_history=1, dt=TAU / 20, fixed_iters_v=10, fixed_iters_p=30, **KW)
    A.init()
    ns = A.info()["nsteps"]
    zero = host.nek_dvector(gm)
    f_re, f_im = [zero] * 3, [zero, None, zero]
    x = []
    for v in range(3):
        a = host.nek_dvector(gm)
        a.rand(True, seed=5 + v)
        x.append(a)
    y = [host.nek_dvector(gm) for _ in range(3)]

    def launches(run):
        run()                                                  # (first use of a lane count sizes the slab)
        a, b = C.c_int64(0), C.c_int64(0)
        host.check(gpu_ctx.lib.nlg_counters(C.byref(a), None))
        run()
        host.check(gpu_ctx.lib.nlg_counters(C.byref(b), None))
        return b.value - a.value, [f.copy() for f in fields(y[0], 2)]

    f1, yf1 = launches(lambda: host.integrate_forced(A, x[0], f_re[0], f_im[0], OMEGA, False, y[0]))
    f3, yf3 = launches(lambda: host.integrate_forced_block(A, x, f_re, f_im, OMEGA, False, y))
    m1, ym1 = launches(lambda: A.matvec(x[0], y[0]))
    m3, ym3 = launches(lambda: A.matvec_block(x, y))
    print("launches per run of %d steps: forced 1 lane %d, 3 lanes %d; matvec 1 lane %d, 3 lanes %d" % (ns, f1, f3, m1, m3))
    assert all(np.array_equal(a, b) for a, b in zip(yf1 + yf3, ym1 + ym3))      # the same runs, but for the forcing kernel
    assert f1 - m1 == ns and f3 - m3 == ns                     # one launch per step whatever s is
    assert f3 - f1 == m3 - m1


def test_forced_block_refusals(gpu_ctx):
    hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, 2)
    A = host.exptA_linop(TAU / 4, gb, **KW)
    A.init()
    f_re, f_im = lanes_of_case(gm, fz)
    o = [host.nek_dvector(gm) for _ in range(5)]
    x = host.nek_dvector(gm)
    x.rand(True, seed=3)
    ref = host.nek_dvector(gm)
    A.matvec(x, ref)

    def refused(*a):
        with pytest.raises(host.NlgError, match="integrate_forced"):
            host.integrate_forced_block(A, *a)
        y = host.nek_dvector(gm)                               # nothing refused disturbs a following matvec
        A.matvec(x, y)
        assert all(np.array_equal(p, q) for p, q in zip(fields(y, 2), fields(ref, 2)))

    refused(None, [], None, OMEGA, False, [])                                          # s = 0
    refused(None, [fz.re] * 5, None, OMEGA, False, o)                                  # s = 5
    refused(None, [fz.re, None], None, OMEGA, False, o[:2])                            # a NULL forcing
    refused(None, [fz.re, fz.im], None, OMEGA, False, [o[0], None])                    # a NULL output
    refused(None, [fz.re, fz.im], [None, o[0]], OMEGA, False, o[:2])                   # output 0 is the forcing of lane 1
    refused([None, o[0]], [fz.re, fz.im], None, OMEGA, False, o[:2])                   # ... the initial condition of lane 1
    refused(None, [fz.re, fz.im], None, OMEGA, False, [o[0], o[0]])                    # the same output twice
    with pytest.raises(host.NlgError, match="integrate_forced"):                      # what the single call refuses, same message
        host.integrate_forced(A, None, fz.re, None, OMEGA, False, fz.re)
    Ob = host.exptA_orbit_linop(TAU / 4, gb, **KW)
    with pytest.raises(host.NlgError, match="integrate_forced.*orbit"):
        host.integrate_forced_block(Ob, None, [fz.re, fz.im], None, OMEGA, False, o[:2])
    with pytest.raises(host.NlgError, match="integrate_forced.*orbit"):
        host.integrate_forced(Ob, None, fz.re, None, OMEGA, False, o[0])
    B = host.exptA_linop(TAU / 4, gb, **KW)                                            # no init
    with pytest.raises(host.NlgError, match="integrate_forced.*nlg_linop_init"):
        host.integrate_forced_block(B, None, [fz.re], None, OMEGA, False, o[:1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the convention of resolvent_matvec, and the linear pair
# ---------------------------------------------------------------------------------------------------------------------
def zmax(z, dim):
    return max(max(np.abs(z.re.get_field(i)).max(), np.abs(z.im.get_field(i)).max()) for i in range(dim))


def zdiff(a, b, dim):
    """max |a - b| over the velocity fields of both parts"""
    return max(max(np.abs(a.re.get_field(i) - b.re.get_field(i)).max(), np.abs(a.im.get_field(i) - b.im.get_field(i)).max()) for i in range(dim))


# One-step scheme on a step that divides the quarter period: the forced time stepper is then a time-invariant linear recurrence
# u_{k+1} = M u_k + B Re[f exp(i omega t_k)] whose periodic solution is Re[z exp(i omega t_k)] with z = (exp(i omega dt) - M)^-1 B f,
# so what the operator returns is complex (anti)linear in f up to the GMRES tolerance.  With bdf3 every run starts impulsively at
# orders 1, 2, 3 and the quarter period takes a step of its own (21 and 6 steps here), so the same identities hold only up to the
# time-discretisation error, (omega dt)^p: measured below, and the reason the convention is pinned on this configuration.
KW_LTI = dict(KW, torder=1, dt=TAU / 20)


def convention_figures(R, f, g, gm):
    """(|matvec(i f) + i matvec(f)|, |rmatvec(i g) - i rmatvec(g)|) over the scale of the result, the same two with the other sign,
    the duality defect of the linear pair and that of the pair built on matvec itself."""
    dev, other = [], []
    for name, x, sign in (("matvec", f, -1.0), ("rmatvec", g, 1.0)):
        jx = x.copy()
        jx.scal(1j)
        a, b = host.nek_zvector(gm), host.nek_zvector(gm)
        getattr(R, name)(x, a)
        getattr(R, name)(jx, b)
        want, wrong = a.copy(), a.copy()
        want.scal(sign * 1j)
        wrong.scal(-sign * 1j)
        sc = zmax(a, gm.dim)
        dev.append(zdiff(b, want, gm.dim) / sc)
        other.append(zdiff(b, wrong, gm.dim) / sc)
    Rf, RHg = host.nek_zvector(gm), host.nek_zvector(gm)
    R.apply_linear_block([f], [Rf], False)
    R.apply_linear_block([g], [RHg], True)
    rhs = RHg.dot(f)                                           # (R^H g)^H f, against g^H (R f)
    defect = abs(g.dot(Rf) - rhs) / (Rf.norm() * g.norm())
    Rf.conj()                                                  # what a pair built on matvec itself would compare
    return dev, other, defect, abs(g.dot(Rf) - rhs) / (Rf.norm() * g.norm())


def test_matvec_is_antilinear_rmatvec_linear_and_the_pair_is_adjoint(gpu_ctx):
    """resolvent_matvec returns conj(R f): matvec(i f) = -i matvec(f), while rmatvec(i g) = +i rmatvec(g), each within 2e-5 scale (two
    GMRES solutions at rtol 1e-6, as test_gpu_resolvent.py) where the stepper is a time-invariant recurrence (KW_LTI).  The linear
    pair of apply_linear_block is then adjoint up to the discretisation error of the continuous adjoint: defect
    |<R f, g> - <f, R^H g>| / (|R f| |g|) < 0.05, in both configurations (the wrong conjugation gives O(1)).
    Measured: bdf1 on T / 20: 1.3e-6 and 4.2e-7 of scale (the other sign: 2.0), defect 1.4e-3 (pair built on matvec
    itself: 0.44); bdf3 on the CFL step: 3.6e-2 and 6.1e-2, the time-discretisation error, defect 2.8e-2 (0.29)."""
    hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, 2)
    g = host.nek_zvector(gm)                                   # smooth like f, so that <R f, g> is not small beside |R f| |g| ...
    g.rand(4)
    g.scal(0.1 * fz.norm() / g.norm())                         # ... plus a tenth of noise
    g.re.axpby(1.0, fz.im, 1.0)
    g.im.axpby(1.0, fz.re, 1.0)
    dev, other, defect, wrong = convention_figures(host.resolvent_linop(OMEGA, gb, **KW_LTI), fz, g, gm)
    print("bdf1, dt = T / 20: matvec(i f) + i matvec(f) %.3e of scale (other sign %.3e), rmatvec(i g) - i rmatvec(g) %.3e (%.3e); "
          "duality defect %.3e (unconjugated matvec: %.3e)" % (dev[0], other[0], dev[1], other[1], defect, wrong))
    assert dev[0] < 2e-5 and dev[1] < 2e-5
    assert defect < 0.05
    dev3, other3, defect3, wrong3 = convention_figures(host.resolvent_linop(OMEGA, gb, **KW), fz, g, gm)
    print("bdf3, CFL step: matvec(i f) + i matvec(f) %.3e of scale (other sign %.3e), rmatvec(i g) - i rmatvec(g) %.3e (%.3e); "
          "duality defect %.3e (unconjugated matvec: %.3e)" % (dev3[0], other3[0], dev3[1], other3[1], defect3, wrong3))
    assert defect3 < 0.05
    assert 10 * max(dev3) < min(other3)                        # the sign of the convention does not depend on the scheme


# ---------------------------------------------------------------------------------------------------------------------
# 3. block applications and the analysis
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [False, True])
def test_block_application_matches_single_applications(gpu_ctx, adjoint):
    """s = 2, rtol 1e-9 on both sides: within 1e-6 scale for re and im.  Each side is within atol |(I - Phi_T)^-1| ~ 1e-9 |b| 3 of the
    exact solution (the slowest mode decays by exp(-pi^2 T / Re) ~ 0.68 per period); three orders of margin cover the
    norm-to-maximum conversion; a swapped lane or a wrong phase shows at 1e-3 or more.  Direct: the 2 x 2 x 2 box at lx1 = 8."""
    if adjoint:
        hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, 2)
        g = host.nek_zvector(gm)
        g.rand(4)
        vs = [fz, g]
    else:
        hm, gm, gb, z = box8(gpu_ctx)
        vs = z[:2]
    dim = gm.dim
    R = host.resolvent_linop(OMEGA, gb, rtol=1e-9, **KW)
    single = [host.nek_zvector(gm) for _ in range(2)]
    for v in range(2):
        (R.rmatvec if adjoint else R.matvec)(vs[v], single[v])
    n1 = R.gmres_matvecs
    blk = [host.nek_zvector(gm) for _ in range(2)]
    (R.rmatvec_block if adjoint else R.matvec_block)(vs, blk)
    print("GMRES matvecs: two single applications %d, the block of two %d" % (n1, R.gmres_matvecs - n1))
    for v in range(2):
        sc = zmax(single[v], dim)
        err = zdiff(blk[v], single[v], dim)
        print("lane %d: block against single %.3e of scale" % (v, err / sc))
        assert err < 1e-6 * sc, (v, err, sc)
    assert zdiff(blk[0], single[1], dim) > 1e-3 * zmax(single[1], dim)     # (the two lanes are different problems)


class SingleApplications:
    """apply_linear_block of a resolvent_linop through single applications only."""

    def __init__(self, R):
        self.R, self.mesh = R, R.mesh

    def apply_linear_block(self, vs, outs, adjoint=False):
        for v, o in zip(vs, outs):
            if adjoint:
                self.R.rmatvec(v, o)
            else:
                self.R.matvec(v, o)
                o.conj()


def test_resolvent_analysis_block_against_singles_and_triplet(gpu_ctx):
    """k = 2, q = 0, the same Omega: sigma on the block path against the same function driven by single applications within 1e-4
    relative at rtol 1e-9 (the application bound 1e-6 times 100 for the conditioning of the sample block).  Then, block only, k = 2,
    q = 1 at the default rtol 1e-6 on the time-invariant configuration KW_LTI: U orthonormal to 1e-10, and one extra single rmatvec
    gives |R^H u_1 - sigma_1 v_1| <= 20 rtol sigma_1 (the project's 2e-5 at 1e-6 ratio).  (With bdf3 on the CFL step R^H is complex
    linear only up to the time-discretisation error and the same figure is 3.2e-2.)"""
    hm, sem, gm, U, gb, fz, fre, fim = case(gpu_ctx, 2)
    Omega = []
    for i in range(2):
        z = host.nek_zvector(gm)
        z.rand(10 + i)
        Omega.append(z)
    R = host.resolvent_linop(OMEGA, gb, rtol=1e-9, **KW)
    sb, Ub, Vb = host.resolvent_analysis(R, 2, power_iters=0, Omega=Omega)
    ss, Us, Vs = host.resolvent_analysis(SingleApplications(R), 2, power_iters=0, Omega=Omega)
    rel = np.max(np.abs(sb - ss) / ss)
    print("sigma (block) %s, (singles) %s: relative difference %.3e" % (sb, ss, rel))
    assert sb[0] >= sb[1] > 0 and rel < 1e-4
    R6 = host.resolvent_linop(OMEGA, gb, **KW_LTI)             # (complex-linear to the GMRES tolerance: see KW_LTI)
    s1, U1, V1 = host.resolvent_analysis(R6, 2, power_iters=1, Omega=Omega)
    G = np.array([[a.dot(b) for b in U1] for a in U1])
    assert np.max(np.abs(G - np.eye(2))) < 1e-10
    y = host.nek_zvector(gm)
    R6.rmatvec(U1[0], y)
    y.axpby(-s1[0], V1[0], 1.0)
    print("q = 1: sigma %s (q = 0: %s); |R^H u1 - sigma1 v1| / sigma1 = %.3e" % (s1, sb, y.norm() / s1[0]))
    assert y.norm() <= 20 * R6.rtol * s1[0]
