"""DNS runs with history points and a recurrence monitor on the GPU (nlg_dns_*; host.nek_dns), with the settings of the Floquet tests:
Re = 50, dt = 0.01, solves converged to 1e-13, Jacobi pressure preconditioner, no pressure projection.  Case A: 2-D, 7 steps.  Case B:
3-D, 4 steps.  Six history points each, a face point and a wall point among them.

Reference: tests/dns_ref.py (the oracle's nonlinear step, the twin's own Lagrange evaluation and recurrence norm).  Tolerances: a run
against the oracle 1e-10 of max|U| (history points) and of |U|_M (recurrence norm), the project's figure for a run against the oracle
(tests/test_gpu_floquet.py, tests/test_gpu_n8.py); the same launches in another grouping (advance(2) + advance(3), another ring length,
nonlinear_map): 1e-13 of scale, bit equality expected and printed.
"""
import ctypes as C

import numpy as np
import pytest

import dns_ref
import floquet_ref as fr
from neklab_amd import _lib, host
from oracle.lns import LNSConfig

pytestmark = pytest.mark.gpu

TOL = 1e-10
NSTEPS = {"A": 7, "B": 4}
_ref = {}


def upload(gm, ov):
    gv = host.nek_dvector(gm)
    for i in range(gm.dim):
        gv.set_field(i, ov.v[i])
    gv.set_field(host.PR, ov.pr)
    return gv


def gpu_cfg(name, **over):
    kw = {k: v for k, v in fr.case_cfg(name).items() if k != "tau"}
    kw.update(pprecond=1, pproj=0)
    kw.update(over)
    return kw


def six_points(name):
    hm, sem = fr.case_mesh(name)
    pts = [p for p in dns_ref.case_points(name, hm) if p[2] == 0][:6]
    labels = [p[0] for p in pts]
    assert "face" in labels and "wall" in labels
    return np.array([p[1] for p in pts]), labels


def reference(name):
    """the twin's run, computed once (the location comes from the host library: it needs no GPU)"""
    if name not in _ref:
        hm, sem = fr.case_mesh(name)
        xyz, labels = six_points(name)
        loc = host.locate_points(hm, xyz)
        X0 = fr.orbit_state(name)
        _ref[name] = (X0, xyz, labels, dns_ref.run(sem, LNSConfig(**fr.case_cfg(name)), X0, NSTEPS[name], loc["elem"], loc["rst"]))
    return _ref[name]


def fields_diff(a, b, dim):
    sc = max(np.abs(b.get_field(i)).max() for i in range(dim))
    d = max(np.max(np.abs(a.get_field(i) - b.get_field(i))) for i in list(range(dim)) + [host.PR])
    return d / sc, all(np.array_equal(a.get_field(i), b.get_field(i)) for i in list(range(dim)) + [host.PR])


def counters(ctx):
    a, b = C.c_int64(0), C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


@pytest.mark.parametrize("name", ["A", "B"])
def test_series_against_the_twin(gpu_ctx, name):
    hm, sem = fr.case_mesh(name)
    X0, xyz, labels, ref = reference(name)
    n, dim = NSTEPS[name], sem.dim
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, X0)
    dns = host.nek_dns(gX0, **gpu_cfg(name))
    hp = host.history_points(gm, xyz)
    dns.set_history_points(hp)
    dns.set_reference()
    dns.advance(n)
    s = dns.series()
    info = dns.info()
    assert info["istep"] == n and abs(info["dt"] - ref["dt"]) < 1e-15 and abs(info["time"] - n * ref["dt"]) < 1e-14
    assert s["probe"].shape == (n + 1, 6, dim + 1) and s["time"].shape == s["dist"].shape == (n + 1,)
    assert np.max(np.abs(s["time"] - ref["time"])) < 1e-14
    umax = max(np.abs(a).max() for a in X0.v)
    unorm = X0.norm()
    ev = np.abs(s["probe"][:, :, :dim] - ref["probe"][:, :, :dim]).max() / umax
    ep = np.abs(s["probe"][:, :, dim] - ref["probe"][:, :, dim]).max() / umax
    ed = np.abs(s["dist"] - ref["dist"]).max() / unorm
    print("case %s, %d steps: history points velocity %.3e, pressure %.3e (of max|U| = %.3f); d(t) %.3e (of |U| = %.3f); d = %s"
          % (name, n, ev, ep, umax, ed, unorm, ["%.4e" % d for d in s["dist"]]))
    # sample 0 is X0 at t = 0, at distance 0 from itself
    assert s["time"][0] == 0.0 and s["dist"][0] == 0.0
    assert np.array_equal(s["probe"][0], hp.sample(gX0))
    # the velocity on the wall is exactly zero in every sample
    w = labels.index("wall")
    assert np.all(s["probe"][:, w, :dim] == 0.0)
    assert np.all(s["dist"][1:] > 0.0)
    assert ev <= TOL and ep <= TOL and ed <= TOL
    # the final state: against the twin, and against nonlinear_map of a second operator over tau = nsteps dt
    end = dns.state()
    etw = max(np.max(np.abs(end.get_field(i).reshape(sem.shape1) - ref["state"].v[i])) for i in range(dim)) / umax
    A = host.exptA_linop(n * fr.DT, gX0, **gpu_cfg(name))
    A.init()
    out = host.nek_dvector(gm)
    host.check(A.lib.nlg_linop_nonlinear_map(A.h, gX0.h, out.h))
    out.axpby(1.0, gX0, 1.0)
    e_map, same = fields_diff(end, out, dim)
    print("case %s final state: against the twin %.3e; against X0 + nonlinear_map(X0): %.3e (%s)" % (name, etw, e_map, "bit-equal" if same else "not bit-equal"))
    assert etw <= TOL and e_map <= 1e-13
    A.close(), dns.close(), hp.close()


def test_grouping_of_the_steps_and_ring_length_do_not_matter(gpu_ctx):
    name = "A"
    hm, sem = fr.case_mesh(name)
    X0, xyz, labels, ref = reference(name)
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, X0)
    hp = host.history_points(gm, xyz)

    def run(groups, chunk):
        dns = host.nek_dns(gX0, chunk=chunk, **gpu_cfg(name))
        dns.set_history_points(hp)
        dns.set_reference(gX0)
        for g in groups:
            dns.advance(g)
        s, end = dns.series(), dns.state()
        dns.close()
        return s, end

    s0, end0 = run([5], 256)
    for groups, chunk in (([2, 3], 256), ([5], 2), ([1, 1, 3], 3)):
        s, end = run(groups, chunk)
        e_state, same_state = fields_diff(end, end0, sem.dim)
        sc = np.abs(s0["probe"]).max()
        ep, ed = np.abs(s["probe"] - s0["probe"]).max() / sc, np.abs(s["dist"] - s0["dist"]).max() / s0["dist"].max()
        same = same_state and np.array_equal(s["probe"], s0["probe"]) and np.array_equal(s["dist"], s0["dist"])
        print("advance%s chunk %d against advance(5) chunk 256: state %.1e, history points %.1e, d(t) %.1e (%s)"
              % (groups, chunk, e_state, ep, ed, "bit-equal" if same else "not bit-equal"))
        assert np.array_equal(s["time"], s0["time"])
        assert e_state <= 1e-13 and ep <= 1e-13 and ed <= 1e-13
    hp.close()


def test_monitors_cost_at_most_three_launches_per_step(gpu_ctx):
    name = "B"
    hm, sem = fr.case_mesh(name)
    X0, xyz, labels, ref = reference(name)
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, X0)
    hp = host.history_points(gm, xyz)

    def cost(monitors):
        dns = host.nek_dns(gX0, **gpu_cfg(name))
        if monitors:
            dns.set_history_points(hp)
            dns.set_reference()
        dns.advance(0)                       # sample 0
        l0, c0 = counters(gpu_ctx)
        dns.advance(5)
        l1, c1 = counters(gpu_ctx)
        dns.close()
        return l1 - l0, c1 - c0

    (lm, cm), (ln, cn) = cost(True), cost(False)
    print("5 steps on B: launches %d with both monitors, %d without (%.1f per step more); collectives %d and %d" % (lm, ln, (lm - ln) / 5.0, cm, cn))
    assert 0 < lm - ln <= 3 * 5
    assert cm == cn
    hp.close()


def test_refusals(gpu_ctx):
    hm, sem = fr.case_mesh("A")
    gm, gm2 = host.Mesh(gpu_ctx, hm), host.Mesh(gpu_ctx, hm)
    gX0 = upload(gm, fr.orbit_state("A"))
    kw = gpu_cfg("A")

    def create(op, X):
        o = _lib.DnsOpts()
        host.check(op.lib.nlg_dns_opts_default(C.byref(o)))
        assert o.chunk == 256
        h = host.vp()
        host.check(op.lib.nlg_dns_create(op.h, X.h, C.byref(o), C.byref(h)))
        return h

    orbit = host.exptA_orbit_linop(5 * fr.DT, gX0, **kw)
    with pytest.raises(host.NlgError, match="orbit mode"):
        create(orbit, gX0)
    orbit.close()
    otd = host.nek_otd(gX0, r=2, **kw)
    otd.init()
    with pytest.raises(host.NlgError, match="nlg_otd"):
        create(otd.op, gX0)
    otd.close()
    proj = host.exptA_proj_linop(5 * fr.DT, gX0, alpha=2.0 * np.pi, idir=1, **kw)
    proj.init()
    with pytest.raises(host.NlgError, match="projection"):
        create(proj, gX0)
    proj.close()
    A = host.exptA_linop(5 * fr.DT, gX0, **kw)
    with pytest.raises(host.NlgError, match="different mesh"):
        create(A, host.nek_dvector(gm2))
    with pytest.raises(host.NlgError, match="scalar"):
        create(A, host.nek_dvector(gm, nscal=1))
    # while a run lives on the operator its other runs are refused; afterwards the operator is the propagator about X0 again
    A.init()
    v, y0, y1 = host.nek_dvector(gm), host.nek_dvector(gm), host.nek_dvector(gm)
    v.rand(True, seed=4)
    A.matvec(v, y0)
    dns = host.nek_dns(gX0, op=A)
    with pytest.raises(host.NlgError, match="already lives"):
        create(A, gX0)
    for call in (lambda: A.matvec(v, y1), lambda: A.init(), lambda: host.check(A.lib.nlg_linop_nonlinear_map(A.h, gX0.h, y1.h)),
                 lambda: host.check(A.lib.nlg_linop_set_tau(A.h, 0.1))):
        with pytest.raises(host.NlgError, match="nlg_dns lives"):
            call()
    o = _lib.OtdOpts()
    host.check(A.lib.nlg_otd_opts_default(C.byref(o)))
    h = host.vp()
    with pytest.raises(host.NlgError, match="nlg_dns"):
        host.check(A.lib.nlg_otd_create(A.h, C.byref(o), None, C.byref(h)))
    assert A.lib.nlg_linop_destroy(A.h) != 0                       # refused, nothing freed
    hp = host.history_points(gm, six_points("A")[0])
    dns.set_history_points(hp)
    with pytest.raises(host.NlgError, match="samples these points"):
        hp.close()
    dns.advance(2)
    assert dns.series()["probe"].shape == (3, 6, 3)
    dns.close()
    hp.close()
    A.matvec(v, y1)
    e, same = fields_diff(y1, y0, sem.dim)
    print("matvec after the run against matvec before it: %.3e (%s)" % (e, "bit-equal" if same else "not bit-equal"))
    assert e <= 1e-13
    A.close()
