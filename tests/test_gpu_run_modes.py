"""The drivers of the time stepper interleaved on ONE operator: every run starts from the same prologue and carries its mode (adjoint,
nonlinear, forcing) by value, so nothing of a run is left on the operator for the next one."""
import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

pytestmark = pytest.mark.gpu

KW = dict(re=30.0, torder=3, dt=0.01, vtol=1e-11, ptol=1e-11, maxit_v=400, maxit_p=4000)
TAU = 0.04          # 4 steps


def case(ctx, dim):
    if dim == 2:
        hm = box_mesh((3, 2), 6, lengths=(3.0, 2.0), periodic=(True, False), deform=0.03)
    else:
        hm = box_mesh((2, 2, 2), 6, lengths=(2.0, 1.0, 1.0), periodic=(True, False, True), deform=0.03)
    sem = SEM(hm)
    gm = host.Mesh(ctx, hm)
    rng = np.random.default_rng(7)

    def field(i, amp):
        return sem.mask[i] * sem.dsavg(amp * np.sin(np.pi * sem.X[0] + i) * np.sin(np.pi * sem.X[1]) + 0.1 * amp * rng.standard_normal(sem.shape1))

    vecs = []
    for amp in (1.0, 0.3, 0.5):          # base flow, perturbation, forcing
        v = host.nek_dvector(gm)
        for i in range(dim):
            v.set_field(i, field(i, amp))
        vecs.append(v)
    return sem, gm, vecs


def fields(v, dim):
    return [v.get_field(f, irst) for irst in range(v.nrst + 1) for f in list(range(dim)) + [host.PR]]


def run_other(A, gm, kind, x, f, adjoint):
    """one run of another kind on A; its result"""
    out = host.nek_dvector(gm)
    if kind == "integrate_forced":
        host.integrate_forced(A, x, f, None, 3.0, adjoint, out)
    else:
        host.check(A.lib.nlg_linop_nonlinear_map(A.h, x.h, out.h))
    return out


@pytest.mark.parametrize("kind", ["nonlinear_map", "integrate_forced"])
def test_lane_iters_reports_the_last_run(gpu_ctx, kind):
    """lane_iters(0) after a run of any kind = the iterations of that run alone (the difference of stats() around it), not the last
    matvec plus everything run since."""
    sem, gm, (U, x, f) = case(gpu_ctx, 2)
    A = host.exptA_linop(TAU, U, **KW)
    A.init()
    A.matvec(x, host.nek_dvector(gm))
    assert A.lane_iters(0)["v_iters"] > 0
    s0 = A.stats()
    run_other(A, gm, kind, x, f, False)
    s1 = A.stats()
    got = A.lane_iters(0)
    assert s1["steps"] - s0["steps"] == 4
    assert s1["v_iters"] > s0["v_iters"] and s1["p_iters"] > s0["p_iters"]
    assert got == {"v_iters": s1["v_iters"] - s0["v_iters"], "p_iters": s1["p_iters"] - s0["p_iters"]}


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", ["integrate_forced", "nonlinear_map"])
def test_a_run_leaves_no_mode_behind(gpu_ctx, dim, kind):
    """matvec -> adjoint forced integration (or nonlinear map, then the original base flow again) -> matvec -> rmatvec -> matvec on one
    operator: the three matvecs are bit for bit the matvec of a fresh operator."""
    sem, gm, (U, x, f) = case(gpu_ctx, dim)
    fresh = host.exptA_linop(TAU, U, **KW)
    fresh.init()
    want = host.nek_dvector(gm)
    fresh.matvec(x, want)
    want = fields(want, dim)
    assert len(want) == 3 * (dim + 1)                     # the main block and the two history slots
    A = host.exptA_linop(TAU, U, **KW)
    A.init()
    outs = [host.nek_dvector(gm) for _ in range(3)]
    A.matvec(x, outs[0])
    run_other(A, gm, kind, x, f, True)
    if kind == "nonlinear_map":
        host.check(A.lib.nlg_linop_set_baseflow(A.h, U.h))
    A.matvec(x, outs[1])
    radj = host.nek_dvector(gm)
    A.rmatvec(x, radj)
    A.matvec(x, outs[2])
    assert not np.array_equal(radj.get_field(0), want[0])     # (the adjoint is another operator: the sequence did switch modes)
    for o in outs:
        got = fields(o, dim)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
