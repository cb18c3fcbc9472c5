"""The reference of one PCG operator application (tests/pcg_step_ref.py) reads the step's definition right: iterated on continuous, masked
inputs with alpha and beta from its own sums, it reproduces the oracle's PCG loops (ExptA.pcg_helm, ExptA.pcg_E with the diagonal
preconditioner) at five fixed iterations.  Five iterations of a small, well-conditioned problem do not amplify rounding beyond 1e-12 of the
solution's max norm: a larger difference is a wrong reading of the step (which sum, which vector, where the mean goes), not rounding."""
import numpy as np
import pytest

import pcg_step_ref as R
from neklab_amd.mesh import box_mesh
from oracle.lns import ExptA, LNSConfig
from oracle.sem import SEM

ITERS = 5
MESHES = {
    "2d": dict(nel=(4, 3), n=6, periodic=(True, False)),
    "3d": dict(nel=(2, 2, 1), n=5, periodic=(True, False, False)),
}
_cache = {}


def setup(kind):
    if kind not in _cache:
        c = MESHES[kind]
        hm = box_mesh(c["nel"], c["n"], periodic=c["periodic"], deform=0.05)
        sem = SEM(hm)
        U = [np.zeros(sem.shape1) for _ in range(sem.dim)]
        A = ExptA(sem, U, LNSConfig(re=40.0, dt=0.01, tau=0.01, fixed_iters_v=ITERS, fixed_iters_p=ITERS, pprecond=1))
        _cache[kind] = (sem, A)
    return _cache[kind]


@pytest.mark.parametrize("kind", list(MESHES))
@pytest.mark.parametrize("zfree", [0, 1])
def test_helmholtz_steps_reproduce_pcg_helm(kind, zfree):
    sem, A = setup(kind)
    dim = sem.dim
    rng = np.random.default_rng(5)
    h2 = 1.5 / 0.01
    b = [sem.mask[i] * sem.gs(sem.bm1 * rng.standard_normal(sem.shape1)) for i in range(dim)]   # continuous and masked
    ref = A.pcg_helm([a.copy() for a in b], h2)
    minv = A.hdiag_inv(h2)
    x = [np.zeros(sem.shape1) for _ in range(dim)]
    r = [a.copy() for a in b]
    z = [sem.mask[i] * minv * r[i] for i in range(dim)]
    p = [np.zeros(sem.shape1) for _ in range(dim)]
    rz = R.fsum(sum(r[i] * z[i] * sem.vmult for i in range(dim)))
    beta = 0.0
    for _ in range(ITERS):
        st = R.helm_step(sem, p, A.nu, h2, zf=r, beta=beta, pcinv=minv) if zfree else R.helm_step(sem, p, A.nu, h2, zf=z, beta=beta)
        p = st["u"]
        alpha = rz / st["pw"]
        for i in range(dim):
            x[i] += alpha * p[i]
            r[i] -= alpha * sem.mask[i] * st["w"][i]       # the solver masks the residual, not w
            z[i] = sem.mask[i] * minv * r[i]
        rz_new = R.fsum(sum(r[i] * z[i] * sem.vmult for i in range(dim)))
        beta, rz = rz_new / rz, rz_new
    scale = max(np.abs(a).max() for a in ref)
    err = max(np.abs(x[i] - ref[i]).max() for i in range(dim)) / scale
    print(kind, "zfree", zfree, "difference after %d iterations: %.2e of the max norm" % (ITERS, err))
    assert scale > 0.0 and err <= 1e-12


@pytest.mark.parametrize("kind", list(MESHES))
def test_plain_step_is_the_fused_step_without_update(kind):
    sem, A = setup(kind)
    rng = np.random.default_rng(6)
    u = [rng.standard_normal(sem.shape1) for _ in range(sem.dim)]
    a = R.helm_step(sem, u, 0.7, 3.0)
    b = R.helm_step(sem, [np.zeros(sem.shape1)] * sem.dim, 0.7, 3.0, zf=u, beta=0.3)
    assert all(np.array_equal(x, y) for x, y in zip(a["w"], b["w"])) and a["pw"] == b["pw"]
    # pw is the sum with the LOCAL w: for a discontinuous u it differs from the assembled, vmult-weighted one
    pw_asm = R.fsum(sum(x * y * sem.vmult for x, y in zip(a["u"], a["w"])))
    assert abs(pw_asm - a["pw"]) > 1e-6 * a["pw_abs"]


@pytest.mark.parametrize("kind", list(MESHES))
def test_pressure_steps_reproduce_pcg_E(kind):
    sem, A = setup(kind)
    assert not sem.has_outflow
    rng = np.random.default_rng(7)
    b = rng.standard_normal(sem.shape2)
    ref = A.pcg_E(b.copy(), 1.0)
    minv = A.ediag_inv
    npts = b.size
    x = np.zeros(sem.shape2)
    r = b - R.fsum(b) / npts
    z = minv * r
    p = np.zeros(sem.shape2)
    rz = R.fsum(r * z)
    beta = 0.0
    for _ in range(ITERS):
        st = R.pres_step(sem, p, z, beta, R.fsum(z) / npts)
        p = st["p"]
        alpha = rz / R.fsum(st["a"])
        x += alpha * p
        r -= alpha * (st["out"] - R.fsum(st["b"]) / npts)
        z = minv * r
        rz_new = R.fsum(r * z)
        beta, rz = rz_new / rz, rz_new
    scale = np.abs(ref).max()
    err = np.abs(x - ref).max() / scale
    print(kind, "difference after %d iterations: %.2e of the max norm" % (ITERS, err))
    assert scale > 0.0 and err <= 1e-12
