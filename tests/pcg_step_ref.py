"""Plain float64 reference of ONE application of the operator of each PCG loop in the form the solver calls it (csrc/lns.hip helm_apply and
pres_apply; on the device: nlg_op_helmholtz_pcg and nlg_op_cdabdtp_pcg): the fused direction update, the operator of oracle/sem.py, and the
first-stage sums as the KERNELS define them.  Every sum is a math.fsum (exactly rounded), so the reference's own error is that of the
operator alone.  Nothing is iterated here: test_cpu_pcg_step_ref.py iterates these steps and recovers the oracle's PCG from them."""
import math

import numpy as np


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def elem_fsum(a, E):
    return np.array([fsum(row) for row in np.asarray(a, dtype=np.float64).reshape(E, -1)])


def helm_step(sem, u, h1, h2, zf=None, beta=0.0, pcinv=None):
    """One lane of the Helmholtz application on the fields u (a list: one field, or the dim velocity components).

    zf None           : u' = u                                    (the plain application of the single-reduction PCG)
    zf, pcinv None    : u' = zf + beta u                          (zf = z, the stored preconditioned residual)
    zf and pcinv      : u' = fl(pc zf) + beta u, pc = mask_c ? pcinv : 0   (zf = r; the product is rounded on its own, as the stored z was)
    w_local = (h1 A + h2 B) u' per element, w = QQ^T w_local WITHOUT the Dirichlet mask (the solver masks elsewhere),
    pw = sum over the local points of u' w_local: w BEFORE the gather-scatter.  (The oracle's PCG sums u' mask w vmult over the assembled w:
    the same number for a continuous masked u', another one for the discontinuous fields the device tests use.)
    Returns dict(u, z, bu, w_local, w: lists of fields; pw; pw_abs = sum |u'| |w_local|)."""
    nf = len(u)
    u = [sem.f1(a) for a in u]
    z, bu, un = [], [], []
    for c in range(nf):
        if zf is None:
            z.append(np.zeros(sem.shape1)), bu.append(u[c].copy()), un.append(u[c].copy())
            continue
        if pcinv is None:
            zc = sem.f1(zf[c]).copy()
        else:
            pc = np.where(sem.mask[c] != 0.0, sem.f1(pcinv), 0.0)
            zc = pc * sem.f1(zf[c])
        z.append(zc), bu.append(beta * u[c]), un.append(zc + beta * u[c])
    wl = [sem.axhelm_local(a, h1, h2) for a in un]
    w = [sem.gs(a) for a in wl]
    pw = fsum(np.concatenate([(a * b).ravel() for a, b in zip(un, wl)]))
    pw_abs = fsum(np.concatenate([np.abs(a * b).ravel() for a, b in zip(un, wl)]))
    return dict(u=un, z=z, bu=bu, w_local=wl, w=w, pw=pw, pw_abs=pw_abs)


def pres_step(sem, p, z=None, beta=0.0, zmean=0.0):
    """One lane of the pressure application: p' = (z - zmean) + beta p (z None: p' = p), out = E p',
    a[e] = sum over element e of p' out, b[e] = sum of out; a_abs, b_abs: the same sums of absolute values."""
    p = sem.f2(p)
    pn = p.copy() if z is None else (sem.f2(z) - zmean) + beta * p
    out = sem.cdabdtp(pn)
    return dict(p=pn, out=out, a=elem_fsum(pn * out, sem.E), b=elem_fsum(out, sem.E), a_abs=elem_fsum(np.abs(pn * out), sem.E),
                b_abs=elem_fsum(np.abs(out), sem.E))
