"""Reference of the strong-form LNS operator (nlg_lns_apply / nlg_op_lns; apply_L and its pieces, reference
src/linops/neklab_linops.f90:268-426), restated in numpy on oracle.sem.SEM:

    u~_k  = mask_k u_k                                     (bcdirvc on read)
    lap_k = sum_i gradm1(gradm1(u~_k)_i)_i                 (lap_1D: pointwise, no mass, no dssum)
    N_k   = lns_conv_weak(U, u~, adjoint)_k / bm1          (local bm1 = Nek convop)
    P     = (I21 x ... x I21) p                            (Nek mappr: Gauss lx1-2 -> GLL lx1)
    out_k = c_lap nu lap_k + c_conv N_k + c_p gradm1(P)_k

and the polynomial fields whose L u is known in closed form.
"""
import numpy as np

from oracle.sem import _ap, interp_matrix

APPLY_L, APPLY_LV, LAPLACIAN, CONV, GRADP = (1.0, -1.0, -1.0), (1.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
ROUTINES = {"apply_L": APPLY_L, "apply_Lv": APPLY_LV, "compute_LNS_laplacian": LAPLACIAN, "compute_LNS_conv": CONV, "compute_LNS_gradp": GRADP}


def pressure_to_gll(sem, p):
    I21 = interp_matrix(sem.z2, sem.z1)
    P = sem.f2(p)
    for a in sem.axes:
        P = _ap(I21, P, a)
    return P


def lns_terms(sem, U, u, p, adjoint=False, mask=None):
    """(lap, N, gp): three lists of dim fields, before the coefficients and nu."""
    mask = sem.mask if mask is None else mask
    dim = sem.dim
    ut = [mask[k] * sem.f1(u[k]) for k in range(dim)]
    lap = []
    for k in range(dim):
        g = sem.gradm1(ut[k])
        lap.append(sum(sem.gradm1(g[i])[i] for i in range(dim)))
    N = [w / sem.bm1 for w in sem.lns_conv_weak(U, ut, adjoint=adjoint)]
    gp = sem.gradm1(pressure_to_gll(sem, p))
    return lap, N, gp


def lns_strong(sem, U, u, p, re, coef=APPLY_L, adjoint=False, mask=None):
    lap, N, gp = lns_terms(sem, U, u, p, adjoint, mask)
    return [coef[0] / re * lap[k] + coef[1] * N[k] + coef[2] * gp[k] for k in range(sem.dim)]


# ---- the polynomial case: U = (1 + y/2, 0.3 x - 0.2 z, 0.1 x), u = (y^2 + x z, x^2 - y z, x y), p = x^2 - y (z = 0 in 2-D) -------------
def poly_fields(sem):
    """(U, u, p on mesh 2, exact) with exact(re, coef, adjoint) -> the dim fields of the closed form."""
    dim = sem.dim
    x, y = sem.X[0], sem.X[1]
    z = sem.X[2] if dim == 3 else np.zeros_like(x)
    one, zero = np.ones_like(x), np.zeros_like(x)
    U = [1.0 + 0.5 * y, 0.3 * x - 0.2 * z, 0.1 * x][:dim]
    u = [y * y + x * z, x * x - y * z, x * y][:dim]
    X2 = [sem.to_mesh2(c) for c in sem.X]
    p = X2[0] ** 2 - X2[1]
    # dU[i][j] = d U_i / d x_j, du likewise
    dU = [[zero, 0.5 * one, zero], [0.3 * one, zero, -0.2 * one], [0.1 * one, zero, zero]]
    du = [[z, 2.0 * y, x], [2.0 * x, -z, -y], [y, x, zero]]
    lap = [2.0 * one, 2.0 * one, zero]
    gp = [2.0 * x, -one, zero]

    def exact(re, coef=APPLY_L, adjoint=False):
        out = []
        for i in range(dim):
            if not adjoint:
                N = sum(U[j] * du[i][j] + u[j] * dU[i][j] for j in range(dim))
            else:
                N = -sum(U[j] * du[i][j] for j in range(dim)) + sum(u[m] * dU[m][i] for m in range(dim))
            out.append(coef[0] / re * lap[i] + coef[1] * N + coef[2] * gp[i])
        return out

    return U, u, p, exact
