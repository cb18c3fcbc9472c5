"""Reference of the eigenvalue sensitivity (nlg_sens_apply, nlg_sens_pairing; host.eigenvalue_sensitivity), in numpy on
oracle.sem.SEM.

For real velocity fields u, a on mesh 1, with u~ = mask (.) u and a~ = mask (.) a (the velocity Dirichlet masks are applied on read;
d_j is the pointwise physical derivative gradm1 of an element: no mass matrix, no gather-scatter):

    T(u, a)_j = - sum_i a~_i d_j u~_i          (transport part)
    P(u, a)_j = + sum_i u~_i d_i a~_j          (production part)
    S(u, a)   = T + P

Then <a, [L(U + dU) - L(U)] u> = <S(u, a), dU> in the nek_ddot inner product, where L is the operator of apply_L, u is solenoidal and
the boundary term of one integration by parts vanishes.  The term (div u) a_j is left out on purpose.

For a complex pair, direct u^ = u_r + i u_i with L u^ = lambda u^, adjoint u^+ = a_r + i a_i with L+ u^+ = conj(lambda) u^+:

    d       = <u^+, u^> = (a_r.u_r + a_i.u_i) + i (a_r.u_i - a_i.u_r)          (nek_ddot)
    S_re    = S(u_r, a_r) + S(u_i, a_i)        S_im = S(u_i, a_r) - S(u_r, a_i)
    grad_U lambda = (S_re + i S_im) / d        (same split for T and P)
    W(x)    = |u^(x)| |u^+(x)| / |d|           (wavemaker; |u^(x)|^2 = sum_i (u_r,i^2 + u_i,i^2), of the masked fields)
    dlambda ~ <Re grad_U lambda, dU> + i <Im grad_U lambda, dU>

S_re + i S_im is S(u^, conj(u^+)) with S taken bilinear, which is how it is formed below: complex arrays, the gradient of the real and
of the imaginary part taken separately (oracle.sem works on real fields).
"""
import numpy as np


def _grad(sem, f):
    """gradm1 of a complex field: dim complex fields"""
    f = np.asarray(f)
    gr = sem.gradm1(np.ascontiguousarray(f.real))
    if not np.iscomplexobj(f):
        return gr
    gi = sem.gradm1(np.ascontiguousarray(f.imag))
    return [a + 1j * b for a, b in zip(gr, gi)]


def parts(sem, u, a, mask=None):
    """(T, P), two lists of dim fields, bilinear in (u, a); u and a lists of dim real or complex fields"""
    mask = sem.mask if mask is None else mask
    dim = sem.dim
    ut = [mask[k] * np.asarray(u[k]).reshape(sem.shape1) for k in range(dim)]
    at = [mask[k] * np.asarray(a[k]).reshape(sem.shape1) for k in range(dim)]
    gu = [_grad(sem, ut[i]) for i in range(dim)]   # gu[i][j] = d_j u~_i
    ga = [_grad(sem, at[j]) for j in range(dim)]   # ga[j][i] = d_i a~_j
    T = [-sum(at[i] * gu[i][j] for i in range(dim)) for j in range(dim)]
    P = [sum(ut[i] * ga[j][i] for i in range(dim)) for j in range(dim)]
    return T, P


def pairing(sem, ur, ui, ar, ai):
    """d = <u^+, u^>, complex (ui = ai = None: a real pair).  Not masked: it is nek_ddot."""
    dim = sem.dim
    uc = [sem.f1(ur[k]) + (1j * sem.f1(ui[k]) if ui is not None else 0.0) for k in range(dim)]
    ac = [sem.f1(ar[k]) + (1j * sem.f1(ai[k]) if ai is not None else 0.0) for k in range(dim)]
    return complex(sum(np.sum(np.conj(ac[k]) * uc[k] * sem.bm1) for k in range(dim)))


def sensitivity(sem, ur, ui, ar, ai, scale=1.0, mask=None, production_sign=1.0):
    """dict of grad_re, grad_im, T_re, T_im (lists of dim real fields) and W (one field) of one pair times the complex `scale`
    (1 / d for the gradient of the eigenvalue).  production_sign = -1: the wrong formula the end-to-end test must tell apart."""
    mask = sem.mask if mask is None else mask
    dim = sem.dim
    uc = [sem.f1(ur[k]) + (1j * sem.f1(ui[k]) if ui is not None else 0.0) for k in range(dim)]
    ac = [sem.f1(ar[k]) - (1j * sem.f1(ai[k]) if ai is not None else 0.0) for k in range(dim)]   # conj(u^+)
    T, P = parts(sem, uc, ac, mask)
    g = [(T[j] + production_sign * P[j]) * scale for j in range(dim)]
    t = [T[j] * scale for j in range(dim)]
    mu = np.sqrt(sum(np.abs(mask[k] * uc[k]) ** 2 for k in range(dim)))
    ma = np.sqrt(sum(np.abs(mask[k] * ac[k]) ** 2 for k in range(dim)))
    return dict(grad_re=[np.real(x) + 0.0 * mu for x in g], grad_im=[np.imag(x) + 0.0 * mu for x in g],
                T_re=[np.real(x) + 0.0 * mu for x in t], T_im=[np.imag(x) + 0.0 * mu for x in t], W=mu * ma * abs(scale))


def ddot(sem, a, b):
    """nek_ddot of two lists of dim velocity fields"""
    return float(sum(np.sum(sem.f1(a[k]) * sem.f1(b[k]) * sem.bm1) for k in range(sem.dim)))


# ---- polynomial fields: the direct field is lns_ref.poly_fields' u = (y^2 + x z, x^2 - y z, x y) (solenoidal); the adjoint is
# a = (x y + z, y^2 - x z, x + y z)  (z = 0 in 2-D) ------------------------------------------------------------------------------------
def poly_pair(sem):
    """(u, a, exact) with exact = dict(T=, P=, S=) of dim fields, written out by hand"""
    dim = sem.dim
    x, y = sem.X[0], sem.X[1]
    z = sem.X[2] if dim == 3 else np.zeros_like(x)
    one, zero = np.ones_like(x), np.zeros_like(x)
    u = [y * y + x * z, x * x - y * z, x * y][:dim]
    a = [x * y + z, y * y - x * z, x + y * z][:dim]
    # du[i][j] = d u_i / d x_j, da likewise
    du = [[z, 2.0 * y, x], [2.0 * x, -z, -y], [y, x, zero]]
    da = [[y, x, one], [-z, 2.0 * y, -x], [one, z, y]]
    T = [-sum(a[i] * du[i][j] for i in range(dim)) for j in range(dim)]
    P = [sum(u[i] * da[j][i] for i in range(dim)) for j in range(dim)]
    return u, a, dict(T=T, P=P, S=[t + p for t, p in zip(T, P)])


def bubble_dU(sem, lengths):
    """dU = b (l_0, l_1, l_2): the bubble b = prod_k x_k (L_k - x_k), zero on the boundary of the box [0, L], times a linear field.
    Degree 3 in every direction."""
    dim = sem.dim
    x, y = sem.X[0], sem.X[1]
    z = sem.X[2] if dim == 3 else np.zeros_like(x)
    b = np.ones_like(x)
    for k in range(dim):
        b = b * sem.X[k] * (lengths[k] - sem.X[k])
    lin = [1.0 + 0.3 * x - 0.2 * y, 0.5 - 0.4 * x + 0.1 * z, 0.2 + y - 0.3 * z][:dim]
    return [b * l for l in lin]
