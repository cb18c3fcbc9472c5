"""Reference twin of the DNS run with history points and a recurrence monitor (numpy only; test infrastructure, never imported by the
product).  The run steps the oracle as FloquetRef's base lane does: `_reset_state(X0, False)`, `nonlinear = True`, `advance()` per step.
The point location, the Lagrange evaluation and the recurrence norm are written here on their own, not taken from the product.
"""
import numpy as np

import floquet_ref as fr
from neklab_amd.mesh import box_mesh, gll_points
from oracle.lns import ExptA, LNSConfig
from oracle.vectors import NekDVector

NEWTON_STOP = 1e-13


def lagrange(z, r):
    """l_j(r) and l_j'(r) on the nodes z, product form (no barycentric weights: a second formula for the same polynomials)"""
    n = len(z)
    w, dw = np.ones(n), np.zeros(n)
    for j in range(n):
        for k in range(n):
            if k != j:
                w[j] *= (r - z[k]) / (z[j] - z[k])
        for i in range(n):
            if i != j:
                t = 1.0 / (z[j] - z[i])
                for k in range(n):
                    if k != j and k != i:
                        t *= (r - z[k]) / (z[j] - z[k])
                dw[j] += t
    return w, dw


def tensor_eval(f, ws):
    """sum_ijk f[k, j, i] w_r[i] w_s[j] w_t[k] for one element's field f (its axes z, y, x as the layout has them)"""
    out = f
    for w in ws:                     # contract the last axis (x first, then y, then z)
        out = out @ w
    return float(out)


def evaluate(field_e, z, r):
    """the interpolant of one element's field (shape (n,) * dim, last axis = x) at r = (r, s[, t])"""
    return tensor_eval(field_e, [lagrange(z, ri)[0] for ri in r])


def _map(Xe, z, r):
    dim = len(r)
    L = [lagrange(z, ri) for ri in r]
    x = np.array([tensor_eval(Xe[c], [L[d][0] for d in range(dim)]) for c in range(dim)])
    J = np.array([[tensor_eval(Xe[c], [L[q][1] if q == d else L[q][0] for q in range(dim)]) for d in range(dim)] for c in range(dim)])
    return x, J


def locate_in(Xe, z, xs):
    """Newton of the issue's recipe in one element: (r, found); found = converged (any |r| up to the clamp)"""
    dim, n = len(xs), len(z)
    d2 = sum((Xe[c] - xs[c]) ** 2 for c in range(dim))
    idx = np.unravel_index(np.argmin(d2), d2.shape)
    r = np.array([z[idx[dim - 1 - d]] for d in range(dim)])
    for _ in range(50):
        x, J = _map(Xe, z, r)
        try:
            dr = np.linalg.solve(J, xs - x)
        except np.linalg.LinAlgError:
            return r, False
        rn = np.clip(r + dr, -1.5, 1.5)
        step = np.max(np.abs(rn - r))
        r = rn
        if step <= NEWTON_STOP:
            return r, True
    return r, False


def holders(hm, xs, tol_r=0.0):
    """[(global element id, local index, r)] of every element that holds xs with |r|_inf <= 1 + tol_r + the Newton stop"""
    dim, n = hm.dim, hm.n
    z = gll_points(n)
    C = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
    out = []
    for e in range(hm.E):
        Xe = [c[e].reshape((n,) * dim) for c in C]
        lo = np.array([a.min() for a in Xe]); hi = np.array([a.max() for a in Xe])
        g = 0.1 * (hi - lo)
        if np.any(xs < lo - g) or np.any(xs > hi + g):
            continue
        r, ok = locate_in(Xe, z, np.asarray(xs, dtype=np.float64))
        if ok and np.max(np.abs(r)) <= 1.0 + tol_r + NEWTON_STOP:
            gid = e if hm.elem_gid is None else int(hm.elem_gid[e])
            out.append((gid, e, r))
    return sorted(out, key=lambda h: h[0])


def map_point(hm, e, r):
    """x_e(r) of local element e"""
    dim, n = hm.dim, hm.n
    C = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
    return _map([c[e].reshape((n,) * dim) for c in C], gll_points(n), np.asarray(r))[0]


def sample(sem, elem, rst, v: NekDVector):
    """[npts][dim + 1 (+ 1)]: velocity, pressure (on the Gauss nodes), temperature at the located points (local elements `elem`)"""
    dim = sem.dim
    nf = dim + 1 + (1 if v.nscal else 0)
    out = np.zeros((len(elem), nf))
    for q, (e, r) in enumerate(zip(elem, rst)):
        for c in range(dim):
            out[q, c] = evaluate(v.v[c][e], sem.z1, r)
        out[q, dim] = evaluate(v.pr[e], sem.z2, r)
        if v.nscal:
            out[q, dim + 1] = evaluate(v.theta[0][e], sem.z1, r)
    return out


def weight_sum(sem, rst, mesh2=False):
    """sum_ijk |w_i w_j w_k| per point: the condition number of the evaluation"""
    z = sem.z2 if mesh2 else sem.z1
    return np.array([np.prod([np.abs(lagrange(z, ri)[0]).sum() for ri in r]) for r in rst])


def recur_dist(sem, u, ref):
    """|u - ref| with the weights of nek_ddot: bm1, velocity (and temperature), no pressure"""
    s = sum(np.sum(sem.bm1 * (a - b) ** 2) for a, b in zip(u.v, ref.v))
    if u.nscal:
        s += np.sum(sem.bm1 * (u.theta[0] - ref.theta[0]) ** 2)
    return float(np.sqrt(s))


def run(sem, cfg: LNSConfig, X0: NekDVector, nsteps, elem, rst, ref=None):
    """-> dict(time, probe [nsteps + 1][npts][nf], dist, state): sample 0 is X0, one sample after every step"""
    lane = ExptA(sem, X0.v, cfg)
    lane._reset_state(X0, False)
    lane.nonlinear = True
    ref = X0 if ref is None else ref
    cur = NekDVector(sem, X0.nscal, X0.lorder)
    time, probe, dist = [], [], []
    for k in range(nsteps + 1):
        if k:
            lane.advance()
        lane._store(cur)
        time.append(k * lane.dt)
        probe.append(sample(sem, elem, rst, cur))
        dist.append(recur_dist(sem, cur, ref))
    return {"time": np.array(time), "probe": np.array(probe), "dist": np.array(dist), "state": cur, "dt": lane.dt}


# ---------------------------------------------------------------------------------------------------------------------
# the meshes and points the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
def mesh_of(name):
    if name == "C":   # undeformed, lx1 = 10, periodic in x
        return box_mesh((2, 2, 2), 10, lengths=(2.0, 1.0, 1.0), periodic=(True, False, False), deform=0.0)
    return fr.case_mesh(name)[0]


def case_points(name, hm):
    """[(label, x*, expected status, number of holders or None)]: the points are images of reference coordinates under the twin's map, so
    that a face point lies on the (deformed) face to rounding"""
    mp = lambda e, r: map_point(hm, e, r)
    if hm.dim == 2:   # A: 3 x 3 elements, walls all round; element 4 is the middle one
        return [("interior", mp(4, (0.31, -0.47)), 0, 1),
                ("face", mp(4, (1.0, 0.3)), 0, 2),
                ("vertex", mp(4, (-1.0, -1.0)), 0, 4),
                ("wall", mp(1, (0.2, -1.0)), 0, 1),
                ("wall corner", np.array([0.0, 0.0]), 0, 1),
                ("node", mp(0, (gll_points(hm.n)[2], gll_points(hm.n)[4])), 0, 1),
                ("outside", np.array([-0.2, 0.5]), 2, 0)]
    return [("interior", mp(3, (0.31, -0.47, 0.052)), 0, 1),
            ("face", mp(0, (0.3, 1.0, -0.6)), 0, 2),
            ("edge", mp(0, (0.3, 1.0, 1.0)), 0, 4),
            ("vertex of all", np.array([1.0, 0.5, 0.5]), 0, 8),
            ("wall", mp(5, (0.2, -0.4, 1.0)), 0, 1),
            ("seam", np.array([0.0, 0.3, 0.6]), 0, 1),
            ("seam far side", np.array([2.0, 0.5, 0.3]), 0, 2),
            ("outside", np.array([-0.2, 0.5, 0.5]), 2, 0)]
