"""Reference for the periodic-orbit Newton (numpy only; test infrastructure, never imported by the product).

Built on tests/floquet_ref.py and the oracle: one run of the coupled step gives everything the bordered system needs.
  residual  R(X0, T) = Phi_T(X0) - X0, velocity and pressure, with dt = T / nsteps;
  f0        = (U^1 - U^0) / dt, velocity and pressure: the reference's compute_fdot at X0, one impulsive first-order step;
  fT        = [b0 U^N - sum_{j<k} bd_j U^{N-1-j}] / dt, the BDF-k derivative of the base flow at level N = nsteps, k = min(N, torder);
              its pressure is the first difference (p^N - p^{N-1}) / dt, p^{N-1} in the mean-free gauge the step puts it in;
  jacobian  (v, t) -> (M v - v + t fT, <f0, v>), M the coupled matvec, <.,.> the inner product of the vector space (velocity only);
  inner product of the extended vectors: <u, v> + t_u t_v.
Also a plain Newton + GMRES on these for the manufactured-root case of the GPU test; `python tests/upo_ref.py` runs it and prints the
number of Newton iterations, which DESIGN.md 3.2 and tests/test_gpu_upo.py record.
"""
import numpy as np

import floquet_ref as fr
from oracle.lns import BDF, LNSConfig
from oracle.vectors import NekDVector


class Ext:
    """(NekDVector, T) with the algebra of the reference's nek_ext_dvector"""

    def __init__(self, vec: NekDVector, T=0.0):
        self.vec, self.T = vec, float(T)

    def copy(self):
        return Ext(self.vec.copy(), self.T)

    def scal(self, a):
        self.vec.scal(a)
        self.T *= a

    def axpby(self, alpha, other, beta):
        self.vec.axpby(alpha, other.vec, beta)
        self.T = beta * self.T + alpha * other.T

    def dot(self, other):
        return self.vec.dot(other.vec) + self.T * other.T

    def norm(self):
        return float(np.sqrt(self.dot(self)))


class UpoRef:
    """kw: the keyword arguments of an LNSConfig (tau = the period when run() is given none; dt = the fixed step when nsteps is
    none).  nsteps: a fixed step count, dt = T / nsteps."""

    def __init__(self, sem, kw, nsteps=None):
        self.sem, self.kw, self.nsteps = sem, dict(kw), nsteps

    def config(self, T=None):
        kw = dict(self.kw)
        if T is not None:
            kw["tau"] = float(T)
        if self.nsteps:
            kw["dt"] = kw["tau"] / self.nsteps
        return LNSConfig(**kw)

    def run(self, X0: NekDVector, T=None, v: NekDVector = None):
        """dict(res, f0, fT, end[, Mv]) of one run from X0 over T; v (optional) rides along as the perturbation lane"""
        sem, cfg = self.sem, self.config(T)
        ref = fr.FloquetRef(sem, cfg)
        base = ref._lane(X0)
        N, dt = base.nsteps, base.dt
        assert not self.nsteps or N == self.nsteps
        base._reset_state(X0, False)
        base.nonlinear = True
        pert = None
        if v is not None:
            pert = ref._lane(X0)
            pert._reset_state(v, False)
        nrst = 0 if cfg.no_history else cfg.torder - 1
        levels = [[a.copy() for a in X0.v]]
        f0, p_prev = NekDVector(sem), None
        for istep in range(1, N + 1):
            if pert is not None:
                pert.U = [a.copy() for a in base.u]
            p_prev = sem.ortho(base.p)
            base.advance()
            if pert is not None:
                pert.advance()
                if istep <= nrst and v.has_rst_fields():
                    tmp = NekDVector(sem, v.nscal, v.lorder)
                    v.get_rst(tmp, istep)
                    pert._load(tmp)
            levels.append([a.copy() for a in base.u])
            if istep == 1:
                for i in range(sem.dim):
                    f0.v[i][...] = (base.u[i] - X0.v[i]) / dt
                f0.pr[...] = (base.p - X0.pr) / dt
        k = min(N, cfg.torder)
        b0, bd = BDF[k]
        fT = NekDVector(sem)
        for i in range(sem.dim):
            fT.v[i][...] = (b0 * levels[N][i] - sum(bd[j] * levels[N - 1 - j][i] for j in range(k))) / dt
        fT.pr[...] = (base.p - p_prev) / dt
        end = NekDVector(sem)
        base._store(end)
        res = end.copy()
        res.axpby(-1.0, X0, 1.0)
        out = dict(res=res, f0=f0, fT=fT, end=end, dt=dt, nsteps=N)
        if pert is not None:
            Mv = NekDVector(sem)
            pert._store(Mv)
            out["Mv"] = Mv
        return out

    def residual(self, X: Ext):
        return Ext(self.run(X.vec, X.T)["res"], 0.0)

    def jacobian(self, X: Ext, v: Ext, run=None):
        """(M v - v + t fT, <f0, v>) about (X, T); the main block only (no restart history)"""
        r = self.run(X.vec, X.T, v.vec)
        out = r["Mv"].copy()
        out.axpby(-1.0, v.vec, 1.0)
        out.axpby(v.T, r["fT"], 1.0)
        return Ext(out, r["f0"].dot(v.vec))


def gmres(matvec, b: Ext, atol, kmax=200):
    """full GMRES (modified Gram-Schmidt in the extended inner product), zero initial guess; (x, residual norm, matvecs)"""
    beta = b.norm()
    V = [b.copy()]
    V[0].scal(1.0 / beta)
    H = np.zeros((kmax + 1, kmax))
    res, k = beta, 0
    y = np.zeros(0)
    while k < kmax and res > atol:
        w = matvec(V[k])
        for j in range(k + 1):
            H[j, k] = w.dot(V[j])
            w.axpby(-H[j, k], V[j], 1.0)
        for j in range(k + 1):                   # second pass
            c = w.dot(V[j])
            H[j, k] += c
            w.axpby(-c, V[j], 1.0)
        H[k + 1, k] = w.norm()
        w.scal(1.0 / H[k + 1, k])
        V.append(w)
        k += 1
        e1 = np.zeros(k + 1)
        e1[0] = beta
        y, *_ = np.linalg.lstsq(H[: k + 1, :k], e1, rcond=None)
        res = float(np.linalg.norm(H[: k + 1, :k] @ y - e1))
    x = b.copy()
    x.scal(0.0)
    for j in range(k):
        x.axpby(y[j], V[j], 1.0)
    return x, res, k


def newton(ref: UpoRef, X: Ext, tol, offset: Ext = None, maxiter=20, log=None):
    """plain Newton on R(X, T) = offset; every linear solve to atol = tol.  Returns (residuals, periods, GMRES matvecs)."""
    residuals, periods, nmv = [], [], 0
    for it in range(maxiter + 1):
        r = ref.residual(X)
        if offset is not None:
            r.axpby(-1.0, offset, 1.0)
        residuals.append(r.norm())
        periods.append(X.T)
        if log:
            log("newton %2d  |R| = %.6e  T = %.9f" % (it, residuals[-1], X.T))
        if residuals[-1] < tol or it == maxiter:
            break
        r.scal(-1.0)
        dx, _, k = gmres(lambda v: ref.jacobian(X, v), r, tol)
        nmv += k
        X.axpby(1.0, dx, 1.0)
    return residuals, periods, nmv


# |[R(X, T + d) - R(X, T - d)] / 2d - fT| / |fT| on case A (6 steps, dt = 0.01, no history, fixed step count): fT is the BDF-3
# derivative of the trajectory at T, the difference quotient that of the discrete map in T at a fixed step count; they agree to first
# order in dt only.  Measured on the CPU (test_reference_jacobian_is_the_derivative_of_the_residual): 7.11e-3.  The bound is twice
# that, on the CPU and on the GPU.
FT_FD_MEASURED = 7.11e-3
FT_FD_BOUND = 2.0 * FT_FD_MEASURED
DELTA_T = 1e-3          # relative step in T


# ---------------------------------------------------------------------------------------------------------------------
# the manufactured root of tests/test_gpu_upo.py: case A, 6 steps, no history, X* the vortex, T* = 6 dt
# ---------------------------------------------------------------------------------------------------------------------
NEWTON_TOL = 1e-9


def manufactured():
    """(ref, X*, start, offset-free residual at the root is the offset): start = (X* + 1e-3 v, 1.01 T*)"""
    hm, sem = fr.case_mesh("A")
    kw = fr.tangent_cfg()
    ref = UpoRef(sem, kw, nsteps=6)
    Xs = Ext(fr.orbit_state("A"), 6 * fr.DT)
    v = fr.start_vector(sem)
    start = Xs.copy()
    start.vec.axpby(1e-3, v, 1.0)
    start.T = 1.01 * Xs.T
    return ref, Xs, start


if __name__ == "__main__":
    ref, Xs, X = manufactured()
    off = ref.residual(Xs)
    res, per, nmv = newton(ref, X, NEWTON_TOL, offset=off, log=print)
    print("Newton iterations %d, GMRES matvecs %d, |T - T*| / T* = %.3e" % (len(res) - 1, nmv, abs(X.T - Xs.T) / Xs.T))
