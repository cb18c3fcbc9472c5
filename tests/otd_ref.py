"""Reference for the OTD mode of the block stepper (numpy only; test infrastructure, never imported by the product).

r oracle propagators (`FilteredExptA`, nothing of their step changed) advance in lockstep as one continuous run.  Before every step
with istep >= startstep the reduced operator Lr_ij = <u_i, L u_j> is formed as the plain local sum  sum u_i . W_j  of the weak form
W_j = D^T p_j - nu A u_j - N(U; u_j)  (sem.opgradt, sem.axhelm_local with h2 = 0, sem.lns_conv_weak), the upper-triangular
C (C_jj = Lr_jj, C_ij = Lr_ij + Lr_ji for i < j) follows, and lane j receives the body force f_j = -sum_{i <= j} u_i C_ij through
the oracle's `force` hook (F += bm1 f).  After every step with istep >= startstep and (istep <= startstep + 10 or istep % orthostep
== 0), and in reduced(), the lanes become U T with T = chol(G)^-T, G_ij = sum bm1 u_i . u_j, applied to u, p, ulag and flag; at
creation twice.  Coupled variant (tests/floquet_ref.py, coupled_matvec): one more lane carries the base flow through the nonlinear
step, and every perturbation lane has its U set to the base flow's velocity before each step.
"""
import numpy as np

from filter_ref import FilteredExptA
from oracle.vectors import NekDVector


class OTDRef:
    def __init__(self, sem, cfg, X0: NekDVector, basis0, startstep=1, orthostep=10, trans=False, solve_baseflow=False,
                 filter_weight=0.0, filter_modes=1):
        self.sem, self.cfg, self.r = sem, cfg, len(basis0)
        self.startstep, self.orthostep, self.trans = startstep, orthostep, trans

        def lane():
            return FilteredExptA(sem, X0.v, cfg, filter_weight=filter_weight, filter_modes=filter_modes)

        self.lanes = []
        for b in basis0:
            ln = lane()
            ln._reset_state(b, trans)
            self.lanes.append(ln)
        self.base = None
        if solve_baseflow:
            self.base = lane()
            self.base._reset_state(X0, False)
            self.base.nonlinear = True
        self.dt = self.lanes[0].dt
        self.istep, self.time = 0, 0.0
        self.G0 = self.orthonormalise()
        self.orthonormalise()

    # ---- inner products, all plain local sums ----
    def gram(self):
        s, L = self.sem, self.lanes
        return np.array([[sum(np.sum(s.bm1 * L[i].u[c] * L[j].u[c]) for c in range(s.dim)) for j in range(self.r)] for i in range(self.r)])

    def weak_L(self, ln):
        """W = D^T p - nu A u - N(U; u), element-local (no assembly, no mask, no mass inverse)"""
        s = self.sem
        gp = s.opgradt(ln.p)
        N = s.lns_conv_weak(ln.U, ln.u, adjoint=self.trans)
        return [gp[c] - s.axhelm_local(ln.u[c], ln.nu, 0.0) - N[c] for c in range(s.dim)]

    def reduced_now(self):
        s, L = self.sem, self.lanes
        W = [self.weak_L(ln) for ln in L]
        return np.array([[sum(np.sum(L[i].u[c] * W[j][c]) for c in range(s.dim)) for j in range(self.r)] for i in range(self.r)])

    @staticmethod
    def forcing_matrix(Lr):
        C = np.triu(Lr) + np.triu(Lr.T, 1)
        return C

    # ---- the transform ----
    def orthonormalise(self):
        """returns the Gram matrix it was made from"""
        G = self.gram()
        T = np.linalg.inv(np.linalg.cholesky(G)).T          # upper triangular
        L, r, dim = self.lanes, self.r, self.sem.dim

        def comb(get, put):
            old = [get(ln).copy() for ln in L]
            for j in range(r):
                put(L[j], sum(T[i, j] * old[i] for i in range(j + 1)))

        for c in range(dim):
            comb(lambda ln: ln.u[c], lambda ln, a: ln.u.__setitem__(c, a))
            for lev in range(2):
                comb(lambda ln: ln.ulag[lev][c], lambda ln, a: ln.ulag[lev].__setitem__(c, a))
                comb(lambda ln: ln.flag[lev][c], lambda ln, a: ln.flag[lev].__setitem__(c, a))
        comb(lambda ln: ln.p, lambda ln, a: setattr(ln, "p", a))
        return G

    # ---- time stepping ----
    def step(self):
        s, L, r = self.sem, self.lanes, self.r
        istep = self.istep + 1
        if self.base is not None:
            for ln in L:
                ln.U = [a.copy() for a in self.base.u]       # U^n, before the base flow moves
        if istep >= self.startstep:
            for ln in L:
                ln.p = s.ortho(ln.p)                          # what advance() does first; the gradient below is of that pressure
            C = self.forcing_matrix(self.reduced_now())
            f = [[-sum(C[i, j] * L[i].u[c] for i in range(j + 1)) for c in range(s.dim)] for j in range(r)]
            for j in range(r):
                L[j].force = (f[j], None, 0.0, 1.0)
        else:
            for ln in L:
                ln.force = None
        if self.base is not None:
            self.base.advance()
        for ln in L:
            ln.advance()
            ln.force = None
        self.istep, self.time = istep, self.time + self.dt
        if istep >= self.startstep and (istep <= self.startstep + 10 or istep % self.orthostep == 0):
            self.orthonormalise()

    def advance(self, n):
        for _ in range(n):
            self.step()

    def reduced(self):
        """(Lr, G before): orthonormalise, then Lr on the current state"""
        G = self.orthonormalise()
        if self.base is not None:
            for ln in self.lanes:
                ln.U = [a.copy() for a in self.base.u]
        for ln in self.lanes:
            ln.p = self.sem.ortho(ln.p)
        return self.reduced_now(), G

    def basis(self, i) -> NekDVector:
        out = NekDVector(self.sem)
        self.lanes[i]._store(out)
        return out

    def baseflow(self) -> NekDVector:
        out = NekDVector(self.sem)
        self.base._store(out)
        return out


def orthonormal_basis(sem, r, seed0=11):
    """r admissible vectors (rand: continuous, masked), orthonormal in the vector-space inner product, with a small pressure"""
    out = []
    for j in range(r):
        v = NekDVector(sem)
        v.rand(ifnorm=True, seed=seed0 + j)
        for w in out:
            v.axpby(-v.dot(w), w, 1.0)
        v.scal(1.0 / v.norm())
        v.pr[...] = 0.01 * np.random.default_rng(seed0 + 100 + j).standard_normal(sem.shape2)
        out.append(v)
    return out


# the known-answer case of tests/test_cpu_otd.py and tests/test_gpu_otd.py: case A at Re = 10 about the frozen orbit_state("A", 1.0),
# dt = 0.01 (CFL 0.34), r = 2; reference eigenvalue from the propagator over tau = 0.2; step count and tolerance: see test_cpu_otd.py
KA = dict(re=10.0, amp=1.0, dt=0.01, tau=0.2, r=2, nsteps=82, tol=7.8e-3)


def leading(Lr):
    """the eigenvalue of Lr with the largest real part"""
    lam = np.linalg.eigvals(Lr)
    return lam[np.argmax(lam.real)]
