"""Reference for the explicit modal filter (numpy only; test infrastructure, never imported by the product).

Restated from memory of Nek5000's build_new_filter / q_filter: on the GLL nodes z_1..z_n, in the basis
phi_1 = L_0, phi_2 = L_1, phi_k = L_{k-1} - L_{k-3} (k >= 3), the last `ncut` modal coefficients are scaled by
d_k = 1 - w ((k - k0) / ncut)^2, k0 = n - ncut:  F = Phi diag(d) Phi^-1, applied along every direction of every element.
"""
import numpy as np
from numpy.polynomial import legendre as npleg

from oracle.lns import ExptA


def modal_basis(z):
    """Phi_jk = phi_k(z_j) (0-based k: column k holds the issue's phi_{k+1})."""
    n = len(z)
    L = np.stack([npleg.legval(z, np.eye(n)[k]) for k in range(n)], axis=1)
    Phi = L.copy()
    Phi[:, 2:] = L[:, 2:] - L[:, :-2]
    return Phi


def transfer_function(n, ncut, w):
    d = np.ones(n)
    k0 = n - ncut
    for k in range(k0 + 1, n + 1):                 # 1-based mode index, as in the definition
        d[k - 1] = 1.0 - w * (k - k0) ** 2 / ncut ** 2
    return d


def filter_matrix(n, ncut, w, z=None):
    """F = Phi diag(d) Phi^-1, straight from the definition."""
    if z is None:
        from neklab_amd.mesh import gll_points
        z = gll_points(n)
    Phi = modal_basis(np.asarray(z, dtype=np.float64))
    return Phi @ np.diag(transfer_function(n, ncut, w)) @ np.linalg.inv(Phi)


def apply_along(field, M, dim):
    """M applied along each of the `dim` trailing axes of field[(E, n, ..., n)]."""
    a = np.asarray(field, dtype=np.float64)
    for ax in range(1, dim + 1):
        a = np.moveaxis(np.tensordot(M, a, axes=([1], [ax])), 0, ax)
    return a


def apply_filter(sem, field, F):
    """(F x F [x F]) field on every element; no gather-scatter."""
    return apply_along(sem.f1(field), F, sem.dim)


class FilteredExptA(ExptA):
    """The oracle's propagator with the filter at the end of every time step: velocity and, with ifheat, temperature; never the
    pressure.  matvec, nonlinear_map and integrate_forced of the oracle all go through advance()."""

    def __init__(self, sem, baseflow, cfg, baseflow_theta=None, filter_weight=0.0, filter_modes=1):
        super().__init__(sem, baseflow, cfg, baseflow_theta)
        self.filter_weight = float(filter_weight)
        self.F = filter_matrix(sem.n, filter_modes, self.filter_weight, sem.z1) if self.filter_weight > 0.0 else None

    def advance(self):
        super().advance()
        if self.F is not None:
            self.u = [apply_filter(self.sem, a, self.F) for a in self.u]
            if self.cfg.ifheat:
                self.t = apply_filter(self.sem, self.t, self.F)
