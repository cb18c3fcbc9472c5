#!/usr/bin/env python3
"""Is the reference's backward-facing-step base flow closer to a fixed point of "step, then filter" than of the plain step?
(DESIGN.md section 2(a').)

The shipped flow X (tests/golden/reference_bfs_baseflow.npz), bdf2, Re = 600, tolerances 1e-8 / 1e-6 (bfs.par), through the
nonlinear map over a short horizon tau, without and with the case's explicit filter (filterWeight 0.01, filterCutoffRatio 0.84 ->
one mode at lx1 = 6): |Phi_tau(X) - X| in the velocity norm, and the discrete divergence of Phi_tau(X) on the Gauss mesh (L2 and
maximum).  Nothing is asserted: the filter damps at w / dt per unit time, and the dt of the CFL rule here need not be the dt
of the Nek5000 run that produced the file.

usage: filter_bfs_fixed_point.py [tau, default 0.5]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from neklab_amd import host  # noqa: E402
from refdata import load_bfs  # noqa: E402

tau = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
hm, ux, uy, p, re, lxd, _ = load_bfs(with_bcs=True)
ctx = host.Context(0)
gm = host.Mesh(ctx, hm, lxd=lxd)
X = host.nek_dvector(gm)
X.set_field(host.VX, ux)
X.set_field(host.VY, uy)
I12 = host._gll_to_gl_matrix(hm.n)                # the file's pressure lives on the velocity mesh (Pn-Pn output of a Pn-Pn-2 run)
X.set_field(host.PR, np.einsum("by,ax,eyx->eba", I12, I12, p.reshape(hm.E, hm.n, hm.n)))
bm2 = gm.get("bm2", 2)


def div_norms(V):
    """discrete divergence on the Gauss mesh, pointwise: L2 (bm2-weighted mean square) and maximum, as in DESIGN.md 2(a')"""
    out = host.nek_dvector(gm)
    host.check(ctx.lib.nlg_op_opdiv(gm.h, V.h, out.h))
    d = out.get_field(host.PR) / bm2
    return np.sqrt(np.sum(d ** 2 * bm2) / np.sum(bm2)), np.abs(d).max()


ncut = host.filter_modes_from_cutoff_ratio(hm.n, 0.84)
print("E = %d, lx1 = %d, Re = %g, tau = %g; |X| = %.6e" % (hm.E, hm.n, re, tau, X.norm()))
print("%-22s                                                        div X: L2 %.6e  max %.6e" % (("the flow itself",) + div_norms(X)))
for name, filt in (("without the filter", {}), ("filter 0.01, %d mode" % ncut, dict(filter_weight=0.01, filter_modes=ncut))):
    S = host.nek_system(tau, X, re=re, torder=2, vtol=1e-8, ptol=1e-6, maxit_v=400, maxit_p=4000, **filt)
    F = host.nek_dvector(gm)
    S.eval(X, F)                                  # Phi_tau(X) - X
    info = S.nl.info()
    Y = F.copy()
    Y.axpby(1.0, X, 1.0)                          # Phi_tau(X)
    print("%-22s dt = %.5f (%d steps)  |Phi(X) - X| = %.6e  div Phi(X): L2 %.6e  max %.6e"
          % ((name, info["dt"], info["nsteps"], F.norm()) + div_norms(Y)))
