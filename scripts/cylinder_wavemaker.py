#!/usr/bin/env python3
"""The wavemaker of the cylinder wake at Re = 50, on the reference's own mesh and base flow (tests/golden fixture; the case of
examples/cylinder/stability/direct and .../adjoint): direct and adjoint stability analysis, the leading modes paired, the structural
sensitivity W = |u^| |u^+| / |<u^+, u^>| and the base-flow gradient of the leading eigenvalue (host.sensitivity_analysis).  Prints
where W peaks and what each stage costs; the record goes to profiles/cylinder_wavemaker.txt.

usage: cylinder_wavemaker.py [kdim] [tol] [outdir]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from neklab_amd import host  # noqa: E402
from refdata import load_cylinder  # noqa: E402

kdim = int(sys.argv[1]) if len(sys.argv) > 1 else 128
tol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-6
outdir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
os.makedirs(outdir, exist_ok=True)
hm, ux, uy, p, re, lxd, _ = load_cylinder(with_bcs=True)
ctx = host.Context(0)
gm = host.Mesh(ctx, hm, lxd=lxd)
bf = host.nek_dvector(gm)
bf.set_field(host.VX, ux)
bf.set_field(host.VY, uy)
A = host.exptA_linop(1.0, bf, re=re, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=400, maxit_p=4000)   # 1cyl.par
A.init()
# the adjoint is the discretised continuous one: its multipliers differ from the direct ones by the discretisation error, not by the
# Ritz residuals, hence a bound of its own on |mu_direct - mu_adjoint|
try:
    out = host.sensitivity_analysis(A, kdim, 2, tol=tol, outdir=outdir, seed=1, match_tol=5e-3)
except host.NlgError as e:
    # the pairing is refused: record what the two runs found (sensitivity_analysis has written both spectra) and stop
    lines = ["cylinder wake, Re = %g, lx1 = %d, E = %d, tau = 1, kdim = %d, tol = %g" % (re, hm.n, hm.E, kdim, tol), "REFUSED: %s" % e]
    for tag in ("dir", "adj"):
        sp = np.load(os.path.join(outdir, tag + "_eigenspectrum.npy"))
        lines.append("%s: lambda = %s, residuals %s" % (tag, ["%.6f%+.6fi" % (a, b) for a, b, _ in sp], ["%.2e" % r for _, _, r in sp]))
    lines.append("stepper %s" % A.stats())
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "cylinder_wavemaker.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(2)
lam, d, W, grad = out["eigvals"][0], out["d"][0], out["W"][0], out["grad"][0]
mu_d, mu_a = out["direct"][3], out["adjoint"][3]
lines = ["cylinder wake, Re = %g, lx1 = %d, E = %d, tau = 1, kdim = %d, tol = %g" % (re, hm.n, hm.E, kdim, tol),
         "direct  multipliers %s  residuals %s" % (np.array2string(mu_d, precision=8), np.array2string(out["direct"][1], precision=2)),
         "adjoint multipliers %s  residuals %s" % (np.array2string(mu_a, precision=8), np.array2string(out["adjoint"][1], precision=2)),
         "lambda = %.8f %+.8fi   d = <u^+, u^> = %.6e %+.6ei" % (lam.real, lam.imag, d.real, d.imag)]
w = W.get_field(0)
x, y = np.asarray(hm.x).ravel(), np.asarray(hm.y).ravel()
k = int(np.argmax(w))
lines.append("wavemaker: max W = %.6e at (x, y) = (%.4f, %.4f)" % (w[k], x[k], y[k]))
for half, sel in (("y > 0", y > 0), ("y < 0", y < 0)):
    kk = int(np.argmax(np.where(sel, w, -1.0)))
    lines.append("  peak in %s: W = %.6e at (%.4f, %.4f)" % (half, w[kk], x[kk], y[kk]))
for name, g in (("Re grad_U lambda", grad[0]), ("Im grad_U lambda", grad[1])):
    f = np.hypot(g.get_field(0), g.get_field(1))
    kk = int(np.argmax(f))
    lines.append("%s: max modulus %.6e at (%.4f, %.4f)" % (name, f[kk], x[kk], y[kk]))
sec = out["seconds"]
lines.append("cost: direct analysis %.1f s, adjoint analysis %.1f s, pairing + sensitivity kernel %.4f s; stepper %s" % (
    sec["direct"], sec["adjoint"], sec["sensitivity"], A.stats()))
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "cylinder_wavemaker.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
