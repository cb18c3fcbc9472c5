#!/usr/bin/env python3
"""Energy budget of the leading eigenpair of the cylinder wake (Re = 50, the fixture of tests/test_gpu_known_answer.py) through the
strong-form operator L ("The operator L itself").

For the leading pair mu = |mu| exp(+-i theta) of exp(tau L), with x, y the real and imaginary parts of the eigenvector (velocity and
the pressure the time stepper left in them), the growth rate log|mu| / tau is set against the Rayleigh quotient
    (<x, L x> + <y, L y>) / (<x, x> + <y, y>)
in the inner product of nek_dvector, split by term into production -<u, N u>, dissipation nu <u, lap u> and pressure work
-<u, grad p>; each term is one nlg_lns_apply (compute_LNS_conv, compute_LNS_laplacian, compute_LNS_gradp), their sum is apply_L.

usage: lns_budget.py [kdim] [tol] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from neklab_amd import host  # noqa: E402
from refdata import load_cylinder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("kdim", nargs="?", type=int, default=128)
ap.add_argument("tol", nargs="?", type=float, default=1e-6)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lns_budget.txt"))
ap.add_argument("--workdir", default=None, help="where eigs leaves its log files (default: a temporary directory)")
args = ap.parse_args()

hm, ux, uy, p, re, lxd, _ = load_cylinder(with_bcs=True)
ctx = host.Context(0)
gm = host.Mesh(ctx, hm, lxd=lxd)
bf = host.nek_dvector(gm)
bf.set_field(host.VX, ux)
bf.set_field(host.VY, uy)
tau = 1.0
A = host.exptA_linop(tau, bf, re=re, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=400, maxit_p=4000)   # 1cyl.par
A.init()
if args.workdir is None:
    import tempfile
    args.workdir = tempfile.mkdtemp()
os.makedirs(args.workdir, exist_ok=True)
eigvals, residuals, eigvecs, mu, nmv = host.linear_stability_analysis_fixed_point(A, args.kdim, 2, tol=args.tol, outdir=args.workdir, seed=1)
pair = eigvecs[:2]                                  # real LAPACK convention: (Re, Im) of the leading pair
L = host.lns_linop(bf, re)
w = host.nek_dvector(gm)
terms = (("production   -<u, N u>", host.compute_LNS_conv, -1.0), ("dissipation  nu <u, lap u>", host.compute_LNS_laplacian, 1.0),
         ("pressure work -<u, grad p>", host.compute_LNS_gradp, -1.0))
norm2 = sum(v.dot(v) for v in pair)
rows, total = [], 0.0
for name, fn, sign in terms:
    val = 0.0
    for v in pair:
        fn(L, v, w)
        val += sign * v.dot(w)
    rows.append((name, val / norm2))
    total += val / norm2
full = 0.0
for v in pair:
    host.apply_L(L, v, w)
    full += v.dot(w)
full /= norm2
growth = np.log(abs(mu[0])) / tau
lines = ["cylinder wake Re = %g, tau = %g, kdim = %d: mu_1 = %.8f %+.8fi, |mu_1| = %.7f, residual %.2e, %d matvecs" % (
    re, tau, args.kdim, mu[0].real, mu[0].imag, abs(mu[0]), residuals[0], nmv)]
lines += ["%-28s %+.6e" % r for r in rows]
lines += ["%-28s %+.6e" % ("sum of the three terms", total), "%-28s %+.6e" % ("Rayleigh quotient of apply_L", full),
          "%-28s %+.6e" % ("growth rate log|mu_1| / tau", growth), "%-28s %+.6e" % ("quotient minus growth rate", full - growth)]
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
