#!/usr/bin/env python3
"""The periodic-orbit workflow from its first stage: DNS with history points and a recurrence monitor -> a guess (X, T) ->
newton_periodic_orbit -> linear_stability_analysis_periodic_orbit.

The reference's case for this is the cylinder at Re = 180 (examples/cylinder/dns/Re180 feeding examples/cylinder/newton/
Re180_periodic_orbit).  It ships the mesh of that case but not its start state (BF_1cyl.fld), and how long a run from rest needs to
settle on the limit cycle has NOT been measured here: that case is not run by this script.  The workflow is shown on a case whose
answer is known instead: a doubly periodic box (4 x 4 elements, lx1 = 8) in which an array of vortices is carried by a uniform stream
U0.  By Galilean invariance the pattern returns to its place after T = Lx / U0 while it decays slowly (by exp(-2 nu k^2 T)), so the
run comes back NEAR its start, not onto it: d(t) has a recurrence minimum of small depth at T, the probe signals oscillate with the
same period, and Newton then reports how well an orbit through that guess closes -- it is not expected to converge to a non-trivial
orbit, since the only exactly periodic states of this case are the uniform streams.

usage: dns_orbit_guess.py [--re R] [--dt DT] [--u0 U0] [--newton N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--re", type=float, default=2000.0)
ap.add_argument("--dt", type=float, default=0.005)
ap.add_argument("--u0", type=float, default=1.0)
ap.add_argument("--newton", type=int, default=2, help="Newton iterations to try from the guess (0: none)")
args = ap.parse_args()

from neklab_amd import host, nekio  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ctx = host.Context(0)
L = 1.0
hm = box_mesh((4, 4), 8, lengths=(L, L), periodic=(True, True), deform=0.0)
gm = host.Mesh(ctx, hm)
k = 2 * np.pi / L
X0 = host.nek_dvector(gm)
X0.set_field(0, args.u0 + 0.2 * np.sin(k * hm.x) * np.cos(k * hm.y))
X0.set_field(1, -0.2 * np.cos(k * hm.x) * np.sin(k * hm.y))
T_exact = L / args.u0
kw = dict(re=args.re, torder=3, vtol=1e-11, ptol=1e-11, maxit_v=400, maxit_p=4000)

# 1. the run: five history points across the box, the start as the reference of the recurrence norm
dns = host.nek_dns(X0, dt=args.dt, **kw)
hp = host.history_points(gm, np.array([[0.1, 0.3], [0.3, 0.3], [0.5, 0.5], [0.7, 0.2], [0.9, 0.8]]) * L)
dns.set_history_points(hp)
nsteps = int(round(1.6 * T_exact / args.dt))
guess = host.dns_orbit_guess(dns, nsteps)
s = dns.series()
got = host.recurrence_period(s["time"], s["dist"])
Tp = host.probe_period(s["time"], s["probe"][:, 0, 1])
print("DNS: %d steps of dt = %g; recurrence minimum at T = %.6f with d / max d = %.3e; probe period (uy at point 1) %.6f; Lx / U0 = %.6f"
      % (nsteps, dns.info()["dt"], got[0], got[1], Tp, T_exact))
nekio.write_his(os.path.join(os.getcwd(), "dns_orbit_guess.his"), hp.xyz, s["time"], s["probe"])
dns.close()
hp.close()
if guess is None:
    sys.exit("no recurrence minimum: no guess")

# 2. Newton-Krylov from the guess: the reference snapshot and the period read off d(t)
if args.newton > 0:
    S = host.nek_upo_system(guess, re=args.re, torder=3, dt=args.dt, vtol=1e-11, ptol=1e-11, maxit_v=400, maxit_p=4000)
    out = host.newton_periodic_orbit(S, guess, 1e-8, maxiter=args.newton, kdim=30, log=print)
    print("Newton: %s after %d iterations, residuals %s, periods %s"
          % ("converged" if out["converged"] else "not converged", out["iterations"], ["%.3e" % r for r in out["residuals"]],
             ["%.6f" % t for t in out["periods"]]))
    S.close()

# 3. Floquet multipliers of the orbit through the (updated) guess
A = host.exptA_orbit_linop(guess.T, guess.vec, dt=args.dt, **kw)
mu, expo, res, _, info = host.linear_stability_analysis_periodic_orbit(A, kdim=24, nev=4, outdir=os.getcwd())
print("orbit closure |Phi_T(X) - X| / |X| = %.3e; leading Floquet multipliers %s (residuals %s)"
      % (A.closure(), ["%.5f%+.5fj" % (m.real, m.imag) for m in mu], ["%.1e" % r for r in res]))
A.close()
