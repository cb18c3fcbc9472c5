#!/usr/bin/env python3
"""Wavenumber sweep of plane Poiseuille flow in lock-step ("Wavenumber lanes").

Re = 7500, tau = 1, the 2 pi box of tests/test_gpu_proj.py ((10, 12) elements, lx1 = 8), alphas = 1, 2, 3, 4.

1. Known answers: linear_stability_analysis_wavenumbers (four lanes on one operator) -- the leading |mu| per alpha against the
   Orr-Sommerfeld value exp(alpha Im(c) tau) of oracle/orr_sommerfeld.py (1.0022375, 0.9447741, 0.9337406, 0.9252785).
2. Cost: four exptA_proj_linop Arnoldi runs of N steps each through nlg_arnoldi_step, one after another, against ONE sweep of four lanes
   with N sweep steps (nlg_sweep_arnoldi_step): wall time of three alternating repetitions, min - max of each side, and kernel launches
   per time step from nlg_counters for both sides.

usage: poiseuille_sweep.py [--kdim K] [--steps N] [--reps R] [--skip-known]"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--kdim", type=int, default=60, help="Krylov dimension of the known-answer run (no restarts)")
ap.add_argument("--steps", type=int, default=12, help="Arnoldi steps per wavenumber in the cost comparison")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--skip-known", action="store_true")
args = ap.parse_args()

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402
from oracle.orr_sommerfeld import orr_sommerfeld  # noqa: E402

RE, TAU, ALPHAS = 7500.0, 1.0, (1.0, 2.0, 3.0, 4.0)
KW = dict(re=RE, torder=3, vtol=1e-11, ptol=1e-10, maxit_p=4000)
ctx = host.Context(0)
hm = box_mesh((10, 12), 8, lengths=(2 * np.pi, 2.0), periodic=(True, False), deform=0.0, origin=(0.0, -1.0))
gm = host.Mesh(ctx, hm)
bf = host.nek_dvector(gm)
bf.set_field(host.VX, 1.0 - np.asarray(hm.y) ** 2)


def counters():
    a, b = C.c_int64(0), C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


print("plane Poiseuille flow, Re = %g, tau = %g, E = %d, lx1 = %d, alphas = %s" % (RE, TAU, hm.E, hm.n, ALPHAS), flush=True)
if not args.skip_known:
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        res = host.linear_stability_analysis_wavenumbers(TAU, bf, ALPHAS, args.kdim, 2, tol=1e-6, seed=1, outdir=tmp, **KW)
        ctx.sync()
        wall = time.perf_counter() - t0
    print("known answers: one sweep of four lanes, kdim = %d, no restarts, %.1f s" % (args.kdim, wall))
    for al, (eigvals, residuals, eigvecs, mu, nmv) in zip(ALPHAS, res):
        c = orr_sommerfeld(RE, al)[0]
        want = abs(np.exp(-1j * al * c * TAU))
        print("  alpha = %g: |mu| = %.7f  Orr-Sommerfeld %.7f  difference %+.2e  residual %.1e  after %d steps"
              % (al, abs(mu[0]), want, abs(mu[0]) - want, residuals[0], nmv), flush=True)

# ---- cost: four single runs against one sweep of four lanes, N Arnoldi steps per wavenumber -------------------------------------
N = args.steps
singles = []
for al in ALPHAS:
    A = host.exptA_proj_linop(TAU, bf, al, idir=1, **KW)
    A.init()
    singles.append(A)
S = host.exptA_sweep_linop(TAU, bf, ALPHAS, idir=1, **KW)
S.init()
steps_per_matvec = S.info()["nsteps"] + KW["torder"] - 1
starts = []
for l in range(len(ALPHAS)):
    x = host.nek_dvector(gm)
    x.rand(True, seed=1 + l)
    starts.append(x)
S.proj_block(starts)
for x in starts:
    x.scal(1.0 / x.norm())
Bs = [host.KrylovBasis(gm, N + 1) for _ in ALPHAS]


def run_singles():
    Hs = []
    for l, A in enumerate(singles):
        Bs[l][0].assign(starts[l])
        H = np.zeros((N + 1, N), order="F")
        for k in range(N):
            host.arnoldi_step(A, Bs[l], k, H)
        Hs.append(H)
    return Hs


def run_sweep():
    for l in range(len(ALPHAS)):
        Bs[l][0].assign(starts[l])
    Hw = np.zeros((len(ALPHAS), N, N + 1))
    for k in range(N):
        host.sweep_arnoldi_step(S, Bs, k, Hw)
    return [Hw[l].T for l in range(len(ALPHAS))]


def timed(fn):
    ctx.sync()
    l0, _ = counters()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return time.perf_counter() - t0, counters()[0] - l0, out


timed(run_singles)          # warm-up of both sides
timed(run_sweep)
t = {"single": [], "sweep": []}
launches = {}
for _ in range(args.reps):
    for name, fn in (("single", run_singles), ("sweep", run_sweep)):
        dt, nl, H = timed(fn)
        t[name].append(dt)
        launches[name] = nl
        if name == "single":
            Href = H
        else:
            dev = max(np.max(np.abs(a - b)) / np.max(np.abs(b)) for a, b in zip(H, Href))
print("cost: %d Arnoldi steps per wavenumber, %d time steps per matvec (dt = %g), %d repetitions, alternating"
      % (N, steps_per_matvec, S.info()["dt"], args.reps))
for name, what in (("single", "four single runs (nlg_arnoldi_step) "), ("sweep", "one sweep of four lanes           ")):
    print("  %s wall %s s   min %.3f  max %.3f;  %d launches = %.1f per time step of the %s"
          % (what, " ".join("%.3f" % a for a in t[name]), min(t[name]), max(t[name]), launches[name],
             launches[name] / (N * steps_per_matvec * (len(ALPHAS) if name == "single" else 1)),
             "single-lane run" if name == "single" else "four-lane block run"))
print("  launches for the four wavenumbers per time step: %.1f (single runs) against %.1f (sweep)"
      % (launches["single"] / (N * steps_per_matvec), launches["sweep"] / (N * steps_per_matvec)))
spread = max(max(t[k]) - min(t[k]) for k in t)
gain = min(t["single"]) - min(t["sweep"])
print("  ratio of the minima: %.2f x;  gain %.3f s, larger spread of the two sides %.3f s: the gain %s twice that spread"
      % (min(t["single"]) / min(t["sweep"]), gain, spread, "exceeds" if gain > 2 * spread else "does NOT exceed"))
if gain <= 0:
    print("  the sweep is NOT faster than the four single runs at this size")
print("  largest deviation of a lane's Hessenberg matrix from its single run: %.1e of max|H|" % dev)
