#!/usr/bin/env python3
"""What a coupled (orbit-mode) time step costs ("Coupled (orbit) mode").

The headline mesh of bench.py -- E = 25 x 20 x 20 = 10^4 elements, lx1 = 8 -- and two kinds of step: a coupled step with s = 1, 2, 3
perturbation lanes (the base flow is lane s + 1 and pays one sem_conv_setup per step) and a frozen block step of s + 1 lanes.  For
each: milliseconds per time step (rounds alternating between the operators after a warm-up of each), kernel launches per time step
(nlg_counters) and the share of the per-step set-up, taken as what the nonlinear step costs more than the linear step of one lane
(the only thing the two differ in), over the coupled step.

usage: floquet_cost.py [--rounds R] [--nel a,b,c] [--lx1 n]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--nel", default="25,20,20")
ap.add_argument("--lx1", type=int, default=8)
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n = args.lx1

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ctx = host.Context(0)
hm = box_mesh(nel, n, deform=0.05)
gm = host.Mesh(ctx, hm)
X0 = host.nek_dvector(gm)
ph = [2 * np.pi * c / L for c, L in zip((hm.x, hm.y, hm.z), hm.lengths)]
U = [np.sin(ph[1]) * np.cos(ph[2]), 0.5 * np.sin(ph[2]) * np.cos(ph[0]), 0.5 * np.sin(ph[0]) * np.cos(ph[1])]
for i in range(3):
    X0.set_field(i, U[i] * hm.mask[i])
NSTEPS, DT = 2, 0.002
kw = dict(re=100.0, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=DT, no_history=1)
vin, vout = [host.nek_dvector(gm) for _ in range(4)], [host.nek_dvector(gm) for _ in range(4)]
for v, x in enumerate(vin):
    x.rand(True, seed=10 + v)

runs = {}
frozen = host.exptA_linop(NSTEPS * DT, X0, **kw)
frozen.init()
orbit = host.exptA_orbit_linop(NSTEPS * DT, X0, **kw)
nonlin = host.exptA_linop(NSTEPS * DT, X0, **kw)
nonlin.init()
for s in (1, 2, 3):
    runs["coupled s=%d" % s] = lambda s=s: orbit.matvec_block(vin[:s], vout[:s])
    runs["frozen block of %d" % (s + 1)] = lambda s=s: frozen.matvec_block(vin[:s + 1], vout[:s + 1])
runs["linear, 1 lane"] = lambda: frozen.matvec(vin[0], vout[0])
runs["nonlinear map"] = lambda: host.check(ctx.lib.nlg_linop_nonlinear_map(nonlin.h, X0.h, vout[0].h))


def launches():
    a = C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), None))
    return a.value


nl = {}
for name, run in runs.items():
    run()                                 # warm-up: code objects, work buffers, iteration-count predictions
    run()
    ctx.sync()
    l0 = launches()
    run()
    ctx.sync()
    nl[name] = (launches() - l0) / NSTEPS
print("E = %d, lx1 = %d, %d time steps of dt = %g per run (no history steps); launches include what a run launches around its steps"
      % (int(np.prod(nel)), n, NSTEPS, DT), flush=True)
ms = {name: [] for name in runs}
for r in range(args.rounds):
    for name, run in runs.items():
        ctx.sync()
        t0 = time.perf_counter()
        run()
        ctx.sync()
        ms[name].append(1e3 * (time.perf_counter() - t0) / NSTEPS)
med = {name: float(np.median(t)) for name, t in ms.items()}
for name, t in ms.items():
    print("%-18s  ms per time step: %s   median %.3f  (min %.3f, max %.3f);  launches per time step %.1f"
          % (name, " ".join("%.3f" % a for a in t), med[name], min(t), max(t), nl[name]))
setup = med["nonlinear map"] - med["linear, 1 lane"]
print("per-step set-up (nonlinear map - linear step of one lane; the map also redoes the operator set-up once per run): %.3f ms" % setup)
for s in (1, 2, 3):
    c, f = med["coupled s=%d" % s], med["frozen block of %d" % (s + 1)]
    print("s = %d: coupled %.3f ms, frozen block of %d %.3f ms, difference %+.3f ms = %.1f %% of the coupled step; launches %+.1f"
          % (s, c, s + 1, f, c - f, 100.0 * (c - f) / c, nl["coupled s=%d" % s] - nl["frozen block of %d" % (s + 1)]))
