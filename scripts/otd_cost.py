#!/usr/bin/env python3
"""What the OTD part of a time step costs ("OTD mode").

The headline mesh of bench.py -- E = 25 x 20 x 20 = 10^4 elements, lx1 = 8 -- and, for r = 1 .. 4 lanes, two runs of the same nek_otd
object kind past its start-up (no transform in the timed steps): with OTD (reduction pass + forcing pass in every step) and with
`startstep` out of reach, which is the plain block step of r lanes (what nlg_linop_matvec_block advances per time step).  For each:
milliseconds per time step (rounds alternating between the runs after a warm-up of each), kernel launches and reduction sites per
time step (nlg_counters), and the time of the "vec_ops" class of nlg_prof_*, in which the OTD kernels run.  Byte counts for comparison
(DESIGN.md): at r = 3 the reduce pass reads about 1.5 GB, the force pass moves about 0.9 GB.

usage: otd_cost.py [--rounds R] [--nel a,b,c] [--lx1 n] [--steps K]"""
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
ap.add_argument("--steps", type=int, default=2)
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n, K = args.lx1, args.steps

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
kw = dict(re=100.0, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=0.002)


def counters():
    a, b = C.c_int64(0), C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


def vec_ops_ms():
    cnt, ms = C.c_int64(0), C.c_double(0.0)
    host.check(ctx.lib.nlg_prof_get(ctx.h, b"vec_ops", C.byref(cnt), C.byref(ms)))
    return ms.value


print("E = %d, lx1 = %d, dt = %g, %d time steps per timed call, past the 12 start-up steps" % (int(np.prod(nel)), n, kw["dt"], K), flush=True)
for r in (1, 2, 3, 4):
    runs = {}
    for name, start in (("with OTD", 1), ("block step", 10 ** 8)):
        O = host.nek_otd(X0, r, **kw)
        O.init(host.otd_opts(startstep=start, orthostep=10 ** 8, solve_baseflow=False))
        O.advance(12)
        runs[name] = O
    info = {}
    for name, O in runs.items():
        ctx.sync()
        l0, c0 = counters()
        host.check(ctx.lib.nlg_prof_reset(ctx.h))
        host.check(ctx.lib.nlg_prof_enable(ctx.h, 1 << 9))      # class 9 = "vec_ops"
        O.advance(K)
        ctx.sync()
        l1, c1 = counters()
        info[name] = ((l1 - l0) / K, (c1 - c0) / K, vec_ops_ms() / K)
        host.check(ctx.lib.nlg_prof_enable(ctx.h, 0))
    ms = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, O in runs.items():
            ctx.sync()
            t0 = time.perf_counter()
            O.advance(K)
            ctx.sync()
            ms[name].append(1e3 * (time.perf_counter() - t0) / K)
    med = {name: float(np.median(t)) for name, t in ms.items()}
    for name in runs:
        print("r = %d  %-10s  ms per time step: %s   median %.3f;  launches %.1f, reduction sites %.1f, vec_ops class %.3f ms per step"
              % (r, name, " ".join("%.3f" % a for a in ms[name]), med[name], *info[name]), flush=True)
    print("r = %d  OTD adds %+.3f ms = %.1f %% of the block step (vec_ops class: %+.3f ms)"
          % (r, med["with OTD"] - med["block step"], 100.0 * (med["with OTD"] - med["block step"]) / med["block step"],
             info["with OTD"][2] - info["block step"][2]), flush=True)
    for O in runs.values():
        O.close()
