#!/usr/bin/env python3
"""What the monitors of a DNS run cost per time step.

The headline mesh of bench.py -- E = 25 x 20 x 20 = 10^4 elements, lx1 = 8 -- and two nek_dns runs from the same state with the same
fixed dt, past their start-up: one with history points and the recurrence norm, one with neither.  Rounds alternate between the two
on the same device in the same process; per run: milliseconds per time step (median and spread over the rounds), kernel launches and
collective sites per time step (nlg_counters).  Done for every point count of --points (random points inside the box).  The monitors
add three launches per step: k_probe_sample reads one element per point and field, k_recur_partial streams the velocity, the
reference and bm1 once (7 fields of lvn doubles = 0.29 GB at this size).

usage: dns_monitor_cost.py [--rounds R] [--nel a,b,c] [--lx1 n] [--steps K] [--points 5,1000]"""
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
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--points", default="5,1000")
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


print("E = %d, lx1 = %d, dt = %g, %d time steps per timed call, past 4 start-up steps, %d rounds alternating" % (int(np.prod(nel)), n, kw["dt"], K, args.rounds),
      flush=True)
rng = np.random.default_rng(1)
for npts in [int(a) for a in args.points.split(",")]:
    xyz = rng.uniform(0.02, 0.98, (npts, 3)) * np.array(hm.lengths)
    t0 = time.perf_counter()
    hp = host.history_points(gm, xyz)
    t_loc = time.perf_counter() - t0
    runs = {}
    for name in ("monitors", "plain"):
        d = host.nek_dns(X0, **kw)
        if name == "monitors":
            d.set_history_points(hp)
            d.set_reference()
        d.advance(4)
        ctx.sync()
        runs[name] = d
    ms = {k: [] for k in runs}
    cnt = {}
    for _ in range(args.rounds):
        for name, d in runs.items():
            l0, c0 = counters()
            ctx.sync()
            t0 = time.perf_counter()
            d.advance(K)
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / K)
            l1, c1 = counters()
            cnt[name] = ((l1 - l0) / K, (c1 - c0) / K)
    s = runs["monitors"].series()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print("%5d points (located in %.2f s on the host): with monitors %.3f ms/step [%.3f .. %.3f], without %.3f ms/step [%.3f .. %.3f]; "
          "difference of the medians %+.3f ms = %+.2f %%; launches/step %.1f vs %.1f, collectives/step %.1f vs %.1f; %d samples, d(t) last %.4e"
          % (npts, t_loc, med["monitors"], min(ms["monitors"]), max(ms["monitors"]), med["plain"], min(ms["plain"]), max(ms["plain"]),
             med["monitors"] - med["plain"], 100.0 * (med["monitors"] - med["plain"]) / med["plain"], cnt["monitors"][0], cnt["plain"][0],
             cnt["monitors"][1], cnt["plain"][1], len(s["time"]), s["dist"][-1]), flush=True)
    for d in runs.values():
        d.close()
    hp.close()
