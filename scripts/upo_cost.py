#!/usr/bin/env python3
"""What the border of the periodic-orbit Jacobian costs ("Periodic-orbit Newton").

The headline mesh of bench.py -- E = 25 x 20 x 20 = 10^4 elements, lx1 = 8 -- an operator in orbit mode, no restart history, and
  * a Jacobian matvec (nlg_upo_jac_matvec: coupled matvec + border) against the bare coupled matvec (nlg_linop_matvec), in
    milliseconds per call, rounds alternating after a warm-up of each;
  * the border alone on an existing M v (nlg_upo_border): the fused pass k_upo_border against the composition sub + axpby + dot,
    in microseconds per call (each call ends with the copy of the phase row to the host, as in use), `--inner` calls per sample.
The time-derivative capture k_bdf_ddt (three launches per run) and the border kernels are a small part of a matvec; their durations
come from a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -o upo --output-format csv -- python3 scripts/upo_cost.py --trace-run
(the warm-up and nothing else: two coupled and two Jacobian matvecs, so four runs capture the derivatives and two carry a border), and
`upo_cost.py --kernel-stats DIR/.../upo_kernel_stats.csv` sets them against the total of the trace.

usage: upo_cost.py [--rounds R] [--inner K] [--nel a,b,c] [--lx1 n] | --trace-run | --kernel-stats CSV"""
import argparse
import csv
import ctypes as C
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--nel", default="25,20,20")
ap.add_argument("--lx1", type=int, default=8)
ap.add_argument("--trace-run", action="store_true", help="the warm-up alone: two coupled and two Jacobian matvecs (to be run under a kernel trace)")
ap.add_argument("--kernel-stats", default=None, help="reduce a rocprofv3 kernel-stats csv of a --trace-run")
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n = args.lx1

if args.kernel_stats:
    rows = list(csv.DictReader(open(args.kernel_stats)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print("# kernel, calls, average us, share of the trace's kernel time (total %.1f ms)" % (total * 1e-6))
    for r in rows:
        m = re.search(r"k_(bdf_ddt|upo_border|dot_partial|axpby)\b", r["Name"])
        if m:
            print("%-16s %6d  %9.1f  %7.3f %%" % (m.group(0), int(r["Calls"]), float(r["AverageNs"]) * 1e-3, 100.0 * float(r["TotalDurationNs"]) / total))
    sys.exit(0)

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
kw = dict(torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=DT, no_history=1)
S = host.nek_upo_system(host.nek_ext_dvector(gm, T=NSTEPS * DT, _vec=X0), re=100.0, fixed_nsteps=NSTEPS, **kw)
lib = ctx.lib
v = host.nek_ext_dvector(gm, T=0.3)
v.vec.rand(True, seed=10)
out, w = host.nek_ext_dvector(gm), host.nek_dvector(gm)
t = C.c_double()

runs = {
    "coupled matvec": lambda: S.op.matvec(v.vec, w),
    "jacobian matvec": lambda: S.jac_matvec(v, out),
}
for run in runs.values():                  # warm-up: code objects, work buffers, iteration-count predictions
    run()
    run()
ctx.sync()
print("E = %d, lx1 = %d, %d time steps of dt = %g per matvec, no history" % (int(np.prod(nel)), n, NSTEPS, DT), flush=True)
if args.trace_run:
    sys.exit(0)

ms = {name: [] for name in runs}
for r in range(args.rounds):
    for name, run in runs.items():
        ctx.sync()
        t0 = time.perf_counter()
        run()
        ctx.sync()
        ms[name].append(1e3 * (time.perf_counter() - t0))
med = {name: float(np.median(a)) for name, a in ms.items()}
for name, a in ms.items():
    print("%-16s ms per call: %s   median %.3f  (min %.3f, max %.3f)" % (name, " ".join("%.3f" % x for x in a), med[name], min(a), max(a)))
d = med["jacobian matvec"] - med["coupled matvec"]
print("border = jacobian - coupled, medians: %+.3f ms = %.2f %% of the Jacobian matvec" % (d, 100.0 * d / med["jacobian matvec"]))

us = {"fused (k_upo_border)": [], "composed (sub + axpby + dot)": []}
for r in range(args.rounds + 1):           # (first round: warm-up)
    for name, composed in zip(us, (0, 1)):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            host.check(lib.nlg_upo_border(S.h, v.vec.h, 1e-6, w.h, C.byref(t), composed))
        ctx.sync()
        if r > 0:
            us[name].append(1e6 * (time.perf_counter() - t0) / args.inner)
mu = {name: float(np.median(a)) for name, a in us.items()}
for name, a in us.items():
    print("%-30s us per call: %s   median %.1f  (min %.1f, max %.1f)" % (name, " ".join("%.1f" % x for x in a), mu[name], min(a), max(a)))
f, c = mu["fused (k_upo_border)"], mu["composed (sub + axpby + dot)"]
print("fused / composed = %.3f  (six streams against nine: 0.667 if both ran at the same bandwidth)" % (f / c))
