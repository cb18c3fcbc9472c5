#!/usr/bin/env python3
"""What the explicit modal filter costs in the time stepper ("Explicit filter").

The headline shape of bench.py -- E = 25 x 20 x 20 = 10^4 elements, lx1 = 8, block of 4 vectors -- advanced by
nlg_linop_matvec_block with the filter off and on (filterWeight 0.01, one mode: the reference's settings at lx1 = 8), on in both
variants: "fused" (the default: velocity update and filter in one kernel) and "separate" (NLG_FILTER_FUSED=0: k_axpy_w, then the
filter alone).  The three operators alternate on one GPU after a warm-up of each; milliseconds per block time step.

The kernels in question are a small part of such a step; their durations come from a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -o filter --output-format csv -- python3 scripts/filter_cost.py --trace-run
(two block matvecs of either variant and nothing else), and `filter_cost.py --kernel-stats DIR/.../filter_kernel_stats.csv` sets the
averages against the algorithmic bytes.

usage: filter_cost.py [--rounds R] [--nel a,b,c] [--lx1 n] [--block s] | --trace-run | --kernel-stats CSV"""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--nel", default="25,20,20")
ap.add_argument("--lx1", type=int, default=8)
ap.add_argument("--block", type=int, default=4)
ap.add_argument("--trace-run", action="store_true", help="two filtered block matvecs of either variant and nothing else (to be run under a kernel trace)")
ap.add_argument("--kernel-stats", default=None, help="reduce a rocprofv3 kernel-stats csv of a --trace-run")
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n, s = args.lx1, args.block
E = int(np.prod(nel))
npts = E * n ** 3
HBM_PEAK = 8.0e12      # bytes per second (MI355X)


def algorithmic_bytes(name):
    """bytes one launch has to move, all lanes and components"""
    if "k_filter3" in name:
        fused = "true" in name.split("k_filter3")[1].split(">")[0]
        b = 16 * npts * 3 * s                        # every velocity point in and out
        if fused:
            b += 8 * npts * 3 * s + 8 * npts * 3 + 4 * n ** 3     # the increment per lane, the weights once, the slot table
        return b
    if "k_axpy_w" in name:
        return 16 * npts * 3 * s + 8 * npts * 3 * s + 8 * npts * 3
    return None


if args.kernel_stats:
    print("# kernel, calls, average us, algorithmic MB, achieved TB/s, share of the %.0f TB/s HBM peak" % (HBM_PEAK / 1e12))
    for row in csv.DictReader(open(args.kernel_stats)):
        b = algorithmic_bytes(row["Name"])
        if b is None:
            continue
        avg = float(row["AverageNs"]) * 1e-9
        short = re.search(r"k_\w+(<[^>]*>)?", row["Name"]).group(0)
        print("%-40s %5d  %9.1f  %8.1f  %6.2f  %5.2f" % (short, int(row["Calls"]), avg * 1e6, b / 1e6, b / avg / 1e12, b / avg / HBM_PEAK))
    sys.exit(0)

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ctx = host.Context(0)
hm = box_mesh(nel, n, deform=0.05)
gm = host.Mesh(ctx, hm)
bf = host.nek_dvector(gm)
ph = [2 * np.pi * c / L for c, L in zip((hm.x, hm.y, hm.z), hm.lengths)]
U = [np.sin(ph[1]) * np.cos(ph[2]), 0.5 * np.sin(ph[2]) * np.cos(ph[0]), 0.5 * np.sin(ph[0]) * np.cos(ph[1])]
for i in range(3):
    bf.set_field(i, U[i] * hm.mask[i])
kw = dict(re=100.0, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=0.002)
filt = dict(filter_weight=0.01, filter_modes=host.filter_modes_from_cutoff_ratio(n, 0.84))
ops = {}
for name, env in (("fused", "1"), ("separate", "0")):      # the switch is read when the operator is created
    os.environ["NLG_FILTER_FUSED"] = env
    ops[name] = host.exptA_linop(0.004, bf, **kw, **filt)
del os.environ["NLG_FILTER_FUSED"]
if not args.trace_run:
    ops["filter off"] = host.exptA_linop(0.004, bf, **kw)
vin, vout = [host.nek_dvector(gm) for _ in range(s)], [host.nek_dvector(gm) for _ in range(s)]
for v, x in enumerate(vin):
    x.rand(True, seed=10 + v)
steps = {}
for name, A in ops.items():
    A.init()
    s0 = A.stats()["steps"]
    A.matvec_block(vin, vout)            # warm-up: code objects, work buffers, iteration-count predictions
    A.matvec_block(vin, vout)
    ctx.sync()
    steps[name] = (A.stats()["steps"] - s0) // (2 * s)
print("E = %d, lx1 = %d, block of %d, %d time steps per block matvec, filter %s" % (E, n, s, steps["fused"], filt), flush=True)
if args.trace_run:
    sys.exit(0)
ms = {name: [] for name in ops}
for r in range(args.rounds):
    for name, A in ops.items():
        ctx.sync()
        t0 = time.perf_counter()
        A.matvec_block(vin, vout)
        ctx.sync()
        ms[name].append(1e3 * (time.perf_counter() - t0) / steps[name])
for name, t in ms.items():
    print("%-10s  ms per block time step, rounds alternating: %s   median %.3f  (min %.3f, max %.3f)"
          % (name, " ".join("%.3f" % a for a in t), float(np.median(t)), min(t), max(t)))
for name in ("fused", "separate"):
    print("%s - filter off, medians: %+.3f ms per block time step" % (name, float(np.median(ms[name])) - float(np.median(ms["filter off"]))))
