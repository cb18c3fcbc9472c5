#!/usr/bin/env python3
"""The reference's OTD case (examples/poiseuille/OTD_steady): plane Poiseuille flow 1 - y^2 at Re = 5000, bdf2, two OTD modes about the
frozen base flow, time step from CFL 0.4, tolerances 1e-8 / 1e-6, no residual projection (poiseuille.par), on the box of
tests/test_gpu_known_answer.py::test_poiseuille_re7500_orr_sommerfeld (10 x 12 elements, lx1 = 8, 2 pi x 2, periodic in x).

Runs host.otd_analysis to `--endtime` (the case's 200 by default) and leaves Ls.dat / Lr.dat and the `rst` basis files in `--outdir`;
what it prints -- the set-up, every `--echo`-th logged row, the last Lr and the time per step -- is the record kept as
profiles/otd_poiseuille.log.  The modes start from random fields (seeds 1, 2; the case's OTDIC files are Nek5000 restart files of its
own mesh).  Expectation: after the transients the leading eigenvalue of Lr is the least stable Orr-Sommerfeld eigenvalue that fits
the box, a complex pair with Re(lambda) slightly negative at this subcritical Reynolds number (Re_c = 5772 at alpha = 1.02).

usage: otd_poiseuille.py [--endtime T] [--printstep N] [--echo K] [--outdir DIR]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--endtime", type=float, default=200.0)
ap.add_argument("--printstep", type=int, default=50)
ap.add_argument("--echo", type=int, default=10)
ap.add_argument("--outdir", default="otd_poiseuille_out")
args = ap.parse_args()

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

os.makedirs(args.outdir, exist_ok=True)
ctx = host.Context(0)
hm = box_mesh((10, 12), 8, lengths=(2 * np.pi, 2.0), periodic=(True, False), deform=0.0, origin=(0.0, -1.0))
gm = host.Mesh(ctx, hm)
bf = host.nek_dvector(gm)
bf.set_field(host.VX, 1.0 - hm.y ** 2)
OTD = host.nek_otd(bf, 2, re=5000.0, torder=2, vtol=1e-8, ptol=1e-6, pproj=0, maxit_p=4000)       # cfl_limit = 0.4 (init_OTD)
OTD.op.init()
dt = OTD.op.info()["dt"]
nsteps = int(np.ceil(args.endtime / dt))
opts = host.otd_opts(startstep=1, printstep=args.printstep, orthostep=10, iostep=0, iorststep=nsteps, solve_baseflow=False)
print("plane Poiseuille flow, Re = 5000, bdf2, r = 2, E = %d, lx1 = %d; dt = %.6f (CFL %.3f), %d steps to t = %.2f, a row every %d steps"
      % (hm.E, hm.n, dt, OTD.op.info()["cfl"], nsteps, nsteps * dt, args.printstep), flush=True)
t0 = time.perf_counter()
rows = host.otd_analysis(OTD, opts, nsteps=nsteps, outdir=args.outdir)
ctx.sync()
wall = time.perf_counter() - t0
for k, row in enumerate(rows):
    if k % args.echo == 0 or k == len(rows) - 1:
        print(host.otd_log_line(row["istep"], row["time"], (" Ls ", row["sigma"]), (" Lr%Re ", row["lambda"].real), (" Lr%Im ", row["lambda"].imag)))
Lr, G = OTD.reduced()
print("Lr at t = %.3f:\n%s\n|G - I| before the read-out: %.3e" % (OTD.info()["time"], Lr, np.abs(G - np.eye(2)).max()))
st = OTD.op.stats()
print("%.1f s for %d steps: %.3f ms per step of 2 lanes (read-outs and files included); iterations per lane step: velocity %.1f, pressure %.1f"
      % (wall, nsteps, 1e3 * wall / nsteps, st["v_iters"] / max(st["steps"], 1), st["p_iters"] / max(st["steps"], 1)))
print("files:", " ".join(sorted(os.listdir(args.outdir))))
OTD.close()
