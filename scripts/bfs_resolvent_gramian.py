#!/usr/bin/env python3
"""The reference's resolvent example on the GPU path: examples/back_fstep/gramian (bfs.usr: a Gaussian actuator in v centred at
(0.6, 1.0), width 0.6; for omega = 0.2, 0.4, ... : R = resolvent_linop(omega, bf); R%matvec(forcing, response); writes omega and
0.5 |response|^2 to amplitude.dat) on the reference's own mesh, boundary tags and base flow (tests/golden/reference_bfs_baseflow.npz),
bdf2, Re = 600, tolerances 1e-8 / 1e-6 (bfs.par).  The reference publishes no amplitudes for it; this run records ours.
The case's explicit filter (bfs.par:17-19: filterWeight = 0.01, filterCutoffRatio = 0.84) is on by default; --no-filter
reproduces the numbers published before the time stepper had it.

usage: bfs_resolvent_gramian.py [--filter | --no-filter] [number of frequencies, default 15]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from neklab_amd import host  # noqa: E402
from refdata import load_bfs  # noqa: E402

use_filter = "--no-filter" not in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--filter", "--no-filter")]
nfreq = int(sys.argv[1]) if len(sys.argv) > 1 else 15
hm, ux, uy, p, re, lxd, _ = load_bfs(with_bcs=True)
ctx = host.Context(0)
gm = host.Mesh(ctx, hm, lxd=lxd)
bf = host.nek_dvector(gm)
bf.set_field(host.VX, ux)
bf.set_field(host.VY, uy)
forcing, response = host.nek_zvector(gm), host.nek_zvector(gm)
forcing.zero()
x, y = hm.x.ravel(), hm.y.ravel()
forcing.re.set_field(host.VY, np.exp(-((x - 0.6) ** 2 + (y - 1.0) ** 2) / 0.6 ** 2))      # make_actuator, bfs.usr
filt = dict(filter_weight=0.01, filter_modes=host.filter_modes_from_cutoff_ratio(hm.n, 0.84)) if use_filter else {}
print("E = %d lx1 = %d, Re = %g, filter %s; actuator norm %.6e" % (hm.E, hm.n, re, filt or "off", forcing.norm()), flush=True)
print("# omega   0.5 |R(omega) f|^2   GMRES matvecs   time steps   seconds")
for i in range(1, nfreq + 1):
    omega = 0.2 * i
    R = host.resolvent_linop(omega, bf, re=re, torder=2, vtol=1e-8, ptol=1e-6, maxit_v=400, maxit_p=4000, **filt)
    response.zero()
    t0 = time.time()
    R.matvec(forcing, response)
    a = response.norm()
    st = R.last_operator.stats()
    print("%.1f   %.8e   %d   %d   %.1f" % (omega, 0.5 * a * a, R.gmres_matvecs, st["steps"], time.time() - t0), flush=True)
