#!/usr/bin/env python3
"""What the sensitivity fields cost: one nlg_sens_apply of four complex pairs (gradient only, and with every
output) at the shape of scripts/lns_cost.py, E = 25 x 20 x 20 = 10^4 elements, lx1 = 8, next to the same gradient fields formed from
calls that existed before: per pair the four real combinations of S_re and S_im, each a lns_linop.set_baseflow(u) +
compute_LNS_conv(a, trans=True) -- the adjoint convective term -(u . grad) a + (grad u)^T a is -S(u, a) -- followed by the axpby that
combines and scales them.  Bytes: the kernel's algorithmic bytes against the HBM peak of 8 TB/s.  A record, not a gate.

usage: sens_cost.py [--rounds R] [--reps K] [--nel a,b,c] [--lx1 n] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--nel", default="25,20,20")
ap.add_argument("--lx1", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sens_cost.txt"))
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n = args.lx1
dim = len(nel)
E = int(np.prod(nel))
npts = E * n ** dim
HBM_PEAK = 8.0e12      # bytes per second (MI355X)

from neklab_amd import host  # noqa: E402
from neklab_amd._lib import dptr, vp  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402


def sens_bytes(s, nout, wm):
    """bytes one launch of k_lns_sens has to move for s complex pairs: per pair the 4 dim input fields, nout output vectors of dim
    fields (and the wavemaker); once per element the dim^2 rst, jac and the masks"""
    return npts * (s * (8 * 4 * dim + 8 * dim * nout + (8 if wm else 0)) + 8 * dim * dim + 8 + 8 * dim)


ctx = host.Context(0)
hm = box_mesh(nel, n, deform=0.05)
gm = host.Mesh(ctx, hm)
S = 4
B = host.KrylovBasis(gm, 4 * S)
for v in range(4 * S):
    B[v].rand(True, seed=30 + v)
pairs = [[B[4 * v + q] for q in range(4)] for v in range(S)]
outs = [[host.nek_dvector(gm) for _ in range(S)] for _ in range(5)]   # grad_re, grad_im, transp_re, transp_im, wavemaker
scale = np.array([[0.8, -0.3]] * S).reshape(-1)


def arr(vs):
    return (vp * S)(*[x.h for x in vs]) if vs is not None else None


def kernel(all_outputs):
    o = [arr(x) for x in outs] if all_outputs else [arr(outs[0]), arr(outs[1]), None, None, None]
    host.check(gm.lib.nlg_sens_apply(gm.h, S, arr([p[0] for p in pairs]), arr([p[1] for p in pairs]), arr([p[2] for p in pairs]),
                                     arr([p[3] for p in pairs]), dptr(scale), *o))


L = host.lns_linop(pairs[0][0], 100.0)
tmp, sre, sim = host.nek_dvector(gm), host.nek_dvector(gm), host.nek_dvector(gm)


def composed():
    """grad_re, grad_im of the four pairs from set_baseflow + compute_LNS_conv(trans=True): S(u, a) = -conv_adjoint(base = u, a)"""
    for v in range(S):
        ur, ui, ar, ai = pairs[v]
        sre.zero()
        sim.zero()
        for u, a, dst, sgn in ((ur, ar, sre, -1.0), (ui, ai, sre, -1.0), (ui, ar, sim, -1.0), (ur, ai, sim, 1.0)):
            L.set_baseflow(u)
            host.compute_LNS_conv(L, a, tmp, True)
            dst.axpby(sgn, tmp, 1.0)
        outs[0][v].zero()
        outs[0][v].axpby(scale[0], sre, 1.0)
        outs[0][v].axpby(-scale[1], sim, 1.0)
        outs[1][v].zero()
        outs[1][v].axpby(scale[0], sim, 1.0)
        outs[1][v].axpby(scale[1], sre, 1.0)


# the two routes form the same fields (the composed one carries the dealiased weak term over the local mass instead of the pointwise
# product: equal to discretisation error only, on random fields not at all) -- the comparison is one of cost
variants = [("nlg_sens_apply, grad only", lambda: kernel(False)), ("nlg_sens_apply, all outputs", lambda: kernel(True)),
            ("set_baseflow + compute_LNS_conv", composed)]
for _, fn in variants:
    fn()
ctx.sync()
us = {name: [] for name, _ in variants}
for r in range(args.rounds):
    for name, fn in variants:
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        ctx.sync()
        us[name].append(1e6 * (time.perf_counter() - t0) / args.reps)
lines = ["E = %d, lx1 = %d, %d-D, %d complex pairs, %d rounds of %d calls; microseconds per call, median (min .. max)" % (E, n, dim, S, args.rounds, args.reps)]
for name, _ in variants:
    t = us[name]
    line = "%-32s %10.1f (%.1f .. %.1f)" % (name, float(np.median(t)), min(t), max(t))
    if name.startswith("nlg_sens_apply"):
        b = sens_bytes(S, 4 if "all" in name else 2, "all" in name)
        line += "   k_lns_sens: %.0f MB algorithmic, %.1f us at 8 TB/s, %.0f %% of the HBM peak" % (b / 1e6, 1e6 * b / HBM_PEAK,
                                                                                                 100 * b / HBM_PEAK / (1e-6 * float(np.median(t))))
    lines.append(line)
lines.append("(the timed call includes the memsets that zero pressure and restart history of the outputs: %.0f MB written per output vector)"
             % (8e-6 * (npts * (3 * dim + 3 * ((n - 2) / n) ** dim) - npts * dim)))
lines.append("composed over kernel (grad only): %.1f" % (float(np.median(us["set_baseflow + compute_LNS_conv"])) / float(np.median(us["nlg_sens_apply, grad only"]))))
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
