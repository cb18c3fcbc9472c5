#!/usr/bin/env python3
"""What one application of the strong-form operator L costs ("The operator L itself").

E = 25 x 20 x 20 = 10^4 elements, lx1 = 8: microseconds per nlg_lns_apply for s = 1 and s = 4 vectors, direct and adjoint, as
  apply_L            (1, -1, -1): the masked copy, the weak convective term (sem_conv_apply) and k_lns_strong, and
  without convection (1,  0, -1): k_lns_strong alone (one launch),
the second against the algorithmic bytes of that kernel at the HBM peak of 8 TB/s, and the s = 4 to 4 x (s = 1) ratio.  The vectors
are consecutive columns of a KrylovBasis, so the lanes are a stride apart and are read and written in place.  Host clock around
`--reps` calls that end in a device synchronise, after a warm-up of every shape; the variants alternate over `--rounds` rounds.

usage: lns_cost.py [--rounds R] [--reps K] [--nel a,b,c] [--lx1 n] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--nel", default="25,20,20")
ap.add_argument("--lx1", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lns_cost.txt"))
args = ap.parse_args()
nel = tuple(int(a) for a in args.nel.split(","))
n = args.lx1
dim = len(nel)
E = int(np.prod(nel))
npts = E * n ** dim
HBM_PEAK = 8.0e12      # bytes per second (MI355X)


def strong_bytes(s, conv):
    """bytes one launch of k_lns_strong has to move: per lane u, out, p (and the weak convective term), once per element the
    dim^2 rst, jac and the masks (and bm1)"""
    lane = 8 * dim + 8 * dim + 8 * ((n - 2) / n) ** dim + (8 * dim if conv else 0)
    shared = 8 * dim * dim + 8 + 8 * dim + (8 if conv else 0)
    return npts * (s * lane + shared)


from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ctx = host.Context(0)
hm = box_mesh(nel, n, deform=0.05)
gm = host.Mesh(ctx, hm)
bf = host.nek_dvector(gm)
coords = (hm.x, hm.y, hm.z) if dim == 3 else (hm.x, hm.y)
ph = [2 * np.pi * c / L for c, L in zip(coords, hm.lengths)]
U = [np.sin(ph[1]) * np.cos(ph[-1]), 0.5 * np.sin(ph[-1]) * np.cos(ph[0]), 0.5 * np.sin(ph[0]) * np.cos(ph[1])][:dim]
for i in range(dim):
    bf.set_field(i, U[i] * hm.mask[i])
L = host.lns_linop(bf, 100.0)
Bi, Bo = host.KrylovBasis(gm, 4), host.KrylovBasis(gm, 4)
for v in range(4):
    Bi[v].rand(True, seed=10 + v)
vin, vout = [Bi[v] for v in range(4)], [Bo[v] for v in range(4)]
variants = [(name, s, trans, coef) for name, coef in (("apply_L", (1.0, -1.0, -1.0)), ("no convection", (1.0, 0.0, -1.0)))
            for s in (1, 4) for trans in (False, True)]
for name, s, trans, coef in variants:      # warm-up of every shape
    L.apply(vin[:s], vout[:s], trans, coef)
ctx.sync()
us = {v[:3]: [] for v in variants}
for r in range(args.rounds):
    for name, s, trans, coef in variants:
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            L.apply(vin[:s], vout[:s], trans, coef)
        ctx.sync()
        us[(name, s, trans)].append(1e6 * (time.perf_counter() - t0) / args.reps)
lines = ["E = %d, lx1 = %d, %d-D, %d rounds of %d calls; microseconds per nlg_lns_apply, median (min .. max)" % (E, n, dim, args.rounds, args.reps)]
med = {}
for name, s, trans, coef in variants:
    t = us[(name, s, trans)]
    med[(name, s, trans)] = float(np.median(t))
    line = "%-14s s = %d %-7s %9.1f (%.1f .. %.1f)" % (name, s, "adjoint" if trans else "direct", med[(name, s, trans)], min(t), max(t))
    if name == "no convection":
        b = strong_bytes(s, False)
        line += "   k_lns_strong: %.0f MB algorithmic, %.1f us at 8 TB/s, %.0f %% of the HBM peak" % (b / 1e6, 1e6 * b / HBM_PEAK,
                                                                                                   100 * b / HBM_PEAK / (1e-6 * med[(name, s, trans)]))
    lines.append(line)
for name in ("apply_L", "no convection"):
    for trans in (False, True):
        lines.append("%-14s %-7s s = 4 over 4 x (s = 1): %.3f" % (name, "adjoint" if trans else "direct", med[(name, 4, trans)] / (4 * med[(name, 1, trans)])))
lines.append("k_lns_strong with the convective term: %.0f MB (s = 1), %.0f MB (s = 4) algorithmic" % (strong_bytes(1, True) / 1e6, strong_bytes(4, True) / 1e6))
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
