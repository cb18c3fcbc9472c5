#!/usr/bin/env python3
"""What the wall-force monitor of a DNS run costs per time step.

Two cases, each with two nek_dns runs from the same state with the same fixed dt, past their start-up, both with history points and the
recurrence norm attached, one of them with wall forces as well:
  box      : the headline mesh of bench.py, E = 25 x 20 x 20 = 10^4 elements, lx1 = 8, walls all round: faces_from_mask gives the
             2 (25 20 + 25 20 + 20 20) = 2800 wall faces, in three objects (one per pair of walls);
  cylinder : the reference's cylinder mesh and Re = 50 base flow (tests/golden/reference_cyl_baseflow.npz): 1996 elements, lx1 = 6,
             the 16 faces of the cylinder in one object.
Rounds alternate between the two runs on the same device in the same process; per run: milliseconds per time step (median and spread
over the rounds), kernel launches and collective sites per time step (nlg_counters).  The monitor adds two launches per step:
k_wall_forces reads the velocity, the pressure and the precomputed geometry of the elements that own a face, k_wall_forces_reduce the
faces' partial sums.  --profile N: only the run with forces, N steps, for a kernel trace.

usage: forces_cost.py [--rounds R] [--steps K] [--cases box,cylinder] [--profile N]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--cases", default="box,cylinder")
ap.add_argument("--profile", type=int, default=0)
args = ap.parse_args()
K = args.steps

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ctx = host.Context(0)


def counters():
    a, b = C.c_int64(0), C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


def box_case():
    hm = box_mesh((25, 20, 20), 8, deform=0.05)
    gm = host.Mesh(ctx, hm)
    X0 = host.nek_dvector(gm)
    ph = [2 * np.pi * c / L for c, L in zip((hm.x, hm.y, hm.z), hm.lengths)]
    U = [np.sin(ph[1]) * np.cos(ph[2]), 0.5 * np.sin(ph[2]) * np.cos(ph[0]), 0.5 * np.sin(ph[0]) * np.cos(ph[1])]
    for i in range(3):
        X0.set_field(i, U[i] * hm.mask[i])
    faces = host.faces_from_mask(hm)
    objects = [[ef for ef in faces if ef[1] in pair] for pair in ((2, 4), (1, 3), (5, 6))]
    xyz = np.random.default_rng(1).uniform(0.02, 0.98, (5, 3)) * np.array(hm.lengths)
    kw = dict(re=100.0, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=0.002)
    return "box: E = %d, lx1 = 8" % hm.E, gm, X0, objects, xyz, kw


def cylinder_case():
    import refdata
    hm, ux, uy, p, re, lxd, _ = refdata.load_cylinder(with_bcs=True)
    d = np.load(os.path.join(ROOT, "tests", "golden", "reference_cyl_baseflow.npz"))
    pos = {int(g): k for k, g in enumerate(d["elmap"])}
    faces = [(pos[int(e)], int(f)) for e, f, t in zip(d["bc_elem"], d["bc_face"], d["bc_tag"]) if str(t) == "W"]
    faces = [(e, f) for e, f in faces if np.hypot(hm.x[e], hm.y[e]).min() < 0.6]
    gm = host.Mesh(ctx, hm, lxd=lxd)
    X0 = host.nek_dvector(gm)
    X0.set_field(0, ux), X0.set_field(1, uy)
    X0.set_field(host.PR, host.pressure_from_mesh1(gm, p))
    xyz = np.array([[1.0, 0.0], [2.0, 0.5], [5.0, 0.0], [3.0, -0.5], [10.0, 0.2]])
    kw = dict(re=re, torder=3, vtol=1e-9, ptol=1e-7, maxit_v=200, maxit_p=4000, dt=0.002)
    return "cylinder: E = %d, lx1 = %d, Re = %g" % (hm.E, hm.n, re), gm, X0, [faces], xyz, kw


for case in args.cases.split(","):
    title, gm, X0, objects, xyz, kw = {"box": box_case, "cylinder": cylinder_case}[case]()
    t0 = time.perf_counter()
    wf = host.wall_forces(gm, objects)
    t_geo = time.perf_counter() - t0
    hp = host.history_points(gm, xyz)
    nfaces = sum(len(o) for o in objects)
    runs = {}
    for name in (("forces",) if args.profile else ("forces", "plain")):
        d = host.nek_dns(X0, **kw)
        d.set_history_points(hp)
        d.set_reference()
        if name == "forces":
            d.set_wall_forces(wf)
        d.advance(4)
        ctx.sync()
        runs[name] = d
    if args.profile:
        runs["forces"].advance(args.profile)
        ctx.sync()
        print("%s: %d faces in %d objects, %d steps with forces for the trace" % (title, nfaces, len(objects), args.profile), flush=True)
    else:
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
        f = runs["forces"].series()["force"]
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print("%s: %d faces in %d objects (geometry in %.3f s on the host), %d steps per timed call, %d rounds alternating: with forces %.3f ms/step "
              "[%.3f .. %.3f], without %.3f ms/step [%.3f .. %.3f]; difference of the medians %+.3f ms = %+.2f %%; launches/step %.1f vs %.1f, "
              "collectives/step %.1f vs %.1f; %d samples, last Fp + Fv of object 0: %s"
              % (title, nfaces, len(objects), t_geo, K, args.rounds, med["forces"], min(ms["forces"]), max(ms["forces"]), med["plain"], min(ms["plain"]),
                 max(ms["plain"]), med["forces"] - med["plain"], 100.0 * (med["forces"] - med["plain"]) / med["plain"], cnt["forces"][0],
                 cnt["plain"][0], cnt["forces"][1], cnt["plain"][1], f.shape[0],
                 np.array2string(f[-1, 0, :gm.dim] + f[-1, 0, gm.dim:2 * gm.dim], precision=6)), flush=True)
    for d in runs.values():
        d.close()
    hp.close(), wf.close()
