#!/usr/bin/env python3
"""Drag, lift, torque and the wall distributions of the reference's cylinder base flow (Re = 50, tests/golden/reference_cyl_baseflow.npz)
with host.wall_forces.

The field file's pressure lives on the velocity mesh: pressure_from_mesh1 carries it to the Gauss points, as Nek5000's restart does.
The 16 faces of the cylinder are the 'W' faces of the boundary list whose element touches r < 0.6.  With U = 1, D = 1, rho = 1:
Cd = 2 Fx, Cl = 2 Fy, F = Fp + Fv.  Per wall point, to the text file: the angle theta (degrees, 0 = rear stagnation point, from the
centre), Cp = 2 p_q (the pressure level is the file's) and Cf = 2 tau_t, tau_t the viscous traction along the tangent (-n_y, n_x) per
unit area.  Reads nothing outside the repository.

usage: cylinder_forces.py [--out cylinder_cp_cf.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="cylinder_cp_cf.txt")
args = ap.parse_args()

import refdata  # noqa: E402
from neklab_amd import host  # noqa: E402
from neklab_amd.nekio import face_nodes  # noqa: E402

hm, ux, uy, p, re, lxd, _ = refdata.load_cylinder(with_bcs=True)
d = np.load(os.path.join(ROOT, "tests", "golden", "reference_cyl_baseflow.npz"))
pos = {int(g): k for k, g in enumerate(d["elmap"])}                      # global element id of the mesh file -> position in the field file
bcs = list(zip(d["bc_elem"], d["bc_face"], d["bc_tag"]))
faces = [(pos[e + 1], f) for e, f in host.faces_from_bcs(bcs, tags=("W",))]
faces = [(e, f) for e, f in faces if np.hypot(hm.x[e], hm.y[e]).min() < 0.6]

ctx = host.Context(0)
gm = host.Mesh(ctx, hm, lxd=lxd)
X = host.nek_dvector(gm)
X.set_field(0, ux), X.set_field(1, uy)
X.set_field(host.PR, host.pressure_from_mesh1(gm, p))
nu = 1.0 / re
wf = host.wall_forces(gm, [faces])
S = wf.parts(wf.sample(X, nu)[0])
F = S["Fp"] + S["Fv"]
print("Re = %g, %d faces, area %.9f (pi = %.9f)" % (re, len(faces), wf.area[0], np.pi))
print("Cd = %.6f = %.6f (pressure) + %.6f (viscous); Cl = %.3e; torque = %.3e" % (2 * F[0], 2 * S["Fp"][0], 2 * S["Fv"][0], 2 * F[1], S["Tp"][0] + S["Tv"][0]))
t = wf.tractions(X, nu)
rows = []
for q, (e, f) in enumerate(faces):
    nodes = face_nodes(hm.n, 2, f)
    ds = np.linalg.norm(t["nds"][q], axis=-1)
    nrm = t["nds"][q] / ds[:, None]
    tv = (t["trac"][q] - t["p"][q][:, None] * t["nds"][q]) / ds[:, None]
    tau = -tv[:, 0] * nrm[:, 1] + tv[:, 1] * nrm[:, 0]
    th = np.degrees(np.arctan2(hm.y[e, nodes], hm.x[e, nodes]))
    rows += list(zip(th, 2.0 * t["p"][q], 2.0 * tau))
rows.sort()
with open(args.out, "w") as fh:
    fh.write("# theta [deg]        Cp              Cf\n")
    for r in rows:
        fh.write("%12.6f %15.8e %15.8e\n" % r)
print("%d wall points written to %s; Cp at the front stagnation point %.4f" % (len(rows), args.out, max(r[1] for r in rows)))
wf.close()
