#!/usr/bin/env python3
"""Generates tests/golden/pprec_exchange.npz (3-D) and pprec_exchange_2d.npz (2-D): the overlapping Schwarz preconditioner
(nlg_op_pprec, overlap = 1) applied to seeded pressure fields on the meshes of tests/test_gpu_pprec_exchange.py, with and
without the coarse level.

Needs the GPU.  The fixtures pin the data protocol of the ghost layers: they were made with the build that summed the two
copies of every face slot by pairs-only gather-scatters (3-D before 9a52353, 2-D before its own change), and the build that
writes every ghost value straight into its consumer's slot must agree with them to rounding.  Run from the repo root:
    python tests/golden/make_pprec_exchange.py {3d|2d} [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

# a deformed box with walls (faces without a neighbour) and a periodic box with two elements in y and z (two faces of one
# element share their neighbour), at the MFMA size lx1 = 8 and the two-waves-per-element size lx1 = 10
CASES = {
    "wall_n8": dict(nel=(4, 3, 3), n=8, periodic=(False, False, False), deform=0.05),
    "per_n8": dict(nel=(3, 2, 2), n=8, periodic=(True, True, True), deform=0.05),
    "wall_n10": dict(nel=(3, 3, 2), n=10, periodic=(False, False, False), deform=0.05),
    "per_n10": dict(nel=(3, 2, 2), n=10, periodic=(True, True, True), deform=0.05),
}
# 2-D: walls at lx1 = 6, a fully periodic box with two elements in y at lx1 = 8, and a row one element wide and periodic in y
# (the two y faces of every element are neighbours of each other)
CASES_2D = {
    "wall2_n6": dict(nel=(4, 3), n=6, periodic=(False, False), deform=0.05),
    "per2_n8": dict(nel=(3, 2), n=8, periodic=(True, True), deform=0.05),
    "self2_n6": dict(nel=(3, 1), n=6, periodic=(False, True), deform=0.05),
}
FIXTURES = {"3d": (CASES, "pprec_exchange.npz"), "2d": (CASES_2D, "pprec_exchange_2d.npz")}
SEEDS = (11,)


def inputs(gm, seed):
    return np.random.default_rng(seed).standard_normal(gm.lpn)


def apply(ctx, gm, r, with_coarse):
    vin, vout = host.nek_dvector(gm), host.nek_dvector(gm)
    vin.set_field(host.PR, r)
    host.check(ctx.lib.nlg_op_pprec(gm.h, vin.h, vout.h, 1, with_coarse))
    return vout.get_field(host.PR).copy()


def main(which, out):
    ctx = host.Context(0)
    data = {}
    for name, kw in FIXTURES[which][0].items():
        gm = host.Mesh(ctx, box_mesh(kw["nel"], kw["n"], periodic=kw["periodic"], deform=kw["deform"]))
        for seed in SEEDS:
            r = inputs(gm, seed)
            for wc in (0, 1):
                data["%s_s%d_c%d" % (name, seed, wc)] = apply(ctx, gm, r, wc)
    np.savez_compressed(out, **data)
    print("wrote", out, len(data), "arrays")


if __name__ == "__main__":
    which = sys.argv[1]
    main(which, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", FIXTURES[which][1]))
