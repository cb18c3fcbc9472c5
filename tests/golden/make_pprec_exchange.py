#!/usr/bin/env python3
"""Generates tests/golden/pprec_exchange.npz: the overlapping Schwarz preconditioner (nlg_op_pprec, overlap = 1) applied to
seeded pressure fields on the meshes of tests/test_gpu_pprec_exchange.py, with and without the coarse level.

Needs the GPU.  The fixture pins the data protocol of the ghost layers: it was made with the build that summed the two
copies of every face slot by pairs-only gather-scatters, and the build that writes every ghost value straight into its
consumer's slot must agree with it to rounding.  Run from the repo root:
    python tests/golden/make_pprec_exchange.py [output.npz]
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
SEEDS = (11,)


def inputs(gm, seed):
    return np.random.default_rng(seed).standard_normal(gm.lpn)


def apply(ctx, gm, r, with_coarse):
    vin, vout = host.nek_dvector(gm), host.nek_dvector(gm)
    vin.set_field(host.PR, r)
    host.check(ctx.lib.nlg_op_pprec(gm.h, vin.h, vout.h, 1, with_coarse))
    return vout.get_field(host.PR).copy()


def main(out):
    ctx = host.Context(0)
    data = {}
    for name, kw in CASES.items():
        gm = host.Mesh(ctx, box_mesh(kw["nel"], kw["n"], periodic=kw["periodic"], deform=kw["deform"]))
        for seed in SEEDS:
            r = inputs(gm, seed)
            for wc in (0, 1):
                data["%s_s%d_c%d" % (name, seed, wc)] = apply(ctx, gm, r, wc)
    np.savez_compressed(out, **data)
    print("wrote", out, len(data), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pprec_exchange.npz"))
