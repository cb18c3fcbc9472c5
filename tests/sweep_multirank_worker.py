"""One rank of tests/test_gpu_sweep_multirank.py: wavenumber lanes (nlg_linop_set_projection_lanes) with the homogeneous direction
ACROSS the rank boundaries, as run_proj of tests/multirank_worker.py -- two lanes with different wavenumbers, projected together
(nlg_linop_project_block) and advanced together (one block matvec); the partial line sums of both lanes travel in ONE all-reduce.  Then the same block on the same handle after nlg_linop_set_projection: one wavenumber, one table, two lanes.
usage: sweep_multirank_worker.py rank world segment outdir mult"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neklab_amd import _lib, host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402

ALPHAS = (2.0, 1.0)


def run(rank, world, segment, outdir, mult):
    nel, n = (2, 2, 2 * mult), 6
    ctx = host.Context(0)
    if world > 1:
        ctx.comm_init_shm(rank, world, segment)
    gnel = (nel[0], nel[1], nel[2] * world)
    hm = box_mesh(gnel, n, lengths=(2.0, 2.0, 2.0 * np.pi), periodic=(True, False, True), deform=0.0,
                  last_range=(rank * nel[2], (rank + 1) * nel[2]))
    gm = host.Mesh(ctx, hm)
    bf = host.nek_dvector(gm)
    bf.set_field(0, hm.mask[0] * (hm.y * (2.0 - hm.y)))
    A = host.exptA_linop(0.03, bf, re=40.0, dt=0.01, vtol=1e-13, ptol=1e-13, maxit_p=2000)
    A.init()

    def name(*coords):      # a global name for the line through a point: its coordinates across the line, hashed
        k = [np.round(np.asarray(c).ravel() / 1e-7).astype(np.int64) for c in coords]
        return np.ascontiguousarray(k[0] * 40000003 + k[1], dtype=np.int64)

    X2 = host.pressure_mesh_coords(gm)
    lab, lab2, z2 = name(hm.x, hm.y), name(X2[0], X2[1]), np.ascontiguousarray(X2[2], dtype=np.float64)
    al = np.array(ALPHAS)
    host.check(gm.lib.nlg_linop_set_projection_lanes(A.h, len(ALPHAS), _lib.dptr(al), 3, lab.ctypes.data_as(_lib.c_int64_p),
                                                      lab2.ctypes.data_as(_lib.c_int64_p), _lib.dptr(z2)))
    s = len(ALPHAS)
    v = [host.nek_dvector(gm) for _ in range(s)]
    for l in range(s):
        v[l].rand(True, seed=21 + l)
        v[l].set_field(host.PR, (np.cos(X2[2]) + np.cos(2.0 * X2[2])) * X2[1])     # the same for both lanes: each keeps its own wavenumber
    pv = [x.copy() for x in v]
    arr = (_lib.vp * s)(*[x.h for x in pv])
    host.check(gm.lib.nlg_linop_project_block(A.h, s, arr))
    out = [host.nek_dvector(gm) for _ in range(s)]
    A.matvec_block(v, out)
    fields = {"scal": np.array([q for l in range(s) for q in (v[l].norm(), pv[l].norm(), out[l].norm(), out[l].dot(pv[l]))]),
              "stats": np.array([A.stats()["p_iters"], A.stats()["v_iters"]], dtype=float)}
    for l in range(s):
        for i in range(3):
            fields["out%d_%d" % (l, i)] = out[l].get_field(i)
            fields["pv%d_%d" % (l, i)] = pv[l].get_field(i)
            fields["v%d_%d" % (l, i)] = v[l].get_field(i)
        fields["outp%d" % l] = out[l].get_field(host.PR)
        fields["pvp%d" % l] = pv[l].get_field(host.PR)
    # one wavenumber for all lanes on the same handle: the block still shares ONE all-reduce, every lane reading the one table
    host.check(gm.lib.nlg_linop_set_projection(A.h, ALPHAS[1], 3, lab.ctypes.data_as(_lib.c_int64_p), lab2.ctypes.data_as(_lib.c_int64_p),
                                                _lib.dptr(z2)))
    one = [host.nek_dvector(gm) for _ in range(s)]
    A.matvec_block(v, one)
    for l in range(s):
        for i in range(3):
            fields["one%d_%d" % (l, i)] = one[l].get_field(i)
        fields["onep%d" % l] = one[l].get_field(host.PR)
    np.savez(os.path.join(outdir, "sweep_w%d_r%d.npz" % (world, rank)), **fields)
    ctx.sync()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]))
    print("WORKER_OK")
