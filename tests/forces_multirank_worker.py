"""One rank of tests/test_gpu_forces_multirank.py: `world` processes share one GPU through the shared-memory validation transport
(nlg_ctx_comm_init_shm) and hold contiguous element blocks of case B (tests/floquet_ref.py).  Every rank passes the same global face
list (forces_ref.case_objects: object 1 has no face on the first rank's elements), samples a fixed random vector and runs 3 steps of
the DNS with the forces attached.
usage: forces_multirank_worker.py rank world segment outdir"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import floquet_ref as fr  # noqa: E402
import forces_ref as fo  # noqa: E402
from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import partition_elements  # noqa: E402

NSTEPS = 3
NU = 0.37


def random_fields(sem):
    rng = np.random.default_rng(23)
    return [rng.standard_normal(sem.shape1) for _ in range(3)], rng.standard_normal(sem.shape2)


def run(rank, world, segment, outdir):
    hm, sem = fr.case_mesh("B")
    mine = partition_elements(hm.E, world)[rank]
    ctx = host.Context(0)
    if world > 1:
        ctx.comm_init_shm(rank, world, segment)
    gm = host.Mesh(ctx, hm.take(mine))
    objects = fo.case_objects("B", hm)
    wf = host.wall_forces(gm, objects)
    vel, pr = random_fields(sem)
    gv = host.nek_dvector(gm)
    for i in range(3):
        gv.set_field(i, vel[i][mine])
    gv.set_field(host.PR, pr[mine])
    sample = wf.sample(gv, NU)
    X0 = fr.orbit_state("B")
    gX0 = host.nek_dvector(gm)
    for i in range(3):
        gX0.set_field(i, X0.v[i][mine])
    kw = {k: v for k, v in fr.case_cfg("B").items() if k != "tau"}
    dns = host.nek_dns(gX0, pprecond=1, pproj=0, chunk=2, **kw)
    dns.set_wall_forces(wf)
    dns.advance(NSTEPS)
    s = dns.series()
    np.savez(os.path.join(outdir, "forces_w%d_r%d.npz" % (world, rank)), sample=sample, area=wf.area, nlocal=len(wf.local), force=s["force"],
             time=s["time"], per_object=np.array([sum(1 for q in wf.local if sum(len(o) for o in objects[:k]) <= q < sum(len(o) for o in objects[:k + 1]))
                                                  for k in range(len(objects))]))
    dns.close()
    wf.close()
    ctx.sync()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4])
    print("WORKER_OK")
