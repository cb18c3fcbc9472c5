"""One rank of tests/test_gpu_dns_multirank.py: `world` processes share one GPU through the shared-memory validation transport
(nlg_ctx_comm_init_shm) and run the DNS of case B (tests/floquet_ref.py) on contiguous element blocks, with history points on the
partition interfaces among the points.
usage: dns_multirank_worker.py rank world segment outdir"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dns_ref  # noqa: E402
import floquet_ref as fr  # noqa: E402
from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import partition_elements  # noqa: E402

NSTEPS = 3


def run(rank, world, segment, outdir):
    hm, sem = fr.case_mesh("B")
    mine = partition_elements(hm.E, world)[rank]
    ctx = host.Context(0)
    if world > 1:
        ctx.comm_init_shm(rank, world, segment)
    gm = host.Mesh(ctx, hm.take(mine))
    X0 = fr.orbit_state("B")
    gX0, one = host.nek_dvector(gm), host.nek_dvector(gm)
    for i in range(3):
        gX0.set_field(i, X0.v[i][mine])
    one.set_field(0, np.ones((len(mine), hm.n ** 3)))
    xyz = np.array([p[1] for p in dns_ref.case_points("B", hm) if p[2] == 0])
    hp = host.history_points(gm, xyz)
    kw = {k: v for k, v in fr.case_cfg("B").items() if k != "tau"}
    dns = host.nek_dns(gX0, pprecond=1, pproj=0, chunk=2, **kw)
    dns.set_history_points(hp)
    dns.set_reference()
    dns.advance(NSTEPS)
    s = dns.series()
    np.savez(os.path.join(outdir, "dns_w%d_r%d.npz" % (world, rank)), time=s["time"], probe=s["probe"], dist=s["dist"],
             ones=hp.sample(one)[:, 0], elem=hp.elem, status=hp.status, rst=hp.rst, umax=max(np.abs(a).max() for a in X0.v), unorm=X0.norm())
    dns.close()
    hp.close()
    ctx.sync()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4])
    print("WORKER_OK")
