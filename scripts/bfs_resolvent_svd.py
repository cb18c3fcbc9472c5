#!/usr/bin/env python3
"""Block resolvent on the reference's resolvent case, examples/back_fstep/gramian (bfs.usr:8 declares `nsv = 4, kdim = 512` next to
resolvent_linop and never uses them): the four leading gains of R(omega) by host.resolvent_analysis, whose four test forcings are
the lanes of block applications, and what one block application (s = 4) costs against four single ones.  Mesh, boundary tags and
base flow come from the committed fixture (tests/golden/reference_bfs_baseflow.npz), the solver settings from bfs.par as in
bfs_resolvent_gramian.py (bdf2, Re = 600, tolerances 1e-8 / 1e-6, the case's explicit filter).  The same comparison is made first on
the small 2-D box of tests/test_gpu_resolvent_block.py (3 x 3 elements, lx1 = 6, omega = 8, Re = 20), block and singles in alternation.

usage: bfs_resolvent_svd.py [--power-iters q, default 1] [--rounds n, default 3: alternations on the box; 0: gains only, on both meshes]
       [--no-box] [--no-bfs] [omega ..., default 0.8]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from neklab_amd import host  # noqa: E402
from neklab_amd.mesh import box_mesh  # noqa: E402


def take(flag, default):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def random_forcings(gm, k, seed=1):
    out = []
    for i in range(k):
        z = host.nek_zvector(gm)
        z.rand(seed + i)
        out.append(z)
    return out


def block_against_singles(R, Omega, rounds, tag):
    """One block application of len(Omega) lanes against as many single applications, `rounds` times in alternation."""
    gm, s = R.mesh, len(Omega)
    outs = [host.nek_zvector(gm) for _ in range(s)]
    print("# %s: seconds, GMRES matvecs (block: %d per block step), time steps (lane steps / lanes for the block)" % (tag, s))
    ratios = []
    for r in range(rounds):
        n0 = R.gmres_matvecs
        t0 = time.time()
        R.matvec_block(Omega, outs)
        tb = time.time() - t0
        nb, stb = R.gmres_matvecs - n0, R.last_operator.stats()["steps"] // s
        ts, ns, sts = 0.0, 0, 0
        for v in range(s):
            n0 = R.gmres_matvecs
            t0 = time.time()
            R.matvec(Omega[v], outs[v])
            ts += time.time() - t0
            ns += R.gmres_matvecs - n0
            sts += R.last_operator.stats()["steps"]
        ratios.append(ts / tb)
        print("%s round %d: block of %d  %.2f s  %d matvecs = %d block steps  %d time steps | %d singles  %.2f s  %d matvecs  %d time steps | singles / block = %.2f"
              % (tag, r + 1, s, tb, nb, nb // s, stb, s, ts, ns, sts, ts / tb), flush=True)
    return ratios


power_iters = take("--power-iters", 1)
rounds = take("--rounds", 3)
with_bfs, with_box = "--no-bfs" not in sys.argv, "--no-box" not in sys.argv
omegas = [float(a) for a in sys.argv[1:] if not a.startswith("--")] or [0.8]
ctx = host.Context(0)

# ---- the test box
if with_box:
    hm = box_mesh((3, 3), 6, lengths=(2.0, 1.0), periodic=(True, False), deform=0.03)
    gm = host.Mesh(ctx, hm)
    gb = host.nek_dvector(gm)
    gb.set_field(host.VX, hm.mask[0] * (4 * hm.y * (1 - hm.y)))
    R = host.resolvent_linop(8.0, gb, re=20.0, torder=3, vtol=1e-12, ptol=1e-12, maxit_v=400, maxit_p=4000)
    print("test box: E = %d lx1 = %d, omega = 8, Re = 20, bdf3, tolerances 1e-12, GMRES rtol 1e-6" % (hm.E, hm.n), flush=True)
    if rounds > 0:
        block_against_singles(R, random_forcings(gm, 4), rounds, "box")
    t0 = time.time()
    sigma, U, V = host.resolvent_analysis(R, 4, power_iters=power_iters, seed=1)
    print("box: gains (nsv = 4, %d power iteration(s), %d block applications, %.2f s): %s" % (power_iters, 2 * power_iters + 2, time.time() - t0, " ".join("%.6e" % s for s in sigma)), flush=True)

# ---- the reference's case
if with_bfs:
    from refdata import load_bfs
    hm, ux, uy, p, re, lxd, _ = load_bfs(with_bcs=True)
    gm = host.Mesh(ctx, hm, lxd=lxd)
    bf = host.nek_dvector(gm)
    bf.set_field(host.VX, ux)
    bf.set_field(host.VY, uy)
    filt = dict(filter_weight=0.01, filter_modes=host.filter_modes_from_cutoff_ratio(hm.n, 0.84))
    print("BFS: E = %d lx1 = %d, Re = %g, bdf2, tolerances 1e-8 / 1e-6, filter %s, GMRES rtol 1e-6" % (hm.E, hm.n, re, filt), flush=True)
    for omega in omegas:
        R = host.resolvent_linop(omega, bf, re=re, torder=2, vtol=1e-8, ptol=1e-6, maxit_v=400, maxit_p=4000, **filt)
        if rounds > 0:
            block_against_singles(R, random_forcings(gm, 4), 1, "BFS omega = %.1f" % omega)
        t0 = time.time()
        sigma, U, V = host.resolvent_analysis(R, 4, power_iters=power_iters, seed=1)
        print("BFS omega = %.1f: gains (nsv = 4, %d power iteration(s), %d block applications, %.1f s): %s"
              % (omega, power_iters, 2 * power_iters + 2, time.time() - t0, " ".join("%.6e" % s for s in sigma)), flush=True)
