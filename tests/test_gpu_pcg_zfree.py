"""The velocity PCG without a stored z (csrc/lns.hip CGProblem::z_free): k_cg_init / k_cg_update keep z = M^-1 r in registers for their sums
and the Helmholtz kernel forms it again -- from the residual, 1 / diag and the point's mask byte, the same product -- while it updates the
search direction (csrc/sem.hip k_axhelm3r / k_axhelm3c, pcinv / pcmb).  Same operands, same operations: a matvec gives the same BITS as with
NLG_PCG_STORE_Z=1, which stores z and loads it back.  The switch is read when the operator is initialised, hence one fresh process per run."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, %r)
from neklab_amd import host
from neklab_amd.mesh import box_mesh
shape = sys.argv[1]
dim = 2 if shape == "2d" else 3
n = {"n10": 10, "n12": 12, "2d": 7}.get(shape, 8)
nel = (3, 2) if dim == 2 else ((2, 2, 2) if n == 8 else (2, 2, 1))
hm = box_mesh(nel, n, periodic=(True,) + (False,) * (dim - 1), deform=0.05)   # walls in y (and z): the masks are not trivial
ctx = host.Context(0); gm = host.Mesh(ctx, hm)
gb = host.nek_dvector(gm)
gb.set_field(0, hm.mask[0] * (1.0 + 0.5 * np.sin(hm.x) * np.cos(hm.y))); gb.set_field(1, hm.mask[1] * 0.3 * np.sin(2 * hm.x))
A = host.exptA_linop(0.02, gb, re=40.0, dt=0.01, torder=3, vtol=1e-12, ptol=1e-11, maxit_v=400, maxit_p=4000); A.init()   # two time steps, tolerance mode
print("ZFREE", A.info()["pcg_z_free"])
if len(sys.argv) > 2 and sys.argv[2] == "path":
    sys.exit(0)
s = 2 if shape == "block" else 1
vin = []
for v in range(s):
    x = host.nek_dvector(gm); x.rand(True, seed=40 + v); x.scal(10.0 ** (-3 * v)); vin.append(x)
out = [host.nek_dvector(gm) for _ in range(s)]
if s > 1: A.matvec_block(vin, out)
elif shape == "adjoint": A.rmatvec(vin[0], out[0])
else: A.matvec(vin[0], out[0])
st = A.stats()
words = []
for w in out:
    for irst in range(w.nrst + 1):     # the vector itself and its history blocks
        for f in list(range(dim)) + [host.PR]:
            words.append(hashlib.sha256(np.ascontiguousarray(w.get_field(f, irst)).tobytes()).hexdigest()[:24])
print("RESULT", st["steps"], st["v_iters"], st["p_iters"], " ".join(words))
''' % ROOT


def run_child(shape, env_extra, path_only=False):
    env = dict(os.environ)
    for k in ("NLG_PCG_STORE_Z", "NLG_PCG_DEFER_X", "NLG_PCG_DEFER_XP", "NLG_PCG_SINGLE_RED", "NLG_PC_MASKB"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, shape] + (["path"] if path_only else []), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    zfree = int([x for x in lines if x.startswith("ZFREE")][-1].split()[1])
    res = [x for x in lines if x.startswith("RESULT")]
    return zfree, (res[-1].split()[1:] if res else None)


# lx1 = 8: k_axhelm3r; lx1 = 10, 12: k_axhelm3c (one and three pairs per block); two lanes: r at the lane stride, the preconditioner shared;
# no direction ring and a ring of three slots that wraps; the adjoint
@pytest.mark.parametrize("shape,extra", [("n8", {}), ("n10", {}), ("n12", {}), ("block", {}), ("n8", {"NLG_PCG_DEFER_X": "0"}),
                                         ("n8", {"NLG_PCG_DEFER_X": "3"}), ("adjoint", {})])
def test_matvec_bits_do_not_depend_on_where_z_is_formed(shape, extra):
    za, a = run_child(shape, extra)
    zb, b = run_child(shape, dict(extra, NLG_PCG_STORE_Z="1"))
    print(shape, extra, "z_free", za, zb, "steps / v_iters / p_iters", a[:3], b[:3])
    assert (za, zb) == (1, 0), "the two runs took the same path"
    steps, v_iters = int(a[0]), int(a[1])
    assert v_iters > 3 * steps, "the velocity solves are too short to wrap a ring of three directions: %s" % a[:3]
    assert a[1:3] == b[1:3], "iteration counts differ: %s / %s" % (a[:3], b[:3])
    assert len(a) > 3 + 4 and len(a) == len(b)      # more than one block of four fields: the history blocks are there
    assert a == b, "output fields differ: %s" % [i for i, (x, y) in enumerate(zip(a, b)) if x != y]


@pytest.mark.parametrize("shape,extra,expect", [("n8", {}, 1), ("n8", {"NLG_PCG_STORE_Z": "1"}, 0), ("2d", {}, 0),
                                                ("n8", {"NLG_PCG_SINGLE_RED": "1"}, 0)])
def test_path_taken(shape, extra, expect):
    zfree, _ = run_child(shape, extra, path_only=True)
    assert zfree == expect
