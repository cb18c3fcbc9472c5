"""The solver-only forms of the Helmholtz and pressure operators, ONE application each against the float64 reference of tests/pcg_step_ref.py:
nlg_op_helmholtz_pcg reproduces helm_apply (csrc/lns.hip: sem_axhelm with the fused direction update, the z-free form, the direction ring,
the slab-permuted layout, the first-stage sums, the done flags and 1 to 4 lanes, then the gated gather-scatter), nlg_op_cdabdtp_pcg
reproduces pres_apply (sem_cdabdtp with nlg_pupd, the sums, the gates, the multi-lane kernels and intermediates).  A converged PCG hides
what these parts can get wrong (a dropped partial sum, a beta or zmean of another lane, a wrong mask bit, a leaking gate: the fixed point
stays, the iteration count moves), and GPU-against-GPU tests share the code under test; one application amplifies nothing.

Bounds (none of them measured):
  direction  |got - ref| <= 4 * 2^-53 * (|z| + |zmean| + |beta p|) pointwise: three roundings, or two with a contraction to an FMA; z-free:
             z = fl(pc r) is rounded on its own (sem.hip k_axhelm3r), so the same form with |pc r|; masked points are exactly beta u
  operator   1e-13 (Helmholtz w, test_gpu_ops.py) and 1e-12 (E p, test_gpu_pop_mfma.py) of the reference's max norm
  sums       the operator bounds carried through the dot product: 1e-13 * sum |u'| |w_local| for a lane's Helmholtz sum,
             1e-12 * sum |p'| |out| and 1e-12 * sum |out| per block of the pressure sums
  done / ring / untouched entries: bit-identical to the sentinel, to the input, or to the run without the flag.
A lane with done != 0 keeps its INPUT in an in-place direction buffer (there is no other buffer to hold the sentinel); with the ring its
destination slot holds the sentinel."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pcg_step_ref as R
from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
SENT = -7.25
H1, H2 = 0.7, 3.0
MESHES3 = {
    "walls": ((2, 2, 1), (True, False, False)),     # E = 4: E * nf with nf = 1 leaves a tail block behind the three slots of k_axhelm3r
    "self": ((3, 1, 2), (False, True, False)),      # an element is its own neighbour
}
MESHES2 = {"4x3": ((4, 3), (True, False)), "3x2": ((3, 2), (True, False))}   # E is no multiple of the elements per block
PATTERNS = {"plain": dict(fused=0, zfree=0, ring=0), "fused": dict(fused=1, zfree=0, ring=0), "zfree": dict(fused=1, zfree=1, ring=0),
            "ring": dict(fused=1, zfree=1, ring=1)}
SWITCHES = ("NLG_POP_MFMA", "NLG_OPDIV_MASKB", "NLG_SMALL_E")

_setups = {}
_refs = {}


def setup(ctx, kind, n):
    """mesh, oracle and inputs of one (mesh, lx1), made once: four lanes of everything, beta and zmean different in every lane"""
    key = (kind, n)
    if key not in _setups:
        if kind == "sym":
            # the walls of box_mesh zero all three components alike, and then any bit of a mask byte serves for every component.  Here the
            # three masks differ: component 0 held on the z walls only, component 1 on the y and z walls, component 2 on the y walls only
            nel = (2, 2, 1)
            hm = box_mesh(nel, n, periodic=(True, False, False), deform=0.05)
            hm.mask[0] = box_mesh(nel, n, periodic=(True, True, False), deform=0.05).mask[0]
            hm.mask[2] = box_mesh(nel, n, periodic=(True, False, True), deform=0.05).mask[2]
            assert not same(hm.mask[0], hm.mask[1]) and not same(hm.mask[1], hm.mask[2]) and not same(hm.mask[0], hm.mask[2])
        elif kind == "star":
            # irregular valence (tests/starmesh.py): edges shared by 3 and 5 elements, vertices by 6 and 10, neighbours turned against
            # one another; used by test_gpu_starmesh.py
            from starmesh import star_mesh
            hm = star_mesh(5, n, 2)
            nel = hm.nel
        else:
            nel, per = (MESHES3 if kind in MESHES3 else MESHES2)[kind]
            hm = box_mesh(nel, n, periodic=per, deform=0.05)
        sem = SEM(hm)
        gm = host.Mesh(ctx, hm)
        rng = np.random.default_rng(1000 * n + len(nel) + sum(map(ord, kind)))
        dim, lvn, lpn = sem.dim, sem.lvn, sem.lpn
        d = dict(hm=hm, sem=sem, gm=gm, u=rng.standard_normal((4, dim, lvn)), zf=rng.standard_normal((4, dim, lvn)),
                 pcinv=rng.uniform(0.5, 1.5, lvn), p=rng.standard_normal((4, lpn)), z=rng.standard_normal((4, lpn)))
        for nm in ("beta", "zmean", "pbeta"):
            d[nm] = 0.3 + 0.35 * (rng.permutation(4) + rng.uniform(0.1, 0.9, 4))    # in [0.3, 1.7], one value per quarter: no two lanes alike
        _setups[key] = d
    return _setups[key]


def helm_ref(S, kind, n, pat, nf, v):
    key = ("h", kind, n, pat if pat != "ring" else "zfree", nf, v)
    if key not in _refs:
        f = PATTERNS[pat]
        u = [S["u"][v, c] for c in range(nf)]
        zf = [S["zf"][v, c] for c in range(nf)] if f["fused"] else None
        _refs[key] = R.helm_step(S["sem"], u, H1, H2, zf=zf, beta=S["beta"][v], pcinv=S["pcinv"] if f["zfree"] else None)
    return _refs[key]


def pres_ref(S, kind, n, fused, v):
    key = ("p", kind, n, fused, v)
    if key not in _refs:
        _refs[key] = R.pres_step(S["sem"], S["p"][v], S["z"][v] if fused else None, S["pbeta"][v], S["zmean"][v])
    return _refs[key]


def helm_blocks(sem, nf):
    if sem.dim == 2:
        epb = max(256 // (sem.n * sem.n), 1)
        return (sem.E + epb - 1) // epb
    slots = 3 if (sem.n <= 8 or sem.n == 12) else 1      # sem.hip: kAxhelm3rWaves, axhelm3c_ppb
    return (sem.E * nf + slots - 1) // slots


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def check_helm(S, kind, n, pat, nf, nl, xp, worst):
    """one call, its rerun with a done lane, all assertions; returns the result for the lane comparison"""
    sem, gm = S["sem"], S["gm"]
    f = PATTERNS[pat]
    u, zf = S["u"][:nl, :nf], S["zf"][:nl, :nf]
    kw = dict(zf=zf if f["fused"] else None, beta=S["beta"][:nl] if f["fused"] else None, pcinv=S["pcinv"] if f["zfree"] else None, xp=xp,
              sentinel=SENT, **f)
    res = gm.helmholtz_pcg(u, H1, H2, **kw)
    nb = helm_blocks(sem, nf)
    assert res["npart"] == nb, (res["npart"], nb)
    tag = "%s n=%d %s nf=%d nl=%d xp=%d" % (kind, n, pat, nf, nl, xp)
    for v in range(nl):
        ref = helm_ref(S, kind, n, pat, nf, v)
        for c in range(nf):
            got = res["u_out"][v, c]
            if not f["fused"]:
                assert same(got, u[v, c]), tag + ": the plain application changed u"
            else:
                bound = 4 * EPS * (np.abs(ref["z"][c]) + np.abs(ref["bu"][c])).ravel()
                err = np.abs(got - ref["u"][c].ravel())
                assert np.all(err <= bound), (tag, v, c, float(np.max(err - bound)))
                worst["dir"] = max(worst["dir"], float(np.max(err / np.maximum(bound, 1e-300))))
                if f["zfree"]:
                    m0 = sem.mask[c].ravel() == 0.0
                    assert same(got[m0], (S["beta"][v] * u[v, c])[m0]), tag + ": a masked point is not exactly beta u"
            assert same(res["u_src"][v, c], got if not f["ring"] else u[v, c]), tag + ": the source buffer of the direction"
            wref = ref["w"][c].ravel()
            e = float(np.max(np.abs(res["w"][v, c] - wref)) / np.max(np.abs(wref)))
            worst["w"] = max(worst["w"], e / 1e-13)
            assert e <= 1e-13, (tag, v, c, e)
        part = res["part"][v]
        assert np.all(part[nb:] == SENT) and not np.any(part[:nb] == SENT), tag + ": the partial sums written"
        e = abs(math.fsum(part[:nb].tolist()) - ref["pw"])
        worst["pw"] = max(worst["pw"], e / (1e-13 * ref["pw_abs"]))
        assert e <= 1e-13 * ref["pw_abs"], (tag, v, e, ref["pw_abs"])
    if nl > 1:
        vd = 1 if nl >= 3 else nl - 1
        done = np.zeros(nl)
        done[vd] = 1.0
        r2 = gm.helmholtz_pcg(u, H1, H2, done=done, **kw)
        for v in range(nl):
            if v == vd:
                assert np.all(r2["u_out"][v] == SENT) if f["ring"] else same(r2["u_out"][v], u[v]), tag + ": a finished lane's direction"
                assert same(r2["u_src"][v], u[v])
                assert np.all(r2["w"][v] == SENT) and np.all(r2["part"][v] == SENT), tag + ": a finished lane was written"
            else:
                for k in ("u_out", "u_src", "w", "part"):
                    assert same(r2[k][v], res[k][v]), tag + ": lane %d changed with lane %d finished (%s)" % (v, vd, k)
    return res


def run_helm(S, kind, n, pat, nfs, nls, xps):
    for nf in nfs:
        for xp in xps:
            worst = dict(dir=0.0, w=0.0, pw=0.0)
            single = {}
            for nl in nls:
                res = check_helm(S, kind, n, pat, nf, nl, xp, worst)
                if nl == 1:
                    single[0] = res
                    continue
                ident = []
                for v in range(nl):     # (printed, not asserted) is lane v of the nl-lane call the one-lane call on the same data, bit for bit?
                    if v not in single:
                        f = PATTERNS[pat]
                        single[v] = S["gm"].helmholtz_pcg(S["u"][v:v + 1, :nf], H1, H2, zf=S["zf"][v:v + 1, :nf] if f["fused"] else None,
                                                          beta=S["beta"][v:v + 1] if f["fused"] else None,
                                                          pcinv=S["pcinv"] if f["zfree"] else None, xp=xp, sentinel=SENT, **f)
                    ident.append(int(all(same(res[k][v], single[v][k][0]) for k in ("u_out", "w", "part"))))
                print("PCGSTEP-LANES helm %s n=%d %s nf=%d nl=%d xp=%d lanes bit-identical to one-lane calls: %s" % (kind, n, pat, nf, nl, xp, ident))
            kern = "k_axhelm2<%d,%d>" % (n, nf) if S["sem"].dim == 2 else "k_axhelm3%s<%d,%s>" % ("r" if n <= 8 else "c", n, "true" if xp else "false")
            print("PCGSTEP helm %s %s %s nf=%d: fraction of the bound: direction %.3f w %.3f pw %.3f" % (kern, kind, pat, nf, worst["dir"], worst["w"], worst["pw"]))


@pytest.mark.parametrize("pat", list(PATTERNS))
@pytest.mark.parametrize("kind", list(MESHES3))
@pytest.mark.parametrize("n", [5, 7, 8, 9, 10, 12])
def test_helmholtz_3d(gpu_ctx, n, kind, pat):
    run_helm(setup(gpu_ctx, kind, n), kind, n, pat, (1, 3), (1, 3, 4), (0, 1))


@pytest.mark.parametrize("pat", ["zfree", "ring"])
@pytest.mark.parametrize("n", [5, 7, 8, 9, 10, 12])
def test_helmholtz_3d_component_masks(gpu_ctx, n, pat):
    """bit c of the mask byte, not any bit: a mesh whose three Dirichlet masks differ (with bit 0 for every component this test fails)"""
    run_helm(setup(gpu_ctx, "sym", n), "sym", n, pat, (1, 3), (1, 3), (0, 1))


@pytest.mark.parametrize("pat", ["plain", "fused"])
@pytest.mark.parametrize("kind", list(MESHES2))
@pytest.mark.parametrize("n", [6, 8])
def test_helmholtz_2d(gpu_ctx, n, kind, pat):
    run_helm(setup(gpu_ctx, kind, n), kind, n, pat, (1, 2), (1, 3), (0,))


def test_helmholtz_refusals(gpu_ctx):
    """combinations the solver never makes are errors, not other paths"""
    S2, S3 = setup(gpu_ctx, "3x2", 6), setup(gpu_ctx, "walls", 5)
    u2, u3 = S2["u"][:1], S3["u"][:1]
    for S, u, kw in ((S2, u2, dict(fused=1, zfree=1, pcinv=S2["pcinv"])), (S2, u2, dict(fused=1, xp=1)), (S3, u3, dict(fused=0, ring=1)),
                     (S3, u3, dict(fused=0, zfree=1, pcinv=S3["pcinv"])), (S3, u3[:, :2], dict(fused=0))):
        with pytest.raises(host.NlgError):
            S["gm"].helmholtz_pcg(u, H1, H2, zf=u if kw.get("fused") else None, beta=np.ones(1) if kw.get("fused") else None, **kw)


# ---- pressure ---------------------------------------------------------------------------------------------------------------------

def block_sums(sem, a):
    """the reference's element sums gathered into the blocks of the divergence kernel: one element in 3-D, 256 / lx1^2 elements in 2-D"""
    epb = 1 if sem.dim == 3 else max(256 // (sem.n * sem.n), 1)
    return np.array([math.fsum(a[b:b + epb].tolist()) for b in range(0, sem.E, epb)])


def check_pres(S, kind, n, nl, fused, ring, worst):
    sem, gm = S["sem"], S["gm"]
    p, z = S["p"][:nl], S["z"][:nl]
    kw = dict(z=z if fused else None, beta=S["pbeta"][:nl] if fused else None, zmean=S["zmean"][:nl] if fused else None, fused=fused, ring=ring,
              sentinel=SENT)
    res = gm.cdabdtp_pcg(p, **kw)
    tag = "%s n=%d nl=%d fused=%d ring=%d" % (kind, n, nl, fused, ring)
    nb = len(block_sums(sem, np.zeros(sem.E)))
    assert res["npart"] == nb, (res["npart"], nb)
    for v in range(nl):
        ref = pres_ref(S, kind, n, fused, v)
        got = res["p_out"][v]
        if not fused:
            assert same(got, p[v]), tag + ": p changed without the update"
        else:
            bound = 4 * EPS * (np.abs(z[v]) + abs(S["zmean"][v]) + np.abs(S["pbeta"][v] * p[v]))
            err = np.abs(got - ref["p"].ravel())
            assert np.all(err <= bound), (tag, v, float(np.max(err - bound)))
            worst["dir"] = max(worst["dir"], float(np.max(err / bound)))
        assert same(res["p_src"][v], p[v] if ring else got), tag + ": the source buffer of the direction"   # ring = 0: updated in place
        oref = ref["out"].ravel()
        e = float(np.max(np.abs(res["out"][v] - oref)) / np.max(np.abs(oref)))
        worst["out"] = max(worst["out"], e / 1e-12)
        assert e <= 1e-12, (tag, v, e)
        part = res["part"][v]
        assert np.all(part[2 * nb:] == SENT) and not np.any(part[:2 * nb] == SENT), tag + ": the partial sums written"
        for half, key in ((0, "a"), (1, "b")):
            want, bnd = block_sums(sem, ref[key]), 1e-12 * block_sums(sem, ref[key + "_abs"])
            err = np.abs(part[half * nb:(half + 1) * nb] - want)
            worst[key] = max(worst[key], float(np.max(err / bnd)))
            assert np.all(err <= bnd), (tag, v, key, err, bnd)
    if nl > 1:
        vd = 1 if nl >= 3 else nl - 1
        done = np.zeros(nl)
        done[vd] = 1.0
        r2 = gm.cdabdtp_pcg(p, done=done, **kw)
        for v in range(nl):
            if v == vd:
                assert np.all(r2["p_out"][v] == SENT) if ring else same(r2["p_out"][v], p[v]), tag + ": a finished lane's direction"
                assert same(r2["p_src"][v], p[v])
                assert np.all(r2["out"][v] == SENT) and np.all(r2["part"][v] == SENT), tag + ": a finished lane was written"
            else:
                for k in ("p_out", "p_src", "out", "part"):
                    assert same(r2[k][v], res[k][v]), tag + ": lane %d changed with lane %d finished (%s)" % (v, vd, k)
    return res


def run_pres(S, kind, n, nls, forms):
    gm = S["gm"]
    for fused, ring in forms:
        worst = dict(dir=0.0, out=0.0, a=0.0, b=0.0)
        single = {}
        for nl in nls:
            res = check_pres(S, kind, n, nl, fused, ring, worst)
            if nl == 1:
                single[0] = res
                continue
            ident = []
            for v in range(nl):
                if v not in single:
                    single[v] = gm.cdabdtp_pcg(S["p"][v:v + 1], z=S["z"][v:v + 1] if fused else None, beta=S["pbeta"][v:v + 1] if fused else None,
                                               zmean=S["zmean"][v:v + 1] if fused else None, fused=fused, ring=ring, sentinel=SENT)
                ident.append(int(all(same(res[k][v], single[v][k][0]) for k in ("p_out", "out", "part"))))
            print("PCGSTEP-LANES pres %s n=%d fused=%d ring=%d nl=%d lanes bit-identical to one-lane calls: %s" % (kind, n, fused, ring, nl, ident))
        print("PCGSTEP pres lx1=%d dim=%d pop_mfma=%d %s fused=%d ring=%d nl=%s: fraction of the bound: direction %.3f out %.3f part[e] %.3f part[E+e] %.3f"
              % (n, S["sem"].dim, gm.pop_mfma(), kind, fused, ring, list(nls), worst["dir"], worst["out"], worst["a"], worst["b"]))


ALL_FORMS = ((0, 0), (1, 0), (1, 1))


@pytest.mark.parametrize("kind", list(MESHES3))
@pytest.mark.parametrize("n", [5, 7, 12, 8, 9, 10])
def test_pressure_3d(gpu_ctx, n, kind):
    S = setup(gpu_ctx, kind, n)
    fuses = n in (8, 9, 10)
    run_pres(S, kind, n, (1, 2, 4), ALL_FORMS if fuses else ((0, 0),))
    with pytest.raises(host.NlgError):       # the solver keeps a ring only where the gradient kernel performs the update
        S["gm"].cdabdtp_pcg(S["p"][:1], fused=0, ring=1)
    if not fuses:
        with pytest.raises(host.NlgError):
            S["gm"].cdabdtp_pcg(S["p"][:1], z=S["z"][:1], beta=np.ones(1), zmean=np.ones(1), fused=1)


@pytest.mark.parametrize("kind", list(MESHES2))
@pytest.mark.parametrize("n", [6, 8])
def test_pressure_2d(gpu_ctx, n, kind):
    run_pres(setup(gpu_ctx, kind, n), kind, n, (1, 2, 4), ((0, 0),))


# lx1 = 8 with one lane has three paths, chosen by switches the library reads once per process: one fresh process per setting, one after
# the other, each with a time limit; the first that fails stops the test
CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
import test_gpu_pcg_step as T
nls = tuple(int(a) for a in sys.argv[1].split(","))
ctx = host.Context(0)
pops = {}
for kind in T.MESHES3:
    S = T.setup(ctx, kind, 8)
    pops[kind] = S["gm"].pop_mfma()
    T.run_pres(S, kind, 8, nls, T.ALL_FORMS)
print("CHILD OK " + json.dumps(pops))
''' % dict(root=ROOT, here=os.path.dirname(os.path.abspath(__file__)))

SETTINGS = {
    "default": ({}, 0, "1"),                                           # a small mesh: k_opgradt3w / k_opdiv3w
    "mfma": ({"NLG_SMALL_E": "0"}, 1, "1"),                            # k_opgradt3m8 / k_opdiv3m8
    "vector": ({"NLG_SMALL_E": "0", "NLG_POP_MFMA": "0"}, 0, "1"),     # k_opgradt3n / k_opdiv3n, ML = false
    "maskb0": ({"NLG_SMALL_E": "0", "NLG_OPDIV_MASKB": "0"}, 1, "1,2,4"),   # the three weight arrays instead of the mask bytes
}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_pressure_lx8_paths(setting):
    extra, pop, nls = SETTINGS[setting]
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([sys.executable, "-c", CHILD, nls], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    pops = json.loads(r.stdout.split("CHILD OK ", 1)[1].splitlines()[0])
    assert all(v == pop for v in pops.values()), (setting, pops)      # which path ran
