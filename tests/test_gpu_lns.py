"""The strong-form LNS operator on the GPU (nlg_lns_*, nlg_op_lns; host.lns_linop, apply_L and its pieces, nek_otd.matvec) against
tests/lns_ref.py.

Meshes: the nine shapes of tests/test_gpu_ops.py (deform = 0.05), random fields.  Tolerance: 1e-12 x max|reference of that same
quantity|, the convention of the convection check there; on the CPU a one-ulp perturbation of the inputs moves the result by <= 7e-16
of scale at every one of these shapes.  Stated per term, so that a term lost under a larger one still fails its own check.
"""
import ctypes as C

import numpy as np
import pytest

import floquet_ref as fr
import lns_ref
import otd_ref
from neklab_amd import host
from neklab_amd._lib import dptr, vp
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

CASES = [
    dict(nel=(4, 3), n=6, periodic=(True, False)),
    dict(nel=(3, 4), n=8, periodic=(False, False)),
    dict(nel=(3, 2, 2), n=6, periodic=(True, False, False)),
    dict(nel=(3, 3, 2), n=8, periodic=(False, False, True)),
    dict(nel=(2, 2, 2), n=5, periodic=(False, False, False)),
    dict(nel=(2, 2, 2), n=10, periodic=(False, False, True)),
    dict(nel=(2, 1, 2), n=12, periodic=(False, False, False)),
    dict(nel=(2, 2, 2), n=9, periodic=(True, False, False)),
    dict(nel=(2, 2, 2), n=7, periodic=(False, True, False)),
]
IDS = ["x".join(map(str, c["nel"])) + "_n%d" % c["n"] for c in CASES]
RE = 37.0
TOL = 1e-12
_host = {}


def host_case(i):
    """mesh, oracle, base flow and four input vectors of case i, drawn once"""
    if i not in _host:
        c = CASES[i]
        hm = box_mesh(c["nel"], c["n"], periodic=c["periodic"], deform=0.05)
        sem = SEM(hm)
        rng = np.random.default_rng(100 + i)
        vecs = []
        for _ in range(5):
            ov = NekDVector(sem, 0)
            for k in range(sem.dim):
                ov.v[k][...] = rng.standard_normal(sem.shape1)
            ov.pr[...] = rng.standard_normal(sem.shape2)
            vecs.append(ov)
        _host[i] = (hm, sem, vecs[0], vecs[1:], {})
    return _host[i]


def ref_terms(i, lane, adjoint):
    hm, sem, base, ins, memo = host_case(i)
    key = (lane, bool(adjoint))
    if key not in memo:
        memo[key] = lns_ref.lns_terms(sem, base.v, ins[lane].v, ins[lane].pr, adjoint=bool(adjoint))
    return memo[key]


def combine(terms, coef, re=RE):
    lap, N, gp = terms
    return [coef[0] / re * lap[k] + coef[1] * N[k] + coef[2] * gp[k] for k in range(len(lap))]


def upload(gm, ov):
    gv = host.nek_dvector(gm)
    for k in range(gm.dim):
        gv.set_field(k, ov.v[k])
    gv.set_field(host.PR, ov.pr)
    return gv


def vel(gv):
    return [gv.get_field(k) for k in range(gv.mesh.dim)]


def err_scale(got, ref):
    scale = max(np.abs(r).max() for r in ref)
    return max(np.abs(g - r.ravel()).max() for g, r in zip(got, ref)), scale


def fill(gv, value):
    for k in range(gv.mesh.dim):
        gv.set_field(k, np.full(gv.mesh.lvn, value))
    gv.set_field(host.PR, np.full(gv.mesh.lpn, value))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the five routines, direct and adjoint, at every shape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_terms_and_both_directions(gpu_ctx, i):
    hm, sem, base, ins, _ = host_case(i)
    gm = host.Mesh(gpu_ctx, hm)
    L = host.lns_linop(upload(gm, base), RE)
    gin, out, out2 = upload(gm, ins[0]), host.nek_dvector(gm), host.nek_dvector(gm)
    worst = 0.0
    for adj in (False, True):
        terms = ref_terms(i, 0, adj)
        for name, coef in lns_ref.ROUTINES.items():
            fill(out, 7.0)
            L.apply(gin, out, trans=adj, coef=coef)
            err, scale = err_scale(vel(out), combine(terms, coef))
            print("%s %s %s: scale %.3e, error / scale %.3e" % (IDS[i], name, "adjoint" if adj else "direct", scale, err / scale))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, adj)
            assert not out.get_field(host.PR).any()
            # the routine under the reference's name is the same call
            fn = getattr(host, name)
            fill(out2, -3.0)
            if name in ("compute_LNS_laplacian", "compute_LNS_gradp"):
                if adj:
                    continue
                fn(L, gin, out2)
            else:
                fn(L, gin, out2, adj)
            assert all(np.array_equal(a, b) for a, b in zip(vel(out), vel(out2))), name
    print("%s: largest error / scale %.3e" % (IDS[i], worst))
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the exact answer on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nel,n", [((2, 2), 5), ((2, 2, 2), 8)], ids=["2d", "3d"])
def test_exact_answer_on_polynomial_fields(gpu_ctx, nel, n):
    hm = box_mesh(nel, n, periodic=(False,) * len(nel), deform=0.0)
    for m in hm.mask:
        m[...] = 1.0   # unmasked
    sem = SEM(hm)
    U, u, p, exact = lns_ref.poly_fields(sem)
    gm = host.Mesh(gpu_ctx, hm)
    gU, gu, out = host.nek_dvector(gm), host.nek_dvector(gm), host.nek_dvector(gm)
    gU.zero()
    for k in range(sem.dim):
        gU.set_field(k, U[k])
        gu.set_field(k, u[k])
    gu.set_field(host.PR, p)
    L = host.lns_linop(gU, 40.0)
    for adj in (False, True):
        host.apply_L(L, gu, out, adj)
        err, scale = err_scale(vel(out), exact(40.0, lns_ref.APPLY_L, adj))
        print("exact %d-D %s: scale %.3g, absolute error %.3e" % (sem.dim, "adjoint" if adj else "direct", scale, err))
        assert err <= TOL * scale
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. lanes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [3, 5], ids=[IDS[3], IDS[5]])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("strided", [False, True], ids=["separate", "basis"])
def test_lanes(gpu_ctx, i, s, strided):
    """a different input per lane, every lane against the reference of its own input.  separate: vectors of their own (a stride for
    s <= 2, the workspace beyond); basis: consecutive vectors of a KrylovBasis, read and written in place.  No public call reaches the
    padding behind a field (and lvs = lvn at both shapes), so the guard sits on what follows the main block: restart level 1 of
    every out vector keeps its sentinel bitwise, and out's pressure is zero."""
    hm, sem, base, ins, _ = host_case(i)
    gm = host.Mesh(gpu_ctx, hm)
    L = host.lns_linop(upload(gm, base), RE)
    gins = [upload(gm, ins[v]) for v in range(s)]
    if strided:
        Bi, Bo = host.KrylovBasis(gm, s), host.KrylovBasis(gm, s)
        for v in range(s):
            Bi[v].assign(gins[v])
        gins, outs = [Bi[v] for v in range(s)], [Bo[v] for v in range(s)]
    else:
        outs = [host.nek_dvector(gm) for _ in range(s)]
    sentinel = host.nek_dvector(gm)
    fill(sentinel, 12345.678)
    for o in outs:
        fill(o, 1.0)
        o.save_rst(sentinel, 1)
    for adj in (False, True):
        L.matvec_block(gins, outs, trans=adj)
        for v in range(s):
            err, scale = err_scale(vel(outs[v]), combine(ref_terms(i, v, adj), lns_ref.APPLY_L))
            assert err <= TOL * scale, (v, adj, err / scale)
            assert not outs[v].get_field(host.PR).any()
            for k in list(range(sem.dim)) + [host.PR]:
                assert np.all(outs[v].get_field(k, 1) == 12345.678)
            # the inputs are not modified
            for k in range(sem.dim):
                assert np.array_equal(gins[v].get_field(k), ins[v].v[k].ravel())
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the mask is applied on read
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_mask_on_read(gpu_ctx, i):
    hm, sem, base, ins, _ = host_case(i)
    assert any((m == 0).any() for m in sem.mask)
    wall = [m == 0 for m in sem.mask]
    assert all(np.abs(ins[0].v[k][wall[k]]).min() > 0 for k in range(sem.dim))   # the input is non-zero on the walls
    gm = host.Mesh(gpu_ctx, hm)
    L = host.lns_linop(upload(gm, base), RE)
    gin, out = upload(gm, ins[0]), host.nek_dvector(gm)
    fill(out, 5.0)
    ones = [np.ones(sem.shape1)] * sem.dim
    for name, coef in (("apply_L", lns_ref.APPLY_L), ("compute_LNS_conv", lns_ref.CONV), ("compute_LNS_laplacian", lns_ref.LAPLACIAN)):
        L.apply(gin, out, coef=coef)
        ref = combine(ref_terms(i, 0, False), coef)
        unmasked = lns_ref.lns_strong(sem, base.v, ins[0].v, ins[0].pr, RE, coef, mask=ones)
        err, scale = err_scale(vel(out), ref)
        far, _ = err_scale(vel(out), unmasked)
        print("%s %s: error / scale %.3e, distance to the unmasked reference / scale %.3e" % (IDS[i], name, err / scale, far / scale))
        assert err <= TOL * scale and far > 1e-6 * scale
        assert any(np.abs(o.reshape(sem.shape1)[w]).max() > 0 for o, w in zip(vel(out), wall))   # the output is not masked
    for k in range(sem.dim):
        assert np.array_equal(gin.get_field(k), ins[0].v[k].ravel())
    assert np.array_equal(gin.get_field(host.PR), ins[0].pr.ravel())
    assert not out.get_field(host.PR).any()
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. state of the object, 6. no communication
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_state_and_counters(gpu_ctx, i):
    hm, sem, base, ins, _ = host_case(i)
    gm = host.Mesh(gpu_ctx, hm)
    lib = gm.lib
    gbase, gin = upload(gm, base), upload(gm, ins[0])
    a, b = host.nek_dvector(gm), host.nek_dvector(gm)
    L = host.lns_linop(gbase, RE)
    coef = np.array(lns_ref.APPLY_L)
    for adj in (0, 1):
        L.apply(gin, a, trans=bool(adj))
        host.check(lib.nlg_op_lns(gm.h, gbase.h, gin.h, b.h, RE, adj, dptr(coef)))
        assert all(np.array_equal(x, y) for x, y in zip(vel(a), vel(b)))
    # another base flow: a stale Ur / GU would give the result about `base`
    gV = upload(gm, ins[1])
    L.set_baseflow(gV)
    L.apply(gin, a)
    ref = lns_ref.lns_strong(sem, ins[1].v, ins[0].v, ins[0].pr, RE)
    err, scale = err_scale(vel(a), ref)
    stale, _ = err_scale(vel(a), combine(ref_terms(i, 0, False), lns_ref.APPLY_L))
    assert err <= TOL * scale and stale > 1e-3 * scale
    # another Reynolds number
    L.set_re(3.0)
    L.apply(gin, a)
    err, scale = err_scale(vel(a), lns_ref.lns_strong(sem, ins[1].v, ins[0].v, ins[0].pr, 3.0))
    assert err <= TOL * scale
    # no collective call
    n0, c0, n1, c1 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    host.check(lib.nlg_counters(C.byref(n0), C.byref(c0)))
    L.apply([gin, gV], [a, b], trans=True)
    host.check(lib.nlg_counters(C.byref(n1), C.byref(c1)))
    assert c1.value == c0.value and n1.value > n0.value
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(gpu_ctx):
    hm, sem, base, ins, _ = host_case(0)
    gm = host.Mesh(gpu_ctx, hm)
    hm2 = host_case(1)[0]
    gm2 = host.Mesh(gpu_ctx, hm2)
    lib = gm.lib
    gbase, gin, out = upload(gm, base), upload(gm, ins[0]), host.nek_dvector(gm)
    other = host.nek_dvector(gm2)
    other.zero()
    L = host.lns_linop(gbase, RE)
    good = np.array(lns_ref.APPLY_L)
    zero3 = np.zeros(3)
    fill(out, 2.5)

    def refused(rc, word):
        msg = lib.nlg_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
        for k in list(range(sem.dim)) + [host.PR]:
            assert np.all(out.get_field(k) == 2.5)

    def arr(*vs):
        return (vp * len(vs))(*[x.h for x in vs])

    # s outside 1..4
    refused(lib.nlg_lns_apply(L.h, 0, arr(gin), arr(out), 0, dptr(good)), "out of range")
    five_in, five_out = [upload(gm, ins[0]) for _ in range(4)] + [gin], [host.nek_dvector(gm) for _ in range(4)] + [out]
    refused(lib.nlg_lns_apply(L.h, 5, arr(*five_in), arr(*five_out), 0, dptr(good)), "out of range")
    # a vector on another mesh
    refused(lib.nlg_lns_apply(L.h, 1, arr(other), arr(out), 0, dptr(good)), "another mesh")
    refused(lib.nlg_lns_apply(L.h, 2, arr(gin, gin), arr(out, other), 0, dptr(good)), "another mesh")
    refused(lib.nlg_op_lns(gm.h, gbase.h, other.h, out.h, RE, 0, dptr(good)), "another mesh")
    # out aliasing an input or the base flow
    fill(gin, 2.5)
    refused(lib.nlg_lns_apply(L.h, 1, arr(gin), arr(gin), 0, dptr(good)), "aliases in[0]")
    refused(lib.nlg_lns_apply(L.h, 2, arr(five_in[0], out), arr(five_out[0], out), 0, dptr(good)), "aliases in[1]")
    fill(gbase, 2.5)
    refused(lib.nlg_lns_apply(L.h, 1, arr(gin), arr(gbase), 0, dptr(good)), "aliases the base flow")
    refused(lib.nlg_op_lns(gm.h, gbase.h, gin.h, gbase.h, RE, 0, dptr(good)), "aliases the base flow")
    refused(lib.nlg_op_lns(gm.h, gbase.h, out.h, out.h, RE, 0, dptr(good)), "aliases in")
    # all three coefficients zero
    refused(lib.nlg_lns_apply(L.h, 1, arr(gin), arr(out), 0, dptr(zero3)), "coefficients are zero")
    refused(lib.nlg_op_lns(gm.h, gbase.h, gin.h, out.h, RE, 0, dptr(zero3)), "coefficients are zero")
    # re <= 0
    refused(lib.nlg_lns_set_re(L.h, 0.0), "must be positive")
    refused(lib.nlg_op_lns(gm.h, gbase.h, gin.h, out.h, -1.0, 0, dptr(good)), "must be positive")
    h = vp()
    refused(lib.nlg_lns_create(gm.h, gbase.h, 0.0, C.byref(h)), "must be positive")
    with pytest.raises(host.NlgError):
        host.lns_linop(gbase, -5.0)
    # the object still works, at the Reynolds number it had
    L.apply(upload(gm, ins[0]), out)
    assert not np.all(out.get_field(0) == 2.5)
    L.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. nek_otd as a linear operator: matvec / rmatvec, reduced(form="strong")
# ---------------------------------------------------------------------------------------------------------------------
# (with solve_baseflow the base flow takes one of the four lanes: r = 3 is the largest basis nlg_otd_create accepts there)
@pytest.mark.parametrize("r,coupled", [(2, False), (4, False), (2, True), (3, True)])
def test_otd_matvec_and_strong_reduced(gpu_ctx, r, coupled):
    hm, sem = fr.case_mesh("A")
    gm = host.Mesh(gpu_ctx, hm)
    kw = fr.case_cfg("A")

    def up(ov):
        gv = host.nek_dvector(gm)
        for k in range(gm.dim):
            gv.set_field(k, ov.v[k])
        gv.set_field(host.PR, ov.pr)
        return gv

    def run():
        O = host.nek_otd(up(fr.orbit_state("A")), r, pprecond=1, pproj=0, **kw)
        O.init(host.otd_opts(solve_baseflow=coupled, orthostep=2), basis0=[up(b) for b in otd_ref.orthonormal_basis(sem, r)])
        O.advance(3)
        return O

    O = run()
    weak0, G0 = O.reduced()
    U = O.current_baseflow()
    Uv = [U.get_field(k).reshape(sem.shape1) for k in range(sem.dim)]
    if coupled:   # the base flow has moved
        assert max(np.abs(U.get_field(k) - O.baseflow.get_field(k)).max() for k in range(sem.dim)) > 1e-8
    out = host.nek_dvector(gm)
    for trans in (False, True):
        b = O.basis(r - 1)
        (O.rmatvec if trans else O.matvec)(b, out)
        bv = [b.get_field(k).reshape(sem.shape1) for k in range(sem.dim)]
        ref = lns_ref.lns_strong(sem, Uv, bv, b.get_field(host.PR).reshape(sem.shape2), kw["re"], adjoint=trans)
        err, scale = err_scale(vel(out), ref)
        print("OTD r=%d coupled=%s %s: error / scale %.3e" % (r, coupled, "rmatvec" if trans else "matvec", err / scale))
        assert err <= TOL * scale
    strong, G = O.reduced(form="strong")
    B = [O.basis(j) for j in range(r)]
    W = [host.nek_dvector(gm) for _ in range(r)]
    for j in range(r):
        O.matvec(B[j], W[j])
    ref = np.array([[B[i].dot(W[j]) for j in range(r)] for i in range(r)])
    assert np.abs(strong - ref).max() <= TOL * np.abs(ref).max()
    weak1, G1 = O.reduced()
    # Every reduced() orthonormalises the lanes again, which by itself moves Lr in its last bits (printed).  What the strong call
    # must not do is disturb the state any further: a twin run with a plain reduced() in its place -- the strong form makes exactly
    # one such call -- ends bitwise where this one does.
    T = run()
    t0, _ = T.reduced()
    T.reduced()
    t1, _ = T.reduced()
    T.close()
    print("OTD r=%d coupled=%s: reduced() after against before the strong call: %.3e of max|Lr|" % (r, coupled, np.abs(weak1 - weak0).max() / np.abs(weak0).max()))
    assert np.array_equal(t0, weak0) and np.array_equal(t1, weak1)
    assert np.abs(weak1 - weak0).max() <= 1e-13 * np.abs(weak0).max()
    print("OTD r=%d coupled=%s: max|Lr| %.3e, strong minus weak %.3e (relative %.3e)" % (r, coupled, np.abs(weak0).max(), np.abs(strong - weak0).max(),
                                                                                     np.abs(strong - weak0).max() / np.abs(weak0).max()))
    O.close()
