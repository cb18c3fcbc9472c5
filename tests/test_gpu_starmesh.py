"""The 3-D path on meshes of irregular valence (tests/starmesh.py; pinned on the CPU by test_cpu_starmesh.py): edges shared by 3, 5
and 9 elements, vertices by 6, 10 and 18, neighbours turned against one another.  Every other 3-D mesh of the suite is a structured
box (4 elements per edge, 8 per vertex), on which the gather-scatter never takes a second round of eight copies, never stores a tail,
and meets an odd number of pairs only by accident.

(a) the gather-scatter as the solvers call it (nlg_op_gs: sem_gs with fields, gates, layout, lanes and strides), against numpy:
    integers exactly in every layout; random data bit for bit in the natural layout (ascending local index, left to right: the order
    the comment above k_gs promises); in the face-grouped and slab-permuted layouts, where the tables order the members otherwise,
    all copies of a group alike and |out - s| <= (m - 1) 2^-53 sum |v_i| against the exact sum s of the group's m members (the
    bound of recursive summation in any order; s is evaluated in long double, whose own error is 2^-11 of that bound), and then bit
    for bit against the sum in ascending order of the layout's own index (the slot tables come from nlg_mesh_get);
    gates, repeatability, lane independence, refusals, and the arrays derived through it (vmult, binvm1).
(b) the operators of test_gpu_ops.py and (c) the preconditioner of test_gpu_pprec_oracle.py against the oracle, bounds unchanged.
(d) the solver forms of test_gpu_pcg_step.py, (e) the propagator as in test_gpu_n8.py, (f) the random start vector.
"""
import os
import sys
import tempfile

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd._lib import dptr
from oracle.lns import ExptA, LNSConfig
from oracle.pprec import SchwarzPrec
from oracle.sem import SEM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_gpu_n8 as t8  # noqa: E402
import test_gpu_ops as tops  # noqa: E402
import test_gpu_pcg_step as tpcg  # noqa: E402
import test_gpu_pprec_oracle as tpp  # noqa: E402
from starmesh import star_mesh  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SENT = -7.25
_host = {}
_dev = {}


def key_id(k):
    return "k%d_n%d_nz%d%s" % (k[0], k[1], k[2], "p" if len(k) > 3 and k[3] else "")


def host_case(key):
    """(mesh, oracle) of star_mesh(*key), made once"""
    if key not in _host:
        hm = star_mesh(*key)
        _host[key] = (hm, SEM(hm))
    return _host[key]


def dev_case(ctx, key):
    if key not in _dev:
        _dev[key] = host.Mesh(ctx, host_case(key)[0])
    return host_case(key) + (_dev[key],)


# ---- (a) the gather-scatter ----------------------------------------------------------------------------------------------------------
GS_MESHES = [(9, 5, 2, False), (5, 5, 3, True), (5, 8, 2, False), (5, 6, 0, False)]


class Groups:
    """the groups of a labelling, members in ascending local index"""

    def __init__(self, glo, pos=None):
        """pos: the index of every point in the layout whose order counts (None: the natural one)"""
        g = np.asarray(glo).ravel()
        self.order = np.argsort(g, kind="stable") if pos is None else np.lexsort((np.asarray(pos).ravel(), g))   # by label, then index
        gs = g[self.order]
        self.start = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
        self.size = np.diff(np.r_[self.start, len(g)])
        self.gid = np.repeat(np.arange(len(self.start)), self.size)   # group of order[i]

    def sums_in_order(self, v):
        """float64, left to right over ascending local index; broadcast back to the members"""
        v = np.asarray(v, dtype=np.float64).ravel()
        s = v[self.order[self.start]].copy()
        for j in range(1, int(self.size.max())):
            sel = self.size > j
            s[sel] = s[sel] + v[self.order[self.start[sel] + j]]
        out = np.empty_like(v)
        out[self.order] = s[self.gid]
        return out

    def sums_long(self, v):
        """(exact sum, sum of absolute values) per member in long double"""
        v = np.asarray(v, dtype=np.longdouble).ravel()
        s = np.add.reduceat(v[self.order], self.start)
        a = np.add.reduceat(np.abs(v[self.order]), self.start)
        so, ao = np.empty_like(v), np.empty_like(v)
        so[self.order], ao[self.order] = s[self.gid], a[self.gid]
        return so, ao

    def members_alike(self, v):
        v = np.asarray(v).ravel()
        return np.array_equal(v[self.order], v[self.order[self.start]][self.gid])

    def count(self):
        out = np.empty(len(self.order))
        out[self.order] = self.size[self.gid]
        return out


def layouts(dim):
    return (0, 1, 2) if dim == 3 else (0,)


@pytest.mark.parametrize("key", GS_MESHES, ids=key_id)
def test_gs_integers_exact(gpu_ctx, key):
    """a missing, doubled or foreign member in any class of group (pairs, the odd pair, quads, one and several rounds of eight)"""
    hm, sem, gm = dev_case(gpu_ctx, key)
    G = Groups(hm.glo_num)
    rng = np.random.default_rng(11)
    for nl in (1, 4):
        for nf in range(1, hm.dim + 1):
            u = rng.integers(-8, 9, size=(nl, nf, gm.lvn)).astype(np.float64)
            ref = np.stack([[G.sums_in_order(u[v, c]) for c in range(nf)] for v in range(nl)])
            for lay in layouts(hm.dim):
                got = gm.gs(u, layout=lay, sentinel=SENT)
                bad = np.argwhere(got != ref)
                assert bad.size == 0, "layout %d nf %d nl %d: %d wrong sums, first at %s: %r for %r" % (
                    lay, nf, nl, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("key", GS_MESHES, ids=key_id)
def test_gs_random_data(gpu_ctx, key):
    hm, sem, gm = dev_case(gpu_ctx, key)
    assert np.finfo(np.longdouble).nmant >= 63
    G = Groups(hm.glo_num)
    m1 = (G.count() - 1.0).astype(np.longdouble)
    # a layout's own index of every point: element * points + slot; its groups are summed in ascending order of THAT index
    Gl = {}
    for lay, nm in ((1, "slot_fg"), (2, "slot_xp")):
        if hm.dim == 3:
            slot = gm.get(nm, hm.npts).astype(np.int64)
            assert np.array_equal(np.sort(slot), np.arange(hm.npts)), nm + " is no permutation"
            Gl[lay] = Groups(hm.glo_num, np.arange(hm.E)[:, None] * hm.npts + slot[None, :])
    rng = np.random.default_rng(12)
    worst = 0.0
    for nl in (1, 4):
        for nf in range(1, hm.dim + 1):
            u = rng.standard_normal((nl, nf, gm.lvn)) * 10.0 ** rng.integers(-3, 4, size=(nl, nf, 1))
            # natural layout: bit for bit
            got = gm.gs(u, layout=0, sentinel=SENT)
            for v in range(nl):
                for c in range(nf):
                    assert np.array_equal(got[v, c], G.sums_in_order(u[v, c])), "natural layout nf %d nl %d lane %d field %d" % (nf, nl, v, c)
            for lay in layouts(hm.dim)[1:]:
                got = gm.gs(u, layout=lay, sentinel=SENT)
                for v in range(nl):
                    for c in range(nf):
                        assert G.members_alike(got[v, c]), "layout %d: the copies of a group differ" % lay
                        s, a = G.sums_long(u[v, c])
                        err, bound = np.abs(got[v, c].astype(np.longdouble) - s), m1 * np.longdouble(EPS) * a
                        assert np.all(err <= bound), "layout %d nf %d nl %d lane %d field %d: %.3e over the bound" % (
                            lay, nf, nl, v, c, float(np.max(err - bound)))
                        worst = max(worst, float(np.max(err[m1 > 0] / bound[m1 > 0])))
                        assert np.array_equal(got[v, c], Gl[lay].sums_in_order(u[v, c])), "layout %d: not the sum in ascending order of the layout's index" % lay
    print("STARMESH gs %s: worst fraction of the bound (m - 1) 2^-53 sum|v| in the permuted layouts: %.3f" % (key_id(key), worst))


@pytest.mark.parametrize("key", GS_MESHES, ids=key_id)
def test_gs_gates_repeatability_lanes(gpu_ctx, key):
    hm, sem, gm = dev_case(gpu_ctx, key)
    rng = np.random.default_rng(13)
    done = np.array([0.0, 1.0, 0.0, 2.5])
    for nf in range(1, hm.dim + 1):
        u = rng.standard_normal((4, nf, gm.lvn))
        for lay in layouts(hm.dim):
            tag = "layout %d nf %d" % (lay, nf)
            full = gm.gs(u, layout=lay, sentinel=SENT)
            assert np.array_equal(gm.gs(u, layout=lay, sentinel=SENT), full), tag + ": two runs differ"
            assert np.array_equal(gm.gs(u, layout=lay, done=np.zeros(4), sentinel=SENT), full), tag + ": open gates change the result"
            gated = gm.gs(u, layout=lay, done=done, sentinel=SENT)
            for v in range(4):
                assert np.array_equal(gated[v], u[v] if done[v] != 0.0 else full[v]), tag + ": lane %d under the gates %s" % (v, done)
                one = gm.gs(u[v:v + 1], layout=lay, sentinel=SENT)
                assert np.array_equal(one[0], full[v]), tag + ": lane %d of four differs from its own one-lane run" % v


def test_gs_refusals(gpu_ctx):
    """out keeps what the test put there"""
    for key in (GS_MESHES[2], GS_MESHES[3]):
        hm, sem, gm = dev_case(gpu_ctx, key)
        dim = hm.dim
        u = np.ones((5, 4, gm.lvn))
        out = np.full((5, 4, gm.lvn), 3.5)
        bad = [(0, 1, 0), (dim + 1, 1, 0), (1, 0, 0), (1, 5, 0), (1, 1, 3), (1, 1, -1)]
        if dim == 2:
            bad += [(1, 1, 1), (1, 1, 2), (2, 4, 1), (2, 4, 2), (3, 1, 0)]
        for nf, nl, lay in bad:
            rc = gm.lib.nlg_op_gs(gm.h, nf, nl, lay, dptr(u), None, SENT, dptr(out))
            assert rc != 0 and b"nlg_op_gs" in gm.lib.nlg_last_error(), (nf, nl, lay)
            assert np.all(out == 3.5), (nf, nl, lay)
        rc = gm.lib.nlg_op_gs(gm.h, 1, 1, 0, dptr(u), None, float("inf"), dptr(out))
        assert rc != 0 and np.all(out == 3.5)
        with pytest.raises(host.NlgError):
            gm.gs(u[:1, :dim], layout=7, out=out[:1, :dim])
        assert np.all(out == 3.5)


@pytest.mark.parametrize("key", GS_MESHES, ids=key_id)
def test_gs_derived_arrays(gpu_ctx, key):
    hm, sem, gm = dev_case(gpu_ctx, key)
    cnt = Groups(hm.glo_num).count()
    assert np.array_equal(gm.get("vmult"), 1.0 / cnt)
    assert tops.relerr(gm.get("binvm1"), sem.binvm1) < 1e-13


# ---- (b) the operators and (c) the preconditioner against the oracle -------------------------------------------------------------------
OPS_MESHES = [(5, 5, 2, False), (5, 8, 2, False), (5, 10, 2, False), (5, 6, 3, True), (5, 6, 0, False), (5, 8, 0, False)]


@pytest.mark.parametrize("key", OPS_MESHES, ids=key_id)
def test_geometry_and_operators(gpu_ctx, key):
    """the checks of test_gpu_ops.py::test_mesh_geometry and ::test_operators, their bounds unchanged"""
    hm, sem, gm = dev_case(gpu_ctx, key)
    tops.check_geometry(sem, gm)
    tops.check_operators(sem, gm)


@pytest.mark.parametrize("key", OPS_MESHES, ids=key_id)
def test_pprec_matches_oracle(gpu_ctx, key):
    """overlap off and on (ghost layers across 3- and 5-valent edges, overlap counts), coarse level off and on (vertices of valence
    6 and 10); bound 1e-12 as on the boxes"""
    err = tpp.check_against_oracle(gpu_ctx, host_case(key)[0], (0, 1))
    print("STARMESH pprec %s: %.2e = %.3f of the bound" % (key_id(key), err, err / 1e-12))


AGG_MAX = 16
AGG_MESHES = [(5, 8, 2, False), (5, 6, 0, False)]
_CHILD_AGG = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
from starmesh import star_mesh
from test_gpu_pprec_oracle import gpu_pprec
from test_gpu_starmesh import AGG_MESHES
ctx = host.Context(0)
out = {}
for i, key in enumerate(AGG_MESHES):
    gm = host.Mesh(ctx, star_mesh(*key))
    r = np.random.default_rng(3).standard_normal(gm.lpn)
    for ov in (0, 1):
        out["c%%d_o%%d" %% (i, ov)] = gpu_pprec(ctx, gm, r, ov, 1)
np.savez(%(out)r, **out)
print("CHILD OK")
'''


def test_pprec_aggregated_coarse_matches_oracle():
    """NLG_COARSE_EXACT_MAX below the vertex count (read at mesh set-up: a fresh process)"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "agg.npz")
        tpp.run_child(_CHILD_AGG % dict(root=ROOT, here=HERE, out=path), {"NLG_COARSE_EXACT_MAX": str(AGG_MAX)}, 300)
        got = dict(np.load(path))
    for i, key in enumerate(AGG_MESHES):
        sem = host_case(key)[1]
        r = np.random.default_rng(3).standard_normal(sem.lpn)
        for ov in (0, 1):
            P = SchwarzPrec(sem, overlap=ov, with_coarse=True, exact_max=AGG_MAX)
            assert P.na < P.nvert and not P.ambiguous, "%s does not test the aggregated mode" % key_id(key)
            err = tpp.relerr(got["c%d_o%d" % (i, ov)], P.apply(r))
            print("STARMESH pprec aggregated %s overlap %d: %.2e" % (key_id(key), ov, err))
            assert err <= 1e-12, "%s overlap %d: relative error %.3e" % (key_id(key), ov, err)


# ---- (d) the solver forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pat", ["plain", "zfree"])
def test_helmholtz_pcg_form(gpu_ctx, pat):
    """helm_apply in the slab-permuted layout, four lanes; bounds: the header of test_gpu_pcg_step.py"""
    S = tpcg.setup(gpu_ctx, "star", 8)
    worst = dict(dir=0.0, w=0.0, pw=0.0)
    tpcg.check_helm(S, "star", 8, pat, 3, 4, 1, worst)
    print("STARMESH helm_pcg star n=8 %s: fraction of the bound: direction %.3f w %.3f pw %.3f" % (pat, worst["dir"], worst["w"], worst["pw"]))


@pytest.mark.parametrize("fused", [0, 1])
def test_cdabdtp_pcg_form(gpu_ctx, fused):
    """pres_apply (face-grouped intermediates between turned neighbours), four lanes"""
    S = tpcg.setup(gpu_ctx, "star", 8)
    worst = dict(dir=0.0, out=0.0, a=0.0, b=0.0)
    tpcg.check_pres(S, "star", 8, 4, fused, 0, worst)
    print("STARMESH cdabdtp_pcg star n=8 fused=%d: fraction of the bound: direction %.3f out %.3f part[e] %.3f part[E+e] %.3f"
          % (fused, worst["dir"], worst["out"], worst["a"], worst["b"]))


# ---- (e) the propagator --------------------------------------------------------------------------------------------------------------
# Fixed iteration counts, Jacobi preconditioner: the iteration is the oracle's own.  At 30 / 200 iterations the pressure PCG is stopped
# in the middle of its convergence on this mesh (the Jacobi-preconditioned solve needs about 570 iterations per step to reach the
# rounding floor), where conjugate gradients have lost the orthogonality of their directions and amplify rounding: the float64 oracle
# given a start vector perturbed by one ulp moves by 4e-5, and it lies as far from its own evaluation in long double
# (tests/starmesh_longdouble.py, same float64 inputs) as the table below says.  1e-11 / 1e-10 cannot be met there by any float64
# code, the oracle included; the bounds at 30 / 200 are 4 times the oracle's measured distance from the long-double value.  At
# 30 / 50 iterations, before the loss of orthogonality, that distance is 5.2e-15 (velocity), 2.8e-14 (pressure), 4.4e-15 (history),
# and the bounds are the 1e-11 (first matvec and history) and 1e-10 (second) of test_gpu_n8.py.
PKEY = (5, 8, 2, False)
PKW = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
FIXED = {50: dict(fixed_iters_v=30, fixed_iters_p=50), 200: dict(fixed_iters_v=30, fixed_iters_p=200)}
# measured: float64 oracle against long double at 30 / 200, (velocity, pressure, history) of the first matvec, (velocity, pressure) of the
# second, chained one (each run chains its own first result)
LD200 = {False: ((1.570e-04, 1.130e-02, 1.923e-05), (3.482e-06, 2.916e-05)), True: ((1.384e-04, 1.056e-02, 2.272e-05), (4.592e-06, 3.754e-05))}
_prop = {}


def fixed_bounds(iters, adjoint):
    """((velocity, pressure, history) of the first matvec, (velocity, pressure) of the second)"""
    if iters == 50:
        return (1e-11, 1e-10, 1e-11), (1e-10, 1e-9)       # test_gpu_n8.py: cmp_vec allows the pressure ten times the velocity's bound
    return tuple(tuple(4.0 * d for d in part) for part in LD200[adjoint])


def prop_oracle(fixed, adjoint, second):
    """(operator, start vector, first result, chained second result or None), once per mode; fixed: 0 (tolerance mode), 50 or 200"""
    key = (fixed, adjoint)
    hm, sem = host_case(PKEY)
    if key not in _prop:
        kw = dict(PKW, **(FIXED[fixed] if fixed else {}))
        oA = ExptA(sem, t8.base_flow(sem), LNSConfig(**kw))
        ov = t8.start_vector(sem)
        o1 = oA.matvec(ov, adjoint=adjoint)
        _prop[key] = [oA, kw, ov, o1, None]
    c = _prop[key]
    if second and c[4] is None:
        c[4] = c[0].matvec(c[3], adjoint=adjoint)
    return c


def prop_gpu(ctx, kw, pprecond, pproj):
    hm, sem, gm = dev_case(ctx, PKEY)
    gb = host.nek_dvector(gm)
    for i, u in enumerate(t8.base_flow(sem)):
        gb.set_field(i, u)
    gA = host.exptA_linop(kw["tau"], gb, pprecond=pprecond, pproj=pproj, **{k: v for k, v in kw.items() if k != "tau"})
    gA.init()
    return gm, gA


def vec_errors(get, nrst, o):
    """(velocity, pressure, history) errors of a result against the oracle's, scaled as test_gpu_n8.py::cmp_vec scales them"""
    sc = max(np.abs(a).max() for a in o.v)
    ev = max(np.abs(get(i, 0) - o.v[i].ravel()).max() for i in range(3)) / sc
    ep = np.abs(get(host.PR, 0) - o.pr.ravel()).max() / max(np.abs(o.pr).max(), sc)
    eh = max(np.abs(get(i, r) - o.v_rst[r - 1][i].ravel()).max() / np.abs(o.v[i]).max() for r in range(1, nrst + 1) for i in range(3)) if nrst else 0.0
    return float(ev), float(ep), float(eh)


def check_fixed(tag, iters, adjoint, e1, e2):
    b1, b2 = fixed_bounds(iters, adjoint)
    print("STARMESH %s 30/%d %s: matvec velocity %.2e pressure %.2e history %.2e (fractions of the bounds %.3f %.3f %.3f), matvec2 %.2e %.2e (%.3f %.3f)"
          % ((tag, iters, "adjoint" if adjoint else "direct") + e1 + tuple(e / b for e, b in zip(e1, b1)) + e2[:2] + tuple(e / b for e, b in zip(e2, b2))))
    assert all(e < b for e, b in zip(e1, b1)), ("matvec", e1, b1)
    assert all(e < b for e, b in zip(e2, b2)), ("matvec2", e2, b2)


def cmp_history(g1, o1, tol):
    assert g1.nrst == o1.nrst == 2
    for r in (1, 2):
        for i in range(3):
            assert np.max(np.abs(g1.get_field(i, r) - o1.v_rst[r - 1][i].ravel())) < tol * np.abs(o1.v[i]).max(), (r, i)


@pytest.mark.parametrize("adjoint", [False, True], ids=["direct", "adjoint"])
@pytest.mark.parametrize("iters", [50, 200])
def test_matvec_fixed_iterations(gpu_ctx, iters, adjoint):
    """iters = 50 is the case that pins the propagator on this mesh: 1e-11 / 1e-10 with an oracle that is within 5e-15 of long double.
    iters = 200 is the issue's count; its bounds (4 x LD200, up to 4.5e-2 on the pressure) only say that the device is no further from
    the oracle than the oracle is from the exact iterate.  test_cpu_starmesh.py runs tests/starmesh_longdouble.py at 50 iterations, so
    the script that produced LD200 keeps working when the oracle changes; LD200 itself is re-measured by hand (python
    tests/starmesh_longdouble.py 200, half a minute)."""
    oA, kw, ov, o1, o2 = prop_oracle(iters, adjoint, True)
    gm, gA = prop_gpu(gpu_ctx, kw, 1, 0)
    info = gA.info()
    assert info["nsteps"] == oA.nsteps and abs(info["dt"] - oA.dt) < 1e-15
    gv, g1, g2 = t8.upload(gm, ov), host.nek_dvector(gm), host.nek_dvector(gm)
    mv = gA.rmatvec if adjoint else gA.matvec
    mv(gv, g1)
    assert g1.nrst == o1.nrst == 2
    mv(g1, g2)                          # replays the restart history
    check_fixed("propagator", iters, adjoint, vec_errors(g1.get_field, 2, o1), vec_errors(g2.get_field, 0, o2))


@pytest.mark.parametrize("adjoint", [False, True], ids=["direct", "adjoint"])
@pytest.mark.parametrize("pprecond,pproj", [(0, 1), (1, 1)])
def test_matvec_tolerance_mode(gpu_ctx, adjoint, pprecond, pproj):
    oA, kw, ov, o1, _ = prop_oracle(0, adjoint, False)
    gm, gA = prop_gpu(gpu_ctx, kw, pprecond, pproj)
    gv, g1 = t8.upload(gm, ov), host.nek_dvector(gm)
    (gA.rmatvec if adjoint else gA.matvec)(gv, g1)
    t8.cmp_vec(g1, o1, 1e-9, "matvec")
    cmp_history(g1, o1, 1e-9)
    st = gA.stats()
    assert st["steps"] == oA.nsteps + 2
    if pprecond != 1:
        assert st["p_iters"] / st["steps"] < 100, st       # the two-level preconditioner at work (Jacobi: several hundred per step)


@pytest.mark.parametrize("pprecond", [1, 0, 2])
def test_pressure_iterations_match_oracle(gpu_ctx, pprecond):
    """as test_gpu_pprec_oracle.py::test_pressure_iterations_match_oracle: with the Jacobi preconditioner the iteration is the
    oracle's own; with the Schwarz preconditioner a wrong ghost layer, overlap count or hat weight at a 3- or 5-valent edge leaves
    the answer right and moves only this count"""
    hm, sem, gm = dev_case(gpu_ctx, PKEY)
    kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-11, ptol=1e-9, maxit_v=400, maxit_p=4000)
    U = t8.base_flow(sem)
    oA = ExptA(sem, U, LNSConfig(pprecond=pprecond, **kw))
    ov = t8.start_vector(sem)
    ov.pr[...] = 0.0
    oA.matvec(ov)
    ref = oA.stats["p_iters"]
    gb = host.nek_dvector(gm)
    for i in range(3):
        gb.set_field(i, U[i])
    gA = host.exptA_linop(kw["tau"], gb, pprecond=pprecond, pproj=0, **{k: v for k, v in kw.items() if k != "tau"})
    gA.init()
    gA.matvec(t8.upload(gm, ov), host.nek_dvector(gm))
    one = gA.stats()["p_iters"]
    print("STARMESH pprecond %d: p_iters %d, oracle %d" % (pprecond, one, ref))
    assert one >= 10 and abs(one - ref) <= 0.02 * ref + 2, (pprecond, one, ref)


_CHILD_HEADLINE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
from neklab_amd import host
import test_gpu_n8 as t8
import test_gpu_starmesh as T
ctx = host.Context(0)
hm, sem = T.host_case(T.PKEY)
ov = t8.start_vector(sem)
out = {}
for iters in (50, 200):
    gm, gA = T.prop_gpu(ctx, dict(T.PKW, **T.FIXED[iters]), 1, 0)
    gv, g1, g2 = t8.upload(gm, ov), host.nek_dvector(gm), host.nek_dvector(gm)
    gA.matvec(gv, g1)
    gA.matvec(g1, g2)
    out["pop"] = np.array(gm.pop_mfma())
    for k, g in ((1, g1), (2, g2)):
        out["p%%d_%%d" %% (iters, k)] = g.get_field(host.PR)
        for r in range(3 if k == 1 else 1):
            out["v%%d_%%d_%%d" %% (iters, k, r)] = np.stack([g.get_field(i, r) for i in range(3)])
np.savez(%(out)r, **out)
print("CHILD OK")
'''


def test_matvec_fixed_iterations_headline_kernels():
    """NLG_SMALL_E=0: the 30-element mesh takes the pressure kernels of large meshes (k_opgradt3n / k_opdiv3n or the matrix-pipe
    kernels) instead of the three-wave ones; a fresh process, since the switch is read once"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "headline.npz")
        tpp.run_child(_CHILD_HEADLINE % dict(root=ROOT, here=HERE, out=path), {"NLG_SMALL_E": "0"}, 300)
        got = dict(np.load(path))
    for iters in (50, 200):
        oA, kw, ov, o1, o2 = prop_oracle(iters, False, True)

        def getter(k):
            return lambda f, r: got["p%d_%d" % (iters, k)] if f == host.PR else got["v%d_%d_%d" % (iters, k, r)][f]
        check_fixed("headline kernels (pop_mfma %d)" % int(got["pop"]), iters, False, vec_errors(getter(1), 2, o1), vec_errors(getter(2), 0, o2))


# ---- (f) the random start vector -----------------------------------------------------------------------------------------------------
def test_rand_continuous_and_zero_on_walls(gpu_ctx):
    """the continuity step of nlg_vec_rand averages over 3, 5, 6 and 10 copies here (1 / 3, 1 / 5: no longer exact)"""
    hm, sem, gm = dev_case(gpu_ctx, PKEY)
    v, w = host.nek_dvector(gm), host.nek_dvector(gm)
    v.rand(ifnorm=True, seed=7)
    w.rand(ifnorm=True, seed=7)
    assert abs(v.norm() - 1.0) < 1e-13
    for i in range(3):
        a = v.get_field(i).reshape(sem.shape1)
        assert np.array_equal(a.ravel(), w.get_field(i))                                   # deterministic per seed
        assert np.max(np.abs(sem.gs(a) * sem.vmult - a)) <= 1e-14 * np.abs(a).max()        # C0
        assert np.all(a[sem.mask[i] == 0] == 0)                                            # walls
        assert np.std(a) > 0
    w.rand(ifnorm=True, seed=8)
    assert not np.array_equal(v.get_field(0), w.get_field(0))
