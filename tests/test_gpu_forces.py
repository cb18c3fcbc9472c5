"""Wall forces, torque and heat flux on the GPU (nlg_forces_*; host.wall_forces, nek_dns.set_wall_forces) against the numpy twin
tests/forces_ref.py.  Cases: A (2-D, lx1 = 6), B (3-D, lx1 = 8: a face is one wave), N10 and N12 (3-D, faces of 100 and 144 points: the
kernel loops).  The face list holds every wall face plus, on B, the interior faces 2 and 4 of one element, split over three objects
(forces_ref.case_objects).

Bounds, as tests/test_cpu_forces_ref.py derives its own: every sum contributes (operations on the path) x eps x (sum of the absolute
values of its summands), carried to first order through the products that follow.  forces_ref.tractions(err=True) states the stages of
p_q (a tensor contraction over n2^dim Gauss values: dim (5 n2 + 5)), of the gradient (a reference derivative: 5n + 5; the metrics and N_q
with the CPU test's bounds) and of a traction component; forces_ref.sample(err=True) those of a sum over an object: the summands' own
bounds, 4 eps more for a torque's cross product, plus (number of summands) x eps x (sum of their absolute values), since the order of the
summation is the kernel's own.
"""
import ctypes as C

import numpy as np
import pytest

import floquet_ref as fr
import forces_ref as fo
from neklab_amd import _lib, host
from oracle.lns import LNSConfig
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NU = 0.37
_vec = {}


def random_vectors(name, count=4):
    """`count` oracle vectors with random velocity, pressure and scalar, made once per case"""
    if name not in _vec:
        hm, sem = fo.mesh_of(name)
        rng = np.random.default_rng(7 + len(name) + sem.n)
        vs = []
        for _ in range(count):
            v = NekDVector(sem, nscal=1)
            for i in range(sem.dim):
                v.v[i][...] = rng.standard_normal(sem.shape1)
            v.pr[...] = rng.standard_normal(sem.shape2)
            v.theta[0][...] = rng.standard_normal(sem.shape1)
            vs.append(v)
        _vec[name] = vs
    return _vec[name]


def upload(gm, ov, heat=True):
    gv = host.nek_dvector(gm, nscal=1 if heat else 0)
    for i in range(gm.dim):
        gv.set_field(i, ov.v[i])
    gv.set_field(host.PR, ov.pr)
    if heat:
        gv.set_field(host.THETA, ov.theta[0])
    return gv


def without_scalar(sem, ov):
    return (ov.v, ov.pr, None)


def counters(ctx):
    a, b = C.c_int64(0), C.c_int64(0)
    host.check(ctx.lib.nlg_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


@pytest.mark.parametrize("name", ["A", "B", "N10", "N12"])
def test_tractions_pointwise(gpu_ctx, name):
    hm, sem = fo.mesh_of(name)
    n, dim = sem.n, sem.dim
    objects = fo.case_objects(name, hm)
    faces = [ef for o in objects for ef in o]
    if name == "B":
        assert sorted(set(f for _, f in faces)) == [1, 2, 3, 4, 5, 6]
    assert all(len(o) > 0 for o in objects) and not any(e < hm.E // 3 for e, _ in objects[1])
    assert any(len(set(k for k, o in enumerate(objects) if any(e == el for el, _ in o))) >= 2 for e in range(hm.E))
    gm = host.Mesh(gpu_ctx, hm)
    ov = random_vectors(name)[0]
    gv = upload(gm, ov)
    wf = host.wall_forces(gm, objects)
    assert wf.local == list(range(len(faces)))
    t = wf.tractions(gv, NU)
    P, T, N, Q, bp, bt, _ = fo.tractions(sem, faces, ov, NU, err=True)
    bn, _ = fo.geometry_err(sem, faces)
    rp, rt = np.max(np.abs(t["p"] - P) / bp), np.max(np.abs(t["trac"] - T) / bt)
    dn = np.abs(t["nds"] - N)
    rn = float(np.max(np.where(dn == 0.0, 0.0, dn / np.maximum(bn, 1e-300))))
    area = fo.areas(sem, objects)
    ea = np.max(np.abs(wf.area - area) / area)
    print("%s, %d faces of %d points: p %.2e of its bound (%.1e of max|p_q| = %.2f), traction %.2e of its bound (%.1e of max|t| = %.2f), N %.2e of its bound; areas %s, off by %.1e"
          % (name, len(faces), N.shape[1], rp, bp.max() / np.abs(P).max(), np.abs(P).max(), rt, bt.max() / np.abs(T).max(), np.abs(T).max(), rn, wf.area, ea))
    assert rp <= 1.0 and rt <= 1.0 and rn <= 1.0
    assert np.all(np.abs(wf.area - area) <= [2.0 * fo.geometry_err(sem, o)[0].sum() + (len(o) * N.shape[1] + 2) * EPS * a for o, a in zip(objects, area)])
    wf.close()


@pytest.mark.parametrize("heat", [True, False])
@pytest.mark.parametrize("name", ["A", "B", "N12"])
def test_sums_of_one_to_four_vectors(gpu_ctx, name, heat):
    hm, sem = fo.mesh_of(name)
    n, dim = sem.n, sem.dim
    objects = fo.case_objects(name, hm)
    centres = np.arange(3 * dim).reshape(3, dim) * 0.25 - 0.5
    gm = host.Mesh(gpu_ctx, hm)
    ovs = random_vectors(name)
    gvs = [upload(gm, ov, heat) for ov in ovs]
    wf = host.wall_forces(gm, objects, centres)
    nq = fo.nq(dim)
    single = [wf.sample(gv, NU) for gv in gvs]
    assert single[0].shape == (3, nq)
    worst = 0.0
    for s in (1, 2, 3, 4):
        out = wf.sample(gvs[:s], NU)
        again = wf.sample(gvs[:s], NU)
        assert out.shape == (s, 3, nq)
        assert np.array_equal(out, again), "two calls differ"
        for v in range(s):
            assert np.array_equal(out[v], single[v]), "vector %d of %d differs from its single call" % (v, s)
    for v, ov in enumerate(ovs):
        ref, bound, _ = fo.sample(sem, objects, ov if heat else without_scalar(sem, ov), NU, centres, err=True)
        d = np.abs(single[v] - ref)
        if not heat:
            assert np.all(single[v][:, -1] == 0.0) and np.all(ref[:, -1] == 0.0)
        worst = max(worst, float(np.max(np.where(d == 0.0, 0.0, d / np.maximum(bound, 1e-300)))))
    print("%s %s a scalar: s = 1..4 bit-equal to the single calls and from call to call; against the twin %.2e of the bound (%.1e of max|sum| = %.2f)"
          % (name, "with" if heat else "without", worst, bound.max() / np.abs(ref).max(), np.abs(ref).max()))
    assert worst <= 1.0
    wf.close()


def test_couette_torque_and_cylinder_drag(gpu_ctx):
    import test_cpu_forces_ref as cpu
    hm, sem, inner, outer = cpu.annulus()
    vel, pr, th, B = cpu.couette_fields(sem)
    gm = host.Mesh(gpu_ctx, hm)
    gv = host.nek_dvector(gm, nscal=1)
    for i in range(2):
        gv.set_field(i, vel[i])
    gv.set_field(host.PR, pr)
    gv.set_field(host.THETA, th)
    wf = host.wall_forces(gm, [inner, outer])
    S = wf.sample(gv, NU)
    T0, q0 = 4.0 * np.pi * NU * B, 2.0 * np.pi / np.log(2.0)
    et = [abs(S[0, 5] + T0) / T0, abs(S[1, 5] - T0) / T0]
    eq = [abs(S[0, 6] + q0) / q0, abs(S[1, 6] - q0) / q0]
    ea = np.abs(wf.area / np.array([2 * np.pi, 4 * np.pi]) - 1.0)
    print("Taylor-Couette on the device: torque %.1e, %.1e; heat flux %.1e, %.1e; forces %.1e; areas %.1e" % (et[0], et[1], eq[0], eq[1], np.abs(S[:, :4]).max(), ea.max()))
    assert max(et) <= 1e-8 and max(eq) <= 1e-8 and np.abs(S[:, :4]).max() <= 1e-12 and ea.max() <= 1e-13
    wf.close()
    hm, sem, faces, v, nu = cpu.cylinder_case()
    gm = host.Mesh(gpu_ctx, hm)
    gv = host.nek_dvector(gm)
    for i in range(2):
        gv.set_field(i, v[0][i])
    gv.set_field(host.PR, v[1])
    wf = host.wall_forces(gm, [faces])
    S = wf.sample(gv, nu)[0]
    cd, cl, tq = 2 * (S[0] + S[2]), 2 * (S[1] + S[3]), S[4] + S[5]
    print("cylinder on the device: Cd = %.6f = %.6f + %.6f, Cl = %.3e, torque = %.3e, area - pi = %.3e" % (cd, 2 * S[0], 2 * S[2], cl, tq, wf.area[0] - np.pi))
    assert abs(cd - 1.42676) <= 1e-5 and abs(cl) <= 1e-6 and abs(tq) <= 1e-6 and abs(wf.area[0] - np.pi) <= 1e-6
    # the tractions behind Cp and Cf along the wall add up to the forces of sample()
    t = wf.tractions(gv, nu)
    assert t["p"].shape == (16, sem.n)
    assert np.abs(t["trac"].sum(axis=(0, 1)) - (S[:2] + S[2:4])).max() <= 1e-13
    wf.close()


def test_refusals(gpu_ctx):
    hm, sem = fo.mesh_of("A")
    gm, gm2 = host.Mesh(gpu_ctx, hm), host.Mesh(gpu_ctx, hm)
    lib = gm.lib

    def create(elem, face, obj, nobj=2):
        el, fc, ob = np.array(elem, dtype=np.int64), np.array(face, dtype=np.int32), np.array(obj, dtype=np.int32)
        h = host.vp()
        host.check(lib.nlg_forces_create(gm.h, nobj, len(el), el.ctypes.data_as(_lib.c_int64_p), fc.ctypes.data_as(_lib.c_int_p),
                                         ob.ctypes.data_as(_lib.c_int_p), None, C.byref(h)))
        return h

    for face in (0, 5):
        with pytest.raises(host.NlgError, match=r"face\[1\]"):
            create([0, 1], [1, face], [0, 1])
    with pytest.raises(host.NlgError, match=r"elem_gid\[1\] = 9 .* no rank holds"):
        create([0, 9], [1, 1], [0, 1])
    with pytest.raises(host.NlgError, match=r"elem_gid / face.*listed twice"):
        create([0, 2, 0], [1, 1, 1], [0, 1, 1])
    for o in (-1, 2):
        with pytest.raises(host.NlgError, match=r"obj\[0\]"):
            create([0, 1], [1, 1], [o, 1])
    wf = host.wall_forces(gm, [[(0, 1), (0, 4)], [(8, 2)]])
    v = [host.nek_dvector(gm) for _ in range(5)]
    sentinel = -7.25
    out = np.full((5, 2, 7), sentinel)

    def sample(vecs, s=None):
        arr = (host.vp * len(vecs))(*[a.h for a in vecs])
        host.check(lib.nlg_forces_sample(wf.h, len(vecs) if s is None else s, arr, NU, host.dptr(out)))

    with pytest.raises(host.NlgError, match="s = 5"):
        sample(v)
    with pytest.raises(host.NlgError, match="s = 0"):
        sample(v[:1], 0)
    with pytest.raises(host.NlgError, match=r"vecs\[1\].*another mesh"):
        sample([v[0], host.nek_dvector(gm2)])
    with pytest.raises(host.NlgError, match=r"vecs\[2\].*nscal"):
        sample([v[0], v[1], host.nek_dvector(gm, nscal=1)])
    assert np.all(out == sentinel)
    # an attached object is not destroyed
    gX0 = host.nek_dvector(gm)
    X0 = fr.orbit_state("A")
    for i in range(2):
        gX0.set_field(i, X0.v[i])
    kw = {k: val for k, val in fr.case_cfg("A").items() if k != "tau"}
    dns = host.nek_dns(gX0, pprecond=1, pproj=0, **kw)
    dns.set_wall_forces(wf)
    with pytest.raises(host.NlgError, match="samples these faces"):
        wf.close()
    wf2 = host.wall_forces(gm2, [[(0, 1)]])
    with pytest.raises(host.NlgError, match="different mesh"):
        dns.set_wall_forces(wf2)
    dns.set_wall_forces(None)
    assert "force" not in dns.series()
    wf.close(), wf2.close()
    dns.close()


def test_dns_force_series(gpu_ctx):
    import dns_ref
    name, n = "A", 5
    hm, sem = fr.case_mesh(name)
    dim = sem.dim
    X0 = fr.orbit_state(name)
    objects = fo.case_objects(name, hm)
    gm = host.Mesh(gpu_ctx, hm)
    gX0 = host.nek_dvector(gm)
    for i in range(dim):
        gX0.set_field(i, X0.v[i])
    gX0.set_field(host.PR, X0.pr)
    kw = {k: v for k, v in fr.case_cfg(name).items() if k != "tau"}
    kw.update(pprecond=1, pproj=0)
    nu = 1.0 / kw["re"]
    xyz = np.array([p[1] for p in dns_ref.case_points(name, hm) if p[2] == 0][:6])
    hp = host.history_points(gm, xyz)
    wf = host.wall_forces(gm, objects)

    def run(forces, chunk, stepwise=False):
        dns = host.nek_dns(gX0, chunk=chunk, **kw)
        dns.set_history_points(hp)
        dns.set_reference()
        if forces:
            dns.set_wall_forces(wf)
        states = [wf.sample(dns.state(), nu)]
        dns.advance(0)
        l0, c0 = counters(gpu_ctx)
        if stepwise:
            for _ in range(n):
                dns.advance(1)
                states.append(wf.sample(dns.state(), nu))
        else:
            dns.advance(n)
        l1, c1 = counters(gpu_ctx)
        s = dns.series()
        dns.close()
        return s, np.array(states), l1 - l0, c1 - c0

    s_step, states, _, _ = run(True, 256, True)
    assert s_step["force"].shape == (n + 1, 3, fo.nq(dim))
    assert np.array_equal(s_step["force"], states), "the series differs from sample(state after step k)"
    s_f, _, lf, cf = run(True, 256)
    s_0, _, l0, c0 = run(False, 256)
    s_2, _, _, _ = run(True, 2)
    s_02, _, _, _ = run(False, 2)
    assert "force" not in s_0
    for a in (s_f, s_2, s_02, s_step):
        for key in ("time", "probe", "dist"):
            assert np.array_equal(a[key], s_0[key]), key
    assert np.array_equal(s_2["force"], s_f["force"]) and np.array_equal(s_step["force"], s_f["force"])
    print("%d steps on %s: launches %d with forces, %d without (%.1f per step more); collectives %d and %d" % (n, name, lf, l0, (lf - l0) / n, cf, c0))
    assert 0 < lf - l0 <= 2 * n and cf <= c0
    ref = fo.dns_force_series(sem, LNSConfig(**fr.case_cfg(name)), X0, n, objects)
    scale = np.abs(ref).max()
    err = np.abs(s_f["force"] - ref).max() / scale
    print("force series against the twin's of the oracle run: %.3e of max|F| = %.3e; Fv_x on the y walls: %s" % (err, scale, ["%.5e" % f for f in s_f["force"][:, 0, dim]]))
    assert err <= 1e-10
    hp.close(), wf.close()
