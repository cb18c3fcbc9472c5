"""CPU suite of the wall forces: the numpy twin (tests/forces_ref.py) against analysis, and the host geometry of the product
(nlg_forces_geometry, neklab_amd/csrc/forces_host.cpp; no GPU needed) against the twin's.

Analytic cases and their bounds.  Taylor-Couette flow in the annulus 1 <= r <= 2 of the thermosyphon fixture (inner wall Omega = 1,
outer at rest: u_theta = A r + B / r, A = -1/3, B = 4/3, p' = u_theta^2 / r): torque -4 pi nu B on the inner wall and +4 pi nu B on the
outer one, to 1e-8 relative -- a prototype of the definitions met them to 3.4e-10 and 5.6e-12 (the spectral error of 1 / r on 8 x 32
elements at lx1 = 8), the margin covers another summation order; a wrong sign or a missing transpose term is off by O(1).  Heat flux of
theta = ln r / ln 2 through the inner wall: -2 pi / ln 2 at the same 1e-8.  Hydrostatic load on the walls of cases A and B: the pressure
is y of the undeformed box on the Gauss points (linear inside every element, so the extrapolation to the walls, where the deformation
vanishes, is exact): Fp = V e_y and the areas 4 and 8 to rounding, 1e-13.  Reference cylinder (Re = 50 base flow of the fixture, the 16
'W' faces with r < 0.6): Cd = 1.42676 = 0.96403 + 0.46273 within 1e-5, |Cl| and |torque| <= 1e-6 (the prototype: 3e-8, 4e-9), area within
1e-6 of pi (the field file's float32 coordinates: 1.6e-7).

Geometry bound (test_geometry_against_the_twin).  Twin and product evaluate the same formulas with different code; a value differs by
at most its rounding-error bound: (operations on the path) x eps x (sum of the absolute values of the summands) for every sum, carried
through the products, the cofactors, the Jacobian and the quotient to first order -- forces_ref.metric_err and geometry_err state every
stage and its constant (a coordinate derivative: 5n + 5; the GLL weights: 32n + 2).  x_q - c: one subtraction, eps (|x| + |c|).
area = sum |N_q|: the bounds of N_q summed (2 for the root) + (points + 2) eps area.
"""
import os

import numpy as np
import pytest

import forces_ref as fo
import refdata
from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
_tc = {}


def annulus():
    if not _tc:
        hm, _ = refdata.load_tsyphon()
        sem = SEM(hm)
        walls = fo.wall_faces(hm)
        r = [np.hypot(hm.x[e], hm.y[e]) for e, _ in walls]
        _tc["v"] = (hm, sem, [w for w, rr in zip(walls, r) if rr.min() < 1.5], [w for w, rr in zip(walls, r) if rr.max() > 1.5])
    return _tc["v"]


def couette_fields(sem):
    x, y = sem.X
    r = np.hypot(x, y)
    A, B = -1.0 / 3.0, 4.0 / 3.0
    ut = A * r + B / r
    p1 = A * A * r * r / 2 + 2 * A * B * np.log(r) - B * B / (2 * r * r)
    return [-ut * y / r, ut * x / r], sem.to_mesh2(p1), np.log(r) / np.log(2.0), B


def cylinder_case():
    """(host mesh, sem, the 16 cylinder faces as (local element, face), (ux, uy, p on the Gauss mesh), nu)"""
    if "cyl" not in _tc:
        hm, ux, uy, p, re, lxd, _ = refdata.load_cylinder(with_bcs=True)
        d = np.load(os.path.join(HERE, "golden", "reference_cyl_baseflow.npz"))
        pos = {int(g): k for k, g in enumerate(d["elmap"])}
        faces = [(pos[int(e)], int(f)) for e, f, t in zip(d["bc_elem"], d["bc_face"], d["bc_tag"]) if str(t) == "W"]
        faces = [(e, f) for e, f in faces if np.hypot(hm.x[e], hm.y[e]).min() < 0.6]
        sem = SEM(hm)
        _tc["cyl"] = (hm, sem, faces, ([sem.f1(ux), sem.f1(uy)], sem.to_mesh2(sem.f1(p)), None), 1.0 / re)
    return _tc["cyl"]


def test_taylor_couette_torque_and_heat_flux():
    hm, sem, inner, outer = annulus()
    assert len(inner) == len(outer) == 32
    vel, pr, th, B = couette_fields(sem)
    nu = 0.37
    S = fo.sample(sem, [inner, outer], (vel, pr, th), nu)
    T0 = 4.0 * np.pi * nu * B
    area = fo.areas(sem, [inner, outer])
    et = [abs(S[0, 5] + T0) / T0, abs(S[1, 5] - T0) / T0]
    ef = np.abs(S[:, :4]).max()
    q0 = 2.0 * np.pi / np.log(2.0)
    eq = [abs(S[0, 6] + q0) / q0, abs(S[1, 6] - q0) / q0]
    ea = np.abs(area / np.array([2 * np.pi, 4 * np.pi]) - 1.0)
    print("Taylor-Couette: torque inner %.10f outer %.10f (4 pi nu B = %.10f): %.1e, %.1e; forces %.1e; pressure torque %.1e; Q %.1e, %.1e; areas %.1e"
          % (S[0, 5], S[1, 5], T0, et[0], et[1], ef, np.abs(S[:, 4]).max(), eq[0], eq[1], ea.max()))
    assert max(et) <= 1e-8 and max(eq) <= 1e-8
    assert ef <= 1e-12 and np.abs(S[:, 4]).max() <= 1e-12 and ea.max() <= 1e-13


@pytest.mark.parametrize("name", ["A", "B"])
def test_hydrostatic_load(name):
    hm, sem = fo.mesh_of(name)
    kw = dict(A=dict(nel=(3, 3), n=6, lengths=(1.0, 1.0)), B=dict(nel=(2, 2, 2), n=8, lengths=(2.0, 1.0, 1.0), periodic=(True, False, False)))[name]
    s0 = SEM(box_mesh(deform=0.0, **kw))
    V, area = (1.0, 4.0) if name == "A" else (2.0, 8.0)
    walls = fo.wall_faces(hm)
    zero = [np.zeros(sem.shape1)] * sem.dim
    S = fo.sample(sem, [walls], (zero, s0.to_mesh2(s0.X[1]), None), 1.0)[0]
    ef = np.abs(S[:sem.dim] - V * np.eye(sem.dim)[1]).max()
    ea = abs(fo.areas(sem, [walls])[0] - area)
    print("case %s, %d wall faces: |Fp - V e_y| = %.1e, area error %.1e" % (name, len(walls), ef, ea))
    assert ef <= 1e-13 and ea <= 1e-13 and np.all(S[sem.dim:2 * sem.dim] == 0.0)


def test_reference_cylinder_drag():
    hm, sem, faces, v, nu = cylinder_case()
    assert len(faces) == 16
    S = fo.sample(sem, [faces], v, nu)[0]
    cd, cdp, cdv, cl, tq = 2 * (S[0] + S[2]), 2 * S[0], 2 * S[2], 2 * (S[1] + S[3]), S[4] + S[5]
    ea = fo.areas(sem, [faces])[0] - np.pi
    print("cylinder Re = 50: Cd = %.6f = %.6f (pressure) + %.6f (viscous); Cl = %.3e; torque = %.3e; area - pi = %.3e" % (cd, cdp, cdv, cl, tq, ea))
    assert abs(cd - 1.42676) <= 1e-5 and abs(cdp - 0.96403) <= 1e-5 and abs(cdv - 0.46273) <= 1e-5
    assert abs(cl) <= 1e-6 and abs(tq) <= 1e-6 and abs(ea) <= 1e-6


def geometry_case(name):
    """(host mesh, sem, faces): every face of every element on the boxes (all orientations and signs, walls and interior faces, 2 dim
    listed faces per element); on the annulus the walls and the four faces of two elements"""
    if name == "annulus":
        hm, sem, inner, outer = annulus()
        return hm, sem, inner + outer + [(5, f) for f in (1, 2, 3, 4) if (5, f) not in inner + outer] + [(100, 2), (100, 4)]
    hm, sem = fo.mesh_of(name)
    return hm, sem, [(e, f) for e in range(hm.E) for f in range(1, 2 * hm.dim + 1)]


@pytest.mark.parametrize("name", ["A", "B", "N10", "N12", "annulus"])
def test_geometry_against_the_twin(name):
    hm, sem, faces = geometry_case(name)
    n, dim = sem.n, sem.dim
    N, G, XC = fo.geometry(sem, faces)
    bN, bG = fo.geometry_err(sem, faces)
    g = host.forces_geometry(hm, faces)
    ratio = lambda d, b: float(np.max(np.where(d == 0.0, 0.0, d / np.maximum(b, 1e-300))))   # 0 / 0 (a coordinate that is 0 along a whole line) is 0
    rN, rG = ratio(np.abs(g["nds"] - N), bN), ratio(np.abs(g["met"] - G), bG)
    rX = ratio(np.abs(g["xc"] - XC), EPS * np.abs(XC))
    area = np.linalg.norm(N, axis=-1).sum()
    bA = 2.0 * bN.sum() + (N.shape[0] * N.shape[1] + 2) * EPS * area
    print("%s: %d faces, |N - N_twin| %.2e of its bound (largest bound %.1e of max |N|), metrics %.2e of theirs, x %.2e eps; area %.15g, off by %.1e (bound %.1e)"
          % (name, len(faces), rN, bN.max() / np.abs(N).max(), rG, rX, g["area"][0], abs(g["area"][0] - area), bA))
    assert rN <= 1.0 and rG <= 1.0 and rX <= 1.0
    assert abs(g["area"][0] - area) <= bA
    # objects and centres: element 0 with two faces in object 1, element 1 with three faces split over objects 0 and 2
    sub = [(0, 1), (0, 2), (1, 1), (1, 2), (1, 3)]
    obj, c = [1, 1, 0, 2, 2], np.arange(3 * dim).reshape(3, dim) + 0.5
    gs = host.forces_geometry(hm, sub, obj=obj, nobj=3, centres=c)
    Ns, _, Xs = fo.geometry(sem, sub, [c[o] for o in obj])
    bNs, _ = fo.geometry_err(sem, sub)
    assert np.all(np.abs(gs["nds"] - Ns) <= bNs)
    assert np.all(np.abs(gs["xc"] - Xs) <= EPS * (np.abs(Xs) + 2 * np.abs(c).max()))
    for o in range(3):
        want = sum(np.linalg.norm(Ns[q], axis=-1).sum() for q in range(5) if obj[q] == o)
        assert abs(gs["area"][o] - want) <= 2.0 * bNs.sum() + (3 * N.shape[1] + 2) * EPS * want


def test_geometry_refuses_bad_arguments():
    hm, sem = fo.mesh_of("A")
    for faces, kw in (([(0, 5)], {}), ([(0, 0)], {}), ([(9, 1)], {}), ([(-1, 1)], {}), ([(0, 1)], dict(obj=[1], nobj=1)), ([(0, 1)], dict(obj=[-1], nobj=1))):
        with pytest.raises(host.NlgError):
            host.forces_geometry(hm, faces, **kw)


def test_face_list_helpers():
    for name in ("A", "B"):
        hm, sem = fo.mesh_of(name)
        assert host.faces_from_mask(hm) == [(int(hm.elem_gid[e]), f) for e, f in fo.wall_faces(hm)]
        part = hm.take(np.arange(hm.E)[1::2])                                  # a partition lists its own elements by their global ids
        assert set(host.faces_from_mask(part)) <= set(host.faces_from_mask(hm)) and all(e % 2 == 1 for e, _ in host.faces_from_mask(part))
    d = np.load(os.path.join(HERE, "golden", "reference_cyl_baseflow.npz"))
    bcs = list(zip(d["bc_elem"], d["bc_face"], d["bc_tag"]))
    hm, sem, faces, _, _ = cylinder_case()
    pos = {int(g): k for k, g in enumerate(d["elmap"])}
    near = lambda e, f: np.hypot(hm.x[pos[e + 1]], hm.y[pos[e + 1]]).min() < 0.6
    got = host.faces_from_bcs(bcs, tags=("W",), select=near)
    assert [(pos[e + 1], f) for e, f in got] == faces and len(got) == 16
    assert len(host.faces_from_bcs(bcs, tags=("W", "v"))) > len(host.faces_from_bcs(bcs)) >= 16
