"""CPU suite of the eigenvalue sensitivity: the entry points are declared, bound and exported and refuse NULL arguments; the numpy
statement tests/sens_ref.py reproduces closed forms and satisfies the identity it is defined by,

    <a, L(U + dU) u - L(U) u> = <S(u, a), dU>        (nek_ddot; u solenoidal, dU zero on the boundary),

exactly where both quadratures are exact and to discretisation error otherwise."""
import os
import re

import numpy as np
import pytest

import lns_ref
import sens_ref
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlg_sens_apply", "nlg_sens_pairing")


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_sens_symbols_are_declared_bound_and_exported(lib):
    from neklab_amd import _lib
    header = open(os.path.join(ROOT, "include", "neklab_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for nm in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % nm, header), "header lacks %s" % nm
        assert nm in _lib.SIGNATURES, "ctypes table lacks %s" % nm
        assert hasattr(lib, nm), "library lacks %s" % nm
    # the Fortran shim binds both and exports eigenvalue_sensitivity
    capi = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    for nm in NEW:
        assert 'name="%s"' % nm in capi
    analysis = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_analysis.f90")).read()
    assert re.search(r"public\s*::.*\beigenvalue_sensitivity\b", analysis) and "subroutine eigenvalue_sensitivity(" in analysis
    from neklab_amd import host
    for nm in ("eigenvalue_sensitivity", "sensitivity_analysis", "predict_eigenvalue_shift"):
        assert hasattr(host, nm)


def test_sens_entry_points_refuse_null_arguments(lib):
    calls = {
        "nlg_sens_apply": lambda: lib.nlg_sens_apply(None, 1, None, None, None, None, None, None, None, None, None, None),
        "nlg_sens_pairing": lambda: lib.nlg_sens_pairing(None, None, None, None, None),
    }
    assert set(calls) == set(NEW)
    for nm, call in calls.items():
        assert call() != 0, nm
        msg = lib.nlg_last_error()
        assert nm.encode() in msg and b"NULL" in msg, (nm, msg)


def unmasked_box(nel, n, deform=0.0):
    hm = box_mesh(nel, n, periodic=(False,) * len(nel), deform=deform)
    for m in hm.mask:
        m[...] = 1.0
    return hm, SEM(hm)


@pytest.mark.parametrize("nel,n", [((2, 2), 5), ((2, 2, 2), 8)], ids=["2d", "3d"])
def test_polynomial_pair_gives_the_closed_form(nel, n):
    """u = (y^2 + x z, x^2 - y z, x y), a = (x y + z, y^2 - x z, x + y z) (z = 0 in 2-D): degree <= 2 per direction, differentiated
    exactly at lx1 >= 5; T, P and S against the products written out by hand, to 1e-12 of the scale of each."""
    hm, sem = unmasked_box(nel, n)
    u, a, exact = sens_ref.poly_pair(sem)
    T, P = sens_ref.parts(sem, u, a)
    got = dict(T=T, P=P, S=[t + p for t, p in zip(T, P)])
    for name in ("T", "P", "S"):
        scale = max(np.abs(r).max() for r in exact[name])
        err = max(np.abs(g - r).max() for g, r in zip(got[name], exact[name]))
        print("%s %d-D: scale %.3g, absolute error %.3e" % (name, sem.dim, scale, err))
        assert err <= 1e-12 * scale
    # the complex split: S(u^, conj(u^+)) with u^ = u + i a', u^+ = a + i u' is the four real combinations of the definition
    ui, ai = [0.5 * f for f in a], [-0.25 * f for f in u]
    out = sens_ref.sensitivity(sem, u, ui, a, ai)
    S = lambda p, q: [t + r for t, r in zip(*sens_ref.parts(sem, p, q))]
    re_ = [x + y for x, y in zip(S(u, a), S(ui, ai))]
    im_ = [x - y for x, y in zip(S(ui, a), S(u, ai))]
    scale = max(np.abs(r).max() for r in re_ + im_)
    assert max(np.abs(g - r).max() for g, r in zip(out["grad_re"] + out["grad_im"], re_ + im_)) <= 1e-12 * scale


def identity_sides(hm, sem, u, a, dU, U):
    p = np.zeros(sem.shape2)
    L0 = lns_ref.lns_strong(sem, U, u, p, 40.0)
    L1 = lns_ref.lns_strong(sem, [b + d for b, d in zip(U, dU)], u, p, 40.0)
    lhs = sens_ref.ddot(sem, a, [x - y for x, y in zip(L1, L0)])
    T, P = sens_ref.parts(sem, u, a)
    rhs = sens_ref.ddot(sem, [t + q for t, q in zip(T, P)], dU)
    return lhs, rhs


POLY_CASES = [((3, 2), 6), ((2, 2, 2), 8)]


@pytest.mark.parametrize("nel,n", POLY_CASES, ids=["3x2_n6", "2x2x2_n8"])
def test_identity_is_exact_on_polynomial_fields(nel, n):
    """Undeformed box [0, nel], unmasked.  Degrees per direction: u and a 2 (u solenoidal), dU 3 (the boundary bubble, degree 2 per
    direction, times a linear field).  Left side: a (dU . grad u + u . grad dU), degree <= 2 + 3 + 2 = 7 per direction, integrated on
    the 3 lx1 / 2 Gauss points of the dealiased weak term (exact to degree 3 lx1 - 1).  Right side: S(u, a) . dU, degree <= 2 + 2 +
    3 = 7, on the GLL points, exact to degree 2 lx1 - 3 = 9 at lx1 = 6 and 13 at lx1 = 8.  Both exact: the sides agree to rounding,
    bound 1e-11 relative."""
    hm, sem = unmasked_box(nel, n)
    u, a, _ = sens_ref.poly_pair(sem)
    U = lns_ref.poly_fields(sem)[0]
    dU = sens_ref.bubble_dU(sem, [float(e) for e in nel])
    lhs, rhs = identity_sides(hm, sem, u, a, dU, U)
    print("identity %s lx1 = %d: <a, dL u> = %.15e, <S, dU> = %.15e, relative difference %.3e" % (nel, n, lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(rhs) > 1e-2
    assert abs(lhs - rhs) <= 1e-11 * abs(rhs)


def smooth_defect(n):
    hm, sem = unmasked_box((3, 2), n, deform=0.05)
    x, y = sem.X
    # u = (d_y psi, -d_x psi) with psi = sin(0.9 x + 0.2) cos(1.1 y): solenoidal
    u = [-1.1 * np.sin(0.9 * x + 0.2) * np.sin(1.1 * y), -0.9 * np.cos(0.9 * x + 0.2) * np.cos(1.1 * y)]
    a = [np.cos(0.7 * x + 0.4 * y), np.sin(0.5 * x - 0.8 * y) + 0.3]
    U = [1.0 + 0.3 * np.sin(0.6 * y), 0.2 * np.cos(0.5 * x)]
    b = np.sin(np.pi * x / 3.0) * np.sin(np.pi * y / 2.0)     # zero on the boundary of [0, 3] x [0, 2]
    dU = [b * np.exp(0.2 * x), b * np.cos(0.6 * y + 0.1 * x)]
    lhs, rhs = identity_sides(hm, sem, u, a, dU, U)
    return abs(lhs - rhs) / abs(rhs), lhs, rhs


def test_identity_holds_to_discretisation_error_on_smooth_fields():
    """Smooth non-polynomial fields on the deformed 3 x 2 box: the defect of the identity is discretisation error and falls by at least
    a factor 4 from lx1 = 6 to lx1 = 8."""
    d6, l6, r6 = smooth_defect(6)
    d8, l8, r8 = smooth_defect(8)
    print("smooth identity: lx1 = 6: lhs %.12e rhs %.12e defect %.3e;  lx1 = 8: lhs %.12e rhs %.12e defect %.3e;  ratio %.1f"
          % (l6, r6, d6, l8, r8, d8, d6 / d8))
    assert d8 * 4.0 <= d6
