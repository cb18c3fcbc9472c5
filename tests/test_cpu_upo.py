"""CPU suite of the periodic-orbit Newton: the entry points are declared, bound and exported and refuse what is not an operator in
orbit mode; the numpy statement tests/upo_ref.py has the properties the GPU tests rely on (the bordered Jacobian is the derivative of
the residual, in X and in T); the extended vector algebra against hand values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import floquet_ref as fr
import upo_ref as ur
from oracle.vectors import NekDVector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlg_linop_set_orbit_steps", "nlg_upo_residual", "nlg_upo_fdot", "nlg_upo_jac_matvec", "nlg_upo_border", "nlg_upo_arnoldi_step")

FT_FD_BOUND, DELTA_T = ur.FT_FD_BOUND, ur.DELTA_T


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_upo_symbols_are_declared_bound_and_exported(lib):
    from neklab_amd import _lib
    header = open(os.path.join(ROOT, "include", "neklab_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for nm in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % nm, header), "header lacks %s" % nm
        assert nm in _lib.SIGNATURES, "ctypes table lacks %s" % nm
        assert hasattr(lib, nm), "library lacks %s" % nm
    # the Fortran shim binds what its systems and its linear solver call
    capi = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    for nm in NEW:
        if nm != "nlg_upo_border":
            assert 'name="%s"' % nm in capi
    from neklab_amd import host
    for nm in ("nek_ext_dvector", "nek_upo_system", "gmres_upo", "newton_periodic_orbit", "outpost_ext_dnek"):
        assert hasattr(host, nm)


def test_upo_entry_points_refuse_what_is_not_an_orbit_operator(lib):
    """Without a device no operator exists; a NULL one is the operator that is not in orbit mode: an error code and a message that
    names the call and nlg_linop_set_orbit, not a crash."""
    t = C.c_double()
    calls = {
        "nlg_linop_set_orbit_steps": lambda: lib.nlg_linop_set_orbit_steps(None, None, 1.0, 3),
        "nlg_upo_residual": lambda: lib.nlg_upo_residual(None, None),
        "nlg_upo_fdot": lambda: lib.nlg_upo_fdot(None, 0, None),
        "nlg_upo_jac_matvec": lambda: lib.nlg_upo_jac_matvec(None, None, 0.0, None, C.byref(t)),
        "nlg_upo_border": lambda: lib.nlg_upo_border(None, None, 0.0, None, C.byref(t), 0),
        "nlg_upo_arnoldi_step": lambda: lib.nlg_upo_arnoldi_step(None, None, None, 0, None, 2),
    }
    assert set(calls) == set(NEW)
    for nm, call in calls.items():
        assert call() != 0, nm
        msg = lib.nlg_last_error()
        assert nm.encode() in msg and b"nlg_linop_set_orbit" in msg, (nm, msg)


def _case():
    hm, sem = fr.case_mesh("A")
    return sem, ur.UpoRef(sem, fr.tangent_cfg(), nsteps=6), ur.Ext(fr.orbit_state("A"), 6 * fr.DT), fr.start_vector(sem)


def test_reference_jacobian_is_the_derivative_of_the_residual():
    """Case A, 6 steps, no history, fixed step count.  x-block: [R(X + eps v, T) - R(X - eps v, T)] / 2 eps against M v - v meets the
    three conditions of floquet_ref.check_tangent (the frozen operator's F v - v is the one that must miss).  T-column: the
    difference quotient in T against fT, first order in dt: printed, bound FT_FD_BOUND."""
    sem, ref, X, v = _case()
    ev = ur.Ext(v, 0.0)
    Jv = ref.jacobian(X, ev).vec                                   # M v - v  (t = 0)
    Fv = fr.FloquetRef(sem, ref.config(X.T)).frozen_matvec(X.vec, v)
    Fv.axpby(-1.0, v, 1.0)

    def R(x):
        return ref.run(x, X.T)["res"]

    e = [fr.tangent_errors(R, Jv, X.vec, v, eps) for eps in fr.EPS]
    e_frozen = fr.tangent_errors(R, Fv, X.vec, v, fr.EPS[1])
    print("x-block (oracle): e(%g) = %.3e, e(%g) = %.3e, ratio %.1f, frozen operator %.3e" % (fr.EPS[0], e[0], fr.EPS[1], e[1], e[0] / e[1], e_frozen))
    fr.check_tangent(e[0], e[1], e_frozen)

    d = DELTA_T * X.T
    fT = ref.run(X.vec, X.T)["fT"]
    q = ref.run(X.vec, X.T + d)["res"]
    q.axpby(-1.0, ref.run(X.vec, X.T - d)["res"], 1.0)
    q.scal(0.5 / d)
    err = fr.vec_err(q, fT)
    print("T-column (oracle): |dR/dT - fT| / |fT| = %.4e (bound %.3e)" % (err, FT_FD_BOUND))
    assert err <= FT_FD_BOUND               # twice the value measured here on the CPU: 7.11e-3 (tests/upo_ref.py)


def test_extended_vector_algebra_against_hand_values():
    hm, sem = fr.case_mesh("A")
    area = float(np.sum(sem.bm1))                                   # <1, 1> over the box
    a, b = ur.Ext(NekDVector(sem), 2.0), ur.Ext(NekDVector(sem), -3.0)
    a.vec.v[0][...] = 1.0
    b.vec.v[0][...] = 4.0
    b.vec.v[1][...] = 5.0
    b.vec.pr[...] = 7.0                                             # the pressure is not part of the inner product
    assert a.dot(b) == pytest.approx(4.0 * area - 6.0, rel=1e-14)
    assert a.norm() == pytest.approx(np.sqrt(area + 4.0), rel=1e-14)
    c = a.copy()
    c.axpby(2.0, b, -1.0)                                           # c = 2 b - a
    assert c.T == -8.0
    assert np.array_equal(c.vec.v[0], np.full(sem.shape1, 7.0)) and np.array_equal(c.vec.v[1], np.full(sem.shape1, 10.0))
    assert np.array_equal(c.vec.pr, np.full(sem.shape2, 14.0))
    c.scal(0.5)
    assert c.T == -4.0 and np.array_equal(c.vec.v[0], np.full(sem.shape1, 3.5))
    assert a.T == 2.0 and np.array_equal(a.vec.v[0], np.ones(sem.shape1))   # copy() copies
    assert c.dot(c) == pytest.approx((3.5 ** 2 + 5.0 ** 2) * area + 16.0, rel=1e-14)
