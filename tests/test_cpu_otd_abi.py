"""CPU suite: the OTD entry points (nlg_otd_*) are declared, exported, bound in ctypes and in the Fortran capi module, fail with a
message on NULL handles, and the host-side pieces of the analysis -- the ordering of spectral_analysis, the Ls.dat / Lr.dat line
format -- are exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTD_SYMBOLS = ["nlg_otd_opts_default", "nlg_otd_create", "nlg_otd_advance", "nlg_otd_reduced", "nlg_otd_get_basis",
               "nlg_otd_get_baseflow", "nlg_otd_info", "nlg_otd_destroy"]


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_otd_symbols_declared_bound_and_exported(lib):
    from neklab_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neklab_gpu.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    for nm in OTD_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % nm, hdr), "header lacks %s" % nm
        assert hasattr(lib, nm), "library lacks %s" % nm
        assert nm in _lib.SIGNATURES, "ctypes table lacks %s" % nm
        assert 'name="%s"' % nm in capi, "Fortran capi module lacks %s" % nm
    assert "typedef struct nlg_otd_opts { int r; int startstep; int orthostep; int trans; int solve_baseflow; } nlg_otd_opts;" in hdr
    assert [f[0] for f in _lib.OtdOpts._fields_] == ["r", "startstep", "orthostep", "trans", "solve_baseflow"]


def test_otd_defaults_and_null_handles(lib):
    from neklab_amd import _lib
    o = _lib.OtdOpts()
    assert lib.nlg_otd_opts_default(C.byref(o)) == 0
    assert (o.r, o.startstep, o.orthostep, o.trans, o.solve_baseflow) == (2, 1, 10, 0, 0)
    h = C.c_void_p()
    buf = np.zeros(16)
    calls = {
        "nlg_otd_opts_default": lambda: lib.nlg_otd_opts_default(None),
        "nlg_otd_create": lambda: lib.nlg_otd_create(None, C.byref(o), None, C.byref(h)),
        "nlg_otd_advance": lambda: lib.nlg_otd_advance(None, 1),
        "nlg_otd_reduced": lambda: lib.nlg_otd_reduced(None, _lib.dptr(buf), _lib.dptr(buf)),
        "nlg_otd_get_basis": lambda: lib.nlg_otd_get_basis(None, 0, None),
        "nlg_otd_get_baseflow": lambda: lib.nlg_otd_get_baseflow(None, None),
        "nlg_otd_info": lambda: lib.nlg_otd_info(None, None, None, None),
    }
    for nm, call in calls.items():
        assert call() != 0, nm
        assert nm.encode() in lib.nlg_last_error(), (nm, lib.nlg_last_error())
    assert lib.nlg_otd_destroy(None) == 0           # like every destroy of the ABI


def test_spectral_analysis_orders_sigma_and_lambda():
    from neklab_amd.host import nek_otd
    # eigenvalues of Lr: the pair 1 +- 2i, and 3 and -4 on the diagonal blocks -> 3, (1 + 2i, 1 - 2i in either order) ... here 3 x 3:
    Lr = np.array([[1.0, 2.0, 0.5], [-2.0, 1.0, 0.0], [0.0, 0.0, 3.0]])
    sigma, svec, lam, eigvec = nek_otd.spectral_analysis(Lr)
    Ls = 0.5 * (Lr + Lr.T)
    assert np.all(np.diff(sigma) <= 0) and np.allclose(sorted(sigma), np.linalg.eigvalsh(Ls), atol=1e-14)
    for k in range(3):
        assert np.linalg.norm(Ls @ svec[:, k] - sigma[k] * svec[:, k]) < 1e-13
    assert np.all(np.diff(lam.real) <= 1e-14)
    assert abs(lam[0] - 3.0) < 1e-13 and abs(lam[1].real - 1.0) < 1e-13 and abs(lam[2].real - 1.0) < 1e-13
    assert sorted([lam[1].imag, lam[2].imag]) == pytest.approx([-2.0, 2.0], abs=1e-13)
    for k in range(3):
        assert np.linalg.norm(Lr @ eigvec[:, k] - lam[k] * eigvec[:, k]) < 1e-13


def test_log_line_format_is_the_reference_format():
    """'(I8,1X,F15.8,A,*(1X,E15.8))': Fortran's E15.8 writes 0.dddddddd E+ee, right-justified"""
    from neklab_amd.host import otd_log_line
    ls = otd_log_line(25, 0.25, (" Ls ", [1.2345678912, -0.000123456789, 0.0]))
    assert ls == "      25      0.25000000 Ls   0.12345679E+01 -0.12345679E-03  0.00000000E+00"
    lr = otd_log_line(12345678, 1234.5, (" Lr%Re ", [-5.2458, 99999999.9]), (" Lr%Im ", [0.7099, -0.7099]))
    assert lr == ("12345678   1234.50000000 Lr%Re  -0.52458000E+01  0.10000000E+09 Lr%Im   0.70990000E+00 -0.70990000E+00")
    # every number field is 1 + 15 wide
    assert len(ls) == 8 + 1 + 15 + 4 + 3 * 16


def test_fortran_shim_carries_the_otd_types():
    """otd_opts / nek_otd in neklab_linops, otd_analysis in neklab_analysis, reached through `use neklab` (that they compile against the
    abstract types is what tests/test_cpu_abi.py builds)"""
    fdir = os.path.join(ROOT, "neklab_amd", "fortran")
    lin = open(os.path.join(fdir, "neklab_linops.f90")).read()
    ana = open(os.path.join(fdir, "neklab_analysis.f90")).read()
    umb = open(os.path.join(fdir, "neklab.f90")).read()
    assert re.search(r"type, public :: otd_opts", lin) and re.search(r"type, public :: nek_otd", lin)
    for field in ("startstep", "printstep", "orthostep", "iostep", "iorststep", "n_usrIC", "trans", "solve_baseflow", "OTDIC_basename"):
        assert re.search(r"::\s*%s\b" % field, lin), field
    assert re.search(r"public :: otd_analysis", ana) and re.search(r"subroutine otd_analysis\(OTD", ana)
    assert "'(I8,1X,F15.8,A,*(1X,E15.8))'" in ana
    assert re.search(r"use neklab_linops\s*$", umb, re.M) and re.search(r"use neklab_analysis\s*$", umb, re.M) and not os.path.exists(os.path.join(fdir, "neklab_otd.f90"))
