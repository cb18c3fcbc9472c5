"""CPU suite: the entry points of the coupled (orbit) mode are declared, bound and exported, and their Python wrappers fail loudly
without a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlg_linop_set_orbit", "nlg_linop_orbit_end", "nlg_linop_lane_iters")


@pytest.fixture(scope="module")
def lib():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import _lib
    return _lib.load()


def test_orbit_symbols_are_declared_bound_and_exported(lib):
    from neklab_amd import _lib
    header = open(os.path.join(ROOT, "include", "neklab_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for nm in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % nm, header), "header lacks %s" % nm
        assert nm in _lib.SIGNATURES, "ctypes table lacks %s" % nm
        assert hasattr(lib, nm), "library lacks %s" % nm
    assert len(_lib.SIGNATURES["nlg_linop_set_orbit"][1]) == 3 and len(_lib.SIGNATURES["nlg_linop_orbit_end"][1]) == 2
    # the Fortran shim binds the two entry points of the mode
    capi = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    for nm in NEW[:2]:
        assert 'name="%s"' % nm in capi


def test_orbit_wrappers_raise_without_a_device(lib):
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        pytest.skip("GPU present")
    from neklab_amd import host
    assert issubclass(host.exptA_orbit_linop, host.exptA_linop)
    assert callable(host.linear_stability_analysis_periodic_orbit)
    with pytest.raises(host.NlgError):
        host.Context(0)
    # NULL handles: an error code and a message, not a crash
    assert lib.nlg_linop_set_orbit(None, None, 1.0) != 0 and b"nlg_linop_set_orbit" in lib.nlg_last_error()
    assert lib.nlg_linop_orbit_end(None, None) != 0 and b"nlg_linop_orbit_end" in lib.nlg_last_error()
    with pytest.raises(host.NlgError, match="nlg_linop_set_orbit"):
        host.check(lib.nlg_linop_set_orbit(None, None, 1.0))
