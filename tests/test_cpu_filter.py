"""Explicit modal filter, CPU side: the 1-D matrix from its definition (tests/filter_ref.py), the cut-off rule of the .par reader,
the filtered oracle propagator, and the three hand-kept mirrors of nlg_exptA_config (C header, ctypes, Fortran bind(C))."""
import os
import re

import numpy as np
import pytest

from filter_ref import FilteredExptA, filter_matrix, modal_basis
from neklab_amd.mesh import box_mesh, gll_points
from oracle.lns import ExptA, LNSConfig
from oracle.sem import SEM
from oracle.vectors import NekDVector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, ncut, w) for n in (6, 8, 10, 12) for ncut in (1, 2, 3) for w in (0.01, 0.05, 1.0)]


@pytest.mark.parametrize("n,ncut,w", CASES)
def test_boundary_rows_are_unit_vectors(n, ncut, w):
    """face values are untouched: C0 continuity and Dirichlet values survive the element-local filter"""
    F = filter_matrix(n, ncut, w)
    e0, e1 = np.eye(n)[0], np.eye(n)[-1]
    assert np.max(np.abs(F[0] - e0)) < 1e-14 and np.max(np.abs(F[-1] - e1)) < 1e-14


@pytest.mark.parametrize("n,ncut,w", CASES)
def test_low_degree_polynomials_are_reproduced(n, ncut, w):
    F = filter_matrix(n, ncut, w)
    z = gll_points(n)
    for deg in range(n - ncut):                     # degree <= n - ncut - 1
        p = z ** deg
        assert np.max(np.abs(F @ p - p)) < 1e-13, deg


@pytest.mark.parametrize("n,ncut,w", CASES)
def test_top_mode_is_scaled_by_one_minus_weight(n, ncut, w):
    F = filter_matrix(n, ncut, w)
    phi_n = modal_basis(gll_points(n))[:, -1]
    assert np.max(np.abs(F @ phi_n - (1.0 - w) * phi_n)) < 1e-13


@pytest.mark.parametrize("n", [6, 8, 10, 12])
def test_full_weight_single_mode_is_a_projector(n):
    F = filter_matrix(n, 1, 1.0)
    assert np.max(np.abs(F @ F - F)) < 1e-13


def test_cutoff_rule_of_the_par_reader():
    from neklab_amd.host import filter_modes_from_cutoff_ratio as f
    assert {n: f(n, 0.84) for n in (6, 8, 10, 12)} == {6: 1, 8: 1, 10: 2, 12: 2}
    assert f(8, 1.0) == 1                           # never fewer than one mode
    assert f(10, 0.75) == 3                         # nint(2.5) = 3: half away from zero -> 3 - 1 + 1
    assert f(8, 0.5) == 4


def _tiny_case():
    hm = box_mesh((2, 2), 6, lengths=(2.0, 1.0), periodic=(True, False), deform=0.03)
    sem = SEM(hm)
    U = [sem.mask[0] * (4 * sem.X[1] * (1 - sem.X[1])), np.zeros(sem.shape1)]
    kw = dict(re=20.0, torder=2, tau=0.03, dt=0.01, vtol=1e-12, ptol=1e-12, maxit_v=200, maxit_p=2000)
    ov = NekDVector(sem)
    ov.rand(ifnorm=True, seed=2)
    return sem, U, kw, ov


def test_filtered_oracle_with_zero_weight_is_the_oracle():
    sem, U, kw, ov = _tiny_case()
    a = ExptA(sem, U, LNSConfig(**kw)).matvec(ov)
    b = FilteredExptA(sem, U, LNSConfig(**kw), filter_weight=0.0, filter_modes=1).matvec(ov)
    for i in range(2):
        assert np.array_equal(a.v[i], b.v[i])
        assert np.array_equal(a.v_rst[0][i], b.v_rst[0][i])
    assert np.array_equal(a.pr, b.pr)


def test_filtered_oracle_differs_with_weight():
    sem, U, kw, ov = _tiny_case()
    a = ExptA(sem, U, LNSConfig(**kw)).matvec(ov)
    b = FilteredExptA(sem, U, LNSConfig(**kw), filter_weight=0.05, filter_modes=1).matvec(ov)
    sc = max(np.abs(x).max() for x in a.v)
    assert max(np.abs(a.v[i] - b.v[i]).max() for i in range(2)) > 1e-6 * sc
    # the filter leaves the Dirichlet values alone (to the rounding of the boundary rows of Phi diag(d) Phi^-1: 1e-14 above)
    for i in range(2):
        assert np.max(np.abs(b.v[i] * (1 - sem.mask[i]))) < 1e-14 * sc


def test_config_mirrors_agree():
    """nlg_exptA_config is kept by hand in three places; the Fortran side passes its own copy by reference, so a shorter or reordered
    type there means the library reads the wrong bytes."""
    from neklab_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "neklab_gpu.h")).read()
    body = re.search(r"typedef struct nlg_exptA_config \{(.*?)\} nlg_exptA_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_names = [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    py_names = [f[0] for f in _lib.ExptAConfig._fields_]
    assert c_names == py_names
    assert c_names[-2:] == ["filter_weight", "filter_modes"]
    f90 = open(os.path.join(ROOT, "neklab_amd", "fortran", "neklab_gpu_capi.f90")).read()
    tbody = re.search(r"type, bind\(C\), public :: nlg_exptA_config\n(.*?)end type", f90, re.S).group(1)
    f_names = []
    for line in tbody.splitlines():
        line = line.split("!")[0]
        if "::" in line:
            for item in re.split(r",(?![^()]*\))", line.split("::")[1]):
                f_names.append(re.sub(r"\(.*\)", "", item.split("=")[0]).strip())
    assert f_names == c_names
