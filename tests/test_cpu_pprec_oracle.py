"""oracle/pprec.py (the two-level Schwarz preconditioner restated from its definition) and the rotated-element meshes of
tests/rotmesh.py, on the CPU.

* the rotated mesh's labels group the points exactly as Nek5000's numbering from the corner vertex ids does
  (nekio.glo_num_from_vertices);
* every oracle operator is equivariant under element rotation: on the rotated mesh with the re-indexed input it gives the
  aligned mesh's result, re-indexed (geometry, gs, axhelm, opdiv, opgradt, cdabdtp, lns_conv_weak, pprec);
* the preconditioner is symmetric positive (semi-)definite on a deformed mesh;
* on one undeformed element, without overlap and coarse level, it is the exact (pseudo-)inverse of E, which is separable there.
"""
import os
import sys

import numpy as np
import pytest

from neklab_amd.mesh import box_mesh
from oracle.pprec import SchwarzPrec, overlap_available
from oracle.sem import SEM

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rotmesh import Rotated, proper_rotations, same_grouping, source_index  # noqa: E402

MESHES = {
    3: dict(nel=(3, 2, 2), n=6, periodic=(True, False, False)),
    2: dict(nel=(4, 3), n=6, periodic=(True, False)),
}


def mesh(dim, **kw):
    a = dict(MESHES[dim])
    a.update(kw)
    return box_mesh(a.pop("nel"), a.pop("n"), deform=a.pop("deform", 0.05), **a)


def test_proper_rotations_are_the_cube_group():
    for dim, cnt in ((3, 24), (2, 4)):
        rots = proper_rotations(dim)
        assert len(rots) == cnt
        srcs = {tuple(source_index(4, dim, *r)) for r in rots}
        assert len(srcs) == cnt                      # all distinct permutations of the points


@pytest.mark.parametrize("dim", [3, 2])
def test_rotated_labels_group_like_nek_numbering(dim):
    for kw in (dict(), dict(periodic=(True,) * dim, nel=(3,) * dim), dict(outflow_xmax=True)):
        R = Rotated(mesh(dim, **kw), seed=4)
        assert any(r is not None and r != proper_rotations(dim)[0] for r in R.rot)
        assert same_grouping(R.mesh.glo_num, R.labels_from_vertices())
        assert same_grouping(R.aligned.glo_num, Rotated(R.aligned, elems=[]).labels_from_vertices())
        # a rotated mesh labelled from its vertices alone describes the same operator
        hm2 = Rotated(R.aligned, seed=4).mesh
        hm2.glo_num = R.labels_from_vertices()
        r = np.random.default_rng(0).standard_normal(SEM(hm2).lpn)
        assert np.allclose(SEM(hm2).cdabdtp(r), SEM(R.mesh).cdabdtp(r), rtol=0, atol=1e-13 * np.abs(SEM(R.mesh).cdabdtp(r)).max())


def _err(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("kind", ["walls", "periodic", "outflow"])
def test_oracle_operators_equivariant_under_rotation(dim, kind):
    kw = {"walls": dict(periodic=(False,) * dim), "periodic": dict(periodic=(True,) * dim), "outflow": dict(outflow_xmax=True)}[kind]
    hm = mesh(dim, **kw)
    R = Rotated(hm, seed=9)
    s0, s1 = SEM(hm), SEM(R.mesh)          # (SEM raises on a non-positive Jacobian)
    f1 = lambda a: R.fwd1(np.asarray(a).reshape(hm.E, -1)).reshape(s0.shape1)   # noqa: E731
    f2 = lambda a: R.fwd2(np.asarray(a).reshape(hm.E, -1)).reshape(s0.shape2)   # noqa: E731
    rng = np.random.default_rng(1)
    u = [s0.mask[i] * rng.standard_normal(s0.shape1) for i in range(dim)]
    U = [s0.mask[i] * (1.0 + 0.3 * np.sin(s0.X[0] + i)) for i in range(dim)]
    p = rng.standard_normal(s0.shape2)
    u1, U1, p1 = [f1(a) for a in u], [f1(a) for a in U], f2(p)
    tol = 1e-13
    for a, b in ((s0.bm1, s1.bm1), (s0.jac, s1.jac), (s0.binvm1, s1.binvm1), (s0.mult, s1.mult), (s0.bm2, s1.bm2)):
        assert _err(b, f2(a) if a.shape == s0.shape2 else f1(a)) < tol
    assert _err(s1.gs(u1[0]), f1(s0.gs(u[0]))) < tol
    assert _err(s1.axhelm_local(u1[0], 0.7, 3.0), f1(s0.axhelm_local(u[0], 0.7, 3.0))) < tol
    assert _err(s1.opdiv(u1), f2(s0.opdiv(u))) < tol
    for a, b in zip(s1.opgradt(p1), s0.opgradt(p)):
        assert _err(a, f1(b)) < tol
    assert _err(s1.cdabdtp(p1), f2(s0.cdabdtp(p))) < tol
    assert _err(s1.e_diag(), f2(s0.e_diag())) < tol
    for adj in (False, True):
        for a, b in zip(s1.lns_conv_weak(U1, u1, adjoint=adj), s0.lns_conv_weak(U, u, adjoint=adj)):
            assert _err(a, f1(b)) < tol
    # (with an outflow face the coarse operator has no shift and a weakly anchored near-constant mode: its inverse
    # amplifies rounding about tenfold)
    tolc = 1e-12 if kind == "outflow" else tol
    for ov in (0, 1):
        for wc in (0, 1):
            z0 = SchwarzPrec(s0, overlap=ov, with_coarse=wc).apply(p)
            z1 = SchwarzPrec(s1, overlap=ov, with_coarse=wc).apply(p1)
            assert _err(z1, f2(z0)) < (tolc if wc else tol), (ov, wc)
    for ov in (0, 1):   # the aggregated coarse mode (vertex order and element order are the same on both meshes)
        z0 = SchwarzPrec(s0, overlap=ov, exact_max=4).apply(p)
        z1 = SchwarzPrec(s1, overlap=ov, exact_max=4).apply(p1)
        assert _err(z1, f2(z0)) < tolc, ov


@pytest.mark.parametrize("dim", [3, 2])
def test_oracle_pprec_symmetric_positive(dim):
    hm = Rotated(mesh(dim, nel=(2, 2, 2)[:dim], periodic=(True,) + (False,) * (dim - 1), deform=0.08), seed=3).mesh
    sem = SEM(hm)
    for ov in (0, 1):
        for wc, emax in ((0, 2048), (1, 2048), (1, 4)):
            P = SchwarzPrec(sem, overlap=ov, with_coarse=wc, exact_max=emax)
            M = np.stack([P.apply(e) for e in np.eye(sem.lpn)], axis=1)
            sc = np.abs(M).max()
            assert np.abs(M - M.T).max() < 1e-13 * sc, (ov, wc, emax)
            lam = np.linalg.eigvalsh(0.5 * (M + M.T))
            assert lam.min() > -1e-12 * lam.max(), (ov, wc, emax, lam.min())
            assert lam[1] > 1e-8 * lam.max()            # at most one (constant) null vector


@pytest.mark.parametrize("dim,n", [(3, 6), (3, 8), (2, 7)])
@pytest.mark.parametrize("outflow", [False, True])
def test_oracle_pprec_exact_on_one_element(dim, n, outflow):
    """One undeformed box element: E is the separable operator itself.  With an outflow face it is invertible and M = E^-1;
    with walls only the constants are its null space and M is a reflexive generalised inverse (E M E = E, M E M = M)."""
    hm = box_mesh((1,) * dim, n, lengths=(2.0, 0.7, 1.3)[:dim], deform=0.0, outflow_xmax=outflow)
    sem = SEM(hm)
    Emat = np.stack([sem.cdabdtp(e).ravel() for e in np.eye(sem.lpn)], axis=1)
    M = np.stack([SchwarzPrec(sem, overlap=False, with_coarse=False).apply(e) for e in np.eye(sem.lpn)], axis=1)
    if outflow:
        assert _err(M, np.linalg.inv(Emat)) < 1e-11
    else:
        assert _err(Emat @ M @ Emat, Emat) < 1e-12
        assert _err(M @ Emat @ M, M) < 1e-12
        assert np.linalg.matrix_rank(M, tol=1e-10 * np.abs(M).max()) == sem.lpn - 1


def test_oracle_pprec_overlap_availability():
    assert [n for n in range(4, 14) if overlap_available(3, n)] == [4, 5, 6, 7, 8, 9, 10, 12]
    assert [n for n in range(4, 14) if overlap_available(2, n)] == [4, 5, 6, 7, 8]
    with pytest.raises(ValueError):
        SchwarzPrec(SEM(box_mesh((2, 1, 1), 11)), overlap=True)
    with pytest.raises(ValueError):   # no shared face
        SchwarzPrec(SEM(box_mesh((1, 1, 1), 6)), overlap=True)
