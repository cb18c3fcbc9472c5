"""tests/starmesh.py on the CPU: the meshes of irregular valence that tests/test_gpu_starmesh.py rests on are what they claim to be.

Copies per global dof (the table below), labels against labels built from coordinates alone, coincident coordinates, a positive
Jacobian, neighbours of differing orientation, and the float64 oracle on them: E = cdabdtp symmetric, the Schwarz preconditioner
symmetric and positive with and without overlap.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle.pprec import SchwarzPrec
from oracle.sem import SEM

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rotmesh import same_grouping  # noqa: E402
from starmesh import labels_from_coordinates, multiplicities, star_mesh  # noqa: E402

# (k, n, nz, periodic_z): copies per global dof -> number of such dofs, smallest Jacobian
TABLE = {
    (5, 6, 0, False): (15, {1: 280, 2: 110, 3: 5, 4: 5, 5: 1}, 0.100),
    (5, 8, 2, False): (30, {1: 8400, 2: 2840, 3: 70, 4: 230, 5: 14, 6: 5, 8: 5, 10: 1}, 0.050),
    (5, 5, 3, True): (45, {1: 1485, 2: 1260, 3: 45, 4: 300, 5: 9, 6: 15, 8: 15, 10: 3}, 0.050),
    (9, 5, 2, False): (54, {1: 2376, 2: 1521, 3: 72, 4: 225, 6: 9, 8: 9, 9: 8, 18: 1}, 0.018),
}
_cache = {}


def case(key):
    if key not in _cache:
        hm = star_mesh(*key)
        _cache[key] = (hm, SEM(hm))          # (SEM raises on a non-positive Jacobian)
    return _cache[key]


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "k%d_n%d_nz%d%s" % (k[0], k[1], k[2], "p" if k[3] else ""))
def test_multiplicities_labels_and_geometry(key):
    hm, sem = case(key)
    E, mult, jmin = TABLE[key]
    k, n, nz, per = key
    assert hm.E == E and hm.dim == (3 if nz else 2) and hm.x.shape == (E, n ** hm.dim)
    assert multiplicities(hm.glo_num) == mult
    if k == 9:
        assert mult[2] % 2 == 1              # an odd number of pairs: the odd-pair branch of k_gs
    # labels from the vertex ids group the points as their coordinates do
    assert same_grouping(hm.glo_num, labels_from_coordinates(hm, fold_z=float(nz) if per else None))
    # coincident points have equal coordinates (z of a periodic mesh: modulo the period)
    cs = [hm.x, hm.y] + ([hm.z % nz if per else hm.z] if hm.dim == 3 else [])
    g = hm.glo_num.ravel()
    for c in cs:
        c = c.ravel()
        lo = np.full(g.max() + 1, np.inf)
        hi = np.full(g.max() + 1, -np.inf)
        np.minimum.at(lo, g, c)
        np.maximum.at(hi, g, c)
        assert np.max(hi - lo) <= 1e-14
    assert sem.jac.min() > 0 and abs(sem.jac.min() - jmin) < 1e-3
    # masks: zero exactly on the faces without a partner -- bottom and top of a mesh that is not periodic, and the outer ring:
    # 2k sides of n - 1 points each per level, all of them beyond the fan (r > 1.85), none of them an irregular point
    zwall = np.zeros(hm.x.shape, dtype=bool)
    if hm.dim == 3 and not per:
        zwall = (hm.z == 0.0) | (hm.z == float(nz))
    held = hm.mask[0] == 0.0
    assert np.all(held[zwall])
    outer = held & ~zwall
    levels = 1 if hm.dim == 2 else (nz * (n - 1) if per else nz * (n - 1) - 1)
    assert len(np.unique(hm.glo_num[outer])) == 2 * k * (n - 1) * levels
    assert np.hypot(hm.x, hm.y)[outer].min() > 1.85
    assert np.all(np.bincount(g)[hm.glo_num[outer]] <= 4)
    assert all(np.array_equal(m, hm.tmask) and set(np.unique(m)) == {0.0, 1.0} for m in hm.mask) and not hm.has_outflow


def relative_orientations(hm):
    """per element: the set of in-plane rotations (quarter turns) of its neighbours against it.  Across my side i (corners listed
    counter-clockwise) an aligned neighbour, as in a structured mesh, has the shared side as its side i + 2."""
    ccw = hm.extra["vert"][:, [0, 1, 3, 2]]
    sides = {}
    for e, q in enumerate(ccw):
        for i in range(4):
            sides.setdefault((min(q[i], q[(i + 1) % 4]), max(q[i], q[(i + 1) % 4])), []).append((e, i))
    out = [set() for _ in range(hm.E)]
    for owners in sides.values():
        for (e, i) in owners:
            for (f, j) in owners:
                if f != e:
                    out[e].add((j - i - 2) % 4)
    return out


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "k%d_n%d_nz%d%s" % (k[0], k[1], k[2], "p" if k[3] else ""))
def test_neighbours_differ_in_orientation(key):
    hm, _ = case(key)
    rel = relative_orientations(hm)
    assert max(len(s) for s in rel) >= 2, rel
    assert any(0 not in s or len(s) > 1 for s in rel)


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "k%d_n%d_nz%d%s" % (k[0], k[1], k[2], "p" if k[3] else ""))
def test_oracle_operators_symmetric(key):
    """u . (E v) = v . (E u) and the same for the preconditioner M, u . (M u) > 0: the oracle assembles these meshes from their
    labels alone"""
    hm, sem = case(key)
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(sem.shape2), rng.standard_normal(sem.shape2)
    u, v = u - u.mean(), v - v.mean()
    Eu, Ev = sem.cdabdtp(u), sem.cdabdtp(v)
    sc = np.sqrt(np.sum(u * u) * np.sum(Ev * Ev))
    assert abs(np.sum(u * Ev) - np.sum(v * Eu)) <= 1e-13 * sc
    assert np.sum(u * Eu) > 0
    for ov in (0, 1):
        for wc in (0, 1):
            P = SchwarzPrec(sem, overlap=ov, with_coarse=wc)
            Mu, Mv = P.apply(u.ravel()), P.apply(v.ravel())
            sc = np.sqrt(np.sum(u * u) * np.sum(Mv * Mv))
            assert abs(np.sum(u.ravel() * Mv) - np.sum(v.ravel() * Mu)) <= 1e-13 * sc, (ov, wc)
            assert np.sum(u.ravel() * Mu) > 0 and np.sum(v.ravel() * Mv) > 0, (ov, wc)


@pytest.mark.parametrize("nz", [0, 1])
def test_oracle_pprec_matrix_symmetric_positive(nz):
    """the whole matrix on the smallest meshes: a 5-valent vertex in 2-D, 3- and 5-valent edges in one layer of 3-D"""
    sem = SEM(star_mesh(5, 6 if nz == 0 else 5, nz))
    for ov in (0, 1):
        for wc in (0, 1):
            P = SchwarzPrec(sem, overlap=ov, with_coarse=wc)
            M = np.stack([P.apply(e) for e in np.eye(sem.lpn)], axis=1)
            sc = np.abs(M).max()
            assert np.abs(M - M.T).max() < 1e-13 * sc, (ov, wc)
            lam = np.linalg.eigvalsh(0.5 * (M + M.T))
            assert lam.min() > -1e-12 * lam.max(), (ov, wc, lam.min())
            assert lam[1] > 1e-8 * lam.max()            # at most one (constant) null vector


def test_refusals():
    with pytest.raises(ValueError):
        star_mesh(5, 5, 2, periodic_z=True)      # vertex-based labels cannot tell the two vertical faces of four elements apart
    with pytest.raises(ValueError):
        star_mesh(5, 5, 1, periodic_z=True)
    with pytest.raises(ValueError):
        star_mesh(2, 5, 2)
    star_mesh(5, 4, 3, periodic_z=True)


@pytest.mark.slow
def test_longdouble_measurement_script_runs():
    """tests/starmesh_longdouble.py, whose output at 200 pressure iterations stands beside the bounds of
    test_gpu_starmesh.py::test_matvec_fixed_iterations, patches the oracle modules to long double: it must go on working when the oracle
    changes.  At 50 iterations (before conjugate gradients lose orthogonality on this mesh) the float64 oracle is within 1e-13 of its
    long-double evaluation; a patch that no longer reaches the oracle's arithmetic would print zeros."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "starmesh_longdouble.py"), "50"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"matvec #(\d): .*velocity (\S+) pressure (\S+) history (\S+)", r.stdout)
    assert len(rows) == 4, r.stdout
    for k, dv, dp, dh in rows:
        for d in (float(dv), float(dp), float(dh)):
            assert 0.0 < d < 1e-13, (k, dv, dp, dh)
