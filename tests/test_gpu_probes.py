"""History points on the GPU (nlg_probes_*, k_probe_sample; host.history_points) on the cases A (2-D, lx1 = 6) and B (3-D, lx1 = 8) of the
Floquet tests and on a 2 x 1 x 1 box at lx1 = 10 and 12.

Tolerances.  Sampling the mesh's own coordinates returns the point: 1e-12 x domain length, the bound of the location (tests/
test_cpu_probe_locate.py).  A field against the twin at the same (e, r): both sum n^dim products u w_i w_j w_k in different orders, each
product with three roundings, so the difference is below 4 n^dim eps sum|w| max|u|, computed per point from the twin's weights.
"""
import numpy as np
import pytest

import dns_ref
import floquet_ref as fr
from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_sem = {}


def case(name):
    if name in ("A", "B"):
        return fr.case_mesh(name)
    if name not in _sem:   # "N10", "N12": 2 x 1 x 1 deformed elements
        hm = box_mesh((2, 1, 1), int(name[1:]), lengths=(2.0, 1.0, 1.0), deform=0.04)
        _sem[name] = (hm, SEM(hm))
    return _sem[name]


def points(name, hm):
    if name in ("A", "B"):
        return np.array([p[1] for p in dns_ref.case_points(name, hm) if p[2] == 0])
    rng = np.random.default_rng(11)
    return np.array([dns_ref.map_point(hm, e, r) for e in range(hm.E) for r in list(rng.uniform(-1, 1, (3, 3))) + [np.array([1.0, 0.2, -1.0])]])


def random_vector(gm, sem, seed):
    rng = np.random.default_rng(seed)
    ov = NekDVector(sem)
    gv = host.nek_dvector(gm)
    for c in range(sem.dim):
        ov.v[c][...] = rng.standard_normal(sem.shape1)
        gv.set_field(c, ov.v[c])
    ov.pr[...] = rng.standard_normal(sem.shape2)
    gv.set_field(host.PR, ov.pr)
    return gv, ov


def local_elems(hm, hp):
    """single rank: the global element id of the winner -> its local index"""
    pos = {int(g): e for e, g in enumerate(hm.elem_gid)}
    return [pos[int(g)] for g in hp.elem]


def check_against_twin(name, gm, hm, sem, hp, seed):
    gv, ov = random_vector(gm, sem, seed)
    got = hp.sample(gv)
    elem = local_elems(hm, hp)
    ref = dns_ref.sample(sem, elem, hp.rst, ov)
    dim = sem.dim
    umax = max(np.abs(a).max() for a in ov.v)
    tol_v = 4 * sem.n ** dim * EPS * dns_ref.weight_sum(sem, hp.rst) * umax
    tol_p = 4 * sem.n2 ** dim * EPS * dns_ref.weight_sum(sem, hp.rst, mesh2=True) * np.abs(ov.pr).max()
    ev = np.abs(got[:, :dim] - ref[:, :dim]).max(axis=1)
    ep = np.abs(got[:, dim] - ref[:, dim])
    print("%s: velocity error / tolerance %s; pressure error / tolerance %s" % (name, ["%.2f" % a for a in ev / tol_v], ["%.2f" % a for a in ep / tol_p]))
    assert got.shape == (hp.npts, dim + 1)
    assert np.all(ev <= tol_v) and np.all(ep <= tol_p)


@pytest.mark.parametrize("name", ["A", "B", "N10", "N12"])
def test_sampling_the_coordinates_returns_the_point(gpu_ctx, name):
    hm, sem = case(name)
    gm = host.Mesh(gpu_ctx, hm)
    xyz = points(name, hm)
    hp = host.history_points(gm, xyz)
    assert np.all(hp.status == 0)
    gv = host.nek_dvector(gm)
    for c, X in enumerate([hm.x, hm.y] + ([hm.z] if hm.dim == 3 else [])):
        gv.set_field(c, X)
    got = hp.sample(gv)[:, :hm.dim]
    err = np.abs(got - xyz).max()
    print("%s: %d points, max |sampled coordinates - point| = %.3e" % (name, hp.npts, err))
    assert err <= 1e-12 * max(hm.lengths)
    hp.close()


@pytest.mark.parametrize("name", ["A", "B", "N10", "N12"])
def test_random_fields_and_pressure_against_the_twin(gpu_ctx, name):
    hm, sem = case(name)
    gm = host.Mesh(gpu_ctx, hm)
    hp = host.history_points(gm, points(name, hm))
    check_against_twin(name, gm, hm, sem, hp, seed=3)
    hp.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_point_at_a_node_returns_the_nodal_value(gpu_ctx, name):
    hm, sem = case(name)
    gm = host.Mesh(gpu_ctx, hm)
    n, dim = hm.n, hm.dim
    nodes = [(4, (2, 4)), (0, (0, 0)), (7, (n - 1, 3))] if dim == 2 else [(6, (2, 5, 3)), (0, (0, 0, 0)), (7, (n - 1, 3, 1))]
    C = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
    flat = lambda idx: sum(i * n ** d for d, i in enumerate(idx))       # (ix, iy[, iz]) -> position in the element
    xyz = np.array([[c[e, flat(idx)] for c in C] for e, idx in nodes])
    hp = host.history_points(gm, xyz)
    gv, ov = random_vector(gm, sem, seed=8)
    got = hp.sample(gv)
    for q, (e, idx) in enumerate(nodes):
        el = local_elems(hm, hp)[q]
        # (a node on an element boundary may be won by a neighbour with a smaller id: the nodal value of the winner then)
        hit = int(np.argmin(sum((c[el] - xyz[q, k]) ** 2 for k, c in enumerate(C))))
        for c in range(dim):
            assert got[q, c] == ov.v[c][el].reshape(-1)[hit], (q, c)
    hp.close()


def test_one_to_four_vectors_equal_the_single_calls(gpu_ctx):
    hm, sem = case("B")
    gm = host.Mesh(gpu_ctx, hm)
    hp = host.history_points(gm, points("B", hm))
    vecs = [random_vector(gm, sem, seed=20 + k)[0] for k in range(4)]
    single = [hp.sample(v) for v in vecs]
    for s in range(1, 5):
        got = hp.sample(vecs[:s])
        assert got.shape == (s, hp.npts, 4)
        for k in range(s):
            assert np.array_equal(got[k], single[k]), (s, k)
    assert np.array_equal(hp.sample(vecs[2]), single[2])               # run to run
    hp.close()


def test_a_point_in_no_element_is_refused(gpu_ctx):
    hm, sem = case("A")
    gm = host.Mesh(gpu_ctx, hm)
    with pytest.raises(host.NlgError, match="status 2"):
        host.history_points(gm, np.array([[0.5, 0.5], [-0.2, 0.5]]))
    with pytest.raises(host.NlgError):
        host.history_points(gm, np.zeros((0, 2)))
