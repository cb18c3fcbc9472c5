"""CPU suite: the host side of a DNS run's series -- history-point files (nekio.read_his / write_his), the two period estimators
(host.recurrence_period, host.probe_period) and the Lagrange evaluation of the reference twin (tests/dns_ref.py).

Bound on the recurrence period of d(t) = |2 sin(pi t / T)|: d^2 = 4 sin^2 is a parabola about t = T up to the relative term
(pi (t - T) / T)^2 / 3, which three samples a step dt apart see as a shift of the vertex of at most dt (pi dt / T)^2.
"""
import os

import numpy as np
import pytest

import dns_ref
from neklab_amd import nekio
from neklab_amd.mesh import box_mesh

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import host
    return host


def test_read_his_reads_the_reference_file():
    his = nekio.read_his(os.path.join(HERE, "golden", "reference_1cyl.his"))
    assert np.array_equal(his["xyz"], [[1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [2.0, 0.5], [2.0, -0.5]])
    assert his["time"].shape == (0,) and his["probe"].shape[:2] == (0, 5)


def test_his_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    xyz = rng.standard_normal((4, 3))
    time = 0.01 * np.arange(7)
    probe = rng.standard_normal((7, 4, 4)) * 10.0 ** rng.integers(-9, 9, (7, 4, 4))
    path = str(tmp_path / "run.his")
    nekio.write_his(path, xyz, time, probe)
    lines = open(path).read().splitlines()
    assert lines[0].strip() == "4" and len(lines) == 1 + 4 + 7 * 4 and all(len(ln) == 15 * 5 for ln in lines[5:])
    back = nekio.read_his(path)
    # 1pE15.7: eight significant digits
    assert np.allclose(back["xyz"], xyz, rtol=5e-8, atol=0.0)
    assert np.allclose(back["time"], time, rtol=5e-8, atol=0.0)
    assert back["probe"].shape == probe.shape and np.allclose(back["probe"], probe, rtol=5e-8, atol=0.0)
    with open(path, "a") as f:
        f.write("  1.0  2.0  3.0  4.0  5.0\n")
    with pytest.raises(ValueError):
        nekio.read_his(path)


def test_recurrence_period_exact_on_a_parabola(host):
    for T, c, dt in ((1.234, 0.3, 0.013), (5.158, 1e-3, 0.05), (0.7371, 0.0, 0.0075)):
        t = np.arange(0.0, 2.0 * T, dt)
        got = host.recurrence_period(t, np.sqrt((t - T) ** 2 + c))
        assert got is not None and abs(got[0] - T) <= 1e-12, (T, got)


@pytest.mark.parametrize("T", [1.0, 0.7371, 5.158])
@pytest.mark.parametrize("dt", [0.0075, 0.008, 0.01, 0.05])
def test_recurrence_period_of_a_periodic_signal(host, T, dt):
    t = np.arange(0.0, 1.6 * T, dt)
    d = np.abs(2.0 * np.sin(np.pi * t / T))
    Tg, depth = host.recurrence_period(t, d)
    print("T = %g dt = %g: error %.3e, bound %.3e, depth %.3e" % (T, dt, abs(Tg - T), dt * (np.pi * dt / T) ** 2, depth))
    assert abs(Tg - T) <= dt * (np.pi * dt / T) ** 2
    assert depth <= np.pi * dt / T              # the minimum lies within half a step of the zero of d


def test_recurrence_period_none_on_a_monotone_signal(host):
    t = np.linspace(0.0, 3.0, 200)
    assert host.recurrence_period(t, t) is None
    assert host.recurrence_period(t, 3.0 - t) is None
    # a dip that is not deep enough is no recurrence
    assert host.recurrence_period(t, 2.0 + 0.1 * np.cos(4.0 * t)) is None


def test_probe_period_of_a_sine_with_an_offset(host):
    t = np.arange(0.0, 5.0, 0.013)
    for T in (0.61, 1.7):
        got = host.probe_period(t, 0.7 + np.sin(2.0 * np.pi * t / T + 0.3))
        # the mean over a non-integer number of periods shifts the zero level by O(T / span); linear interpolation adds O(dt^2)
        assert abs(got - T) <= 1e-3 * T, (T, got)
    assert host.probe_period(t, t) is None


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 8), (3, 10)])
def test_twin_sampling_is_exact_for_polynomials(dim, n):
    """a polynomial of degree <= N in every coordinate on the undeformed box is its own interpolant"""
    hm = box_mesh((2,) * dim, n, lengths=(2.0, 1.0, 1.0)[:dim], deform=0.0)
    N = n - 1
    C = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
    poly = lambda X: sum((0.3 + d) * X[d] ** N - 0.7 * X[d] ** (N - 2) + X[d] for d in range(dim)) + X[0] ** N * X[1] ** N
    f = poly(C).reshape((hm.E,) + (n,) * dim)
    z = dns_ref.gll_points(n)
    rng = np.random.default_rng(2)
    for e in range(hm.E):
        for r in list(rng.uniform(-1.0, 1.0, (3, dim))) + [np.array([1.0, -1.0, z[2]][:dim])]:
            xs = dns_ref.map_point(hm, e, r)
            assert abs(dns_ref.evaluate(f[e], z, r) - poly(list(xs))) <= 1e-12
