"""CPU suite: point location of the history points (nlg_probe_locate, neklab_amd/csrc/probe_host.cpp) through ctypes, against the numpy
twin of tests/dns_ref.py: status, the winner among several holders (smallest global element id), |x_e(r) - x*|, the reference's curved
cylinder mesh with the five points of its 1cyl.his, independence of the partition, and the same code as a stand-alone program under
AddressSanitizer / UBSan (tests/cpp/probe_host_main.cpp; nothing is loaded into Python under a sanitizer).

Bound on |x_e(r) - x*|: the Newton stop 1e-13 in r times the Jacobian scale (at most half the domain length per unit r) -> 1e-12 L.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dns_ref
from dns_ref import case_points, mesh_of
from neklab_amd import nekio
from neklab_amd.mesh import box_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "neklab_amd", "csrc")


def _cxx():
    """ROCm's clang++ (beside the hipcc that builds the library), else the system's c++"""
    cands = []
    for hipcc in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if hipcc and os.path.exists(hipcc):
            rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
            cands += [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")]
    cands += [shutil.which("amdclang++"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler found (neither ROCm's clang++ nor c++)")


@pytest.fixture(scope="module")
def host():
    from neklab_amd import build
    build.build_library()
    from neklab_amd import host
    return host


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_locate_on_boxes(host, name):
    hm = mesh_of(name)
    pts = case_points(name, hm)
    xyz = np.array([p[1] for p in pts])
    got = host.locate_points(hm, xyz)
    L = max(hm.lengths)
    for q, (label, xs, status, nhold) in enumerate(pts):
        assert got["status"][q] == status, (label, got["status"][q])
        twin = dns_ref.holders(hm, xs)
        assert len(twin) == nhold, (label, [h[0] for h in twin])
        if status == 2:
            assert got["elem"][q] == -1
            continue
        e = int(got["elem"][q])
        assert int(hm.elem_gid[e]) == twin[0][0], (label, e, [h[0] for h in twin])     # the smallest global id among the holders
        r = got["rst"][q]
        assert np.max(np.abs(r)) <= 1.0
        err = np.linalg.norm(dns_ref.map_point(hm, e, r) - xs)
        print("%s %-14s elem %d r %s |x_e(r) - x*| = %.2e (dist %.2e)" % (name, label, e, r, err, got["dist"][q]))
        assert err <= 1e-12 * L and got["dist"][q] <= 1e-12 * L, (label, err)
        assert np.max(np.abs(r - twin[0][2])) <= 1e-11, (label, r, twin[0][2])          # same element: the same r as the twin


def test_node_returns_the_node_exactly(host):
    """a point at a GLL node: r is the node bit for bit (the weights are then exactly one and zero)"""
    hm = mesh_of("B")
    z = dns_ref.gll_points(hm.n)
    idx = (2, 5, 3)
    e = 6
    xs = np.array([c[e].reshape(hm.n, hm.n, hm.n)[idx[2], idx[1], idx[0]] for c in (hm.x, hm.y, hm.z)])
    got = host.locate_points(hm, xs[None])
    assert got["status"][0] == 0 and got["elem"][0] == e
    assert np.max(np.abs(got["rst"][0] - z[list(idx)])) <= 1e-15


def test_cylinder_mesh_and_its_his_points(host):
    from refdata import load_cylinder
    hm = load_cylinder(geometry="re2")[0]
    his = nekio.read_his(os.path.join(HERE, "golden", "reference_1cyl.his"))
    assert his["xyz"].shape == (5, 2)
    circle = np.array([0.5 * np.cos(0.3), 0.5 * np.sin(0.3)])
    xyz = np.vstack([his["xyz"], [[0.0, 0.0]], circle[None]])
    got = host.locate_points(hm, xyz)
    assert list(got["status"][:5]) == [0] * 5, got["status"]
    for q in range(5):
        e = int(got["elem"][q])
        assert np.linalg.norm(dns_ref.map_point(hm, e, got["rst"][q]) - xyz[q]) <= 1e-12 * 66.0     # the domain is 66 long
        twin = dns_ref.holders(hm, xyz[q])
        assert twin and twin[0][0] == int(hm.elem_gid[e]), (q, e, [h[0] for h in twin])
        if abs(xyz[q, 1]) == 0.0:
            assert len(twin) == 2, (q, [h[0] for h in twin])       # the wake centre line is an element interface
    assert got["status"][5] == 2 and got["elem"][5] == -1              # inside the cylinder
    assert got["status"][6] == 2                                      # on the true circle: the degree-5 side is not the circle
    tol_r = 1e-3
    wide = host.locate_points(hm, circle[None], tol_r=tol_r)
    assert wide["status"][0] == 1
    e = int(wide["elem"][0])
    extent = max(np.ptp(hm.x[e]), np.ptp(hm.y[e]))
    print("circle point: elem %d r %s dist %.3e (extent %.3e)" % (e, wide["rst"][0], wide["dist"][0], extent))
    assert np.max(np.abs(wide["rst"][0])) == 1.0 and 0.0 < wide["dist"][0] <= tol_r * extent
    assert abs(np.linalg.norm(dns_ref.map_point(hm, e, wide["rst"][0]) - circle) - wide["dist"][0]) <= 1e-14


def test_winner_does_not_depend_on_the_partition(host):
    hm = mesh_of("B")
    pts = [p for p in case_points("B", hm) if p[2] == 0]
    xyz = np.array([p[1] for p in pts])
    whole = host.locate_points(hm, xyz)
    for parts in ([np.arange(0, 4), np.arange(4, 8)], [np.array([0, 3, 5]), np.array([1, 2, 7]), np.array([4, 6])]):
        best = np.full(len(pts), np.iinfo(np.int64).max)
        for elems in parts:
            sub = hm.take(elems)
            got = host.locate_points(sub, xyz)
            for q in range(len(pts)):
                if got["status"][q] == 0:
                    best[q] = min(best[q], int(sub.elem_gid[got["elem"][q]]))
        assert np.array_equal(best, hm.elem_gid[whole["elem"]]), (best, hm.elem_gid[whole["elem"]])


def test_standalone_program_under_sanitizers(host, tmp_path):
    """probe_host.cpp with its own main, built with -fsanitize=address,undefined and run on case A and a small 3-D mesh: it must end
    clean and return what the library returns"""
    exe = str(tmp_path / "probe_host_main")
    cmd = [_cxx(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "probe_host_main.cpp"), os.path.join(CSRC, "probe_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    small = box_mesh((2, 1, 2), 5, lengths=(1.0, 0.5, 1.0), deform=0.04)
    for hm, pts in ((mesh_of("A"), case_points("A", mesh_of("A"))),
                    (small, [("in", dns_ref.map_point(small, 2, (0.1, -0.2, 0.7)), 0, 1), ("face", dns_ref.map_point(small, 0, (1.0, 0.2, 0.1)), 0, 2),
                             ("out", np.array([3.0, 0.1, 0.1]), 2, 0)])):
        xyz = np.array([p[1] for p in pts])
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<4q", hm.dim, hm.n, hm.E, len(xyz)))
            f.write(struct.pack("<d", 1e-10))
            for c in [hm.x, hm.y] + ([hm.z] if hm.dim == 3 else []):
                f.write(np.ascontiguousarray(c, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(hm.elem_gid, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(xyz, dtype="<f8").tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, "probe_host_main failed (%d): %s" % (r.returncode, r.stderr[-3000:])
        raw = open(fout, "rb").read()
        npts, dim = len(xyz), hm.dim
        elem = np.frombuffer(raw, "<i8", npts, 0)
        rst = np.frombuffer(raw, "<f8", npts * dim, 8 * npts).reshape(npts, dim)
        status = np.frombuffer(raw, "<i4", npts, 8 * npts * (1 + dim))
        w = np.frombuffer(raw, "<f8", npts * dim * hm.n, 8 * npts * (2 + dim) + 4 * npts).reshape(npts, dim, hm.n)
        got = host.locate_points(hm, xyz)
        assert np.array_equal(elem, got["elem"]) and np.array_equal(status, got["status"]) and list(status) == [p[2] for p in pts]
        assert np.max(np.abs(rst - got["rst"])) <= 1e-14     # (the two builds differ in optimisation level and contraction)
        for q in range(npts):
            if status[q] == 0:                                # barycentric weights against the twin's product form
                for d in range(dim):
                    assert np.max(np.abs(w[q, d] - dns_ref.lagrange(dns_ref.gll_points(hm.n), rst[q, d])[0])) <= 1e-13
