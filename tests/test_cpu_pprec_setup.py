"""The host stages of the pressure preconditioner's set-up (neklab_amd/csrc/pprec_host.cpp) against oracle/pprec.py, stage
by stage and without a GPU: tests/cpp/pprec_host_main.cpp is compiled with the host C++ compiler, reads a mesh from a flat
binary file, runs the stages and writes their outputs back.

Compared per mesh (1e-12 relative, the tolerance of tests/test_gpu_pprec_oracle.py for this preconditioner against this
oracle; integers exactly): edge lengths and end-point factors; the local solve with the program's tables in the oracle's
formula, without and with overlap (eigenvector signs and order are free, so the operator is compared, not the tables);
has_nb; the overlap destinations against the oracle's ghost map; vg, nvert and the vertex-to-element CSR; the colouring;
the aggregates, 1 / diag and P^T A_c P (+ shift) from the oracle's A_c.
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from neklab_amd.mesh import box_mesh
from oracle.pprec import SchwarzPrec, _den
from oracle.sem import SEM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "neklab_amd", "csrc")
sys.path.insert(0, HERE)
from rotmesh import Rotated  # noqa: E402

TOL = 1e-12
# (elements, lx1, box_mesh keywords, rotated elements, exact_max): the last two are the aggregated cases 3 and 1 of
# tests/test_gpu_pprec_oracle.py (AGG_CASES, NLG_COARSE_EXACT_MAX = 16)
SHAPES = {
    "3d_walls": ((3, 2, 2), 6, dict(), False, 2048),
    "3d_self": ((3, 1, 2), 6, dict(periodic=(False, True, False)), False, 2048),   # an element is its own neighbour
    "2d_outflow": ((4, 3), 6, dict(outflow_xmax=True), False, 2048),
    "2d_agg": ((6, 5), 8, dict(), True, 16),
    "3d_agg_periodic": ((4, 4, 4), 6, dict(periodic=(True, True, True)), False, 16),
}


def _cxx():
    """ROCm's clang++ (beside the hipcc that builds the library), else the system's c++."""
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
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pprec_host") / "pprec_host_main")
    cmd = [_cxx(), "-O2", "-std=c++17", "-I" + CSRC, os.path.join(HERE, "cpp", "pprec_host_main.cpp"),
           os.path.join(CSRC, "pprec_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def run_program(exe, td, sem, hw=None, pairs=None, coo=None, exact_max=2048):
    dim = sem.dim
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    ncoo = 0 if coo is None else len(coo[0])
    with open(fin, "wb") as f:
        f.write(struct.pack("<8q", dim, sem.n, sem.E, int(sem.has_outflow), int(hw is not None), 0 if pairs is None else len(pairs),
                            ncoo, exact_max))
        for a in [sem.X[c] for c in range(dim)] + [sem.mask[c] for c in range(dim)] + [sem.vmult, sem.w1, sem.w2, sem.z2, sem.D12, sem.I12]:
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(sem.glo, dtype="<i8").tobytes())
        if hw is not None:
            f.write(np.ascontiguousarray(hw, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(pairs, dtype="<i4").tobytes())
        if ncoo:
            f.write(np.ascontiguousarray(coo[0], dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(coo[1], dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(coo[2], dtype="<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, "pprec_host_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    out = {}
    raw = open(fout, "rb").read()
    pos = 0
    while pos < len(raw):
        name = raw[pos: pos + 16].rstrip(b"\0").decode()
        kind, count = struct.unpack_from("<2q", raw, pos + 16)
        dt = ("<f8", "<i4", "i1")[kind]
        out[name] = np.frombuffer(raw, dtype=dt, count=count, offset=pos + 32).copy()
        pos += 32 + count * np.dtype(dt).itemsize
    return out


def two_copy_groups(glo):
    """The groups of exactly two local points with one label, natural indices."""
    order = np.argsort(glo, kind="stable")
    srt = glo[order]
    first = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
    size = np.diff(np.r_[first, len(srt)])
    f2 = first[size == 2]
    return np.stack([order[f2], order[f2 + 1]], axis=1)


def relerr(a, b):
    return float(np.max(np.abs(np.ravel(a) - np.ravel(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_host_stages_match_oracle(program, tmp_path, shape):
    nel, n, kw, rot, exact_max = SHAPES[shape]
    hm = box_mesh(nel, n, deform=0.05, **kw)
    if rot:
        hm = Rotated(hm, seed=5).mesh
    sem = SEM(hm)
    dim, E, n2, np2 = sem.dim, sem.E, sem.n2, sem.n2 ** sem.dim
    NP, NC = n ** dim, 1 << dim
    r = np.random.default_rng(3).standard_normal(sem.lpn)
    P0 = SchwarzPrec(sem, overlap=False, with_coarse=True, exact_max=exact_max)
    P1 = SchwarzPrec(sem, overlap=True, with_coarse=False)
    z0, z1 = P0.local(r), P1.local(r)
    Ac = P0.Ac
    if exact_max < 2048:   # a tie could pass as a match
        assert P0.na < P0.nvert and not P0.ambiguous, "%s does not test the aggregated mode" % shape
    else:
        assert P0.na == P0.nvert

    # first run: the stages before the gather-scatter, and the face-length field it sums
    td = str(tmp_path)
    first = run_program(program, td, sem)
    hw = sem.gs(first["face_len"].reshape(sem.shape1))
    rows, cols = np.nonzero(Ac)
    out = run_program(program, td, sem, hw=hw, pairs=two_copy_groups(sem.glo), coo=(rows, cols, Ac[rows, cols]), exact_max=exact_max)
    for k in first:
        assert np.array_equal(first[k], out[k]), k

    # ---- edge lengths and end-point factors
    assert relerr(out["Lall"].reshape(E, 3)[:, :dim], P0.L) <= TOL
    assert relerr(out["endfac"].reshape(E, 3, 2)[:, :dim], P0.endfac) <= TOL

    # ---- local solve, no overlap: the program's S / invden in the oracle's formula
    P0.S = out["S"].reshape(E, 3, n2, n2)[:, :dim]
    P0.invden = out["invden"].reshape(sem.shape2)
    err = relerr(P0.local(r), z0)
    print("%s local solve: %.2e" % (shape, err))
    assert err <= TOL

    # ---- has_nb, and the local solve with overlap: invden rebuilt from lamx and thrx the way the kernels do it
    assert np.array_equal(out["hasnb"].reshape(E, 3, 2)[:, :dim].astype(bool), P1.has_nb)
    lamx, thrx = out["lamx"].reshape(E, 3, n)[:, :dim], out["thrx"][0]
    den = np.stack([_den(lamx[e], dim) for e in range(E)])
    P1.Sx = out["Sx"].reshape(E, 3, n, n)[:, :dim]
    P1.invden = np.where(den > thrx, 1.0 / np.where(den > thrx, den, 1.0), 0.0)
    P1.wq = out["wq"]
    err = relerr(P1.local(r), z1)
    print("%s local solve with overlap: %.2e" % (shape, err))
    assert err <= TOL

    # ---- overlap destinations: the layer of e next to its face point k goes to the ghost point that the oracle fills from it
    F = n2 ** (dim - 1)
    pin, pret = out["pin"].reshape(E, 2 * dim * F), out["pret"].reshape(E, 2 * dim * F)
    assert np.array_equal(pin >= 0, np.repeat(P1.has_nb.reshape(E, 2 * dim), F, axis=1))
    assert np.array_equal(pret >= 0, pin >= 0) and (dim == 3 or np.array_equal(pret, pin))
    for e in range(E):
        for k in range(2 * dim * F):
            if pin[e, k] < 0:
                continue
            dd, side, u, v = k // F // 2, (k // F) & 1, k % n2, (k % F) // n2
            abc = [u, v]
            abc.insert(dd, n2 - 1 if side else 0)
            gq = e * np2 + abc[0] + n2 * (abc[1] + (n2 * abc[2] if dim == 3 else 0))
            assert P1.ghost[pin[e, k] // NP, pin[e, k] % NP] == gq, (e, k)
    assert np.count_nonzero(pin >= 0) == np.count_nonzero(P1.ghost >= 0) - E * np2

    # ---- coarse topology
    vg = out["vg"].reshape(E, NC)
    assert out["nvert"][0] == P0.nvert and np.array_equal(vg, P0.vg)
    vp, vi = out["vp"], out["vi"]
    assert vp[0] == 0 and vp[-1] == E * NC and len(vp) == P0.nvert + 1
    for v in range(P0.nvert):
        assert np.array_equal(np.sort(vi[vp[v]: vp[v + 1]]), np.flatnonzero(vg.ravel() == v))
    share = np.zeros((E, P0.nvert), dtype=np.int64)
    share[np.repeat(np.arange(E), NC), vg.ravel()] = 1
    adj = (share @ share.T) > 0                          # share a vertex (an element is adjacent to itself)
    adjp, adji = out["adjp"], out["adji"]
    for e in range(E):
        assert np.array_equal(adji[adjp[e]: adjp[e + 1]], np.flatnonzero(adj[e]))
    common = (adj.astype(np.int64) @ adj.astype(np.int64)) > 0   # have a common neighbour
    colour = out["colour"]
    assert colour.min() == 0 and colour.max() == out["ncol"][0] - 1
    same = (colour[:, None] == colour[None, :]) & ~np.eye(E, dtype=bool)
    assert not np.any(same & common), "two elements of one colour share a neighbour"

    # ---- coarse-operator rows, aggregates, aggregate-level operator
    assert np.array_equal(out["rp"], np.r_[0, np.cumsum(np.count_nonzero(Ac, axis=1))]) and np.array_equal(out["ci"], cols)
    assert relerr(out["av"], Ac[rows, cols]) <= TOL and relerr(out["dinv"], P0.dinv) <= TOL
    assert np.array_equal(out["agg"], P0.agg)
    na = P0.na
    Acc = P0.P.T @ Ac @ P0.P
    if not sem.has_outflow:
        Acc = Acc + np.trace(Acc) / na / na
    err = relerr(out["Acc"].reshape(na, na), Acc)
    print("%s Acc: %.2e" % (shape, err))
    assert err <= TOL
    ap, am = out["ap"], out["am"]
    for a in range(na):
        assert np.array_equal(am[ap[a]: ap[a + 1]], np.flatnonzero(P0.agg == a))
