"""The tail of CGS2 in consistent mode (csrc/vec.hip, basis_cgs2_dev): second subtraction on the main block, norm, ONE sweep over the
history levels that applies both passes' coefficients and the scale, scale of the main block.  nlg_basis_cgs2 and nlg_basis_cgs2_batch
on 2 x 2 x 2 elements at lx1 = 4 and 8 and on a 2-D mesh, k on both sides of the tile of 8 columns and of the fused sweep (24), w with
0, 1 and 2 valid history levels, one lane and three lanes with different level counts.

What is checked, per lane:
  (i)   every point of the main block and of the valid history levels against (w - V c) / beta evaluated in extended precision with the
        RETURNED c = h and beta.  The tolerance is derived, not chosen: the kernels form w - V c with at most k + 2 roundings per point
        (k fused multiply-adds, the subtraction, the scale), twice on the main block (two passes) and with c = h1 + h2 rounded once, each
        relative to a partial result bounded by |w_i| + sum_j |c_j| |V_ji|:  4 (k + 2) eps (|w_i| + sum_j |c_j| |V_ji|) / beta;
  (ii)  the history levels beyond the lane's nrst come back bit for bit;
  (iii) h and beta bit for bit against the public primitives composed in the order of CGS2 (block_dot, block_axpy, block_dot,
        block_axpy, dot) wherever they perform the same launches: every batch, and a single vector below k = 24.  A single vector at
        k >= 24 takes the fused sweep (k_block_axpy_dot), whose partial sums are partitioned differently: there h and beta are held to the
        extended-precision reference with the tolerances of tests/krylov_ref.py (1e-12 relative);
  (iv)  literal mode (nlg_set_axpby_rst_consistent(0)) in a fresh child process, the setting being global: the results of
        krylov_ref.cgs2_ref(consistent=False) as before, h and beta bit for bit against the primitives."""
import os
import subprocess
import sys

import numpy as np
import pytest

import krylov_ref as kr
from neklab_amd import host

MESHES = {"3d4": ((2, 2, 2), 4), "3d8": ((2, 2, 2), 8), "2d5": ((2, 2), 5)}
KS = (1, 7, 8, 9, 23, 24, 25)
KMAX = max(KS)
LANE_NRST = ((0, 1, 2), (1, 2, 0), (2, 0, 1))      # three lanes, every lane with every level count once
EPS = float(np.finfo(np.float64).eps)


def make_cases(mid):
    """Three cases (one per lane, own seed) of KMAX columns on one mesh, all vectors with lorder = 3."""
    from neklab_amd.mesh import box_mesh
    from oracle.sem import SEM
    nel, n = MESHES[mid]
    hm = box_mesh(nel, n, periodic=(True,) + (False,) * (len(nel) - 1), deform=0.04)
    sem = SEM(hm)
    return hm, [kr.make_case(sem, KMAX, seed=40 + l) for l in range(3)]


class Lane:
    def __init__(self, gm, case):
        self.case = case
        self.B = host.KrylovBasis(gm, KMAX + 1, nscal=0, lorder=3)
        self.w = host.nek_dvector(gm, nscal=0, lorder=3)
        self.tmp = host.nek_dvector(gm, nscal=0, lorder=3)
        for j in range(KMAX):
            kr.upload(self.B[j], case, np.stack([case.cols[lev][j] for lev in range(3)]), 2, self.tmp)

    def put_w(self, w, nrst):
        kr.upload(self.w, self.case, w, nrst, self.tmp)


def pointwise(case, k, w, nrst, got):
    """(i) and (ii) for one lane: `got` = {h, beta, w (lorder, ntot), nrst} as returned."""
    assert got["nrst"] == nrst
    c = np.asarray(got["h"], dtype=kr.LD)
    beta = kr.LD(got["beta"])
    worst = 0.0
    for lev in range(nrst + 1):
        V = case.cols_ld(lev)[:k]
        ref = (w[lev].astype(kr.LD) - c @ V) / beta
        bound = 4 * (k + 2) * EPS * (np.abs(w[lev]).astype(kr.LD) + np.abs(c) @ np.abs(V)) / beta
        err = np.abs(got["w"][lev].astype(kr.LD) - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), "level %d: %d points beyond the bound, worst %.2f of it" % (lev, int(np.sum(err > bound)), float(np.max(err / bound)))
    for lev in range(nrst + 1, case.lorder):
        assert np.array_equal(got["w"][lev], w[lev]), "history level %d beyond nrst = %d was written" % (lev, nrst)
    return worst


def composed(lane, k, w, nrst):
    """(iii): h and beta of CGS2 from the public primitives, in its order."""
    lane.put_w(w, nrst)
    h1 = lane.B.block_dot(k, lane.w)
    lane.B.block_axpy(k, h1, lane.w)
    h2 = lane.B.block_dot(k, lane.w)
    lane.B.block_axpy(k, h2, lane.w)
    return h1 + h2, float(np.sqrt(lane.w.dot(lane.w)))


def check_lanes(lanes, k, ws, nrsts, batch):
    """Run CGS2 of the lanes (one call of nlg_basis_cgs2, or one batch) and check (i) - (iii) lane by lane."""
    for ln, w, nr in zip(lanes, ws, nrsts):
        ln.put_w(w, nr)
    if batch:
        h, beta = host.KrylovBasis.cgs2_batch([ln.B for ln in lanes], k, [ln.w for ln in lanes])
    else:
        h0, b0 = lanes[0].B.cgs2(k, lanes[0].w)
        h, beta = [h0], [b0]
    gots = [{"h": np.array(h[l]), "beta": float(beta[l]), "w": kr.download(ln.w, ln.case), "nrst": ln.w.nrst} for l, ln in enumerate(lanes)]
    fused = len(lanes) == 1 and k >= 24
    for ln, w, nr, got in zip(lanes, ws, nrsts, gots):
        worst = pointwise(ln.case, k, w, nr, got)
        if fused:
            ref = kr.cgs2_ref(ln.case, k, w=w, nrst=nr)
            dh = float(np.max(np.abs(got["h"] - ref["h"])) / np.max(np.abs(ref["h"])))
            db = abs(got["beta"] - ref["beta"]) / ref["beta"]
            print("k %d nrst %d fused: worst point %.3f of its bound, h %.2e beta %.2e" % (k, nr, worst, dh, db))
            assert dh < kr.TOL["h"] and db < kr.TOL["beta"]
        else:
            hc, bc = composed(ln, k, w, nr)
            print("k %d nrst %d: worst point %.3f of its bound" % (k, nr, worst))
            assert np.array_equal(got["h"], hc), "h differs from the composed primitives by %.2e" % np.max(np.abs(got["h"] - hc))
            assert got["beta"] == bc, "beta %r, composed primitives %r" % (got["beta"], bc)


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    cache = {}

    def get(mid):
        if mid not in cache:
            hm, cases = make_cases(mid)
            gm = host.Mesh(gpu_ctx, hm)
            cache[mid] = [Lane(gm, c) for c in cases]
        return cache[mid]

    yield get
    for lanes in cache.values():
        for ln in lanes:
            ln.B.close()
    cache.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mid", list(MESHES))
def test_cgs2_single_vector(rigs, mid, k):
    """nlg_basis_cgs2 and a batch of one lane, w with 0, 1 and 2 valid history levels."""
    ln = rigs(mid)[0]
    for nr in (0, 1, 2):
        check_lanes([ln], k, [ln.case.w[0]], [nr], batch=False)
        check_lanes([ln], k, [ln.case.w[0]], [nr], batch=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mid", list(MESHES))
def test_cgs2_batch_of_three_lanes(rigs, mid, k):
    """Three lanes, each with its own basis, its own w (scaled by 10^-l: own norm) and its own number of history levels."""
    lanes = rigs(mid)
    ws = [ln.case.w[0] * 10.0 ** -l for l, ln in enumerate(lanes)]
    for nrsts in LANE_NRST:
        check_lanes(lanes, k, ws, nrsts, batch=True)


def literal_worker():
    """(iv), run as a child process: literal history mode for the whole process."""
    ctx = host.Context(0)
    host.check(ctx.lib.nlg_set_axpby_rst_consistent(0))
    for mid in MESHES:
        hm, cases = make_cases(mid)
        gm = host.Mesh(ctx, hm)
        lanes = [Lane(gm, c) for c in cases]
        ws = [ln.case.w[0] * 10.0 ** -l for l, ln in enumerate(lanes)]
        for k in KS:
            for nlanes, nrsts in ((1, (2,)), (1, (0,)), (3, LANE_NRST[0]), (3, LANE_NRST[1])):
                use = lanes[:nlanes]
                for ln, w, nr in zip(use, ws, nrsts):
                    ln.put_w(w, nr)
                h, beta = host.KrylovBasis.cgs2_batch([ln.B for ln in use], k, [ln.w for ln in use])
                gots = [{"h": np.array(h[l]), "beta": float(beta[l]), "w": kr.download(ln.w, ln.case), "nrst": ln.w.nrst}
                        for l, ln in enumerate(use)]
                for ln, w, nr, got in zip(use, ws, nrsts, gots):
                    kr.check(ln.case, got, kr.cgs2_ref(ln.case, k, consistent=False, w=w, nrst=nr), w)
                    hc, bc = composed(ln, k, w, nr)      # literal mode has no fused sweep: the same launches at every k
                    assert np.array_equal(got["h"], hc) and got["beta"] == bc, (mid, k, nr)
        for ln in lanes:
            ln.B.close()
    print("LITERAL_OK")


@pytest.mark.gpu
def test_cgs2_literal_mode_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))      # the child finds krylov_ref beside this file and the package one level up
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_cgs2_split_tail as t; t.literal_worker()" % (here, os.path.dirname(here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "LITERAL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
