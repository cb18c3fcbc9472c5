"""The Gram-Schmidt and Krylov-basis kernels of csrc/vec.hip against the extended-precision reference of tests/krylov_ref.py, on
bases that are OFF orthonormal by eps = 1e-2 (so that the second projection of CGS2 carries 1e-2 of the first and a kernel that lost
it is nine orders above the tolerance, tests/test_cpu_krylov_ref.py), at the smallest meshes that reach the kernels' edges
(krylov_ref.MESHES).  Every comparison runs level by level and field by field: coefficients, beta, velocity, scalar, pressure, every
valid history level, nrst, and bit for bit that the invalid history levels come back as they went in.  The tolerances are the
project's own (krylov_ref.TOL); the oracle agrees with the reference to 1e-14 on the same cases, 100x below them."""
import numpy as np
import pytest

import krylov_ref as kr
from neklab_amd import host
from oracle.krylov import block_cgs2 as o_block_cgs2

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", [kr.PRECISION])]


class Rig:
    """One case on the device: its columns uploaded once into a basis with one spare column, a vector for w and a scratch vector."""

    def __init__(self, gm, case, spare=1):
        self.gm, self.case = gm, case
        self.B = host.KrylovBasis(gm, case.k + spare, nscal=case.nscal, lorder=case.lorder)
        self.w = host.nek_dvector(gm, nscal=case.nscal, lorder=case.lorder)
        self.tmp = host.nek_dvector(gm, nscal=case.nscal, lorder=case.lorder)
        self.refs = {}
        for j in range(case.k):
            self.put_column(j)

    def put_column(self, j):
        c = self.case
        kr.upload(self.B[j], c, np.stack([c.cols[lev][j] for lev in range(c.lorder)]), int(c.col_nrst[j]), self.tmp)

    def ref(self, k, consistent=True, iw=0, nrst=None):
        key = (k, consistent, iw, nrst)
        if key not in self.refs:
            self.refs[key] = kr.cgs2_ref(self.case, k, consistent, iw, nrst=nrst)
        return self.refs[key]

    def cgs2(self, k, iw=0, nrst=None, in_basis=False):
        """Upload w (into column k of the basis itself for the Arnoldi usage), run nlg_basis_cgs2, bring everything back."""
        c = self.case
        gv = self.B[k] if in_basis else self.w
        kr.upload(gv, c, c.w[iw], c.w_nrst[iw] if nrst is None else nrst, self.tmp)
        try:
            h, beta = self.B.cgs2(k, gv)
            return {"h": h, "beta": beta, "w": kr.download(gv, c), "nrst": gv.nrst}
        finally:
            if in_basis and k < c.k:
                self.put_column(k)


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    """rigs(mesh id, lorder, eps, seed, k): meshes, cases and uploaded bases, each built once for the module."""
    meshes, cache = {}, {}

    def get(mid, lorder=3, eps=1e-2, seed=11, k=None):
        key = (mid, lorder, eps, seed, k)
        if key not in cache:
            if mid not in meshes:
                meshes[mid] = host.Mesh(gpu_ctx, kr.host_mesh(mid))
            case = kr.mesh_case(mid, lorder, seed, k)
            cache[key] = Rig(meshes[mid], case if eps == 1e-2 else case.with_eps(eps))
        return cache[key]

    yield get
    for r in cache.values():
        r.B.close()
    cache.clear()
    kr.clear_cases()


@pytest.fixture
def literal_history(gpu_ctx):
    host.check(gpu_ctx.lib.nlg_set_axpby_rst_consistent(0))
    try:
        yield
    finally:
        host.check(gpu_ctx.lib.nlg_set_axpby_rst_consistent(1))


# ---- nlg_basis_cgs2 ----
@pytest.mark.parametrize("k", kr.CGS2_K["A"])
def test_cgs2_second_trip_of_the_fused_sweeps(rigs, prec, k):
    """Mesh A: nv = 73728 > 65536 launched threads, so threads 0 .. 8191 of k_block_axpy_dot (24 <= k <= 64) and k_block_axpy_dot2
    (65 <= k; above 128 behind a separate sweep over the first k - 128 columns) make a second trip over live accumulators and a
    rewritten stash, the others do not.  k < 24 takes the separate kernels.  w carries two history levels, and so do the columns."""
    r = rigs("A")
    kr.check(r.case, r.cgs2(k), r.ref(k), r.case.w[0])


@pytest.mark.parametrize("k", [24, 65, 131])
def test_cgs2_on_an_orthonormal_basis(rigs, prec, k):
    """eps = 0, the set-up of the older tests: the result is also orthogonal to the basis (meaningful only here)."""
    r = rigs("A", eps=0.0)
    kr.check(r.case, r.cgs2(k), r.ref(k), r.case.w[0])
    assert np.max(np.abs(r.B.block_dot(k, r.w))) < 1e-12


@pytest.mark.parametrize("k", [24, 131])
def test_cgs2_of_a_column_of_the_basis_itself(rigs, prec, k):
    """B.cgs2(k, B[k]): how nlg_arnoldi_step and nlg_svds call it."""
    r = rigs("A")
    kr.check(r.case, r.cgs2(k, in_basis=True), r.ref(k), r.case.w[0])


@pytest.mark.parametrize("mid,k", [(m, k) for m in "BCD" for k in kr.CGS2_K[m]])
def test_cgs2_uneven_chunks_2d_and_scalar(rigs, prec, mid, k):
    """Mesh B: three uneven reduction chunks; mesh C: 2-D, both field lengths padded; mesh D: a scalar in the inner product
    (bm1[i % lvs] wraps four times in the fused sweep)."""
    r = rigs(mid)
    kr.check(r.case, r.cgs2(k), r.ref(k), r.case.w[0])


@pytest.mark.parametrize("k", kr.CGS2_K["C"])
def test_cgs2_without_history_levels(rigs, prec, k):
    """lorder = 1: the vectors are their main blocks."""
    r = rigs("C", lorder=1)
    kr.check(r.case, r.cgs2(k), r.ref(k), r.case.w[0])


@pytest.mark.parametrize("k", kr.CGS2_K["C"])
def test_cgs2_of_a_vector_with_a_shorter_history(rigs, prec, k):
    """w with one valid level against columns with two: level 1 combined and scaled, level 2 untouched bit for bit."""
    r = rigs("C")
    kr.check(r.case, r.cgs2(k, nrst=1), r.ref(k, nrst=1), r.case.w[0])


@pytest.mark.parametrize("mid,k", [("C", 9), ("C", 30), ("B", 9)])
def test_cgs2_literal_history(rigs, literal_history, prec, mid, k):
    """nlg_set_axpby_rst_consistent(0): both history levels of w receive the main-block corrections V h1 and V h2."""
    r = rigs(mid)
    kr.check(r.case, r.cgs2(k), r.ref(k, consistent=False), r.case.w[0])


# ---- nlg_basis_block_dot / nlg_basis_block_axpy / nlg_vec_dot alone ----
@pytest.mark.parametrize("k", [1, 7, 8, 9, 16, 17])
def test_block_dot_and_block_axpy(rigs, prec, k):
    """One pass each on mesh B (uneven chunks), around the tile of 8 columns of k_block_dot and the unrolled 8 of k_block_axpy."""
    r = rigs("B")
    c = r.case
    kr.upload(r.w, c, c.w[0], 2, r.tmp)
    href = kr.block_dot_ref(c, k, c.w[0])
    h = r.B.block_dot(k, r.w)
    print("block_dot deviation %.2e" % (np.max(np.abs(h - href)) / np.max(np.abs(href))))
    assert np.max(np.abs(h - href)) < 1e-13 * np.max(np.abs(href))
    r.B.block_axpy(k, href, r.w)
    kr.check(c, {"w": kr.download(r.w, c), "nrst": r.w.nrst}, {"w": kr.block_axpy_ref(c, k, href, c.w[0], 2), "nrst": 2})


@pytest.mark.parametrize("mid", ["C", "B"])
def test_block_axpy_literal_history(rigs, literal_history, prec, mid):
    """k_block_axpy with nrst > 0 in literal mode: every valid history level receives the main-block correction -- the very sum that
    goes into the main block, so history levels that start as copies of the main block must stay copies of it bit for bit; with
    independent levels, the reference's literal rule to tolerance."""
    r = rigs(mid)
    c, k = r.case, 9
    href = kr.block_dot_ref(c, k, c.w[0])
    kr.upload(r.w, c, c.w[0], 2, r.tmp)
    r.B.block_axpy(k, href, r.w)
    kr.check(c, {"w": kr.download(r.w, c), "nrst": r.w.nrst}, {"w": kr.block_axpy_ref(c, k, href, c.w[0], 2, consistent=False), "nrst": 2})
    kr.upload(r.w, c, np.stack([c.w[0][0]] * 3), 2, r.tmp)
    r.B.block_axpy(k, href, r.w)
    got = kr.download(r.w, c)
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])
    assert not np.array_equal(got[0], c.w[0][0])


def test_dot_and_norm_with_uneven_chunks(rigs, prec):
    """nek_dvector.dot / norm on mesh B (k_dot_partial: three chunks of 2134, 2134, 2132 double2).  A sum of N products carries a
    rounding error of a modest multiple of 2^-53 * sum|a b bm1| <= 2^-53 |a|_B |b|_B, hence the scale; 1e-13 as for block_dot."""
    r = rigs("B")
    c = r.case
    kr.upload(r.w, c, c.w[0], 0, r.tmp)
    kr.upload(r.tmp, c, c.w[1], 0, None)
    bm, n = c.bm.astype(kr.LD), c.nipn
    a, b = c.w[0][0, :n].astype(kr.LD), c.w[1][0, :n].astype(kr.LD)
    na, nb = float(np.sqrt(np.sum(bm * a * a))), float(np.sqrt(np.sum(bm * b * b)))
    d = r.w.dot(r.tmp)
    print("dot deviation %.2e, norm deviation %.2e" % (abs(d - float(np.sum(bm * a * b))) / (na * nb), abs(r.w.norm() - na) / na))
    assert abs(d - float(np.sum(bm * a * b))) < 1e-13 * na * nb
    assert abs(r.w.norm() - na) < 1e-13 * na and abs(r.tmp.norm() - nb) < 1e-13 * nb


# ---- nlg_basis_cgs2_batch ----
@pytest.mark.parametrize("mid,s", [("C", 1), ("C", 3), ("C", 4), ("D", 3)])
@pytest.mark.parametrize("k", [0, 1, 9, 24, 25])
def test_cgs2_batch_lane_by_lane(rigs, prec, mid, s, k):
    """One basis per lane (different seeds), w of lane l scaled by 10^-l, odd lanes with two history levels and even lanes with none:
    each lane against the reference of that lane, not against nlg_basis_cgs2."""
    lanes = [rigs(mid, seed=20 + l, k=25) for l in range(s)]
    ws, nrst = [], []
    for l, r in enumerate(lanes):
        ws.append(r.case.w[0] * 10.0 ** -l)
        nrst.append(2 if l % 2 else 0)
        kr.upload(r.w, r.case, ws[l], nrst[l], r.tmp)
    h, beta = host.KrylovBasis.cgs2_batch([r.B for r in lanes], k, [r.w for r in lanes])
    for l, r in enumerate(lanes):
        got = {"h": h[l], "beta": beta[l], "w": kr.download(r.w, r.case), "nrst": r.w.nrst}
        kr.check(r.case, got, kr.cgs2_ref(r.case, k, w=ws[l], nrst=nrst[l]), ws[l])


def same_bits(a, b):
    """Two results {h, beta, w, nrst} agree bit for bit, every level of w included, valid or not."""
    assert a["nrst"] == b["nrst"]
    assert np.array_equal(a["h"], b["h"]) and a["beta"] == b["beta"]
    assert np.array_equal(a["w"], b["w"])


def batch_lanes(rigs, mid, s, nrst):
    """Lane l of a batch on its own rig (krylov_ref.lane_case), w scaled by 10^-l with nrst[l] valid levels, uploaded."""
    lanes = [rigs(mid, seed=20 + l, k=25) for l in range(s)]
    ws = [kr.lane_w(r.case, l) for l, r in enumerate(lanes)]
    for l, r in enumerate(lanes):
        kr.upload(r.w, r.case, ws[l], nrst[l], r.tmp)
    return lanes, ws


def run_batch(lanes, k):
    h, beta = host.KrylovBasis.cgs2_batch([r.B for r in lanes], k, [r.w for r in lanes])
    return [{"h": h[l], "beta": beta[l], "w": kr.download(r.w, r.case), "nrst": r.w.nrst} for l, r in enumerate(lanes)]


@pytest.mark.parametrize("mid,k", [("C", 0), ("C", 9), ("C", 24), ("C", 40), ("A", 65)])
def test_cgs2_batch_of_one_is_the_single_call(rigs, prec, mid, k):
    """One driver: a batch of one lane is nlg_basis_cgs2 bit for bit, the separate kernels below k = 24 and the fused sweeps from
    there (mesh A at k = 65: the two-tile kernel)."""
    r = rigs(mid)
    c = r.case
    single = r.cgs2(k)
    kr.upload(r.w, c, c.w[0], c.w_nrst[0], r.tmp)
    same_bits(run_batch([r], k)[0], single)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("k", [1, 9, 23])
def test_cgs2_batch_lanes_are_single_calls(rigs, prec, s, k):
    """Below k = 24 every lane of a batch runs the operations of a single call in the same order: lane l is bit for bit
    nlg_basis_cgs2 on a copy of its input.  Odd lanes carry two history levels, even lanes none."""
    nrst = [2 if l % 2 else 0 for l in range(s)]
    lanes, ws = batch_lanes(rigs, "C", s, nrst)
    got = run_batch(lanes, k)
    for l, r in enumerate(lanes):
        kr.upload(r.w, r.case, ws[l], nrst[l], r.tmp)
        h, beta = r.B.cgs2(k, r.w)
        same_bits(got[l], {"h": h, "beta": beta, "w": kr.download(r.w, r.case), "nrst": r.w.nrst})


def test_cgs2_batch_literal_history(rigs, literal_history, prec):
    """nlg_set_axpby_rst_consistent(0) in a batch: every valid history level of lane l receives that lane's main-block corrections,
    lanes with 0, 2 and 1 valid levels side by side; the levels beyond come back bit for bit (kr.check with the input).  The
    references are checked against the oracle in tests/test_cpu_krylov_ref.py."""
    lb = kr.LITERAL_BATCH
    lanes, ws = batch_lanes(rigs, lb["mid"], len(lb["nrst"]), lb["nrst"])
    for l, (r, got) in enumerate(zip(lanes, run_batch(lanes, lb["k"]))):
        kr.check(r.case, got, kr.cgs2_ref(r.case, lb["k"], consistent=False, w=ws[l], nrst=lb["nrst"][l]), ws[l])


# ---- nlg_basis_block_cgs2 ----
@pytest.mark.parametrize("mid", ["C", "B"])
@pytest.mark.parametrize("s", [2, 4])
def test_block_cgs2_against_a_skewed_basis(rigs, prec, mid, s):
    """Against oracle.krylov.block_cgs2 (checked against its formulas on these very cases in tests/test_cpu_krylov_ref.py) with the
    tolerances of test_block_cgs2_matches_oracle.  The leading k columns are not orthonormal by construction, so only the Gram matrix
    of the s new columns is the identity."""
    r = rigs(mid)
    c, k = r.case, 9
    B = host.KrylovBasis(r.gm, k + s, nscal=c.nscal, lorder=c.lorder)
    oV = [kr.oracle_column(c, j) for j in range(k)] + [kr.to_oracle(c, c.w[v], 2) for v in range(s)]
    for j in range(k):
        kr.upload(B[j], c, np.stack([c.cols[lev][j] for lev in range(c.lorder)]), 2, r.tmp)
    for v in range(s):
        kr.upload(B[k + v], c, c.w[v], 2, r.tmp)
    coef = B.block_cgs2(k, s)
    ocoef = o_block_cgs2(oV, k, s)
    assert B.last_block_rank() == s
    print("coefficient deviation %.2e" % (np.max(np.abs(coef - ocoef)) / np.max(np.abs(ocoef))))
    assert np.max(np.abs(coef - ocoef)) < 1e-11 * np.max(np.abs(ocoef))
    assert np.allclose(np.tril(coef[k:], -1), 0.0)
    for v in range(s):
        kr.check(c, {"w": kr.download(B[k + v], c), "nrst": B[k + v].nrst}, {"w": kr.from_oracle(c, oV[k + v]), "nrst": 2},
                 tol={"main": 1e-10, "hist": 1e-10})
    G = np.array([[B[k + a].dot(B[k + b]) for b in range(s)] for a in range(s)])
    assert np.max(np.abs(G - np.eye(s))) < 1e-13
    B.close()


# ---- nlg_basis_combine ----
@pytest.mark.parametrize("k", [1, 9, 17])
@pytest.mark.parametrize("consistent", [True, False])
def test_combine_columns_with_mixed_history(rigs, gpu_ctx, prec, k, consistent):
    """Columns with 1, 2, 0, 1, .. valid levels: consistent mode carries max nrst combined levels (from whatever the columns hold
    there), literal mode none; everything else of `out`, which arrives full of other data, is zero."""
    r = rigs("C")
    c = r.case
    saved = c.col_nrst.copy()
    host.check(gpu_ctx.lib.nlg_set_axpby_rst_consistent(int(consistent)))
    try:
        c.col_nrst[:] = (np.arange(c.k) + 1) % 3
        for j in range(k):
            r.put_column(j)
        coef = np.random.default_rng(k).standard_normal(k)
        kr.upload(r.w, c, c.w[0], 2, r.tmp)
        r.B.combine(k, coef, r.w)
        kr.check(c, {"w": kr.download(r.w, c), "nrst": r.w.nrst}, kr.combine_ref(c, k, coef, consistent), np.zeros_like(c.w[0]))
    finally:
        host.check(gpu_ctx.lib.nlg_set_axpby_rst_consistent(1))
        c.col_nrst[:] = saved
        for j in range(k):
            r.put_column(j)
