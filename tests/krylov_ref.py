"""Reference for the Gram-Schmidt and Krylov-basis kernels (numpy only; test infrastructure, never imported by the product).

Works on stacked host arrays, not on the oracle classes: oracle/vectors.py and oracle/krylov.py are checked against it in turn
(tests/test_cpu_krylov_ref.py), the kernels of csrc/vec.hip in tests/test_gpu_krylov_oracle.py.  Sums run in `np.longdouble` where
that is an extended format (eps < 1e-18), else in float64; `PRECISION` names which and goes into the test ids.

One level of one vector is a flat array  [ v_0 | .. | v_{dim-1} | theta_0 .. | pr ]  of `ntot = nip * lvn + lpn` unpadded entries
(nip = dim + nscal fields enter the inner product, weight bm1 tiled over them as NekDVector.dot sums them).  A vector is `lorder`
such levels: the main block and lorder - 1 restart-history levels, `nrst` of them valid.

The basis of a case is deliberately OFF orthonormal by a known eps: against an orthonormal basis the second projection of CGS2 is
rounding noise, and a kernel that dropped it would pass every comparison (Krylov section).
"""
import functools

import numpy as np

LD = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64
PRECISION = "longdouble" if LD is np.longdouble else "float64"

PR, THETA = 3, 4                       # field numbers of the C ABI (include/neklab_gpu.h); velocity components are 0 .. dim-1

# the project's tolerances for these kernels (test_cgs2_fused_sweep_matches_separate_kernels, test_block_kernels), relative to
# max|h_ref|, beta_ref, max|field_ref| and max|level_ref|
TOL = {"h": 1e-12, "beta": 1e-12, "main": 1e-12, "hist": 1e-11}


# The meshes of the kernel tests, each the smallest that reaches its edge, and the k at which cgs2 runs on them:
#   A  nv = 3 * 24576 = 73728 > 256 * 256: the grid-stride loops of the fused sweeps take a partial second trip (threads 0 .. 8191)
#   B  lvs = 12800: nblk = 3 does not divide n2 = 6400, the reduction chunks of k_block_dot / k_dot_partial are uneven
#   C  2-D (ncomp = 2); lvn = 1225 and lpn = 625 are both padded (lvs = 1248, lps = 640)
#   D  one scalar: ncomp = 4 in the fused sweep and in the lane kernels
MESHES = {"A": ((4, 4, 3), 8, 0), "B": ((5, 5, 1), 8, 0), "C": ((5, 5), 7, 0), "D": ((3, 2, 2), 6, 1)}      # elements, lx1, nscal
CGS2_K = {"A": (1, 8, 9, 23, 24, 63, 64, 65, 127, 128, 129, 131), "B": (9, 25), "C": (9, 24, 40), "D": (5, 24, 30)}


def host_mesh(mid):
    from neklab_amd.mesh import box_mesh
    nel, n, _ = MESHES[mid]
    return box_mesh(nel, n, periodic=(True,) + (False,) * (len(nel) - 1), deform=0.04)


class Case:
    """k basis columns and nw vectors w on one mesh.  cols[lev] is (k, ntot), w[i] is (lorder, ntot), all float64."""

    def __init__(self, sem, k, nscal, lorder):
        self.sem, self.k, self.nscal, self.lorder = sem, k, nscal, lorder
        self.dim, self.lvn, self.lpn = sem.dim, sem.lvn, sem.lpn
        self.nip = sem.dim + nscal
        self.nipn = self.nip * sem.lvn
        self.ntot = self.nipn + sem.lpn
        self.bm = np.tile(np.asarray(sem.bm1, dtype=np.float64).ravel(), self.nip)
        ids = list(range(sem.dim)) + [THETA + m for m in range(nscal)]
        self.fields = [(f, slice(i * sem.lvn, (i + 1) * sem.lvn)) for i, f in enumerate(ids)] + [(PR, slice(self.nipn, self.ntot))]
        self._ld = {}

    def cols_ld(self, lev):
        if lev not in self._ld:
            self._ld[lev] = self.cols[lev].astype(LD)
        return self._ld[lev]

    def with_eps(self, eps):
        """The same Q, S, pressure, history and w-residual with another distance from orthonormality (eps = 0: V = Q)."""
        c = Case(self.sem, self.k, self.nscal, self.lorder)
        c.eps, c.Q, c.S, c.wres, c.wcoef = eps, self.Q, self.S, self.wres, self.wcoef
        c.col_nrst, c.w_nrst = self.col_nrst, self.w_nrst
        V = self.Q @ (np.eye(self.k) + eps * self.S) if eps else self.Q
        main = self.cols[0].copy()
        main[:, :self.nipn] = V.T
        c.cols = [main] + self.cols[1:]
        c.w = []
        for w0, r, cf in zip(self.w, self.wres, self.wcoef):
            w = w0.copy()
            w[0, :self.nipn] = r + V @ cf
            c.w.append(w)
        return c


def make_case(sem, k, nscal=0, lorder=3, eps=1e-2, seed=0, nw=1):
    """V = Q (I + eps S): Q B-orthonormal (QR of a random matrix scaled by sqrt(bm1), unscaled again), S_ij ~ N(0, 1/k).  Pressure and all
    history levels of the columns and of w are independent random fields of the columns' magnitude.  The inner-product part of each w
    is a B-unit random field plus V c, c_j ~ N(0, 1/k): a component of order one inside the span and one outside it.  Every vector
    starts with all lorder - 1 history levels valid; the tests lower `col_nrst[j]` / `w_nrst[i]` where they want fewer."""
    rng = np.random.default_rng(seed)
    c = Case(sem, k, nscal, lorder)
    sq = np.sqrt(c.bm)
    Q, _ = np.linalg.qr(rng.standard_normal((c.nipn, k)) * sq[:, None])
    Q /= sq[:, None]
    c.eps, c.Q, c.S = eps, Q, rng.standard_normal((k, k)) / np.sqrt(k)
    amp = float(np.sqrt(np.mean(Q * Q)))
    c.cols = [amp * rng.standard_normal((k, c.ntot)) for _ in range(lorder)]
    c.w, c.wres, c.wcoef = [], [], []
    for _ in range(nw):
        r = rng.standard_normal(c.nipn)
        c.wres.append(r / np.sqrt(np.sum(c.bm * r * r)))
        c.wcoef.append(rng.standard_normal(k) / np.sqrt(k))
        c.w.append(amp * rng.standard_normal((lorder, c.ntot)))
    c.col_nrst = np.full(k, lorder - 1)
    c.w_nrst = [lorder - 1] * nw
    return c.with_eps(eps)


@functools.lru_cache(maxsize=None)
def _sem(mid):
    from oracle.sem import SEM
    return SEM(host_mesh(mid))


@functools.lru_cache(maxsize=None)
def mesh_case(mid, lorder=3, seed=11, k=None):
    """The eps = 1e-2 case of a mesh with four w, built once per process; prefixes of its columns serve every k of that mesh
    (clear_cases() at the end of a test module gives the memory back)."""
    return make_case(_sem(mid), k or max(CGS2_K[mid]), nscal=MESHES[mid][2], lorder=lorder, eps=1e-2, seed=seed, nw=4)


def lane_case(mid, l):
    """Lane l of the batched tests: its own basis of 25 columns (seed 20 + l)."""
    return mesh_case(mid, seed=20 + l, k=25)


def lane_w(case, l):
    """... and its vector, scaled by 10^-l so that no lane can stand in for another."""
    return case.w[0] * 10.0 ** -l


LITERAL_BATCH = {"mid": "C", "k": 9, "nrst": (0, 2, 1)}      # the literal-history batch of tests/test_gpu_krylov_oracle.py


def clear_cases():
    mesh_case.cache_clear()
    _sem.cache_clear()


def chunk_tail(case):
    """The two points of the last double2 of the first reduction chunk of k_block_dot / k_dot_partial in field 0 (csrc/vec.hip: fields
    padded to 32 doubles, lvs / 4096 chunks of ceil(n2 / nblk) double2 each), moved inside the field where the chunk ends in the padding."""
    lvs = (case.lvn + 31) // 32 * 32
    nblk = max(1, lvs // 4096)
    per = (lvs // 2 + nblk - 1) // nblk
    e = min(2 * per, case.lvn)
    return slice(e - 2, e)


def block_dot_ref(case, k, w):
    """h = V^T (bm1 o w) over the inner-product fields of the main blocks (one pass); w is one (lorder, ntot) vector."""
    V = case.cols_ld(0)[:k, :case.nipn]
    return np.asarray(V @ (case.bm.astype(LD) * w[0, :case.nipn].astype(LD)), dtype=np.float64)


def _subtract(case, k, w, nrst, hs, consistent, main=True):
    """w (LD, in place) minus the combinations of the first k columns with each coefficient set of `hs` in turn, as axpby applies them:
    main block from the columns' main blocks; valid history level r from the columns' level r (consistent) or main blocks (literal)."""
    for h in hs:
        if main:
            w[0] -= h @ case.cols_ld(0)[:k]
        for r in range(1, nrst + 1):
            w[r] -= h @ case.cols_ld(r if consistent else 0)[:k]


def block_axpy_ref(case, k, h, w, nrst, consistent=True):
    """w - V h on the main block (pressure included) and the nrst valid history levels, unscaled (one pass)."""
    out = w.astype(LD)
    _subtract(case, k, out, nrst, [np.asarray(h, dtype=LD)], consistent)
    return np.asarray(out, dtype=np.float64)


def cgs2_ref(case, k, consistent=True, iw=0, w=None, nrst=None, mutant=None):
    """h1 = V^T (bm1 o w), w1 = w - V h1, h2 = V^T (bm1 o w1), w2 = w1 - V h2, beta = |w2|_B; returns h = h1 + h2, beta, and w2 / beta
    with the pressure and the valid history levels combined as NekDVector.axpby does inside cgs2_step, all scaled by 1 / beta.
    Invalid levels are returned untouched.  `mutant` (tests/test_cpu_krylov_ref.py only) breaks one step on purpose."""
    w = case.w[iw] if w is None else w
    nrst = case.w_nrst[iw] if nrst is None else nrst
    n = case.nipn
    bm = case.bm.astype(LD)
    out = w.astype(LD)
    if k > 0:
        V = case.cols_ld(0)[:k, :n]
        h1 = V @ (bm * out[0, :n])
        w1 = out[0, :n] - h1 @ V
        x = bm * (out[0, :n] if mutant == "h2_from_w" else w1)
        if mutant == "h2_drops_chunk_tail":
            x[chunk_tail(case)] = 0
        h2 = V @ x
        if mutant == "h2_zero":
            h2 = 0 * h2
        h2s = h2.copy()                                    # what the second subtraction applies to the inner-product fields
        if mutant is not None and mutant.startswith("skip_column_"):
            h2s[int(mutant[12:])] = 0
        hh1 = 0 * h1 if mutant == "history_h2_only" else h1
        _subtract(case, k, out, nrst, [hh1, h2], consistent, main=False)
        out[0, :n] = w1 - h2s @ V
        if mutant != "pressure_untouched":
            out[0, n:] -= (h1 + h2) @ case.cols_ld(0)[:k, n:]
        h = h1 + h2
    else:
        h = np.zeros(0, dtype=LD)
    beta = np.sqrt(np.sum(bm * out[0, :n] ** 2))
    out[:nrst + 1] /= beta
    return {"h": np.asarray(h, dtype=np.float64), "beta": float(beta), "w": np.asarray(out, dtype=np.float64), "nrst": nrst}


def combine_ref(case, k, c, consistent=True):
    """oracle.krylov.lincomb restated: sum_i c_i V_i on the main block; consistent mode: nrst = max over the k columns and every level
    below it combined from the columns' levels (whatever they hold); literal mode: no history.  Invalid levels are zero."""
    c = np.asarray(c, dtype=LD)
    nrst = int(max(case.col_nrst[:k])) if consistent else 0
    out = np.zeros((case.lorder, case.ntot), dtype=LD)
    for r in range(nrst + 1):
        out[r] = c @ case.cols_ld(r)[:k]
    return {"w": np.asarray(out, dtype=np.float64), "nrst": nrst}


def block_cgs2_ref(case, k, W):
    """oracle.krylov.block_cgs2 by its formulas for a block that is not deflated: two passes  H = V^T B W, W -= V H  (all columns of a pass
    from the same W; pressure and history follow, consistent mode, every vector with all levels valid), then twice  G = W^T B W = L L^T,
    W <- W L^-T, R <- L^T R.  W is a list of s (lorder, ntot) vectors; returns the (k + s, s) coefficients and the new W."""
    s, n = len(W), case.nipn
    bm = case.bm.astype(LD)
    W = [w.astype(LD) for w in W]
    coef = np.zeros((k + s, s), dtype=LD)
    for _ in range(2 if k else 0):
        V = case.cols_ld(0)[:k, :n]
        H = np.stack([V @ (bm * w[0, :n]) for w in W], axis=1)
        for v in range(s):
            _subtract(case, k, W[v], case.lorder - 1, [H[:, v]], True)
        coef[:k] += H
    R = np.eye(s, dtype=LD)
    for _ in range(2):
        G = np.array([[np.sum(bm * a[0, :n] * b[0, :n]) for b in W] for a in W], dtype=LD)
        L = np.zeros((s, s), dtype=LD)
        for i in range(s):
            for j in range(i + 1):
                a = G[i, j] - np.dot(L[i, :j], L[j, :j])
                L[i, j] = np.sqrt(a) if i == j else a / L[j, j]
        T = np.zeros((s, s), dtype=LD)                     # T = L^-T, column by column (back substitution)
        for b in range(s):
            for i in range(s - 1, -1, -1):
                T[i, b] = ((1.0 if i == b else 0.0) - np.dot(L[i + 1:, i], T[i + 1:, b])) / L[i, i]
        W = [sum(T[a, b] * W[a] for a in range(s)) for b in range(s)]
        R = L.T @ R
    coef[k:] = R
    return np.asarray(coef, dtype=np.float64), [np.asarray(w, dtype=np.float64) for w in W]


def deviations(case, got, ref, orig=None):
    """Relative deviations of a result {h, beta, w, nrst} from the reference, keyed by the tolerance class of TOL: coefficients over
    max|h_ref|, beta relative, main-block fields over max|field_ref|, valid history levels field by field over max|level_ref|.  With
    `orig` (the vector as it went in) the invalid levels must have come back bit for bit."""
    dev = {}
    if "h" in ref and len(ref["h"]):
        dev["h"] = float(np.max(np.abs(got["h"] - ref["h"])) / np.max(np.abs(ref["h"])))
    if "beta" in ref:
        dev["beta"] = abs(got["beta"] - ref["beta"]) / ref["beta"]
    assert got["nrst"] == ref["nrst"], (got["nrst"], ref["nrst"])
    for f, sl in case.fields:
        dev["main", f] = float(np.max(np.abs(got["w"][0, sl] - ref["w"][0, sl])) / np.max(np.abs(ref["w"][0, sl])))
    for r in range(1, ref["nrst"] + 1):
        sc = np.max(np.abs(ref["w"][r]))
        for f, sl in case.fields:
            dev["hist", r, f] = float(np.max(np.abs(got["w"][r, sl] - ref["w"][r, sl])) / sc)
    if orig is not None:
        for r in range(ref["nrst"] + 1, case.lorder):
            assert np.array_equal(got["w"][r], orig[r]), "invalid history level %d was written" % r
    return dev


def check(case, got, ref, orig=None, tol=TOL):
    """Assert every deviation against the tolerance of its class; the figures are printed first so that a run can record them."""
    dev = deviations(case, got, ref, orig)
    worst = {}
    for key, d in dev.items():
        cls = key if isinstance(key, str) else key[0]
        worst[cls] = max(worst.get(cls, 0.0), d)
    print("deviations:", "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    for key, d in dev.items():
        cls = key if isinstance(key, str) else key[0]
        assert d < tol[cls], (key, d, tol[cls])
    return worst


# ---- to and from the oracle classes and the device ----
def to_oracle(case, w, nrst):
    """One (lorder, ntot) vector as an oracle NekDVector with `nrst` valid levels (the others carry their data all the same)."""
    from oracle.vectors import NekDVector
    sem = case.sem
    ov = NekDVector(sem, case.nscal, case.lorder)
    for lev in range(case.lorder):
        dst = ov.main_fields() if lev == 0 else ov.rst_fields(lev - 1)       # v.., pr, theta..
        for f, sl in case.fields:
            i = f if f < PR else (case.dim if f == PR else case.dim + 1 + f - THETA)
            dst[i][...] = w[lev, sl].reshape(sem.shape2 if f == PR else sem.shape1)
    ov.nrst = nrst
    return ov


def from_oracle(case, ov):
    w = np.zeros((case.lorder, case.ntot))
    for lev in range(case.lorder):
        src = ov.main_fields() if lev == 0 else ov.rst_fields(lev - 1)
        for f, sl in case.fields:
            i = f if f < PR else (case.dim if f == PR else case.dim + 1 + f - THETA)
            w[lev, sl] = src[i].ravel()
    return w


def oracle_column(case, j):
    return to_oracle(case, np.stack([case.cols[lev][j] for lev in range(case.lorder)]), int(case.col_nrst[j]))


def upload(gv, case, w, nrst, tmp=None):
    """Every field of every level of one (lorder, ntot) vector into the device vector gv (like `upload` of tests/test_gpu_block.py, with
    scalars and any lorder), invalid levels included, then `nrst` levels declared valid.  `tmp`: a scratch device vector of the same
    layout, needed where nrst > 0 (the level count only moves through save_rst)."""
    for lev in range(case.lorder):
        for f, sl in case.fields:
            gv.set_field(f, w[lev, sl], lev)
    gv.clear_rst_fields()
    if nrst > 0:
        gv.get_rst(tmp, nrst)
        gv.save_rst(tmp, nrst)
    assert gv.nrst == nrst


def download(gv, case):
    """Every field of every level, valid or not, as one (lorder, ntot) array."""
    w = np.empty((case.lorder, case.ntot))
    for lev in range(case.lorder):
        for f, sl in case.fields:
            w[lev, sl] = gv.get_field(f, lev)
    return w
