"""Wavenumber sweep in lock-step: one wavenumber per lane of the block propagator (nlg_linop_set_projection_lanes), the batched CGS2
of s vectors each against its own basis (nlg_basis_cgs2_batch), the sweep Arnoldi step and the driver -- against the
single-wavenumber operator (exptA_proj_linop), the single-lane CGS2 and the oracle twin.  Wavenumbers in an order that is not
sorted, so that a lane / table mix-up cannot hide."""
import os

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh
from oracle.lns import ExptA, LNSConfig
from oracle.sem import SEM
from oracle.vectors import NekDVector

pytestmark = pytest.mark.gpu

ALPHAS = (3.0, 1.0, 4.0, 2.0)
KW = dict(re=200.0, torder=3, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000)
TAU = 0.1


class Case:
    """One channel mesh with its parabolic base flow, the single-wavenumber operators (made on demand, kept) and one sweep operator."""

    def __init__(self, ctx, dim):
        nel = (4, 3) if dim == 2 else (3, 2, 2)
        if dim == 2:
            self.hm = box_mesh(nel, 6, lengths=(2 * np.pi, 2.0), periodic=(True, False), deform=0.0, origin=(0.0, -1.0))
        else:
            self.hm = box_mesh(nel, 6, lengths=(2 * np.pi, 2.0, 1.0), periodic=(True, False, True), deform=0.0, origin=(0.0, -1.0, 0.0))
        self.dim = dim
        self.sem = SEM(self.hm)
        self.gm = host.Mesh(ctx, self.hm)
        self.gb = host.nek_dvector(self.gm)
        self.gb.set_field(0, 1.0 - self.sem.X[1] ** 2)
        self._single = {}
        self.sweep = host.exptA_sweep_linop(TAU, self.gb, ALPHAS, idir=1, **KW)
        self.sweep.init()

    def single(self, alpha):
        if alpha not in self._single:
            A = host.exptA_proj_linop(TAU, self.gb, alpha, idir=1, **KW)
            A.init()
            self._single[alpha] = A
        return self._single[alpha]

    def vec(self, seed, scale=1.0):
        """a random state with a random pressure"""
        x = host.nek_dvector(self.gm)
        x.rand(True, seed=seed)
        n2 = x.get_field(host.PR).size
        x.set_field(host.PR, 0.1 * np.random.default_rng(seed).standard_normal(n2))
        if scale != 1.0:
            x.scal(scale)
        return x


_cases = {}


@pytest.fixture
def case(gpu_ctx, request):
    dim = request.param
    if dim not in _cases:
        _cases[dim] = Case(gpu_ctx, dim)
    return _cases[dim]


def fields_of(c, v, levels=(0,)):
    return [v.get_field(i, r) for r in levels for i in list(range(c.dim)) + [host.PR]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the projection per lane, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 3], indirect=True)
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_proj_block_equals_the_single_alpha_projection_bit_for_bit(case, s):
    c = case
    for alphas in (ALPHAS[:s], (2.0,) * s):
        c.sweep.set_alphas(alphas)
        xs = [c.vec(30 + l, 10.0 ** (-l)) for l in range(s)]
        want = []
        for l in range(s):
            y = xs[l].copy()
            c.single(alphas[l]).proj(y)
            want.append(y)
        c.sweep.proj_block(xs)
        for l in range(s):
            for a, b in zip(fields_of(c, xs[l]), fields_of(c, want[l])):
                assert np.array_equal(a, b), (alphas, l, np.max(np.abs(a - b)))
            assert np.max(np.abs(xs[l].get_field(host.PR))) > 0.0
    # proj (the block of one) uses alphas[0]
    c.sweep.set_alphas(ALPHAS)
    x = c.vec(40)
    y = x.copy()
    c.sweep.proj(x)
    c.single(ALPHAS[0]).proj(y)
    for a, b in zip(fields_of(c, x), fields_of(c, y)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", [2], indirect=True)
def test_set_projection_after_set_alphas_takes_effect(case):
    """Both setters feed one projection path: nlg_linop_set_projection on a handle that had wavenumber lanes replaces the tables (alpha = 1
    is not alphas[0] = 3) and the lanes -- proj is the single-alpha operator's bit for bit, and proj_block has nothing to work on."""
    c = case
    S = c.sweep
    S.set_alphas(ALPHAS[:2])
    lab = host.line_labels(c.gm, 1)
    lab2, x2 = host.line_labels_pressure(c.gm, 1)
    i64 = host._lib.c_int64_p
    host.check(c.gm.lib.nlg_linop_set_projection(S.h, 1.0, 1, lab.ctypes.data_as(i64), lab2.ctypes.data_as(i64), host.dptr(x2)))
    x = c.vec(45)
    y = x.copy()
    S.proj(x)
    c.single(1.0).proj(y)
    for a, b in zip(fields_of(c, x), fields_of(c, y)):
        assert np.array_equal(a, b)
    assert np.max(np.abs(x.get_field(0))) > 0.0 and np.max(np.abs(x.get_field(host.PR))) > 0.0
    with pytest.raises(host.NlgError, match="nlg_linop_project_block: the operator has no wavenumber lanes"):
        S.proj_block([c.vec(46), c.vec(47)])
    S.set_alphas(ALPHAS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the block matvec per lane
# ---------------------------------------------------------------------------------------------------------------------
def lane_inputs(c, alphas, transpose, seed0=20):
    """the set-up of test_projected_matvec_block_equals_single_matvecs: lanes scaled by 10^-l, odd lanes carry a restart history (the
    image of a first matvec at their own wavenumber)"""
    vin = []
    for l, al in enumerate(alphas):
        x = host.nek_dvector(c.gm)
        x.rand(True, seed=seed0 + l)
        x.scal(10.0 ** (-l))
        if l % 2 == 1:
            y = host.nek_dvector(c.gm)
            A = c.single(al)
            (A.rmatvec if transpose else A.matvec)(x, y)
            x = y
        vin.append(x)
    return vin


def assert_lane_equal(c, got, want, vbar=1e-11, pbar=1e-9, tag=None):
    sc = max(np.abs(want.get_field(i)).max() for i in range(c.dim))
    for r in range(3):
        for i in range(c.dim):
            assert np.max(np.abs(got.get_field(i, r) - want.get_field(i, r))) < vbar * sc, (tag, r, i)
        pw = want.get_field(host.PR, r)
        assert np.max(np.abs(got.get_field(host.PR, r) - pw)) < pbar * max(sc, np.abs(pw).max()), (tag, r)


@pytest.mark.parametrize("case,s,transpose", [(2, 2, False), (2, 3, False), (2, 4, False), (2, 2, True), (2, 3, True), (2, 4, True),
                                              (3, 3, False)], indirect=["case"])
def test_block_matvec_runs_every_lane_at_its_own_wavenumber(case, s, transpose):
    c = case
    alphas = ALPHAS[:s]
    c.sweep.set_alphas(alphas)
    vin = lane_inputs(c, alphas, transpose)
    single = [host.nek_dvector(c.gm) for _ in range(s)]
    for l in range(s):
        A = c.single(alphas[l])
        (A.rmatvec if transpose else A.matvec)(vin[l], single[l])
    blk = [host.nek_dvector(c.gm) for _ in range(s)]
    c.sweep.matvec_block(vin, blk, transpose=transpose)
    for l in range(s):
        assert_lane_equal(c, blk[l], single[l], tag=l)
        assert blk[l].nrst == 2
    assert np.max(np.abs(single[0].get_field(0))) > 0.0          # (not a comparison of zero fields)
    # exchanging two wavenumbers together with their input vectors exchanges the outputs
    perm = list(range(s))
    perm[0], perm[-1] = perm[-1], perm[0]
    c.sweep.set_alphas([alphas[p] for p in perm])
    blk2 = [host.nek_dvector(c.gm) for _ in range(s)]
    c.sweep.matvec_block([vin[p] for p in perm], blk2, transpose=transpose)
    for l in range(s):
        assert_lane_equal(c, blk2[l], blk[perm[l]], tag=("swap", l))
    # matvec (the block of one) runs at alphas[0]
    if s == 2 and not transpose:
        c.sweep.set_alphas(alphas)
        y = host.nek_dvector(c.gm)
        c.sweep.matvec(vin[0], y)
        assert_lane_equal(c, y, single[0], tag="matvec")


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the oracle twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2], indirect=True)
def test_block_matvec_lanes_match_the_oracle(case):
    c = case
    sem, s = c.sem, 3
    alphas = ALPHAS[:s]
    U = [1.0 - sem.X[1] ** 2, np.zeros(sem.shape1)]
    oA = ExptA(sem, U, LNSConfig(tau=TAU, **KW))
    lab = host.line_labels(c.gm, 1)
    lab2, x2 = host.line_labels_pressure(c.gm, 1)
    rng = np.random.default_rng(0)
    ovs, gvs = [], []
    for l in range(s):
        ov, gv = NekDVector(sem), host.nek_dvector(c.gm)
        for i in range(2):
            ov.v[i][...] = 10.0 ** (-l) * sem.mask[i] * sem.dsavg(rng.standard_normal(sem.shape1))
            gv.set_field(i, ov.v[i])
        ovs.append(ov)
        gvs.append(gv)
    c.sweep.set_alphas(alphas)
    gout = [host.nek_dvector(c.gm) for _ in range(s)]
    c.sweep.matvec_block(gvs, gout)
    for l in range(s):
        oA.set_projection(alphas[l], 1, lab, lab2, x2)
        oout = oA.matvec(ovs[l])
        sc = max(np.abs(a).max() for a in oout.v)
        for i in range(2):
            assert np.max(np.abs(gout[l].get_field(i).reshape(sem.shape1) - oout.v[i])) < 1e-9 * sc, (l, i)
        assert np.max(np.abs(gout[l].get_field(host.PR).reshape(sem.shape2) - oout.pr)) < 1e-7 * max(np.abs(oout.pr).max(), 1e-30), l


# ---------------------------------------------------------------------------------------------------------------------
# 4. batched CGS2
# ---------------------------------------------------------------------------------------------------------------------
KMAX = 25
_bases = {}


def hist_vec(c, seed, with_history, scale=1.0):
    x = c.vec(seed)
    if with_history:
        for r in (1, 2):
            x.save_rst(c.vec(1000 * r + seed), r)
    if scale != 1.0:
        x.scal(scale)
    return x


def orthonormal_bases(c, s):
    """s bases of KMAX orthonormal random columns with history, different per lane (built once by the single-lane path)"""
    if s not in _bases:
        out = []
        for l in range(s):
            B = host.KrylovBasis(c.gm, KMAX + 1)
            for j in range(KMAX):
                B[j].assign(hist_vec(c, 100 * (l + 1) + j, True))
                B.cgs2(j, B[j])
            G = np.array([B.block_dot(KMAX, B[j]) for j in range(KMAX)])
            assert np.max(np.abs(G - np.eye(KMAX))) < 1e-13
            out.append(B)
        _bases[s] = out
    return _bases[s]


def check_cgs2_lane(c, B, k, w, w0, h, beta, tag):
    """lane result (w, h, beta) of the batched call against nlg_basis_cgs2 on a copy w0 of the lane's input"""
    href, bref = B.cgs2(k, w0)
    if k:
        assert np.max(np.abs(h - href)) <= 1e-11 * np.max(np.abs(href)), (tag, np.max(np.abs(h - href)))
    assert abs(beta - bref) <= 1e-12 * bref, (tag, beta, bref)
    sc = max(np.abs(w0.get_field(i)).max() for i in range(c.dim))
    for i in range(c.dim):
        assert np.max(np.abs(w.get_field(i) - w0.get_field(i))) < 1e-10 * sc, (tag, i)
        assert np.max(np.abs(w.get_field(i, 2) - w0.get_field(i, 2))) < 1e-10 * max(sc, np.abs(w0.get_field(i, 2)).max()), (tag, i, "history")
    assert np.max(np.abs(w.get_field(host.PR) - w0.get_field(host.PR))) < 1e-10 * max(sc, np.abs(w0.get_field(host.PR)).max()), tag
    assert w.nrst == w0.nrst
    # Gram matrix of the columns 0 .. k-1 plus w: the columns themselves are orthonormal (orthonormal_bases), so the last row / column
    if k:
        assert np.max(np.abs(B.block_dot(k, w))) < 1e-13, tag
    assert abs(w.dot(w) - 1.0) < 1e-13, tag


@pytest.mark.parametrize("case", [2], indirect=True)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("k", [0, 1, 8, 9, 23, 24, 25])
def test_cgs2_batch_equals_cgs2_lane_by_lane(case, s, k):
    c = case
    bases = orthonormal_bases(c, s)
    ws = [hist_vec(c, 500 + 10 * k + l, l % 2 == 1, 10.0 ** (-l)) for l in range(s)]       # odd lanes carry a history
    w0 = [w.copy() for w in ws]
    h, beta = host.KrylovBasis.cgs2_batch(bases, k, ws)
    assert h.shape == (s, k) and beta.shape == (s,)
    for l in range(s):
        check_cgs2_lane(c, bases[l], k, ws[l], w0[l], h[l], beta[l], (s, k, l))
        assert ws[l].nrst == (2 if l % 2 == 1 else 0)


@pytest.mark.parametrize("case", [2], indirect=True)
def test_cgs2_batch_leaves_a_zero_lane_zero(case):
    c = case
    s, k = 4, 9
    bases = orthonormal_bases(c, s)
    ws = [hist_vec(c, 700 + l, l % 2 == 0, 10.0 ** (-l)) for l in range(s)]
    ws[2].zero()
    w0 = [w.copy() for w in ws]
    h, beta = host.KrylovBasis.cgs2_batch(bases, k, ws)
    assert beta[2] == 0.0 and np.all(h[2] == 0.0)
    for a in fields_of(c, ws[2], levels=(0, 1, 2)):
        assert np.all(a == 0.0)
    for l in (0, 1, 3):
        check_cgs2_lane(c, bases[l], k, ws[l], w0[l], h[l], beta[l], ("zero", l))
    # the same basis or the same vector in two lanes, and a vector that is one of the columns it is orthogonalised against
    with pytest.raises(host.NlgError, match="nlg_basis_cgs2_batch"):
        host.KrylovBasis.cgs2_batch([bases[0], bases[0]], k, ws[:2])
    with pytest.raises(host.NlgError, match="nlg_basis_cgs2_batch"):
        host.KrylovBasis.cgs2_batch(bases[:2], k, [ws[0], bases[0][3]])
    with pytest.raises(host.NlgError, match="nlg_basis_cgs2_batch"):
        host.KrylovBasis.cgs2_batch(bases[:2], KMAX + 2, ws[:2])


# ---------------------------------------------------------------------------------------------------------------------
# 5. sweep Arnoldi
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2], indirect=True)
def test_sweep_arnoldi_equals_one_arnoldi_per_wavenumber(case):
    c = case
    s, m = 3, 6
    alphas = ALPHAS[:s]
    c.sweep.set_alphas(alphas)
    starts = [c.vec(60 + l) for l in range(s)]
    c.sweep.proj_block(starts)
    for x in starts:
        x.scal(1.0 / x.norm())
    bases = [host.KrylovBasis(c.gm, m + 1) for _ in range(s)]
    for l in range(s):
        bases[l][0].assign(starts[l])
    Hs = np.zeros((s, m, m + 1))
    for k in range(m):
        host.sweep_arnoldi_step(c.sweep, bases, k, Hs)
    for l in range(s):
        B = host.KrylovBasis(c.gm, m + 1)
        B[0].assign(starts[l])
        H = np.zeros((m + 1, m), order="F")
        for k in range(m):
            host.arnoldi_step(c.single(alphas[l]), B, k, H)
        assert np.max(np.abs(Hs[l].T - H)) < 1e-9 * np.max(np.abs(H)), (l, np.max(np.abs(Hs[l].T - H)))
        G = np.array([bases[l].block_dot(m + 1, bases[l][j]) for j in range(m + 1)])
        assert np.max(np.abs(G - np.eye(m + 1))) < 1e-12, l
        B.close()
    for B in bases:
        B.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the driver
# ---------------------------------------------------------------------------------------------------------------------
DRIVER_ALPHAS = (3.0, 1.0, 4.0, 2.0, 2.0)      # two groups: four lanes, then one
# a loose tol, chosen from the residual histories of a first run so that lanes finish at different steps: with seed 1 the five
# wavenumbers take 12, 7, 12, 8, 10 steps (alpha = 1 and 2 are retired at steps 7 and 8, the other two lanes go on to kdim)
DRIVER_TOL, DRIVER_SEED, DRIVER_KDIM = 2e-3, 1, 12


@pytest.mark.parametrize("case", [2], indirect=True)
def test_driver_retires_lanes_and_matches_eigs_per_wavenumber(case, tmp_path):
    c = case
    res = host.linear_stability_analysis_wavenumbers(TAU, c.gb, DRIVER_ALPHAS, DRIVER_KDIM, 1, tol=DRIVER_TOL, seed=DRIVER_SEED,
                                                     outdir=str(tmp_path), **KW)
    assert len(res) == len(DRIVER_ALPHAS)
    steps = [r[4] for r in res]
    print("steps per wavenumber:", steps)
    # the retirement path: in the group of four at least one lane finished before another (recorded for this seed and tol: see above)
    assert min(steps[:4]) < max(steps[:4]), steps
    for i, al in enumerate(DRIVER_ALPHAS):
        eigvals, residuals, eigvecs, mu, nmv = res[i]
        assert os.path.exists(os.path.join(str(tmp_path), "dir_eigenspectrum_alpha%d.npy" % i))
        A = c.single(al)
        x0 = host.nek_dvector(c.gm)
        x0.rand(True, seed=DRIVER_SEED + i)
        A.proj(x0)
        X = [host.nek_dvector(c.gm)]
        mu_e, res_e, info = host.eigs(A, X, kdim=DRIVER_KDIM, tol=DRIVER_TOL, x0=x0, write_intermediate=False, max_restarts=0)
        d = min(abs(mu[0] - mu_e[0]), abs(mu[0] - np.conj(mu_e[0])))
        print("alpha %g: mu %s eigs %s steps %d / %d" % (al, mu[0], mu_e[0], nmv, info))
        assert d <= 1e-7 * abs(mu_e[0]), (i, al, mu[0], mu_e[0])
        assert abs(eigvals[0] - np.log(mu[0]) / TAU) < 1e-12 * abs(eigvals[0])
        assert eigvecs[0].norm() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2], indirect=True)
def test_refusals_name_their_reason_and_leave_the_operator_alone(case):
    c = case
    lib, gm = c.gm.lib, c.gm
    i64, dp = host._lib.c_int64_p, host._lib.c_double_p
    lab = host.line_labels(gm, 1)
    labp = lab.ctypes.data_as(i64)
    al = np.array(ALPHAS + (5.0,))

    def set_lanes(op, n, alpha=al):
        host.check(lib.nlg_linop_set_projection_lanes(op.h, n, None if alpha is None else host.dptr(alpha), 1, labp, None, None))

    def block_result(op, vin):
        out = [host.nek_dvector(gm) for _ in vin]
        op.matvec_block(vin, out)
        return [a for y in out for a in fields_of(c, y, levels=(0, 1, 2))]

    def unchanged(op, vin, before):
        for a, b in zip(block_result(op, vin), before):
            assert np.array_equal(a, b)

    S = c.sweep
    S.set_alphas(ALPHAS[:2])
    vin = [c.vec(80 + l) for l in range(3)]
    before = block_result(S, vin[:2])
    y3 = [host.nek_dvector(gm) for _ in range(3)]
    bases = [host.KrylovBasis(gm, 3) for _ in range(3)]
    Hs = np.zeros((3, 2, 3))
    plain = host.exptA_linop(TAU, c.gb, **KW)
    plain.init()
    o = host._lib.OtdOpts()
    host.check(lib.nlg_otd_opts_default(host.C.byref(o)))
    o.r = 2
    otd = host.vp()
    refusals = [
        (lambda: set_lanes(S, 0), "nlg_linop_set_projection_lanes"),
        (lambda: set_lanes(S, 5), "nlg_linop_set_projection_lanes"),
        (lambda: set_lanes(S, 2, None), "nlg_linop_set_projection_lanes"),
        (lambda: S.matvec_block(vin, y3), "wavenumber lanes"),                                   # s = 3 > nalpha = 2
        (lambda: S.proj_block(vin), "wavenumber lanes"),
        (lambda: host.integrate_forced(S, None, vin[0], None, 1.0, False, y3[0]), "wavenumber lanes"),
        (lambda: host.integrate_forced_block(S, None, vin[:2], None, 1.0, False, y3[:2]), "wavenumber lanes"),
        (lambda: host.sweep_arnoldi_step(S, bases, 0, Hs), "nlg_sweep_arnoldi_step"),            # s = 3 > nalpha = 2
        (lambda: host.sweep_arnoldi_step(S, bases[:2], 2, Hs), "nlg_sweep_arnoldi_step"),        # k + 1 >= nvec
        (lambda: host.check(lib.nlg_otd_create(S.h, host.C.byref(o), None, host.C.byref(otd))), "wavenumber projection"),
        (lambda: host.check(lib.nlg_linop_set_orbit(S.h, c.gb.h, TAU)), "wavenumber projection"),
    ]
    for call, word in refusals:
        with pytest.raises(host.NlgError, match=word):
            call()
        unchanged(S, vin[:2], before)
    # an operator without wavenumber lanes: the sweep step refuses it -- a plain one and one with a single alpha for all lanes
    pbefore = block_result(plain, vin[:2])
    for op in (plain, c.single(2.0)):
        with pytest.raises(host.NlgError, match="nlg_sweep_arnoldi_step.*wavenumber lanes"):
            host.sweep_arnoldi_step(op, bases[:2], 0, Hs)
    unchanged(plain, vin[:2], pbefore)
    # a live nlg_otd
    host.check(lib.nlg_otd_create(plain.h, host.C.byref(o), None, host.C.byref(otd)))
    with pytest.raises(host.NlgError, match="nlg_linop_set_projection_lanes.*nlg_otd"):
        set_lanes(plain, 2)
    host.check(lib.nlg_otd_destroy(otd))
    unchanged(plain, vin[:2], pbefore)
    plain.close()
    # orbit mode
    Ob = host.exptA_orbit_linop(TAU, c.gb, **KW)
    obefore = block_result(Ob, vin[:2])
    with pytest.raises(host.NlgError, match="nlg_linop_set_projection_lanes.*orbit mode"):
        set_lanes(Ob, 2)
    unchanged(Ob, vin[:2], obefore)
    Ob.close()
    # cfg.ifheat
    bT = host.nek_dvector(gm, 1, 3)
    bT.set_field(0, 1.0 - c.sem.X[1] ** 2)
    Ht = host.exptA_linop(TAU, bT, ifheat=1, conductivity=0.3, rhocp=1.5, **KW)
    Ht.init()
    with pytest.raises(host.NlgError, match="nlg_linop_set_projection_lanes.*ifheat"):
        set_lanes(Ht, 2)
    Ht.close()
    # nlg_linop_set_projection after the lane call: bit for bit the single-alpha operator's matvec, for every lane of a block
    host.check(lib.nlg_linop_set_projection(S.h, 2.0, 1, labp, None, None))
    P = host.exptA_proj_linop(TAU, c.gb, 2.0, idir=1, project_pressure=False, **KW)
    P.init()
    got, want = host.nek_dvector(gm), host.nek_dvector(gm)
    S.matvec(vin[0], got)
    P.matvec(vin[0], want)
    for a, b in zip(fields_of(c, got, levels=(0, 1, 2)), fields_of(c, want, levels=(0, 1, 2))):
        assert np.array_equal(a, b)
    for a, b in zip(block_result(S, vin), block_result(P, vin)):
        assert np.array_equal(a, b)
    P.close()
    for B in bases:
        B.close()
    S.set_alphas(ALPHAS)
