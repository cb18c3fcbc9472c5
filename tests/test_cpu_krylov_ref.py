"""The reference of tests/krylov_ref.py checked on the CPU: the oracle's Gram-Schmidt (oracle/krylov.py on oracle/vectors.py) agrees
with it to 1e-14, which is what admits the 1e-12 tolerances of tests/test_gpu_krylov_oracle.py (the reference's own float64 noise sits
100x under them), and the comparison it feeds can see the faults it is there for: each mutant of the second CGS2 pass moves a compared
quantity by 1000x the tolerance on a basis that is off orthonormal by 1e-2 -- and by nothing measurable on an orthonormal one."""
import functools

import numpy as np
import pytest

import krylov_ref as kr
from oracle.krylov import block_cgs2 as o_block_cgs2
from oracle.krylov import cgs2_step, lincomb
from oracle.vectors import NekDVector

pytestmark = pytest.mark.parametrize("prec", [kr.PRECISION])
AGREE = 1e-14


case_of = kr.mesh_case


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    for f in (oracle_columns, ref_of):
        f.cache_clear()
    kr.clear_cases()


@functools.lru_cache(maxsize=None)
def ref_of(mid, k):
    return kr.cgs2_ref(case_of(mid), k)


@functools.lru_cache(maxsize=None)
def oracle_columns(mid, lorder=3):
    case = case_of(mid, lorder)
    return [kr.oracle_column(case, j) for j in range(case.k)]


def oracle_cgs2(case, X, k, consistent, nrst, w=None):
    old = NekDVector.CONSISTENT_RST
    NekDVector.CONSISTENT_RST = consistent
    try:
        w = kr.to_oracle(case, case.w[0] if w is None else w, nrst)
        h = cgs2_step(X[:k], w)
        beta = w.norm()
        w.scal(1.0 / beta)
    finally:
        NekDVector.CONSISTENT_RST = old
    return {"h": h, "beta": beta, "w": kr.from_oracle(case, w), "nrst": w.nrst}


def agree(case, got, ref, orig=None):
    dev = kr.deviations(case, got, ref, orig)
    print("largest deviation %.2e" % max(dev.values()))
    assert max(dev.values()) < AGREE, dev


@pytest.mark.parametrize("mid,k", [(m, k) for m in "ABCD" for k in kr.CGS2_K[m]])
def test_oracle_cgs2_matches_reference(prec, mid, k):
    """cgs2_step + norm + scal on NekDVectors, consistent history, at every mesh and k of the GPU file.  Measured: the largest
    deviation of any compared quantity is 2.1e-15 (mesh A, k = 128), against the bound of 1e-14."""
    case = case_of(mid)
    agree(case, oracle_cgs2(case, oracle_columns(mid), k, True, 2), ref_of(mid, k), case.w[0])


@pytest.mark.parametrize("mid,k", [("B", 9), ("C", 9), ("C", 30)])
def test_oracle_cgs2_literal_history_matches_reference(prec, mid, k):
    """NekDVector.axpby(consistent_rst=False): the history of w receives the main-block corrections V h1 and V h2."""
    case = case_of(mid)
    ref = kr.cgs2_ref(case, k, consistent=False)
    agree(case, oracle_cgs2(case, oracle_columns(mid), k, False, 2), ref, case.w[0])
    dev = kr.deviations(case, kr.cgs2_ref(case, k, consistent=True), ref)                # the two modes are different answers
    assert min(d for key, d in dev.items() if isinstance(key, tuple) and key[0] == "hist") > 1e-3


def test_oracle_cgs2_literal_history_of_the_batch_lanes(prec):
    """The references of the literal-history batch of tests/test_gpu_krylov_oracle.py: lanes on their own bases with 0, 2 and 1 valid
    levels, w scaled by 10^-l.  Levels beyond nrst come back bit for bit."""
    k = kr.LITERAL_BATCH["k"]
    for l, nrst in enumerate(kr.LITERAL_BATCH["nrst"]):
        case = kr.lane_case(kr.LITERAL_BATCH["mid"], l)
        w = kr.lane_w(case, l)
        X = [kr.oracle_column(case, j) for j in range(k)]
        agree(case, oracle_cgs2(case, X, k, False, nrst, w), kr.cgs2_ref(case, k, consistent=False, w=w, nrst=nrst), w)


def test_oracle_cgs2_short_history_and_lorder_1(prec):
    """w with one valid level against columns with two: level 1 is combined and scaled, level 2 comes back bit for bit; lorder = 1:
    no history at all."""
    case = case_of("C")
    agree(case, oracle_cgs2(case, oracle_columns("C"), 24, True, 1), kr.cgs2_ref(case, 24, nrst=1), case.w[0])
    c1 = case_of("C", 1)
    agree(c1, oracle_cgs2(c1, oracle_columns("C", 1), 24, True, 0), kr.cgs2_ref(c1, 24, nrst=0), c1.w[0])


@pytest.mark.parametrize("mid", ["B", "C"])
@pytest.mark.parametrize("s", [2, 4])
def test_oracle_block_cgs2_matches_its_formulas(prec, mid, s):
    case, k = case_of(mid), 9
    V = oracle_columns(mid)[:k] + [kr.to_oracle(case, case.w[v], 2) for v in range(s)]
    coef = o_block_cgs2(V, k, s)
    rcoef, rW = kr.block_cgs2_ref(case, k, case.w[:s])
    assert np.max(np.abs(coef - rcoef)) < AGREE * np.max(np.abs(rcoef)), np.max(np.abs(coef - rcoef))
    for v in range(s):
        agree(case, {"w": kr.from_oracle(case, V[k + v]), "nrst": V[k + v].nrst}, {"w": rW[v], "nrst": 2})


@pytest.mark.parametrize("k", [1, 9, 17])
@pytest.mark.parametrize("consistent", [True, False])
def test_oracle_lincomb_matches_reference(prec, k, consistent):
    """Columns with 0, 1 and 2 valid levels: the combination carries max nrst levels in consistent mode, none in literal mode."""
    case = case_of("C")
    X = oracle_columns("C")
    c = np.random.default_rng(k).standard_normal(k)
    saved = case.col_nrst.copy()
    old = NekDVector.CONSISTENT_RST
    NekDVector.CONSISTENT_RST = consistent
    try:
        case.col_nrst[:] = (np.arange(case.k) + 1) % 3                         # 1, 2, 0, 1, ..
        for j in range(k):
            X[j].nrst = int(case.col_nrst[j])
        out = lincomb(X, c, k)
        agree(case, {"w": kr.from_oracle(case, out), "nrst": out.nrst}, kr.combine_ref(case, k, c, consistent))
    finally:
        NekDVector.CONSISTENT_RST = old
        case.col_nrst[:] = saved
        for j in range(k):
            X[j].nrst = int(saved[j])


MUTANTS = ["h2_zero", "h2_from_w", "h2_drops_chunk_tail", "skip_column_last", "skip_column_64", "history_h2_only", "pressure_untouched"]


@pytest.mark.parametrize("mid,k,mutant", [(m, k, mu) for m, k in (("A", 131), ("A", 24), ("C", 40), ("D", 30)) for mu in MUTANTS
                                           if k > 64 or mu != "skip_column_64"])
def test_comparison_sees_a_broken_second_pass(prec, mid, k, mutant):
    """Each mutant of the reference moves a compared quantity by at least 1e-9 relative (1000x the tolerance) when the basis is off
    orthonormal by 1e-2."""
    case = case_of(mid)
    name = {"skip_column_last": "skip_column_%d" % (k - 1)}.get(mutant, mutant)
    dev = kr.deviations(case, kr.cgs2_ref(case, k, mutant=name), ref_of(mid, k))
    print(mutant, "moves the result by %.2e" % max(dev.values()))
    assert max(dev.values()) > 1e-9, dev


def test_orthonormal_basis_hides_the_second_pass(prec):
    """eps = 0, what the older tests build: dropping the second projection altogether moves nothing by more than 1e-13 -- why an
    orthonormal set-up cannot test a re-orthogonalising kernel."""
    case = case_of("C").with_eps(0.0)
    dev = kr.deviations(case, kr.cgs2_ref(case, 40, mutant="h2_zero"), kr.cgs2_ref(case, 40))
    print("h2 := 0 on an orthonormal basis moves the result by %.2e" % max(dev.values()))
    assert max(dev.values()) < 1e-13, dev
