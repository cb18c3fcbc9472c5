"""CPU: the numpy reference of the convective terms (tests/conv_ref.py), on the meshes and fields of tests/test_gpu_conv_lanes.py.

1. It agrees with the oracle (conv_weak, scalar_times_grad_weak, lns_conv_weak of oracle/sem.py), which sums in another order:
   8.0e-16 of max|reference| at worst (lx1 = 12) when this was written.
2. Re-evaluated in long double from the same float64 inputs it moves by at most 5.9e-16 of max|reference| (the worst case, at
   lx1 = 9; printed).  Asserted: 1e-14, 16 times that and 100 times under the 1e-12 bound of the GPU test.
   The oracle check uses the same 1e-14: two float64 evaluations that far from the long-double value are at most twice that apart.
3. The scalar gradient term is the transpose of the (u . grad) Theta part of the transport term.
4. On an undeformed box with polynomial fields of total degree <= 2 every term is bm1 times its pointwise closed form.
5. The random fields load every precomputed base-flow factor: within Ur, within GU and within GT the component maxima differ by
   less than a factor 10, so no kernel input is hidden under another."""
import numpy as np
import pytest

import conv_ref as cr
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

TOL = 1e-14
ADJ = pytest.mark.parametrize("adjoint", [False, True], ids=["direct", "adjoint"])
EACH = pytest.mark.parametrize("i", range(len(cr.CASES)), ids=cr.IDS)


def dist(got, ref):
    """max|got - ref| over max|ref|, in the number format of the arguments"""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@EACH
@ADJ
def test_agrees_with_the_oracle(i, adjoint):
    _, sem, U, Theta, ins = cr.case(i)
    worst = 0.0
    for v in range(cr.NLANES):
        u, theta = ins[v]
        vel, tr, gr = cr.case_refs(i, v, adjoint)
        o_tr = -sem.conv_weak(U, theta) if adjoint else sem.conv_weak(U, theta) + sem.conv_weak(u, Theta)
        o_gr = sem.scalar_times_grad_weak(theta, Theta)
        o_vel = sem.lns_conv_weak(U, u, adjoint=adjoint)
        d = [dist(tr, o_tr)] + [dist(a, b) for a, b in zip(gr, o_gr)] + [dist(a, b) for a, b in zip(vel, o_vel)]
        worst = max(worst, max(d))
        assert max(d) <= TOL, (v, d)
    print("%s %s: reference against the oracle, worst %.2e of max|ref|" % (cr.IDS[i], "adjoint" if adjoint else "direct", worst))


@EACH
@ADJ
def test_long_double_re_evaluation(i, adjoint):
    _, sem, U, Theta, ins = cr.case(i)
    assert np.finfo(np.longdouble).eps < 1e-18   # a real extended format, not an alias of float64
    u, theta = ins[0]
    vel, tr, gr = cr.case_refs(i, 0, adjoint)
    L = np.longdouble
    d = [dist(tr, cr.scalar_transport(sem, U, Theta, u, theta, adjoint, dtype=L))]
    d += [dist(a, b) for a, b in zip(gr, cr.scalar_grad(sem, Theta, theta, dtype=L))]
    d += [dist(a, b) for a, b in zip(vel, cr.velocity_term(sem, U, u, adjoint, dtype=L))]
    print("%s %s: float64 against long double, worst %.2e of max|ref|" % (cr.IDS[i], "adjoint" if adjoint else "direct", max(d)))
    assert max(d) <= TOL, d


@EACH
def test_gradient_term_is_the_transpose(i):
    _, sem, U, Theta, ins = cr.case(i)
    u, theta = ins[0]
    L = np.longdouble
    zero = [np.zeros(sem.shape1)] * sem.dim
    for dtype, bound in ((np.float64, 1e-13), (L, 1e-16)):
        ugt = cr.scalar_transport(sem, zero, Theta, u, np.zeros(sem.shape1), dtype=dtype)   # J^T[u . GT] alone
        gr = cr.scalar_grad(sem, Theta, theta, dtype=dtype)
        lhs = np.sum(theta.astype(dtype) * ugt)
        terms = [u[k].astype(dtype) * gr[k] for k in range(sem.dim)]
        rhs = sum(np.sum(t) for t in terms)
        size = sum(np.abs(t).sum() for t in terms)
        print("%s %s: sum theta J^T[u.GT] = %.6e, difference to sum u_i grad_i %.2e of the sum of magnitudes" %
              (cr.IDS[i], np.dtype(dtype).name, float(lhs), float(abs(lhs - rhs) / size)))
        assert abs(lhs - rhs) <= bound * size


@pytest.mark.parametrize("nel,n", [((2, 2), 5), ((2, 2, 2), 8), ((2, 1, 2), 6)], ids=["2d_n5", "3d_n8", "3d_n6"])
def test_exact_answer_on_polynomial_fields(nel, n):
    sem = SEM(box_mesh(nel, n, periodic=(False,) * len(nel), deform=0.0))
    U, Theta, u, theta, exact = cr.poly_fields(sem)
    for adjoint in (False, True):
        pairs = [("transport", cr.scalar_transport(sem, U, Theta, u, theta, adjoint), exact["transport"][adjoint])]
        pairs += [("velocity %d" % k, g, e) for k, (g, e) in enumerate(zip(cr.velocity_term(sem, U, u, adjoint), exact["velocity"][adjoint]))]
        pairs += [("gradient %d" % k, g, e) for k, (g, e) in enumerate(zip(cr.scalar_grad(sem, Theta, theta), exact["grad"]))]
        for name, got, ref in pairs:
            d = dist(got, ref)
            print("%d-D lx1 = %d %s %s: %.2e of max|exact|" % (sem.dim, n, "adjoint" if adjoint else "direct", name, d))
            assert d <= 1e-12, name


@EACH
def test_every_base_flow_factor_carries_weight(i):
    _, sem, U, Theta, ins = cr.case(i)
    for name, group in zip(("Ur", "GU", "GT"), cr.base_factors(sem, U, Theta)):
        top = [np.abs(g).max() for g in group]
        print("%s %s: component maxima %s" % (cr.IDS[i], name, " ".join("%.2e" % t for t in top)))
        assert max(top) < 10.0 * min(top), name
    # and every input: lane v at 10^(-3 v) of lane 0, all components of one lane alike
    for v, (u, theta) in enumerate(ins):
        top = [np.abs(a).max() for a in u] + [np.abs(theta).max()]
        assert max(top) < 10.0 * min(top) and 0.1 * cr.LANE_SCALE[v] < max(top) < 10.0 * cr.LANE_SCALE[v]
