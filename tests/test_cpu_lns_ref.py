"""CPU: the numpy restatement of the strong-form LNS operator (tests/lns_ref.py) gives the exact answer on polynomial fields.

Undeformed boxes; U = (1 + y/2, 0.3 x - 0.2 z, 0.1 x), u = (y^2 + x z, x^2 - y z, x y), p = x^2 - y sampled on mesh 2, unmasked,
Re = 40: L u = (2, 2, 0) / Re - [(U.grad) u + (u.grad) U] - (2 x, -1, 0), with the matching closed form of the adjoint term.  Every
product has degree <= 2 <= lx1 - 2, for which the dealiased weak term over the lumped mass is the pointwise product exactly; what is
left is rounding: 2.1e-13 absolute at an output scale of 9 when this was written.  Bound: 1e-12 x scale."""
import numpy as np
import pytest

import lns_ref
from neklab_amd.mesh import box_mesh
from oracle.sem import SEM

MESHES = [dict(nel=(2, 2), n=5, periodic=(False, False)), dict(nel=(2, 2, 2), n=8, periodic=(False, False, False)),
          dict(nel=(2, 1, 2), n=6, periodic=(True, False, False))]


@pytest.mark.parametrize("case", MESHES, ids=lambda c: "x".join(map(str, c["nel"])) + "_n%d" % c["n"])
@pytest.mark.parametrize("adjoint", [False, True], ids=["direct", "adjoint"])
def test_polynomial_fields_give_the_closed_form(case, adjoint):
    sem = SEM(box_mesh(case["nel"], case["n"], periodic=case["periodic"], deform=0.0))
    U, u, p, exact = lns_ref.poly_fields(sem)
    ones = [np.ones(sem.shape1)] * sem.dim
    # the bound is on L u itself, at the scale of L u: a term on its own (the Laplacian is 2 / Re = 0.05 here) carries the rounding
    # of its O(1) input through two differentiations and is printed only
    for name, coef in lns_ref.ROUTINES.items():
        got = lns_ref.lns_strong(sem, U, u, p, 40.0, coef, adjoint, mask=ones)
        ref = exact(40.0, coef, adjoint)
        scale = max(np.abs(r).max() for r in ref)
        err = max(np.abs(g - r).max() for g, r in zip(got, ref))
        print("%s %s: scale %.3g, absolute error %.3e" % (name, "adjoint" if adjoint else "direct", scale, err))
        if name == "apply_L":
            assert err <= 1e-12 * scale


def test_mask_is_applied_to_the_input_only():
    sem = SEM(box_mesh((2, 2), 5, periodic=(False, False), deform=0.0))
    U, u, p, _ = lns_ref.poly_fields(sem)
    assert any((m == 0).any() for m in sem.mask)
    masked = lns_ref.lns_strong(sem, U, [m * a for m, a in zip(sem.mask, u)], p, 40.0, mask=[np.ones(sem.shape1)] * 2)
    got = lns_ref.lns_strong(sem, U, u, p, 40.0)
    assert all(np.array_equal(a, b) for a, b in zip(got, masked))
    assert any(np.abs(g[m == 0]).max() > 0 for g, m in zip(got, sem.mask))   # the output is not masked
