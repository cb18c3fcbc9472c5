"""nlg_basis_block_dot (k_block_dot of csrc/vec.hip: tiles of 8 basis vectors, chunk and tile both carried by blockIdx.x) on
2 x 2 x 2 elements at lx1 = 8, k on both sides of one, two and eight tiles: against the extended-precision reference with the bound
of tests/test_gpu_krylov_oracle.py::test_block_dot_and_block_axpy (1e-13 of max|h_ref|), and bit for bit against itself with the same
vectors placed in a basis of another nvec -- the partial sums of column j must not depend on where the last tile ends or on how many
tiles the launch carries."""
import numpy as np
import pytest

import krylov_ref as kr
from neklab_amd import host

KS = (1, 8, 9, 16, 17, 64)


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    from neklab_amd.mesh import box_mesh
    from oracle.sem import SEM
    hm = box_mesh((2, 2, 2), 8, periodic=(True, False, False), deform=0.04)
    case = kr.make_case(SEM(hm), max(KS), seed=7)
    gm = host.Mesh(gpu_ctx, hm)
    # the same 64 columns in a basis of 65 and in one of 71 vectors (nvec = 71: nine tiles would cover it, the last one of 7)
    bases = [host.KrylovBasis(gm, nvec) for nvec in (max(KS) + 1, max(KS) + 7)]
    w, tmp = host.nek_dvector(gm), host.nek_dvector(gm)
    for B in bases:
        for j in range(case.k):
            kr.upload(B[j], case, np.stack([case.cols[lev][j] for lev in range(3)]), 2, tmp)
    kr.upload(w, case, case.w[0], 2, tmp)
    yield case, bases, w
    for B in bases:
        B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_block_dot_against_the_reference_and_across_bases(rig, k):
    case, bases, w = rig
    href = kr.block_dot_ref(case, k, case.w[0])
    h = bases[0].block_dot(k, w)
    print("block_dot deviation %.2e" % (np.max(np.abs(h - href)) / np.max(np.abs(href))))
    assert np.max(np.abs(h - href)) < 1e-13 * np.max(np.abs(href))
    assert np.array_equal(h, bases[1].block_dot(k, w)), "the coefficients depend on nvec of the basis"
    if k > 1:      # ... and column j < k - 1 has the same sum whether or not a further column shares its launch
        assert np.array_equal(h[:k - 1], bases[0].block_dot(k - 1, w))
