"""The overlapping Schwarz preconditioner after the change of its data protocol (every ghost value written once, by its
producer, into the slot its consumer reads) against the output of the protocol it replaced (pairs-only gather-scatters
summing the two copies of every face slot): tests/golden/pprec_exchange.npz (3-D) and pprec_exchange_2d.npz (2-D), made by
tests/golden/make_pprec_exchange.py.
3-D: walls, periodic faces and two faces of one element with the same neighbour; lx1 = 8 (k_fdm_ext_mfma8) and 10
(k_fdm_ext<10, 1, 2>, k_q1_restrict_local3s<8>).  2-D (k_fdm_ext2): walls, a fully periodic box, and elements whose two y faces
are neighbours of each other; lx1 = 6 and 8."""
import os
import sys

import numpy as np
import pytest

from neklab_amd import host
from neklab_amd.mesh import box_mesh

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_pprec_exchange import FIXTURES, SEEDS, apply, inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = [(which, name) for which in sorted(FIXTURES) for name in sorted(FIXTURES[which][0])]


@pytest.mark.parametrize("which,name", PARAMS, ids=[name for _, name in PARAMS])
def test_pprec_matches_pairs_protocol(gpu_ctx, which, name):
    cases, fixture = FIXTURES[which]
    kw = cases[name]
    gm = host.Mesh(gpu_ctx, box_mesh(kw["nel"], kw["n"], periodic=kw["periodic"], deform=kw["deform"]))
    ref = np.load(os.path.join(GOLDEN, fixture))
    for seed in SEEDS:
        r = inputs(gm, seed)
        for wc in (0, 1):
            z = apply(gpu_ctx, gm, r, wc)
            z0 = ref["%s_s%d_c%d" % (name, seed, wc)]
            err = np.linalg.norm(z - z0) / np.linalg.norm(z0)
            assert err <= 1e-13, "%s seed %d coarse %d: relative difference %.3e" % (name, seed, wc, err)
            z2 = apply(gpu_ctx, gm, r, wc)
            assert np.array_equal(z, z2), "%s seed %d coarse %d: two applications differ" % (name, seed, wc)
