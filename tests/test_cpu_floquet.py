"""CPU suite: the numpy statement of the coupled (orbit) step, tests/floquet_ref.py, has the properties the GPU tests rely on, on the
GPU tests' own inputs."""
import numpy as np

import floquet_ref as fr
from oracle.lns import LNSConfig
from oracle.vectors import NekDVector


def test_zero_base_flow_coupled_equals_frozen():
    """U = 0 with homogeneous walls stays 0 under the nonlinear step, so the coupled operator is the frozen one about zero: both
    history slots included, to 1e-14.  (dt fixed: a zero base flow has no CFL number.)"""
    hm, sem = fr.case_mesh("A")
    ref = fr.FloquetRef(sem, LNSConfig(**fr.case_cfg("A")))
    X0 = NekDVector(sem)
    v = fr.start_vector(sem)
    c, end = ref.coupled_matvec(X0, v)
    f = ref.frozen_matvec(X0, v)
    assert all(np.array_equal(a, 0.0 * a) for a in end.v)
    sc = max(np.abs(a).max() for a in f.v)
    worst = max(np.max(np.abs(a - b)) for a, b in zip(c.main_fields(), f.main_fields())) / sc
    for r in range(2):
        worst = max(worst, max(np.max(np.abs(a - b)) for a, b in zip(c.rst_fields(r), f.rst_fields(r))) / sc)
    print("zero base flow, coupled against frozen: %.3e" % worst)
    assert c.nrst == f.nrst == 2
    assert worst <= 1e-14


def test_coupled_step_is_the_tangent_of_the_nonlinear_map():
    """2-D walled box, 3 x 3 elements, lx1 = 6, Re = 50; X0 the vortex of floquet_ref.orbit_state("A") at amplitude 1; dt = 0.01
    fixed, 6 steps, no_history, vtol = ptol = 1e-13; v a normalised random vector.  With
    e(eps) = |[Phi(X0 + eps v) - Phi(X0 - eps v)] / 2 eps - M v| / |M v|:  e(1e-2) / e(1e-3) >= 50, e(1e-3) <= 1e-5, and the frozen
    operator about X0 misses at eps = 1e-3 by more than 100 e(1e-3).
    Measured with this pair and amplitude (nothing had to be moved): X0 loses 6.1 % of its norm over the interval, e(1e-2) = 4.05e-6,
    e(1e-3) = 4.05e-8 (ratio 100.0), frozen operator 1.54e-2."""
    hm, sem = fr.case_mesh("A")
    ref = fr.FloquetRef(sem, LNSConfig(**fr.tangent_cfg()))
    X0 = fr.orbit_state("A")
    v = fr.start_vector(sem)
    Mv, end = ref.coupled_matvec(X0, v)
    Fv = ref.frozen_matvec(X0, v)
    assert ref.nsteps == 6 and Mv.nrst == 0
    # the base-flow half of the coupled step is the oracle's nonlinear map, and the vortex decays visibly
    assert fr.vec_err(end, ref.flow(X0)) <= 1e-12
    decay = 1.0 - end.norm() / X0.norm()
    e = [fr.tangent_errors(ref.flow, Mv, X0, v, eps) for eps in fr.EPS]
    e_frozen = fr.tangent_errors(ref.flow, Fv, X0, v, fr.EPS[1])
    print("tangent test (oracle): decay of X0 %.3f, e(%g) = %.3e, e(%g) = %.3e, ratio %.1f, frozen operator %.3e"
          % (decay, fr.EPS[0], e[0], fr.EPS[1], e[1], e[0] / e[1], e_frozen))
    assert decay > 0.02
    fr.check_tangent(e[0], e[1], e_frozen)
