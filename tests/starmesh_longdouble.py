"""The float64 oracle's propagator on the star mesh of tests/test_gpu_starmesh.py (k = 5, lx1 = 8, two layers) against the SAME code
evaluated in long double from the same float64 inputs: how far the reference itself lies from the exact result of its own iteration
at a fixed iteration count.  Not a test: a measurement, run by hand,

    python tests/starmesh_longdouble.py 200      (fixed_iters_p; fixed_iters_v = 30)

whose output stands beside the bounds of test_gpu_starmesh.py::test_matvec_fixed_iterations.  The oracle modules are made to
allocate and accumulate in long double by a numpy stand-in patched into them, in this process only.
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle.lns as olns  # noqa: E402
import oracle.sem as osem  # noqa: E402
import oracle.vectors as ovec  # noqa: E402
import test_gpu_n8 as t8  # noqa: E402
from oracle.lns import ExptA, LNSConfig  # noqa: E402
from oracle.sem import SEM  # noqa: E402
from oracle.vectors import NekDVector  # noqa: E402
from starmesh import star_mesh  # noqa: E402

L = np.longdouble


class LongDoubleNumpy:
    """numpy with long double as the default floating type, and a bincount that takes long-double weights"""

    def __getattr__(self, k):
        return getattr(np, k)

    def zeros(self, shape, dtype=None, **kw):
        return np.zeros(shape, dtype=L if dtype is None else dtype, **kw)

    def ones(self, shape, dtype=None, **kw):
        return np.ones(shape, dtype=L if dtype is None else dtype, **kw)

    def empty(self, shape, dtype=None, **kw):
        return np.empty(shape, dtype=L if dtype is None else dtype, **kw)

    def asarray(self, a, dtype=None, **kw):
        return np.asarray(a, dtype=L if dtype in (np.float64, float) else dtype, **kw)

    def bincount(self, x, weights=None, minlength=0):
        if weights is None:
            return np.bincount(x, minlength=minlength)
        out = np.zeros(max(int(x.max()) + 1, minlength), dtype=L)
        np.add.at(out, x, np.asarray(weights, dtype=L))
        return out


def main(itp):
    assert np.finfo(L).eps < 1e-18
    hm = star_mesh(5, 8, 2)
    sem = SEM(hm)
    U, ov = t8.base_flow(sem), t8.start_vector(sem)
    kw = dict(re=50.0, torder=3, tau=0.03, vtol=1e-13, ptol=1e-13, maxit_v=400, maxit_p=4000, fixed_iters_v=30, fixed_iters_p=itp)
    res = {}
    for adj in (False, True):
        oA = ExptA(sem, U, LNSConfig(**kw))
        o1 = oA.matvec(ov, adjoint=adj)
        res[adj] = (o1, oA.matvec(o1, adjoint=adj))
    # ---- the same in long double: arrays allocated by the oracle, its scalars (float(...)) and its gather-scatter
    for mod in (osem, olns, ovec):
        mod.np = LongDoubleNumpy()
    olns.float = osem.float = L
    seml = SEM(dataclasses.replace(hm, x=hm.x.astype(L), y=hm.y.astype(L), z=hm.z.astype(L), mask=[m.astype(L) for m in hm.mask],
                                   tmask=hm.tmask.astype(L)))
    vin = NekDVector(seml)
    for a, b in zip(vin.v, ov.v):
        a[...] = b
    vin.pr[...] = ov.pr
    for adj in (False, True):
        oA = ExptA(seml, [a.astype(L) for a in U], LNSConfig(**kw))
        l1 = oA.matvec(vin, adjoint=adj)
        assert l1.v[0].dtype == L and l1.pr.dtype == L
        l2 = oA.matvec(l1, adjoint=adj)          # chained, as the float64 run chains its own first result
        for k, (o, l) in enumerate(zip(res[adj], (l1, l2)), 1):
            sc = max(np.abs(a).max() for a in o.v)
            dv = float(max(np.abs(a - b).max() for a, b in zip(o.v, l.v)) / sc)
            dp = float(np.abs(o.pr - l.pr).max() / max(np.abs(o.pr).max(), sc))
            dr = float(max(np.abs(a - b).max() / np.abs(c).max() for r in range(2) for a, b, c in zip(o.v_rst[r], l.v_rst[r], o.v)))
            print("30/%d %s matvec #%d: float64 oracle against long double: velocity %.3e pressure %.3e history %.3e"
                  % (itp, "adjoint" if adj else "direct", k, dv, dp, dr), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]))
