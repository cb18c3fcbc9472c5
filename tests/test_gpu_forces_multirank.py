"""Wall forces on 2 and 3 ranks (one GPU, the shared-memory validation transport) against the single-rank run: case B, the face list of
tests/test_gpu_forces.py, the same on every rank; object 1 has no face on the first rank's elements.  Every face must be counted by
exactly one rank: the local face counts sum to the list's length and the areas equal the single-rank areas.

Bounds.  sample() of a fixed vector: every face's share is the same arithmetic on every partition, only the grouping of the sum over
the faces changes (per rank, then across the ranks), so |difference| <= (number of faces of the object + number of ranks) x eps x (the
twin's sum of the absolute values of the summands).  The areas the same with |N_q|.  The DNS force series: 1e-10 of max|F|, the bound
of a run against another run of the same discretisation (tests/test_gpu_dns_multirank.py)."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import floquet_ref as fr
import forces_ref as fo
import forces_multirank_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "forces_multirank_worker.py")
EPS = np.finfo(np.float64).eps


def launch(world, outdir):
    seg = "/nlg_%s" % uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), seg, str(outdir)], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=240)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        try:
            os.unlink("/dev/shm" + seg)
        except OSError:
            pass
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "WORKER_OK" in o, "rank %d of %d:\n%s" % (r, world, o[-3000:])
    return [dict(np.load(os.path.join(outdir, "forces_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    return launch(1, tmp_path_factory.mktemp("forces_w1"))[0]


@pytest.mark.parametrize("world", [2, 3])
def test_forces_do_not_depend_on_the_partition(tmp_path, single, world):
    hm, sem = fr.case_mesh("B")
    objects = fo.case_objects("B", hm)
    parts = launch(world, tmp_path)
    for p in parts[1:]:                                   # sample, info and the flush all-reduce: every rank holds the global sums
        for key in ("sample", "area", "force", "time"):
            assert np.array_equal(p[key], parts[0][key]), key
    got = parts[0]
    nfaces = sum(len(o) for o in objects)
    assert sum(int(p["nlocal"]) for p in parts) == nfaces == int(single["nlocal"])   # every face exactly once
    assert np.array_equal(sum(p["per_object"] for p in parts), [len(o) for o in objects])
    assert parts[0]["per_object"][1] == 0                 # object 1 has no face on the first rank
    vel, pr = worker.random_fields(sem)
    _, _, refa = fo.sample(sem, objects, (vel, pr, None), worker.NU, err=True)
    nf = np.array([len(o) for o in objects])[:, None]
    bound = (nf + world) * EPS * refa
    d = np.abs(got["sample"] - single["sample"])
    rs = float(np.max(np.where(d == 0.0, 0.0, d / np.maximum(bound, 1e-300))))
    ea = np.abs(got["area"] - single["area"])
    ba = (nf[:, 0] + world) * EPS * single["area"]
    scale = np.abs(single["force"]).max()
    ef = np.abs(got["force"] - single["force"]).max() / scale
    print("%d ranks against one: sample %.2e of the regrouping bound, areas %s off by %.1e (bound %.1e), force series %.3e of max|F| = %.3e"
          % (world, rs, got["area"], ea.max(), ba.min(), ef, scale))
    assert rs <= 1.0 and np.all(ea <= ba)
    assert got["force"].shape == single["force"].shape == (worker.NSTEPS + 1, 3, 13)
    assert np.array_equal(got["time"], single["time"]) and ef <= 1e-10
