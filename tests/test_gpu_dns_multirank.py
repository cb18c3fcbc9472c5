"""A DNS run with history points on 2 and 3 ranks (one GPU, the shared-memory validation transport) against the single-rank run: case
B, 3 steps, points on the partition interfaces among the points (an edge four elements share, the vertex all eight share).  Every point
must be sampled by exactly one rank -- a field that is 1 everywhere samples to 1, not to 0 or 2 -- and the winner (global element id,
reference coordinates) must not depend on the partition.  Series: 1e-10 of max|U| and of |U|_M, the bound of a run against another
run of the same discretisation (tests/test_gpu_dns.py)."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "dns_multirank_worker.py")
_single = {}


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
    return [dict(np.load(os.path.join(outdir, "dns_w%d_r%d.npz" % (world, r)))) for r in range(world)]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    return launch(1, tmp_path_factory.mktemp("dns_w1"))[0]


@pytest.mark.parametrize("world", [2, 3])
def test_series_do_not_depend_on_the_partition(tmp_path, single, world):
    parts = launch(world, tmp_path)
    for p in parts[1:]:                                   # the flush all-reduces: every rank holds the global series
        for key in ("time", "probe", "dist", "ones", "elem", "status", "rst"):
            assert np.array_equal(p[key], parts[0][key]), key
    got = parts[0]
    assert got["probe"].shape == single["probe"].shape == (4, 7, 4)
    assert np.array_equal(got["elem"], single["elem"]) and np.array_equal(got["status"], single["status"])
    assert np.max(np.abs(got["rst"] - single["rst"])) <= 1e-14
    assert np.max(np.abs(got["ones"] - 1.0)) <= 1e-13, got["ones"]        # every point has exactly one owner
    ep = np.abs(got["probe"] - single["probe"]).max() / single["umax"]
    ed = np.abs(got["dist"] - single["dist"]).max() / single["unorm"]
    print("%d ranks against one: history points %.3e of max|U|, d(t) %.3e of |U|" % (world, ep, ed))
    assert np.array_equal(got["time"], single["time"])
    assert ep <= 1e-10 and ed <= 1e-10
