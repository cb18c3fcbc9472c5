"""Wavenumber lanes across ranks: 2 ranks on ONE GPU (shared-memory validation transport, as tests/test_gpu_multirank.py), the
homogeneous direction crossing the rank boundary, two lanes with different wavenumbers.  nlg_linop_project_block and one block matvec
against the single-rank run of the same global mesh, to the tolerances of the `proj` case of test_partition_independent."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "sweep_multirank_worker.py")


def launch(world, outdir, mult):
    seg = "/nlg_%s" % uuid.uuid4().hex[:16]
    env = dict(os.environ, NLG_PCG_SINGLE_RED="0")
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), seg, str(outdir), str(mult)], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=300)
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
    return [np.load(os.path.join(outdir, "sweep_w%d_r%d.npz" % (world, r))) for r in range(world)]


def test_wavenumber_lanes_are_partition_independent(tmp_path):
    world = 2
    parts = launch(world, tmp_path, 1)
    ref = launch(1, tmp_path, world)[0]          # the single-rank run of the same global mesh
    for p in parts:
        np.testing.assert_array_equal(p["scal"], parts[0]["scal"])
    np.testing.assert_allclose(parts[0]["scal"], ref["scal"], rtol=1e-10, atol=1e-12)
    assert parts[0]["stats"][0] <= 1.25 * ref["stats"][0] + 5, (parts[0]["stats"], ref["stats"])
    for key in ref.files:
        if key in ("scal", "stats"):
            continue
        got = np.concatenate([p[key].reshape(-1) for p in parts])
        want = ref[key].reshape(-1)
        assert got.shape == want.shape, key
        tol = 1e-13 if key.startswith("v") else 1e-9
        scale = np.max(np.abs(want)) + 1e-300
        assert np.max(np.abs(got - want)) <= tol * scale, (key, np.max(np.abs(got - want)) / scale)
    # the lanes ran at different wavenumbers: of the pressure (cos z + cos 2z) y both were given, lane 0 keeps cos 2z and lane 1 cos z
    p0, p1 = (np.concatenate([p["pvp%d" % l].reshape(-1) for p in parts]) for l in range(2))
    assert np.max(np.abs(p0 - p1)) > 0.5 * np.max(np.abs(p0))
