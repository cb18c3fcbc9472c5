"""The convective terms as the time stepper launches them (nlg_op_conv_lanes, nlg_op_conv_scalar: s = 1..4 vectors as lanes of one
buffer, ONE sem_conv_apply / sem_conv_scalar_apply / sem_scalar_grad_apply call) against tests/conv_ref.py.

Shapes (tests/conv_ref.py CASES, deform = 0.05): the smallest that select each path

    lx1       nel       velocity term                              temperature terms
    6 (2-D)   (3,2)     generic tensor path, once per lane         generic
    5, 6, 7   (2,2,2)   k_conv3<N, 3N/2, NT, false, ML> (lane loop) generic
    8         (2,2,2)   k_conv3m<8>, set-up by k_interp4_mfma       k_conv3m_scalar<8>
    9         (2,2,2)   k_conv3<9,13,256,true> (dynamic LDS)        k_conv3s_scalar<9>
    10        (2,2,2)   k_conv3m<10,true>                           k_conv3m_scalar<10,true>
    10/lxd16  (3,1,1)   generic 3-D                                 generic
    12        (2,1,2)   k_conv3s<12,18,7,1>, E * nl blocks          generic

(The generic 3-D path is what lx1 = 11 would take; nlg_mesh_create refuses lx1 = 11, so the path is reached through a fine mesh that
is not 3 lx1 / 2: lx1 = 10 with lxd = 16, the fine mesh lx1 = 11 would have.)

Every component of the base flow, the base temperature and of each lane's input is an independent standard-normal field (all three
Ur, nine GU and three GT of comparable size: tests/test_cpu_conv_ref.py); lane v is scaled by 10^(-3 v) and compared with the
reference of its OWN input, per field and against that field's own maximum, so a small lane cannot hide behind a large one.

Tolerance: max|gpu - ref| < 1e-12 max|ref|, the convention for this operator in tests/test_gpu_ops.py and tests/test_gpu_lns.py; it
covers the 1e-13 geometry difference between device and oracle that test_mesh_geometry allows.  The reference itself is within 7e-16 of
its long-double value (tests/test_cpu_conv_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as cr
from neklab_amd import host
from neklab_amd._lib import vp

pytestmark = pytest.mark.gpu

TOL = 1e-12
SENTINEL = 12345.678
_dev = {}


def fresh(gm, value=SENTINEL):
    """a vector with one scalar that holds `value` in every field of every level, pressure and restart history included"""
    gv = host.nek_dvector(gm, 1)
    for k in list(range(gm.dim)) + [host.THETA]:
        gv.set_field(k, np.full(gm.lvn, value))
    gv.set_field(host.PR, np.full(gm.lpn, value))
    for irst in (1, 2):
        gv.save_rst(gv, irst)
    return gv


def dev_case(ctx, i):
    """the device mesh, base flow and the four input vectors of case i, uploaded once"""
    if i not in _dev:
        hm, sem, U, Theta, ins = cr.case(i)
        gm = host.Mesh(ctx, hm, lxd=cr.CASES[i].get("lxd", 0))

        def up(vel, theta):
            gv = fresh(gm, 0.5)
            for k in range(sem.dim):
                gv.set_field(k, vel[k])
            gv.set_field(host.THETA, theta)
            return gv

        _dev[i] = (gm, up(U, Theta), [up(u, theta) for u, theta in ins])
    return _dev[i]


def fields(gv):
    return [gv.get_field(k) for k in list(range(gv.mesh.dim)) + [host.THETA]]


def untouched(gv, written):
    """every field outside `written`, the pressure and all restart levels still hold the sentinel"""
    dim = gv.mesh.dim
    for irst in (0, 1, 2):
        for k in list(range(dim)) + [host.THETA, host.PR]:
            if irst == 0 and k in written:
                continue
            assert np.all(gv.get_field(k, irst) == SENTINEL), (k, irst)


def check_field(got, ref, what):
    """-> error as a fraction of the bound"""
    assert not np.isnan(got).any(), what
    scale = np.abs(ref).max()
    err = np.abs(got - ref.ravel()).max()
    assert err < TOL * scale, (what, err / scale)
    return err / (TOL * scale)


def run_both(gm, base, gins, adjoint):
    s = len(gins)
    ov, ot = [fresh(gm) for _ in range(s)], [fresh(gm) for _ in range(s)]
    gm.conv_lanes(base, gins, ov, adjoint)
    gm.conv_scalar(base, gins, ot, adjoint)
    return ov, ot


@pytest.mark.parametrize("adjoint", [0, 1], ids=["direct", "adjoint"])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=cr.IDS)
def test_lanes_against_reference(gpu_ctx, i, s, adjoint):
    gm, base, gins = dev_case(gpu_ctx, i)
    dim = gm.dim
    vel_w, sc_w = list(range(dim)), list(range(dim)) + [host.THETA]
    ov, ot = run_both(gm, base, gins[:s], adjoint)
    frac = {"velocity": 0.0, "transport": 0.0, "gradient": 0.0}
    for v in range(s):
        r_vel, r_tr, r_gr = cr.case_refs(i, v, adjoint)
        untouched(ov[v], vel_w)
        untouched(ot[v], sc_w)
        got_v, got_t = fields(ov[v]), fields(ot[v])
        for k in range(dim):
            frac["velocity"] = max(frac["velocity"], check_field(got_v[k], r_vel[k], ("velocity term", v, k)))
            frac["gradient"] = max(frac["gradient"], check_field(got_t[k], r_gr[k], ("scalar gradient term", v, k)))
        frac["transport"] = max(frac["transport"], check_field(got_t[dim], r_tr, ("scalar transport term", v)))
    print("FRACTION %s s=%d %s: velocity %.5f transport %.5f gradient %.5f of the 1e-12 bound" %
          (cr.IDS[i], s, "adjoint" if adjoint else "direct", frac["velocity"], frac["transport"], frac["gradient"]))
    if s == 1:
        # one lane: the kernels of nlg_op_conv, bit for bit
        one = fresh(gm)
        host.check(gm.lib.nlg_op_conv(gm.h, base.h, gins[0].h, one.h, adjoint))
        assert all(np.array_equal(a, b) for a, b in zip(fields(one)[:dim], fields(ov[0])[:dim]))
        untouched(one, vel_w)
    if s < 4:
        # no state survives a call: after a four-lane call the same call on fresh outputs gives the same bits
        run_both(gm, base, gins, adjoint)
        ov2, ot2 = run_both(gm, base, gins[:s], adjoint)
        for v in range(s):
            assert all(np.array_equal(a, b) for a, b in zip(fields(ov[v]), fields(ov2[v]))), v
            assert all(np.array_equal(a, b) for a, b in zip(fields(ot[v]), fields(ot2[v]))), v
            untouched(ov2[v], vel_w)
            untouched(ot2[v], sc_w)


@pytest.mark.parametrize("adjoint", [0, 1], ids=["direct", "adjoint"])
@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=cr.IDS)
def test_lane_order(gpu_ctx, i, adjoint):
    """permuting the inputs permutes the outputs, bit for bit"""
    gm, base, gins = dev_case(gpu_ctx, i)
    perm = [2, 0, 3, 1]
    ov, ot = run_both(gm, base, gins, adjoint)
    pv, pt = run_both(gm, base, [gins[p] for p in perm], adjoint)
    for v, p in enumerate(perm):
        assert all(np.array_equal(a, b) for a, b in zip(fields(pv[v]), fields(ov[p]))), (v, p)
        assert all(np.array_equal(a, b) for a, b in zip(fields(pt[v]), fields(ot[p]))), (v, p)


def test_refusals_leave_out_untouched(gpu_ctx):
    gm, base, gins = dev_case(gpu_ctx, 0)
    gm2 = dev_case(gpu_ctx, 1)[0]
    lib = gm.lib
    out = fresh(gm)
    other, bare_in, bare_out = fresh(gm2), host.nek_dvector(gm), host.nek_dvector(gm)
    for k in list(range(gm.dim)) + [host.PR]:
        bare_in.set_field(k, np.full(gm.lpn if k == host.PR else gm.lvn, 0.25))
        bare_out.set_field(k, np.full(gm.lpn if k == host.PR else gm.lvn, SENTINEL))

    def arr(*vs):
        return (vp * len(vs))(*[x.h for x in vs])

    def refused(rc, word):
        msg = lib.nlg_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
        untouched(out, [])
        for k in list(range(gm.dim)) + [host.PR]:
            assert np.all(bare_out.get_field(k) == SENTINEL)

    for fn in (lib.nlg_op_conv_lanes, lib.nlg_op_conv_scalar):
        refused(fn(gm.h, base.h, 0, arr(gins[0]), arr(out), 0), "out of range")
        refused(fn(gm.h, base.h, 5, arr(*(gins + [gins[0]])), arr(*([out] * 5)), 0), "out of range")
        refused(fn(gm.h, base.h, 1, arr(other), arr(out), 0), "another mesh")
        refused(fn(gm.h, base.h, 2, arr(gins[0], gins[1]), arr(out, other), 1), "another mesh")
        refused(fn(gm.h, other.h, 1, arr(gins[0]), arr(out), 0), "another mesh")
        refused(fn(gm2.h, base.h, 1, arr(gins[0]), arr(out), 0), "another mesh")
    refused(lib.nlg_op_conv_scalar(gm.h, bare_in.h, 1, arr(gins[0]), arr(out), 0), "no scalar")
    refused(lib.nlg_op_conv_scalar(gm.h, base.h, 2, arr(gins[0], bare_in), arr(out, out), 0), "no scalar")
    refused(lib.nlg_op_conv_scalar(gm.h, base.h, 2, arr(gins[0], gins[1]), arr(out, bare_out), 0), "no scalar")
    # the velocity term needs no scalar, and both entries still work
    gm.conv_lanes(bare_in, [bare_in], [bare_out])
    assert not np.any(bare_out.get_field(0) == SENTINEL) and np.all(bare_out.get_field(host.PR) == SENTINEL)
    gm.conv_scalar(base, [gins[0]], [out])
    assert not np.any(out.get_field(host.THETA) == SENTINEL)


def test_no_device_memory_is_kept(gpu_ctx):
    """Free device memory as hipMemGetInfo reports it, before and after 50 calls of each entry (after one call that lets the mesh
    allocate its scratch fields).  The figure is the card's and moves in the 2 MiB chunks the runtime takes memory in: of two runs
    when this was written, one gave equal figures and one a single chunk.  Asserted: less than a quarter of what keeping only the
    SMALLEST of a call's three buffers on every call would take (16.6 MB here; all three: 435 MB).  Both figures are printed."""
    i = cr.IDS.index("2x1x2_n12")
    gm, base, gins = dev_case(gpu_ctx, i)
    lib = gm.lib
    lib.hipMemGetInfo.restype = C.c_int
    lib.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert lib.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    outs = [fresh(gm) for _ in range(4)]
    gm.conv_lanes(base, gins, outs)
    gm.conv_scalar(base, gins, outs)
    before = free_bytes()
    for _ in range(50):
        gm.conv_lanes(base, gins, outs, 1)
        gm.conv_scalar(base, gins, outs, 0)
    after = free_bytes()
    smallest = 8 * 4 * 3 * gm.lvn   # the lane buffer of nlg_op_conv_lanes: [4 lanes][3 components][lvn]
    print("free device memory: %d before, %d after 100 calls (smallest buffer of a call: %d bytes)" % (before, after, smallest))
    assert before - after < 100 * smallest // 4
