"""Host-side mirror of the reference's operator / plugin interface for the hot path, on top of the
C ABI (include/neklab_gpu.h).  Names, argument meaning and error behaviour follow the reference:

* `nek_dvector`   <- type nek_dvector           /root/reference/src/vectors/neklab_vectors.f90:26-50
* `exptA_linop`   <- type exptA_linop           /root/reference/src/linops/neklab_linops.f90:35-44
* `linear_stability_analysis_fixed_point` <-    /root/reference/src/neklab_analysis.f90:38-105
* `nek2vec` / `vec2nek` field movers       <-    /root/reference/src/neklab_utils.f90:84-134

In the reference these are Fortran 2008 types driven by LightKrylov; the Fortran shim with the same
bindings is neklab_amd/fortran/neklab_gpu.f90.  This Python mirror exists so that parity tests can be
written the way the reference's own driver reads.  All arithmetic happens in HIP kernels; nothing here
computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib
from ._lib import NlgError, check, dptr, vp

VX, VY, VZ, PR, THETA = 0, 1, 2, 3, 4


class Context:
    """Device + stream (+ RCCL communicator).  One per process / GPU."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = vp()
        check(self.lib.nlg_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.rank, self.nranks = 0, 1

    def comm_init(self, rank: int, nranks: int, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        check(self.lib.nlg_ctx_comm_init(self.h, rank, nranks, C.cast(buf, vp)))
        self.rank, self.nranks = rank, nranks

    def comm_init_shm(self, rank: int, nranks: int, name: str, slot_bytes: int = 64 << 20):
        """Validation transport (several test ranks on one GPU), see include/neklab_gpu.h."""
        check(self.lib.nlg_ctx_comm_init_shm(self.h, rank, nranks, name.encode(), slot_bytes))
        self.rank, self.nranks = rank, nranks

    @staticmethod
    def unique_id() -> bytes:
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        check(lib.nlg_comm_unique_id(C.cast(buf, vp)))
        return buf.raw

    def sync(self):
        check(self.lib.nlg_ctx_sync(self.h))

    def close(self):
        if self.h:
            self.lib.nlg_ctx_destroy(self.h)
            self.h = None


class Mesh:
    """The Nek5000 state the reference reads from SIZE/TOTAL commons, uploaded once."""

    def __init__(self, ctx: Context, mesh, lxd: int = 0):
        self.ctx, self.lib = ctx, ctx.lib
        self.host = mesh
        d = _lib.MeshDesc()
        d.dim, d.n, d.lxd, d.nelv = mesh.dim, mesh.n, int(lxd), mesh.E
        keep = []

        def f64(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return dptr(a)

        d.xm1, d.ym1 = f64(mesh.x), f64(mesh.y)
        d.zm1 = f64(mesh.z) if mesh.dim == 3 else None
        g = np.ascontiguousarray(mesh.glo_num, dtype=np.int64)
        keep.append(g)
        d.glo_num = g.ctypes.data_as(_lib.c_int64_p)
        if mesh.elem_gid is not None:
            eg = np.ascontiguousarray(mesh.elem_gid, dtype=np.int64)
            keep.append(eg)
            d.lglel = eg.ctypes.data_as(_lib.c_int64_p)
        d.v1mask, d.v2mask = f64(mesh.mask[0]), f64(mesh.mask[1])
        d.v3mask = f64(mesh.mask[2]) if mesh.dim == 3 else None
        d.tmask = f64(mesh.tmask)
        d.has_outflow = int(mesh.has_outflow)
        h = vp()
        check(self.lib.nlg_mesh_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        lvn, lpn = C.c_int64(), C.c_int64()
        check(self.lib.nlg_mesh_sizes(h, C.byref(lvn), C.byref(lpn), None, None))
        self.lvn, self.lpn = lvn.value, lpn.value
        self.dim, self.n = mesh.dim, mesh.n
        self.E = mesh.E

    def get(self, name: str, on_mesh: int = 1) -> np.ndarray:
        npts = {1: self.lvn, 2: self.lpn}.get(on_mesh, on_mesh)
        out = np.empty(npts)
        check(self.lib.nlg_mesh_get(self.h, name.encode(), dptr(out), npts))
        return out

    def pop_mfma(self) -> int:
        """1 if single-vector launches of the pressure operator on this mesh take the matrix-pipe kernels (NLG_POP_MFMA=0 -> 0)."""
        out = C.c_int()
        check(self.lib.nlg_mesh_pop_mfma(self.h, C.byref(out)))
        return out.value

    # ---- one application of a PCG loop's operator in the solver-only form (include/neklab_gpu.h: nlg_op_helmholtz_pcg, nlg_op_cdabdtp_pcg)
    def helmholtz_pcg(self, u, h1, h2, zf=None, beta=None, done=None, pcinv=None, xp=0, zfree=0, ring=0, fused=0, sentinel=-7.25):
        """u, zf: [nl][nf][lvn]; beta, done: [nl]; pcinv: [lvn].  Returns dict(u_out, u_src, w: [nl][nf][lvn], part: [nl][cap], npart)."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        nl, nf = u.shape[:2]
        assert u.shape[2:] == (self.lvn,)
        f = lambda a, shape: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))
        zf, beta, pcinv = f(zf, u.shape), f(beta, (nl,)), f(pcinv, (self.lvn,))
        done = f(np.zeros(nl) if done is None else done, (nl,))
        cap = self.E * nf
        out = dict(u_out=np.empty_like(u), u_src=np.empty_like(u), w=np.empty_like(u), part=np.empty((nl, cap)))
        npart = C.c_int()
        p = lambda a: None if a is None else dptr(a)
        check(self.lib.nlg_op_helmholtz_pcg(self.h, nf, nl, float(h1), float(h2), p(u), p(zf), p(beta), p(done), p(pcinv), int(xp), int(zfree),
                                            int(ring), int(fused), float(sentinel), p(out["u_out"]), p(out["u_src"]), p(out["w"]), p(out["part"]),
                                            cap, C.byref(npart)))
        out["npart"] = npart.value
        return out

    def cdabdtp_pcg(self, p, z=None, beta=None, zmean=None, done=None, fused=0, ring=0, sentinel=-7.25):
        """p, z: [nl][lpn]; beta, zmean, done: [nl].  Returns dict(p_out, p_src, out: [nl][lpn], part: [nl][cap], npart)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        nl = p.shape[0]
        assert p.shape[1:] == (self.lpn,)
        f = lambda a, shape: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))
        z, beta, zmean = f(z, p.shape), f(beta, (nl,)), f(zmean, (nl,))
        done = f(np.zeros(nl) if done is None else done, (nl,))
        cap = 2 * self.E
        out = dict(p_out=np.empty_like(p), p_src=np.empty_like(p), out=np.empty_like(p), part=np.empty((nl, cap)))
        npart = C.c_int()
        q = lambda a: None if a is None else dptr(a)
        check(self.lib.nlg_op_cdabdtp_pcg(self.h, nl, q(p), q(z), q(beta), q(zmean), q(done), int(fused), int(ring), float(sentinel),
                                          q(out["p_out"]), q(out["p_src"]), q(out["out"]), q(out["part"]), cap, C.byref(npart)))
        out["npart"] = npart.value
        return out

    def gs(self, u, layout=0, done=None, sentinel=-7.25, out=None):
        """The gather-scatter as the solvers call it (nlg_op_gs).  u: [nl][nf][lvn]; layout 0 natural, 1 face-grouped, 2 slab-permuted;
        done: [nl] or None (no gate); out: the array to write (left untouched by a refused call)."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        nl, nf = u.shape[:2]
        assert u.shape[2:] == (self.lvn,)
        out = np.empty_like(u) if out is None else out
        assert out.shape == u.shape and out.dtype == np.float64 and out.flags.c_contiguous
        done = None if done is None else np.ascontiguousarray(np.broadcast_to(np.asarray(done, dtype=np.float64), (nl,)))
        check(self.lib.nlg_op_gs(self.h, nf, nl, int(layout), dptr(u), None if done is None else dptr(done), float(sentinel), dptr(out)))
        return out

    # ---- the convective terms as the time stepper launches them: len(vec_in) lanes, one operator call (nlg_op_conv_lanes, nlg_op_conv_scalar)
    def conv_lanes(self, base, vec_in, vec_out, adjoint=False):
        s = len(vec_in)
        assert len(vec_out) == s
        check(self.lib.nlg_op_conv_lanes(self.h, base.h, s, (vp * s)(*[x.h for x in vec_in]), (vp * s)(*[x.h for x in vec_out]), int(bool(adjoint))))

    def conv_scalar(self, base, vec_in, vec_out, adjoint=False):
        s = len(vec_in)
        assert len(vec_out) == s
        check(self.lib.nlg_op_conv_scalar(self.h, base.h, s, (vp * s)(*[x.h for x in vec_in]), (vp * s)(*[x.h for x in vec_out]), int(bool(adjoint))))

    def close(self):
        if self.h:
            self.lib.nlg_mesh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class nek_dvector:
    """reference: type nek_dvector (neklab_vectors.f90:26-50).  Fields live in HBM."""

    def __init__(self, mesh: Mesh, nscal: int = 0, lorder: int = 3, _handle=None, _owns=True):
        self.mesh, self.lib = mesh, mesh.lib
        self.nscal, self.lorder = nscal, lorder
        self._owns = _owns
        if _handle is None:
            h = vp()
            check(self.lib.nlg_vec_create(mesh.h, nscal, lorder, C.byref(h)))
            self.h = h
        else:
            self.h = _handle

    # ---- the six deferred procedures of abstract_vector_rdp (neklab_vectors.f90:39-44)
    def zero(self):
        check(self.lib.nlg_vec_zero(self.h))

    def rand(self, ifnorm: bool = False, seed: int = 0):
        check(self.lib.nlg_vec_rand(self.h, int(bool(ifnorm)), int(seed)))

    def scal(self, alpha: float):
        check(self.lib.nlg_vec_scal(self.h, float(alpha)))

    def axpby(self, alpha: float, vec: "nek_dvector", beta: float):
        """self = alpha*vec + beta*self  (argument order of nek_daxpby with pass(self))."""
        if not isinstance(vec, nek_dvector):
            raise TypeError("type_error: vec must be nek_dvector (reference: real_vectors.f90:202-204)")
        check(self.lib.nlg_vec_axpby(float(alpha), vec.h, float(beta), self.h))

    def dot(self, vec: "nek_dvector") -> float:
        if not isinstance(vec, nek_dvector):
            raise TypeError("type_error: vec must be nek_dvector (reference: real_vectors.f90:229-231)")
        out = C.c_double()
        check(self.lib.nlg_vec_dot(self.h, vec.h, C.byref(out)))
        return out.value

    def get_size(self) -> int:
        out = C.c_int64()
        check(self.lib.nlg_vec_size(self.h, C.byref(out)))
        return out.value

    # ---- inherited helpers LightKrylov provides on top of the deferred set
    def norm(self) -> float:
        out = C.c_double()
        check(self.lib.nlg_vec_norm(self.h, C.byref(out)))
        return out.value

    def sub(self, vec):
        self.axpby(-1.0, vec, 1.0)

    def add(self, vec):
        self.axpby(1.0, vec, 1.0)

    # ---- neklab-specific restart history (neklab_vectors.f90:46-49)
    def save_rst(self, vec_rst: "nek_dvector", irst: int):
        check(self.lib.nlg_vec_save_rst(self.h, vec_rst.h, int(irst)))

    def get_rst(self, vec_rst: "nek_dvector", irst: int):
        check(self.lib.nlg_vec_get_rst(self.h, vec_rst.h, int(irst)))

    def has_rst_fields(self) -> bool:
        out = C.c_int()
        check(self.lib.nlg_vec_has_rst_fields(self.h, C.byref(out)))
        return bool(out.value)

    def clear_rst_fields(self):
        check(self.lib.nlg_vec_clear_rst_fields(self.h))

    @property
    def nrst(self) -> int:
        out = C.c_int()
        check(self.lib.nlg_vec_nrst(self.h, C.byref(out)))
        return out.value

    # ---- Fortran assignment semantics / host transfer
    def copy(self) -> "nek_dvector":
        h = vp()
        check(self.lib.nlg_vec_clone(self.h, C.byref(h)))
        return nek_dvector(self.mesh, self.nscal, self.lorder, _handle=h)

    def assign(self, other: "nek_dvector"):
        check(self.lib.nlg_vec_copy(self.h, other.h))

    def set_field(self, field: int, data, irst: int = 0):
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        check(self.lib.nlg_vec_set_field(self.h, int(field), int(irst), dptr(a), a.size))

    def get_field(self, field: int, irst: int = 0) -> np.ndarray:
        n = self.mesh.lpn if field == PR else self.mesh.lvn
        out = np.empty(n)
        check(self.lib.nlg_vec_get_field(self.h, int(field), int(irst), dptr(out), n))
        return out

    def close(self):
        if self.h and self._owns:
            self.lib.nlg_vec_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nek2vec(vec: nek_dvector, vx, vy, vz=None, pr=None, t=None):
    """reference: neklab_utils.f90:84-108 (nopcopy :279-301): host fields -> vector."""
    vec.set_field(VX, vx)
    vec.set_field(VY, vy)
    if vec.mesh.dim == 3 and vz is not None:
        vec.set_field(VZ, vz)
    if pr is not None:
        vec.set_field(PR, pr)
    if t is not None:
        for m, tm in enumerate(t[: vec.nscal]):
            vec.set_field(THETA + m, tm)


def vec2nek(vec: nek_dvector):
    """reference: neklab_utils.f90:110-134: vector -> host fields (vx, vy, vz|None, pr, [theta])."""
    vz = vec.get_field(VZ) if vec.mesh.dim == 3 else None
    return (vec.get_field(VX), vec.get_field(VY), vz, vec.get_field(PR),
            [vec.get_field(THETA + m) for m in range(vec.nscal)])


class KrylovBasis:
    """Contiguous array of nek_dvector (what LightKrylov allocates as X(kdim+1)) with block kernels."""

    def __init__(self, mesh: Mesh, nvec: int, nscal: int = 0, lorder: int = 3):
        self.mesh, self.lib, self.nvec = mesh, mesh.lib, nvec
        h = vp()
        check(self.lib.nlg_basis_create(mesh.h, nscal, lorder, nvec, C.byref(h)))
        self.h = h
        self.nscal, self.lorder = nscal, lorder

    def __getitem__(self, i: int) -> nek_dvector:
        h = vp()
        check(self.lib.nlg_basis_vec(self.h, int(i), C.byref(h)))
        return nek_dvector(self.mesh, self.nscal, self.lorder, _handle=h, _owns=False)

    def block_dot(self, k: int, w: nek_dvector) -> np.ndarray:
        out = np.empty(k)
        check(self.lib.nlg_basis_block_dot(self.h, k, w.h, dptr(out)))
        return out

    def block_axpy(self, k: int, h, w: nek_dvector):
        a = np.ascontiguousarray(h, dtype=np.float64)
        check(self.lib.nlg_basis_block_axpy(self.h, k, dptr(a), w.h))

    def cgs2(self, k: int, w: nek_dvector):
        h = np.empty(max(k, 1))
        beta = C.c_double()
        check(self.lib.nlg_basis_cgs2(self.h, k, w.h, dptr(h), C.byref(beta)))
        return h[:k], beta.value

    @staticmethod
    def cgs2_batch(bases: list, k: int, ws: list):
        """ws[l] against columns 0 .. k-1 of bases[l], all lanes in one launch per stage (nlg_basis_cgs2_batch); returns
        (h of shape (len(bases), k), beta of shape (len(bases),))."""
        s = len(bases)
        assert len(ws) == s and s >= 1
        ldh = max(int(k), 1)
        h, beta = np.zeros((s, ldh)), np.zeros(s)
        ab = (vp * s)(*[b.h for b in bases])
        aw = (vp * s)(*[w.h for w in ws])
        check(bases[0].lib.nlg_basis_cgs2_batch(s, ab, int(k), aw, dptr(h), ldh, dptr(beta)))
        return h[:, :k], beta

    def block_cgs2(self, k: int, s: int) -> np.ndarray:
        """Columns k .. k+s-1 orthogonalised against 0 .. k-1 and among themselves (nlg_basis_block_cgs2); returns the
        (k+s, s) coefficient matrix: projection coefficients on top, the upper-triangular R below."""
        coef = np.zeros((k + s, s), order="F")
        check(self.lib.nlg_basis_block_cgs2(self.h, int(k), int(s), dptr(coef)))
        return coef

    def last_block_rank(self) -> int:
        """columns the last block_cgs2 kept (< s: numerically dependent columns were deflated to zero vectors)"""
        r = C.c_int()
        check(self.lib.nlg_basis_last_block_rank(self.h, C.byref(r)))
        return r.value

    def combine(self, k: int, c, out: nek_dvector):
        a = np.ascontiguousarray(c, dtype=np.float64)
        check(self.lib.nlg_basis_combine(self.h, k, dptr(a), out.h))

    def close(self):
        if self.h:
            self.lib.nlg_basis_destroy(self.h)
            self.h = None


def filter_modes_from_cutoff_ratio(lx1: int, ratio: float) -> int:
    """`filter_modes` (the number of attenuated modes of the explicit filter) from Nek5000's `filterCutoffRatio`, by the rule of its
    .par reader: max(nint(lx1 (1 - ratio)) - 1, 0) + 1 with nint rounding half away from zero.  At the reference's 0.84
    (examples/back_fstep/transient_growth/bfs.par:17-19): lx1 = 6, 8 -> 1; 10, 12 -> 2."""
    x = lx1 * (1.0 - ratio)
    nint = int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)
    return max(nint - 1, 0) + 1


class exptA_linop:
    """reference: type exptA_linop (neklab_linops.f90:35-44); constructor idiom `exptA_linop(tau, bf)`
    (examples/cylinder/stability/direct/1cyl.usr:20)."""

    def __init__(self, tau: float, baseflow: nek_dvector, **cfg):
        self.mesh, self.lib = baseflow.mesh, baseflow.lib
        c = _lib.ExptAConfig()
        check(self.lib.nlg_exptA_config_default(C.byref(c)))
        c.tau = float(tau)
        for k, v in cfg.items():
            if not hasattr(c, k):
                raise TypeError("unknown exptA option %r" % k)
            if k == "buoy":
                v = (C.c_double * 3)(*[float(a) for a in tuple(v) + (0.0,) * (3 - len(tuple(v)))])
            setattr(c, k, v)
        self.cfg = c
        self.baseflow = baseflow
        h = vp()
        check(self.lib.nlg_linop_create(self.mesh.h, C.byref(c), baseflow.h, C.byref(h)))
        self.h = h

    @property
    def tau(self) -> float:
        return self.info()["tau"]

    @tau.setter
    def tau(self, v: float):
        check(self.lib.nlg_linop_set_tau(self.h, float(v)))

    def init(self):
        check(self.lib.nlg_linop_init(self.h))

    def matvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        if not isinstance(vec_in, nek_dvector) or not isinstance(vec_out, nek_dvector):
            raise TypeError("type_error: nek_dvector expected (reference: exponential_propagator.f90:53-58)")
        check(self.lib.nlg_linop_matvec(self.h, vec_in.h, vec_out.h))

    def rmatvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        if not isinstance(vec_in, nek_dvector) or not isinstance(vec_out, nek_dvector):
            raise TypeError("type_error: nek_dvector expected (reference: exponential_propagator.f90:100-105)")
        check(self.lib.nlg_linop_rmatvec(self.h, vec_in.h, vec_out.h))

    def matvec_block(self, vecs_in: list, vecs_out: list, transpose: bool = False):
        """len(vecs_in) <= 4 vectors advanced together (nlg_linop_matvec_block)."""
        s = len(vecs_in)
        assert len(vecs_out) == s
        ai = (vp * s)(*[x.h for x in vecs_in])
        ao = (vp * s)(*[x.h for x in vecs_out])
        check(self.lib.nlg_linop_matvec_block(self.h, s, ai, ao, int(bool(transpose))))

    def info(self) -> dict:
        tau, dt, cfl, ns = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(self.lib.nlg_linop_get_info(self.h, C.byref(tau), C.byref(dt), C.byref(ns), C.byref(cfl)))
        zf = C.c_int()
        check(self.lib.nlg_linop_pcg_z_free(self.h, C.byref(zf)))   # 1: the velocity PCG does not store z (NLG_PCG_STORE_Z=1 -> 0)
        return {"tau": tau.value, "dt": dt.value, "nsteps": ns.value, "cfl": cfl.value, "pcg_z_free": zf.value}

    def stats(self) -> dict:
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.nlg_linop_get_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"steps": a.value, "v_iters": b.value, "p_iters": c.value, "matvecs": d.value}

    def lane_iters(self, lane: int, istep: int = 0) -> dict:
        """Iterations of one lane in the last run (a matvec or block, a forced integration, a nonlinear map), of time step
        `istep` (1-based) or summed (0); in orbit mode the base flow is the lane after the last perturbation."""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.nlg_linop_lane_iters(self.h, int(lane), int(istep), C.byref(a), C.byref(b)))
        return {"v_iters": a.value, "p_iters": b.value}

    def close(self):
        if self.h:
            self.lib.nlg_linop_destroy(self.h)
            self.h = None


class exptA_orbit_linop(exptA_linop):
    """Propagator over one period about a time-periodic base flow: the monodromy operator of the orbit through `X0`, whose
    eigenvalues are the Floquet multipliers (the time stepper under the reference's periodic-orbit Jacobian,
    src/systems/periodic_orbit.f90:59-92).  A matvec advances the base flow (nonlinear step, from X0) and 1 to 3 perturbations
    (step linearised about the base flow's current state) in the same time steps and the same kernel launches
    (nlg_linop_set_orbit).  cfl_limit defaults to 0.4, as in the reference's call.  No adjoint: rmatvec raises."""

    def __init__(self, period: float, X0: nek_dvector, **cfg):
        cfg.setdefault("cfl_limit", 0.4)
        super().__init__(period, X0, **cfg)
        self.period, self.X0 = float(period), X0
        check(self.lib.nlg_linop_set_orbit(self.h, X0.h, self.period))     # (includes init)

    def orbit_end(self, out: nek_dvector | None = None) -> nek_dvector:
        """Phi_T(X0): the base flow after the time steps of the last matvec."""
        out = out if out is not None else nek_dvector(self.mesh, 0, self.X0.lorder)
        check(self.lib.nlg_linop_orbit_end(self.h, out.h))
        return out

    def closure(self) -> float:
        """|Phi_T(X0) - X0| / |X0| in the norm of the vector space, from the last matvec."""
        d = self.orbit_end()
        d.axpby(-1.0, self.X0, 1.0)
        return d.norm() / self.X0.norm()


# ------------------------------------------------------------------------------------------------------------------
# Resolvent operator by time stepping.  Reference: resolvent_linop (src/linops/neklab_linops.f90:198-205,
# src/linops/resolvent.f90) acting on nek_zvector = (re, im) pairs of nek_dvector (src/vectors/neklab_vectors.f90).
class nek_zvector:
    """Complex state as a pair of real vectors (the reference's nek_zvector holds `re` and `im` of type nek_dvector)."""

    def __init__(self, mesh: "Mesh"):
        self.mesh = mesh
        self.re, self.im = nek_dvector(mesh), nek_dvector(mesh)

    def zero(self):
        self.re.zero()
        self.im.zero()

    def axpby(self, alpha: complex, vec: "nek_zvector", beta: complex):
        """self = alpha * vec + beta * self with complex scalars."""
        a, b = complex(alpha), complex(beta)
        re, im = self.re.copy(), self.im.copy()
        self.re.scal(b.real)
        self.re.axpby(-b.imag, im, 1.0)
        self.re.axpby(a.real, vec.re, 1.0)
        self.re.axpby(-a.imag, vec.im, 1.0)
        self.im.scal(b.real)
        self.im.axpby(b.imag, re, 1.0)
        self.im.axpby(a.real, vec.im, 1.0)
        self.im.axpby(a.imag, vec.re, 1.0)

    def dot(self, vec: "nek_zvector") -> complex:
        """<self, vec> = sum conj(self) vec in the mass-weighted velocity inner product."""
        return complex(self.re.dot(vec.re) + self.im.dot(vec.im), self.re.dot(vec.im) - self.im.dot(vec.re))

    def norm(self) -> float:
        return float(np.sqrt(self.re.dot(self.re) + self.im.dot(self.im)))

    def rand(self, seed: int = 0):
        """Admissible random real and imaginary parts (nek_dvector.rand), from the two seeds 2 seed + 1 and 2 seed + 2."""
        self.re.rand(False, 2 * int(seed) + 1)
        self.im.rand(False, 2 * int(seed) + 2)

    def scal(self, alpha: complex):
        a = complex(alpha)
        if a.imag == 0.0:
            self.re.scal(a.real)
            self.im.scal(a.real)
        else:
            self.axpby(0.0, self, a)

    def copy(self) -> "nek_zvector":
        z = nek_zvector.__new__(nek_zvector)
        z.mesh = self.mesh
        z.re, z.im = self.re.copy(), self.im.copy()
        return z

    def conj(self):
        """self = conj(self), in place."""
        self.im.scal(-1.0)


def integrate_forced(exptA: exptA_linop, ic, f_re: nek_dvector, f_im, omega: float, adjoint: bool, out: nek_dvector):
    check(exptA.lib.nlg_linop_integrate_forced(exptA.h, ic.h if ic is not None else None, f_re.h,
                                               f_im.h if f_im is not None else None, float(omega), int(bool(adjoint)), out.h))


def integrate_forced_block(exptA: exptA_linop, ics, f_res: list, f_ims, omega: float, adjoint: bool, outs: list):
    """len(f_res) <= 4 forced integrations as the lanes of one block run (nlg_linop_integrate_forced_block): lane v starts from
    ics[v] (ics None, or a None entry: rest) under Re[(f_res[v] + i f_ims[v]) exp(i s omega t)] (f_ims None, or a None entry: a
    real forcing) and is stored into outs[v]."""
    s = len(f_res)
    if len(outs) != s or (ics is not None and len(ics) != s) or (f_ims is not None and len(f_ims) != s):
        raise ValueError("integrate_forced_block: %d forcings need as many initial conditions, imaginary parts and outputs" % s)

    def arr(vs):
        return (vp * max(s, 1))(*[x.h if x is not None else None for x in vs])

    check(exptA.lib.nlg_linop_integrate_forced_block(exptA.h, s, arr(ics) if ics is not None else None, arr(f_res),
                                                     arr(f_ims) if f_ims is not None else None, float(omega), int(bool(adjoint)), arr(outs)))


class resolvent_linop:
    """R(omega) f: the time-periodic response to the forcing Re[f exp(i omega t)] about `baseflow`, by time stepping
    (resolvent_matvec, src/linops/resolvent.f90:17-44): b = one period from rest under the forcing (evaluate_rhs),
    Re x from (I - exp(T L)) x = b by GMRES(64), rtol 1e-6 (solve_resolvent_real_part, :113-131), Im part = the state a
    quarter period later (evaluate_imaginary_part).  `rmatvec` integrates the adjoint equations with exp(-i omega t).
    rtol, kdim: of that GMRES (the reference's values by default).  `matvec_block` / `rmatvec_block` apply the operator to up to four
    vectors as the lanes of one run (block GMRES), `apply_linear_block` is the linear pair (R, R^H) that `resolvent_analysis` uses."""

    def __init__(self, omega: float, baseflow: nek_dvector, rtol: float = 1.0e-6, kdim: int = 64, **cfg):
        self.omega, self.baseflow, self.cfg = float(omega), baseflow, dict(cfg)
        self.rtol, self.kdim = float(rtol), int(kdim)      # of the GMRES for the real part (the reference's: 1e-6, 64)
        self.mesh = baseflow.mesh
        self.gmres_matvecs = 0

    def _apply(self, vin: nek_zvector, vout: nek_zvector, adjoint: bool):
        tau = 1.0 if self.omega == 0.0 else 2.0 * np.pi / abs(self.omega)
        A = exptA_linop(tau, self.baseflow, **self.cfg)
        A.init()
        b = nek_dvector(self.mesh)
        integrate_forced(A, None, vin.re, vin.im, self.omega, adjoint, b)
        # (I - exp(T L)) x = b  <=>  (exp(T L) - I) x = -b
        rhs = b.copy()
        rhs.scal(-1.0)
        x = nek_dvector(self.mesh)
        res, nmv = gmres(A, rhs, x, atol=max(self.rtol * b.norm(), 1.0e-12), kdim=self.kdim, transpose=adjoint)
        self.gmres_matvecs += nmv
        x.clear_rst_fields()
        vout.re.assign(x)
        A.tau = tau / 4.0                      # exptA%tau = tau/4; call exptA%init(), resolvent.f90:35
        integrate_forced(A, x, vin.re, vin.im, self.omega, adjoint, vout.im)
        self.last_operator = A
        return res

    def matvec(self, vin: nek_zvector, vout: nek_zvector):
        return self._apply(vin, vout, False)

    def rmatvec(self, vin: nek_zvector, vout: nek_zvector):
        return self._apply(vin, vout, True)

    def _apply_block(self, vins: list, vouts: list, adjoint: bool):
        """`_apply` for s = len(vins) <= 4 forcings as the lanes of ONE operator: a forced block period from rest, block GMRES on
        (exp(T L) - I) X = -B, a forced block quarter period from the X_v.  All lanes share omega, dt and the step count."""
        s = len(vins)
        if len(vouts) != s:
            raise ValueError("resolvent block: %d inputs, %d outputs" % (s, len(vouts)))
        tau = 1.0 if self.omega == 0.0 else 2.0 * np.pi / abs(self.omega)
        A = exptA_linop(tau, self.baseflow, **self.cfg)
        A.init()
        f_re, f_im = [v.re for v in vins], [v.im for v in vins]
        bs = [nek_dvector(self.mesh) for _ in range(s)]
        integrate_forced_block(A, None, f_re, f_im, self.omega, adjoint, bs)
        atols = [max(self.rtol * b.norm(), 1.0e-12) for b in bs]
        for b in bs:
            b.scal(-1.0)
        xs = [nek_dvector(self.mesh) for _ in range(s)]
        res, nmv = gmres_block(A, bs, xs, atols, kdim=self.kdim, transpose=adjoint)
        self.gmres_matvecs += nmv
        for v in range(s):
            xs[v].clear_rst_fields()
            vouts[v].re.assign(xs[v])
        A.tau = tau / 4.0
        integrate_forced_block(A, xs, f_re, f_im, self.omega, adjoint, [o.im for o in vouts])
        self.last_operator = A
        return res

    def matvec_block(self, vins: list, vouts: list):
        return self._apply_block(vins, vouts, False)

    def rmatvec_block(self, vins: list, vouts: list):
        return self._apply_block(vins, vouts, True)

    def apply_linear_block(self, vs: list, outs: list, adjoint: bool = False):
        """The LINEAR pair the analyses are built on: outs[v] = R vs[v] (adjoint: R^H vs[v]).  `matvec` returns conj(R f): the
        response to Re[f exp(i omega t)] is Re[x exp(i omega t)] with x = R f, and its state a quarter period later is
        Re[i x] = -Im x, which resolvent_matvec stores as the imaginary part; that map is antilinear in f, so the direct result
        is conjugated here.  The adjoint run uses exp(-i omega t), its quarter-period state is +Im y: `rmatvec` is R^H itself."""
        if adjoint:
            return self.rmatvec_block(vs, outs)
        res = self.matvec_block(vs, outs)
        for o in outs:
            o.conj()
        return res


def _zorth(Ys: list) -> np.ndarray:
    """Modified Gram-Schmidt, applied twice, on a list of complex vectors in place, in the inner product of their `dot`
    (<a, b> = sum conj(a) b).  Returns the upper-triangular T with Y_in = Y_out T."""
    k = len(Ys)
    T = np.eye(k, dtype=complex)
    for _ in range(2):
        S = np.zeros((k, k), dtype=complex)
        for j in range(k):
            for i in range(j):
                c = Ys[i].dot(Ys[j])
                Ys[j].axpby(-c, Ys[i], 1.0)
                S[i, j] = c
            nrm = Ys[j].norm()
            S[j, j] = nrm
            if nrm > 0.0:
                Ys[j].scal(1.0 / nrm)
        T = S @ T
    return T


def resolvent_analysis(R, nsv: int, power_iters: int = 1, seed: int = 1, Omega: "list | None" = None):
    """The nsv <= 4 leading singular triplets of the resolvent R by a randomised SVD whose k = nsv samples are the lanes of block
    applications (the reference's case file asks for `nsv = 4` next to resolvent_linop, examples/back_fstep/gramian/bfs.usr:8):
    Y = R Omega; power_iters times Q = orth(Y), Z = R^H Q, Q' = orth(Z), Y = R Q'; then Q = orth(Y), Z = R^H Q = V^ T
    (Gram-Schmidt), T^H = W Sigma P^H, U = Q W, V = V^ P: 2 power_iters + 2 block applications.  Returns (sigma descending,
    U: the responses, V: the forcings), R v_j ~ sigma_j u_j and R^H u_j = sigma_j v_j.

    R is touched through R.apply_linear_block(vs, outs, adjoint) only and the vectors through nek_zvector's methods (copy, dot,
    norm, axpby, scal), so anything that offers those can stand in.  Omega: the k test forcings (default: nek_zvector.rand of
    seed, seed + 1, ...); they are not modified."""
    k = int(nsv)
    if not 1 <= k <= 4:
        raise ValueError("resolvent_analysis: nsv = %d unsupported (1..4: the singular vectors are the lanes of one block run)" % k)
    if Omega is None:
        Omega = []
        for i in range(k):
            z = nek_zvector(R.mesh)
            z.rand(seed + i)
            Omega.append(z)
    if len(Omega) != k:
        raise ValueError("resolvent_analysis: %d test forcings for nsv = %d" % (len(Omega), k))
    Y = [z.copy() for z in Omega]
    Z = [z.copy() for z in Omega]
    R.apply_linear_block(Omega, Y, False)
    for _ in range(int(power_iters)):
        _zorth(Y)
        R.apply_linear_block(Y, Z, True)
        _zorth(Z)
        R.apply_linear_block(Z, Y, False)
    _zorth(Y)                                  # Y = Q
    R.apply_linear_block(Y, Z, True)
    T = _zorth(Z)                              # Z = V^
    W, sigma, Ph = np.linalg.svd(T.conj().T)
    P = Ph.conj().T

    def combine(basis, C):
        out = []
        for j in range(k):
            u = basis[0].copy()
            u.scal(C[0, j])
            for i in range(1, k):
                u.axpby(C[i, j], basis[i], 1.0)
            out.append(u)
        return out

    return sigma, combine(Y, W), combine(Z, P)


def line_labels(mesh: "Mesh", idir: int, decimals: int = 9) -> np.ndarray:
    """One label per line of velocity points along direction idir (1-based): points with the same remaining coordinates
    (rounded) share it.  What Nek5000's gtpp_gs_setup derives from (nelx, nely, nelz) for extruded box meshes
    (init_exptA_proj, src/linops/exponential_propagator_proj.f90:18-22); needs a mesh that is not deformed along idir."""
    hm = mesh.host
    coords = [hm.x, hm.y] + ([hm.z] if hm.dim == 3 else [])
    others = [np.round(np.asarray(c).ravel(), decimals) for d, c in enumerate(coords) if d != idir - 1]
    key = np.stack(others, axis=1)
    _, lab = np.unique(key, axis=0, return_inverse=True)
    return np.ascontiguousarray(lab.ravel(), dtype=np.int64)


def _gll_to_gl_matrix(n: int) -> np.ndarray:
    """(n-2 x n) Lagrange interpolation from the GLL velocity points to the Gauss-Legendre pressure points."""
    from .mesh import gll_points
    z1 = gll_points(n)
    z2 = np.polynomial.legendre.leggauss(n - 2)[0]
    M = np.ones((n - 2, n))
    for k in range(n):
        for l in range(n):
            if l != k:
                M[:, k] *= (z2 - z1[l]) / (z1[k] - z1[l])
    return M


def pressure_mesh_coords(mesh: "Mesh"):
    """Coordinates of the pressure (GL) points: the isoparametric map evaluated there."""
    hm = mesh.host
    n, dim, E = hm.n, hm.dim, hm.E
    M = _gll_to_gl_matrix(n)
    out = []
    for c in [hm.x, hm.y] + ([hm.z] if dim == 3 else []):
        a = np.asarray(c).reshape((E,) + (n,) * dim)
        for ax in range(1, dim + 1):
            a = np.moveaxis(np.tensordot(M, a, axes=([1], [ax])), 0, ax)
        out.append(a.reshape(-1))
    return out


def line_labels_pressure(mesh: "Mesh", idir: int, decimals: int = 9):
    """(labels, coordinate along idir) of the pressure points, see line_labels."""
    X2 = pressure_mesh_coords(mesh)
    key = np.stack([np.round(c, decimals) for d, c in enumerate(X2) if d != idir - 1], axis=1)
    _, lab = np.unique(key, axis=0, return_inverse=True)
    return np.ascontiguousarray(lab.ravel(), dtype=np.int64), np.ascontiguousarray(X2[idir - 1], dtype=np.float64)


class exptA_proj_linop(exptA_linop):
    """reference: exptA_proj_linop(tau=, baseflow=, alpha=) (src/linops/neklab_linops.f90:130-152; constructed with
    keywords at examples/poiseuille/stability/direct_alpha_1/poiseuille.usr:24): the propagator restricted to the
    streamwise wavenumber alpha by projecting the initial condition and the final state."""

    def __init__(self, tau: float, baseflow: nek_dvector, alpha: float, idir: int = 1, project_pressure: bool = True, **cfg):
        super().__init__(tau, baseflow, **cfg)
        self.alpha, self.idir, self.project_pressure = float(alpha), int(idir), bool(project_pressure)

    def init(self):
        super().init()
        lab = line_labels(self.mesh, self.idir)
        if self.project_pressure:
            lab2, x2 = line_labels_pressure(self.mesh, self.idir)
            check(self.lib.nlg_linop_set_projection(self.h, self.alpha, self.idir, lab.ctypes.data_as(_lib.c_int64_p),
                                                    lab2.ctypes.data_as(_lib.c_int64_p), x2.ctypes.data_as(_lib.c_double_p)))
        else:
            check(self.lib.nlg_linop_set_projection(self.h, self.alpha, self.idir, lab.ctypes.data_as(_lib.c_int64_p), None, None))

    def proj(self, vec: nek_dvector):
        check(self.lib.nlg_linop_project(self.h, vec.h))


class exptA_sweep_linop(exptA_proj_linop):
    """Wavenumber sweep in lock-step: up to four wavenumbers ride the lanes of one block propagator
    (nlg_linop_set_projection_lanes).  Lane l of matvec_block runs at alphas[l]; matvec / rmatvec / proj are the block of
    one and use alphas[0]."""

    def __init__(self, tau: float, baseflow: nek_dvector, alphas, idir: int = 1, project_pressure: bool = True, **cfg):
        alphas = [float(a) for a in alphas]
        super().__init__(tau, baseflow, alphas[0] if alphas else 0.0, idir=idir, project_pressure=project_pressure, **cfg)
        self.alphas = alphas
        self._labels = None

    def init(self):
        exptA_linop.init(self)
        self.set_alphas(self.alphas)

    def set_alphas(self, alphas):
        """Replace the set of wavenumbers (the driver retires converged lanes this way)."""
        alphas = [float(a) for a in alphas]
        if self._labels is None:
            lab = line_labels(self.mesh, self.idir)
            lab2, x2 = line_labels_pressure(self.mesh, self.idir) if self.project_pressure else (None, None)
            self._labels = (lab, lab2, x2)
        lab, lab2, x2 = self._labels
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        check(self.lib.nlg_linop_set_projection_lanes(
            self.h, len(alphas), dptr(a) if len(alphas) else None, self.idir, lab.ctypes.data_as(_lib.c_int64_p),
            lab2.ctypes.data_as(_lib.c_int64_p) if lab2 is not None else None, dptr(x2) if x2 is not None else None))
        self.alphas = alphas
        self.alpha = alphas[0]

    def proj_block(self, vecs: list):
        """vecs[l] <- P_{alphas[l]} vecs[l] (nlg_linop_project_block)."""
        s = len(vecs)
        arr = (vp * s)(*[x.h for x in vecs])
        check(self.lib.nlg_linop_project_block(self.h, s, arr))


# ------------------------------------------------------------------------------------------------------------------
# Newton-Krylov fixed-point solver.  Reference: nek_system / nek_jacobian
# (src/systems/neklab_systems.f90, fixed_point.f90:4-96) driven by LightKrylov's `newton` + `gmres_rdp`
# (src/neklab_analysis.f90:158-205).  LightKrylov is absent from the reference tree, so Newton and GMRES are restated
# from the published algorithms (Saad & Schultz 1986: restarted GMRES with Givens rotations; inexact Newton with the
# reference's own tolerance schedulers) -- parity at LightKrylov's internals is unpinned, as for `eigs`.
class nek_system:
    """`eval` = nonlinear_map: F(X) = Phi_tau(X) - X (fixed_point.f90:4-38); `jacobian` = exp(tau J(X)) - I about the
    frozen state X (fixed_point.f90:40-96).  Two operator objects, as the reference switches Nek5000 between its
    nonlinear (CFL limit 0.4) and linearised (0.5) set-ups."""

    def __init__(self, tau: float, X0: nek_dvector, re: float, torder: int = 3, **cfg):
        self.mesh, self.lib, self.tau = X0.mesh, X0.lib, float(tau)
        self.nl = exptA_linop(tau, X0, re=re, torder=torder, cfl_limit=0.4, **cfg)
        self.jac = exptA_linop(tau, X0, re=re, torder=torder, cfl_limit=0.5, **cfg)
        self.nl.init()
        self.jac.init()
        self.n_eval = 0

    def set_tolerance(self, tol: float):
        """nek_constant_tol / nek_dynamic_tol set param(21) = param(22) = tol; nonlinear_map then solves to tol * 0.1
        (fixed_point.f90:16-17), the Jacobian to tol * 0.5 (:58-59)."""
        check(self.lib.nlg_linop_set_tolerances(self.nl.h, 0.1 * tol, 0.1 * tol))
        check(self.lib.nlg_linop_set_tolerances(self.jac.h, 0.5 * tol, 0.5 * tol))

    def eval(self, X: nek_dvector, out: nek_dvector):
        check(self.lib.nlg_linop_nonlinear_map(self.nl.h, X.h, out.h))
        self.n_eval += 1

    def set_jacobian_state(self, X: nek_dvector):
        check(self.lib.nlg_linop_set_baseflow(self.jac.h, X.h))


def nek_dynamic_tol(tol_old: float, target: float, rnorm: float):
    """neklab_systems.f90:273-335: tol = max(0.1 rnorm, target), snapped to the target when within a decade of it,
    capped at 1e-4; the target itself is clipped to [10 atol_dp, 1e-4]."""
    maxtol, mintol = 1.0e-4, 10.0 * 10.0 ** -12
    target = min(max(target, mintol), maxtol)
    tol = max(0.1 * rnorm, target)
    if tol < 10.0 * target:
        tol = target
    return min(tol, maxtol)


def nek_constant_tol(tol_old: float, target: float, rnorm: float):
    """neklab_systems.f90:229-261."""
    return max(target, 10.0 * 10.0 ** -12)


def _gmres(b, x, atol: float, kdim: int, maxiter: int, history, first, column, assemble, residual):
    """The restarted GMRES(kdim) loop of `gmres` and `gmres_upo`: Givens rotations, restarts, the residual history.  What differs
    between the two comes in as four functions: first(r, beta) makes r / beta column 0 of the Krylov basis; column(k) makes column
    k + 1 and returns column k of the Hessenberg matrix (k + 2 entries); assemble(k, y) returns the combination of the first k
    columns; residual(x, r) writes the true residual b - A x into r.  The arithmetic is plain sequential sums and
    sqrt(a * a + b * b), so that the Fortran shim's loop is the same operation by operation (tests/test_gpu_upo_fortran.py)."""
    x.zero()
    r = b.copy()
    nmv = 0
    res = r.norm()
    if history is not None:
        history.append(res)
    for _ in range(maxiter):
        beta = res
        if beta <= atol:
            break
        first(r, beta)
        R = np.zeros((kdim + 1, kdim))
        cs, sn = np.zeros(kdim), np.zeros(kdim)
        g = np.zeros(kdim + 1)
        g[0] = beta
        k = 0
        while k < kdim:
            h = column(k)
            nmv += 1
            for i in range(k):                                   # previous rotations
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                h[i] = t
            d = np.sqrt(h[k] * h[k] + h[k + 1] * h[k + 1])
            cs[k], sn[k] = (1.0, 0.0) if d == 0.0 else (h[k] / d, h[k + 1] / d)
            h[k], h[k + 1] = d, 0.0
            R[: k + 1, k] = h[: k + 1]
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            k += 1
            res = abs(g[k])
            if history is not None:
                history.append(res)
            if res <= atol:
                break
        y = np.zeros(k)                                          # R y = g
        for i in range(k - 1, -1, -1):
            t = g[i]
            for j in range(i + 1, k):
                t = t - R[i, j] * y[j]
            y[i] = t / R[i, i]
        x.axpby(1.0, assemble(k, y), 1.0)
        if res <= atol:
            break
        residual(x, r)                                           # true residual for the restart
        nmv += 1
        res = r.norm()
    return res, nmv


def gmres(exptA: exptA_linop, b: nek_dvector, x: nek_dvector, atol: float, kdim: int = 30, maxiter: int = 10,
          shift: float = -1.0, basis: "KrylovBasis | None" = None, replay_history: bool = False, transpose: bool = False,
          history: "list | None" = None):
    """Restarted GMRES(kdim) for (A + shift I) x = b, zero initial guess, stop at |residual| <= atol.  The Krylov space of
    A + shift I is that of A, so the Arnoldi relation comes from the device Arnoldi step of A (`nlg_arnoldi_step`:
    matvec + block CGS2) with `shift` added to the diagonal of H.  Returns (residual norm, number of matvecs).

    history (a list): receives the residual norm at the start and after every inner step (what LightKrylov logs as
    "GMRES(k) init step" / "inner step").
    replay_history = False strips the restart history from every new Krylov vector, so that each matvec starts
    impulsively like the nonlinear map whose Jacobian it stands for.  The reference's jac_exptA_matvec replays the
    history (fixed_point.f90:73); measured on a lid-driven cavity (scripts/newton_cavity_oracle.py, tau = 0.4): Newton
    needs 17 iterations with the replay (the Krylov operator is then the start-up-free continuation map, not the
    derivative of the map being solved) and 3 without.  The converged fixed point is the same."""
    mesh = b.mesh
    B = basis if basis is not None else KrylovBasis(mesh, kdim + 1, b.nscal, b.lorder)
    H = np.zeros((kdim + 2, kdim + 1), order="F")

    def first(r, beta):
        H[:] = 0.0
        B[0].assign(r)
        B[0].scal(1.0 / beta)

    def column(k):
        arnoldi_step(exptA, B, k, H, transpose)
        if not replay_history:
            B[k + 1].clear_rst_fields()
        h = H[: k + 2, k].copy()
        h[k] += shift
        return h

    def assemble(k, y):
        dx = nek_dvector(mesh, b.nscal, b.lorder)
        B.combine(k, y, dx)
        return dx

    def residual(x, r):                                          # r = b - (A + shift I) x
        Ax = nek_dvector(mesh, b.nscal, b.lorder)
        (exptA.rmatvec if transpose else exptA.matvec)(x, Ax)
        r.assign(b)
        r.axpby(-1.0, Ax, 1.0)
        r.axpby(-shift, x, 1.0)

    return _gmres(b, x, atol, kdim, maxiter, history, first, column, assemble, residual)


def _block_gmres_ls(H: np.ndarray, R0: np.ndarray, s: int, j: int, shift: float):
    """The small problem of block GMRES after j block steps of size s: min | E1 R0 - (H~ + shift I~) Y | column by column, where
    H~ = H[:(j + 1) s, :j s] is the block Hessenberg matrix of A (A Q_j = Q_{j+1} H~), I~ the identity on top of s zero rows and
    R0 (s x s) the coefficients of the residual block on the first s basis vectors.  Returns Y (j s x s) and the s residual norms,
    which are those of (A + shift I) Q_j Y - Q_0 R0 as long as the basis is orthonormal.  Least squares by SVD (numpy.linalg.lstsq,
    minimum norm): a deflated basis column -- a zero vector, a zero column of H~ and a zero row of R0 -- gets the coefficient 0 and
    needs no special case."""
    m = j * s
    Hs = np.array(H[: m + s, :m], dtype=np.float64)
    Hs[np.arange(m), np.arange(m)] += shift
    rhs = np.zeros((m + s, s))
    rhs[:s, :] = R0
    Y = np.linalg.lstsq(Hs, rhs, rcond=None)[0]
    return Y, np.linalg.norm(rhs - Hs @ Y, axis=0)


def gmres_block(exptA: exptA_linop, Bs: list, Xs: list, atols, kdim: int = 32, maxiter: int = 10, shift: float = -1.0,
                transpose: bool = False, replay_history: bool = False):
    """Restarted block GMRES for (A + shift I) X = B with s = len(Bs) <= 4 right-hand sides, zero initial guess, on the device's
    block Krylov pieces: the residual block is orthonormalised by `nlg_basis_block_cgs2`, every block step is one
    `nlg_block_arnoldi_step` (one `nlg_linop_matvec_block` of s lanes + block CGS2), `shift` goes on the diagonal of H as in
    `gmres`, and the small least-squares problem is solved on the host after every block step (`_block_gmres_ls`).  A cycle has at
    most `kdim` block steps and stops when every column's residual norm is at or below its atols[v]; a restart starts from the true
    residual block (one more matvec_block).  replay_history as in `gmres`.  Returns (residual norms per column, matvecs)."""
    s = len(Bs)
    if not (1 <= s <= 4 and len(Xs) == s and len(atols) == s):
        raise ValueError("gmres_block: 1..4 right-hand sides with as many solutions and tolerances, got %d, %d, %d" % (s, len(Xs), len(atols)))
    atols = np.asarray(atols, dtype=np.float64)
    mesh, nscal, lorder = Bs[0].mesh, Bs[0].nscal, Bs[0].lorder
    basis = KrylovBasis(mesh, (kdim + 1) * s, nscal, lorder)
    H = np.zeros(((kdim + 1) * s, kdim * s), order="F")
    for x in Xs:
        x.zero()
    Rs = [b.copy() for b in Bs]
    res = np.array([r.norm() for r in Rs])
    nmv = 0
    for _ in range(maxiter):
        if np.all(res <= atols):
            break
        for v in range(s):
            basis[v].assign(Rs[v])
        R0 = basis.block_cgs2(0, s)
        H[:] = 0.0
        j, Y = 0, None
        while j < kdim:
            block_arnoldi_step(exptA, basis, j * s, s, H, transpose)
            nmv += s
            rank = basis.last_block_rank() if s > 1 else 1
            if not replay_history:
                for v in range(s):
                    basis[(j + 1) * s + v].clear_rst_fields()
            j += 1
            Y, res = _block_gmres_ls(H, R0, s, j, shift)
            if np.all(res <= atols) or rank == 0:
                break
        for v in range(s):
            dx = nek_dvector(mesh, nscal, lorder)
            basis.combine(j * s, Y[:, v], dx)
            Xs[v].axpby(1.0, dx, 1.0)
        if np.all(res <= atols):
            break
        AX = [nek_dvector(mesh, nscal, lorder) for _ in range(s)]            # true residual block for the restart
        exptA.matvec_block(Xs, AX, transpose)
        nmv += s
        for v in range(s):
            Rs[v].assign(Bs[v])
            Rs[v].axpby(-1.0, AX[v], 1.0)
            Rs[v].axpby(-shift, Xs[v], 1.0)
        res = np.array([r.norm() for r in Rs])
    basis.close()
    return res, nmv


def _newton(sys, X, r, solve, tol: float, tol_mode: int, maxiter: int, line, log=None, offset=None, each=None):
    """The inexact Newton loop of `newton_fixed_point_iteration` and `newton_periodic_orbit` on F(X) = 0 (= offset, when given):
    the tolerance scheduler nek_constant_tol (tol_mode 1) or nek_dynamic_tol called at the top of an iteration, as LightKrylov's
    newton calls it; a residual below the target only counts when computed at the tightest level the scheduler will ever set;
    maxiter iterations at most, no bisection.  r: work vector for the residual; solve(r, atol, history) -> (dx, matvecs) is the
    GMRES on the Jacobian at X; line(it, rnorm, tol) the log line; each() runs before every evaluation.  `X` is updated in place."""
    sched = nek_constant_tol if tol_mode == 1 else nek_dynamic_tol
    final = sched(0.0, tol, 0.0)
    cur, rnorm = 0.0, 1.0
    residuals, nmv_total, converged = [], 0, False
    gmres_hist = []
    for it in range(maxiter + 1):
        new = sched(cur, tol, rnorm)
        if new != cur:
            cur = new
            sys.set_tolerance(cur)
        if each is not None:
            each()
        sys.eval(X, r)
        if offset is not None:
            r.axpby(-1.0, offset, 1.0)
        rnorm = r.norm()
        residuals.append(rnorm)
        if log is not None:
            log(line(it, rnorm, cur))
        if rnorm < tol and cur <= final:
            converged = True
            break
        if it == maxiter:
            break
        sys.set_jacobian_state(X)
        r.scal(-1.0)
        gh = []
        dx, nmv = solve(r, sched(cur, tol, rnorm), gh)
        gmres_hist.append(gh)
        nmv_total += nmv
        X.axpby(1.0, dx, 1.0)
    return {"converged": converged, "iterations": len(residuals) - 1, "residuals": residuals, "gmres_matvecs": nmv_total,
            "evals": sys.n_eval, "gmres_residuals": gmres_hist}


def newton_fixed_point_iteration(sys: nek_system, bf: nek_dvector, tol: float, tol_mode: int = 1, maxiter: int = 40,
                                 kdim: int = 30, outdir: str | None = None, session: str = "neklab", log=None,
                                 replay_history: bool = False):
    """reference: newton_fixed_point_iteration (src/neklab_analysis.f90:158-205): Newton on F(X) = Phi_tau(X) - X with
    GMRES on the Jacobian exp(tau J) - I, tolerance scheduler nek_constant_tol (tol_mode 1) or nek_dynamic_tol, 40
    iterations at most, no bisection; on convergence the fixed point is written as `nwt<session>0.f00001`.
    `bf` is updated in place.  Returns dict(converged, iterations, residuals, gmres_matvecs, evals, gmres_residuals)."""
    mesh = bf.mesh
    dx = nek_dvector(mesh, bf.nscal, bf.lorder)
    B = KrylovBasis(mesh, kdim + 1, bf.nscal, bf.lorder)     # (with the scalar of a temperature-coupled system)

    def solve(r, atol, gh):
        return dx, gmres(sys.jac, r, dx, atol=atol, kdim=kdim, basis=B, replay_history=replay_history, history=gh)[1]

    out = _newton(sys, bf, nek_dvector(mesh, bf.nscal, bf.lorder), solve, tol, tol_mode, maxiter,
                  lambda it, rnorm, cur: "newton %2d  |F(X)| = %.6e  solver tol %.3e" % (it, rnorm, cur), log)
    if out["converged"] and outdir is not None:
        outpost_dnek(bf, "nwt", session, outdir)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Periodic orbits: Newton-Krylov for the state and the period.  Reference: nek_ext_dvector (src/vectors/real_extended_vectors.f90),
# nek_upo_system / nek_upo_jacobian (src/systems/periodic_orbit.f90, neklab_systems.f90:147-223), driven by
# examples/cylinder/newton/Re180_periodic_orbit/1cyl.usr.  The Jacobian's time stepping is the coupled (orbit) matvec; the border
# (period column, phase row), the two time derivatives and the extended Arnoldi step are device work (nlg_upo_*); GMRES and Newton
# run in the host loops `_gmres` / `_newton` on extended vectors.  DESIGN.md 3.2 "Periodic-orbit Newton".
class nek_ext_dvector:
    """reference: type nek_ext_dvector: a nek_dvector (`vec`) plus the period `T`; the inner product adds T T."""

    def __init__(self, mesh: Mesh, lorder: int = 3, T: float = 0.0, _vec: "nek_dvector | None" = None):
        self.vec = _vec if _vec is not None else nek_dvector(mesh, 0, lorder)
        self.mesh, self.lib, self.lorder = mesh, mesh.lib, self.vec.lorder
        self.T = float(T)

    def zero(self):
        self.vec.zero()
        self.T = 0.0

    def rand(self, ifnorm: bool = False, seed: int = 0):
        """the field as nek_dvector.rand; T uniform in [0, 1) from the same seed (the reference draws it from the compiler's RNG)"""
        self.vec.rand(False, seed)
        self.T = float(np.random.default_rng(seed).random())
        if ifnorm:
            self.scal(1.0 / self.norm())

    def scal(self, alpha: float):
        self.vec.scal(alpha)
        self.T *= float(alpha)

    def axpby(self, alpha: float, vec: "nek_ext_dvector", beta: float):
        """self = alpha*vec + beta*self"""
        if not isinstance(vec, nek_ext_dvector):
            raise TypeError("type_error: vec must be nek_ext_dvector (reference: real_extended_vectors.f90:216-218)")
        self.vec.axpby(alpha, vec.vec, beta)
        self.T = float(beta) * self.T + float(alpha) * vec.T

    def dot(self, vec: "nek_ext_dvector") -> float:
        if not isinstance(vec, nek_ext_dvector):
            raise TypeError("type_error: vec must be nek_ext_dvector (reference: real_extended_vectors.f90:245-247)")
        return self.vec.dot(vec.vec) + self.T * vec.T

    def norm(self) -> float:
        return float(np.sqrt(self.dot(self)))

    def sub(self, vec: "nek_ext_dvector"):
        self.axpby(-1.0, vec, 1.0)

    def copy(self) -> "nek_ext_dvector":
        return nek_ext_dvector(self.mesh, self.lorder, self.T, _vec=self.vec.copy())

    def assign(self, other: "nek_ext_dvector"):
        self.vec.assign(other.vec)
        self.T = other.T


def outpost_ext_dnek(vecs, prefix: str, session: str = "neklab", outdir: str = ".", first_index: int = 1):
    """reference: outpost_ext_dnek (src/neklab_utils.f90): the field file of outpost_dnek with the period in the header's time."""
    if isinstance(vecs, nek_ext_dvector):
        vecs = [vecs]
    return outpost_dnek([v.vec for v in vecs], prefix, session, outdir, first_index=first_index, time=[v.T for v in vecs])


class nek_upo_system:
    """One operator in orbit mode for F(X, T) = Phi_T(X) - X and its bordered Jacobian
    [M - I, fT; f0^T, 0] (nek_upo_system / nek_upo_jacobian).  cfl_limit defaults to 0.4, as in both of the reference's calls
    (periodic_orbit.f90:18, :67).  The step count follows the CFL rule once per `set_jacobian_state` and is held through the GMRES of
    that iteration; fixed_nsteps > 0 pins it for good.  no_history = 1 by default: every matvec starts impulsively, like the map
    whose derivative it is (see `gmres`), and the border is then the fused device pass."""

    def __init__(self, X: nek_ext_dvector, re: float, torder: int = 3, fixed_nsteps: int = 0, **cfg):
        cfg.setdefault("cfl_limit", 0.4)
        cfg.setdefault("no_history", 1)
        self.mesh, self.lib = X.mesh, X.lib
        self.fixed_nsteps = int(fixed_nsteps)
        self.op = exptA_orbit_linop(X.T, X.vec, re=re, torder=torder, **cfg)
        self.h = self.op.h
        if self.fixed_nsteps:                      # (with the count left to the rule the constructor's set_orbit is this state already)
            self._state(X)
        self.n_eval = 0

    def _state(self, X: nek_ext_dvector):
        check(self.lib.nlg_linop_set_orbit_steps(self.h, X.vec.h, float(X.T), self.fixed_nsteps))

    def set_tolerance(self, tol: float):
        """both maps solve to 0.1 tol (periodic_orbit.f90:19-20, :68-69)"""
        check(self.lib.nlg_linop_set_tolerances(self.h, 0.1 * tol, 0.1 * tol))

    def eval(self, X: nek_ext_dvector, out: nek_ext_dvector):
        """out = (Phi_T(X) - X, 0)"""
        self._state(X)
        check(self.lib.nlg_upo_residual(self.h, out.vec.h))
        out.T = 0.0
        self.n_eval += 1

    def set_jacobian_state(self, X: nek_ext_dvector):
        self._state(X)

    def jac_matvec(self, v: nek_ext_dvector, out: nek_ext_dvector):
        t = C.c_double()
        check(self.lib.nlg_upo_jac_matvec(self.h, v.vec.h, float(v.T), out.vec.h, C.byref(t)))
        out.T = t.value

    def fdot(self, which: int, out: "nek_dvector | None" = None) -> nek_dvector:
        """f0 (which = 0) or fT (which = 1) of the last run"""
        out = out if out is not None else nek_dvector(self.mesh, 0, self.op.X0.lorder)
        check(self.lib.nlg_upo_fdot(self.h, int(which), out.h))
        return out

    def info(self) -> dict:
        return self.op.info()

    def close(self):
        self.op.close()


def upo_arnoldi_step(sys: nek_upo_system, basis: KrylovBasis, tcol: np.ndarray, k: int, H: np.ndarray):
    """nlg_upo_arnoldi_step: column k -> k + 1 of the extended basis (fields in `basis`, period components in `tcol`)."""
    assert H.flags.f_contiguous and tcol.dtype == np.float64 and tcol.flags.c_contiguous and tcol.size >= k + 2
    check(sys.lib.nlg_upo_arnoldi_step(sys.h, basis.h, dptr(tcol), int(k), dptr(H), H.shape[0]))


def gmres_upo(sys: nek_upo_system, b: nek_ext_dvector, x: nek_ext_dvector, atol: float, kdim: int = 30, maxiter: int = 10,
              history: "list | None" = None, replay_history: bool = False, basis: "KrylovBasis | None" = None):
    """The loop of `gmres` for J x = b on extended vectors, J the bordered Jacobian of `sys` (which contains -I: no shift), on the
    device's extended Arnoldi step.  replay_history = False for the reason measured in `gmres`'s docstring.  Returns (residual
    norm, number of Jacobian matvecs)."""
    mesh = b.mesh
    B = basis if basis is not None else KrylovBasis(mesh, kdim + 1, 0, b.lorder)
    H = np.zeros((kdim + 2, kdim + 1), order="F")
    tcol = np.zeros(kdim + 2)                                    # the period components of the basis

    def first(r, beta):
        H[:] = 0.0
        tcol[:] = 0.0
        B[0].assign(r.vec)
        B[0].scal(1.0 / beta)
        tcol[0] = r.T / beta

    def column(k):
        upo_arnoldi_step(sys, B, tcol, k, H)
        if not replay_history:
            B[k + 1].clear_rst_fields()
        return H[: k + 2, k].copy()

    def assemble(k, y):
        dx = nek_ext_dvector(mesh, b.lorder)
        B.combine(k, y, dx.vec)
        dx.T = 0.0
        for j in range(k):                                       # (a plain sequential sum, see _gmres)
            dx.T = dx.T + float(tcol[j] * y[j])
        return dx

    def residual(x, r):
        Jx = nek_ext_dvector(mesh, b.lorder)
        sys.jac_matvec(x, Jx)
        if not replay_history:
            Jx.vec.clear_rst_fields()
        r.assign(b)
        r.axpby(-1.0, Jx, 1.0)

    return _gmres(b, x, atol, kdim, maxiter, history, first, column, assemble, residual)


def newton_periodic_orbit(sys: nek_upo_system, X: nek_ext_dvector, tol: float, tol_mode: int = 1, maxiter: int = 40,
                          kdim: int = 30, offset: "nek_ext_dvector | None" = None, fixed_nsteps: int = 0,
                          outdir: str | None = None, session: str = "neklab", log=None):
    """The loop of `newton_fixed_point_iteration` on extended vectors: Newton on F(X, T) = Phi_T(X) - X (= offset, when given: a
    manufactured root, or the continuation from a nearly closed orbit) with GMRES on the bordered Jacobian; same schedulers, same
    convergence rule.  `X` is updated in place.  fixed_nsteps > 0 pins the step count of the orbit.  On convergence the orbit is
    written as `upo<session>0.f00001` with the period as the header's time.  The result feeds Floquet analysis as
    `exptA_orbit_linop(X.T, X.vec)`.  Returns the dictionary of newton_fixed_point_iteration plus `periods`, one per iteration."""
    mesh = X.mesh
    if fixed_nsteps:
        sys.fixed_nsteps = int(fixed_nsteps)
    dx = nek_ext_dvector(mesh, X.lorder)
    B = KrylovBasis(mesh, kdim + 1, 0, X.lorder)
    periods = []

    def each():
        if X.T <= 0.0:
            raise NlgError("newton_periodic_orbit: the period estimate became %g" % X.T)
        periods.append(X.T)

    def solve(r, atol, gh):
        return dx, gmres_upo(sys, r, dx, atol=atol, kdim=kdim, basis=B, history=gh)[1]

    out = _newton(sys, X, nek_ext_dvector(mesh, X.lorder), solve, tol, tol_mode, maxiter,
                  lambda it, rnorm, cur: "newton %2d  |F(X, T)| = %.6e  T = %.9f  solver tol %.3e" % (it, rnorm, X.T, cur),
                  log, offset, each)
    out["periods"] = periods
    if out["converged"] and outdir is not None:
        outpost_ext_dnek(X, "upo", session, outdir)
    return out


def arnoldi_step(exptA: exptA_linop, basis: KrylovBasis, k: int, H: np.ndarray, transpose: bool = False):
    """H is Fortran-ordered (kdim+1, kdim)."""
    assert H.flags.f_contiguous
    check(exptA.lib.nlg_arnoldi_step(exptA.h, basis.h, int(k), dptr(H), H.shape[0], int(bool(transpose))))


def block_arnoldi_step(exptA: exptA_linop, basis: KrylovBasis, k: int, s: int, H: np.ndarray, transpose: bool = False):
    """Columns k .. k+s-1 -> k+s .. k+2s-1; H (Fortran-ordered) receives H[0:k+2s, k:k+s]."""
    assert H.flags.f_contiguous
    check(exptA.lib.nlg_block_arnoldi_step(exptA.h, basis.h, int(k), int(s), dptr(H), H.shape[0], int(bool(transpose))))


def sweep_arnoldi_step(A: "exptA_sweep_linop", bases: list, k: int, Hs: np.ndarray, transpose: bool = False):
    """One Arnoldi step of len(bases) <= 4 separate eigenproblems in lock-step (nlg_sweep_arnoldi_step): lane l at A.alphas[l] on its
    own basis.  Hs is C-ordered (lanes, kdim, kdim+1): Hs[l].T is lane l's Hessenberg matrix in the layout of arnoldi_step."""
    s = len(bases)
    assert Hs.flags.c_contiguous and Hs.ndim == 3 and Hs.shape[0] >= s
    ab = (vp * s)(*[b.h for b in bases])
    check(A.lib.nlg_sweep_arnoldi_step(A.h, s, ab, int(k), dptr(Hs), Hs.shape[2], Hs.shape[1] * Hs.shape[2], int(bool(transpose))))


def _ritz_from_hessenberg(H: np.ndarray, k: int):
    """Ritz pairs of the leading k x k block of a (>= k+1, >= k) Hessenberg matrix, by the rule of `ritz_pairs` in csrc/krylov.hip:
    eigenpairs of H[:k, :k] (unit eigenvectors), residuals |H[k, k-1]| |y[k-1]|, sorted by decreasing modulus (stable).
    Returns (lam[k], Y[k, k] with the eigenvectors as columns, res[k])."""
    lam, Y = np.linalg.eig(np.asarray(H)[:k, :k])
    Y = Y / np.linalg.norm(Y, axis=0)
    res = abs(H[k, k - 1]) * np.abs(Y[k - 1, :])
    order = np.argsort(-np.abs(lam), kind="stable")
    return lam[order], Y[:, order], res[order]


def linear_stability_analysis_wavenumbers(tau: float, baseflow: nek_dvector, alphas, kdim: int, nev: int, tol: float = 1e-6,
                                          seed: int = 0, transpose: bool = False, outdir: str = ".", idir: int = 1,
                                          project_pressure: bool = True, **cfg):
    """Leading eigenvalues of the propagator restricted to each of the wavenumbers `alphas` (a dispersion relation), in lock-step: groups
    of at most four wavenumbers ride the lanes of one exptA_sweep_linop, each lane with its own Krylov basis and Hessenberg matrix
    (sweep_arnoldi_step).  After every step each lane's Ritz pairs are taken (_ritz_from_hessenberg); a lane is finished when nev
    residuals are below tol, or at breakdown (beta below 1e-12 of the column norm of H); finished lanes are retired (set_alphas with
    the remaining wavenumbers) and the run goes on with fewer lanes until all are finished or kdim steps are done.  Plain Arnoldi:
    there are NO Krylov-Schur restarts (as for block_size > 1 in nlg_eigs), so kdim bounds the Krylov space of every wavenumber.
    Start vector of wavenumber i: rand(True, seed=seed + i), projected.  Writes <dir|adj>_eigenspectrum_alpha<i>.npy per wavenumber.
    Returns one tuple per alpha, as linear_stability_analysis_fixed_point does: (eigvals = log(mu) / tau, residuals, eigvecs, mu,
    matvecs); a complex pair's eigenvectors are its real and imaginary parts, as nlg_eigs returns them."""
    alphas = [float(a) for a in alphas]
    mesh = baseflow.mesh
    prefix = "adj" if transpose else "dir"
    results = [None] * len(alphas)
    A = None
    for g0 in range(0, len(alphas), 4):
        group = list(range(g0, min(g0 + 4, len(alphas))))
        if A is None:
            A = exptA_sweep_linop(tau, baseflow, [alphas[i] for i in group], idir=idir, project_pressure=project_pressure, **cfg)
            A.init()
        else:
            A.set_alphas([alphas[i] for i in group])
        bases = {i: KrylovBasis(mesh, kdim + 1) for i in group}
        Hs = {i: np.zeros((kdim + 1, kdim)) for i in group}
        for i in group:
            bases[i][0].rand(True, seed=seed + i)
        A.proj_block([bases[i][0] for i in group])
        for i in group:
            nrm = bases[i][0].norm()
            bases[i][0].scal(1.0 / nrm)
        active = list(group)
        done = {}
        k = 0
        while active and k < kdim:
            s = len(active)
            Hw = np.zeros((s, kdim, kdim + 1))
            sweep_arnoldi_step(A, [bases[i] for i in active], k, Hw, transpose=transpose)
            k += 1
            finished = []
            for l, i in enumerate(active):
                Hs[i][:k + 1, k - 1] = Hw[l, k - 1, :k + 1]
                lam, Y, res = _ritz_from_hessenberg(Hs[i], k)
                breakdown = Hs[i][k, k - 1] <= 1e-12 * np.linalg.norm(Hs[i][:k + 1, k - 1])
                if breakdown or np.count_nonzero(res < tol) >= nev or k == kdim:
                    done[i] = (k, lam, Y, res)
                    finished.append(i)
            if finished:
                active = [i for i in active if i not in finished]
                if active and k < kdim:
                    A.set_alphas([alphas[i] for i in active])
        tau_ = A.info()["tau"]
        for i in group:
            kf, lam, Y, res = done[i]
            n = min(nev, kf)
            eigvecs = [nek_dvector(mesh, 0, 3) for _ in range(nev)]
            for v in eigvecs:
                v.zero()
            j = 0
            while j < n:
                bases[i].combine(kf, np.real(Y[:, j]), eigvecs[j])
                if abs(lam[j].imag) > 0.0:
                    if j + 1 < n:
                        bases[i].combine(kf, (1.0 if lam[j].imag > 0.0 else -1.0) * np.imag(Y[:, j]), eigvecs[j + 1])
                    j += 2
                else:
                    j += 1
            mu = np.zeros(nev, dtype=complex)
            residuals = np.zeros(nev)
            mu[:n], residuals[:n] = lam[:n], res[:n]
            with np.errstate(divide="ignore"):
                eigvals = np.log(mu) / tau_
            save_eigenspectrum(eigvals, residuals, os.path.join(outdir, "%s_eigenspectrum_alpha%d.npy" % (prefix, i)))
            results[i] = (eigvals, residuals, eigvecs, mu, kf)
            bases[i].close()
    if A is not None:
        A.close()
    return results


def eigs(exptA: exptA_linop, X: list, kdim: int = 0, tol: float = 0.0, x0: nek_dvector | None = None,
         transpose: bool = False, write_intermediate: bool = True, logfile: str | None = None, seed: int = 0,
         max_restarts: int = 50, block_size: int = 0, warm_start: bool = False):
    """reference call: eigs(exptA, eigvecs, eigvals, residuals, info, x0=, kdim=, transpose=,
    write_intermediate=) at neklab_analysis.f90:80-81.  Returns (eigvals complex[nev], residuals, info)."""
    lib = exptA.lib
    nev = len(X)
    o = _lib.EigsOpts()
    check(lib.nlg_eigs_opts_default(C.byref(o)))
    o.kdim, o.transpose, o.write_intermediate, o.tol, o.seed = int(kdim), int(bool(transpose)), int(bool(write_intermediate)), float(tol), int(seed)
    o.max_restarts = int(max_restarts)
    o.block_size, o.warm_start = int(block_size), int(bool(warm_start))
    if logfile is not None:
        o.logfile = logfile.encode()
    re, im, res = np.zeros(nev), np.zeros(nev), np.zeros(nev)
    info = C.c_int()
    arr = (vp * nev)(*[x.h for x in X])
    check(lib.nlg_eigs(exptA.h, arr, nev, dptr(re), dptr(im), dptr(res), C.byref(info), x0.h if x0 is not None else None,
                       C.byref(o)))
    return re + 1j * im, res, info.value


def svds(exptA: exptA_linop, U: list, V: list, kdim: int = 0, tol: float = 0.0, u0: nek_dvector | None = None,
         write_intermediate: bool = True, logfile: str | None = None, seed: int = 0):
    """reference call: svds(exptA, U, S, V, residuals, info, kdim=, write_intermediate=) at neklab_analysis.f90:136.
    Returns (S[nsv], residuals, info)."""
    lib = exptA.lib
    nsv = len(U)
    assert len(V) == nsv
    o = _lib.EigsOpts()
    check(lib.nlg_eigs_opts_default(C.byref(o)))
    o.kdim, o.write_intermediate, o.tol, o.seed = int(kdim), int(bool(write_intermediate)), float(tol), int(seed)
    if logfile is not None:
        o.logfile = logfile.encode()
    S, res = np.zeros(nsv), np.zeros(nsv)
    info = C.c_int()
    au = (vp * nsv)(*[x.h for x in U])
    av = (vp * nsv)(*[x.h for x in V])
    check(lib.nlg_svds(exptA.h, au, av, nsv, dptr(S), dptr(res), C.byref(info), u0.h if u0 is not None else None, C.byref(o)))
    return S, res, info.value


def transient_growth_analysis_fixed_point(exptA: exptA_linop, nsv: int, kdim: int, tol: float = 0.0, outdir: str = ".",
                                          seed: int = 0, outpost: bool = False, session: str = "neklab"):
    """reference: neklab_analysis.f90:107-156.  Returns (S, residuals, U (optimal responses), V (optimal
    perturbations), info) and writes singular_spectrum.dat (:139-143)."""
    mesh = exptA.mesh
    U = [nek_dvector(mesh, 0, 3) for _ in range(nsv)]
    V = [nek_dvector(mesh, 0, 3) for _ in range(nsv)]
    S, residuals, info = svds(exptA, U, V, kdim=kdim, tol=tol, write_intermediate=True,
                              logfile=os.path.join(outdir, "svds_output.txt"), seed=seed)
    with open(os.path.join(outdir, "singular_spectrum.dat"), "w") as f:
        f.write(" ".join("%.16e" % s for s in S) + "\n")
    if outpost:                                                      # :146-147
        outpost_dnek(V, "prt", session, outdir)
        outpost_dnek(U, "rsp", session, outdir)
    return S, residuals, U, V, info


def _gl_to_gll_matrix(n: int) -> np.ndarray:
    """(n x n-2) Lagrange interpolation from the Gauss-Legendre pressure points to the GLL velocity points."""
    from .mesh import gll_points
    z1 = gll_points(n)
    z2 = np.polynomial.legendre.leggauss(n - 2)[0]
    M = np.ones((n, n - 2))
    for k in range(n - 2):
        for l in range(n - 2):
            if l != k:
                M[:, k] *= (z1 - z2[l]) / (z2[k] - z2[l])
    return M


def pressure_from_mesh1(mesh: "Mesh", p1) -> np.ndarray:
    """A pressure given on the velocity mesh (what a field file holds) on the pressure mesh: tensor interpolation GLL -> GL inside
    every element, as Nek5000's restart does for a Pn-Pn-2 run (`map_pm1_to_pr`).  Returns the flat array for set_field(PR, .)."""
    n, dim, E = mesh.host.n, mesh.host.dim, mesh.host.E
    M = _gll_to_gl_matrix(n)
    p = np.asarray(p1, dtype=np.float64).reshape((E,) + (n,) * dim)
    for ax in range(1, dim + 1):
        p = np.moveaxis(np.tensordot(M, p, axes=([1], [ax])), 0, ax)
    return np.ascontiguousarray(p.reshape(-1))


def pressure_to_mesh1(vec: nek_dvector) -> np.ndarray:
    """Pressure of `vec` on the velocity mesh, as Nek5000's outpost writes it for a Pn-Pn-2 run (`mappr`: tensor
    interpolation GL -> GLL inside every element, then the direct-stiffness average across elements)."""
    mesh = vec.mesh
    n, dim, E = mesh.host.n, mesh.host.dim, mesh.host.E
    M = _gl_to_gll_matrix(n)
    p = vec.get_field(PR).reshape((E,) + (n - 2,) * dim)
    for ax in range(1, dim + 1):
        p = np.moveaxis(np.tensordot(M, p, axes=([1], [ax])), 0, ax)
    tmp = nek_dvector(mesh)
    tmp.set_field(VX, p.reshape(-1))
    check(mesh.lib.nlg_op_dssum(mesh.h, tmp.h))
    return tmp.get_field(VX) * mesh.get("vmult")


def outpost_dnek(vecs, prefix: str, session: str = "neklab", outdir: str = ".", first_index: int = 1, time: float = 0.0):
    """reference: outpost_dnek (src/neklab_utils.f90:305-333, called at neklab_analysis.f90:93,146,147): every vector
    becomes one Nek5000 field file `<prefix><session>0.f%05d` with the GLL coordinates in the first file only (Nek5000's
    default `ifxyo` behaviour), velocity and the pressure mapped to the velocity mesh.  `time`: the header's time, one value or one
    per vector.  Single-rank writer."""
    from . import nekio
    if isinstance(vecs, nek_dvector):
        vecs = [vecs]
    if len(prefix) != 3:
        raise ValueError("outpost_dnek: the prefix has three characters in Nek5000 (got %r)" % prefix)
    paths = []
    for i, v in enumerate(vecs):
        hm = v.mesh.host
        n, dim, E = hm.n, hm.dim, hm.E
        coords = None
        if i == 0:
            coords = [hm.x, hm.y] + ([hm.z] if dim == 3 else [])
            coords = [np.asarray(c).reshape(E, -1) for c in coords]
        vel = [v.get_field(c).reshape(E, -1) for c in range(dim)]
        path = os.path.join(outdir, "%s%s0.f%05d" % (prefix, session, first_index + i))
        nekio.write_fld(path, n, dim, coords=coords, vel=vel, p=pressure_to_mesh1(v).reshape(E, -1), time=time[i] if np.ndim(time) else time,
                        istep=first_index + i)
        paths.append(path)
    return paths


def save_eigenspectrum(eigvals, residuals, filename: str):
    """reference call site: neklab_analysis.f90:90 (LightKrylov save_eigenspectrum): (n,3) array
    [Re, Im, residual] in .npy format, the layout examples/*/plot_eigenvalues.py reads."""
    data = np.column_stack([np.real(eigvals), np.imag(eigvals), residuals])
    np.save(filename, data)


def linear_stability_analysis_fixed_point(exptA: exptA_linop, kdim: int, nev: int, adjoint: bool = False,
                                          X0: nek_dvector | None = None, tol: float = 0.0, outdir: str = ".",
                                          seed: int = 0, outpost: bool = False, session: str = "neklab",
                                          block_size: int = 0, warm_start: bool = False):
    """reference: neklab_analysis.f90:38-105.  Returns (eigvals continuous-time, residuals, eigvecs)."""
    mesh = exptA.mesh
    eigvecs = [nek_dvector(mesh, 0, 3) for _ in range(nev)]   # lorder = 3 as in every reference SIZE file
    for v in eigvecs:
        v.zero()                                                     # zero_basis, :77
    prefix = "adj" if adjoint else "dir"
    mu, residuals, info = eigs(exptA, eigvecs, kdim=kdim, x0=X0, transpose=adjoint, write_intermediate=True,
                               logfile=os.path.join(outdir, "eigs_output.txt"), tol=tol, seed=seed,
                               block_size=block_size, warm_start=warm_start)
    eigvals = np.log(mu.astype(complex)) / exptA.info()["tau"]       # :84
    save_eigenspectrum(eigvals, residuals, os.path.join(outdir, prefix + "_eigenspectrum.npy"))   # :90
    if outpost:
        outpost_dnek(eigvecs, prefix, session, outdir)               # :93
    return eigvals, residuals, eigvecs, mu, info


def linear_stability_analysis_periodic_orbit(op: exptA_orbit_linop, kdim: int, nev: int, X0: nek_dvector | None = None,
                                             tol: float = 0.0, outdir: str = ".", seed: int = 0, outpost: bool = False,
                                             session: str = "neklab", block_size: int = 0, max_restarts: int = 50):
    """Floquet analysis of the orbit `op` was built about: the device Krylov loop of linear_stability_analysis_fixed_point
    (nlg_eigs) on the coupled propagator.  Returns (mu, exponents, residuals, eigvecs, info): the Floquet multipliers mu, the
    Floquet exponents log(mu) / T and the residuals nlg_eigs reports.  block_size <= 3 (the base flow takes one lane)."""
    mesh = op.mesh
    eigvecs = [nek_dvector(mesh, 0, 3) for _ in range(nev)]
    for v in eigvecs:
        v.zero()
    mu, residuals, info = eigs(op, eigvecs, kdim=kdim, x0=X0, transpose=False, write_intermediate=True,
                               logfile=os.path.join(outdir, "eigs_output.txt"), tol=tol, seed=seed, block_size=block_size,
                               max_restarts=max_restarts)
    exponents = np.log(mu.astype(complex)) / op.info()["tau"]
    save_eigenspectrum(exponents, residuals, os.path.join(outdir, "floquet_eigenspectrum.npy"))
    if outpost:
        outpost_dnek(eigvecs, "flq", session, outdir)
    return mu, exponents, residuals, eigvecs, info


# ------------------------------------------------------------------------------------------------------------------
# The operator L itself, in strong form (nlg_lns_*; apply_L and its pieces, src/linops/neklab_linops.f90:24-28, :268-426)
LNS_COEF = {"apply_L": (1.0, -1.0, -1.0), "apply_Lv": (1.0, -1.0, 0.0), "compute_LNS_laplacian": (1.0, 0.0, 0.0),
            "compute_LNS_conv": (0.0, 1.0, 0.0), "compute_LNS_gradp": (0.0, 0.0, 1.0)}


class lns_linop:
    """L about `baseflow` at Reynolds number `re`: out = c_lap / re lap(u~) + c_conv conv(U, u~) / bm1 + c_p grad(P), element-local,
    neither masked nor assembled (include/neklab_gpu.h: nlg_lns_apply).  matvec / rmatvec are apply_L, direct and adjoint."""

    def __init__(self, baseflow: nek_dvector, re: float):
        self.mesh, self.lib, self.baseflow, self.re = baseflow.mesh, baseflow.lib, baseflow, float(re)
        self.h = None
        h = vp()
        check(self.lib.nlg_lns_create(self.mesh.h, baseflow.h, float(re), C.byref(h)))
        self.h = h

    def set_baseflow(self, baseflow: nek_dvector):
        check(self.lib.nlg_lns_set_baseflow(self.h, baseflow.h))
        self.baseflow = baseflow

    def set_re(self, re: float):
        check(self.lib.nlg_lns_set_re(self.h, float(re)))
        self.re = float(re)

    def apply(self, vecs, outs, trans: bool = False, coef=(1.0, -1.0, -1.0)):
        """outs[v] = L vecs[v] for up to four vectors in one launch (a single vector may be given as such)."""
        vecs = [vecs] if isinstance(vecs, nek_dvector) else list(vecs)
        outs = [outs] if isinstance(outs, nek_dvector) else list(outs)
        if len(vecs) != len(outs) or not all(isinstance(x, nek_dvector) for x in vecs + outs):
            raise TypeError("type_error: as many nek_dvector in as out expected")
        s = len(vecs)
        ai = (vp * max(s, 1))(*[x.h for x in vecs])
        ao = (vp * max(s, 1))(*[x.h for x in outs])
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.shape != (3,):
            raise ValueError("coef = (c_lap, c_conv, c_p)")
        check(self.lib.nlg_lns_apply(self.h, s, ai, ao, int(bool(trans)), dptr(c)))

    def matvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        self.apply([vec_in], [vec_out], False)

    def rmatvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        self.apply([vec_in], [vec_out], True)

    def matvec_block(self, vecs: list, outs: list, trans: bool = False):
        self.apply(vecs, outs, trans)

    def close(self):
        if self.h:
            self.lib.nlg_lns_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def apply_L(lns: lns_linop, vec_in, vec_out, trans: bool = False):
    """reference: apply_L (neklab_linops.f90:382-404): nu lap(u) - conv(u) - grad(p)"""
    lns.apply(vec_in, vec_out, trans, LNS_COEF["apply_L"])


def apply_Lv(lns: lns_linop, vec_in, vec_out, trans: bool = False):
    """reference: apply_Lv (neklab_linops.f90:406-426): apply_L without the pressure gradient"""
    lns.apply(vec_in, vec_out, trans, LNS_COEF["apply_Lv"])


def compute_LNS_conv(lns: lns_linop, vec_in, vec_out, trans: bool = False):
    """reference: compute_LNS_conv (neklab_linops.f90:268-313): the linearised convective term, pointwise (+ sign)"""
    lns.apply(vec_in, vec_out, trans, LNS_COEF["compute_LNS_conv"])


def compute_LNS_laplacian(lns: lns_linop, vec_in, vec_out):
    """reference: compute_LNS_laplacian (neklab_linops.f90:315-330): nu lap(u)"""
    lns.apply(vec_in, vec_out, False, LNS_COEF["compute_LNS_laplacian"])


def compute_LNS_gradp(lns: lns_linop, vec_in, vec_out):
    """reference: compute_LNS_gradp (neklab_linops.f90:368-380): grad of the pressure mapped to the velocity mesh"""
    lns.apply(vec_in, vec_out, False, LNS_COEF["compute_LNS_gradp"])


# ------------------------------------------------------------------------------------------------------------------
# Eigenvalue sensitivity: wavemaker and base-flow gradient of an eigenvalue from a direct / adjoint pair (nlg_sens_apply,
# nlg_sens_pairing; the definitions stand in include/neklab_gpu.h)
def _sens_pairs(x, what: str):
    """(re, im | None) or a list of up to four such pairs -> (list of pairs, was a single pair)"""
    single = len(x) == 2 and isinstance(x[0], nek_dvector) and (x[1] is None or isinstance(x[1], nek_dvector))
    pairs = [tuple(x)] if single else [tuple(p) for p in x]
    for p in pairs:
        if len(p) != 2 or not isinstance(p[0], nek_dvector) or not (p[1] is None or isinstance(p[1], nek_dvector)):
            raise TypeError("type_error: %s is a pair (re, im | None) of nek_dvector or a list of such pairs" % what)
    return pairs, single


def sens_pairing(direct, adjoint) -> complex:
    """d = <u^+, u^> = (a_r.u_r + a_i.u_i) + i (a_r.u_i - a_i.u_r) of one pair, in the nek_ddot inner product (nlg_sens_pairing)."""
    (ur, ui), (ar, ai) = direct, adjoint
    d = np.zeros(2)
    check(ur.lib.nlg_sens_pairing(ur.h, ui.h if ui is not None else None, ar.h, ai.h if ai is not None else None, dptr(d)))
    return complex(d[0], d[1])


def eigenvalue_sensitivity(direct, adjoint, parts: bool = False, wavemaker: bool = True, average: bool = False, scale=None):
    """Structural sensitivity and base-flow gradient of an eigenvalue.  For real velocity fields u, a on mesh 1, with u~ = mask (.) u and
    a~ = mask (.) a (the velocity Dirichlet masks are applied on read, as apply_L does; d_j is the pointwise physical derivative gradm1
    of an element: no mass matrix, no gather-scatter):

        T(u, a)_j = - sum_i a~_i d_j u~_i          (transport part)
        P(u, a)_j = + sum_i u~_i d_i a~_j          (production part)
        S(u, a)   = T + P

    Then <a, [L(U + dU) - L(U)] u> = <S(u, a), dU> in the nek_ddot inner product, where L is the operator of apply_L, u is solenoidal
    and the boundary term of one integration by parts vanishes.  The term (div u) a_j is left out on purpose.  For a complex pair,
    direct u^ = u_r + i u_i with L u^ = lambda u^, adjoint u^+ = a_r + i a_i with L+ u^+ = conj(lambda) u^+:

        d       = <u^+, u^> = (a_r.u_r + a_i.u_i) + i (a_r.u_i - a_i.u_r)          (nek_ddot)
        S_re    = S(u_r, a_r) + S(u_i, a_i)        S_im = S(u_i, a_r) - S(u_r, a_i)
        grad_U lambda = (S_re + i S_im) / d        (same split for T and P)
        W(x)    = |u^(x)| |u^+(x)| / |d|           (wavemaker; |u^(x)|^2 = sum_i (u_r,i^2 + u_i,i^2))
        dlambda ~ <Re grad_U lambda, dU> + i <Im grad_U lambda, dU>

    `direct`, `adjoint`: (re, im | None) pairs of nek_dvector -- a real eigenpair has no imaginary parts -- or lists of up to four such
    pairs, which go through the kernel in one launch.  Returns (d, grad, transport, W): d complex; grad = (re, im) of nek_dvector, the
    gradient of the eigenvalue; transport the same of T alone (parts=True, else None); W a nek_dvector whose first velocity component
    carries the wavemaker (wavemaker=True, else None); lists of these when lists were given.  The fields are element-local, the form
    whose `dot` with a dU is the quadrature of the integrand; average=True replaces them by their multiplicity-weighted gather-scatter
    average (what `rand` applies), for plotting.  scale: the complex factor(s) used instead of 1 / d."""
    dpairs, single = _sens_pairs(direct, "direct")
    apairs, single_a = _sens_pairs(adjoint, "adjoint")
    if single != single_a or len(dpairs) != len(apairs):
        raise TypeError("type_error: as many direct as adjoint pairs expected")
    s = len(dpairs)
    mesh = dpairs[0][0].mesh
    lib = mesh.lib
    d = [sens_pairing(dp, ap) for dp, ap in zip(dpairs, apairs)] if s <= 4 else []
    if scale is None:
        if any(x == 0.0 for x in d):
            raise NlgError("eigenvalue_sensitivity: <adjoint, direct> vanishes: the pair cannot be normalised")
        fac = [1.0 / x for x in d]
    else:
        fac = [complex(x) for x in (np.atleast_1d(scale))]
        if len(fac) != s:
            raise ValueError("scale: one complex factor per pair")
    sc = np.array([[f.real, f.imag] for f in fac], dtype=np.float64).reshape(-1)
    new = lambda: nek_dvector(mesh, dpairs[0][0].nscal, dpairs[0][0].lorder)
    grad = [(new(), new()) for _ in range(s)]
    transport = [(new(), new()) for _ in range(s)] if parts else None
    W = [new() for _ in range(s)] if wavemaker else None
    n = max(s, 1)

    def arr(vs):
        if vs is None:
            return None
        return (vp * n)(*[(x.h if x is not None else None) for x in vs])

    check(lib.nlg_sens_apply(mesh.h, s, arr([p[0] for p in dpairs]), arr([p[1] for p in dpairs]), arr([p[0] for p in apairs]),
                             arr([p[1] for p in apairs]), dptr(sc), arr([g[0] for g in grad]), arr([g[1] for g in grad]),
                             arr([t[0] for t in transport]) if parts else None, arr([t[1] for t in transport]) if parts else None,
                             arr(W)))
    if average:
        vmult = mesh.get("vmult")
        for v in [x for g in grad for x in g] + ([x for t in transport for x in t] if parts else []) + (W or []):
            check(lib.nlg_op_dssum(mesh.h, v.h))
            for k in range(mesh.dim):
                v.set_field(k, v.get_field(k) * vmult)
    if single:
        return d[0], grad[0], transport[0] if parts else None, W[0] if wavemaker else None
    return d, grad, transport, W


def predict_eigenvalue_shift(grad, dU: nek_dvector) -> complex:
    """First-order shift of the eigenvalue under the base-flow change dU: <Re grad_U lambda, dU> + i <Im grad_U lambda, dU> with
    grad = (re, im) as eigenvalue_sensitivity returns it (element-local form)."""
    gre, gim = (grad.re, grad.im) if isinstance(grad, nek_zvector) else grad
    return complex(gre.dot(dU), gim.dot(dU))


def _match_adjoint_modes(lam_d, res_d, lam_a, res_a, match_tol):
    """For every direct eigenvalue the index of the adjoint eigenvalue closest to it; raises where they differ by more than the bound."""
    idx = []
    for k, lam in enumerate(lam_d):
        j = int(np.argmin(np.abs(lam_a - lam)))
        bound = match_tol if match_tol is not None else 10.0 * (abs(res_d[k]) + abs(res_a[j])) + 1e-10 * abs(lam)
        if abs(lam_a[j] - lam) > bound:
            raise NlgError("sensitivity_analysis: direct eigenvalue %d (%.12g%+.12gj) has no adjoint partner: the closest adjoint "
                           "eigenvalue is %.12g%+.12gj, %.3e away (bound %.3e)" % (k, lam.real, lam.imag, lam_a[j].real, lam_a[j].imag,
                                                                                   abs(lam_a[j] - lam), bound))
        idx.append(j)
    return idx


def sensitivity_analysis(exptA: exptA_linop, kdim: int, nev: int, tol: float = 0.0, outdir: str = ".", seed: int = 0,
                         outpost: bool = False, session: str = "neklab", parts: bool = False, average: bool = False,
                         match_tol: "float | None" = None, X0: "nek_dvector | None" = None):
    """Direct and adjoint stability analysis of the fixed point `exptA` was built about (linear_stability_analysis_fixed_point twice),
    the modes paired by eigenvalue, and eigenvalue_sensitivity of every pair.

    Pairing.  Both runs return their eigenvectors in the real LAPACK pair convention: for a complex pair at (k, k + 1), X[k] + i X[k+1]
    belongs to the eigenvalue of positive imaginary part, mu+.  The direct mode of lambda = log(mu+) / tau is u^ = X[k] + i X[k+1].
    The adjoint run's Y[j] + i Y[j+1] belongs to mu+ of the (real) adjoint propagator too, while the adjoint partner of lambda is the
    adjoint eigenvector of conj(lambda): u^+ = Y[j] - i Y[j+1].  (With Y[j] + i Y[j+1] instead, <u^+, u^> is the pairing with the mode of
    conj(lambda) and vanishes to rounding.)  One sensitivity per real eigenvalue and one per complex pair (for its mu+ member; that of
    the conjugate eigenvalue is the conjugate field).

    Raises if a direct eigenvalue has no adjoint eigenvalue within 10 x the sum of the two Ritz residuals of the multipliers (match_tol:
    another absolute bound on |mu_direct - mu_adjoint|; the adjoint is the discretised continuous one, so on a coarse mesh or with a
    large time step the two spectra differ by more than their residuals), or if |d| / (|u^| |u^+|) <= 1e-10: that level means the wrong
    partner.

    Writes sensitivity.npy, rows [Re lambda, Im lambda, Re d, Im d], and with outpost=True the field files sgr (Re grad), sgi (Im grad)
    and wmk (wavemaker).  Returns a dict: eigvals, d, grad, transport, W (lists, one entry per sensitivity), modes = the (direct, adjoint)
    pairs used, direct / adjoint = what the two stability runs returned, and seconds = the wall time of the three stages."""
    clock = [time.perf_counter()]
    run_d = linear_stability_analysis_fixed_point(exptA, kdim, nev, adjoint=False, X0=X0, tol=tol, outdir=outdir, seed=seed,
                                                  outpost=outpost, session=session)
    clock.append(time.perf_counter())
    run_a = linear_stability_analysis_fixed_point(exptA, kdim, nev, adjoint=True, X0=X0, tol=tol, outdir=outdir, seed=seed,
                                                  outpost=outpost, session=session)
    clock.append(time.perf_counter())
    lam_d, res_d, Xd, mu_d, _ = run_d
    lam_a, res_a, Xa, mu_a, _ = run_a
    match = _match_adjoint_modes(mu_d, res_d, mu_a, res_a, match_tol)
    # pairs of the adjoint run, as nlg_eigs forms them: a complex eigenvalue and its successor
    ahead, j = [-1] * nev, 0
    while j < nev:
        if mu_a[j].imag != 0.0:
            if j + 1 < nev:
                ahead[j] = ahead[j + 1] = j
            j += 2
        else:
            ahead[j] = j
            j += 1
    heads, lams, direct, adjoint = [], [], [], []
    k = 0
    while k < nev:
        j = match[k]
        lams.append(lam_d[k])
        if mu_d[k].imag == 0.0:
            heads.append(k)
            direct.append((Xd[k], None))
            adjoint.append((Xa[j], None))
            k += 1
            continue
        if k + 1 >= nev:
            lams.pop()
            break                                                    # the second member of the pair was not asked for
        jh = ahead[j]                                                # the adjoint run's pair that holds eigenvalue j
        if jh < 0:
            raise NlgError("sensitivity_analysis: the adjoint run returned one member only of the pair of eigenvalue %d" % k)
        # X[k] + i X[k+1] belongs to mu+ whichever member came first; lambda = the eigenvalue of positive imaginary part
        lams[-1] = lam_d[k] if mu_d[k].imag > 0.0 else lam_d[k + 1]
        aim = Xa[jh + 1].copy()
        aim.scal(-1.0)                                               # u^+ = Y[j] - i Y[j+1]
        heads.append(k)
        direct.append((Xd[k], Xd[k + 1]))
        adjoint.append((Xa[jh], aim))
        k += 2
    d, grad, transport, W = [], [], [], []
    for b in range(0, len(heads), 4):
        db, gb, tb, wb = eigenvalue_sensitivity(direct[b:b + 4], adjoint[b:b + 4], parts=parts, wavemaker=True, average=average)
        for q, (dp, ap) in enumerate(zip(direct[b:b + 4], adjoint[b:b + 4])):
            nd = np.sqrt(sum(x.dot(x) for x in dp if x is not None))
            na = np.sqrt(sum(x.dot(x) for x in ap if x is not None))
            if abs(db[q]) <= 1e-10 * nd * na:
                raise NlgError("sensitivity_analysis: |<u^+, u^>| = %.3e of |u^| |u^+| for eigenvalue %d: the adjoint mode is not its "
                               "partner" % (abs(db[q]) / (nd * na), heads[b + q]))
        d += db
        grad += gb
        transport += tb if parts else []
        W += wb
    exptA.mesh.ctx.sync()
    clock.append(time.perf_counter())
    lam = np.array(lams)
    np.save(os.path.join(outdir, "sensitivity.npy"), np.column_stack([lam.real, lam.imag, np.real(d), np.imag(d)]))
    if outpost:
        outpost_dnek([g[0] for g in grad], "sgr", session, outdir)
        outpost_dnek([g[1] for g in grad], "sgi", session, outdir)
        outpost_dnek(W, "wmk", session, outdir)
    return dict(eigvals=lam, d=d, grad=grad, transport=transport if parts else None, W=W, modes=list(zip(direct, adjoint)),
                direct=run_d, adjoint=run_a, seconds=dict(direct=clock[1] - clock[0], adjoint=clock[2] - clock[1], sensitivity=clock[3] - clock[2]))


# ------------------------------------------------------------------------------------------------------------------
# Optimally time-dependent (OTD) modes.  Reference: otd_opts / nek_otd (src/neklab_otd.f90), otd_analysis
# (src/neklab_analysis.f90:214-344).  The time stepping, the reduced operator, the forcing and the re-orthonormalisation are
# device work (nlg_otd_*, DESIGN.md 3.2 "OTD mode"); the r x r spectral analysis and the log files are host work, as in the
# reference.
class otd_opts:
    """reference: type otd_opts (src/neklab_otd.f90:51-72), same fields and defaults."""

    def __init__(self, startstep: int = 1, printstep: int = 5, orthostep: int = 10, iostep: int = 100, iorststep: int = 100,
                 n_usrIC: int = 0, trans: bool = False, solve_baseflow: bool = True, OTDIC_basename: str = "OTDIC_"):
        self.startstep, self.printstep, self.orthostep = int(startstep), int(printstep), int(orthostep)
        self.iostep, self.iorststep, self.n_usrIC = int(iostep), int(iorststep), int(n_usrIC)
        self.trans, self.solve_baseflow, self.OTDIC_basename = bool(trans), bool(solve_baseflow), str(OTDIC_basename)


def _fortran_e(x: float, w: int = 15, d: int = 8) -> str:
    """Fortran's Ew.d edit descriptor: 0.dddddddd E+ee, right-justified in w characters."""
    x = float(x)
    if x == 0.0 or not np.isfinite(x):
        body = ("0." + "0" * d + "E+00") if x == 0.0 else str(x)
        return body.rjust(w)
    mant, exp = ("%.*e" % (d - 1, abs(x))).split("e")          # d significant digits: m.ddd e ee with 1 <= m < 10
    digits, e = mant.replace(".", ""), int(exp) + 1
    body = "%s0.%sE%s%02d" % ("-" if x < 0 else "", digits, "-" if e < 0 else "+", abs(e))
    return body.rjust(w)


def otd_log_line(istep: int, time: float, *tagged) -> str:
    """One line of Ls.dat / Lr.dat: '(I8,1X,F15.8,A,*(1X,E15.8))', the (tag, values) groups following each other
    (spectral_analysis, src/neklab_otd.f90:225, :242, :262)."""
    s = "%8d %15.8f" % (istep, time)
    for tag, vals in tagged:
        s += tag + "".join(" " + _fortran_e(v) for v in vals)
    return s


class nek_otd:
    """reference: type nek_otd (src/neklab_otd.f90:37-49): r OTD modes about `baseflow`.  Keyword arguments are the options
    of exptA_linop (re, torder, dt, tolerances, filter ...); cfl_limit defaults to 0.4 as in init_OTD."""

    def __init__(self, baseflow: nek_dvector, r: int = 2, **cfg):
        cfg.setdefault("cfl_limit", 0.4)
        self.mesh, self.lib, self.baseflow, self.r = baseflow.mesh, baseflow.lib, baseflow, int(r)
        # OTD has no tau, but the operator's rule snaps dt to tau / ceil(tau / dt): with a given dt, tau = dt keeps the step as given;
        # with the CFL rule (dt = 0) the step is tau / ceil(tau c / cfl_limit), at most the CFL step, for tau = 1 unless `tau` is passed
        tau = cfg.pop("tau", None)
        if cfg.get("dt", 0.0) > 0.0:
            tau = cfg["dt"]
        self.op = exptA_linop(1.0 if tau is None else tau, baseflow, **cfg)
        self.h = None
        self.opts = None
        self._lns, self._lns_bf = None, None   # the strong-form L of matvec / rmatvec, created by the first call

    def init(self, opts: "otd_opts | None" = None, basis0: "list | None" = None, icdir: str = "."):
        """init_OTD (src/neklab_otd.f90:118-204): random basis (seeds 1 .. r), the first n_usrIC modes from
        `<OTDIC_basename>nn.fld`, orthonormalised; `basis0` (r vectors) replaces both."""
        opts = opts if opts is not None else otd_opts()
        if not 0 <= opts.n_usrIC <= self.r:
            raise ValueError("init_OTD: inconsistent number of IC fields to load: nIC = %d, r = %d" % (opts.n_usrIC, self.r))
        if basis0 is None and opts.n_usrIC > 0:
            from . import nekio
            basis0 = []
            for i in range(self.r):
                v = nek_dvector(self.mesh, 0, 1)
                if i < opts.n_usrIC:
                    path = os.path.join(icdir, "%s%02d.fld" % (opts.OTDIC_basename, i + 1))
                    if not os.path.exists(path):
                        raise FileNotFoundError("init_OTD: cannot find IC file: %s" % path)
                    f = nekio.read_fld(path)
                    nek2vec(v, f["ux"], f["uy"], f.get("uz"), pressure_from_mesh1(self.mesh, f["p"]) if "p" in f else None)
                else:
                    v.rand(True, seed=i + 1)
                basis0.append(v)
        o = _lib.OtdOpts()
        check(self.lib.nlg_otd_opts_default(C.byref(o)))
        o.r, o.startstep, o.orthostep = self.r, opts.startstep, opts.orthostep
        o.trans, o.solve_baseflow = int(opts.trans), int(opts.solve_baseflow)
        arr = None
        if basis0 is not None:
            if len(basis0) != self.r:
                raise ValueError("init_OTD: %d basis vectors for r = %d" % (len(basis0), self.r))
            arr = (vp * self.r)(*[x.h for x in basis0])
        h = vp()
        check(self.lib.nlg_otd_create(self.op.h, C.byref(o), arr, C.byref(h)))
        self.h, self.opts = h, opts

    def advance(self, n: int = 1):
        check(self.lib.nlg_otd_advance(self.h, int(n)))

    def reduced(self, form: str = "weak"):
        """(Lr, G): the basis is orthonormalised, then Lr_ij = <u_i, L u_j> on the current state; G is the Gram matrix before.
        form = "weak": L u_j in weak form from the operators of the time step (nlg_otd_reduced).  form = "strong": the reference's
        route (otd_analysis, src/neklab_analysis.f90:291-298), Lr_ij = <u_i, matvec(u_j)> (trans: rmatvec) with the pointwise L,
        the same G."""
        if form not in ("weak", "strong"):
            raise ValueError("reduced: form is 'weak' or 'strong'")
        Lr, G = np.zeros((self.r, self.r), order="F"), np.zeros((self.r, self.r), order="F")
        check(self.lib.nlg_otd_reduced(self.h, dptr(Lr), dptr(G)))
        if form == "strong":
            B = [self.basis(j) for j in range(self.r)]
            W = [nek_dvector(self.mesh) for _ in range(self.r)]
            self._apply_lns(B, W, bool(self.opts.trans))
            for i in range(self.r):
                for j in range(self.r):
                    Lr[i, j] = B[i].dot(W[j])
        return Lr, G

    # ---- nek_otd as an abstract_linop_rdp (src/neklab_otd.f90:44-45, :76-116): matvec = apply_LNS, rmatvec = apply_adjLNS
    def _apply_lns(self, vecs, outs, trans: bool):
        """apply_L with the vectors' own pressure, about the operator's base flow when it is frozen and about current_baseflow()
        when solve_baseflow is on (the base-flow side of the convective term is rebuilt before every such call)"""
        moving = self.h is not None and self.opts is not None and self.opts.solve_baseflow
        if self._lns is None:
            self._lns = lns_linop(self.baseflow, self.op.cfg.re)
        if moving:
            self._lns_bf = self.current_baseflow(self._lns_bf)
            self._lns.set_baseflow(self._lns_bf)
        self._lns.apply(vecs, outs, trans)

    def matvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        self._apply_lns([vec_in], [vec_out], False)

    def rmatvec(self, vec_in: nek_dvector, vec_out: nek_dvector):
        self._apply_lns([vec_in], [vec_out], True)

    def basis(self, i: int, out: "nek_dvector | None" = None) -> nek_dvector:
        out = out if out is not None else nek_dvector(self.mesh)
        check(self.lib.nlg_otd_get_basis(self.h, int(i), out.h))
        return out

    def current_baseflow(self, out: "nek_dvector | None" = None) -> nek_dvector:
        out = out if out is not None else nek_dvector(self.mesh)
        check(self.lib.nlg_otd_get_baseflow(self.h, out.h))
        return out

    def info(self) -> dict:
        a, t, dt = C.c_int64(), C.c_double(), C.c_double()
        check(self.lib.nlg_otd_info(self.h, C.byref(a), C.byref(t), C.byref(dt)))
        return {"istep": a.value, "time": t.value, "dt": dt.value}

    @staticmethod
    def spectral_analysis(Lr):
        """spectral_analysis (src/neklab_otd.f90:206-265), pure numpy: (sigma, svec, lambda, eigvec) -- the eigenvalues of
        (Lr + Lr^T) / 2 in descending order with their vectors, and the eigenvalues of Lr sorted by real part, descending, with
        theirs."""
        Lr = np.asarray(Lr, dtype=np.float64)
        s, v = np.linalg.eigh(0.5 * (Lr + Lr.T))
        idx = np.argsort(-s, kind="stable")
        lam, ev = np.linalg.eig(Lr)
        jdx = np.argsort(-lam.real, kind="stable")
        return s[idx], v[:, idx], lam[jdx].astype(complex), ev[:, jdx].astype(complex)

    def outpost_OTDmodes(self, eigvec, outdir: str = ".", session: str = "neklab", index: int = 1, time: float = 0.0):
        """outpost_OTDmodes (src/neklab_otd.f90:267-300): mode i = sum_j u_j Re(eigvec_ji) with the pressure of basis vector
        i, written as `m<ii><session>0.f<index>`."""
        B = [self.basis(j) for j in range(self.r)]
        paths = []
        for i in range(self.r):
            m = B[i].copy()
            m.scal(float(np.real(eigvec[i, i])))
            for j in range(self.r):
                if j != i:
                    m.axpby(float(np.real(eigvec[j, i])), B[j], 1.0)
            m.set_field(PR, B[i].get_field(PR))
            paths += outpost_dnek(m, "m%02d" % (i + 1), session, outdir, first_index=index, time=time)
        return paths

    def close(self):
        if getattr(self, "_lns", None) is not None:
            self._lns.close()
            self._lns = None
        if self.h:
            self.lib.nlg_otd_destroy(self.h)
            self.h = None
        if self.op is not None:
            self.op.close()
            self.op = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def otd_analysis(OTD: nek_otd, opts: "otd_opts | None" = None, nsteps: int = 100, outdir: str = ".", session: str = "neklab",
                 basis0: "list | None" = None):
    """reference: otd_analysis (src/neklab_analysis.f90:214-344).  The time loop runs on the device in chunks that end at the next
    print / io / restart step; there the basis is orthonormalised, Lr read out, and Ls.dat / Lr.dat, the projected modes
    (`m01`, ...) and the basis (`rst`) written.  Returns the logged rows: dicts of istep, time, sigma, lambda."""
    opts = opts if opts is not None else otd_opts()
    OTD.init(opts, basis0=basis0, icdir=outdir)
    for name in ("Ls.dat", "Lr.dat"):
        open(os.path.join(outdir, name), "w").close()
    every = [s for s in (opts.printstep, opts.iostep, opts.iorststep) if s > 0]
    rows, istep, nio, nrst = [], 0, 0, 0
    while istep < nsteps:
        nxt = min([nsteps] + [(istep // s + 1) * s for s in every])
        OTD.advance(nxt - istep)
        istep = nxt
        if istep < opts.startstep:
            continue
        hit = {k: getattr(opts, k) > 0 and istep % getattr(opts, k) == 0 for k in ("printstep", "iostep", "iorststep")}
        if not any(hit.values()):
            continue
        time = OTD.info()["time"]
        if hit["printstep"] or hit["iostep"]:
            Lr, _ = OTD.reduced()
            sigma, svec, lam, eigvec = OTD.spectral_analysis(Lr)
        if hit["printstep"]:
            with open(os.path.join(outdir, "Ls.dat"), "a") as f:
                f.write(otd_log_line(istep, time, (" Ls ", sigma)) + "\n")
            with open(os.path.join(outdir, "Lr.dat"), "a") as f:
                f.write(otd_log_line(istep, time, (" Lr%Re ", lam.real), (" Lr%Im ", lam.imag)) + "\n")
            rows.append({"istep": istep, "time": time, "sigma": sigma, "lambda": lam})
        if hit["iostep"]:
            nio += 1
            OTD.outpost_OTDmodes(eigvec, outdir, session, index=nio, time=time)
        if hit["iorststep"]:
            outpost_dnek([OTD.basis(j) for j in range(OTD.r)], "rst", session, outdir, first_index=nrst * OTD.r + 1, time=time)
            nrst += 1
    return rows


# ------------------------------------------------------------------------------------------------------------------
# DNS runs with history points and a recurrence monitor: the first stage of the reference's periodic-orbit workflow
# (examples/cylinder/dns/Re180: a nonlinear run whose userchk calls hpts() and prints rnorm = |u(t) - u_ref|; the period guess of
# examples/cylinder/newton/Re180_periodic_orbit was read off those two signals).
def locate_points(mesh, xyz, tol_r: float = 1e-10):
    """nlg_probe_locate on a host mesh (neklab_amd.mesh.BoxMesh or anything with dim, n, x, y, z, elem_gid): pure host code.
    -> dict(elem [local, -1], rst, status, dist)"""
    lib = _lib.load()
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, mesh.dim))
    npts = xyz.shape[0]
    x, y = np.ascontiguousarray(mesh.x, dtype=np.float64), np.ascontiguousarray(mesh.y, dtype=np.float64)
    z = np.ascontiguousarray(mesh.z, dtype=np.float64) if mesh.dim == 3 else None
    gid = None if mesh.elem_gid is None else np.ascontiguousarray(mesh.elem_gid, dtype=np.int64)
    elem, rst = np.zeros(npts, dtype=np.int64), np.zeros((npts, mesh.dim))
    status, dist = np.zeros(npts, dtype=np.int32), np.zeros(npts)
    rc = lib.nlg_probe_locate(mesh.dim, mesh.n, x.shape[0], dptr(x), dptr(y), None if z is None else dptr(z),
                              None if gid is None else gid.ctypes.data_as(_lib.c_int64_p), npts, dptr(xyz), float(tol_r),
                              elem.ctypes.data_as(_lib.c_int64_p), dptr(rst), status.ctypes.data_as(_lib.c_int_p), dptr(dist))
    if rc != 0:
        raise NlgError("nlg_probe_locate: bad argument")
    return {"elem": elem, "rst": rst, "status": status, "dist": dist}


class history_points:
    """Points at which fields are evaluated by their Lagrange interpolant (Nek5000's hpts with a .his file).  `status`, `elem`
    (global element id), `rst` and `dist` describe the location (nlg_probe_locate); a point in no element raises."""

    def __init__(self, mesh: Mesh, xyz, tol_r: float = 1e-10):
        self.mesh, self.lib = mesh, mesh.lib
        self.xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, mesh.dim))
        self.npts = self.xyz.shape[0]
        h = vp()
        check(self.lib.nlg_probes_create(mesh.h, self.npts, dptr(self.xyz), float(tol_r), C.byref(h)))
        self.h = h
        self.status, self.elem = np.zeros(self.npts, dtype=np.int32), np.zeros(self.npts, dtype=np.int64)
        self.rst, self.dist = np.zeros((self.npts, mesh.dim)), np.zeros(self.npts)
        check(self.lib.nlg_probes_status(h, self.status.ctypes.data_as(_lib.c_int_p), self.elem.ctypes.data_as(_lib.c_int64_p), dptr(self.rst),
                                         dptr(self.dist)))

    def sample(self, vecs) -> np.ndarray:
        """Fields of 1 to 4 nek_dvector at every point in one launch: [len(vecs)][npts][nf] (a single vector: [npts][nf]), fields =
        velocity components, pressure, temperature if the vectors carry one."""
        single = isinstance(vecs, nek_dvector)
        vecs = [vecs] if single else list(vecs)
        nf = self.mesh.dim + 1 + (1 if vecs[0].nscal >= 1 else 0)
        out = np.zeros((len(vecs), self.npts, nf))
        arr = (vp * len(vecs))(*[v.h for v in vecs])
        check(self.lib.nlg_probes_sample(self.h, len(vecs), arr, dptr(out)))
        return out[0] if single else out

    def close(self):
        if self.h:
            check(self.lib.nlg_probes_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------------------------
# Wall forces, torque and heat flux on sets of element faces (nlg_forces_*): drag, lift and Strouhal number of the reference's cylinder
# cases, the Nusselt number of its temperature cases.  Coefficients are the caller's division: Cd = 2 Fx / (rho U^2 L) with
# Fx = Fp[0] + Fv[0], Cl the same with Fy; the heat flux is -conductivity * Q.
def faces_from_bcs(bcs, tags=("W",), select=None):
    """[(elem_gid 0-based, face)] of the boundary faces of nekio.read_re2_bcs (its third return value) that carry one of `tags`;
    select(elem_gid, face) -> bool picks among them (e.g. the faces of one body)."""
    out = [(int(e) - 1, int(f)) for e, f, t in bcs if str(t) in tags]
    return [ef for ef in out if select is None or select(*ef)]


def faces_from_mask(hostmesh):
    """[(elem_gid, face)] of the faces of a host mesh on which every velocity mask is 0: the walls of a box mesh."""
    from .nekio import face_nodes
    n, dim, E = hostmesh.n, hostmesh.dim, hostmesh.E
    m = np.max(np.stack([np.asarray(a).reshape(E, -1) for a in hostmesh.mask]), axis=0)
    gid = np.arange(E) if hostmesh.elem_gid is None else hostmesh.elem_gid
    return [(int(gid[e]), f) for e in range(E) for f in range(1, 2 * dim + 1) if not m[e, face_nodes(n, dim, f)].any()]


def forces_geometry(hostmesh, faces, obj=None, nobj: int = 1, centres=None):
    """nlg_forces_geometry on a host mesh (anything with dim, n, x, y, z): pure host code.  faces = [(LOCAL element, face)].
    -> dict(nds [nf, nfp, dim], met [nf, nfp, dim, dim] (d r_j / d x_i at [j, i]), xc [nf, nfp, dim], area [nobj])"""
    lib = _lib.load()
    dim, n = hostmesh.dim, hostmesh.n
    x, y = np.ascontiguousarray(hostmesh.x, dtype=np.float64), np.ascontiguousarray(hostmesh.y, dtype=np.float64)
    z = np.ascontiguousarray(hostmesh.z, dtype=np.float64) if dim == 3 else None
    el = np.ascontiguousarray([e for e, _ in faces], dtype=np.int64)
    fc = np.ascontiguousarray([f for _, f in faces], dtype=np.int32)
    ob = None if obj is None else np.ascontiguousarray(obj, dtype=np.int32)
    c = None if centres is None else np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(nobj, dim))
    nf, nfp = len(faces), n ** (dim - 1)
    nds, met, xc, area = np.zeros((nf, nfp, dim)), np.zeros((nf, nfp, dim, dim)), np.zeros((nf, nfp, dim)), np.zeros(nobj)
    rc = lib.nlg_forces_geometry(dim, n, x.shape[0], dptr(x), dptr(y), None if z is None else dptr(z), nf, el.ctypes.data_as(_lib.c_int64_p),
                                 fc.ctypes.data_as(_lib.c_int_p), None if ob is None else ob.ctypes.data_as(_lib.c_int_p), int(nobj),
                                 None if c is None else dptr(c), dptr(nds), dptr(met), dptr(xc), dptr(area))
    if rc != 0:
        raise NlgError("nlg_forces_geometry: bad argument")
    return {"nds": nds, "met": met, "xc": xc, "area": area}


class wall_forces:
    """Forces, torque and heat flux on objects = list of lists of (elem_gid, face): see include/neklab_gpu.h (nlg_forces_*).  `area` is
    the objects' area (global); `local` the positions in the flattened list of the faces this rank holds, the rows of tractions()."""

    def __init__(self, mesh: Mesh, objects, centres=None):
        self.mesh, self.lib = mesh, mesh.lib
        self.nobj, self.dim = len(objects), mesh.dim
        self.faces = [(int(e), int(f)) for faces in objects for e, f in faces]
        obj = np.ascontiguousarray([o for o, faces in enumerate(objects) for _ in faces], dtype=np.int32)
        el = np.ascontiguousarray([e for e, _ in self.faces], dtype=np.int64)
        fc = np.ascontiguousarray([f for _, f in self.faces], dtype=np.int32)
        c = None if centres is None else np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(self.nobj, self.dim))
        self.nq = 2 * self.dim + 2 * (3 if self.dim == 3 else 1) + 1
        h = vp()
        self.h = None
        check(self.lib.nlg_forces_create(mesh.h, self.nobj, len(self.faces), el.ctypes.data_as(_lib.c_int64_p), fc.ctypes.data_as(_lib.c_int_p),
                                         obj.ctypes.data_as(_lib.c_int_p), None if c is None else dptr(c), C.byref(h)))
        self.h = h
        self.area = np.zeros(self.nobj)
        nl = C.c_int64()
        check(self.lib.nlg_forces_info(h, dptr(self.area), C.byref(nl)))
        held = set(int(g) for g in (np.arange(mesh.host.E) if mesh.host.elem_gid is None else mesh.host.elem_gid))
        self.local = [q for q, (e, _) in enumerate(self.faces) if e in held]
        assert len(self.local) == nl.value

    def sample(self, vecs, nu: float) -> np.ndarray:
        """[len(vecs)][nobj][NQ] (a single vector: [nobj][NQ]) in the order Fp[dim], Fv[dim], Tp[nt], Tv[nt], Q; global sums."""
        single = isinstance(vecs, nek_dvector)
        vecs = [vecs] if single else list(vecs)
        out = np.zeros((len(vecs), self.nobj, self.nq))
        arr = (vp * max(len(vecs), 1))(*[v.h for v in vecs])
        check(self.lib.nlg_forces_sample(self.h, len(vecs), arr, float(nu), dptr(out)))
        return out[0] if single else out

    def parts(self, out) -> dict:
        """the named parts of sample()'s last axis"""
        d, nt = self.dim, (3 if self.dim == 3 else 1)
        out = np.asarray(out)
        return {"Fp": out[..., :d], "Fv": out[..., d:2 * d], "Tp": out[..., 2 * d:2 * d + nt], "Tv": out[..., 2 * d + nt:2 * d + 2 * nt], "Q": out[..., -1]}

    def tractions(self, vec: nek_dvector, nu: float) -> dict:
        """Per face point of this rank's faces (rows = self.local): p [nl, nfp], trac [nl, nfp, dim] = p N - nu (grad u + grad u^T) N,
        nds [nl, nfp, dim] = N.  Cp and Cf along a wall follow by division by |N| and the dynamic pressure."""
        nl, nfp, d = len(self.local), self.mesh.host.n ** (self.dim - 1), self.dim
        p, t, nds = np.zeros((nl, nfp)), np.zeros((nl, nfp, d)), np.zeros((nl, nfp, d))
        check(self.lib.nlg_forces_tractions(self.h, vec.h, float(nu), dptr(p), dptr(t), dptr(nds)))
        return {"p": p, "trac": t, "nds": nds}

    def close(self):
        if self.h:
            check(self.lib.nlg_forces_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class nek_dns:
    """A nonlinear run from X0 with a fixed time step (`dt`, or the CFL rule at X0 with cfl_limit, 0.4 by default), sampled after every
    step: the fields at the history points and d(t) = |u(t) - u_ref|.  Keyword arguments are the options of exptA_linop.  While the run
    lives its operator refuses every other run; after close() a borrowed operator (`op=`) is the propagator about X0."""

    def __init__(self, X0: nek_dvector, re: float = 0.0, torder: int = 3, dt: float = 0.0, chunk: int = 256, op: "exptA_linop | None" = None, **cfg):
        self.mesh, self.lib, self.X0 = X0.mesh, X0.lib, X0
        self._own_op = op is None
        if op is None:
            cfg.setdefault("cfl_limit", 0.4)
            # a run has no tau, but the operator's rule snaps dt to tau / ceil(tau / dt): tau = dt keeps a given step as given (see nek_otd)
            tau = cfg.pop("tau", None)
            if dt > 0.0:
                tau = dt
            op = exptA_linop(1.0 if tau is None else tau, X0, re=re, torder=torder, dt=dt, **cfg)
        elif cfg or re or dt:
            raise TypeError("nek_dns: an existing operator brings its own options")
        self.op = op   # `op=`: the run borrows an existing operator (its dt rule, tolerances, filter); X0 becomes its base flow
        self.hp = None
        self.wf = None
        o = _lib.DnsOpts()
        check(self.lib.nlg_dns_opts_default(C.byref(o)))
        o.chunk = int(chunk)
        h = vp()
        self.h = None
        check(self.lib.nlg_dns_create(self.op.h, X0.h, C.byref(o), C.byref(h)))
        self.h = h

    def set_history_points(self, hp: "history_points | None"):
        """The series starts again from the state as it stands."""
        check(self.lib.nlg_dns_set_probes(self.h, None if hp is None else hp.h))
        self.hp = hp

    def set_wall_forces(self, wf: "wall_forces | None"):
        """Every sample also holds wf.sample(state, 1 / Re).  The series starts again from the state as it stands."""
        check(self.lib.nlg_dns_set_forces(self.h, None if wf is None else wf.h))
        self.wf = wf

    def set_reference(self, vec: "nek_dvector | None" = None):
        """u_ref of the recurrence norm: `vec`, or the state as it stands.  The series starts again from the state as it stands."""
        check(self.lib.nlg_dns_set_reference(self.h, None if vec is None else vec.h))

    def advance(self, nsteps: int = 1):
        check(self.lib.nlg_dns_advance(self.h, int(nsteps)))

    def series(self) -> dict:
        """time[nsamples], probe[nsamples, npts, nf], dist[nsamples], with wall forces attached also force[nsamples, nobj, NQ]; sample 0 is
        the state the series started from."""
        check(self.lib.nlg_dns_advance(self.h, 0))
        n = C.c_int64()
        check(self.lib.nlg_dns_count(self.h, C.byref(n)))
        npts = 0 if self.hp is None else self.hp.npts
        nf = self.mesh.dim + 1 + (1 if self.op.cfg.ifheat else 0)
        t, p, d = np.zeros(n.value), np.zeros((n.value, npts, nf)), np.zeros(n.value)
        check(self.lib.nlg_dns_series(self.h, 0, n.value, dptr(t), dptr(p) if p.size else None, dptr(d)))
        out = {"time": t, "probe": p, "dist": d}
        if self.wf is not None:
            f = np.zeros((n.value, self.wf.nobj, self.wf.nq))
            check(self.lib.nlg_dns_force_series(self.h, 0, n.value, dptr(f)))
            out["force"] = f
        return out

    def state(self, out: "nek_dvector | None" = None) -> nek_dvector:
        out = out if out is not None else nek_dvector(self.mesh, self.X0.nscal, self.X0.lorder)
        check(self.lib.nlg_dns_get_state(self.h, out.h))
        return out

    def info(self) -> dict:
        a, t, dt = C.c_int64(), C.c_double(), C.c_double()
        check(self.lib.nlg_dns_info(self.h, C.byref(a), C.byref(t), C.byref(dt)))
        return {"istep": a.value, "time": t.value, "dt": dt.value}

    def close(self):
        if self.h:
            self.lib.nlg_dns_destroy(self.h)
            self.h = None
        if self.op is not None and self._own_op:
            self.op.close()
        self.op = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def recurrence_period(time, dist, depth: float = 0.5):
    """The first return of a run to its reference state: the first interior sample k with d_k < d_{k-1}, d_k <= d_{k+1} and
    d_k <= depth * max_{j <= k} d_j; the period is the vertex of the parabola through the three samples of d^2 around it.
    -> (T, d_k / max d), or None if there is no such sample."""
    t, d = np.asarray(time, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    run_max = np.maximum.accumulate(d)
    for k in range(1, len(d) - 1):
        if d[k] < d[k - 1] and d[k] <= d[k + 1] and d[k] <= depth * run_max[k]:
            y0, y1, y2 = d[k - 1] ** 2, d[k] ** 2, d[k + 1] ** 2
            h0, h1 = t[k] - t[k - 1], t[k + 1] - t[k]
            # vertex of the parabola through (t[k] - h0, y0), (t[k], y1), (t[k] + h1, y2)
            s0, s1 = (y1 - y0) / h0, (y2 - y1) / h1
            curv = (s1 - s0) / (0.5 * (h0 + h1))
            T = t[k] if curv <= 0.0 else 0.5 * (t[k - 1] + t[k]) - s0 / curv
            return float(T), float(d[k] / d.max())
    return None


def probe_period(time, signal):
    """Mean spacing of the upward zero crossings of `signal` minus its mean, the crossings interpolated linearly; None with fewer
    than two crossings."""
    t, s = np.asarray(time, dtype=np.float64), np.asarray(signal, dtype=np.float64)
    s = s - s.mean()
    k = np.nonzero((s[:-1] < 0.0) & (s[1:] >= 0.0))[0]
    if len(k) < 2:
        return None
    tc = t[k] + (t[k + 1] - t[k]) * (-s[k]) / (s[k + 1] - s[k])
    return float((tc[-1] - tc[0]) / (len(tc) - 1))


def dns_orbit_guess(dns: nek_dns, nsteps: int, depth: float = 0.5):
    """A starting guess for newton_periodic_orbit from a run: the state as it stands becomes the reference snapshot, the run advances
    nsteps, and the first recurrence of d(t) gives the period.  -> nek_ext_dvector(X, T) where X IS THE REFERENCE SNAPSHOT, the state
    the run returned to after T, not the state at the end of the run; None if d(t) has no recurrence minimum in nsteps."""
    ref = dns.state()
    dns.set_reference(ref)
    dns.advance(nsteps)
    s = dns.series()
    got = recurrence_period(s["time"] - s["time"][0], s["dist"], depth)
    if got is None:
        return None
    return nek_ext_dvector(dns.mesh, ref.lorder, got[0], _vec=ref)
