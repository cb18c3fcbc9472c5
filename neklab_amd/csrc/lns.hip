// exptA_linop: exponential propagator of the linearised Navier-Stokes operator (gfx950).
//
// In-tree protocol followed (file:line under /root/reference):
//   exptA_matvec / exptA_rmatvec   src/linops/exponential_propagator.f90:15-60, :62-107
//   exptA_compute_rst / get_rst    src/linops/exponential_propagator.f90:109-142
//   init_exptA                     src/linops/exponential_propagator.f90:4-13
//   dt / nsteps rule               src/neklab_nek_setup.f90:195-200
// The time integrator behind `nek_advance` is Nek5000 code that is not in the reference tree; it is
// restated here from the published Pn-Pn-2 BDFk/EXTk splitting exactly as in oracle/lns.py.
//
// All solver scalars (alpha, beta, residual norms, the convergence flag) live in device memory; the
// host only reads the flag once per chunk of launched iterations, and every kernel of an iteration
// returns immediately once the flag is set, so the result is identical to stopping at convergence.
#include <cmath>
#include <functional>
#include <map>
#include <string>

#include "internal.h"

using namespace nlg;

namespace {

constexpr int NT = 256;
constexpr int NB = 512;   // fixed first-stage reduction grid

struct F3 {
    double *p[3];
};
struct CF3 {
    const double *p[3];
};
// Lane batching (block stepper): the per-lane work buffers of all lanes live in ONE slab at a constant stride `ld` doubles, so a
// kernel launched with gridDim.y = lanes reaches lane v's copy of every per-lane argument at `lane-0 pointer + v * ld`
// (blockIdx.y is wave-uniform: the offset is scalar arithmetic, no lane loop in the kernel body).  Single-vector launches pass
// gridDim.y = 1.  Arrays that belong to the mesh or to the base flow (weights, preconditioners, masks) are not offset.
__device__ __forceinline__ int64_t lane_lo(int64_t ld) { return (int64_t)blockIdx.y * ld; }
__device__ __forceinline__ F3 lane_f3(F3 a, int64_t lo) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (a.p[c]) a.p[c] += lo;
    return a;
}
__device__ __forceinline__ CF3 lane_f3(CF3 a, int64_t lo) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (a.p[c]) a.p[c] += lo;
    return a;
}

// solver scalar slots (doubles) inside a per-solver device block
enum { S_RZ = 0, S_PW = 1, S_RZN = 2, S_RN2 = 3, S_DONE = 4, S_ITERS = 5, S_ALPHA = 6, S_BETA = 7, S_T0 = 8, S_T1 = 9, S_T2 = 10,
       S_WMEAN = 11, S_ZMEAN = 12, S_RN20 = 13, S_AH = 16, S_N = 48 };
constexpr int kAlphaRing = 32;   // S_AH .. S_AH + 31: the step lengths of the last 32 iterations (iteration i at i mod 32), for the deferred solution update
constexpr double kFloor2 = 1e-28;   // stop when |r|^2 has dropped by 1e-28: further iterations only divide 0 by 0

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// two simultaneous block sums; results valid in thread 0
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sm) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        sm[wid] = a;
        sm[4 + wid] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = sm[0] + sm[1] + sm[2] + sm[3];
        b = sm[4] + sm[5] + sm[6] + sm[7];
    }
}

// three simultaneous block sums; results valid in thread 0
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double *sm) {
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        sm[wid] = a;
        sm[4 + wid] = b;
        sm[8 + wid] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = sm[0] + sm[1] + sm[2] + sm[3];
        b = sm[4] + sm[5] + sm[6] + sm[7];
        c = sm[8] + sm[9] + sm[10] + sm[11];
    }
}

// Projected PCG (P = I - 1 1^T / n on the mean-free subspace, see oracle/lns.py pcg_E): the means of
// w = A p and of z = M^-1 r ride along as extra partial sums of kernels that exist anyway.
// x = 0, r = b (in place), z = pc*r (stored unless store_z == 0) ; partial sums of (r,z)_ipw, (r,r)_nw and sum(z)
template <int NF>
__global__ __launch_bounds__(NT) void k_cg_init(int64_t n, F3 x, F3 r, F3 z, CF3 pc, const double *ipw,
                                                const double *nw, double *partial, int64_t ld, const unsigned char *__restrict__ mb, int defer_x,
                                                int store_z) {
    __shared__ double sm[12];
    const int64_t lo = lane_lo(ld);
    x = lane_f3(x, lo), r = lane_f3(r, lo), z = lane_f3(z, lo), partial += lo;
    double a = 0.0, b = 0.0, c3 = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double wi = ipw ? ipw[i] : 1.0, wn = nw[i];
        // mb: the preconditioner of component c is pc.p[0] (1 / diag) where bit c of the point's mask byte is set and 0 elsewhere
        const double inv = mb ? pc.p[0][i] : 0.0;
        const unsigned mk = mb ? mb[i] : 0u;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double rv = r.p[c][i];
            if (!defer_x) x.p[c][i] = 0.0;   // (deferred solution update: x is first WRITTEN by k_x_flush / never read before that)
            b += rv * rv * wn;
            if (mb || pc.p[c]) {      // pointwise (Jacobi) preconditioner; otherwise z comes from an operator
                const double zv = (mb ? (((mk >> c) & 1u) ? inv : 0.0) : pc.p[c][i]) * rv;
                if (store_z) z.p[c][i] = zv;   // (0: the operator kernel forms z from r and the same two operands, CGProblem::z_free)
                a += rv * zv * wi;
                c3 += zv;
            }
        }
    }
    block_sum3(a, b, c3, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = a;
        partial[NB + blockIdx.x] = b;
        partial[2 * NB + blockIdx.x] = c3;
    }
}

template <int NF>
__global__ __launch_bounds__(NT) void k_cg_pw(const double *s, int64_t n, CF3 p, CF3 w, const double *ipw, double *partial, int64_t ld) {
    __shared__ double sm[8];
    const int64_t lo = lane_lo(ld);
    s += lo, p = lane_f3(p, lo), w = lane_f3(w, lo), partial += lo;
    if (s[S_DONE] != 0.0) return;
    double a = 0.0, b = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double wi = ipw ? ipw[i] : 1.0;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double wv = w.p[c][i];
            a += p.p[c][i] * wv * wi;
            b += wv;
        }
    }
    block_sum2(a, b, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = a;
        partial[NB + blockIdx.x] = b;
    }
}

// x += alpha p (unless deferred) ; r -= alpha (w - wmean) ; z = pc r ; partial (r,z)_ipw, (r,r)_nw, sum(z)
// store_z == 0 (CGProblem::z_free): z lives in registers for the sums only -- its one reader, the direction update fused into the
// operator kernel, forms it again from r, 1 / diag and the mask byte (three streams fewer here, 1 1/8 more there)
// Two points per lane (16-byte accesses; every field length is a multiple of 32): eight streams per component are
// what this kernel is, so the width of an access is its efficiency.
template <int NF>
__global__ __launch_bounds__(NT) void k_cg_update(const double *s, int64_t n, F3 x, F3 r, F3 z, CF3 p, CF3 w, CF3 pc,
                                                  const double *ipw, const double *nw, double *partial, int64_t ld, int defer_x,
                                                  const unsigned char *__restrict__ mb, int store_z) {
    __shared__ double sm[12];
    const int64_t lo = lane_lo(ld);
    s += lo, x = lane_f3(x, lo), r = lane_f3(r, lo), z = lane_f3(z, lo), p = lane_f3(p, lo), w = lane_f3(w, lo), partial += lo;
    if (s[S_DONE] != 0.0) return;
    const double alpha = s[S_ALPHA], wmean = s[S_WMEAN];
    const bool dox = defer_x == 0;   // deferred: x is assembled from the direction history afterwards (k_x_flush / k_add_hist), p is not read here
    double a = 0.0, b = 0.0, c3 = 0.0;
    const int64_t n2 = n >> 1;
    const double2 *ipw2 = reinterpret_cast<const double2 *>(ipw), *nw2 = reinterpret_cast<const double2 *>(nw);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) {
        const double2 wi = ipw ? ipw2[i] : make_double2(1.0, 1.0), wn = nw2[i];
        // mb: pc.p[0] = 1 / diag for all components, the masks are the bits of one byte per point (3 arrays -> 1 + 1/8)
        const double2 inv = mb ? reinterpret_cast<const double2 *>(pc.p[0])[i] : make_double2(0.0, 0.0);
        const unsigned mk = mb ? reinterpret_cast<const unsigned short *>(mb)[i] : 0u;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            double2 *x2 = reinterpret_cast<double2 *>(x.p[c]), *r2 = reinterpret_cast<double2 *>(r.p[c]);
            const double2 wv = reinterpret_cast<const double2 *>(w.p[c])[i];
            double2 rv = r2[i];
            if (dox) {
                const double2 pv = reinterpret_cast<const double2 *>(p.p[c])[i];
                double2 xv = x2[i];
                xv.x += alpha * pv.x;
                xv.y += alpha * pv.y;
                x2[i] = xv;
            }
            rv.x -= alpha * (wv.x - wmean);
            rv.y -= alpha * (wv.y - wmean);
            double2 pcv = make_double2(1.0, 1.0);
            if (mb)
                pcv = make_double2(((mk >> c) & 1u) ? inv.x : 0.0, ((mk >> (8 + c)) & 1u) ? inv.y : 0.0);
            else if (pc.p[c])
                pcv = reinterpret_cast<const double2 *>(pc.p[c])[i];
            if (pcv.x == 0.0) rv.x = 0.0;   // Dirichlet dof (the Helmholtz preconditioner carries the mask): w is not masked
            if (pcv.y == 0.0) rv.y = 0.0;
            r2[i] = rv;
            b += rv.x * rv.x * wn.x + rv.y * rv.y * wn.y;
            if (mb || pc.p[c]) {
                double2 zv;
                zv.x = pcv.x * rv.x;
                zv.y = pcv.y * rv.y;
                if (store_z) reinterpret_cast<double2 *>(z.p[c])[i] = zv;
                a += rv.x * zv.x * wi.x + rv.y * zv.y * wi.y;
                c3 += zv.x + zv.y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // odd length: the last point
        const int64_t i = n - 1;
        const double wi = ipw ? ipw[i] : 1.0, wn = nw[i];
        for (int c = 0; c < NF; ++c) {
            if (dox) x.p[c][i] += alpha * p.p[c][i];
            double rv = r.p[c][i] - alpha * (w.p[c][i] - wmean);
            const double pcv = mb ? (((mb[i] >> c) & 1u) ? pc.p[0][i] : 0.0) : (pc.p[c] ? pc.p[c][i] : 1.0);
            if (pcv == 0.0) rv = 0.0;
            r.p[c][i] = rv;
            b += rv * rv * wn;
            if (mb || pc.p[c]) {
                const double zv = pcv * rv;
                if (store_z) z.p[c][i] = zv;
                a += rv * zv * wi;
                c3 += zv;
            }
        }
    }
    block_sum3(a, b, c3, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = a;
        partial[NB + blockIdx.x] = b;
        partial[2 * NB + blockIdx.x] = c3;
    }
}

// single-reduction PCG: p <- u + beta p ; s <- w + beta s ; x += alpha p ; r -= alpha s ; u = pc r  (u lives in `z`); partial (r, u)_ipw, (r, r)_nw.
// The first update of a solve (ITERS == 1 after the logic) takes p = u, s = w whatever the buffers held.
template <int NF>
__global__ __launch_bounds__(NT) void k_cg_update_sr(const double *s, int64_t n, F3 x, F3 r, F3 z, F3 p, F3 sd, CF3 w, CF3 pc,
                                                     const double *ipw, const double *nw, double *partial, int64_t ld) {
    __shared__ double sm[12];
    const int64_t lo = lane_lo(ld);
    s += lo, x = lane_f3(x, lo), r = lane_f3(r, lo), z = lane_f3(z, lo), p = lane_f3(p, lo), sd = lane_f3(sd, lo), w = lane_f3(w, lo), partial += lo;
    if (s[S_DONE] != 0.0) return;
    const double alpha = s[S_ALPHA], beta = s[S_BETA];
    const bool first = s[S_ITERS] == 1.0;
    double a = 0.0, b = 0.0, c3 = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double wi = ipw ? ipw[i] : 1.0, wn = nw[i];
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double uv = z.p[c][i], wv = w.p[c][i];
            const double pv = first ? uv : uv + beta * p.p[c][i];
            const double sv = first ? wv : wv + beta * sd.p[c][i];
            p.p[c][i] = pv;
            sd.p[c][i] = sv;
            x.p[c][i] += alpha * pv;
            double rv = r.p[c][i] - alpha * sv;
            const double pcv = pc.p[c][i];
            if (pcv == 0.0) rv = 0.0;   // Dirichlet dof (the preconditioner carries the mask): w is not masked
            r.p[c][i] = rv;
            const double zv = pcv * rv;
            z.p[c][i] = zv;
            a += rv * zv * wi;
            b += rv * rv * wn;
        }
    }
    block_sum3(a, b, c3, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = a;
        partial[NB + blockIdx.x] = b;
    }
}

// partial sums of (r,z)_ipw and sum(z) when z was produced by a preconditioning operator
// `xc`/`npe` (xc may be null): the coarse-grid part of z, one value per element of npe points, kept separate so
// that the coarse branch can run concurrently with the element-wise solves: z_total = z + xc[i / npe]
// Deferred solution update of the velocity PCG.  x = sum_i alpha_i p_i never changes the iteration, so k_cg_update does not touch it:
// the fused direction update of the operator kernel stores direction i into slot i mod PH of a ring of PH direction buffers (the
// write it makes anyway, at another address), the scalar logic keeps alpha_i, and x is assembled afterwards in the order of the
// iteration -- the same additions on the same operands, hence the same bits -- by k_add_hist (the velocity update that consumes x)
// and, for the rare solve with more than PH iterations, by k_x_flush every PH iterations.  Saves the two x streams and the p
// stream of every iteration of k_cg_update (26 -> 17 streams at three components) for one sweep over the directions per solve.
struct PHist {
    const double *p0[3];   // slot 0, one pointer per component; slot q is q * stride doubles behind
    int64_t stride;
    int ph;
};
// x += sum over the PH iterations `last` - PH + 1 .. `last`; launched right after the k_cg_update of iteration `last` (before the scalar
// logic that counts it), so "not converged yet" = the solve did run them all
template <int NF>
__global__ __launch_bounds__(NT) void k_x_flush(const double *__restrict__ s, int64_t n, F3 x, PHist H, int last, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    s += lo, x = lane_f3(x, lo);
    if (s[S_DONE] != 0.0) return;   // converged inside this window: k_add_hist takes what there is of it
    const int w0 = last - H.ph + 1;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double *__restrict__ pc = H.p0[c] + lo + i;
            double t = w0 > 0 ? x.p[c][i] : 0.0;   // the first window starts the sum (k_cg_init leaves x alone)
#pragma unroll 4
            for (int q = 0; q < H.ph; ++q) t += s[S_AH + ((w0 + q) & (kAlphaRing - 1))] * pc[q * H.stride];   // (alpha: wave-uniform scalar loads)
            x.p[c][i] = t;
        }
    }
}
// y = a + (x + sum of alpha_i p_i over the iterations since the last full window); x, p in the layout of the solve (slot: slab-permuted -> natural)
template <int NF>
__global__ __launch_bounds__(NT) void k_add_hist(const double *__restrict__ s, int64_t n, int np, const int *__restrict__ slot, F3 y, CF3 a, CF3 x, PHist H,
                                                 int64_t ld) {
    const int64_t lo = lane_lo(ld);
    s += lo, y = lane_f3(y, lo), a = lane_f3(a, lo), x = lane_f3(x, lo);
    const int iters = (int)s[S_ITERS];
    const int w0 = (iters / H.ph) * H.ph, cnt = iters - w0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        int64_t q = i;
        if (slot) {
            const int64_t e = i / np;
            q = e * np + slot[(int)(i - e * np)];
        }
        // the components side by side, four directions per trip: 4 NF independent loads in flight per lane (the sums stay per component, in
        // iteration order)
        double t[NF];
#pragma unroll
        for (int c = 0; c < NF; ++c) t[c] = w0 > 0 ? x.p[c][q] : 0.0;   // x holds the full windows, if there were any
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const double al = s[S_AH + ((w0 + k) & (kAlphaRing - 1))];
#pragma unroll
            for (int c = 0; c < NF; ++c) t[c] += al * H.p0[c][lo + q + k * H.stride];
        }
#pragma unroll
        for (int c = 0; c < NF; ++c) y.p[c][i] = a.p[c] ? a.p[c][i] + t[c] : t[c];   // (a == null: the solution itself, the pressure solve)
    }
}

template <int NF>
__global__ __launch_bounds__(NT) void k_cg_rz(const double *s, int gate, int64_t n, CF3 r, CF3 z, const double *ipw,
                                              const double *xc, int npe, double *partial, int64_t ld) {
    __shared__ double sm[8];
    const int64_t lo = lane_lo(ld);
    s += lo, r = lane_f3(r, lo), z = lane_f3(z, lo), partial += lo;
    if (gate && s[S_DONE] != 0.0) return;
    double a = 0.0, b = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double wi = ipw ? ipw[i] : 1.0;
        const double xv = xc ? xc[i / npe] : 0.0;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double zv = z.p[c][i] + xv;
            a += r.p[c][i] * zv * wi;
            b += zv;
        }
    }
    block_sum2(a, b, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = a;
        partial[2 * NB + blockIdx.x] = b;
    }
}

template <int NF>
__global__ __launch_bounds__(NT) void k_cg_pupdate(const double *s, int64_t n, F3 p, CF3 z, const double *xc, int npe, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    s += lo, p = lane_f3(p, lo), z = lane_f3(z, lo);
    if (s[S_DONE] != 0.0) return;
    const double beta = s[S_BETA], zmean = s[S_ZMEAN];
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double xv = xc ? xc[i / npe] : 0.0;
#pragma unroll
        for (int c = 0; c < NF; ++c) p.p[c][i] = (z.p[c][i] + xv - zmean) + beta * p.p[c][i];
    }
}

// where the first-stage partial sums of up to three reductions live (they may come from different kernels)
struct Red {
    const double *p[3];
    int n[3];
};

// scalar logic, one thread. mode 0: after init (T0 = rz, T1 = rn2, T2 = sum z) ; 1: after pw (T0 = pw, T1 = sum w) ;
// 2: after update (T0 = rz, T1 = rn2, T2 = sum z).  inv_n = 1/n for the projected solve, 0 otherwise.
__device__ __forceinline__ void cg_post_logic(double *s, int mode, double tol2, int use_tol, int maxit, double inv_n) {
    if (mode != 0 && s[S_DONE] != 0.0) return;
    if (mode == 0) {
        s[S_RZ] = s[S_T0];
        s[S_RN2] = s[S_T1];
        s[S_ZMEAN] = s[S_T2] * inv_n;
        s[S_WMEAN] = 0.0;
        s[S_BETA] = 0.0;
        s[S_ITERS] = 0.0;
        s[S_DONE] = 0.0;     // the first p-update must run; the convergence test happens in mode 3
    } else if (mode == 3) {
        s[S_RN20] = s[S_RN2];
        s[S_DONE] = ((use_tol && s[S_RN2] < tol2) || maxit <= 0 || s[S_RN2] <= 0.0) ? 1.0 : 0.0;
    } else if (mode == 1) {
        s[S_PW] = s[S_T0];
        s[S_WMEAN] = s[S_T1] * inv_n;
        s[S_ALPHA] = s[S_RZ] / s[S_T0];
        s[S_AH + ((int)s[S_ITERS] & (kAlphaRing - 1))] = s[S_ALPHA];
    } else if (mode == 4) {
        // single-reduction PCG (Chronopoulos & Gear 1989): T0 = (w, u) with w = A u, u = M^-1 r;  T1 = (r, u);  T2 = |r|^2 -- all of the
        // CURRENT residual, in one reduction.  The convergence test standard PCG makes before applying the operator comes one operator
        // application late here (the price of the merged reduction): one wasted application per solve.
        if (s[S_ITERS] > 0.0 && ((use_tol && s[S_T2] < tol2) || s[S_ITERS] >= (double)maxit || s[S_T2] <= kFloor2 * s[S_RN20])) {
            s[S_RN2] = s[S_T2];
            s[S_DONE] = 1.0;
            return;
        }
        const bool first = s[S_ITERS] == 0.0;
        const double beta = first ? 0.0 : s[S_T1] / s[S_RZ];
        s[S_ALPHA] = first ? s[S_T1] / s[S_T0] : s[S_T1] / (s[S_T0] - beta * s[S_T1] / s[S_ALPHA]);
        s[S_BETA] = beta;
        s[S_RZ] = s[S_T1];
        s[S_RN2] = s[S_T2];
        s[S_PW] = s[S_T0];
        s[S_ITERS] += 1.0;
    } else {
        s[S_BETA] = s[S_T0] / s[S_RZ];
        s[S_RZ] = s[S_T0];
        s[S_RN2] = s[S_T1];
        s[S_ZMEAN] = s[S_T2] * inv_n;
        s[S_ITERS] += 1.0;
        if ((use_tol && s[S_T1] < tol2) || s[S_ITERS] >= (double)maxit || s[S_T1] <= kFloor2 * s[S_RN20]) s[S_DONE] = 1.0;
    }
}

// `red` (several ranks): the all-reduced sums of all lanes, [lane][3]; copied into the lane's S_T slots first
__global__ void k_cg_post(double *s, int mode, double tol2, int use_tol, int maxit, double inv_n, int64_t ld, const double *red, int nsums) {
    s += lane_lo(ld);
    if (red)
        for (int q = 0; q < nsums; ++q) s[S_T0 + q] = red[3 * blockIdx.y + q];
    cg_post_logic(s, mode, tol2, use_tol, maxit, inv_n);
}

// Second-stage reduction and (single rank: no all-reduce in between) the scalar logic in one launch.  One block of
// 1024 threads; the (up to three) sums are accumulated together so that their loads overlap, and the per-thread
// loop is unrolled four-fold for the same reason: the kernel is pure load latency.
constexpr int NTF = 1024;
__global__ __launch_bounds__(NTF) void k_cg_final_post(double *s, Red rd, int nsums, int gate, int mode, double tol2,
                                                       int use_tol, int maxit, double inv_n, int post, int64_t ld, double *red) {
    __shared__ double sm[3][NTF / 64];
    const int64_t lo = lane_lo(ld);
    s += lo;
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (rd.p[q]) rd.p[q] += lo;
    if (gate && s[S_DONE] != 0.0) {
        // several ranks: a finished lane still takes part in the all-reduce of the lanes that are not; it contributes zeros
        if (red && threadIdx.x < 3) red[3 * blockIdx.y + threadIdx.x] = 0.0;
        return;
    }
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q >= nsums) break;
        const double *__restrict__ p = rd.p[q];
        const int n = rd.n[q];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int i = threadIdx.x;
        for (; i + 3 * NTF < n; i += 4 * NTF) {
            a0 += p[i];
            a1 += p[i + NTF];
            a2 += p[i + 2 * NTF];
            a3 += p[i + 3 * NTF];
        }
        for (; i < n; i += NTF) a0 += p[i];
        acc[q] = (a0 + a1) + (a2 + a3);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double a = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) sm[q][wid] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 0; q < nsums; ++q) {
            double a = 0.0;
            for (int w = 0; w < NTF / 64; ++w) a += sm[q][w];
            s[S_T0 + q] = a;
            if (red) red[3 * blockIdx.y + q] = a;
        }
        if (post) cg_post_logic(s, mode, tol2, use_tol, maxit, inv_n);   // several ranks: the all-reduce comes first
    }
}

// ---- residual projection of the pressure solve (Fischer 1998; Nek5000 `residualProj = yes`, 1cyl.par:23) ----
// X = up to PROJ_L previous solution increments, A-orthonormal (A = P E P), B = A X.  All on the device, no host sync.
constexpr int PROJ_L = 8;
// partial[v * NB + blk] = sum over the block's share of X_v . y   (v < nvec <= PROJ_L)
__global__ __launch_bounds__(NT) void k_proj_dots(int64_t n, const double *__restrict__ X, int64_t stride, int nvec,
                                                  const double *__restrict__ y, double *__restrict__ partial, int64_t ld) {
    __shared__ double sm[PROJ_L][NT / 64];
    const int64_t lo = lane_lo(ld);
    X += lo, y += lo, partial += lo;
    double a[PROJ_L];
#pragma unroll
    for (int v = 0; v < PROJ_L; ++v) a[v] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double yv = y[i];
#pragma unroll
        for (int v = 0; v < PROJ_L; ++v)
            if (v < nvec) a[v] += X[v * stride + i] * yv;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < PROJ_L; ++v) {
        double t = a[v];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if (lane == 0) sm[v][wid] = t;
    }
    __syncthreads();
    if (threadIdx.x < PROJ_L) {
        double t = 0.0;
        for (int w = 0; w < NT / 64; ++w) t += sm[threadIdx.x][w];
        partial[threadIdx.x * NB + blockIdx.x] = t;
    }
}
// out[v] = sum_blk partial[v * NB + blk]
__global__ __launch_bounds__(NT) void k_proj_reduce(const double *__restrict__ partial, int nblk, int nvec, double *__restrict__ out, int64_t ld) {
    __shared__ double sm[NT / 64];
    partial += lane_lo(ld), out += lane_lo(ld);
    for (int v = 0; v < nvec; ++v) {
        double t = 0.0;
        for (int i = threadIdx.x; i < nblk; i += NT) t += partial[v * NB + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0;
            for (int w = 0; w < NT / 64; ++w) a += sm[w];
            out[v] = a;
        }
        __syncthreads();
    }
}
// y += sgn * sum_v c[v] M_v
__global__ __launch_bounds__(NT) void k_proj_comb(int64_t n, double *__restrict__ y, const double *__restrict__ M, int64_t stride,
                                                  int nvec, const double *__restrict__ c, double sgn, int64_t ld) {
    double cv[PROJ_L];
    y += lane_lo(ld), M += lane_lo(ld), c += lane_lo(ld);
#pragma unroll
    for (int v = 0; v < PROJ_L; ++v) cv[v] = v < nvec ? sgn * c[v] : 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        double a = y[i];
#pragma unroll
        for (int v = 0; v < PROJ_L; ++v)
            if (v < nvec) a += cv[v] * M[v * stride + i];
        y[i] = a;
    }
}
// new basis pair: X_new = v / sqrt(nrm2), B_new = w / sqrt(nrm2); a non-positive nrm2 stores zeros (a harmless member)
__global__ __launch_bounds__(NT) void k_proj_store(int64_t n, const double *__restrict__ v, const double *__restrict__ w,
                                                   const double *__restrict__ nrm2, double *__restrict__ Xn, double *__restrict__ Bn, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    v += lo, w += lo, nrm2 += lo, Xn += lo, Bn += lo;
    const double q = nrm2[0];
    const double sc = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        Xn[i] = sc * v[i];
        Bn[i] = sc * w[i];
    }
}

// ---- wavenumber projection of the projected propagator (proj_alpha, src/linops/exponential_propagator_proj.f90:135-173):
// every velocity component keeps only its cos(alpha x) / sin(alpha x) content along the homogeneous direction,
//   u <- cv <2 u cv> + sv <2 u sv>,   <f> = sum_line bm1 f / sum_line bm1 over the points of a line along that direction
// (Nek5000's planar_avg over the gtpp gather-scatter handle).  One wave per line; the lane of a block run sits in gridDim.y (a
// single vector is the block of one): lane l's fields lie l * ld behind lane 0's (the slab), its cos / sin tables l * tld behind
// lane 0's -- tld = 0: one wavenumber for all lanes, tld = n: one per lane (wavenumber lanes) -- and the lines, the weights and the
// denominators are shared.  Lanes whose bit in `mask` is clear are left alone (history replay: only the lanes that carry a history
// level are reloaded and projected).  The summation order of a line is fixed (stride 64, then the butterfly), so a lane's result
// depends on its own field and table only, not on the block it is part of.
//
// the line of this wave, with u, cv, sv moved to the lane; false: nothing to do (lane not in `mask`, or past the last line)
template <typename U>
__device__ __forceinline__ bool proj_line(int64_t nlines, const int *__restrict__ off, unsigned mask, int64_t ld, int64_t tld, U &u,
                                          const double *__restrict__ &cv, const double *__restrict__ &sv, int64_t &g, int &b, int &e) {
    if (!((mask >> blockIdx.y) & 1u)) return false;
    g = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (g >= nlines) return false;
    u = lane_f3(u, lane_lo(ld));
    cv += lane_lo(tld), sv += lane_lo(tld);
    b = off[g], e = off[g + 1];
    return true;
}
// ac[c], as[c] = sum over the points b .. e-1 of the line of 2 bm1 u_c cv and 2 bm1 u_c sv, in every lane of the wave
template <int NF>
__device__ __forceinline__ void proj_line_sums(int b, int e, const int *__restrict__ idx, const double *__restrict__ bm1, const double *cv,
                                               const double *sv, const CF3 &u, double (&ac)[NF], double (&as)[NF]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < NF; ++c) ac[c] = as[c] = 0.0;
    for (int q = b + lane; q < e; q += 64) {
        const int i = idx[q];
        const double w = 2.0 * bm1[i], c0 = cv[i], s0 = sv[i];
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double v = u.p[c][i];
            ac[c] += w * v * c0;
            as[c] += w * v * s0;
        }
    }
#pragma unroll
    for (int c = 0; c < NF; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ac[c] += __shfl_xor(ac[c], o, 64);
            as[c] += __shfl_xor(as[c], o, 64);
        }
    }
}
// u_c = cv (ac[c] / den) + sv (as[c] / den) on the points of the line, id = 1 / den
template <int NF>
__device__ __forceinline__ void proj_line_write(int b, int e, const int *__restrict__ idx, const double *cv, const double *sv, double id,
                                                const double (&ac)[NF], const double (&as)[NF], const F3 &u) {
    for (int q = b + (threadIdx.x & 63); q < e; q += 64) {
        const int i = idx[q];
#pragma unroll
        for (int c = 0; c < NF; ++c) u.p[c][i] = cv[i] * (ac[c] * id) + sv[i] * (as[c] * id);
    }
}
// one rank: sums and write-back in one kernel
template <int NF>
__global__ __launch_bounds__(NT) void k_proj_alpha(int64_t nlines, const int *__restrict__ off, const int *__restrict__ idx,
                                                   const double *__restrict__ bm1, const double *__restrict__ cv,
                                                   const double *__restrict__ sv, int64_t tld, const double *__restrict__ inv_den,
                                                   F3 u, int64_t ld, unsigned mask) {
    int64_t g;
    int b, e;
    if (!proj_line(nlines, off, mask, ld, tld, u, cv, sv, g, b, e)) return;
    double ac[NF], as[NF];
    proj_line_sums<NF>(b, e, idx, bm1, cv, sv, CF3{{u.p[0], u.p[1], u.p[2]}}, ac, as);
    proj_line_write<NF>(b, e, idx, cv, sv, inv_den[g], ac, as, u);
}
// Several ranks: a line along the homogeneous direction may cross rank boundaries.  The weighted sums of a rank's part of a
// line go to the line's slots in a global array, [gslot][gridDim.y][2][NF] (one gslot per distinct line label over all ranks),
// the array is all-reduced -- one all-reduce for all lanes -- and a second kernel applies the projection with the global sums.
template <int NF>
__global__ __launch_bounds__(NT) void k_proj_sums(int64_t nlines, const int *__restrict__ off, const int *__restrict__ idx,
                                                  const int *__restrict__ gslot, const double *__restrict__ bm1,
                                                  const double *__restrict__ cv, const double *__restrict__ sv, int64_t tld, CF3 u,
                                                  int64_t ld, unsigned mask, double *__restrict__ glob) {
    int64_t g;
    int b, e;
    if (!proj_line(nlines, off, mask, ld, tld, u, cv, sv, g, b, e)) return;
    double ac[NF], as[NF];
    proj_line_sums<NF>(b, e, idx, bm1, cv, sv, u, ac, as);
    if ((threadIdx.x & 63) == 0) {
        double *dst = glob + ((int64_t)gslot[g] * gridDim.y + blockIdx.y) * (2 * NF);
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            dst[2 * c] = ac[c];
            dst[2 * c + 1] = as[c];
        }
    }
}
template <int NF>
__global__ __launch_bounds__(NT) void k_proj_apply(int64_t nlines, const int *__restrict__ off, const int *__restrict__ idx,
                                                   const int *__restrict__ gslot, const double *__restrict__ cv,
                                                   const double *__restrict__ sv, int64_t tld, const double *__restrict__ inv_den,
                                                   const double *__restrict__ glob, F3 u, int64_t ld, unsigned mask) {
    int64_t g;
    int b, e;
    if (!proj_line(nlines, off, mask, ld, tld, u, cv, sv, g, b, e)) return;
    const double *src = glob + ((int64_t)gslot[g] * gridDim.y + blockIdx.y) * (2 * NF);
    double ac[NF], as[NF];
#pragma unroll
    for (int c = 0; c < NF; ++c) ac[c] = src[2 * c], as[c] = src[2 * c + 1];
    proj_line_write<NF>(b, e, idx, cv, sv, inv_den[g], ac, as, u);
}
// weights of a rank's part of every line into the global slots (set-up: the denominators)
__global__ __launch_bounds__(NT) void k_proj_wsum(int64_t nlines, const int *__restrict__ off, const int *__restrict__ idx,
                                                  const int *__restrict__ gslot, const double *__restrict__ w, double *__restrict__ glob) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (g >= nlines) return;
    double a = 0.0;
    for (int q = off[g] + lane; q < off[g + 1]; q += 64) a += w[idx[q]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) glob[gslot[g]] = a;
}
__global__ __launch_bounds__(NT) void k_proj_iden(int64_t nlines, const int *__restrict__ gslot, const double *__restrict__ glob, double *__restrict__ iden) {
    for (int64_t g = blockIdx.x * (int64_t)NT + threadIdx.x; g < nlines; g += (int64_t)gridDim.x * NT) iden[g] = 1.0 / glob[gslot[g]];
}

__global__ __launch_bounds__(NT) void k_cossin(int64_t n, const double *__restrict__ x, double alpha, double *__restrict__ cv,
                                               double *__restrict__ sv) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        cv[i] = cos(alpha * x[i]);
        sv[i] = sin(alpha * x[i]);
    }
}

// F_v -= bm1 (cr f_re,v + ci f_im,v) for the NL lanes of a forced run: a body force in the explicit term (the stored F is +N, the
// right-hand side takes -EXT(F)).  Every lane has its own forcing vectors (by value: they are the caller's, not part of the slab;
// a null f_im is a real forcing); lane v of F lies v * ld behind lane 0; bm1 is read once per point for all lanes.
struct ForceLanes {
    const double *re[kMaxLanes][3], *im[kMaxLanes][3];
};
template <int NF, int NL>
__global__ __launch_bounds__(NT) void k_add_force(int64_t n, F3 F, const double *__restrict__ bm1, ForceLanes f, double cr, double ci, int64_t ld) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double b = bm1[i];
#pragma unroll
        for (int v = 0; v < NL; ++v)
#pragma unroll
            for (int c = 0; c < NF; ++c) F.p[c][v * ld + i] -= b * (cr * f.re[v][c][i] + (f.im[v][c] ? ci * f.im[v][c][i] : 0.0));
    }
}

// ---- optimally time-dependent modes (nlg_otd_*): R <= 4 lanes of the slab, lane v at v * ld behind the lane-0 pointers ----
// device block of an nlg_otd: the reduced sums S and G (what the all-reduce carries), then Lr, C, T, the Gram matrix the last
// transform was made from, and a flag (non-zero: that matrix was not positive definite); all R x R column-major, 16 doubles each
enum { OTD_S = 0, OTD_G = 16, OTD_LR = 32, OTD_C = 48, OTD_T = 64, OTD_G0 = 80, OTD_FLAG = 96, OTD_N = 128 };

// First stage of the 2 R^2 sums  S_ij = sum_c sum u_i,c (gp_j,c - w_j,c - N_j,c)  and  G_ij = sum_c sum bm1 u_i,c u_j,c  (WITH_S =
// false: G only): every field is read once for all (i, j); partial[q * NB + block], q = i + R j (S), R^2 + i + R j (G).  Fixed grid
// and fixed summation order, no atomics.
template <int DIM, int R, bool WITH_S>
__global__ __launch_bounds__(NT) void k_otd_reduce(int64_t n, CF3 u, CF3 gp, CF3 w, CF3 N, const double *__restrict__ bm1, int64_t ld,
                                                   double *__restrict__ partial) {
    __shared__ double sm[2 * R * R][NT / 64];
    double S[R * R], G[R * R];
#pragma unroll
    for (int q = 0; q < R * R; ++q) S[q] = G[q] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double b = bm1[i];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double uv[R], Wv[R];
#pragma unroll
            for (int v = 0; v < R; ++v) {
                const int64_t q = v * ld + i;
                uv[v] = u.p[c][q];
                Wv[v] = WITH_S ? (gp.p[c][q] - w.p[c][q]) - N.p[c][q] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const double bu = b * uv[j];
#pragma unroll
                for (int a = 0; a < R; ++a) {
                    if (WITH_S) S[a + R * j] += uv[a] * Wv[j];
                    if (a <= j) G[a + R * j] += uv[a] * bu;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int a = j + 1; a < R; ++a) G[a + R * j] = G[j + R * a];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < R * R; ++q) {
        const double s = wave_sum(S[q]), g = wave_sum(G[q]);
        if (lane == 0) {
            sm[q][wid] = s;
            sm[R * R + q][wid] = g;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * R * R) {
        double t = 0.0;
        for (int k = 0; k < NT / 64; ++k) t += sm[threadIdx.x][k];
        partial[threadIdx.x * NB + blockIdx.x] = t;
    }
}
// second stage: block q sums its row of first-stage sums; out[q] for q < R^2, out[OTD_G + q - R^2] above
__global__ __launch_bounds__(NT) void k_otd_reduce2(const double *__restrict__ partial, int nblk, int rr, double *__restrict__ out) {
    static_assert(NT == 256, "the pairwise sum of the four wave sums below is written out for 256 threads");
    __shared__ double sm[NT / 64];
    const int q = blockIdx.x;
    double t = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NT) t += partial[q * NB + i];
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[q < rr ? OTD_S + q : OTD_G + (q - rr)] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
// Lr = S + h2 G (the w of the time step carries h2 B u) and the upper-triangular C = Lr - Phi of the forcing, Phi skew:
// C_jj = Lr_jj, C_ij = Lr_ij + Lr_ji (i < j), 0 below the diagonal.  One thread.
__global__ void k_otd_coef(double *d, int r, double h2) {
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < r; ++i) d[OTD_LR + i + r * j] = d[OTD_S + i + r * j] + h2 * d[OTD_G + i + r * j];
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < r; ++i)
            d[OTD_C + i + r * j] = i == j ? d[OTD_LR + i + r * j] : (i < j ? d[OTD_LR + i + r * j] + d[OTD_LR + j + r * i] : 0.0);
}
// F_j += bm1 sum_{i <= j} u_i C_ij for all lanes (the stored F is +N and enters the right-hand side with -EXT: this is -bm1 U C)
template <int DIM, int R>
__global__ __launch_bounds__(NT) void k_otd_force(int64_t n, F3 F, CF3 u, const double *__restrict__ bm1, const double *__restrict__ d, int64_t ld) {
    double C[R * R];
#pragma unroll
    for (int q = 0; q < R * R; ++q) C[q] = d[OTD_C + q];
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double b = bm1[i];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double uv[R];
#pragma unroll
            for (int v = 0; v < R; ++v) uv[v] = u.p[c][v * ld + i];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                double a = 0.0;
#pragma unroll
                for (int v = 0; v <= j; ++v) a += uv[v] * C[v + R * j];
                F.p[c][j * ld + i] += b * a;
            }
        }
    }
}
// T = chol(G)^-T, upper triangular (G = L L^T, T = L^-T: the columns of U T are orthonormal, and the leading k x k block of T is the
// T of the first k modes); G is kept in OTD_G0.  One thread; a pivot that is not positive raises the flag and leaves T = I.
__global__ void k_otd_chol(double *d, int r) {
    double L[16], Li[16];
    bool ok = true;
    for (int q = 0; q < r * r; ++q) {
        d[OTD_G0 + q] = d[OTD_G + q];
        L[q] = Li[q] = 0.0;
    }
    for (int j = 0; j < r && ok; ++j) {
        double s = d[OTD_G + j + r * j];
        for (int k = 0; k < j; ++k) s -= L[j + r * k] * L[j + r * k];
        if (!(s > 0.0)) {
            ok = false;
            break;
        }
        L[j + r * j] = sqrt(s);
        for (int i = j + 1; i < r; ++i) {
            double t = d[OTD_G + i + r * j];
            for (int k = 0; k < j; ++k) t -= L[i + r * k] * L[j + r * k];
            L[i + r * j] = t / L[j + r * j];
        }
    }
    for (int j = 0; j < r && ok; ++j) {   // column j of L^-1 by forward substitution
        Li[j + r * j] = 1.0 / L[j + r * j];
        for (int i = j + 1; i < r; ++i) {
            double t = 0.0;
            for (int k = j; k < i; ++k) t -= L[i + r * k] * Li[k + r * j];
            Li[i + r * j] = t / L[i + r * i];
        }
    }
    if (!ok) d[OTD_FLAG] = 1.0;
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < r; ++i) d[OTD_T + i + r * j] = ok ? Li[j + r * i] : (i == j ? 1.0 : 0.0);
}
// X <- X T in place for a list of slab levels (blockIdx.y): every point loads its R lane values, combines them and stores them
struct OtdLevels {
    double *p[20];
    int64_t n[20];
};
template <int R>
__global__ __launch_bounds__(NT) void k_otd_transform(OtdLevels lv, const double *__restrict__ d, int64_t ld) {
    double T[R * R];
#pragma unroll
    for (int q = 0; q < R * R; ++q) T[q] = d[OTD_T + q];
    double *__restrict__ x = lv.p[blockIdx.y];
    const int64_t n = lv.n[blockIdx.y];
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        double xv[R];
#pragma unroll
        for (int v = 0; v < R; ++v) xv[v] = x[v * ld + i];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            double a = 0.0;
#pragma unroll
            for (int v = 0; v <= j; ++v) a += xv[v] * T[v + R * j];
            x[j * ld + i] = a;
        }
    }
}

// F_i -= bm1 * buoy_i * theta : Boussinesq buoyancy in the explicit term (the stored F is +N)
template <int NF>
__global__ __launch_bounds__(NT) void k_buoyancy(int64_t n, F3 F, const double *__restrict__ bm1, const double *__restrict__ theta,
                                                 double b0, double b1, double b2) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double t = bm1[i] * theta[i];
        F.p[0][i] -= b0 * t;
        if (NF > 1) F.p[1][i] -= b1 * t;
        if (NF > 2) F.p[2][i] -= b2 * t;
    }
}

// generic pointwise helpers
template <int NF>
__global__ __launch_bounds__(NT) void k_colmul_gated(const double *s, F3 w, CF3 wt, int64_t n, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    if (s) s += lo;
    w = lane_f3(w, lo);
    if (s && s[S_DONE] != 0.0) return;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
#pragma unroll
        for (int c = 0; c < NF; ++c) w.p[c][i] *= wt.p[c][i];
    }
}

// rhs_i = sum_j ab_j F_j,i + (bm1/dt) sum_j bd_j u_j,i
struct Hist {
    const double *f[3][3];   // [level][component]
    const double *u[3][3];
    double ab[3], bd[3];
    int k;
    int half_lane = -1;   // the lane whose explicit terms enter with a factor 1/2 (coupled mode: the base-flow lane, N(U) = 1/2 lns_conv(U; U))
};
// `gp` / `w` non-null: the residual form of the tentative-velocity problem in the same pass, rhs_i += gp_i - w_i (D^T p - H u)
// XP: the result is written masked and in the slab-permuted layout of the velocity solve (slot = element-local table), so that its
// gather-scatter runs on that layout's lists and the solve needs no permutation pass (the Dirichlet mask is the same for every copy
// of a dof, so masking before the gather-scatter gives the bits masking after it gave)
template <int NF, bool XP = false>
__global__ __launch_bounds__(NT) void k_rhs(int64_t n, Hist h, const double *bm1, double rdt, F3 rhs, int64_t ld, CF3 gp = CF3{{nullptr, nullptr, nullptr}},
                                            CF3 w = CF3{{nullptr, nullptr, nullptr}}, const int *__restrict__ slot = nullptr, int np = 1,
                                            CF3 mask = CF3{{nullptr, nullptr, nullptr}}, const unsigned char *__restrict__ mb = nullptr) {
    // mb (XP): the three masks as the bits of one byte per point, in the slab-permuted layout (the velocity solve's maskb_v), instead of
    // `mask`; a product with 1.0 or 0.0 as before, so a masked entry keeps the sign of its zero
    // (the lane offset is added at the loads: writing it into `h` would move the by-value struct from the kernel-argument segment,
    //  where the runtime index j costs a scalar load, into scratch memory -- measured 123 -> 315 us)
    const int64_t lo = lane_lo(ld);
    rhs = lane_f3(rhs, lo);
    // (1.0 and 0.5 scale the coefficients exactly: every other lane sums what it summed without the factor, bit for bit, and the
    //  base-flow lane what the nonlinear step sums with its -1/2 EXT coefficients)
    const double fs = (int)blockIdx.y == h.half_lane ? 0.5 : 1.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double b = bm1[i] * rdt;
        int64_t q = i;
        if (XP) {
            const int64_t e = i / np;
            q = e * np + slot[(int)(i - e * np)];
        }
        const unsigned mk = (XP && mb) ? mb[q] : 0u;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            double a = 0.0, u = 0.0;
            for (int j = 0; j < h.k; ++j) {
                a += (fs * h.ab[j]) * h.f[j][c][lo + i];
                u += h.bd[j] * h.u[j][c][lo + i];
            }
            double v = a + b * u;
            if (gp.p[c]) v = (v + gp.p[c][lo + i]) - w.p[c][lo + i];
            rhs.p[c][q] = XP ? (mb ? (((mk >> c) & 1u) ? 1.0 : 0.0) : mask.p[c][i]) * v : v;
        }
    }
}

// y_c = a_c + s1 * b_c + s2 * c_c   (any of b, c may be null)
template <int NF>
__global__ __launch_bounds__(NT) void k_lin3(int64_t n, F3 y, CF3 a, CF3 b, double s1, CF3 c, double s2, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    y = lane_f3(y, lo), a = lane_f3(a, lo), b = lane_f3(b, lo), c = lane_f3(c, lo);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            double v = a.p[q][i];
            if (b.p[q]) v += s1 * b.p[q][i];
            if (c.p[q]) v += s2 * c.p[q][i];
            y.p[q][i] = v;
        }
    }
}

// y_c = a_c + b_c with b stored in the slab-permuted element layout (the solution of the velocity PCG): the un-permutation rides in
// the update of the velocity instead of being a pass of its own
template <int NF>
__global__ __launch_bounds__(NT) void k_add_xp(int64_t n, int np, const int *__restrict__ slot, F3 y, CF3 a, CF3 b, int64_t ld) {
    const int64_t lo = lane_lo(ld);
    y = lane_f3(y, lo), a = lane_f3(a, lo), b = lane_f3(b, lo);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int64_t e = i / np;
        const int64_t q = e * np + slot[(int)(i - e * np)];
#pragma unroll
        for (int c = 0; c < NF; ++c) y.p[c][i] = a.p[c][i] + b.p[c][q];
    }
}

// y_c += s * wt_c * x_c  (velocity correction: the inverse mass / mask weights of opbinv ride in the update)
template <int NF, bool SLOT = false>
__global__ __launch_bounds__(NT) void k_axpy_w(int64_t n, F3 y, CF3 x, CF3 wt, double s, int64_t ld, const int *__restrict__ slot = nullptr, int np = 1,
                                               const unsigned char *__restrict__ mb = nullptr) {
    // SLOT: x is stored in an element-local permutation (the face-grouped layout of the pressure operator's intermediates)
    // mb: wt_c = bit c of mb ? wt.p[0] : 0 with wt.p[0] = binvm1 and the mask bytes both in the layout of x (3 weight arrays -> 1 + 1/8;
    // the masks are zeros and ones, so these are the values of mask_c * binvm1)
    const int64_t lo = lane_lo(ld);
    y = lane_f3(y, lo), x = lane_f3(x, lo);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        int64_t q = i;
        if (SLOT) {
            const int64_t e = i / np;
            q = e * np + slot[(int)(i - e * np)];
        }
        const double bv = mb ? wt.p[0][q] : 0.0;
        const unsigned mk = mb ? mb[q] : 0u;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            const double wv = mb ? (((mk >> c) & 1u) ? bv : 0.0) : wt.p[c][i];
            y.p[c][i] += s * (wv * x.p[c][q]);
        }
    }
}

__global__ __launch_bounds__(NT) void k_scale1(int64_t n, double *y, const double *x, double s) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] = s * x[i];
}
__global__ __launch_bounds__(NT) void k_axpy1(int64_t n, double *y, const double *x, double s, int64_t ld) {
    y += lane_lo(ld), x += lane_lo(ld);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] += s * x[i];
}
__global__ __launch_bounds__(NT) void k_recipmask(int64_t n, double *y, const double *d, const double *mask) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] = mask[i] / d[i];
}
__global__ __launch_bounds__(NT) void k_maskbits(int64_t n, double *y, const double *m0, const double *m1, const double *m2) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        y[i] = (m0[i] != 0.0 ? 1.0 : 0.0) + (m1 && m1[i] != 0.0 ? 2.0 : 0.0) + (m2 && m2[i] != 0.0 ? 4.0 : 0.0);
}
__global__ __launch_bounds__(NT) void k_to_bytes(int64_t n, unsigned char *y, const double *x) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] = (unsigned char)x[i];
}
__global__ __launch_bounds__(NT) void k_recip1(int64_t n, double *y, const double *d) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] = 1.0 / d[i];
}
__global__ __launch_bounds__(NT) void k_mul3_acc(int64_t n, double *y, const double *a, const double *b, double s) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] += s * a[i] * b[i];
}
__global__ __launch_bounds__(NT) void k_mul3(int64_t n, double *y, const double *a, const double *b, double s) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) y[i] = s * a[i] * b[i];
}

// Time derivative of a state from the levels a time step keeps (periodic-orbit Newton, nlg_upo_fdot): field f = blockIdx.y of
// `nf` fields (the velocity components, then the pressure) in ONE launch,
//   out_f = (acc ? out_f : 0) + sum_j c[f][j] src[f][j]        (a null source is skipped),
// so that the BDF-k sum over the velocity levels and the first difference of the pressure are the same pass.
struct DdtArgs {
    double *out[4];
    const double *src[4][3];
    double c[4][3];
    int64_t n[4];
    int acc;
};
__global__ __launch_bounds__(NT) void k_bdf_ddt(DdtArgs A) {
    const int f = blockIdx.y;
    const int64_t n = A.n[f];
    double *__restrict__ out = A.out[f];
    const double *s0 = A.src[f][0], *s1 = A.src[f][1], *s2 = A.src[f][2];
    const double c0 = A.c[f][0], c1 = A.c[f][1], c2 = A.c[f][2];
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        double v = A.acc ? out[i] : 0.0;
        if (s0) v += c0 * s0[i];
        if (s1) v += c1 * s1[i];
        if (s2) v += c2 * s2[i];
        out[i] = v;
    }
}

inline int grid_for(int64_t n) {
    int64_t g = (n + NT - 1) / NT;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}
inline int red_grid(int64_t n) {
    int64_t g = (n + NT * 4 - 1) / (NT * 4);
    if (g > NB) g = NB;
    if (g < 1) g = 1;
    return (int)g;
}

const double BDF_B0[4] = {0.0, 1.0, 1.5, 11.0 / 6.0};
const double BDF_C[4][3] = {{0, 0, 0}, {1.0, 0, 0}, {2.0, -0.5, 0}, {3.0, -1.5, 1.0 / 3.0}};
const double EXT_C[4][3] = {{0, 0, 0}, {1.0, 0, 0}, {2.0, -1.0, 0}, {3.0, -3.0, 1.0}};

// the iteration counts of one solve in one lane: they predict how many iterations the next solve launches before the host first
// looks at the convergence flags (CGProblem::chunk), so each lane keeps its own, as if it ran alone
struct IterPred {
    int last;
    std::vector<int> hist;   // iteration counts of the previous matvec, by time-step index (the pattern repeats)
    int predict(int istep) const { return (istep < (int)hist.size() && hist[istep] > 0) ? hist[istep] : last; }
    void record(int istep, int iters) {
        last = iters;
        if ((int)hist.size() <= istep) hist.resize(istep + 1, 0);
        hist[istep] = iters;
    }
};
struct LanePred {
    IterPred v{8}, p{16};   // velocity and pressure solves
    int last_titers = 8;    // scalar solve
};

// wavenumber projection on one mesh: lines along the homogeneous direction (groups of local dofs, off / idx), cos / sin of alpha x,
// 1 / sum of the weights of a line; several ranks: slot of every local line in the global line list, number of global lines and
// the all-reduce buffer ([nglob][lanes of the block][2][nf]).  Lane l of a block reads the tables at cv + l * tld and sv + l * tld:
// tld = 0, one table, one wavenumber for all lanes (nlg_linop_set_projection); tld = n, nalpha tables, one wavenumber per lane
// (nlg_linop_set_projection_lanes).  Nothing else distinguishes the two kinds of operator here.
struct ProjLines {
    int nlines = 0;
    int *off = nullptr, *idx = nullptr, *gslot = nullptr;
    int64_t nglob = 0;
    int64_t tld = 0;
    double *cv = nullptr, *sv = nullptr, *iden = nullptr, *glob = nullptr;
    const double *weight = nullptr;   // the mesh's mass matrix (not owned)
    void free() {
        for (int *q : {off, idx, gslot}) (void)hipFree(q);
        for (double *q : {cv, sv, iden, glob}) (void)hipFree(q);
        *this = ProjLines();
    }
};

}  // namespace

struct nlg_otd;
struct nlg_dns;

struct nlg_linop {
    nlg_mesh *mesh = nullptr;
    nlg_otd *otd = nullptr;    // an OTD run lives on this operator: the lanes of the slab hold its state (nlg_otd_create)
    nlg_dns *dns = nullptr;    // a DNS run lives on this operator: lane 0 holds its state (nlg_dns_create)
    nlg_exptA_config cfg;
    nlg_vec *baseflow = nullptr;
    bool inited = false;
    bool set_up = false;   // the allocations that do not depend on the base flow or tau are made (nlg_linop_init)
    double dt = 0, cfl = 0;
    int nsteps = 0;
    // convective-term precomputation on the fine mesh
    double *Ur[3] = {}, *GU[9] = {};
    // Every pointer of the list in lane_buffers is lane 0's copy of a per-lane work buffer; lane v's copy is at_lane(op, ptr, v).
    // state: three rotating velocity buffers and three rotating forcing buffers per component
    double *ubuf[3][3] = {};   // [slot][component]; slot 0 = current, 1 = lag1, 2 = lag2 (after rotation)
    double *fbuf[3][3] = {};
    double *p = nullptr;
    // work
    double *rhs[3] = {}, *x[3] = {}, *z[3] = {}, *pv[3] = {}, *w[3] = {}, *gp[3] = {};
    // single-reduction PCG (Chronopoulos-Gear; opt-in, NLG_PCG_SINGLE_RED=1): the search direction and its image as recurrences
    bool use_sr = false;
    int php = 0;               // the same for the pressure PCG (ring prh[php][lps]; the update rides in the preconditioner, the direction update in the gradient kernel)
    double *prh = nullptr;
    int ph = 0;                // depth of the direction ring of the velocity PCG (deferred solution update, k_add_hist); 0 = x updated every iteration
    double *phist = nullptr;   // [ph][dim][lvs]
    double *cgs[3] = {}, *tcgs = nullptr;
    bool rhs_in_xp = false;   // adv_a -> helm_problem: the right-hand side already is masked and in the slab-permuted layout
    double *pr_r = nullptr, *pr_x = nullptr, *pr_z = nullptr, *pr_p = nullptr, *pr_w = nullptr;
    double *pr_b = nullptr;    // the right-hand side the pressure PCG started from (after the projection): A x = b - r afterwards
    double *pcv[4][3] = {};    // mask_i / diag(H) per BDF order
    // velocity PCG in the x-planes-first layout (3-D, lx1 <= 8: internal.h xp_slot): the preconditioners and the residual
    // weight permuted once; 0 = natural layout (2-D)
    int use_xp = -1;
    double *pcv_xp[4][3] = {}, *nwv_xp = nullptr;
    // the same preconditioners as ONE array 1 / diag(H) per BDF order plus one mask byte per point (bit c = mask of component c), in the
    // layout of the velocity solve: what k_cg_init / k_cg_update read (3 streams -> 1 + 1/8); pci_l[k] = {pci[k], pci[k], pci[k]}
    double *pci[4] = {}, *pci_l[4][3] = {};
    unsigned char *maskb_v = nullptr;
    // the velocity PCG does not store z = pc r: the operator kernel forms it (3-D, compact preconditioner, not the single-reduction
    // variant, a size sem_axhelm_forms_z accepts; NLG_PCG_STORE_Z=1 restores the stored z).  Decided by nlg_linop_init
    bool z_free = false;
    bool store_z = false;   // NLG_PCG_STORE_Z=1
    double *pce = nullptr;     // 1 / diag(E)
    double *prX = nullptr, *prB = nullptr, *d_pc = nullptr;   // pressure residual projection: PROJ_L solution / image pairs, coefficients
    int nproj = 0;
    double *nwv = nullptr;     // binvm1 * vmult / volvm1
    double *nwp = nullptr;     // bm2inv / volvm2
    double *d_s = nullptr;     // solver scalars (two blocks of S_N)
    double *d_part = nullptr;  // first-stage sums written by opdiv ([2][E]) and by the FDM kernel ([2][E/4])
    double *d_cgpart = nullptr;   // [3][NB] first-stage sums of the PCG vector kernels
    double *d_red = nullptr;      // several ranks: [lanes][3] sums of all lanes for ONE all-reduce (not in the slab)
    double *h_s = nullptr;     // pinned
    // All per-lane work buffers (integrator state, PCG vectors, projection space, scalars, partial sums) are carved from ONE
    // allocation of `slab_cap` lanes at a constant stride `slab_ld` doubles: lane v's copy of any of them is lane 0's
    // pointer + v * slab_ld, which is what lets one launch with gridDim.y = lanes serve the whole block (lane_lo()).
    double *slab = nullptr;
    int64_t slab_ld = 0;
    int slab_cap = 0;
    int istep = 0;   // the lanes of a block step advance in lockstep: one time-step index for all (the mode of the run: struct Lanes)
    LanePred pred[kMaxLanes];
    int adv_k = 1;             // state handed from one phase of a time step to the next (adv_a / adv_b / adv_c)
    double adv_b0 = 1.0, adv_h2 = 0.0;
    ProjLines proj_v, proj_p;   // wavenumber projection (exptA_proj_linop) on the velocity mesh and on the pressure mesh (no lines = not projected)
    int proj_lanes = 0;         // > 0: lane l of a block run projects onto its own wavenumber, proj_lanes of them (nlg_linop_set_projection_lanes)
    // Boussinesq coupling (cfg.ifheat): temperature levels, its explicit terms, PCG work fields, Jacobi preconditioners per
    // BDF order, gradient of the base temperature on the fine mesh
    double *tbuf[3] = {}, *ftbuf[3] = {}, *trhs = nullptr, *tx = nullptr, *tz = nullptr, *tpv = nullptr, *tw = nullptr;
    double *pct[4] = {}, *GT[3] = {};
    bool filt_fused = true;
    double *d_filt = nullptr;  // explicit modal filter (cfg.filter_weight > 0): the dense 1-D matrix F, [n][n]; belongs to the operator, not the mesh
    // coupled (orbit) mode, nlg_linop_set_orbit: `baseflow` holds X0, the state the base-flow lane starts every matvec from; that lane
    // is one more lane of the block step (the last one), advanced by the nonlinear step while the lanes before it are advanced by
    // the step linearised about its current state.  orbit_end: its state after the nsteps of the last matvec, Phi_T(X0).
    bool orbit = false, orbit_end_valid = false;
    nlg_vec *orbit_end = nullptr;
    // periodic-orbit Newton (nlg_upo_*): a fixed step count for the orbit (0 = the usual rule) and the two time derivatives of the
    // base flow taken from the run, upo_f0 = (U^1 - U^0) / dt and upo_fT = BDF-k derivative at level nsteps (capture_fdot)
    int orbit_nsteps = 0;
    bool upo_fdot_valid = false;
    nlg_vec *upo_f0 = nullptr, *upo_fT = nullptr;
    int64_t lane_viters[kMaxLanes] = {}, lane_piters[kMaxLanes] = {};   // iterations per lane of the last run (begin_run)
    int64_t st_steps = 0, st_viters = 0, st_piters = 0, st_titers = 0, st_matvecs = 0;   // summed over the lanes
};

// Optimally time-dependent modes: r lanes of the operator's slab advanced as ONE continuous run (no restart-history protocol), the
// base flow as lane r when it is solved alongside (coupled mode of the block step).  d: the device block OTD_*; part: first-stage sums.
struct nlg_otd {
    nlg_linop *op = nullptr;
    nlg_otd_opts o;
    int r = 0, nl = 0, lb = -1;
    double *d = nullptr, *part = nullptr;
    double time = 0.0;
};
// A DNS run: lane 0 of the operator's slab advanced by the nonlinear step as ONE continuous run, sampled after every step into a ring
// on the device -- slot k = [npts][nf] history-point values, then dist2 = |u - u_ref|^2, then the [nobj][NQ] wall forces if any are
// attached -- that is copied to the host series when it fills and when the series is read.
struct nlg_dns {
    nlg_linop *op = nullptr;
    nlg_dns_opts o;
    nlg_probes *probes = nullptr;
    nlg_vec *ref = nullptr;
    nlg_forces *forces = nullptr;
    int nf = 0;               // fields per point: velocity, pressure, temperature if carried
    int64_t np = 0, nforce = 0;   // npts * nf history-point values, nobj * NQ force values
    int64_t slot_len = 1;     // np + 1 + nforce
    int fill = 0;             // slots of the ring in use
    bool started = false;     // sample 0 of the series is taken
    double *ring = nullptr, *part = nullptr;
    std::vector<double> time, probe, dist2, force;   // the series on the host
};
// every entry point that would overwrite the lanes refuses while an OTD or a DNS run lives on the operator
#define NLG_NO_OTD(op, who)                                                                                                                           \
    do {                                                                                                                                              \
        NLG_CHECK(!(op)->otd, "%s: an nlg_otd lives on this operator and its lanes hold the OTD state; nlg_otd_destroy it first", who);              \
        NLG_CHECK(!(op)->dns, "%s: an nlg_dns lives on this operator and lane 0 holds its state; nlg_dns_destroy it first", who);                     \
    } while (0)

namespace {

int lalloc(nlg_linop *op, double **p, int64_t n) {
    NLG_HIP(hipMalloc(p, sizeof(double) * (size_t)n));
    NLG_HIP(hipMemsetAsync(*p, 0, sizeof(double) * (size_t)n, op->mesh->ctx->stream));
    return 0;
}

// ---- the lane slab ----------------------------------------------------------------------------------------------------
// every per-lane work buffer of the integrator, in slab order: f(pointer member, length in doubles).  The rotating history
// buffers come first and are contiguous, so that one strided memset clears the integrator state of all lanes.
template <typename F>
void lane_buffers(nlg_linop *op, F f) {
    nlg_mesh *m = op->mesh;
    const int dim = m->dim;
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < dim; ++c) f(&op->ubuf[s][c], m->lvs);
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < dim; ++c) f(&op->fbuf[s][c], m->lvs);
    if (op->cfg.ifheat) {
        for (int q = 0; q < 3; ++q) f(&op->tbuf[q], m->lvs);
        for (int q = 0; q < 3; ++q) f(&op->ftbuf[q], m->lvs);
    }
    for (int c = 0; c < dim; ++c) {
        f(&op->rhs[c], m->lvs);
        f(&op->x[c], m->lvs);
        f(&op->z[c], m->lvs);
        f(&op->pv[c], m->lvs);
        f(&op->w[c], m->lvs);
        f(&op->gp[c], m->lvs);
    }
    if (op->cfg.ifheat)
        for (double **v : {&op->trhs, &op->tx, &op->tz, &op->tpv, &op->tw}) f(v, m->lvs);
    if (op->ph > 0) f(&op->phist, (int64_t)op->ph * dim * m->lvs);
    if (op->php > 0) f(&op->prh, (int64_t)op->php * m->lps);
    if (op->use_sr) {
        for (int c = 0; c < dim; ++c) f(&op->cgs[c], m->lvs);
        if (op->cfg.ifheat) f(&op->tcgs, m->lvs);
    }
    for (double **q : {&op->p, &op->pr_r, &op->pr_x, &op->pr_z, &op->pr_p, &op->pr_w, &op->pr_b}) f(q, m->lps);
    if (op->cfg.pproj) {
        f(&op->prX, (int64_t)PROJ_L * m->lps);
        f(&op->prB, (int64_t)PROJ_L * m->lps);
        f(&op->d_pc, 4 * PROJ_L + PROJ_L * NB);
    }
    f(&op->d_s, 4 * S_N);
    f(&op->d_part, 3 * m->E + 16);
    f(&op->d_cgpart, 3 * NB);
}

int64_t lane_stride(nlg_linop *op) {
    int64_t off = 0;
    lane_buffers(op, [&](double **, int64_t len) { off += round_up(len, kAlign); });
    return off;
}

// point the lane-0 work buffers at the slab (null without one); the rotating buffers return to their canonical places
void lane_bind(nlg_linop *op) {
    int64_t off = 0;
    lane_buffers(op, [&](double **p, int64_t len) {
        *p = op->slab ? op->slab + off : nullptr;
        off += round_up(len, kAlign);
    });
}

// lane v's copy of a work buffer of the list in lane_buffers, from lane 0's pointer
inline double *at_lane(const nlg_linop *op, double *p, int v) { return p + (int64_t)v * op->slab_ld; }
inline F3 at_lane3(const nlg_linop *op, double *const *a, int v) {
    F3 r = {{a[0], a[1], a[2]}};
    for (double *&q : r.p)
        if (q) q = at_lane(op, q, v);
    return r;
}

// rotate three levels (of every lane, by the lane-0 pointers): the oldest becomes the newest
template <typename T>
void rotate3(T (&levels)[3]) {
    std::swap(levels[2], levels[1]);
    std::swap(levels[1], levels[0]);
}

// make room for `cap` lanes (the work buffers hold no state between two matvecs, so growing = a new allocation).  A grow that
// fails leaves no slab and null work-buffer pointers; the next call allocates again at the size it needs.
int slab_ensure(nlg_linop *op, int cap) {
    if (op->slab && op->slab_cap >= cap) return 0;
    nlg_ctx *ctx = op->mesh->ctx;
    NLG_HIP(hipStreamSynchronize(ctx->stream));
    if (op->slab) NLG_HIP(hipFree(op->slab));   // (first: the old and the new slab need not exist together)
    op->slab = nullptr;
    op->slab_cap = 0;
    lane_bind(op);
    // the direction rings (deferred solution update) are bandwidth bought with memory: where the slab does not fit with them -- a block of
    // lanes next to a Krylov basis that fills the card -- they shrink and finally go (k_cg_update then updates x every iteration again)
    int64_t ld = 0;
    double *nslab = nullptr;
    for (;;) {
        ld = lane_stride(op);
        const bool rings = op->ph > 0 || op->php > 0;
        if (hipMalloc(&nslab, sizeof(double) * (size_t)(ld * cap)) == hipSuccess) {
            size_t free_b = 0, total_b = 0;
            // with rings, a tenth of the card must stay free for what is allocated later (lane scratch of the pressure operator and of the
            // preconditioner, solver work space): the rings are the one thing here that is optional
            if (!rings || hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= total_b / 10) break;
            (void)hipFree(nslab);
        } else {
            (void)hipGetLastError();
            NLG_CHECK(rings, "exptA: out of device memory for the work buffers of %d lane(s) (%.1f GB)", cap, 8e-9 * (double)(ld * cap));
        }
        nslab = nullptr;
        if (op->php > 0)
            op->php = 0;
        else if (op->ph > 3)
            op->ph = std::max(3, op->ph / 2);
        else
            op->ph = 0;
    }
    NLG_HIP(hipMemsetAsync(nslab, 0, sizeof(double) * (size_t)(ld * cap), ctx->stream));
    op->slab = nslab;
    op->slab_ld = ld;
    op->slab_cap = cap;
    lane_bind(op);
    return 0;
}

template <typename K, typename... A>
void launch_nf(int nf, K k1, K k2, K k3, dim3 g, hipStream_t s, A... a) {
    if (nf == 1)
        NLG_LAUNCH(k1, g, dim3(NT), 0, s, a...);
    else if (nf == 2)
        NLG_LAUNCH(k2, g, dim3(NT), 0, s, a...);
    else
        NLG_LAUNCH(k3, g, dim3(NT), 0, s, a...);
}

F3 f3(double *const *a, int nf) {
    F3 r = {{a[0], nf > 1 ? a[1] : nullptr, nf > 2 ? a[2] : nullptr}};
    return r;
}
CF3 cf3(double *const *a, int nf) {
    CF3 r = {{a[0], nf > 1 ? a[1] : nullptr, nf > 2 ? a[2] : nullptr}};
    return r;
}
inline dim3 lgrid(int g, int nl) { return dim3((unsigned)g, (unsigned)nl); }

// One PCG problem for nl lanes in lockstep: every pointer is lane 0's, lane v's copy sits v * ld doubles behind it (the lanes
// share a slab); tolerances, iteration limits and the operator are the same for all lanes, alpha / beta / residual norms / the
// convergence flag are per lane (device scalars), so each lane performs exactly the iteration it would perform on its own.
struct CGProblem {
    int nf;
    int64_t n;           // entries per field
    double *const *x, *const *r, *const *z, *const *p, *const *w;
    double *const *pc;
    const unsigned char *pc_mb = nullptr;   // non-null: pc[0] = 1 / diag for every component, bit c of byte i = mask of component c at point i
    const double *ipw, *nw;
    double tol2;         // squared tolerance on sum r^2 nw
    int use_tol, maxit;
    double *s;           // device scalars
    int chunk;           // iterations launched before the host first looks at the done flags (the prediction)
    int chunk_next = 2;  // ... and per look afterwards
    double inv_n;        // 1/n for the mean-free projected solve, 0 = no projection
    int nl = 1;          // lanes
    int64_t ld = 0;      // lane stride
    // non-pointwise M^-1 (nf = 1): writes the element-wise part to z and returns the coarse part per element in *xc
    std::function<int(const double *flag, const double *r, double *z, const double **xc)> precond;
    int npe = 1;         // points per element (for the per-element coarse part)
    // first-stage sums produced by the operator / preconditioner kernels themselves (null = separate kernels)
    const double *pw_part = nullptr;   // [2][pw_n]: sum p.w , sum w   (written by `apply`)
    int pw_n = 0;
    bool pw_sum = true;                // false: the sum of w is not provided (and not needed: inv_n == 0)
    bool fused_pupdate = false;        // `apply` itself performs p <- z + beta p (gated by the done flag) before w = A p
    bool z_free = false;               // ... and forms z = pc r itself, from r and pc / pc_mb: k_cg_init and k_cg_update do not store z
    const double *rz_part = nullptr;   // [2][rz_n]: sum r.z , sum z   (written by `precond`)
    int rz_n = 0;
    const double *rr_part = nullptr;   // [rr_n]: sum r^2 nw, written by `precond`, which then also performs the update
    int rr_n = 0;                      // x += alpha p, r -= alpha (w - wmean) of the iteration (no k_cg_update launch)
    // single-reduction variant (pointwise preconditioner only): `sd` holds s = A p by recurrence, `apply_plain` computes w = A z (the
    // preconditioned residual itself, no direction update inside) and its first-stage sums (z, w) into pw_part
    double *const *sd = nullptr;
    std::function<int()> apply_plain;
    // deferred solution update (k_x_flush / k_add_hist): `apply` stores direction i into slot i mod ph of the direction ring `hist`;
    // x is then NOT complete when run_pcg returns -- its consumer assembles it (adv_b)
    PHist hist = {{nullptr, nullptr, nullptr}, 0, 0};
};

// Device-scalar PCG for P.nl lanes.  `apply` computes w = A p for ALL lanes (stream-ordered, gated by each lane's s[S_DONE]).
// Every kernel of the iteration is ONE launch with gridDim.y = lanes; several ranks: ONE all-reduce per reduction carries the
// sums of all lanes.  iters_out[v]: iterations of lane v.
template <typename Apply>
int run_pcg(nlg_linop *op, const CGProblem &P, Apply apply, int *iters_out) {
    nlg_ctx *ctx = op->mesh->ctx;
    hipStream_t st = ctx->stream;
    const int nf = P.nf, nl = P.nl;
    const int64_t ld = P.ld;
    const int g = red_grid(P.n);
    double *partial = op->d_cgpart;
    double *s = P.s;
    F3 x = f3(P.x, nf), r = f3(P.r, nf), z = f3(P.z, nf), p = f3(P.p, nf);
    CF3 pc = cf3(P.pc, nf), cp = cf3(P.p, nf), cw = cf3(P.w, nf), cz = cf3(P.z, nf);
    CF3 cr = cf3(P.r, nf);
    const Red rd_std = {{partial, partial + NB, partial + 2 * NB}, {g, g, g}};
    auto reduce_post = [&](const Red &rd, int nsums, int gate, int mode) -> int {
        if (!ctx->distributed()) {
            ++g_collectives;   // (the all-reduce a partitioned run issues here; counted on one rank too, nlg_counters)
            NLG_LAUNCH(k_cg_final_post, lgrid(1, nl), dim3(NTF), 0, st, s, rd, nsums, gate, mode, P.tol2, P.use_tol, P.maxit,
                       P.inv_n, 1, ld, (double *)nullptr);
        } else {
            NLG_LAUNCH(k_cg_final_post, lgrid(1, nl), dim3(NTF), 0, st, s, rd, nsums, gate, mode, P.tol2, P.use_tol, P.maxit,
                       P.inv_n, 0, ld, op->d_red);
            NLG_TRY(allreduce_sum(ctx, op->d_red, 3 * nl));
            NLG_LAUNCH(k_cg_post, lgrid(1, nl), dim3(1), 0, st, s, mode, P.tol2, P.use_tol, P.maxit, P.inv_n, ld, (const double *)op->d_red, nsums);
        }
        return 0;
    };
    launch_nf(nf, k_cg_init<1>, k_cg_init<2>, k_cg_init<3>, lgrid(g, nl), st, P.n, x, r, z, pc, P.ipw, P.nw, partial, ld, P.pc_mb, (int)(P.hist.ph > 0), (int)!P.z_free);
    if (P.sd && P.apply_plain && !P.precond && P.pw_part) {
        // ---- single-reduction PCG (Chronopoulos-Gear): ONE reduction per iteration carries (w, u), (r, u) and |r|^2; several ranks: one
        // all-reduce instead of two.  u = M^-1 r lives in z, p and s = A p are recurrences.  Same iterates as the loop below in exact
        // arithmetic; the convergence test lags one operator application (cg_post_logic mode 4).
        NLG_TRY(reduce_post(rd_std, 3, 0, 0));
        NLG_LAUNCH(k_cg_post, lgrid(1, nl), dim3(1), 0, st, s, 3, P.tol2, P.use_tol, P.maxit, P.inv_n, ld, (const double *)nullptr, 0);
        const Red rd_sr = {{P.pw_part, partial, partial + NB}, {P.pw_n, g, g}};
        F3 sdv = f3(P.sd, nf);
        auto body_sr = [&]() -> int {
            NLG_TRY(P.apply_plain());
            NLG_TRY(reduce_post(rd_sr, 3, 1, 4));
            ProfScope pu(ctx, P_CGUPDATE);
            launch_nf(nf, k_cg_update_sr<1>, k_cg_update_sr<2>, k_cg_update_sr<3>, lgrid(g, nl), st, (const double *)s, P.n, x, r, z, p, sdv, cw,
                      pc, P.ipw, P.nw, partial, ld);
            return 0;
        };
        int launched = 0;
        while (true) {
            int todo = launched == 0 ? P.chunk + 1 : P.chunk_next;   // (+ 1: the iteration that notices the convergence)
            if (launched + todo > P.maxit + 1) todo = P.maxit + 1 - launched;
            for (int it = 0; it < todo; ++it) NLG_TRY(body_sr());
            launched += todo;
            NLG_HIP(hipGetLastError());
            for (int v = 0; v < nl; ++v)
                NLG_HIP(hipMemcpyAsync(op->h_s + (size_t)v * S_N, s + (int64_t)v * ld, sizeof(double) * S_N, hipMemcpyDeviceToHost, st));
            NLG_HIP(hipStreamSynchronize(st));
            bool all_done = true;
            for (int v = 0; v < nl; ++v) all_done = all_done && op->h_s[(size_t)v * S_N + S_DONE] != 0.0;
            if (all_done || launched >= P.maxit + 1) break;
        }
        for (int v = 0; v < nl; ++v) {
            const double *h = op->h_s + (size_t)v * S_N;
            if (!std::isfinite(h[S_RN2])) {
                set_error("PCG (single reduction) diverged (residual is not finite) after %d iterations (lane %d of %d)", (int)h[S_ITERS], v, nl);
                return 1;
            }
            iters_out[v] = (int)h[S_ITERS];
        }
        return 0;
    }
    const double *xc = nullptr;
    Red rd_rz = rd_std;
    if (P.precond) {
        NLG_TRY(P.precond(nullptr, P.r[0], P.z[0], &xc));
        if (P.rz_part) {
            rd_rz.p[0] = P.rz_part;
            rd_rz.n[0] = P.rz_n;
            rd_rz.p[2] = P.rz_part + P.rz_n;
            rd_rz.n[2] = P.rz_n;
        } else {
            launch_nf(nf, k_cg_rz<1>, k_cg_rz<2>, k_cg_rz<3>, lgrid(g, nl), st, (const double *)s, 0, P.n, cr, cz, P.ipw, xc, P.npe, partial, ld);
        }
    }
    Red rd_rz_loop = rd_rz;   // inside the loop the r^2 sums may come from the preconditioner's first kernel
    if (P.rr_part) {
        rd_rz_loop.p[1] = P.rr_part;
        rd_rz_loop.n[1] = P.rr_n;
    }
    Red rd_pw = rd_std;
    if (P.pw_part) {
        rd_pw.p[0] = P.pw_part;
        rd_pw.n[0] = P.pw_n;
        rd_pw.p[1] = P.pw_part + P.pw_n;
        rd_pw.n[1] = P.pw_sum ? P.pw_n : 0;
    }
    NLG_TRY(reduce_post(rd_rz, 3, 0, 0));
    if (!P.fused_pupdate)
        launch_nf(nf, k_cg_pupdate<1>, k_cg_pupdate<2>, k_cg_pupdate<3>, lgrid(g, nl), st, (const double *)s, P.n, p, cz, xc, P.npe, ld);   // p = z - zmean
    NLG_LAUNCH(k_cg_post, lgrid(1, nl), dim3(1), 0, st, s, 3, P.tol2, P.use_tol, P.maxit, P.inv_n, ld, (const double *)nullptr, 0);
    int nbody = 0;   // iterations launched so far = the iteration index the device is at while it has not converged
    auto body = [&]() -> int {
        NLG_TRY(apply(s));
        const bool prof_cg = prof_want(ctx, P_CGVEC);
        if (prof_cg) prof_begin(ctx, P_CGVEC);
        if (!P.pw_part)
            launch_nf(nf, k_cg_pw<1>, k_cg_pw<2>, k_cg_pw<3>, lgrid(g, nl), st, (const double *)s, P.n, cp, cw, P.ipw, partial, ld);
        NLG_TRY(reduce_post(rd_pw, 2, 1, 1));
        if (!P.rr_part) {
            ProfScope pu(ctx, P_CGUPDATE);   // the largest single kernel of a step by time: its own class inside cg_vec (bench.py quotes its roofline)
            launch_nf(nf, k_cg_update<1>, k_cg_update<2>, k_cg_update<3>, lgrid(g, nl), st, (const double *)s, P.n, x, r, z, cp, cw,
                      pc, P.ipw, P.nw, partial, ld, (int)(P.hist.ph > 0), P.pc_mb, (int)!P.z_free);
        }
        ++nbody;
        if (prof_cg) prof_end(ctx, P_CGVEC);
        if (P.precond) {
            NLG_TRY(P.precond(s + S_DONE, P.r[0], P.z[0], &xc));
            if (!P.rz_part)
                launch_nf(nf, k_cg_rz<1>, k_cg_rz<2>, k_cg_rz<3>, lgrid(g, nl), st, (const double *)s, 1, P.n, cr, cz, P.ipw, xc, P.npe, partial, ld);
        }
        if (P.hist.ph > 0 && nbody % P.hist.ph == 0)   // the direction ring is full: its PH terms go into x before slot 0 is overwritten
            launch_nf(nf, k_x_flush<1>, k_x_flush<2>, k_x_flush<3>, lgrid(grid_for(P.n), nl), st, (const double *)s, P.n, x, P.hist, nbody - 1, ld);
        NLG_TRY(reduce_post(rd_rz_loop, 3, 1, 2));
        if (!P.fused_pupdate)
            launch_nf(nf, k_cg_pupdate<1>, k_cg_pupdate<2>, k_cg_pupdate<3>, lgrid(g, nl), st, (const double *)s, P.n, p, cz, xc, P.npe, ld);
        return 0;
    };
    int launched = 0;
    while (true) {
        int todo = launched == 0 ? P.chunk : P.chunk_next;
        if (launched + todo > P.maxit) todo = P.maxit - launched;
        for (int it = 0; it < todo; ++it) NLG_TRY(body());
        launched += todo;
        NLG_HIP(hipGetLastError());
        for (int v = 0; v < nl; ++v)
            NLG_HIP(hipMemcpyAsync(op->h_s + (size_t)v * S_N, s + (int64_t)v * ld, sizeof(double) * S_N, hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
        bool all_done = true;
        for (int v = 0; v < nl; ++v) all_done = all_done && op->h_s[(size_t)v * S_N + S_DONE] != 0.0;
        if (all_done || launched >= P.maxit) break;
    }
    for (int v = 0; v < nl; ++v) {
        const double *h = op->h_s + (size_t)v * S_N;
        if (!std::isfinite(h[S_RN2])) {
            set_error("PCG diverged (residual is not finite) after %d iterations (lane %d of %d)", (int)h[S_ITERS], v, nl);
            return 1;
        }
        iters_out[v] = (int)h[S_ITERS];
    }
    return 0;
}

// The lanes 0 .. nl - 1 of a time step in the operator's slab; nl = 1 is the single-vector path.  Every phase launches once for
// all lanes and keeps the iteration predictions per lane.  The mode of the run travels with them, by value: the operator keeps none.
struct Lanes {
    nlg_linop *op;
    int nl;
    int lb = -1;         // coupled mode: the lane that carries the base flow (nl - 1); -1: the base flow is frozen
    int adjoint = 0;     // the adjoint equations (never together with nonlinear)
    int nonlinear = 0;   // 1: full Navier-Stokes step, N(u) = (u.grad)u = half of the linearised term about U = u; one lane
    // time-harmonic body force Re[(f_re[v] + i f_im[v]) exp(i sign omega t)] of the resolvent integrations, one per lane (f_re[0]
    // null = an unforced run; a null f_im[v] = a real forcing); omega and sign are shared
    const nlg_vec *f_re[kMaxLanes] = {}, *f_im[kMaxLanes] = {};
    double omega = 0.0, sign = 1.0;
    int64_t ld() const { return nl > 1 ? op->slab_ld : 0; }   // the lane stride the kernels receive
};

// One Helmholtz solve w = QQ^T (h1 A + h2 B) p by Jacobi-PCG -- the velocity's (helm_problem) and the temperature's (heat_problem) -- in
// pieces: problem set-up, one operator application, the run; the iteration bookkeeping stays with the two callers.  The solve carries
// all that an application needs: the operator is not consulted again.
struct HelmSolve {
    CGProblem P;
    double *x[1], *r[1], *z[1], *p[1], *w[1], *pc[1], *sd[1];   // the pointer arrays of a one-field solve (the velocity's are the operator's)
    bool xp = false;      // every vector of the iteration in the x-planes-first layout
    double h1 = 0.0, h2 = 0.0;
    double *pw_part = nullptr;
    double *ring = nullptr;   // direction ring (deferred solution update): slot 0 of field 0; field q is q * ring_field doubles behind
    int64_t ring_field = 0;
    mutable int it = 0;   // operator applications so far (= the slot of the direction ring the next one writes, modulo its depth)
};

// the settings common to the two solves; the vectors, the preconditioner and the prediction are the caller's
void helm_common(const Lanes &L, int nf, double h1, double h2, HelmSolve &H) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    const auto &c = op->cfg;
    CGProblem &P = H.P;
    H.h1 = h1;
    H.h2 = h2;
    P.nf = nf;
    P.n = m->lvn;
    P.tol2 = c.vtol * c.vtol;
    P.use_tol = c.fixed_iters_v > 0 ? 0 : 1;
    P.maxit = c.fixed_iters_v > 0 ? c.fixed_iters_v : c.maxit_v;
    P.s = op->d_s;
    P.inv_n = 0.0;
    P.nl = L.nl;
    P.ld = L.ld();
    // The Dirichlet mask is not applied to w: p is masked (z = pc r with pc = mask/diag), so (p, w) does not see the masked
    // entries, and k_cg_update zeroes the residual where pc == 0.
    // (p, w) = sum over the local dofs of p . w_local (p is continuous), summed inside the operator kernel, which also
    // performs p <- z + beta p while it loads p.
    H.pw_part = op->d_part;
    P.pw_part = H.pw_part;
    P.pw_n = sem_axhelm_blocks(m, P.nf);
    P.pw_sum = false;
    P.fused_pupdate = true;
    // deferred solution update: one ring serves both solves, the scalar's directions one field wide (the two solves never overlap:
    // each ring is consumed right after its solve).  The single-reduction variant keeps p itself: it runs without a ring (ph = 0)
    if (op->ph > 0) {
        H.ring = op->phist;
        H.ring_field = m->lvs;
        for (int q = 0; q < P.nf; ++q) P.hist.p0[q] = H.ring + q * H.ring_field;
        P.hist.stride = P.nf * H.ring_field;
        P.hist.ph = op->ph;
    }
}

int helm_problem(const Lanes &L, int order, double h2, HelmSolve &H) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    const int dim = m->dim;
    const auto &c = op->cfg;
    CGProblem &P = H.P;
    // x-planes-first layout for every vector of the iteration: the right-hand side is permuted on the way in (into gp,
    // free at this point), the solution on the way out (into rhs, which the caller reads as the increment)
    const bool xp = op->use_xp > 0;
    H.xp = xp;
    const bool born_xp = xp && op->rhs_in_xp;   // adv_a wrote the right-hand side masked and slab-permuted already
    op->rhs_in_xp = false;
    if (xp && !born_xp) NLG_TRY(sem_to_xp(m, op->rhs, op->gp, dim, L.nl, L.ld(), m->d_mask));   // ... and masked on the way
    helm_common(L, dim, 1.0 / c.re, h2, H);
    P.x = op->x;
    P.r = (xp && !born_xp) ? op->gp : op->rhs;
    P.z = op->z;
    P.p = op->pv;
    P.w = op->w;
    P.pc = xp ? op->pcv_xp[order] : op->pcv[order];
    if (op->maskb_v) {   // 1 / diag and the mask bytes instead of the three masked arrays (same values)
        P.pc = op->pci_l[order];
        P.pc_mb = op->maskb_v;
    }
    P.ipw = xp ? m->d_vmult_xp : m->d_vmult;
    P.nw = xp ? op->nwv_xp : op->nwv;
    if (op->use_sr) P.sd = op->cgs;
    // the iteration count barely changes from one time step to the next: launch exactly the previous count, then look at
    // the flags every second iteration; launches issued after convergence are gated on the device but still cost a launch
    P.chunk = 2;
    for (int v = 0; v < L.nl; ++v) P.chunk = std::max(P.chunk, std::min(op->pred[v].v.predict(op->istep), 64));
    // z = pc r is a pointwise product of what the operator kernel can read itself: it is not stored (NLG_PCG_STORE_Z=1 keeps it)
    P.z_free = op->z_free;
    return 0;
}

// The temperature's solve at BDF order k: one field, natural layout, z stored, the masked Jacobi array pct[k]; the right-hand side is in
// trhs, the increment goes to tx.  The compact preconditioner (one 1 / diag and a mask byte in place of three masked arrays: nothing to
// save with one field), z-free (which builds on it) and the slab-permuted layout (pct and tmask exist in the natural one only) are the
// velocity's alone.
void heat_problem(const Lanes &L, int k, double h1, double h2, HelmSolve &H) {
    nlg_linop *op = L.op;
    CGProblem &P = H.P;
    helm_common(L, 1, h1, h2, H);
    H.x[0] = op->tx, H.r[0] = op->trhs, H.z[0] = op->tz, H.p[0] = op->tpv, H.w[0] = op->tw, H.pc[0] = op->pct[k], H.sd[0] = op->tcgs;
    P.x = H.x, P.r = H.r, P.z = H.z, P.p = H.p, P.w = H.w, P.pc = H.pc;
    if (op->use_sr) P.sd = H.sd;
    P.ipw = op->mesh->d_vmult;
    P.nw = op->nwv;
    P.chunk = 2;
    for (int v = 0; v < L.nl; ++v) P.chunk = std::max(P.chunk, std::min(op->pred[v].last_titers, 64));
}

int helm_apply(const Lanes &L, const HelmSolve &H) {
    nlg_mesh *m = L.op->mesh;
    const CGProblem &P = H.P;
    // z-free: the kernel reads the residual where it read z, and 1 / diag and the mask bytes of the solve (P.pc, P.pc_mb)
    double *const *zf = P.z_free ? P.r : P.z;
    const double *pcinv = P.z_free ? P.pc[0] : nullptr;
    const unsigned char *pcmb = P.z_free ? P.pc_mb : nullptr;
    if (P.hist.ph > 0) {
        // direction ring: read direction it - 1, store direction it one slot further (the first application multiplies slot ph - 1 by
        // beta = 0: the ring is zeroed with the slab and holds finite values ever after)
        const int ph = P.hist.ph, so = H.it % ph, si = (H.it + ph - 1) % ph;
        ++H.it;
        double *pin[3] = {nullptr, nullptr, nullptr};
        for (int q = 0; q < P.nf; ++q) pin[q] = H.ring + si * P.hist.stride + q * H.ring_field;
        NLG_TRY(sem_axhelm(m, pin, P.w, P.nf, H.h1, H.h2, H.pw_part, zf, P.s + S_BETA, P.s + S_DONE, H.xp, P.nl, P.ld, (so - si) * P.hist.stride, pcinv, pcmb));
    } else {
        NLG_TRY(sem_axhelm(m, P.p, P.w, P.nf, H.h1, H.h2, H.pw_part, zf, P.s + S_BETA, P.s + S_DONE, H.xp, P.nl, P.ld, 0, pcinv, pcmb));
    }
    NLG_TRY(sem_gs(m, P.w, P.nf, P.s + S_DONE, H.xp ? LAYOUT_XP : LAYOUT_NAT, P.nl, P.ld, P.ld));
    return 0;
}

// the PCG of a filled solve; iters[v]: the iterations of lane v
int helm_run(const Lanes &L, HelmSolve &H, int *iters) {
    nlg_mesh *m = L.op->mesh;
    if (H.P.sd) {   // single-reduction variant
        H.P.apply_plain = [&H, m]() -> int {   // w = QQ^T (h1 A + h2 B) z and the first-stage sums of (z, w): no direction update inside
            const CGProblem &P = H.P;
            NLG_TRY(sem_axhelm(m, P.z, P.w, P.nf, H.h1, H.h2, H.pw_part, nullptr, nullptr, P.s + S_DONE, H.xp, P.nl, P.ld));
            return sem_gs(m, P.w, P.nf, P.s + S_DONE, H.xp ? LAYOUT_XP : LAYOUT_NAT, P.nl, P.ld, P.ld);
        };
    }
    auto apply = [&](double *) -> int { return helm_apply(L, H); };
    return run_pcg(L.op, H.P, apply, iters);
}

int helm_solve(const Lanes &L, int order, double h2) {
    nlg_linop *op = L.op;
    HelmSolve H;
    NLG_TRY(helm_problem(L, order, h2, H));
    int iters[kMaxLanes] = {};
    NLG_TRY(helm_run(L, H, iters));
    // (slab-permuted solve: the increment stays in that layout, adv_b reads it through the slot table)
    for (int v = 0; v < L.nl; ++v) {
        op->st_viters += iters[v];
        op->lane_viters[v] += iters[v];
        op->pred[v].v.record(op->istep, iters[v]);
    }
    return 0;
}

// One scalar (temperature) step of the Boussinesq coupling, see oracle/lns.py advance (ifheat branch):
//   rhocp (b0 theta^{n+1} - sum bd_j theta^{n-j}) / dt = -rhocp EXT[(U.grad) theta + (u.grad) Theta] + conductivity lap theta^{n+1}
// in residual form; the solve is an instance of the velocity's Helmholtz PCG (HelmSolve, heat_problem); the new level ends in tbuf[0].
int heat_step(const Lanes &L, int k, double b0) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const auto &c = op->cfg;
    const int nl = L.nl;
    const int64_t ld = L.ld();
    const double dt = op->dt, rc = c.rhocp;
    // explicit term into the oldest buffer, then rotate.  The transport term is one launch per lane (base-flow data shared); everything
    // after it -- right-hand side, operator, gather-scatter, the whole PCG -- is ONE launch for all lanes (gridDim.y), as in the velocity solve
    const int adj = L.adjoint;
    NLG_TRY(sem_conv_scalar_apply(m, op->Ur, op->GT, op->ubuf[0], op->tbuf[0], op->ftbuf[2], adj, nl, ld));
    if (adj) {
        // adjoint temperature equation: rhocp theta+_t = rhocp (U.grad) theta+ + conductivity lap theta+ + rhocp b . u+
        // (stored term N_t = -conv(U, theta+) - bm1 b . u+ ; oracle/lns.py advance, adjoint branch)
        for (int v = 0; v < nl; ++v)
            for (int i = 0; i < m->dim; ++i)
                if (c.buoy[i] != 0.0)
                    NLG_LAUNCH(k_mul3_acc, dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, at_lane(op, op->ftbuf[2], v), (const double *)m->d_bm1,
                               (const double *)at_lane(op, op->ubuf[0][i], v), -c.buoy[i]);
    }
    rotate3(op->ftbuf);
    Hist h;
    h.k = k;
    for (int j = 0; j < 3; ++j) {
        h.ab[j] = -(L.nonlinear ? 0.5 : 1.0) * rc * EXT_C[k][j];   // nonlinear: (u.grad)theta = 1/2 [(U.grad)theta + (u.grad)Theta] at U = u, Theta = theta
        h.bd[j] = BDF_C[k][j];
        for (int q = 0; q < 3; ++q) {
            h.f[j][q] = q == 0 ? op->ftbuf[j] : nullptr;
            h.u[j][q] = q == 0 ? op->tbuf[j] : nullptr;
        }
    }
    F3 rhs = {{op->trhs, nullptr, nullptr}};
    NLG_LAUNCH(k_rhs<1>, lgrid(grid_for(m->lvn), nl), dim3(NT), 0, st, m->lvn, h, (const double *)m->d_bm1, rc / dt, rhs, ld);
    const double h1 = c.conductivity, h2 = rc * b0 / dt;
    double *tin[1] = {op->tbuf[0]}, *tw[1] = {op->tw}, *trhs[1] = {op->trhs};
    NLG_TRY(sem_axhelm(m, tin, tw, 1, h1, h2, nullptr, nullptr, nullptr, nullptr, false, nl, ld));
    {
        CF3 a = {{op->trhs, nullptr, nullptr}}, b = {{op->tw, nullptr, nullptr}}, none = {{nullptr, nullptr, nullptr}};
        NLG_LAUNCH(k_lin3<1>, lgrid(grid_for(m->lvn), nl), dim3(NT), 0, st, m->lvn, rhs, a, b, -1.0, none, 0.0, ld);
    }
    NLG_TRY(sem_gs(m, trhs, 1, nullptr, LAYOUT_NAT, nl, ld, 0));
    {
        CF3 mk = {{m->d_tmask, nullptr, nullptr}};
        NLG_LAUNCH(k_colmul_gated<1>, lgrid(grid_for(m->lvn), nl), dim3(NT), 0, st, (const double *)nullptr, rhs, mk, m->lvn, ld);
    }
    HelmSolve H;
    heat_problem(L, k, h1, h2, H);
    int iters[kMaxLanes] = {};
    NLG_TRY(helm_run(L, H, iters));
    for (int v = 0; v < nl; ++v) {
        op->st_titers += iters[v];
        op->pred[v].last_titers = iters[v];
    }
    // theta^{n+1} = theta^n + x into the oldest level, then rotate: new -> current
    {
        F3 y = {{op->tbuf[2], nullptr, nullptr}};
        CF3 a = {{op->tbuf[0], nullptr, nullptr}}, b = {{op->tx, nullptr, nullptr}}, none = {{nullptr, nullptr, nullptr}};
        if (H.P.hist.ph > 0)   // the directions are still in the ring (deferred solution update)
            NLG_LAUNCH(k_add_hist<1>, lgrid(grid_for(m->lvn), nl), dim3(NT), 0, st, (const double *)op->d_s, m->lvn, 1, (const int *)nullptr, y, a, b, H.P.hist, ld);
        else
            NLG_LAUNCH(k_lin3<1>, lgrid(grid_for(m->lvn), nl), dim3(NT), 0, st, m->lvn, y, a, b, 1.0, none, 0.0, ld);
        rotate3(op->tbuf);
    }
    NLG_HIP(hipGetLastError());
    return 0;
}

// The pressure solve in three pieces (see HelmSolve): set-up incl. the residual projection onto the previous increments,
// one application of E, and the update of the projection space afterwards.
struct PresSolve {
    CGProblem P;
    double *x[1], *r[1], *z[1], *p[1], *w[1], *pc[1], *nopc[1];
    double *pw_part = nullptr;
    bool proj = false;
    int nold = 0;
    mutable int it = 0;   // operator applications so far (slot of the direction ring, modulo its depth)
};

int pres_problem(const Lanes &L, double scale, PresSolve &Q) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    const auto &c = op->cfg;
    const int nl = L.nl;
    const int64_t ld = L.ld();
    Q.x[0] = op->pr_x, Q.r[0] = op->pr_r, Q.z[0] = op->pr_z, Q.p[0] = op->pr_p, Q.w[0] = op->pr_w, Q.pc[0] = op->pce, Q.nopc[0] = nullptr;
    CGProblem &P = Q.P;
    P.nf = 1;
    P.n = m->lpn;
    P.x = Q.x;
    P.r = Q.r;
    P.z = Q.z;
    P.p = Q.p;
    P.w = Q.w;
    P.pc = Q.pc;
    P.ipw = nullptr;
    P.nw = op->nwp;
    P.tol2 = (c.ptol / scale) * (c.ptol / scale);
    P.use_tol = c.fixed_iters_p > 0 ? 0 : 1;
    P.maxit = c.fixed_iters_p > 0 ? c.fixed_iters_p : c.maxit_p;
    P.s = op->d_s + S_N;
    P.inv_n = m->has_outflow ? 0.0 : 1.0 / (double)m->lpn_global;
    P.nl = nl;
    P.ld = ld;
    if (c.pprecond == 0 || c.pprecond == 2) {   // two-level Schwarz (pprec.hip): 0 = with overlap where available, 2 = without; 1 = Jacobi on diag(E), as in the oracle
        const bool overlap = c.pprecond == 0 && m->pprec.overlap;
        P.pc = Q.nopc;
        P.npe = m->np2;
        // r.z / z sums from the last kernel of the preconditioner
        double *rzp = op->d_part + 2 * m->E;
        // the PCG update of an iteration rides in the preconditioner's first kernel (which reads r anyway)
        nlg_pcg_upd upd;
        upd.alpha = op->d_s + S_N + S_ALPHA;
        upd.wmean = op->d_s + S_N + S_WMEAN;
        upd.x = op->pr_x;
        upd.p = op->pr_p;
        {
            // deferred solution update (as in the velocity solve, k_cg_update): the gradient kernel's fused direction update stores direction
            // i into slot i mod php of a ring, the update kernel of the preconditioner streams neither x nor p, pres_solve assembles x
            if (op->php > 0 && sem_opgradt_fuses_pupdate(m)) {
                upd.x = nullptr;
                upd.p = nullptr;
                P.hist.p0[0] = op->prh;
                P.hist.stride = m->lps;
                P.hist.ph = op->php;
            }
        }
        upd.w = op->pr_w;
        upd.nw = op->nwp;
        upd.rr_part = op->d_part + 2 * m->E + 2 * ((m->E + 3) / 4);
        P.rr_part = upd.rr_part;
        P.rr_n = (int)((m->E + 3) / 4);
        P.precond = [m, rzp, overlap, upd, nl, ld](const double *flag, const double *rr, double *zz, const double **xc) -> int {
            // one stream: a fork/join through events costs more than it hides (measured: 98 vs 84 us per apply)
            nlg_ctx *c = m->ctx;
            ProfScope ps(c, P_PPREC);
            NLG_TRY(pprec_apply(m, c->stream, flag, rr, zz, rzp, overlap, true, flag ? &upd : nullptr, nl, ld));   // flag == null: the initial residual
            *xc = nullptr;
            return 0;
        };
    }
    P.chunk = 2;
    for (int v = 0; v < nl; ++v) P.chunk = std::max(P.chunk, std::min(op->pred[v].p.predict(op->istep), 96));
    // fused first-stage sums (rank-local; the all-reduce follows the second stage): p.w and sum w from the divergence kernel,
    // r.z and sum z from the preconditioner's last kernel
    Q.pw_part = op->d_part;
    P.pw_part = Q.pw_part;
    P.pw_n = sem_opdiv_blocks(m);
    P.fused_pupdate = sem_opgradt_fuses_pupdate(m);
    if (P.precond) {
        P.rz_part = op->d_part + 2 * m->E;
        P.rz_n = (int)((m->E + 3) / 4);
    }
    // ---- residual projection (c.pproj): start from the A-orthogonal projection of the solution onto the span of the
    // previous increments of this matvec; the PCG then solves for the remainder
    hipStream_t st = m->ctx->stream;
    // (not in the fixed-iteration parity mode: there the iteration is the oracle's, run on the full right-hand side)
    Q.proj = c.pproj != 0 && op->prX != nullptr && c.fixed_iters_p <= 0;
    Q.nold = op->nproj;
    if (Q.proj && Q.nold > 0) {
        double *alpha = op->d_pc, *ppart = op->d_pc + 4 * PROJ_L;
        const int gp = red_grid(m->lpn);
        ProfScope ps(m->ctx, P_VECOPS);
        NLG_LAUNCH(k_proj_dots, lgrid(gp, nl), dim3(NT), 0, st, m->lpn, (const double *)op->prX, m->lps, Q.nold, (const double *)op->pr_r, ppart, ld);
        NLG_LAUNCH(k_proj_reduce, lgrid(1, nl), dim3(NT), 0, st, (const double *)ppart, gp, Q.nold, alpha, ld);
        for (int v = 0; v < nl; ++v) NLG_TRY(allreduce_sum(m->ctx, alpha + v * ld, Q.nold));                       // alpha = X^T b
        NLG_LAUNCH(k_proj_comb, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, op->pr_r, (const double *)op->prB, m->lps,
                   Q.nold, (const double *)alpha, -1.0, ld);               // b <- b - B alpha
    }
    if (Q.proj)   // the right-hand side of the PCG, kept for the update of the projection space: A d = b - r_final
        NLG_HIP(hipMemcpy2DAsync(op->pr_b, sizeof(double) * (size_t)std::max<int64_t>(ld, m->lpn), op->pr_r, sizeof(double) * (size_t)std::max<int64_t>(ld, m->lpn),
                                 sizeof(double) * (size_t)m->lpn, (size_t)nl, hipMemcpyDeviceToDevice, st));
    return 0;
}

// gated: launches past convergence (the host only looks at the flags once per chunk) return at once
int pres_apply(const Lanes &L, const PresSolve &Q) {
    nlg_linop *op = L.op;
    // direction ring (deferred solution update): read direction it - 1, the fused update stores direction it one slot further
    double *p_in = op->pr_p, *p_out = op->pr_p;
    if (Q.P.hist.ph > 0) {
        const int ph = Q.P.hist.ph, so = Q.it % ph, si = (Q.it + ph - 1) % ph;
        ++Q.it;
        p_in = op->prh + (int64_t)si * Q.P.hist.stride;
        p_out = op->prh + (int64_t)so * Q.P.hist.stride;
    }
    // E p for all lanes; with the fused update p <- (z - zmean) + beta p while the gradient kernel loads p
    nlg_pupd u;
    u.z = op->pr_z, u.beta = op->d_s + S_N + S_BETA, u.zmean = op->d_s + S_N + S_ZMEAN, u.p = p_out;
    return sem_cdabdtp(op->mesh, p_in, op->pr_w, Q.pw_part, op->d_s + S_N + S_DONE, Q.P.fused_pupdate ? &u : nullptr, L.nl, L.ld());
}

int pres_finish(const Lanes &L, const PresSolve &Q, const int *iters) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int nl = L.nl;
    const int64_t ld = L.ld();
    for (int v = 0; v < nl; ++v) {
        op->st_piters += iters[v];
        op->lane_piters[v] += iters[v];
        op->pred[v].p.record(op->istep, iters[v]);
    }
    if (Q.proj) {
        double *alpha = op->d_pc, *beta = op->d_pc + PROJ_L, *nrm2 = op->d_pc + 2 * PROJ_L, *ppart = op->d_pc + 4 * PROJ_L;
        const int gp = red_grid(m->lpn);
        const int nold = Q.nold;
        auto dots = [&](const double *y, int nvec, const double *M, double *out) -> int {
            NLG_LAUNCH(k_proj_dots, lgrid(gp, nl), dim3(NT), 0, st, m->lpn, M, m->lps, nvec, y, ppart, ld);
            NLG_LAUNCH(k_proj_reduce, lgrid(1, nl), dim3(NT), 0, st, (const double *)ppart, gp, nvec, out, ld);
            for (int v = 0; v < nl; ++v) NLG_TRY(allreduce_sum(m->ctx, out + v * ld, nvec));
            return 0;
        };
        // new member from the increment d = pr_x: w = A d, A-orthogonalised against the old members, normalised.  A d is not
        // computed by another application of E (three launches, 4 % of a time step): the PCG started from r = b and updated
        // r <- r - alpha A p with x <- x + alpha p, so A d = b - r_final, mean-free like b and r (A = P E P)
        {
            F3 y = {{op->pr_w, nullptr, nullptr}};
            CF3 a = {{op->pr_b, nullptr, nullptr}}, b = {{op->pr_r, nullptr, nullptr}}, none = {{nullptr, nullptr, nullptr}};
            NLG_LAUNCH(k_lin3<1>, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, y, a, b, -1.0, none, 0.0, ld);
        }
        ProfScope ps(m->ctx, P_VECOPS);
        NLG_HIP(hipMemcpy2DAsync(op->pr_z, sizeof(double) * (size_t)std::max<int64_t>(ld, m->lpn), op->pr_x, sizeof(double) * (size_t)std::max<int64_t>(ld, m->lpn),
                                 sizeof(double) * (size_t)m->lpn, (size_t)nl, hipMemcpyDeviceToDevice, st));   // v = d (all lanes)
        if (nold > 0) {
            NLG_TRY(dots(op->pr_w, nold, op->prX, beta));                    // beta = X^T A d
            NLG_LAUNCH(k_proj_comb, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, op->pr_z, (const double *)op->prX, m->lps,
                       nold, (const double *)beta, -1.0, ld);
            NLG_LAUNCH(k_proj_comb, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, op->pr_w, (const double *)op->prB, m->lps,
                       nold, (const double *)beta, -1.0, ld);
            // total solution: x = d + X alpha
            NLG_LAUNCH(k_proj_comb, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, op->pr_x, (const double *)op->prX, m->lps,
                       nold, (const double *)alpha, 1.0, ld);
        }
        NLG_TRY(dots(op->pr_w, 1, op->pr_z, nrm2));                          // v^T A v
        const int slot = nold < PROJ_L ? nold : 0;                           // full: start over with the newest member
        NLG_LAUNCH(k_proj_store, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, (const double *)op->pr_z, (const double *)op->pr_w,
                   (const double *)nrm2, op->prX + (size_t)slot * m->lps, op->prB + (size_t)slot * m->lps, ld);
        op->nproj = nold < PROJ_L ? nold + 1 : 1;
        NLG_HIP(hipGetLastError());
    }
    return 0;
}

int pres_solve(const Lanes &L, double scale) {
    PresSolve Q;
    NLG_TRY(pres_problem(L, scale, Q));
    auto apply = [&](double *) -> int { return pres_apply(L, Q); };
    int iters[kMaxLanes] = {};
    NLG_TRY(run_pcg(L.op, Q.P, apply, iters));
    if (Q.P.hist.ph > 0) {   // x = sum alpha_i p_i, in iteration order (k_add_hist without an addend)
        nlg_linop *op = L.op;
        nlg_mesh *m = op->mesh;
        F3 y = {{op->pr_x, nullptr, nullptr}};
        CF3 none = {{nullptr, nullptr, nullptr}}, x = {{op->pr_x, nullptr, nullptr}};
        NLG_LAUNCH(k_add_hist<1>, lgrid(grid_for(m->lpn), L.nl), dim3(NT), 0, m->ctx->stream, (const double *)Q.P.s, m->lpn, 1, (const int *)nullptr, y, none, x,
                   Q.P.hist, L.ld());
    }
    return pres_finish(L, Q, iters);
}

// ---- OTD modes: the device side of nlg_otd_* ------------------------------------------------------------------------------
// the 2 r^2 sums of k_otd_reduce over the r OTD lanes (Nf = null: the Gram matrix alone), second stage, ONE all-reduce
int otd_sums(const nlg_otd *ot, double *const *gp, double *const *w, double *const *Nf) {
    nlg_linop *op = ot->op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    ProfScope ps(m->ctx, P_VECOPS);
    const int dim = m->dim, r = ot->r, g = red_grid(m->lvn);
    const CF3 u = cf3(op->ubuf[0], dim), none = {{nullptr, nullptr, nullptr}};
    const CF3 a = Nf ? cf3(gp, dim) : none, b = Nf ? cf3(w, dim) : none, c = Nf ? cf3(Nf, dim) : none;
#define OTD_RED(D_, R_)                                                                                                                              \
    if (Nf)                                                                                                                                          \
        NLG_LAUNCH((k_otd_reduce<D_, R_, true>), dim3(g), dim3(NT), 0, st, m->lvn, u, a, b, c, (const double *)m->d_bm1, op->slab_ld, ot->part);    \
    else                                                                                                                                             \
        NLG_LAUNCH((k_otd_reduce<D_, R_, false>), dim3(g), dim3(NT), 0, st, m->lvn, u, a, b, c, (const double *)m->d_bm1, op->slab_ld, ot->part)
#define OTD_RED_D(D_)          \
    if (r == 1) {              \
        OTD_RED(D_, 1);        \
    } else if (r == 2) {       \
        OTD_RED(D_, 2);        \
    } else if (r == 3) {       \
        OTD_RED(D_, 3);        \
    } else {                   \
        OTD_RED(D_, 4);        \
    }
    if (dim == 3) {
        OTD_RED_D(3)
    } else {
        OTD_RED_D(2)
    }
#undef OTD_RED_D
#undef OTD_RED
    NLG_LAUNCH(k_otd_reduce2, dim3(2 * r * r), dim3(NT), 0, st, (const double *)ot->part, g, r * r, ot->d);
    // (S and G are 16 doubles each in the block whatever r is: one call carries both)
    NLG_TRY(allreduce_sum(m->ctx, ot->d + OTD_S, 32));
    NLG_HIP(hipGetLastError());
    return 0;
}

// U <- U chol(G)^-T on every stored level of the OTD lanes: current and lagged velocities, explicit-term levels, pressure
int otd_orthonormalise(const nlg_otd *ot) {
    nlg_linop *op = ot->op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    NLG_TRY(otd_sums(ot, nullptr, nullptr, nullptr));
    ProfScope ps(m->ctx, P_VECOPS);
    NLG_LAUNCH(k_otd_chol, dim3(1), dim3(1), 0, st, ot->d, ot->r);
    OtdLevels lv;
    int nf = 0;
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < m->dim; ++c) {
            lv.p[nf] = op->ubuf[s][c], lv.n[nf++] = m->lvn;
            lv.p[nf] = op->fbuf[s][c], lv.n[nf++] = m->lvn;
        }
    lv.p[nf] = op->p, lv.n[nf++] = m->lpn;
    for (int q = nf; q < 20; ++q) lv.p[q] = nullptr, lv.n[q] = 0;
    const dim3 g(grid_for(m->lvn), nf);
    if (ot->r == 1)
        NLG_LAUNCH(k_otd_transform<1>, g, dim3(NT), 0, st, lv, (const double *)ot->d, op->slab_ld);
    else if (ot->r == 2)
        NLG_LAUNCH(k_otd_transform<2>, g, dim3(NT), 0, st, lv, (const double *)ot->d, op->slab_ld);
    else if (ot->r == 3)
        NLG_LAUNCH(k_otd_transform<3>, g, dim3(NT), 0, st, lv, (const double *)ot->d, op->slab_ld);
    else
        NLG_LAUNCH(k_otd_transform<4>, g, dim3(NT), 0, st, lv, (const double *)ot->d, op->slab_ld);
    NLG_HIP(hipGetLastError());
    return 0;
}

// inside a time step: Lr from the step's own D^T p, (nu A + h2 B) u and N of every lane, then F_j += bm1 sum_{i <= j} u_i C_ij
int otd_force(const nlg_otd *ot, double *const *Fnew, double h2) {
    nlg_linop *op = ot->op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    NLG_TRY(otd_sums(ot, op->gp, op->w, Fnew));
    ProfScope ps(m->ctx, P_VECOPS);
    NLG_LAUNCH(k_otd_coef, dim3(1), dim3(1), 0, st, ot->d, ot->r, h2);
    const int dim = m->dim, g = grid_for(m->lvn);
    const F3 F = f3(Fnew, dim);
    const CF3 u = cf3(op->ubuf[0], dim);
#define OTD_F(D_, R_) NLG_LAUNCH((k_otd_force<D_, R_>), dim3(g), dim3(NT), 0, st, m->lvn, F, u, (const double *)m->d_bm1, (const double *)ot->d, op->slab_ld)
#define OTD_F_D(D_)      \
    if (ot->r == 1)      \
        OTD_F(D_, 1);    \
    else if (ot->r == 2) \
        OTD_F(D_, 2);    \
    else if (ot->r == 3) \
        OTD_F(D_, 3);    \
    else                 \
        OTD_F(D_, 4)
    if (dim == 3) {
        OTD_F_D(3);
    } else {
        OTD_F_D(2);
    }
#undef OTD_F_D
#undef OTD_F
    NLG_HIP(hipGetLastError());
    return 0;
}

// one restated nek_advance step (perturbation mode), see oracle/lns.py ExptA.advance; three phases around the two solves
int adv_a(const Lanes &L) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int dim = m->dim, nl = L.nl;
    const int64_t ld = L.ld();
    const double dt = op->dt, nu = 1.0 / op->cfg.re;
    op->istep += 1;
    // gauge: keep the pressure mean-free (see oracle/lns.py advance)
    NLG_TRY(sem_ortho(m, op->p, nl, ld));
    const int k = std::min(op->istep, op->cfg.torder);
    const double b0 = BDF_B0[k];
    op->adv_k = k, op->adv_b0 = b0, op->adv_h2 = b0 / dt;
    if (L.nonlinear) {   // the "base flow" is the current state (velocity, and temperature when coupled); one lane only
        NLG_TRY(sem_conv_setup(m, op->ubuf[0], op->Ur, op->GU));
        if (op->cfg.ifheat) NLG_TRY(sem_conv_scalar_setup(m, op->tbuf[0], op->GT));
    } else if (L.lb >= 0) {
        // coupled mode: the fine-mesh factors of the base-flow lane's velocity at the level this step starts from, once for all lanes
        NLG_TRY(sem_conv_setup(m, at_lane3(op, op->ubuf[0], L.lb).p, op->Ur, op->GU));
    }
    if (op->cfg.ifheat) NLG_TRY(heat_step(L, k, b0));   // scalar first: the fluid sees the new temperature (Nek5000's order)
    // F = -N(u): written into the oldest forcing buffer, then the buffers rotate
    double **Fnew = op->fbuf[2];
    NLG_TRY(sem_conv_apply(m, op->Ur, op->GU, op->ubuf[0], Fnew, L.adjoint, nl, ld));   // all lanes against the shared base flow
    if (op->cfg.ifheat && L.adjoint) {
        // adjoint momentum equation: - theta+ grad Theta with the new theta+ (stored F is +N: add the weak term)
        NLG_TRY(sem_scalar_grad_apply(m, op->GT, op->tbuf[0], Fnew, 1.0, nl, ld));
    } else if (op->cfg.ifheat) {
        const double bs = L.nonlinear ? 2.0 : 1.0;   // the nonlinear step halves the whole stored term (F holds 2 N there)
        for (int v = 0; v < nl; ++v)
            launch_nf(dim, k_buoyancy<1>, k_buoyancy<2>, k_buoyancy<3>, dim3(grid_for(m->lvn)), st, m->lvn, f3(at_lane3(op, Fnew, v).p, dim),
                      (const double *)m->d_bm1, (const double *)at_lane(op, op->tbuf[0], v), bs * op->cfg.buoy[0], bs * op->cfg.buoy[1], bs * op->cfg.buoy[2]);
    }
    if (L.f_re[0]) {
        // forcing of this step: evaluated at the time level the step starts from, (istep - 1) dt, like the explicit terms
        // (resolvent.f90:97-103: alpha = exp(sign i omega time) before nek_advance); one launch for all lanes
        const double ph = L.sign * L.omega * (op->istep - 1) * dt;
        ForceLanes f;
        memset(&f, 0, sizeof(f));
        for (int v = 0; v < nl; ++v)
            for (int c = 0; c < dim; ++c) {
                f.re[v][c] = L.f_re[v]->vel(c);
                if (L.f_im[v]) f.im[v][c] = L.f_im[v]->vel(c);
            }
#define ADD_F(D_, NL_) NLG_LAUNCH((k_add_force<D_, NL_>), dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, f3(Fnew, dim), (const double *)m->d_bm1, f, std::cos(ph), -std::sin(ph), ld)
#define ADD_F_D(D_)   \
    if (nl == 1)      \
        ADD_F(D_, 1); \
    else if (nl == 2) \
        ADD_F(D_, 2); \
    else if (nl == 3) \
        ADD_F(D_, 3); \
    else              \
        ADD_F(D_, 4)
        if (dim == 3) {
            ADD_F_D(3);
        } else {
            ADD_F_D(2);
        }
#undef ADD_F_D
#undef ADD_F
    }
    // OTD modes: D^T p and H u are computed before the explicit term is final, because the forcing needs the reduced operator they give
    const double h2 = b0 / dt;
    const bool otd_on = op->otd && op->istep >= op->otd->o.startstep;
    if (otd_on) {
        NLG_TRY(sem_opgradt(m, op->p, op->gp, false, nullptr, nullptr, nl, ld, ld));
        NLG_TRY(sem_axhelm(m, op->ubuf[0], op->w, dim, nu, h2, nullptr, nullptr, nullptr, nullptr, false, nl, ld));
        NLG_TRY(otd_force(op->otd, Fnew, h2));
    }
    rotate3(op->fbuf);
    Hist h;
    h.k = k;
    h.half_lane = L.lb;   // the base-flow lane's own term -1/2 lns_conv(U; U): a coefficient of the history sum, not a pass
    for (int j = 0; j < 3; ++j) {
        h.ab[j] = -(L.nonlinear ? 0.5 : 1.0) * EXT_C[k][j];   // F = -N ; nonlinear: (u.grad)u = 1/2 [(U.grad)u + (u.grad)U] at U = u
        h.bd[j] = BDF_C[k][j];
        for (int c = 0; c < 3; ++c) {
            h.f[j][c] = op->fbuf[j][c];
            h.u[j][c] = op->ubuf[j][c];
        }
    }
    // residual form: res = mask QQ^T (rhs + D^T p - H u); the history sums and the two operator terms in ONE pass over the fields
    if (!otd_on) {
        NLG_TRY(sem_opgradt(m, op->p, op->gp, false, nullptr, nullptr, nl, ld, ld));
        NLG_TRY(sem_axhelm(m, op->ubuf[0], op->w, dim, nu, h2, nullptr, nullptr, nullptr, nullptr, false, nl, ld));
    }
    if (op->use_xp > 0) {
        // slab-permuted velocity solve: the right-hand side is born masked in that layout (no permutation pass in helm_problem, and
        // its gather-scatter moves the layout's 64-byte runs instead of the natural layout's single points)
        CF3 mk = {{m->d_mask[0], m->d_mask[1], m->d_mask[2]}};
        launch_nf(dim, k_rhs<1, true>, k_rhs<2, true>, k_rhs<3, true>, lgrid(grid_for(m->lvn), nl), st, m->lvn, h, (const double *)m->d_bm1, 1.0 / dt,
                  f3(op->rhs, dim), ld, cf3(op->gp, dim), cf3(op->w, dim), (const int *)m->d_slot_xp, m->np1, mk,
                  (const unsigned char *)op->maskb_v);   // (the bytes are in this layout: nlg_linop_init; null = the three mask arrays)
        NLG_TRY(sem_gs(m, op->rhs, dim, nullptr, LAYOUT_XP, nl, ld, 0));
        op->rhs_in_xp = true;
        return 0;
    }
    launch_nf(dim, k_rhs<1>, k_rhs<2>, k_rhs<3>, lgrid(grid_for(m->lvn), nl), st, m->lvn, h, (const double *)m->d_bm1, 1.0 / dt,
              f3(op->rhs, dim), ld, cf3(op->gp, dim), cf3(op->w, dim), (const int *)nullptr, 1, CF3{{nullptr, nullptr, nullptr}}, (const unsigned char *)nullptr);
    NLG_TRY(sem_gs(m, op->rhs, dim, nullptr, LAYOUT_NAT, nl, ld, 0));
    if (op->use_xp <= 0) {   // (slab-permuted velocity solve: the mask is applied by the permutation of the right-hand side, helm_problem)
        CF3 mk = {{m->d_mask[0], m->d_mask[1], m->d_mask[2]}};
        launch_nf(dim, k_colmul_gated<1>, k_colmul_gated<2>, k_colmul_gated<3>, lgrid(grid_for(m->lvn), nl), st,
                  (const double *)nullptr, f3(op->rhs, dim), mk, m->lvn, ld);
    }
    return 0;
}

int adv_b(const Lanes &L) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int dim = m->dim, nl = L.nl;
    const int64_t ld = L.ld();
    const double dt = op->dt, b0 = op->adv_b0;
    // uh = u + du -> into the oldest velocity buffer (slot 2), which becomes the new current after rotation
    double **unew = op->ubuf[2];
    if (op->ph > 0) {
        // deferred solution update of the velocity PCG: the increment is assembled from the direction ring here (k_add_hist)
        PHist Hh = {{nullptr, nullptr, nullptr}, (int64_t)dim * m->lvs, op->ph};
        for (int q = 0; q < dim; ++q) Hh.p0[q] = op->phist + (int64_t)q * m->lvs;
        launch_nf(dim, k_add_hist<1>, k_add_hist<2>, k_add_hist<3>, lgrid(grid_for(m->lvn), nl), st, (const double *)op->d_s, m->lvn, m->np1,
                  op->use_xp > 0 ? (const int *)m->d_slot_xp : (const int *)nullptr, f3(unew, dim), cf3(op->ubuf[0], dim), cf3(op->x, dim), Hh, ld);
    } else if (op->use_xp > 0) {
        launch_nf(dim, k_add_xp<1>, k_add_xp<2>, k_add_xp<3>, lgrid(grid_for(m->lvn), nl), st, m->lvn, m->np1, (const int *)m->d_slot_xp, f3(unew, dim),
                  cf3(op->ubuf[0], dim), cf3(op->x, dim), ld);
    } else {
        CF3 none = {{nullptr, nullptr, nullptr}};
        launch_nf(dim, k_lin3<1>, k_lin3<2>, k_lin3<3>, lgrid(grid_for(m->lvn), nl), st, m->lvn, f3(unew, dim), cf3(op->ubuf[0], dim),
                  cf3(op->x, dim), 1.0, none, 0.0, ld);
    }
    // pressure correction
    NLG_TRY(sem_opdiv(m, unew, op->pr_r, -(b0 / dt), nullptr, false, nullptr, nullptr, nullptr, nl, ld, ld));
    NLG_TRY(sem_ortho(m, op->pr_r, nl, ld));
    return 0;
}

int adv_c(const Lanes &L) {
    nlg_linop *op = L.op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int dim = m->dim, nl = L.nl;
    const int64_t ld = L.ld();
    const double dt = op->dt, b0 = op->adv_b0;
    double **unew = op->ubuf[2];
    NLG_LAUNCH(k_axpy1, lgrid(grid_for(m->lpn), nl), dim3(NT), 0, st, m->lpn, op->p, (const double *)op->pr_x, 1.0, ld);
    // the gradient of the pressure increment in the face-grouped layout of the pressure operator's intermediates where that exists
    // (3-D): its gather-scatter then moves whole faces (50 us against 100 us in the natural layout at 10^4 elements), and the update
    // below reads it through the element-local slot table
    const bool fg = sem_opgradt_has_fg(m);
    NLG_TRY(sem_opgradt(m, op->pr_x, op->gp, fg, nullptr, nullptr, nl, ld, ld));
    // u = uh + (dt / b0) mask binv QQ^T D^T dp: gather-scatter, then weights and update in one pass
    NLG_TRY(sem_gs(m, op->gp, dim, nullptr, fg ? LAYOUT_FG : LAYOUT_NAT, nl, ld, 0));
    const bool fused = op->d_filt && op->filt_fused;
    if (!fused) {
        CF3 wt = {{m->d_mbinv[0], m->d_mbinv[1], m->d_mbinv[2]}};
        // compact weights (as the velocity preconditioner's, and under its switch): binvm1 and the mask bytes in the face-grouped layout
        const bool wb = fg && op->maskb_v && m->d_maskb_fg && m->d_binv_fg;
        if (wb) wt.p[0] = m->d_binv_fg;
        if (fg)
            launch_nf(dim, k_axpy_w<1, true>, k_axpy_w<2, true>, k_axpy_w<3, true>, lgrid(grid_for(m->lvn), nl), st, m->lvn, f3(unew, dim), cf3(op->gp, dim),
                      wt, dt / b0, ld, (const int *)m->d_slot_fg, m->np1, wb ? (const unsigned char *)m->d_maskb_fg : (const unsigned char *)nullptr);
        else
            launch_nf(dim, k_axpy_w<1>, k_axpy_w<2>, k_axpy_w<3>, lgrid(grid_for(m->lvn), nl), st, m->lvn, f3(unew, dim), cf3(op->gp, dim), wt, dt / b0,
                      ld, (const int *)nullptr, 1, (const unsigned char *)nullptr);
    }
    if (op->d_filt) {
        // explicit filter, the last thing a step does: the velocity of every lane and, coupled, the new temperature (which the fluid
        // has seen unfiltered in its buoyancy term) in one launch; the pressure is never filtered
        double *fl[4] = {unew[0], unew[1], dim == 3 ? unew[2] : op->tbuf[0], op->tbuf[0]};
        const int nf = dim + (op->cfg.ifheat ? 1 : 0);
        if (fused)   // the update above rides in the filter's load
            NLG_TRY(sem_filter(m, op->d_filt, fl, nf, nl, ld, op->gp, m->d_mbinv, dt / b0, fg ? (const int *)m->d_slot_fg : nullptr));
        else
            NLG_TRY(sem_filter(m, op->d_filt, fl, nf, nl, ld));
    }
    NLG_HIP(hipGetLastError());
    // rotate velocity history: new -> current, current -> lag1, lag1 -> lag2
    rotate3(op->ubuf);
    op->st_steps += nl;
    return 0;
}

int advance(const Lanes &L) {
    NLG_TRY(adv_a(L));
    NLG_TRY(helm_solve(L, L.op->adv_k, L.op->adv_h2));
    NLG_TRY(adv_b(L));
    NLG_TRY(pres_solve(L, L.op->dt / L.op->adv_b0));
    return adv_c(L);
}

// integrator state of nl lanes <- 0, in a slab of at least nl lanes: the rotating velocity / forcing (/ temperature) levels are the
// first buffers of a lane, in canonical order after the re-binding, so ONE strided memset clears them in every lane
int reset_state(nlg_linop *op, int nl) {
    nlg_mesh *m = op->mesh;
    NLG_TRY(slab_ensure(op, nl));
    lane_bind(op);
    const int64_t nlev = (int64_t)(6 * m->dim + (op->cfg.ifheat ? 6 : 0)) * m->lvs;
    // one 1-D fill per lane: the 2-D fill of the runtime (hipMemset2DAsync over the slab pitch) ran at 0.2 TB/s -- 14.6 ms per block
    // step of four lanes, 8.5 % of it -- against 4.6 TB/s for the 1-D fill
    for (int v = 0; v < nl; ++v) NLG_HIP(hipMemsetAsync(op->slab + (size_t)v * (size_t)op->slab_ld, 0, sizeof(double) * (size_t)nlev, m->ctx->stream));
    return 0;
}

// Every run of the time stepper starts here: nl lanes at rest, time-step index 0, no per-lane iteration counts, nothing kept from
// the run before -- neither the pressure projection space nor what an orbit run left for nlg_linop_orbit_end / nlg_upo_fdot.
// (The projection space belongs to one run: the result must not depend on earlier calls.  Keeping it across matvecs, as a
// Nek5000 run does across time steps, was measured in round 4: 11.76 -> 11.40 pressure iterations per time step over 844 matvecs
// of a real Arnoldi / Krylov-Schur run -- successive Krylov vectors are orthogonal, their pressure increments share little --
// while bench.py, which re-applies the operator to the SAME column every step, would show 12.5 -> 6.5: an artefact, not adopted.)
int begin_run(nlg_linop *op, int nl) {
    NLG_TRY(reset_state(op, nl));
    op->istep = 0;
    op->nproj = 0;
    for (int v = 0; v < kMaxLanes; ++v) op->lane_viters[v] = op->lane_piters[v] = 0;
    op->orbit_end_valid = op->upo_fdot_valid = false;
    return 0;
}

int load_state(nlg_linop *op, int lane, const nlg_vec *v, int irst) {
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    for (int c = 0; c < m->dim; ++c)
        NLG_HIP(hipMemcpyAsync(at_lane(op, op->ubuf[0][c], lane), v->vel(c, irst), sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, st));
    NLG_HIP(hipMemcpyAsync(at_lane(op, op->p, lane), v->pr(irst), sizeof(double) * (size_t)m->lpn, hipMemcpyDeviceToDevice, st));
    if (op->cfg.ifheat)
        NLG_HIP(hipMemcpyAsync(at_lane(op, op->tbuf[0], lane), v->theta(0, irst), sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, st));
    return 0;
}

int store_state(nlg_linop *op, int lane, nlg_vec *v, int irst) {
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    for (int c = 0; c < m->dim; ++c)
        NLG_HIP(hipMemcpyAsync(v->vel(c, irst), at_lane(op, op->ubuf[0][c], lane), sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, st));
    NLG_HIP(hipMemcpyAsync(v->pr(irst), at_lane(op, op->p, lane), sizeof(double) * (size_t)m->lpn, hipMemcpyDeviceToDevice, st));
    if (op->cfg.ifheat)
        NLG_HIP(hipMemcpyAsync(v->theta(0, irst), at_lane(op, op->tbuf[0], lane), sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, st));
    return 0;
}

// An intent(out) vector, default-initialised (history cleared, nrst = 0), whose blocks 0 .. nfill are about to be filled by
// store_state: zero only the blocks behind them.  store_state writes every field the operator carries (the callers check that the
// vector carries the same ones) and leaves the padding behind a field alone, which is zero in every vector from its creation on
// (vec.hip), so a fill of the blocks 0 .. nfill would be overwritten to the last byte that matters.
int clear_for_store(nlg_vec *v, int nfill) {
    const int ntail = v->lorder - 1 - nfill;
    if (ntail > 0)
        NLG_HIP(hipMemsetAsync(v->d + (int64_t)(1 + nfill) * v->main_len, 0, sizeof(double) * (size_t)(ntail * v->main_len), v->mesh->ctx->stream));
    v->nrst = 0;
    return 0;
}

// out (velocity and pressure of its main block) = c (state of lane `lane` - X0), X0 = the operator's base flow, in one pass
int state_minus_x0(nlg_linop *op, int lane, double c, nlg_vec *out) {
    nlg_mesh *m = op->mesh;
    const int dim = m->dim;
    DdtArgs A;
    memset(&A, 0, sizeof(A));
    for (int f = 0; f <= dim; ++f) {
        const bool pr = f == dim;
        A.out[f] = pr ? out->pr() : out->vel(f), A.n[f] = pr ? m->lpn : m->lvn;
        A.src[f][0] = at_lane(op, pr ? op->p : op->ubuf[0][f], lane), A.c[f][0] = c;
        A.src[f][1] = pr ? op->baseflow->pr() : op->baseflow->vel(f), A.c[f][1] = -c;
    }
    NLG_LAUNCH(k_bdf_ddt, dim3(grid_for(m->lvn), dim + 1), dim3(NT), 0, m->ctx->stream, A);
    NLG_HIP(hipGetLastError());
    return 0;
}

// The two time derivatives of the base flow that the bordered Jacobian of a periodic orbit needs (the reference's compute_fdot,
// src/systems/periodic_orbit.f90:96-102), taken from the run of lane `lane` instead of from two extra impulsive restarts:
//   FDOT_START (after the first step)  f0 = (U^1 - U^0) / dt, velocity and pressure: compute_fdot at X0 literally;
//   FDOT_PRE   (before the last step)  fT = -sum_{j<k} bd_j U^{N-1-j} / dt, while the step still holds the level it overwrites;
//   FDOT_END   (after the last step)   fT += b0 U^N / dt: the BDF-k derivative the step itself used, k = min(nsteps, torder);
//                                      its pressure is (p^N - p^{N-1}) / dt = dp / dt, the one pressure level a step keeps.
enum { FDOT_START = 0, FDOT_PRE, FDOT_END };
int capture_fdot(nlg_linop *op, int lane, int phase) {
    nlg_mesh *m = op->mesh;
    const int dim = m->dim;
    const double idt = 1.0 / op->dt;
    if (phase == FDOT_START) return state_minus_x0(op, lane, idt, op->upo_f0);
    nlg_vec *o = op->upo_fT;
    DdtArgs A;
    memset(&A, 0, sizeof(A));
    for (int c = 0; c < dim; ++c) A.out[c] = o->vel(c), A.n[c] = m->lvn;
    A.out[dim] = o->pr(), A.n[dim] = m->lpn;
    if (phase == FDOT_PRE) {
        const int k = std::min(op->nsteps, op->cfg.torder);
        for (int c = 0; c < dim; ++c)
            for (int j = 0; j < k; ++j) A.src[c][j] = at_lane(op, op->ubuf[j][c], lane), A.c[c][j] = -BDF_C[k][j] * idt;
    } else {
        const int k = std::min(op->nsteps, op->cfg.torder);
        A.acc = 1;
        for (int c = 0; c < dim; ++c) A.src[c][0] = at_lane(op, op->ubuf[0][c], lane), A.c[c][0] = BDF_B0[k] * idt;
        A.src[dim][0] = at_lane(op, op->pr_x, lane), A.c[dim][0] = idt;
        op->upo_fdot_valid = true;
    }
    NLG_LAUNCH(k_bdf_ddt, dim3(grid_for(m->lvn), dim + 1), dim3(NT), 0, m->ctx->stream, A);
    NLG_HIP(hipGetLastError());
    return 0;
}

// The op->nsteps time steps of a run.  fdot_lane >= 0: that lane carries a base flow started from X0, and the three captures of its
// time derivatives ride along (capture_fdot).  after_step(istep) is the caller's hook (the history replay of a matvec).
template <typename Hook>
int run_steps(const Lanes &L, int fdot_lane, Hook after_step) {
    nlg_linop *op = L.op;
    for (int istep = 1; istep <= op->nsteps; ++istep) {
        if (fdot_lane >= 0 && istep == op->nsteps) NLG_TRY(capture_fdot(op, fdot_lane, FDOT_PRE));
        NLG_TRY(advance(L));
        if (fdot_lane >= 0 && istep == 1) NLG_TRY(capture_fdot(op, fdot_lane, FDOT_START));
        NLG_TRY(after_step(istep));
    }
    if (fdot_lane >= 0) NLG_TRY(capture_fdot(op, fdot_lane, FDOT_END));
    return 0;
}
int run_steps(const Lanes &L, int fdot_lane = -1) {
    return run_steps(L, fdot_lane, [](int) { return 0; });
}

// the projection of nf fields on one mesh for the lanes 0 .. s-1 of the slab whose bit in `mask` is set (f: lane 0's fields), lane l
// with the table at l * P.tld: one kernel; several ranks: partial sums -> global slots -> ONE all-reduce for all lanes -> apply (the
// reference's planar_avg is a global operation, exponential_propagator_proj.f90:146-169)
int project_lines(nlg_linop *op, const ProjLines &P, int nf, F3 f, int s, unsigned mask) {
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int64_t nl = P.nlines, ld = op->slab_ld, tld = P.tld;
    const dim3 g((unsigned)((nl + NT / 64 - 1) / (NT / 64)), (unsigned)s);
    const int *off = P.off, *idx = P.idx, *gs = P.gslot;
    const double *cv = P.cv, *sv = P.sv, *iden = P.iden, *glob = P.glob;
    if (!gs) {
        launch_nf(nf, k_proj_alpha<1>, k_proj_alpha<2>, k_proj_alpha<3>, g, st, nl, off, idx, P.weight, cv, sv, tld, iden, f, ld, mask);
    } else {
        const int64_t cnt = P.nglob * s * 2 * nf;
        NLG_HIP(hipMemsetAsync(P.glob, 0, sizeof(double) * (size_t)cnt, st));
        if (nl > 0)
            launch_nf(nf, k_proj_sums<1>, k_proj_sums<2>, k_proj_sums<3>, g, st, nl, off, idx, gs, P.weight, cv, sv, tld,
                      CF3{{f.p[0], f.p[1], f.p[2]}}, ld, mask, P.glob);
        NLG_TRY(allreduce_sum(m->ctx, P.glob, (int)cnt));
        if (nl > 0) launch_nf(nf, k_proj_apply<1>, k_proj_apply<2>, k_proj_apply<3>, g, st, nl, off, idx, gs, cv, sv, tld, iden, glob, f, ld, mask);
    }
    NLG_HIP(hipGetLastError());
    return 0;
}

// no-op unless a projection has been set: projects level `slot` of the state of the lanes 0 .. s-1 (those in `mask`), in one
// launch per mesh; lane l onto wavenumber l on an operator with wavenumber lanes, every lane onto the one wavenumber otherwise
int project_alpha(nlg_linop *op, int s, int slot, unsigned mask) {
    if (op->proj_v.nlines == 0) return 0;
    NLG_TRY(project_lines(op, op->proj_v, op->mesh->dim, f3(op->ubuf[slot], op->mesh->dim), s, mask));
    // the pressure is part of the state the integrator starts from (lagged pressure of the correction scheme) but not
    // of the inner product: left unprojected it is a subspace the Arnoldi norm cannot see (observed: a spurious
    // |mu| = 1.41 for plane Poiseuille flow at alpha = 2 instead of 0.945)
    const ProjLines &Pp = op->proj_p;
    if ((Pp.gslot || Pp.nlines > 0) && slot == 0) NLG_TRY(project_lines(op, Pp, 1, F3{{op->p, nullptr, nullptr}}, s, mask));
    return 0;
}

// =====================================================================================================================
// Multi-vector (block) propagator: s <= 4 perturbations advanced together, time step by time step (the reference advances
// several perturbations together through Nek5000's lpert / npert, src/neklab_nek_setup.f90:39-247, src/neklab_otd.f90:37-49).
// Every vector has a LANE: its own integrator state, PCG work vectors and device scalars, all lanes carved from one slab at a
// constant stride (struct nlg_linop); the base-flow data (fine-mesh fields of the convective term, preconditioners, weights)
// is shared.  The time step is the single-vector one (advance(Lanes)) with every kernel launched ONCE for all lanes
// (gridDim.y = lanes, or a lane loop inside the fused element kernels), own alpha / beta / convergence flag per lane -- each
// lane performs exactly the iteration of the single-vector path -- and, across ranks, ONE halo exchange / all-reduce per
// gather-scatter / reduction carrying all lanes.  A single matvec is the block of one.
// =====================================================================================================================
int do_matvec_block(nlg_linop *op, int s, const nlg_vec *const *vin, nlg_vec *const *vout, int adjoint) {
    NLG_CHECK(op && vin && vout, "exptA block matvec: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "exptA block matvec: %d vectors unsupported (1..%d)", s, kMaxLanes);
    NLG_CHECK(op->inited, "exptA block matvec: nlg_linop_init has not been called");
    NLG_NO_OTD(op, "exptA matvec");
    if (op->orbit) {
        NLG_CHECK(s <= kMaxLanes - 1, "exptA block matvec: orbit mode advances the base flow as one of the %d lanes, %d vectors unsupported (1..%d)",
                  kMaxLanes, s, kMaxLanes - 1);
        NLG_CHECK(!adjoint, "exptA rmatvec: orbit mode has no adjoint (the adjoint of a time-dependent linearisation needs U(T - t); nlg_linop_set_orbit)");
    }
    nlg_mesh *m = op->mesh;
    const int want_scal = op->cfg.ifheat ? 1 : 0;
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(vin[v] && vout[v] && vin[v]->mesh == m && vout[v]->mesh == m, "exptA block matvec: vector %d NULL or on a different mesh", v);
        NLG_CHECK(vin[v]->nscal == want_scal && vout[v]->nscal == want_scal, "exptA block matvec: vector %d carries %d scalars, the operator %d", v,
                  vin[v]->nscal, want_scal);
        NLG_CHECK(op->cfg.no_history || (vin[v]->lorder >= op->cfg.torder && vout[v]->lorder >= op->cfg.torder), "exptA block matvec: vector lorder < time order");
        for (int u = 0; u < s; ++u) NLG_CHECK(vin[v] != vout[u], "exptA block matvec: an input vector is also an output vector");
        for (int u = 0; u < v; ++u) NLG_CHECK(vout[v] != vout[u], "exptA block matvec: the same output vector twice");
    }
    const int nrst = op->cfg.no_history ? 0 : op->cfg.torder - 1;   // no_history: impulsive start, no history steps (include/neklab_gpu.h)
    // coupled (orbit) mode: lane s carries the base flow, from X0 (impulsive start, no history: periodic_orbit.f90:59-92 with
    // solve_baseflow = .true.) through the same time steps and the same launches as the s perturbation lanes before it
    const int nl = op->orbit ? s + 1 : s, lb = op->orbit ? s : -1;
    NLG_CHECK(op->proj_lanes == 0 || s <= op->proj_lanes, "exptA block matvec: %d vectors on an operator with %d wavenumber lanes (nlg_linop_set_projection_lanes)", s,
              op->proj_lanes);
    const unsigned all = (1u << s) - 1u;
    NLG_TRY(begin_run(op, nl));
    for (int v = 0; v < s; ++v) NLG_TRY(load_state(op, v, vin[v], 0));
    NLG_TRY(project_alpha(op, s, 0, all));   // exptA_proj_matvec: initial condition, exponential_propagator_proj.f90:51
    if (lb >= 0) NLG_TRY(load_state(op, lb, op->baseflow, 0));
    Lanes L{op, nl, lb};
    L.adjoint = adjoint;
    NLG_TRY(run_steps(L, lb, [&](int istep) -> int {
        if (istep <= nrst) {
            unsigned replayed = 0;
            for (int v = 0; v < s; ++v)
                if (vin[v]->nrst > 0) {
                    NLG_TRY(load_state(op, v, vin[v], istep));   // get_rst, exponential_propagator.f90:129-142
                    replayed |= 1u << v;
                }
            if (replayed) NLG_TRY(project_alpha(op, s, 0, replayed));   // (projected operator: replayed states are projected as well, see below)
        }
        return 0;
    }));
    // ... and the final state, :66.  The reference projects the initial condition and the final state only.  Here the
    // replayed history states and the lagged states of the multistep scheme are projected too: otherwise the extended map
    // (state, history) that the Arnoldi process iterates has a spurious unstable mode -- observed for plane Poiseuille flow
    // at alpha = 2, Re = 7500: a "converged" |mu| = 1.41 in front of the Orr-Sommerfeld pair |mu| = 0.9448; with the
    // consistent projection the leading pair is 0.94454.
    for (int slot = 0; slot < 3; ++slot) NLG_TRY(project_alpha(op, s, slot, all));
    for (int v = 0; v < s; ++v) {
        // vec_out is intent(out): default-initialised (history cleared, nrst = 0), then filled -- the main block here, the
        // history blocks 1 .. nrst below
        NLG_TRY(clear_for_store(vout[v], nrst));
        NLG_TRY(store_state(op, v, vout[v], 0));
    }
    if (lb >= 0) {   // Phi_T(X0), before the history steps (which advance the base flow as well, periodic_orbit.f90:185-213)
        NLG_TRY(clear_for_store(op->orbit_end, 0));
        NLG_TRY(store_state(op, lb, op->orbit_end, 0));
        op->orbit_end_valid = true;
    }
    for (int irst = 1; irst <= nrst; ++irst) {   // compute_rst, :109-127
        NLG_TRY(advance(L));
        for (int v = 0; v < s; ++v) {
            NLG_TRY(store_state(op, v, vout[v], irst));
            vout[v]->nrst = std::max(vout[v]->nrst, irst);
        }
    }
    op->st_matvecs += s;
    return 0;
}

int do_matvec(nlg_linop *op, const nlg_vec *vin, nlg_vec *vout, int adjoint) {
    NLG_CHECK(op && vin && vout, "exptA matvec: NULL argument");
    NLG_CHECK(op->inited, "exptA matvec: nlg_linop_init has not been called (reference: exptA%%init(), 1cyl.usr:20)");
    nlg_mesh *m = op->mesh;
    NLG_CHECK(vin->mesh == m && vout->mesh == m,
              "exptA matvec: vector on a different mesh (reference: type_error, exponential_propagator.f90:53-58)");
    NLG_CHECK(vin->nscal == (op->cfg.ifheat ? 1 : 0) && vout->nscal == vin->nscal,
              "exptA matvec: the vectors carry %d scalar(s), the operator expects %d (cfg.ifheat)", vin->nscal, op->cfg.ifheat ? 1 : 0);
    NLG_CHECK(op->cfg.no_history || (vin->lorder >= op->cfg.torder && vout->lorder >= op->cfg.torder),
              "exptA matvec: vector lorder %d < time order %d", vin->lorder, op->cfg.torder);
    NLG_CHECK(vin != vout, "exptA matvec: vec_in and vec_out must be distinct (intent(in) / intent(out))");
    return do_matvec_block(op, 1, &vin, &vout, adjoint);
}

// vec_out = state after the nsteps of one application started from `ic` (null: rest) under the time-harmonic body force
// Re[(f_re + i f_im) exp(i s omega t)], s = -1 for the adjoint equations: evaluate_rhs / evaluate_imaginary_part of the
// resolvent (src/linops/resolvent.f90:80-111, :133-166).  No restart-history replay, no history in the result.  s <= 4 such runs are
// the lanes of one block run (lane v: ic[v], f_re[v], f_im[v] -> vout[v]; omega, the adjoint flag, dt and the step count are
// shared), as Nek5000 advances npert > 1 perturbations together (src/neklab_nek_setup.f90:39-247).
int do_integrate_forced_block(nlg_linop *op, int s, const nlg_vec *const *ic, const nlg_vec *const *f_re, const nlg_vec *const *f_im, double omega,
                              int adjoint, nlg_vec *const *vout) {
    NLG_CHECK(op && f_re && vout, "integrate_forced: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "integrate_forced: %d forcings unsupported (1..%d)", s, kMaxLanes);
    NLG_CHECK(op->inited, "integrate_forced: nlg_linop_init has not been called");
    NLG_NO_OTD(op, "integrate_forced");
    NLG_CHECK(!op->orbit, "integrate_forced: not available in orbit mode (the forced response about a time-periodic base flow is not built; nlg_linop_set_orbit)");
    NLG_CHECK(op->proj_lanes == 0, "integrate_forced: not available on an operator with wavenumber lanes (a forced run does not project; nlg_linop_set_projection_lanes)");
    nlg_mesh *m = op->mesh;
    Lanes L{op, s};
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(f_re[v] && vout[v], "integrate_forced: NULL argument (forcing or output of lane %d)", v);
        L.f_re[v] = f_re[v];
        L.f_im[v] = f_im ? f_im[v] : nullptr;
    }
    for (int v = 0; v < s; ++v) {
        const nlg_vec *icv = ic ? ic[v] : nullptr;
        NLG_CHECK(L.f_re[v]->mesh == m && vout[v]->mesh == m && (!icv || icv->mesh == m) && (!L.f_im[v] || L.f_im[v]->mesh == m),
                  "integrate_forced: vector on a different mesh");
        for (int u = 0; u < s; ++u)
            NLG_CHECK(vout[v] != L.f_re[u] && vout[v] != L.f_im[u] && !(ic && vout[v] == ic[u]), "integrate_forced: the output must be distinct from the inputs");
        for (int u = 0; u < v; ++u) NLG_CHECK(vout[v] != vout[u], "integrate_forced: the same output vector twice");
        NLG_CHECK(L.f_re[v]->nscal == 0 && vout[v]->nscal == 0, "integrate_forced: scalar (temperature) coupling is not built yet");
    }
    hipStream_t st = m->ctx->stream;
    NLG_TRY(begin_run(op, s));
    for (int v = 0; v < s; ++v) {
        NLG_HIP(hipMemsetAsync(at_lane(op, op->p, v), 0, sizeof(double) * (size_t)m->lps, st));
        if (ic && ic[v]) NLG_TRY(load_state(op, v, ic[v], 0));
    }
    L.adjoint = adjoint;
    L.omega = omega, L.sign = adjoint ? -1.0 : 1.0;
    NLG_TRY(run_steps(L));
    for (int v = 0; v < s; ++v) {
        NLG_TRY(clear_for_store(vout[v], 0));
        NLG_TRY(store_state(op, v, vout[v], 0));
    }
    return 0;
}

int do_integrate_forced(nlg_linop *op, const nlg_vec *ic, const nlg_vec *f_re, const nlg_vec *f_im, double omega, int adjoint, nlg_vec *vout) {
    NLG_CHECK(op && f_re && vout, "integrate_forced: NULL argument");
    return do_integrate_forced_block(op, 1, &ic, &f_re, &f_im, omega, adjoint, &vout);
}

// vec_out = Phi_tau(vec_in) - vec_in with the NONLINEAR integrator (reference: nonlinear_map, src/systems/fixed_point.f90:4-38):
// dt from the CFL number of vec_in itself, no restart-history replay, no history in the result
int do_nonlinear_map(nlg_linop *op, const nlg_vec *vin, nlg_vec *vout) {
    NLG_CHECK(op && vin && vout, "nonlinear_map: NULL argument");
    NLG_NO_OTD(op, "nonlinear_map");
    nlg_mesh *m = op->mesh;
    NLG_CHECK(vin->mesh == m && vout->mesh == m, "nonlinear_map: vector on a different mesh (reference: type_error, fixed_point.f90:31-36)");
    NLG_CHECK(vin->nscal == (op->cfg.ifheat ? 1 : 0) && vout->nscal == vin->nscal,
              "nonlinear_map: the vectors carry %d scalar(s), the operator expects %d (cfg.ifheat)", vin->nscal, op->cfg.ifheat ? 1 : 0);
    NLG_CHECK(vin != vout, "nonlinear_map: vec_in and vec_out must be distinct");
    NLG_CHECK(!op->orbit, "nonlinear_map: the operator is in orbit mode and holds X0 as its base flow (use a second operator, or nlg_linop_set_orbit(op, NULL, 0))");
    // "setup_nonlinear_solver(recompute_dt = .true.)": the time step follows the state that is integrated
    NLG_TRY(nlg_vec_copy(op->baseflow, vin));
    NLG_TRY(nlg_linop_init(op));
    NLG_TRY(begin_run(op, 1));
    NLG_TRY(load_state(op, 0, vin, 0));
    Lanes L{op, 1};
    L.nonlinear = 1;
    NLG_TRY(run_steps(L));
    NLG_TRY(clear_for_store(vout, 0));
    NLG_TRY(store_state(op, 0, vout, 0));
    NLG_TRY(nlg_vec_axpby(-1.0, vin, 1.0, vout));   // vec_out%sub(vec_in), fixed_point.f90:29
    // the base-flow dependent set-up now belongs to vec_in: a later linear matvec needs nlg_linop_set_baseflow
    return 0;
}

}  // namespace

namespace nlg {
int linop_proj_lanes(const nlg_linop *op) { return op->proj_lanes; }

// one byte per velocity point, bit c = mask_c != 0, in the natural or (xp) the slab-permuted layout: the compact Dirichlet mask of the
// velocity PCG (out: m->lvs bytes; scratch fields 3 and 4 are overwritten)
int vel_mask_bytes(nlg_mesh *m, bool xp, unsigned char *out) {
    hipStream_t st = m->ctx->stream;
    double *t0 = sem_scratch1(m, 3), *t1 = xp ? sem_scratch1(m, 4) : nullptr;
    NLG_CHECK(t0 && (t1 || !xp), "vel_mask_bytes: scratch allocation failed");
    NLG_LAUNCH(k_maskbits, dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, t0, (const double *)m->d_mask[0], (const double *)m->d_mask[1],
                       (const double *)m->d_mask[2]);
    if (xp) {
        double *a[1] = {t0}, *b[1] = {t1};
        NLG_TRY(sem_to_xp(m, a, b, 1));
    }
    NLG_LAUNCH(k_to_bytes, dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, out, (const double *)(xp ? t1 : t0));
    NLG_HIP(hipGetLastError());
    return 0;
}
}  // namespace nlg

extern "C" {

int nlg_exptA_config_default(nlg_exptA_config *c) {
    NLG_CHECK(c, "nlg_exptA_config_default: NULL");
    memset(c, 0, sizeof(*c));
    c->tau = 1.0;
    c->re = 100.0;
    c->cfl_limit = 0.5;
    c->vtol = 1e-9;
    c->ptol = 1e-7;
    c->dt = 0.0;
    c->torder = 3;
    c->maxit_v = 200;
    c->maxit_p = 2000;
    c->ifheat = 0;
    c->conductivity = 1.0;
    c->rhocp = 1.0;
    c->pproj = 1;   // residualProj = yes for the pressure, as in the reference's cylinder case (1cyl.par:23)
    c->no_history = 0;
    c->filter_weight = 0.0;
    c->filter_modes = 0;
    return 0;
}

int nlg_linop_create(nlg_mesh *mesh, const nlg_exptA_config *cfg, const nlg_vec *baseflow, nlg_linop **out) {
    NLG_CHECK(mesh && cfg && baseflow && out, "nlg_linop_create: NULL argument");
    NLG_CHECK(baseflow->mesh == mesh, "nlg_linop_create: baseflow lives on a different mesh");
    NLG_CHECK(cfg->torder >= 1 && cfg->torder <= 3, "nlg_linop_create: torder %d unsupported (1..3)", cfg->torder);
    NLG_CHECK(cfg->tau > 0.0 && cfg->re > 0.0, "nlg_linop_create: tau and re must be positive");
    NLG_CHECK(!cfg->ifheat || (baseflow->nscal >= 1 && cfg->conductivity > 0.0 && cfg->rhocp > 0.0),
              "nlg_linop_create: ifheat needs a base flow with its temperature (nscal >= 1) and positive conductivity / rhocp");
    NLG_CHECK(cfg->filter_weight >= 0.0 && cfg->filter_weight <= 1.0, "nlg_linop_create: filter_weight %g outside [0, 1]", cfg->filter_weight);
    std::vector<double> filt;
    if (cfg->filter_weight > 0.0) {
        NLG_CHECK(cfg->filter_modes >= 1 && cfg->filter_modes <= mesh->n - 2, "nlg_linop_create: filter_modes %d outside [1, lx1 - 2 = %d]",
                  cfg->filter_modes, mesh->n - 2);
        NLG_CHECK(sem_filter_available(mesh), "nlg_linop_create: the explicit filter has no kernel for lx1 = %d in %d-D (2-D: 6, 8, 10; 3-D: 6, 8, 10, 12)",
                  mesh->n, mesh->dim);
        NLG_TRY(sem_filter_matrix(mesh, cfg->filter_modes, cfg->filter_weight, filt));
    }
    nlg_linop *op = new nlg_linop();
    op->mesh = mesh;
    op->cfg = *cfg;
    if (!filt.empty()) {
        op->filt_fused = !(getenv("NLG_FILTER_FUSED") && atoi(getenv("NLG_FILTER_FUSED")) == 0);
        NLG_HIP(hipMalloc(&op->d_filt, sizeof(double) * filt.size()));
        NLG_HIP(hipMemcpy(op->d_filt, filt.data(), sizeof(double) * filt.size(), hipMemcpyHostToDevice));
    }
    NLG_TRY(nlg_vec_clone(baseflow, &op->baseflow));
    *out = op;
    return 0;
}

int nlg_linop_destroy(nlg_linop *op) {
    if (!op) return 0;
    NLG_NO_OTD(op, "nlg_linop_destroy");
    hipDeviceSynchronize();
    auto fr = [](double *p) {
        if (p) hipFree(p);
    };
    fr(op->slab);        // every per-lane work buffer (lane_buffers)
    fr(op->d_filt);
    fr(op->d_red);
    for (int c = 0; c < 3; ++c) {
        fr(op->Ur[c]);
        for (int k = 0; k < 4; ++k) fr(op->pcv[k][c]);
        for (int k = 0; k < 4; ++k) fr(op->pcv_xp[k][c]);
    }
    for (int k = 0; k < 4; ++k) fr(op->pci[k]);
    if (op->maskb_v) hipFree(op->maskb_v);
    for (int q = 0; q < 9; ++q) fr(op->GU[q]);
    fr(op->pce);
    for (int q = 0; q < 3; ++q) fr(op->GT[q]);
    for (int k = 0; k < 4; ++k) fr(op->pct[k]);
    op->proj_v.free();
    op->proj_p.free();
    fr(op->nwv);
    fr(op->nwv_xp);
    fr(op->nwp);
    if (op->h_s) hipHostFree(op->h_s);
    if (op->baseflow) nlg_vec_destroy(op->baseflow);
    if (op->orbit_end) nlg_vec_destroy(op->orbit_end);
    if (op->upo_f0) nlg_vec_destroy(op->upo_f0);
    if (op->upo_fT) nlg_vec_destroy(op->upo_fT);
    delete op;
    return 0;
}

// dg = QQ^T diag(h1 A + h2 B), then the Jacobi preconditioners pc[c] = mask[c] / dg of nf fields
static int jacobi_pc(nlg_mesh *m, double h1, double h2, int nf, double *const *mask, double *const *pc, double *dg) {
    NLG_TRY(sem_helm_diag(m, dg, h1, h2));
    double *f[1] = {dg};
    NLG_TRY(sem_gs(m, f, 1));
    for (int c = 0; c < nf; ++c)
        NLG_LAUNCH(k_recipmask, dim3(grid_for(m->lvn)), dim3(NT), 0, m->ctx->stream, m->lvn, pc[c], (const double *)dg, (const double *)mask[c]);
    return 0;
}

int nlg_linop_init(nlg_linop *op) {
    NLG_CHECK(op, "nlg_linop_init: NULL");
    NLG_NO_OTD(op, "nlg_linop_init");
    nlg_mesh *m = op->mesh;
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int dim = m->dim;
    NLG_HIP(hipSetDevice(ctx->device));
    if (!op->set_up) {
        for (int c = 0; c < dim; ++c) {
            NLG_HIP(hipMalloc(&op->Ur[c], sizeof(double) * (size_t)m->lfn));
            for (int k = 1; k <= op->cfg.torder; ++k) NLG_TRY(lalloc(op, &op->pcv[k][c], m->lvs));
        }
        for (int q = 0; q < dim * dim; ++q) NLG_HIP(hipMalloc(&op->GU[q], sizeof(double) * (size_t)m->lfn));
        NLG_TRY(lalloc(op, &op->pce, m->lps));
        NLG_TRY(lalloc(op, &op->nwv, m->lvs));
        NLG_TRY(lalloc(op, &op->nwp, m->lps));
        NLG_HIP(hipHostMalloc(&op->h_s, sizeof(double) * kMaxLanes * S_N, hipHostMallocDefault));
        NLG_TRY(reduce_ws_reserve(ctx, 4));
        // single-reduction PCG for the pointwise-preconditioned solves, opt-in (NLG_PCG_SINGLE_RED=1; decided before the slab is laid
        // out: it needs one more vector per solve).  One all-reduce per iteration instead of two, for two more vector streams per
        // iteration: measured +9 % per time step on one rank at 10,240 elements, +3 % at 1,300, and 23 of 454 collectives per time step
        // fewer on 2 ranks -- it pays only where an all-reduce costs more than ~15 us, which this pool cannot measure
        op->use_sr = getenv("NLG_PCG_SINGLE_RED") && atoi(getenv("NLG_PCG_SINGLE_RED")) != 0;
        // deferred solution update of the velocity PCG (k_add_hist): depth of the direction ring, NLG_PCG_DEFER_X=0 switches it off
        // (default 16 slots, fewer where 16 would take more than 8 GB per lane: a solve that outlasts the ring pays one k_x_flush per
        // ring length, which still moves fewer bytes than updating x in every iteration as long as the ring holds >= 3 directions)
        const int64_t slot_bytes = (int64_t)sizeof(double) * dim * m->lvs;
        const int ph_auto = (int)std::max<int64_t>(3, std::min<int64_t>(16, ((int64_t)8 << 30) / std::max<int64_t>(slot_bytes, 1)));
        op->ph = op->use_sr ? 0 : std::max(0, std::min(kAlphaRing, getenv("NLG_PCG_DEFER_X") ? atoi(getenv("NLG_PCG_DEFER_X")) : ph_auto));
        // ... and of the pressure PCG, where the gradient kernel performs the direction update (3-D, lx1 = 8 .. 10).  Opt-in
        // (NLG_PCG_DEFER_XP=16): measured neutral at 10^4 elements -- the update kernel of the preconditioner drops 3 of its 9 streams
        // (preconditioner class 7.06 -> 6.83 ms per step), the assembly of x and the colder directions give it back (44.5 ms either way)
        op->php = (dim == 3 && sem_opgradt_fuses_pupdate(m) && getenv("NLG_PCG_DEFER_XP")) ? std::max(0, std::min(kAlphaRing, atoi(getenv("NLG_PCG_DEFER_XP")))) : 0;
        // z = pc r of the velocity PCG formed by the operator kernel instead of stored and loaded back; NLG_PCG_STORE_Z=1 keeps the stored z
        op->store_z = getenv("NLG_PCG_STORE_Z") && atoi(getenv("NLG_PCG_STORE_Z")) != 0;
        NLG_TRY(slab_ensure(op, 1));   // the work buffers of one lane; a block matvec grows the slab on first use
        NLG_TRY(lalloc(op, &op->d_red, 3 * kMaxLanes));
        op->set_up = true;
    }
    double *U[3] = {op->baseflow->vel(0), op->baseflow->vel(1), dim == 3 ? op->baseflow->vel(2) : nullptr};
    // dt / nsteps (reference: neklab_nek_setup.f90:195-198)
    if (op->orbit && op->orbit_nsteps > 0) {   // nlg_linop_set_orbit_steps: the count is given, dt follows the period
        op->nsteps = op->orbit_nsteps;
        op->dt = op->cfg.tau / op->nsteps;
        NLG_TRY(sem_cfl(m, U, op->dt, &op->cfl));
    } else if (op->cfg.dt > 0.0) {
        op->nsteps = (int)std::ceil(op->cfg.tau / op->cfg.dt - 1e-12);
        op->dt = op->cfg.tau / op->nsteps;
        NLG_TRY(sem_cfl(m, U, op->dt, &op->cfl));
    } else {
        double c1 = 0.0;
        NLG_TRY(sem_cfl(m, U, 1.0, &c1));
        NLG_CHECK(c1 > 0.0, "nlg_linop_init: base flow has zero CFL; give cfg.dt explicitly");
        const double dt0 = op->cfg.cfl_limit / c1;
        op->nsteps = (int)std::ceil(op->cfg.tau / dt0);
        op->dt = op->cfg.tau / op->nsteps;
        op->cfl = c1 * op->dt;
    }
    // convective-term precomputation
    NLG_TRY(sem_conv_setup(m, U, op->Ur, op->GU));
    // Jacobi preconditioners of the velocity solve, per BDF order, all from one diagonal: pcv = mask_c / diag (pcv_xp: in the layout of
    // the slab-permuted solve) and, in compact form for the streaming kernels of the PCG, pci = 1 / diag in the layout of the solve plus
    // one mask byte per point.  The compact form needs masks of zeros and ones (sem.hip checked that when it built the byte masks of
    // the pressure operator: m->d_maskb_fg exists) -- NLG_PC_MASKB=0 keeps the three arrays
    const double nu = 1.0 / op->cfg.re;
    if (op->use_xp < 0) op->use_xp = (dim == 3 && m->d_slot_xp && (m->gs.d_indices_xp || m->gs.ngroups == 0)) ? 1 : 0;
    const bool xp = op->use_xp > 0;
    const bool compact = dim == 3 && m->d_maskb_fg && !op->use_sr && !(getenv("NLG_PC_MASKB") && atoi(getenv("NLG_PC_MASKB")) == 0);
    double *t0 = sem_scratch1(m, 3), *t1 = compact ? sem_scratch1(m, 4) : nullptr;   // t0: the diagonal (jacobi_pc)
    NLG_CHECK(t0 && (t1 || !compact), "nlg_linop_init: scratch allocation failed");
    for (int k = 1; k <= op->cfg.torder; ++k) {
        NLG_TRY(jacobi_pc(m, nu, BDF_B0[k] / op->dt, dim, m->d_mask, op->pcv[k], t0));
        if (compact) {
            if (!op->pci[k]) NLG_TRY(lalloc(op, &op->pci[k], m->lvs));
            NLG_LAUNCH(k_recip1, dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, xp ? t1 : op->pci[k], (const double *)t0);
            if (xp) {
                double *a[1] = {t1}, *b[1] = {op->pci[k]};
                NLG_TRY(sem_to_xp(m, a, b, 1));
            }
            for (int c = 0; c < 3; ++c) op->pci_l[k][c] = op->pci[k];
        }
        if (xp) {
            for (int c = 0; c < dim; ++c)
                if (!op->pcv_xp[k][c]) NLG_TRY(lalloc(op, &op->pcv_xp[k][c], m->lvs));
            NLG_TRY(sem_to_xp(m, op->pcv[k], op->pcv_xp[k], dim));
        }
    }
    if (compact) {
        if (!op->maskb_v) {
            NLG_HIP(hipMalloc(&op->maskb_v, (size_t)m->lvs));
            NLG_HIP(hipMemsetAsync(op->maskb_v, 0, (size_t)m->lvs, st));
        }
        NLG_TRY(vel_mask_bytes(m, xp, op->maskb_v));
    }
    // (the velocity solve always runs the direction update inside the operator kernel, helm_problem)
    op->z_free = dim == 3 && op->maskb_v && !op->use_sr && !op->store_z && sem_axhelm_forms_z(m);
    if (op->cfg.ifheat) {
        if (!op->pct[1]) {
            for (int k = 1; k <= op->cfg.torder; ++k) NLG_TRY(lalloc(op, &op->pct[k], m->lvs));
            for (int q = 0; q < dim; ++q) NLG_HIP(hipMalloc(&op->GT[q], sizeof(double) * (size_t)m->lfn));
        }
        NLG_TRY(sem_conv_scalar_setup(m, op->baseflow->theta(0), op->GT));
        for (int k = 1; k <= op->cfg.torder; ++k)
            NLG_TRY(jacobi_pc(m, op->cfg.conductivity, op->cfg.rhocp * BDF_B0[k] / op->dt, 1, &m->d_tmask, &op->pct[k], t0));
    }
    {
        double *ed = sem_scratch2(m, 5);
        NLG_CHECK(ed, "nlg_linop_init: scratch allocation failed");
        NLG_TRY(sem_ediag(m, ed));
        NLG_LAUNCH(k_recip1, dim3(grid_for(m->lpn)), dim3(NT), 0, st, m->lpn, op->pce, (const double *)ed);
    }
    NLG_LAUNCH(k_mul3, dim3(grid_for(m->lvn)), dim3(NT), 0, st, m->lvn, op->nwv, (const double *)m->d_binvm1,
                       (const double *)m->d_vmult, 1.0 / m->volvm1);
    NLG_LAUNCH(k_scale1, dim3(grid_for(m->lpn)), dim3(NT), 0, st, m->lpn, op->nwp, (const double *)m->d_bm2inv,
                       1.0 / m->volvm2);
    if (op->use_xp > 0) {
        if (!op->nwv_xp) NLG_TRY(lalloc(op, &op->nwv_xp, m->lvs));
        double *a[1] = {op->nwv}, *b[1] = {op->nwv_xp};
        NLG_TRY(sem_to_xp(m, a, b, 1));
    }
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipStreamSynchronize(st));
    op->inited = true;
    return 0;
}

int nlg_linop_matvec(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out) { return do_matvec(op, vec_in, vec_out, 0); }
int nlg_linop_rmatvec(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out) { return do_matvec(op, vec_in, vec_out, 1); }
int nlg_linop_matvec_block(nlg_linop *op, int s, const nlg_vec *const *vec_in, nlg_vec *const *vec_out, int transpose) {
    return do_matvec_block(op, s, vec_in, vec_out, transpose ? 1 : 0);
}

int nlg_linop_nonlinear_map(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out) { return do_nonlinear_map(op, vec_in, vec_out); }

int nlg_linop_integrate_forced(nlg_linop *op, const nlg_vec *ic, const nlg_vec *f_re, const nlg_vec *f_im, double omega, int adjoint,
                               nlg_vec *vec_out) {
    return do_integrate_forced(op, ic, f_re, f_im, omega, adjoint, vec_out);
}
int nlg_linop_integrate_forced_block(nlg_linop *op, int s, const nlg_vec *const *ic, const nlg_vec *const *f_re, const nlg_vec *const *f_im, double omega,
                                     int adjoint, nlg_vec *const *vec_out) {
    return do_integrate_forced_block(op, s, ic, f_re, f_im, omega, adjoint, vec_out);
}

int nlg_linop_set_baseflow(nlg_linop *op, const nlg_vec *baseflow) {
    NLG_CHECK(op && baseflow && baseflow->mesh == op->mesh, "nlg_linop_set_baseflow: bad argument");
    NLG_NO_OTD(op, "nlg_linop_set_baseflow");
    NLG_CHECK(!op->orbit, "nlg_linop_set_baseflow: the operator is in orbit mode; nlg_linop_set_orbit replaces X0");
    NLG_TRY(nlg_vec_copy(op->baseflow, baseflow));
    return nlg_linop_init(op);
}

// the lines of one mesh into P (empty on entry; the caller frees it whatever this returns): lines = groups of local dofs with the same
// label, ordered by label then by index.  The coordinate along the homogeneous direction is on the device (d_x) or on the host (h_x).
// nalpha wavenumbers: the lines once, one cos / sin table per wavenumber (k_cossin each: table l is the table of a single alpha[l]).
// per_lane: lane l of a block reads table l (tld = n); otherwise nalpha = 1 and every lane reads the one table (tld = 0).
static int proj_build(nlg_mesh *m, const char *who, int nalpha, const double *alpha, bool per_lane, int64_t n, const int64_t *lab, const double *d_x, const double *h_x,
                      ProjLines &P) {
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    std::vector<int> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [lab](int a, int b) { return lab[a] < lab[b] || (lab[a] == lab[b] && a < b); });
    std::vector<int> off{0};
    for (int64_t q = 1; q <= n; ++q)
        if (q == n || lab[order[q]] != lab[order[q - 1]]) off.push_back((int)q);
    const int nlines = (int)off.size() - 1;
    std::vector<double> wt((size_t)n), iden((size_t)nlines);
    NLG_HIP(hipMemcpyAsync(wt.data(), P.weight, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    for (int g = 0; g < nlines; ++g) {
        double sum = 0.0;
        for (int q = off[g]; q < off[g + 1]; ++q) sum += wt[order[q]];
        NLG_CHECK(sum > 0.0, "%s: empty line", who);
        iden[g] = 1.0 / sum;
    }
    P.nlines = nlines;
    P.tld = per_lane ? n : 0;
    NLG_HIP(hipMalloc(&P.off, sizeof(int) * off.size()));
    NLG_HIP(hipMalloc(&P.idx, sizeof(int) * (size_t)n));
    NLG_HIP(hipMalloc(&P.iden, sizeof(double) * (size_t)nlines));
    NLG_HIP(hipMalloc(&P.cv, sizeof(double) * (size_t)(n * nalpha)));
    NLG_HIP(hipMalloc(&P.sv, sizeof(double) * (size_t)(n * nalpha)));
    NLG_HIP(hipMemcpy(P.off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice));
    NLG_HIP(hipMemcpy(P.idx, order.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    NLG_HIP(hipMemcpy(P.iden, iden.data(), sizeof(double) * (size_t)nlines, hipMemcpyHostToDevice));
    DevBuf<double> xs;
    if (h_x) {   // (pressure mesh)
        NLG_HIP(hipMalloc(&xs.p, sizeof(double) * (size_t)n));
        NLG_HIP(hipMemcpy(xs.p, h_x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        d_x = xs.p;
    }
    for (int l = 0; l < nalpha; ++l) NLG_LAUNCH(k_cossin, dim3(grid_for(n)), dim3(NT), 0, st, n, d_x, alpha[l], P.cv + l * n, P.sv + l * n);
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipStreamSynchronize(st));
    if (!ctx->distributed()) return 0;
    // the labels are global line names: gather every rank's distinct labels, number the union (identically on all
    // ranks), and sum the weights of the parts of a line over the ranks for the denominators
    const int nr = ctx->nranks;
    const double mine = (double)nlines;
    std::vector<double> cnts(nr);
    int64_t maxc = 1;
    {
        DevBuf<double> cnt;
        NLG_HIP(hipMalloc(&cnt.p, sizeof(double) * (nr + 1)));
        NLG_HIP(hipMemcpy(cnt.p + nr, &mine, sizeof(double), hipMemcpyHostToDevice));
        NLG_TRY(allgather_f64(ctx, cnt.p + nr, cnt.p, 1));
        NLG_HIP(hipMemcpyAsync(cnts.data(), cnt.p, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
    }
    for (double c : cnts) maxc = std::max<int64_t>(maxc, (int64_t)c);
    std::vector<int64_t> mylab((size_t)maxc, -1), all((size_t)maxc * nr);
    for (int g = 0; g < nlines; ++g) mylab[g] = lab[order[off[g]]];
    {
        DevBuf<double> labs;   // (labels travel as 8-byte words)
        NLG_HIP(hipMalloc(&labs.p, sizeof(int64_t) * (size_t)maxc * (nr + 1)));
        NLG_HIP(hipMemcpy(labs.p + (size_t)maxc * nr, mylab.data(), sizeof(int64_t) * (size_t)maxc, hipMemcpyHostToDevice));
        NLG_TRY(allgather_f64(ctx, labs.p + (size_t)maxc * nr, labs.p, maxc));
        NLG_HIP(hipMemcpyAsync(all.data(), labs.p, sizeof(int64_t) * (size_t)maxc * nr, hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
    }
    std::vector<int64_t> uni;
    for (int q = 0; q < nr; ++q)
        for (int64_t g = 0; g < (int64_t)cnts[q]; ++g) uni.push_back(all[(size_t)q * maxc + g]);
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    std::vector<int> gs((size_t)std::max(nlines, 1));
    for (int g = 0; g < nlines; ++g) gs[g] = (int)(std::lower_bound(uni.begin(), uni.end(), mylab[g]) - uni.begin());
    NLG_HIP(hipMalloc(&P.gslot, sizeof(int) * gs.size()));
    NLG_HIP(hipMemcpy(P.gslot, gs.data(), sizeof(int) * gs.size(), hipMemcpyHostToDevice));
    P.nglob = (int64_t)uni.size();
    // sized for the largest block that can be projected, kMaxLanes lanes of three fields, whatever tld: a block on a single-alpha
    // operator shares one all-reduce as the lanes of a sweep do (a few KB either way)
    NLG_HIP(hipMalloc(&P.glob, sizeof(double) * (size_t)(P.nglob * kMaxLanes * 2 * 3)));
    NLG_HIP(hipMemsetAsync(P.glob, 0, sizeof(double) * (size_t)P.nglob, st));
    const unsigned g1 = (unsigned)((nlines + NT / 64 - 1) / (NT / 64));
    if (nlines > 0)
        NLG_LAUNCH(k_proj_wsum, dim3(g1), dim3(NT), 0, st, (int64_t)nlines, (const int *)P.off, (const int *)P.idx, (const int *)P.gslot, P.weight, P.glob);
    NLG_TRY(allreduce_sum(ctx, P.glob, (int)P.nglob));
    if (nlines > 0)
        NLG_LAUNCH(k_proj_iden, dim3(grid_for(nlines)), dim3(NT), 0, st, (int64_t)nlines, (const int *)P.gslot, (const double *)P.glob, P.iden);
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

// nlg_linop_set_projection / nlg_linop_set_projection_lanes (include/neklab_gpu.h): one table for all lanes of a block, or one per lane
static int set_projection(nlg_linop *op, const char *who, int nalpha, const double *alpha, bool per_lane, int idir, const int64_t *line_label,
                          const int64_t *line_label2, const double *x2) {
    NLG_CHECK(op && line_label, "%s: NULL argument", who);
    NLG_CHECK(alpha, "%s: NULL alpha (one wavenumber per lane)", who);
    NLG_CHECK(nalpha >= 1 && nalpha <= kMaxLanes, "%s: %d wavenumber lanes unsupported (1..%d)", who, nalpha, kMaxLanes);
    NLG_NO_OTD(op, who);
    nlg_mesh *m = op->mesh;
    NLG_CHECK(idir >= 1 && idir <= m->dim, "%s: idir %d out of range", who, idir);
    NLG_CHECK(op->inited, "%s: call init first", who);
    NLG_CHECK(!op->orbit, "%s: not available in orbit mode (the base-flow lane is a full state, not one wavenumber; nlg_linop_set_orbit)", who);
    NLG_CHECK(!per_lane || !op->cfg.ifheat, "%s: not available with cfg.ifheat (the projection does not touch the scalar)", who);
    NLG_CHECK((line_label2 == nullptr) == (x2 == nullptr), "%s: pressure-mesh labels and coordinates go together", who);
    // built beside the operator's and swapped in on success: a call that fails leaves the operator as it was
    ProjLines pv, pp;
    pv.weight = m->d_bm1, pp.weight = m->d_bm2;
    int rc = proj_build(m, who, nalpha, alpha, per_lane, m->lvn, line_label, m->d_x[idir - 1], nullptr, pv);
    if (!rc && line_label2) rc = proj_build(m, who, nalpha, alpha, per_lane, m->lpn, line_label2, nullptr, x2, pp);
    if (!rc) {
        std::swap(op->proj_v, pv);
        std::swap(op->proj_p, pp);
        op->proj_lanes = per_lane ? nalpha : 0;
    }
    (void)hipStreamSynchronize(m->ctx->stream);   // nothing in flight may still use what is freed now
    pv.free();
    pp.free();
    return rc;
}

int nlg_linop_set_projection(nlg_linop *op, double alpha, int idir, const int64_t *line_label, const int64_t *line_label2,
                             const double *x2) {
    return set_projection(op, "nlg_linop_set_projection", 1, &alpha, false, idir, line_label, line_label2, x2);
}

int nlg_linop_set_projection_lanes(nlg_linop *op, int nalpha, const double *alpha, int idir, const int64_t *line_label, const int64_t *line_label2,
                                   const double *x2) {
    return set_projection(op, "nlg_linop_set_projection_lanes", nalpha, alpha, true, idir, line_label, line_label2, x2);
}

// nlg_linop_project / nlg_linop_project_block after their own checks: the vectors through the lanes 0 .. s-1 of the slab
static int project_vecs(nlg_linop *op, int s, nlg_vec *const *v) {
    NLG_TRY(slab_ensure(op, s));
    for (int l = 0; l < s; ++l) NLG_TRY(load_state(op, l, v[l], 0));
    NLG_TRY(project_alpha(op, s, 0, (1u << s) - 1u));
    for (int l = 0; l < s; ++l) NLG_TRY(store_state(op, l, v[l], 0));
    return 0;
}

int nlg_linop_project_block(nlg_linop *op, int s, nlg_vec *const *v) {
    NLG_CHECK(op && v, "nlg_linop_project_block: NULL argument");
    NLG_CHECK(op->proj_lanes > 0, "nlg_linop_project_block: the operator has no wavenumber lanes (nlg_linop_set_projection_lanes)");
    NLG_CHECK(s >= 1 && s <= op->proj_lanes, "nlg_linop_project_block: %d vectors on an operator with %d wavenumber lanes", s, op->proj_lanes);
    NLG_NO_OTD(op, "nlg_linop_project_block");
    for (int l = 0; l < s; ++l) {
        NLG_CHECK(v[l] && v[l]->mesh == op->mesh, "nlg_linop_project_block: vector %d NULL or on a different mesh", l);
        for (int u = 0; u < l; ++u) NLG_CHECK(v[l] != v[u], "nlg_linop_project_block: the same vector twice");
    }
    return project_vecs(op, s, v);
}

int nlg_linop_project(nlg_linop *op, nlg_vec *v) {
    NLG_CHECK(op && v && v->mesh == op->mesh, "nlg_linop_project: bad argument");
    NLG_CHECK(op->proj_v.nlines > 0, "nlg_linop_project: no projection set (nlg_linop_set_projection)");
    return project_vecs(op, 1, &v);   // (wavenumber lanes: alpha[0])
}

int nlg_linop_set_tolerances(nlg_linop *op, double vtol, double ptol) {
    NLG_CHECK(op && vtol > 0.0 && ptol > 0.0, "nlg_linop_set_tolerances: bad argument");
    NLG_NO_OTD(op, "nlg_linop_set_tolerances");
    op->cfg.vtol = vtol;
    op->cfg.ptol = ptol;
    return 0;
}

int nlg_linop_set_tau(nlg_linop *op, double tau) {
    NLG_CHECK(op && tau > 0.0, "nlg_linop_set_tau: bad argument");
    NLG_NO_OTD(op, "nlg_linop_set_tau");
    NLG_CHECK(!op->orbit || tau == op->cfg.tau, "nlg_linop_set_tau: in orbit mode tau is the period; set it with nlg_linop_set_orbit");
    if (tau != op->cfg.tau) {
        op->cfg.tau = tau;
        if (op->inited) return nlg_linop_init(op);
    }
    return 0;
}

// Coupled (orbit) mode, see do_matvec_block.  X0 becomes the operator's base flow (dt / nsteps by the usual rule applied to it, the
// preconditioners for that dt); the fine-mesh factors of the convective term are rebuilt every step from the base-flow lane, and from
// X0 again when the mode is left.
int nlg_linop_set_orbit(nlg_linop *op, const nlg_vec *X0, double period) {
    NLG_CHECK(op, "nlg_linop_set_orbit: NULL operator");
    NLG_NO_OTD(op, "nlg_linop_set_orbit");
    if (!X0) {
        if (!op->orbit) return 0;
        op->orbit = false;
        op->orbit_end_valid = false;
        op->upo_fdot_valid = false;
        op->orbit_nsteps = 0;
        return op->inited ? nlg_linop_init(op) : 0;   // the frozen operator about X0 with tau = period
    }
    NLG_CHECK(X0->mesh == op->mesh, "nlg_linop_set_orbit: X0 lives on a different mesh");
    NLG_CHECK(period > 0.0, "nlg_linop_set_orbit: the period must be positive");
    NLG_CHECK(!op->cfg.ifheat, "nlg_linop_set_orbit: orbit mode does not carry the temperature (cfg.ifheat); not built");
    NLG_CHECK(op->proj_v.nlines == 0, "nlg_linop_set_orbit: orbit mode and the wavenumber projection exclude each other");
    NLG_TRY(nlg_vec_copy(op->baseflow, X0));
    if (!op->orbit_end) NLG_TRY(nlg_vec_clone(op->baseflow, &op->orbit_end));
    for (nlg_vec **f : {&op->upo_f0, &op->upo_fT})
        if (!*f) {
            NLG_TRY(nlg_vec_clone(op->baseflow, f));
            NLG_TRY(nlg_vec_zero(*f));
        }
    op->orbit_end_valid = false;
    op->upo_fdot_valid = false;
    op->orbit_nsteps = 0;
    op->cfg.tau = period;
    op->orbit = true;
    return nlg_linop_init(op);
}

// ---- periodic-orbit Newton (include/neklab_gpu.h; nek_upo_system / nek_upo_jacobian of the reference) ------------------------------
#define NLG_NEED_ORBIT(op, who) NLG_CHECK((op) && (op)->orbit, "%s: %s (nlg_linop_set_orbit)", who, (op) ? "the operator is not in orbit mode" : "NULL operator, one in orbit mode is needed")

int nlg_linop_set_orbit_steps(nlg_linop *op, const nlg_vec *X0, double period, int nsteps) {
    NLG_NEED_ORBIT(op, "nlg_linop_set_orbit_steps");
    NLG_CHECK(X0, "nlg_linop_set_orbit_steps: NULL argument");
    NLG_CHECK(nsteps >= 0, "nlg_linop_set_orbit_steps: nsteps %d is negative (0 = CFL rule / cfg.dt)", nsteps);
    if (nsteps == 0) return nlg_linop_set_orbit(op, X0, period);
    NLG_NO_OTD(op, "nlg_linop_set_orbit_steps");
    NLG_CHECK(X0->mesh == op->mesh, "nlg_linop_set_orbit_steps: X0 lives on a different mesh");
    NLG_CHECK(period > 0.0, "nlg_linop_set_orbit_steps: the period must be positive");
    NLG_TRY(nlg_vec_copy(op->baseflow, X0));
    op->orbit_end_valid = false;
    op->upo_fdot_valid = false;
    op->orbit_nsteps = nsteps;
    op->cfg.tau = period;
    return nlg_linop_init(op);
}

// Phi_T(X0) - X0 with the base-flow lane alone: the nonlinear step from X0 with the operator's dt / nsteps (nonlinear_map_UPO,
// periodic_orbit.f90:4-45; the pressure is differenced as well, vec_out%sub(vec_in))
int nlg_upo_residual(nlg_linop *op, nlg_vec *out) {
    NLG_NEED_ORBIT(op, "nlg_upo_residual");
    NLG_CHECK(out, "nlg_upo_residual: NULL argument");
    NLG_NO_OTD(op, "nlg_upo_residual");
    NLG_CHECK(op->inited, "nlg_upo_residual: nlg_linop_init has not been called");
    nlg_mesh *m = op->mesh;
    NLG_CHECK(out->mesh == m && out->nscal == 0, "nlg_upo_residual: the output lives on a different mesh or carries scalars");
    NLG_TRY(begin_run(op, 1));
    NLG_TRY(load_state(op, 0, op->baseflow, 0));
    Lanes L{op, 1};
    L.nonlinear = 1;
    NLG_TRY(run_steps(L, 0));
    NLG_TRY(nlg_vec_zero(out));
    return state_minus_x0(op, 0, 1.0, out);
}

int nlg_upo_fdot(nlg_linop *op, int which, nlg_vec *out) {
    NLG_NEED_ORBIT(op, "nlg_upo_fdot");
    NLG_CHECK(out, "nlg_upo_fdot: NULL argument");
    NLG_CHECK(which == 0 || which == 1, "nlg_upo_fdot: which = %d (0: f0 at X0, 1: fT at the end of the period)", which);
    NLG_CHECK(op->upo_fdot_valid, "nlg_upo_fdot: no run yet (a matvec in orbit mode or nlg_upo_residual fills the derivatives)");
    nlg_mesh *m = op->mesh;
    NLG_CHECK(out->mesh == m && out->nscal == 0, "nlg_upo_fdot: the output lives on a different mesh or carries scalars");
    return vec_copy_main(out, which == 0 ? op->upo_f0 : op->upo_fT);
}

// The border of the orbit's Jacobian on an existing w = M v_in (jac_direct_map, periodic_orbit.f90:91-103): w <- w - v_in + t_in fT,
// t_out = <f0, v_in>.  Without restart history on either vector it is one pass (upo_border_dev, vec.hip: six streams); with it, the
// vector operations, whose history semantics the result then follows.  composed != 0 forces the vector operations.
int nlg_upo_border(nlg_linop *op, const nlg_vec *v_in, double t_in, nlg_vec *w, double *t_out, int composed) {
    NLG_NEED_ORBIT(op, "nlg_upo_border");
    NLG_CHECK(v_in && w && t_out, "nlg_upo_border: NULL argument");
    NLG_CHECK(op->upo_fdot_valid, "nlg_upo_border: no run yet (a matvec in orbit mode or nlg_upo_residual fills the derivatives)");
    NLG_CHECK(v_in->mesh == op->mesh && w->mesh == op->mesh && v_in->nscal == 0 && w->nscal == 0 && v_in != w,
              "nlg_upo_border: the vectors live on a different mesh, carry scalars or are the same");
    NLG_CHECK(op->upo_fT->nscal == 0, "nlg_upo_border: the operator's base flow carries scalars; orbit mode does not");
    if (!composed && v_in->nrst == 0 && w->nrst == 0) {
        NLG_TRY(upo_border_dev(w, v_in, op->upo_fT, op->upo_f0, t_in, 0));
    } else {
        NLG_TRY(nlg_vec_axpby(-1.0, v_in, 1.0, w));
        NLG_TRY(nlg_vec_axpby(t_in, op->upo_fT, 1.0, w));
        NLG_TRY(dev_dot(v_in, op->upo_f0, 0));
    }
    return scalars_to_host(op->mesh->ctx, 0, 1, t_out);
}

int nlg_upo_jac_matvec(nlg_linop *op, const nlg_vec *v_in, double t_in, nlg_vec *v_out, double *t_out) {
    NLG_NEED_ORBIT(op, "nlg_upo_jac_matvec");
    NLG_CHECK(v_in && v_out && t_out, "nlg_upo_jac_matvec: NULL argument");
    NLG_TRY(do_matvec(op, v_in, v_out, 0));
    return nlg_upo_border(op, v_in, t_in, v_out, t_out, 0);
}

int nlg_linop_orbit_end(nlg_linop *op, nlg_vec *out) {
    NLG_CHECK(op && out && out->mesh == op->mesh, "nlg_linop_orbit_end: bad argument");
    NLG_CHECK(op->orbit, "nlg_linop_orbit_end: the operator is not in orbit mode (nlg_linop_set_orbit)");
    NLG_CHECK(op->orbit_end_valid, "nlg_linop_orbit_end: no matvec in orbit mode yet");
    NLG_CHECK(out->nscal == 0, "nlg_linop_orbit_end: orbit mode carries no scalars");
    return vec_copy_main(out, op->orbit_end);
}

int nlg_linop_lane_iters(const nlg_linop *op, int lane, int istep, int64_t *v_iters, int64_t *p_iters) {
    NLG_CHECK(op && lane >= 0 && lane < kMaxLanes && istep >= 0, "nlg_linop_lane_iters: bad argument");
    if (istep == 0) {
        if (v_iters) *v_iters = op->lane_viters[lane];
        if (p_iters) *p_iters = op->lane_piters[lane];
        return 0;
    }
    // (the per-step counts are the ones the iteration predictor keeps from the last run)
    const LanePred &lp = op->pred[lane];
    NLG_CHECK(istep < (int)lp.v.hist.size() && istep < (int)lp.p.hist.size(), "nlg_linop_lane_iters: lane %d has not run a time step %d", lane, istep);
    if (v_iters) *v_iters = lp.v.hist[istep];
    if (p_iters) *p_iters = lp.p.hist[istep];
    return 0;
}

int nlg_linop_pcg_z_free(const nlg_linop *op, int *out) {
    NLG_CHECK(op && out, "nlg_linop_pcg_z_free: bad argument");
    *out = op->z_free ? 1 : 0;
    return 0;
}

// ---- OTD modes (include/neklab_gpu.h; nek_otd / otd_analysis of the reference) ----------------------------------------------------
int nlg_otd_opts_default(nlg_otd_opts *o) {
    NLG_CHECK(o, "nlg_otd_opts_default: NULL");
    o->r = 2;
    o->startstep = 1;
    o->orthostep = 10;
    o->trans = 0;
    o->solve_baseflow = 0;
    return 0;
}

static int otd_check_flag(nlg_otd *ot, const char *who) {
    double flag = 0.0;
    hipStream_t st = ot->op->mesh->ctx->stream;
    NLG_HIP(hipMemcpyAsync(&flag, ot->d + OTD_FLAG, sizeof(double), hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    NLG_CHECK(flag == 0.0, "%s: the Gram matrix of the OTD basis is not positive definite (dependent or non-finite modes)", who);
    return 0;
}

int nlg_otd_destroy(nlg_otd *ot) {
    if (!ot) return 0;
    hipDeviceSynchronize();
    nlg_linop *op = ot->op;
    const bool live = op && op->otd == ot;
    if (live) op->otd = nullptr;
    if (ot->d) hipFree(ot->d);
    if (ot->part) hipFree(ot->part);
    const bool moved = live && ot->lb >= 0;
    delete ot;
    if (moved) {
        // the base-flow lane rebuilt the fine-mesh factors of the convective term in every step: they belong to the operator's own
        // (frozen) base flow again, so that a later matvec is the one it was before the run
        nlg_mesh *m = op->mesh;
        double *U[3] = {op->baseflow->vel(0), op->baseflow->vel(1), m->dim == 3 ? op->baseflow->vel(2) : nullptr};
        NLG_TRY(sem_conv_setup(m, U, op->Ur, op->GU));
    }
    return 0;
}

int nlg_otd_create(nlg_linop *op, const nlg_otd_opts *o, const nlg_vec *const *basis0, nlg_otd **out) {
    NLG_CHECK(op && o && out, "nlg_otd_create: NULL argument");
    const int rmax = o->solve_baseflow ? kMaxLanes - 1 : kMaxLanes;
    NLG_CHECK(o->r >= 1 && o->r <= rmax, "nlg_otd_create: r = %d out of range (1..%d%s)", o->r, rmax,
              o->solve_baseflow ? ": with solve_baseflow the base flow takes one of the lanes" : "");
    NLG_CHECK(!(o->trans && o->solve_baseflow), "nlg_otd_create: trans with solve_baseflow: the adjoint about a moving base flow needs U(T - t) and is not built");
    NLG_CHECK(!op->cfg.ifheat, "nlg_otd_create: OTD modes do not carry the temperature (cfg.ifheat); not built");
    NLG_CHECK(op->proj_v.nlines == 0, "nlg_otd_create: OTD modes and the wavenumber projection exclude each other");
    NLG_CHECK(!op->orbit, "nlg_otd_create: the operator is in orbit mode (nlg_linop_set_orbit); use solve_baseflow on a frozen operator");
    NLG_CHECK(!op->otd, "nlg_otd_create: an nlg_otd already lives on this operator");
    NLG_CHECK(!op->dns, "nlg_otd_create: an nlg_dns lives on this operator; nlg_dns_destroy it first");
    NLG_CHECK(o->startstep >= 1 && o->orthostep >= 1, "nlg_otd_create: startstep and orthostep must be positive");
    nlg_mesh *m = op->mesh;
    if (basis0)
        for (int v = 0; v < o->r; ++v)
            NLG_CHECK(basis0[v] && basis0[v]->mesh == m && basis0[v]->nscal == 0, "nlg_otd_create: basis vector %d NULL, on a different mesh or with scalars", v);
    if (!op->inited) NLG_TRY(nlg_linop_init(op));
    nlg_otd *ot = new nlg_otd();
    ot->op = op;
    ot->o = *o;
    ot->r = o->r;
    ot->nl = o->r + (o->solve_baseflow ? 1 : 0);
    ot->lb = o->solve_baseflow ? o->r : -1;
    auto fail = [&](int rc) {
        nlg_otd_destroy(ot);
        return rc;
    };
    hipStream_t st = m->ctx->stream;
    if (hipMalloc(&ot->d, sizeof(double) * OTD_N) != hipSuccess || hipMalloc(&ot->part, sizeof(double) * 32 * NB) != hipSuccess) {
        set_error("nlg_otd_create: out of device memory");
        return fail(1);
    }
    int rc = 0;
    if (hipMemsetAsync(ot->d, 0, sizeof(double) * OTD_N, st) != hipSuccess) rc = 1;
    if (!rc) rc = begin_run(op, ot->nl);   // the run goes on across the calls of nlg_otd_advance: op->istep is its time-step index
    for (int v = 0; v < ot->r && !rc; ++v) {
        if (basis0) {
            rc = load_state(op, v, basis0[v], 0);
        } else {   // rand_basis of init_OTD
            nlg_vec *tmp = nullptr;
            rc = nlg_vec_create(m, 0, 1, &tmp);
            if (!rc) rc = nlg_vec_rand(tmp, 1, (uint64_t)(v + 1));
            if (!rc) rc = load_state(op, v, tmp, 0);
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = 1;
            if (tmp) nlg_vec_destroy(tmp);
        }
    }
    if (!rc && ot->lb >= 0) rc = load_state(op, ot->lb, op->baseflow, 0);
    // at creation the basis may be far from orthonormal: twice
    if (!rc) rc = otd_orthonormalise(ot);
    if (!rc) rc = otd_orthonormalise(ot);
    if (!rc) rc = otd_check_flag(ot, "nlg_otd_create");
    if (rc) return fail(rc);
    op->otd = ot;
    *out = ot;
    return 0;
}

int nlg_otd_advance(nlg_otd *ot, int nsteps) {
    NLG_CHECK(ot && nsteps >= 0, "nlg_otd_advance: bad argument");
    nlg_linop *op = ot->op;
    Lanes L{op, ot->nl, ot->lb};
    L.adjoint = ot->o.trans ? 1 : 0;
    bool ortho = false;
    for (int s = 0; s < nsteps; ++s) {
        NLG_TRY(advance(L));
        ot->time += op->dt;
        const int is = op->istep, s0 = ot->o.startstep;
        if (is >= s0 && (is <= s0 + 10 || is % ot->o.orthostep == 0)) {
            NLG_TRY(otd_orthonormalise(ot));
            ortho = true;
        }
    }
    // a Gram matrix that was not positive definite left T = I: say so here, not at the next read-out (one small copy per call)
    if (ortho) NLG_TRY(otd_check_flag(ot, "nlg_otd_advance"));
    return 0;
}

int nlg_otd_reduced(nlg_otd *ot, double *Lr, double *G) {
    NLG_CHECK(ot && Lr, "nlg_otd_reduced: NULL argument");
    nlg_linop *op = ot->op;
    nlg_mesh *m = op->mesh;
    hipStream_t st = m->ctx->stream;
    const int dim = m->dim, r = ot->r;
    const int64_t ld = r > 1 ? op->slab_ld : 0;
    NLG_TRY(otd_orthonormalise(ot));
    // L u_j in weak form from the operators of the time step, on the state as it stands (h2 = 0: the viscous term alone)
    NLG_TRY(sem_ortho(m, op->p, r, ld));
    if (ot->lb >= 0) NLG_TRY(sem_conv_setup(m, at_lane3(op, op->ubuf[0], ot->lb).p, op->Ur, op->GU));
    NLG_TRY(sem_conv_apply(m, op->Ur, op->GU, op->ubuf[0], op->rhs, ot->o.trans ? 1 : 0, r, ld));
    NLG_TRY(sem_opgradt(m, op->p, op->gp, false, nullptr, nullptr, r, ld, ld));
    NLG_TRY(sem_axhelm(m, op->ubuf[0], op->w, dim, 1.0 / op->cfg.re, 0.0, nullptr, nullptr, nullptr, nullptr, false, r, ld));
    NLG_TRY(otd_sums(ot, op->gp, op->w, op->rhs));
    NLG_LAUNCH(k_otd_coef, dim3(1), dim3(1), 0, st, ot->d, r, 0.0);
    double h[OTD_N];
    NLG_HIP(hipMemcpyAsync(h, ot->d, sizeof(double) * OTD_N, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    NLG_CHECK(h[OTD_FLAG] == 0.0, "nlg_otd_reduced: the Gram matrix of the OTD basis is not positive definite (dependent or non-finite modes)");
    for (int q = 0; q < r * r; ++q) {
        Lr[q] = h[OTD_LR + q];
        if (G) G[q] = h[OTD_G0 + q];
    }
    return 0;
}

int nlg_otd_get_basis(nlg_otd *ot, int i, nlg_vec *out) {
    NLG_CHECK(ot && out && out->mesh == ot->op->mesh && out->nscal == 0, "nlg_otd_get_basis: bad argument");
    NLG_CHECK(i >= 0 && i < ot->r, "nlg_otd_get_basis: mode %d out of range (0..%d)", i, ot->r - 1);
    NLG_TRY(nlg_vec_zero(out));
    return store_state(ot->op, i, out, 0);
}

int nlg_otd_get_baseflow(nlg_otd *ot, nlg_vec *out) {
    NLG_CHECK(ot && out && out->mesh == ot->op->mesh && out->nscal == 0, "nlg_otd_get_baseflow: bad argument");
    if (ot->lb < 0) return vec_copy_main(out, ot->op->baseflow);
    NLG_TRY(nlg_vec_zero(out));
    return store_state(ot->op, ot->lb, out, 0);
}

int nlg_otd_info(const nlg_otd *ot, int64_t *istep, double *time, double *dt) {
    NLG_CHECK(ot, "nlg_otd_info: NULL");
    if (istep) *istep = ot->op->istep;
    if (time) *time = ot->time;
    if (dt) *dt = ot->op->dt;
    return 0;
}

// ---- DNS runs with history points and a recurrence monitor (include/neklab_gpu.h; examples/cylinder/dns of the reference) ----------
int nlg_dns_opts_default(nlg_dns_opts *o) {
    NLG_CHECK(o, "nlg_dns_opts_default: NULL");
    o->chunk = 256;
    return 0;
}

// the ring goes to the host series: one all-reduce over its filled part (history points and dist2 together), one copy
static int dns_flush(nlg_dns *d) {
    if (d->fill == 0) return 0;
    nlg_mesh *m = d->op->mesh;
    hipStream_t st = m->ctx->stream;
    const int64_t cnt = d->fill * d->slot_len, np = d->np;
    NLG_CHECK(cnt < ((int64_t)1 << 31), "nlg_dns: a ring of %lld values is too long for one all-reduce; use a smaller chunk", (long long)cnt);
    NLG_TRY(allreduce_sum(m->ctx, d->ring, (int)cnt));
    std::vector<double> h((size_t)cnt);
    NLG_HIP(hipMemcpyAsync(h.data(), d->ring, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipMemsetAsync(d->ring, 0, sizeof(double) * (size_t)cnt, st));   // slots of points another rank owns are never written
    NLG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < d->fill; ++k) {
        const double *s = h.data() + k * d->slot_len;
        d->probe.insert(d->probe.end(), s, s + np);
        d->dist2.push_back(s[np]);
        d->force.insert(d->force.end(), s + np + 1, s + np + 1 + d->nforce);
    }
    d->fill = 0;
    return 0;
}

// one sample of the state as it stands: at most three launches, two more with wall forces; nothing waits for the device
static int dns_sample(nlg_dns *d) {
    nlg_linop *op = d->op;
    nlg_mesh *m = op->mesh;
    const int dim = m->dim;
    if (d->fill == d->o.chunk) NLG_TRY(dns_flush(d));
    double *slot = d->ring + d->fill * d->slot_len;
    if (d->probes) {
        ProbeFields F;
        memset(&F, 0, sizeof(F));
        F.nf = d->nf;
        F.mesh2 = dim;
        for (int c = 0; c < dim; ++c) F.f[0][c] = op->ubuf[0][c];
        F.f[0][dim] = op->p;
        if (op->cfg.ifheat) F.f[0][dim + 1] = op->tbuf[0];
        NLG_TRY(probes_sample(d->probes, 1, F, slot));
    }
    if (d->ref) {
        const double *u[4] = {}, *r[4] = {};
        for (int c = 0; c < dim; ++c) u[c] = op->ubuf[0][c], r[c] = d->ref->vel(c);
        if (op->cfg.ifheat) u[dim] = op->tbuf[0], r[dim] = d->ref->theta(0);
        NLG_TRY(recur_dist2(m, dim + (op->cfg.ifheat ? 1 : 0), u, r, d->part, slot + d->np));
    }
    if (d->forces) {
        ForceFields F;
        memset(&F, 0, sizeof(F));
        for (int c = 0; c < dim; ++c) F.u[0][c] = op->ubuf[0][c];
        F.p[0] = op->p;
        if (op->cfg.ifheat) F.th[0] = op->tbuf[0];
        NLG_TRY(forces_sample(d->forces, 1, F, 1.0 / op->cfg.re, slot + d->np + 1, d->nforce));
    }
    d->time.push_back(op->istep * op->dt);
    d->fill += 1;
    return 0;
}

// the monitors changed: the series starts again, with the state as it stands as its sample 0
static int dns_restart_series(nlg_dns *d) {
    hipStream_t st = d->op->mesh->ctx->stream;
    NLG_HIP(hipStreamSynchronize(st));
    (void)hipFree(d->ring);
    d->ring = nullptr;
    d->np = d->probes ? d->probes->npts * d->nf : 0;
    d->nforce = d->forces ? (int64_t)d->forces->nobj * d->forces->nq : 0;
    d->slot_len = d->np + 1 + d->nforce;
    NLG_HIP(hipMalloc(&d->ring, sizeof(double) * (size_t)(d->o.chunk * d->slot_len)));
    NLG_HIP(hipMemsetAsync(d->ring, 0, sizeof(double) * (size_t)(d->o.chunk * d->slot_len), st));
    d->fill = 0;
    d->started = false;
    d->time.clear(), d->probe.clear(), d->dist2.clear(), d->force.clear();
    return 0;
}

int nlg_dns_destroy(nlg_dns *d) {
    if (!d) return 0;
    hipDeviceSynchronize();
    nlg_linop *op = d->op;
    const bool live = op && op->dns == d;
    if (live) op->dns = nullptr;
    if (d->probes) d->probes->attached -= 1;
    if (d->forces) d->forces->attached -= 1;
    if (d->ref) nlg_vec_destroy(d->ref);
    (void)hipFree(d->ring);
    (void)hipFree(d->part);
    delete d;
    if (live) {
        // the run rebuilt the fine-mesh factors of the convective term in every step: they belong to the operator's base flow (X0)
        // again, so that a later matvec is the propagator about X0
        nlg_mesh *m = op->mesh;
        double *U[3] = {op->baseflow->vel(0), op->baseflow->vel(1), m->dim == 3 ? op->baseflow->vel(2) : nullptr};
        NLG_TRY(sem_conv_setup(m, U, op->Ur, op->GU));
        if (op->cfg.ifheat) NLG_TRY(sem_conv_scalar_setup(m, op->baseflow->theta(0), op->GT));
    }
    return 0;
}

int nlg_dns_create(nlg_linop *op, const nlg_vec *X0, const nlg_dns_opts *o, nlg_dns **out) {
    NLG_CHECK(op && X0 && o && out, "nlg_dns_create: NULL argument");
    NLG_CHECK(o->chunk >= 1, "nlg_dns_create: chunk = %d must be positive", o->chunk);
    NLG_CHECK(!op->orbit, "nlg_dns_create: the operator is in orbit mode (nlg_linop_set_orbit) and holds X0 as its base flow; use a second operator");
    NLG_CHECK(!op->otd, "nlg_dns_create: an nlg_otd lives on this operator");
    NLG_CHECK(!op->dns, "nlg_dns_create: an nlg_dns already lives on this operator");
    NLG_CHECK(op->proj_v.nlines == 0, "nlg_dns_create: a DNS run and the wavenumber projection exclude each other");
    nlg_mesh *m = op->mesh;
    NLG_CHECK(X0->mesh == m, "nlg_dns_create: X0 lives on a different mesh");
    NLG_CHECK(X0->nscal == (op->cfg.ifheat ? 1 : 0), "nlg_dns_create: X0 carries %d scalar(s), the operator expects %d (cfg.ifheat)", X0->nscal,
              op->cfg.ifheat ? 1 : 0);
    // the time step follows X0 (cfg.dt, or the CFL rule at X0), as in nonlinear_map, and then stays
    NLG_TRY(nlg_vec_copy(op->baseflow, X0));
    NLG_TRY(nlg_linop_init(op));
    nlg_dns *d = new nlg_dns();
    d->op = op;
    d->o = *o;
    d->nf = m->dim + 1 + (op->cfg.ifheat ? 1 : 0);
    int rc = hipMalloc(&d->part, sizeof(double) * kRecurBlocks) == hipSuccess ? 0 : 1;
    if (rc) set_error("nlg_dns_create: out of device memory");
    if (!rc) rc = dns_restart_series(d);
    if (!rc) rc = begin_run(op, 1);   // the run goes on across the calls of nlg_dns_advance: op->istep is its time-step index
    if (!rc) rc = load_state(op, 0, X0, 0);
    if (rc) {
        nlg_dns_destroy(d);
        return rc;
    }
    op->dns = d;
    *out = d;
    return 0;
}

int nlg_dns_set_probes(nlg_dns *d, nlg_probes *p) {
    NLG_CHECK(d, "nlg_dns_set_probes: NULL");
    NLG_CHECK(!p || p->mesh == d->op->mesh, "nlg_dns_set_probes: the history points were located on a different mesh");
    if (d->probes) d->probes->attached -= 1;
    d->probes = p;
    if (p) p->attached += 1;
    return dns_restart_series(d);
}

int nlg_dns_set_forces(nlg_dns *d, nlg_forces *f) {
    NLG_CHECK(d, "nlg_dns_set_forces: NULL");
    NLG_CHECK(!f || f->mesh == d->op->mesh, "nlg_dns_set_forces: the faces were listed on a different mesh");
    if (d->forces) d->forces->attached -= 1;
    d->forces = f;
    if (f) f->attached += 1;
    return dns_restart_series(d);
}

int nlg_dns_set_reference(nlg_dns *d, const nlg_vec *ref) {
    NLG_CHECK(d, "nlg_dns_set_reference: NULL");
    nlg_linop *op = d->op;
    NLG_CHECK(!ref || (ref->mesh == op->mesh && ref->nscal == (op->cfg.ifheat ? 1 : 0)), "nlg_dns_set_reference: the reference lives on another mesh or carries other scalars");
    if (!d->ref) NLG_TRY(nlg_vec_create(op->mesh, op->cfg.ifheat ? 1 : 0, 1, &d->ref));
    if (ref) {
        NLG_TRY(vec_copy_main(d->ref, ref));
        if (op->cfg.ifheat)
            NLG_HIP(hipMemcpyAsync(d->ref->theta(0), ref->theta(0), sizeof(double) * (size_t)op->mesh->lvn, hipMemcpyDeviceToDevice, op->mesh->ctx->stream));
    } else {
        NLG_TRY(store_state(op, 0, d->ref, 0));
    }
    return dns_restart_series(d);
}

int nlg_dns_advance(nlg_dns *d, int nsteps) {
    NLG_CHECK(d && nsteps >= 0, "nlg_dns_advance: bad argument");
    nlg_linop *op = d->op;
    Lanes L{op, 1};
    L.nonlinear = 1;
    if (!d->started) {
        NLG_TRY(dns_sample(d));
        d->started = true;
    }
    for (int s = 0; s < nsteps; ++s) {
        NLG_TRY(advance(L));
        NLG_TRY(dns_sample(d));
    }
    return 0;
}

int nlg_dns_count(const nlg_dns *d, int64_t *nsamples) {
    NLG_CHECK(d && nsamples, "nlg_dns_count: NULL argument");
    *nsamples = (int64_t)d->time.size();
    return 0;
}

int nlg_dns_series(nlg_dns *d, int64_t first, int64_t count, double *time, double *probe, double *dist) {
    NLG_CHECK(d, "nlg_dns_series: NULL");
    NLG_TRY(nlg_dns_advance(d, 0));   // sample 0, if nothing has been taken yet
    NLG_TRY(dns_flush(d));
    NLG_CHECK(first >= 0 && count >= 0 && first + count <= (int64_t)d->time.size(), "nlg_dns_series: samples %lld .. %lld out of range (%lld taken)",
              (long long)first, (long long)(first + count), (long long)d->time.size());
    const int64_t np = d->np;
    for (int64_t k = 0; k < count; ++k) {
        if (time) time[k] = d->time[first + k];
        if (dist) dist[k] = d->ref ? std::sqrt(std::max(d->dist2[first + k], 0.0)) : 0.0;
    }
    if (probe && np > 0) memcpy(probe, d->probe.data() + first * np, sizeof(double) * (size_t)(count * np));
    return 0;
}

int nlg_dns_force_series(nlg_dns *d, int64_t first, int64_t count, double *force) {
    NLG_CHECK(d && force, "nlg_dns_force_series: NULL argument");
    NLG_CHECK(d->forces, "nlg_dns_force_series: no wall forces are attached (nlg_dns_set_forces)");
    NLG_TRY(nlg_dns_advance(d, 0));
    NLG_TRY(dns_flush(d));
    NLG_CHECK(first >= 0 && count >= 0 && first + count <= (int64_t)d->time.size(), "nlg_dns_force_series: samples %lld .. %lld out of range (%lld taken)",
              (long long)first, (long long)(first + count), (long long)d->time.size());
    if (count > 0) memcpy(force, d->force.data() + first * d->nforce, sizeof(double) * (size_t)(count * d->nforce));
    return 0;
}

int nlg_dns_get_state(nlg_dns *d, nlg_vec *out) {
    NLG_CHECK(d && out && out->mesh == d->op->mesh && out->nscal == (d->op->cfg.ifheat ? 1 : 0), "nlg_dns_get_state: bad argument");
    NLG_TRY(clear_for_store(out, 0));
    return store_state(d->op, 0, out, 0);
}

int nlg_dns_info(const nlg_dns *d, int64_t *istep, double *time, double *dt) {
    NLG_CHECK(d, "nlg_dns_info: NULL");
    if (istep) *istep = d->op->istep;
    if (time) *time = d->op->istep * d->op->dt;
    if (dt) *dt = d->op->dt;
    return 0;
}

int nlg_linop_get_info(const nlg_linop *op, double *tau, double *dt, int *nsteps, double *cfl) {
    NLG_CHECK(op, "nlg_linop_get_info: NULL");
    if (tau) *tau = op->cfg.tau;
    if (dt) *dt = op->dt;
    if (nsteps) *nsteps = op->nsteps;
    if (cfl) *cfl = op->cfl;
    return 0;
}

int nlg_linop_get_stats(const nlg_linop *op, int64_t *steps, int64_t *v_iters, int64_t *p_iters, int64_t *matvecs) {
    NLG_CHECK(op, "nlg_linop_get_stats: NULL");
    if (steps) *steps = op->st_steps;
    if (v_iters) *v_iters = op->st_viters;
    if (p_iters) *p_iters = op->st_piters;
    if (matvecs) *matvecs = op->st_matvecs;
    return 0;
}

int nlg_op_conv(nlg_mesh *m, const nlg_vec *base, const nlg_vec *in, nlg_vec *out, int adjoint) {
    NLG_CHECK(m && base && in && out && base->mesh == m && in->mesh == m && out->mesh == m, "nlg_op_conv: bad arguments");
    const int dim = m->dim;
    double *Ur[3] = {}, *GU[9] = {};
    for (int c = 0; c < dim; ++c) NLG_HIP(hipMalloc(&Ur[c], sizeof(double) * (size_t)m->lfn));
    for (int q = 0; q < dim * dim; ++q) NLG_HIP(hipMalloc(&GU[q], sizeof(double) * (size_t)m->lfn));
    double *U[3] = {base->vel(0), base->vel(1), dim == 3 ? base->vel(2) : nullptr};
    double *u[3] = {in->vel(0), in->vel(1), dim == 3 ? in->vel(2) : nullptr};
    double *o[3] = {out->vel(0), out->vel(1), dim == 3 ? out->vel(2) : nullptr};
    int rc = sem_conv_setup(m, U, Ur, GU);
    if (!rc) rc = sem_conv_apply(m, Ur, GU, u, o, adjoint);
    hipStreamSynchronize(m->ctx->stream);
    for (int c = 0; c < dim; ++c) hipFree(Ur[c]);
    for (int q = 0; q < dim * dim; ++q) hipFree(GU[q]);
    return rc;
}

// The convective terms as the time stepper launches them (adv_a, heat_step): s vectors as lanes of ONE buffer [s][nc][lvs] (components
// lvs apart, lanes ld = nc * lvs apart), one sem_conv_apply / sem_conv_scalar_apply / sem_scalar_grad_apply call with (s, ld).  nc = dim
// (velocity term) or dim + 1 (temperature term: the scalar behind the velocity).  The callers own the three buffers.
static int op_conv_lanes_run(nlg_mesh *m, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint, bool scalar,
                             double *fine, double *bin, double *bout) {
    const int dim = m->dim, nc = dim + (scalar ? 1 : 0);
    const int64_t ld = (int64_t)nc * m->lvs;
    hipStream_t st = m->ctx->stream;
    double *Ur[3] = {}, *GU[9] = {}, *GT[3] = {};
    for (int c = 0; c < dim; ++c) Ur[c] = fine + (int64_t)c * m->lfn;
    for (int q = 0; q < dim * dim; ++q) GU[q] = fine + (int64_t)(dim + q) * m->lfn;
    for (int c = 0; c < dim; ++c) GT[c] = fine + (int64_t)(dim + dim * dim + c) * m->lfn;
    double *U[3] = {base->vel(0), base->vel(1), dim == 3 ? base->vel(2) : nullptr};
    NLG_TRY(sem_conv_setup(m, U, Ur, GU));
    if (scalar) NLG_TRY(sem_conv_scalar_setup(m, base->theta(0), GT));
    // vel(0) .. theta(0) of a vector are consecutive fields lvs apart: one copy per lane
    for (int v = 0; v < s; ++v) NLG_HIP(hipMemcpyAsync(bin + v * ld, in[v]->vel(0), sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, st));
    NLG_HIP(hipMemsetAsync(bout, 0, sizeof(double) * (size_t)(s * ld), st));
    double *u[3] = {}, *o[3] = {};
    for (int c = 0; c < dim; ++c) u[c] = bin + (int64_t)c * m->lvs, o[c] = bout + (int64_t)c * m->lvs;
    const int64_t lds = s > 1 ? ld : 0;   // the stride the stepper passes (Lanes::ld)
    if (!scalar) {
        NLG_TRY(sem_conv_apply(m, Ur, GU, u, o, adjoint, s, lds));
    } else {
        NLG_TRY(sem_conv_scalar_apply(m, Ur, GT, u, bin + (int64_t)dim * m->lvs, bout + (int64_t)dim * m->lvs, adjoint, s, lds));
        NLG_TRY(sem_scalar_grad_apply(m, GT, bin + (int64_t)dim * m->lvs, o, 1.0, s, lds));   // onto the zeros of the memset
    }
    // the points of the nc fields only: the padding behind a field of out[v] and its pressure are not written
    for (int v = 0; v < s; ++v)
        for (int c = 0; c < nc; ++c)
            NLG_HIP(hipMemcpyAsync(out[v]->vel(0) + (int64_t)c * m->lvs, bout + v * ld + (int64_t)c * m->lvs, sizeof(double) * (size_t)m->lvn,
                                   hipMemcpyDeviceToDevice, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

static int op_conv_lanes(const char *name, nlg_mesh *m, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint,
                         bool scalar) {
    NLG_CHECK(m && base && in && out, "%s: NULL argument", name);
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "%s: s = %d out of range (1 to %d)", name, s, kMaxLanes);
    NLG_CHECK(base->mesh == m, "%s: the base flow lives on another mesh", name);
    NLG_CHECK(!scalar || base->nscal >= 1, "%s: the base flow carries no scalar", name);
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(in[v] && out[v], "%s: vector %d is NULL", name, v);
        NLG_CHECK(in[v]->mesh == m && out[v]->mesh == m, "%s: vector %d lives on another mesh", name, v);
        NLG_CHECK(!scalar || (in[v]->nscal >= 1 && out[v]->nscal >= 1), "%s: vector %d carries no scalar", name, v);
    }
    const int dim = m->dim, nc = dim + (scalar ? 1 : 0);
    nlg::DevBuf<> fine, bin, bout;
    int rc = 1;
    if (hipMalloc(&fine.p, sizeof(double) * (size_t)(dim * dim + 2 * dim) * m->lfn) == hipSuccess &&
        hipMalloc(&bin.p, sizeof(double) * (size_t)s * nc * m->lvs) == hipSuccess &&
        hipMalloc(&bout.p, sizeof(double) * (size_t)s * nc * m->lvs) == hipSuccess)
        rc = op_conv_lanes_run(m, base, s, in, out, adjoint, scalar, fine.p, bin.p, bout.p);
    else
        nlg::set_error("%s: out of device memory", name);
    if (rc) hipStreamSynchronize(m->ctx->stream);   // nothing in flight may still use the buffers
    return rc;
}

int nlg_op_conv_lanes(nlg_mesh *m, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint) {
    return op_conv_lanes("nlg_op_conv_lanes", m, base, s, in, out, adjoint, false);
}

int nlg_op_conv_scalar(nlg_mesh *m, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint) {
    return op_conv_lanes("nlg_op_conv_scalar", m, base, s, in, out, adjoint, true);
}

// the copies in, the launch and the copies out of nlg_op_filter; its caller owns (and frees) the two buffers whatever this returns
static int op_filter_run(nlg_mesh *m, int nvec, nlg_vec *const *vecs, const std::vector<double> &filt, double *dF, double *buf) {
    // the kernel takes lanes as a stride: the fields of the vectors go through one buffer [nvec][ncomp][lvs]
    const int nc = vecs[0]->ncomp;
    const int64_t ld = (int64_t)nc * m->lvs;
    hipStream_t st = m->ctx->stream;
    NLG_HIP(hipMemcpyAsync(dF, filt.data(), sizeof(double) * filt.size(), hipMemcpyHostToDevice, st));
    for (int v = 0; v < nvec; ++v)
        NLG_HIP(hipMemcpyAsync(buf + v * ld, vecs[v]->vel(0), sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, st));
    double *f[4] = {};
    for (int c = 0; c < nc; ++c) f[c] = buf + (int64_t)c * m->lvs;
    NLG_TRY(sem_filter(m, dF, f, nc, nvec, ld));
    for (int v = 0; v < nvec; ++v)
        NLG_HIP(hipMemcpyAsync(vecs[v]->vel(0), buf + v * ld, sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

int nlg_op_filter(nlg_mesh *m, int nvec, nlg_vec *const *vecs, double filter_weight, int filter_modes) {
    NLG_CHECK(m && vecs && nvec >= 1 && nvec <= kMaxLanes, "nlg_op_filter: bad arguments");
    for (int v = 0; v < nvec; ++v)
        NLG_CHECK(vecs[v] && vecs[v]->mesh == m && vecs[v]->ncomp == vecs[0]->ncomp && vecs[v]->ncomp <= 4, "nlg_op_filter: vector %d NULL, on another mesh or of another shape", v);
    NLG_CHECK(filter_weight >= 0.0 && filter_weight <= 1.0, "nlg_op_filter: filter_weight %g outside [0, 1]", filter_weight);
    std::vector<double> filt;
    NLG_TRY(sem_filter_matrix(m, filter_modes, filter_weight, filt));
    double *dF = nullptr, *buf = nullptr;
    int rc = 1;
    if (hipMalloc(&dF, sizeof(double) * filt.size()) == hipSuccess &&
        hipMalloc(&buf, sizeof(double) * (size_t)vecs[0]->ncomp * m->lvs * nvec) == hipSuccess)
        rc = op_filter_run(m, nvec, vecs, filt, dF, buf);
    else
        nlg::set_error("nlg_op_filter: out of device memory");
    if (rc) hipStreamSynchronize(m->ctx->stream);   // nothing in flight may still use the buffers
    if (dF) hipFree(dF);
    if (buf) hipFree(buf);
    return rc;
}

}  // extern "C"
