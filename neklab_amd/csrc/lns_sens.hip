// Eigenvalue sensitivity on the GPU (gfx950): the wavemaker and the base-flow gradient of an eigenvalue from a direct / adjoint pair,
// element-local, pointwise (gradm1: no mass, no gather-scatter, no halo).  Definitions: include/neklab_gpu.h (nlg_sens_apply);
// tests/sens_ref.py restates them in numpy.  A file of its own beside lns_strong.hip, whose LnsGeom, LnsShape and lns_grad it shares
// through lns_elem.h: compiled in one translation unit with k_lns_strong, that kernel's register allocation changed.
#include <algorithm>
#include <cmath>

#include "internal.h"
#include "lns_elem.h"

using namespace nlg;

namespace {

// For real velocity fields u, a on mesh 1, u~ = mask u, a~ = mask a, d_j the pointwise physical derivative (gradm1):
//   T(u, a)_j = - sum_i a~_i d_j u~_i   (transport part)     P(u, a)_j = + sum_i u~_i d_i a~_j   (production part)     S = T + P
// and for a complex pair u^ = u_r + i u_i, u^+ = a_r + i a_i:
//   S_re = S(u_r, a_r) + S(u_i, a_i),  S_im = S(u_i, a_r) - S(u_r, a_i)  (the same split for T),  out = (S_re + i S_im) * (sr + i si),
//   W = |u^~| |u^+~| |sr + i si|.   The term (div u) a_j is left out on purpose: the modes are solenoidal.
// The fields of a pair come as pointers (component 0; component c is c * fs doubles behind), so that vectors of a basis and vectors of
// their own take the same path.  di / ai null: a real pair.  A null output is neither computed nor stored (uniform branches).
struct SensArgs {
    const double *dr[kMaxLanes], *di[kMaxLanes], *ar[kMaxLanes], *ai[kMaxLanes];
    double *gr[kMaxLanes], *gi[kMaxLanes], *tr[kMaxLanes], *ti[kMaxLanes], *w[kMaxLanes];
    double sr[kMaxLanes], si[kMaxLanes], sw[kMaxLanes];   // 1 / d and its modulus
};

// entry c of a register array of DIM, c known only at run time
template <int DIM>
__device__ __forceinline__ double lns_pick(const double *a, int c) {
    double x = a[0];
#pragma unroll
    for (int i = 1; i < DIM; ++i) x = c == i ? a[i] : x;
    return x;
}

// k_lns_sens<N, DIM>: the block and thread layout of k_lns_strong, the pairs of a call in a loop inside the block, rst, jac and the masks
// read once per element for all of them.  Per pair each of the 4 dim (real pair: 2 dim) masked fields goes through LDS once; its
// gradient at the thread's point is consumed at once -- a direct component's into T weighted by the adjoint values at the point, an
// adjoint component's into P weighted by the direct values -- and no gradient is kept.  Two LDS field buffers taken in turn: the
// barrier after the fill of one also ends the reads of the other, ONE barrier per field.  The direct values stay in registers from
// their fill to the production part; the adjoint weights are read again at the point (from cache) instead of being held.
// Algorithmic bytes per point and complex pair (3-D, all outputs): 96 (in) + 96 (grad, transport) + 8 (W); shared by the pairs: 72 (rst)
// + 8 (jac) + 24 (masks).  Flops per point and field: 2 N DIM + 2 DIM^2 for the gradient, 4 DIM for the accumulation.
template <int N, int DIM>
__global__ __launch_bounds__((LnsShape<N, DIM>::NT), (LnsShape<N, DIM>::MINW)) void k_lns_sens(LnsGeom G, const double *__restrict__ Dt, SensArgs A,
                                                                                            int64_t fs, int np) {
    using S = LnsShape<N, DIM>;
    constexpr int NP = S::NP, NT = S::NT, PPT = S::PPT, NQ = N + 1;
    constexpr int NB = DIM == 3 ? NQ * N * N : NQ * N;
    constexpr int CU = PPT > 1 ? 1 : DIM;   // unroll count of the component loops
    __shared__ double sDt[N * N];
    __shared__ double sF[2][NB];
    const int t = threadIdx.x;
    const int64_t eb = (int64_t)blockIdx.x * NP;
    for (int q = t; q < N * N; q += NT) sDt[q] = Dt[q];

    int pq[PPT], pl[PPT], pi[PPT], pj[PPT], pk[PPT];
    bool act[PPT];
    double rs[PPT][DIM * DIM], jinv[PPT], mk[PPT][DIM];
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int q = t + r * NT;
        act[r] = q < NP;
        const int qq = act[r] ? q : 0;
        pq[r] = qq;
        pi[r] = qq % N;
        pj[r] = (qq / N) % N;
        pk[r] = DIM == 3 ? qq / (N * N) : 0;
        pl[r] = pi[r] + NQ * (pj[r] + N * pk[r]);
#pragma unroll
        for (int a = 0; a < DIM * DIM; ++a) rs[r][a] = G.rst[a][eb + qq];
        jinv[r] = 1.0 / G.jac[eb + qq];
#pragma unroll
        for (int c = 0; c < DIM; ++c) mk[r][c] = G.mask[c][eb + qq];
    }

    int buf = 0;
    for (int v = 0; v < np; ++v) {
        const double *din[2] = {A.dr[v], A.di[v]}, *ain[2] = {A.ar[v], A.ai[v]};
        const int nq = din[1] ? 2 : 1;
        const double sr = A.sr[v], si = A.si[v];
        double *gr = A.gr[v], *gi = A.gi[v], *tr = A.tr[v], *ti = A.ti[v], *w = A.w[v];
        double uv[2][PPT][DIM], Ta[2][PPT][DIM], a2[PPT];
#pragma unroll
        for (int r = 0; r < PPT; ++r) {
            a2[r] = 0.0;
#pragma unroll
            for (int c = 0; c < DIM; ++c) uv[0][r][c] = uv[1][r][c] = Ta[0][r][c] = Ta[1][r][c] = 0.0;
        }
        // transport part: gradients of the direct components, weighted by the adjoint values at the point.  The component loops are
        // unrolled at one point per thread; at four (lx1 = 12 in 3-D) they stay loops, the register arrays indexed by selects: unrolled,
        // the loads of all fields are hoisted there and 2348 instead of 720 bytes per lane spill
#pragma unroll(CU)
        for (int c = 0; c < DIM; ++c) {
            auto pass = [&](const int q) __attribute__((always_inline)) {
                const double *f = din[q] + (int64_t)c * fs + eb;
                double *sf = sF[buf];
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    const double val = lns_pick<DIM>(mk[r], c) * f[pq[r]];
#pragma unroll
                    for (int i = 0; i < DIM; ++i) uv[q][r][i] = c == i ? val : uv[q][r][i];
                    if (act[r]) sf[pl[r]] = val;
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    const int64_t o = (int64_t)c * fs + eb + pq[r];
                    const double mc = lns_pick<DIM>(mk[r], c);
                    const double a0 = mc * ain[0][o], a1 = nq == 2 ? mc * ain[1][o] : 0.0;
                    // u_r: T_re -= a_r g, T_im += a_i g;   u_i: T_re -= a_i g, T_im -= a_r g
                    const double wre = q == 0 ? -a0 : -a1, wim = q == 0 ? a1 : -a0;
                    double g[DIM];
                    lns_grad<N, DIM>(sf, sDt, pi[r], pj[r], pk[r], rs[r], jinv[r], g);
#pragma unroll
                    for (int j = 0; j < DIM; ++j) {
                        Ta[0][r][j] = __fma_rn(wre, g[j], Ta[0][r][j]);
                        Ta[1][r][j] = __fma_rn(wim, g[j], Ta[1][r][j]);
                    }
                }
                buf ^= 1;
            };
            pass(0);
            if (nq == 2) pass(1);
        }
        // production part: gradients of the adjoint components, weighted by the direct values at the point; component j of the
        // outputs is complete after the (two) fields of adjoint component j
#pragma unroll(CU)
        for (int j = 0; j < DIM; ++j) {
            double P0[PPT], P1[PPT];
#pragma unroll
            for (int r = 0; r < PPT; ++r) P0[r] = P1[r] = 0.0;
            auto pass = [&](const int q) __attribute__((always_inline)) {
                const double *f = ain[q] + (int64_t)j * fs + eb;
                double *sf = sF[buf];
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    const double val = lns_pick<DIM>(mk[r], j) * f[pq[r]];
                    a2[r] = __fma_rn(val, val, a2[r]);
                    if (act[r]) sf[pl[r]] = val;
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    double g[DIM];
                    lns_grad<N, DIM>(sf, sDt, pi[r], pj[r], pk[r], rs[r], jinv[r], g);
                    double pr = 0.0, pm = 0.0;
#pragma unroll
                    for (int i = 0; i < DIM; ++i) {
                        pr = __fma_rn(uv[0][r][i], g[i], pr);
                        pm = __fma_rn(uv[1][r][i], g[i], pm);
                    }
                    // a_r: P_re += u_r . g, P_im += u_i . g;   a_i: P_re += u_i . g, P_im -= u_r . g
                    P0[r] += q == 0 ? pr : pm;
                    P1[r] += q == 0 ? pm : -pr;
                }
                buf ^= 1;
            };
            pass(0);
            if (nq == 2) pass(1);
#pragma unroll
            for (int r = 0; r < PPT; ++r) {
                if (!act[r]) continue;
                const int64_t o = (int64_t)j * fs + eb + pq[r];
                const double t0 = lns_pick<DIM>(Ta[0][r], j), t1 = lns_pick<DIM>(Ta[1][r], j);
                const double s0 = t0 + P0[r], s1 = t1 + P1[r];
                gr[o] = __fma_rn(-si, s1, __dmul_rn(sr, s0));
                if (gi) gi[o] = __fma_rn(si, s0, __dmul_rn(sr, s1));
                if (tr) tr[o] = __fma_rn(-si, t1, __dmul_rn(sr, t0));
                if (ti) ti[o] = __fma_rn(si, t0, __dmul_rn(sr, t1));
            }
        }
        if (w) {
#pragma unroll
            for (int r = 0; r < PPT; ++r) {
                if (!act[r]) continue;
                double u2 = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) u2 = __fma_rn(uv[1][r][c], uv[1][r][c], __fma_rn(uv[0][r][c], uv[0][r][c], u2));
                w[eb + pq[r]] = sqrt(u2) * sqrt(a2[r]) * A.sw[v];
            }
        }
    }
}

bool lns_supported(int n) { return (n >= 4 && n <= 10) || n == 12; }

template <int N, int DIM>
void sens_launch(nlg_mesh *m, const SensArgs &A, int np) {
    NLG_LAUNCH((k_lns_sens<N, DIM>), dim3((unsigned)m->E), dim3(LnsShape<N, DIM>::NT), 0, m->ctx->stream, lns_geom(m), (const double *)m->d_Dt, A, m->lvs,
               np);
}

// the sensitivity fields of np pairs in ONE launch
int sem_lns_sens(nlg_mesh *m, const SensArgs &A, int np) {
    NLG_CHECK(m->E <= 0x7fffffff, "sem_lns_sens: %lld elements exceed the launch grid", (long long)m->E);
#define NLG_SENS_CASE(N_)                          \
    case N_:                                       \
        if (m->dim == 3)                           \
            sens_launch<N_, 3>(m, A, np);          \
        else                                       \
            sens_launch<N_, 2>(m, A, np);          \
        break;
    switch (m->n) {
        NLG_SENS_CASE(4)
        NLG_SENS_CASE(5)
        NLG_SENS_CASE(6)
        NLG_SENS_CASE(7)
        NLG_SENS_CASE(8)
        NLG_SENS_CASE(9)
        NLG_SENS_CASE(10)
        NLG_SENS_CASE(12)
        default: set_error("sem_lns_sens: unsupported lx1 = %d (built for 4..10, 12)", m->n); return 1;
    }
#undef NLG_SENS_CASE
    NLG_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int nlg_sens_apply(nlg_mesh *m, int s, const nlg_vec *const *dir_re, const nlg_vec *const *dir_im, const nlg_vec *const *adj_re,
                   const nlg_vec *const *adj_im, const double *scale, nlg_vec *const *grad_re, nlg_vec *const *grad_im,
                   nlg_vec *const *transp_re, nlg_vec *const *transp_im, nlg_vec *const *wavemaker) {
    NLG_CHECK(m && dir_re && adj_re && grad_re, "nlg_sens_apply: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_sens_apply: s = %d out of range (1..%d)", s, kMaxLanes);
    NLG_CHECK(lns_supported(m->n), "nlg_sens_apply: unsupported lx1 = %d (built for 4..10, 12)", m->n);
    // the vectors of the call: the inputs first, then the outputs
    const nlg_vec *const *ins[4] = {dir_re, dir_im, adj_re, adj_im};
    nlg_vec *const *outs[5] = {grad_re, grad_im, transp_re, transp_im, wavemaker};
    static const char *const in_name[4] = {"dir_re", "dir_im", "adj_re", "adj_im"};
    static const char *const out_name[5] = {"grad_re", "grad_im", "transp_re", "transp_im", "wavemaker"};
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(dir_re[v] && adj_re[v] && grad_re[v], "nlg_sens_apply: dir_re, adj_re or grad_re of pair %d is NULL", v);
        const bool di = dir_im && dir_im[v], ai = adj_im && adj_im[v];
        NLG_CHECK(di == ai, "nlg_sens_apply: pair %d has %s without %s", v, di ? "dir_im" : "adj_im", di ? "adj_im" : "dir_im");
        for (int a = 0; a < 4; ++a)
            NLG_CHECK(!ins[a] || !ins[a][v] || ins[a][v]->mesh == m, "nlg_sens_apply: %s[%d] lives on another mesh", in_name[a], v);
        for (int b = 0; b < 5; ++b)
            NLG_CHECK(!outs[b] || !outs[b][v] || outs[b][v]->mesh == m, "nlg_sens_apply: %s[%d] lives on another mesh", out_name[b], v);
    }
    for (int b = 0; b < 5; ++b)
        for (int v = 0; v < s; ++v) {
            const nlg_vec *o = outs[b] ? outs[b][v] : nullptr;
            if (!o) continue;
            for (int a = 0; a < 4; ++a)
                for (int w = 0; w < s; ++w) {
                    const nlg_vec *x = ins[a] ? ins[a][w] : nullptr;
                    NLG_CHECK(!x || (o != x && o->d != x->d), "nlg_sens_apply: %s[%d] aliases %s[%d]", out_name[b], v, in_name[a], w);
                }
            for (int c = 0; c < 5; ++c)
                for (int w = 0; w < s; ++w) {
                    const nlg_vec *x = outs[c] ? outs[c][w] : nullptr;
                    NLG_CHECK(!x || (c == b && w == v) || (o != x && o->d != x->d), "nlg_sens_apply: %s[%d] aliases %s[%d]", out_name[b], v,
                              out_name[c], w);
                }
        }
    hipStream_t st = m->ctx->stream;
    SensArgs A = {};
    for (int v = 0; v < s; ++v) {
        A.dr[v] = dir_re[v]->vel(0), A.ar[v] = adj_re[v]->vel(0);
        if (dir_im && dir_im[v]) A.di[v] = dir_im[v]->vel(0), A.ai[v] = adj_im[v]->vel(0);
        A.sr[v] = scale ? scale[2 * v] : 1.0, A.si[v] = scale ? scale[2 * v + 1] : 0.0;
        A.sw[v] = std::hypot(A.sr[v], A.si[v]);
        double **dst[5] = {&A.gr[v], &A.gi[v], &A.tr[v], &A.ti[v], &A.w[v]};
        for (int b = 0; b < 5; ++b) {
            nlg_vec *o = outs[b] ? outs[b][v] : nullptr;
            if (!o) continue;
            *dst[b] = o->vel(0);
            // everything but the velocity of the main block is zero afterwards (the wavemaker: everything but its first component)
            const int64_t keep = b == 4 ? m->lvs : (int64_t)m->dim * m->lvs;
            NLG_HIP(hipMemsetAsync(o->d + keep, 0, sizeof(double) * (size_t)(o->total_len - keep), st));
            o->nrst = 0;
        }
    }
    return sem_lns_sens(m, A, s);
}

}  // extern "C"
