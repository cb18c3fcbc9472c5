// The linearised Navier-Stokes operator L itself, in strong (pointwise) form, element-local (gfx950):
//   out_k = c_lap nu lap(u~_k) + c_conv N_k / bm1 + c_p gradm1(P)_k ,   u~ = mask u,  P = p on the GLL mesh
// with lap = sum_i gradm1(gradm1(.)_i)_i (no mass, no dssum), N the weak dealiased convective term of sem_conv_apply and
// P = (I21 x I21 [x I21]) p.  Reference: apply_L, apply_Lv, compute_LNS_conv, compute_LNS_laplacian, compute_LNS_gradp
// (src/linops/neklab_linops.f90:268-426); tests/lns_ref.py restates it in numpy.  No gather-scatter, no halo, no solver.
//
// k_lns_strong<N, DIM>: one block per element, one thread per point (four at lx1 = 12 in 3-D), the lanes of a call in a loop inside
// the block, so that the 9 (4) rst, jac, bm1 and the masks are read ONCE per element for all lanes and components and stay in
// registers.  Per lane: p goes Gauss -> GLL through LDS (one direction at a time) and its gradient stays in registers; per component
// the masked field goes to LDS, its physical gradient to three LDS arrays, the second gradient and the combination to HBM.  No
// intermediate leaves the block.  Rows are padded to N + 1 doubles (the x-derivative's lanes then differ in bank at every N).
// Algorithmic bytes per point and lane (3-D, all terms): 24 (u) + 24 (N) + 24 (out) + 8 (n2 / n)^3 (p); per point, shared by the
// lanes: 72 (rst) + 8 (jac) + 8 (bm1) + 24 (masks).  Flops per point and component: 2 N (3 + 12) + 30, plus the interpolation.
#include <algorithm>
#include <cmath>

#include "internal.h"
#include "lns_elem.h"

using namespace nlg;

namespace {

// u, p, nk, out: lane 0's; lane v of u and p sits v * ldi doubles behind, of nk v * ldn, of out v * ldo.  Component c of u, nk and
// out is c * fs doubles behind component 0.  nk (the weak convective term) may be out itself: a thread reads and writes its own
// points only.  clap = c_lap nu.  A zero coefficient skips that term's loads and work (uniform branches).
template <int N, int DIM>
__global__ __launch_bounds__((LnsShape<N, DIM>::NT), (LnsShape<N, DIM>::MINW)) void k_lns_strong(LnsGeom G, const double *__restrict__ Dt, const double *__restrict__ I21,
                                                                      const double *u, const double *p, int64_t ldi, const double *nk,
                                                                      int64_t ldn, double *out, int64_t ldo, int64_t fs, int nl, double clap,
                                                                      double cconv, double cp) {
    using S = LnsShape<N, DIM>;
    constexpr int NP = S::NP, NT = S::NT, PPT = S::PPT, N2 = N - 2, NQ = N + 1;
    constexpr int NP2 = DIM == 3 ? N2 * N2 * N2 : N2 * N2;
    constexpr int NB = DIM == 3 ? NQ * N * N : NQ * N;
    __shared__ double sDt[N * N];
    __shared__ double sI[N * N2];
    __shared__ double sF[NB];
    __shared__ double sG[DIM][NB];
    const int t = threadIdx.x;
    const int64_t eb = (int64_t)blockIdx.x * NP, eb2 = (int64_t)blockIdx.x * NP2;
    const bool do_lap = clap != 0.0, do_conv = cconv != 0.0, do_p = cp != 0.0;
    for (int q = t; q < N * N; q += NT) sDt[q] = Dt[q];
    if (do_p)
        for (int q = t; q < N * N2; q += NT) sI[q] = I21[q];

    // this thread's points and their geometry, for all lanes and components
    int pq[PPT], pi[PPT], pj[PPT], pk[PPT];
    bool act[PPT];
    double rs[PPT][DIM * DIM], jinv[PPT], binv[PPT], mk[PPT][DIM];
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int q = t + r * NT;
        act[r] = q < NP;
        const int qq = act[r] ? q : 0;
        pq[r] = qq;
        pi[r] = qq % N;
        pj[r] = (qq / N) % N;
        pk[r] = DIM == 3 ? qq / (N * N) : 0;
#pragma unroll
        for (int a = 0; a < DIM * DIM; ++a) rs[r][a] = G.rst[a][eb + qq];
        jinv[r] = 1.0 / G.jac[eb + qq];
        binv[r] = do_conv ? 1.0 / G.bm1[eb + qq] : 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) mk[r][c] = do_lap ? G.mask[c][eb + qq] : 0.0;
    }

    for (int v = 0; v < nl; ++v) {
        double gp[PPT][DIM];
#pragma unroll
        for (int r = 0; r < PPT; ++r)
#pragma unroll
            for (int c = 0; c < DIM; ++c) gp[r][c] = 0.0;
        __syncthreads();   // the tables are in LDS; the previous lane is done with sG
        if (do_p) {
            // Gauss (n2) -> GLL (n), one direction at a time: p -> A = sG[0], x -> B = sG[1], y -> A (3-D), last -> sF
            const double *__restrict__ pv = p + (int64_t)v * ldi + eb2;
            double *A = sG[0], *B = sG[1];
            for (int q = t; q < NP2; q += NT) A[q] = pv[q];
            __syncthreads();
            constexpr int R2 = DIM == 3 ? N2 * N2 : N2;   // rows of the x pass
            for (int q = t; q < R2 * N; q += NT) {
                const int i = q % N, row = q / N;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < N2; ++l) s += sI[i * N2 + l] * A[row * N2 + l];
                B[row * N + i] = s;
            }
            __syncthreads();
            if (DIM == 3) {
                for (int q = t; q < N2 * N * N; q += NT) {
                    const int i = q % N, j = (q / N) % N, k2 = q / (N * N);
                    double s = 0.0;
#pragma unroll
                    for (int l = 0; l < N2; ++l) s += sI[j * N2 + l] * B[(k2 * N2 + l) * N + i];
                    A[(k2 * N + j) * N + i] = s;
                }
                __syncthreads();
            }
            const double *T = DIM == 3 ? A : B;   // [N2][N (j)][N (i)] in 3-D, [N2][N (i)] in 2-D
            for (int q = t; q < NP; q += NT) {
                const int i = q % N, j = (q / N) % N, k = DIM == 3 ? q / (N * N) : 0;
                const int m = DIM == 3 ? k : j;   // the index the last pass interpolates
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < N2; ++l) s += sI[m * N2 + l] * (DIM == 3 ? T[(l * N + j) * N + i] : T[l * N + i]);
                sF[i + NQ * (j + N * k)] = s;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PPT; ++r) lns_grad<N, DIM>(sF, sDt, pi[r], pj[r], pk[r], rs[r], jinv[r], gp[r]);
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double lap[PPT];
#pragma unroll
            for (int r = 0; r < PPT; ++r) lap[r] = 0.0;
            if (do_lap) {
                const double *__restrict__ uc = u + (int64_t)v * ldi + (int64_t)c * fs + eb;
                if (c == 0) __syncthreads();   // the pressure gradient has read sF
#pragma unroll
                for (int r = 0; r < PPT; ++r)
                    if (act[r]) sF[pi[r] + NQ * (pj[r] + N * pk[r])] = mk[r][c] * uc[pq[r]];
                __syncthreads();
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    double g[DIM];
                    lns_grad<N, DIM>(sF, sDt, pi[r], pj[r], pk[r], rs[r], jinv[r], g);
                    if (act[r]) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) sG[a][pi[r] + NQ * (pj[r] + N * pk[r])] = g[a];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    const int i = pi[r], j = pj[r], k = pk[r];
                    double acc = 0.0;
#pragma unroll
                    for (int l = 0; l < N; ++l) {
                        const int ix = l + NQ * (j + N * k), iy = i + NQ * (l + N * k), iz = i + NQ * (j + N * l);
                        double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
                        for (int a = 0; a < DIM; ++a) {
                            sx += rs[r][0 * DIM + a] * sG[a][ix];
                            sy += rs[r][1 * DIM + a] * sG[a][iy];
                            if (DIM == 3) sz += rs[r][(DIM - 1) * DIM + a] * sG[a][iz];
                        }
                        acc += sDt[l * N + i] * sx + sDt[l * N + j] * sy;
                        if (DIM == 3) acc += sDt[l * N + k] * sz;
                    }
                    lap[r] = acc * jinv[r];
                }
            }
#pragma unroll
            for (int r = 0; r < PPT; ++r) {
                if (!act[r]) continue;
                const int64_t o = (int64_t)c * fs + eb + pq[r];
                double res = clap * lap[r] + cp * gp[r][c];
                if (do_conv) res += cconv * (nk[(int64_t)v * ldn + o] * binv[r]);
                out[(int64_t)v * ldo + o] = res;
            }
        }
    }
}

// w_c = mask_c u_c for the dim components of nl lanes: the input of the convective term (bcdirvc on a copy; u is not modified)
__global__ void k_lns_mask(int dim, int nl, int64_t lvn, int64_t fs, LnsGeom G, const double *u, int64_t ldu, double *w, int64_t ldw) {
    const int c = blockIdx.y % dim, v = blockIdx.y / dim;
    if (v >= nl) return;
    const double *__restrict__ mk = G.mask[c];
    const double *__restrict__ uc = u + (int64_t)v * ldu + (int64_t)c * fs;
    double *__restrict__ wc = w + (int64_t)v * ldw + (int64_t)c * fs;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < lvn; q += (int64_t)gridDim.x * blockDim.x) wc[q] = mk[q] * uc[q];
}

// I21[k][j] = l_j(z1_k), the Lagrange basis on the Gauss points z2 at the GLL points z1 (Nek mappr), barycentric form
void gauss_to_gll(const nlg_ops1d &o, std::vector<double> &M) {
    const int n = o.n, n2 = o.n2;
    std::vector<double> bw((size_t)n2, 1.0);
    for (int j = 0; j < n2; ++j)
        for (int k = 0; k < n2; ++k)
            if (k != j) bw[j] /= (o.z2[j] - o.z2[k]);
    M.assign((size_t)n * n2, 0.0);
    for (int k = 0; k < n; ++k) {
        int hit = -1;
        for (int j = 0; j < n2; ++j)
            if (std::fabs(o.z1[k] - o.z2[j]) < 1e-15) hit = j;
        if (hit >= 0) {
            M[(size_t)k * n2 + hit] = 1.0;
            continue;
        }
        double sum = 0.0;
        for (int j = 0; j < n2; ++j) sum += bw[j] / (o.z1[k] - o.z2[j]);
        for (int j = 0; j < n2; ++j) M[(size_t)k * n2 + j] = bw[j] / (o.z1[k] - o.z2[j]) / sum;
    }
}

template <int N, int DIM>
void lns_launch(nlg_mesh *m, const LnsGeom &G, const double *I21, const double *u, const double *p, int64_t ldi, const double *nk, int64_t ldn,
                double *out, int64_t ldo, int nl, double clap, double cconv, double cp) {
    NLG_LAUNCH((k_lns_strong<N, DIM>), dim3((unsigned)m->E), dim3(LnsShape<N, DIM>::NT), 0, m->ctx->stream, G, (const double *)m->d_Dt, I21, u, p, ldi,
               nk, ldn, out, ldo, m->lvs, nl, clap, cconv, cp);
}

// the strong-form combination for nl lanes in ONE launch.  u, p: lane 0's velocity (component 0) and pressure, lane v at v * ldi;
// nk: the weak convective term (null when coef[1] == 0), lane v at v * ldn; out: lane v at v * ldo; components lvs apart throughout.
int sem_lns_strong(nlg_mesh *m, const double *I21, const double *u, const double *p, int64_t ldi, const double *nk, int64_t ldn, double *out,
                   int64_t ldo, int nl, double nu, const double *coef) {
    NLG_CHECK(nl >= 1 && nl <= kMaxLanes, "sem_lns_strong: %d lanes", nl);
    NLG_CHECK(m->E <= 0x7fffffff, "sem_lns_strong: %lld elements exceed the launch grid", (long long)m->E);
    NLG_CHECK(coef[1] == 0.0 || nk, "sem_lns_strong: the convective term is missing");
    const LnsGeom G = lns_geom(m);
    const double clap = coef[0] * nu, cconv = coef[1], cp = coef[2];
#define NLG_LNS_CASE(N_)                                                                              \
    case N_:                                                                                          \
        if (m->dim == 3)                                                                              \
            lns_launch<N_, 3>(m, G, I21, u, p, ldi, nk, ldn, out, ldo, nl, clap, cconv, cp);          \
        else                                                                                          \
            lns_launch<N_, 2>(m, G, I21, u, p, ldi, nk, ldn, out, ldo, nl, clap, cconv, cp);          \
        break;
    switch (m->n) {
        NLG_LNS_CASE(4)
        NLG_LNS_CASE(5)
        NLG_LNS_CASE(6)
        NLG_LNS_CASE(7)
        NLG_LNS_CASE(8)
        NLG_LNS_CASE(9)
        NLG_LNS_CASE(10)
        NLG_LNS_CASE(12)
        default: set_error("sem_lns_strong: unsupported lx1 = %d (built for 4..10, 12)", m->n); return 1;
    }
#undef NLG_LNS_CASE
    NLG_HIP(hipGetLastError());
    return 0;
}

// lanes as a stride: true if vector v's storage starts v * (*ld) doubles behind vector 0's for every v (always so for s <= 2)
bool lane_stride(int s, const nlg_vec *const *vecs, int64_t *ld) {
    *ld = 0;
    if (s == 1) return true;
    const intptr_t d1 = (intptr_t)vecs[1]->d - (intptr_t)vecs[0]->d;
    if (d1 % (intptr_t)sizeof(double)) return false;
    for (int v = 2; v < s; ++v)
        if ((intptr_t)vecs[v]->d - (intptr_t)vecs[0]->d != v * d1) return false;
    *ld = (int64_t)(d1 / (intptr_t)sizeof(double));
    return true;
}

}  // namespace

// owns the base-flow side of the convective term and the workspaces of an apply; nothing of the time stepper
struct nlg_lns {
    nlg_mesh *mesh = nullptr;
    const nlg_vec *base = nullptr;   // the vector last given to create / set_baseflow: compared with `out`, never read after the call
    double re = 0.0;
    double *Ur[3] = {}, *GU[9] = {};
    double *d_I21 = nullptr;
    // workspaces, allocated by the first apply that needs them, for as many lanes as it has (cap_*), and kept
    int cap_conv = 0, cap_in = 0, cap_out = 0;
    double *wm = nullptr, *wn = nullptr;      // [cap_conv][dim lvs]: masked input of the convective term, its weak result
    double *win = nullptr, *wout = nullptr;   // [cap_in][dim lvs + lps], [cap_out][dim lvs]: lanes that are not a stride apart go through these
};

namespace {

// buf holds s lanes of per_lane doubles afterwards (have: the lanes it holds now)
int lns_reserve(nlg_lns *L, double **buf, int64_t per_lane, int s, int have) {
    if (*buf && have >= s) return 0;
    if (*buf) {
        NLG_HIP(hipStreamSynchronize(L->mesh->ctx->stream));
        NLG_HIP(hipFree(*buf));
        *buf = nullptr;
    }
    NLG_HIP(hipMalloc(buf, sizeof(double) * (size_t)per_lane * s));
    return 0;
}

}  // namespace

extern "C" {

int nlg_lns_set_baseflow(nlg_lns *L, const nlg_vec *baseflow) {
    NLG_CHECK(L && baseflow, "nlg_lns_set_baseflow: NULL argument");
    NLG_CHECK(baseflow->mesh == L->mesh, "nlg_lns_set_baseflow: the base flow lives on another mesh");
    nlg_mesh *m = L->mesh;
    double *U[3] = {baseflow->vel(0), baseflow->vel(1), m->dim == 3 ? baseflow->vel(2) : nullptr};
    NLG_TRY(sem_conv_setup(m, U, L->Ur, L->GU));
    L->base = baseflow;
    return 0;
}

int nlg_lns_set_re(nlg_lns *L, double re) {
    NLG_CHECK(L, "nlg_lns_set_re: NULL argument");
    NLG_CHECK(re > 0.0, "nlg_lns_set_re: re = %g must be positive", re);
    L->re = re;
    return 0;
}

int nlg_lns_destroy(nlg_lns *L) {
    if (!L) return 0;
    if (L->mesh) hipStreamSynchronize(L->mesh->ctx->stream);
    for (double *q : L->Ur) (void)hipFree(q);
    for (double *q : L->GU) (void)hipFree(q);
    for (double *q : {L->d_I21, L->wm, L->wn, L->win, L->wout}) (void)hipFree(q);
    delete L;
    return 0;
}

int nlg_lns_create(nlg_mesh *m, const nlg_vec *baseflow, double re, nlg_lns **out) {
    NLG_CHECK(m && baseflow && out, "nlg_lns_create: NULL argument");
    NLG_CHECK(baseflow->mesh == m, "nlg_lns_create: the base flow lives on another mesh");
    NLG_CHECK(re > 0.0, "nlg_lns_create: re = %g must be positive", re);
    NLG_HIP(hipSetDevice(m->ctx->device));
    nlg_lns *L = new nlg_lns();
    L->mesh = m;
    L->re = re;
    std::vector<double> I21;
    gauss_to_gll(m->ops, I21);
    bool ok = hipMalloc(&L->d_I21, sizeof(double) * I21.size()) == hipSuccess;
    for (int c = 0; c < m->dim && ok; ++c) ok = hipMalloc(&L->Ur[c], sizeof(double) * (size_t)m->lfn) == hipSuccess;
    for (int q = 0; q < m->dim * m->dim && ok; ++q) ok = hipMalloc(&L->GU[q], sizeof(double) * (size_t)m->lfn) == hipSuccess;
    // (a synchronous copy: I21 is a local)
    ok = ok && hipMemcpy(L->d_I21, I21.data(), sizeof(double) * I21.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        nlg_lns_destroy(L);
        set_error("nlg_lns_create: out of device memory");
        return 1;
    }
    if (int rc = nlg_lns_set_baseflow(L, baseflow)) {
        nlg_lns_destroy(L);
        return rc;
    }
    *out = L;
    return 0;
}

int nlg_lns_apply(nlg_lns *L, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint, const double *coef) {
    NLG_CHECK(L && in && out && coef, "nlg_lns_apply: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_lns_apply: s = %d out of range (1..%d)", s, kMaxLanes);
    nlg_mesh *m = L->mesh;
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(in[v] && out[v], "nlg_lns_apply: vector %d is NULL", v);
        NLG_CHECK(in[v]->mesh == m && out[v]->mesh == m, "nlg_lns_apply: vector %d lives on another mesh", v);
        NLG_CHECK(in[v]->ncomp == in[0]->ncomp && out[v]->ncomp == out[0]->ncomp, "nlg_lns_apply: vector %d has another number of scalars than vector 0", v);
    }
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(out[v] != L->base && out[v]->d != (L->base ? L->base->d : nullptr), "nlg_lns_apply: out[%d] aliases the base flow", v);
        for (int w = 0; w < s; ++w) {
            NLG_CHECK(out[v] != in[w] && out[v]->d != in[w]->d, "nlg_lns_apply: out[%d] aliases in[%d]", v, w);
            NLG_CHECK(w == v || out[v]->d != out[w]->d, "nlg_lns_apply: out[%d] aliases out[%d]", v, w);
        }
    }
    NLG_CHECK(coef[0] != 0.0 || coef[1] != 0.0 || coef[2] != 0.0, "nlg_lns_apply: all three coefficients are zero");
    NLG_CHECK(L->re > 0.0, "nlg_lns_apply: re = %g must be positive", L->re);
    const int dim = m->dim;
    hipStream_t st = m->ctx->stream;
    const int64_t lv = (int64_t)dim * m->lvs, lw = lv + m->lps;
    const bool do_conv = coef[1] != 0.0;
    int64_t ldi = 0, ldo = 0;
    const double *u = in[0]->vel(0), *p = in[0]->pr();
    double *o = out[0]->vel(0);
    const bool stage_in = !lane_stride(s, in, &ldi), stage_out = !lane_stride(s, (const nlg_vec *const *)out, &ldo);
    if (stage_in) {
        NLG_TRY(lns_reserve(L, &L->win, lw, s, L->cap_in));
        L->cap_in = std::max(L->cap_in, s);
        for (int v = 0; v < s; ++v) {
            NLG_HIP(hipMemcpyAsync(L->win + v * lw, in[v]->vel(0), sizeof(double) * (size_t)lv, hipMemcpyDeviceToDevice, st));
            NLG_HIP(hipMemcpyAsync(L->win + v * lw + lv, in[v]->pr(), sizeof(double) * (size_t)m->lps, hipMemcpyDeviceToDevice, st));
        }
        u = L->win, p = L->win + lv, ldi = lw;
    }
    if (stage_out) {
        NLG_TRY(lns_reserve(L, &L->wout, lv, s, L->cap_out));
        L->cap_out = std::max(L->cap_out, s);
        o = L->wout, ldo = lv;
    }
    const double *nk = nullptr;
    if (do_conv) {
        NLG_TRY(lns_reserve(L, &L->wm, lv, s, L->cap_conv));
        NLG_TRY(lns_reserve(L, &L->wn, lv, s, L->cap_conv));
        L->cap_conv = std::max(L->cap_conv, s);
        NLG_LAUNCH(k_lns_mask, dim3((unsigned)std::min<int64_t>((m->lvn + 255) / 256, 2048), (unsigned)(dim * s)), dim3(256), 0, st, dim, s, m->lvn,
                   m->lvs, lns_geom(m), u, ldi, L->wm, lv);
        double *wu[3] = {L->wm, L->wm + m->lvs, dim == 3 ? L->wm + 2 * m->lvs : nullptr};
        double *wo[3] = {L->wn, L->wn + m->lvs, dim == 3 ? L->wn + 2 * m->lvs : nullptr};
        NLG_TRY(sem_conv_apply(m, L->Ur, L->GU, wu, wo, adjoint ? 1 : 0, s, lv));
        nk = L->wn;
    }
    NLG_TRY(sem_lns_strong(m, L->d_I21, u, p, ldi, nk, lv, o, ldo, s, 1.0 / L->re, coef));
    for (int v = 0; v < s; ++v) {
        if (stage_out)
            for (int c = 0; c < dim; ++c)
                NLG_HIP(hipMemcpyAsync(out[v]->vel(c), L->wout + v * lv + c * m->lvs, sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, st));
        for (int q = 0; q < out[v]->nscal; ++q) NLG_HIP(hipMemsetAsync(out[v]->theta(q), 0, sizeof(double) * (size_t)m->lvn, st));
        NLG_HIP(hipMemsetAsync(out[v]->pr(), 0, sizeof(double) * (size_t)m->lpn, st));
    }
    return 0;
}

int nlg_op_lns(nlg_mesh *m, const nlg_vec *base, const nlg_vec *in, nlg_vec *out, double re, int adjoint, const double *coef) {
    NLG_CHECK(m && base && in && out && coef, "nlg_op_lns: NULL argument");
    NLG_CHECK(base->mesh == m && in->mesh == m && out->mesh == m, "nlg_op_lns: a vector lives on another mesh");
    NLG_CHECK(out != base && out->d != base->d, "nlg_op_lns: out aliases the base flow");
    NLG_CHECK(out != in && out->d != in->d, "nlg_op_lns: out aliases in");
    NLG_CHECK(coef[0] != 0.0 || coef[1] != 0.0 || coef[2] != 0.0, "nlg_op_lns: all three coefficients are zero");
    NLG_CHECK(re > 0.0, "nlg_op_lns: re = %g must be positive", re);
    nlg_lns *L = nullptr;
    NLG_TRY(nlg_lns_create(m, base, re, &L));
    const int rc = nlg_lns_apply(L, 1, &in, &out, adjoint, coef);
    nlg_lns_destroy(L);   // waits for the stream
    return rc;
}

}  // extern "C"
