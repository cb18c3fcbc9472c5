// Two-level preconditioner of the consistent Poisson operator E = D (mask B^-1 QQ^T) D^T (gfx950).
//
// Role in the reference: `preconditioner = semg_xxt` of the pressure solve inside nek_advance
// (/root/reference/examples/cylinder/stability/direct/1cyl.par:21); Nek5000's implementation is not in the
// reference tree.  This is a restatement of the published idea (Fischer 1997; Lottes & Fischer 2005) in its
// simplest robust form, chosen from a numpy prototype (docs/prototypes/precond_proto.py: Jacobi 680 iterations,
// element-wise FDM 192, FDM + exact piecewise-constant coarse grid 81, FDM + the V-cycle below 110, all at
// E = 512, independent of E for the two-level variants):
//   M^-1 r = sum_e R_e^T Etilde_e^-1 R_e r                     (element-wise fast diagonalisation, additive)
//          + R_1   V(A_c) R_1^T r                              (trilinear coarse space on the element vertices)
//   Etilde_e : E restricted to element e with the element replaced by a box of its mean edge lengths and the
//              neighbours' mass lumped on shared faces: separable, inverted exactly by 1-D generalised
//              eigen-decompositions (n2 x n2 per direction).
//   R_1     : columns = the trilinear (bilinear in 2-D) hat functions of the element vertices evaluated at the GL
//             pressure points; continuous across elements although the pressure space is not.  Prototype
//             (docs/prototypes/precond_proto2.py, precond_proto3.py, explicit sparse E): against the piecewise-constant
//             space used first (R_0) the vertex space halves the iteration count (73 -> 37 at lx1 = 8 with exact
//             element blocks; 30 at lx1 = 6), mesh-independent, and one V-cycle is as good as the exact solve.
//   A_c = R_1^T E R_1 : Galerkin, sparse nvert x nvert (125-point on structured meshes).  Assembled by probing E on
//             the device: elements are coloured so that no two of one colour share a neighbour, one E application
//             per (colour, corner) gives the 2^dim x 2^dim blocks phi_c'^T E_{e',e} phi_c of every neighbouring pair.
//   V(A_c)  : additive two-grid approximation of A_c^-1: omega diag(A_c)^-1 + P (P^T A_c P)^-1 P^T with P the
//             piecewise-constant prolongation from greedy aggregates of vertices (dense inverse on the aggregates).
//             In the prototype it needs as few PCG iterations as the exact coarse solve or a multiplicative V-cycle
//             (29-30), and it needs no product with A_c at run time.  When nvert is small the aggregates are the
//             vertices (exact solve, no Jacobi term).
//   With several ranks the coarse level is rank-local (E without the halo exchange): block-diagonal, still SPD.
// M is a fixed symmetric positive (semi-)definite operator, so plain PCG stays valid.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <string>

#include <rocsolver/rocsolver.h>

#include "internal.h"
#include "pprec_host.h"

using namespace nlg;

namespace {

constexpr int NT = 256;

struct Hat {
    double h1[12];   // (1 + z)/2 at the GL points; the lower-corner hat is 1 - h1
};

template <int S0, int S1, int S2, int AX, int NOUT, bool TRANS>
__device__ __forceinline__ void contract(const double *__restrict__ in, double *__restrict__ out,
                                         const double *__restrict__ M, int tid, int nth) {
    // out[.., o, ..] = sum_l Mop[o][l] in[.., l, ..] ; Mop = M (NOUT x NIN row-major) or its transpose
    constexpr int NIN = AX == 0 ? S0 : (AX == 1 ? S1 : S2);
    constexpr int O0 = AX == 0 ? NOUT : S0, O1 = AX == 1 ? NOUT : S1, O2 = AX == 2 ? NOUT : S2;
    for (int p = tid; p < O0 * O1 * O2; p += nth) {
        const int a = p % O0, b = (p / O0) % O1, c = p / (O0 * O1);
        const int o = AX == 0 ? a : (AX == 1 ? b : c);
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < NIN; ++l) {
            const int q = AX == 0 ? (l + S0 * (b + S1 * c)) : (AX == 1 ? (a + S0 * (l + S1 * c)) : (a + S0 * (b + S1 * l)));
            s += (TRANS ? M[l * NOUT + o] : M[o * NIN + l]) * in[q];
        }
        out[p] = s;
    }
}

// The same transform in place: a lane reads its whole column into registers before it writes the outputs, and the
// columns of one stage are disjoint, so one LDS array serves as input and output (half the LDS per element -> twice
// the resident elements per CU for a kernel that mostly waits).
template <int N2, bool FWD, int AX, int ST = 64>
__device__ __forceinline__ void fdm_stage_inplace3(double *buf, const double *S, int lane) {
    constexpr int NCOL = N2 * N2;
    for (int col = lane; col < NCOL; col += ST) {
        int base, stride;
        if (AX == 0) {
            base = col * N2;
            stride = 1;
        } else if (AX == 1) {
            base = (col % N2) + N2 * N2 * (col / N2);
            stride = N2;
        } else {
            base = col;
            stride = N2 * N2;
        }
        double v[N2];
#pragma unroll
        for (int l = 0; l < N2; ++l) v[l] = buf[base + stride * l];
        double o_[N2];
#pragma unroll
        for (int o = 0; o < N2; ++o) {
            double a = 0.0;
#pragma unroll
            for (int l = 0; l < N2; ++l) a += (FWD ? S[l * N2 + o] : S[o * N2 + l]) * v[l];
            o_[o] = a;
        }
#pragma unroll
        for (int o = 0; o < N2; ++o) buf[base + stride * o] = o_[o];
    }
}

// z_e = (Sz x Sy x Sx) [ invden o ((Sz x Sy x Sx)^T r_e) ] + xc[e]      (S stored row-major [point][mode])
// One wave per element, four elements per block: the six 1-D transforms of an element are tiny (N2^3 points), so
// the kernel is bound by launch/barrier latency, not by bytes; each lane owns whole columns and keeps them in
// registers between the load and the N2 outputs.
template <int N2, int DIM, bool FWD, int AX>
__device__ __forceinline__ void fdm_stage(const double *__restrict__ in, double *__restrict__ out,
                                          const double *__restrict__ S, int lane) {
    constexpr int NZ = DIM == 3 ? N2 : 1;
    constexpr int NCOL = (N2 * N2 * NZ) / N2;
    for (int col = lane; col < NCOL; col += 64) {
        // column base index and stride along axis AX of an [NZ][N2][N2] array
        int base, stride;
        if (AX == 0) {
            base = col * N2;
            stride = 1;
        } else if (AX == 1) {
            base = (col % N2) + N2 * N2 * (col / N2);
            stride = N2;
        } else {
            base = col;
            stride = N2 * N2;
        }
        double v[N2];
#pragma unroll
        for (int l = 0; l < N2; ++l) v[l] = in[base + stride * l];
#pragma unroll
        for (int o = 0; o < N2; ++o) {
            double a = 0.0;
#pragma unroll
            for (int l = 0; l < N2; ++l) a += (FWD ? S[l * N2 + o] : S[o * N2 + l]) * v[l];
            out[base + stride * o] = a;
        }
    }
}

template <int N2, int DIM>
__global__ __launch_bounds__(NT) void k_fdm(const double *__restrict__ flag, int64_t E, const double *__restrict__ S,
                                            const double *__restrict__ invden, const double *__restrict__ r,
                                            const double *__restrict__ xc, const double *__restrict__ xa,
                                            const int *__restrict__ agg, const int *__restrict__ vg, Hat hat,
                                            double *__restrict__ z, double *__restrict__ part, int64_t ld, int64_t lv, int64_t la) {
    constexpr int NP = DIM == 3 ? N2 * N2 * N2 : N2 * N2;
    __shared__ double sS[4][3][N2 * N2];
    __shared__ double sA[4][NP], sB[4][NP];
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        r += lo, z += lo;
        if (part) part += lo;
        if (xc) xc += (int64_t)blockIdx.y * lv, xa += (int64_t)blockIdx.y * la;
    }
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wv;
    const bool act = e < E;
    const int64_t ee = act ? e : 0;
    for (int q = lane; q < DIM * N2 * N2; q += 64) sS[wv][q / (N2 * N2)][q % (N2 * N2)] = S[ee * (3 * N2 * N2) + q];
    for (int q = lane; q < NP; q += 64) sA[wv][q] = r[ee * NP + q];
    __syncthreads();
    fdm_stage<N2, DIM, true, 0>(sA[wv], sB[wv], sS[wv][0], lane);
    __syncthreads();
    fdm_stage<N2, DIM, true, 1>(sB[wv], sA[wv], sS[wv][1], lane);
    __syncthreads();
    if constexpr (DIM == 3) {
        fdm_stage<N2, DIM, true, 2>(sA[wv], sB[wv], sS[wv][2], lane);
        __syncthreads();
        for (int q = lane; q < NP; q += 64) sB[wv][q] *= invden[ee * NP + q];
        __syncthreads();
        fdm_stage<N2, DIM, false, 2>(sB[wv], sA[wv], sS[wv][2], lane);
        __syncthreads();
    } else {
        for (int q = lane; q < NP; q += 64) sA[wv][q] *= invden[ee * NP + q];
        __syncthreads();
    }
    fdm_stage<N2, DIM, false, 1>(sA[wv], sB[wv], sS[wv][1], lane);
    __syncthreads();
    fdm_stage<N2, DIM, false, 0>(sB[wv], sA[wv], sS[wv][0], lane);
    __syncthreads();
    double srz = 0.0, sz = 0.0;
    if (act) {
        // coarse correction prolonged on the fly: trilinear interpolation of the 2^DIM vertex values of the element
        constexpr int NC = 1 << DIM;
        double cv[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int v = xc ? vg[e * NC + c] : 0;
            cv[c] = xc ? xc[v] + xa[agg[v]] : 0.0;   // Jacobi term + aggregate-level correction
        }
        for (int q = lane; q < NP; q += 64) {
            const double ha = hat.h1[q % N2], hb = hat.h1[(q / N2) % N2];
            double c0 = (cv[0] + ha * (cv[1] - cv[0])), c1 = (cv[2] + ha * (cv[3] - cv[2]));
            double cc = c0 + hb * (c1 - c0);
            if constexpr (DIM == 3) {
                const double hc = hat.h1[q / (N2 * N2)];
                const double d0 = (cv[4] + ha * (cv[5] - cv[4])), d1 = (cv[6] + ha * (cv[7] - cv[6]));
                cc += hc * ((d0 + hb * (d1 - d0)) - cc);
            }
            const double zv = sA[wv][q] + cc;
            z[e * NP + q] = zv;
            if (part) {
                srz += r[e * NP + q] * zv;
                sz += zv;
            }
        }
    }
    if (part) {   // first-stage sums of the surrounding PCG: part[blk] = sum r.z, part[nblk + blk] = sum z
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            srz += __shfl_down(srz, o, 64);
            sz += __shfl_down(sz, o, 64);
        }
        __syncthreads();
        if (lane == 0) {
            sB[0][wv] = srz;
            sB[0][4 + wv] = sz;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            part[blockIdx.x] = sB[0][0] + sB[0][1] + sB[0][2] + sB[0][3];
            part[gridDim.x + blockIdx.x] = sB[0][4] + sB[0][5] + sB[0][6] + sB[0][7];
        }
    }
}

// the vertex gather and the aggregate restriction of the coarse chain, both straight from the element-corner values t: they ride
// in the launch of k_fdm_ext* / k_fdm_ext2, so that the coarse chain adds one launch (k_dense_gemv) to the fine level.  The restriction
// recomputes the vertex sums of its members in the order of the gather, so ra is bit-identical to restricting rc.
struct ChainArgs {
    int nb_gather;                 // blocks of the vertex gather; the blocks of the aggregate restriction follow
    int nvert;
    const int *vp, *vi;            // vertex -> incident (element, corner) entries, CSR
    const double *t;
    double *rc;
    const double *dinv;
    double om;
    double *x;
    int na;
    const int *ap, *am;            // aggregate -> member vertices, CSR
    double *ra;
    int64_t lt, lv, la;
};
// (as a part of a merged launch: `bx` = block index inside this part, any multiple of 64 threads per block)
__device__ __forceinline__ void chain_body(int bx, const double *flag, int64_t ld, const ChainArgs &g) {
    if (flag) flag += (int64_t)blockIdx.y * ld;
    if (flag && flag[0] != 0.0) return;
    const double *__restrict__ t = g.t + (int64_t)blockIdx.y * g.lt;
    if (bx < g.nb_gather) {   // rc[v] = sum of t over the entries incident to v (fixed order); first damped-Jacobi sweep from zero
        double *rc = g.rc + (int64_t)blockIdx.y * g.lv, *x = g.x + (int64_t)blockIdx.y * g.lv;
        const int v = bx * (int)blockDim.x + (int)threadIdx.x;
        if (v >= g.nvert) return;
        double a = 0.0;
        for (int q = g.vp[v]; q < g.vp[v + 1]; ++q) a += t[g.vi[q]];
        rc[v] = a;
        x[v] = g.om * g.dinv[v] * a;
        return;
    }
    // ra[a] = sum of rc over the members of aggregate a, one wave per aggregate
    double *ra = g.ra + (int64_t)blockIdx.y * g.la;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int a = (bx - g.nb_gather) * wpb + wid;
    if (a >= g.na) return;
    double s = 0.0;
    for (int q = g.ap[a] + lane; q < g.ap[a + 1]; q += 64) {
        const int v = g.am[q];
        double c = 0.0;
        for (int j = g.vp[v]; j < g.vp[v + 1]; ++j) c += t[g.vi[j]];
        s += c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) ra[a] = s;
}

// ---- overlapping variant ------------------------------------------------------------------------------------
// Extended local problems: element e plus the layer of GL points of each face neighbour that is adjacent to the
// shared face -> an N^dim grid (N = N2 + 2, the size of the velocity mesh), solved by fast diagonalisation with 1-D
// operators built from the line of up to three elements (pprec_setup).  Every ghost value is written once, by its
// producer, into the slot its consumer reads (the destinations per element face point come from pprec_setup: pin, pret):
//   k_q1_restrict_local* (pack)  Win[e]        = extended grid of e: r wq in the interior, and each element writes r wq of
//                                                its adjacent layers into the ghost slots of its neighbours' grids
//   k_fdm_ext*, k_fdm_ext2       z_e = interior of the solve on Win[e];  the solve at the ghost points -> the neighbour's
//                                                face slot of Wret
//   k_sch_finish, k_sch_finish2  z += Wret at the element's faces (+ coarse correction), r.z sums
// i.e. z = sum_e R_e^T Atilde_e^-1 R_e r with overlapping index sets R_e: symmetric, additive.  Win and Wret are two
// velocity-shaped arrays: a solve reads its grid while the neighbours' solves write their ghost values.  Win is in the
// natural layout; Wret is in the face-grouped layout in 3-D and in the natural one in 2-D (pin = pret there).  Edge and
// corner slots, and the ghost slots of faces without a neighbour, are never written and stay zero.  A face on a rank
// boundary has the element itself as destination: the copy-mode halo exchange replaces the own value by the neighbour's.
template <int DIM = 3>
__device__ __forceinline__ int face_pt(int N, int a, int b, int c = 1) {
    // compact index (0 .. 2 DIM (N-2)^(DIM-1) - 1) of an interior point of an element face of the N^DIM grid, the order of
    // fg_slot's face blocks (3-D)
    const int M = N - 2, M2 = DIM == 3 ? M : 1;   // points per face: M M2
    if (a == 0 || a == N - 1) return (a == N - 1) * M * M2 + (b - 1) + M * (c - 1);
    if (b == 0 || b == N - 1) return (2 + (b == N - 1)) * M * M2 + (a - 1) + M * (c - 1);
    return (4 + (c == N - 1)) * M * M2 + (a - 1) + M * (b - 1);
}

// WPB waves (= elements) per block.  WPB = 1 makes every __syncthreads a single-wave barrier: the stages of one element
// never wait for another element's.
// WPE > 1 (with WPB = 1): WPE waves share ONE element -- for lx1 > 8 a single wave has to sweep N N = 100 (144) columns
// with 64 lanes in two (three) rounds, 56 % (75 %) of them busy; two (three) waves take one column per lane.
template <int N, int WPB, int WPE = 1>
__global__ __launch_bounds__(64 * WPB * WPE) void k_fdm_ext(const double *__restrict__ flag, int64_t E, const double *__restrict__ S,
                                                const double *__restrict__ lam, double thr, const double *__restrict__ Win,
                                                double *__restrict__ Wr, double *__restrict__ z, const int *__restrict__ pret,
                                                int64_t ld, int64_t lW, int nb_fdm, ChainArgs cg) {
    constexpr int N2 = N - 2, NP = N * N * N, NP2 = N2 * N2 * N2, NF = 6 * N2 * N2;
    __shared__ double sL[WPB][3][N];
    __shared__ double sA[WPB][NP];   // the six transforms run in place (fdm_stage_inplace3)
    if ((int)blockIdx.x >= nb_fdm) {   // merged launch: the blocks behind the elements run the coarse chain up to the dense solve
        chain_body((int)blockIdx.x - nb_fdm, flag, ld, cg);
        return;
    }
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        z += lo, Win += (int64_t)blockIdx.y * lW, Wr += (int64_t)blockIdx.y * lW;
    }
    if (flag && flag[0] != 0.0) return;
    static_assert(WPB == 1 || WPE == 1, "either several elements per block or several waves per element");
    constexpr int ST = 64 * WPE;                                   // threads that share one element
    const int lane = WPE > 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63), wv = WPE > 1 ? 0 : (int)(threadIdx.x >> 6);
    const int64_t e = (int64_t)blockIdx.x * WPB + wv;
    const bool act = e < E;
    const int64_t ee = act ? e : 0;
    // the element index is wave-uniform: with the pointer made provably uniform the 1-D eigenvector matrices are read by
    // scalar loads straight into FMA operands instead of 384 broadcast LDS reads per lane
    const int eu = __builtin_amdgcn_readfirstlane((int)ee);
    const double *__restrict__ Sgg = S + (int64_t)eu * (3 * N * N);
    // lx1 <= 8: the three N x N matrices of the element go to LDS (three coalesced loads per lane) and are read from there at
    // wave-uniform addresses (broadcast).  As scalar-load operands they need 384 SGPRs: 100 of them were spilled to VGPR lanes
    // and a quarter of the kernel's instructions were v_readlane / v_writelane moves on the (saturated) vector pipe.
    constexpr bool SLDS = (N <= 8 && WPE == 1);
    __shared__ double sS[SLDS ? WPB : 1][SLDS ? 3 * N * N : 1];
    if (SLDS)
        for (int q = lane; q < 3 * N * N; q += ST) sS[wv][q] = Sgg[q];
    const double *Sg = SLDS ? sS[wv] : Sgg;
    for (int q = lane; q < 3 * N; q += ST) sL[wv][q / N][q % N] = lam[ee * (3 * N) + q];
    // one coalesced round trip: the extended grid, and the destinations of the ghost values (kept in registers for the store
    // phase; clamped loads at the points that are not face points)
    constexpr int NQL = (NP + ST - 1) / ST;
    int pr[NQL];
    {
        const double *We = Win + ee * NP;
        const int *pe = pret + ee * NF;
        double w[NQL];
#pragma unroll
        for (int u = 0; u < NQL; ++u) {
            const int q = lane + ST * u;
            const int qc = q < NP ? q : 0;
            const int a = qc % N, b = (qc / N) % N, c = qc / (N * N);
            const int nb = (a == 0 || a == N - 1) + (b == 0 || b == N - 1) + (c == 0 || c == N - 1);
            w[u] = We[qc];
            pr[u] = pe[nb == 1 ? face_pt(N, a, b, c) : 0];
        }
#pragma unroll
        for (int u = 0; u < NQL; ++u) {
            const int q = lane + ST * u;
            if (q >= NP) break;
            sA[wv][q] = w[u];
        }
    }
    __syncthreads();
    fdm_stage_inplace3<N, true, 0, ST>(sA[wv], Sg + 0 * N * N, lane);
    __syncthreads();
    fdm_stage_inplace3<N, true, 1, ST>(sA[wv], Sg + 1 * N * N, lane);
    __syncthreads();
    fdm_stage_inplace3<N, true, 2, ST>(sA[wv], Sg + 2 * N * N, lane);
    __syncthreads();
    for (int q = lane; q < NP; q += ST) {
        const double den = sL[wv][0][q % N] + sL[wv][1][(q / N) % N] + sL[wv][2][q / (N * N)];
        sA[wv][q] = den > thr ? sA[wv][q] / den : 0.0;
    }
    __syncthreads();
    fdm_stage_inplace3<N, false, 2, ST>(sA[wv], Sg + 2 * N * N, lane);
    __syncthreads();
    fdm_stage_inplace3<N, false, 1, ST>(sA[wv], Sg + 1 * N * N, lane);
    __syncthreads();
    fdm_stage_inplace3<N, false, 0, ST>(sA[wv], Sg + 0 * N * N, lane);
    __syncthreads();
    if (act) {
#pragma unroll
        for (int u = 0; u < NQL; ++u) {
            const int q = lane + ST * u;
            if (q >= NP) break;
            const int a = q % N, b = (q / N) % N, c = q / (N * N);
            const int nb = (a == 0 || a == N - 1) + (b == 0 || b == N - 1) + (c == 0 || c == N - 1);
            const double v = sA[wv][q];
            if (nb == 0)
                z[e * NP2 + (a - 1) + N2 * ((b - 1) + N2 * (c - 1))] = v;
            else if (nb == 1 && pr[u] >= 0)
                Wr[pr[u]] = v;   // ghost value: belongs to the neighbour's adjacent layer
        }
    }
}

// ---- the same extended local solve with the six 1-D transforms on the matrix pipe (lx1 = 8) --------------------------------
// One wave per element.  A transform along one axis is the GEMM  out(8 x 64 columns) = S(8 x 8) in(8 x 64 columns), issued as
// v_mfma_f64_16x16x4_f64 tiles: M = output index (8 of the 16 rows used), N = 16 data columns, K = 8 in two steps -> 8 MFMA per
// stage and 48 per element instead of 384 vector FMAs per lane, with 8 LDS reads and 8 LDS writes per lane and stage as the only
// other work.  Operand layout (guide, "f64 MFMA"): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15]: registers 0 and 1 of a lane are outputs o = lane >> 4 and o + 4 of its column,
// registers 2 and 3 belong to the unused rows 8 .. 15.  The cube is stored with the x rows padded to 9 doubles (index
// a + 9 (b + 8 c)) so that the 16 columns of a tile fall into different LDS banks for all three axes.
typedef double v4f64_t __attribute__((ext_vector_type(4)));
template <int AX, bool FWD>
__device__ __forceinline__ void fdm_stage_mfma8(double *__restrict__ buf, const double *__restrict__ sS, int l15, int lg) {
    // A operand of this stage from the element's matrices in LDS: forward = S^T (out[o] = sum_l S[l][o] in[l]), backward = S;
    // rows 8 .. 15 of the tile are zero.  (Held in registers for all six stages they cost 24 VGPRs and a wave per SIMD.)
    const int o = l15 & 7;
    const double live = l15 < 8 ? 1.0 : 0.0;
    const double a0 = live * (FWD ? sS[AX * 64 + lg * 8 + o] : sS[AX * 64 + o * 8 + lg]);
    const double a1 = live * (FWD ? sS[AX * 64 + (lg + 4) * 8 + o] : sS[AX * 64 + o * 8 + lg + 4]);
    constexpr int str = AX == 0 ? 1 : (AX == 1 ? 9 : 72);
    const v4f64_t zero = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // two tiles (32 columns) at a time: half the operand / result registers
        int base[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int col = 16 * (2 * h + t) + l15;
            base[t] = AX == 0 ? 9 * col : (AX == 1 ? (col & 7) + 72 * (col >> 3) : (col & 7) + 9 * (col >> 3));
        }
        double b0[2], b1[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            b0[t] = buf[base[t] + str * lg];
            b1[t] = buf[base[t] + str * (lg + 4)];
        }
        v4f64_t d[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0[t], zero, 0, 0, 0);
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1[t], d[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            buf[base[t] + str * lg] = d[t][0];
            buf[base[t] + str * (lg + 4)] = d[t][1];
        }
    }
}

__global__ __launch_bounds__(64, 4) void k_fdm_ext_mfma8(const double *__restrict__ flag, int64_t E, const double *__restrict__ S,
                                                      const double *__restrict__ lam, double thr, const double *__restrict__ Win,
                                                      double *__restrict__ Wr, double *__restrict__ z, const int *__restrict__ pret,
                                                      int64_t ld, int64_t lW, int nb_fdm, ChainArgs cg) {
    constexpr int N = 8, N2 = 6, NP = 512, NP2 = 216, NF = 216;
    __shared__ double sL[3][N];
    __shared__ double sA[9 * 64];
    if ((int)blockIdx.x >= nb_fdm) {   // merged launch: the blocks behind the elements run the coarse chain up to the dense solve
        chain_body((int)blockIdx.x - nb_fdm, flag, ld, cg);
        return;
    }
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        z += lo, Win += (int64_t)blockIdx.y * lW, Wr += (int64_t)blockIdx.y * lW;
    }
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x, l15 = lane & 15, lg = lane >> 4;
    const int64_t e = blockIdx.x;
    const double *__restrict__ Sg = S + e * (3 * N * N);
    __shared__ double sS[3 * N * N];
#pragma unroll
    for (int m = 0; m < 3; ++m) sS[m * N * N + lane] = Sg[m * N * N + lane];
    if (lane < 3 * N) sL[lane / N][lane % N] = lam[e * (3 * N) + lane];
    // one coalesced round trip: the extended grid (point q = lane + 64 u: a = lane & 7, b = lane >> 3, c = u), and the
    // destinations of the ghost values (kept in registers for the store phase; clamped loads at the points that are not face points)
    int pr[8];
    {
        const double *We = Win + e * NP;
        const int *pe = pret + e * NF;
        double w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = lane + 64 * u, a = q & 7, b = (q >> 3) & 7, c = q >> 6;
            const int nb = (a == 0 || a == N - 1) + (b == 0 || b == N - 1) + (c == 0 || c == N - 1);
            w[u] = We[q];
            pr[u] = pe[nb == 1 ? face_pt(N, a, b, c) : 0];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = lane + 64 * u;
            sA[q + (q >> 3)] = w[u];
        }
    }
    __syncthreads();
    fdm_stage_mfma8<0, true>(sA, sS, l15, lg);
    __syncthreads();
    fdm_stage_mfma8<1, true>(sA, sS, l15, lg);
    __syncthreads();
    fdm_stage_mfma8<2, true>(sA, sS, l15, lg);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = lane + 64 * u;
        const double den = sL[0][q % N] + sL[1][(q / N) % N] + sL[2][q / (N * N)];
        const double v = sA[q + (q >> 3)];
        sA[q + (q >> 3)] = den > thr ? v / den : 0.0;
    }
    __syncthreads();
    fdm_stage_mfma8<2, false>(sA, sS, l15, lg);
    __syncthreads();
    fdm_stage_mfma8<1, false>(sA, sS, l15, lg);
    __syncthreads();
    fdm_stage_mfma8<0, false>(sA, sS, l15, lg);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = lane + 64 * u, a = q & 7, b = (q >> 3) & 7, c = q >> 6;
        const int nb = (a == 0 || a == N - 1) + (b == 0 || b == N - 1) + (c == 0 || c == N - 1);
        const double v = sA[q + (q >> 3)];
        if (nb == 0)
            z[e * NP2 + (a - 1) + N2 * ((b - 1) + N2 * (c - 1))] = v;
        else if (nb == 1 && pr[u] >= 0)
            Wr[pr[u]] = v;   // ghost value: belongs to the neighbour's adjacent layer
    }
}

// z += (neighbours' ghost values at this point: at most three return slots of the element's own faces) x wq + prolonged
// coarse correction; r.z and z sums

template <int N>
__global__ __launch_bounds__(NT) void k_sch_finish(const double *__restrict__ flag, int64_t E, const double *__restrict__ W,
                                                   const double *__restrict__ r, const double *__restrict__ wq,
                                                   const double *__restrict__ xc, const double *__restrict__ xa,
                                                   const int *__restrict__ agg, const int *__restrict__ vg, Hat hat,
                                                   double *__restrict__ z, double *__restrict__ part,
                                                   int64_t ld, int64_t lW, int64_t lv, int64_t la) {
    constexpr int N2 = N - 2, NP = N * N * N, NP2 = N2 * N2 * N2;
    __shared__ double sred[8];
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        r += lo, z += lo, W += (int64_t)blockIdx.y * lW;
        if (part) part += lo;
        if (xc) xc += (int64_t)blockIdx.y * lv, xa += (int64_t)blockIdx.y * la;
    }
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wv;
    const bool act = e < E;
    double srz = 0.0, sz = 0.0;
    if (act) {
        // all loads of a group of points first, unconditional and with clamped indices (a conditional load inside the point
        // loop costs a branch and a full wait per point), then the arithmetic with selects
        constexpr int NIT = 4;   // points per lane in flight (lx1 = 8: the whole element)
        constexpr int M = N2, MM = N2 * N2, FB = 8 + 12 * N2;   // FB: first face slot of the face-grouped layout (fg_slot)
        const double *We = W + e * NP;
        double cv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) cv[c] = 0.0;
        for (int q0 = 0; q0 < NP2; q0 += 64 * NIT) {
            double zv[NIT], qv[NIT], rv[NIT], gh[NIT][3];
            int sl[NIT][3];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int q = q0 + lane + 64 * it;
                const int qc = q < NP2 ? q : 0;
                const int64_t i = e * NP2 + qc;
                zv[it] = z[i];
                qv[it] = wq[i];
                rv[it] = r[i];
                const int a = qc % N2, b = (qc / N2) % N2, c = qc / (N2 * N2);   // return slots of the faces next to qc
                sl[it][0] = a == 0 ? FB + b + M * c : (a == M - 1 ? FB + MM + b + M * c : -1);
                sl[it][1] = b == 0 ? FB + 2 * MM + a + M * c : (b == M - 1 ? FB + 3 * MM + a + M * c : -1);
                sl[it][2] = c == 0 ? FB + 4 * MM + a + M * b : (c == M - 1 ? FB + 5 * MM + a + M * b : -1);
            }
            if (q0 == 0 && xc) {
                int vv[8], av[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) vv[c] = vg[e * 8 + c];
#pragma unroll
                for (int c = 0; c < 8; ++c) av[c] = agg[vv[c]];
#pragma unroll
                for (int c = 0; c < 8; ++c) cv[c] = xc[vv[c]] + xa[av[c]];
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it)
#pragma unroll
                for (int d = 0; d < 3; ++d) gh[it][d] = We[sl[it][d] >= 0 ? sl[it][d] : 0];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int q = q0 + lane + 64 * it;
                if (q >= NP2) continue;
                const int a = q % N2, b = (q / N2) % N2, c = q / (N2 * N2);
                double v = zv[it];
                v += sl[it][0] >= 0 ? gh[it][0] : 0.0;
                v += sl[it][1] >= 0 ? gh[it][1] : 0.0;
                v += sl[it][2] >= 0 ? gh[it][2] : 0.0;
                v *= qv[it];
                const double ha = hat.h1[a], hb = hat.h1[b], hc = hat.h1[c];
                const double c0 = cv[0] + ha * (cv[1] - cv[0]), c1 = cv[2] + ha * (cv[3] - cv[2]);
                const double d0 = cv[4] + ha * (cv[5] - cv[4]), d1 = cv[6] + ha * (cv[7] - cv[6]);
                double cc = c0 + hb * (c1 - c0);
                cc += hc * ((d0 + hb * (d1 - d0)) - cc);
                v += cc;
                z[e * NP2 + q] = v;
                srz += rv[it] * v;
                sz += v;
            }
        }
    }
    if (part) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            srz += __shfl_down(srz, o, 64);
            sz += __shfl_down(sz, o, 64);
        }
        if (lane == 0) {
            sred[wv] = srz;
            sred[4 + wv] = sz;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            part[blockIdx.x] = sred[0] + sred[1] + sred[2] + sred[3];
            part[gridDim.x + blockIdx.x] = sred[4] + sred[5] + sred[6] + sred[7];
        }
    }
}

// ---- 2-D twins: Win and Wret are velocity-shaped fields in the natural layout (N x N per element), the ghost layers are the
// interior points of the element edges; one wave per element, four elements per block, one lane per extended point.
template <int N, bool FWD, int AX>
__device__ __forceinline__ void fdm_stage2(const double *__restrict__ in, double *__restrict__ out,
                                           const double *__restrict__ S, int p) {
    // out[o, b] = sum_l Sop[o][l] in[l, b] along axis AX; Sop = S^T (FWD) or S;  S row-major [point][mode]
    const int a = p % N, b = p / N;
    const int o = AX == 0 ? a : b;
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < N; ++l) {
        const double sv = FWD ? S[l * N + o] : S[o * N + l];
        acc += sv * (AX == 0 ? in[l + N * b] : in[a + N * l]);
    }
    out[p] = acc;
}

template <int N>
__global__ __launch_bounds__(NT) void k_fdm_ext2(const double *__restrict__ flag, int64_t E, const double *__restrict__ S,
                                                 const double *__restrict__ lam, double thr, const double *__restrict__ Win,
                                                 double *__restrict__ Wr, double *__restrict__ z, const int *__restrict__ pret,
                                                 int64_t ld, int64_t lW, int nb_fdm, ChainArgs cg) {
    static_assert(N * N <= 64, "one lane per extended point");
    constexpr int N2 = N - 2, NP = N * N, NP2 = N2 * N2, NF = 4 * N2;
    __shared__ double sS[4][2][N * N];
    __shared__ double sA[4][NP], sB[4][NP];
    if ((int)blockIdx.x >= nb_fdm) {   // merged launch: the coarse chain up to the dense solve (see k_fdm_ext)
        chain_body((int)blockIdx.x - nb_fdm, flag, ld, cg);
        return;
    }
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        z += lo, Win += (int64_t)blockIdx.y * lW, Wr += (int64_t)blockIdx.y * lW;
    }
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wv;
    const bool act = e < E;
    const int64_t ee = act ? e : 0;
    for (int q = lane; q < 2 * N * N; q += 64) sS[wv][q / (N * N)][q % (N * N)] = S[ee * (3 * N * N) + q];
    const bool on = lane < NP;
    const int p = on ? lane : 0;
    const int a = p % N, b = p / N;
    const int nb = (a == 0 || a == N - 1) + (b == 0 || b == N - 1);
    const int pr = pret[ee * NF + (nb == 1 ? face_pt<2>(N, a, b) : 0)];
    if (on) sA[wv][p] = Win[ee * NP + p];
    __syncthreads();
    if (on) fdm_stage2<N, true, 0>(sA[wv], sB[wv], sS[wv][0], p);
    __syncthreads();
    if (on) fdm_stage2<N, true, 1>(sB[wv], sA[wv], sS[wv][1], p);
    __syncthreads();
    if (on) {
        const double den = lam[ee * (3 * N) + a] + lam[ee * (3 * N) + N + b];
        sA[wv][p] = den > thr ? sA[wv][p] / den : 0.0;
    }
    __syncthreads();
    if (on) fdm_stage2<N, false, 1>(sA[wv], sB[wv], sS[wv][1], p);
    __syncthreads();
    if (on) fdm_stage2<N, false, 0>(sB[wv], sA[wv], sS[wv][0], p);
    __syncthreads();
    if (act && on) {
        if (nb == 0)
            z[e * NP2 + (a - 1) + N2 * (b - 1)] = sA[wv][p];
        else if (nb == 1 && pr >= 0)
            Wr[pr] = sA[wv][p];   // ghost value: belongs to the neighbour's adjacent layer
    }
}

// z += (neighbours' ghost values at this point: at most two return slots of the element's own faces) x wq + prolonged
// coarse correction; r.z and z sums.  One wave per element, four elements per block: the partial sums of k_sch_finish
template <int N>
__global__ __launch_bounds__(NT) void k_sch_finish2(const double *__restrict__ flag, int64_t E, const double *__restrict__ W,
                                                    const double *__restrict__ r, const double *__restrict__ wq,
                                                    const double *__restrict__ xc, const double *__restrict__ xa,
                                                    const int *__restrict__ agg, const int *__restrict__ vg, Hat hat,
                                                    double *__restrict__ z, double *__restrict__ part,
                                                    int64_t ld, int64_t lW, int64_t lv, int64_t la) {
    constexpr int N2 = N - 2, NP = N * N, NP2 = N2 * N2;
    static_assert(NP2 <= 64, "one lane per point");
    __shared__ double sred[8];
    {   // blockIdx.y = lane of a block step
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        r += lo, z += lo, W += (int64_t)blockIdx.y * lW;
        if (part) part += lo;
        if (xc) xc += (int64_t)blockIdx.y * lv, xa += (int64_t)blockIdx.y * la;
    }
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wv;
    double srz = 0.0, sz = 0.0;
    if (e < E && lane < NP2) {
        const int a = lane % N2, b = lane / N2;
        const int64_t i = e * NP2 + lane;
        const double *We = W + e * NP;
        double v = z[i];
        if (a == 0) v += We[0 + N * (b + 1)];
        if (a == N2 - 1) v += We[(N - 1) + N * (b + 1)];
        if (b == 0) v += We[(a + 1) + N * 0];
        if (b == N2 - 1) v += We[(a + 1) + N * (N - 1)];
        v *= wq[i];
        if (xc) {
            double cv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int vv = vg[e * 4 + c];
                cv[c] = xc[vv] + xa[agg[vv]];
            }
            const double ha = hat.h1[a], hb = hat.h1[b];
            const double c0 = cv[0] + ha * (cv[1] - cv[0]), c1 = cv[2] + ha * (cv[3] - cv[2]);
            v += c0 + hb * (c1 - c0);
        }
        z[i] = v;
        srz = r[i] * v;
        sz = v;
    }
    if (part) {   // first-stage sums of the PCG: part[blk] = sum r.z, part[nblk + blk] = sum z
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            srz += __shfl_down(srz, o, 64);
            sz += __shfl_down(sz, o, 64);
        }
        if (lane == 0) {
            sred[wv] = srz;
            sred[4 + wv] = sz;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            part[blockIdx.x] = sred[0] + sred[1] + sred[2] + sred[3];
            part[gridDim.x + blockIdx.x] = sred[4] + sred[5] + sred[6] + sred[7];
        }
    }
}

// t[e][c] = sum_q phi_c(q) r_e(q): the element-local part of R_1^T r, one wave per element
template <int DIM>
__global__ __launch_bounds__(NT) void k_q1_restrict_local(const double *__restrict__ flag, int64_t E, int n2, Hat hat,
                                                          double *__restrict__ r, double *__restrict__ t,
                                                          double *__restrict__ W, const double *__restrict__ wq,
                                                          const int *__restrict__ pin, nlg_pcg_upd u, int64_t ld = 0, int64_t lt = 0,
                                                          int64_t lW = 0) {
    __shared__ double srr[4];
    {   // blockIdx.y = lane of a block step: solver fields ld doubles apart (the integrator's slab), the preconditioner's own scratch at its strides
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        r += lo;
        t += (int64_t)blockIdx.y * lt;
        if (W) W += (int64_t)blockIdx.y * lW;
        if (u.alpha) u.alpha += lo, u.wmean += lo, u.w += lo, u.rr_part += lo;
        if (u.x) u.x += lo, u.p += lo;   // (x == null: deferred solution update, the directions stay in the ring of the solver)
    }
    if (flag && flag[0] != 0.0) return;
    constexpr int NC = 1 << DIM;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wid;
    const bool act = e < E;
    const int np2 = DIM == 3 ? n2 * n2 * n2 : n2 * n2;
    const bool upd = u.alpha != nullptr;
    const double alpha = upd ? u.alpha[0] : 0.0, wmean = upd ? u.wmean[0] : 0.0;
    double rr = 0.0;
    double a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = 0.0;
    for (int q = lane; act && q < np2; q += 64) {
        double v = r[e * np2 + q];
        if (upd) {   // the PCG update of this point: the new residual is what gets restricted
            const int64_t i = e * np2 + q;
            if (u.x) u.x[i] += alpha * u.p[i];
            v -= alpha * (u.w[i] - wmean);
            r[i] = v;
            rr += v * v * u.nw[i];
        }
        const double ha = hat.h1[q % n2], hb = hat.h1[(q / n2) % n2];
        const double hc = DIM == 3 ? hat.h1[q / (n2 * n2)] : 0.0;
        if (W) {
            // overlapping Schwarz: the own value into the interior of the element's extended grid, and the layers adjacent to
            // the element faces straight into the ghost slots of the neighbours' extended grids (pin, pprec_setup)
            const int N = n2 + 2, M = n2, a = q % n2, b = (q / n2) % n2, c = DIM == 3 ? q / (n2 * n2) : 0;
            const int F = DIM == 3 ? n2 * n2 : n2;   // points per face
            const double vw = v * wq[e * np2 + q];
            W[e * (int64_t)(DIM == 3 ? N * N * N : N * N) + (a + 1) + N * ((b + 1) + (DIM == 3 ? N * (c + 1) : 0))] = vw;
            const int *pe = pin + e * (int64_t)(2 * DIM * F);
            int pk;
            if (a == 0 && (pk = pe[0 * F + b + M * c]) >= 0) W[pk] = vw;
            if (a == M - 1 && (pk = pe[1 * F + b + M * c]) >= 0) W[pk] = vw;
            if (b == 0 && (pk = pe[2 * F + a + M * c]) >= 0) W[pk] = vw;
            if (b == M - 1 && (pk = pe[3 * F + a + M * c]) >= 0) W[pk] = vw;
            if (DIM == 3 && c == 0 && (pk = pe[4 * F + a + M * b]) >= 0) W[pk] = vw;
            if (DIM == 3 && c == M - 1 && (pk = pe[5 * F + a + M * b]) >= 0) W[pk] = vw;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double w = ((c & 1) ? ha : 1.0 - ha) * ((c & 2) ? hb : 1.0 - hb);
            if (DIM == 3) w *= (c & 4) ? hc : 1.0 - hc;
            a[c] += w * v;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[c] += __shfl_down(a[c], o, 64);
    }
    if (lane == 0 && act) {
#pragma unroll
        for (int c = 0; c < NC; ++c) t[e * NC + c] = a[c];
    }
    if (upd) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rr += __shfl_down(rr, o, 64);
        if (lane == 0) srr[wid] = rr;
        __syncthreads();
        if (threadIdx.x == 0) u.rr_part[blockIdx.x] = (srr[0] + srr[1]) + (srr[2] + srr[3]);
    }
}

// The same for 3-D with the pressure-mesh size known at compile time (lx1 = 8, 10, 12): the point loop is unrolled, so all loads
// of a wave are in flight at once and the index arithmetic is constant-folded; the destinations of the layer values in the
// neighbours' extended grids (pin) are loaded with the residual, not after it.  Same summation order as the generic kernel:
// bit-identical results.
template <int N2>
__global__ __launch_bounds__(NT) void k_q1_restrict_local3s(const double *__restrict__ flag, int64_t E, Hat hat, double *__restrict__ r,
                                                            double *__restrict__ t, double *__restrict__ W, const double *__restrict__ wq,
                                                            const int *__restrict__ pin, nlg_pcg_upd u, int64_t ld, int64_t lt, int64_t lW) {
    __shared__ double srr[4];
    {   // blockIdx.y = lane of a block step: solver fields ld doubles apart (the integrator's slab), the preconditioner's own scratch at its strides
        const int64_t lo = (int64_t)blockIdx.y * ld;
        if (flag) flag += lo;
        r += lo;
        t += (int64_t)blockIdx.y * lt;
        if (W) W += (int64_t)blockIdx.y * lW;
        if (u.alpha) u.alpha += lo, u.wmean += lo, u.w += lo, u.rr_part += lo;
        if (u.x) u.x += lo, u.p += lo;   // (x == null: deferred solution update, the directions stay in the ring of the solver)
    }
    if (flag && flag[0] != 0.0) return;
    constexpr int NP2 = N2 * N2 * N2, N = N2 + 2, NIT = 4;   // four points per lane in flight (lx1 = 8: the whole element)
    constexpr int M = N2, MM = N2 * N2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wid;
    const bool act = e < E;
    const bool upd = u.alpha != nullptr;
    const double alpha = upd ? u.alpha[0] : 0.0, wmean = upd ? u.wmean[0] : 0.0;
    const int *__restrict__ pe = pin + (act ? e : 0) * (6 * MM);
    double rr = 0.0;
    double a[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] = 0.0;
    for (int q0 = 0; q0 < NP2; q0 += 64 * NIT) {
        double v[NIT], pv[NIT], wv[NIT], xv[NIT], nv[NIT], qv[NIT], hh[NIT][3];
        int pk[NIT][3], kk[NIT][3];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int q = q0 + lane + 64 * it;
            const int qc = q < NP2 ? q : 0;                 // (unconditional loads at clamped addresses: no branch, no wait per point)
            const int64_t i = (act ? e : 0) * NP2 + qc;
            v[it] = r[i];
            if (upd) {
                wv[it] = u.w[i];
                nv[it] = u.nw[i];
                if (u.x) pv[it] = u.p[i], xv[it] = u.x[i];
            }
            if (W) {
                qv[it] = wq[i];
                // face point next to qc in each direction (-1: qc is not in that boundary layer) -> its destination
                const int ia = qc % N2, ib = (qc / N2) % N2, ic = qc / (N2 * N2);
                const int k0 = ia == 0 ? ib + M * ic : (ia == M - 1 ? MM + ib + M * ic : -1);
                const int k1 = ib == 0 ? 2 * MM + ia + M * ic : (ib == M - 1 ? 3 * MM + ia + M * ic : -1);
                const int k2 = ic == 0 ? 4 * MM + ia + M * ib : (ic == M - 1 ? 5 * MM + ia + M * ib : -1);
                pk[it][0] = pe[k0 >= 0 ? k0 : 0];   // (clamped, selected below)
                pk[it][1] = pe[k1 >= 0 ? k1 : 0];
                pk[it][2] = pe[k2 >= 0 ? k2 : 0];
                kk[it][0] = k0, kk[it][1] = k1, kk[it][2] = k2;
            }
            hh[it][0] = hat.h1[qc % N2], hh[it][1] = hat.h1[(qc / N2) % N2], hh[it][2] = hat.h1[qc / (N2 * N2)];   // (a load too)
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int q = q0 + lane + 64 * it;
            if (!(act && q < NP2)) continue;
            const int64_t i = e * NP2 + q;
            double vv = v[it];
            if (upd) {
                if (u.x) u.x[i] = xv[it] + alpha * pv[it];
                vv -= alpha * (wv[it] - wmean);
                r[i] = vv;
                rr += vv * vv * nv[it];
            }
            const double ha = hh[it][0], hb = hh[it][1], hc = hh[it][2];
            if (W) {
                const int ia = q % N2, ib = (q / N2) % N2, ic = q / (N2 * N2);
                const double vw = vv * qv[it];
                W[e * (int64_t)(N * N * N) + (ia + 1) + N * ((ib + 1) + N * (ic + 1))] = vw;   // own value: interior of the extended grid
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    if (kk[it][d] >= 0 && pk[it][d] >= 0) W[pk[it][d]] = vw;   // layer value: a neighbour's ghost slot
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                double w = ((c & 1) ? ha : 1.0 - ha) * ((c & 2) ? hb : 1.0 - hb);
                w *= (c & 4) ? hc : 1.0 - hc;
                a[c] += w * vv;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[c] += __shfl_down(a[c], o, 64);
    }
    if (lane == 0 && act) {
#pragma unroll
        for (int c = 0; c < 8; ++c) t[e * 8 + c] = a[c];
    }
    if (upd) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rr += __shfl_down(rr, o, 64);
        if (lane == 0) srr[wid] = rr;
        __syncthreads();
        if (threadIdx.x == 0) u.rr_part[blockIdx.x] = (srr[0] + srr[1]) + (srr[2] + srr[3]);
    }
}

// rc[v] = sum of t over the (element, corner) entries incident to vertex v (fixed order), and the first damped-Jacobi
// sweep from a zero guess
__global__ __launch_bounds__(NT) void k_q1_gather(const double *__restrict__ flag, int nvert, const int *__restrict__ vp,
                                                  const int *__restrict__ vi, const double *__restrict__ t,
                                                  double *__restrict__ rc, const double *__restrict__ dinv, double om,
                                                  double *__restrict__ x, int64_t ld = 0, int64_t lt = 0, int64_t lv = 0) {
    if (flag) flag += (int64_t)blockIdx.y * ld;
    t += (int64_t)blockIdx.y * lt, rc += (int64_t)blockIdx.y * lv, x += (int64_t)blockIdx.y * lv;
    if (flag && flag[0] != 0.0) return;
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= nvert) return;
    double a = 0.0;
    for (int q = vp[v]; q < vp[v + 1]; ++q) a += t[vi[q]];
    rc[v] = a;
    x[v] = om * dinv[v] * a;
}

// probing vector of the coarse-operator assembly: p = phi_c on the elements of colour `col`, 0 elsewhere
template <int DIM>
__global__ __launch_bounds__(NT) void k_q1_probe(int64_t E, int n2, Hat hat, const int *__restrict__ colour, int col, int c,
                                                 double *__restrict__ p) {
    const int np2 = DIM == 3 ? n2 * n2 * n2 : n2 * n2;
    const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
    if (i >= E * np2) return;
    const int64_t e = i / np2;
    const int q = (int)(i % np2);
    double w = 0.0;
    if (colour[e] == col) {
        const double ha = hat.h1[q % n2], hb = hat.h1[(q / n2) % n2];
        w = ((c & 1) ? ha : 1.0 - ha) * ((c & 2) ? hb : 1.0 - hb);
        if (DIM == 3) {
            const double hc = hat.h1[q / (n2 * n2)];
            w *= (c & 4) ? hc : 1.0 - hc;
        }
    }
    p[i] = w;
}

// probing vector of the GLOBAL aggregate operator (several ranks): p = R_1 P_a e_a, the prolongation of the indicator
// of aggregate `a` (a < 0: this rank is not the probing one, p = 0)
template <int DIM>
__global__ __launch_bounds__(NT) void k_agg_probe(int64_t E, int n2, Hat hat, const int *__restrict__ vg,
                                                  const int *__restrict__ agg, int a, double *__restrict__ p) {
    constexpr int NC = 1 << DIM;
    const int np2 = DIM == 3 ? n2 * n2 * n2 : n2 * n2;
    const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
    if (i >= E * np2) return;
    double w = 0.0;
    if (a >= 0) {
        const int64_t e = i / np2;
        const int q = (int)(i % np2);
        const double ha = hat.h1[q % n2], hb = hat.h1[(q / n2) % n2];
        const double hc = DIM == 3 ? hat.h1[q / (n2 * n2)] : 0.0;
        for (int c = 0; c < NC; ++c)
            if (agg[vg[e * NC + c]] == a) {
                double t = ((c & 1) ? ha : 1.0 - ha) * ((c & 2) ? hb : 1.0 - hb);
                if (DIM == 3) t *= (c & 4) ? hc : 1.0 - hc;
                w += t;
            }
    }
    p[i] = w;
}

// column `col` of this rank's rows of the global aggregate operator
__global__ void k_store_col(int na, const double *__restrict__ ra, double *__restrict__ rows, int64_t ncols, int64_t col) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) rows[(size_t)i * ncols + col] = ra[i];
}

// gathered operator -> invertible: unit diagonal on the padding rows, symmetrised, constant null space shifted
__global__ void k_glob_fix(int64_t n, int na_max, const int *__restrict__ na_of, double alpha, double *__restrict__ A) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= n || j < i) return;
    const bool ri = (int)(i % na_max) < na_of[i / na_max], rj = (int)(j % na_max) < na_of[j / na_max];
    double v;
    if (ri && rj)
        v = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]) + alpha;
    else
        v = i == j ? 1.0 : 0.0;
    A[(size_t)i * n + j] = v;
    A[(size_t)j * n + i] = v;
}

__global__ void k_mirror_upper(int n, double *__restrict__ A) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < i) A[(size_t)i * n + j] = A[(size_t)j * n + i];
}

// ra[a] = sum of rr over the members of aggregate a, one wave per aggregate
__global__ __launch_bounds__(NT) void k_agg_restrict(const double *flag, int na, const int *__restrict__ ap,
                                                     const int *__restrict__ am, const double *__restrict__ rr,
                                                     double *__restrict__ ra, int64_t ld = 0, int64_t lv = 0, int64_t la = 0) {
    if (flag) flag += (int64_t)blockIdx.y * ld;
    rr += (int64_t)blockIdx.y * lv, ra += (int64_t)blockIdx.y * la;
    if (flag && flag[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int a = blockIdx.x * 4 + wid;
    if (a >= na) return;
    double s = 0.0;
    for (int q = ap[a] + lane; q < ap[a + 1]; q += 64) s += rr[am[q]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) ra[a] = s;
}

// xa = Ainv ra (dense, row-major), one wave per row.  T = float for the global aggregate level of several ranks: the
// rows of the inverse are the largest per-iteration read there (2.4k x 19.6k at 8 x 10^4 elements), a preconditioner
// needs no more than single precision, and the symmetric matrix is rounded entry by entry, so it stays symmetric
// across the ranks that hold its rows; sums in double.
template <typename T>
struct GemvArgs {
    int na, ncols;
    const T *Ainv;
    const double *ra;
    double *xa;
    int64_t la;
    int na_max, nlanes;
};
// lanes of a block step (blockIdx.y): one rank -- ra, xa la doubles apart; several ranks -- ra is the all-gathered array
// [rank][lane][na_max] (na_max > 0), column c of the global aggregate level = entry c % na_max of rank c / na_max
template <typename T>
__device__ __forceinline__ void dense_gemv_body(int bx, const double *flag, int64_t ld, const GemvArgs<T> &g) {
    if (flag) flag += (int64_t)blockIdx.y * ld;
    if (flag && flag[0] != 0.0) return;
    double *xa = g.xa + (int64_t)blockIdx.y * g.la;
    const double *ra = g.na_max == 0 ? g.ra + (int64_t)blockIdx.y * g.la : g.ra;
    const int na = g.na, ncols = g.ncols;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = bx * 4 + wid;
    if (row >= na) return;
    const T *__restrict__ Ar = g.Ainv + (size_t)row * ncols;
    double s = 0.0;
    if (g.na_max > 0 && g.nlanes > 1) {   // (strided gather of the lane's entries; set-up sizes: a few thousand columns)
        for (int j = lane; j < ncols; j += 64)
            s += (double)Ar[j] * ra[((int64_t)(j / g.na_max) * g.nlanes + blockIdx.y) * g.na_max + j % g.na_max];
    } else {
        // eight loads of the row in flight per lane (same summation order as the plain loop: the products are added one after the
        // other); a wave per row gives only ~1.3 waves per SIMD at 1300 rows, so the loads of one wave must overlap themselves
        int j = lane;
        for (; j + 7 * 64 < ncols; j += 8 * 64) {
            double av[8], rv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                av[u] = (double)Ar[j + 64 * u];
                rv[u] = ra[j + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += av[u] * rv[u];
        }
        for (; j < ncols; j += 64) s += (double)Ar[j] * ra[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) xa[row] = s;
}
template <typename T>
__global__ __launch_bounds__(NT) void k_dense_gemv(const double *flag, int na, int ncols, const T *__restrict__ Ainv,
                                                   const double *__restrict__ ra, double *__restrict__ xa, int64_t ld = 0, int64_t la = 0,
                                                   int na_max = 0, int nlanes = 1) {
    const GemvArgs<T> g = {na, ncols, Ainv, ra, xa, la, na_max, nlanes};
    dense_gemv_body<T>((int)blockIdx.x, flag, ld, g);
}

__global__ void k_to_float(int64_t n, const double *__restrict__ a, float *__restrict__ b) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) b[i] = (float)a[i];
}

// ---- dense SPD inverse on the device (set-up): in-place Gauss-Jordan without pivoting, two launches per pivot ----
// rk = row k / pivot, ck = column k (before the step); bad[0] is raised when a pivot is not positive
__global__ __launch_bounds__(NT) void k_gj_prep(int n, int k, const double *__restrict__ A, double *__restrict__ rk,
                                                double *__restrict__ ck, int *__restrict__ bad) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    const double p = A[(size_t)k * n + k];
    if (j == 0 && !(p > 0.0)) bad[0] = 1;
    rk[j] = A[(size_t)k * n + j] / p;
    ck[j] = A[(size_t)j * n + k];
}
__global__ __launch_bounds__(NT) void k_gj_update(int n, int k, double *__restrict__ A, const double *__restrict__ rk,
                                                  const double *__restrict__ ck) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    const double p = ck[k];   // the pivot
    double v;
    if (i == k)
        v = j == k ? 1.0 / p : rk[j];
    else
        v = j == k ? -ck[i] / p : A[(size_t)i * n + j] - ck[i] * rk[j];
    A[(size_t)i * n + j] = v;
}

// ---- set-up: the device parts (the host arithmetic of the stages is in pprec_host.cpp) ---------------------------------
template <typename T>
int up(const std::vector<T> &v, T **d) {
    NLG_HIP(hipMalloc(d, sizeof(T) * std::max<size_t>(v.size(), 1)));
    if (!v.empty()) NLG_HIP(hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return 0;
}

struct HaloOff {   // the operator without the halo exchange for the life of the guard
    nlg_halo &h;
    const bool was;
    explicit HaloOff(nlg_halo &halo) : h(halo), was(halo.active) { h.active = false; }
    ~HaloOff() { h.active = was; }
};
struct BlasHandle {
    rocblas_handle h = nullptr;
    ~BlasHandle() { if (h) rocblas_destroy_handle(h); }
};

int env_int(const char *name, int dflt) {
    const char *ev = getenv(name);
    return ev ? atoi(ev) : dflt;
}
// a host stage's failure becomes the library's error
int stage(int rc, const std::string &err) {
    if (rc) set_error("%s", err.c_str());
    return rc;
}

Hat hat_of(const nlg_mesh *m) {
    Hat hat;
    for (int k = 0; k < 12; ++k) hat.h1[k] = k < m->n2 ? m->pprec.hat1[k] : 0.0;
    return hat;
}
// pp = the hat of corner c of every element of colour `col`
void probe_vertex(nlg_mesh *m, const int *d_colour, int col, int c, double *pp) {
    const dim3 gp((unsigned)((m->lpn + NT - 1) / NT));
    if (m->dim == 3)
        NLG_LAUNCH(k_q1_probe<3>, gp, dim3(NT), 0, m->ctx->stream, m->E, m->n2, hat_of(m), d_colour, col, c, pp);
    else
        NLG_LAUNCH(k_q1_probe<2>, gp, dim3(NT), 0, m->ctx->stream, m->E, m->n2, hat_of(m), d_colour, col, c, pp);
}
// pp = the indicator of aggregate a prolonged to the pressure points (a < 0: zero)
void probe_aggregate(nlg_mesh *m, int a, double *pp) {
    const nlg_pprec &P = m->pprec;
    const dim3 gp((unsigned)((m->lpn + NT - 1) / NT));
    if (m->dim == 3)
        NLG_LAUNCH(k_agg_probe<3>, gp, dim3(NT), 0, m->ctx->stream, m->E, m->n2, hat_of(m), (const int *)P.d_vg, (const int *)P.d_agg, a, pp);
    else
        NLG_LAUNCH(k_agg_probe<2>, gp, dim3(NT), 0, m->ctx->stream, m->E, m->n2, hat_of(m), (const int *)P.d_vg, (const int *)P.d_agg, a, pp);
}
// out[e][corner] = R_1^T ep per element, the plain restriction (no extended grids, no PCG update)
void restrict_corners(nlg_mesh *m, double *ep, double *out) {
    const dim3 ge((unsigned)((m->E + 3) / 4));
    if (m->dim == 3)
        NLG_LAUNCH(k_q1_restrict_local<3>, ge, dim3(NT), 0, m->ctx->stream, (const double *)nullptr, m->E, m->n2, hat_of(m), ep, out, (double *)nullptr, (const double *)nullptr, (const int *)nullptr, nlg_pcg_upd{});
    else
        NLG_LAUNCH(k_q1_restrict_local<2>, ge, dim3(NT), 0, m->ctx->stream, (const double *)nullptr, m->E, m->n2, hat_of(m), ep, out, (double *)nullptr, (const double *)nullptr, (const int *)nullptr, nlg_pcg_upd{});
}

// hw <- QQ^T hw through the device.  Halo on: a face neighbour on another rank counts like a local one (its ghost layer
// travels with the halo exchange of the array W, pprec_apply)
int sum_face_lengths(nlg_mesh *m, std::vector<double> &hw) {
    hipStream_t st = m->ctx->stream;
    double *dw = sem_scratch1(m, 0);
    NLG_CHECK(dw, "pprec_setup: scratch allocation failed");
    NLG_HIP(hipMemcpyAsync(dw, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice, st));
    double *f1[1] = {dw};
    NLG_TRY(sem_gs(m, f1, 1));
    NLG_HIP(hipMemcpyAsync(hw.data(), dw, sizeof(double) * hw.size(), hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

// The overlapping variant: extended 1-D operators from the line left neighbour | element | right neighbour, the overlap
// destinations and the exchange arrays (return array Wr in the face-grouped layout in 3-D, in the natural layout in 2-D)
int setup_overlap(nlg_mesh *m, const pph::Shape &s, const pph::Ops &o, const pph::Lengths &L) {
    nlg_pprec &P = m->pprec;
    hipStream_t st = m->ctx->stream;
    std::string err;
    std::vector<double> hw;
    pph::face_lengths(s, L, hw);
    NLG_TRY(sum_face_lengths(m, hw));
    pph::ExtLines X;
    NLG_TRY(stage(pph::extended_lines(s, o, L, hw, X, err), err));
    NLG_TRY(up(X.wq, &P.d_wq));
    P.thrx = X.thrx;
    NLG_TRY(up(X.Sx, &P.d_Sx));
    std::vector<int> pidx((size_t)2 * m->gs.npairs);   // the two-copy groups of the gather-scatter in the layout of Wr
    NLG_HIP(hipMemcpy(pidx.data(), s.dim == 3 ? m->gs.d_indices_fg : m->gs.d_indices, sizeof(int) * pidx.size(), hipMemcpyDeviceToHost));
    pph::OverlapDest D;
    NLG_TRY(stage(pph::overlap_destinations(s, pidx, X.hasnb, m->halo.active, D, err), err));
    NLG_TRY(up(D.pin, &P.d_pin));
    NLG_TRY(up(D.pret, &P.d_pret));
    NLG_HIP(hipMalloc(&P.d_Wr, sizeof(double) * (size_t)m->lvs));
    NLG_HIP(hipMemsetAsync(P.d_Wr, 0, sizeof(double) * (size_t)m->lvs, st));
    NLG_TRY(up(X.lamx, &P.d_lamx));
    NLG_HIP(hipMalloc(&P.d_W, sizeof(double) * (size_t)m->lvs));
    NLG_HIP(hipMemsetAsync(P.d_W, 0, sizeof(double) * (size_t)m->lvs, st));
    P.overlap = true;
    return 0;
}

// A_c = R_1^T E R_1 by probing E on the device (rank-local: without the halo exchange): one E application per
// (colour, corner) gives the 2^dim x 2^dim blocks of every neighbouring pair of elements
int probe_coarse_operator(nlg_mesh *m, const pph::CoarseTopo &T, pph::ProbedRows &rows) {
    hipStream_t st = m->ctx->stream;
    const int NC = 1 << m->dim;
    const int64_t E = m->E;
    DevBuf<int> d_colour;
    DevBuf<double> d_t8;
    NLG_TRY(up(T.colour, &d_colour.p));
    NLG_HIP(hipMalloc(&d_t8.p, sizeof(double) * (size_t)E * NC));
    double *pp = sem_scratch2(m, 0), *ep = sem_scratch2(m, 1);
    NLG_CHECK(pp && ep, "pprec_setup: scratch allocation failed");
    HaloOff halo_off(m->halo);
    rows.assign((size_t)T.nvert, std::unordered_map<int, double>());
    std::vector<double> t8((size_t)E * NC);
    std::vector<int> owner((size_t)E);
    for (int col = 0; col < T.ncol; ++col) {
        std::fill(owner.begin(), owner.end(), -1);
        for (int64_t e = 0; e < E; ++e)
            if (T.colour[e] == col)
                for (int e1 : T.adj[e]) owner[e1] = (int)e;
        for (int c = 0; c < NC; ++c) {
            probe_vertex(m, d_colour.p, col, c, pp);
            NLG_TRY(sem_cdabdtp(m, pp, ep));
            restrict_corners(m, ep, d_t8.p);
            if (hipMemcpyAsync(t8.data(), d_t8.p, sizeof(double) * t8.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) {
                set_error("pprec_setup: device error while probing the coarse operator");
                return 1;
            }
            for (int64_t e1 = 0; e1 < E; ++e1) {
                const int e0 = owner[e1];
                if (e0 < 0) continue;
                const int vcol = T.vg[(size_t)e0 * NC + c];
                for (int c1 = 0; c1 < NC; ++c1) {
                    const double val = t8[(size_t)e1 * NC + c1];
                    if (val != 0.0) rows[T.vg[(size_t)e1 * NC + c1]][vcol] += val;
                }
            }
        }
    }
    return 0;
}

// dense SPD inverse in place (row-major): Gauss-Jordan without pivoting, two launches per pivot
int gj_inverse(hipStream_t st, double *dA, int nn) {
    DevBuf<double> rk, ck;
    DevBuf<int> bad;
    int hbad = 0;
    NLG_HIP(hipMalloc(&rk.p, sizeof(double) * (size_t)nn));
    NLG_HIP(hipMalloc(&ck.p, sizeof(double) * (size_t)nn));
    NLG_HIP(hipMalloc(&bad.p, sizeof(int)));
    NLG_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), st));
    const unsigned gx = (unsigned)((nn + NT - 1) / NT);
    for (int k = 0; k < nn; ++k) {
        NLG_LAUNCH(k_gj_prep, dim3(gx), dim3(NT), 0, st, nn, k, (const double *)dA, rk.p, ck.p, bad.p);
        NLG_LAUNCH(k_gj_update, dim3(gx, (unsigned)nn), dim3(NT), 0, st, nn, k, dA, (const double *)rk.p, (const double *)ck.p);
    }
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    NLG_CHECK(hbad == 0, "pprec_setup: aggregate operator is not positive definite");
    return 0;
}

// The dense inverse of the aggregate level.  From lib_min unknowns (NLG_LIB_INVERSE_MIN; several ranks): Cholesky
// factorisation and inverse from rocSOLVER — set-up only, a plain dense library call; the two-launches-per-pivot
// Gauss-Jordan above streams the matrix once per pivot (18k unknowns: 25 s)
int spd_inverse_dev(hipStream_t st, double *dA, int nn, int lib_min) {
    if (nn < lib_min) return gj_inverse(st, dA, nn);
    BlasHandle hb;
    NLG_CHECK(rocblas_create_handle(&hb.h) == rocblas_status_success, "pprec_setup: rocblas_create_handle failed");
    rocblas_set_stream(hb.h, st);
    DevBuf<int> dinfo;
    int hinfo[2] = {0, 0};
    NLG_HIP(hipMalloc(&dinfo.p, 2 * sizeof(int)));
    const rocblas_status s1 = rocsolver_dpotrf(hb.h, rocblas_fill_lower, nn, dA, nn, dinfo.p);
    const rocblas_status s2 = s1 == rocblas_status_success ? rocsolver_dpotri(hb.h, rocblas_fill_lower, nn, dA, nn, dinfo.p + 1) : s1;
    NLG_HIP(hipMemcpyAsync(hinfo, dinfo.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    NLG_CHECK(s1 == rocblas_status_success && s2 == rocblas_status_success, "pprec_setup: rocSOLVER potrf/potri failed (%d, %d)", (int)s1, (int)s2);
    NLG_CHECK(hinfo[0] == 0 && hinfo[1] == 0, "pprec_setup: aggregate operator is not positive definite (potrf info %d)", hinfo[0]);
    // column-major lower triangle = row-major upper triangle: mirror it
    NLG_LAUNCH(k_mirror_upper, dim3((unsigned)((nn + 255) / 256), (unsigned)nn), dim3(256), 0, st, nn, dA);
    NLG_HIP(hipGetLastError());
    return 0;
}

// out = the vectors `in` (one length on every rank) of all ranks, one after the other
int gather_host(nlg_ctx *ctx, const std::vector<double> &in, std::vector<double> &out) {
    hipStream_t st = ctx->stream;
    const size_t c = in.size(), nr = (size_t)ctx->nranks;
    DevBuf<double> di, d_o;
    NLG_HIP(hipMalloc(&di.p, sizeof(double) * c));
    NLG_HIP(hipMalloc(&d_o.p, sizeof(double) * c * nr));
    NLG_HIP(hipMemcpyAsync(di.p, in.data(), sizeof(double) * c, hipMemcpyHostToDevice, st));
    NLG_TRY(allgather_f64(ctx, di.p, d_o.p, (int64_t)c));
    out.resize(c * nr);
    NLG_HIP(hipMemcpyAsync(out.data(), d_o.p, sizeof(double) * c * nr, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

// Several ranks: ONE aggregate level over all ranks.  The vertex hats are cut at the rank boundaries (the
// pressure space is discontinuous, so the cut functions are admissible), hence the diagonal block of a rank is the
// halo-free operator assembled before and only the aggregates that touch an element with a shared node couple to
// other ranks.  Those columns are probed with the global operator (halo on), one aggregate of one rank at a time;
// the rows are gathered, the (12k x 12k at 8 x 10^4 elements) operator is inverted redundantly on every rank
// and each rank keeps its own rows of the inverse.  Per application: one all-gather of na_max doubles.
// (Rank-local coarse solves — the first version — took 45 pressure iterations on 2 x 512 elements against 14
// on one rank: the block-Jacobi coarse solve over-corrects the nearly constant-per-rank modes.)
int global_aggregate_level(nlg_mesh *m, const pph::CoarseTopo &T, const std::vector<int> &agg, const pph::AggLevel &G, int lib_min) {
    nlg_pprec &P = m->pprec;
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int nr = ctx->nranks, me = ctx->rank, na = G.na, nvert = T.nvert, NC = 1 << m->dim;
    const int64_t E = m->E;
    const std::vector<double> &Acc = G.Acc;
    // aggregates whose support holds an element with a node shared with another rank
    std::vector<char> velem((size_t)E, 0), aflag((size_t)na, 0);
    for (int idx : m->halo.h_cidx) velem[idx / m->np1] = 1;
    for (int64_t e = 0; e < E; ++e)
        if (velem[e])
            for (int c = 0; c < NC; ++c) aflag[agg[T.vg[(size_t)e * NC + c]]] = 1;
    std::vector<int> ifa;
    for (int a = 0; a < na; ++a)
        if (aflag[a]) ifa.push_back(a);
    double tr = 0.0;
    for (int i = 0; i < na; ++i) tr += Acc[(size_t)i * na + i];
    std::vector<double> info;
    NLG_TRY(gather_host(ctx, {(double)na, (double)ifa.size(), tr}, info));
    std::vector<int> na_all(nr), ni_all(nr);
    int na_max = 0, ni_max = 0;
    double tr_all = 0.0, nreal = 0.0;
    for (int q = 0; q < nr; ++q) {
        na_all[q] = (int)info[3 * q];
        ni_all[q] = (int)info[3 * q + 1];
        tr_all += info[3 * q + 2];
        nreal += na_all[q];
        na_max = std::max(na_max, na_all[q]);
        ni_max = std::max(ni_max, ni_all[q]);
    }
    const int64_t ntot = (int64_t)nr * na_max;
    NLG_CHECK(ntot <= 60000, "pprec_setup: global aggregate level of %lld unknowns is too large for the dense inverse", (long long)ntot);
    std::vector<double> ifa_pad((size_t)std::max(ni_max, 1), -1.0), ifa_all;
    for (size_t i = 0; i < ifa.size(); ++i) ifa_pad[i] = ifa[i];
    NLG_TRY(gather_host(ctx, ifa_pad, ifa_all));
    // this rank's rows: diagonal block from the halo-free assembly, the rest by probing
    DevBuf<double> d_rows, d_full;
    {
        std::vector<double> rowsH((size_t)na_max * ntot, 0.0);
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < na; ++j) rowsH[(size_t)i * ntot + (size_t)me * na_max + j] = Acc[(size_t)i * na + j];
        NLG_TRY(up(rowsH, &d_rows.p));
    }
    NLG_HIP(hipMalloc(&P.d_ra, sizeof(double) * (size_t)na_max));
    NLG_HIP(hipMemsetAsync(P.d_ra, 0, sizeof(double) * (size_t)na_max, st));
    NLG_HIP(hipMalloc(&P.d_rag, sizeof(double) * (size_t)ntot));
    double *pp = sem_scratch2(m, 0), *ep = sem_scratch2(m, 1);
    NLG_CHECK(pp && ep, "pprec_setup: scratch allocation failed");
    const size_t stride_i = (size_t)std::max(ni_max, 1);
    for (int r = 0; r < nr; ++r)
        for (int i = 0; i < ni_all[r]; ++i) {
            const int a_src = (int)ifa_all[(size_t)r * stride_i + i];
            probe_aggregate(m, me == r ? a_src : -1, pp);
            NLG_TRY(sem_cdabdtp(m, pp, ep));
            if (me == r) continue;   // own block: already there
            restrict_corners(m, ep, P.d_tq);
            NLG_LAUNCH(k_q1_gather, dim3((nvert + NT - 1) / NT), dim3(NT), 0, st, (const double *)nullptr, nvert, P.d_v2e_p, P.d_v2e_i, P.d_tq, P.d_rc, P.d_dinv, 0.0, P.d_x);
            NLG_LAUNCH(k_agg_restrict, dim3((na + 3) / 4), dim3(NT), 0, st, (const double *)nullptr, na, P.d_ap, P.d_am, P.d_rc, P.d_ra);
            NLG_LAUNCH(k_store_col, dim3((na + 255) / 256), dim3(256), 0, st, na, (const double *)P.d_ra, d_rows.p, ntot, (int64_t)r * na_max + a_src);
        }
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipMalloc(&d_full.p, sizeof(double) * (size_t)ntot * ntot));
    NLG_TRY(allgather_f64(ctx, d_rows.p, d_full.p, (int64_t)na_max * ntot));
    DevBuf<int> d_na_of;
    NLG_TRY(up(na_all, &d_na_of.p));
    const double alpha = m->has_outflow ? 0.0 : tr_all / nreal / nreal;
    NLG_LAUNCH(k_glob_fix, dim3((unsigned)((ntot + 255) / 256), (unsigned)ntot), dim3(256), 0, st, ntot, na_max, (const int *)d_na_of.p, alpha, d_full.p);
    NLG_TRY(spd_inverse_dev(st, d_full.p, (int)ntot, lib_min));
    const int64_t nrow_el = (int64_t)std::max(na, 1) * ntot;
    NLG_HIP(hipMalloc(&P.d_Ainv32, sizeof(float) * (size_t)nrow_el));
    NLG_LAUNCH(k_to_float, dim3((unsigned)((nrow_el + 255) / 256)), dim3(256), 0, st, (int64_t)na * ntot,
               (const double *)(d_full.p + (size_t)me * na_max * ntot), P.d_Ainv32);
    NLG_HIP(hipGetLastError());
    NLG_HIP(hipStreamSynchronize(st));
    P.na_max = na_max;
    P.ncols = (int)ntot;
    return 0;
}

struct FreeUnlessReady {   // a set-up that fails leaves nlg_pprec empty, never half filled
    nlg_mesh *m;
    ~FreeUnlessReady() { if (!m->pprec.ready) pprec_free(m); }
};

}  // namespace

namespace nlg {

// The stages of the set-up in order: the host arithmetic of pprec_host.cpp with the device work in between.
int pprec_setup(nlg_mesh *m, const nlg_mesh_desc *d) {
    FreeUnlessReady guard{m};
    nlg_pprec &P = m->pprec;
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int exact_max = env_int("NLG_COARSE_EXACT_MAX", 2048);   // more vertices than this: aggregates
    const int lib_min = env_int("NLG_LIB_INVERSE_MIN", 4096);      // from this many unknowns: rocSOLVER
    const bool multi = ctx->distributed() && ctx->nranks > 1;
    const int dim = m->dim, n = m->n, NC = 1 << dim;
    pph::Shape s;
    s.dim = dim, s.n = n, s.n2 = m->n2, s.E = m->E;
    const pph::Ops o = {m->ops.w1.data(), m->ops.w2.data(), m->ops.D12.data(), m->ops.I12.data()};
    std::string err;
    std::vector<double> vmult((size_t)m->lvn);
    NLG_HIP(hipMemcpyAsync(vmult.data(), m->d_vmult, sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    const double *X[3] = {d->xm1, d->ym1, d->zm1};
    const double *msk[3] = {d->v1mask, d->v2mask, d->v3mask};

    // local solves: edge lengths, element-wise fast diagonalisation and, where the mesh has shared faces, the overlap
    pph::Lengths L;
    pph::LocalFdm F;
    pph::edge_lengths(s, X, msk, vmult.data(), L);
    NLG_TRY(stage(pph::local_fdm(s, o, L, F, err), err));
    NLG_TRY(up(F.S, &P.d_S));
    NLG_TRY(up(F.invden, &P.d_invden));
    if (((dim == 3 && m->gs.d_indices_fg && n <= 12 && n != 11) || (dim == 2 && n <= 8)) && m->gs.npairs > 0)
        NLG_TRY(setup_overlap(m, s, o, L));

    // coarse space: element vertices, trilinear hats at the GL points; A_c probed colour by colour
    P.ncorner = NC;
    for (int k = 0; k < m->n2; ++k) P.hat1[k] = 0.5 * (1.0 + m->ops.z2[k]);
    pph::CoarseTopo T;
    pph::coarse_topology(s, d->glo_num, T);
    P.nvert = T.nvert;
    pph::ProbedRows rows;
    NLG_TRY(probe_coarse_operator(m, T, rows));
    pph::CoarseCsr A;
    pph::coarse_rows(rows, A);

    // aggregates of vertices and the operator on them
    std::vector<char> viface;   // vertex on a rank boundary
    pph::boundary_vertices(s, T, multi ? m->halo.h_cidx : std::vector<int>(), viface);
    std::vector<int> agg;
    const int na = pph::aggregate(s, T, A, exact_max, multi, viface, agg);
    pph::AggLevel G;
    pph::assemble_acc(A, agg, na, !m->has_outflow && !multi, G);
    P.na = na;
    NLG_TRY(up(T.vg, &P.d_vg));
    NLG_TRY(up(T.vp, &P.d_v2e_p));
    NLG_TRY(up(T.vi, &P.d_v2e_i));
    NLG_TRY(up(A.dinv, &P.d_dinv));
    NLG_TRY(up(agg, &P.d_agg));
    NLG_TRY(up(G.ap, &P.d_ap));
    NLG_TRY(up(G.am, &P.d_am));
    NLG_HIP(hipMalloc(&P.d_tq, sizeof(double) * (size_t)m->E * NC));
    for (double **v : {&P.d_rc, &P.d_x}) NLG_HIP(hipMalloc(v, sizeof(double) * (size_t)std::max(T.nvert, 1)));
    NLG_HIP(hipMalloc(&P.d_xa, sizeof(double) * (size_t)std::max(na, 1)));

    // the dense inverse: of this rank's aggregates, or of the global aggregate level
    if (multi) {
        NLG_TRY(global_aggregate_level(m, T, agg, G, lib_min));
    } else {
        NLG_TRY(up(G.Acc, &P.d_Ainv));
        NLG_TRY(spd_inverse_dev(st, P.d_Ainv, na, lib_min));
        P.na_max = P.ncols = na;
        NLG_HIP(hipMalloc(&P.d_ra, sizeof(double) * (size_t)std::max(na, 1)));
    }
    P.ready = true;
    return 0;
}

// Scratch of the preconditioner for `nl` lanes of a block step: nl copies of the exchange array W, the element-corner
// residuals, the vertex-level and the aggregate-level vectors at constant strides (the kernels reach lane v through blockIdx.y).
// One copy exists after pprec_setup; more are made on first use.
int pprec_reserve_lanes(nlg_mesh *m, int nl) {
    nlg_pprec &P = m->pprec;
    NLG_CHECK(P.ready, "pprec: preconditioner not set up");
    NLG_CHECK(nl >= 1 && nl <= kMaxLanes, "pprec: %d lanes", nl);
    if (nl <= P.lanes_cap) return 0;
    hipStream_t st = m->ctx->stream;
    NLG_HIP(hipStreamSynchronize(st));
    const int NC = 1 << m->dim;
    auto regrow = [&](double **p, int64_t len1, int64_t *stride, bool exact = false) -> int {
        if (!*p) {
            *stride = 0;
            return 0;
        }
        const int64_t sd = exact ? std::max<int64_t>(len1, 1) : round_up(std::max<int64_t>(len1, 1), kAlign);
        double *q = nullptr;
        NLG_HIP(hipMalloc(&q, sizeof(double) * (size_t)(sd * nl)));
        NLG_HIP(hipMemsetAsync(q, 0, sizeof(double) * (size_t)(sd * nl), st));
        NLG_HIP(hipMemcpyAsync(q, *p, sizeof(double) * (size_t)len1, hipMemcpyDeviceToDevice, st));
        NLG_HIP(hipStreamSynchronize(st));
        NLG_HIP(hipFree(*p));
        *p = q;
        *stride = sd;
        return 0;
    };
    NLG_TRY(regrow(&P.d_W, m->lvs, &P.lW));
    int64_t lW2 = 0;
    NLG_TRY(regrow(&P.d_Wr, m->lvs, &lW2));   // (overlapping variant: the return array beside the extended grids)
    NLG_CHECK(!P.d_Wr || lW2 == P.lW, "pprec: inconsistent lane strides");
    NLG_TRY(regrow(&P.d_tq, m->E * NC, &P.lt));
    int64_t lv2 = 0, la2 = 0;
    NLG_TRY(regrow(&P.d_rc, P.nvert, &P.lv));
    NLG_TRY(regrow(&P.d_x, P.nvert, &lv2));
    const bool glob = P.ncols != P.na;                         // several ranks: d_ra holds na_max entries (zero-padded)
    NLG_TRY(regrow(&P.d_ra, glob ? P.na_max : P.na, &P.la, glob));   // several ranks: the lanes contiguous, [lane][na_max]
    NLG_TRY(regrow(&P.d_xa, P.na, &la2));
    if (glob) {
        // all-gathered aggregate residuals [rank][lane][na_max]: the lanes of a rank stay together in one all-gather
        NLG_HIP(hipFree(P.d_rag));
        NLG_HIP(hipMalloc(&P.d_rag, sizeof(double) * (size_t)P.ncols * nl));
    }
    NLG_CHECK(lv2 == P.lv && (la2 == P.la || glob), "pprec: inconsistent lane strides");
    P.la_x = la2;
    P.lanes_cap = nl;
    return 0;
}

// ghost layers of face neighbours on other ranks (copy mode): the element has put its own value into its own slot of a
// rank-boundary face, the exchange replaces it by the neighbour's.  Edge and corner slots are never written and travel as zeros.
static int overlap_halo(nlg_mesh *m, hipStream_t st, double *w, int layout, int nl) {
    ++g_collectives;
    if (!m->halo.active) return 0;
    NLG_CHECK(st == m->ctx->stream, "pprec: the overlap exchange across ranks runs on the context's stream");
    double *f1[1] = {w};
    return halo_exchange(m, f1, 1, layout, nl, m->pprec.lW, true);
}

// z = M^-1 r on `st`: the local solves (with or without the face overlap) plus, when with_coarse, the prolonged coarse
// correction xc[v] + xa[agg[v]] (xc = omega dinv (R_1^T r), xa = aggregate-level solve).  rz_part: r.z and z sums of the last
// kernel ((E + 3) / 4 blocks).  upd: the PCG update of r rides in the restriction.  nl > 1: the lanes of a block step in the
// same launches (flag, r, z, rz_part and the fused PCG update of lane v sit v * ld doubles behind the given pointers).
// Launches per application: restriction, coarse chain (without overlap: gather, aggregate restriction; with overlap they ride
// in the local solves), dense aggregate solve, local solves, and with overlap the finish.
int pprec_apply(nlg_mesh *m, hipStream_t st, const double *flag, const double *r, double *z, double *rz_part, bool overlap,
                bool with_coarse, const nlg_pcg_upd *upd, int nl, int64_t ld) {
    const nlg_pcg_upd uu = upd ? *upd : nlg_pcg_upd{};
    double *rw = const_cast<double *>(r);   // written only when the PCG update rides along
    nlg_pprec &P = m->pprec;
    NLG_CHECK(P.ready, "pprec: preconditioner not set up");
    NLG_CHECK(!overlap || P.overlap, "pprec: the overlapping variant is not set up for this mesh");
    NLG_TRY(pprec_reserve_lanes(m, nl));
    const int64_t E = m->E;
    const int nv = P.nvert;
    const double om = P.na == nv ? 0.0 : 0.7;   // exact coarse solve when every vertex is its own aggregate
    const bool glob = P.ncols != P.na;
    const int64_t la_x = glob ? P.la_x : P.la;
    const double *xc = with_coarse ? P.d_x : nullptr;   // the Jacobi term; the finish adds xa[agg[v]] while prolonging
    const int *vg = P.d_vg;
    Hat hat;
    for (int k = 0; k < 12; ++k) hat.h1[k] = P.hat1[k];
    const dim3 gb((unsigned)((E + 3) / 4), (unsigned)nl);

    // (1) element-local restriction t = R_1^T r per element (+ the extended grids Win of the overlapping variant)
    double *Wp = overlap ? P.d_W : (double *)nullptr;
    const int *pin = P.d_pin;
    if (m->dim == 3) {
        if (pin && m->n2 == 6)
            NLG_LAUNCH(k_q1_restrict_local3s<6>, gb, dim3(NT), 0, st, flag, E, hat, rw, P.d_tq, Wp, (const double *)P.d_wq, pin, uu, ld, P.lt, P.lW);
        else if (pin && m->n2 == 8)
            NLG_LAUNCH(k_q1_restrict_local3s<8>, gb, dim3(NT), 0, st, flag, E, hat, rw, P.d_tq, Wp, (const double *)P.d_wq, pin, uu, ld, P.lt, P.lW);
        else if (pin && m->n2 == 10)
            NLG_LAUNCH(k_q1_restrict_local3s<10>, gb, dim3(NT), 0, st, flag, E, hat, rw, P.d_tq, Wp, (const double *)P.d_wq, pin, uu, ld, P.lt, P.lW);
        else
            NLG_LAUNCH(k_q1_restrict_local<3>, gb, dim3(NT), 0, st, flag, E, m->n2, hat, rw, P.d_tq, Wp, (const double *)P.d_wq, pin, uu, ld, P.lt, P.lW);
    } else {
        NLG_LAUNCH(k_q1_restrict_local<2>, gb, dim3(NT), 0, st, flag, E, m->n2, hat, rw, P.d_tq, Wp, (const double *)P.d_wq, pin, uu, ld, P.lt, P.lW);
    }
    // dense aggregate solve xa = Ainv ra
    auto dense_solve = [&]() -> int {
        const double *ra = P.d_ra;
        int na_max = 0;
        if (glob) {   // several ranks: the aggregate level is global; ONE all-gather carries the lanes of every rank
            NLG_CHECK(st == m->ctx->stream, "pprec: the global aggregate level runs on the context's stream");
            NLG_TRY(allgather_f64(m->ctx, P.d_ra, P.d_rag, (int64_t)P.na_max * nl));
            ra = P.d_rag;
            na_max = nl > 1 ? P.na_max : 0;   // (one lane: the gathered array is the plain column vector)
        }
        const dim3 gg((unsigned)((P.na + 3) / 4), (unsigned)nl);
        if (P.d_Ainv32)
            NLG_LAUNCH(k_dense_gemv<float>, gg, dim3(NT), 0, st, flag, P.na, P.ncols, (const float *)P.d_Ainv32, ra, P.d_xa, ld, la_x, na_max, nl);
        else
            NLG_LAUNCH(k_dense_gemv<double>, gg, dim3(NT), 0, st, flag, P.na, P.ncols, (const double *)P.d_Ainv, ra, P.d_xa, ld, la_x, na_max, nl);
        return 0;
    };

    if (!overlap) {
        // (2) coarse chain: vertex gather, aggregate restriction, dense solve; (3) local solves + prolonged coarse correction
        if (with_coarse) {
            NLG_LAUNCH(k_q1_gather, dim3((nv + NT - 1) / NT, nl), dim3(NT), 0, st, flag, nv, P.d_v2e_p, P.d_v2e_i, P.d_tq, P.d_rc, P.d_dinv, om, P.d_x, ld, P.lt, P.lv);
            NLG_LAUNCH(k_agg_restrict, dim3((P.na + 3) / 4, nl), dim3(NT), 0, st, flag, P.na, P.d_ap, P.d_am, P.d_rc, P.d_ra, ld, P.lv, P.la);
            NLG_TRY(dense_solve());
        }
#define FDM_CASE(N_)                                                                                                  \
    case N_:                                                                                                          \
        if (m->dim == 3)                                                                                              \
            NLG_LAUNCH((k_fdm<N_ - 2, 3>), gb, dim3(NT), 0, st, flag, E, P.d_S, P.d_invden, r, xc, P.d_xa, P.d_agg, vg, hat, z, rz_part, ld, P.lv, la_x); \
        else                                                                                                          \
            NLG_LAUNCH((k_fdm<N_ - 2, 2>), gb, dim3(NT), 0, st, flag, E, P.d_S, P.d_invden, r, xc, P.d_xa, P.d_agg, vg, hat, z, rz_part, ld, P.lv, la_x); \
        break;
        switch (m->n) {
            FDM_CASE(4) FDM_CASE(5) FDM_CASE(6) FDM_CASE(7) FDM_CASE(8) FDM_CASE(9) FDM_CASE(10) FDM_CASE(12)
            default: set_error("pprec: unsupported lx1 = %d", m->n); return 1;
        }
#undef FDM_CASE
        NLG_HIP(hipGetLastError());
        return 0;
    }

    // (2) local solves on Win; the vertex gather and the aggregate restriction ride behind the elements
    NLG_TRY(overlap_halo(m, st, P.d_W, LAYOUT_NAT, nl));
    ChainArgs cg = {};
    auto chain_blocks = [&](int threads) -> int {
        if (!with_coarse) return 0;
        cg = ChainArgs{(nv + threads - 1) / threads, nv, P.d_v2e_p, P.d_v2e_i, P.d_tq, P.d_rc, P.d_dinv, om, P.d_x,
                       P.na, P.d_ap, P.d_am, P.d_ra, P.lt, P.lv, P.la};
        return cg.nb_gather + (P.na + threads / 64 - 1) / (threads / 64);   // one wave per aggregate
    };
    if (m->dim == 2) {
        const int nb_c = chain_blocks(NT);
#define FX2_CASE(N_)                                                                                                  \
    case N_:                                                                                                          \
        NLG_LAUNCH((k_fdm_ext2<N_>), dim3(gb.x + nb_c, (unsigned)nl), dim3(NT), 0, st, flag, E, P.d_Sx, P.d_lamx, P.thrx, \
                   (const double *)P.d_W, P.d_Wr, z, (const int *)P.d_pret, ld, P.lW, (int)gb.x, cg);               \
        break;
        switch (m->n) {
            FX2_CASE(4) FX2_CASE(5) FX2_CASE(6) FX2_CASE(7) FX2_CASE(8)
            default: set_error("pprec: overlapping variant built for lx1 = 4..8, got %d", m->n); return 1;
        }
#undef FX2_CASE
    } else {
#define FX_CASE(N_)                                                                                                   \
    case N_: {                                                                                                        \
        constexpr int WPE_ = (N_ * N_ + 63) / 64;   /* one column per lane: 1 wave up to lx1 = 8, 2 at 9 / 10, 3 at 12 */ \
        const int nb_c = chain_blocks(64 * WPE_);                                                                     \
        NLG_LAUNCH((k_fdm_ext<N_, 1, WPE_>), dim3((unsigned)(E + nb_c), (unsigned)nl), dim3(64 * WPE_), 0, st, flag, E, P.d_Sx, P.d_lamx, P.thrx, \
                   (const double *)P.d_W, P.d_Wr, z, (const int *)P.d_pret, ld, P.lW, (int)E, cg);                 \
    } break;
        switch (m->n) {
            FX_CASE(4) FX_CASE(5) FX_CASE(6) FX_CASE(7)
            case 8: {   // the six transforms on the matrix pipe
                const int nb_c = chain_blocks(64);
                NLG_LAUNCH(k_fdm_ext_mfma8, dim3((unsigned)(E + nb_c), (unsigned)nl), dim3(64), 0, st, flag, E, P.d_Sx, P.d_lamx, P.thrx,
                           (const double *)P.d_W, P.d_Wr, z, (const int *)P.d_pret, ld, P.lW, (int)E, cg);
            } break;
            FX_CASE(9) FX_CASE(10) FX_CASE(12)
            default: set_error("pprec: overlapping variant built for lx1 = 4..10 and 12, got %d", m->n); return 1;
        }
#undef FX_CASE
    }
    // (3) dense aggregate solve
    if (with_coarse) NLG_TRY(dense_solve());
    // (4) neighbours' ghost values + prolonged coarse correction, r.z sums
    NLG_TRY(overlap_halo(m, st, P.d_Wr, m->dim == 3 ? LAYOUT_FG : LAYOUT_NAT, nl));
#define FF_CASE(K_, N_)                                                                                               \
    case N_:                                                                                                          \
        NLG_LAUNCH((K_<N_>), gb, dim3(NT), 0, st, flag, E, (const double *)P.d_Wr, r, P.d_wq, xc, P.d_xa, P.d_agg, vg, hat, z, rz_part, ld, P.lW, P.lv, la_x); \
        break;
    if (m->dim == 2) {
        switch (m->n) {
            FF_CASE(k_sch_finish2, 4) FF_CASE(k_sch_finish2, 5) FF_CASE(k_sch_finish2, 6) FF_CASE(k_sch_finish2, 7) FF_CASE(k_sch_finish2, 8)
            default: break;
        }
    } else {
        switch (m->n) {
            FF_CASE(k_sch_finish, 4) FF_CASE(k_sch_finish, 5) FF_CASE(k_sch_finish, 6) FF_CASE(k_sch_finish, 7) FF_CASE(k_sch_finish, 8)
            FF_CASE(k_sch_finish, 9) FF_CASE(k_sch_finish, 10) FF_CASE(k_sch_finish, 12)
            default: break;
        }
    }
#undef FF_CASE
    NLG_HIP(hipGetLastError());
    return 0;
}

void pprec_free(nlg_mesh *m) {
    nlg_pprec &P = m->pprec;
    double *dp[] = {P.d_S, P.d_invden, P.d_dinv, P.d_Ainv, P.d_rc, P.d_x, P.d_ra, P.d_xa, P.d_rag, P.d_tq, P.d_Sx, P.d_lamx, P.d_W, P.d_Wr, P.d_wq};
    for (double *p : dp)
        if (p) hipFree(p);
    int *ip[] = {P.d_agg, P.d_ap, P.d_am, P.d_vg, P.d_v2e_p, P.d_v2e_i, P.d_pin, P.d_pret};
    for (int *p : ip)
        if (p) hipFree(p);
    if (P.d_Ainv32) hipFree(P.d_Ainv32);
    P = nlg_pprec();
}

}  // namespace nlg
