// Element-local pieces shared by the strong-form kernels (lns_strong.hip: k_lns_strong, lns_sens.hip: k_lns_sens): the geometry one
// block needs, the block shape of an element, and the pointwise physical gradient from a field in LDS.  Not part of the C ABI.
#pragma once
#include "internal.h"

namespace nlg {

struct LnsGeom {
    const double *rst[9];
    const double *jac, *bm1;
    const double *mask[3];
};

template <int N, int DIM>
struct LnsShape {
    static constexpr int NP = DIM == 3 ? N * N * N : N * N;
    static constexpr int PPT = NP > 1024 ? 4 : 1;                         // points per thread (lx1 = 12 in 3-D: 448 threads, 36 bytes of scratch; 2 points on 896 threads: 160, 3 on 576: 244)
    static constexpr int NT = (((NP + PPT - 1) / PPT + 63) / 64) * 64;    // threads per block
    // waves per SIMD asked of the compiler.  lx1 = 8 in 3-D (512 threads, 8 waves): 4, i.e. at most 128 VGPRs, so that TWO blocks share
    // a CU and one computes while the other waits at a barrier (122 VGPRs, no scratch; uncapped: 136, one block per CU)
    static constexpr int MINW = NT == 512 ? 4 : 1;
};

// physical gradient at point (i, j, k) of the field in sF: g_c = (1 / jac) sum_a rst[a][c] D_a f
template <int N, int DIM>
__device__ __forceinline__ void lns_grad(const double *sF, const double *sDt, int i, int j, int k, const double *rs, double jinv, double *g) {
    constexpr int NQ = N + 1;
    double d[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) d[a] = 0.0;
#pragma unroll
    for (int l = 0; l < N; ++l) {
        d[0] += sDt[l * N + i] * sF[l + NQ * (j + N * k)];
        d[1] += sDt[l * N + j] * sF[i + NQ * (l + N * k)];
        if (DIM == 3) d[DIM - 1] += sDt[l * N + k] * sF[i + NQ * (j + N * l)];
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) s += rs[a * DIM + c] * d[a];
        g[c] = s * jinv;
    }
}

inline LnsGeom lns_geom(const nlg_mesh *m) {
    LnsGeom G = {};
    for (int q = 0; q < m->dim * m->dim; ++q) G.rst[q] = m->d_rst[q];
    G.jac = m->d_jac, G.bm1 = m->d_bm1;
    for (int c = 0; c < m->dim; ++c) G.mask[c] = m->d_mask[c];
    return G;
}

}  // namespace nlg
