// Host arithmetic of the wall forces: see forces_host.h.  No HIP in this file.
#include "forces_host.h"

#include <cmath>

#include "neklab_gpu.h"
#include "probe_host.h"

namespace nlg {
namespace forces {

void gll_weights(int n, const double *z, double *w) {
    const int N = n - 1;
    for (int i = 0; i < n; ++i) {   // P_N(z_i) by the three-term recurrence
        double p0 = 1.0, p1 = z[i];
        for (int k = 2; k <= N; ++k) {
            const double p2 = ((2 * k - 1) * z[i] * p1 - (k - 1) * p0) / k;
            p0 = p1;
            p1 = p2;
        }
        w[i] = 2.0 / (N * (N + 1) * p1 * p1);
    }
}

void deriv_matrix(int n, const double *z, double *D) {
    double bw[kMaxN], w[kMaxN];
    probe::bary_weights(n, z, bw);
    for (int i = 0; i < n; ++i) probe::lagrange(n, z, bw, z[i], w, D + (size_t)i * n);
}

void gl_to_gll(int n, const double *z1, int n2, const double *z2, double *M) {
    double bw[kMaxN];
    probe::bary_weights(n2, z2, bw);
    for (int i = 0; i < n; ++i) probe::lagrange(n2, z2, bw, z1[i], M + (size_t)i * n2, nullptr);
}

int geometry(int dim, int n, const double *z, int64_t E, const double *const X[3], int64_t nfaces, const int64_t *elem, const int *face,
             const int *obj, int nobj, const double *centre, double *nds, double *met, double *xc, double *area) {
    if ((dim != 2 && dim != 3) || n < 2 || n > kMaxN || E < 0 || nfaces < 0 || nobj < 1 || !z || !X[0] || !X[1] || (dim == 3 && !X[2]) ||
        (nfaces > 0 && (!elem || !face)))
        return 1;
    for (int64_t f = 0; f < nfaces; ++f)
        if (elem[f] < 0 || elem[f] >= E || face[f] < 1 || face[f] > 2 * dim || (obj && (obj[f] < 0 || obj[f] >= nobj))) return 1;
    double D[kMaxN * kMaxN], w[kMaxN];
    deriv_matrix(n, z, D);
    gll_weights(n, z, w);
    const int nfp = face_points(dim, n);
    const size_t np = dim == 3 ? (size_t)n * n * n : (size_t)n * n;
    const int stride[3] = {1, n, n * n};
    if (area)
        for (int o = 0; o < nobj; ++o) area[o] = 0.0;
    for (int64_t f = 0; f < nfaces; ++f) {
        const int a = face_dir(face[f]), sg = face_side(face[f]);
        const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;   // the tangential directions, b < c
        const int o = obj ? obj[f] : 0;
        double fa = 0.0;
        for (int q = 0; q < nfp; ++q) {
            int idx[3] = {0, 0, 0};
            idx[a] = sg > 0 ? n - 1 : 0;
            idx[b] = q % n;
            if (dim == 3) idx[c] = q / n;
            const size_t p = (size_t)idx[0] + (size_t)n * idx[1] + (size_t)n * n * idx[2];
            double dx[3][3];   // dx[i][j] = d x_i / d r_j
            for (int i = 0; i < dim; ++i) {
                const double *Xe = X[i] + (size_t)elem[f] * np;
                for (int j = 0; j < dim; ++j) {
                    const double *line = Xe + p - (size_t)idx[j] * stride[j];
                    const double *Dr = D + (size_t)idx[j] * n;
                    double s = 0.0;
                    for (int m = 0; m < n; ++m) s += Dr[m] * line[(size_t)m * stride[j]];
                    dx[i][j] = s;
                }
            }
            double r[3][3], jac;   // r[j][i] = J d r_j / d x_i
            if (dim == 2) {
                r[0][0] = dx[1][1], r[0][1] = -dx[0][1];
                r[1][0] = -dx[1][0], r[1][1] = dx[0][0];
                jac = dx[0][0] * dx[1][1] - dx[0][1] * dx[1][0];
            } else {
                for (int j = 0; j < 3; ++j) {
                    const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                    for (int i = 0; i < 3; ++i) {
                        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
                        r[j][i] = dx[i1][j1] * dx[i2][j2] - dx[i1][j2] * dx[i2][j1];
                    }
                }
                jac = dx[0][0] * r[0][0] + dx[0][1] * r[1][0] + dx[0][2] * r[2][0];
            }
            const double wq = dim == 3 ? w[idx[b]] * w[idx[c]] : w[idx[b]];
            const size_t fq = (size_t)f * nfp + q;
            double nn = 0.0;
            for (int i = 0; i < dim; ++i) {
                const double Ni = sg * r[a][i] * wq;
                if (nds) nds[fq * dim + i] = Ni;
                nn += Ni * Ni;
                if (xc) xc[fq * dim + i] = X[i][(size_t)elem[f] * np + p] - (centre ? centre[(size_t)o * dim + i] : 0.0);
                if (met)
                    for (int j = 0; j < dim; ++j) met[fq * dim * dim + j * dim + i] = r[j][i] / jac;
            }
            fa += std::sqrt(nn);
        }
        if (area) area[o] += fa;
    }
    return 0;
}

}  // namespace forces
}  // namespace nlg

extern "C" int nlg_forces_geometry(int dim, int n, int64_t nel, const double *x, const double *y, const double *z, int64_t nfaces,
                                   const int64_t *elem_local, const int *face, const int *obj, int nobj, const double *centre, double *nds,
                                   double *met, double *xc, double *area) {
    if (n < 2 || n > nlg::forces::kMaxN) return 1;
    double zn[nlg::forces::kMaxN];
    nlg::probe::gll_nodes(n, zn);
    const double *X[3] = {x, y, z};
    return nlg::forces::geometry(dim, n, zn, nel, X, nfaces, elem_local, face, obj, nobj, centre, nds, met, xc, area);
}
