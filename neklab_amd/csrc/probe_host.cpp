// Host arithmetic of the history points: see probe_host.h.  No HIP in this file.
#include "probe_host.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "neklab_gpu.h"

namespace nlg {
namespace probe {

namespace {

// P_N(x) and P_{N-1}(x) by the three-term recurrence
void legendre(int N, double x, double &pN, double &pNm1) {
    double p0 = 1.0, p1 = x;
    if (N == 0) {
        pN = 1.0, pNm1 = 0.0;
        return;
    }
    for (int k = 2; k <= N; ++k) {
        const double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
        p0 = p1;
        p1 = p2;
    }
    pN = p1, pNm1 = p0;
}

void antisymmetrise(int n, double *z) {
    std::vector<double> s(z, z + n);
    for (int i = 0; i < n; ++i) z[i] = 0.5 * (s[i] - s[n - 1 - i]);
}

struct Elem {   // one element's coordinate fields and the 1-D basis
    int dim, n;
    const double *z, *bw;
    const double *X[3];
};

// x = x_e(r); J[c][d] = d x_c / d r_d (J may be null)
void map_point(const Elem &el, const double *r, double *x, double (*J)[3]) {
    const int dim = el.dim, n = el.n;
    double w[3][kMaxN], dw[3][kMaxN];
    for (int d = 0; d < dim; ++d) lagrange(n, el.z, el.bw, r[d], w[d], J ? dw[d] : nullptr);
    const int nk = dim == 3 ? n : 1;
    for (int c = 0; c < dim; ++c) {
        double s = 0.0, g[3] = {0.0, 0.0, 0.0};
        const double *Xc = el.X[c];
        for (int k = 0; k < nk; ++k) {
            const double wk = dim == 3 ? w[2][k] : 1.0, dk = dim == 3 && J ? dw[2][k] : 0.0;
            for (int j = 0; j < n; ++j) {
                double a = 0.0, b = 0.0;   // sum over i of X w_i and X w_i'
                const double *row = Xc + (size_t)n * (j + (size_t)n * k);
                for (int i = 0; i < n; ++i) a += row[i] * w[0][i];
                if (J)
                    for (int i = 0; i < n; ++i) b += row[i] * dw[0][i];
                s += a * w[1][j] * wk;
                if (J) {
                    g[0] += b * w[1][j] * wk;
                    g[1] += a * dw[1][j] * wk;
                    g[2] += a * w[1][j] * dk;
                }
            }
        }
        x[c] = s;
        if (J)
            for (int d = 0; d < dim; ++d) J[c][d] = g[d];
    }
}

// J dr = f by Gaussian elimination with partial pivoting; false: singular
bool solve_small(int dim, double (*J)[3], const double *f, double *dr) {
    double A[3][4];
    for (int c = 0; c < dim; ++c) {
        for (int d = 0; d < dim; ++d) A[c][d] = J[c][d];
        A[c][dim] = f[c];
    }
    for (int p = 0; p < dim; ++p) {
        int q = p;
        for (int c = p + 1; c < dim; ++c)
            if (std::fabs(A[c][p]) > std::fabs(A[q][p])) q = c;
        if (A[q][p] == 0.0 || !std::isfinite(A[q][p])) return false;
        if (q != p)
            for (int d = 0; d <= dim; ++d) std::swap(A[p][d], A[q][d]);
        for (int c = p + 1; c < dim; ++c) {
            const double m = A[c][p] / A[p][p];
            for (int d = p; d <= dim; ++d) A[c][d] -= m * A[p][d];
        }
    }
    for (int p = dim - 1; p >= 0; --p) {
        double s = A[p][dim];
        for (int d = p + 1; d < dim; ++d) s -= A[p][d] * dr[d];
        dr[p] = s / A[p][p];
    }
    return true;
}

double distance(int dim, const double *a, const double *b) {
    double s = 0.0;
    for (int c = 0; c < dim; ++c) s += (a[c] - b[c]) * (a[c] - b[c]);
    return std::sqrt(s);
}

// Newton for x_e(r) = xs from the nearest GLL node.  -1: the element does not hold the point; else the status (0, 1), r and dist
int locate_in(const Elem &el, const double *xs, double tol_r, double *r, double *dist) {
    const int dim = el.dim, n = el.n;
    const int np = dim == 3 ? n * n * n : n * n;
    int best = 0;
    double bd = INFINITY;
    for (int q = 0; q < np; ++q) {
        double s = 0.0;
        for (int c = 0; c < dim; ++c) s += (el.X[c][q] - xs[c]) * (el.X[c][q] - xs[c]);
        if (s < bd) bd = s, best = q;
    }
    r[0] = el.z[best % n], r[1] = el.z[(best / n) % n];
    if (dim == 3) r[2] = el.z[best / (n * n)];
    bool converged = false;
    for (int it = 0; it < kNewtonMax && !converged; ++it) {
        double x[3], J[3][3], f[3], dr[3];
        map_point(el, r, x, J);
        for (int c = 0; c < dim; ++c) f[c] = xs[c] - x[c];
        if (!solve_small(dim, J, f, dr)) return -1;
        double step = 0.0;
        for (int d = 0; d < dim; ++d) {
            const double rn = std::min(kClamp, std::max(-kClamp, r[d] + dr[d]));
            if (!std::isfinite(rn)) return -1;
            step = std::max(step, std::fabs(rn - r[d]));
            r[d] = rn;
        }
        converged = step <= kNewtonStop;
    }
    if (!converged) return -1;
    // r is known to the Newton stop: a component that close to a face lies on it
    double rmax = 0.0;
    for (int d = 0; d < dim; ++d) {
        if (std::fabs(std::fabs(r[d]) - 1.0) <= kNewtonStop) r[d] = r[d] > 0.0 ? 1.0 : -1.0;
        rmax = std::max(rmax, std::fabs(r[d]));
    }
    if (rmax > 1.0 + tol_r) return -1;
    const int status = rmax > 1.0 ? 1 : 0;
    for (int d = 0; d < dim; ++d) r[d] = std::min(1.0, std::max(-1.0, r[d]));
    double x[3];
    map_point(el, r, x, nullptr);
    *dist = distance(dim, x, xs);
    return status;
}

}  // namespace

void gll_nodes(int n, double *z) {
    const int N = n - 1;
    for (int i = 0; i < n; ++i) z[i] = -std::cos(M_PI * i / N);
    for (int it = 0; it < 100; ++it) {
        double mx = 0.0;
        for (int i = 1; i < n - 1; ++i) {
            double pN, pNm1;
            legendre(N, z[i], pN, pNm1);
            const double dx = N * (pNm1 - z[i] * pN) / (-(double)N * (N + 1) * pN);
            z[i] -= dx;
            mx = std::max(mx, std::fabs(dx));
        }
        if (mx < 1e-16) break;
    }
    z[0] = -1.0, z[n - 1] = 1.0;
    antisymmetrise(n, z);
}

void gl_nodes(int n, double *z) {
    for (int k = 1; k <= n; ++k) z[k - 1] = -std::cos(M_PI * (k - 0.25) / (n + 0.5));
    for (int it = 0; it < 100; ++it) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i) {
            double pn, pnm1;
            legendre(n, z[i], pn, pnm1);
            const double dx = pn / (n * (z[i] * pn - pnm1) / (z[i] * z[i] - 1.0));
            z[i] -= dx;
            mx = std::max(mx, std::fabs(dx));
        }
        if (mx < 1e-16) break;
    }
    antisymmetrise(n, z);
}

void bary_weights(int n, const double *z, double *bw) {
    for (int j = 0; j < n; ++j) {
        double w = 1.0;
        for (int k = 0; k < n; ++k)
            if (k != j) w /= (z[j] - z[k]);
        bw[j] = w;
    }
}

void lagrange(int n, const double *z, const double *bw, double r, double *w, double *dw) {
    int hit = -1;
    for (int j = 0; j < n; ++j)
        if (r == z[j]) hit = j;
    if (hit >= 0) {
        for (int j = 0; j < n; ++j) w[j] = j == hit ? 1.0 : 0.0;
        if (dw) {   // the row of the differentiation matrix
            double s = 0.0;
            for (int j = 0; j < n; ++j)
                if (j != hit) {
                    dw[j] = (bw[j] / bw[hit]) / (z[hit] - z[j]);
                    s += dw[j];
                }
            dw[hit] = -s;
        }
        return;
    }
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
        w[j] = bw[j] / (r - z[j]);
        s += w[j];
    }
    for (int j = 0; j < n; ++j) w[j] /= s;
    if (dw) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += w[j] / (r - z[j]);
        for (int j = 0; j < n; ++j) dw[j] = w[j] * (t - 1.0 / (r - z[j]));
    }
}

int locate(int dim, int n, const double *z, int64_t E, const double *const X[3], const int64_t *lglel, int64_t npts, const double *xyz,
           double tol_r, int64_t *elem, double *rst, int *status, double *dist, double *key) {
    const int np = dim == 3 ? n * n * n : n * n;
    double bw[kMaxN];
    bary_weights(n, z, bw);
    std::vector<double> box((size_t)E * 2 * dim);   // [E][dim][lo, hi], grown
    for (int64_t e = 0; e < E; ++e)
        for (int c = 0; c < dim; ++c) {
            const double *Xc = X[c] + (size_t)e * np;
            const auto mm = std::minmax_element(Xc, Xc + np);
            const double grow = kBoxGrow * (*mm.second - *mm.first);
            box[((size_t)e * dim + c) * 2] = *mm.first - grow;
            box[((size_t)e * dim + c) * 2 + 1] = *mm.second + grow;
        }
    const double kStatus1 = 1099511627776.0;   // 2^40: a status-1 holder ranks behind every status-0 holder
    for (int64_t p = 0; p < npts; ++p) {
        const double *xs = xyz + (size_t)p * dim;
        double bestkey = -1.0;
        elem[p] = -1;
        status[p] = 2;
        if (dist) dist[p] = 0.0;
        for (int d = 0; d < dim; ++d) rst[(size_t)p * dim + d] = 0.0;
        for (int64_t e = 0; e < E; ++e) {
            bool in = true;
            for (int c = 0; c < dim && in; ++c)
                in = xs[c] >= box[((size_t)e * dim + c) * 2] && xs[c] <= box[((size_t)e * dim + c) * 2 + 1];
            if (!in) continue;
            Elem el{dim, n, z, bw, {X[0] + (size_t)e * np, X[1] + (size_t)e * np, dim == 3 ? X[2] + (size_t)e * np : nullptr}};
            double r[3] = {0.0, 0.0, 0.0}, ds = 0.0;
            const int st = locate_in(el, xs, tol_r, r, &ds);
            if (st < 0) continue;
            const double k = (double)(lglel ? lglel[e] : e) + (st == 1 ? kStatus1 : 0.0);
            if (bestkey < 0.0 || k < bestkey) {
                bestkey = k;
                elem[p] = e;
                status[p] = st;
                if (dist) dist[p] = ds;
                for (int d = 0; d < dim; ++d) rst[(size_t)p * dim + d] = r[d];
            }
        }
        if (key) key[p] = bestkey;
    }
    return 0;
}

}  // namespace probe
}  // namespace nlg

extern "C" int nlg_probe_locate(int dim, int n, int64_t E, const double *x, const double *y, const double *z, const int64_t *lglel,
                                int64_t npts, const double *xyz, double tol_r, int64_t *elem, double *rst, int *status, double *dist) {
    using namespace nlg::probe;
    if ((dim != 2 && dim != 3) || n < 2 || n > kMaxN || E < 0 || npts < 0 || !x || !y || (dim == 3 && !z) || (npts > 0 && !xyz) || !elem ||
        !rst || !status || !(tol_r >= 0.0))
        return 1;
    double zn[kMaxN];
    gll_nodes(n, zn);
    const double *X[3] = {x, y, z};
    return locate(dim, n, zn, E, X, lglel, npts, xyz, tol_r, elem, rst, status, dist, nullptr);
}
