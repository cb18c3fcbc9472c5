// Host arithmetic of the pressure preconditioner's set-up: see pprec_host.h.  No HIP here.
#include "pprec_host.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "fg_slot.h"

namespace nlg {
namespace pph {

namespace {

int fail(std::string &err, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return 1;
}
#define PPH_CHECK(cond, ...)                         \
    do {                                             \
        if (!(cond)) return fail(err, __VA_ARGS__);  \
    } while (0)

// symmetric eigen-decomposition by cyclic Jacobi rotations (n <= 16): A = V diag(w) V^T
void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &V, std::vector<double> &w) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - s * akq;
                    A[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - s * aqk;
                    A[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = c * vkp - s * vkq;
                    V[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    w.resize(n);
    for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}

// generalised symmetric problem A s = lam B s, B SPD: S^T B S = I, S^T A S = diag(lam). S row-major [point][mode].
int gen_eig(int n, const std::vector<double> &A, const std::vector<double> &B, std::vector<double> &S,
            std::vector<double> &lam) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double d = B[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) return 1;
        L[(size_t)j * n + j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double s = B[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
        }
    }
    // Linv (lower)
    std::vector<double> Li((size_t)n * n, 0.0);
    for (int c = 0; c < n; ++c) {
        Li[(size_t)c * n + c] = 1.0 / L[(size_t)c * n + c];
        for (int i = c + 1; i < n; ++i) {
            double s = 0.0;
            for (int k = c; k < i; ++k) s += L[(size_t)i * n + k] * Li[(size_t)k * n + c];
            Li[(size_t)i * n + c] = -s / L[(size_t)i * n + i];
        }
    }
    std::vector<double> T((size_t)n * n, 0.0), Cm((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += Li[(size_t)i * n + k] * A[(size_t)k * n + j];
            T[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += T[(size_t)i * n + k] * Li[(size_t)j * n + k];
            Cm[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) Cm[(size_t)i * n + j] = Cm[(size_t)j * n + i] = 0.5 * (Cm[(size_t)i * n + j] + Cm[(size_t)j * n + i]);
    std::vector<double> V;
    jacobi_eig(n, Cm, V, lam);
    S.assign((size_t)n * n, 0.0);   // S = Li^T V
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += Li[(size_t)k * n + i] * V[(size_t)k * n + j];
            S[(size_t)i * n + j] = s;
        }
    return 0;
}

// Dh = diag(w2) D12, Ih = diag(w2) I12 (n2 x n)
void weighted_ops(const Shape &s, const Ops &o, std::vector<double> &Dh, std::vector<double> &Ih) {
    const int n = s.n, n2 = s.n2;
    Dh.resize((size_t)n2 * n);
    Ih.resize((size_t)n2 * n);
    for (int k = 0; k < n2; ++k)
        for (int j = 0; j < n; ++j) {
            Dh[(size_t)k * n + j] = o.w2[k] * o.D12[(size_t)k * n + j];
            Ih[(size_t)k * n + j] = o.w2[k] * o.I12[(size_t)k * n + j];
        }
}

// natural index of point (u, v) of face (dd, side)
int face_node(const Shape &s, int dd, int side, int u, int v) {
    const int n = s.n, dim = s.dim;
    int ijk[3] = {0, 0, 0};
    ijk[dd] = side == 0 ? 0 : n - 1;
    ijk[(dd + 1) % dim] = u;
    if (dim == 3) ijk[(dd + 2) % 3] = v;
    return ijk[0] + n * (ijk[1] + n * ijk[2]);
}

}  // namespace

void edge_lengths(const Shape &s, const double *const X[3], const double *const msk[3], const double *vmult, Lengths &L) {
    const int dim = s.dim, n = s.n, np1 = s.np1(), mid = n / 2;
    const int64_t E = s.E;
    L.Lall.assign((size_t)E * 3, 0.0);
    L.endfac.assign((size_t)E * 6, 0.0);
    for (int64_t e = 0; e < E; ++e)
        for (int dd = 0; dd < dim; ++dd) {
            // face centres in direction dd
            double c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
            int cnt = 0;
            for (int p = 0; p < np1; ++p) {
                const int ijk[3] = {p % n, (p / n) % n, p / (n * n)};
                if (ijk[dd] == 0) {
                    for (int c = 0; c < dim; ++c) c0[c] += X[c][e * np1 + p];
                    ++cnt;
                } else if (ijk[dd] == n - 1) {
                    for (int c = 0; c < dim; ++c) c1[c] += X[c][e * np1 + p];
                }
            }
            double l = 0.0;
            for (int c = 0; c < dim; ++c) l += (c1[c] - c0[c]) * (c1[c] - c0[c]) / ((double)cnt * cnt);
            L.Lall[(size_t)e * 3 + dd] = std::sqrt(l);
            for (int side = 0; side < 2; ++side) {
                int ijk[3] = {mid, mid, dim == 3 ? mid : 0};
                ijk[dd] = side == 0 ? 0 : n - 1;
                const int64_t q = e * np1 + ijk[0] + n * (ijk[1] + n * ijk[2]);
                L.endfac[(size_t)e * 6 + dd * 2 + side] = (msk[dd][q] == 0.0) ? 0.0 : vmult[q];
            }
        }
}

int local_fdm(const Shape &s, const Ops &o, const Lengths &L, LocalFdm &F, std::string &err) {
    const int dim = s.dim, n = s.n, n2 = s.n2, np2 = s.np2();
    const int64_t E = s.E;
    std::vector<double> Dh, Ih;
    weighted_ops(s, o, Dh, Ih);
    F.S.assign((size_t)E * 3 * n2 * n2, 0.0);
    F.invden.assign((size_t)E * np2, 0.0);
    std::vector<double> lam3((size_t)3 * n2);
    double denmax = 0.0;
    for (int64_t e = 0; e < E; ++e) {
        for (int dd = 0; dd < dim; ++dd) {
            const double l = L.Lall[(size_t)e * 3 + dd];
            std::vector<double> bi(n);
            for (int i = 0; i < n; ++i) bi[i] = 1.0 / (0.5 * l * o.w1[i]);
            for (int side = 0; side < 2; ++side) {
                const int k = side == 0 ? 0 : n - 1;
                const double ef = L.endfac[(size_t)e * 6 + dd * 2 + side];
                bi[k] = ef == 0.0 ? 0.0 : bi[k] * ef;
            }
            std::vector<double> A((size_t)n2 * n2), B((size_t)n2 * n2), S, lam;
            for (int a = 0; a < n2; ++a)
                for (int b = 0; b < n2; ++b) {
                    double sa = 0.0, sb = 0.0;
                    for (int j = 0; j < n; ++j) {
                        sa += Dh[(size_t)a * n + j] * bi[j] * Dh[(size_t)b * n + j];
                        sb += Ih[(size_t)a * n + j] * bi[j] * Ih[(size_t)b * n + j];
                    }
                    A[(size_t)a * n2 + b] = sa;
                    B[(size_t)a * n2 + b] = 0.25 * l * l * sb;
                }
            PPH_CHECK(gen_eig(n2, A, B, S, lam) == 0, "pprec_setup: 1-D mass matrix not positive definite (element %lld)", (long long)e);
            for (int q = 0; q < n2 * n2; ++q) F.S[((size_t)e * 3 + dd) * n2 * n2 + q] = S[q];
            for (int a = 0; a < n2; ++a) lam3[(size_t)dd * n2 + a] = std::max(lam[a], 0.0);
        }
        for (int q = 0; q < np2; ++q) {
            const int a = q % n2, b = (q / n2) % n2, c = q / (n2 * n2);
            double den = lam3[a] + lam3[n2 + b] + (dim == 3 ? lam3[2 * n2 + c] : 0.0);
            F.invden[(size_t)e * np2 + q] = den;
            denmax = std::max(denmax, den);
        }
    }
    for (auto &v : F.invden) v = (v > 1e-12 * denmax) ? 1.0 / v : 0.0;
    return 0;
}

void face_lengths(const Shape &s, const Lengths &L, std::vector<double> &hw) {
    const int dim = s.dim, n = s.n, np1 = s.np1();
    hw.assign((size_t)s.E * np1, 0.0);
    for (int64_t e = 0; e < s.E; ++e)
        for (int dd = 0; dd < dim; ++dd)
            for (int side = 0; side < 2; ++side)
                for (int v = 1; v < (dim == 3 ? n - 1 : 2); ++v)
                    for (int u = 1; u < n - 1; ++u) hw[(size_t)e * np1 + face_node(s, dd, side, u, v)] = L.Lall[(size_t)e * 3 + dd];
}

// The extended 1-D operators of the overlapping variant.
// Symmetric weighting D M D, D = diag(count^-1/2), count = number of extended subdomains that contain the point
// (1 + one per face neighbour whose ghost layer it is).  Prototype (docs/prototypes/precond_proto5.py, 6^3 elements,
// lx1 = 6): unweighted 21 / 29 iterations with the exact / approximate coarse solve, weighted 14 / 18;
// without overlap 29.
int extended_lines(const Shape &s, const Ops &o, const Lengths &L, const std::vector<double> &hw, ExtLines &X, std::string &err) {
    const int dim = s.dim, n = s.n, n2 = s.n2, np1 = s.np1(), np2 = s.np2(), mid = n / 2;
    const int64_t E = s.E;
    std::vector<double> Dh, Ih;
    weighted_ops(s, o, Dh, Ih);
    const int mx = n;   // extended 1-D size
    X.Sx.assign((size_t)E * 3 * mx * mx, 0.0);
    X.lamx.assign((size_t)E * 3 * mx, 0.0);
    X.wq.assign((size_t)E * np2, 1.0);
    X.hasnb.assign((size_t)E * 6, 0);
    std::vector<double> &hSx = X.Sx, &hlx = X.lamx, &hwq = X.wq;
    std::vector<double> Bl((size_t)3 * n), bq((size_t)3 * n), Ae((size_t)mx * mx), Be((size_t)mx * mx), Sx, lx;
    std::vector<double> Dl((size_t)mx * 3 * n), Il((size_t)mx * 3 * n);   // rows: the mx extended pressure points
    double dmax = 0.0;
    for (int64_t e = 0; e < E; ++e) {
        for (int dd = 0; dd < dim; ++dd) {
            const double lm = L.Lall[(size_t)e * 3 + dd];
            double ln[2];
            for (int side = 0; side < 2; ++side) {
                const double sum = hw[(size_t)e * np1 + face_node(s, dd, side, mid, dim == 3 ? mid : 0)];
                ln[side] = sum - lm > 1e-10 * lm ? sum - lm : 0.0;
                X.hasnb[(size_t)e * 6 + dd * 2 + side] = ln[side] > 0.0;
            }
            const double len[3] = {ln[0], lm, ln[1]};
            for (int side = 0; side < 2; ++side)
                if (ln[side] > 0.0)
                    for (int q = 0; q < np2; ++q) {
                        const int idx3[3] = {q % n2, (q / n2) % n2, q / (n2 * n2)};
                        if (idx3[dd] == (side == 0 ? 0 : n2 - 1)) hwq[(size_t)e * np2 + q] += 1.0;
                    }
            const int nvl = 3 * n - 2;
            std::fill(Bl.begin(), Bl.end(), 0.0);
            std::fill(Dl.begin(), Dl.end(), 0.0);
            std::fill(Il.begin(), Il.end(), 0.0);
            for (int q = 0; q < 3; ++q) {
                if (len[q] == 0.0) continue;
                const int ov = q * (n - 1);
                for (int i = 0; i < n; ++i) Bl[ov + i] += 0.5 * len[q] * o.w1[i];
                // extended rows owned by element q of the line: left -> row 0 (its last pressure point),
                // middle -> rows 1..n2, right -> row mx-1 (its first pressure point)
                const int r0 = q == 0 ? 0 : (q == 1 ? 1 : mx - 1);
                const int k0 = q == 0 ? n2 - 1 : 0, nk = q == 1 ? n2 : 1;
                for (int k = 0; k < nk; ++k)
                    for (int i = 0; i < n; ++i) {
                        Dl[(size_t)(r0 + k) * 3 * n + ov + i] = Dh[(size_t)(k0 + k) * n + i];
                        Il[(size_t)(r0 + k) * 3 * n + ov + i] = 0.5 * len[q] * Ih[(size_t)(k0 + k) * n + i];
                    }
            }
            for (int i = 0; i < nvl; ++i) bq[i] = Bl[i] > 0.0 ? 1.0 / Bl[i] : 0.0;
            // end points: with a neighbour, the far end of the neighbour is lumped as an interior interface (1/2);
            // without one, the own end point follows the rule of the non-overlapping operator (wall -> 0)
            if (len[0] > 0.0) bq[0] *= 0.5; else bq[n - 1] *= L.endfac[(size_t)e * 6 + dd * 2 + 0];
            if (len[2] > 0.0) bq[nvl - 1] *= 0.5; else bq[2 * (n - 1)] *= L.endfac[(size_t)e * 6 + dd * 2 + 1];
            for (int a = 0; a < mx; ++a)
                for (int b = 0; b < mx; ++b) {
                    double sa = 0.0, sb = 0.0;
                    for (int i = 0; i < nvl; ++i) {
                        sa += Dl[(size_t)a * 3 * n + i] * bq[i] * Dl[(size_t)b * 3 * n + i];
                        sb += Il[(size_t)a * 3 * n + i] * bq[i] * Il[(size_t)b * 3 * n + i];
                    }
                    Ae[(size_t)a * mx + b] = sa;
                    Be[(size_t)a * mx + b] = sb;
                }
            for (int side = 0; side < 2; ++side)
                if (ln[side] == 0.0) {   // no neighbour: the ghost point is decoupled (its right-hand side is zero)
                    const int g = side == 0 ? 0 : mx - 1;
                    for (int b = 0; b < mx; ++b) Ae[(size_t)g * mx + b] = Ae[(size_t)b * mx + g] = Be[(size_t)g * mx + b] = Be[(size_t)b * mx + g] = 0.0;
                    Ae[(size_t)g * mx + g] = 1.0;
                    Be[(size_t)g * mx + g] = 1.0;
                }
            PPH_CHECK(gen_eig(mx, Ae, Be, Sx, lx) == 0, "pprec_setup: extended 1-D mass matrix not positive definite (element %lld)", (long long)e);
            for (int q = 0; q < mx * mx; ++q) hSx[((size_t)e * 3 + dd) * mx * mx + q] = Sx[q];
            for (int a = 0; a < mx; ++a) hlx[((size_t)e * 3 + dd) * mx + a] = std::max(lx[a], 0.0);
        }
        double mxl = 0.0;
        for (int dd = 0; dd < dim; ++dd) {
            double mm = 0.0;
            for (int a = 0; a < mx; ++a) mm = std::max(mm, hlx[((size_t)e * 3 + dd) * mx + a]);
            mxl += mm;
        }
        dmax = std::max(dmax, mxl);
    }
    for (auto &v : hwq) v = 1.0 / std::sqrt(v);
    X.thrx = 1e-12 * dmax;
    return 0;
}

// destinations of the overlap values per element face point k (compact, the order of face_pt / fg_slot's face blocks):
//   pin[e][k]  = index in Win (natural layout) of the ghost point that the pressure layer of e next to k is for;
//   pret[e][k] = index in Wret of the face slot that the solve of e at ghost point k is for (3-D: face-grouped
//                layout, 2-D: natural layout, so pret = pin);
// the neighbour's face point for a face inside this rank, the own one for a face on a rank boundary (copy-mode halo
// exchange), -1 without a neighbour.  The local partners are the two-copy groups of the gather-scatter in the
// layout of Wret.
int overlap_destinations(const Shape &s, const std::vector<int> &pidx, const std::vector<char> &hasnb, bool halo_active, OverlapDest &D,
                         std::string &err) {
    const int dim = s.dim, n = s.n, n2 = s.n2;
    const int64_t E = s.E, npairs = (int64_t)(pidx.size() / 2);
    const int M = n2, F = dim == 3 ? n2 * n2 : n2, NF = 2 * dim * F, NP = dim == 3 ? n * n * n : n * n, FB = 8 + 12 * M;
    std::vector<int> fnat(NF), fret(NF), kof(NP, -1);   // face point -> slot in Win, in Wret; slot in Wret -> face point
    for (int f = 0; f < 2 * dim; ++f)
        for (int v = 0; v < (dim == 3 ? M : 1); ++v)
            for (int u = 0; u < M; ++u) {
                const int dd = f >> 1, x = (f & 1) ? n - 1 : 0;
                const int a = dd == 0 ? x : u + 1, b = dd == 0 ? u + 1 : (dd == 1 ? x : v + 1);
                const int c = dim == 3 ? (dd == 2 ? x : v + 1) : 0;
                const int k = f * F + u + M * v;
                fnat[k] = a + n * (b + n * c);
                PPH_CHECK(dim == 2 || fg_slot(n, a, b, c) == FB + k, "pprec_setup: internal (face point order)");
                fret[k] = dim == 3 ? FB + k : fnat[k];
                kof[fret[k]] = k;
            }
    PPH_CHECK((int64_t)E * NP < INT32_MAX, "pprec_setup: %lld elements are too many for 32-bit overlap indices", (long long)E);
    std::vector<int> mate((size_t)E * NP, -1);
    for (int64_t g = 0; g < npairs; ++g) {
        const int i0 = pidx[2 * g], i1 = pidx[2 * g + 1];
        PPH_CHECK(i0 >= 0 && i1 >= 0 && i0 < E * NP && i1 < E * NP, "pprec_setup: pair index out of range");
        if (kof[i0 % NP] >= 0 && kof[i1 % NP] >= 0) mate[i0] = i1, mate[i1] = i0;
    }
    std::vector<int> &pin = D.pin, &pret = D.pret;
    pin.assign((size_t)E * NF, -1);
    pret.assign((size_t)E * NF, -1);
    for (int64_t e = 0; e < E; ++e)
        for (int k = 0; k < NF; ++k) {
            const int own = (int)(e * NP + fret[k]), mt = mate[own];
            const bool nb = hasnb[(size_t)e * 6 + k / F];
            int di = -1, dr = -1;
            if (mt >= 0) {
                PPH_CHECK(nb, "pprec_setup: element %lld face %d has a partner but no neighbour length", (long long)e, k / F);
                di = (mt / NP) * NP + fnat[kof[mt % NP]];
                dr = mt;
            } else if (nb) {
                PPH_CHECK(halo_active, "pprec_setup: element %lld face %d: neighbour without a partner point", (long long)e, k / F);
                di = (int)(e * NP + fnat[k]);
                dr = own;
            }
            pin[(size_t)e * NF + k] = di;
            pret[(size_t)e * NF + k] = dr;
        }
    // every ghost slot of a face with a neighbour has exactly one producer, every other slot none (a wrong index in the
    // scatter stores of the kernels would be a fault on the device, not a wrong number)
    std::vector<unsigned char> cin((size_t)E * NP, 0), cret((size_t)E * NP, 0);
    int64_t nw = 0;
    for (size_t i = 0; i < pin.size(); ++i) {
        if (pin[i] < 0) continue;
        PPH_CHECK(pin[i] < E * NP && pret[i] >= 0 && pret[i] < E * NP, "pprec_setup: overlap destination out of range");
        PPH_CHECK(++cin[pin[i]] == 1 && ++cret[pret[i]] == 1, "pprec_setup: overlap slot with two producers");
        ++nw;
    }
    int64_t nexp = 0;
    for (int64_t e = 0; e < E; ++e)
        for (int k = 0; k < NF; ++k) {
            const int want = pin[(size_t)e * NF + k] >= 0;
            PPH_CHECK(cin[(size_t)e * NP + fnat[k]] == want && cret[(size_t)e * NP + fret[k]] == want,
                      "pprec_setup: ghost slot of element %lld face %d without its producer", (long long)e, k / F);
            nexp += want;
        }
    PPH_CHECK(nexp == nw, "pprec_setup: overlap values written outside the ghost slots");
    return 0;
}

void coarse_topology(const Shape &s, const int64_t *glo, CoarseTopo &T) {
    const int n = s.n, np1 = s.np1(), NC = s.ncorner();
    const int64_t E = s.E;
    std::vector<int> &vg = T.vg, &vp = T.vp, &vi = T.vi;
    vg.assign((size_t)E * NC, 0);
    int nvert = 0;
    {
        std::vector<int64_t> lab((size_t)E * NC);
        for (int64_t e = 0; e < E; ++e)
            for (int c = 0; c < NC; ++c) {
                const int i = (c & 1) ? n - 1 : 0, j = (c & 2) ? n - 1 : 0, k = (c & 4) ? n - 1 : 0;
                lab[(size_t)e * NC + c] = glo[e * np1 + i + n * (j + n * k)];
            }
        std::vector<int64_t> u(lab);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        nvert = (int)u.size();
        for (size_t q = 0; q < lab.size(); ++q) vg[q] = (int)(std::lower_bound(u.begin(), u.end(), lab[q]) - u.begin());
    }
    T.nvert = nvert;
    // vertex -> incident (element, corner) entries
    vp.assign((size_t)nvert + 1, 0);
    vi.assign((size_t)E * NC, 0);
    for (size_t q = 0; q < vg.size(); ++q) vp[vg[q] + 1]++;
    for (int v = 0; v < nvert; ++v) vp[v + 1] += vp[v];
    {
        std::vector<int> pos(vp.begin(), vp.end() - 1);
        for (size_t q = 0; q < vg.size(); ++q) vi[pos[vg[q]]++] = (int)q;
    }
    // element adjacency (conforming hexahedra that share any node share a vertex)
    T.adj.assign((size_t)E, std::vector<int>());
    for (int64_t e = 0; e < E; ++e) {
        auto &a = T.adj[e];
        for (int c = 0; c < NC; ++c) {
            const int v = vg[(size_t)e * NC + c];
            for (int q = vp[v]; q < vp[v + 1]; ++q) a.push_back(vi[q] / NC);
        }
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
    }
    // greedy colouring: two elements of one colour have no common neighbour
    T.colour.assign((size_t)E, -1);
    int ncol = 0;
    std::vector<int> mark;
    for (int64_t e = 0; e < E; ++e) {
        mark.assign((size_t)ncol + 1, 0);
        for (int e1 : T.adj[e])
            for (int e2 : T.adj[e1])
                if (T.colour[e2] >= 0) mark[T.colour[e2]] = 1;
        int cidx = 0;
        while (cidx < ncol && mark[cidx]) ++cidx;
        T.colour[e] = cidx;
        if (cidx == ncol) ++ncol;
    }
    T.ncol = ncol;
}

void boundary_vertices(const Shape &s, const CoarseTopo &T, const std::vector<int> &cidx, std::vector<char> &viface) {
    const int n = s.n, np1 = s.np1(), NC = s.ncorner();
    viface.assign((size_t)T.nvert, 0);
    for (int idx : cidx) {
        const int64_t e = idx / np1;
        const int pt = idx % np1;
        for (int c = 0; c < NC; ++c) {
            const int i = (c & 1) ? n - 1 : 0, j = (c & 2) ? n - 1 : 0, k = (c & 4) ? n - 1 : 0;
            if (pt == i + n * (j + n * k)) viface[T.vg[(size_t)e * NC + c]] = 1;
        }
    }
}

// symmetrise (the probing is symmetric up to rounding) and build the CSR
void coarse_rows(ProbedRows &rows, CoarseCsr &A) {
    const int nvert = (int)rows.size();
    for (int u = 0; u < nvert; ++u)
        for (auto &kv : rows[u])
            if (kv.first > u) {
                auto it = rows[kv.first].find(u);
                const double other = it == rows[kv.first].end() ? kv.second : it->second;
                const double avg = 0.5 * (kv.second + other);
                kv.second = avg;
                rows[kv.first][u] = avg;
            }
    A.rp.assign((size_t)nvert + 1, 0);
    A.ci.clear();
    A.av.clear();
    A.dinv.assign((size_t)nvert, 0.0);
    for (int u = 0; u < nvert; ++u) {
        std::vector<std::pair<int, double>> r(rows[u].begin(), rows[u].end());
        std::sort(r.begin(), r.end());
        for (auto &kv : r) {
            A.ci.push_back(kv.first);
            A.av.push_back(kv.second);
            if (kv.first == u) A.dinv[u] = kv.second > 0 ? 1.0 / kv.second : 0.0;
        }
        A.rp[u + 1] = (int)A.ci.size();
    }
}

// aggregates of vertices (greedy over the vertices that share an element); at most exact_max vertices: every vertex its own
int aggregate(const Shape &s, const CoarseTopo &T, CoarseCsr &A, int exact_max, bool iface, const std::vector<char> &viface, std::vector<int> &agg) {
    const int NC = s.ncorner(), nvert = T.nvert;
    const int64_t E = s.E;
    const std::vector<int> &vg = T.vg, &vp = T.vp, &vi = T.vi;
    agg.assign((size_t)nvert, -1);
    int na = 0;
    if (nvert <= exact_max) {
        for (int v = 0; v < nvert; ++v) agg[v] = v;
        return nvert;
    }
    auto near = [&](int v, std::vector<int> &out) {
        out.clear();
        for (int q = vp[v]; q < vp[v + 1]; ++q) {
            const int e = vi[q] / NC;
            for (int c = 0; c < NC; ++c) out.push_back(vg[(size_t)e * NC + c]);
        }
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
    };
    auto coupling = [&](int v, int w) {   // |A_c[v][w]|, zero outside the pattern
        const int *b = A.ci.data() + A.rp[v], *e = A.ci.data() + A.rp[v + 1];
        const int *it = std::lower_bound(b, e, w);
        return it == e || *it != w ? 0.0 : std::fabs(A.av[it - A.ci.data()]);
    };
    std::vector<int> nb;
    // several ranks: the hats of the vertices on a rank boundary are cut there, and the two halves of one hat are
    // coupled as strongly as the operator penalises a jump, which inflates the diagonal the vertex-level Jacobi term
    // divides by.  Such vertices therefore become aggregates of their own: the aggregate level is global,
    // knows the coupling between the halves and solves them exactly; their Jacobi term is dropped.
    // 3 x 16^3 elements, pressure iterations per time step: plain 2x2x2 aggregates 41.75, planar 2x2 patches of
    // boundary vertices 21, the same without their Jacobi term 16.5, singletons 12.75 (the two patch variants were
    // removed); one rank 12.5.
    if (iface)
        for (int64_t e = 0; e < E; ++e) {
            int cnt = 0;
            for (int c = 0; c < NC; ++c) {
                const int v = vg[(size_t)e * NC + c];
                if (viface[v] && agg[v] < 0) ++cnt;
            }
            if (cnt < 1) continue;
            for (int c = 0; c < NC; ++c) {
                const int v = vg[(size_t)e * NC + c];
                if (viface[v] && agg[v] < 0) agg[v] = na++;
            }
        }
    // an element whose corners are all free becomes an aggregate (2 x 2 x 2 vertices on structured meshes): the
    // aggregate-level operator stays small enough for a dense inverse (nvert / 8 rows) and, unlike the
    // vertex-plus-all-neighbours aggregates used first (27 vertices), accurate enough for the overlapping local
    // solves (12^3 elements: 30.5 iterations with the 27-vertex aggregates, 21.75 with the exact coarse solve)
    for (int64_t e = 0; e < E; ++e) {
        bool free_all = true;
        for (int c = 0; c < NC; ++c)
            if (agg[vg[(size_t)e * NC + c]] >= 0) free_all = false;
        if (!free_all) continue;
        for (int c = 0; c < NC; ++c) agg[vg[(size_t)e * NC + c]] = na;
        ++na;
    }
    if (iface)   // the far-side corners of the boundary elements
        for (int64_t e = 0; e < E; ++e) {
            int cnt = 0;
            for (int c = 0; c < NC; ++c)
                if (agg[vg[(size_t)e * NC + c]] < 0) ++cnt;
            if (cnt < NC / 2) continue;
            for (int c = 0; c < NC; ++c)
                if (agg[vg[(size_t)e * NC + c]] < 0) agg[vg[(size_t)e * NC + c]] = na;
            ++na;
        }
    for (int v = 0; v < nvert; ++v) {
        if (agg[v] >= 0) continue;
        near(v, nb);
        int best = -1;
        double bv = -1.0;
        for (int pass = 0; pass < 2 && best < 0; ++pass)   // first among the vertices of the same kind
            for (int w : nb) {
                if (w == v || agg[w] < 0 || (pass == 0 && viface[w] != viface[v])) continue;
                const double cv = coupling(v, w);
                if (cv > bv) {
                    bv = cv;
                    best = agg[w];
                }
            }
        agg[v] = best >= 0 ? best : na++;
    }
    if (iface)
        for (int v = 0; v < nvert; ++v)
            if (viface[v]) A.dinv[v] = 0.0;
    return na;
}

void assemble_acc(const CoarseCsr &A, const std::vector<int> &agg, int na, bool shift_null_space, AggLevel &G) {
    const int nvert = (int)agg.size();
    G.na = na;
    std::vector<double> &Acc = G.Acc;
    Acc.assign((size_t)na * na, 0.0);
    for (int u = 0; u < nvert; ++u)
        for (int q = A.rp[u]; q < A.rp[u + 1]; ++q) Acc[(size_t)agg[u] * na + agg[A.ci[q]]] += A.av[q];
    for (int i = 0; i < na; ++i)
        for (int j = i + 1; j < na; ++j) Acc[(size_t)i * na + j] = Acc[(size_t)j * na + i] = 0.5 * (Acc[(size_t)i * na + j] + Acc[(size_t)j * na + i]);
    if (shift_null_space) {
        // constant null space (the hats sum to one): shift it so that the inverse acts as the pseudo-inverse on
        // mean-free data.  (Several ranks: the shift is applied to the gathered global operator.)
        double tr = 0.0;
        for (int i = 0; i < na; ++i) tr += Acc[(size_t)i * na + i];
        const double alpha = tr / na / na;   // the null vector of the aggregated operator is the vector of ones
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < na; ++j) Acc[(size_t)i * na + j] += alpha;
    }
    G.ap.assign((size_t)na + 1, 0);
    G.am.assign((size_t)nvert, 0);
    for (int v = 0; v < nvert; ++v) G.ap[agg[v] + 1]++;
    for (int a = 0; a < na; ++a) G.ap[a + 1] += G.ap[a];
    std::vector<int> pos(G.ap.begin(), G.ap.end() - 1);
    for (int v = 0; v < nvert; ++v) G.am[pos[agg[v]]++] = v;
}

}  // namespace pph
}  // namespace nlg
