// Arnoldi / Krylov-Schur eigensolver driving the device kernels: the LightKrylov `eigs` call of
// /root/reference/src/neklab_analysis.f90:80-81, restated (LightKrylov itself is not in the reference
// tree) exactly as in oracle/krylov.py:
//   - Arnoldi with classical Gram-Schmidt + one re-orthogonalisation pass as two block projections
//     (one fused reduction per pass instead of k dots),
//   - Ritz pairs of the projected matrix, residual |h_{k+1,:} y|, sorted by decreasing modulus,
//   - thick restart on the wanted Ritz subspace (Krylov-Schur in its orthonormal-basis form),
//   - eigs_output.txt rows "i Re Im modulus residual T|F" as parsed by
//     /root/reference/test/lib/neklabTestCase.py:425-449.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <numeric>

#include "internal.h"

using namespace nlg;

namespace {

typedef std::complex<double> cplx;

struct Ritz {
    std::vector<cplx> lam;             // sorted by decreasing modulus
    std::vector<std::vector<cplx>> y;  // y[j] = eigenvector j (length k), unit norm
    std::vector<double> res;
};

// H column-major (ldh), leading k x k block + the nrows rows below it (1 for Arnoldi, s for block Arnoldi)
int ritz_pairs(const std::vector<double> &H, int ldh, int k, Ritz &out, int nrows = 1) {
    std::vector<double> A((size_t)k * k), wr(k), wi(k), vr((size_t)k * k);
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < k; ++i) A[(size_t)j * k + i] = H[(size_t)j * ldh + i];
    int rc = nlg_dense_eig(k, A.data(), k, wr.data(), wi.data(), vr.data(), k);
    NLG_CHECK(rc == 0, "eigs: dense eigen-solver failed (rc=%d) on the %d x %d projected matrix", rc, k, k);
    std::vector<cplx> lam(k);
    std::vector<std::vector<cplx>> y(k, std::vector<cplx>(k));
    int j = 0;
    while (j < k) {
        if (wi[j] > 0.0 && j + 1 < k) {
            lam[j] = cplx(wr[j], wi[j]);
            lam[j + 1] = cplx(wr[j], -wi[j]);
            for (int i = 0; i < k; ++i) {
                y[j][i] = cplx(vr[(size_t)j * k + i], vr[(size_t)(j + 1) * k + i]);
                y[j + 1][i] = std::conj(y[j][i]);
            }
            j += 2;
        } else {
            lam[j] = cplx(wr[j], 0.0);
            for (int i = 0; i < k; ++i) y[j][i] = cplx(vr[(size_t)j * k + i], 0.0);
            j += 1;
        }
    }
    std::vector<double> res(k);
    for (int c = 0; c < k; ++c) {
        double r2 = 0.0;
        for (int a = 0; a < nrows; ++a) {
            cplx s = 0.0;
            for (int i = 0; i < k; ++i) s += H[(size_t)i * ldh + k + a] * y[c][i];
            r2 += std::norm(s);
        }
        res[c] = std::sqrt(r2);
    }
    std::vector<int> order(k);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::abs(lam[a]) > std::abs(lam[b]); });
    out.lam.resize(k);
    out.y.resize(k);
    out.res.resize(k);
    for (int c = 0; c < k; ++c) {
        out.lam[c] = lam[order[c]];
        out.y[c] = y[order[c]];
        out.res[c] = res[order[c]];
    }
    return 0;
}

int select_wanted(const std::vector<cplx> &lam, int nkeep_min) {
    const int k = (int)lam.size();
    std::vector<double> mod(k);
    for (int i = 0; i < k; ++i) mod[i] = std::abs(lam[i]);
    std::vector<double> srt(mod);
    std::sort(srt.begin(), srt.end());
    const double med = (k % 2) ? srt[k / 2] : 0.5 * (srt[k / 2 - 1] + srt[k / 2]);
    int p = 0;
    for (int i = 0; i < k; ++i)
        if (mod[i] > med) ++p;
    p = std::max(p, nkeep_min);
    p = std::min(p, k - 1);
    if (p >= 1 && p < k && std::fabs(lam[p - 1].imag()) > 0.0) {
        const cplx d = lam[p - 1] - std::conj(lam[p]);
        if (std::abs(d) <= 1e-10 * std::abs(lam[p]) + 1e-14) ++p;
    }
    return std::min(p, k - 1);
}

// real orthonormal basis (k x p', column-major) of the span of the first p Ritz vectors
void real_basis(const Ritz &r, int k, int p, std::vector<double> &Q, int &pout) {
    std::vector<std::vector<double>> cols;
    int j = 0;
    while (j < p) {
        std::vector<double> re(k), im(k);
        for (int i = 0; i < k; ++i) {
            re[i] = r.y[j][i].real();
            im[i] = r.y[j][i].imag();
        }
        if (std::fabs(r.lam[j].imag()) > 0.0 && j + 1 < p) {
            cols.push_back(re);
            cols.push_back(im);
            j += 2;
        } else {
            cols.push_back(re);
            j += 1;
        }
    }
    // modified Gram-Schmidt, twice
    pout = (int)cols.size();
    for (int c = 0; c < pout; ++c) {
        for (int pass = 0; pass < 2; ++pass)
            for (int b = 0; b < c; ++b) {
                double s = 0.0;
                for (int i = 0; i < k; ++i) s += cols[b][i] * cols[c][i];
                for (int i = 0; i < k; ++i) cols[c][i] -= s * cols[b][i];
            }
        double nrm = 0.0;
        for (int i = 0; i < k; ++i) nrm += cols[c][i] * cols[c][i];
        nrm = std::sqrt(nrm);
        for (int i = 0; i < k; ++i) cols[c][i] /= nrm;
    }
    Q.assign((size_t)k * pout, 0.0);
    for (int c = 0; c < pout; ++c)
        for (int i = 0; i < k; ++i) Q[(size_t)c * k + i] = cols[c][i];
}

void write_log(const char *path, int nmv, const Ritz &r, double tol) {
    FILE *f = fopen(path, "w");
    if (!f) return;
    fprintf(f, "# matvecs = %d   tolerance = %.6e\n", nmv, tol);
    fprintf(f, "#   i              Re                      Im                  modulus                residual   conv\n");
    for (size_t i = 0; i < r.lam.size(); ++i)
        fprintf(f, "%5zu  %22.15e  %22.15e  %22.15e  %14.6e  %s\n", i + 1, r.lam[i].real(), r.lam[i].imag(),
                std::abs(r.lam[i]), r.res[i], r.res[i] < tol ? "T" : "F");
    fclose(f);
}

// One Arnoldi step of s lanes in lock-step, the arguments checked by the caller: lane l's column k through the (block) propagator
// into its column k + 1, CGS2 of every lane against its OWN k + 1 columns, one read-back into column k of every lane's H.
int arnoldi_lanes(nlg_linop *op, int s, nlg_basis *const *basis, int k, double *H, int ldh, int64_t hstride, int transpose) {
    const nlg_vec *vi[kMaxLanes];
    nlg_vec *vo[kMaxLanes];
    for (int l = 0; l < s; ++l) vi[l] = basis[l]->views[k], vo[l] = basis[l]->views[k + 1];
    NLG_TRY(nlg_linop_matvec_block(op, s, vi, vo, transpose));
    double *col = H + (size_t)k * ldh;
    return basis_cgs2_host(s, basis, k + 1, vo, col, hstride, col + k + 1, hstride);
}

}  // namespace

extern "C" {

int nlg_arnoldi_step(nlg_linop *op, nlg_basis *basis, int k, double *H, int ldh, int transpose) {
    NLG_CHECK(op && basis && H, "nlg_arnoldi_step: NULL argument");
    NLG_CHECK(k >= 0 && k + 1 < basis->nvec, "nlg_arnoldi_step: k=%d needs basis columns %d, %d (nvec=%d)", k, k, k + 1, basis->nvec);
    NLG_CHECK(ldh >= k + 2, "nlg_arnoldi_step: ldh=%d too small for k=%d", ldh, k);
    return arnoldi_lanes(op, 1, &basis, k, H, ldh, 0, transpose);
}

// One Arnoldi step of the bordered Jacobian of a periodic orbit on extended vectors (field, T): column k of the basis with period
// component tcol[k] -> column k + 1 / tcol[k + 1], CGS2 in the extended inner product <u, v> + t_u t_v (the reference's
// nek_ext_dvector dot, src/vectors/real_extended_vectors.f90), from the block projections of the basis with the scalar terms added on
// the host.
int nlg_upo_arnoldi_step(nlg_linop *op, nlg_basis *basis, double *tcol, int k, double *H, int ldh) {
    NLG_CHECK(op, "nlg_upo_arnoldi_step: NULL operator, one in orbit mode is needed (nlg_linop_set_orbit)");
    NLG_CHECK(basis && tcol && H, "nlg_upo_arnoldi_step: NULL argument");
    NLG_CHECK(k >= 0 && k + 1 < basis->nvec, "nlg_upo_arnoldi_step: k=%d needs basis columns %d, %d (nvec=%d)", k, k, k + 1, basis->nvec);
    NLG_CHECK(ldh >= k + 2, "nlg_upo_arnoldi_step: ldh=%d too small for k=%d", ldh, k);
    nlg_vec *vk = basis->views[k], *w = basis->views[k + 1];
    double tw = 0.0;
    NLG_TRY(nlg_upo_jac_matvec(op, vk, tcol[k], w, &tw));   // (refuses an operator that is not in orbit mode)
    const int kk = k + 1;
    std::vector<double> h(kk, 0.0), hp(kk);
    for (int pass = 0; pass < 2; ++pass) {
        NLG_TRY(nlg_basis_block_dot(basis, kk, w, hp.data()));
        for (int j = 0; j < kk; ++j) hp[j] += tcol[j] * tw;
        NLG_TRY(nlg_basis_block_axpy(basis, kk, hp.data(), w));
        for (int j = 0; j < kk; ++j) {
            tw -= hp[j] * tcol[j];
            h[j] += hp[j];
        }
    }
    double ww = 0.0;
    NLG_TRY(nlg_vec_dot(w, w, &ww));
    const double beta = std::sqrt(ww + tw * tw);
    if (beta > 0.0) NLG_TRY(nlg_vec_scal(w, 1.0 / beta));
    tcol[k + 1] = beta > 0.0 ? tw / beta : 0.0;
    for (int j = 0; j < kk; ++j) H[(size_t)k * ldh + j] = h[j];
    H[(size_t)k * ldh + k + 1] = beta;
    return 0;
}

int nlg_block_arnoldi_step(nlg_linop *op, nlg_basis *basis, int k, int s, double *H, int ldh, int transpose) {
    NLG_CHECK(op && basis && H, "nlg_block_arnoldi_step: NULL argument");
    NLG_CHECK(s >= 1 && s <= 4, "nlg_block_arnoldi_step: block size %d unsupported (1..4)", s);
    NLG_CHECK(k >= 0 && k + 2 * s <= basis->nvec, "nlg_block_arnoldi_step: k=%d, s=%d need basis columns up to %d (nvec=%d)", k, s,
              k + 2 * s - 1, basis->nvec);
    NLG_CHECK(ldh >= k + 2 * s, "nlg_block_arnoldi_step: ldh=%d too small for k=%d, s=%d", ldh, k, s);
    if (s > 1) {   // the s vectors advance together (shared operator data per iteration)
        const nlg_vec *vi[4];
        nlg_vec *vo[4];
        for (int v = 0; v < s; ++v) vi[v] = basis->views[k + v], vo[v] = basis->views[k + s + v];
        NLG_TRY(nlg_linop_matvec_block(op, s, vi, vo, transpose));
    } else {
        for (int v = 0; v < s; ++v) {
            nlg_vec *vin = basis->views[k + v], *w = basis->views[k + s + v];
            NLG_TRY(transpose ? nlg_linop_rmatvec(op, vin, w) : nlg_linop_matvec(op, vin, w));
        }
    }
    const int kk = k + s;
    std::vector<double> coef((size_t)(kk + s) * s);
    NLG_TRY(nlg_basis_block_cgs2(basis, kk, s, coef.data()));
    for (int v = 0; v < s; ++v)
        for (int i = 0; i < kk + s; ++i) H[(size_t)(k + v) * ldh + i] = coef[(size_t)v * (kk + s) + i];
    return 0;
}

// One Arnoldi step of s separate eigenproblems in lock-step (a wavenumber sweep): lane l's column k through the block propagator, at
// lane l's wavenumber, into its column k + 1, then the batched CGS2 of every lane against its OWN basis.
int nlg_sweep_arnoldi_step(nlg_linop *op, int s, nlg_basis *const *basis, int k, double *H, int ldh, int64_t hstride, int transpose) {
    NLG_CHECK(op && basis && H, "nlg_sweep_arnoldi_step: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_sweep_arnoldi_step: %d lanes unsupported (1..%d)", s, kMaxLanes);
    const int nalpha = linop_proj_lanes(op);
    NLG_CHECK(nalpha > 0, "nlg_sweep_arnoldi_step: the operator has no wavenumber lanes (nlg_linop_set_projection_lanes)");
    NLG_CHECK(s <= nalpha, "nlg_sweep_arnoldi_step: %d lanes on an operator with %d wavenumber lanes", s, nalpha);
    for (int l = 0; l < s; ++l) {
        NLG_CHECK(basis[l], "nlg_sweep_arnoldi_step: NULL basis in lane %d", l);
        NLG_CHECK(k >= 0 && k + 1 < basis[l]->nvec, "nlg_sweep_arnoldi_step: k=%d needs basis columns %d, %d (nvec=%d)", k, k, k + 1, basis[l]->nvec);
        for (int u = 0; u < l; ++u) NLG_CHECK(basis[l] != basis[u], "nlg_sweep_arnoldi_step: the same basis in two lanes");
    }
    NLG_CHECK(ldh >= k + 2, "nlg_sweep_arnoldi_step: ldh=%d too small for k=%d", ldh, k);
    for (int l = 1; l < s; ++l)
        NLG_CHECK(basis[l]->mesh == basis[0]->mesh && basis[l]->nscal == basis[0]->nscal && basis[l]->lorder == basis[0]->lorder && basis[l]->nvec == basis[0]->nvec,
                  "nlg_sweep_arnoldi_step: the bases differ in shape (lane %d)", l);
    return arnoldi_lanes(op, s, basis, k, H, ldh, hstride, transpose);
}

int nlg_eigs_opts_default(nlg_eigs_opts *o) {
    NLG_CHECK(o, "nlg_eigs_opts_default: NULL");
    o->kdim = 0;
    o->transpose = 0;
    o->max_restarts = 50;
    o->write_intermediate = 1;
    o->tol = 0.0;
    o->logfile = nullptr;
    o->seed = 0;
    o->block_size = 0;
    o->warm_start = 0;
    return 0;
}

int nlg_eigs(nlg_linop *op, nlg_vec **X, int nev, double *eig_re, double *eig_im, double *residuals, int *info,
             const nlg_vec *x0, const nlg_eigs_opts *opts_in) {
    NLG_CHECK(op && X && eig_re && eig_im && residuals && info, "nlg_eigs: NULL argument");
    NLG_CHECK(nev >= 1, "nlg_eigs: nev must be >= 1");
    nlg_eigs_opts o;
    nlg_eigs_opts_default(&o);
    if (opts_in) o = *opts_in;
    const int kdim = o.kdim > 0 ? o.kdim : 4 * nev;   // LightKrylov default kdim = 4*nev
    NLG_CHECK(kdim > nev, "nlg_eigs: kdim=%d must exceed nev=%d", kdim, nev);
    const double tol = o.tol > 0.0 ? o.tol : std::sqrt(1e-15);
    const char *logfile = o.logfile ? o.logfile : "eigs_output.txt";
    nlg_vec *proto = X[0];
    NLG_CHECK(proto, "nlg_eigs: X[0] is NULL");
    nlg_mesh *mesh = proto->mesh;
    *info = -1;

    const int bs = o.block_size > 1 ? o.block_size : 1;
    NLG_CHECK(bs <= 4, "nlg_eigs: block_size %d unsupported (1..4)", bs);
    NLG_CHECK(bs == 1 || (kdim / bs) * bs > nev, "nlg_eigs: kdim=%d leaves no room for nev=%d with blocks of %d", kdim, nev, bs);
    nlg_basis *V = nullptr, *T = nullptr;
    NLG_TRY(nlg_basis_create(mesh, proto->nscal, proto->lorder, kdim + bs, &V));
    auto cleanup = [&]() {
        nlg_basis_destroy(V);
        if (T) nlg_basis_destroy(T);
    };
    int rc = 0;
#define EIGS_TRY(call)  \
    do {                \
        rc = (call);    \
        if (rc) {       \
            cleanup();  \
            return rc;  \
        }               \
    } while (0)

    // start vector
    if (x0) {
        EIGS_TRY(nlg_vec_copy(V->views[0], x0));
    } else {
        EIGS_TRY(nlg_vec_zero(V->views[0]));
        EIGS_TRY(nlg_vec_rand(V->views[0], 0, o.seed));
    }
    {
        double nrm = 0.0;
        EIGS_TRY(nlg_vec_norm(V->views[0], &nrm));
        if (!(nrm > 0.0)) {
            cleanup();
            set_error("nlg_eigs: start vector has zero norm");
            return 1;
        }
        EIGS_TRY(nlg_vec_scal(V->views[0], 1.0 / nrm));
    }
    const int ldh = kdim + bs;
    std::vector<double> H((size_t)ldh * kdim, 0.0);
    Ritz r;
    int kstart = 0, nmv = 0, k = 0;
    bool done = false;
    // Warm start: replace a start column by its IMAGE.  A random start vector has no restart history, so its matvec starts
    // impulsively (BDF1) while every later Krylov vector is continued at full order: the first column of the Arnoldi
    // relation then belongs to a different linear map than the others, a rank-one inconsistency that does not decay -- the
    // converged Ritz values depend on the start vector (cylinder, Re = 50: |mu_1| between 1.015705 and 1.015865 over eight
    // seeds at residual 1e-9; from the image: 1.0157265 for every seed, profiles/r02_cylinder_*.txt).  Off by default: the
    // reference (LightKrylov) starts from the raw vector.
    auto warm = [&](int col) -> int {
        nlg_vec *w = nullptr;
        NLG_TRY(nlg_vec_clone(V->views[col], &w));
        int rc2 = o.transpose ? nlg_linop_rmatvec(op, w, V->views[col]) : nlg_linop_matvec(op, w, V->views[col]);
        nlg_vec_destroy(w);
        if (rc2) return rc2;
        ++nmv;
        double nrm = 0.0;
        NLG_TRY(nlg_vec_norm(V->views[col], &nrm));
        NLG_CHECK(nrm > 0.0, "nlg_eigs: the image of the start vector vanishes");
        return nlg_vec_scal(V->views[col], 1.0 / nrm);
    };
    if (o.warm_start) EIGS_TRY(warm(0));
    if (bs > 1) {
        // ---- block Arnoldi (BASELINE.json config 5): s vectors per step, the basis read once per s vectors in every
        // Gram-Schmidt pass (nlg_basis_block_cgs2); no restart -- kdim is the size of the block Krylov space
        const int kd = (kdim / bs) * bs;
        for (int v = 1; v < bs; ++v) {
            EIGS_TRY(nlg_vec_zero(V->views[v]));
            EIGS_TRY(nlg_vec_rand(V->views[v], 0, o.seed + 7919ull * (uint64_t)v));
            if (o.warm_start) EIGS_TRY(warm(v));
        }
        std::vector<double> c0((size_t)bs * bs);
        EIGS_TRY(nlg_basis_block_cgs2(V, 0, bs, c0.data()));
        while (k < kd) {
            EIGS_TRY(nlg_block_arnoldi_step(op, V, k, bs, H.data(), ldh, o.transpose));
            nmv += bs;
            k += bs;
            EIGS_TRY(ritz_pairs(H, ldh, k, r, bs));
            int conv = 0;
            for (int i = 0; i < k; ++i)
                if (r.res[i] < tol) ++conv;
            if (o.write_intermediate) write_log(logfile, nmv, r, tol);
            if (conv >= nev) break;
            // a deflated column in the new block: the block Krylov space has (numerically) reached an invariant subspace -- the block
            // counterpart of beta = 0.  The Ritz pairs of the space built so far are returned instead of an error.
            if (V->last_block_rank < bs) break;
        }
    } else
    for (int restart = 0; restart <= o.max_restarts; ++restart) {
        k = kstart;
        while (k < kdim) {
            EIGS_TRY(nlg_arnoldi_step(op, V, k, H.data(), ldh, o.transpose));
            ++nmv;
            ++k;
            EIGS_TRY(ritz_pairs(H, ldh, k, r));
            int conv = 0;
            for (int i = 0; i < k; ++i)
                if (r.res[i] < tol) ++conv;
            if (o.write_intermediate) write_log(logfile, nmv, r, tol);
            if (conv >= nev) {
                done = true;
                break;
            }
        }
        if (done || k < kdim) break;
        if (restart == o.max_restarts) break;
        // thick restart
        int p = select_wanted(r.lam, nev);
        std::vector<double> Q;
        int pq = 0;
        real_basis(r, k, p, Q, pq);
        p = pq;
        if (!T) EIGS_TRY(nlg_basis_create(mesh, proto->nscal, proto->lorder, kdim, &T));
        for (int j = 0; j < p; ++j) EIGS_TRY(nlg_basis_combine(V, k, Q.data() + (size_t)j * k, T->views[j]));
        // S = Q^T H_k Q ; b = H[k, :k] Q
        std::vector<double> HQ((size_t)k * p, 0.0), S((size_t)p * p, 0.0), b(p, 0.0);
        for (int j = 0; j < p; ++j)
            for (int i = 0; i < k; ++i) {
                double s = 0.0;
                for (int l = 0; l < k; ++l) s += H[(size_t)l * ldh + i] * Q[(size_t)j * k + l];
                HQ[(size_t)j * k + i] = s;
            }
        for (int j = 0; j < p; ++j) {
            for (int i = 0; i < p; ++i) {
                double s = 0.0;
                for (int l = 0; l < k; ++l) s += Q[(size_t)i * k + l] * HQ[(size_t)j * k + l];
                S[(size_t)j * p + i] = s;
            }
            double s = 0.0;
            for (int l = 0; l < k; ++l) s += H[(size_t)l * ldh + k] * Q[(size_t)j * k + l];
            b[j] = s;
        }
        EIGS_TRY(nlg_vec_copy(T->views[p], V->views[k]));
        std::fill(H.begin(), H.end(), 0.0);
        for (int j = 0; j < p; ++j) {
            for (int i = 0; i < p; ++i) H[(size_t)j * ldh + i] = S[(size_t)j * p + i];
            H[(size_t)j * ldh + p] = b[j];
        }
        for (int j = 0; j <= p; ++j) EIGS_TRY(nlg_vec_copy(V->views[j], T->views[j]));
        kstart = p;
    }
    const int kf = k;
    const int nout = std::min(nev, kf);
    // eigenvectors (real LAPACK convention)
    {
        int j = 0;
        std::vector<double> c(kf);
        while (j < nout) {
            if (std::fabs(r.lam[j].imag()) > 0.0) {
                const bool pos = r.lam[j].imag() > 0.0;
                for (int i = 0; i < kf; ++i) c[i] = r.y[j][i].real();
                EIGS_TRY(nlg_basis_combine(V, kf, c.data(), X[j]));
                if (j + 1 < nout) {
                    for (int i = 0; i < kf; ++i) c[i] = pos ? r.y[j][i].imag() : -r.y[j][i].imag();
                    EIGS_TRY(nlg_basis_combine(V, kf, c.data(), X[j + 1]));
                }
                j += 2;
            } else {
                for (int i = 0; i < kf; ++i) c[i] = r.y[j][i].real();
                EIGS_TRY(nlg_basis_combine(V, kf, c.data(), X[j]));
                j += 1;
            }
        }
    }
    for (int j = 0; j < nev; ++j) {
        if (j < nout) {
            eig_re[j] = r.lam[j].real();
            eig_im[j] = r.lam[j].imag();
            residuals[j] = r.res[j];
        } else {
            eig_re[j] = eig_im[j] = 0.0;
            residuals[j] = -1.0;
        }
    }
    *info = nmv;
    cleanup();
#undef EIGS_TRY
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// svds: the LightKrylov call of transient_growth_analysis_fixed_point (src/neklab_analysis.f90:136), restated as
// Golub-Kahan-Lanczos bidiagonalisation with full re-orthogonalisation (CGS2 against all previous left / right
// vectors, block kernels): A^T u_k -> v_k, A v_k -> u_{k+1};  B_k (k x k upper part of the lower-bidiagonal matrix)
// = P S Q^T, triplets (S_i, U_k p_i, V_k q_i), residual |beta_{k+1} q_i[k]|.  rmatvec is the (continuous) adjoint
// propagator, as in the reference.
int nlg_svds(nlg_linop *op, nlg_vec **U, nlg_vec **V, int nsv, double *S, double *residuals, int *info,
             const nlg_vec *u0, const nlg_eigs_opts *opts_in) {
    NLG_CHECK(op && U && V && S && residuals && info, "nlg_svds: NULL argument");
    NLG_CHECK(nsv >= 1, "nlg_svds: nsv must be >= 1");
    nlg_eigs_opts o;
    nlg_eigs_opts_default(&o);
    if (opts_in) o = *opts_in;
    const int kdim = o.kdim > 0 ? o.kdim : 4 * nsv;
    NLG_CHECK(kdim >= nsv, "nlg_svds: kdim=%d must be >= nsv=%d", kdim, nsv);
    const double tol = o.tol > 0.0 ? o.tol : std::sqrt(1e-15);
    const char *logfile = o.logfile ? o.logfile : "svds_output.txt";
    nlg_vec *proto = U[0];
    NLG_CHECK(proto && V[0], "nlg_svds: U[0] / V[0] is NULL");
    nlg_mesh *mesh = proto->mesh;
    *info = -1;
    nlg_basis *Ub = nullptr, *Vb = nullptr;
    NLG_TRY(nlg_basis_create(mesh, proto->nscal, proto->lorder, kdim + 1, &Ub));
    int rc = nlg_basis_create(mesh, proto->nscal, proto->lorder, kdim, &Vb);
    if (rc) {
        nlg_basis_destroy(Ub);
        return rc;
    }
    auto cleanup = [&]() {
        nlg_basis_destroy(Ub);
        nlg_basis_destroy(Vb);
    };
#define SVDS_TRY(call)  \
    do {                \
        rc = (call);    \
        if (rc) {       \
            cleanup();  \
            return rc;  \
        }               \
    } while (0)
    if (u0) {
        SVDS_TRY(nlg_vec_copy(Ub->views[0], u0));
    } else {
        SVDS_TRY(nlg_vec_zero(Ub->views[0]));
        SVDS_TRY(nlg_vec_rand(Ub->views[0], 0, o.seed));
    }
    {
        double nrm = 0.0;
        SVDS_TRY(nlg_vec_norm(Ub->views[0], &nrm));
        if (!(nrm > 0.0)) {
            cleanup();
            set_error("nlg_svds: start vector has zero norm");
            return 1;
        }
        SVDS_TRY(nlg_vec_scal(Ub->views[0], 1.0 / nrm));
    }
    std::vector<double> alpha(kdim, 0.0), beta(kdim + 1, 0.0), hh(kdim + 2);
    std::vector<double> sig, Q, Pm;
    std::vector<double> res_all;
    int k = 0, nmv = 0;
    bool done = false;
    while (k < kdim && !done) {
        double b = 0.0;
        // right vector: v_k = A^T u_k, orthogonalised against v_0..v_{k-1}
        SVDS_TRY(nlg_linop_rmatvec(op, Ub->views[k], Vb->views[k]));
        SVDS_TRY(nlg_basis_cgs2(Vb, k, Vb->views[k], hh.data(), &b));
        alpha[k] = b;
        // left vector: u_{k+1} = A v_k, orthogonalised against u_0..u_k
        SVDS_TRY(nlg_linop_matvec(op, Vb->views[k], Ub->views[k + 1]));
        SVDS_TRY(nlg_basis_cgs2(Ub, k + 1, Ub->views[k + 1], hh.data(), &b));
        beta[k + 1] = b;
        nmv += 2;
        ++k;
        // SVD of the k x k part: B[i][i] = alpha_i, B[i+1][i] = beta_{i+1}  ->  T = B^T B (tridiagonal)
        std::vector<double> d(k), e(k, 0.0), Z((size_t)k * k);
        for (int i = 0; i < k; ++i) {
            d[i] = alpha[i] * alpha[i] + (i + 1 < k ? beta[i + 1] * beta[i + 1] : 0.0);
            if (i > 0) e[i] = alpha[i] * beta[i];
        }
        if (nlg_symtridiag_eig(k, d.data(), e.data(), Z.data()) != 0) {
            cleanup();
            set_error("nlg_svds: tridiagonal eigen-solver failed at k=%d", k);
            return 1;
        }
        sig.assign(k, 0.0);
        Q.assign((size_t)k * k, 0.0);
        res_all.assign(k, 0.0);
        int conv = 0;
        for (int i = 0; i < k; ++i) {   // descending singular values
            const int src = k - 1 - i;
            sig[i] = std::sqrt(std::max(d[src], 0.0));
            for (int r = 0; r < k; ++r) Q[(size_t)i * k + r] = Z[(size_t)r * k + src];
            res_all[i] = std::fabs(beta[k] * Q[(size_t)i * k + (k - 1)]);
            if (res_all[i] < tol) ++conv;
        }
        if (o.write_intermediate) {
            FILE *f = fopen(logfile, "w");
            if (f) {
                fprintf(f, "# matvecs = %d   tolerance = %.6e\n#   i          sigma                residual   conv\n", nmv, tol);
                for (int i = 0; i < k; ++i)
                    fprintf(f, "%5d  %22.15e  %14.6e  %s\n", i + 1, sig[i], res_all[i], res_all[i] < tol ? "T" : "F");
                fclose(f);
            }
        }
        if (conv >= nsv) done = true;
    }
    // singular vectors: v_i = V_k q_i ; u_i = U_k p_i with p_i = B q_i / sigma_i (k components)
    const int nout = std::min(nsv, k);
    std::vector<double> c(k);
    for (int i = 0; i < nout; ++i) {
        for (int r = 0; r < k; ++r) c[r] = Q[(size_t)i * k + r];
        SVDS_TRY(nlg_basis_combine(Vb, k, c.data(), V[i]));
        for (int r = 0; r < k; ++r) {
            double s = alpha[r] * Q[(size_t)i * k + r];
            if (r > 0) s += beta[r] * Q[(size_t)i * k + r - 1];
            c[r] = sig[i] > 0 ? s / sig[i] : 0.0;
        }
        SVDS_TRY(nlg_basis_combine(Ub, k, c.data(), U[i]));
    }
    for (int i = 0; i < nsv; ++i) {
        S[i] = i < nout ? sig[i] : 0.0;
        residuals[i] = i < nout ? res_all[i] : -1.0;
    }
    *info = nmv;
    cleanup();
#undef SVDS_TRY
    return 0;
}

}  // extern "C"
