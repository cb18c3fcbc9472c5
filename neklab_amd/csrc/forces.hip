// Wall forces, torque and heat flux on sets of element faces (nlg_forces_*, include/neklab_gpu.h; the observable of the reference's
// cylinder and temperature cases, Nek5000's torque_calc convention).  The geometry of the faces is computed on the host once
// (forces_host.cpp); a sample is two launches: one wave per (face, vector) forms the face's share of every quantity, then one block per
// (object, vector) sums the faces of the object in the order fixed at creation.  No atomics: the results repeat bit for bit.
//
// Definitions.  A face is (global element id, face), face in the preprocessor's numbering 1 = s-, 2 = r+, 3 = s+, 4 = r-, 5 = t-, 6 = t+;
// an object is a set of faces.  At face point q of a face normal to reference direction a on side sigma the area-weighted outward normal
// is N_q = sigma (J grad r_a)_q w_q, w_q the GLL weights of the tangential directions.  (grad u)_q is the pointwise element-local
// gradient; p_q the element's Gauss-mesh pressure carried to the face point by the tensor Lagrange interpolation GL -> GLL, element by
// element, without the direct-stiffness average of `mappr`.  No masks.  Per object, with the centre c:
//   Fp_i = sum p_q N_q,i                      Fv_i = -nu sum_j (d_j u_i + d_i u_j)_q N_q,j
//   Tp   = sum (x_q - c) x (p_q N_q)          Tv   = the same with the viscous traction          Q = sum (grad theta)_q . N_q
// With the outward normals pointing into the body, Fp + Fv is the force the fluid exerts on the body.
// Output per (vector, object): Fp[dim], Fv[dim], Tp[nt], Tv[nt], Q; nt = 1 (z) in 2-D, 3 in 3-D.
#include "internal.h"
#include "forces_host.h"

#include <algorithm>

using namespace nlg;

namespace {

constexpr int NTF = 64;     // one wave per (face, vector)
constexpr int NTR = 256;
constexpr int kMaxNQ = 13;

struct FaceArgs {
    ForceFields F;
    int dim, n, n2;
    const int *elem, *face;
    const double *nds, *met, *xc, *D, *M;
    double nu;
    int64_t nfl;
    double *part;   // [lanes][nfl][nq]
    double *trac;   // null, or [nfl][nfp][1 + 2 dim] of lane 0: p, traction, N
};

// Face f of vector v.  The 1-D matrices go to LDS first; the pressure is contracted along the face normal with row ia of M once per face
// (sP), then every face point takes the tangential rows.  A point's normal derivative comes from the line through it normal to the
// face, its tangential derivatives from the face's own values; faces of more than 64 points loop.
__global__ __launch_bounds__(NTF) void k_wall_forces(FaceArgs A) {
    __shared__ double sD[forces::kMaxN * forces::kMaxN], sM[forces::kMaxN * forces::kMaxN], sP[forces::kMaxN * forces::kMaxN];
    const int t = threadIdx.x, v = blockIdx.y;
    const int64_t f = blockIdx.x;
    const int dim = A.dim, n = A.n, n2 = A.n2;
    for (int i = t; i < n * n; i += NTF) sD[i] = A.D[i];
    for (int i = t; i < n * n2; i += NTF) sM[i] = A.M[i];
    const int e = A.elem[f], fc = A.face[f];
    const int a = forces::face_dir(fc), sg = forces::face_side(fc);
    const int ia = sg > 0 ? n - 1 : 0;
    const int nfp = dim == 3 ? n * n : n, nfp2 = dim == 3 ? n2 * n2 : n2;
    const int np = nfp * n, np2 = nfp2 * n2;
    const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    const int st1[3] = {1, n, n * n}, st2[3] = {1, n2, n2 * n2};
    const int sa2 = a == 0 ? st2[0] : (a == 1 ? st2[1] : st2[2]), sb2 = b == 0 ? st2[0] : st2[1], sc2 = c == 1 ? st2[1] : st2[2];
    __syncthreads();
    {
        const double *__restrict__ p = A.F.p[v] + (int64_t)e * np2;
        for (int r = t; r < nfp2; r += NTF) {
            const int kb = r % n2, kc = r / n2;
            const double *line = p + kb * sb2 + (dim == 3 ? kc * sc2 : 0);
            double s = 0.0;
            for (int ka = 0; ka < n2; ++ka) s += sM[ia * n2 + ka] * line[ka * sa2];
            sP[r] = s;
        }
    }
    __syncthreads();
    const double *__restrict__ th = A.F.th[v] ? A.F.th[v] + (int64_t)e * np : nullptr;
    double acc[kMaxNQ];
#pragma unroll
    for (int k = 0; k < kMaxNQ; ++k) acc[k] = 0.0;
    for (int q = t; q < nfp; q += NTF) {
        const int tb = q % n, tc = q / n;
        double pq = 0.0;
        for (int kc = 0; kc < (dim == 3 ? n2 : 1); ++kc) {
            double s = 0.0;
            for (int kb = 0; kb < n2; ++kb) s += sM[tb * n2 + kb] * sP[kb + n2 * kc];
            pq += dim == 3 ? sM[tc * n2 + kc] * s : s;
        }
        const int i0 = a == 0 ? ia : tb, i1 = a == 1 ? ia : (a == 0 ? tb : tc), i2 = a == 2 ? ia : tc;
        const int pidx = i0 + n * i1 + n * n * (dim == 3 ? i2 : 0);
        const int64_t fq = f * nfp + q;
        double N[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0}, G[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < dim) N[i] = A.nds[fq * dim + i], X[i] = A.xc[fq * dim + i];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) G[j][i] = j < dim && i < dim ? A.met[fq * dim * dim + j * dim + i] : 0.0;
        // g[ci][i] = d_i u_ci; row dim holds grad theta
        double g[4][3];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const double *__restrict__ u = ci < 3 ? (ci < dim ? A.F.u[v][ci] + (int64_t)e * np : nullptr) : th;
            double ur[3] = {0.0, 0.0, 0.0};
            if (u) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < dim) {
                        const int ij = j == 0 ? i0 : (j == 1 ? i1 : i2);
                        const double *line = u + pidx - ij * st1[j];
                        double s = 0.0;
                        for (int m = 0; m < n; ++m) s += sD[ij * n + m] * line[m * st1[j]];
                        ur[j] = s;
                    }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) g[ci][i] = G[0][i] * ur[0] + G[1][i] * ur[1] + G[2][i] * ur[2];
        }
        double fp[3], fv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            fp[i] = pq * N[i];
            fv[i] = -A.nu * ((g[i][0] + g[0][i]) * N[0] + (g[i][1] + g[1][i]) * N[1] + (g[i][2] + g[2][i]) * N[2]);
        }
        const double qn = g[3][0] * N[0] + g[3][1] * N[1] + g[3][2] * N[2];
        if (dim == 2) {
            acc[0] += fp[0], acc[1] += fp[1], acc[2] += fv[0], acc[3] += fv[1];
            acc[4] += X[0] * fp[1] - X[1] * fp[0];
            acc[5] += X[0] * fv[1] - X[1] * fv[0];
            acc[6] += qn;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int i1c = (i + 1) % 3, i2c = (i + 2) % 3;
                acc[i] += fp[i], acc[3 + i] += fv[i];
                acc[6 + i] += X[i1c] * fp[i2c] - X[i2c] * fp[i1c];
                acc[9 + i] += X[i1c] * fv[i2c] - X[i2c] * fv[i1c];
            }
            acc[12] += qn;
        }
        if (A.trac && v == 0) {
            double *o = A.trac + fq * (1 + 2 * dim);
            o[0] = pq;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (i < dim) o[1 + i] = fp[i] + fv[i], o[1 + dim + i] = N[i];
        }
    }
    const int nq = forces::nquant(dim);
#pragma unroll
    for (int k = 0; k < kMaxNQ; ++k) {
        double s = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (t == 0 && k < nq) A.part[((int64_t)v * A.nfl + f) * nq + k] = s;
    }
}

// out[v * ldo + o * nq + k] = the sum over the faces of object o, in the order of oidx: thread t takes faces t, t + NTR, ..., then the
// fixed shuffle tree and the waves in turn
__global__ __launch_bounds__(NTR) void k_wall_forces_reduce(const double *__restrict__ part, int64_t nfl, int nq, const int *__restrict__ ooff,
                                                            const int *__restrict__ oidx, double *__restrict__ out, int64_t ldo) {
    __shared__ double sm[NTR / 64][kMaxNQ];
    const int o = blockIdx.x, v = blockIdx.y, t = threadIdx.x;
    double acc[kMaxNQ];
#pragma unroll
    for (int k = 0; k < kMaxNQ; ++k) acc[k] = 0.0;
    for (int r = ooff[o] + t; r < ooff[o + 1]; r += NTR) {
        const double *__restrict__ pf = part + ((int64_t)v * nfl + oidx[r]) * nq;
#pragma unroll
        for (int k = 0; k < kMaxNQ; ++k)
            if (k < nq) acc[k] += pf[k];
    }
#pragma unroll
    for (int k = 0; k < kMaxNQ; ++k) {
        double s = acc[k];
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) s += __shfl_down(s, w, 64);
        if ((t & 63) == 0) sm[t >> 6][k] = s;
    }
    __syncthreads();
    if (t < nq) {
        double s = 0.0;
        for (int w = 0; w < NTR / 64; ++w) s += sm[w][t];
        out[(int64_t)v * ldo + (int64_t)o * nq + t] = s;
    }
}

template <typename T>
int upload(T **dst, const std::vector<T> &src, hipStream_t st) {
    NLG_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(src.size(), 1)));
    if (!src.empty()) NLG_HIP(hipMemcpyAsync(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, st));
    return 0;
}

int launch_faces(nlg_forces *f, int s, const ForceFields &F, double nu, double *trac) {
    if (f->nfl == 0) return 0;
    nlg_mesh *m = f->mesh;
    FaceArgs A;
    A.F = F;
    A.dim = m->dim, A.n = m->n, A.n2 = m->n2;
    A.elem = f->d_elem, A.face = f->d_face;
    A.nds = f->d_nds, A.met = f->d_met, A.xc = f->d_xc, A.D = m->d_D, A.M = f->d_M;
    A.nu = nu;
    A.nfl = f->nfl;
    A.part = f->d_part;
    A.trac = trac;
    NLG_LAUNCH(k_wall_forces, dim3((unsigned)f->nfl, (unsigned)s), dim3(NTF), 0, m->ctx->stream, A);
    return 0;
}

ForceFields fields_of(int s, const nlg_vec *const *vecs) {
    ForceFields F;
    memset(&F, 0, sizeof(F));
    for (int v = 0; v < s; ++v) {
        for (int c = 0; c < vecs[v]->mesh->dim; ++c) F.u[v][c] = vecs[v]->vel(c);
        F.p[v] = vecs[v]->pr();
        if (vecs[v]->nscal >= 1) F.th[v] = vecs[v]->theta(0);
    }
    return F;
}

// validate the global list, keep this rank's faces in sorted order, compute and upload their geometry, all-reduce the areas
int forces_build(nlg_forces *f, const int64_t *elem_gid, const int *face, const int *obj, const double *centre) {
    nlg_mesh *m = f->mesh;
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int dim = m->dim, n = m->n, nobj = f->nobj;
    const int64_t nf = f->nfaces;
    for (int64_t q = 0; q < nf; ++q) {
        NLG_CHECK(face[q] >= 1 && face[q] <= 2 * dim, "nlg_forces_create: face[%lld] = %d outside 1..%d", (long long)q, face[q], 2 * dim);
        NLG_CHECK(obj[q] >= 0 && obj[q] < nobj, "nlg_forces_create: obj[%lld] = %d outside 0..%d", (long long)q, obj[q], nobj - 1);
        NLG_CHECK(elem_gid[q] >= 0, "nlg_forces_create: elem_gid[%lld] = %lld is negative", (long long)q, (long long)elem_gid[q]);
    }
    std::vector<int64_t> ord((size_t)nf);   // the list sorted by (element, face)
    for (int64_t q = 0; q < nf; ++q) ord[q] = q;
    std::sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) {
        return elem_gid[x] != elem_gid[y] ? elem_gid[x] < elem_gid[y] : (face[x] != face[y] ? face[x] < face[y] : x < y);
    });
    for (int64_t q = 1; q < nf; ++q)
        NLG_CHECK(elem_gid[ord[q]] != elem_gid[ord[q - 1]] || face[ord[q]] != face[ord[q - 1]],
                  "nlg_forces_create: elem_gid / face: face %d of element %lld is listed twice (entries %lld and %lld)", face[ord[q]],
                  (long long)elem_gid[ord[q]], (long long)ord[q - 1], (long long)ord[q]);
    std::map<int64_t, int> local;
    for (int64_t e = 0; e < m->E; ++e) local[m->h_lglel[e]] = (int)e;
    // this rank's faces, sorted; their rank in creation order
    std::vector<int64_t> el, mine;
    std::vector<int> fc, ob;
    std::vector<double> red((size_t)(nf + nobj), 0.0);   // holders of every face, then the areas: one all-reduce
    for (int64_t q = 0; q < nf; ++q) {
        auto it = local.find(elem_gid[ord[q]]);
        if (it == local.end()) continue;
        el.push_back(it->second), fc.push_back(face[ord[q]]), ob.push_back(obj[ord[q]]), mine.push_back(ord[q]);
        red[ord[q]] = 1.0;
    }
    const int64_t nfl = f->nfl = (int64_t)el.size();
    std::vector<int64_t> byq(mine);
    std::sort(byq.begin(), byq.end());
    f->order.resize((size_t)nfl);
    for (int64_t r = 0; r < nfl; ++r) f->order[r] = std::lower_bound(byq.begin(), byq.end(), mine[r]) - byq.begin();
    // geometry on the host, from the coordinates the mesh holds
    std::vector<double> X[3];
    const double *Xp[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < dim; ++c) {
        X[c].resize((size_t)std::max<int64_t>(m->lvn, 1));
        NLG_HIP(hipMemcpyAsync(X[c].data(), m->d_x[c], sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToHost, st));
        Xp[c] = X[c].data();
    }
    NLG_HIP(hipStreamSynchronize(st));
    const int nfp = f->nfp;
    std::vector<double> nds((size_t)nfl * nfp * dim), met((size_t)nfl * nfp * dim * dim), xc((size_t)nfl * nfp * dim);
    NLG_CHECK(forces::geometry(dim, n, m->ops.z1.data(), m->E, Xp, nfl, el.data(), fc.data(), ob.data(), nobj, centre, nds.data(), met.data(),
                               xc.data(), red.data() + nf) == 0,
              "nlg_forces_create: the face geometry refused its arguments");
    {
        DevBuf<double> d;
        NLG_CHECK(nf + nobj < ((int64_t)1 << 31), "nlg_forces_create: nfaces = %lld is too many", (long long)nf);
        NLG_HIP(hipMalloc(&d.p, sizeof(double) * red.size()));
        NLG_HIP(hipMemcpyAsync(d.p, red.data(), sizeof(double) * red.size(), hipMemcpyHostToDevice, st));
        if (ctx->distributed()) NLG_TRY(allreduce_sum(ctx, d.p, (int)red.size()));
        NLG_HIP(hipMemcpyAsync(red.data(), d.p, sizeof(double) * red.size(), hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
    }
    for (int64_t q = 0; q < nf; ++q)
        NLG_CHECK(red[q] == 1.0, "nlg_forces_create: elem_gid[%lld] = %lld is an element %s", (long long)q, (long long)elem_gid[q],
                  red[q] == 0.0 ? "no rank holds" : "several ranks hold");
    f->area.assign(red.begin() + nf, red.end());
    // the faces of every object, ascending in the sorted order
    std::vector<int> ooff((size_t)nobj + 1, 0), oidx((size_t)nfl);
    for (int64_t r = 0; r < nfl; ++r) ooff[ob[r] + 1] += 1;
    for (int o = 0; o < nobj; ++o) ooff[o + 1] += ooff[o];
    {
        std::vector<int> pos(ooff.begin(), ooff.end() - 1);
        for (int64_t r = 0; r < nfl; ++r) oidx[pos[ob[r]]++] = (int)r;
    }
    std::vector<int> el32(el.begin(), el.end());
    std::vector<double> M((size_t)n * m->n2);
    forces::gl_to_gll(n, m->ops.z1.data(), m->n2, m->ops.z2.data(), M.data());
    NLG_TRY(upload(&f->d_elem, el32, st));
    NLG_TRY(upload(&f->d_face, fc, st));
    NLG_TRY(upload(&f->d_nds, nds, st));
    NLG_TRY(upload(&f->d_met, met, st));
    NLG_TRY(upload(&f->d_xc, xc, st));
    NLG_TRY(upload(&f->d_ooff, ooff, st));
    NLG_TRY(upload(&f->d_oidx, oidx, st));
    NLG_TRY(upload(&f->d_M, M, st));
    NLG_HIP(hipMalloc(&f->d_part, sizeof(double) * (size_t)std::max<int64_t>(kMaxLanes * nfl * f->nq, 1)));
    NLG_HIP(hipMalloc(&f->d_out, sizeof(double) * (size_t)(kMaxLanes * nobj * f->nq)));
    NLG_HIP(hipStreamSynchronize(st));   // the host vectors go out of scope
    return 0;
}

}  // namespace

namespace nlg {

int forces_sample(nlg_forces *f, int s, const ForceFields &F, double nu, double *out, int64_t ldo) {
    NLG_TRY(launch_faces(f, s, F, nu, nullptr));
    NLG_LAUNCH(k_wall_forces_reduce, dim3((unsigned)f->nobj, (unsigned)s), dim3(NTR), 0, f->mesh->ctx->stream, (const double *)f->d_part, f->nfl,
               f->nq, (const int *)f->d_ooff, (const int *)f->d_oidx, out, ldo);
    NLG_HIP(hipGetLastError());
    return 0;
}

}  // namespace nlg

extern "C" {

int nlg_forces_destroy(nlg_forces *f) {
    if (!f) return 0;
    NLG_CHECK(f->attached == 0, "nlg_forces_destroy: an nlg_dns samples these faces; nlg_dns_set_forces(dns, NULL) or nlg_dns_destroy first");
    hipDeviceSynchronize();
    (void)hipFree(f->d_elem);
    (void)hipFree(f->d_face);
    (void)hipFree(f->d_nds);
    (void)hipFree(f->d_met);
    (void)hipFree(f->d_xc);
    (void)hipFree(f->d_ooff);
    (void)hipFree(f->d_oidx);
    (void)hipFree(f->d_M);
    (void)hipFree(f->d_part);
    (void)hipFree(f->d_out);
    (void)hipFree(f->d_trac);
    delete f;
    return 0;
}

int nlg_forces_create(nlg_mesh *m, int nobj, int64_t nfaces, const int64_t *elem_gid, const int *face, const int *obj, const double *centre,
                      nlg_forces **out) {
    NLG_CHECK(m && elem_gid && face && obj && out, "nlg_forces_create: NULL argument");
    NLG_CHECK(nobj >= 1 && nobj <= (1 << 16), "nlg_forces_create: nobj = %d out of range (1..65536)", nobj);
    NLG_CHECK(nfaces >= 1 && nfaces <= (1 << 24), "nlg_forces_create: nfaces = %lld out of range (1..2^24)", (long long)nfaces);
    NLG_CHECK(m->n <= forces::kMaxN, "nlg_forces_create: lx1 = %d above %d", m->n, forces::kMaxN);
    nlg_forces *f = new nlg_forces();
    f->mesh = m;
    f->nobj = nobj;
    f->nfaces = nfaces;
    f->nq = forces::nquant(m->dim);
    f->nfp = forces::face_points(m->dim, m->n);
    const int rc = forces_build(f, elem_gid, face, obj, centre);
    if (rc) {
        nlg_forces_destroy(f);
        return rc;
    }
    *out = f;
    return 0;
}

int nlg_forces_info(const nlg_forces *f, double *area, int64_t *nfaces_local) {
    NLG_CHECK(f, "nlg_forces_info: NULL");
    if (area)
        for (int o = 0; o < f->nobj; ++o) area[o] = f->area[o];
    if (nfaces_local) *nfaces_local = f->nfl;
    return 0;
}

int nlg_forces_sample(nlg_forces *f, int s, const nlg_vec *const *vecs, double nu, double *out) {
    NLG_CHECK(f && vecs && out, "nlg_forces_sample: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_forces_sample: s = %d vectors unsupported (1..%d)", s, kMaxLanes);
    nlg_mesh *m = f->mesh;
    for (int v = 0; v < s; ++v) {
        NLG_CHECK(vecs[v] && vecs[v]->mesh == m, "nlg_forces_sample: vecs[%d] is NULL or lives on another mesh", v);
        NLG_CHECK(vecs[v]->nscal == vecs[0]->nscal, "nlg_forces_sample: vecs[%d] carries %d scalar(s), vecs[0] %d (nscal)", v, vecs[v]->nscal,
                  vecs[0]->nscal);
    }
    hipStream_t st = m->ctx->stream;
    const int64_t ldo = (int64_t)f->nobj * f->nq, cnt = s * ldo;
    NLG_TRY(forces_sample(f, s, fields_of(s, vecs), nu, f->d_out, ldo));
    if (m->ctx->distributed()) NLG_TRY(allreduce_sum(m->ctx, f->d_out, (int)cnt));
    NLG_HIP(hipMemcpyAsync(out, f->d_out, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

int nlg_forces_tractions(nlg_forces *f, const nlg_vec *vec, double nu, double *p, double *trac, double *nds) {
    NLG_CHECK(f && vec, "nlg_forces_tractions: NULL argument");
    nlg_mesh *m = f->mesh;
    NLG_CHECK(vec->mesh == m, "nlg_forces_tractions: vec lives on another mesh");
    if (f->nfl == 0) return 0;
    hipStream_t st = m->ctx->stream;
    const int dim = m->dim, w = 1 + 2 * dim;
    const size_t cnt = (size_t)f->nfl * f->nfp * w;
    if (!f->d_trac) NLG_HIP(hipMalloc(&f->d_trac, sizeof(double) * cnt));
    const nlg_vec *vs[1] = {vec};
    NLG_TRY(launch_faces(f, 1, fields_of(1, vs), nu, f->d_trac));
    NLG_HIP(hipGetLastError());
    std::vector<double> h(cnt);
    NLG_HIP(hipMemcpyAsync(h.data(), f->d_trac, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < f->nfl; ++r)
        for (int q = 0; q < f->nfp; ++q) {
            const double *src = h.data() + ((size_t)r * f->nfp + q) * w;
            const size_t dst = (size_t)f->order[r] * f->nfp + q;
            if (p) p[dst] = src[0];
            for (int i = 0; i < dim; ++i) {
                if (trac) trac[dst * dim + i] = src[1 + i];
                if (nds) nds[dst * dim + i] = src[1 + dim + i];
            }
        }
    return 0;
}

}  // extern "C"
