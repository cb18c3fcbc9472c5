// History points and the recurrence norm of a DNS run (nlg_probes_*, include/neklab_gpu.h; the reference's `call hpts()` and the
// `rnorm` of examples/cylinder/dns/Re180/1cyl.usr: userchk).  The points are located on the host once (probe_host.cpp); per sample the
// device evaluates the Lagrange interpolant of every field at every point in one launch.
#include "internal.h"
#include "probe_host.h"

using namespace nlg;

namespace {

constexpr int NT = 256;
constexpr int PPB = NT / 64;   // points per block: one wave each

struct SampleArgs {
    ProbeFields F;
    int64_t npts;
    const int *elem;
    const double *w1, *w2;
    int dim, n, n2;
    double *out;
};

// One wave per (point, lane): the element's n^dim values of every field times w_r[i] w_s[j] w_t[k], summed by the fixed shuffle tree.
__global__ __launch_bounds__(NT) void k_probe_sample(SampleArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t pt = (int64_t)blockIdx.x * PPB + (threadIdx.x >> 6);
    if (pt >= A.npts) return;
    const int e = A.elem[pt];
    if (e < 0) return;   // another rank's point: its slot stays 0
    const int v = blockIdx.y, dim = A.dim;
    for (int f = 0; f < A.F.nf; ++f) {
        const bool m2 = f == A.F.mesh2;
        const int n = m2 ? A.n2 : A.n;
        const int np = dim == 3 ? n * n * n : n * n;
        const double *__restrict__ w = (m2 ? A.w2 : A.w1) + pt * dim * n;
        const double *__restrict__ u = A.F.f[v][f] + (int64_t)e * np;
        double acc = 0.0;
        for (int q = lane; q < np; q += 64) {
            const int i = q % n, j = (q / n) % n;
            double wt = w[i] * w[n + j];
            if (dim == 3) wt *= w[2 * n + q / (n * n)];
            acc += u[q] * wt;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) A.out[((int64_t)v * A.npts + pt) * A.F.nf + f] = acc;
    }
}

struct RecurArgs {
    const double *u[4], *ref[4];
    int nf;
    int64_t n;
    const double *bm1;
    double *part;
};

// part[block] = the block's share of sum_c sum_i bm1_i (u_c,i - ref_c,i)^2; the grid is fixed (kRecurBlocks)
__global__ __launch_bounds__(NT) void k_recur_partial(RecurArgs A) {
    __shared__ double sm[NT / 64];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * NT) {
        double s = 0.0;
        for (int c = 0; c < A.nf; ++c) {
            const double d = A.u[c][i] - A.ref[c][i];
            s += d * d;
        }
        acc += A.bm1[i] * s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < NT / 64; ++w) t += sm[w];
        A.part[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(NT) void k_recur_final(const double *__restrict__ part, int nblk, double *__restrict__ out) {
    __shared__ double sm[NT / 64];
    double t = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NT) t += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int w = 0; w < NT / 64; ++w) a += sm[w];
        out[0] = a;
    }
}

template <typename T>
int upload(T **dst, const std::vector<T> &src, hipStream_t st) {
    NLG_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(src.size(), 1)));
    if (!src.empty()) NLG_HIP(hipMemcpyAsync(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, st));
    return 0;
}

// locate, settle the ownership across the ranks, build and upload the weights
int probes_build(nlg_probes *p, const double *xyz, double tol_r) {
    nlg_mesh *m = p->mesh;
    nlg_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int dim = m->dim, n = m->n, n2 = m->n2;
    const int64_t npts = p->npts;
    std::vector<double> X[3];
    const double *Xp[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < dim; ++c) {
        X[c].resize((size_t)std::max<int64_t>(m->lvn, 1));
        NLG_HIP(hipMemcpyAsync(X[c].data(), m->d_x[c], sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToHost, st));
        Xp[c] = X[c].data();
    }
    NLG_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> elem((size_t)npts);
    std::vector<int> status((size_t)npts);
    std::vector<double> key((size_t)npts);
    p->rst.assign((size_t)npts * dim, 0.0);
    p->dist.assign((size_t)npts, 0.0);
    NLG_TRY(probe::locate(dim, n, m->ops.z1.data(), m->E, Xp, m->h_lglel.data(), npts, xyz, tol_r, elem.data(), p->rst.data(), status.data(),
                          p->dist.data(), key.data()));
    // the smallest key over all ranks wins: one all-reduce (max of -key) settles who owns a point on a partition interface
    const int64_t nr = npts * (dim + 1);
    DevBuf<double> red;
    NLG_HIP(hipMalloc(&red.p, sizeof(double) * (size_t)std::max(npts, nr)));
    std::vector<double> h((size_t)npts);
    for (int64_t q = 0; q < npts; ++q) h[q] = key[q] < 0.0 ? -1e300 : -key[q];
    NLG_HIP(hipMemcpyAsync(red.p, h.data(), sizeof(double) * (size_t)npts, hipMemcpyHostToDevice, st));
    NLG_TRY(allreduce_max(ctx, red.p, (int)npts));
    NLG_HIP(hipMemcpyAsync(h.data(), red.p, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    const double kStatus1 = 1099511627776.0;   // 2^40, as in probe::locate
    p->status.assign((size_t)npts, 2);
    p->elem_global.assign((size_t)npts, -1);
    p->owned.assign((size_t)npts, 0);
    for (int64_t q = 0; q < npts; ++q) {
        const double win = -h[q];
        NLG_CHECK(win < 1e299, "nlg_probes_create: point %lld (%g, %g%s) lies in no element (status 2); pass the points through nlg_probe_locate and drop those",
                  (long long)q, xyz[q * dim], xyz[q * dim + 1], dim == 3 ? ", ..." : "");
        p->status[q] = win >= kStatus1 ? 1 : 0;
        p->elem_global[q] = (int64_t)(win - (win >= kStatus1 ? kStatus1 : 0.0));
        p->owned[q] = key[q] == win;
    }
    // reference coordinates and distance of the winner, on every rank
    std::vector<double> hr((size_t)nr, 0.0);
    for (int64_t q = 0; q < npts; ++q)
        if (p->owned[q]) {
            for (int d = 0; d < dim; ++d) hr[q * (dim + 1) + d] = p->rst[q * dim + d];
            hr[q * (dim + 1) + dim] = p->dist[q];
        }
    NLG_HIP(hipMemcpyAsync(red.p, hr.data(), sizeof(double) * (size_t)nr, hipMemcpyHostToDevice, st));
    NLG_TRY(allreduce_sum(ctx, red.p, (int)nr));
    NLG_HIP(hipMemcpyAsync(hr.data(), red.p, sizeof(double) * (size_t)nr, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    for (int64_t q = 0; q < npts; ++q) {
        for (int d = 0; d < dim; ++d) p->rst[q * dim + d] = hr[q * (dim + 1) + d];
        p->dist[q] = hr[q * (dim + 1) + dim];
    }
    // the weights in barycentric form, on the mesh's own nodes
    double bw1[probe::kMaxN], bw2[probe::kMaxN];
    probe::bary_weights(n, m->ops.z1.data(), bw1);
    probe::bary_weights(n2, m->ops.z2.data(), bw2);
    std::vector<double> w1((size_t)npts * dim * n, 0.0), w2((size_t)npts * dim * n2, 0.0);
    std::vector<int> el((size_t)npts, -1);
    for (int64_t q = 0; q < npts; ++q) {
        if (!p->owned[q]) continue;
        el[q] = (int)elem[q];
        for (int d = 0; d < dim; ++d) {
            probe::lagrange(n, m->ops.z1.data(), bw1, p->rst[q * dim + d], &w1[(q * dim + d) * n], nullptr);
            probe::lagrange(n2, m->ops.z2.data(), bw2, p->rst[q * dim + d], &w2[(q * dim + d) * n2], nullptr);
        }
    }
    NLG_TRY(upload(&p->d_elem, el, st));
    NLG_TRY(upload(&p->d_w1, w1, st));
    NLG_TRY(upload(&p->d_w2, w2, st));
    NLG_HIP(hipMalloc(&p->d_out, sizeof(double) * (size_t)(kMaxLanes * npts * kMaxProbeFields)));
    NLG_HIP(hipStreamSynchronize(st));   // the host vectors go out of scope
    return 0;
}

}  // namespace

namespace nlg {

int probes_sample(const nlg_probes *p, int s, const ProbeFields &F, double *out) {
    nlg_mesh *m = p->mesh;
    SampleArgs A;
    A.F = F;
    A.npts = p->npts;
    A.elem = p->d_elem;
    A.w1 = p->d_w1, A.w2 = p->d_w2;
    A.dim = m->dim, A.n = m->n, A.n2 = m->n2;
    A.out = out;
    NLG_LAUNCH(k_probe_sample, dim3((unsigned)((p->npts + PPB - 1) / PPB), (unsigned)s), dim3(NT), 0, m->ctx->stream, A);
    NLG_HIP(hipGetLastError());
    return 0;
}

int recur_dist2(nlg_mesh *m, int nf, const double *const *u, const double *const *ref, double *part, double *out) {
    RecurArgs A;
    memset(&A, 0, sizeof(A));
    for (int c = 0; c < nf; ++c) A.u[c] = u[c], A.ref[c] = ref[c];
    A.nf = nf;
    A.n = m->lvn;
    A.bm1 = m->d_bm1;
    A.part = part;
    hipStream_t st = m->ctx->stream;
    NLG_LAUNCH(k_recur_partial, dim3(kRecurBlocks), dim3(NT), 0, st, A);
    NLG_LAUNCH(k_recur_final, dim3(1), dim3(NT), 0, st, (const double *)part, kRecurBlocks, out);
    NLG_HIP(hipGetLastError());
    return 0;
}

}  // namespace nlg

extern "C" {

int nlg_probes_destroy(nlg_probes *p) {
    if (!p) return 0;
    NLG_CHECK(p->attached == 0, "nlg_probes_destroy: an nlg_dns samples these points; nlg_dns_set_probes(dns, NULL) or nlg_dns_destroy first");
    hipDeviceSynchronize();
    (void)hipFree(p->d_elem);
    (void)hipFree(p->d_w1);
    (void)hipFree(p->d_w2);
    (void)hipFree(p->d_out);
    delete p;
    return 0;
}

int nlg_probes_create(nlg_mesh *m, int64_t npts, const double *xyz, double tol_r, nlg_probes **out) {
    NLG_CHECK(m && xyz && out, "nlg_probes_create: NULL argument");
    NLG_CHECK(npts >= 1 && npts <= (1 << 24), "nlg_probes_create: %lld points out of range (1..2^24)", (long long)npts);
    NLG_CHECK(tol_r >= 0.0, "nlg_probes_create: tol_r must not be negative");
    NLG_CHECK(m->n <= probe::kMaxN, "nlg_probes_create: lx1 = %d above %d", m->n, probe::kMaxN);
    nlg_probes *p = new nlg_probes();
    p->mesh = m;
    p->npts = npts;
    const int rc = probes_build(p, xyz, tol_r);
    if (rc) {
        nlg_probes_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

int nlg_probes_status(const nlg_probes *p, int *status, int64_t *elem_global, double *rst, double *dist) {
    NLG_CHECK(p, "nlg_probes_status: NULL");
    const int dim = p->mesh->dim;
    for (int64_t q = 0; q < p->npts; ++q) {
        if (status) status[q] = p->status[q];
        if (elem_global) elem_global[q] = p->elem_global[q];
        if (dist) dist[q] = p->dist[q];
        if (rst)
            for (int d = 0; d < dim; ++d) rst[q * dim + d] = p->rst[q * dim + d];
    }
    return 0;
}

int nlg_probes_sample(nlg_probes *p, int s, const nlg_vec *const *vecs, double *out) {
    NLG_CHECK(p && vecs && out, "nlg_probes_sample: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_probes_sample: %d vectors unsupported (1..%d)", s, kMaxLanes);
    nlg_mesh *m = p->mesh;
    const int dim = m->dim;
    for (int v = 0; v < s; ++v)
        NLG_CHECK(vecs[v] && vecs[v]->mesh == m && vecs[v]->nscal == vecs[0]->nscal, "nlg_probes_sample: vector %d NULL, on another mesh or of another shape", v);
    const bool heat = vecs[0]->nscal >= 1;
    ProbeFields F;
    memset(&F, 0, sizeof(F));
    F.nf = dim + 1 + (heat ? 1 : 0);
    F.mesh2 = dim;
    for (int v = 0; v < s; ++v) {
        for (int c = 0; c < dim; ++c) F.f[v][c] = vecs[v]->vel(c);
        F.f[v][dim] = vecs[v]->pr();
        if (heat) F.f[v][dim + 1] = vecs[v]->theta(0);
    }
    hipStream_t st = m->ctx->stream;
    const int64_t cnt = (int64_t)s * p->npts * F.nf;
    NLG_HIP(hipMemsetAsync(p->d_out, 0, sizeof(double) * (size_t)cnt, st));
    NLG_TRY(probes_sample(p, s, F, p->d_out));
    if (m->ctx->distributed()) NLG_TRY(allreduce_sum(m->ctx, p->d_out, (int)cnt));   // every point has one owner: the others hold 0
    NLG_HIP(hipMemcpyAsync(out, p->d_out, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
