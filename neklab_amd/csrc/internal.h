// Internal declarations of libneklab_gpu (gfx950 only). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "fg_slot.h"
#include "neklab_gpu.h"

namespace nlg {

void set_error(const char *fmt, ...);

#define NLG_HIP(call)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            nlg::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

#define NLG_NCCL(call)                                                                            \
    do {                                                                                          \
        ncclResult_t r_ = (call);                                                                 \
        if (r_ != ncclSuccess) {                                                                  \
            nlg::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

#define NLG_CHECK(cond, ...)             \
    do {                                 \
        if (!(cond)) {                   \
            nlg::set_error(__VA_ARGS__); \
            return 1;                    \
        }                                \
    } while (0)

#define NLG_TRY(call)           \
    do {                        \
        int rc_ = (call);       \
        if (rc_) return rc_;    \
    } while (0)

// every kernel launch of the library goes through this macro: the count is what bench.py reports as launches per step
extern int64_t g_launches, g_collectives;
#define NLG_LAUNCH(...)                     \
    do {                                    \
        ++nlg::g_launches;                  \
        hipLaunchKernelGGL(__VA_ARGS__);    \
    } while (0)

constexpr int kMaxLanes = 4;            // vectors advanced together by the block stepper
constexpr int kMaxBlocksReduce = 1024;  // fixed first-stage grid => run-to-run deterministic sums
constexpr int kAlign = 32;              // field starts aligned to 32 doubles (256 B)

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

template <typename T = double>
struct DevBuf {   // a device temporary, released on every path out of its scope
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(p); }
};

}  // namespace nlg

// kernel classes that can be timed with HIP events on the launch stream (bench.py roofline leg)
enum { P_AXHELM = 0, P_GS, P_OPGRADT, P_OPDIV, P_COLMUL, P_BLOCKDOT, P_BLOCKAXPY, P_CGVEC, P_CONV, P_VECOPS, P_PPREC, P_AXPYDOT, P_CGUPDATE, P_COUNT };

struct nlg_prof_slot {
    std::vector<hipEvent_t> ev;   // pairs (begin, end)
    int used = 0;
    double total_ms = 0.0;
    int64_t count = 0;
};

namespace nlg {
struct nlg_shm;   // host-staged validation transport (shm_transport.hip)
}

struct nlg_ctx {
    int prof_on = 0;
    int prof_stride = 1;                      // time every prof_stride-th launch of an enabled class (nlg_prof_sample)
    int64_t prof_seq[16] = {};
    nlg_prof_slot prof[P_COUNT];
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;            // side stream: coarse-grid branch of the pressure preconditioner
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ncclComm_t comm = nullptr;
    nlg::nlg_shm *shm = nullptr;              // set only by nlg_ctx_comm_init_shm (several test ranks on one GPU)
    bool distributed() const { return comm != nullptr || shm != nullptr; }
    int rank = 0, nranks = 1;
    // reduction workspace
    double *d_partial = nullptr;   // [kMaxVecReduce * kMaxBlocksReduce]
    double *d_scalars = nullptr;   // small device scalars (results of reductions)
    double *h_scalars = nullptr;   // pinned host mirror
    int n_scalars = 0;
    int max_red_vec = 0;
};

// Small dense operators of the discretisation, host copies (device copies live in nlg_mesh::d_ops)
struct nlg_ops1d {
    int n = 0, n2 = 0, nd = 0;
    std::vector<double> z1, w1, z2, w2, zd, wd;
    std::vector<double> D;     // n  x n   d/dr on GLL
    std::vector<double> I12;   // n2 x n   GLL -> GL(n2)
    std::vector<double> D12;   // n2 x n
    std::vector<double> Jd;    // nd x n   GLL -> GL(nd)
    std::vector<double> DJd;   // nd x n
    std::vector<double> rdr;   // n  inverse reference spacing (CFL)
};

// "Slab-permuted" slot of point (a, j, k) (historically "xp", x-planes first): every k-slab of an element stays one dense run
// of N N doubles, but inside the slab the points are permuted so that the element-boundary points are contiguous:
//   [ a = 0 row (j = 0..N-1) | a = N-1 row | j = 0 row (a = 1..N-2) | j = N-1 row | interior ]
// and, at N = 8, two interior points pad each j-row so that it sits inside one 64-byte sector.  A kernel whose lanes are
// (a, j) columns reads a slab as ONE coalesced run exactly as in the natural layout (the permutation only decides which
// lane gets which word), while the copies of a shared x-face -- one 8-byte word per 64-byte row in the natural layout --
// become sector-aligned runs of N, y-faces runs of N-2 inside one sector, z-faces whole slabs.  Used for the vectors of
// the velocity PCG (3-D), whose gather-scatter moved 3.2 times its algorithmic bytes in the natural layout.
// Measured on the way here (10^4 elements, lx1 = 8, ms per step): natural gs 7.09 / operator 6.07; x-faces as two separate
// N x N planes: gs 6.2 / operator 6.7 (half-line rows); both x-rows of a slab in one line, rest natural: 6.07 / 6.32.
inline void sp_slab_table(int N, int *tab /* [N*N], index a + N*j */) {
    std::vector<int> order;   // slab positions (a + N*j) in storage order
    std::vector<char> used((size_t)N * N, 0);
    auto put = [&](int a, int j) {
        order.push_back(a + N * j);
        used[a + N * j] = 1;
    };
    for (int j = 0; j < N; ++j) put(0, j);
    for (int j = 0; j < N; ++j) put(N - 1, j);
    auto filler = [&](int count) {
        for (int j = 1; j < N - 1 && count > 0; ++j)
            for (int a = 1; a < N - 1 && count > 0; ++a)
                if (!used[a + N * j]) {
                    put(a, j);
                    --count;
                }
    };
    for (int a = 1; a < N - 1; ++a) put(a, 0);
    if (N == 8) filler(2);
    for (int a = 1; a < N - 1; ++a) put(a, N - 1);
    if (N == 8) filler(2);
    filler(N * N);
    for (int q = 0; q < N * N; ++q) tab[order[q]] = q;
}
inline int xp_slot(int N, int a, int j, int k) {
    static thread_local int cachedN = 0;
    static thread_local std::vector<int> tab;
    if (cachedN != N) {
        tab.assign((size_t)N * N, 0);
        sp_slab_table(N, tab.data());
        cachedN = N;
    }
    return N * N * k + tab[a + N * j];
}

struct nlg_gs_tab {   // one table of groups as k_gs reads it: pairs first, then quads, then the rest (CSR)
    int64_t ngroups = 0, npairs = 0, nquads = 0;
    int *d_off = nullptr, *d_idx = nullptr;
};
struct nlg_gs {
    // groups of local dofs that share a global label (only groups of size >= 2 are stored)
    int64_t ngroups = 0;
    int64_t nshared = 0;
    int64_t npairs = 0;         // the first npairs groups have exactly two copies (same count in both layouts)
    int64_t nquads = 0;         // the next nquads groups have exactly four
    int *d_offsets = nullptr;   // [ngroups + 1]
    int *d_indices = nullptr;   // [nshared] local dof index
    // the same groups in the face-grouped element layout used for the intermediate fields of the consistent
    // Poisson operator (3-D): element-boundary points first, face by face, so that the copies of a shared face
    // are contiguous runs instead of stride-n points
    int *d_offsets_fg = nullptr;
    int *d_indices_fg = nullptr;
    // ... and in the x-planes-first layout of the velocity PCG (3-D)
    int *d_offsets_xp = nullptr;
    int *d_indices_xp = nullptr;
    // several ranks: the groups split into those holding a dof that another rank shares (summed first, so that the halo
    // exchange can start) and all others (summed while the exchange is under way); one pair of tables per layout
    bool split = false;
    nlg_gs_tab tab_halo[3], tab_rest[3];
    std::vector<std::vector<int>> h_groups;   // the groups in natural indices; kept only until halo_setup has split them
};
enum { LAYOUT_NAT = 0, LAYOUT_FG = 1, LAYOUT_XP = 2 };

struct nlg_halo {
    bool active = false;
    std::vector<int> neigh;          // neighbour ranks (ascending)
    std::vector<int64_t> noff, ncnt; // offset / count of each neighbour's shared labels in the packed buffers
    int64_t ntot = 0, nlab = 0;
    int *d_send_idx = nullptr;       // [ntot] representative local dof per (neighbour, label)
    int *d_roff = nullptr, *d_rpos = nullptr;   // per distinct shared label: positions in the recv buffer
    int *d_coff = nullptr, *d_cidx = nullptr;   // per distinct shared label: all local copies
    int *d_send_idx_fg = nullptr, *d_cidx_fg = nullptr;   // d_send_idx / d_cidx for the face-grouped element layout
    int *d_send_idx_xp = nullptr, *d_cidx_xp = nullptr;   // ... and for the x-planes-first layout
    double *d_send = nullptr, *d_recv = nullptr;
    std::vector<int> h_cidx;         // host copy of d_cidx: every local dof that another rank shares
    bool overlap = false;            // send / receive on the side stream while the interior groups are summed (NLG_HALO_OVERLAP)
    hipEvent_t ev_packed = nullptr, ev_recv = nullptr;
};

// two-level preconditioner of the pressure operator (pprec.hip)
struct nlg_pprec {
    bool ready = false;
    int na = 0;                                  // aggregates
    int nvert = 0, ncorner = 0;                  // coarse dofs: element vertices (trilinear coarse space), 2^dim per element
    int *d_vg = nullptr;                         // [E][ncorner] vertex id of every element corner
    int *d_v2e_p = nullptr, *d_v2e_i = nullptr;  // vertex -> incident (element*ncorner + corner) entries, CSR
    double *d_tq = nullptr;                      // [E][ncorner] element-local restriction
    double hat1[16] = {};                        // (1 + z2)/2 at the GL points: the 1-D hat function of the upper corner
    double *d_S = nullptr, *d_invden = nullptr;  // FDM: [E][3][n2*n2] eigenvector matrices, [E][n2^dim] 1/(sum of eigenvalues)
    double *d_dinv = nullptr;                    // 1 / diag(A_c)
    // overlapping variant: extended 1-D eigen-decompositions [E][3][n*n], eigenvalues [E][3][n], the velocity-shaped
    // exchange arrays and the zero-denominator threshold.  W = the extended grids (natural layout) the restriction writes and
    // the local solves read, Wr = the return values at the face slots (3-D: face-grouped layout, 2-D: natural layout) the
    // local solves write and the finish reads; each ghost value goes straight to its consumer
    bool overlap = false;
    int *d_pin = nullptr;                        // [E][2 dim n2^(dim-1)] index in W the layer value next to an element face point goes to, -1 = none
    int *d_pret = nullptr;                       // [E][2 dim n2^(dim-1)] index in Wr the solve at a ghost point goes to, -1 = none (2-D: = d_pin)
    double *d_Sx = nullptr, *d_lamx = nullptr, *d_W = nullptr, *d_Wr = nullptr, *d_wq = nullptr;   // d_wq: count^-1/2 weights [E][n2^dim]
    double thrx = 0.0;
    int *d_agg = nullptr, *d_ap = nullptr, *d_am = nullptr;
    double *d_Ainv = nullptr;                    // dense inverse on the aggregates: this rank's rows, [na][ncols]
    float *d_Ainv32 = nullptr;                   // several ranks: the rows in single precision instead of d_Ainv
    int na_max = 0, ncols = 0;                   // several ranks: ncols = nranks * na_max columns (global aggregate level)
    double *d_rag = nullptr;                     // [ncols] aggregate residuals of all ranks (all-gather of d_ra)
    double *d_rc = nullptr, *d_x = nullptr, *d_ra = nullptr, *d_xa = nullptr;
    // lanes of a block step: `lanes_cap` copies of W, Wr, tq, rc / x, ra, xa at these strides (pprec_reserve_lanes)
    int lanes_cap = 1;
    int64_t lW = 0, lt = 0, lv = 0, la = 0, la_x = 0;
};

struct nlg_mesh {
    nlg_pprec pprec;
    nlg_halo halo;
    nlg_ctx *ctx = nullptr;
    int dim = 3, n = 8, n2 = 6, nd = 12;
    int64_t E = 0;
    int np1 = 0, np2 = 0, npd = 0;      // points per element on the three meshes
    int64_t lvn = 0, lpn = 0, lvs = 0, lps = 0, lfn = 0;  // lvs/lps: padded field strides
    int has_outflow = 0;
    nlg_ops1d ops;
    // device copies of the 1-D operators, row-major; transposes stored too
    double *d_D = nullptr, *d_Dt = nullptr, *d_I12 = nullptr, *d_I12t = nullptr, *d_D12 = nullptr, *d_D12t = nullptr;
    double *d_Jd = nullptr, *d_Jdt = nullptr, *d_DJd = nullptr, *d_DJdt = nullptr, *d_rdr = nullptr;
    double *d_w1 = nullptr, *d_w2 = nullptr, *d_wd = nullptr;
    // geometry (velocity mesh), each lvn
    double *d_x[3] = {nullptr, nullptr, nullptr};
    double *d_rst[9] = {};     // rst[j*dim+i] = J * dr_j/dx_i
    double *d_jac = nullptr, *d_bm1 = nullptr, *d_binvm1 = nullptr, *d_vmult = nullptr;
    double *d_G[6] = {};       // 3-D: 11,12,13,22,23,33 ; 2-D: 11,12,22
    double *d_mask[3] = {nullptr, nullptr, nullptr};
    double *d_tmask = nullptr;
    double *d_mbinv[3] = {nullptr, nullptr, nullptr};   // mask_i * binvm1 (fused opbinv weight)
    double *d_mbinv_fg[3] = {nullptr, nullptr, nullptr};   // the same in the face-grouped layout
    double *d_binv_fg = nullptr;                           // binvm1 alone, face-grouped, and ...
    unsigned char *d_maskb_fg = nullptr;                   // ... one byte per point, bit i = mask_i: the three weights of k_opdiv3n in 8.5 bytes per point
    // pressure mesh
    double *d_rst2w[9] = {};   // each lpn
    double *d_bm2 = nullptr, *d_bm2inv = nullptr;
    // fine mesh
    double *d_rstdw[9] = {};   // each lfn
    int64_t *d_lglel = nullptr;
    std::vector<int64_t> h_lglel;
    std::vector<int> h_slot;   // natural point -> face-grouped slot inside an element (3-D)
    std::vector<int> h_slot_xp;   // natural point -> x-planes-first slot (3-D)
    int *d_slot_xp = nullptr;
    int *d_slot_fg = nullptr;   // device copy of h_slot (lx1 > 8 pressure kernels read it instead of computing the slot)
    double *d_vmult_xp = nullptr;
    double *d_wlanes = nullptr;   // [kMaxLanes][3][lvs] intermediate fields of the pressure operator of a block step (lazy)
    nlg_gs gs;
    double volvm1 = 0, volvm2 = 0;
    int64_t lpn_global = 0;   // global pressure dof count (ortho)
    // scratch fields
    std::vector<double *> scratch1, scratchd, scratch2;   // velocity-mesh / fine-mesh / pressure-mesh scratch
    std::map<std::string, const double *> named;          // for nlg_mesh_get
    std::map<std::string, int64_t> named_len;
};

struct nlg_vec {
    nlg_mesh *mesh = nullptr;
    int nscal = 0, lorder = 3;
    int ncomp = 0;             // dim + nscal : fields in the inner product
    int64_t main_len = 0;      // ncomp*lvs + lps
    int64_t total_len = 0;     // main_len * lorder
    double *d = nullptr;
    bool owns = true;
    int nrst = 0;
    // field pointers
    double *vel(int i, int irst = 0) const { return d + irst * main_len + (int64_t)i * mesh->lvs; }
    double *theta(int m, int irst = 0) const { return d + irst * main_len + (int64_t)(mesh->dim + m) * mesh->lvs; }
    double *pr(int irst = 0) const { return d + irst * main_len + (int64_t)ncomp * mesh->lvs; }
};

struct nlg_basis {
    nlg_mesh *mesh = nullptr;
    int nvec = 0, nscal = 0, lorder = 3;
    int64_t stride = 0;        // doubles between consecutive vectors
    double *d = nullptr;
    std::vector<nlg_vec *> views;
    // The one coefficient workspace of every orthogonalisation on this basis, for up to kMaxLanes vectors at once (lanes of a batch,
    // columns of a block): [ first-pass coefficients, s * k <= 4 nvec, |w_l|^2 right behind them | second pass | Gram | T ].  One
    // vector: coefficients at 0 and |w|^2 at k, so that a step's read-back is one copy.
    double *d_h = nullptr;
    static size_t h_len(int nvec) { return (size_t)8 * nvec + 40; }
    double *h1() const { return d_h; }                                // [s][k] (batch) or [k][s] (block)
    double *hnorm(int s, int k) const { return d_h + (size_t)s * k; } // [s] squared norms before scaling
    double *h2() const { return d_h + (size_t)4 * nvec + 8; }         // second-pass coefficients, laid out as the first
    double *gram() const { return d_h + (size_t)8 * nvec + 8; }       // [4][4] Gram matrix of the new columns of a block
    double *tmat() const { return gram() + 16; }                      // [4][4] its inverse Cholesky factor
    int last_block_rank = 0;   // columns kept by the last nlg_basis_block_cgs2 (< s: dependent columns were deflated)
};

// History points (probe.hip): per located point the local element and the 1-D Lagrange weights at its reference coordinates, on the
// GLL nodes (velocity mesh) and on the Gauss nodes (pressure mesh).  A point another rank owns has elem -1 and is skipped.
struct nlg_probes {
    nlg_mesh *mesh = nullptr;
    int64_t npts = 0;
    int attached = 0;                     // nlg_dns objects that sample these points (nlg_probes_destroy refuses while > 0)
    std::vector<int> status;              // global: of the winning element, the same on every rank
    std::vector<int64_t> elem_global;
    std::vector<double> rst, dist;        // [npts][dim], [npts]
    std::vector<char> owned;
    int *d_elem = nullptr;                // [npts] local element, -1 = not this rank's
    double *d_w1 = nullptr, *d_w2 = nullptr;   // [npts][dim][n], [npts][dim][n2]
    double *d_out = nullptr;              // [kMaxLanes][npts][kMaxProbeFields]: the result of nlg_probes_sample before it goes to the host
};

// Wall forces (forces.hip): the listed faces this rank holds, sorted by global element id, then face -- the order every sum runs in --
// with their precomputed geometry (forces_host.h) and, per object, the positions of its faces in that order.
struct nlg_forces {
    nlg_mesh *mesh = nullptr;
    int nobj = 0, nq = 0, nfp = 0;        // objects, quantities per object (Fp, Fv, Tp, Tv, Q), points per face
    int64_t nfaces = 0, nfl = 0;          // faces of the global list, faces on this rank's elements
    int attached = 0;                     // nlg_dns objects that sample these faces (nlg_forces_destroy refuses while > 0)
    std::vector<double> area;             // [nobj], global
    std::vector<int64_t> order;           // [nfl] sorted position -> position among this rank's faces in creation order
    int *d_elem = nullptr, *d_face = nullptr;                        // [nfl] local element, face
    double *d_nds = nullptr, *d_met = nullptr, *d_xc = nullptr;      // [nfl][nfp][dim], [dim * dim], [dim]
    int *d_ooff = nullptr, *d_oidx = nullptr;                        // [nobj + 1], [nfl]: the faces of every object, ascending
    double *d_M = nullptr;                // [n][n2] Gauss points -> GLL points
    double *d_part = nullptr;             // [kMaxLanes][nfl][nq] the faces' partial sums
    double *d_out = nullptr;              // [kMaxLanes][nobj][nq] the result of nlg_forces_sample before it goes to the host
    double *d_trac = nullptr;             // [nfl][nfp][1 + 2 dim] p, traction, N of nlg_forces_tractions (lazy)
};

namespace nlg {

// ---- forces.hip ----
// the fields of s lanes: velocity, pressure (Gauss mesh), temperature (null: none)
struct ForceFields {
    const double *u[kMaxLanes][3], *p[kMaxLanes], *th[kMaxLanes];
};
// out[v * ldo + o * nq + k] = this rank's share of quantity k of object o for the lanes v < s: two launches, nothing waits
int forces_sample(nlg_forces *f, int s, const ForceFields &F, double nu, double *out, int64_t ldo);

// ---- probe.hip ----
constexpr int kMaxProbeFields = 5;   // velocity (dim), pressure, temperature
constexpr int kRecurBlocks = 512;    // fixed first-stage grid of the recurrence norm
// the fields of s lanes, lane 0's pointers and every other lane's: f[v][q], q < nf; field `mesh2` (-1: none) lives on the pressure mesh
struct ProbeFields {
    const double *f[kMaxLanes][kMaxProbeFields];
    int nf, mesh2;
};
// out[v][point][field] for the lanes v < s, one launch; points of other ranks are not written
int probes_sample(const nlg_probes *p, int s, const ProbeFields &F, double *out);
// *out = sum_c sum_i bm1_i (u_c,i - ref_c,i)^2 over nf <= 4 velocity-mesh fields of this rank, two launches; part: [kRecurBlocks]
int recur_dist2(nlg_mesh *m, int nf, const double *const *u, const double *const *ref, double *part, double *out);

// ---- ctx.hip: optional per-kernel-class event timing ----
void prof_begin(nlg_ctx *ctx, int id);
void prof_end(nlg_ctx *ctx, int id);
int prof_flush(nlg_ctx *ctx);
// is this launch of class `id` to be timed?  Enabled classes are sampled: every prof_stride-th launch gets its pair of events
// (an event pair around a 50-us kernel costs ~12 us of stream time: timing every launch of the dominant class took 2 % off the
// benchmark it was measuring)
inline bool prof_want(nlg_ctx *c, int id) {
    if (!(c->prof_on & (1 << id))) return false;
    return (c->prof_seq[id]++ % c->prof_stride) == 0;
}
struct ProfScope {
    nlg_ctx *c;
    int id;
    bool on;
    ProfScope(nlg_ctx *ctx, int i) : c(ctx), id(i), on(prof_want(ctx, i)) {
        if (on) prof_begin(c, id);
    }
    ~ProfScope() {
        if (on) prof_end(c, id);
    }
};

// ---- vec.hip ----
int reduce_ws_reserve(nlg_ctx *ctx, int nvec);
// weighted dot over the inner-product part, result left on device at ctx->d_scalars[slot]; allreduced
int dev_dot(const nlg_vec *a, const nlg_vec *b, int slot);
// border of the periodic-orbit Jacobian in one pass: w <- w - v + t fT (main block), <f0, v> at ctx->d_scalars[slot]; allreduced
int upo_border_dev(nlg_vec *w, const nlg_vec *v, const nlg_vec *fT, const nlg_vec *f0, double t, int slot);
int scalars_to_host(nlg_ctx *ctx, int first, int count, double *out);   // syncs the stream
int vec_copy_main(nlg_vec *dst, const nlg_vec *src);   // dst <- 0, then velocity and pressure of src's main block
int allreduce_sum(nlg_ctx *ctx, double *d_buf, int count);
int allreduce_max(nlg_ctx *ctx, double *d_buf, int count);
int allgather_f64(nlg_ctx *ctx, const double *d_in, double *d_out, int64_t count);   // count doubles per rank
int shm_allreduce(nlg_ctx *ctx, double *d_buf, int count, bool is_max);
int shm_allgather_i64(nlg_ctx *ctx, const int64_t *d_in, int64_t *d_out, int64_t count);
int shm_exchange(nlg_ctx *ctx, const nlg_halo &h, int nf, hipStream_t st);   // st: the stream the staging copies are ordered on
void shm_close(nlg_ctx *ctx);

// CGS2 + norm + scale of s vectors, w[l] against columns 0 .. k-1 of its own basis b[l], one launch per stage for all lanes; one lane
// takes the fused subtract-and-project sweep from k = 24 (nlg_basis_cgs2, nlg_basis_cgs2_batch).  ONE read-back from b[0]'s
// workspace: lane l's k coefficients to h[l * hstride + 0:k], its norm before scaling to beta[l * bstride]
int basis_cgs2_host(int s, nlg_basis *const *b, int k, nlg_vec *const *w, double *h, int64_t hstride, double *beta, int64_t bstride);

// ---- lns.hip ----
int linop_proj_lanes(const nlg_linop *op);   // wavenumber lanes of the operator (nlg_linop_set_projection_lanes), 0 = none
int vel_mask_bytes(nlg_mesh *m, bool xp, unsigned char *out);   // the mask bytes of the velocity PCG (pcmb of sem_axhelm): bit c = mask_c != 0; xp: slab-permuted

// ---- pprec.hip ----
int pprec_setup(nlg_mesh *m, const nlg_mesh_desc *d);
// PCG update fused into the first kernel of the preconditioner (null alpha: none): x += alpha p, r -= alpha (w - wmean)
// written back, rr_part[block] = sum r^2 nw -- the residual is in registers there anyway
struct nlg_pcg_upd {
    const double *alpha = nullptr, *wmean = nullptr;
    double *x = nullptr;
    const double *p = nullptr, *w = nullptr, *nw = nullptr;
    double *rr_part = nullptr;   // [(E + 3) / 4]
};
// z = M^-1 r (rz_part: r.z and z sums, (E + 3) / 4 blocks); nl lanes of a block step v * ld doubles apart
int pprec_apply(nlg_mesh *m, hipStream_t st, const double *flag, const double *r, double *z, double *rz_part, bool overlap,
                bool with_coarse, const nlg_pcg_upd *upd = nullptr, int nl = 1, int64_t ld = 0);
int pprec_reserve_lanes(nlg_mesh *m, int nl);
void pprec_free(nlg_mesh *m);

// ---- halo.hip ----
int halo_setup(nlg_mesh *m, const int64_t *glo_num);
// LAYOUT_*; = halo_begin + halo_finish.  assign: every local copy of a shared point becomes the sum of the OTHER ranks' copies
// (copy mode: a value that exactly one element on another rank produced for this rank's element), instead of adding that sum
int halo_exchange(nlg_mesh *m, double *const *fields, int nf, int layout = 0, int nl = 1, int64_t ld = 0, bool assign = false);
int gs_split(nlg_mesh *m);   // builds gs.tab_halo / tab_rest from gs.h_groups and the halo lists
int halo_begin(nlg_mesh *m, double *const *fields, int nf, int layout, int nl = 1, int64_t ld = 0);    // pack + start of the exchange
int halo_finish(nlg_mesh *m, double *const *fields, int nf, int layout, int nl = 1, int64_t ld = 0, bool assign = false);   // end of the exchange + unpack
void halo_free(nlg_mesh *m);

// ---- sem.hip (device-pointer level operators; all on ctx->stream) ----
// Lanes (everywhere below): nl <= kMaxLanes vectors of a block step in one call.  Every pointer argument is lane 0's; lane v of a
// per-lane field, flag or sum sits v * ld doubles behind it.  ldv: the same for the velocity-mesh fields of the pressure
// operators (sem_opgradt, sem_opdiv), whose pressure-mesh arguments step by ld.  ldg: the gates of sem_gs.  Where a kernel has
// no lane dimension the operator launches it once per lane.
int sem_gs(nlg_mesh *m, double *const *fields, int nf, const double *gate = nullptr, int layout = 0, int nl = 1, int64_t ld = 0, int64_t ldg = 0);   // in place QQ^T; gate: device flag, non-zero = skip; layout: LAYOUT_NAT or LAYOUT_XP
int sem_to_xp(nlg_mesh *m, double *const *src, double *const *dst, int nf, int nl = 1, int64_t ld = 0, double *const *wts = nullptr);     // natural -> x-planes-first (out of place); wts: dst = wts * src
int sem_from_xp(nlg_mesh *m, double *const *src, double *const *dst, int nf, int nl = 1, int64_t ld = 0);
int sem_axhelm(nlg_mesh *m, double *const *u, double *const *w, int nf, double h1, double h2, double *pw_part = nullptr,
               double *const *zf = nullptr, const double *beta_p = nullptr, const double *done_p = nullptr, bool xp = false, int nl = 1, int64_t ld = 0, int64_t uoff = 0,
               const double *pcinv = nullptr, const unsigned char *pcmb = nullptr);   // uoff: the updated direction is stored uoff doubles behind u (direction history of the PCG); zf: fused u <- zf + beta u; xp: u, zf, w in the x-planes-first layout (3-D, lx1 <= 8); pcinv, pcmb (3-D): zf is the residual r, u <- pc r + beta u with pc = bit c of pcmb ? pcinv : 0 (shared by the lanes, layout of zf)
bool sem_axhelm_forms_z(const nlg_mesh *m);   // the sizes at which the operator kernel takes pcinv / pcmb without losing a wave per SIMD
int sem_opdiv_blocks(const nlg_mesh *m);
int sem_axhelm_blocks(nlg_mesh *m, int nf);   // 3-D: number of per-block sums of u . w_local written to pw_part
int sem_helm_diag(nlg_mesh *m, double *out, double h1, double h2);   // local diag (not assembled)
// direction update of a PCG performed by the operator while it loads p:  p <- (z - zmean[0]) + beta[0] p   (device scalars; per lane at ld)
struct nlg_pupd {
    const double *z = nullptr, *beta = nullptr, *zmean = nullptr;
    double *p = nullptr;
};
bool sem_opgradt_has_fg(const nlg_mesh *m);
int sem_opgradt(nlg_mesh *m, const double *p, double *const *w, bool face_grouped = false, const double *gate = nullptr, const nlg_pupd *upd = nullptr,
                int nl = 1, int64_t ld = 0, int64_t ldv = 0);
int sem_opdiv(nlg_mesh *m, double *const *u, double *out, double scale, double *const *wts = nullptr, bool face_grouped = false,
              const double *pdot = nullptr, double *pw_part = nullptr, const double *gate = nullptr, int nl = 1, int64_t ld = 0, int64_t ldv = 0);
int sem_opbinv(nlg_mesh *m, double *const *w, int nl = 1, int64_t ld = 0);                       // w_i <- mask_i binv QQ^T w_i
bool sem_opgradt_fuses_pupdate(const nlg_mesh *m);
bool sem_small_mesh(const nlg_mesh *m);   // local element count below the threshold of the strong-scaling kernel variants (NLG_SMALL_E)
bool sem_pop_mfma(const nlg_mesh *m);     // single-vector opgradt / opdiv launches take the matrix-pipe kernels (3-D, lx1 = 8, not a small mesh; NLG_POP_MFMA)
int sem_cdabdtp(nlg_mesh *m, const double *p, double *out, double *pw_part = nullptr, const double *gate = nullptr, const nlg_pupd *upd = nullptr,
                int nl = 1, int64_t ld = 0);
int sem_ediag(nlg_mesh *m, double *out);
int sem_tensor(nlg_mesh *m, const double *in, double *out, int nin, int nout, const double *Mx, const double *My,
               const double *Mz, const double *wt);
int sem_conv_setup(nlg_mesh *m, double *const *U, double **Ur, double **GU);
int sem_conv_apply(nlg_mesh *m, double *const *Ur, double *const *GU, double *const *u, double *const *out, int adjoint, int nl = 1, int64_t ld = 0);
int sem_conv_apply_generic(nlg_mesh *m, double *const *Ur, double *const *GU, double *const *u, double *const *out, int adjoint);
int sem_conv_scalar_setup(nlg_mesh *m, const double *Theta, double **GT);
int sem_conv_scalar_apply(nlg_mesh *m, double *const *Ur, double *const *GT, double *const *u, const double *theta, double *out, int adjoint = 0,
                          int nl = 1, int64_t ld = 0);
int sem_scalar_grad_apply(nlg_mesh *m, double *const *GT, const double *theta, double *const *out, double sgn, int nl = 1, int64_t ld = 0);
int sem_cfl(nlg_mesh *m, double *const *U, double dt, double *cfl_host);
int sem_ortho(nlg_mesh *m, double *p, int nl = 1, int64_t ld = 0);
// explicit modal filter: the dense 1-D matrix F (n x n, row-major, host; ncut attenuated modes, weight of the last one), and its
// element-local action fields_c <- (F x F [x F]) fields_c on nf <= 4 fields of nl lanes in ONE launch.  upd_x: the velocity
// correction fields_c += upd_s * upd_wt_c * upd_x_c (c < dim; x through the element-local table `slot` when given) rides in the load
bool sem_filter_available(const nlg_mesh *m);   // kernels exist for 2-D lx1 = 6, 8, 10 and 3-D lx1 = 6, 8, 10, 12
int sem_filter_matrix(const nlg_mesh *m, int ncut, double weight, std::vector<double> &F);
int sem_filter(nlg_mesh *m, const double *F, double *const *fields, int nf, int nl = 1, int64_t ld = 0, double *const *upd_x = nullptr,
               double *const *upd_wt = nullptr, double upd_s = 0.0, const int *slot = nullptr);
double *sem_scratch1(nlg_mesh *m, int i);
double *sem_scratchd(nlg_mesh *m, int i);
double *sem_scratch2(nlg_mesh *m, int i);

}  // namespace nlg
