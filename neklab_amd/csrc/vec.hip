// nek_dvector vector space and Krylov-basis block kernels (gfx950).
//
// Layout of one vector in HBM (doubles):
//   [ v_0 | v_1 | (v_2) | theta_0.. | pr ]  main block, `main_len = ncomp*lvs + lps`
//   followed by lorder-1 history blocks of the same shape (reference: neklab_vectors.f90:30-35).
// `lvs`/`lps` are the field lengths rounded up to 32 doubles; the padding is zero in every vector and
// in the weight `bm1`, so every kernel can sweep whole padded ranges with 16-byte accesses.
//
// Roofline: every kernel here is HBM-bound (<= 0.25 flop/B).  Algorithmic bytes per call:
//   scal 16 B/dof, axpby 24 B/dof, dot 24 B/dof (a, b, bm1), block_dot 8*(k+2) B per inner-product
//   dof, block_axpy 8*(k+2) B per dof.
#include <algorithm>

#include "internal.h"

using namespace nlg;

namespace {

constexpr int NT = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over the 256 threads of a block; valid in thread 0. `sm` needs 4 doubles.
__device__ __forceinline__ double block_sum(double v, double *sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r += sm[i];
    }
    return r;
}

// A load of the basis in a kernel that passes over it once: non-temporal, so that the 8 - 27 GB of a sweep do not push the arrays
// that ARE re-used (w, bm1, the coefficients) out of L2 and the Infinity Cache.  NTL = false: a plain load, for the few columns of a
// small k that DO survive in the Infinity Cache from one pass of CGS2 to the next (stream_basis below).  The two fused sweeps
// (k_block_axpy_dot, k_block_axpy_dot2: one wave per SIMD, 64 loads in flight per wave) keep plain loads: non-temporal ones were
// 0.05 ms faster on one grade of MI355X box and 0.04 ms slower on the other (profiles/arnoldi_tail_ab_same_box.txt)
template <bool NTL = true>
__device__ __forceinline__ double2 ld_once(const double2 *p) {
    if (!NTL) return *p;
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(p));
    return make_double2(t.x, t.y);
}
// k columns of `len` doubles each, read by every pass of an orthogonalisation: streamed past the caches from four times the
// Infinity Cache (256 MB) on.  Below that part of the basis is still there when the next pass comes (measured at 140 MB per column:
// CGS2 at k = 1, 2 loses 0.09 / 0.06 ms with non-temporal loads, k = 4 is even, k = 8 gains 0.08 ms)
inline bool stream_basis(int k, int64_t len) { return (int64_t)k * len * (int64_t)sizeof(double) >= ((int64_t)1 << 30); }

__global__ __launch_bounds__(NT) void k_fill(double2 *x, double v, int64_t n2) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) x[i] = make_double2(v, v);
}

__global__ __launch_bounds__(NT) void k_copy(double2 *y, const double2 *x, int64_t n2) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) y[i] = x[i];
}

// reference cmult: x(i) = x(i)*alpha  (real_vectors.f90:131)
__global__ __launch_bounds__(NT) void k_scal(double2 *x, double a, int64_t n2) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) {
        double2 v = x[i];
        v.x = __dmul_rn(v.x, a);
        v.y = __dmul_rn(v.y, a);
        x[i] = v;
    }
}

// ---- Lanes.  The orthogonalisation kernels below (k_scal_dev, k_dot_partial, k_block_dot, k_block_axpy) carry a lane in the grid:
// lane l is one vector with its OWN basis (the wavenumbers of a sweep are s separate eigenproblems advanced in lock-step,
// nlg_basis_cgs2_batch), and a single vector is the launch with one lane.  The base pointers of lane l come by value, its
// coefficients lie l * k behind lane 0's, its partial sums in the rows l * k .. l * k + k - 1 of the reduction workspace.
struct LaneVW {
    const double *V[kMaxLanes];   // column 0 of lane l's basis
    double *w[kMaxLanes];
    int nrst[kMaxLanes];          // valid history blocks of w[l]
};
struct LaneAB {
    const double *a[kMaxLanes], *b[kMaxLanes];
};

// the normalisation factor of a vector whose squared norm is sv (0 where sv is not positive): ONE expression for every kernel that
// scales by it, so that they all multiply by the same bits
__device__ __forceinline__ double inv_norm(double sv) { return sv > 0.0 ? 1.0 / sqrt(sv) : 0.0; }

// blockIdx.y = lane: w_l *= inv_norm(q[l]) over the main block (n2 double2 entries) and, with `hist`, the valid history blocks, the
// scalar on device
__global__ __launch_bounds__(NT) void k_scal_dev(LaneVW P, const double *q, int64_t n2, int hist) {
    const int l = blockIdx.y;
    const double a = inv_norm(q[l]);
    const int64_t n2all = hist ? n2 * (1 + P.nrst[l]) : n2;
    double2 *x = reinterpret_cast<double2 *>(P.w[l]);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2all; i += (int64_t)gridDim.x * NT) {
        double2 v = x[i];
        v.x = __dmul_rn(v.x, a);
        v.y = __dmul_rn(v.y, a);
        x[i] = v;
    }
}

// reference nek_daxpby (real_vectors.f90:162-206): scal(beta) then add2s2(self, vec, alpha) on the main
// block, and for each valid history slot of self: slot += alpha * (vec main | vec slot).
// Rounding mirrors the two sweeps: fl(fl(beta*y) + fl(alpha*x)).
__global__ __launch_bounds__(NT) void k_axpby(double2 *y, const double2 *x, double a, double b, int64_t n2,
                                              int nrst, int64_t blk2, int consistent) {
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) {
        const double2 xv = x[i];
        const double ax0 = __dmul_rn(a, xv.x), ax1 = __dmul_rn(a, xv.y);
        double2 yv = y[i];
        yv.x = __dadd_rn(__dmul_rn(yv.x, b), ax0);
        yv.y = __dadd_rn(__dmul_rn(yv.y, b), ax1);
        y[i] = yv;
        for (int r = 1; r <= nrst; ++r) {
            double2 rv = y[i + r * blk2];
            double s0 = ax0, s1 = ax1;
            if (consistent) {
                const double2 xr = x[i + r * blk2];
                s0 = __dmul_rn(a, xr.x);
                s1 = __dmul_rn(a, xr.y);
            }
            rv.x = __dadd_rn(__dmul_rn(rv.x, b), s0);
            rv.y = __dadd_rn(__dmul_rn(rv.y, b), s1);
            y[i + r * blk2] = rv;
        }
    }
}

// first stage of glsc3-type sums over the ncomp inner-product fields:
// partial[l*nper + c*nblk + blk] = sum_{i in chunk} a_c[i] b_c[i] bm1[i]  of lane l = blockIdx.z (nper = ncomp*nblk)
__global__ __launch_bounds__(NT) void k_dot_partial(LaneAB P, const double *bm1, int64_t lvs, int nblk, int nper, double *partial) {
    __shared__ double sm[4];
    const int c = blockIdx.y, l = blockIdx.z;
    const int64_t n2 = lvs >> 1;
    const int64_t per = (n2 + nblk - 1) / nblk;
    const int64_t beg = blockIdx.x * per, end = (beg + per < n2) ? beg + per : n2;
    const double2 *a2 = reinterpret_cast<const double2 *>(P.a[l] + c * lvs);
    const double2 *b2 = reinterpret_cast<const double2 *>(P.b[l] + c * lvs);
    const double2 *m2 = reinterpret_cast<const double2 *>(bm1);
    double acc = 0.0;
    for (int64_t i = beg + threadIdx.x; i < end; i += NT) {
        const double2 av = a2[i], bv = b2[i], mv = m2[i];
        acc += av.x * bv.x * mv.x + av.y * bv.y * mv.y;
    }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) partial[(int64_t)l * nper + c * nblk + blockIdx.x] = s;
}

// Border of the periodic-orbit Jacobian in one pass (nlg_upo_border): over the main block of the vectors, field c = blockIdx.y of
// ncomp + 1 (the pressure last),  w_c <- (w_c - v_c) + t fT_c  with the rounding of the two axpby sweeps it replaces, and over the
// ncomp inner-product fields the first stage of <f0, v> in the partition and summation order of k_dot_partial:
// partial[c*nblk + blk] = sum v_c f0_c bm1.  Reads w, v, fT, f0, bm1 and writes w: six streams against the nine of sub + axpby + dot.
__global__ __launch_bounds__(NT) void k_upo_border(double *w, const double *v, const double *fT, const double *f0, const double *bm1,
                                                   double t, int64_t lvs, int64_t lps, int ncomp, int nblk, double *partial) {
    __shared__ double sm[4];
    const int c = blockIdx.y;
    const bool ip = c < ncomp;
    const int64_t n2 = (ip ? lvs : lps) >> 1;
    const int64_t per = (n2 + nblk - 1) / nblk;
    const int64_t beg = blockIdx.x * per, end = (beg + per < n2) ? beg + per : n2;
    const int64_t off = (int64_t)c * lvs;
    double2 *w2 = reinterpret_cast<double2 *>(w + off);
    const double2 *v2 = reinterpret_cast<const double2 *>(v + off);
    const double2 *t2 = reinterpret_cast<const double2 *>(fT + off);
    const double2 *f2 = reinterpret_cast<const double2 *>(f0 + off);
    const double2 *m2 = reinterpret_cast<const double2 *>(bm1);
    double acc = 0.0;
    for (int64_t i = beg + threadIdx.x; i < end; i += NT) {
        const double2 vv = v2[i], tv = t2[i];
        double2 wv = w2[i];
        wv.x = __dadd_rn(__dadd_rn(wv.x, -vv.x), __dmul_rn(t, tv.x));
        wv.y = __dadd_rn(__dadd_rn(wv.y, -vv.y), __dmul_rn(t, tv.y));
        w2[i] = wv;
        if (ip) {
            const double2 fv = f2[i], mv = m2[i];
            acc += vv.x * fv.x * mv.x + vv.y * fv.y * mv.y;
        }
    }
    if (ip) {   // (uniform per block)
        const double s = block_sum(acc, sm);
        if (threadIdx.x == 0) partial[c * nblk + blockIdx.x] = s;
    }
}

// second stage, fixed order => deterministic: out[row] (+)= sum_b partial[row*nper + b]
__global__ __launch_bounds__(NT) void k_reduce_rows(const double *partial, int nper, double *out, int accumulate,
                                                    double *out2) {
    __shared__ double sm[4];
    const double *p = partial + (int64_t)blockIdx.x * nper;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nper; i += NT) acc += p[i];
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = s;
        if (accumulate) out2[blockIdx.x] += s;
    }
}

// The block projections cut the work into reduction chunks (points) x tiles (KB basis vectors); every tile of a chunk reads the same
// w and bm1.  blockIdx.x carries both so that the tiles of a chunk are dispatched next to each other AND onto the same XCD, where the
// first of them leaves w and bm1 in L2 for the others: workgroups go round the 8 XCDs in the order of blockIdx.x, so within a group
// of 8 chunks the chunk is blockIdx.x mod 8 and the tile the quotient.  Placement is only observed, not promised: it decides where
// the re-reads are served from, never a result.  (k = 64, 10^4 elements: k_block_dot 1.455 -> 1.396 ms beside tiles in blockIdx.z.)
constexpr int kXcd = 8;
inline unsigned chunk_tile_grid(int nblk, int ntile) { return (unsigned)((nblk + kXcd - 1) / kXcd * kXcd * ntile); }
__device__ __forceinline__ void chunk_tile(int ntile, int &chunk, int &tile) {
    const int grp = blockIdx.x / (kXcd * ntile), rem = blockIdx.x - grp * kXcd * ntile;
    chunk = grp * kXcd + rem % kXcd;      // may lie beyond nblk in the last group: such a block has nothing to do
    tile = rem / kXcd;
}

// h_j = V_j^T (bm1 o w) for a tile of KB basis vectors; V is read exactly once.
// blockIdx.x = chunk and tile (chunk_tile), blockIdx.y = lane * ncomp + field; partial row (lane * k + j)
template <int KB, bool NTL>
__global__ __launch_bounds__(NT) void k_block_dot(LaneVW P, int64_t vstride, int k, int ncomp, const double *bm1, int64_t lvs, int nblk,
                                                  int nper, double *partial) {
    __shared__ double sm[4 * KB];
    const int l = blockIdx.y / ncomp, c = blockIdx.y - l * ncomp;
    const double *V = P.V[l];
    const double *w = P.w[l];
    int chunk, tile;
    chunk_tile((k + KB - 1) / KB, chunk, tile);
    if (chunk >= nblk) return;
    const int j0 = tile * KB;
    const int kc = (k - j0 < KB) ? (k - j0) : KB;
    const int64_t n2 = lvs >> 1;
    const int64_t per = (n2 + nblk - 1) / nblk;
    const int64_t beg = chunk * per, end = (beg + per < n2) ? beg + per : n2;
    const double2 *w2 = reinterpret_cast<const double2 *>(w + c * lvs);
    const double2 *m2 = reinterpret_cast<const double2 *>(bm1);
    const double2 *v2[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        const int jj = (j < kc) ? j : 0;
        v2[j] = reinterpret_cast<const double2 *>(V + (int64_t)(j0 + jj) * vstride + c * lvs);
    }
    double acc[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) acc[j] = 0.0;
    for (int64_t i = beg + threadIdx.x; i < end; i += NT) {
        const double2 wv = w2[i], mv = m2[i];
        const double x0 = wv.x * mv.x, x1 = wv.y * mv.y;
        double2 vv[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) vv[j] = ld_once<NTL>(v2[j] + i);
#pragma unroll
        for (int j = 0; j < KB; ++j) acc[j] += vv[j].x * x0 + vv[j].y * x1;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        const double s = wave_sum(acc[j]);
        if (lane == 0) sm[wid * KB + j] = s;
    }
    __syncthreads();
    if (threadIdx.x < kc) {
        const int j = threadIdx.x;
        const double s = sm[j] + sm[KB + j] + sm[2 * KB + j] + sm[3 * KB + j];
        partial[((int64_t)l * k + j0 + j) * nper + c * nblk + chunk] = s;
    }
}

// CGS2, first subtraction and second projection in ONE sweep over the basis (k <= KMAX):
//   w <- w - V h   on the velocity (+ scalar) part of the main block,   partial[j] = V_j^T (bm1 o w_new).
// The second projection needs the finished w at a point and the k basis values at the same point — which the thread
// that has just computed w there still holds in registers.  One point per lane, the k values and the k running sums
// in registers (2 x KMAX doubles: one wave per SIMD, 64 independent loads in flight per wave), one block per CU.
// Saves one of the four reads of the basis that CGS2 otherwise makes.
template <int KMAX>
__global__ __launch_bounds__(NT) void k_block_axpy_dot(const double *__restrict__ V, int64_t vstride, int k,
                                                       const double *__restrict__ h, double *__restrict__ w,
                                                       const double *__restrict__ bm1, int64_t lvs, int64_t nv,
                                                       double *__restrict__ partial) {
    __shared__ double sh[KMAX];
    __shared__ double sm[4][KMAX];
    for (int j = threadIdx.x; j < KMAX; j += NT) sh[j] = j < k ? h[j] : 0.0;
    __syncthreads();
    double acc[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) acc[j] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * NT) {
        double v[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) v[j] = j < k ? V[(int64_t)j * vstride + i] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) s += sh[j] * v[j];
        const double wn = w[i] - s;
        w[i] = wn;
        const double x = wn * bm1[i % lvs];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) acc[j] += v[j] * x;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        const double t = wave_sum(acc[j]);
        if (lane == 0) sm[wid][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const int j = threadIdx.x;
        partial[(int64_t)j * gridDim.x + blockIdx.x] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
    }
}

// The same sweep for 64 < k <= 128 (round 4; BASELINE configs 4 and 5 name m = 128 and 256): k values and k running sums no longer fit
// one lane's registers, so the SECOND half of the basis values of a point is parked in LDS (one column of 64 doubles per thread: 128 KB of
// dynamic LDS, one block per CU as before) between the subtraction, which needs all k of them, and the projection, which needs them again
// together with the finished w: the basis is still read ONCE per pass.  Before, the 64 vectors in front of the fused tile cost a separate
// subtraction and a separate projection (k = 128: 448 vector reads per CGS2 instead of 384).
template <int KH>
__global__ __launch_bounds__(NT) void k_block_axpy_dot2(const double *__restrict__ V, int64_t vstride, int k,
                                                        const double *__restrict__ h, double *__restrict__ w,
                                                        const double *__restrict__ bm1, int64_t lvs, int64_t nv,
                                                        double *__restrict__ partial) {
    extern __shared__ double dyn2[];
    double *sh = dyn2;                    // 2 KH coefficients (zero beyond k)
    double *stash = dyn2 + 2 * KH;        // [KH][NT]: the second half of a point's basis values, column of this thread
    __shared__ double sm[4][2 * KH];
    for (int j = threadIdx.x; j < 2 * KH; j += NT) sh[j] = j < k ? h[j] : 0.0;
    __syncthreads();
    double acc0[KH], acc1[KH];
#pragma unroll
    for (int j = 0; j < KH; ++j) acc0[j] = 0.0, acc1[j] = 0.0;
    double *mine = stash + threadIdx.x;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * NT) {
        double v[KH];
#pragma unroll
        for (int j = 0; j < KH; ++j) v[j] = KH + j < k ? V[(int64_t)(KH + j) * vstride + i] : 0.0;
        double s1 = 0.0;
#pragma unroll
        for (int j = 0; j < KH; ++j) {
            s1 += sh[KH + j] * v[j];
            mine[j * NT] = v[j];
        }
#pragma unroll
        for (int j = 0; j < KH; ++j) v[j] = V[(int64_t)j * vstride + i];
        double s0 = 0.0;
#pragma unroll
        for (int j = 0; j < KH; ++j) s0 += sh[j] * v[j];
        const double wn = w[i] - (s0 + s1);
        w[i] = wn;
        const double x = wn * bm1[i % lvs];
#pragma unroll
        for (int j = 0; j < KH; ++j) {
            acc0[j] += v[j] * x;
            acc1[j] += mine[j * NT] * x;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KH; ++j) {
        const double t0 = wave_sum(acc0[j]), t1 = wave_sum(acc1[j]);
        if (lane == 0) sm[wid][j] = t0, sm[wid][KH + j] = t1;
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const int j = threadIdx.x;
        partial[(int64_t)j * gridDim.x + blockIdx.x] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
    }
}

// blockIdx.y = lane.  w_l += sign * V_l h_l on the main block (n2 double2 entries); the nrst[l] valid history blocks behind it
// follow `hist`: left alone, swept with the main block as one contiguous range (consistent mode: every entry receives the same
// linear combination of the basis at its own place), or given the main block's correction (the reference's axpby quirk).
// `hh` (may be null; HIST_SWEEP): a second coefficient set for the entries at or beyond n2: CGS2 applies the second-pass
// coefficients to the main block and the SUM of both passes to the history, which no inner product ever reads -> the history is
// swept once, not twice.
// TAIL (the end of CGS2, `hist` = HIST_ONLY): the history blocks alone (a lane without any: nothing), every updated entry then
// multiplied by inv_norm(q[l]) -- the update rounded first, the product after, as k_scal_dev would do to the stored value in a pass
// of its own.  A template parameter, so that the plain sweep compiles as if the tail did not exist.
enum { HIST_NONE = 0, HIST_SWEEP = 1, HIST_MAIN = 2, HIST_ONLY = 3 };
template <bool TAIL, bool NTL>
__global__ __launch_bounds__(NT) void k_block_axpy(LaneVW P, int64_t vstride, int k, const double *h, const double *hh, int64_t n2,
                                                   int hist, double sign, const double *q) {
    extern __shared__ double sh0[];
    double *sh1 = sh0 + k;
    const int l = blockIdx.y;
    if (TAIL && P.nrst[l] == 0) return;
    h += (int64_t)l * k;
    if (hh) hh += (int64_t)l * k;
    for (int j = threadIdx.x; j < k; j += NT) {
        sh0[j] = h[j];
        sh1[j] = hh ? hh[j] : h[j];
    }
    __syncthreads();
    const int64_t n2all = (TAIL || hist == HIST_SWEEP) ? n2 * (1 + P.nrst[l]) : n2;
    const int64_t ibeg = TAIL ? n2 : 0;
    const int ncopy = (!TAIL && hist == HIST_MAIN) ? P.nrst[l] : 0;
    const double a = TAIL ? inv_norm(q[l]) : 1.0;
    double2 *w2 = reinterpret_cast<double2 *>(P.w[l]);
    const double2 *V2 = reinterpret_cast<const double2 *>(P.V[l]);
    const int64_t vs2 = vstride >> 1;
    for (int64_t i = ibeg + blockIdx.x * (int64_t)NT + threadIdx.x; i < n2all; i += (int64_t)gridDim.x * NT) {
        const double *sh = (hh && i >= n2) ? sh1 : sh0;
        double s0 = 0.0, s1 = 0.0;
        const double2 *v = V2 + i;
        int j = 0;
        for (; j + 8 <= k; j += 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = ld_once<NTL>(v + (int64_t)(j + u) * vs2);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s0 += sh[j + u] * t[u].x;
                s1 += sh[j + u] * t[u].y;
            }
        }
        for (; j < k; ++j) {
            const double2 t = ld_once<NTL>(v + (int64_t)j * vs2);
            s0 += sh[j] * t.x;
            s1 += sh[j] * t.y;
        }
        double2 wv = w2[i];
        wv.x += sign * s0;
        wv.y += sign * s1;
        if (TAIL) {
            wv.x = __dmul_rn(wv.x, a);
            wv.y = __dmul_rn(wv.y, a);
        }
        w2[i] = wv;
        for (int r = 1; r <= ncopy; ++r) {
            double2 rv = w2[i + r * n2];
            rv.x += sign * s0;
            rv.y += sign * s1;
            w2[i + r * n2] = rv;
        }
    }
}

// ---- block (multi-vector) orthogonalisation: S new vectors W = [w_0 .. w_{S-1}] (consecutive basis columns, wstride apart)
// against k basis vectors in ONE sweep over the basis per pass -- the basis is read once per S vectors instead of once per
// vector.  Partial sums: row (j * S + v) of the reduction workspace holds V_j^T (bm1 o w_v).
template <int KB, int S>
__global__ __launch_bounds__(NT) void k_block_dot_s(const double *V, int64_t vstride, int k, const double *W, int64_t wstride,
                                                    const double *bm1, int64_t lvs, int nblk, int nper, double *partial) {
    __shared__ double sm[4 * KB * S];
    const int c = blockIdx.y;
    int chunk, tile;
    chunk_tile((k + KB - 1) / KB, chunk, tile);
    if (chunk >= nblk) return;
    const int j0 = tile * KB;
    const int kc = (k - j0 < KB) ? (k - j0) : KB;
    const int64_t n2 = lvs >> 1;
    const int64_t per = (n2 + nblk - 1) / nblk;
    const int64_t beg = chunk * per, end = (beg + per < n2) ? beg + per : n2;
    const double2 *m2 = reinterpret_cast<const double2 *>(bm1);
    const double2 *v2[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        const int jj = (j < kc) ? j : 0;
        v2[j] = reinterpret_cast<const double2 *>(V + (int64_t)(j0 + jj) * vstride + c * lvs);
    }
    double acc[KB][S];
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
        for (int v = 0; v < S; ++v) acc[j][v] = 0.0;
    for (int64_t i = beg + threadIdx.x; i < end; i += NT) {
        const double2 mv = m2[i];
        double x0[S], x1[S];
#pragma unroll
        for (int v = 0; v < S; ++v) {
            const double2 wv = reinterpret_cast<const double2 *>(W + (int64_t)v * wstride + c * lvs)[i];
            x0[v] = wv.x * mv.x;
            x1[v] = wv.y * mv.y;
        }
        double2 vv[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) vv[j] = ld_once(v2[j] + i);
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int v = 0; v < S; ++v) acc[j][v] += vv[j].x * x0[v] + vv[j].y * x1[v];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
        for (int v = 0; v < S; ++v) {
            const double t = wave_sum(acc[j][v]);
            if (lane == 0) sm[wid * KB * S + j * S + v] = t;
        }
    __syncthreads();
    if (threadIdx.x < kc * S) {
        const int q = threadIdx.x;   // j * S + v
        const double t = (sm[q] + sm[KB * S + q]) + (sm[2 * KB * S + q] + sm[3 * KB * S + q]);
        partial[((int64_t)j0 * S + q) * nper + c * nblk + chunk] = t;
    }
}

// w_v += sign * sum_j h[j * S + v] V_j for v < S over [0, n2) double2 entries; entries at or beyond blk2 (the history
// blocks) use the coefficient set hh instead (CGS2: second-pass coefficients on the main block, the sum of both passes on
// the history, which no inner product reads).  The k basis values of a point are loaded once for all S vectors.
template <int S>
__global__ __launch_bounds__(NT) void k_block_axpy_s(const double *V, int64_t vstride, int k, const double *h, const double *hh,
                                                     double *W, int64_t wstride, int64_t n2, int64_t blk2, double sign) {
    extern __shared__ double shs[];
    double *sh0 = shs, *sh1 = shs + (size_t)k * S;
    for (int j = threadIdx.x; j < k * S; j += NT) {
        sh0[j] = h[j];
        sh1[j] = hh ? hh[j] : h[j];
    }
    __syncthreads();
    const int64_t vs2 = vstride >> 1, ws2 = wstride >> 1;
    double2 *w2 = reinterpret_cast<double2 *>(W);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) {
        const double *sh = (hh && i >= blk2) ? sh1 : sh0;
        const double2 *v = reinterpret_cast<const double2 *>(V) + i;
        double s0[S], s1[S];
#pragma unroll
        for (int q = 0; q < S; ++q) s0[q] = s1[q] = 0.0;
        int j = 0;
        for (; j + 8 <= k; j += 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = ld_once(v + (int64_t)(j + u) * vs2);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    s0[q] += sh[(j + u) * S + q] * t[u].x;
                    s1[q] += sh[(j + u) * S + q] * t[u].y;
                }
        }
        for (; j < k; ++j) {
            const double2 t = ld_once(v + (int64_t)j * vs2);
#pragma unroll
            for (int q = 0; q < S; ++q) {
                s0[q] += sh[j * S + q] * t.x;
                s1[q] += sh[j * S + q] * t.y;
            }
        }
#pragma unroll
        for (int q = 0; q < S; ++q) {
            double2 wv = w2[i + q * ws2];
            wv.x += sign * s0[q];
            wv.y += sign * s1[q];
            w2[i + q * ws2] = wv;
        }
    }
}

// W <- W T with a small S x S matrix T (row-major, on the device) over [0, n2) double2 entries of every vector: the
// triangular solve of a Cholesky QR, applied to all fields and history blocks like `scal`
template <int S>
__global__ __launch_bounds__(NT) void k_block_rmul(double *W, int64_t wstride, const double *T, int64_t n2) {
    double t[S][S];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) t[a][b] = T[a * S + b];
    const int64_t ws2 = wstride >> 1;
    double2 *w2 = reinterpret_cast<double2 *>(W);
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * NT) {
        double2 x[S], y[S];
#pragma unroll
        for (int a = 0; a < S; ++a) x[a] = w2[i + a * ws2];
#pragma unroll
        for (int b = 0; b < S; ++b) {
            y[b].x = y[b].y = 0.0;
#pragma unroll
            for (int a = 0; a < S; ++a) {
                y[b].x += x[a].x * t[a][b];
                y[b].y += x[a].y * t[a][b];
            }
        }
#pragma unroll
        for (int b = 0; b < S; ++b) w2[i + b * ws2] = y[b];
    }
}

__global__ void k_vadd(double *a, const double *b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] += b[i];
}

inline int grid_for(int64_t n2) {
    int64_t g = (n2 + NT - 1) / NT;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

inline int dot_nblk(const nlg_vec *v) {
    int64_t nb = v->mesh->lvs / 4096;
    int cap = kMaxBlocksReduce / v->ncomp;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return (int)nb;
}

int check_same(const nlg_vec *a, const nlg_vec *b, const char *who) {
    NLG_CHECK(a && b, "%s: NULL vector", who);
    NLG_CHECK(a->mesh == b->mesh && a->nscal == b->nscal && a->lorder == b->lorder,
              "%s: vectors live on different meshes / layouts (reference: type_error, real_vectors.f90:202-204)", who);
    return 0;
}

}  // namespace

namespace nlg {

int dev_dot(const nlg_vec *a, const nlg_vec *b, int slot) {
    nlg_ctx *ctx = a->mesh->ctx;
    const int nblk = dot_nblk(a);
    LaneAB P = {};
    P.a[0] = a->d, P.b[0] = b->d;
    NLG_LAUNCH(k_dot_partial, dim3(nblk, a->ncomp), dim3(NT), 0, ctx->stream, P, (const double *)a->mesh->d_bm1, a->mesh->lvs, nblk,
               nblk * a->ncomp, ctx->d_partial);
    NLG_LAUNCH(k_reduce_rows, dim3(1), dim3(NT), 0, ctx->stream, ctx->d_partial, nblk * a->ncomp,
                       ctx->d_scalars + slot, 0, (double *)nullptr);
    NLG_HIP(hipGetLastError());
    NLG_TRY(allreduce_sum(ctx, ctx->d_scalars + slot, 1));
    return 0;
}

// w <- w - v + t fT on the main block, <f0, v> left on device at ctx->d_scalars[slot] (allreduced); no vector carries history
int upo_border_dev(nlg_vec *w, const nlg_vec *v, const nlg_vec *fT, const nlg_vec *f0, double t, int slot) {
    nlg_mesh *m = w->mesh;
    nlg_ctx *ctx = m->ctx;
    const int nblk = dot_nblk(w);
    NLG_LAUNCH(k_upo_border, dim3(nblk, w->ncomp + 1), dim3(NT), 0, ctx->stream, w->d, (const double *)v->d, (const double *)fT->d,
               (const double *)f0->d, (const double *)m->d_bm1, t, m->lvs, m->lps, w->ncomp, nblk, ctx->d_partial);
    NLG_LAUNCH(k_reduce_rows, dim3(1), dim3(NT), 0, ctx->stream, ctx->d_partial, nblk * w->ncomp, ctx->d_scalars + slot, 0, (double *)nullptr);
    NLG_HIP(hipGetLastError());
    NLG_TRY(allreduce_sum(ctx, ctx->d_scalars + slot, 1));
    return 0;
}

// dst <- 0, then the velocity and the pressure of src's main block (no scalars, no restart history)
int vec_copy_main(nlg_vec *dst, const nlg_vec *src) {
    nlg_mesh *m = src->mesh;
    NLG_TRY(nlg_vec_zero(dst));
    for (int c = 0; c < m->dim; ++c)
        NLG_HIP(hipMemcpyAsync(dst->vel(c), src->vel(c), sizeof(double) * (size_t)m->lvn, hipMemcpyDeviceToDevice, m->ctx->stream));
    NLG_HIP(hipMemcpyAsync(dst->pr(), src->pr(), sizeof(double) * (size_t)m->lpn, hipMemcpyDeviceToDevice, m->ctx->stream));
    return 0;
}

}  // namespace nlg

static int g_axpby_consistent = 1;   // default reproduces the reference's published eigenvalue, see include/neklab_gpu.h

extern "C" {

int nlg_set_axpby_rst_consistent(int flag) {
    g_axpby_consistent = flag ? 1 : 0;
    return 0;
}

// ---- handle lifetimes for by-value host languages (the Fortran shim) ---------------------------------------------------
// The reference's vectors are plain arrays: intrinsic assignment, sourced allocation, array constructors and reallocation on
// assignment copy them bit by bit (neklab_analysis.f90:250 `allocate(Lu(r), source=..)`).  A shim object holding a handle is
// then duplicated behind its type's back, and its finaliser may run on the ORIGINAL while a copy is still going to be used
// (`X = [X, v]`: the temporary holds the copies, the old X is finalised, the new X receives the bits).  So the owner's
// finaliser does not free: it RELEASES the handle (state "released", buffer kept); a copy that turns up later ADOPTS it --
// released: the copy becomes the owner, nothing is copied or leaked; still owned elsewhere: the caller clones.  Every handle
// carries a generation number, so that a copy whose handle has meanwhile been freed and whose address has been reused is
// recognised instead of reading someone else's data.  Released buffers are freed oldest first once they hold more than
// g_pool_limit bytes (nlg_vec_pool_limit) or when an allocation fails, and all of them by nlg_vec_pool_trim.
namespace {
struct VecInfo {
    uint64_t gen = 0;
    bool released = false;      // the owner's finaliser ran: in the pool, evictable, any copy may adopt it
    bool pinned = false;        // released, then READ by a copy that cannot take ownership (intent(in) use): out of the pool, still adoptable
    uint64_t released_at = 0;
};
std::map<const nlg_vec *, VecInfo> g_vecs;      // every live or released handle
uint64_t g_next_gen = 1, g_release_tick = 0;
int64_t g_pool_bytes = 0, g_pool_limit = (int64_t)32 << 30;

void pool_free_oldest() {
    const nlg_vec *old = nullptr;
    uint64_t at = ~0ull;
    for (auto &kv : g_vecs)
        if (kv.second.released && kv.second.released_at < at) at = kv.second.released_at, old = kv.first;
    if (!old) return;
    nlg_vec *v = const_cast<nlg_vec *>(old);
    g_pool_bytes -= (int64_t)sizeof(double) * v->total_len;
    g_vecs.erase(old);
    if (v->owns && v->d) hipFree(v->d);
    delete v;
}
}  // namespace

int nlg_vec_create(nlg_mesh *mesh, int nscal, int lorder, nlg_vec **out) {
    NLG_CHECK(mesh && out, "nlg_vec_create: NULL argument");
    NLG_CHECK(nscal >= 0 && nscal <= 8, "nlg_vec_create: nscal %d out of range", nscal);
    NLG_CHECK(lorder >= 1 && lorder <= 4, "nlg_vec_create: lorder %d out of range", lorder);
    nlg_vec *v = new nlg_vec();
    v->mesh = mesh;
    v->nscal = nscal;
    v->lorder = lorder;
    v->ncomp = mesh->dim + nscal;
    v->main_len = (int64_t)v->ncomp * mesh->lvs + mesh->lps;
    v->total_len = v->main_len * lorder;
    NLG_HIP(hipSetDevice(mesh->ctx->device));
    hipError_t e = hipMalloc(&v->d, sizeof(double) * (size_t)v->total_len);
    while (e != hipSuccess && g_pool_bytes > 0) {   // give released buffers back before failing
        (void)hipGetLastError();
        pool_free_oldest();
        e = hipMalloc(&v->d, sizeof(double) * (size_t)v->total_len);
    }
    if (e != hipSuccess) {
        delete v;
        set_error("nlg_vec_create: hipMalloc(%zu bytes) failed: %s", sizeof(double) * (size_t)v->total_len,
                  hipGetErrorString(e));
        return 1;
    }
    NLG_HIP(hipMemsetAsync(v->d, 0, sizeof(double) * (size_t)v->total_len, mesh->ctx->stream));
    g_vecs[v].gen = g_next_gen++;
    *out = v;
    return 0;
}

int nlg_vec_destroy(nlg_vec *v) {
    if (!v) return 0;
    auto it = g_vecs.find(v);
    if (it != g_vecs.end()) {
        if (it->second.released) g_pool_bytes -= (int64_t)sizeof(double) * v->total_len;
        g_vecs.erase(it);
    }
    if (v->owns && v->d) hipFree(v->d);   // hipFree synchronises; never touch the parent mesh here
    delete v;
    return 0;
}

int nlg_vec_generation(const nlg_vec *v, int64_t *gen) {
    NLG_CHECK(v && gen, "nlg_vec_generation: NULL argument");
    auto it = g_vecs.find(v);
    NLG_CHECK(it != g_vecs.end(), "nlg_vec_generation: unknown handle (freed, or not created by nlg_vec_create)");
    *gen = (int64_t)it->second.gen;
    return 0;
}

int nlg_vec_release(nlg_vec *v) {
    if (!v) return 0;
    auto it = g_vecs.find(v);
    NLG_CHECK(it != g_vecs.end(), "nlg_vec_release: unknown handle");
    if (it->second.released) return 0;
    it->second.released = true;
    it->second.released_at = ++g_release_tick;
    g_pool_bytes += (int64_t)sizeof(double) * v->total_len;
    while (g_pool_bytes > g_pool_limit) pool_free_oldest();
    return 0;
}

int nlg_vec_adopt(nlg_vec *v, int64_t gen, int *status) {
    NLG_CHECK(v && status, "nlg_vec_adopt: NULL argument");
    auto it = g_vecs.find(v);
    NLG_CHECK(it != g_vecs.end() && (int64_t)it->second.gen == gen,
              "nlg_vec_adopt: the handle of this copy has been freed (a bitwise copy of a vector was used after more than "
              "nlg_vec_pool_limit bytes of released vectors piled up, or after nlg_vec_pool_trim)");
    if (it->second.released || it->second.pinned) {
        if (it->second.released) g_pool_bytes -= (int64_t)sizeof(double) * v->total_len;
        it->second.released = it->second.pinned = false;
        *status = 1;   // the caller owns the handle now
    } else {
        *status = 0;   // owned by a live object: the caller clones
    }
    return 0;
}

int nlg_vec_pin(nlg_vec *v, int64_t gen) {
    NLG_CHECK(v, "nlg_vec_pin: NULL argument");
    auto it = g_vecs.find(v);
    NLG_CHECK(it != g_vecs.end() && (int64_t)it->second.gen == gen,
              "nlg_vec_pin: the handle of this copy has been freed (a bitwise copy of a vector was used after more than "
              "nlg_vec_pool_limit bytes of released vectors piled up, or after nlg_vec_pool_trim)");
    if (it->second.released) {   // read through a released handle: keep it out of the eviction pool from now on
        it->second.released = false;
        it->second.pinned = true;
        g_pool_bytes -= (int64_t)sizeof(double) * v->total_len;
    }
    return 0;
}

int nlg_vec_unpin(nlg_vec *v, int64_t gen) {
    if (!v) return 0;
    auto it = g_vecs.find(v);
    if (it == g_vecs.end() || (int64_t)it->second.gen != gen || !it->second.pinned) return 0;   // not this copy's business
    it->second.pinned = false;
    it->second.released = true;
    it->second.released_at = ++g_release_tick;
    g_pool_bytes += (int64_t)sizeof(double) * v->total_len;
    while (g_pool_bytes > g_pool_limit) pool_free_oldest();
    return 0;
}

int64_t nlg_vec_size_checked(const nlg_vec *v, int64_t gen) {
    auto it = g_vecs.find(v);
    if (!v || it == g_vecs.end() || (int64_t)it->second.gen != gen) return -1;
    return (int64_t)v->ncomp * v->mesh->lvn + v->mesh->lpn;
}

int nlg_vec_has_rst_checked(const nlg_vec *v, int64_t gen) {
    auto it = g_vecs.find(v);
    if (!v || it == g_vecs.end() || (int64_t)it->second.gen != gen) return -1;
    return v->nrst > 0 ? 1 : 0;
}

int nlg_vec_pool_limit(int64_t bytes) {
    NLG_CHECK(bytes >= 0, "nlg_vec_pool_limit: negative limit");
    g_pool_limit = bytes;
    while (g_pool_bytes > g_pool_limit) pool_free_oldest();
    return 0;
}

int nlg_vec_pool_trim(int64_t *freed_bytes) {
    const int64_t before = g_pool_bytes;
    while (g_pool_bytes > 0) pool_free_oldest();
    if (freed_bytes) *freed_bytes = before;
    return 0;
}

int nlg_vec_copy(nlg_vec *dst, const nlg_vec *src) {
    NLG_TRY(check_same(dst, src, "nlg_vec_copy"));
    if (dst->d != src->d)
        NLG_HIP(hipMemcpyAsync(dst->d, src->d, sizeof(double) * (size_t)src->total_len, hipMemcpyDeviceToDevice,
                               src->mesh->ctx->stream));
    dst->nrst = src->nrst;
    return 0;
}

int nlg_vec_clone(const nlg_vec *src, nlg_vec **out) {
    NLG_CHECK(src && out, "nlg_vec_clone: NULL argument");
    NLG_TRY(nlg_vec_create(src->mesh, src->nscal, src->lorder, out));
    return nlg_vec_copy(*out, src);
}

int nlg_vec_zero(nlg_vec *self) {
    NLG_CHECK(self, "nlg_vec_zero: NULL vector");
    NLG_HIP(hipMemsetAsync(self->d, 0, sizeof(double) * (size_t)self->total_len, self->mesh->ctx->stream));
    self->nrst = 0;
    return 0;
}

int nlg_vec_scal(nlg_vec *self, double alpha) {
    NLG_CHECK(self, "nlg_vec_scal: NULL vector");
    const int64_t n2 = self->main_len * (1 + self->nrst) / 2;
    NLG_LAUNCH(k_scal, dim3(grid_for(n2)), dim3(NT), 0, self->mesh->ctx->stream,
                       reinterpret_cast<double2 *>(self->d), alpha, n2);
    NLG_HIP(hipGetLastError());
    return 0;
}

int nlg_vec_axpby(double alpha, const nlg_vec *vec, double beta, nlg_vec *self) {
    NLG_TRY(check_same(self, vec, "nlg_vec_axpby"));
    const int64_t n2 = self->main_len / 2;
    NLG_LAUNCH(k_axpby, dim3(grid_for(n2)), dim3(NT), 0, self->mesh->ctx->stream,
                       reinterpret_cast<double2 *>(self->d), reinterpret_cast<const double2 *>(vec->d), alpha, beta, n2,
                       self->nrst, n2, g_axpby_consistent);
    NLG_HIP(hipGetLastError());
    return 0;
}

int nlg_vec_dot(const nlg_vec *self, const nlg_vec *vec, double *out) {
    NLG_TRY(check_same(self, vec, "nlg_vec_dot"));
    NLG_CHECK(out, "nlg_vec_dot: out is NULL");
    NLG_TRY(dev_dot(self, vec, 0));
    return scalars_to_host(self->mesh->ctx, 0, 1, out);
}

int nlg_vec_norm(const nlg_vec *self, double *out) {
    double d = 0.0;
    NLG_TRY(nlg_vec_dot(self, self, &d));
    *out = sqrt(d);
    return 0;
}

int nlg_vec_size(const nlg_vec *self, int64_t *out) {
    NLG_CHECK(self && out, "nlg_vec_size: NULL argument");
    *out = (int64_t)self->ncomp * self->mesh->lvn + self->mesh->lpn;
    return 0;
}

int nlg_vec_save_rst(nlg_vec *self, const nlg_vec *vec_rst, int irst) {
    NLG_TRY(check_same(self, vec_rst, "nlg_vec_save_rst"));
    // reference: "Cannot save rst fields <torder> for a simulation of temporal order <torder>"
    NLG_CHECK(irst >= 1 && irst < self->lorder, "nlg_vec_save_rst: cannot save rst fields %d for temporal order %d", irst,
              self->lorder);
    NLG_HIP(hipMemcpyAsync(self->d + (int64_t)irst * self->main_len, vec_rst->d, sizeof(double) * (size_t)self->main_len,
                           hipMemcpyDeviceToDevice, self->mesh->ctx->stream));
    if (irst > self->nrst) self->nrst = irst;
    return 0;
}

int nlg_vec_get_rst(const nlg_vec *self, nlg_vec *vec_rst, int irst) {
    NLG_TRY(check_same(self, vec_rst, "nlg_vec_get_rst"));
    NLG_CHECK(irst >= 1 && irst < self->lorder, "nlg_vec_get_rst: invalid input for irst: %d", irst);
    NLG_HIP(hipMemcpyAsync(vec_rst->d, self->d + (int64_t)irst * self->main_len, sizeof(double) * (size_t)self->main_len,
                           hipMemcpyDeviceToDevice, self->mesh->ctx->stream));
    return 0;
}

int nlg_vec_has_rst_fields(const nlg_vec *self, int *out) {
    NLG_CHECK(self && out, "nlg_vec_has_rst_fields: NULL argument");
    *out = self->nrst > 0;
    return 0;
}

int nlg_vec_clear_rst_fields(nlg_vec *self) {
    NLG_CHECK(self, "nlg_vec_clear_rst_fields: NULL vector");
    self->nrst = 0;
    return 0;
}

int nlg_vec_nrst(const nlg_vec *self, int *out) {
    NLG_CHECK(self && out, "nlg_vec_nrst: NULL argument");
    *out = self->nrst;
    return 0;
}

static int field_ptr(const nlg_vec *v, int field, int irst, double **p, int64_t *len) {
    NLG_CHECK(v, "field access: NULL vector");
    NLG_CHECK(irst >= 0 && irst < v->lorder, "field access: irst %d out of range", irst);
    const nlg_mesh *m = v->mesh;
    if (field >= NLG_VX && field <= NLG_VZ) {
        NLG_CHECK(field < m->dim, "field access: component %d on a %d-D mesh", field, m->dim);
        *p = v->vel(field, irst);
        *len = m->lvn;
    } else if (field == NLG_PR) {
        *p = v->pr(irst);
        *len = m->lpn;
    } else {
        const int s = field - NLG_THETA;
        NLG_CHECK(s >= 0 && s < v->nscal, "field access: scalar %d not active (nscal=%d)", s, v->nscal);
        *p = v->theta(s, irst);
        *len = m->lvn;
    }
    return 0;
}

int nlg_vec_set_field(nlg_vec *self, int field, int irst, const double *host, int64_t count) {
    double *p;
    int64_t len;
    NLG_TRY(field_ptr(self, field, irst, &p, &len));
    NLG_CHECK(host && count == len, "nlg_vec_set_field: count %lld != field length %lld", (long long)count, (long long)len);
    NLG_HIP(hipMemcpyAsync(p, host, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, self->mesh->ctx->stream));
    NLG_HIP(hipStreamSynchronize(self->mesh->ctx->stream));
    return 0;
}

int nlg_vec_get_field(const nlg_vec *self, int field, int irst, double *host, int64_t count) {
    double *p;
    int64_t len;
    NLG_TRY(field_ptr(self, field, irst, &p, &len));
    NLG_CHECK(host && count == len, "nlg_vec_get_field: count %lld != field length %lld", (long long)count, (long long)len);
    NLG_HIP(hipMemcpyAsync(host, p, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, self->mesh->ctx->stream));
    NLG_HIP(hipStreamSynchronize(self->mesh->ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Krylov basis
// ------------------------------------------------------------------------------------------------
int nlg_basis_create(nlg_mesh *mesh, int nscal, int lorder, int nvec, nlg_basis **out) {
    NLG_CHECK(mesh && out, "nlg_basis_create: NULL argument");
    NLG_CHECK(nvec >= 1 && nvec <= 4096, "nlg_basis_create: nvec %d out of range", nvec);
    nlg_basis *b = new nlg_basis();
    b->mesh = mesh;
    b->nvec = nvec;
    b->nscal = nscal;
    b->lorder = lorder;
    const int ncomp = mesh->dim + nscal;
    const int64_t main_len = (int64_t)ncomp * mesh->lvs + mesh->lps;
    b->stride = main_len * lorder;
    NLG_HIP(hipSetDevice(mesh->ctx->device));
    const size_t bytes = sizeof(double) * (size_t)b->stride * nvec;
    hipError_t e = hipMalloc(&b->d, bytes);
    if (e != hipSuccess) {
        delete b;
        set_error("nlg_basis_create: hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return 1;
    }
    NLG_HIP(hipMemsetAsync(b->d, 0, bytes, mesh->ctx->stream));
    NLG_HIP(hipMalloc(&b->d_h, sizeof(double) * nlg_basis::h_len(nvec)));
    NLG_HIP(hipMemsetAsync(b->d_h, 0, sizeof(double) * nlg_basis::h_len(nvec), mesh->ctx->stream));
    NLG_TRY(reduce_ws_reserve(mesh->ctx, nvec + 8));
    b->views.resize(nvec);
    for (int i = 0; i < nvec; ++i) {
        nlg_vec *v = new nlg_vec();
        v->mesh = mesh;
        v->nscal = nscal;
        v->lorder = lorder;
        v->ncomp = ncomp;
        v->main_len = main_len;
        v->total_len = b->stride;
        v->d = b->d + (int64_t)i * b->stride;
        v->owns = false;
        b->views[i] = v;
    }
    *out = b;
    return 0;
}

int nlg_basis_destroy(nlg_basis *b) {
    if (!b) return 0;
    for (auto *v : b->views) delete v;
    if (b->d) hipFree(b->d);
    if (b->d_h) hipFree(b->d_h);
    delete b;
    return 0;
}

int nlg_basis_vec(nlg_basis *b, int i, nlg_vec **out) {
    NLG_CHECK(b && out, "nlg_basis_vec: NULL argument");
    NLG_CHECK(i >= 0 && i < b->nvec, "nlg_basis_vec: index %d out of range [0,%d)", i, b->nvec);
    *out = b->views[i];
    return 0;
}

}  // extern "C"

namespace nlg {

// the tail of every reduction here: `rows` rows of `per` partial sums in the reduction workspace -> out[0:rows], all-reduced (ONE
// collective, whatever the rows stand for), optionally acc += out.  One rank: the accumulation rides in the row reduction, and the
// collective is counted all the same (nlg_counters)
static int reduce_rows_all(nlg_ctx *ctx, int rows, int per, double *out, double *acc) {
    hipStream_t st = ctx->stream;
    if (ctx->distributed()) {
        NLG_LAUNCH(k_reduce_rows, dim3(rows), dim3(NT), 0, st, ctx->d_partial, per, out, 0, (double *)nullptr);
        NLG_TRY(allreduce_sum(ctx, out, rows));
        if (acc) NLG_LAUNCH(k_vadd, dim3((rows + 255) / 256), dim3(256), 0, st, acc, out, rows);
    } else {
        ++g_collectives;
        NLG_LAUNCH(k_reduce_rows, dim3(rows), dim3(NT), 0, st, ctx->d_partial, per, out, acc ? 1 : 0, acc);
    }
    return 0;
}

// the lanes of a call: w[l] against columns of the basis b[l] (the struct travels whole: the spare entries repeat lane 0)
static LaneVW lanes_of(int s, const nlg_basis *const *b, nlg_vec *const *w) {
    LaneVW P;
    for (int l = 0; l < kMaxLanes; ++l) {
        const int u = l < s ? l : 0;
        P.V[l] = b[u]->d, P.w[l] = w[u]->d, P.nrst[l] = w[u]->nrst;
    }
    return P;
}
static LaneVW one_lane(const nlg_basis *b, const nlg_vec *w) {
    nlg_vec *wl = const_cast<nlg_vec *>(w);
    return lanes_of(1, &b, &wl);
}
static int max_nrst(int s, const LaneVW &P) { return *std::max_element(P.nrst, P.nrst + s); }

// device-resident block projection of s lanes: d_out[l * k + j] = V_{l,j}^T B w_l (allreduced, one collective for all lanes);
// optionally d_acc += d_out.  b0: any of the bases (they agree in shape)
static int lanes_block_dot(const nlg_basis *b0, int s, const LaneVW &P, int k, double *d_out, double *d_acc) {
    nlg_mesh *m = b0->mesh;
    nlg_ctx *ctx = m->ctx;
    const nlg_vec *v0 = b0->views[0];
    constexpr int KB = 8;
    const int nblk = dot_nblk(v0), nper = nblk * v0->ncomp;
    NLG_TRY(reduce_ws_reserve(ctx, s * k));
    ProfScope ps(ctx, P_BLOCKDOT);
    const dim3 g(chunk_tile_grid(nblk, (k + KB - 1) / KB), v0->ncomp * s);
    if (stream_basis(k, v0->main_len))
        NLG_LAUNCH((k_block_dot<KB, true>), g, dim3(NT), 0, ctx->stream, P, b0->stride, k, v0->ncomp, (const double *)m->d_bm1, m->lvs, nblk,
                   nper, ctx->d_partial);
    else
        NLG_LAUNCH((k_block_dot<KB, false>), g, dim3(NT), 0, ctx->stream, P, b0->stride, k, v0->ncomp, (const double *)m->d_bm1, m->lvs, nblk,
                   nper, ctx->d_partial);
    NLG_TRY(reduce_rows_all(ctx, s * k, nper, d_out, d_acc));
    NLG_HIP(hipGetLastError());
    return 0;
}

// w_l += sign * V_l h_l of s lanes, the history blocks as `hist` says (k_block_axpy); d_q (may be null): the squared norms by
// whose inv_norm the updated entries are scaled.  HIST_ONLY without a history block in any lane: no launch
static int lanes_block_axpy(const nlg_basis *b0, int s, const LaneVW &P, int k, const double *d_h, const double *d_hh, int hist,
                            double sign, const double *d_q = nullptr) {
    nlg_ctx *ctx = b0->mesh->ctx;
    const int64_t n2 = b0->views[0]->main_len / 2;
    const int mr = max_nrst(s, P);
    if (hist == HIST_ONLY && mr == 0) return 0;
    const int64_t n2all = hist == HIST_SWEEP ? n2 * (1 + mr) : hist == HIST_ONLY ? n2 * mr : n2;
    ProfScope ps(ctx, P_BLOCKAXPY);
    const bool ntl = stream_basis(k, 2 * n2);
#define BAX(T_, N_) NLG_LAUNCH((k_block_axpy<T_, N_>), dim3(grid_for(n2all), s), dim3(NT), sizeof(double) * 2 * k, ctx->stream, P, b0->stride, k, \
                               d_h, d_hh, n2, hist, sign, d_q)
    if (hist == HIST_ONLY) {
        if (ntl) BAX(true, true);
        else BAX(true, false);
    } else {
        if (ntl) BAX(false, true);
        else BAX(false, false);
    }
#undef BAX
    NLG_HIP(hipGetLastError());
    return 0;
}

// what a whole-vector update does to the history of w: consistent mode combines the history of the basis, literal mode repeats the
// main block's correction (nlg_set_axpby_rst_consistent)
static int hist_mode() { return g_axpby_consistent ? HIST_SWEEP : HIST_MAIN; }

// CGS2 of ONE vector, consistent mode, k >= 24: the first subtraction and the second projection in one sweep over the LAST kf <= 128
// basis vectors (k_block_axpy_dot); the k0 = k - kf vectors before them are subtracted first and projected after.  h holds the
// first-pass coefficients; on return h2 the second-pass ones and h the sum.
// (measured, CGS2 + norm + scale at 10^4 elements: k = 64: 6.29 -> 4.94 ms, 32: 3.28 -> 2.79, 16: 1.78 -> 1.88,
// 8: 1.04 -> 1.46 — the fully unrolled KMAX = 64 kernel does all 128 FMAs whatever k — hence the lower bound)
static int cgs2_fused_sweep(const nlg_basis *b, int k, nlg_vec *w, double *h, double *h2) {
    nlg_ctx *ctx = b->mesh->ctx;
    const nlg_vec *v0 = b->views[0];
    const LaneVW P = one_lane(b, w);
    // k <= 64: one register tile (k_block_axpy_dot<64>); up to 128: two tiles, the second parked in LDS (k_block_axpy_dot2<64>)
    const int kf = std::min(k, 128);
    const int k0 = k - kf;
    const int64_t nv = (int64_t)v0->ncomp * b->mesh->lvs;   // velocity (+ scalar) part; the pressure follows
    const int G = 256;                                     // one block per CU (one wave per SIMD)
    NLG_TRY(reduce_ws_reserve(ctx, k));
    if (k0 > 0) NLG_TRY(lanes_block_axpy(b, 1, P, k0, h, nullptr, HIST_NONE, -1.0));
    const double *Vf = b->d + (int64_t)k0 * b->stride;
    {
        ProfScope ps(ctx, P_AXPYDOT);
        if (kf > 64) {
            constexpr size_t lds2 = sizeof(double) * (2 * 64 + 64 * NT);
            static bool attr_set = false;
            if (!attr_set) {
                NLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_block_axpy_dot2<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
                attr_set = true;
            }
            NLG_LAUNCH(k_block_axpy_dot2<64>, dim3(G), dim3(NT), lds2, ctx->stream, Vf, b->stride, kf, (const double *)(h + k0), w->d,
                       (const double *)b->mesh->d_bm1, b->mesh->lvs, nv, ctx->d_partial);
        } else {
            NLG_LAUNCH(k_block_axpy_dot<64>, dim3(G), dim3(NT), 0, ctx->stream, Vf, b->stride, kf, (const double *)(h + k0), w->d,
                       (const double *)b->mesh->d_bm1, b->mesh->lvs, nv, ctx->d_partial);
        }
    }
    {
        ProfScope ps(ctx, P_BLOCKAXPY);
        const int64_t np2 = (w->main_len - nv) / 2;        // pressure part of the main block: subtraction only
        if (np2 > 0) {
            LaneVW Pp = {};
            Pp.V[0] = Vf + nv, Pp.w[0] = w->d + nv;
            if (stream_basis(kf, w->main_len))
                NLG_LAUNCH((k_block_axpy<false, true>), dim3(grid_for(np2)), dim3(NT), sizeof(double) * 2 * kf, ctx->stream, Pp, b->stride, kf,
                           (const double *)(h + k0), (const double *)nullptr, np2, (int)HIST_NONE, -1.0, (const double *)nullptr);
            else
                NLG_LAUNCH((k_block_axpy<false, false>), dim3(grid_for(np2)), dim3(NT), sizeof(double) * 2 * kf, ctx->stream, Pp, b->stride, kf,
                           (const double *)(h + k0), (const double *)nullptr, np2, (int)HIST_NONE, -1.0, (const double *)nullptr);
        }
    }
    NLG_TRY(reduce_rows_all(ctx, kf, G, h2 + k0, h + k0));
    if (k0 > 0) NLG_TRY(lanes_block_dot(b, 1, P, k0, h2, h));
    return 0;
}

// CGS2 + norm + scale of s vectors, each against its own basis, everything stream-ordered on device.  Results in b[0]'s workspace:
// h1() coefficients [s][k], hnorm(s, k) the |w_l|^2 before normalisation.
// Consistent mode touches the history blocks of w ONCE.  No inner product reads them, so both subtractions and the scale can wait
// until the norm is known:
//   1. projection, first subtraction, second projection on the main block (three launches, or the fused sweep of one vector at
//      k >= 24), then the second subtraction on the main block alone (H2);
//   2. |w|^2 of the main block (k_dot_partial + row reduction);
//   3. ONE launch over the history blocks: w_hist <- fl(w_hist - V_hist (H1 + H2)) * inv_norm(|w|^2), lane by lane with its own
//      number of blocks and its own norm (nothing for a lane, or a call, without history);
//   4. the scale of the main block.
// Every stored value is what a sweep over all blocks followed by a scale of all blocks gives, bit for bit (the subtraction is
// rounded before the product either way); the history is read and written once instead of twice.
// Literal mode repeats the main block's correction in the history, which ties the two together: sweep, sweep, norm, scale of all.
static int basis_cgs2_dev(int s, nlg_basis *const *b, int k, nlg_vec *const *w) {
    nlg_basis *b0 = b[0];
    nlg_mesh *m = b0->mesh;
    nlg_ctx *ctx = m->ctx;
    double *H1 = b0->h1(), *H2 = b0->h2(), *Q = b0->hnorm(s, k);
    const LaneVW P = lanes_of(s, b, w);
    const bool split = k > 0 && g_axpby_consistent;   // the history waits for the norm (step 3)
    if (k > 0) {
        NLG_TRY(lanes_block_dot(b0, s, P, k, H1, nullptr));
        if (g_axpby_consistent) {
            // the second block_dot accumulates H2 into H1: H1 = the sum of both passes, what the history receives
            if (s == 1 && k >= 24) {
                NLG_TRY(cgs2_fused_sweep(b0, k, w[0], H1, H2));
            } else {
                NLG_TRY(lanes_block_axpy(b0, s, P, k, H1, nullptr, HIST_NONE, -1.0));
                NLG_TRY(lanes_block_dot(b0, s, P, k, H2, H1));
            }
            NLG_TRY(lanes_block_axpy(b0, s, P, k, H2, nullptr, HIST_NONE, -1.0));
        } else {
            NLG_TRY(lanes_block_axpy(b0, s, P, k, H1, nullptr, HIST_MAIN, -1.0));
            NLG_TRY(lanes_block_dot(b0, s, P, k, H2, H1));
            NLG_TRY(lanes_block_axpy(b0, s, P, k, H2, nullptr, HIST_MAIN, -1.0));
        }
    }
    const nlg_vec *v0 = b0->views[0];
    const int nblk = dot_nblk(v0), nper = nblk * v0->ncomp;
    const int64_t n2 = v0->main_len / 2;
    LaneAB A;
    for (int l = 0; l < kMaxLanes; ++l) A.a[l] = A.b[l] = P.w[l];
    NLG_LAUNCH(k_dot_partial, dim3(nblk, v0->ncomp, s), dim3(NT), 0, ctx->stream, A, (const double *)m->d_bm1, m->lvs, nblk, nper,
               ctx->d_partial);
    NLG_TRY(reduce_rows_all(ctx, s, nper, Q, nullptr));
    if (split) NLG_TRY(lanes_block_axpy(b0, s, P, k, H1, nullptr, HIST_ONLY, -1.0, Q));
    NLG_LAUNCH(k_scal_dev, dim3(grid_for(split ? n2 : n2 * (1 + max_nrst(s, P))), s), dim3(NT), 0, ctx->stream, P, (const double *)Q, n2,
               split ? 0 : 1);
    NLG_HIP(hipGetLastError());
    return 0;
}

// basis_cgs2_dev and ONE read-back for all lanes: lane l's k coefficients to h[l * hstride + 0:k], its norm to beta[l * bstride]
int basis_cgs2_host(int s, nlg_basis *const *b, int k, nlg_vec *const *w, double *h, int64_t hstride, double *beta, int64_t bstride) {
    NLG_TRY(basis_cgs2_dev(s, b, k, w));
    std::vector<double> tmp((size_t)s * k + s);   // (hnorm lies right behind the coefficients)
    hipStream_t st = b[0]->mesh->ctx->stream;
    NLG_HIP(hipMemcpyAsync(tmp.data(), b[0]->h1(), sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, st));
    NLG_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < s; ++l) {
        for (int j = 0; j < k; ++j) h[l * hstride + j] = tmp[(size_t)l * k + j];
        beta[l * bstride] = sqrt(tmp[(size_t)s * k + l]);
    }
    return 0;
}

}  // namespace nlg

extern "C" {

int nlg_basis_cgs2_batch(int s, nlg_basis *const *b, int k, nlg_vec *const *w, double *h, int ldh, double *beta) {
    NLG_CHECK(b && w && h && beta, "nlg_basis_cgs2_batch: NULL argument");
    NLG_CHECK(s >= 1 && s <= kMaxLanes, "nlg_basis_cgs2_batch: %d lanes unsupported (1..%d)", s, kMaxLanes);
    for (int l = 0; l < s; ++l) NLG_CHECK(b[l] && w[l], "nlg_basis_cgs2_batch: NULL basis or vector in lane %d", l);
    NLG_CHECK(k >= 0 && k <= b[0]->nvec, "nlg_basis_cgs2_batch: k=%d out of range [0,%d]", k, b[0]->nvec);
    NLG_CHECK(ldh >= k, "nlg_basis_cgs2_batch: ldh=%d too small for k=%d", ldh, k);
    for (int l = 0; l < s; ++l) {
        NLG_CHECK(b[l]->mesh == b[0]->mesh && b[l]->nscal == b[0]->nscal && b[l]->lorder == b[0]->lorder && b[l]->nvec == b[0]->nvec,
                  "nlg_basis_cgs2_batch: the bases differ in shape (lane %d)", l);
        NLG_TRY(check_same(b[l]->views[0], w[l], "nlg_basis_cgs2_batch"));
        for (int u = 0; u < l; ++u) NLG_CHECK(b[l] != b[u] && w[l] != w[u], "nlg_basis_cgs2_batch: the same basis or vector in two lanes");
        for (int u = 0; u < s; ++u)
            NLG_CHECK(!(w[l]->d >= b[u]->d && w[l]->d < b[u]->d + (int64_t)k * b[u]->stride),
                      "nlg_basis_cgs2_batch: the vector of lane %d is one of the columns 0..%d it is orthogonalised against", l, k - 1);
    }
    return nlg::basis_cgs2_host(s, b, k, w, h, ldh, beta, 1);
}

// d = <u^+, u^> = (a_r . u_r + a_i . u_i) + i (a_r . u_i - a_i . u_r): the four dots as four lanes of the first stage, one row
// reduction, ONE all-reduce and one read-back (a real pair: one dot)
int nlg_sens_pairing(const nlg_vec *dir_re, const nlg_vec *dir_im, const nlg_vec *adj_re, const nlg_vec *adj_im, double *d) {
    NLG_CHECK(dir_re && adj_re && d, "nlg_sens_pairing: NULL argument");
    NLG_CHECK((dir_im != nullptr) == (adj_im != nullptr), "nlg_sens_pairing: %s given without %s", dir_im ? "dir_im" : "adj_im",
              dir_im ? "adj_im" : "dir_im");
    NLG_TRY(check_same(dir_re, adj_re, "nlg_sens_pairing"));
    if (dir_im) {
        NLG_TRY(check_same(dir_re, dir_im, "nlg_sens_pairing"));
        NLG_TRY(check_same(dir_re, adj_im, "nlg_sens_pairing"));
    }
    nlg_mesh *m = dir_re->mesh;
    nlg_ctx *ctx = m->ctx;
    const int rows = dir_im ? 4 : 1;
    const int nblk = dot_nblk(dir_re), nper = nblk * dir_re->ncomp;
    LaneAB P = {};
    P.a[0] = adj_re->d, P.b[0] = dir_re->d;
    if (dir_im) {
        P.a[1] = adj_im->d, P.b[1] = dir_im->d;
        P.a[2] = adj_re->d, P.b[2] = dir_im->d;
        P.a[3] = adj_im->d, P.b[3] = dir_re->d;
    }
    NLG_TRY(reduce_ws_reserve(ctx, rows));
    NLG_LAUNCH(k_dot_partial, dim3(nblk, dir_re->ncomp, rows), dim3(NT), 0, ctx->stream, P, (const double *)m->d_bm1, m->lvs, nblk, nper,
               ctx->d_partial);
    NLG_TRY(reduce_rows_all(ctx, rows, nper, ctx->d_scalars, nullptr));
    NLG_HIP(hipGetLastError());
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    NLG_TRY(scalars_to_host(ctx, 0, rows, q));
    d[0] = q[0] + q[1], d[1] = q[2] - q[3];
    return 0;
}

int nlg_basis_block_dot(const nlg_basis *b, int k, const nlg_vec *w, double *h) {
    NLG_CHECK(b && w && h, "nlg_basis_block_dot: NULL argument");
    NLG_CHECK(k >= 1 && k <= b->nvec, "nlg_basis_block_dot: k=%d out of range [1,%d]", k, b->nvec);
    NLG_TRY(check_same(b->views[0], w, "nlg_basis_block_dot"));
    NLG_TRY(nlg::lanes_block_dot(b, 1, nlg::one_lane(b, w), k, b->h1(), nullptr));
    NLG_HIP(hipMemcpyAsync(h, b->h1(), sizeof(double) * k, hipMemcpyDeviceToHost, b->mesh->ctx->stream));
    NLG_HIP(hipStreamSynchronize(b->mesh->ctx->stream));
    return 0;
}

int nlg_basis_block_axpy(const nlg_basis *b, int k, const double *h, nlg_vec *w) {
    NLG_CHECK(b && w && h, "nlg_basis_block_axpy: NULL argument");
    NLG_CHECK(k >= 1 && k <= b->nvec, "nlg_basis_block_axpy: k=%d out of range [1,%d]", k, b->nvec);
    NLG_TRY(check_same(b->views[0], w, "nlg_basis_block_axpy"));
    NLG_HIP(hipMemcpyAsync(b->h1(), h, sizeof(double) * k, hipMemcpyHostToDevice, b->mesh->ctx->stream));
    NLG_TRY(nlg::lanes_block_axpy(b, 1, nlg::one_lane(b, w), k, b->h1(), nullptr, nlg::hist_mode(), -1.0));
    NLG_HIP(hipStreamSynchronize(b->mesh->ctx->stream));
    return 0;
}

int nlg_basis_cgs2(const nlg_basis *bc, int k, nlg_vec *w, double *h, double *beta) {
    nlg_basis *b = const_cast<nlg_basis *>(bc);
    NLG_CHECK(b && w && h && beta, "nlg_basis_cgs2: NULL argument");
    NLG_CHECK(k >= 0 && k <= b->nvec, "nlg_basis_cgs2: k=%d out of range [0,%d]", k, b->nvec);
    NLG_TRY(check_same(b->views[0], w, "nlg_basis_cgs2"));
    return nlg::basis_cgs2_host(1, &b, k, &w, h, 0, beta, 0);
}

// Block classical Gram-Schmidt with re-orthogonalisation for the s consecutive columns k .. k+s-1 against the columns
// 0 .. k-1, followed by a Cholesky QR (twice) among the s columns themselves; see include/neklab_gpu.h.
int nlg_basis_block_cgs2(nlg_basis *b, int k, int s, double *coef) {
    NLG_CHECK(b && coef, "nlg_basis_block_cgs2: NULL argument");
    NLG_CHECK(s >= 1 && s <= 4, "nlg_basis_block_cgs2: block size %d unsupported (1..4)", s);
    NLG_CHECK(k >= 0 && k + s <= b->nvec, "nlg_basis_block_cgs2: columns %d..%d outside the basis (nvec=%d)", k, k + s - 1, b->nvec);
    NLG_CHECK(g_axpby_consistent, "nlg_basis_block_cgs2: the block path implements the consistent restart-history update only");
    nlg_ctx *ctx = b->mesh->ctx;
    hipStream_t st = ctx->stream;
    const int ld = k + s;
    if (s == 1) {   // the single-vector path, same output convention
        std::vector<double> h(std::max(k, 1));
        double beta = 0.0;
        NLG_TRY(nlg_basis_cgs2(b, k, b->views[k], h.data(), &beta));
        for (int j = 0; j < k; ++j) coef[j] = h[j];
        coef[k] = beta;
        return 0;
    }
    nlg_vec *w0 = b->views[k];
    int nrst = 0;
    for (int v = 0; v < s; ++v) nrst = std::max(nrst, b->views[k + v]->nrst);
    for (int v = 0; v < s; ++v) {
        // the sweeps below run over the main block and `nrst` history blocks of EVERY column: a column that carries fewer (a
        // freshly drawn one next to an x0 with a restart history) gets zeros there, not whatever its memory held
        nlg_vec *c = b->views[k + v];
        if (c->nrst < nrst)
            NLG_HIP(hipMemsetAsync(c->d + (int64_t)(1 + c->nrst) * c->main_len, 0, sizeof(double) * (size_t)((nrst - c->nrst) * c->main_len), st));
        c->nrst = nrst;
    }
    b->last_block_rank = s;
    double *W = w0->d;
    double *H1 = b->h1(), *H2 = b->h2(), *dG = b->gram(), *dT = b->tmat();
    const int nblk = dot_nblk(w0), nper = nblk * w0->ncomp;
    const int64_t n2 = w0->main_len / 2, n2all = n2 * (1 + nrst);
    constexpr int KB = 8;
    NLG_TRY(reduce_ws_reserve(ctx, std::max(k, s) * s));
    auto dots = [&](const double *V, int kk, double *out, double *acc) -> int {
        ProfScope ps(ctx, P_BLOCKDOT);
        const dim3 g(chunk_tile_grid(nblk, (kk + KB - 1) / KB), w0->ncomp);
#define BD(S_) NLG_LAUNCH((k_block_dot_s<KB, S_>), g, dim3(NT), 0, st, V, b->stride, kk, (const double *)W, b->stride, \
                                  (const double *)b->mesh->d_bm1, b->mesh->lvs, nblk, nper, ctx->d_partial)
        if (s == 2) BD(2);
        else if (s == 3) BD(3);
        else BD(4);
#undef BD
        return nlg::reduce_rows_all(ctx, kk * s, nper, out, acc);
    };
    auto axpy = [&](const double *h, const double *hh, int64_t n, int64_t blk2) -> int {
        ProfScope ps(ctx, P_BLOCKAXPY);
        const size_t lds = sizeof(double) * 2 * (size_t)k * s;
#define BA(S_) NLG_LAUNCH((k_block_axpy_s<S_>), dim3(grid_for(n)), dim3(NT), lds, st, (const double *)b->d, b->stride, k, h, hh, W, \
                                  b->stride, n, blk2, -1.0)
        if (s == 2) BA(2);
        else if (s == 3) BA(3);
        else BA(4);
#undef BA
        return 0;
    };
    if (k > 0) {
        NLG_TRY(dots(b->d, k, H1, nullptr));
        NLG_TRY(axpy(H1, nullptr, n2, n2));          // first pass: main block only
        NLG_TRY(dots(b->d, k, H2, H1));              // H1 <- H1 + H2
        NLG_TRY(axpy(H2, H1, n2all, n2));            // second pass: H2 on the main block, the sum on the history blocks
    }
    // Cholesky QR among the s new columns, twice.  A (numerically) dependent column -- a block Krylov space that has reached an
    // invariant subspace, the "lucky breakdown" of converged eigenvalues, or a drawn column close to x0 -- is not an error: what is
    // left of it after the projections is below the rounding level of what it was, so it is DEFLATED: its coefficients on the
    // columns before it go into R as for any column, its diagonal entry of R is 0 and the column itself becomes the zero vector
    // (harmless in every later projection).  b->last_block_rank = number of columns kept; nlg_eigs stops expanding the space when
    // it falls below s, as it does at beta = 0 in the single-vector iteration.
    // Two tests, both relative to what the column was when the step that can lose it began: (1) against the BASIS -- the squared
    // norm a column brought to this call is what is left of it plus the squares of its coefficients on the (orthonormal) basis,
    // |w|^2 = |w - V h|^2 + |h|^2; CGS2 leaves a remainder of about eps |w| of a column that lies in span(V), so a remainder below
    // 1e-12 |w| (1e-24 on the squares) is rounding noise, whatever the other columns of the block look like; (2) among the columns
    // of the block -- the Cholesky pivot against the diagonal entry at entry to the CURRENT round (the second round sees
    // normalised columns: a threshold carried over from the first would deflate any healthy column that came in with a norm above 1e7).
    double R[4][4] = {};
    for (int a = 0; a < s; ++a) R[a][a] = 1.0;
    bool dep[4] = {false, false, false, false};
    double hsq[4] = {0.0, 0.0, 0.0, 0.0};   // |h_v|^2: squared norm of the part of column v that the projections removed
    std::vector<double> hs((size_t)std::max(k, 1) * s);
    if (k > 0) {
        NLG_HIP(hipMemcpyAsync(hs.data(), H1, sizeof(double) * (size_t)k * s, hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
        for (int v = 0; v < s; ++v)
            for (int j = 0; j < k; ++j) hsq[v] += hs[(size_t)j * s + v] * hs[(size_t)j * s + v];
    }
    for (int round = 0; round < 2; ++round) {
        NLG_TRY(dots(W, s, dG, nullptr));
        double G[16];
        NLG_HIP(hipMemcpyAsync(G, dG, sizeof(double) * s * s, hipMemcpyDeviceToHost, st));
        NLG_HIP(hipStreamSynchronize(st));
        double L[4][4] = {};
        for (int i = 0; i < s; ++i) {
            NLG_CHECK(std::isfinite(G[i * s + i]), "nlg_basis_block_cgs2: column %d is not finite", k + i);
            const double gin = G[i * s + i];   // squared norm of column i at entry to this round
            if (round == 0 && !(gin > 1e-24 * (gin + hsq[i]))) dep[i] = true;   // nothing left of it beside span(V)
            for (int j = 0; j <= i; ++j) {
                double a = G[i * s + j];
                for (int q = 0; q < j; ++q) a -= L[i][q] * L[j][q];
                if (i == j) {
                    // the pivot is the squared norm of column i after the columns before it have been projected out: a block with
                    // condition number above ~1e7 loses it to rounding (CholQR works on the SQUARED condition number)
                    if (dep[i] || !(a > 1e-14 * gin) || !(gin > 0.0)) {
                        dep[i] = true;
                        L[i][i] = 0.0;
                    } else {
                        L[i][i] = std::sqrt(a);
                    }
                } else {
                    L[i][j] = dep[j] ? 0.0 : a / L[j][j];
                }
            }
        }
        // Rr = L^T (upper); T = Rr^-1 (upper, back substitution column by column); W <- W T; R <- Rr R.  A deflated column takes a
        // unit pivot in the inverse and a zero column in T afterwards: W T then holds the zero vector in its place.
        double T[4][4] = {};
        for (int c = 0; c < s; ++c) {
            T[c][c] = dep[c] ? 1.0 : 1.0 / L[c][c];
            for (int r = c - 1; r >= 0; --r) {
                double a = 0.0;
                for (int q = r + 1; q <= c; ++q) a += L[q][r] * T[q][c];
                T[r][c] = dep[r] ? -a : -a / L[r][r];
            }
        }
        for (int c = 0; c < s; ++c)
            if (dep[c])
                for (int r = 0; r < s; ++r) T[r][c] = 0.0;
        double Tf[16], Rn[4][4] = {};
        for (int a = 0; a < s; ++a)
            for (int c = 0; c < s; ++c) {
                Tf[a * s + c] = T[a][c];
                for (int q = 0; q < s; ++q) Rn[a][c] += L[q][a] * R[q][c];
            }
        memcpy(R, Rn, sizeof(R));
        NLG_HIP(hipMemcpyAsync(dT, Tf, sizeof(double) * s * s, hipMemcpyHostToDevice, st));
        {
            ProfScope ps(ctx, P_BLOCKAXPY);
#define BR(S_) NLG_LAUNCH((k_block_rmul<S_>), dim3(grid_for(n2all)), dim3(NT), 0, st, W, b->stride, (const double *)dT, n2all)
            if (s == 2) BR(2);
            else if (s == 3) BR(3);
            else BR(4);
#undef BR
        }
        NLG_HIP(hipStreamSynchronize(st));   // Tf lives on this stack frame
    }
    for (int v = 0; v < s; ++v)
        if (dep[v]) --b->last_block_rank;
    for (int v = 0; v < s; ++v) {
        for (int j = 0; j < k; ++j) coef[(size_t)v * ld + j] = hs[(size_t)j * s + v];
        for (int a = 0; a < s; ++a) coef[(size_t)v * ld + k + a] = R[a][v];
    }
    NLG_HIP(hipGetLastError());
    return 0;
}

int nlg_basis_last_block_rank(const nlg_basis *b, int *rank) {
    NLG_CHECK(b && rank, "nlg_basis_last_block_rank: NULL argument");
    *rank = b->last_block_rank;
    return 0;
}

int nlg_basis_combine(const nlg_basis *b, int k, const double *c, nlg_vec *out) {
    NLG_CHECK(b && c && out, "nlg_basis_combine: NULL argument");
    NLG_CHECK(k >= 1 && k <= b->nvec, "nlg_basis_combine: k=%d out of range [1,%d]", k, b->nvec);
    NLG_TRY(check_same(b->views[0], out, "nlg_basis_combine"));
    NLG_TRY(nlg_vec_zero(out));
    if (g_axpby_consistent) {
        // consistent history: the combination carries the combined history slots of the basis vectors
        int nr = 0;
        for (int j = 0; j < k; ++j) nr = std::max(nr, b->views[j]->nrst);
        out->nrst = nr;
    }
    NLG_HIP(hipMemcpyAsync(b->h1(), c, sizeof(double) * k, hipMemcpyHostToDevice, b->mesh->ctx->stream));
    NLG_TRY(nlg::lanes_block_axpy(b, 1, nlg::one_lane(b, out), k, b->h1(), nullptr, nlg::hist_mode(), +1.0));
    NLG_HIP(hipStreamSynchronize(b->mesh->ctx->stream));
    return 0;
}

}  // extern "C"
