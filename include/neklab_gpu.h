/*
 * neklab_gpu.h -- C ABI of the MI355X-native hot path of nekStab/neklab.
 *
 * Drop-in boundary: the reference consumes this path through Fortran 2008 type-bound
 * procedures of LightKrylov's abstract_vector_rdp / abstract_exptA_linop_rdp.  A Fortran shim
 * (neklab_amd/fortran/neklab_vectors.f90, neklab_linops.f90, neklab_utils.f90; bind(C) interfaces in neklab_gpu_capi.f90) extends
 * those abstract types under the reference's module and type names and forwards every binding to one
 * entry point of this header through ISO_C_BINDING.  Each declaration cites the reference interface
 * (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - every function returns int: 0 = ok, non-zero = error (text in nlg_last_error()).  The reference
 *     has no status codes on the vector API and aborts through type_error / stop_error
 *     (src/vectors/real_vectors.f90:202-204, src/neklab_nek_setup.f90:406-417); the shim turns a
 *     non-zero return into stop_error.
 *   - handles are opaque; all field data lives in HBM and is owned by the library.
 *   - host arrays handed in are plain double / int64_t arrays in Nek5000's element-major layout
 *     ijke = ix + n*(iy + n*(iz + n*e))   (src/vectors/real_vectors.f90:69).
 *   - single-threaded per rank, every call collective across ranks (SURVEY.md §8b "Threading").
 *   - there is NO CPU fallback: every entry point fails with an error if no HIP device is usable.
 */
#ifndef NEKLAB_GPU_H
#define NEKLAB_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nlg_ctx nlg_ctx;     /* device + stream + communicator                                   */
typedef struct nlg_mesh nlg_mesh;   /* SEM discretisation: what Nek5000 keeps in SIZE/TOTAL commons     */
typedef struct nlg_vec nlg_vec;     /* nek_dvector  (src/vectors/neklab_vectors.f90:26-50)               */
typedef struct nlg_basis nlg_basis; /* array of nek_dvector as LightKrylov allocates for the Krylov basis */
typedef struct nlg_linop nlg_linop; /* exptA_linop  (src/linops/neklab_linops.f90:35-44)                 */

/* field selectors for nlg_vec_set_field / nlg_vec_get_field */
enum { NLG_VX = 0, NLG_VY = 1, NLG_VZ = 2, NLG_PR = 3, NLG_THETA = 4 /* + scalar index */ };

/* ---------------------------------------------------------------------------------------------- */
/* context                                                                                          */
/* ---------------------------------------------------------------------------------------------- */
const char *nlg_last_error(void);
int nlg_version(void);
int nlg_ctx_create(int device, nlg_ctx **out);
int nlg_ctx_destroy(nlg_ctx *ctx);
int nlg_ctx_sync(nlg_ctx *ctx);
/* RCCL communicator over xGMI: rank 0 calls nlg_comm_unique_id, the 128 bytes are broadcast by the
 * host program (MPI_Bcast in a Nek5000 host, torch.distributed in bench.py), every rank then calls
 * nlg_ctx_comm_init.  Replaces the MPI_Allreduce inside glsc3 (src/vectors/real_vectors.f90:217-224) and gslib's gs_op
 * behind opdssum (real_vectors.f90:100-104): per gather-scatter the library sums the groups that hold a dof another rank
 * shares, packs, exchanges (grouped ncclSend / ncclRecv), sums the interior groups and unpacks; with NLG_HALO_OVERLAP=1 in
 * the environment the exchange runs on a side stream beside the interior groups. */
int nlg_comm_unique_id(void *out128);
int nlg_ctx_comm_init(nlg_ctx *ctx, int rank, int nranks, const void *unique_id128);
int nlg_ctx_rank(const nlg_ctx *ctx, int *rank, int *nranks);
/* VALIDATION transport, not a product path: the same four collectives staged through a POSIX shared-memory
 * segment `name` (slot_bytes per rank), so that several ranks can share ONE GPU — which RCCL refuses — and the
 * whole distributed path except the RCCL calls themselves can be tested on a one-GPU box
 * (tests/test_gpu_multirank.py).  Every wait times out with an error after 120 s. */
int nlg_ctx_comm_init_shm(nlg_ctx *ctx, int rank, int nranks, const char *name, int64_t slot_bytes);
/* Host-side planning step of the multi-rank gather-scatter (gslib's gs_setup behind opdssum,
 * src/vectors/real_vectors.f90:100): given the ascending unique labels of every rank, concatenated rank after
 * rank (counts[q] each), return for `rank` the labels it shares with every other rank (neigh_counts[q], and the
 * labels themselves in shared_out, neighbour after neighbour, ascending).  Pure host code, no GPU needed.
 * Returns the total number of shared entries, or -1 if `capacity` is too small. */
int64_t nlg_halo_plan(int rank, int nranks, const int64_t *counts, const int64_t *labels_concat,
                      int64_t *neigh_counts, int64_t *shared_out, int64_t capacity);
/* The two remaining pure-host steps of that set-up, exported so that the index lists the GPU exchange uses can be
 * checked on the CPU with emulated ranks (tests/test_cpu_dist.py): the ascending unique labels of the element-boundary
 * dofs of one rank (its contribution to labels_concat; returns their number, -1 if capacity is too small), and the
 * lists themselves -- send_idx[e] = local dof packed for entry e of the send buffer (entries ordered neighbour after
 * neighbour, labels ascending), and per shared label l < *nlab_out the positions rpos[roff[l]:roff[l+1]] of the received
 * contributions and the local copies cidx[coff[l]:coff[l+1]] that receive their sum.  Returns the number of entries. */
int64_t nlg_halo_boundary_labels(int n, int dim, int64_t E, const int64_t *glo, int64_t *labels_out, int64_t capacity);
int64_t nlg_halo_lists(int n, int dim, int64_t E, const int64_t *glo, int rank, int nranks, const int64_t *counts,
                       const int64_t *labels_concat, int64_t *neigh_counts, int32_t *send_idx, int64_t cap_send,
                       int32_t *roff, int32_t *rpos, int32_t *coff, int32_t *cidx, int64_t cap_copies, int64_t *nlab_out);
/* Per-kernel-class timing with HIP events recorded on the launch stream (the reference's counterpart
 * is LightKrylov's timer object, src/neklab_analysis.f90:66-67, :98-101).  Classes: "axhelm", "gs",
 * "opgradt", "opdiv", "colmul", "block_dot", "block_axpy", "cg_vec", "conv", "vec_ops". */
int nlg_prof_enable(nlg_ctx *ctx, int class_mask); /* bit i = class i in the order above; -1 = all; 0 = off */
/* time only every stride-th launch of an enabled class (default 1): a pair of events around a 50-us kernel costs ~12 us of
 * stream time, so timing every launch of the dominant class would slow the run it measures by 2 %; nlg_prof_get then returns
 * the number of TIMED launches and their total */
int nlg_prof_sample(nlg_ctx *ctx, int stride);
int nlg_prof_reset(nlg_ctx *ctx);
int nlg_prof_get(nlg_ctx *ctx, const char *name, int64_t *count, double *total_ms);
/* Running totals since the library was loaded: kernel launches issued, and collective sites passed (all-reduce, all-gather and
 * gather-scatter / Schwarz halo exchanges -- counted on one rank too, where they move nothing: what a partitioned run of the same
 * calls issues).  bench.py reports the difference over its timed region per step.  The reference's counterpart: every glsc3 /
 * gs_op / nekgsync inside nek_advance, which it does not count. */
int nlg_counters(int64_t *launches, int64_t *collectives);

/* ---------------------------------------------------------------------------------------------- */
/* mesh: replaces the Nek5000 commons the reference reads through include "SIZE"/"TOTAL"            */
/* (src/vectors/neklab_vectors.f90:8-14: lx1, lelv, lv, lp; real_vectors.f90: xm1, ym1, zm1, bm1,   */
/*  vmult, v1mask..v3mask, lglel; gather-scatter handle behind opdssum/dsavg :100-104)              */
/* ---------------------------------------------------------------------------------------------- */
typedef struct nlg_mesh_desc {
    int dim;                /* ldim: 2 or 3                                           */
    int n;                  /* lx1 (= ly1 = lz1 in 3-D); pressure mesh is lx2 = n - 2 */
    int lxd;                /* dealiasing points, 0 => 3*n/2                          */
    int64_t nelv;           /* local element count                                    */
    const double *xm1;      /* [nelv * n^dim] GLL coordinates                         */
    const double *ym1;
    const double *zm1;      /* NULL in 2-D                                            */
    const int64_t *glo_num; /* [nelv * n^dim] global (assembled) dof labels           */
    const int64_t *lglel;   /* [nelv] global element ids (0-based), NULL => 0..nelv-1 */
    const double *v1mask;   /* [nelv * n^dim] Dirichlet masks, 0/1                    */
    const double *v2mask;
    const double *v3mask;   /* NULL in 2-D                                            */
    const double *tmask;    /* NULL => no scalar mask                                 */
    int has_outflow;        /* 0 => pressure defined up to a constant (Nek ifvcor)    */
} nlg_mesh_desc;

int nlg_mesh_create(nlg_ctx *ctx, const nlg_mesh_desc *desc, nlg_mesh **out);
int nlg_mesh_destroy(nlg_mesh *mesh);
int nlg_mesh_sizes(const nlg_mesh *mesh, int64_t *lvn, int64_t *lpn, int *dim, int *n);
/* read back a derived array by name for verification: "bm1", "binvm1", "vmult", "jac", "bm2",
 * "g11".."g33" (Nek g1m1..g6m1 ordering by index pair), "rxm1"... (as "rst11".."rst33");
 * 3-D: "slot_fg", "slot_xp" = the slot of each natural point of an element in the face-grouped / slab-permuted layout (lx1^3 values) */
int nlg_mesh_get(const nlg_mesh *mesh, const char *name, double *out, int64_t count);
/* *out = 1 if single-vector launches of the pressure operator (opgradt, opdiv) on this mesh take the matrix-pipe kernels: 3-D, lx1 = 8,
 * at least NLG_SMALL_E local elements, NLG_POP_MFMA not 0 */
int nlg_mesh_pop_mfma(const nlg_mesh *mesh, int *out);

/* ---------------------------------------------------------------------------------------------- */
/* nek_dvector                                                                                      */
/* ---------------------------------------------------------------------------------------------- */
/* type(nek_dvector) storage, src/vectors/neklab_vectors.f90:26-36; nscal = active scalars (ifto /
 * ifpsco), lorder as in SIZE (restart history holds lorder-1 slots). */
int nlg_vec_create(nlg_mesh *mesh, int nscal, int lorder, nlg_vec **out);
int nlg_vec_destroy(nlg_vec *v);
/* Handle lifetimes for host languages whose objects are copied bit by bit behind the type's back (the reference's vectors are
 * plain static arrays: src/vectors/neklab_vectors.f90:26-36; Fortran intrinsic assignment / sourced allocation / reallocation on
 * assignment duplicate a shim object together with its handle).  The owner's finaliser RELEASES instead of destroying; a copy
 * that is used later ADOPTS: *status = 1 -- the handle had been released and now belongs to the caller (nothing copied, nothing
 * leaked); *status = 0 -- it is still owned by a live object: the caller clones.  `gen` is the generation number the caller read
 * when it last owned or copied the handle (nlg_vec_generation): a handle that was freed in between is an error, not a crash.
 * Released buffers are freed oldest first above nlg_vec_pool_limit bytes (default 32 GiB), when an allocation fails, and by
 * nlg_vec_pool_trim.  nlg_vec_destroy frees at once, as before (hosts with reference semantics: the Python mirror). */
int nlg_vec_generation(const nlg_vec *v, int64_t *gen);
int nlg_vec_release(nlg_vec *v);
int nlg_vec_adopt(nlg_vec *v, int64_t gen, int *status);
/* A copy that only READS (an intent(in) use cannot take ownership) pins a released handle: it leaves the eviction pool and stays
 * adoptable; the finaliser of a non-owning copy un-pins (back into the pool).  Both validate `gen` like nlg_vec_adopt. */
int nlg_vec_pin(nlg_vec *v, int64_t gen);
int nlg_vec_unpin(nlg_vec *v, int64_t gen);
int nlg_vec_pool_limit(int64_t bytes);
int nlg_vec_pool_trim(int64_t *freed_bytes);
/* Fortran intrinsic assignment / sourced allocation of a nek_dvector */
int nlg_vec_clone(const nlg_vec *src, nlg_vec **out);
int nlg_vec_copy(nlg_vec *dst, const nlg_vec *src);
/* nek_dzero   src/vectors/real_vectors.f90:37-50   (interface neklab_vectors.f90:65-67) */
int nlg_vec_zero(nlg_vec *self);
/* nek_drand   real_vectors.f90:52-123   (interface :69-72); seed replaces the compiler RNG */
int nlg_vec_rand(nlg_vec *self, int ifnorm, uint64_t seed);
/* The two halves of nek_drand, exported so that each can be compared with the oracle on its own: the mth_rand noise
 * (neklab_vectors.f90:305-314) added to every active field, real_vectors.f90:62-98 -- and the part that makes the
 * field admissible: opdssum * vmult, dsavg, bcdirvc / bcdirsc, optional normalisation, nrst = 0 (:100-122).
 * nlg_vec_rand = noise + finish. */
int nlg_vec_rand_noise(nlg_vec *self, uint64_t seed);
int nlg_vec_rand_finish(nlg_vec *self, int ifnorm);
/* nek_dscal   real_vectors.f90:125-160  (interface :74-77) */
int nlg_vec_scal(nlg_vec *self, double alpha);
/* nek_daxpby  real_vectors.f90:162-206  (interface :79-84): self = alpha*vec + beta*self */
int nlg_vec_axpby(double alpha, const nlg_vec *vec, double beta, nlg_vec *self);
/* nek_ddot    real_vectors.f90:208-233  (interface :86-89): globally reduced, same on all ranks */
int nlg_vec_dot(const nlg_vec *self, const nlg_vec *vec, double *out);
/* %norm() inherited from abstract_vector_rdp, used at real_vectors.f90:117 */
int nlg_vec_norm(const nlg_vec *self, double *out);
/* nek_dsize   real_vectors.f90:235-247  (interface :91-93) */
int nlg_vec_size(const nlg_vec *self, int64_t *out);
/* the same as a plain function value (-1: NULL handle): the reference declares nek_dsize `pure`
 * (neklab_vectors.f90:91-93), and a pure Fortran function can only call interfaces that are themselves pure */
int64_t nlg_vec_size_value(const nlg_vec *self);
/* dhas_rst_fields as a plain function value for the same reason: the reference declares it `pure` (neklab_vectors.f90:107-110) */
int nlg_vec_has_rst_value(const nlg_vec *self);
/* the two plain-value forms for handles that may be stale (the Fortran shim's bitwise copies): -1 when the handle is unknown or
 * its generation is not `gen`; they never dereference a freed handle */
int64_t nlg_vec_size_checked(const nlg_vec *self, int64_t gen);
int nlg_vec_has_rst_checked(const nlg_vec *self, int64_t gen);
/* outpost_dnek  src/neklab_utils.f90:305-333 (Nek5000 `outpost(vx, vy, vz, pr, t, prefix)`): one vector -> one Nek5000
 * field file at `path` ("#std" header, fp64): GLL coordinates when with_coords != 0 (Nek5000 writes them into the first
 * file of a series only), velocity, the pressure mapped to the velocity mesh (Nek5000's `mappr` for a Pn-Pn-2 run), the
 * first scalar if the vector carries one.  Single rank. */
int nlg_vec_outpost(const nlg_vec *self, const char *path, int with_coords, double time, int istep);
/* dsave_rst / dget_rst / dhas_rst_fields / dclear_rst_fields  real_vectors.f90:249-346 (irst 1-based) */
int nlg_vec_save_rst(nlg_vec *self, const nlg_vec *vec_rst, int irst);
int nlg_vec_get_rst(const nlg_vec *self, nlg_vec *vec_rst, int irst);
int nlg_vec_has_rst_fields(const nlg_vec *self, int *out);
int nlg_vec_clear_rst_fields(nlg_vec *self);
int nlg_vec_nrst(const nlg_vec *self, int *out);
/* nek2vec / vec2nek  src/neklab_utils.f90:84-134 (nopcopy :279-301): move one field between a host
 * array and the vector.  field = NLG_VX.., irst = 0 main field, 1..lorder-1 history slot. */
int nlg_vec_set_field(nlg_vec *self, int field, int irst, const double *host, int64_t count);
int nlg_vec_get_field(const nlg_vec *self, int field, int irst, double *host, int64_t count);
/* Restart history in axpby / block updates.
 * 1 (default): history slot r of self receives alpha * (history slot r of vec).
 * 0           : literal reading of real_vectors.f90:188-192: every slot receives alpha * vec's MAIN field.
 * The literal reading does not reproduce the reference's own known answer (cylinder Re = 50, |mu_1| = 1.0156
 * +- 1e-4, test/neklabTests.py:43-45): it gives 1.0194 (dt = 0.01) / 1.0177 (dt = 0.005), an O(dt) pollution of
 * the BDF start-up of every matvec, while mode 1 gives 1.01578 independent of dt.
 * Process-wide switch. */
int nlg_set_axpby_rst_consistent(int flag);

/* ---------------------------------------------------------------------------------------------- */
/* Krylov basis: what LightKrylov's allocate(X(kdim+1)) + innerprod / linear_combination do with     */
/* k separate dot/axpby calls (call sites src/neklab_analysis.f90:5-8, :77-81), as block kernels     */
/* ---------------------------------------------------------------------------------------------- */
int nlg_basis_create(nlg_mesh *mesh, int nscal, int lorder, int nvec, nlg_basis **out);
int nlg_basis_destroy(nlg_basis *b);
int nlg_basis_vec(nlg_basis *b, int i, nlg_vec **out); /* borrowed view of column i (0-based) */
/* h[0:k] = V(:,0:k)^T B w   (LightKrylov innerprod(X(1:k), w); k allreduces fused into one) */
int nlg_basis_block_dot(const nlg_basis *b, int k, const nlg_vec *w, double *h);
/* w -= V(:,0:k) h           (LightKrylov linear_combination + axpby loop) */
int nlg_basis_block_axpy(const nlg_basis *b, int k, const double *h, nlg_vec *w);
/* classical Gram-Schmidt with one re-orthogonalisation pass, then norm and scale:
 * h[0:k] accumulated coefficients, *beta = ||w|| before normalisation */
int nlg_basis_cgs2(const nlg_basis *b, int k, nlg_vec *w, double *h, double *beta);
/* The same for s <= 4 vectors, EACH against its own basis: for every lane l what nlg_basis_cgs2(b[l], k, w[l], h + l*ldh,
 * beta + l) does (restart history and pressure as in the consistent history update, a zero norm leaves a zero vector), with
 * the lane in the grid of every kernel: one launch per stage and one all-reduce per reduction (k*s, then s values) for all
 * lanes.  The bases have equal shape (mesh, nscal, lorder, nvec) and are distinct; no w[l] may be one of the columns 0 .. k-1
 * of any of them; the w[l] may differ in their number of valid history levels.  nlg_basis_cgs2 is this call with one lane, so
 * s = 1 equals it bit for bit at every k: one lane takes the fused subtraction-and-projection sweep from k = 24.  Several
 * lanes take the separate kernels at every k: below k = 24 every lane equals its single call bit for bit, from there on to
 * rounding.  nlg_set_axpby_rst_consistent(0) holds for the lanes as for a single vector (same kernels). */
int nlg_basis_cgs2_batch(int s, nlg_basis *const *b, int k, nlg_vec *const *w, double *h, int ldh, double *beta);
/* Block variant for s <= 4 NEW vectors held in the consecutive columns k .. k+s-1 (block Arnoldi, BASELINE.json config 5;
 * the reference advances several perturbations together through Nek5000's lpert / npert, src/neklab_nek_setup.f90:39-247,
 * src/neklab_otd.f90:37-49): classical Gram-Schmidt with one re-orthogonalisation pass against the columns 0 .. k-1 --
 * every pass reads the basis ONCE for all s vectors -- then a Cholesky QR (applied twice) among the s columns.
 * coef is column-major with leading dimension k+s, one column per new vector: rows 0 .. k-1 the projection coefficients
 * (both passes summed), rows k .. k+s-1 the upper-triangular factor R with  W_old = V(:,0:k) coef(0:k,:) + W_new R.
 * Restart history and pressure follow as in axpby / scal (consistent history update only). */
int nlg_basis_block_cgs2(nlg_basis *b, int k, int s, double *coef);
/* Number of columns the last nlg_basis_block_cgs2 on this basis kept.  A column is deflated -- not an error: its coefficients are
 * returned as for any column with a zero diagonal entry in R, and the column becomes the zero vector -- when (1) what the two
 * projections left of it is below 1e-12 of the norm it came with (|w|^2 = |w - V h|^2 + |h|^2: the column lies in span(V) to
 * rounding; the block Krylov space has reached an invariant subspace), or (2) its Cholesky pivot among the columns of the block falls
 * below 1e-14 of its squared norm at entry to the current round of the twofold CholQR (dependent on the columns before it).  The
 * tests are scale-free: columns of any norm may be passed. */
int nlg_basis_last_block_rank(const nlg_basis *b, int *rank);
/* out = sum_j c[j] V(:,j)  over ALL fields (eigenvector reconstruction, LightKrylov eigs tail) */
int nlg_basis_combine(const nlg_basis *b, int k, const double *c, nlg_vec *out);

/* ---------------------------------------------------------------------------------------------- */
/* exptA_linop                                                                                      */
/* ---------------------------------------------------------------------------------------------- */
typedef struct nlg_exptA_config {
    double tau;        /* abstract_exptA_linop_rdp%tau; exptA_linop(1.0_dp, bf) in 1cyl.usr:20       */
    double re;         /* 1/viscosity; 1cyl.par: viscosity = -50                                      */
    double cfl_limit;  /* 0.5 at src/linops/exponential_propagator.f90:12                             */
    double vtol;       /* Helmholtz residual tolerance (param(22), neklab_nek_setup.f90:228)          */
    double ptol;       /* pressure residual tolerance  (param(21), neklab_nek_setup.f90:227)          */
    double dt;         /* > 0: fixed dt, skips the CFL rule (recompute_dt = .false. branch, :218-220) */
    int torder;        /* |param(27)|: 1cyl.par timeStepper = bdf3                                    */
    int maxit_v;
    int maxit_p;
    int fixed_iters_v; /* > 0: run exactly this many PCG iterations (parity / benchmarking mode)      */
    int fixed_iters_p;
    int pprecond;      /* pressure preconditioner: 0 = two-level Schwarz (element FDM with one layer of face overlap
                          where it is set up -- 3-D lx1 <= 12 except 11, 2-D lx1 <= 8 -- + vertex coarse space),
                          1 = Jacobi, 2 = two-level without overlap                                                 */
    int pproj;         /* pressure residual projection onto the previous increments of the matvec (Nek5000
                          `residualProj = yes`, examples/cylinder/stability/direct/1cyl.par:23): 0 = off, 1 = on    */
    int ifheat;        /* Boussinesq coupling with one scalar (temperature): the vectors carry theta (nscal = 1), the base
                          flow its base temperature.  rhocp (d/dt + U.grad) theta + rhocp u.grad Theta = conductivity
                          lap theta, momentum forcing buoy[i] * theta -- Nek5000's [TEMPERATURE] block and the buoyancy of
                          the case's userf (examples/rayBen/baseflow/rayBen.par:39-45, rayBen.usr:77-103).  rmatvec
                          integrates the adjoint of the coupled operator in the velocity + temperature inner product:
                          u+_t = L_u^+ u+ - theta+ grad Theta,  rhocp theta+_t = rhocp U.grad theta+ + conductivity lap
                          theta+ + rhocp buoy . u+   (exponential_propagator_temp.f90:62-107).                       */
    double conductivity;
    double rhocp;
    double buoy[3];
    int no_history;    /* 1: no restart history -- every matvec starts impulsively (BDF1, then BDF2, ...) from vec_in alone and
                          fills no history slots: vec_in's slots are ignored, vec_out%nrst = 0, vectors of lorder = 1 are accepted.
                          The reference always carries lorder - 1 history copies (src/vectors/neklab_vectors.f90:26-36,
                          exponential_propagator.f90:44,52), which triples the memory of every Krylov vector; this switch is the
                          memory plan for bases that do not fit otherwise (DESIGN.md "memory plan"): the propagator it defines is a
                          slightly different discretisation of exp(tau L) (start-up at first order: +4e-5 in the cylinder's leading
                          multiplier), but ONE linear map for every column of the Arnoldi relation.  0 (default): the reference's
                          protocol. */
    double filter_weight; /* Nek5000's explicit modal filter (`filtering = explicit`, `filterWeight`; e.g. examples/back_fstep/
                          transient_growth/bfs.par): > 0: at the end of every time step the velocity of every lane, and the temperature
                          with ifheat, become (F x F [x F]) u element by element, F = Phi diag(d) Phi^-1 in the basis L_0, L_1,
                          L_{k-1} - L_{k-3} with d = 1 - filter_weight ((k - k0) / filter_modes)^2 on the last filter_modes modes
                          (DESIGN.md 3.2).  The pressure is never filtered; the same F serves direct, adjoint, nonlinear and forced
                          integration.  0 (default): off -- the time step is launch for launch the unfiltered one.  Range [0, 1];
                          kernels exist for lx1 = 6, 8, 10 (and 12 in 3-D). */
    int filter_modes;  /* number of attenuated modes (what Nek5000's .par reader derives from `filterCutoffRatio`), 1 .. lx1 - 2;
                          read only when filter_weight > 0 */
} nlg_exptA_config;

int nlg_exptA_config_default(nlg_exptA_config *cfg);
/* exptA_linop(tau, baseflow) constructor (1cyl.usr:20); baseflow is copied (held by value in the
 * reference, neklab_linops.f90:36) */
int nlg_linop_create(nlg_mesh *mesh, const nlg_exptA_config *cfg, const nlg_vec *baseflow, nlg_linop **out);
int nlg_linop_destroy(nlg_linop *op);
/* init_exptA  src/linops/exponential_propagator.f90:4-13: dt / nsteps from CFL, solver set-up */
int nlg_linop_init(nlg_linop *op);
/* exptA_matvec  exponential_propagator.f90:15-60   (interface neklab_linops.f90:52-56) */
int nlg_linop_matvec(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out);
/* exptA_rmatvec exponential_propagator.f90:62-107  (interface neklab_linops.f90:58-62) */
int nlg_linop_rmatvec(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out);
/* s <= 4 vectors through the propagator TOGETHER (vec_out[v] = exp(tau L) vec_in[v], transpose != 0: the adjoint), time
 * step by time step: what Nek5000 does with npert > 1 perturbations (src/neklab_nek_setup.f90:39-247, src/neklab_otd.f90:
 * 37-49).  The s velocity solves and the s pressure solves run as independent PCGs in lockstep (own scalars and
 * convergence flag per vector: every vector gets exactly the iteration of nlg_linop_matvec), with the operator
 * applications of an iteration issued together, so that metric factors, base-flow fields of the convective term and
 * preconditioner data are read once per iteration for all vectors.  Each vector keeps its restart-history protocol
 * (replay of vec_in's history, history of vec_out).  Round 4: also with cfg.ifheat (the scalar's solve is lane-batched like the
 * velocity's: exponential_propagator_temp.f90:15-60, :62-107) and with a wavenumber projection (exptA_proj_linop: every projection
 * of the single-vector path applied lane by lane against the operator's tables, exponential_propagator_proj.f90:30-75). */
int nlg_linop_matvec_block(nlg_linop *op, int s, const nlg_vec *const *vec_in, nlg_vec *const *vec_out, int transpose);
/* Newton-Krylov base-flow solver.
 * nonlinear_map  src/systems/fixed_point.f90:4-38 : vec_out = Phi_tau(vec_in) - vec_in with the nonlinear integrator,
 *   time step from the CFL number of vec_in (cfg.cfl_limit; the reference uses 0.4), tolerances cfg.vtol / cfg.ptol.
 *   Afterwards the operator's base-flow dependent set-up belongs to vec_in.
 * set_baseflow   the `self%X` of jac_exptA_matvec (fixed_point.f90:52): replaces the frozen base flow of the linearised
 *   operator and redoes init (dt / nsteps from its CFL number); the Jacobian of the map is then matvec - identity.
 * set_tolerances the tolerance schedulers nek_constant_tol / nek_dynamic_tol (src/systems/neklab_systems.f90:229-335). */
int nlg_linop_nonlinear_map(nlg_linop *op, const nlg_vec *vec_in, nlg_vec *vec_out);
int nlg_linop_set_baseflow(nlg_linop *op, const nlg_vec *baseflow);
int nlg_linop_set_tolerances(nlg_linop *op, double vtol, double ptol);
/* Wavenumber-projected propagator (exptA_proj_linop, src/linops/neklab_linops.f90:130-152,
 * exponential_propagator_proj.f90): after this call matvec / rmatvec project the initial condition and the final state
 * onto the cos(alpha x_idir) / sin(alpha x_idir) content along the homogeneous direction idir (1-based):
 * u <- cv <2 u cv> + sv <2 u sv> with the bm1-weighted average <.> over every line of points along that direction
 * (proj_alpha, :135-173).  line_label[i] identifies the line of local velocity dof i (what Nek5000's gtpp_gs_setup
 * derives from nelx, nely, nelz).  line_label2 / x2 (both or neither): the same for the pressure mesh, with the
 * coordinate along idir of every pressure point -- the pressure is then projected as well (bm2 weights); the reference
 * projects the velocity only, see DESIGN.md for why that is not enough behind an inner product that ignores the
 * pressure.  Several ranks: the labels are GLOBAL line names (the same line carries the same label on every rank
 * that holds a part of it); the weighted sums are all-reduced, as the reference's planar_avg is a global operation
 * (exponential_propagator_proj.f90:146-169).  A block run (nlg_linop_matvec_block) projects all its lanes onto alpha in
 * one launch per level, several ranks: one all-reduce for all lanes; a single run is the block of one.
 * nlg_linop_project applies the projection to the state held by a vector. */
int nlg_linop_set_projection(nlg_linop *op, double alpha, int idir, const int64_t *line_label, const int64_t *line_label2,
                             const double *x2);
int nlg_linop_project(nlg_linop *op, nlg_vec *v);
/* Wavenumber lanes: one wavenumber per lane of a block run, for sweeps over alpha (dispersion relations, neutral curves) in
 * lock-step.  nlg_linop_set_projection_lanes is nlg_linop_set_projection with nalpha = 1 .. 4 wavenumbers (same preconditions,
 * same optional pressure-mesh pair, swapped in on success only): the lines are built once and shared, the cos / sin tables
 * exist once per lane (each the table a single-alpha operator builds, bit for bit).  Afterwards lane l of
 * nlg_linop_matvec_block (s <= nalpha vectors) projects onto alpha[l] wherever a projected run projects -- initial condition,
 * replayed history states, final state with its lagged levels, pressure -- by the kernels and the driver of
 * nlg_linop_set_projection, which differ only in the table a lane reads: each lane has the result a single-alpha operator
 * at alpha[l] gives, bit for bit.  nlg_linop_matvec / rmatvec / nlg_linop_project are the block of one and use alpha[0].  A later
 * nlg_linop_set_projection returns the operator to one alpha for all lanes; calling this again replaces the set (fewer
 * lanes: a sweep retires the wavenumbers that have converged).  Refused: nalpha outside 1..4, a NULL alpha, orbit mode, a
 * live nlg_otd, cfg.ifheat (the projection does not touch the scalar); on such an operator: a block run of more than nalpha
 * vectors and nlg_linop_integrate_forced*.  nlg_otd_create and nlg_linop_set_orbit refuse it as they refuse any projection.
 * nlg_linop_project_block: v[l] <- P_{alpha[l]} v[l] for s <= nalpha distinct vectors. */
int nlg_linop_set_projection_lanes(nlg_linop *op, int nalpha, const double *alpha, int idir, const int64_t *line_label,
                                   const int64_t *line_label2, const double *x2);
int nlg_linop_project_block(nlg_linop *op, int s, nlg_vec *const *v);
/* Resolvent operator by time stepping (resolvent_linop, src/linops/resolvent.f90): the building
 * block of evaluate_rhs (:80-111) and evaluate_imaginary_part (:133-166): vec_out = state after the nsteps of one
 * application started from `ic` (NULL: rest, zero pressure) under the body force Re[(f_re + i f_im) exp(i s omega t)]
 * (velocity fields of f_re / f_im; f_im may be NULL), s = +1 direct, -1 adjoint; the force enters the explicit term and
 * is evaluated at the time level each step starts from.  The driver (real part through GMRES on I - exp(tau L), imaginary
 * part from a quarter period) lives on the host: neklab_amd/host.py resolvent_linop. */
int nlg_linop_integrate_forced(nlg_linop *op, const nlg_vec *ic, const nlg_vec *f_re, const nlg_vec *f_im, double omega, int adjoint,
                               nlg_vec *vec_out);
/* s <= 4 forced integrations TOGETHER, as the lanes of one block run (evaluate_rhs / evaluate_imaginary_part of
 * src/linops/resolvent.f90:80-111, :133-166 for s forcings at once; Nek5000 advances npert > 1 perturbations the same way,
 * src/neklab_nek_setup.f90:39-247, src/neklab_otd.f90:37-49, see nlg_linop_matvec_block).  Lane v starts from ic[v] (ic == NULL or a
 * NULL entry: rest, zero pressure), is forced by Re[(f_re[v] + i f_im[v]) exp(i s omega t)] (f_im == NULL or a NULL entry: a real
 * forcing) and is stored into vec_out[v] exactly as the single call stores its result: forcing at the time level each step starts
 * from, no restart-history replay, no history in the result.  omega, the adjoint flag and the operator's dt / nsteps are shared;
 * every kernel of a time step, the forcing included, is launched once for all lanes, and each lane performs the iterations of the
 * single call, which is the block of one.  Refused: what nlg_linop_integrate_forced refuses (orbit mode, a live nlg_otd, vectors
 * with scalars, a foreign mesh, no nlg_linop_init), s outside 1 .. 4, a NULL f_re[v] or vec_out[v], an output that is also an
 * input of any lane, the same output twice.  The block resolvent built on it lives on the host: neklab_amd/host.py
 * resolvent_linop.matvec_block, resolvent_analysis. */
int nlg_linop_integrate_forced_block(nlg_linop *op, int s, const nlg_vec *const *ic, const nlg_vec *const *f_re,
                                     const nlg_vec *const *f_im, double omega, int adjoint, nlg_vec *const *vec_out);
/* Coupled (orbit) mode: the propagator about a base flow that moves in time -- the monodromy operator of a periodic orbit, whose
 * eigenvalues are its Floquet multipliers (the time stepper under the reference's periodic-orbit Jacobian,
 * src/systems/periodic_orbit.f90:59-92: setup_linear_solver(solve_baseflow = .true., endtime = period)).
 * nlg_linop_set_orbit(op, X0, period): X0 (copied) becomes the state the base flow starts every matvec from, tau = period, dt / nsteps
 *   by the usual rule applied to X0 (cfg.cfl_limit, or cfg.dt when positive).  From then on a matvec advances, in the same time
 *   steps and the same kernel launches, the base flow U by the nonlinear step (impulsive start from X0, explicit term
 *   -1/2 lns_conv(U^n; U^n)) and the 1 .. 3 perturbations by the step linearised about U^n, the level the step starts from (explicit
 *   term -lns_conv(U^n; u^n)); the fine-mesh factors of U^n are built once per step for all of them.  BDF / EXT order
 *   min(istep, torder) for every lane; the perturbations replay their restart history as in nlg_linop_matvec, the base flow does
 *   not; the history steps after the result advance the base flow as well.  With cfg.no_history and a fixed cfg.dt this is the exact
 *   derivative of the discrete map of nlg_linop_nonlinear_map.  nlg_linop_matvec, nlg_linop_matvec_block (s <= 3), nlg_arnoldi_step,
 *   nlg_block_arnoldi_step and nlg_eigs work on such an operator unchanged.  Refused with a message that names the mode:
 *   nlg_linop_rmatvec / transpose (the adjoint of a time-dependent linearisation needs U(T - t); the reference's forward-run adjoint,
 *   periodic_orbit.f90:117-183, is not reproduced on purpose), cfg.ifheat, the wavenumber projection, nlg_linop_integrate_forced,
 *   nlg_linop_set_tau, nlg_linop_set_baseflow, nlg_linop_nonlinear_map.  X0 = NULL (period ignored) leaves the mode: the operator is
 *   the frozen propagator about X0 over tau = period again.
 * nlg_linop_orbit_end(op, out): the base flow after the nsteps of the last matvec, before the history steps: Phi_T(X0), so that
 *   |out - X0| tells how well the orbit closes.
 * nlg_linop_lane_iters: Helmholtz and pressure iterations of one lane in the last run on the operator, whatever kind it was (a matvec
 *   or block, nlg_linop_integrate_forced, nlg_linop_nonlinear_map, nlg_upo_residual, an OTD run): of its time step istep (1-based,
 *   the history steps of a matvec follow the nsteps), or summed over its steps for istep = 0; in orbit mode the base flow is the lane
 *   after the last perturbation.  Valid for any operator.  (nlg_linop_get_stats sums over the lanes, the base-flow lane included.)
 * nlg_linop_pcg_z_free: *out = 1 if the velocity PCG of this operator does not store z = M^-1 r (the Helmholtz kernel forms it from the
 *   residual, 1 / diag and one mask byte per point while it updates the search direction), 0 if it stores it: before nlg_linop_init,
 *   in 2-D, with NLG_PCG_SINGLE_RED=1, NLG_PC_MASKB=0 or NLG_PCG_STORE_Z=1 in the environment when the operator was initialised.  Same
 *   results either way. */
int nlg_linop_set_orbit(nlg_linop *op, const nlg_vec *X0, double period);
int nlg_linop_orbit_end(nlg_linop *op, nlg_vec *out);
int nlg_linop_lane_iters(const nlg_linop *op, int lane, int istep, int64_t *v_iters, int64_t *p_iters);
int nlg_linop_pcg_z_free(const nlg_linop *op, int *out);
/* Periodic orbits: Newton-Krylov for the state X0 and the period T (nek_ext_dvector, src/vectors/real_extended_vectors.f90;
 * nek_upo_system / nek_upo_jacobian, src/systems/periodic_orbit.f90, neklab_systems.f90:147-223).  Every entry point below works on an
 * operator in orbit mode and refuses any other with a message that names nlg_linop_set_orbit.  One perturbation per call; no adjoint.
 * nlg_linop_set_orbit_steps: nlg_linop_set_orbit with a fixed step count, dt = period / nsteps; nsteps = 0 is nlg_linop_set_orbit itself
 *   (CFL rule with cfg.cfl_limit, or cfg.dt).  A Newton iteration calls it with its new (X, T); the count is held through the
 *   iteration's GMRES, so that the residual does not jump where ceil() does (the reference recomputes it in every call,
 *   periodic_orbit.f90:63-69).
 * nlg_upo_residual: out = Phi_T(X0) - X0, pressure included (nonlinear_map_UPO, :4-45): the base-flow lane alone through the nonlinear
 *   step with the operator's dt / nsteps; equal to orbit_end - X0 of a coupled matvec on the same operator.
 * nlg_upo_fdot: the two time derivatives of the base flow (the reference's compute_fdot), taken from the last run -- any coupled matvec
 *   or nlg_upo_residual -- and kept by the operator.  which = 0: f0 = (U^1 - U^0) / dt from the first step, compute_fdot at X0
 *   literally (one impulsive first-order step; velocity and pressure).  which = 1: fT = the BDF-k derivative of the base flow at level
 *   nsteps, k = min(nsteps, torder), from the time levels of the last step -- the derivative the scheme itself uses, at no extra time
 *   step (the reference restarts impulsively from X(T): DESIGN.md 8); its pressure part is the first difference (p^N - p^{N-1}) / dt,
 *   the one pressure level a step keeps.  An error before the first run.
 * nlg_upo_jac_matvec: the bordered Jacobian (jac_direct_map, :47-115): v_out = M v_in - v_in + t_in fT, *t_out = <f0, v_in> in the
 *   inner product of the vector space (velocity only); M = nlg_linop_matvec, unchanged.  nlg_upo_border: the border alone on w = M v_in
 *   (in place) -- one fused pass when neither vector carries restart history (and composed == 0), else the vector operations
 *   sub / axpby / dot, whose history semantics then apply.
 * nlg_upo_arnoldi_step: nlg_upo_jac_matvec on column k of the basis, whose period components live in the host array tcol[0 .. k+1],
 *   then CGS2 in the extended inner product <u, v> + t_u t_v; H(0:k+1, k) as nlg_arnoldi_step. */
int nlg_linop_set_orbit_steps(nlg_linop *op, const nlg_vec *X0, double period, int nsteps);
int nlg_upo_residual(nlg_linop *op, nlg_vec *out);
int nlg_upo_fdot(nlg_linop *op, int which, nlg_vec *out);
int nlg_upo_jac_matvec(nlg_linop *op, const nlg_vec *v_in, double t_in, nlg_vec *v_out, double *t_out);
int nlg_upo_border(nlg_linop *op, const nlg_vec *v_in, double t_in, nlg_vec *w, double *t_out, int composed);
int nlg_upo_arnoldi_step(nlg_linop *op, nlg_basis *basis, double *tcol, int k, double *H, int ldh);
/* Optimally time-dependent (OTD) modes (nek_otd, src/neklab_otd.f90; otd_analysis, src/neklab_analysis.f90:214-344): r <= 4
 * perturbations u_1 .. u_r, orthonormal in the inner product of the vector space, follow dU/dt = L(t) U - U C with C = Lr - Phi,
 * Lr_ij = <u_i, L u_j> and Phi skew-symmetric such that C is upper triangular (C_jj = Lr_jj, C_ij = Lr_ij + Lr_ji for i < j): mode j
 * is forced by the modes i <= j only.  The modes are lanes of the operator's block step; Lr comes from what the step has in memory
 * anyway (D^T p, (nu A + h2 B) u and the convective term of every lane: one reduction pass), the forcing -bm1 U C joins the explicit
 * term (extrapolated like the convective term), both without a copy to the host.  Steps before `startstep` are plain block steps.
 * After every step istep >= startstep with istep <= startstep + 10 or istep % orthostep == 0, and in nlg_otd_reduced, the lanes
 * are re-orthonormalised with T = chol(G)^-T, G_ij = <u_i, u_j>, applied to every stored level (velocities, pressure, explicit
 * terms); at creation twice.  DESIGN.md 3.2 "OTD mode"; section 8 lists where this departs from the reference's literal loop.
 *   create  op is initialised if it is not; dt by its usual rule (cfg.dt, or CFL with cfg.cfl_limit); impulsive start, order
 *           min(istep, torder).  basis0: r vectors (copied), NULL = nlg_vec_rand with seeds 1 .. r.  solve_baseflow (r <= 3): the
 *           operator's base flow becomes one more lane, advanced by the nonlinear step as in nlg_linop_set_orbit.  trans: the
 *           adjoint equations (frozen base flow only).  Refused with a message that names the reason: trans with solve_baseflow,
 *           cfg.ifheat, a wavenumber projection, an operator in orbit mode, r out of range, a second nlg_otd on the operator.
 *           While the nlg_otd lives, every matvec, set_*, init, integrate_forced and nonlinear_map call on op is refused, and so is
 *           nlg_linop_destroy (it returns an error and frees nothing: destroy the nlg_otd first).
 *   advance a Gram matrix that is not positive definite (dependent or non-finite modes) is an error of the call that met it.
 *   destroy after a run with solve_baseflow the operator's base-flow set-up is rebuilt from its own base flow: matvecs on op are
 *           what they were before the run.
 *   reduced orthonormalise, then evaluate Lr (column-major r x r) on the current state; G = the Gram matrix BEFORE that. */
typedef struct nlg_otd nlg_otd;
typedef struct nlg_otd_opts { int r; int startstep; int orthostep; int trans; int solve_baseflow; } nlg_otd_opts;
int nlg_otd_opts_default(nlg_otd_opts *o);                 /* r = 2, startstep = 1, orthostep = 10, trans = 0, solve_baseflow = 0 */
int nlg_otd_create(nlg_linop *op, const nlg_otd_opts *o, const nlg_vec *const *basis0, nlg_otd **out);
int nlg_otd_advance(nlg_otd *otd, int nsteps);
int nlg_otd_reduced(nlg_otd *otd, double *Lr, double *G);
int nlg_otd_get_basis(nlg_otd *otd, int i, nlg_vec *out);   /* i 0-based */
int nlg_otd_get_baseflow(nlg_otd *otd, nlg_vec *out);       /* its current state (the operator's base flow when it is frozen) */
int nlg_otd_info(const nlg_otd *otd, int64_t *istep, double *time, double *dt);
int nlg_otd_destroy(nlg_otd *otd);
/* History points (Nek5000's `hpts` with a .his file; examples/cylinder/dns/Re180/1cyl.his, 1cyl.usr: userchk).
 * nlg_probe_locate: pure host code, no GPU needed.  For every point x* = xyz[p] find the element e and the reference coordinates
 *   r in [-1, 1]^dim with x_e(r) = x*, x_e the Lagrange interpolant of xm1, ym1, zm1 on the GLL nodes.  Candidates: the elements whose
 *   GLL-node bounding box, grown by 10 % of its extent, holds the point.  Newton from the nearest GLL node of each candidate, every
 *   iterate clamped to [-1.5, 1.5], stopped at |dr|_inf <= 1e-13, given up after 50 iterations; a component of r within the stop of a
 *   face is set onto it.  status: 0 = found with |r|_inf <= 1; 1 = found with 1 < |r|_inf <= 1 + tol_r (points meant to lie on a curved
 *   wall, whose polynomial side is not the true curve): r is then clamped to the element; 2 = not found, elem = -1.  dist (may be NULL)
 *   = |x_e(r) - x*| of what is returned.  Several holders (a face, an edge, a vertex, a periodic seam): the smallest global element id
 *   lglel (NULL: 0 .. E-1) among the holders with status 0 wins, among those with status 1 if there is none: independent of the
 *   partition.  elem is the local index.  Returns non-zero for a bad argument (dim, n outside 2..16, NULL arrays, negative tol_r).
 * nlg_probes: the located points on the device -- per point the local element and the 1-D Lagrange weights at r (barycentric form,
 *   exact at a node) on the GLL nodes and on the Gauss nodes of the pressure mesh.  Several ranks: create is collective with the same
 *   points on every rank; the rank that holds the winning element owns the point (one all-reduce at creation), so that a point on a
 *   partition interface is sampled exactly once.  A point that no rank holds (status 2) is refused with a message that names it.
 *   status: the winner's status, global element id, r and dist, the same on every rank (any array may be NULL).
 *   sample: fields of s = 1..4 vectors at every point in ONE launch of k_probe_sample (one wave per point and vector, fixed summation
 *   order: bitwise reproducible, a vector in a call of several equals its single call, a point at a GLL node returns the nodal value):
 *   out[s][npts][nf], nf = dim + 1 (+ 1 with a scalar): velocity components, pressure (interpolated on the Gauss nodes), temperature.
 *   Several ranks: one all-reduce; every rank receives all values.
 * nlg_dns: a nonlinear run of the operator's time stepper as ONE continuous run (impulsive start from X0, BDF / EXT order min(istep,
 *   torder), cfg.filter_* as in every run), with two monitors evaluated on the device after every step: the fields at the history points
 *   and the recurrence norm d(t) = |u(t) - u_ref| in the nek_ddot inner product (velocity, temperature if carried; no pressure).
 *   create: X0 becomes the operator's base flow and the operator is initialised: dt = cfg.dt, or from the CFL rule at X0 (cfg.cfl_limit),
 *     as nlg_linop_nonlinear_map does, and fixed from then on.  Refused with a message: an operator in orbit mode, with a live nlg_otd or
 *     nlg_dns, with a wavenumber projection; X0 on another mesh or with the wrong number of scalars.  While the nlg_dns lives, every
 *     matvec, set_*, init, integrate_forced, nonlinear_map and nlg_otd_create on op is refused, and so is nlg_linop_destroy.
 *   set_probes / set_reference (ref NULL: the state as it stands; never called: no recurrence, dist = 0): the series starts again, with
 *     the state as it stands as its sample 0.  The points must outlive their use: nlg_probes_destroy refuses while they are attached.
 *   advance: sample 0 is the state the series starts from (X0 at t = 0 unless the monitors were changed later); every step appends one
 *     sample.  The monitors cost at most three launches per step and neither a host synchronisation nor a collective: samples go to a
 *     ring of `chunk` slots on the device, which is copied to the host series when it fills and by nlg_dns_series (several ranks: one
 *     all-reduce per copy).  The series does not depend on chunk.
 *   series: time[count], probe[count][npts][nf], dist[count] of the samples first .. first + count - 1 (any array may be NULL).
 *   destroy: the operator's base-flow set-up is rebuilt from X0: matvecs on op are the propagator about X0. */
int nlg_probe_locate(int dim, int n, int64_t E, const double *x, const double *y, const double *z, const int64_t *lglel, int64_t npts,
                     const double *xyz, double tol_r, int64_t *elem, double *rst, int *status, double *dist);
typedef struct nlg_probes nlg_probes;
int nlg_probes_create(nlg_mesh *mesh, int64_t npts, const double *xyz, double tol_r, nlg_probes **out);
int nlg_probes_status(const nlg_probes *p, int *status, int64_t *elem_global, double *rst, double *dist);
int nlg_probes_sample(nlg_probes *p, int s, const nlg_vec *const *vecs, double *out);
int nlg_probes_destroy(nlg_probes *p);
typedef struct nlg_dns nlg_dns;
typedef struct nlg_dns_opts { int chunk; /* ring length in steps, default 256 */ } nlg_dns_opts;
int nlg_dns_opts_default(nlg_dns_opts *o);
int nlg_dns_create(nlg_linop *op, const nlg_vec *X0, const nlg_dns_opts *o, nlg_dns **out);
int nlg_dns_set_probes(nlg_dns *d, nlg_probes *p);
int nlg_dns_set_reference(nlg_dns *d, const nlg_vec *ref);
int nlg_dns_advance(nlg_dns *d, int nsteps);
int nlg_dns_series(nlg_dns *d, int64_t first, int64_t count, double *time, double *probe, double *dist);
int nlg_dns_count(const nlg_dns *d, int64_t *nsamples);
int nlg_dns_get_state(nlg_dns *d, nlg_vec *out);
int nlg_dns_info(const nlg_dns *d, int64_t *istep, double *time, double *dt);
int nlg_dns_destroy(nlg_dns *d);
/* Wall forces, torque and heat flux on sets of element faces (Nek5000's `torque_calc` convention: symmetric 2 nu S . n, pressure and
 * viscous parts apart; the drag, lift and Nusselt number of the reference's cylinder and temperature cases).
 * A face is (global element id, face), face in the preprocessor's numbering 1 = s-, 2 = r+, 3 = s+, 4 = r-, 5 = t-, 6 = t+; it need not lie
 * on the boundary.  An object is a set of faces; an element may carry several faces, in the same or in different objects.
 * At face point q of a face normal to reference direction a on side sigma = +-1 the area-weighted outward normal is
 *   N_q = sigma (J grad r_a)_q w_q,   w_q = the product of the GLL weights of the other dim - 1 directions.
 * x_q is the face point, (grad u)_q the pointwise element-local gradient (D along every direction, metrics, division by J; not averaged
 * across elements), p_q the element's pressure-mesh (Gauss) values carried to the face point by the tensor Lagrange interpolation
 * GL -> GLL (it extrapolates along the normal), element-local: WITHOUT the direct-stiffness average of Nek5000's `mappr`, so that
 * neither a gather-scatter nor a halo is needed.  No masks are applied.  Per object, summed over its faces and face points, with the
 * object's centre c (0 by default):
 *   Fp_i = sum p_q N_q,i               Fv_i = -nu sum_j (d_j u_i + d_i u_j)_q N_q,j
 *   Tp   = sum (x_q - c) x (p_q N_q)   Tv   = the same with the viscous traction     (z component in 2-D, three components in 3-D)
 *   Q    = sum (grad theta)_q . N_q    (0 for vectors without a scalar; times -conductivity it is the heat flux)
 *   area = sum |N_q|                   (computed at creation)
 * Sign: with the faces' outward normals pointing into the body, Fp + Fv is the force the fluid exerts on the body.  Coefficients are the
 * caller's division, e.g. Cd = 2 (Fp_x + Fv_x) / (rho U^2 L).  Everything is linear in (u, p, theta): it applies to perturbations and
 * modes as to flows; a complex mode passes its real and imaginary parts as two vectors.
 * Output per (vector, object): NQ = 2 dim + 2 nt + 1 doubles Fp[dim], Fv[dim], Tp[nt], Tv[nt], Q; nt = 1 in 2-D, 3 in 3-D.
 *   nlg_forces_geometry: pure host code, no GPU needed.  For the faces (elem_local[f], face[f]) of a mesh given by its GLL coordinates:
 *     nds[nfaces][nfp][dim] = N_q, met[nfaces][nfp][dim * dim] = (d r_j / d x_i)_q at index j * dim + i, xc[nfaces][nfp][dim] = x_q - c,
 *     area[nobj]; nfp = lx1^(dim-1) face points, the lower tangential direction fastest (nekio.face_nodes).  obj NULL: one object;
 *     centre NULL: 0; any output may be NULL.  Returns 1 on a bad argument.
 *   create: the face list is global and the same on every rank; a face belongs to the rank that holds its element.  Refused with a
 *     message that names the argument: face outside 1..2 dim, an element id no rank holds, the same (element, face) twice, obj outside
 *     0..nobj-1.  Several ranks: one all-reduce (holders and areas).
 *   sample: s = 1..4 vectors in two launches -- k_wall_forces, one wave per (face, vector), and k_wall_forces_reduce, which sums the
 *     faces of every (vector, object) in a fixed order (by global element id, then face) -- so the results repeat bit for bit and a vector
 *     in a call of several equals its single call.  out[s][nobj][NQ], global sums (several ranks: one all-reduce).  Refused: s outside
 *     1..4, vectors of another mesh or of differing nscal.
 *   tractions: per face point of this rank's faces, in the order of the list: p[.][nfp] = p_q, trac[.][nfp][dim] = p_q N_q -
 *     nu (grad u + grad u^T)_q N_q, nds[.][nfp][dim] = N_q (any may be NULL): the pressure and friction distribution along a wall.
 *   destroy: refused while an nlg_dns samples the faces.
 *   nlg_dns_set_forces (NULL detaches; the series starts again, as nlg_dns_set_probes): every sample also holds the nobj * NQ sums of the
 *     state, with nu = 1 / Re of the run's operator: two more launches per step, no host synchronisation and no collective of their own.
 *   nlg_dns_force_series: force[count][nobj][NQ] of the samples first .. first + count - 1. */
int nlg_forces_geometry(int dim, int n, int64_t nel, const double *x, const double *y, const double *z, int64_t nfaces,
                        const int64_t *elem_local, const int *face, const int *obj, int nobj, const double *centre, double *nds, double *met,
                        double *xc, double *area);
typedef struct nlg_forces nlg_forces;
int nlg_forces_create(nlg_mesh *mesh, int nobj, int64_t nfaces, const int64_t *elem_gid, const int *face, const int *obj,
                      const double *centre, nlg_forces **out);
int nlg_forces_info(const nlg_forces *f, double *area, int64_t *nfaces_local);
int nlg_forces_sample(nlg_forces *f, int s, const nlg_vec *const *vecs, double nu, double *out);
int nlg_forces_tractions(nlg_forces *f, const nlg_vec *vec, double nu, double *p, double *trac, double *nds);
int nlg_forces_destroy(nlg_forces *f);
int nlg_dns_set_forces(nlg_dns *d, nlg_forces *f);
int nlg_dns_force_series(nlg_dns *d, int64_t first, int64_t count, double *force);
/* %tau read/written by the driver (src/neklab_analysis.f90:84; apply_exptA neklab_linops.f90:252) */
int nlg_linop_set_tau(nlg_linop *op, double tau);
int nlg_linop_get_info(const nlg_linop *op, double *tau, double *dt, int *nsteps, double *cfl);
/* counters since creation: time steps, Helmholtz iterations, pressure iterations, matvecs
 * (LightKrylov's per-linop matvec counter/timer, src/neklab_analysis.f90:98) */
int nlg_linop_get_stats(const nlg_linop *op, int64_t *steps, int64_t *v_iters, int64_t *p_iters, int64_t *matvecs);

/* Building blocks of the matvec, exposed for operator-level parity tests and for the
 * "operator applies per second" unit of SURVEY.md §8(d).  They act on the fields of nlg_vec objects
 * that live on the same mesh.
 *   helmholtz : out.v_i = [mask_i * QQ^T] (h1 * A + h2 * B) in.v_i    (assemble=0: element-local only)
 *               operator pieces spelled out at src/linops/neklab_linops.f90:332-366
 *   dssum     : v_i <- QQ^T v_i                     (opdssum, real_vectors.f90:100)
 *   cdabdtp   : out.pr = D (mask B^-1 QQ^T) D^T in.pr
 *   opdiv     : out.pr = sum_i D_i in.v_i ;  opgradt: out.v_i = D_i^T in.pr (neklab_linops.f90:368-380)
 *   conv      : out.v_i = weak linearised convective term around `base` (neklab_linops.f90:268-313)
 */
int nlg_op_helmholtz(nlg_mesh *mesh, const nlg_vec *in, nlg_vec *out, double h1, double h2, int assemble);
int nlg_op_dssum(nlg_mesh *mesh, nlg_vec *v);
int nlg_op_cdabdtp(nlg_mesh *mesh, const nlg_vec *in, nlg_vec *out);
/* out%pr = M^-1 in%pr, the two-level Schwarz preconditioner the pressure solve uses for E (Nek5000's role:
   `preconditioner = semg_xxt`, examples/cylinder/stability/direct/1cyl.par:21).  overlap != 0: local solves with one
   layer of face overlap (3-D lx1 <= 12 except 11, 2-D lx1 <= 8; an error elsewhere); with_coarse == 0: local solves
   only.  M is symmetric positive semi-definite. */
int nlg_op_pprec(nlg_mesh *mesh, const nlg_vec *in, nlg_vec *out, int overlap, int with_coarse);
int nlg_op_opdiv(nlg_mesh *mesh, const nlg_vec *in, nlg_vec *out);
int nlg_op_opgradt(nlg_mesh *mesh, const nlg_vec *in, nlg_vec *out);
int nlg_op_conv(nlg_mesh *mesh, const nlg_vec *base, const nlg_vec *in, nlg_vec *out, int adjoint);
/* The convective terms in the form the time stepper launches them, for tests against a reference: the s = 1..4 vectors go through one
 * buffer with the lanes a constant stride apart (the stepper's slab layout) and the operator is called ONCE with (s, stride).
 *   conv_lanes : out[v].v_i = conv(base, in[v], adjoint)_i, the term of nlg_op_conv; s = 1 launches the kernels of nlg_op_conv.
 *   conv_scalar: the temperature (Boussinesq) terms; base, in[v] and out[v] carry one scalar (theta = scalar 0):
 *       out[v].theta = J^T W [(U . grad) theta_v + (u_v . grad) Theta]     (adjoint = 0; weak, dealiased, element-local)
 *                    = - J^T W [(U . grad) theta_v]                        (adjoint != 0: transport of the adjoint temperature)
 *       out[v].v_i   = J^T W [theta_v dTheta/dx_i]                         (both values of adjoint: the temperature term of the adjoint
 *                                                                           momentum equation, the transpose of (u . grad) Theta)
 *     no buoyancy term and no bm1 b . u term.
 * Only the fields named are written: the pressure, the restart history and (conv_lanes) the scalars of out[v] are left alone.  in and
 * out may alias.  Refused with a message, out untouched: s outside 1..4, a vector on another mesh, (conv_scalar) a vector without a
 * scalar. */
int nlg_op_conv_lanes(nlg_mesh *mesh, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint);
int nlg_op_conv_scalar(nlg_mesh *mesh, const nlg_vec *base, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint);
/* ONE application of the operator of a PCG loop in the form that only the solver calls, for tests against a reference (nothing is
 * iterated, so nothing is amplified).  Host arrays, natural element layout, lane-major: a per-lane field argument is [nl][nf][points],
 * a per-lane scalar [nl].  On the device the lanes sit a padded stride apart, as in the solver's slab.  Every output buffer holds
 * `sentinel` (finite) before the launch: what a kernel does not write comes back as the sentinel.
 *
 * helmholtz_pcg = the velocity / temperature solve's application (helm_apply): the Helmholtz kernel with the first-stage sums and the
 * done flags, then the gather-scatter gated by the same flags; no mask is applied to w.
 *   fused = 0 : w = QQ^T (h1 A + h2 B) u                       (the single-reduction PCG's plain application; zf, beta, pcinv unused)
 *   fused = 1 : u <- zf + beta[lane] u, then the same           (direction update inside the kernel)
 *   zfree = 1 : u <- pc zf + beta[lane] u with pc = mask_c ? pcinv : 0, the product rounded on its own; pcinv [points] is shared by the
 *               fields and lanes, the mask bytes are built from the mesh's Dirichlet masks as nlg_linop_init builds them
 *   ring  = 1 : the updated direction goes to the next slot of a direction ring instead of over u
 *   xp    = 1 : every vector in the slab-permuted layout of the 3-D velocity solve (inputs permuted on the way in, outputs on the way out)
 *   nf: 1 or dim.  Refused: zfree or xp in 2-D, zfree or ring without fused, xp on a mesh without the tables.
 *   u_out = the direction after the call (ring = 0: the buffer u was read from), u_src = the buffer u was read from, w_out = w,
 *   part [nl][part_cap] = the sums of u . w_local per block (w before the gather-scatter), *npart of them per lane.
 * cdabdtp_pcg = the pressure solve's application (pres_apply): out = E p with the done flags as gates, part [nl][part_cap] with
 *   part[b] = sum p out and part[*npart + b] = sum out over block b (3-D: one element per block).
 *   fused = 1 : p <- (z - zmean[lane]) + beta[lane] p inside the gradient kernel (3-D, lx1 = 8..10; refused elsewhere), the sums with
 *               the updated p;  ring = 1 (fused only): the updated p goes to another buffer, ring = 0: over p
 *   p_out = the direction after the call, p_src = the buffer p was read from.
 * A lane with done != 0 is skipped by every kernel. */
int nlg_op_helmholtz_pcg(nlg_mesh *mesh, int nf, int nl, double h1, double h2, const double *u, const double *zf, const double *beta,
                         const double *done, const double *pcinv, int xp, int zfree, int ring, int fused, double sentinel, double *u_out,
                         double *u_src, double *w_out, double *part, int part_cap, int *npart);
int nlg_op_cdabdtp_pcg(nlg_mesh *mesh, int nl, const double *p, const double *z, const double *beta, const double *zmean, const double *done,
                       int fused, int ring, double sentinel, double *p_out, double *p_src, double *out, double *part, int part_cap, int *npart);
/* The gather-scatter in the form the solvers call it, for tests against a reference: ONE call of the library's gather-scatter with
 * (fields, nf, gates, layout, nl, lane stride, gate stride), under the conventions of the *_pcg entries above.  in and out are
 * [nl][nf][points] in the natural element layout; done is [nl] (a lane with done != 0 is skipped) or NULL for no gate.
 *   layout = 0 : natural;  1 : face-grouped (the intermediate fields of the pressure operator);  2 : slab-permuted (the velocity
 *   solve).  The input is permuted into the layout on the way in (1: on the host, with the mesh's slot table; 2: by the kernel that
 *   permutes the solver's right-hand side) and back on the way out.
 * After the call the entry reads the whole slab and the gates back: a value outside the nf fields of a lane (the tail of a padded field,
 * the gap between the lanes) that no longer equals `sentinel`, or a changed gate, is an error ("... were overwritten"), out untouched.
 * Refused with a message, out untouched: nf outside 1..dim, nl outside 1..4, layout 1 or 2 on a mesh without those tables (2-D), a
 * sentinel that is not finite (it is compared for equality). */
int nlg_op_gs(nlg_mesh *mesh, int nf, int nl, int layout, const double *in, const double *done, double sentinel, double *out);
/* The operator L itself in strong (pointwise) form, element-local: apply_L, apply_Lv, compute_LNS_conv, compute_LNS_laplacian and
 * compute_LNS_gradp of the reference (src/linops/neklab_linops.f90:24-28, :268-426) are this one call with other coefficients:
 *   u~_k  = mask_k in.v_k                                   (bcdirvc on read: `in` is not modified)
 *   out.v_k = coef[0] / re * sum_i gradm1(gradm1(u~_k)_i)_i (lap_1D: no mass, no dssum)
 *           + coef[1] * conv(base, u~, adjoint)_k / bm1     (the weak dealiased term of nlg_op_conv over the local mass = Nek convop)
 *           + coef[2] * gradm1(P)_k,   P = in.pr interpolated from the Gauss to the GLL mesh (Nek mappr)
 * out is neither masked nor assembled; out.pr and the scalars of out are set to zero; restart history of out is left alone.  A zero
 * coefficient skips its term.  apply_L = (1, -1, -1), apply_Lv = (1, -1, 0), laplacian = (1, 0, 0), conv = (0, 1, 0), gradp = (0, 0, 1).
 * adjoint: the convective term of the adjoint equations as nlg_op_conv defines it (the reference's `trans` branch also adds the saved
 * base flow to the result, neklab_linops.f90:301-312: not reproduced).  No collective call: correct on a partitioned mesh
 * as it stands.
 * nlg_lns keeps the base-flow side of the convective term between calls (nothing of the time stepper: no preconditioner, no Krylov
 * workspace) and applies to s = 1..4 vectors in one launch of the strong-form kernel: lanes that lie a constant stride apart in memory
 * (one vector, two vectors, consecutive vectors of a basis) are read and written in place, others go through a workspace.
 * Refused with a message: s outside 1..4, a vector on another mesh, out[v] aliasing any in[w], another out[w] or the base flow last
 * given, all three coefficients zero, re <= 0.  A refused call leaves out untouched. */
typedef struct nlg_lns nlg_lns;
int nlg_lns_create(nlg_mesh *mesh, const nlg_vec *baseflow, double re, nlg_lns **out);
int nlg_lns_set_baseflow(nlg_lns *lns, const nlg_vec *baseflow);
int nlg_lns_set_re(nlg_lns *lns, double re);
int nlg_lns_apply(nlg_lns *lns, int s, const nlg_vec *const *in, nlg_vec *const *out, int adjoint, const double *coef);
int nlg_lns_destroy(nlg_lns *lns);
int nlg_op_lns(nlg_mesh *mesh, const nlg_vec *base, const nlg_vec *in, nlg_vec *out, double re, int adjoint, const double *coef);
/* Eigenvalue sensitivity from a direct / adjoint pair: the wavemaker and the gradient of the eigenvalue with respect to the base flow.
 * For real velocity fields u, a on mesh 1, with u~ = mask (.) u and a~ = mask (.) a (the velocity Dirichlet masks are applied on read,
 * as nlg_lns_apply does; d_j is the pointwise physical derivative gradm1 of an element: no mass matrix, no gather-scatter):
 *   T(u, a)_j = - sum_i a~_i d_j u~_i          (transport part)
 *   P(u, a)_j = + sum_i u~_i d_i a~_j          (production part)
 *   S(u, a)   = T + P
 * Then <a, [L(U + dU) - L(U)] u> = <S(u, a), dU> in the nek_ddot inner product, where L is the operator of nlg_lns_apply, u is
 * solenoidal and the boundary term of one integration by parts vanishes.  The term (div u) a_j is left out on purpose.
 * For a complex pair, direct u^ = u_r + i u_i with L u^ = lambda u^, adjoint u^+ = a_r + i a_i with L+ u^+ = conj(lambda) u^+:
 *   d       = <u^+, u^> = (a_r.u_r + a_i.u_i) + i (a_r.u_i - a_i.u_r)          (nek_ddot)
 *   S_re    = S(u_r, a_r) + S(u_i, a_i)        S_im = S(u_i, a_r) - S(u_r, a_i)
 *   grad_U lambda = (S_re + i S_im) / d        (same split for T and P)
 *   W(x)    = |u^(x)| |u^+(x)| / |d|           (wavemaker; |u^(x)|^2 = sum_i (u_r,i^2 + u_i,i^2), of the masked fields)
 *   dlambda ~ <Re grad_U lambda, dU> + i <Im grad_U lambda, dU>
 * A real eigenpair has no imaginary parts: pass them as NULL.
 * nlg_sens_apply: s = 1..4 pairs in one launch of k_lns_sens.  dir_im, adj_im: NULL, or arrays whose entries are NULL for the real
 *   pairs.  scale: the complex factor 1 / d of pair v at scale[2 v], scale[2 v + 1] (NULL: 1).  grad_re[v] receives Re(S scale),
 *   grad_im[v] Im(S scale), transp_re / transp_im the same of T alone, wavemaker[v] carries W |scale| in its first velocity component.
 *   grad_im, transp_re, transp_im, wavemaker: NULL, or arrays with NULL entries, for what is not asked for: neither computed nor stored.
 *   Of every output vector the velocity carries the field; its pressure, scalars and restart history are zeroed, so that nlg_vec_dot
 *   against a dU and the field writers work on it.  Element-local and without a collective call: correct on a partitioned mesh.
 *   Refused with a message: NULL dir_re / adj_re / grad_re (or entries), s outside 1..4, a vector on another mesh, an output that
 *   aliases an input or another output, dir_im[v] without adj_im[v] or the reverse, lx1 outside 4..10, 12.  A refused call leaves
 *   nothing changed.
 * nlg_sens_pairing: d[0] + i d[1] = <u^+, u^>, four dots in one reduction with one all-reduce (dir_im = adj_im = NULL: one dot). */
int nlg_sens_apply(nlg_mesh *mesh, int s, const nlg_vec *const *dir_re, const nlg_vec *const *dir_im, const nlg_vec *const *adj_re,
                   const nlg_vec *const *adj_im, const double *scale, nlg_vec *const *grad_re, nlg_vec *const *grad_im,
                   nlg_vec *const *transp_re, nlg_vec *const *transp_im, nlg_vec *const *wavemaker);
int nlg_sens_pairing(const nlg_vec *dir_re, const nlg_vec *dir_im, const nlg_vec *adj_re, const nlg_vec *adj_im, double *d);
/* the explicit modal filter of the time stepper (nlg_exptA_config.filter_weight / filter_modes) on its own, in place on the velocity
 * fields (and scalars) of nvec <= 4 vectors, which go through the kernel together as the lanes of a block step do */
int nlg_op_filter(nlg_mesh *mesh, int nvec, nlg_vec *const *vecs, double filter_weight, int filter_modes);
int nlg_op_cfl(nlg_mesh *mesh, const nlg_vec *base, double dt, double *cfl);

/* ---------------------------------------------------------------------------------------------- */
/* eigs: the LightKrylov call at src/neklab_analysis.f90:80-81                                       */
/* ---------------------------------------------------------------------------------------------- */
/* one Arnoldi step on device: basis column k -> column k+1, H(0:k+1, k) written to H (column-major,
 * leading dimension ldh). transpose != 0 uses rmatvec. */
int nlg_arnoldi_step(nlg_linop *op, nlg_basis *basis, int k, double *H, int ldh, int transpose);

/* one BLOCK Arnoldi step: the s columns k .. k+s-1 of the basis -> columns k+s .. k+2s-1 (s matvecs, then
 * nlg_basis_block_cgs2 against the k+s columns before them); H(0:k+2s, k:k+s) written (column-major, ldh >= k+2s). */
int nlg_block_arnoldi_step(nlg_linop *op, nlg_basis *basis, int k, int s, double *H, int ldh, int transpose);

/* one Arnoldi step of s <= 4 SEPARATE eigenproblems in lock-step (wavenumber sweep): column k of basis[l] goes through
 * nlg_linop_matvec_block, lane l at the operator's wavenumber alpha[l], into column k+1 of basis[l]; then
 * nlg_basis_cgs2_batch orthogonalises every lane against its own k+1 columns.  Column k of lane l's Hessenberg matrix is
 * written to H + l*hstride in the layout of nlg_arnoldi_step (H[k*ldh + 0..k], H[k*ldh + k+1] = beta); one device-to-host
 * copy for all lanes.  Refused: an operator without wavenumber lanes (nlg_linop_set_projection_lanes), s > nalpha,
 * k + 1 >= nvec. */
int nlg_sweep_arnoldi_step(nlg_linop *op, int s, nlg_basis *const *basis, int k, double *H, int ldh, int64_t hstride,
                           int transpose);

typedef struct nlg_eigs_opts {
    int kdim;               /* kdim=  (1cyl.usr:11: 128)                                          */
    int transpose;          /* transpose= adjoint_                                                 */
    int max_restarts;       /* Krylov-Schur restarts                                               */
    int write_intermediate; /* write_intermediate=.true. -> eigs_output.txt rewritten every step   */
    double tol;             /* tolerance=, <= 0 => sqrt(1e-15) (LightKrylov rtol_dp)               */
    const char *logfile;    /* NULL => "eigs_output.txt"                                           */
    uint64_t seed;          /* start vector seed when x0 == NULL                                   */
    int block_size;         /* > 1: block Arnoldi with this many vectors per step (<= 4): the basis is read once per
                               block in every Gram-Schmidt pass; the first column is x0 / seed, the others are drawn;
                               no restart (kdim = size of the block Krylov space).  0 / 1: Arnoldi + Krylov-Schur  */
    int warm_start;         /* != 0: start from the image A x0 (which carries a restart history like every later Krylov
                               vector) instead of x0 itself; removes the start-vector dependence of the converged Ritz
                               values that the history-free first column causes.  Default 0 = LightKrylov */
} nlg_eigs_opts;

int nlg_eigs_opts_default(nlg_eigs_opts *o);
/* eigs(A, X, eigvals, residuals, info, x0, kdim, transpose, write_intermediate):
 * X[nev] are existing vectors (allocate(eigvecs(nev)); zero_basis, neklab_analysis.f90:77) and are
 * overwritten; eigvals (re, im) and residuals have nev entries; *info = number of matvecs (>0) or
 * a negative error.  Eigenvectors follow the real LAPACK convention (pair = Re, Im consecutive). */
int nlg_eigs(nlg_linop *op, nlg_vec **X, int nev, double *eig_re, double *eig_im, double *residuals,
             int *info, const nlg_vec *x0, const nlg_eigs_opts *opts);

/* svds(A, U, S, V, residuals, info, kdim=, write_intermediate=) -- the LightKrylov call of
 * transient_growth_analysis_fixed_point (src/neklab_analysis.f90:136; examples/back_fstep/transient_growth/
 * bfs.usr:8-21): leading singular triplets of exp(tau L) by Lanczos bidiagonalisation with matvec + rmatvec.
 * U[nsv] (optimal responses) and V[nsv] (optimal perturbations) are existing vectors and are overwritten;
 * S and residuals have nsv entries; *info = number of operator applications.  opts->kdim, tol, seed,
 * write_intermediate, logfile ("svds_output.txt") as for nlg_eigs; u0 (may be NULL) is the start vector. */
int nlg_svds(nlg_linop *op, nlg_vec **U, nlg_vec **V, int nsv, double *S, double *residuals, int *info,
             const nlg_vec *u0, const nlg_eigs_opts *opts);

/* symmetric tridiagonal eigen-decomposition (diagonal d[n], sub-diagonal e[1..n-1]); eigenvalues ascending in d,
 * eigenvectors as columns of the row-major n x n array Z.  Host helper of nlg_svds, exported for unit tests. */
int nlg_symtridiag_eig(int n, double *d, double *e, double *Z);

/* host-side dense helper used by nlg_eigs, exported for unit tests: eigen-decomposition of a real
 * n x n matrix (column-major, lda); vr column-major complex pairs as LAPACK dgeev. */
int nlg_dense_eig(int n, const double *A, int lda, double *wr, double *wi, double *vr, int ldvr);

#ifdef __cplusplus
}
#endif
#endif /* NEKLAB_GPU_H */
