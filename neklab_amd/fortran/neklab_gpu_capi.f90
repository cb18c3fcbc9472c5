!> ISO_C_BINDING view of include/neklab_gpu.h: one bind(C) interface per entry point the Fortran shim forwards to,
!! the two interoperable structs, the process-wide handles and the case parameters.
!!
!! The reference keeps the corresponding state in Nek5000 commons (SIZE / TOTAL / INPUT): lx1, nelv, the coordinates and
!! masks, `param(2)` (viscosity), `param(21/22)` (tolerances), `param(27)` (time order), `ifheat`, `lorder`, `ldimt`
!! (e.g. /root/reference/src/vectors/neklab_vectors.f90:8-14, src/neklab_nek_setup.f90:227-230,
!! src/linops/exponential_propagator.f90:23).  A Nek5000 host calls neklab_gpu_init / neklab_gpu_set_mesh /
!! neklab_gpu_set_case once from `usrdat3` or at the top of `userchk` (INTEGRATION.md).
module neklab_gpu_capi
   use iso_c_binding
   use iso_fortran_env, only: real64
   implicit none
   private :: real64
   integer, parameter, private :: dp = real64

   !> process-wide handles
   type(c_ptr), save, public :: nlg_ctx = c_null_ptr
   type(c_ptr), save, public :: nlg_mesh = c_null_ptr

   type, bind(C), public :: nlg_mesh_desc
      integer(c_int) :: dim, n, lxd
      integer(c_int64_t) :: nelv
      type(c_ptr) :: xm1, ym1, zm1, glo_num, lglel, v1mask, v2mask, v3mask, tmask
      integer(c_int) :: has_outflow
   end type

   !> nlg_exptA_config, every component default-initialised to what nlg_exptA_config_default returns
   type, bind(C), public :: nlg_exptA_config
      real(c_double) :: tau = 1.0_c_double, re = 100.0_c_double, cfl_limit = 0.5_c_double
      real(c_double) :: vtol = 1.0e-9_c_double, ptol = 1.0e-7_c_double, dt = 0.0_c_double
      integer(c_int) :: torder = 3, maxit_v = 200, maxit_p = 2000, fixed_iters_v = 0, fixed_iters_p = 0, pprecond = 0, pproj = 1
      integer(c_int) :: ifheat = 0
      real(c_double) :: conductivity = 1.0_c_double, rhocp = 1.0_c_double, buoy(3) = 0.0_c_double
      integer(c_int) :: no_history = 0
      real(c_double) :: filter_weight = 0.0_c_double   ! Nek5000 `filtering = explicit`: filterWeight, 0 = off
      integer(c_int) :: filter_modes = 0               ! attenuated modes (from filterCutoffRatio), 1 .. lx1 - 2
   end type

   type, bind(C), public :: nlg_eigs_opts
      integer(c_int) :: kdim = 0, transpose = 0, max_restarts = 50, write_intermediate = 1
      real(c_double) :: tol = 0.0_c_double
      type(c_ptr) :: logfile = c_null_ptr
      integer(c_int64_t) :: seed = 0
      integer(c_int) :: block_size = 0, warm_start = 0
   end type

   !> nlg_otd_opts with the defaults of nlg_otd_opts_default
   type, bind(C), public :: nlg_otd_opts
      integer(c_int) :: r = 2, startstep = 1, orthostep = 10, trans = 0, solve_baseflow = 0
   end type

   !> nlg_dns_opts with the default of nlg_dns_opts_default
   type, bind(C), public :: nlg_dns_opts
      integer(c_int) :: chunk = 256
   end type

   !> what the reference reads from Nek5000's `param(.)` / logical flags: the template every exptA_linop starts from,
   !! the number of active scalars (ifto / ifpsco) and `lorder` of SIZE for every nek_dvector
   type(nlg_exptA_config), save, public :: nek_case
   integer, save, public :: nek_nscal = 0, nek_lorder = 3
   integer(c_int64_t), save, public :: nek_lvn = 0, nek_lpn = 0
   integer, save, public :: nek_ldim = 0, nek_lx1 = 0
   !> Nek5000's endTime (param(10)): the horizon the nonlinear map of the Newton systems integrates over (fixed_point.f90:14-24)
   real(c_double), save, public :: nek_endtime = 1.0_c_double

   interface
      function c_last_error() bind(C, name="nlg_last_error") result(p)
         import c_ptr
         type(c_ptr) :: p
      end function
      function c_ctx_create(device, ctx) bind(C, name="nlg_ctx_create") result(rc)
         import c_int, c_ptr
         integer(c_int), value :: device
         type(c_ptr), intent(out) :: ctx
         integer(c_int) :: rc
      end function
      function c_ctx_destroy(ctx) bind(C, name="nlg_ctx_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: ctx
         integer(c_int) :: rc
      end function
      function c_mesh_create(ctx, desc, mesh) bind(C, name="nlg_mesh_create") result(rc)
         import c_int, c_ptr, nlg_mesh_desc
         type(c_ptr), value :: ctx
         type(nlg_mesh_desc), intent(in) :: desc
         type(c_ptr), intent(out) :: mesh
         integer(c_int) :: rc
      end function
      function c_mesh_destroy(mesh) bind(C, name="nlg_mesh_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int) :: rc
      end function
      function c_vec_create(mesh, nscal, lorder, v) bind(C, name="nlg_vec_create") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int), value :: nscal, lorder
         type(c_ptr), intent(out) :: v
         integer(c_int) :: rc
      end function
      function c_vec_destroy(v) bind(C, name="nlg_vec_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: v
         integer(c_int) :: rc
      end function
      function c_vec_generation(v, gen) bind(C, name="nlg_vec_generation") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), intent(out) :: gen
         integer(c_int) :: rc
      end function
      function c_vec_release(v) bind(C, name="nlg_vec_release") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: v
         integer(c_int) :: rc
      end function
      function c_vec_adopt(v, gen, status) bind(C, name="nlg_vec_adopt") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), value :: gen
         integer(c_int), intent(out) :: status
         integer(c_int) :: rc
      end function
      function c_vec_pin(v, gen) bind(C, name="nlg_vec_pin") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), value :: gen
         integer(c_int) :: rc
      end function
      function c_vec_unpin(v, gen) bind(C, name="nlg_vec_unpin") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), value :: gen
         integer(c_int) :: rc
      end function
      pure function c_vec_has_rst_checked(v, gen) bind(C, name="nlg_vec_has_rst_checked") result(flag)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), value :: gen
         integer(c_int) :: flag
      end function
      pure function c_vec_size_checked(v, gen) bind(C, name="nlg_vec_size_checked") result(n)
         import c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), value :: gen
         integer(c_int64_t) :: n
      end function
      function c_vec_pool_trim(freed) bind(C, name="nlg_vec_pool_trim") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: freed
         integer(c_int) :: rc
      end function
      pure function c_vec_has_rst_value(v) bind(C, name="nlg_vec_has_rst_value") result(flag)
         import c_int, c_ptr
         type(c_ptr), value :: v
         integer(c_int) :: flag
      end function
      function c_vec_clone(src, v) bind(C, name="nlg_vec_clone") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: src
         type(c_ptr), intent(out) :: v
         integer(c_int) :: rc
      end function
      function c_vec_copy(dst, src) bind(C, name="nlg_vec_copy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dst, src
         integer(c_int) :: rc
      end function
      function c_vec_zero(v) bind(C, name="nlg_vec_zero") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: v
         integer(c_int) :: rc
      end function
      function c_vec_rand(v, ifnorm, seed) bind(C, name="nlg_vec_rand") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int), value :: ifnorm
         integer(c_int64_t), value :: seed
         integer(c_int) :: rc
      end function
      function c_vec_scal(v, alpha) bind(C, name="nlg_vec_scal") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: v
         real(c_double), value :: alpha
         integer(c_int) :: rc
      end function
      function c_vec_axpby(alpha, x, beta, self) bind(C, name="nlg_vec_axpby") result(rc)
         import c_int, c_ptr, c_double
         real(c_double), value :: alpha, beta
         type(c_ptr), value :: x, self
         integer(c_int) :: rc
      end function
      function c_vec_dot(a, b, res) bind(C, name="nlg_vec_dot") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: a, b
         real(c_double), intent(out) :: res
         integer(c_int) :: rc
      end function
      function c_vec_size(v, n) bind(C, name="nlg_vec_size") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t), intent(out) :: n
         integer(c_int) :: rc
      end function
      function c_vec_save_rst(self, v, irst) bind(C, name="nlg_vec_save_rst") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: self, v
         integer(c_int), value :: irst
         integer(c_int) :: rc
      end function
      function c_vec_get_rst(self, v, irst) bind(C, name="nlg_vec_get_rst") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: self, v
         integer(c_int), value :: irst
         integer(c_int) :: rc
      end function
      function c_vec_has_rst(self, flag) bind(C, name="nlg_vec_has_rst_fields") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: self
         integer(c_int), intent(out) :: flag
         integer(c_int) :: rc
      end function
      function c_vec_clear_rst(self) bind(C, name="nlg_vec_clear_rst_fields") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: self
         integer(c_int) :: rc
      end function
      function c_vec_set_field(v, field, irst, host, count) bind(C, name="nlg_vec_set_field") result(rc)
         import c_int, c_ptr, c_double, c_int64_t
         type(c_ptr), value :: v
         integer(c_int), value :: field, irst
         real(c_double), intent(in) :: host(*)
         integer(c_int64_t), value :: count
         integer(c_int) :: rc
      end function
      function c_vec_get_field(v, field, irst, host, count) bind(C, name="nlg_vec_get_field") result(rc)
         import c_int, c_ptr, c_double, c_int64_t
         type(c_ptr), value :: v
         integer(c_int), value :: field, irst
         real(c_double), intent(out) :: host(*)
         integer(c_int64_t), value :: count
         integer(c_int) :: rc
      end function
      function c_cfg_default(cfg) bind(C, name="nlg_exptA_config_default") result(rc)
         import c_int, nlg_exptA_config
         type(nlg_exptA_config), intent(out) :: cfg
         integer(c_int) :: rc
      end function
      function c_linop_create(mesh, cfg, baseflow, op) bind(C, name="nlg_linop_create") result(rc)
         import c_int, c_ptr, nlg_exptA_config
         type(c_ptr), value :: mesh, baseflow
         type(nlg_exptA_config), intent(in) :: cfg
         type(c_ptr), intent(out) :: op
         integer(c_int) :: rc
      end function
      function c_linop_destroy(op) bind(C, name="nlg_linop_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op
         integer(c_int) :: rc
      end function
      function c_linop_init(op) bind(C, name="nlg_linop_init") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op
         integer(c_int) :: rc
      end function
      function c_linop_set_tau(op, tau) bind(C, name="nlg_linop_set_tau") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op
         real(c_double), value :: tau
         integer(c_int) :: rc
      end function
      function c_linop_set_orbit(op, X0, period) bind(C, name="nlg_linop_set_orbit") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, X0
         real(c_double), value :: period
         integer(c_int) :: rc
      end function
      function c_linop_orbit_end(op, vout) bind(C, name="nlg_linop_orbit_end") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vout
         integer(c_int) :: rc
      end function
      ! periodic-orbit Newton (include/neklab_gpu.h, nlg_upo_*) and the Krylov basis its GMRES keeps on the device
      function c_linop_set_orbit_steps(op, X0, period, nsteps) bind(C, name="nlg_linop_set_orbit_steps") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, X0
         real(c_double), value :: period
         integer(c_int), value :: nsteps
         integer(c_int) :: rc
      end function
      function c_upo_residual(op, vout) bind(C, name="nlg_upo_residual") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vout
         integer(c_int) :: rc
      end function
      function c_upo_fdot(op, which, vout) bind(C, name="nlg_upo_fdot") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vout
         integer(c_int), value :: which
         integer(c_int) :: rc
      end function
      function c_upo_jac_matvec(op, vin, t_in, vout, t_out) bind(C, name="nlg_upo_jac_matvec") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, vin, vout
         real(c_double), value :: t_in
         real(c_double), intent(out) :: t_out
         integer(c_int) :: rc
      end function
      function c_upo_arnoldi_step(op, basis, tcol, k, H, ldh) bind(C, name="nlg_upo_arnoldi_step") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, basis
         real(c_double), intent(inout) :: tcol(*), H(*)
         integer(c_int), value :: k, ldh
         integer(c_int) :: rc
      end function
      function c_basis_create(mesh, nscal, lorder, nvec, b) bind(C, name="nlg_basis_create") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int), value :: nscal, lorder, nvec
         type(c_ptr), intent(out) :: b
         integer(c_int) :: rc
      end function
      function c_basis_destroy(b) bind(C, name="nlg_basis_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: b
         integer(c_int) :: rc
      end function
      function c_basis_vec(b, i, v) bind(C, name="nlg_basis_vec") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: b
         integer(c_int), value :: i
         type(c_ptr), intent(out) :: v
         integer(c_int) :: rc
      end function
      function c_basis_combine(b, k, c, vout) bind(C, name="nlg_basis_combine") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: b, vout
         integer(c_int), value :: k
         real(c_double), intent(in) :: c(*)
         integer(c_int) :: rc
      end function
      function c_dense_eig(n, A, lda, wr, wi, vr, ldvr) bind(C, name="nlg_dense_eig") result(rc)
         import c_int, c_double
         integer(c_int), value :: n, lda, ldvr
         real(c_double), intent(in) :: A(*)
         real(c_double), intent(out) :: wr(*), wi(*), vr(*)
         integer(c_int) :: rc
      end function
      ! OTD modes (include/neklab_gpu.h, nlg_otd_*)
      function c_otd_opts_default(o) bind(C, name="nlg_otd_opts_default") result(rc)
         import c_int, nlg_otd_opts
         type(nlg_otd_opts), intent(out) :: o
         integer(c_int) :: rc
      end function
      function c_otd_create(op, o, basis0, otd) bind(C, name="nlg_otd_create") result(rc)
         import c_int, c_ptr, nlg_otd_opts
         type(c_ptr), value :: op
         type(nlg_otd_opts), intent(in) :: o
         type(c_ptr), value :: basis0      ! address of an array of r vector handles, or c_null_ptr
         type(c_ptr), intent(out) :: otd
         integer(c_int) :: rc
      end function
      function c_otd_advance(otd, nsteps) bind(C, name="nlg_otd_advance") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: otd
         integer(c_int), value :: nsteps
         integer(c_int) :: rc
      end function
      function c_otd_reduced(otd, Lr, G) bind(C, name="nlg_otd_reduced") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: otd
         real(c_double), intent(out) :: Lr(*), G(*)
         integer(c_int) :: rc
      end function
      function c_otd_get_basis(otd, i, vout) bind(C, name="nlg_otd_get_basis") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: otd, vout
         integer(c_int), value :: i
         integer(c_int) :: rc
      end function
      function c_otd_get_baseflow(otd, vout) bind(C, name="nlg_otd_get_baseflow") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: otd, vout
         integer(c_int) :: rc
      end function
      function c_otd_info(otd, istep, time, dt) bind(C, name="nlg_otd_info") result(rc)
         import c_int, c_ptr, c_double, c_int64_t
         type(c_ptr), value :: otd
         integer(c_int64_t), intent(out) :: istep
         real(c_double), intent(out) :: time, dt
         integer(c_int) :: rc
      end function
      function c_otd_destroy(otd) bind(C, name="nlg_otd_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: otd
         integer(c_int) :: rc
      end function
      ! history points and DNS runs (include/neklab_gpu.h, nlg_probes_*, nlg_dns_*)
      function c_probe_locate(dim, n, E, x, y, z, lglel, npts, xyz, tol_r, elem, rst, status, dist) bind(C, name="nlg_probe_locate") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         integer(c_int), value :: dim, n
         integer(c_int64_t), value :: E, npts
         real(c_double), intent(in) :: x(*), y(*), z(*), xyz(*)
         type(c_ptr), value :: lglel          ! address of E global element ids, or c_null_ptr
         real(c_double), value :: tol_r
         integer(c_int64_t), intent(out) :: elem(*)
         real(c_double), intent(out) :: rst(*), dist(*)
         integer(c_int), intent(out) :: status(*)
         integer(c_int) :: rc
      end function
      function c_probes_create(mesh, npts, xyz, tol_r, p) bind(C, name="nlg_probes_create") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int64_t), value :: npts
         real(c_double), intent(in) :: xyz(*)
         real(c_double), value :: tol_r
         type(c_ptr), intent(out) :: p
         integer(c_int) :: rc
      end function
      function c_probes_status(p, status, elem_global, rst, dist) bind(C, name="nlg_probes_status") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: p
         integer(c_int), intent(out) :: status(*)
         integer(c_int64_t), intent(out) :: elem_global(*)
         real(c_double), intent(out) :: rst(*), dist(*)
         integer(c_int) :: rc
      end function
      function c_probes_sample(p, s, vecs, out) bind(C, name="nlg_probes_sample") result(rc)
         import c_int, c_double, c_ptr
         type(c_ptr), value :: p
         integer(c_int), value :: s
         type(c_ptr), value :: vecs           ! address of an array of s vector handles
         real(c_double), intent(out) :: out(*)
         integer(c_int) :: rc
      end function
      function c_probes_destroy(p) bind(C, name="nlg_probes_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: p
         integer(c_int) :: rc
      end function
      function c_dns_opts_default(o) bind(C, name="nlg_dns_opts_default") result(rc)
         import c_int, nlg_dns_opts
         type(nlg_dns_opts), intent(out) :: o
         integer(c_int) :: rc
      end function
      function c_dns_create(op, X0, o, dns) bind(C, name="nlg_dns_create") result(rc)
         import c_int, c_ptr, nlg_dns_opts
         type(c_ptr), value :: op, X0
         type(nlg_dns_opts), intent(in) :: o
         type(c_ptr), intent(out) :: dns
         integer(c_int) :: rc
      end function
      function c_dns_set_probes(dns, p) bind(C, name="nlg_dns_set_probes") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns, p
         integer(c_int) :: rc
      end function
      function c_dns_set_reference(dns, ref) bind(C, name="nlg_dns_set_reference") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns, ref       ! ref c_null_ptr: the state as it stands
         integer(c_int) :: rc
      end function
      function c_dns_advance(dns, nsteps) bind(C, name="nlg_dns_advance") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns
         integer(c_int), value :: nsteps
         integer(c_int) :: rc
      end function
      function c_dns_series(dns, first, count, time, probe, dist) bind(C, name="nlg_dns_series") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: dns
         integer(c_int64_t), value :: first, count
         real(c_double), intent(out) :: time(*), probe(*), dist(*)
         integer(c_int) :: rc
      end function
      function c_dns_count(dns, nsamples) bind(C, name="nlg_dns_count") result(rc)
         import c_int, c_int64_t, c_ptr
         type(c_ptr), value :: dns
         integer(c_int64_t), intent(out) :: nsamples
         integer(c_int) :: rc
      end function
      function c_dns_get_state(dns, vout) bind(C, name="nlg_dns_get_state") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns, vout
         integer(c_int) :: rc
      end function
      function c_dns_info(dns, istep, time, dt) bind(C, name="nlg_dns_info") result(rc)
         import c_int, c_ptr, c_double, c_int64_t
         type(c_ptr), value :: dns
         integer(c_int64_t), intent(out) :: istep
         real(c_double), intent(out) :: time, dt
         integer(c_int) :: rc
      end function
      function c_dns_destroy(dns) bind(C, name="nlg_dns_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns
         integer(c_int) :: rc
      end function
      ! wall forces, torque and heat flux (include/neklab_gpu.h, nlg_forces_*)
      function c_forces_create(mesh, nobj, nfaces, elem_gid, face, obj, centre, f) bind(C, name="nlg_forces_create") result(rc)
         import c_int, c_int64_t, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int), value :: nobj
         integer(c_int64_t), value :: nfaces
         integer(c_int64_t), intent(in) :: elem_gid(*)      ! 0-based, as the C ABI has them
         integer(c_int), intent(in) :: face(*), obj(*)
         type(c_ptr), value :: centre                       ! address of centre(ldim, nobj), or c_null_ptr
         type(c_ptr), intent(out) :: f
         integer(c_int) :: rc
      end function
      function c_forces_info(f, area, nfaces_local) bind(C, name="nlg_forces_info") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: f
         real(c_double), intent(out) :: area(*)
         integer(c_int64_t), intent(out) :: nfaces_local
         integer(c_int) :: rc
      end function
      function c_forces_sample(f, s, vecs, nu, out) bind(C, name="nlg_forces_sample") result(rc)
         import c_int, c_double, c_ptr
         type(c_ptr), value :: f
         integer(c_int), value :: s
         type(c_ptr), value :: vecs           ! address of an array of s vector handles
         real(c_double), value :: nu
         real(c_double), intent(out) :: out(*)
         integer(c_int) :: rc
      end function
      function c_forces_destroy(f) bind(C, name="nlg_forces_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: f
         integer(c_int) :: rc
      end function
      function c_dns_set_forces(dns, f) bind(C, name="nlg_dns_set_forces") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: dns, f         ! f c_null_ptr: detach
         integer(c_int) :: rc
      end function
      function c_dns_force_series(dns, first, count, force) bind(C, name="nlg_dns_force_series") result(rc)
         import c_int, c_int64_t, c_double, c_ptr
         type(c_ptr), value :: dns
         integer(c_int64_t), value :: first, count
         real(c_double), intent(out) :: force(*)
         integer(c_int) :: rc
      end function
      ! the operator L itself in strong form (include/neklab_gpu.h, nlg_lns_*)
      function c_lns_create(mesh, baseflow, re, lns) bind(C, name="nlg_lns_create") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: mesh, baseflow
         real(c_double), value :: re
         type(c_ptr), intent(out) :: lns
         integer(c_int) :: rc
      end function
      function c_lns_set_baseflow(lns, baseflow) bind(C, name="nlg_lns_set_baseflow") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: lns, baseflow
         integer(c_int) :: rc
      end function
      function c_lns_set_re(lns, re) bind(C, name="nlg_lns_set_re") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: lns
         real(c_double), value :: re
         integer(c_int) :: rc
      end function
      function c_lns_apply(lns, s, vin, vout, adjoint, coef) bind(C, name="nlg_lns_apply") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: lns
         integer(c_int), value :: s, adjoint
         type(c_ptr), intent(in) :: vin(*), vout(*)
         real(c_double), intent(in) :: coef(3)
         integer(c_int) :: rc
      end function
      !> the array arguments are C arrays of vector handles (c_loc of a type(c_ptr) array), c_null_ptr for what is absent
      function c_sens_apply(mesh, s, dir_re, dir_im, adj_re, adj_im, scale, grad_re, grad_im, transp_re, transp_im, wavemaker) &
         bind(C, name="nlg_sens_apply") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: mesh
         integer(c_int), value :: s
         type(c_ptr), value :: dir_re, dir_im, adj_re, adj_im, scale, grad_re, grad_im, transp_re, transp_im, wavemaker
         integer(c_int) :: rc
      end function
      function c_sens_pairing(dir_re, dir_im, adj_re, adj_im, d) bind(C, name="nlg_sens_pairing") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: dir_re, dir_im, adj_re, adj_im
         real(c_double), intent(out) :: d(2)
         integer(c_int) :: rc
      end function
      function c_lns_destroy(lns) bind(C, name="nlg_lns_destroy") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: lns
         integer(c_int) :: rc
      end function
      function c_linop_matvec(op, vin, vout) bind(C, name="nlg_linop_matvec") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vin, vout
         integer(c_int) :: rc
      end function
      function c_linop_rmatvec(op, vin, vout) bind(C, name="nlg_linop_rmatvec") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vin, vout
         integer(c_int) :: rc
      end function
      function c_linop_nonlinear_map(op, vin, vout) bind(C, name="nlg_linop_nonlinear_map") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, vin, vout
         integer(c_int) :: rc
      end function
      function c_linop_set_baseflow(op, bf) bind(C, name="nlg_linop_set_baseflow") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, bf
         integer(c_int) :: rc
      end function
      function c_linop_set_tolerances(op, vtol, ptol) bind(C, name="nlg_linop_set_tolerances") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op
         real(c_double), value :: vtol, ptol
         integer(c_int) :: rc
      end function
      function c_strlen(s) bind(C, name="strlen") result(n)
         import c_ptr, c_size_t
         type(c_ptr), value :: s
         integer(c_size_t) :: n
      end function
         pure function c_vec_size_value(v) bind(C, name="nlg_vec_size_value") result(n)
         import c_ptr, c_int64_t
         type(c_ptr), value :: v
         integer(c_int64_t) :: n
      end function
      function c_vec_nrst(v, n) bind(C, name="nlg_vec_nrst") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: v
         integer(c_int), intent(out) :: n
         integer(c_int) :: rc
      end function
      function c_vec_outpost(v, path, with_coords, time, istep) bind(C, name="nlg_vec_outpost") result(rc)
         import c_int, c_ptr, c_double, c_char
         type(c_ptr), value :: v
         character(kind=c_char), intent(in) :: path(*)
         integer(c_int), value :: with_coords, istep
         real(c_double), value :: time
         integer(c_int) :: rc
      end function
      function c_mesh_sizes(mesh, lvn, lpn, dim, n) bind(C, name="nlg_mesh_sizes") result(rc)
         import c_int, c_ptr, c_int64_t
         type(c_ptr), value :: mesh
         integer(c_int64_t), intent(out) :: lvn, lpn
         integer(c_int), intent(out) :: dim, n
         integer(c_int) :: rc
      end function
      function c_linop_get_info(op, tau, dt, nsteps, cfl) bind(C, name="nlg_linop_get_info") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op
         real(c_double), intent(out) :: tau, dt, cfl
         integer(c_int), intent(out) :: nsteps
         integer(c_int) :: rc
      end function
      function c_linop_set_projection(op, alpha, idir, lab, lab2, x2) bind(C, name="nlg_linop_set_projection") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, lab, lab2, x2
         real(c_double), value :: alpha
         integer(c_int), value :: idir
         integer(c_int) :: rc
      end function
      function c_linop_project(op, v) bind(C, name="nlg_linop_project") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op, v
         integer(c_int) :: rc
      end function
      ! wavenumber lanes (a sweep over alpha in lock-step): bindings only, the reference has no type or driver for this
      function c_linop_set_projection_lanes(op, nalpha, alpha, idir, lab, lab2, x2) bind(C, name="nlg_linop_set_projection_lanes") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, lab, lab2, x2
         integer(c_int), value :: nalpha, idir
         real(c_double), intent(in) :: alpha(*)
         integer(c_int) :: rc
      end function
      function c_linop_project_block(op, s, v) bind(C, name="nlg_linop_project_block") result(rc)
         import c_int, c_ptr
         type(c_ptr), value :: op
         integer(c_int), value :: s
         type(c_ptr), intent(in) :: v(*)
         integer(c_int) :: rc
      end function
      function c_basis_cgs2_batch(s, b, k, w, h, ldh, beta) bind(C, name="nlg_basis_cgs2_batch") result(rc)
         import c_int, c_ptr, c_double
         integer(c_int), value :: s, k, ldh
         type(c_ptr), intent(in) :: b(*), w(*)
         real(c_double), intent(out) :: h(*), beta(*)
         integer(c_int) :: rc
      end function
      function c_sweep_arnoldi_step(op, s, basis, k, H, ldh, hstride, transpose) bind(C, name="nlg_sweep_arnoldi_step") result(rc)
         import c_int, c_int64_t, c_ptr, c_double
         type(c_ptr), value :: op
         integer(c_int), value :: s, k, ldh, transpose
         integer(c_int64_t), value :: hstride
         type(c_ptr), intent(in) :: basis(*)
         real(c_double), intent(inout) :: H(*)
         integer(c_int) :: rc
      end function
      function c_linop_integrate_forced(op, ic, f_re, f_im, omega, adjoint, vout) bind(C, name="nlg_linop_integrate_forced") result(rc)
         import c_int, c_ptr, c_double
         type(c_ptr), value :: op, ic, f_re, f_im, vout
         real(c_double), value :: omega
         integer(c_int), value :: adjoint
         integer(c_int) :: rc
      end function
      function c_eigs_opts_default(o) bind(C, name="nlg_eigs_opts_default") result(rc)
         import c_int, nlg_eigs_opts
         type(nlg_eigs_opts), intent(out) :: o
         integer(c_int) :: rc
      end function
      function c_eigs(op, X, nev, eig_re, eig_im, residuals, info, x0, opts) bind(C, name="nlg_eigs") result(rc)
         import c_int, c_ptr, c_double, nlg_eigs_opts
         type(c_ptr), value :: op, x0
         type(c_ptr), intent(in) :: X(*)
         integer(c_int), value :: nev
         real(c_double), intent(out) :: eig_re(*), eig_im(*), residuals(*)
         integer(c_int), intent(out) :: info
         type(nlg_eigs_opts), intent(in) :: opts
         integer(c_int) :: rc
      end function
      function c_svds(op, U, V, nsv, S, residuals, info, u0, opts) bind(C, name="nlg_svds") result(rc)
         import c_int, c_ptr, c_double, nlg_eigs_opts
         type(c_ptr), value :: op, u0
         type(c_ptr), intent(in) :: U(*), V(*)
         integer(c_int), value :: nsv
         real(c_double), intent(out) :: S(*), residuals(*)
         integer(c_int), intent(out) :: info
         type(nlg_eigs_opts), intent(in) :: opts
         integer(c_int) :: rc
      end function
   end interface

contains

   subroutine nlg_check(rc, where)
      integer(c_int), intent(in) :: rc
      character(len=*), intent(in) :: where
      type(c_ptr) :: p
      character(kind=c_char), pointer :: msg(:)
      integer :: n, i
      character(len=1024) :: txt
      if (rc == 0) return
      p = c_last_error()
      n = int(c_strlen(p))
      txt = ''
      if (n > 0) then
         call c_f_pointer(p, msg, [n])
         do i = 1, min(n, 1024)
            txt(i:i) = msg(i)
         end do
      end if
      write (*, '(A)') 'ERROR in '//trim(where)//': '//trim(txt)
      error stop 1
   end subroutine

   !> Create the device context (once per rank).
   subroutine neklab_gpu_init(device)
      integer, intent(in) :: device
      call nlg_check(c_ctx_create(int(device, c_int), nlg_ctx), 'neklab_gpu_init')
   end subroutine

   !> Upload what the reference reads from Nek5000's SIZE/TOTAL commons (xm1, ym1, zm1, glo_num, masks).
   subroutine neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo_num, v1mask, v2mask, v3mask, has_outflow, lxd, tmask)
      integer, intent(in) :: ldim, lx1, nelv
      real(dp), target, intent(in) :: xm1(*), ym1(*), zm1(*)
      integer(c_int64_t), target, intent(in) :: glo_num(*)
      real(dp), target, intent(in) :: v1mask(*), v2mask(*), v3mask(*)
      logical, intent(in) :: has_outflow
      integer, optional, intent(in) :: lxd
      real(dp), target, optional, intent(in) :: tmask(*)
      type(nlg_mesh_desc) :: d
      integer(c_int) :: cdim, cn
      d%dim = ldim; d%n = lx1; d%lxd = 0; d%nelv = nelv
      if (present(lxd)) d%lxd = lxd
      d%xm1 = c_loc(xm1); d%ym1 = c_loc(ym1)
      d%zm1 = c_null_ptr; d%v3mask = c_null_ptr
      if (ldim == 3) then
         d%zm1 = c_loc(zm1); d%v3mask = c_loc(v3mask)
      end if
      d%glo_num = c_loc(glo_num); d%lglel = c_null_ptr
      d%v1mask = c_loc(v1mask); d%v2mask = c_loc(v2mask); d%tmask = c_null_ptr
      if (present(tmask)) d%tmask = c_loc(tmask)
      d%has_outflow = merge(1, 0, has_outflow)
      call nlg_check(c_mesh_create(nlg_ctx, d, nlg_mesh), 'neklab_gpu_set_mesh')
      call nlg_check(c_mesh_sizes(nlg_mesh, nek_lvn, nek_lpn, cdim, cn), 'neklab_gpu_set_mesh')
      nek_ldim = cdim; nek_lx1 = cn
   end subroutine

   !> The case parameters the reference takes from the .par file / SIZE through Nek5000's commons: viscosity (as
   !! Reynolds number), |param(27)| = time order, param(21) / param(22) = pressure / velocity tolerances, ifheat with
   !! its properties, the number of active scalars and `lorder`.  Omitted arguments keep their current value.
   subroutine neklab_gpu_set_case(re, torder, ptol, vtol, dt, cfl_limit, ifheat, conductivity, rhocp, buoy, nscal, lorder, &
                                  maxit_v, maxit_p, pprecond, pproj, endtime)
      real(dp), optional, intent(in) :: re, ptol, vtol, dt, cfl_limit, conductivity, rhocp, buoy(3), endtime
      integer, optional, intent(in) :: torder, nscal, lorder, maxit_v, maxit_p, pprecond, pproj
      logical, optional, intent(in) :: ifheat
      if (present(re)) nek_case%re = re
      if (present(endtime)) nek_endtime = endtime
      if (present(torder)) nek_case%torder = torder
      if (present(ptol)) nek_case%ptol = ptol
      if (present(vtol)) nek_case%vtol = vtol
      if (present(dt)) nek_case%dt = dt
      if (present(cfl_limit)) nek_case%cfl_limit = cfl_limit
      if (present(ifheat)) nek_case%ifheat = merge(1, 0, ifheat)
      if (present(conductivity)) nek_case%conductivity = conductivity
      if (present(rhocp)) nek_case%rhocp = rhocp
      if (present(buoy)) nek_case%buoy = buoy
      if (present(maxit_v)) nek_case%maxit_v = maxit_v
      if (present(maxit_p)) nek_case%maxit_p = maxit_p
      if (present(pprecond)) nek_case%pprecond = pprecond
      if (present(pproj)) nek_case%pproj = pproj
      if (present(nscal)) nek_nscal = nscal
      if (present(lorder)) nek_lorder = lorder
      if (nek_case%ifheat /= 0 .and. nek_nscal < 1) nek_nscal = 1      ! ifto: the vectors carry the temperature
      if (nek_lorder < nek_case%torder) nek_lorder = nek_case%torder
   end subroutine

   subroutine neklab_gpu_finalize()
      integer(c_int) :: rc
      rc = c_vec_pool_trim(c_null_ptr)      ! vectors released by finalisers and never adopted
      if (c_associated(nlg_mesh)) rc = c_mesh_destroy(nlg_mesh)
      if (c_associated(nlg_ctx)) rc = c_ctx_destroy(nlg_ctx)
      nlg_mesh = c_null_ptr; nlg_ctx = c_null_ptr
   end subroutine

end module neklab_gpu_capi
