!> Drop-in for the reference's module of the same name: `exptA_linop` (and the wavenumber-projected variant) with every
!! type-bound procedure forwarded to libneklab_gpu.so.
!!
!! Mapping (file:line under /root/reference):
!!   type exptA_linop                     src/linops/neklab_linops.f90:35-44   (constructor idiom exptA_linop(1.0_dp, bf),
!!                                        examples/cylinder/stability/direct/1cyl.usr:20: tau is the parent's component,
!!                                        baseflow the first own component -- positional construction works unchanged)
!!     init / matvec / rmatvec            src/linops/exponential_propagator.f90:4-107
!!     compute_rst / get_rst              src/linops/exponential_propagator.f90:109-142
!!   type exptA_proj_linop                src/linops/neklab_linops.f90:130-152, exponential_propagator_proj.f90
!! plus what the reference reaches through LightKrylov and neklab_systems on this path, bound to the device block path:
!!   nek_eigs / nek_svds                  the eigs / svds calls of src/neklab_analysis.f90:80-81, :136 (nlg_eigs, nlg_svds)
!!   nonlinear_map / set_baseflow / set_tolerances   src/systems/fixed_point.f90:4-96, neklab_systems.f90:229-335
!!   integrate_forced                     src/linops/resolvent.f90:80-111, :133-166
!! and the operator L itself in strong form (nlg_lns_*):
!!   apply_exptA                          src/linops/neklab_linops.f90:224-266
!!   compute_LNS_conv / _laplacian / _gradp, apply_L, apply_Lv   src/linops/neklab_linops.f90:268-426 (host arrays, as there)
!!   nek_otd%matvec / rmatvec = apply_LNS / apply_adjLNS          src/neklab_otd.f90:44-45, :76-116
module neklab_linops
   use iso_c_binding
   use LightKrylov, only: dp, abstract_vector_rdp, abstract_linop_rdp, abstract_exptA_linop_rdp, abstract_vector_cdp, abstract_linop_cdp, type_error
   use neklab_gpu_capi
   use neklab_vectors
   implicit none
   private
   character(len=*), parameter, private :: this_module = 'neklab_linops'

   public :: nek_eigs, nek_svds
   public :: apply_exptA, apply_L, apply_Lv, compute_LNS_conv, compute_LNS_laplacian, compute_LNS_gradp, set_lns_baseflow

   !> state of the array routines apply_L ... compute_LNS_gradp: the reference reads the base flow from Nek5000's vx, vy, vz; here
   !! set_lns_baseflow(bf) hands it over (Re is the case's).  Their arrays go through two scratch vectors.
   type(c_ptr), save, private :: lns_arrays_h = c_null_ptr
   type(nek_dvector), save, private :: lns_arrays_in, lns_arrays_out
   real(dp), parameter, private :: coef_L(3) = [1.0_dp, -1.0_dp, -1.0_dp], coef_Lv(3) = [1.0_dp, -1.0_dp, 0.0_dp], &
                                   coef_lap(3) = [1.0_dp, 0.0_dp, 0.0_dp], coef_conv(3) = [0.0_dp, 1.0_dp, 0.0_dp], &
                                   coef_gradp(3) = [0.0_dp, 0.0_dp, 1.0_dp]

   !------------------------------------------
   !-----     EXPONENTIAL PROPAGATOR     -----
   !------------------------------------------
   type, extends(abstract_exptA_linop_rdp), public :: exptA_linop
      type(nek_dvector) :: baseflow
      !> solver configuration; taken from the case (neklab_gpu_set_case: what the reference reads from param(.)) at init
      !! unless `cfg_set` says the caller filled it in
      type(nlg_exptA_config) :: cfg = nlg_exptA_config()
      logical :: cfg_set = .false.
      type(c_ptr), private :: h = c_null_ptr
      integer(c_intptr_t), private :: owner = 0
      real(dp), private :: tau_built = -1.0_dp
   contains
      private
      procedure, pass(self), public :: init => init_exptA
      procedure, pass(self), public :: matvec => exptA_matvec
      procedure, pass(self), public :: rmatvec => exptA_rmatvec
      procedure, pass(self), public :: compute_rst => exptA_compute_rst
      procedure, pass(self), public :: get_rst => exptA_get_rst
      ! Newton-Krylov row: what nek_system%eval (nonlinear_map) and nek_jacobian (self%X) forward to
      procedure, pass(self), public :: nonlinear_map => exptA_nonlinear_map
      procedure, pass(self), public :: set_baseflow => exptA_set_baseflow
      procedure, pass(self), public :: set_tolerances => exptA_set_tolerances
      ! resolvent building block (evaluate_rhs / evaluate_imaginary_part)
      procedure, pass(self), public :: integrate_forced => exptA_integrate_forced
      procedure, pass(self), public :: handle => exptA_handle
      procedure, pass(self), public :: nsteps => exptA_nsteps
      final :: finalize_exptA
   end type exptA_linop

   !> exptA_temp_linop (src/linops/neklab_linops.f90:82-93, exponential_propagator_temp.f90: the propagator of the temperature-
   !! coupled equations; the reference's file is a clone of the plain one because the temperature already travels in
   !! nek_dvector%theta) and, under the name the reference's umbrella module and its thermosyphon case use, exptA_linop_temp
   !! (src/neklab.f90:45, examples/thermosyphon/baseflow/tsyphon.usr:13,52 `exptA_linop_temp(1.0_dp, bf)`).  Here the coupling
   !! is a property of the case (neklab_gpu_set_case(ifheat=.true., ..)); the two types insist on it at init().
   type, extends(exptA_linop), public :: exptA_temp_linop
   contains
      procedure, pass(self), public :: init => init_exptA_temp
   end type exptA_temp_linop
   type, extends(exptA_temp_linop), public :: exptA_linop_temp
   end type exptA_linop_temp

   !> exptA_proj_linop(tau=.., baseflow=.., alpha=..) (examples/poiseuille/stability/direct_alpha_1/poiseuille.usr:24).
   !! `set_lines` hands over what Nek5000's gtpp_gs_setup derives from (nelx, nely, nelz): one label per velocity point
   !! naming its line along the homogeneous direction.
   type, extends(exptA_linop), public :: exptA_proj_linop
      real(dp) :: alpha = 0.0_dp
      integer :: idir = 1
   contains
      procedure, pass(self), public :: set_lines => proj_set_lines
      procedure, pass(self), public :: proj => proj_apply
   end type exptA_proj_linop

   !> exptA_orbit_linop(T, X0): the propagator over one period T about the time-periodic base flow through X0 (held in `baseflow`),
   !! the time stepper under the reference's periodic-orbit Jacobian (src/systems/periodic_orbit.f90:59-92: the nonlinear equations
   !! and the perturbation integrated together, cfl_limit = 0.4).  Its eigenvalues are the Floquet multipliers of the orbit.  The
   !! base flow rides as one more lane of the perturbation's kernel launches (nlg_linop_set_orbit).  No adjoint: rmatvec stops.
   type, extends(exptA_linop), public :: exptA_orbit_linop
   contains
      procedure, pass(self), public :: init => init_exptA_orbit
      procedure, pass(self), public :: rmatvec => exptA_orbit_rmatvec
      procedure, pass(self), public :: orbit_end => exptA_orbit_end
   end type exptA_orbit_linop

   !--------------------------------------
   !-----     RESOLVENT OPERATOR     -----
   !--------------------------------------
   !> resolvent_linop(omega, baseflow) (src/linops/neklab_linops.f90:198-205, resolvent.f90): R(omega) f by time stepping -- one
   !! forcing period from rest (nlg_linop_integrate_forced), the real part from (I - exp(T L)) x = b by GMRES(64) at rtol 1e-6
   !! (resolvent.f90:113-131; restated here on the type-bound procedures, LightKrylov's gmres options are not in the reference
   !! tree), the imaginary part = the state a quarter period later; rmatvec integrates the adjoint equations.
   type, extends(abstract_linop_cdp), public :: resolvent_linop
      real(kind=dp) :: omega = 0.0_dp
      type(nek_dvector) :: baseflow
   contains
      private
      procedure, pass(self), public :: matvec => resolvent_matvec
      procedure, pass(self), public :: rmatvec => resolvent_rmatvec
   end type

   !---------------------------------------------
   !-----     THE OPERATOR L ITSELF         -----
   !---------------------------------------------
   !> L about `baseflow` in strong form, device-resident (nlg_lns_*): matvec / rmatvec are apply_L, direct and adjoint, on
   !! nek_dvector.  re <= 0: the case's.  init() after the base flow is set (and again after it changes).
   type, extends(abstract_linop_rdp), public :: lns_linop
      type(nek_dvector) :: baseflow
      real(dp) :: re = 0.0_dp
      type(c_ptr), private :: h = c_null_ptr
      integer(c_intptr_t), private :: owner = 0
   contains
      private
      procedure, pass(self), public :: init => init_lns
      procedure, pass(self), public :: matvec => lns_matvec
      procedure, pass(self), public :: rmatvec => lns_rmatvec
      final :: finalize_lns
   end type lns_linop

   !---------------------------------------------------
   !-----     OPTIMALLY TIME-DEPENDENT MODES      -----
   !---------------------------------------------------
   !> otd_opts (src/neklab_otd.f90:51-72), same components and defaults
   type, public :: otd_opts
      integer :: startstep = 1
      integer :: printstep = 5
      integer :: orthostep = 10
      integer :: iostep = 100
      integer :: iorststep = 100
      integer :: n_usrIC = 0
      logical :: trans = .false.
      logical :: solve_baseflow = .true.
      logical :: if_output_initial_conditions = .false.
      character(len=128) :: OTDIC_basename = 'OTDIC_'
   end type otd_opts

   !> nek_otd (src/neklab_otd.f90:37-49): r OTD modes about `baseflow` as lanes of the device block step (nlg_otd_*).  The reduced
   !! operator, the forcing (generate_forcing) and the re-orthonormalisation run inside the device time step; `basis` is filled by
   !! get_basis.  cfg as for exptA_linop (from the case unless cfg_set), cfl_limit 0.4 as in init_OTD.  User initial conditions
   !! (n_usrIC) are handed over in `basis` before init(); the reference reads them with Nek5000's load_fld.
   !! matvec / rmatvec = apply_LNS / apply_adjLNS (src/neklab_otd.f90:44-45, :76-116): the strong-form L with vec_in's own pressure,
   !! about `baseflow` when it is frozen and about the current base flow of the run with solve_baseflow.  The reference's type
   !! extends abstract_linop_rdp; here nek_otd_linop (below) is that view of a nek_otd.
   type, public :: nek_otd
      integer :: r = 2
      type(nek_dvector) :: baseflow
      type(nek_dvector), allocatable :: basis(:)
      type(nlg_exptA_config) :: cfg = nlg_exptA_config()
      logical :: cfg_set = .false.
      type(c_ptr), private :: hop = c_null_ptr, h = c_null_ptr, hlns = c_null_ptr
      type(nek_dvector), private :: bf_now
      logical, private :: moving = .false.
      integer(c_intptr_t), private :: owner = 0
   contains
      private
      procedure, pass(self), public :: matvec => apply_LNS
      procedure, pass(self), public :: rmatvec => apply_adjLNS
      procedure, pass(self), public :: init => init_OTD
      procedure, pass(self), public :: advance => otd_advance
      procedure, pass(self), public :: reduced => otd_reduced
      procedure, pass(self), public :: get_basis => otd_get_basis
      procedure, pass(self), public :: get_baseflow => otd_get_baseflow
      procedure, pass(self), public :: info => otd_info
      procedure, pass(self), public :: spectral_analysis => otd_spectral_analysis
      procedure, pass(self), public :: close => otd_close
      final :: finalize_otd
   end type nek_otd

   !> a nek_otd where LightKrylov expects a class(abstract_linop_rdp): `A%otd => OTD`, then A%matvec / A%rmatvec are OTD's
   type, extends(abstract_linop_rdp), public :: nek_otd_linop
      type(nek_otd), pointer :: otd => null()
   contains
      private
      procedure, pass(self), public :: matvec => otd_linop_matvec
      procedure, pass(self), public :: rmatvec => otd_linop_rmatvec
   end type nek_otd_linop

contains

   function exptA_handle(self) result(h)
      class(exptA_linop), intent(in) :: self
      type(c_ptr) :: h
      if (.not. c_associated(self%h) .or. self%owner /= loc(self)) then
         write (*, '(A)') 'ERROR in '//this_module//': exptA%init() has not been called on this object (1cyl.usr:20)'
         error stop 1
      end if
      h = self%h
   end function

   integer function exptA_nsteps(self) result(n)
      class(exptA_linop), intent(in) :: self
      real(c_double) :: tau, dt, cfl
      integer(c_int) :: ns
      call nlg_check(c_linop_get_info(exptA_handle(self), tau, dt, ns, cfl), 'exptA_nsteps')
      n = ns
   end function

   subroutine init_exptA(self)
      class(exptA_linop), intent(inout) :: self
      integer(c_int) :: rc
      if (c_associated(self%h) .and. self%owner == loc(self)) rc = c_linop_destroy(self%h)
      self%h = c_null_ptr
      if (.not. self%cfg_set) self%cfg = nek_case      ! param(2), param(21/22), |param(27)|, ifheat ... of the Nek5000 host
      self%cfg%tau = self%tau
      call nlg_check(c_linop_create(nlg_mesh, self%cfg, nek_dvector_handle(self%baseflow), self%h), 'init_exptA')
      self%owner = loc(self)
      call nlg_check(c_linop_init(self%h), 'init_exptA')
      self%tau_built = self%tau
   end subroutine

   subroutine init_exptA_temp(self)
      class(exptA_temp_linop), intent(inout) :: self
      if (.not. self%cfg_set) self%cfg = nek_case
      if (self%cfg%ifheat == 0) then
         write (*, '(A)') 'ERROR in '//this_module//': exptA_temp_linop needs the temperature coupling of the case (neklab_gpu_set_case(ifheat=.true.))'
         error stop 1
      end if
      self%cfg_set = .true.
      call init_exptA(self)
   end subroutine

   subroutine init_exptA_orbit(self)
      class(exptA_orbit_linop), intent(inout) :: self
      if (.not. self%cfg_set) then
         self%cfg = nek_case
         self%cfg%cfl_limit = 0.4_dp                ! periodic_orbit.f90:73
         self%cfg_set = .true.
      end if
      call init_exptA(self)
      call nlg_check(c_linop_set_orbit(exptA_handle(self), nek_dvector_handle(self%baseflow), self%tau), 'init_exptA_orbit')
   end subroutine

   !> the adjoint of a time-dependent linearisation needs U(T - t); the reference's forward-run adjoint (periodic_orbit.f90:117-183)
   !! is not reproduced on purpose.  The library refuses with its own message; this stops with it.
   subroutine exptA_orbit_rmatvec(self, vec_in, vec_out)
      class(exptA_orbit_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            call nek_dvector_ensure(vec_out)
            call nlg_check(c_linop_rmatvec(exptA_handle(self), nek_dvector_handle(vec_in), vec_out%h), 'exptA_orbit_rmatvec')
         end select
      end select
      write (*, '(A)') 'ERROR in '//this_module//': exptA_orbit_linop has no adjoint (orbit mode)'
      error stop 1
   end subroutine

   !> Phi_T(X0): the base flow after the time steps of the last matvec (how well the orbit closes)
   subroutine exptA_orbit_end(self, vec_out)
      class(exptA_orbit_linop), intent(in) :: self
      type(nek_dvector), intent(inout) :: vec_out
      call nek_dvector_ensure(vec_out)
      call nlg_check(c_linop_orbit_end(exptA_handle(self), vec_out%h), 'exptA_orbit_end')
   end subroutine

   subroutine sync_tau(self, where)
      class(exptA_linop), intent(inout) :: self
      character(len=*), intent(in) :: where
      if (self%tau /= self%tau_built) then       ! apply_exptA sets A%tau before the call (neklab_linops.f90:252)
         call nlg_check(c_linop_set_tau(exptA_handle(self), self%tau), where); self%tau_built = self%tau
      end if
   end subroutine

   subroutine exptA_matvec(self, vec_in, vec_out)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call sync_tau(self, 'exptA_matvec')
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            call nek_dvector_ensure(vec_out)
            call nlg_check(c_linop_matvec(exptA_handle(self), nek_dvector_handle(vec_in), vec_out%h), 'exptA_matvec')
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'exptA_matvec')
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'exptA_matvec')
      end select
   end subroutine

   subroutine exptA_rmatvec(self, vec_in, vec_out)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call sync_tau(self, 'exptA_rmatvec')
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            call nek_dvector_ensure(vec_out)
            call nlg_check(c_linop_rmatvec(exptA_handle(self), nek_dvector_handle(vec_in), vec_out%h), 'exptA_rmatvec')
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'exptA_rmatvec')
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'exptA_rmatvec')
      end select
   end subroutine

   !> exptA_compute_rst (exponential_propagator.f90:109-127).  In the reference the matvec calls it after the final state
   !! has been copied out, to run `nrst` extra steps that fill the history of vec_out.  The device matvec does exactly that
   !! internally (the integrator state lives on the device), so the history is already in place when the matvec returns:
   !! this binding exists for callers that invoke it themselves and only checks that claim.
   subroutine exptA_compute_rst(self, vec_out, nrst)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(inout) :: vec_out
      integer, intent(in) :: nrst
      integer(c_int) :: have
      select type (vec_out)
      type is (nek_dvector)
         call nlg_check(c_vec_nrst(nek_dvector_handle(vec_out), have), 'exptA_compute_rst')
         if (have < nrst) then
            write (*, '(A,I0,A,I0)') 'ERROR in exptA_compute_rst: the vector holds ', have, ' restart fields, expected ', nrst
            error stop 1
         end if
      class default
         call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'exptA_compute_rst')
      end select
   end subroutine

   !> exptA_get_rst (exponential_propagator.f90:129-142): replay of vec_in's history slot `istep` -- performed inside the
   !! device matvec after time step istep <= nrst whenever vec_in%has_rst_fields(); kept for interface completeness.
   subroutine exptA_get_rst(self, vec_in, istep)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      integer, intent(in) :: istep
      select type (vec_in)
      type is (nek_dvector)
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'exptA_get_rst')
      end select
   end subroutine

   subroutine exptA_nonlinear_map(self, vec_in, vec_out)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            call nek_dvector_ensure(vec_out)
            call nlg_check(c_linop_nonlinear_map(exptA_handle(self), nek_dvector_handle(vec_in), vec_out%h), 'nonlinear_map')
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'nonlinear_map')
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'nonlinear_map')
      end select
   end subroutine

   subroutine exptA_set_baseflow(self, X)
      class(exptA_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: X
      select type (X)
      type is (nek_dvector)
         call nlg_check(c_linop_set_baseflow(exptA_handle(self), nek_dvector_handle(X)), 'set_baseflow')
      class default
         call type_error('X', 'nek_dvector', 'IN', this_module, 'set_baseflow')
      end select
   end subroutine

   subroutine exptA_set_tolerances(self, vtol, ptol)
      class(exptA_linop), intent(inout) :: self
      real(dp), intent(in) :: vtol, ptol
      call nlg_check(c_linop_set_tolerances(exptA_handle(self), vtol, ptol), 'set_tolerances')
   end subroutine

   !> vec_out = state after one application started from `ic` (absent: rest) under the body force
   !! Re[(f_re + i f_im) exp(+- i omega t)]  (resolvent.f90:80-111, :133-166)
   subroutine exptA_integrate_forced(self, f_re, omega, vec_out, ic, f_im, adjoint)
      class(exptA_linop), intent(inout) :: self
      type(nek_dvector), intent(in) :: f_re
      real(dp), intent(in) :: omega
      type(nek_dvector), intent(inout) :: vec_out
      type(nek_dvector), optional, intent(in) :: ic, f_im
      logical, optional, intent(in) :: adjoint
      type(c_ptr) :: hic, him
      integer(c_int) :: adj
      hic = c_null_ptr; him = c_null_ptr; adj = 0
      if (present(ic)) hic = nek_dvector_handle(ic)
      if (present(f_im)) him = nek_dvector_handle(f_im)
      if (present(adjoint)) adj = merge(1, 0, adjoint)
      call sync_tau(self, 'integrate_forced')
      call nek_dvector_ensure(vec_out)
      call nlg_check(c_linop_integrate_forced(exptA_handle(self), hic, nek_dvector_handle(f_re), him, omega, adj, vec_out%h), 'integrate_forced')
   end subroutine

   subroutine finalize_exptA(self)
      type(exptA_linop), intent(inout) :: self
      integer(c_int) :: rc
      if (c_associated(self%h) .and. self%owner == loc(self)) rc = c_linop_destroy(self%h)
      self%h = c_null_ptr; self%owner = 0
   end subroutine

   !---- nek_otd ------------------------------------------------------------------------------------------------------
   function otd_handle(self) result(h)
      class(nek_otd), intent(in) :: self
      type(c_ptr) :: h
      if (.not. c_associated(self%h) .or. self%owner /= loc(self)) then
         write (*, '(A)') 'ERROR in '//this_module//': OTD%init() has not been called on this object'
         error stop 1
      end if
      h = self%h
   end function

   subroutine otd_close(self)
      class(nek_otd), intent(inout) :: self
      integer(c_int) :: rc
      if (self%owner == loc(self)) then
         if (c_associated(self%hlns)) rc = c_lns_destroy(self%hlns)
         if (c_associated(self%h)) rc = c_otd_destroy(self%h)
         if (c_associated(self%hop)) rc = c_linop_destroy(self%hop)
      end if
      self%h = c_null_ptr; self%hop = c_null_ptr; self%hlns = c_null_ptr; self%owner = 0
   end subroutine

   subroutine finalize_otd(self)
      type(nek_otd), intent(inout) :: self
      call otd_close(self)
   end subroutine

   !> init_OTD (src/neklab_otd.f90:118-204).  `basis` allocated with r vectors on entry: they are the initial conditions;
   !! otherwise the library draws r random modes (seeds 1 .. r).  Either way the basis is orthonormalised (twice).
   subroutine init_OTD(self, opts)
      class(nek_otd), intent(inout) :: self
      type(otd_opts), intent(in) :: opts
      type(nlg_otd_opts) :: o
      type(c_ptr), allocatable, target :: hb(:)
      integer :: i
      call otd_close(self)
      if (.not. self%cfg_set) then
         self%cfg = nek_case
         self%cfg%cfl_limit = 0.4_dp                ! setup_linear_solver(cfl_limit = 0.4_dp), neklab_otd.f90:203
      end if
      if (self%cfg%dt > 0.0_dp) self%cfg%tau = self%cfg%dt      ! OTD has no tau: the step is the given one, not tau / ceil(tau / dt)
      call nlg_check(c_linop_create(nlg_mesh, self%cfg, nek_dvector_handle(self%baseflow), self%hop), 'init_OTD')
      self%owner = loc(self)
      o%r = self%r; o%startstep = opts%startstep; o%orthostep = opts%orthostep
      o%trans = merge(1, 0, opts%trans); o%solve_baseflow = merge(1, 0, opts%solve_baseflow)
      self%moving = opts%solve_baseflow
      if (allocated(self%basis)) then
         if (size(self%basis) /= self%r) then
            write (*, '(A,I0,A,I0)') 'ERROR in '//this_module//': init_OTD: ', size(self%basis), ' initial conditions for r = ', self%r
            error stop 1
         end if
         allocate (hb(self%r))
         do i = 1, self%r
            hb(i) = nek_dvector_handle(self%basis(i))
         end do
         call nlg_check(c_otd_create(self%hop, o, c_loc(hb), self%h), 'init_OTD')
      else
         call nlg_check(c_otd_create(self%hop, o, c_null_ptr, self%h), 'init_OTD')
         allocate (self%basis(self%r))
      end if
      call otd_get_basis(self)
   end subroutine

   subroutine otd_advance(self, nsteps)
      class(nek_otd), intent(inout) :: self
      integer, intent(in) :: nsteps
      call nlg_check(c_otd_advance(otd_handle(self), int(nsteps, c_int)), 'otd_advance')
   end subroutine

   !> orthonormalise, then Lr_ij = <u_i, L u_j> on the current state; G (optional): the Gram matrix before
   subroutine otd_reduced(self, Lr, G)
      class(nek_otd), intent(inout) :: self
      real(dp), intent(out) :: Lr(self%r, self%r)
      real(dp), intent(out), optional :: G(self%r, self%r)
      real(dp) :: Gl(self%r, self%r)
      call nlg_check(c_otd_reduced(otd_handle(self), Lr, Gl), 'otd_reduced')
      if (present(G)) G = Gl
   end subroutine

   !> the current modes -> self%basis
   subroutine otd_get_basis(self)
      class(nek_otd), intent(inout) :: self
      integer :: i
      do i = 1, self%r
         call nek_dvector_ensure(self%basis(i))
         call nlg_check(c_otd_get_basis(otd_handle(self), int(i - 1, c_int), self%basis(i)%h), 'otd_get_basis')
      end do
   end subroutine

   subroutine otd_get_baseflow(self, vec_out)
      class(nek_otd), intent(in) :: self
      type(nek_dvector), intent(inout) :: vec_out
      call nek_dvector_ensure(vec_out)
      call nlg_check(c_otd_get_baseflow(otd_handle(self), vec_out%h), 'otd_get_baseflow')
   end subroutine

   subroutine otd_info(self, istep, time, dt)
      class(nek_otd), intent(in) :: self
      integer, intent(out) :: istep
      real(dp), intent(out) :: time, dt
      integer(c_int64_t) :: is
      call nlg_check(c_otd_info(otd_handle(self), is, time, dt), 'otd_info')
      istep = int(is)
   end subroutine

   !> spectral_analysis (src/neklab_otd.f90:206-265) without the log files (otd_analysis writes them): sigma = eigenvalues of
   !! (Lr + Lr^T) / 2, descending, with vectors; lambda = eigenvalues of Lr by real part, descending, with vectors
   subroutine otd_spectral_analysis(self, Lr, sigma, svec, lambda, eigvec)
      class(nek_otd), intent(in) :: self
      real(dp), intent(in) :: Lr(self%r, self%r)
      real(dp), intent(out) :: sigma(self%r), svec(self%r, self%r)
      complex(dp), intent(out) :: lambda(self%r), eigvec(self%r, self%r)
      real(dp) :: A(self%r, self%r), wr(self%r), wi(self%r), vr(self%r, self%r)
      complex(dp) :: l(self%r), v(self%r, self%r)
      integer :: r, j, idx(self%r)
      r = self%r
      A = 0.5_dp*(Lr + transpose(Lr))
      call nlg_check(c_dense_eig(int(r, c_int), A, int(r, c_int), wr, wi, vr, int(r, c_int)), 'otd_spectral_analysis')
      call order_desc(wr, idx)
      do j = 1, r
         sigma(j) = wr(idx(j)); svec(:, j) = vr(:, idx(j))
      end do
      A = Lr
      call nlg_check(c_dense_eig(int(r, c_int), A, int(r, c_int), wr, wi, vr, int(r, c_int)), 'otd_spectral_analysis')
      j = 1
      do while (j <= r)                       ! LAPACK's real convention: a complex pair is (Re, Im) in consecutive columns
         if (wi(j) /= 0.0_dp .and. j < r) then
            l(j) = cmplx(wr(j), wi(j), dp); l(j + 1) = cmplx(wr(j + 1), wi(j + 1), dp)
            v(:, j) = cmplx(vr(:, j), vr(:, j + 1), dp); v(:, j + 1) = conjg(v(:, j))
            j = j + 2
         else
            l(j) = cmplx(wr(j), 0.0_dp, dp); v(:, j) = cmplx(vr(:, j), 0.0_dp, dp)
            j = j + 1
         end if
      end do
      call order_desc(wr, idx)
      do j = 1, r
         lambda(j) = l(idx(j)); eigvec(:, j) = v(:, idx(j))
      end do
   contains
      subroutine order_desc(x, ix)          ! stable insertion sort of the indices, largest first
         real(dp), intent(in) :: x(:)
         integer, intent(out) :: ix(:)
         integer :: a, b, t
         do a = 1, size(x)
            ix(a) = a
         end do
         do a = 2, size(x)
            t = ix(a); b = a - 1
            do while (b >= 1)
               if (x(ix(b)) >= x(t)) exit
               ix(b + 1) = ix(b); b = b - 1
            end do
            ix(b + 1) = t
         end do
      end subroutine
   end subroutine

   !---- exptA_proj_linop ---------------------------------------------------------------------------------------------
   !> after init(): line labels of the velocity points (and, optionally, of the pressure points with their coordinate along
   !! idir: the pressure is then projected as well, see include/neklab_gpu.h nlg_linop_set_projection)
   subroutine proj_set_lines(self, line_label, line_label2, x2)
      class(exptA_proj_linop), intent(inout) :: self
      integer(c_int64_t), target, intent(in) :: line_label(*)
      integer(c_int64_t), target, optional, intent(in) :: line_label2(*)
      real(dp), target, optional, intent(in) :: x2(*)
      type(c_ptr) :: l2, xx
      l2 = c_null_ptr; xx = c_null_ptr
      if (present(line_label2) .and. present(x2)) then
         l2 = c_loc(line_label2); xx = c_loc(x2)
      end if
      call nlg_check(c_linop_set_projection(exptA_handle(self), self%alpha, int(self%idir, c_int), c_loc(line_label), l2, xx), 'exptA_proj set_lines')
   end subroutine

   !> proj_alpha (exponential_propagator_proj.f90:135-173) applied to the state held by `vec`
   subroutine proj_apply(self, vec)
      class(exptA_proj_linop), intent(inout) :: self
      type(nek_dvector), intent(inout) :: vec
      call nek_dvector_ensure(vec)
      call nlg_check(c_linop_project(exptA_handle(self), vec%h), 'exptA_proj proj')
   end subroutine

   !---- resolvent ------------------------------------------------------------------------------------------------------
   subroutine resolvent_apply(self, vec_in, vec_out, adjoint)
      class(resolvent_linop), intent(inout) :: self
      class(abstract_vector_cdp), intent(in) :: vec_in
      class(abstract_vector_cdp), intent(out) :: vec_out
      logical, intent(in) :: adjoint
      real(dp), parameter :: two_pi = 8.0_dp*atan(1.0_dp)
      type(exptA_linop) :: exptA
      type(nek_dvector) :: b
      real(dp) :: tau
      tau = 1.0_dp
      if (self%omega /= 0.0_dp) tau = two_pi/abs(self%omega)
      exptA%tau = tau; exptA%baseflow = self%baseflow
      call exptA%init()
      select type (vec_in)
      type is (nek_zvector)
         select type (vec_out)
         type is (nek_zvector)
            call exptA%integrate_forced(vec_in%re, self%omega, b, f_im=vec_in%im, adjoint=adjoint)      ! evaluate_rhs
            call solve_real_part(exptA, b, vec_out%re, adjoint)
            exptA%tau = 0.25_dp*tau                                                                      ! resolvent.f90:35
            call exptA%integrate_forced(vec_in%re, self%omega, vec_out%im, ic=vec_out%re, f_im=vec_in%im, adjoint=adjoint)
         class default
            call type_error('vec_out', 'nek_zvector', 'OUT', this_module, 'resolvent_matvec')
         end select
      class default
         call type_error('vec_in', 'nek_zvector', 'IN', this_module, 'resolvent_matvec')
      end select
   end subroutine

   subroutine resolvent_matvec(self, vec_in, vec_out)
      class(resolvent_linop), intent(inout) :: self
      class(abstract_vector_cdp), intent(in) :: vec_in
      class(abstract_vector_cdp), intent(out) :: vec_out
      call resolvent_apply(self, vec_in, vec_out, .false.)
   end subroutine

   subroutine resolvent_rmatvec(self, vec_in, vec_out)
      class(resolvent_linop), intent(inout) :: self
      class(abstract_vector_cdp), intent(in) :: vec_in
      class(abstract_vector_cdp), intent(out) :: vec_out
      call resolvent_apply(self, vec_in, vec_out, .true.)
   end subroutine

   !> (I - exp(T L)) x = b, x0 = 0, restarted GMRES(64) with Givens rotations, |r| <= max(1e-6 |b|, 1e-12).  Krylov vectors lose their
   !! restart history (each application starts impulsively, like the forced integration whose periodic state is sought).
   subroutine solve_real_part(exptA, b, x, adjoint)
      type(exptA_linop), intent(inout) :: exptA
      type(nek_dvector), intent(in) :: b
      type(nek_dvector), intent(inout) :: x
      logical, intent(in) :: adjoint
      integer, parameter :: kd = 64, maxcycle = 10
      type(nek_dvector), allocatable :: V(:)
      type(nek_dvector) :: w
      real(dp) :: H(kd + 1, kd), cs(kd), sn(kd), g(kd + 1), y(kd), beta, t, d, tol
      integer :: k, i, j, cyc
      tol = max(1.0e-6_dp*b%norm(), 1.0e-12_dp)
      call x%zero()
      allocate (V(kd + 1))
      do cyc = 1, maxcycle
         call V(1)%zero(); call V(1)%axpby(1.0_dp, b, 0.0_dp)
         if (cyc > 1) then                                   ! r = b - (x - A x)
            if (adjoint) then
               call exptA%rmatvec(x, w)
            else
               call exptA%matvec(x, w)
            end if
            call w%clear_rst_fields()
            call V(1)%axpby(-1.0_dp, x, 1.0_dp); call V(1)%axpby(1.0_dp, w, 1.0_dp)
         end if
         beta = V(1)%norm()
         if (beta <= tol) return
         call V(1)%scal(1.0_dp/beta)
         H = 0.0_dp; g = 0.0_dp; g(1) = beta; k = 0
         do j = 1, kd
            if (adjoint) then
               call exptA%rmatvec(V(j), V(j + 1))
            else
               call exptA%matvec(V(j), V(j + 1))
            end if
            call V(j + 1)%clear_rst_fields()
            call V(j + 1)%axpby(1.0_dp, V(j), -1.0_dp)         ! (I - A) v_j
            do i = 1, j
               H(i, j) = V(i)%dot(V(j + 1)); call V(j + 1)%axpby(-H(i, j), V(i), 1.0_dp)
            end do
            H(j + 1, j) = V(j + 1)%norm()
            if (H(j + 1, j) > 0.0_dp) call V(j + 1)%scal(1.0_dp/H(j + 1, j))
            do i = 1, j - 1
               t = cs(i)*H(i, j) + sn(i)*H(i + 1, j); H(i + 1, j) = -sn(i)*H(i, j) + cs(i)*H(i + 1, j); H(i, j) = t
            end do
            d = hypot(H(j, j), H(j + 1, j)); cs(j) = H(j, j)/d; sn(j) = H(j + 1, j)/d
            H(j, j) = d; H(j + 1, j) = 0.0_dp
            g(j + 1) = -sn(j)*g(j); g(j) = cs(j)*g(j)
            k = j
            if (abs(g(j + 1)) <= tol) exit
         end do
         do i = k, 1, -1
            y(i) = (g(i) - dot_product(H(i, i + 1:k), y(i + 1:k)))/H(i, i)
         end do
         do i = 1, k
            call x%axpby(y(i), V(i), 1.0_dp)
         end do
         if (abs(g(k + 1)) <= tol) return
      end do
   end subroutine

   !---- the operator L itself -------------------------------------------------------------------------------------------
   !> one vector through nlg_lns_apply
   subroutine lns_apply_one(h, vec_in, vec_out, trans, coef, where)
      type(c_ptr), intent(in) :: h
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(inout) :: vec_out
      logical, intent(in) :: trans
      real(dp), intent(in) :: coef(3)
      character(len=*), intent(in) :: where
      type(c_ptr) :: hi(1), ho(1)
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            call nek_dvector_ensure(vec_out)
            hi(1) = nek_dvector_handle(vec_in); ho(1) = vec_out%h
            call nlg_check(c_lns_apply(h, 1_c_int, hi, ho, merge(1_c_int, 0_c_int, trans), coef), where)
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, where)
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, where)
      end select
   end subroutine

   subroutine init_lns(self)
      class(lns_linop), intent(inout) :: self
      integer(c_int) :: rc
      if (c_associated(self%h) .and. self%owner == loc(self)) rc = c_lns_destroy(self%h)
      self%h = c_null_ptr
      if (self%re <= 0.0_dp) self%re = nek_case%re
      call nlg_check(c_lns_create(nlg_mesh, nek_dvector_handle(self%baseflow), self%re, self%h), 'init_lns')
      self%owner = loc(self)
   end subroutine

   function lns_handle(self) result(h)
      class(lns_linop), intent(in) :: self
      type(c_ptr) :: h
      if (.not. c_associated(self%h) .or. self%owner /= loc(self)) then
         write (*, '(A)') 'ERROR in '//this_module//': lns_linop%init() has not been called on this object'
         error stop 1
      end if
      h = self%h
   end function

   subroutine lns_matvec(self, vec_in, vec_out)
      class(lns_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call lns_apply_one(lns_handle(self), vec_in, vec_out, .false., coef_L, 'lns_matvec')
   end subroutine

   subroutine lns_rmatvec(self, vec_in, vec_out)
      class(lns_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call lns_apply_one(lns_handle(self), vec_in, vec_out, .true., coef_L, 'lns_rmatvec')
   end subroutine

   subroutine finalize_lns(self)
      type(lns_linop), intent(inout) :: self
      integer(c_int) :: rc
      if (c_associated(self%h) .and. self%owner == loc(self)) rc = c_lns_destroy(self%h)
      self%h = c_null_ptr; self%owner = 0
   end subroutine

   !> nek_otd%matvec / rmatvec (apply_LNS / apply_adjLNS, src/neklab_otd.f90:76-116)
   subroutine otd_apply_lns(self, vec_in, vec_out, trans, where)
      class(nek_otd), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(inout) :: vec_out
      logical, intent(in) :: trans
      character(len=*), intent(in) :: where
      if (self%owner /= loc(self)) then
         if (self%owner /= 0) then
            write (*, '(A)') 'ERROR in '//this_module//': '//where//': this nek_otd is a copy of an initialised one: call init() on it'
            error stop 1
         end if
         self%owner = loc(self)      ! before init(): about the frozen base flow, with the case's Re
         if (.not. self%cfg_set) self%cfg = nek_case
      end if
      if (.not. c_associated(self%hlns)) &
         call nlg_check(c_lns_create(nlg_mesh, nek_dvector_handle(self%baseflow), self%cfg%re, self%hlns), where)
      if (self%moving .and. c_associated(self%h)) then
         call nek_dvector_ensure(self%bf_now)
         call nlg_check(c_otd_get_baseflow(self%h, self%bf_now%h), where)
         call nlg_check(c_lns_set_baseflow(self%hlns, self%bf_now%h), where)
      end if
      call lns_apply_one(self%hlns, vec_in, vec_out, trans, coef_L, where)
   end subroutine

   subroutine apply_LNS(self, vec_in, vec_out)
      class(nek_otd), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call otd_apply_lns(self, vec_in, vec_out, .false., 'apply_LNS')
   end subroutine

   subroutine apply_adjLNS(self, vec_in, vec_out)
      class(nek_otd), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call otd_apply_lns(self, vec_in, vec_out, .true., 'apply_adjLNS')
   end subroutine

   subroutine otd_linop_matvec(self, vec_in, vec_out)
      class(nek_otd_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      if (.not. associated(self%otd)) then
         write (*, '(A)') 'ERROR in '//this_module//': nek_otd_linop%otd points to no nek_otd'
         error stop 1
      end if
      call otd_apply_lns(self%otd, vec_in, vec_out, .false., 'apply_LNS')
   end subroutine

   subroutine otd_linop_rmatvec(self, vec_in, vec_out)
      class(nek_otd_linop), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      if (.not. associated(self%otd)) then
         write (*, '(A)') 'ERROR in '//this_module//': nek_otd_linop%otd points to no nek_otd'
         error stop 1
      end if
      call otd_apply_lns(self%otd, vec_in, vec_out, .true., 'apply_adjLNS')
   end subroutine

   !> apply_exptA (src/linops/neklab_linops.f90:224-266): the interface expmlib expects, on top of matvec / rmatvec
   subroutine apply_exptA(vec_out, A, vec_in, tau, info, trans)
      class(abstract_vector_rdp), intent(out) :: vec_out
      class(abstract_linop_rdp), intent(inout) :: A
      class(abstract_vector_rdp), intent(in) :: vec_in
      real(dp), intent(in) :: tau
      integer, intent(out) :: info
      logical, optional, intent(in) :: trans
      logical :: transpose
      transpose = .false.
      if (present(trans)) transpose = trans
      info = 0
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            select type (A)
            class is (abstract_exptA_linop_rdp)
               A%tau = tau
               if (transpose) then
                  call A%rmatvec(vec_in, vec_out)
               else
                  call A%matvec(vec_in, vec_out)
               end if
            class default
               call type_error('A', 'abstract_exptA_linop', 'INOUT', this_module, 'apply_exptA')
            end select
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'apply_exptA')
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'apply_exptA')
      end select
   end subroutine

   !> the base flow of the array routines below (the reference reads Nek5000's vx, vy, vz); Re is the case's
   subroutine set_lns_baseflow(bf)
      type(nek_dvector), intent(in) :: bf
      if (c_associated(lns_arrays_h)) then
         call nlg_check(c_lns_set_baseflow(lns_arrays_h, nek_dvector_handle(bf)), 'set_lns_baseflow')
         call nlg_check(c_lns_set_re(lns_arrays_h, nek_case%re), 'set_lns_baseflow')
      else
         call nlg_check(c_lns_create(nlg_mesh, nek_dvector_handle(bf), nek_case%re, lns_arrays_h), 'set_lns_baseflow')
      end if
   end subroutine

   !> host arrays (Nek5000's element-major layout) -> scratch vector -> nlg_lns_apply -> host arrays.  u / p absent: zero
   subroutine lns_arrays(who, coef, trans, ox, oy, oz, ux, uy, uz, pp)
      character(len=*), intent(in) :: who
      real(dp), intent(in) :: coef(3)
      logical, intent(in) :: trans
      real(dp), intent(inout) :: ox(*), oy(*), oz(*)
      real(dp), optional, intent(in) :: ux(*), uy(*), uz(*), pp(*)
      type(c_ptr) :: hi(1), ho(1)
      if (.not. c_associated(lns_arrays_h)) then
         write (*, '(A)') 'ERROR in '//this_module//': '//who//': no base flow: call set_lns_baseflow(bf) first'
         error stop 1
      end if
      call nek_dvector_ensure(lns_arrays_in); call nek_dvector_ensure(lns_arrays_out)
      call nlg_check(c_vec_zero(lns_arrays_in%h), who)
      if (present(ux)) then
         call nlg_check(c_vec_set_field(lns_arrays_in%h, 0_c_int, 0_c_int, ux, nek_lvn), who)
         call nlg_check(c_vec_set_field(lns_arrays_in%h, 1_c_int, 0_c_int, uy, nek_lvn), who)
         if (nek_ldim == 3) call nlg_check(c_vec_set_field(lns_arrays_in%h, 2_c_int, 0_c_int, uz, nek_lvn), who)
      end if
      if (present(pp)) call nlg_check(c_vec_set_field(lns_arrays_in%h, 3_c_int, 0_c_int, pp, nek_lpn), who)
      hi(1) = lns_arrays_in%h; ho(1) = lns_arrays_out%h
      call nlg_check(c_lns_apply(lns_arrays_h, 1_c_int, hi, ho, merge(1_c_int, 0_c_int, trans), coef), who)
      call nlg_check(c_vec_get_field(lns_arrays_out%h, 0_c_int, 0_c_int, ox, nek_lvn), who)
      call nlg_check(c_vec_get_field(lns_arrays_out%h, 1_c_int, 0_c_int, oy, nek_lvn), who)
      if (nek_ldim == 3) call nlg_check(c_vec_get_field(lns_arrays_out%h, 2_c_int, 0_c_int, oz, nek_lvn), who)
   end subroutine

   logical function is_trans(trans)
      logical, optional, intent(in) :: trans
      is_trans = .false.
      if (present(trans)) is_trans = trans
   end function

   subroutine compute_LNS_conv(c_x, c_y, c_z, uxp, uyp, uzp, trans)
      real(dp), intent(inout) :: c_x(*), c_y(*), c_z(*)
      real(dp), intent(in) :: uxp(*), uyp(*), uzp(*)
      logical, optional :: trans
      call lns_arrays('compute_LNS_conv', coef_conv, is_trans(trans), c_x, c_y, c_z, uxp, uyp, uzp)
   end subroutine

   subroutine compute_LNS_laplacian(d_x, d_y, d_z, uxp, uyp, uzp)
      real(dp), intent(inout) :: d_x(*), d_y(*), d_z(*)
      real(dp), intent(in) :: uxp(*), uyp(*), uzp(*)
      call lns_arrays('compute_LNS_laplacian', coef_lap, .false., d_x, d_y, d_z, uxp, uyp, uzp)
   end subroutine

   subroutine compute_LNS_gradp(gp_x, gp_y, gp_z, pp)
      real(dp), intent(inout) :: gp_x(*), gp_y(*), gp_z(*)
      real(dp), intent(in) :: pp(*)
      call lns_arrays('compute_LNS_gradp', coef_gradp, .false., gp_x, gp_y, gp_z, pp=pp)
   end subroutine

   subroutine apply_L(Lux, Luy, Luz, ux, uy, uz, pres, trans)
      real(dp), intent(inout) :: Lux(*), Luy(*), Luz(*)
      real(dp), intent(in) :: ux(*), uy(*), uz(*), pres(*)
      logical, optional, intent(in) :: trans
      call lns_arrays('apply_L', coef_L, is_trans(trans), Lux, Luy, Luz, ux, uy, uz, pres)
   end subroutine

   subroutine apply_Lv(Lux, Luy, Luz, ux, uy, uz, trans)
      real(dp), intent(inout) :: Lux(*), Luy(*), Luz(*)
      real(dp), intent(in) :: ux(*), uy(*), uz(*)
      logical, optional, intent(in) :: trans
      call lns_arrays('apply_Lv', coef_Lv, is_trans(trans), Lux, Luy, Luz, ux, uy, uz)
   end subroutine

   !---- eigs / svds on the device block path ---------------------------------------------------------------------------
   !> Same argument list as the LightKrylov call at src/neklab_analysis.f90:80-81; the Krylov basis lives in one
   !! allocation on the device and every Gram-Schmidt pass is two kernels and one all-reduce (nlg_eigs).
   subroutine nek_eigs(A, X, eigvals, residuals, info, x0, kdim, tolerance, transpose, write_intermediate)
      class(exptA_linop), intent(inout) :: A
      type(nek_dvector), intent(inout) :: X(:)
      complex(dp), allocatable, intent(out) :: eigvals(:)
      real(dp), allocatable, intent(out) :: residuals(:)
      integer, intent(out) :: info
      type(nek_dvector), optional, intent(in) :: x0
      integer, optional, intent(in) :: kdim
      real(dp), optional, intent(in) :: tolerance
      logical, optional, intent(in) :: transpose, write_intermediate
      type(nlg_eigs_opts) :: o
      type(c_ptr), allocatable :: hx(:)
      type(c_ptr) :: h0
      real(dp), allocatable :: re(:), im(:)
      integer(c_int) :: cinfo
      integer :: i, nev
      nev = size(X)
      call nlg_check(c_eigs_opts_default(o), 'nek_eigs')
      if (present(kdim)) o%kdim = kdim
      if (present(tolerance)) o%tol = tolerance
      if (present(transpose)) o%transpose = merge(1, 0, transpose)
      o%write_intermediate = 0
      if (present(write_intermediate)) o%write_intermediate = merge(1, 0, write_intermediate)
      allocate (hx(nev), re(nev), im(nev), residuals(nev), eigvals(nev))
      do i = 1, nev
         call nek_dvector_ensure(X(i)); hx(i) = X(i)%h
      end do
      h0 = c_null_ptr
      if (present(x0)) h0 = nek_dvector_handle(x0)
      call sync_tau(A, 'nek_eigs')
      call nlg_check(c_eigs(exptA_handle(A), hx, int(nev, c_int), re, im, residuals, cinfo, h0, o), 'nek_eigs')
      info = cinfo
      eigvals = cmplx(re, im, kind=dp)
   end subroutine

   !> svds(exptA, U, S, V, residuals, info, kdim=, write_intermediate=) of src/neklab_analysis.f90:136 (nlg_svds)
   subroutine nek_svds(A, U, S, V, residuals, info, u0, kdim, tolerance, write_intermediate)
      class(exptA_linop), intent(inout) :: A
      type(nek_dvector), intent(inout) :: U(:), V(:)
      real(dp), allocatable, intent(out) :: S(:), residuals(:)
      integer, intent(out) :: info
      type(nek_dvector), optional, intent(in) :: u0
      integer, optional, intent(in) :: kdim
      real(dp), optional, intent(in) :: tolerance
      logical, optional, intent(in) :: write_intermediate
      type(nlg_eigs_opts) :: o
      type(c_ptr), allocatable :: hu(:), hv(:)
      type(c_ptr) :: h0
      integer(c_int) :: cinfo
      integer :: i, nsv
      nsv = size(U)
      call nlg_check(c_eigs_opts_default(o), 'nek_svds')
      if (present(kdim)) o%kdim = kdim
      if (present(tolerance)) o%tol = tolerance
      o%write_intermediate = 0
      if (present(write_intermediate)) o%write_intermediate = merge(1, 0, write_intermediate)
      allocate (hu(nsv), hv(nsv), S(nsv), residuals(nsv))
      do i = 1, nsv
         call nek_dvector_ensure(U(i)); hu(i) = U(i)%h
         call nek_dvector_ensure(V(i)); hv(i) = V(i)%h
      end do
      h0 = c_null_ptr
      if (present(u0)) h0 = nek_dvector_handle(u0)
      call sync_tau(A, 'nek_svds')
      call nlg_check(c_svds(exptA_handle(A), hu, hv, int(nsv, c_int), S, residuals, cinfo, h0, o), 'nek_svds')
      info = cinfo
   end subroutine

end module neklab_linops
