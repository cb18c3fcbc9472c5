!> Drop-in for the fixed-point part of the reference's module of the same name (SURVEY.md 8f row 3):
!!   nek_system   / nek_jacobian        /root/reference/src/systems/neklab_systems.f90:42-55,  fixed_point.f90:4-96
!!   nek_temp_system / nek_temp_jacobian                      neklab_systems.f90:97-110, fixed_point_temp.f90 (the same with the
!!        temperature: here the case's `ifheat` decides, the types are the first pair under the reference's second names; the
!!        reference's umbrella module and its thermosyphon case spell them nek_system_temp / nek_jacobian_temp,
!!        src/neklab.f90:63-64, examples/thermosyphon/baseflow/tsyphon.usr:13,38-39 -- both spellings exist here)
!!   nek_constant_tol / nek_dynamic_tol  neklab_systems.f90:229-335
!!   nek_upo_system / nek_upo_jacobian    neklab_systems.f90:147-223, periodic_orbit.f90 (below, with gmres_upo)
!! The reference integrates with Nek5000's global solver state; here each system / Jacobian owns a device propagator
!! (exptA_linop) over the horizon `endtime` of the case (neklab_gpu_set_case(endtime=..): Nek5000's endTime, which
!! setup_nonlinear_solver integrates to) and forwards:
!!   response(X, F, atol)  ->  nlg_linop_nonlinear_map at tolerances 0.1 atol, CFL limit 0.4   (fixed_point.f90:4-38)
!!   jacobian%matvec       ->  nlg_linop_set_baseflow(X), tolerances 0.5 atol, exptA matvec, minus the input
!!                              (fixed_point.f90:40-96); rmatvec likewise with the adjoint propagator
module neklab_systems
   use iso_c_binding
   use LightKrylov, only: dp, atol_dp, abstract_vector_rdp, abstract_linop_rdp, abstract_system_rdp, abstract_jacobian_linop_rdp, type_error
   use neklab_gpu_capi
   use neklab_vectors
   use neklab_linops
   implicit none
   private
   character(len=*), parameter, private :: this_module = 'neklab_systems'

   public :: nek_constant_tol, nek_dynamic_tol

   type, extends(abstract_system_rdp), public :: nek_system
      type(exptA_linop), allocatable, private :: prop      ! allocatable: `nek_system()` (tsyphon.usr:38) names no component
      logical, private :: ready = .false.
   contains
      private
      procedure, pass(self), public :: response => nonlinear_map
   end type nek_system

   type, extends(abstract_jacobian_linop_rdp), public :: nek_jacobian
      type(exptA_linop), allocatable, private :: prop
      logical, private :: ready = .false.
   contains
      private
      procedure, pass(self), public :: matvec => jac_exptA_matvec
      procedure, pass(self), public :: rmatvec => jac_exptA_rmatvec
   end type nek_jacobian

   type, extends(nek_system), public :: nek_temp_system
   end type
   type, extends(nek_jacobian), public :: nek_temp_jacobian
   end type
   type, extends(nek_system), public :: nek_system_temp
   end type
   type, extends(nek_jacobian), public :: nek_jacobian_temp
   end type

   !> nek_upo_system / nek_upo_jacobian (neklab_systems.f90:147-223, src/systems/periodic_orbit.f90): Newton-Krylov for a periodic
   !! orbit on nek_ext_dvector = (state, period).  Each owns one device propagator in orbit mode and forwards
   !!   response(X, F, atol)  ->  nlg_linop_set_orbit_steps(X, T), tolerances 0.1 atol, nlg_upo_residual; F%T = 0      (:4-45)
   !!   jacobian%matvec       ->  the same state call about self%X, tolerances 0.1 of the scheduler's, nlg_upo_jac_matvec:
   !!                              (M - I) dx + dT fT, <f0, dx>                                                        (:47-115)
   !!   jacobian%rmatvec      ->  stops: orbit mode has no adjoint (jac_adjoint_map is not built)
   !! compute_rst / get_rst as exptA_linop has them: the device matvec does both internally.  The umbrella's names
   !! nek_system_upo / nek_jacobian_upo (src/neklab.f90:63-64) exist as well.  upo_fixed_nsteps > 0 pins the step count of the orbit
   !! (0: the CFL rule with cfl_limit 0.4, or the case's dt, applied to every new (X, T)).  The system and the Jacobian are separate
   !! objects here as in the reference, so each holds an operator of its own (work buffers and the two derivative vectors twice);
   !! matvec sets the state about self%X -- a full operator set-up -- on every application, gmres_upo once per solve.
   type, extends(abstract_system_rdp), public :: nek_upo_system
      type(exptA_orbit_linop), allocatable, private :: prop
      logical, private :: ready = .false.
   contains
      private
      procedure, pass(self), public :: response => nonlinear_map_upo
   end type nek_upo_system

   type, extends(abstract_jacobian_linop_rdp), public :: nek_upo_jacobian
      type(exptA_orbit_linop), allocatable, private :: prop
      logical, private :: ready = .false.
   contains
      private
      procedure, pass(self), public :: matvec => jac_direct_map
      procedure, pass(self), public :: rmatvec => jac_adjoint_map
      procedure, pass(self), public :: compute_rst => jac_compute_rst
      procedure, pass(self), public :: get_rst => jac_get_rst
   end type nek_upo_jacobian

   type, extends(nek_upo_system), public :: nek_system_upo
   end type
   type, extends(nek_upo_jacobian), public :: nek_jacobian_upo
   end type

   integer, save, public :: upo_fixed_nsteps = 0, upo_gmres_kdim = 30
   public :: gmres_upo

   !> Forces, torque and heat flux on sets of element faces (include/neklab_gpu.h, nlg_forces_*): drag and lift of the reference's
   !! cylinder cases, the Nusselt number of its temperature cases.  init: elem(:) global element ids, 1-BASED as Nek5000's lglel, face(:)
   !! in the preprocessor's numbering, obj(:) in 1..nobj, centres(ldim, nobj) optional.  sample: out(nq, nobj, size(vecs)) in the order
   !! Fp(ldim), Fv(ldim), Tp(nt), Tv(nt), Q; coefficients are the caller's division, Cd = 2 (Fp_x + Fv_x) / (rho U^2 L).
   type, public :: nek_wall_forces
      integer :: nobj = 0, nq = 0
      real(dp), allocatable :: area(:)
      type(c_ptr), private :: h = c_null_ptr
      integer(c_intptr_t), private :: owner = 0
   contains
      procedure, pass(self), public :: init => wf_init
      procedure, pass(self), public :: sample => wf_sample
      procedure, pass(self), public :: finalize => wf_close
      final :: finalize_wf
   end type

   !> A nonlinear run with history points and a recurrence monitor (include/neklab_gpu.h, nlg_dns_*): what the reference's case
   !! examples/cylinder/dns/Re180 does in its userchk with `call hpts()` and rnorm = |u(t) - u_ref|.  A plain type, not a LightKrylov
   !! object.  init(X0): the options of nek_case (dt > 0: that step; else the CFL rule at X0 with cfl_limit = 0.4), the step is then fixed.
   type, public :: nek_dns
      integer :: chunk = 256                                 ! ring length in steps
      type(c_ptr), private :: h = c_null_ptr, hop = c_null_ptr, hp = c_null_ptr
      integer(c_intptr_t), private :: owner = 0              ! the object that created the handles (a bitwise copy does not own them)
      integer, private :: npts = 0, nf = 0, nobj = 0, nq = 0
      real(dp), allocatable, private :: xyz(:, :)
   contains
      procedure, pass(self), public :: init => dns_init
      procedure, pass(self), public :: advance => dns_advance
      procedure, pass(self), public :: set_history_points => dns_set_history_points
      procedure, pass(self), public :: set_reference => dns_set_reference
      procedure, pass(self), public :: set_wall_forces => dns_set_wall_forces
      procedure, pass(self), public :: force_series => dns_force_series
      procedure, pass(self), public :: series => dns_series
      procedure, pass(self), public :: nsamples => dns_nsamples
      procedure, pass(self), public :: state => dns_state
      procedure, pass(self), public :: info => dns_info
      procedure, pass(self), public :: hpts => dns_hpts
      procedure, pass(self), public :: finalize => dns_close
      final :: finalize_dns
   end type

   !> the solver tolerance the schedulers last chose = what Nek5000 keeps in param(21) / param(22) (neklab_systems.f90:261-264)
   !> the reference's param(22) (Nek5000's velocity tolerance), which its schedulers, nonlinear_map and the Jacobian products read and
   !! write in turn (neklab_systems.f90:259-260, fixed_point.f90:14-17, :49-62, :87): ONE variable here too, so that the tolerance of
   !! a Jacobian product depends on who set it last exactly as it does there
   real(dp), save, private :: solver_tol = 1.0e-9_dp

contains

   subroutine make_propagator(prop, about, cfl_limit)
      type(exptA_linop), intent(inout) :: prop
      type(nek_dvector), intent(in) :: about
      real(dp), intent(in) :: cfl_limit
      prop%tau = nek_endtime
      prop%baseflow = about
      prop%cfg = nek_case
      prop%cfg%cfl_limit = cfl_limit
      prop%cfg_set = .true.
      call prop%init()
   end subroutine

   subroutine nonlinear_map(self, vec_in, vec_out, atol)
      class(nek_system), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      real(dp), intent(in) :: atol
      select type (vec_in)
      type is (nek_dvector)
         select type (vec_out)
         type is (nek_dvector)
            if (.not. self%ready) then
               allocate (self%prop)
               call make_propagator(self%prop, vec_in, 0.4_dp)
               self%ready = .true.
            end if
            call self%prop%set_tolerances(0.1_dp*atol, 0.1_dp*atol)
            solver_tol = 0.1_dp*atol      ! setup_nonlinear_solver(vtol = atol*0.1) leaves param(22) at this value (neklab_nek_setup.f90:228)
            call self%prop%nonlinear_map(vec_in, vec_out)      ! Phi_T(X) - X; the time step follows the CFL number of X
         class default
            call type_error('vec_out', 'nek_dvector', 'OUT', this_module, 'nonlinear_map')
         end select
      class default
         call type_error('vec_in', 'nek_dvector', 'IN', this_module, 'nonlinear_map')
      end select
   end subroutine nonlinear_map

   subroutine jac_apply(self, vec_in, vec_out, transposed)
      class(nek_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      logical, intent(in) :: transposed
      if (.not. allocated(self%X)) then
         write (*, '(A)') 'ERROR in '//this_module//': jacobian%X is not set (tsyphon.usr:40)'
         error stop 1
      end if
      select type (state => self%X)
      type is (nek_dvector)
         ! linearise about the current X on every application, as the reference does (abs_vec2nek(.., self%X) and
         ! setup_linear_solver(recompute_dt = .true.) inside jac_exptA_matvec, fixed_point.f90:52-59): X is updated in place by
         ! Newton, so there is no cheaper way to know that it is still the state of the last call
         if (.not. self%ready) then
            allocate (self%prop)
            call make_propagator(self%prop, state, 0.5_dp)
            self%ready = .true.
         else
            call self%prop%set_baseflow(state)
         end if
         ! fixed_point.f90:49-62: atol = param(22) AS IT STANDS at the call -- the value the scheduler wrote if it ran last, a tenth of it
         ! if nonlinear_map ran last -- the solves run at half of it, and param(22) is put back afterwards (:87)
         call self%prop%set_tolerances(0.5_dp*solver_tol, 0.5_dp*solver_tol)
         if (transposed) then
            call self%prop%rmatvec(vec_in, vec_out)
         else
            call self%prop%matvec(vec_in, vec_out)
         end if
         call vec_out%sub(vec_in)                       ! [exp(T J) - I] dx
      class default
         call type_error('self%X', 'nek_dvector', 'IN', this_module, 'jac_exptA_matvec')
      end select
   end subroutine

   subroutine jac_exptA_matvec(self, vec_in, vec_out)
      class(nek_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call jac_apply(self, vec_in, vec_out, .false.)
   end subroutine

   subroutine jac_exptA_rmatvec(self, vec_in, vec_out)
      class(nek_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      call jac_apply(self, vec_in, vec_out, .true.)
   end subroutine

   !---- periodic orbits ------------------------------------------------------------------------------------------------------
   !> the operator in orbit mode about (X, T): created on first use, afterwards nlg_linop_set_orbit_steps with the new state
   subroutine orbit_state(prop, ready, X)
      type(exptA_orbit_linop), allocatable, intent(inout) :: prop
      logical, intent(inout) :: ready
      type(nek_ext_dvector), intent(in) :: X
      if (.not. ready) then
         allocate (prop)
         prop%tau = X%T
         prop%baseflow = X%vec
         call prop%init()                              ! cfl_limit 0.4 (periodic_orbit.f90:18, :67), nlg_linop_set_orbit
         ready = .true.
         if (upo_fixed_nsteps <= 0) return              ! the count is left to the rule: set_orbit has set this state already
      end if
      prop%tau = X%T
      call nlg_check(c_linop_set_orbit_steps(prop%handle(), nek_dvector_handle(X%vec), X%T, int(upo_fixed_nsteps, c_int)), 'nek_upo: state')
   end subroutine

   subroutine nonlinear_map_upo(self, vec_in, vec_out, atol)
      class(nek_upo_system), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      real(dp), intent(in) :: atol
      select type (vec_in)
      type is (nek_ext_dvector)
         select type (vec_out)
         type is (nek_ext_dvector)
            call orbit_state(self%prop, self%ready, vec_in)
            call self%prop%set_tolerances(0.1_dp*atol, 0.1_dp*atol)
            call nek_dvector_ensure(vec_out%vec)
            call nlg_check(c_upo_residual(self%prop%handle(), vec_out%vec%h), 'nonlinear_map_upo')      ! Phi_T(X) - X
            vec_out%T = 0.0_dp
         class default
            call type_error('vec_out', 'nek_ext_dvector', 'OUT', this_module, 'nonlinear_map_upo')
         end select
      class default
         call type_error('vec_in', 'nek_ext_dvector', 'IN', this_module, 'nonlinear_map_upo')
      end select
   end subroutine

   !> handle of the Jacobian's operator, set about self%X at the scheduler's tolerance
   function upo_jacobian_handle(self) result(h)
      class(nek_upo_jacobian), intent(inout) :: self
      type(c_ptr) :: h
      if (.not. allocated(self%X)) then
         write (*, '(A)') 'ERROR in '//this_module//': jacobian%X is not set'
         error stop 1
      end if
      h = c_null_ptr
      select type (state => self%X)
      type is (nek_ext_dvector)
         call orbit_state(self%prop, self%ready, state)
         call self%prop%set_tolerances(0.1_dp*solver_tol, 0.1_dp*solver_tol)
         h = self%prop%handle()
      class default
         call type_error('self%X', 'nek_ext_dvector', 'IN', this_module, 'nek_upo_jacobian')
      end select
   end function

   subroutine jac_direct_map(self, vec_in, vec_out)
      class(nek_upo_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      type(c_ptr) :: h
      ! about the current X on every application, as the reference does (abs_ext_vec2nek(.., self%X), periodic_orbit.f90:60)
      h = upo_jacobian_handle(self)
      select type (vec_in)
      type is (nek_ext_dvector)
         select type (vec_out)
         type is (nek_ext_dvector)
            call nek_dvector_ensure(vec_out%vec)
            call nlg_check(c_upo_jac_matvec(h, nek_dvector_handle(vec_in%vec), vec_in%T, vec_out%vec%h, vec_out%T), 'jac_direct_map')
         class default
            call type_error('vec_out', 'nek_ext_dvector', 'OUT', this_module, 'jac_direct_map')
         end select
      class default
         call type_error('vec_in', 'nek_ext_dvector', 'IN', this_module, 'jac_direct_map')
      end select
   end subroutine

   !> the library's refusal, then stop (as exptA_orbit_linop%rmatvec)
   subroutine jac_adjoint_map(self, vec_in, vec_out)
      class(nek_upo_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      class(abstract_vector_rdp), intent(out) :: vec_out
      type(c_ptr) :: h
      h = upo_jacobian_handle(self)
      select type (vec_in)
      type is (nek_ext_dvector)
         select type (vec_out)
         type is (nek_ext_dvector)
            call self%prop%rmatvec(vec_in%vec, vec_out%vec)
         end select
      end select
      write (*, '(A)') 'ERROR in '//this_module//': nek_upo_jacobian has no adjoint (orbit mode)'
      error stop 1
   end subroutine

   subroutine jac_compute_rst(self, vec_out, nrst)
      class(nek_upo_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(inout) :: vec_out
      integer, intent(in) :: nrst
      select type (vec_out)
      type is (nek_ext_dvector)
         if (allocated(self%prop)) call self%prop%compute_rst(vec_out%vec, nrst)
      class default
         call type_error('vec_out', 'nek_ext_dvector', 'OUT', this_module, 'jac_compute_rst')
      end select
   end subroutine

   !> Replay of vec_in's history slot: with restart history on (no_history = 0 in the case) the device matvec performs it inside its
   !! time loop for the field part, as for exptA_linop; the period component of the slots (nek_ext_dvector%Trst) is carried by the
   !! vector algebra only, the Jacobian does not read it.  Under the drivers' default, no_history = 1, there is nothing to replay.
   subroutine jac_get_rst(self, vec_in, istep)
      class(nek_upo_jacobian), intent(inout) :: self
      class(abstract_vector_rdp), intent(in) :: vec_in
      integer, intent(in) :: istep
      select type (vec_in)
      type is (nek_ext_dvector)
      class default
         call type_error('vec_in', 'nek_ext_dvector', 'IN', this_module, 'jac_get_rst')
      end select
   end subroutine

   !> Restarted GMRES(kdim) for the bordered Jacobian J x = b on extended vectors, zero initial guess, stop at |r| <= atol: a linear
   !! solver with LightKrylov's interface (newton(sys, X, gmres_upo, ..)) whose Krylov loop runs on the device -- the basis in one
   !! allocation, nlg_upo_arnoldi_step (Jacobian matvec + CGS2 in the extended inner product) per step, Givens rotations on the host.
   !! No restart-history replay: every new Krylov vector is stripped of its history.  Krylov dimension upo_gmres_kdim, at most 10
   !! cycles.  info = Jacobian matvecs.
   subroutine gmres_upo(A, b, x, info, atol)
      class(abstract_linop_rdp), intent(inout) :: A
      class(abstract_vector_rdp), intent(in) :: b
      class(abstract_vector_rdp), intent(inout) :: x
      integer, intent(out) :: info
      real(dp), intent(in) :: atol
      integer, parameter :: nmax = 10
      type(c_ptr) :: h, basis, col
      type(nek_ext_dvector) :: r, dx, Jx
      real(dp), allocatable :: Hm(:, :), Rm(:, :), cs(:), sn(:), g(:), hk(:), y(:), tcol(:)
      real(dp) :: res, beta, t, d
      integer :: kd, k, i, j, cyc
      kd = upo_gmres_kdim
      info = 0
      select type (A)
      class is (nek_upo_jacobian)
         h = upo_jacobian_handle(A)
      class default
         call type_error('A', 'nek_upo_jacobian', 'IN', this_module, 'gmres_upo')
      end select
      select type (b)
      type is (nek_ext_dvector)
         r = b
      class default
         call type_error('b', 'nek_ext_dvector', 'IN', this_module, 'gmres_upo')
      end select
      call x%zero()
      call nlg_check(c_basis_create(nlg_mesh, 0_c_int, int(nek_lorder, c_int), int(kd + 1, c_int), basis), 'gmres_upo')
      allocate (Hm(kd + 2, kd + 1), Rm(kd + 1, kd), cs(kd), sn(kd), g(kd + 1), hk(kd + 2), y(kd), tcol(kd + 2))
      res = r%norm()
      do cyc = 1, nmax
         beta = res
         if (beta <= atol) exit
         tcol = 0.0_dp
         call nlg_check(c_basis_vec(basis, 0_c_int, col), 'gmres_upo')
         call nlg_check(c_vec_copy(col, nek_dvector_handle(r%vec)), 'gmres_upo')
         call nlg_check(c_vec_scal(col, 1.0_dp/beta), 'gmres_upo')
         tcol(1) = r%T/beta
         Hm = 0.0_dp; Rm = 0.0_dp; cs = 0.0_dp; sn = 0.0_dp; g = 0.0_dp
         g(1) = beta
         k = 0
         do while (k < kd)
            call nlg_check(c_upo_arnoldi_step(h, basis, tcol, int(k, c_int), Hm, int(kd + 2, c_int)), 'gmres_upo')
            info = info + 1
            call nlg_check(c_basis_vec(basis, int(k + 1, c_int), col), 'gmres_upo')
            call nlg_check(c_vec_clear_rst(col), 'gmres_upo')
            hk(1:k + 2) = Hm(1:k + 2, k + 1)
            do i = 1, k                                    ! previous rotations
               t = cs(i)*hk(i) + sn(i)*hk(i + 1)
               hk(i + 1) = -sn(i)*hk(i) + cs(i)*hk(i + 1)
               hk(i) = t
            end do
            d = sqrt(hk(k + 1)*hk(k + 1) + hk(k + 2)*hk(k + 2))
            if (d == 0.0_dp) then
               cs(k + 1) = 1.0_dp; sn(k + 1) = 0.0_dp
            else
               cs(k + 1) = hk(k + 1)/d; sn(k + 1) = hk(k + 2)/d
            end if
            hk(k + 1) = d; hk(k + 2) = 0.0_dp
            Rm(1:k + 1, k + 1) = hk(1:k + 1)
            g(k + 2) = -sn(k + 1)*g(k + 1)
            g(k + 1) = cs(k + 1)*g(k + 1)
            k = k + 1
            res = abs(g(k + 1))
            if (res <= atol) exit
         end do
         do i = k, 1, -1                                   ! R y = g, summed in the order of the Python driver
            t = g(i)
            do j = i + 1, k
               t = t - Rm(i, j)*y(j)
            end do
            y(i) = t/Rm(i, i)
         end do
         call nek_dvector_ensure(dx%vec)
         call nlg_check(c_basis_combine(basis, int(k, c_int), y, dx%vec%h), 'gmres_upo')
         dx%T = 0.0_dp
         do j = 1, k
            dx%T = dx%T + tcol(j)*y(j)
         end do
         call x%axpby(1.0_dp, dx, 1.0_dp)
         if (res <= atol) exit
         select type (x)                                   ! true residual for the restart
         type is (nek_ext_dvector)
            call nek_dvector_ensure(Jx%vec)
            call nlg_check(c_upo_jac_matvec(h, nek_dvector_handle(x%vec), x%T, Jx%vec%h, Jx%T), 'gmres_upo')
            info = info + 1
            call Jx%vec%clear_rst_fields()
         end select
         select type (b)
         type is (nek_ext_dvector)
            r = b
         end select
         call r%axpby(-1.0_dp, Jx, 1.0_dp)
         res = r%norm()
      end do
      call nlg_check(c_basis_destroy(basis), 'gmres_upo')
   end subroutine gmres_upo

   !> constant solver tolerance = the target, never below 10 atol_dp
   subroutine nek_constant_tol(tol, target_tol, rnorm, iter, info)
      real(dp), intent(out) :: tol
      real(dp), intent(in) :: target_tol, rnorm
      integer, intent(in) :: iter
      integer, intent(out) :: info
      tol = max(target_tol, 10.0_dp*atol_dp)
      solver_tol = tol
      info = 0
   end subroutine

   !> solver tolerance a tenth of the current residual, between the target and 1e-4; the target itself once within a factor 10
   subroutine nek_dynamic_tol(tol, target_tol, rnorm, iter, info)
      real(dp), intent(out) :: tol
      real(dp), intent(in) :: target_tol, rnorm
      integer, intent(in) :: iter
      integer, intent(out) :: info
      real(dp), parameter :: loosest = 1.0e-4_dp
      real(dp) :: goal
      goal = min(max(target_tol, 10.0_dp*atol_dp), loosest)
      tol = max(0.1_dp*rnorm, goal)
      if (tol < 10.0_dp*goal) tol = goal
      tol = min(tol, loosest)
      solver_tol = tol
      info = 0
   end subroutine

   !---- nek_wall_forces ----------------------------------------------------------------------------------------------
   subroutine wf_close(self)
      class(nek_wall_forces), intent(inout) :: self
      if (self%owner == loc(self) .and. c_associated(self%h)) then
         call nlg_check(c_forces_destroy(self%h), 'nek_wall_forces finalize')      ! refused while a nek_dns samples the faces
      end if
      self%h = c_null_ptr; self%owner = 0; self%nobj = 0
   end subroutine

   subroutine finalize_wf(self)
      type(nek_wall_forces), intent(inout) :: self
      integer(c_int) :: rc
      if (self%owner == loc(self) .and. c_associated(self%h)) rc = c_forces_destroy(self%h)
      self%h = c_null_ptr; self%owner = 0
   end subroutine

   subroutine wf_init(self, elem, face, obj, nobj, centres)
      class(nek_wall_forces), intent(inout) :: self
      integer, intent(in) :: elem(:), face(:), obj(:), nobj
      real(dp), target, intent(in), optional :: centres(:, :)
      integer(c_int64_t), allocatable :: e0(:)
      integer(c_int), allocatable :: f(:), o0(:)
      integer(c_int64_t) :: nl
      type(c_ptr) :: c
      call wf_close(self)
      if (size(face) /= size(elem) .or. size(obj) /= size(elem)) then
         write (*, '(A)') 'ERROR in '//this_module//': nek_wall_forces init: elem, face and obj differ in length'
         error stop 1
      end if
      e0 = int(elem, c_int64_t) - 1_c_int64_t
      f = int(face, c_int)
      o0 = int(obj, c_int) - 1_c_int
      c = c_null_ptr
      if (present(centres)) then
         if (size(centres, 1) /= nek_ldim .or. size(centres, 2) /= nobj) then
            write (*, '(A)') 'ERROR in '//this_module//': nek_wall_forces init: centres must be (ldim, nobj)'
            error stop 1
         end if
         c = c_loc(centres)
      end if
      call nlg_check(c_forces_create(nlg_mesh, int(nobj, c_int), int(size(elem), c_int64_t), e0, f, o0, c, self%h), 'nek_wall_forces init')
      self%owner = loc(self)
      self%nobj = nobj
      self%nq = 2*nek_ldim + 2*merge(3, 1, nek_ldim == 3) + 1
      if (allocated(self%area)) deallocate (self%area)
      allocate (self%area(nobj))
      call nlg_check(c_forces_info(self%h, self%area, nl), 'nek_wall_forces init')
   end subroutine

   !> out(nq, nobj, size(vecs)) for 1 to 4 vectors in one call: global sums
   subroutine wf_sample(self, vecs, nu, out)
      class(nek_wall_forces), intent(in) :: self
      type(nek_dvector), intent(in) :: vecs(:)
      real(dp), intent(in) :: nu
      real(dp), allocatable, intent(out) :: out(:, :, :)
      type(c_ptr), target :: hs(max(size(vecs), 1))
      integer :: v
      if (.not. c_associated(self%h) .or. self%owner /= loc(self)) then
         write (*, '(A)') 'ERROR in '//this_module//': nek_wall_forces%init() has not been called on this object'
         error stop 1
      end if
      do v = 1, size(vecs)
         hs(v) = nek_dvector_handle(vecs(v))
      end do
      allocate (out(self%nq, self%nobj, size(vecs)))
      call nlg_check(c_forces_sample(self%h, int(size(vecs), c_int), c_loc(hs), nu, out), 'nek_wall_forces sample')
   end subroutine

   !---- nek_dns ------------------------------------------------------------------------------------------------------
   function dns_handle(self) result(h)
      class(nek_dns), intent(in) :: self
      type(c_ptr) :: h
      if (.not. c_associated(self%h) .or. self%owner /= loc(self)) then
         write (*, '(A)') 'ERROR in '//this_module//': DNS%init() has not been called on this object'
         error stop 1
      end if
      h = self%h
   end function

   subroutine dns_close(self)
      class(nek_dns), intent(inout) :: self
      integer(c_int) :: rc
      if (self%owner == loc(self)) then
         if (c_associated(self%h)) rc = c_dns_destroy(self%h)
         if (c_associated(self%hp)) rc = c_probes_destroy(self%hp)
         if (c_associated(self%hop)) rc = c_linop_destroy(self%hop)
      end if
      self%h = c_null_ptr; self%hop = c_null_ptr; self%hp = c_null_ptr; self%owner = 0; self%npts = 0; self%nobj = 0; self%nq = 0
   end subroutine

   subroutine finalize_dns(self)
      type(nek_dns), intent(inout) :: self
      call dns_close(self)
   end subroutine

   subroutine dns_init(self, X0)
      class(nek_dns), intent(inout) :: self
      type(nek_dvector), intent(in) :: X0
      type(nlg_exptA_config) :: cfg
      type(nlg_dns_opts) :: o
      call dns_close(self)
      cfg = nek_case
      cfg%cfl_limit = 0.4_dp
      if (cfg%dt > 0.0_dp) cfg%tau = cfg%dt       ! a run has no tau: the step is the given one, not tau / ceil(tau / dt)
      call nlg_check(c_linop_create(nlg_mesh, cfg, nek_dvector_handle(X0), self%hop), 'nek_dns init')
      self%owner = loc(self)
      o%chunk = int(self%chunk, c_int)
      call nlg_check(c_dns_create(self%hop, nek_dvector_handle(X0), o, self%h), 'nek_dns init')
      self%nf = nek_ldim + 1 + merge(1, 0, cfg%ifheat /= 0)
   end subroutine

   subroutine dns_advance(self, nsteps)
      class(nek_dns), intent(inout) :: self
      integer, intent(in) :: nsteps
      call nlg_check(c_dns_advance(dns_handle(self), int(nsteps, c_int)), 'nek_dns advance')
   end subroutine

   !> xyz(ldim, npts); tol_r (default 1e-10) as in nlg_probe_locate.  The series starts again from the state as it stands.
   subroutine dns_set_history_points(self, xyz, tol_r)
      class(nek_dns), intent(inout) :: self
      real(dp), intent(in) :: xyz(:, :)
      real(dp), intent(in), optional :: tol_r
      real(dp) :: tol
      type(c_ptr) :: hnew
      integer(c_int) :: rc
      tol = 1.0e-10_dp
      if (present(tol_r)) tol = tol_r
      if (size(xyz, 1) /= nek_ldim) then
         write (*, '(A)') 'ERROR in '//this_module//': set_history_points: xyz must be (ldim, npts)'
         error stop 1
      end if
      call nlg_check(c_probes_create(nlg_mesh, int(size(xyz, 2), c_int64_t), xyz, tol, hnew), 'nek_dns set_history_points')
      call nlg_check(c_dns_set_probes(dns_handle(self), hnew), 'nek_dns set_history_points')
      if (c_associated(self%hp)) rc = c_probes_destroy(self%hp)
      self%hp = hnew
      self%npts = size(xyz, 2)
      self%xyz = xyz
   end subroutine

   !> u_ref of the recurrence norm: vec, or the state as it stands.  The series starts again from the state as it stands.
   subroutine dns_set_reference(self, vec)
      class(nek_dns), intent(inout) :: self
      type(nek_dvector), intent(in), optional :: vec
      if (present(vec)) then
         call nlg_check(c_dns_set_reference(dns_handle(self), nek_dvector_handle(vec)), 'nek_dns set_reference')
      else
         call nlg_check(c_dns_set_reference(dns_handle(self), c_null_ptr), 'nek_dns set_reference')
      end if
   end subroutine

   !> every sample also holds wf%sample(state, 1 / Re); without wf: detach.  The series starts again from the state as it stands.
   !! wf must outlive its use: its finalize is refused while it is attached.
   subroutine dns_set_wall_forces(self, wf)
      class(nek_dns), intent(inout) :: self
      type(nek_wall_forces), intent(in), optional :: wf
      if (present(wf)) then
         call nlg_check(c_dns_set_forces(dns_handle(self), wf%h), 'nek_dns set_wall_forces')
         self%nobj = wf%nobj; self%nq = wf%nq
      else
         call nlg_check(c_dns_set_forces(dns_handle(self), c_null_ptr), 'nek_dns set_wall_forces')
         self%nobj = 0; self%nq = 0
      end if
   end subroutine

   !> force(nq, nobj, nsamples) of the attached wall forces: (re)allocated
   subroutine dns_force_series(self, force)
      class(nek_dns), intent(inout) :: self
      real(dp), allocatable, intent(out) :: force(:, :, :)
      integer :: n
      n = dns_nsamples(self)
      allocate (force(self%nq, self%nobj, n))
      call nlg_check(c_dns_force_series(dns_handle(self), 0_c_int64_t, int(n, c_int64_t), force), 'nek_dns force_series')
   end subroutine

   function dns_nsamples(self) result(n)
      class(nek_dns), intent(inout) :: self
      integer :: n
      integer(c_int64_t) :: cnt
      call nlg_check(c_dns_advance(dns_handle(self), 0_c_int), 'nek_dns nsamples')      ! sample 0, if nothing has been taken yet
      call nlg_check(c_dns_count(dns_handle(self), cnt), 'nek_dns nsamples')
      n = int(cnt)
   end function

   !> time(nsamples), probe(nf, npts, nsamples), dist(nsamples): (re)allocated; sample 1 is the state the series started from
   subroutine dns_series(self, time, probe, dist)
      class(nek_dns), intent(inout) :: self
      real(dp), allocatable, intent(out) :: time(:), probe(:, :, :), dist(:)
      integer :: n
      n = dns_nsamples(self)
      allocate (time(n), dist(n), probe(self%nf, max(self%npts, 1), n))
      probe = 0.0_dp
      call nlg_check(c_dns_series(dns_handle(self), 0_c_int64_t, int(n, c_int64_t), time, probe, dist), 'nek_dns series')
      if (self%npts == 0) then
         deallocate (probe); allocate (probe(self%nf, 0, n))
      end if
   end subroutine

   subroutine dns_state(self, vec_out)
      class(nek_dns), intent(in) :: self
      type(nek_dvector), intent(inout) :: vec_out
      call nek_dvector_ensure(vec_out)
      call nlg_check(c_dns_get_state(dns_handle(self), vec_out%h), 'nek_dns state')
   end subroutine

   subroutine dns_info(self, istep, time, dt)
      class(nek_dns), intent(in) :: self
      integer, intent(out) :: istep
      real(dp), intent(out) :: time, dt
      integer(c_int64_t) :: is
      call nlg_check(c_dns_info(dns_handle(self), is, time, dt), 'nek_dns info')
      istep = int(is)
   end subroutine

   !> the series as text: the number of points and their coordinates, then per sample and point one line `time, fields...` in
   !! 1pE15.7 (Nek5000's hpts layout restated from memory, unverified; the layout of nekio.write_his)
   subroutine dns_hpts(self, filename)
      class(nek_dns), intent(inout) :: self
      character(len=*), intent(in) :: filename
      real(dp), allocatable :: time(:), probe(:, :, :), dist(:)
      integer :: u, k, q
      call dns_series(self, time, probe, dist)
      open (newunit=u, file=filename, status='replace', action='write')
      write (u, '(I0)') self%npts
      do q = 1, self%npts
         write (u, '(1p,3E15.7)') self%xyz(:, q)
      end do
      do k = 1, size(time)
         do q = 1, self%npts
            write (u, '(1p,6E15.7)') time(k), probe(:, q, k)
         end do
      end do
      close (u)
   end subroutine

end module neklab_systems
