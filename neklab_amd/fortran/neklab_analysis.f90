!> Analysis drivers over the device hot path: the two entry points of the reference's module of the same name that consume it,
!!   linear_stability_analysis_fixed_point   (/root/reference/src/neklab_analysis.f90:38-105)
!!   transient_growth_analysis_fixed_point   (/root/reference/src/neklab_analysis.f90:107-156)
!! plus newton_fixed_point_iteration (:158-212) for the base-flow step upstream of them.  Same names, dummy arguments and
!! files written (`dir|adj_eigenspectrum.npy`, `singular_spectrum.dat`, the `dir` / `adj` / `prt` / `rsp` / `nwt` field files),
!! so a case file that calls them needs no edit.  With `device_eigs = .true.` the Krylov loop itself runs on the device
!! (nek_eigs / nek_svds -> nlg_eigs / nlg_svds: basis in one allocation, one fused projection kernel and one all-reduce per
!! Gram-Schmidt pass); with `.false.` LightKrylov's own eigs / svds drive the vectors and the operator through their
!! type-bound procedures.  Logger and timer plumbing of the reference is LightKrylov's and is not repeated here.
!! (In a build against the real LightKrylov the reference's own file works unchanged on top of neklab_vectors / neklab_linops;
!!  this module exists for the device switch.)
module neklab_analysis
   use LightKrylov, only: dp, eigs, svds, save_eigenspectrum, zero_basis, initialize_krylov_subspace, newton, gmres_rdp, &
                          newton_dp_opts, newton_dp_metadata
   use LightKrylov, only: abstract_vector_rdp, abstract_exptA_linop_rdp, abstract_system_rdp
   use iso_c_binding, only: c_int, c_ptr, c_null_ptr, c_loc, c_double
   use neklab_gpu_capi, only: nlg_check, c_vec_get_field, c_vec_set_field, nek_lpn, nlg_mesh, c_sens_apply, c_sens_pairing
   use neklab_vectors
   use neklab_linops
   use neklab_utils
   use neklab_systems, only: nek_constant_tol, nek_dynamic_tol
   implicit none
   private

   public :: linear_stability_analysis_fixed_point, transient_growth_analysis_fixed_point, newton_fixed_point_iteration
   public :: otd_analysis, eigenvalue_sensitivity
   !> .true.: Arnoldi / Lanczos on the device; .false.: LightKrylov's loops over the type-bound procedures
   logical, save, public :: device_eigs = .false.

contains

   !> Leading eigenpairs of exp(tau L) (adjoint: of its transpose) -> growth rates and frequencies log(mu) / tau.
   subroutine linear_stability_analysis_fixed_point(exptA, kdim, nev, adjoint, X0)
      class(abstract_exptA_linop_rdp), intent(inout) :: exptA
      integer, intent(in) :: kdim, nev
      logical, intent(in), optional :: adjoint
      type(nek_dvector), optional, intent(in) :: X0
      type(nek_dvector), allocatable :: modes(:)
      complex(dp), allocatable :: spectrum(:)
      real(dp), allocatable :: res(:)
      character(len=3) :: tag
      integer :: nmatvec
      logical :: transposed, on_device

      transposed = .false.
      if (present(adjoint)) transposed = adjoint
      tag = 'dir'
      if (transposed) tag = 'adj'

      allocate (modes(nev))
      call zero_basis(modes)

      on_device = .false.
      if (device_eigs) then
         select type (exptA)
         class is (exptA_linop)
            on_device = .true.
            call nek_eigs(exptA, modes, spectrum, res, nmatvec, x0=X0, kdim=kdim, transpose=transposed, write_intermediate=.true.)
         end select
      end if
      if (.not. on_device) then
         call eigs(exptA, modes, spectrum, res, nmatvec, x0=X0, kdim=kdim, transpose=transposed, write_intermediate=.true.)
      end if

      spectrum = log(spectrum)/exptA%tau                       ! multipliers of the propagator -> continuous-time eigenvalues
      call save_eigenspectrum(spectrum, res, tag//'_eigenspectrum.npy')
      call outpost_dnek(modes(:nev), tag)
      call exptA%finalize_timer()
   end subroutine linear_stability_analysis_fixed_point

   !> Largest singular triplets of exp(tau L): optimal perturbations (V, prefix prt), optimal responses (U, prefix rsp).
   subroutine transient_growth_analysis_fixed_point(exptA, nsv, kdim)
      class(abstract_exptA_linop_rdp), intent(inout) :: exptA
      integer, intent(in) :: nsv, kdim
      type(nek_dvector), allocatable :: resp(:), pert(:)
      real(dp), allocatable :: sigma(:), res(:)
      integer :: nmatvec, u
      logical :: on_device

      allocate (resp(nsv), pert(nsv))
      call initialize_krylov_subspace(resp)
      call initialize_krylov_subspace(pert)

      on_device = .false.
      if (device_eigs) then
         select type (exptA)
         class is (exptA_linop)
            on_device = .true.
            call nek_svds(exptA, resp, sigma, pert, res, nmatvec, kdim=kdim, write_intermediate=.true.)
         end select
      end if
      if (.not. on_device) call svds(exptA, resp, sigma, pert, res, nmatvec, kdim=kdim, write_intermediate=.true.)

      open (newunit=u, file='singular_spectrum.dat', status='replace', action='write')
      write (u, *) sigma
      close (u)
      call outpost_dnek(pert(:nsv), 'prt')
      call outpost_dnek(resp(:nsv), 'rsp')
      call exptA%finalize_timer()
   end subroutine transient_growth_analysis_fixed_point

   !> Newton-Krylov iteration for a fixed point of sys, at most 40 iterations, no bisection; tol_mode 1: constant solver
   !! tolerance, otherwise tied to the residual (the two schedulers of neklab_systems).  The converged state is written with the
   !! prefix nwt.
   subroutine newton_fixed_point_iteration(sys, bf, tol, tol_mode, input_is_fixed_point)
      class(abstract_system_rdp), intent(inout) :: sys
      class(abstract_vector_rdp), intent(inout) :: bf
      real(dp), intent(inout) :: tol
      integer, optional, intent(in) :: tol_mode
      logical, optional, intent(out) :: input_is_fixed_point
      integer :: info, mode
      type(newton_dp_opts) :: opts
      type(newton_dp_metadata) :: meta
      mode = 1
      if (present(tol_mode)) mode = tol_mode
      opts = newton_dp_opts(maxiter=40, ifbisect=.false.)      ! LightKrylov's own interface, as the reference calls it (neklab_analysis.f90:186-196)
      if (mode == 1) then
         call newton(sys, bf, gmres_rdp, info, atol=tol, options=opts, scheduler=nek_constant_tol, meta=meta)
      else
         call newton(sys, bf, gmres_rdp, info, atol=tol, options=opts, scheduler=nek_dynamic_tol, meta=meta)
      end if
      if (.not. meta%converged) write (*, '(A)') 'WARNING in newton_fixed_point_iteration: not converged after 40 iterations'
      select type (bf)
      type is (nek_dvector)
         call outpost_dnek(bf, 'nwt')
      end select
      if (present(input_is_fixed_point)) input_is_fixed_point = meta%input_is_fixed_point
      call sys%finalize_timer()
      call sys%jacobian%finalize_timer()
   end subroutine newton_fixed_point_iteration

   !> Structural sensitivity and base-flow gradient of an eigenvalue from its direct mode u^ = dir_re + i dir_im and its adjoint mode
   !! u^+ = adj_re + i adj_im (a real eigenpair: no imaginary parts), on the device (nlg_sens_pairing, nlg_sens_apply; the definitions
   !! stand in include/neklab_gpu.h):  d = <u^+, u^>,  grad_re + i grad_im = grad_U lambda = [S(u_r, a_r) + S(u_i, a_i) + i (S(u_i, a_r)
   !! - S(u_r, a_i))] / d  with  S(u, a)_j = - sum_i a_i d_j u_i + sum_i u_i d_i a_j  of the masked fields (element-local; the term
   !! (div u) a_j is left out on purpose),  transp_re + i transp_im the same of the first sum alone,  wavemaker: |u^| |u^+| / |d| in its
   !! first velocity component.  The first-order shift of the eigenvalue under a base-flow change dU is
   !! cmplx(grad_re%dot(dU), grad_im%dot(dU)).
   subroutine eigenvalue_sensitivity(dir_re, adj_re, d, grad_re, grad_im, dir_im, adj_im, wavemaker, transp_re, transp_im)
      type(nek_dvector), intent(in) :: dir_re, adj_re
      complex(dp), intent(out) :: d
      type(nek_dvector), intent(inout) :: grad_re, grad_im
      type(nek_dvector), optional, intent(in) :: dir_im, adj_im
      type(nek_dvector), optional, intent(inout) :: wavemaker, transp_re, transp_im
      type(c_ptr), target :: h(9)
      type(c_ptr) :: a(9)
      real(c_double), target :: fac(2)
      real(c_double) :: dd(2)
      complex(dp) :: inv
      integer :: i

      if (present(dir_im) .neqv. present(adj_im)) then
         write (*, '(A)') 'ERROR in eigenvalue_sensitivity: dir_im and adj_im come together or not at all'
         error stop 1
      end if
      h = c_null_ptr
      h(1) = nek_dvector_handle(dir_re)
      h(3) = nek_dvector_handle(adj_re)
      if (present(dir_im)) then
         h(2) = nek_dvector_handle(dir_im)
         h(4) = nek_dvector_handle(adj_im)
      end if
      call nlg_check(c_sens_pairing(h(1), h(2), h(3), h(4), dd), 'eigenvalue_sensitivity')
      d = cmplx(dd(1), dd(2), kind=dp)
      if (abs(d) == 0.0_dp) then
         write (*, '(A)') 'ERROR in eigenvalue_sensitivity: <adjoint, direct> vanishes: the pair cannot be normalised'
         error stop 1
      end if
      inv = 1.0_dp/d
      fac = [real(inv, dp), aimag(inv)]
      call nek_dvector_ensure(grad_re); h(5) = grad_re%h
      call nek_dvector_ensure(grad_im); h(6) = grad_im%h
      if (present(transp_re)) then
         call nek_dvector_ensure(transp_re); h(7) = transp_re%h
      end if
      if (present(transp_im)) then
         call nek_dvector_ensure(transp_im); h(8) = transp_im%h
      end if
      if (present(wavemaker)) then
         call nek_dvector_ensure(wavemaker); h(9) = wavemaker%h
      end if
      ! one pair: every array of the call has one entry, h(i) itself
      do i = 1, 9
         a(i) = c_loc(h(i))
      end do
      call nlg_check(c_sens_apply(nlg_mesh, 1_c_int, a(1), a(2), a(3), a(4), c_loc(fac), a(5), a(6), a(7), a(8), a(9)), 'eigenvalue_sensitivity')
   end subroutine eigenvalue_sensitivity

   !> otd_analysis (src/neklab_analysis.f90:214-344): nsteps device time steps of the OTD modes in chunks that end at the next print /
   !! io / restart step; there the basis is orthonormalised and Lr read out, Ls.dat / Lr.dat are appended in the reference's formats,
   !! the projected modes (prefixes m01, m02, ..) and the basis (rst) written.
   subroutine otd_analysis(OTD, nsteps, opts_)
      type(nek_otd), intent(inout) :: OTD
      integer, intent(in) :: nsteps
      type(otd_opts), optional, intent(in) :: opts_
      type(otd_opts) :: opts
      real(dp), allocatable :: Lr(:, :), sigma(:), svec(:, :), pr(:)
      complex(dp), allocatable :: lambda(:), eigvec(:, :)
      type(nek_dvector) :: mode
      character(len=3) :: prefix
      real(dp) :: time, dt
      integer :: r, istep, nxt, i, j, is, u
      logical :: hp, hi, hr

      opts = otd_opts()
      if (present(opts_)) opts = opts_
      call OTD%init(opts)
      r = OTD%r
      allocate (Lr(r, r), sigma(r), svec(r, r), lambda(r), eigvec(r, r), pr(nek_lpn))
      open (newunit=u, file='Ls.dat', status='replace', action='write'); close (u)
      open (newunit=u, file='Lr.dat', status='replace', action='write'); close (u)
      istep = 0
      do while (istep < nsteps)
         nxt = nsteps
         if (opts%printstep > 0) nxt = min(nxt, (istep/opts%printstep + 1)*opts%printstep)
         if (opts%iostep > 0) nxt = min(nxt, (istep/opts%iostep + 1)*opts%iostep)
         if (opts%iorststep > 0) nxt = min(nxt, (istep/opts%iorststep + 1)*opts%iorststep)
         call OTD%advance(nxt - istep)
         istep = nxt
         if (istep < opts%startstep) cycle
         hp = .false.; hi = .false.; hr = .false.
         if (opts%printstep > 0) hp = mod(istep, opts%printstep) == 0
         if (opts%iostep > 0) hi = mod(istep, opts%iostep) == 0
         if (opts%iorststep > 0) hr = mod(istep, opts%iorststep) == 0
         if (.not. (hp .or. hi .or. hr)) cycle
         call OTD%info(is, time, dt)
         if (hp .or. hi) then
            call OTD%reduced(Lr)
            call OTD%spectral_analysis(Lr, sigma, svec, lambda, eigvec)
         end if
         if (hp) then
            open (newunit=u, file='Ls.dat', status='old', action='write', position='append')
            write (u, '(I8,1X,F15.8,A,*(1X,E15.8))') istep, time, ' Ls ', sigma
            close (u)
            open (newunit=u, file='Lr.dat', status='old', action='write', position='append')
            write (u, '(I8,1X,F15.8,A,*(1X,E15.8))', advance='no') istep, time, ' Lr%Re ', real(lambda)
            write (u, '(A,*(1X,E15.8))') ' Lr%Im ', aimag(lambda)
            close (u)
         end if
         if (hi .or. hr) call OTD%get_basis()
         if (hi) then                            ! outpost_OTDmodes: mode i = sum_j u_j Re(eigvec_ji), pressure of basis vector i
            do i = 1, r
               mode = OTD%basis(i)
               call mode%scal(real(eigvec(i, i)))
               do j = 1, r
                  if (j /= i) call mode%axpby(real(eigvec(j, i)), OTD%basis(j), 1.0_dp)
               end do
               call nlg_check(c_vec_get_field(nek_dvector_handle(OTD%basis(i)), 3_c_int, 0_c_int, pr, nek_lpn), 'otd_analysis pr')
               call nlg_check(c_vec_set_field(mode%h, 3_c_int, 0_c_int, pr, nek_lpn), 'otd_analysis pr')
               write (prefix, '(A,I2.2)') 'm', i
               call outpost_dnek(mode, prefix)
            end do
         end if
         if (hr) call outpost_dnek(OTD%basis, 'rst')
      end do
   end subroutine otd_analysis

end module neklab_analysis
