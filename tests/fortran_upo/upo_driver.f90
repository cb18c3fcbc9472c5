!> Newton-Krylov for a periodic orbit through the shim, with the reference's names (nek_ext_dvector, nek_system_upo / nek_jacobian_upo,
!! examples/cylinder/newton/Re180_periodic_orbit/1cyl.usr): the loop of the Python driver newton_periodic_orbit, written on
!! class(abstract_vector_rdp) and the type-bound procedures -- response, the scheduler, the linear solver gmres_upo -- on the
!! manufactured root of tests/test_gpu_upo.py.  Nek5000 is replaced by `case.bin` (written by tests/test_gpu_upo_fortran.py).
program upo_driver
   use iso_c_binding, only: c_int64_t
   use LightKrylov, only: abstract_vector_rdp, abstract_system_rdp
   use neklab
   implicit none
   integer :: ldim, lx1, nelv, lvn, lpn, nsteps, kdim, maxiter, u
   integer(c_int64_t), allocatable :: glo(:)
   real(dp), allocatable :: xm1(:), ym1(:), zm1(:), v1mask(:), v2mask(:), v3mask(:), vx(:), vy(:), vz(:), pr(:), t(:)
   real(dp) :: re, dt, vtol, ptol, tol, Tstar, Tstart, offtol
   type(nek_system_upo), allocatable :: sys
   type(nek_ext_dvector) :: Xs, X, off
   character(len=3) :: prefix

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='old')
   read (u) ldim, lx1, nelv, nsteps, kdim, maxiter
   read (u) re, dt, vtol, ptol, tol, Tstar, Tstart, offtol
   lvn = nelv*lx1**ldim
   lpn = nelv*(lx1 - 2)**ldim
   allocate (xm1(lvn), ym1(lvn), zm1(lvn), v1mask(lvn), v2mask(lvn), v3mask(lvn), vx(lvn), vy(lvn), vz(lvn), glo(lvn), pr(lpn), t(lvn))
   zm1 = 0; v3mask = 0; vz = 0; t = 0
   read (u) xm1, ym1
   read (u) glo
   read (u) v1mask, v2mask

   call neklab_gpu_init(0)
   call neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo, v1mask, v2mask, v3mask, .false.)
   call neklab_gpu_set_case(re=re, torder=3, vtol=vtol, ptol=ptol, maxit_v=400, maxit_p=4000, dt=dt, pprecond=1, pproj=0)
   nek_case%no_history = 1
   upo_fixed_nsteps = nsteps
   upo_gmres_kdim = kdim

   read (u) vx, vy, pr                      ! X*
   call nek2ext_vec(Xs, vx, vy, vz, pr, t); Xs%T = Tstar
   read (u) vx, vy, pr                      ! the start: X* + 1e-3 v
   call nek2ext_vec(X, vx, vy, vz, pr, t); X%T = Tstart
   close (u)

   sys = nek_system_upo()
   sys%jacobian = nek_jacobian_upo()

   call sys%response(Xs, off, offtol)                ! the offset F(X*, T*), solves at 0.1 offtol
   write (*, '(A,ES24.16)') 'OFFNORM ', off%norm()
   call newton_on(sys, X, off)

   write (*, '(A,ES24.16)') 'PERIOD ', get_period(X)
   prefix = 'upo'
   call outpost_ext_dnek(X, prefix)
   call ext_vec2nek(vx, vy, vz, pr, t, X)
   write (*, '(A,2ES24.16)') 'XMAX ', maxval(abs(vx)), maxval(abs(vy))
   deallocate (sys)
   call neklab_gpu_finalize()

contains

   !> newton_periodic_orbit (neklab_amd/host.py) with tol_mode = 1: scheduler first, residual minus offset, GMRES to the scheduler's
   !! tolerance, update; a residual below the target counts when computed at the final solver tolerance
   subroutine newton_on(sys, X, offset)
      class(abstract_system_rdp), intent(inout) :: sys
      class(abstract_vector_rdp), intent(inout) :: X
      class(abstract_vector_rdp), intent(in) :: offset
      class(abstract_vector_rdp), allocatable :: r, dx
      real(dp) :: cur, final, rnorm, gtol
      integer :: it, info, nmv, nmv_total
      allocate (r, mold=X); allocate (dx, mold=X)
      call nek_constant_tol(final, tol, 0.0_dp, 0, info)
      rnorm = 1.0_dp; nmv_total = 0
      do it = 0, maxiter
         call nek_constant_tol(cur, tol, rnorm, it, info)
         call sys%response(X, r, cur)
         call r%axpby(-1.0_dp, offset, 1.0_dp)
         rnorm = r%norm()
         select type (X)
         type is (nek_ext_dvector)
            write (*, '(A,I3,2ES24.16)') 'NEWTON ', it, rnorm, X%T
         end select
         if (rnorm < tol .and. cur <= final) then
            write (*, '(A,I0)') 'CONVERGED ', it
            exit
         end if
         if (it == maxiter) exit
         if (allocated(sys%jacobian%X)) deallocate (sys%jacobian%X)
         allocate (sys%jacobian%X, source=X)
         call r%scal(-1.0_dp)
         call nek_constant_tol(gtol, tol, rnorm, it, info)
         call gmres_upo(sys%jacobian, r, dx, nmv, gtol)
         nmv_total = nmv_total + nmv
         call X%add(dx)
      end do
      write (*, '(A,I0)') 'MATVECS ', nmv_total
   end subroutine

end program upo_driver
