!> Wall forces through the shim's nek_wall_forces and nek_dns%set_wall_forces (neklab_amd/fortran/neklab_systems.f90): the calls of the
!! Python driver host.wall_forces in the same order.  Nek5000 is replaced by `case.bin` (written by tests/test_gpu_forces_fortran.py);
!! the sample of the initial state, the areas and the force series go to `forces.bin`.
program forces_driver
   use iso_c_binding, only: c_int64_t
   use neklab
   implicit none
   integer :: ldim, lx1, nelv, lvn, lpn, nsteps, nfaces, nobj, u
   integer(c_int64_t), allocatable :: glo(:)
   integer, allocatable :: elem(:), face(:), obj(:)
   real(dp), allocatable :: xm1(:), ym1(:), zm1(:), v1mask(:), v2mask(:), v3mask(:), vx(:), vy(:), vz(:), pr(:), t(:), centres(:, :)
   real(dp), allocatable :: out(:, :, :), force(:, :, :)
   real(dp) :: re, dt, vtol, ptol, nu
   type(nek_dvector) :: X0
   type(nek_dns) :: dns
   type(nek_wall_forces) :: wf

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='old')
   read (u) ldim, lx1, nelv, nsteps, nfaces, nobj
   read (u) re, dt, vtol, ptol, nu
   lvn = nelv*lx1**ldim
   lpn = nelv*(lx1 - 2)**ldim
   allocate (xm1(lvn), ym1(lvn), zm1(lvn), v1mask(lvn), v2mask(lvn), v3mask(lvn), vx(lvn), vy(lvn), vz(lvn), glo(lvn), pr(lpn), t(lvn))
   allocate (elem(nfaces), face(nfaces), obj(nfaces), centres(ldim, nobj))
   zm1 = 0; v3mask = 0; vz = 0; t = 0
   read (u) xm1, ym1
   read (u) glo
   read (u) v1mask, v2mask
   read (u) vx, vy, pr
   read (u) elem, face, obj
   read (u) centres
   close (u)

   call neklab_gpu_init(0)
   call neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo, v1mask, v2mask, v3mask, .false.)
   call neklab_gpu_set_case(re=re, torder=3, vtol=vtol, ptol=ptol, maxit_v=400, maxit_p=4000, dt=dt, pprecond=1, pproj=0)
   call nek2vec(X0, vx, vy, vz, pr, t)

   call wf%init(elem, face, obj, nobj, centres)
   call wf%sample([X0], nu, out)
   call dns%init(X0)
   call dns%set_wall_forces(wf)
   call dns%advance(nsteps)
   call dns%force_series(force)
   write (*, '(A,3I6)') 'SHAPE ', size(force, 3), size(force, 2), size(force, 1)
   open (newunit=u, file='forces.bin', access='stream', form='unformatted', status='replace')
   write (u) wf%area, out, force
   close (u)
   call dns%finalize()
   call wf%finalize()
   call neklab_gpu_finalize()
end program forces_driver
