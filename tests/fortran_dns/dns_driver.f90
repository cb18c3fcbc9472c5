!> A DNS run with history points and a recurrence monitor through the shim's nek_dns (neklab_amd/fortran/neklab_systems.f90): the calls
!! of the Python driver host.nek_dns in the same order.  Nek5000 is replaced by `case.bin` (written by tests/test_gpu_dns_fortran.py);
!! the series goes to `series.bin` and, as text, to `run.his`.
program dns_driver
   use iso_c_binding, only: c_int64_t
   use neklab
   implicit none
   integer :: ldim, lx1, nelv, lvn, lpn, nsteps, npts, u, n, istep
   integer(c_int64_t), allocatable :: glo(:)
   real(dp), allocatable :: xm1(:), ym1(:), zm1(:), v1mask(:), v2mask(:), v3mask(:), vx(:), vy(:), vz(:), pr(:), t(:), xyz(:, :)
   real(dp), allocatable :: time(:), probe(:, :, :), dist(:)
   real(dp) :: re, dt, vtol, ptol, tnow, dtnow
   type(nek_dvector) :: X0, fin
   type(nek_dns) :: dns

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='old')
   read (u) ldim, lx1, nelv, nsteps, npts
   read (u) re, dt, vtol, ptol
   lvn = nelv*lx1**ldim
   lpn = nelv*(lx1 - 2)**ldim
   allocate (xm1(lvn), ym1(lvn), zm1(lvn), v1mask(lvn), v2mask(lvn), v3mask(lvn), vx(lvn), vy(lvn), vz(lvn), glo(lvn), pr(lpn), t(lvn))
   allocate (xyz(ldim, npts))
   zm1 = 0; v3mask = 0; vz = 0; t = 0
   read (u) xm1, ym1
   read (u) glo
   read (u) v1mask, v2mask
   read (u) vx, vy, pr
   read (u) xyz
   close (u)

   call neklab_gpu_init(0)
   call neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo, v1mask, v2mask, v3mask, .false.)
   call neklab_gpu_set_case(re=re, torder=3, vtol=vtol, ptol=ptol, maxit_v=400, maxit_p=4000, dt=dt, pprecond=1, pproj=0)
   call nek2vec(X0, vx, vy, vz, pr, t)

   call dns%init(X0)
   call dns%set_history_points(xyz)
   call dns%set_reference()
   call dns%advance(nsteps)
   call dns%series(time, probe, dist)
   call dns%info(istep, tnow, dtnow)
   n = size(time)
   write (*, '(A,I6,2ES24.16)') 'INFO ', istep, tnow, dtnow
   write (*, '(A,I6,2I4)') 'SHAPE ', n, size(probe, 2), size(probe, 1)
   open (newunit=u, file='series.bin', access='stream', form='unformatted', status='replace')
   write (u) time, probe, dist
   close (u)
   call dns%hpts('run.his')
   call dns%state(fin)
   write (*, '(A,ES24.16)') 'NORM ', fin%norm()
   call dns%finalize()
   call neklab_gpu_finalize()
end program dns_driver
