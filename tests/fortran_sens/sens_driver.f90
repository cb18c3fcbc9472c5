!> eigenvalue_sensitivity of the shim, called on two mode pairs -- a complex one, with every optional output, and a real one -- read
!! from `case.bin` (written by tests/test_gpu_sens_fortran.py, which stands in for Nek5000).  Prints, per pair, d = <u^+, u^> and the
!! largest modulus of every velocity component of every field returned; the test compares them with the Python call's.
program sens_driver
   use iso_c_binding, only: c_int64_t
   use neklab
   implicit none
   integer :: ldim, lx1, nelv, lvn, lpn, u, q
   integer(c_int64_t), allocatable :: glo(:)
   real(dp), allocatable :: xm1(:), ym1(:), zm1(:), v1mask(:), v2mask(:), v3mask(:), pr(:), t(:), vz(:)
   real(dp), allocatable :: fx(:, :), fy(:, :), ox(:), oy(:), oz(:)
   type(nek_dvector) :: m(6), gre, gim, tre, tim, wmk, sre, sim
   complex(dp) :: d

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='old')
   read (u) ldim, lx1, nelv
   lvn = nelv*lx1**ldim
   lpn = nelv*(lx1 - 2)**ldim
   allocate (xm1(lvn), ym1(lvn), zm1(lvn), v1mask(lvn), v2mask(lvn), v3mask(lvn), glo(lvn), pr(lpn), t(lvn), vz(lvn))
   allocate (fx(lvn, 6), fy(lvn, 6), ox(lvn), oy(lvn), oz(lvn))
   zm1 = 0; v3mask = 0; vz = 0; t = 0; pr = 0
   read (u) xm1, ym1
   read (u) glo
   read (u) v1mask, v2mask
   do q = 1, 6                              ! u_r, u_i, a_r, a_i of the complex pair; u, a of the real pair
      read (u) fx(:, q), fy(:, q)
   end do
   close (u)

   call neklab_gpu_init(0)
   call neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo, v1mask, v2mask, v3mask, .false.)
   do q = 1, 6
      call nek2vec(m(q), fx(:, q), fy(:, q), vz, pr, t)
   end do

   call eigenvalue_sensitivity(m(1), m(3), d, gre, gim, dir_im=m(2), adj_im=m(4), wavemaker=wmk, transp_re=tre, transp_im=tim)
   write (*, '(A,2(1X,ES24.16))') 'D1', real(d), aimag(d)
   call show('GRE1', gre); call show('GIM1', gim); call show('TRE1', tre); call show('TIM1', tim); call show('WMK1', wmk)

   call eigenvalue_sensitivity(m(5), m(6), d, sre, sim)
   write (*, '(A,2(1X,ES24.16))') 'D2', real(d), aimag(d)
   call show('GRE2', sre); call show('GIM2', sim)
   write (*, '(A)') 'DONE'

contains

   subroutine show(tag, vec)
      character(len=*), intent(in) :: tag
      type(nek_dvector), intent(in) :: vec
      call vec2nek(ox, oy, oz, pr, t, vec)
      write (*, '(A,2(1X,ES24.16))') tag, maxval(abs(ox)), maxval(abs(oy))
   end subroutine

end program sens_driver
