!> Every name the shim exports for the strong-form operator L, called once, with the reference's argument lists: the five array
!! routines (direct and adjoint where they take `trans`), lns_linop%matvec / rmatvec, nek_otd%matvec / rmatvec through a
!! class(abstract_linop_rdp) pointer (nek_otd_linop), and apply_exptA.  Nek5000 is replaced by `case.bin` (written by tests/test_gpu_lns_fortran.py);
!! the results go to `out.bin`, two velocity fields each, in the order of the calls.  `lns_driver nobase` calls an array routine without
!! set_lns_baseflow and must stop with the message that names it.
program lns_driver
   use iso_c_binding, only: c_int64_t
   use LightKrylov, only: abstract_linop_rdp
   use neklab
   implicit none
   integer :: ldim, lx1, nelv, lvn, lpn, r, nsteps, u, w, i, info
   integer(c_int64_t), allocatable :: glo(:)
   real(dp), allocatable :: xm1(:), ym1(:), zm1(:), v1mask(:), v2mask(:), v3mask(:), vx(:), vy(:), vz(:), pr(:), t(:)
   real(dp), allocatable :: ux(:), uy(:), uz(:), pp(:), ox(:), oy(:), oz(:), bx(:, :), by(:, :), bp(:, :)
   real(dp) :: re, dt, vtol, ptol, tau
   type(nek_dvector) :: bf, vin, vout
   type(lns_linop), target :: L
   type(nek_otd), target :: OTD
   type(nek_otd_linop), target :: OTDop
   type(exptA_linop), target :: A
   class(abstract_linop_rdp), pointer :: op
   type(otd_opts) :: opts
   character(len=32) :: arg

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='old')
   read (u) ldim, lx1, nelv, r, nsteps
   read (u) re, dt, vtol, ptol, tau
   lvn = nelv*lx1**ldim
   lpn = nelv*(lx1 - 2)**ldim
   allocate (xm1(lvn), ym1(lvn), zm1(lvn), v1mask(lvn), v2mask(lvn), v3mask(lvn), vx(lvn), vy(lvn), vz(lvn), glo(lvn), pr(lpn), t(lvn))
   allocate (ux(lvn), uy(lvn), uz(lvn), pp(lpn), ox(lvn), oy(lvn), oz(lvn), bx(lvn, r), by(lvn, r), bp(lpn, r))
   zm1 = 0; v3mask = 0; vz = 0; t = 0; uz = 0; oz = 0
   read (u) xm1, ym1
   read (u) glo
   read (u) v1mask, v2mask
   read (u) vx, vy, pr                      ! the base flow
   read (u) ux, uy, pp                      ! the input
   do i = 1, r
      read (u) bx(:, i), by(:, i), bp(:, i)   ! the OTD basis
   end do
   close (u)

   call neklab_gpu_init(0)
   call neklab_gpu_set_mesh(ldim, lx1, nelv, xm1, ym1, zm1, glo, v1mask, v2mask, v3mask, .false.)
   call neklab_gpu_set_case(re=re, torder=3, vtol=vtol, ptol=ptol, maxit_v=400, maxit_p=4000, dt=dt, cfl_limit=0.4_dp, pprecond=1, pproj=0)

   call get_command_argument(1, arg)
   if (trim(arg) == 'nobase') then
      call apply_Lv(ox, oy, oz, ux, uy, uz)
      stop 0
   end if

   call nek2vec(bf, vx, vy, vz, pr, t)
   call nek2vec(vin, ux, uy, uz, pp, t)
   open (newunit=w, file='out.bin', access='stream', form='unformatted', status='replace')

   ! the array routines
   call set_lns_baseflow(bf)
   call apply_L(ox, oy, oz, ux, uy, uz, pp); write (w) ox, oy
   call apply_L(ox, oy, oz, ux, uy, uz, pp, trans=.true.); write (w) ox, oy
   call apply_Lv(ox, oy, oz, ux, uy, uz); write (w) ox, oy
   call apply_Lv(ox, oy, oz, ux, uy, uz, trans=.true.); write (w) ox, oy
   call compute_LNS_conv(ox, oy, oz, ux, uy, uz); write (w) ox, oy
   call compute_LNS_conv(ox, oy, oz, ux, uy, uz, trans=.true.); write (w) ox, oy
   call compute_LNS_laplacian(ox, oy, oz, ux, uy, uz); write (w) ox, oy
   call compute_LNS_gradp(ox, oy, oz, pp); write (w) ox, oy

   ! the device-resident operator
   L%baseflow = bf
   call L%init()
   op => L
   call op%matvec(vin, vout); call dump(vout)
   call op%rmatvec(vin, vout); call dump(vout)

   ! nek_otd as a linear operator, after a few steps
   OTD%r = r
   OTD%baseflow = bf
   allocate (OTD%basis(r))
   do i = 1, r
      call nek2vec(OTD%basis(i), bx(:, i), by(:, i), vz, bp(:, i), t)
   end do
   opts%solve_baseflow = .true.; opts%orthostep = 2      ! L about the base flow as the run has moved it
   call OTD%init(opts)
   call OTD%advance(nsteps)
   OTDop%otd => OTD
   op => OTDop
   call op%matvec(vin, vout); call dump(vout)
   call op%rmatvec(vin, vout); call dump(vout)
   call OTD%close()

   ! apply_exptA
   A%baseflow = bf
   A%tau = 1.0_dp
   call A%init()
   op => A
   call apply_exptA(vout, op, vin, tau, info); call dump(vout)
   call apply_exptA(vout, op, vin, tau, info, trans=.true.); call dump(vout)
   write (*, '(A,I0)') 'INFO ', info
   close (w)
   write (*, '(A)') 'DONE'

contains

   subroutine dump(vec)
      type(nek_dvector), intent(in) :: vec
      call vec2nek(ox, oy, oz, pr, t, vec)
      write (w) ox, oy
   end subroutine

end program lns_driver
