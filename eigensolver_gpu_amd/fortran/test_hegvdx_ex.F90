! test_hegvdx_ex.F90 -- Fortran driver for the extended generalized driver (modules zhegvdx_gpu / dsygvdx_gpu, procedures
! zhegvdx_ex_gpu / dsygvdx_ex_gpu): seeded random Hermitian / symmetric pairs (B positive definite) of order 200, every
! (itype, jobz, range) in both precisions, eigenvalues against LAPACK ?hegvd(itype) on the host.
!     ./test_hegvdx_ex          prints one line per solve and PASSED when every solve agrees
program test_hegvdx_ex
  use iso_c_binding
  use hip_min
  use zhegvdx_gpu
  use dsygvdx_gpu
  use lapack_host
  implicit none
  integer, parameter :: N = 200
  character, parameter :: jobzs(2) = ['N', 'V'], ranges(3) = ['A', 'V', 'I']
  complex(8), allocatable, target :: Az(:,:), Bz(:,:), Tz(:,:), Uz(:,:)
  real(8), allocatable, target :: Ad(:,:), Bd(:,:), Td(:,:), Ud(:,:), wref(:), wh(:), re(:,:), im(:,:)
  type(c_ptr) :: A_d, B_d, Z_d, w_d, work_d, rwork_d
  integer :: prec, itype, jz, rg, info, meig, il, iu, k1, k2, want, lwork, lrwork, nbad, i
  integer(c_int) :: istat
  real(8) :: vl, vu, err, nrm
  integer(c_size_t) :: esz

  nbad = 0
  allocate(Az(N,N), Bz(N,N), Tz(N,N), Uz(N,N), Ad(N,N), Bd(N,N), Td(N,N), Ud(N,N), wref(N), wh(N), re(N,N), im(N,N))
  do prec = 1, 2                          ! 1: complex (zhegvdx_ex_gpu), 2: real (dsygvdx_ex_gpu)
    esz = merge(16_c_size_t, 8_c_size_t, prec == 1)
    lwork = 2 * 64 * 64 + merge(65, 66, prec == 1) * N
    lrwork = N
    istat = hipMalloc(A_d, esz * N * N)
    istat = hipMalloc(B_d, esz * N * N)
    istat = hipMalloc(Z_d, esz * N * N)
    istat = hipMalloc(w_d, 8_c_size_t * N)
    istat = hipMalloc(work_d, esz * lwork)
    istat = hipMalloc(rwork_d, 8_c_size_t * lrwork)
    do itype = 1, 3
      call random_pair(prec, 100 * prec + itype)
      ! host reference: all eigenvalues of the pair (A, B copies are overwritten)
      if (prec == 1) then
        Tz = Az
        Uz = Bz
        call host_zhegvd(N, Tz, N, Uz, N, wref, info, itype)
      else
        Td = Ad
        Ud = Bd
        call host_dsygvd(N, Td, N, Ud, N, wref, info, itype)
      end if
      if (info /= 0) then
        print '(a,i0)', " host LAPACK failed, info = ", info
        nbad = nbad + 1
        cycle
      end if
      nrm = maxval(abs(wref))
      il = N / 5; iu = N / 2
      k1 = N / 4; k2 = (3 * N) / 4          ! (vl, vu] at the midpoints of the gaps after wref(k1) and wref(k2)
      vl = 0.5d0 * (wref(k1) + wref(k1 + 1)); vu = 0.5d0 * (wref(k2) + wref(k2 + 1))
      do jz = 1, 2
        do rg = 1, 3
          call upload(prec)
          if (prec == 1) then
            call zhegvdx_ex_gpu(itype, jobzs(jz), ranges(rg), N, A_d, N, B_d, N, vl, vu, il, iu, meig, w_d, Z_d, N, &
                                work_d, lwork, rwork_d, lrwork, info)
          else
            call dsygvdx_ex_gpu(itype, jobzs(jz), ranges(rg), N, A_d, N, B_d, N, vl, vu, il, iu, meig, w_d, Z_d, N, &
                                work_d, lwork, info)
          end if
          select case (ranges(rg))
          case ('A'); want = N; k1 = 0
          case ('V'); want = k2 - N / 4; k1 = N / 4
          case default; want = iu - il + 1; k1 = il - 1
          end select
          err = huge(1.0d0)
          if (info == 0 .and. meig == want) then
            istat = hipMemcpy(c_loc(wh), w_d, 8_c_size_t * meig, hipMemcpyDeviceToHost)
            err = 0.0d0
            do i = 1, meig
              err = max(err, abs(wh(i) - wref(k1 + i)) / nrm)
            end do
          end if
          k1 = N / 4
          print '(a,a,i2,a,a,a,a,a,i4,a,i4,a,es10.3)', merge("zhegvdx_ex_gpu", "dsygvdx_ex_gpu", prec == 1), " itype", itype, &
                " jobz ", jobzs(jz), " range ", ranges(rg), ": info", info, " meig", meig, "  max rel err(w) vs ?hegvd", err
          if (err > 1.0d-11) nbad = nbad + 1
        end do
      end do
    end do
    istat = hipFree(A_d); istat = hipFree(B_d); istat = hipFree(Z_d); istat = hipFree(w_d)
    istat = hipFree(work_d); istat = hipFree(rwork_d)
  end do
  if (nbad == 0) then
    print '(a)', " PASSED"
  else
    print '(a,i0,a)', " FAILED (", nbad, " solves)"
    stop 1
  end if

contains

  ! A Hermitian (symmetric), B = X X^H + N I, from a seeded generator
  subroutine random_pair(p, seed)
    integer, intent(in) :: p, seed
    integer :: ns
    integer, allocatable :: sv(:)
    call random_seed(size=ns)
    allocate(sv(ns))
    sv = seed + 37 * [(i, i = 1, ns)]
    call random_seed(put=sv)
    call random_number(re); call random_number(im)
    if (p == 1) then
      Tz = cmplx(re - 0.5d0, im - 0.5d0, kind=8)
      Az = Tz + conjg(transpose(Tz))
      call random_number(re); call random_number(im)
      Tz = cmplx(re - 0.5d0, im - 0.5d0, kind=8)
      Bz = matmul(Tz, conjg(transpose(Tz)))
      do i = 1, N
        Bz(i, i) = Bz(i, i) + N
      end do
    else
      Ad = re + transpose(re) - 1.0d0
      Bd = matmul(im, transpose(im))
      do i = 1, N
        Bd(i, i) = Bd(i, i) + N
      end do
    end if
  end subroutine random_pair

  subroutine upload(p)
    integer, intent(in) :: p
    if (p == 1) then
      istat = hipMemcpy(A_d, c_loc(Az), 16_c_size_t * N * N, hipMemcpyHostToDevice)
      istat = hipMemcpy(B_d, c_loc(Bz), 16_c_size_t * N * N, hipMemcpyHostToDevice)
    else
      istat = hipMemcpy(A_d, c_loc(Ad), 8_c_size_t * N * N, hipMemcpyHostToDevice)
      istat = hipMemcpy(B_d, c_loc(Bd), 8_c_size_t * N * N, hipMemcpyHostToDevice)
    end if
  end subroutine upload

end program test_hegvdx_ex
