! zhegvdx_gpu.F90 -- drop-in replacement for module zhegvdx_gpu (lib_eigsolve/zhegvdx_gpu.F90:24-184).
! Same module name, same procedure name, same argument order and meaning.  The reference
! declares A,B,Z,w,work,rwork with the CUDA-Fortran `device` attribute; standard Fortran has no
! such attribute, so device arrays are passed as type(c_ptr) holding DEVICE addresses
! (hipMalloc / hipfort / OpenMP `use_device_ptr`).  Host arrays keep their Fortran types; the
! reference asks for `pinned` memory, pageable memory works too.
module zhegvdx_gpu
  use iso_c_binding
  implicit none

  interface
    integer(c_int) function eigsolve_zhegvdx(N, A, lda, B, ldb, Z, ldz, il, iu, w, work, lwork, rwork, lrwork, &
                                             work_h, lwork_h, rwork_h, lrwork_h, iwork_h, liwork_h, Z_h, ldz_h,  &
                                             w_h, info, skip_host_copy) bind(C, name="eigsolve_zhegvdx")
      import :: c_int, c_ptr, c_double, c_double_complex
      integer(c_int), value :: N, lda, ldb, ldz, il, iu, lwork, lrwork, lwork_h, lrwork_h, liwork_h, ldz_h
      integer(c_int), value :: skip_host_copy
      type(c_ptr), value    :: A, B, Z, w, work, rwork
      complex(c_double_complex), dimension(*) :: work_h, Z_h
      real(c_double), dimension(*)            :: rwork_h, w_h
      integer(c_int), dimension(*)            :: iwork_h
      integer(c_int)                          :: info
    end function eigsolve_zhegvdx
    integer(c_int) function eigsolve_zhegvdx_ex(itype, jobz, range, N, A, lda, B, ldb, vl, vu, il, iu, meig, w, Z, ldz, &
                                                work, lwork, rwork, lrwork, info) bind(C, name="eigsolve_zhegvdx_ex")
      import :: c_int, c_ptr, c_double, c_char
      integer(c_int), value :: itype, N, lda, ldb, il, iu, ldz, lwork, lrwork
      character(kind=c_char), value :: jobz, range
      real(c_double), value :: vl, vu
      type(c_ptr), value :: A, B, w, Z, work, rwork
      integer(c_int) :: meig, info
    end function eigsolve_zhegvdx_ex
  end interface

contains

  ! See the reference header comment (zhegvdx_gpu.F90:30-74) for the full contract: A x = lambda B x,
  ! eigenpairs il..iu, upper triangles populated (LAPACK ZHEGVX ITYPE=1, JOBZ='V', RANGE='I', UPLO='U').
  subroutine zhegvdx_gpu(N, A, lda, B, ldb, Z, ldz, il, iu, w, work, lwork, rwork, lrwork, &
                         work_h, lwork_h, rwork_h, lrwork_h, iwork_h, liwork_h, Z_h, ldz_h, w_h, info, _skip_host_copy)
    integer                                   :: N, lda, ldb, ldz, il, iu, ldz_h, info
    integer                                   :: lwork_h, lrwork_h, liwork_h, lwork, lrwork
    type(c_ptr)                               :: A, B, Z, w, work, rwork          ! DEVICE pointers
    real(8), dimension(1:lrwork_h)            :: rwork_h
    complex(8), dimension(1:lwork_h)          :: work_h
    integer, dimension(1:liwork_h)            :: iwork_h
    complex(8), dimension(1:ldz_h, 1:N)       :: Z_h
    real(8), dimension(1:N)                   :: w_h
    logical, optional                         :: _skip_host_copy
    integer(c_int) :: skip, istat, cinfo

    skip = 0
    if (present(_skip_host_copy)) then
      if (_skip_host_copy) skip = 1
    end if
    cinfo = 0
    istat = eigsolve_zhegvdx(int(N, c_int), A, int(lda, c_int), B, int(ldb, c_int), Z, int(ldz, c_int), int(il, c_int), &
                             int(iu, c_int), w, work, int(lwork, c_int), rwork, int(lrwork, c_int), work_h,            &
                             int(lwork_h, c_int), rwork_h, int(lrwork_h, c_int), iwork_h, int(liwork_h, c_int), Z_h,   &
                             int(ldz_h, c_int), w_h, cinfo, skip)
    info = cinfo
  end subroutine zhegvdx_gpu

  ! Extended driver (include/eigsolve_gpu.h, eigsolve_zhegvdx_ex): itype 1 / 2 / 3, jobz 'N' / 'V', range 'A' / 'V' / 'I'
  ! (LAPACK ZHEGVX's ITYPE, JOBZ, RANGE, VL, VU, IL, IU, M), UPLO = 'U'.  meig eigenvalues ascending in w(1:meig), eigenvectors
  ! in Z(:, 1:meig) for jobz = 'V' (Z may be c_null_ptr for jobz = 'N').  Device workspaces as zhegvdx_gpu, no host ones.
  subroutine zhegvdx_ex_gpu(itype, jobz, range, N, A, lda, B, ldb, vl, vu, il, iu, meig, w, Z, ldz, work, lwork, rwork, lrwork, &
                            info)
    integer                :: itype, N, lda, ldb, il, iu, meig, ldz, lwork, lrwork, info
    character              :: jobz, range
    real(8)                :: vl, vu
    type(c_ptr)            :: A, B, w, Z, work, rwork          ! DEVICE pointers
    integer(c_int) :: istat, cinfo, cm
    cinfo = 0; cm = 0
    istat = eigsolve_zhegvdx_ex(int(itype, c_int), jobz, range, int(N, c_int), A, int(lda, c_int), B, int(ldb, c_int), vl, vu, &
                                int(il, c_int), int(iu, c_int), cm, w, Z, int(ldz, c_int), work, int(lwork, c_int), rwork,   &
                                int(lrwork, c_int), cinfo)
    meig = cm
    info = cinfo
  end subroutine zhegvdx_ex_gpu

end module zhegvdx_gpu
