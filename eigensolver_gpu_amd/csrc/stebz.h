// stebz.h -- device bisection for the symmetric tridiagonal (internal).
#pragma once
#include "blas3.h"

namespace eig {

// Eigenvalues of T = tridiag(e, d, e) (d_d[N], e_d[N-1] on the device) by Sturm counts, LAPACK dstebz with abstol = 0.
// stebz_prepare writes a scaled copy of T and its Gershgorin bounds into the context's scratch; the two calls below read them.
void stebz_prepare(Ctx& c, hipStream_t st, int N, const double* d_d, const double* e_d);
// (vl, vu] -> the index range il..iu of the eigenvalues inside it (il > iu: none).  Synchronises st.
void stebz_value_range(Ctx& c, hipStream_t st, int N, double vl, double vu, int* il, int* iu);
// w_d[0 : iu - il + 1) <- eigenvalues il..iu (1-based), ascending.  Each value depends only on (d, e, its index).
void stebz_index(Ctx& c, hipStream_t st, int N, int il, int iu, double* w_d);

}  // namespace eig
