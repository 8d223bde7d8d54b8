// stebz.hip -- eigenvalues of the symmetric tridiagonal by Sturm-count multisection, on the device.
//
// The eigenvalues-only path of the extended driver (evd.hip, eigsolve_?hegvdx_ex with jobz = 'N') and the index range of a
// value-range solve.  Algorithm: LAPACK dstebz / dlaebz with abstol = 0 (published algorithm, restated):
//   * T is scaled by its largest absolute entry first (the e_i^2 of the recurrence overflow / underflow near 1e+-154);
//   * the count of sigma is the number of non-positive pivots of T - sigma I,
//         q_1 = d_1 - sigma,   q_i = (d_i - sigma) - e_{i-1}^2 / q_{i-1},   |q_i| < pivmin -> q_i = -pivmin,
//     with pivmin = safmin * max(1, max e_i^2): 1 / q never overflows, and eigenvalues within pivmin of sigma count as below it;
//   * start interval: the Gershgorin bounds widened as dstebz widens them; an interval [lo, hi] with count(lo) < k <= count(hi)
//     holds eigenvalue k; it has converged when hi - lo < max(ulp * ||T||, pivmin, 2 ulp * max(|lo|, |hi|)); the result is the
//     midpoint.
// Parallel shape (MI355X): a group of G lanes per eigenvalue, 64 / G eigenvalues per wave.  The G lanes count at the G interior
// points of a (G+1)-section of the group's interval; one ballot gives every group the first point whose count reaches k, and the
// interval shrinks G + 1 times per step.  Every lane walks the whole recurrence with a wave-uniform index, so (d_i, e_{i-1}^2) is
// one scalar load per step (scalar cache / L2, for every order: no LDS).  Divisions are v_rcp_f64 + two Newton steps (lanes.h).
// G depends on N only, so a value depends only on (d, e, its index): single call, subsets and repeated calls give the same bits.
// Output is ascending by construction: every group starts from the same interval and cuts it at the same points, and a group
// looking for a larger k never picks an earlier point, so the intervals of k < k' are equal or disjoint in that order.
#include <algorithm>
#include <cfloat>

#include "stebz.h"
#include "lanes.h"

namespace eig {

namespace {

constexpr int kUnroll = 8;            // recurrence steps per batch of scalar loads; the scaled copy is padded to a multiple
constexpr double kPadDiag = 1e300;    // padding entries (d = 1e300, e^2 = 0): a positive pivot, never counted
constexpr int kMaxSteps = 128;        // multisection steps (convergence takes ~53 / log2(G + 1); the bound only guards termination)
enum { P_GL = 0, P_GU, P_ATOL, P_PIVMIN, P_SCALE, P_COUNT };

__device__ __forceinline__ int sturm_count(int npad, const double2* __restrict__ de, double sigma, double pivmin) {
    int cnt = 0;
    double q = 1.0;   // (the first entry carries e^2 = 0)
    for (int i = 0; i < npad; i += kUnroll) {
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            const double2 v = de[i + j];
            q = fma(-v.y, fast_rcp(q), v.x - sigma);
            q = fabs(q) < pivmin ? -pivmin : q;
            cnt += q <= 0.0 ? 1 : 0;
        }
    }
    return cnt;
}

__device__ __forceinline__ double block_reduce_1024(double v, double* sh, bool is_min) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = is_min ? fmin(v, u) : fmax(v, u);
    }
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    v = sh[0];
    for (int w = 1; w < 16; ++w) v = is_min ? fmin(v, sh[w]) : fmax(v, sh[w]);
    return v;
}

// One workgroup: scale, scaled copy de[i] = (d_i, e_{i-1}^2) / scale^(1, 2) padded to npad, Gershgorin bounds, pivmin, atol.
__global__ void __launch_bounds__(1024) stebz_prep_kernel(int N, int npad, const double* __restrict__ d, const double* __restrict__ e,
                                                         double2* __restrict__ de, double* __restrict__ par) {
    __shared__ double sh[16];
    const int tid = threadIdx.x;
    double mx = 0.0;
    for (int i = tid; i < N; i += 1024) {
        mx = fmax(mx, fabs(d[i]));
        if (i < N - 1) mx = fmax(mx, fabs(e[i]));
    }
    const double scale = block_reduce_1024(mx, sh, false);   // (0: T = 0, every eigenvalue is exactly 0)
    const double inv = scale > 0.0 ? 1.0 / scale : 1.0;
    double lo = DBL_MAX, hi = -DBL_MAX, e2max = 0.0;
    for (int i = tid; i < npad; i += 1024) {
        if (i < N) {
            const double di = d[i] * inv;
            const double el = i > 0 ? fabs(e[i - 1]) * inv : 0.0, er = i < N - 1 ? fabs(e[i]) * inv : 0.0;
            de[i] = make_double2(di, el * el);
            lo = fmin(lo, di - el - er);
            hi = fmax(hi, di + el + er);
            e2max = fmax(e2max, el * el);
        } else {
            de[i] = make_double2(kPadDiag, 0.0);
        }
    }
    lo = block_reduce_1024(lo, sh, true);
    hi = block_reduce_1024(hi, sh, false);
    e2max = block_reduce_1024(e2max, sh, false);
    if (tid == 0) {
        const double ulp = DBL_EPSILON, fudge = 2.1;
        const double pivmin = DBL_MIN * fmax(1.0, e2max);
        const double tnorm = fmax(fabs(lo), fabs(hi));
        par[P_GL] = lo - fudge * tnorm * ulp * N - fudge * 2.0 * pivmin;
        par[P_GU] = hi + fudge * tnorm * ulp * N + fudge * pivmin;
        par[P_ATOL] = ulp * tnorm;
        par[P_PIVMIN] = pivmin;
        par[P_SCALE] = scale;
    }
}

// cnt[0] = count(vl), cnt[1] = count(vu) (one wave; a sigma outside the Gershgorin interval counts 0 or N without a recurrence)
__global__ void __launch_bounds__(64) stebz_count_kernel(int N, int npad, const double2* __restrict__ de, const double* __restrict__ par,
                                                         double vl, double vu, int* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const double v = lane == 0 ? vl : vu, scale = par[P_SCALE];
    const double s = scale > 0.0 ? v / scale : v;
    const double gl = par[P_GL], gu = par[P_GU];
    int c = sturm_count(npad, de, fmin(fmax(s, gl), gu), par[P_PIVMIN]);
    if (s <= gl) c = 0;
    if (s >= gu) c = N;
    if (scale == 0.0) c = v >= 0.0 ? N : 0;
    if (lane < 2) cnt[lane] = c;
}

// Eigenvalues k0 + 1 .. k0 + m (1-based) -> w[0 .. m).  G = 1 << lg lanes per eigenvalue.
__global__ void __launch_bounds__(256) stebz_bisect_kernel(int npad, const double2* __restrict__ de, const double* __restrict__ par, int lg,
                                                          int k0, int m, double* __restrict__ w) {
    const int G = 1 << lg, per_wave = 64 >> lg;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave * per_wave >= m) return;   // (wave-uniform)
    const int grp = lane >> lg, sub = lane & (G - 1);
    const int j = wave * per_wave + grp;
    const int k = k0 + min(j, m - 1) + 1;   // (groups past the end repeat the last eigenvalue and write nothing)
    const double atol = par[P_ATOL], pivmin = par[P_PIVMIN], reltol = 2.0 * DBL_EPSILON;
    const double frac = (double)(sub + 1) / (double)(G + 1);
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    double lo = par[P_GL], hi = par[P_GU];
    for (int it = 0; it < kMaxSteps; ++it) {
        const bool conv = (hi - lo) < fmax(fmax(atol, pivmin), reltol * fmax(fabs(lo), fabs(hi)));
        if (__ballot(!conv) == 0ull) break;
        const double sigma = fma(hi - lo, frac, lo);
        const int cnt = sturm_count(npad, de, sigma, pivmin);
        const unsigned long long gb = (__ballot(cnt >= k) >> (grp << lg)) & gmask;
        const int f = gb ? __ffsll((long long)gb) - 1 : G;   // first point with count >= k (G: none)
        const double s_hi = __shfl(sigma, (grp << lg) + min(f, G - 1));
        const double s_lo = __shfl(sigma, (grp << lg) + max(f - 1, 0));
        if (!conv) {
            if (f < G) hi = s_hi;
            if (f > 0) lo = s_lo;
        }
    }
    if (sub == 0 && j < m) w[j] = 0.5 * (lo + hi) * par[P_SCALE];   // (T = 0: scale 0, exact zeros)
}

// lanes per eigenvalue: enough lanes in flight to fill the chip at the orders the library solves (about 2 waves per SIMD when all
// N eigenvalues are wanted), from N alone so that a value never depends on how many are wanted
int stebz_lg(int N) {
    int lg = 5;
    while (lg > 2 && (long)N << lg > 131072L) --lg;
    return lg;
}

int padded(int N) { return (N + kUnroll - 1) / kUnroll * kUnroll; }

}  // namespace

void stebz_prepare(Ctx& c, hipStream_t st, int N, const double* d_d, const double* e_d) {
    const int npad = padded(N);
    double2* de = c.scratch<double2>("stebz_de", (size_t)npad);
    double* par = c.scratch<double>("stebz_par", P_COUNT);
    hipLaunchKernelGGL(stebz_prep_kernel, dim3(1), dim3(1024), 0, st, N, npad, d_d, e_d, de, par);
    EIG_HIP(hipGetLastError());
}

void stebz_value_range(Ctx& c, hipStream_t st, int N, double vl, double vu, int* il, int* iu) {
    const int npad = padded(N);
    int* cnt_d = c.scratch<int>("stebz_cnt", 2);
    int* cnt_h = reinterpret_cast<int*>(c.host_scratch_bytes("stebz_cnt_h", 2 * sizeof(int)));
    hipLaunchKernelGGL(stebz_count_kernel, dim3(1), dim3(64), 0, st, N, npad, (const double2*)c.scratch<double2>("stebz_de", npad),
                       (const double*)c.scratch<double>("stebz_par", P_COUNT), vl, vu, cnt_d);
    EIG_HIP(hipGetLastError());
    EIG_HIP(hipMemcpyAsync(cnt_h, cnt_d, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    c.sync(st);
    *il = cnt_h[0] + 1;
    *iu = cnt_h[1];
}

void stebz_index(Ctx& c, hipStream_t st, int N, int il, int iu, double* w_d) {
    const int m = iu - il + 1;
    if (m <= 0) return;
    const int npad = padded(N), lg = stebz_lg(N);
    const int waves = (m + (64 >> lg) - 1) / (64 >> lg);
    hipLaunchKernelGGL(stebz_bisect_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, npad,
                       (const double2*)c.scratch<double2>("stebz_de", npad), (const double*)c.scratch<double>("stebz_par", P_COUNT), lg,
                       il - 1, m, w_d);
    EIG_HIP(hipGetLastError());
}

}  // namespace eig
