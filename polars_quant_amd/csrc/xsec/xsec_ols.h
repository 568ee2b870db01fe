// xsec/xsec_ols.h -- the moments and L D L^T core of D-17, shared by regress.hip (D-17), orth.hip (D-19) and rolling_regress.hip (D-28),
// and D-17's fit on it, which regress.hip and linear.hip (D-24) share.
//
// D-17's return is one more column behind the factors: with NV = K + 1 columns f_0 .. f_{K-1}, r its pass 2 is the packed lower triangle
// of the centred cross-products, s[j (j + 1) / 2 + l] = sum d_j d_l (l <= j): C in rows 0 .. K-1, then c and Srr in row K.  D-19's pass 2 is
// the same triangle of its K factors, so the last level of orthogonalize(K) is regress(K - 1) with r = f_{K-1}.  Both files get from here:
//  * combine:  one thread per unit adds the block sums in ascending block order from 0.0 (xo_combine); after pass 1 it writes n and
//              the means (xo_means_kernel).
//  * solve:    xo_ldl factorises the leading R x R block C = L D L^T by rows and counts the leading pivots that are not singular; it is
//              prefix-consistent, so the leading k x k block is what D-17 factorises for k regressors.  xo_forward and xo_back solve
//              on that block.  The operation order is D-17's, restated in tests/xsec_regress_ref.py and tests/xsec_orth_ref.py.
//  * fit:      xo_fit is the whole of D-17's solve on one triangle: the factorization, b, the intercept, and diag(C^-1) and
//              1/n + xbar^T C^-1 xbar for the standard errors.  rg_solve_kernel and ln_solve_kernel are calls of it, so the two agree
//              bit for bit by construction.  Two callers stay on xo_ldl / xo_forward / xo_back: orth.hip's or_solve_kernel solves
//              K - 1 nested prefix systems without an intercept, and rr_window_kernel (rolling_regress.hip) keeps the fit's first half
//              in its row loop (its header says why).
//  * host:     xo_workspace carves what both workspaces begin with; each caller appends its own rows.
// The blocked pass kernels, and with them the structs of input columns, stay one per file: one kernel on NV columns compiles to other
// code for regress.hip and its time-series form ran slower (EXPERIMENTS.md, "One pass kernel for regress.hip and orth.hip").
#pragma once
#include <type_traits>
#include "xsec_dev.h"

namespace {

constexpr int XO_MAX_K = 8;             // PQ_REGRESS_MAX_K
constexpr double XO_SINGULAR = 1e-12;   // pivot D_j <= 1e-12 * C[j][j]: singular

constexpr int xo_tri(int nv) { return nv * (nv + 1) / 2; }                    // entries of the packed triangle; row j starts at xo_tri(j)
constexpr int xo_ahead(int nv) { return nv <= 2 ? 8 : (nv <= 4 ? 4 : 2); }    // indices loaded ahead: about 16 loads in flight per lane

template <int NA>
__device__ __forceinline__ void xo_combine(const double *ps, int64_t nblk, int64_t units, int64_t u, double (&s)[NA]) {
#pragma unroll
    for (int q = 0; q < NA; q++) s[q] = 0.0;
    for (int64_t k = 0; k < nblk; k++)
#pragma unroll
        for (int q = 0; q < NA; q++) s[q] += ps[(k * NA + q) * units + u];
}

// after pass 1: n and the NV means, [NV][units]
template <int NV>
__global__ __launch_bounds__(64) void xo_means_kernel(const double *ps, const int32_t *pcnt, int64_t nblk, int64_t units, int32_t *n_out,
                                                      double *mean) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    double s[NV];
    xo_combine<NV>(ps, nblk, units, u, s);
    int32_t n = 0;
    for (int64_t k = 0; k < nblk; k++) n += pcnt[k * units + u];
    n_out[u] = n;
    const double dn = (double)n;
#pragma unroll
    for (int q = 0; q < NV; q++) mean[(int64_t)q * units + u] = s[q] / dn;
}

// ---------------------------------------------------------------- solve
// C = L D L^T by rows on the leading R x R block of the packed triangle s; W[j][k] is the numerator of L[j][k].  Returns the number of
// leading pivots with D_j > 1e-12 C[j][j]: a NaN pivot (from an overflow) is singular, and so is every pivot behind a singular one.
template <int R> __device__ __forceinline__ int xo_ldl(const double *s, double (&L)[R][R], double (&D)[R]) {
    double W[R][R];
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
        for (int k = 0; k < R; k++) { L[j][k] = j == k ? 1.0 : 0.0; W[j][k] = 0.0; }
    int npiv = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
#pragma unroll
        for (int k = 0; k < j; k++) {
            double w = s[xo_tri(j) + k];
#pragma unroll
            for (int m = 0; m < k; m++) w -= W[j][m] * L[k][m];
            W[j][k] = w;
            L[j][k] = w / D[k];
        }
        const double cjj = s[xo_tri(j) + j];
        double dj = cjj;
#pragma unroll
        for (int m = 0; m < j; m++) dj -= W[j][m] * L[j][m];
        D[j] = dj;
        if (npiv == j && dj > XO_SINGULAR * cjj) npiv = j + 1;
    }
    return npiv;
}

// forward substitution on the leading k x k block: z_m = v_m - sum_{i < m} L[m][i] z_i (sum ascending from 0.0)
template <int R> __device__ __forceinline__ void xo_forward(const double (&L)[R][R], const double *v, int k, double (&z)[R]) {
#pragma unroll
    for (int m = 0; m < k; m++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < m; i++) s += L[m][i] * z[i];
        z[m] = v[m] - s;
    }
}

// back substitution on the leading k x k block: y_j = z_j / D_j; b_j = y_j - sum_{m > j} L[m][j] b_m (m ascending, from 0.0)
template <int R>
__device__ __forceinline__ void xo_back(const double (&L)[R][R], const double (&D)[R], const double (&z)[R], int k, double (&b)[R]) {
#pragma unroll
    for (int j = k - 1; j >= 0; j--) {
        double t = 0.0;
#pragma unroll
        for (int m = j + 1; m < k; m++) t += L[m][j] * b[m];
        b[j] = z[j] / D[j] - t;
    }
}

// D-17's fit on the packed triangle s of the K + 1 columns x_0 .. x_{K-1}, y (C in rows 0 .. K-1, then c and Syy in row K), n members:
// b[0 .. K) and the intercept b[K] = ybar - sum_j b_j xbar_j, v[0 .. K) = diag(C^-1) and v[K] = 1/n + xbar^T C^-1 xbar for the standard
// errors.  xbar, b and v are read and written `stride` doubles apart: a [rows][units] workspace, or arrays (stride 1).  Returns whether
// the system solved; without a solution nothing is read or written.
template <int K>
__device__ __forceinline__ bool xo_fit(const double *s, int64_t n, const double *xbar, const double *ybar, double *b, double *v,
                                       int64_t stride) {
    double L[K][K], D[K];
    if (!(xo_ldl<K>(s, L, D) == K && n >= K + 2)) return false;
    double z[K], bb[K], fbar[K];
#pragma unroll
    for (int j = 0; j < K; j++) fbar[j] = xbar[j * stride];
    xo_forward<K>(L, s + xo_tri(K), K, z);   // c = row K of the triangle
    xo_back<K>(L, D, z, K, bb);
    double sa = 0.0;
#pragma unroll
    for (int j = 0; j < K; j++) sa += bb[j] * fbar[j];
#pragma unroll
    for (int j = 0; j < K; j++) b[j * stride] = bb[j];
    b[K * stride] = *ybar - sa;
    // (C^-1)_jj = sum_m (L^-1 e_j)_m^2 / D_m, m ascending from 0.0
#pragma unroll
    for (int j = 0; j < K; j++) {
        double e[K], w[K];
#pragma unroll
        for (int m = 0; m < K; m++) e[m] = m == j ? 1.0 : 0.0;
        xo_forward<K>(L, e, K, w);
        double vj = 0.0;
#pragma unroll
        for (int m = 0; m < K; m++) vj += w[m] * w[m] / D[m];
        v[j * stride] = vj;
    }
    double w[K], q = 0.0;
    xo_forward<K>(L, fbar, K, w);
#pragma unroll
    for (int m = 0; m < K; m++) q += w[m] * w[m] / D[m];
    v[K * stride] = 1.0 / (double)n + q;
    return true;
}

// ---------------------------------------------------------------- host
// f(std::integral_constant<int, k>) for a runtime k in [1, MAX] (the entry points check the range): one instantiation per K
template <int MAX, int K = 1, class F> auto xo_with_k(int k, F &&f) {
    if constexpr (K == MAX) return f(std::integral_constant<int, K>{});
    else return k == K ? f(std::integral_constant<int, K>{}) : xo_with_k<MAX, K + 1>(k, f);
}

// workspace: n, flag (i32) | `rows` f64 rows, `row` doubles apart: the nv means, then the caller's own | block partials [nblk][na][units]
// (f64) | block counts (i32)
struct XoWs {
    int32_t *n, *flag;
    double *mean, *own;   // own = the caller's rows, behind the nv means
    size_t row;
    double *ps;
    int32_t *pcnt;
};
inline pq_status xo_workspace(pq_ctx *ctx, const char *who, int64_t units, int64_t nblk, int nv, int rows, int na, XoWs *w) {
    const size_t U = (size_t)units, part = (size_t)nblk * U;
    w->row = XsWs::pitch<double>(U);
    return xs_ws_carve(ctx, who, [&](XsWs &c) {
        c.take(w->n, U).take(w->flag, U).take(w->mean, U, nv).take(w->own, U, rows - nv).take(w->ps, part * na).take(w->pcnt, part);
    });
}

} // namespace
