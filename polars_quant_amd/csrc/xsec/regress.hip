// xsec/regress.hip -- OLS with t-tests: the per-day cross-sectional regression (Factor.factor_return / fama_macbeth), the per-symbol
// time-series regression (Factor.time_series_regression) and the correlation t-test (Factor.ic_test); README.md:1521-1600,
// README-only => decision D-17, DESIGN.md section 2.
//
// Columns are symbol-major [n_series][stride].  A "unit" is what one regression is fitted for: a day (cross-sectional form: the sums run
// over the symbols of a strided column) or a symbol (time-series form: the sums run over the days of a row).  Model r = a + sum_j b_j f_j.
//  1. passes:  one thread per (unit, block of 256 summation indices) sums its block in ascending index order from 0.0, members only:
//              pass 1 n, sum r, sum f_j; pass 2 the centred cross-products C[j][k] (k <= j), c[j] and Srr; pass 3 the squared
//              residuals.  Cross-sectional: consecutive threads on consecutive days (coalesced).  Time-series: consecutive threads on
//              consecutive symbols, each walking its own row; a factor flagged in series_mask is one [len] series read by every symbol.
//  2. combine: one thread per unit adds the block sums in ascending block order from 0.0.  After pass 2 it factorises C = L D L^T,
//              solves for b and the intercept, and keeps diag(C^-1) and fbar^T C^-1 fbar for the standard errors; after pass 3 it
//              writes coef / t / p / R^2 / n.  The operation order is D-17's, restated in tests/xsec_regress_ref.py.  The combine,
//              the means, the factorization, the two substitutions and the head of the workspace are in xsec_ols.h, which orth.hip
//              (D-19) shares: pass 2's sums are the packed triangle of the K + 1 columns f_0 .. f_{K-1}, r, and D-19's last level is
//              this regression with r = f_{K-1}.  The whole solve after pass 2 is xo_fit (xsec_ols.h) and the statistics after
//              pass 3 are rg_coef_stats / rg_r2 (xsec_ttest.h): linear.hip (D-24) calls the same two.  The pass kernel is this
//              file's own (xsec_ols.h says why).
//  3. summary: (cross-sectional) one 64-lane workgroup per regressor: the Fama-MacBeth mean / std / t / p over the days with a solution.
// p-values: two-sided Student t, p = I_{df / (df + t^2)}(df / 2, 1/2), by the Lentz continued fraction in double-double arithmetic
// (near x = 1 the fraction loses ~log10(1 / (1 - x)) digits in plain f64), with log Gamma(a + 1/2) / Gamma(a) from its asymptotic
// series (lgamma(a) - lgamma(a + 1/2) cancels at large df).  Accurate to a few 1e-13 relative on df in [1, 1e5], |t| <= 50.
#include "xsec_ols.h"
#include "xsec_ttest.h"

namespace {

// ---------------------------------------------------------------- passes
enum RgPass { RG_P1 = 1, RG_P2 = 2, RG_P3 = 3 };

template <int K> struct RgNa {   // accumulators per pass
    static constexpr int P1 = K + 1, P2 = K * (K + 1) / 2 + K + 1, P3 = 1;
};

struct RgIn {
    const double *f[XO_MAX_K];
    const double *r;
    uint32_t series;       // time-series form: bit j = f[j] is one [len] series shared by every symbol
    Dims d;
};

// per-unit state: [rows][units] f64 rows
struct RgUnit {
    int32_t *n;
    int32_t *ok;       // 1: solved
    double *mean;      // [K + 1]: rbar, fbar_0 .. fbar_{K-1}
    double *b;         // [K + 1]: b_0 .. b_{K-1}, intercept
    double *v;         // [K + 1]: diag(C^-1), then 1/n + fbar^T C^-1 fbar
    double *srr;
};

template <int K, int P, bool TS>
__global__ __launch_bounds__(64) void rg_pass_kernel(RgIn in, RgUnit un, double *ps, int32_t *pcnt) {
    constexpr int NA = P == RG_P1 ? RgNa<K>::P1 : (P == RG_P2 ? RgNa<K>::P2 : RgNa<K>::P3);
    const Dims d = in.d;
    const int64_t units = TS ? d.n : d.len, span = TS ? d.len : d.n;
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    double rbar = 0.0, fbar[K], b[K];
#pragma unroll
    for (int j = 0; j < K; j++) { fbar[j] = 0.0; b[j] = 0.0; }
    if (P >= RG_P2) {
        rbar = un.mean[u];
#pragma unroll
        for (int j = 0; j < K; j++) fbar[j] = un.mean[(int64_t)(j + 1) * units + u];
    }
    if (P == RG_P3) {
#pragma unroll
        for (int j = 0; j < K; j++) b[j] = un.b[(int64_t)j * units + u];
    }
    double acc[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) acc[q] = 0.0;
    int cnt = 0;
    const int64_t i_lo = (int64_t)blockIdx.y * XS_BLOCK, i_hi = i_lo + XS_BLOCK < span ? i_lo + XS_BLOCK : span;
    constexpr int B = xo_ahead(K + 1);
    for (int64_t i0 = i_lo; i0 < i_hi; i0 += B) {
        double rv[B], fv[B][K];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t i = i0 + k < i_hi ? i0 + k : i_hi - 1;
            const int64_t s = TS ? u : i, t = TS ? i : u, o = s * d.stride + t;
            rv[k] = in.r[o];
#pragma unroll
            for (int j = 0; j < K; j++) fv[k][j] = (TS && ((in.series >> j) & 1u)) ? in.f[j][t] : in.f[j][o];
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (i0 + k >= i_hi) break;
            bool mem = xs_valid(rv[k]);
#pragma unroll
            for (int j = 0; j < K; j++) mem = mem && xs_valid(fv[k][j]);
            if (!mem) continue;
            cnt += 1;
            if (P == RG_P1) {
                acc[0] += rv[k];
#pragma unroll
                for (int j = 0; j < K; j++) acc[1 + j] += fv[k][j];
                continue;
            }
            const double dr = rv[k] - rbar;
            double df[K];
#pragma unroll
            for (int j = 0; j < K; j++) df[j] = fv[k][j] - fbar[j];
            if (P == RG_P2) {
#pragma unroll
                for (int j = 0; j < K; j++)
#pragma unroll
                    for (int l = 0; l <= j; l++) acc[j * (j + 1) / 2 + l] += df[j] * df[l];
#pragma unroll
                for (int j = 0; j < K; j++) acc[K * (K + 1) / 2 + j] += df[j] * dr;
                acc[NA - 1] += dr * dr;
                continue;
            }
            double fit = 0.0;
#pragma unroll
            for (int j = 0; j < K; j++) fit += b[j] * df[j];
            const double e = dr - fit;
            acc[0] += e * e;
        }
    }
#pragma unroll
    for (int q = 0; q < NA; q++) ps[((int64_t)blockIdx.y * NA + q) * units + u] = acc[q];
    if (P == RG_P1) pcnt[(int64_t)blockIdx.y * units + u] = cnt;
}

// after pass 2: the combined triangle goes through xo_fit, which leaves b, the intercept, diag(C^-1) and 1/n + fbar^T C^-1 fbar in the
// unit's rows
template <int K>
__global__ __launch_bounds__(64) void rg_solve_kernel(const double *ps, int64_t nblk, int64_t units, RgUnit un) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    constexpr int NA = RgNa<K>::P2;
    double s[NA];
    xo_combine<NA>(ps, nblk, units, u, s);
    un.srr[u] = s[NA - 1];
    un.ok[u] = xo_fit<K>(s, un.n[u], un.mean + units + u, un.mean + u, un.b + u, un.v + u, units) ? 1 : 0;
}

// after pass 3: s^2 = SSE / (n - K - 1), se_j = sqrt(s^2 V_jj), t_j = b_j / se_j, p on n - K - 1, R^2 = 1 - SSE / Srr.
// Outputs [K + 1][units] (cross-sectional) or [units][K + 1] (time-series, TS).
template <int K, bool TS>
__global__ __launch_bounds__(64) void rg_final_kernel(const double *ps, int64_t nblk, int64_t units, RgUnit un, double *coef,
                                                      double *tst, double *pv, double *r2, int32_t *n_obs) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= units) return;
    double sse[1];
    xo_combine<1>(ps, nblk, units, u, sse);
    const int32_t n = un.n[u];
    n_obs[u] = n;
    const bool ok = un.ok[u] != 0;
    const double df = (double)(n - K - 1), s2 = sse[0] / df, srr = ok ? un.srr[u] : 0.0;
    r2[u] = rg_r2(ok, sse[0], srr);
#pragma unroll
    for (int j = 0; j <= K; j++) {
        const int64_t o = TS ? u * (K + 1) + j : (int64_t)j * units + u, w = (int64_t)j * units + u;
        rg_coef_stats(ok, un.b + w, un.v + w, s2, df, coef + o, tst + o, pv + o);
    }
}

// t = r sqrt((n - 2) / (1 - r r)), p on n - 2; NULL where r is NaN, n < 3 or 1 - r r == 0
__global__ __launch_bounds__(256) void rg_corr_t_kernel(const double *corr, const int32_t *n_valid, int64_t len, double *tst, double *pv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const double r = corr[i];
    const int32_t n = n_valid[i];
    const double den = 1.0 - r * r;
    if (r != r || n < 3 || den == 0.0) { tst[i] = pq_null(); pv[i] = pq_null(); return; }
    const double df = (double)(n - 2), t = r * sqrt(df / den);
    tst[i] = t;
    pv[i] = rg_t_pvalue(t, df);
}

struct RgOut {
    double *coef, *tst, *pv, *r2;
    int32_t *n_obs;
    double *summary;
};

template <int K, bool TS>
pq_status rg_run(pq_ctx *ctx, const RgIn &in, const RgOut &out) {
    const Dims d = in.d;
    const int64_t units = TS ? d.n : d.len, span = TS ? d.len : d.n;
    const int64_t nblk = xs_nblk(span);
    XoWs w;
    PQ_TRY(xo_workspace(ctx, "factor regression", units, nblk, K + 1, 3 * (K + 1) + 1, RgNa<K>::P2, &w));   // own rows: b, v [K + 1] and srr
    const RgUnit un{w.n, w.flag, w.mean, w.own, w.own + (K + 1) * w.row, w.own + 2 * (K + 1) * w.row};
    double *ps = w.ps;
    int32_t *pc = w.pcnt;
    const dim3 gp((unsigned)((units + 63) / 64), (unsigned)nblk), gu((unsigned)((units + 63) / 64));
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL((rg_pass_kernel<K, RG_P1, TS>), gp, dim3(64), 0, st, in, un, ps, pc);
    hipLaunchKernelGGL(xo_means_kernel<K + 1>, gu, dim3(64), 0, st, (const double *)ps, (const int32_t *)pc, nblk, units, un.n, un.mean);
    hipLaunchKernelGGL((rg_pass_kernel<K, RG_P2, TS>), gp, dim3(64), 0, st, in, un, ps, pc);
    hipLaunchKernelGGL(rg_solve_kernel<K>, gu, dim3(64), 0, st, (const double *)ps, nblk, units, un);
    hipLaunchKernelGGL((rg_pass_kernel<K, RG_P3, TS>), gp, dim3(64), 0, st, in, un, ps, pc);
    hipLaunchKernelGGL((rg_final_kernel<K, TS>), gu, dim3(64), 0, st, (const double *)ps, nblk, units, un, out.coef, out.tst, out.pv,
                       out.r2, out.n_obs);
    if (!TS && out.summary)
        hipLaunchKernelGGL(rg_summary_kernel, dim3(K + 1), dim3(64), 0, st, (const double *)out.coef, units, out.summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

template <bool TS>
pq_status rg_dispatch(pq_ctx *ctx, int k, const RgIn &in, const RgOut &out) {
    return xo_with_k<XO_MAX_K>(k, [&](auto K) { return rg_run<decltype(K)::value, TS>(ctx, in, out); });
}

pq_status rg_args(pq_ctx *ctx, const pq_batch *b, const char *what, const double *const *factors, int32_t k, const double *ret, RgIn &in) {
    PQ_TRY(pq_check(ctx, b));
    if (k < 1 || k > XO_MAX_K) { pq_set_error("%s: k must be in [1, 8]", what); return PQ_ERR_ARG; }
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", what); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", what); return PQ_ERR_UNSUPPORTED; }
    const bool empty = b->n_series == 0 || b->len == 0;
    if (!empty && (!factors || !ret)) { pq_set_error("%s: null pointer", what); return PQ_ERR_ARG; }
    in = RgIn{};
    in.r = ret;
    in.d = dims_of(b);
    for (int j = 0; j < k && !empty; j++) {
        if (!factors[j]) { pq_set_error("%s: null factor pointer", what); return PQ_ERR_ARG; }
        in.f[j] = factors[j];
    }
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_xsec_regress(pq_ctx *ctx, const pq_batch *b, const double *const *factors, int32_t k, const double *fwd_return, double *coef,
                          double *t_stat, double *p_value, double *r2, int32_t *n_obs, double *summary) {
    RgIn in;
    PQ_TRY(rg_args(ctx, b, "pq_xsec_regress", factors, k, fwd_return, in));
    PQ_REQUIRE(b->len == 0 || (coef && t_stat && p_value && r2 && n_obs), "pq_xsec_regress: null output pointer");
    if (b->len == 0) return PQ_OK;
    return rg_dispatch<false>(ctx, k, in, RgOut{coef, t_stat, p_value, r2, n_obs, summary});
}

pq_status pq_ts_regress(pq_ctx *ctx, const pq_batch *b, const double *const *factors, int32_t k, uint32_t series_mask, const double *ret,
                        double *coef, double *t_stat, double *p_value, double *r2, int32_t *n_obs) {
    RgIn in;
    PQ_TRY(rg_args(ctx, b, "pq_ts_regress", factors, k, ret, in));
    PQ_REQUIRE((series_mask >> k) == 0, "pq_ts_regress: series_mask names a factor beyond k");
    PQ_REQUIRE(b->n_series == 0 || (coef && t_stat && p_value && r2 && n_obs), "pq_ts_regress: null output pointer");
    if (b->n_series == 0) return PQ_OK;
    in.series = series_mask;
    return rg_dispatch<true>(ctx, k, in, RgOut{coef, t_stat, p_value, r2, n_obs, nullptr});
}

pq_status pq_corr_t_test(pq_ctx *ctx, const double *corr, const int32_t *n_valid, int64_t len, double *t_stat, double *p_value) {
    PQ_REQUIRE(ctx, "pq_corr_t_test: null context");
    PQ_REQUIRE(len >= 0, "pq_corr_t_test: negative length");
    PQ_REQUIRE(len == 0 || (corr && n_valid && t_stat && p_value), "pq_corr_t_test: null pointer");
    if (ctx->rec) { pq_set_error("pq_corr_t_test cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    if (len == 0) return PQ_OK;
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rg_corr_t_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, corr, n_valid, len, t_stat, p_value);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
