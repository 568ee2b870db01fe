// xsec/rolling_regress.hip -- rolling-window OLS along the days of every symbol: rolling beta, alpha, residual volatility, R^2 and the
// last day's residual (Factor.rolling_regression / rolling_beta / idiosyncratic_volatility; the README computes one whole-history beta
// with `linear`, README.md:231; a factor needs one per (symbol, day) => decision D-28).
//
// Columns are symbol-major [n_series][stride]; a regressor flagged in series_mask is one [len] series shared by every symbol.  Model
// y = a + sum_j b_j x_j over the `window` days that end at the row, K = n_x regressors (1 .. 4).  The sample rule is rolling.hip's (D-21):
// a row has a result only if all K + 1 values are non-null and finite on every day of its window.  The arithmetic is D-17's
// (regress.hip, restated in tests/xsec_regress_ref.py) with n = window and every blocked sum replaced by a plain sum over the window in
// ascending day order from 0.0; the L D L^T core is xsec_ols.h's.  The row's solve is the first half of xo_fit (b and the intercept,
// no standard errors) written out here on xo_ldl / xo_forward / xo_back: through xo_fit the kernel compiled to other code and one
// timing left the parent's range (EXPERIMENTS.md, "One fit and one window stage for the regress / rolling kernels").
//  stage:   xsec_window.h's, on all K + 1 columns in dynamic LDS sized by the actual window ((K + 1)(255 + window) f64 and (255 + window)
//           i32: 6.3 KB at K = 1, window = 60; 56.3 KB at K = 4, window = 1024); one last[] marks an entry unusable if any column is.
//           The kernel keeps its own copy of xw_walk's loop, as it keeps its own solve: through xw_walk<K + 1> it compiled to 77 / 117 /
//           105 / 113 VGPRs against 77 / 91 / 125 / 134 (EXPERIMENTS.md, "One window walk for the rolling, ts and OLS kernels").
//  rows:    three passes over the window.  The kernel is templated on K: every index of the xo_* arrays is static and nothing goes to
//           scratch (rolling_regress.resources.txt).
#include "xsec_ols.h"
#include "xsec_window.h"

namespace {

constexpr int RR_MAX_K = PQ_ROLLING_REGRESS_MAX_K;

struct RrIn {
    const double *x[RR_MAX_K];
    const double *y;
    uint32_t series;       // bit j: x[j] is one [len] series shared by every symbol
    Dims d;
};

struct RrOut {             // each may be null: not written
    double *beta;          // [K][n][stride]
    double *alpha, *resid_std, *r2, *resid;
};

// xw_walk<K + 1>, written out (see above).  LDS: column c (0 .. K-1 the regressors, K = y) at val + c * M, then last[M].
template <int K>
__global__ __launch_bounds__(XW_TILE) void rr_window_kernel(RrIn in, RrOut out, int w, int64_t chunks, int64_t total) {
    extern __shared__ double rr_lds[];
    __shared__ int wave_last[XW_TILE / 64];
    constexpr int NV = K + 1, NA = xo_tri(NV);
    const Dims d = in.d;
    const int tid = threadIdx.x, M = XW_TILE + w - 1;
    double *val = rr_lds;
    int *last = (int *)(rr_lds + (size_t)NV * M);               // index of the last unusable entry <= l, -1 without one
    const int64_t plane = d.n * d.stride;
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, w);
        const double *col[NV];
#pragma unroll
        for (int c = 0; c < K; c++) col[c] = in.x[c] + (((in.series >> c) & 1u) ? 0 : s * d.stride);
        col[K] = in.y + s * d.stride;
        for (int l = tid; l < M; l += XW_TILE) {
            const int64_t g = g0 + l;
            const bool inside = g >= 0 && g < d.len;
            bool ok = inside;
#pragma unroll
            for (int c = 0; c < NV; c++) {
                const double v = inside ? col[c][g] : 0.0;
                ok = ok && xs_valid(v);
                val[c * M + l] = v;
            }
            last[l] = ok ? -1 : l;
        }
        xw_last_scan(last, M, wave_last);
        const int64_t t = t0 + tid;
        if (t < d.len) {
            const int e = tid + w - 1;
            const double *win = val + tid;                      // column c of the window: win[c * M + k], k = 0 .. w-1
            const double dw = (double)w;
            double b[K], alpha = pq_null(), rstd = pq_null(), r2 = pq_null(), res = pq_null();
#pragma unroll
            for (int j = 0; j < K; j++) b[j] = pq_null();
            if (e - last[e] >= w) {
                double mean[NV];
#pragma unroll
                for (int c = 0; c < NV; c++) mean[c] = 0.0;
#pragma unroll 4
                for (int k = 0; k < w; k++)
#pragma unroll
                    for (int c = 0; c < NV; c++) mean[c] += win[c * M + k];
#pragma unroll
                for (int c = 0; c < NV; c++) mean[c] = mean[c] / dw;
                // pass 2: the packed triangle of the K + 1 columns x_0 .. x_{K-1}, y (xsec_ols.h): C, then c and Syy in row K
                double sq[NA];
#pragma unroll
                for (int q = 0; q < NA; q++) sq[q] = 0.0;
#pragma unroll 4
                for (int k = 0; k < w; k++) {
                    double dv[NV];
#pragma unroll
                    for (int c = 0; c < NV; c++) dv[c] = win[c * M + k] - mean[c];
#pragma unroll
                    for (int j = 0; j < NV; j++)
#pragma unroll
                        for (int l = 0; l <= j; l++) sq[xo_tri(j) + l] += dv[j] * dv[l];
                }
                double L[K][K], D[K];
                if (xo_ldl<K>(sq, L, D) == K) {
                    double z[K], bb[K];
                    xo_forward<K>(L, sq + xo_tri(K), K, z);
                    xo_back<K>(L, D, z, K, bb);
                    double sa = 0.0;
#pragma unroll
                    for (int j = 0; j < K; j++) sa += bb[j] * mean[j];
                    const double a = mean[K] - sa;
                    double sse = 0.0, el = 0.0;
#pragma unroll 4
                    for (int k = 0; k < w; k++) {
                        double fit = 0.0;
#pragma unroll
                        for (int j = 0; j < K; j++) fit += bb[j] * (win[j * M + k] - mean[j]);
                        el = (win[K * M + k] - mean[K]) - fit;
                        sse += el * el;
                    }
                    const double syy = sq[NA - 1], sd = sqrt(sse / (double)(w - K - 1)), rr = 1.0 - sse / syy;
                    bool num = a == a && sd == sd && el == el && (syy == 0.0 || rr == rr);
#pragma unroll
                    for (int j = 0; j < K; j++) num = num && bb[j] == bb[j];
                    if (num) {                                  // a row with a NaN result has none at all
#pragma unroll
                        for (int j = 0; j < K; j++) b[j] = bb[j];
                        alpha = a; rstd = sd; res = el;
                        if (syy != 0.0) r2 = rr;
                    }
                }
            }
            const int64_t o = s * d.stride + t;
            if (out.beta) {
#pragma unroll
                for (int j = 0; j < K; j++) out.beta[j * plane + o] = b[j];
            }
            if (out.alpha) out.alpha[o] = alpha;
            if (out.resid_std) out.resid_std[o] = rstd;
            if (out.r2) out.r2[o] = r2;
            if (out.resid) out.resid[o] = res;
        }
        __syncthreads();                                        // the next tile restages val / last
    }
}

} // namespace

extern "C" {

pq_status pq_factor_rolling_regress(pq_ctx *ctx, const pq_batch *b, const double *const *x, int32_t n_x, uint32_t series_mask,
                                    const double *y, int64_t window, double *beta, double *alpha, double *resid_std, double *r_squared,
                                    double *resid) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(n_x >= 1 && n_x <= RR_MAX_K, "pq_factor_rolling_regress: n_x must be in [1, 4]");
    PQ_REQUIRE((series_mask >> n_x) == 0, "pq_factor_rolling_regress: series_mask names a regressor beyond n_x");
    PQ_REQUIRE(window >= n_x + 2 && window <= XW_MAX_W, "pq_factor_rolling_regress: window must be in [n_x + 2, 1024]");
    XwGrid g;
    PQ_TRY(xw_prepare(ctx, b, "pq_factor_rolling_regress cannot be recorded into a suite",
                      "pq_factor_rolling_regress: ragged batches are not supported (a column is [n_series][stride])", PQ_ERR_ARG, &g));
    if (g.total == 0) return PQ_OK;
    PQ_REQUIRE(x && y, "pq_factor_rolling_regress: null pointer");
    const Dims d = g.d;
    RrIn in{};
    in.y = y;
    in.series = series_mask;
    in.d = d;
    const uintptr_t plane = xw_plane_bytes(d), colb = plane - (uintptr_t)(d.stride - d.len) * 8;   // a column without its last padding
    XwSpan ins[RR_MAX_K + 1], outs[5];
    int n_in = 0, n_out = 0;
    ins[n_in++] = xw_span(y, colb);
    for (int j = 0; j < n_x; j++) {
        PQ_REQUIRE(x[j], "pq_factor_rolling_regress: null regressor pointer");
        in.x[j] = x[j];
        ins[n_in++] = xw_span(x[j], ((series_mask >> j) & 1u) ? (uintptr_t)d.len * 8 : colb);
    }
    if (beta) outs[n_out++] = xw_span(beta, (uintptr_t)(n_x - 1) * plane + colb);
    for (double *p : {alpha, resid_std, r_squared, resid})
        if (p) outs[n_out++] = xw_span(p, colb);
    PQ_TRY(xw_no_overlap(outs, n_out, ins, n_in, "pq_factor_rolling_regress: an output must not overlap an input",
                         "pq_factor_rolling_regress: two outputs must not overlap"));
    if (n_out == 0) return PQ_OK;
    const RrOut out{beta, alpha, resid_std, r_squared, resid};
    const int w = (int)window;
    const size_t M = (size_t)(XW_TILE + w - 1), lds = (size_t)(n_x + 1) * M * 8 + M * 4;
    xo_with_k<RR_MAX_K>(n_x, [&](auto K) {
        hipLaunchKernelGGL(rr_window_kernel<decltype(K)::value>, g.grid, dim3(XW_TILE), lds, ctx->stream, in, out, w, g.chunks, g.total);
    });
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
