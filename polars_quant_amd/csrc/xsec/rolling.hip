// xsec/rolling.hip -- the README's common technical factors: rolling mean, momentum, volatility, skewness and relative strength along
// the days of every symbol (Factor.moving_average / momentum / volatility / skewness / relative_strength; README.md:1423-1426,
// :1472-1477; README-only => decision D-21).
//
// The column is symbol-major [n_series][stride]; everything runs along one symbol's days and nothing crosses symbols.  A row whose
// sample is incomplete is NULL, so is a result that comes out NaN.
//  windowed ops (mean, volatility, skewness, relative strength): xsec_window.h's walk.  Staged is the column itself for the mean, else
//               the derived series, written once (r[j] = (x[j] - x[j-1]) / x[j-1] or d[j] = x[j] - x[j-1]: one division per element,
//               not one per window).
//  momentum:    two loads per row, no LDS.
#include "xsec_window.h"

namespace {

enum RlOp { RL_MEAN = 0, RL_MOM = 1, RL_VOL = 2, RL_SKEW = 3, RL_RS = 4 };

template <int OP>
__global__ __launch_bounds__(XW_TILE) void rl_window_kernel(const double *x, Dims d, int w, int64_t chunks, int64_t total, double *out) {
    __shared__ double val[XW_STAGE];
    __shared__ int last[XW_STAGE];          // index of the last unusable entry <= l, -1 without one
    __shared__ int wave_last[XW_TILE / 64];
    xw_walk<1>(val, last, wave_last, d, w, chunks, total,
        [&](int64_t s, int64_t g, double *v) {
            const double *row = x + s * d.stride;
            bool ok = false;
            v[0] = 0.0;
            if (OP == RL_MEAN) {
                if (g >= 0 && g < d.len) { v[0] = row[g]; ok = xs_valid(v[0]); }
            } else if (g >= 1 && g < d.len) {
                const double p = row[g - 1], c = row[g];
                if (OP == RL_RS) {                              // & : one 16-byte load of both days in front of both tests
                    if (xs_valid(p) & xs_valid(c)) { v[0] = c - p; ok = true; }
                } else if (xs_valid(p) && xs_valid(c)) {
                    v[0] = (c - p) / p;
                    ok = isfinite(v[0]);
                }
            }
            return ok;
        },
        [&](int64_t s, int64_t t, const double *win, int, bool usable) {
            const double dw = (double)w;
            double r = pq_null();
            if (usable) {
                if (OP == RL_MEAN) {
                    r = xw_sum(win, w) / dw;
                } else if (OP == RL_RS) {
                    double G = 0.0, L = 0.0;
                    for (int k = 0; k < w; k++) {
                        const double dv = win[k];
                        G += dv > 0.0 ? dv : 0.0;               // a +0.0 term leaves a sum that started at +0.0 unchanged
                        L += dv < 0.0 ? -dv : 0.0;
                    }
                    const double den = G + L;
                    if (den != 0.0) r = (100.0 * G) / den;
                } else if (OP == RL_VOL) {
                    r = sqrt(xw_mean_q2(win, w).q2 / (double)(w - 1));
                } else {
                    const double mean = xw_mean(win, w);
                    double q2 = 0.0, q3 = 0.0;
                    for (int k = 0; k < w; k++) {
                        const double dv = win[k] - mean, sq = dv * dv;
                        q2 += sq;
                        q3 += sq * dv;
                    }
                    const double m2 = q2 / dw, m3 = q3 / dw;
                    if (m2 != 0.0) r = m3 / (m2 * sqrt(m2));
                }
                if (r != r) r = pq_null();
            }
            out[s * d.stride + t] = r;
        });
}

// (a - b) / b with a = x[t - skip], b = x[t - skip - w]
__global__ __launch_bounds__(XW_TILE) void rl_momentum_kernel(const double *x, Dims d, int64_t w, int64_t skip, int64_t chunks, int64_t total,
                                                              double *out) {
    xw_rows(d, chunks, total, [&](int64_t s, int64_t t) {
        const double *row = x + s * d.stride;
        const int64_t ia = t - skip, ib = ia - w;
        double r = pq_null();
        if (ib >= 0) {
            const double a = row[ia], b = row[ib];
            if (xs_valid(a) && xs_valid(b)) {
                r = (a - b) / b;
                if (r != r) r = pq_null();
            }
        }
        out[s * d.stride + t] = r;
    });
}

} // namespace

extern "C" {

pq_status pq_factor_rolling(pq_ctx *ctx, const pq_batch *b, const double *x, int32_t op, int64_t window, int64_t skip, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op >= RL_MEAN && op <= RL_RS,
               "pq_factor_rolling: op must be 0 (mean), 1 (momentum), 2 (volatility), 3 (skewness) or 4 (relative strength)");
    PQ_REQUIRE(window >= 1 && window <= XW_MAX_W, "pq_factor_rolling: window must be in [1, 1024]");
    PQ_REQUIRE(op != RL_VOL || window >= 2, "pq_factor_rolling: volatility needs window >= 2");
    PQ_REQUIRE(op != RL_SKEW || window >= 3, "pq_factor_rolling: skewness needs window >= 3");
    PQ_REQUIRE(skip >= 0, "pq_factor_rolling: skip must be >= 0");
    PQ_REQUIRE(op == RL_MOM || skip == 0, "pq_factor_rolling: skip is momentum's alone, it must be 0 for the other ops");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && out), "pq_factor_rolling: null pointer");
    XwGrid g;
    PQ_TRY(xw_prepare(ctx, b, "pq_factor_rolling cannot be recorded into a suite",
                      "pq_factor_rolling (the column of a factor is [n_series][stride]): ragged batches are not supported", PQ_ERR_UNSUPPORTED, &g));
    if (g.total == 0) return PQ_OK;
    const Dims d = g.d;
    const XwSpan in = xw_span(x, xw_plane_bytes(d)), o = xw_span(out, xw_plane_bytes(d));
    PQ_TRY(xw_no_overlap(&o, 1, &in, 1, "pq_factor_rolling: out must not overlap x", nullptr));
    const dim3 block(XW_TILE);
    hipStream_t st = ctx->stream;
    const int w = (int)window;
    if (skip > d.len) skip = d.len;                             // every row is NULL from skip + window >= len on
    switch (op) {
    case RL_MEAN: hipLaunchKernelGGL(rl_window_kernel<RL_MEAN>, g.grid, block, 0, st, x, d, w, g.chunks, g.total, out); break;
    case RL_MOM: hipLaunchKernelGGL(rl_momentum_kernel, g.grid, block, 0, st, x, d, window, skip, g.chunks, g.total, out); break;
    case RL_VOL: hipLaunchKernelGGL(rl_window_kernel<RL_VOL>, g.grid, block, 0, st, x, d, w, g.chunks, g.total, out); break;
    case RL_SKEW: hipLaunchKernelGGL(rl_window_kernel<RL_SKEW>, g.grid, block, 0, st, x, d, w, g.chunks, g.total, out); break;
    default: hipLaunchKernelGGL(rl_window_kernel<RL_RS>, g.grid, block, 0, st, x, d, w, g.chunks, g.total, out); break;
    }
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
