// xsec/rolling.hip -- the README's common technical factors: rolling mean, momentum, volatility, skewness and relative strength along
// the days of every symbol (Factor.moving_average / momentum / volatility / skewness / relative_strength; README.md:1423-1426,
// :1472-1477; README-only => decision D-21).
//
// The column is symbol-major [n_series][stride]; everything runs along one symbol's days and nothing crosses symbols.  A row whose
// sample is incomplete is NULL, so is a result that comes out NaN.
//  windowed ops (mean, volatility, skewness, relative strength): one workgroup of 256 threads per (symbol, tile of 256 days), walked
//               with a grid stride.  The workgroup stages the tile and a halo of window - 1 earlier entries in LDS, loads coalesced along
//               days: the column itself for the mean, else the derived series, written once (r[j] = (x[j] - x[j-1]) / x[j-1] or
//               d[j] = x[j] - x[j-1]: one division per element, not one per window).  Beside every entry goes the index of the last
//               unusable entry at or before it (a max-scan over the staged stretch: every thread scans a short run, the runs are joined
//               by a wave scan), so "is the whole window usable" is one compare.  Each thread then evaluates its own row's window
//               directly, in ascending order from 0.0, out of LDS: consecutive threads read consecutive 8-byte words at every step (no
//               bank conflict), and the order of the additions is the definition's, which a sliding sum would not keep.  The tile
//               constant, the job split, the scan (xw_last_scan), the launch shape and the overlap check are xsec_window.h's, which
//               rolling_regress.hip (D-28) shares.
//  momentum:    two loads per row, no LDS.
#include "xsec_window.h"

namespace {

constexpr int RL_TILE = XW_TILE;                                // days per workgroup = threads per workgroup
constexpr int RL_MAX_W = PQ_FACTOR_ROLLING_MAX_WINDOW;
constexpr int RL_STAGE = RL_TILE + RL_MAX_W - 1;                // staged entries at the widest window: 10 KiB of f64 + 5 KiB of i32

enum RlOp { RL_MEAN = 0, RL_MOM = 1, RL_VOL = 2, RL_SKEW = 3, RL_RS = 4 };

// one workgroup per (symbol, tile of RL_TILE days); entry l of the staged stretch is day g0 + l, row t0 + i is entry i + w - 1 and its
// window is entries [i, i + w)
template <int OP>
__global__ __launch_bounds__(RL_TILE) void rl_window_kernel(const double *x, Dims d, int w, int64_t chunks, int64_t total, double *out) {
    __shared__ double val[RL_STAGE];
    __shared__ int last[RL_STAGE];          // index of the last unusable entry <= l, -1 without one
    __shared__ int wave_last[RL_TILE / 64];
    const int tid = threadIdx.x, M = RL_TILE + w - 1;
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, w);
        const double *row = x + s * d.stride;
        for (int l = tid; l < M; l += RL_TILE) {
            const int64_t g = g0 + l;
            double v = 0.0;
            bool ok = false;
            if (OP == RL_MEAN) {
                if (g >= 0 && g < d.len) { v = row[g]; ok = xs_valid(v); }
            } else if (g >= 1 && g < d.len) {
                const double p = row[g - 1], c = row[g];
                if (xs_valid(p) && xs_valid(c)) {
                    if (OP == RL_RS) { v = c - p; ok = true; }
                    else { v = (c - p) / p; ok = isfinite(v); }
                }
            }
            val[l] = v;
            last[l] = ok ? -1 : l;
        }
        xw_last_scan(last, M, wave_last);
        const int64_t t = t0 + tid;
        if (t < d.len) {
            const int e = tid + w - 1;
            const double *win = val + tid;
            const double dw = (double)w;
            double r = pq_null();
            if (e - last[e] >= w) {
                if (OP == RL_MEAN) {
                    double sum = 0.0;
                    for (int k = 0; k < w; k++) sum += win[k];
                    r = sum / dw;
                } else if (OP == RL_RS) {
                    double G = 0.0, L = 0.0;
                    for (int k = 0; k < w; k++) {
                        const double dv = win[k];
                        G += dv > 0.0 ? dv : 0.0;               // a +0.0 term leaves a sum that started at +0.0 unchanged
                        L += dv < 0.0 ? -dv : 0.0;
                    }
                    const double den = G + L;
                    if (den != 0.0) r = (100.0 * G) / den;
                } else {
                    double sum = 0.0;
                    for (int k = 0; k < w; k++) sum += win[k];
                    const double mean = sum / dw;
                    if (OP == RL_VOL) {
                        double q2 = 0.0;
                        for (int k = 0; k < w; k++) {
                            const double dv = win[k] - mean;
                            q2 += dv * dv;
                        }
                        r = sqrt(q2 / (double)(w - 1));
                    } else {
                        double q2 = 0.0, q3 = 0.0;
                        for (int k = 0; k < w; k++) {
                            const double dv = win[k] - mean, sq = dv * dv;
                            q2 += sq;
                            q3 += sq * dv;
                        }
                        const double m2 = q2 / dw, m3 = q3 / dw;
                        if (m2 != 0.0) r = m3 / (m2 * sqrt(m2));
                    }
                }
                if (r != r) r = pq_null();
            }
            out[s * d.stride + t] = r;
        }
        __syncthreads();                                        // the next tile restages val / last
    }
}

// (a - b) / b with a = x[t - skip], b = x[t - skip - w]: one workgroup per (symbol, RL_TILE days), walked with a grid stride
__global__ __launch_bounds__(RL_TILE) void rl_momentum_kernel(const double *x, Dims d, int64_t w, int64_t skip, int64_t chunks, int64_t total,
                                                              double *out) {
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, 1);        // nothing is staged: no halo
        const int64_t t = t0 + threadIdx.x;
        if (t >= d.len) continue;
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
    }
}

} // namespace

extern "C" {

pq_status pq_factor_rolling(pq_ctx *ctx, const pq_batch *b, const double *x, int32_t op, int64_t window, int64_t skip, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op >= RL_MEAN && op <= RL_RS,
               "pq_factor_rolling: op must be 0 (mean), 1 (momentum), 2 (volatility), 3 (skewness) or 4 (relative strength)");
    PQ_REQUIRE(window >= 1 && window <= RL_MAX_W, "pq_factor_rolling: window must be in [1, 1024]");
    PQ_REQUIRE(op != RL_VOL || window >= 2, "pq_factor_rolling: volatility needs window >= 2");
    PQ_REQUIRE(op != RL_SKEW || window >= 3, "pq_factor_rolling: skewness needs window >= 3");
    PQ_REQUIRE(skip >= 0, "pq_factor_rolling: skip must be >= 0");
    PQ_REQUIRE(op == RL_MOM || skip == 0, "pq_factor_rolling: skip is momentum's alone, it must be 0 for the other ops");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && out), "pq_factor_rolling: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_rolling cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_rolling (the column of a factor is [n_series][stride])");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    // a workgroup reads a halo of days that another workgroup writes: the two [n_series][stride] columns must be disjoint
    const uintptr_t bytes = (uintptr_t)d.n * (uintptr_t)d.stride * 8;
    PQ_REQUIRE(xw_disjoint(xw_span(x, bytes), xw_span(out, bytes)), "pq_factor_rolling: out must not overlap x");
    const XwGrid g = xw_grid(d);
    const dim3 block(RL_TILE);
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
