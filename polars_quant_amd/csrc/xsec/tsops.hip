// xsec/tsops.hip -- the time-series operators that formulaic alphas are written in, along the days of every symbol: ts_sum / ts_std /
// ts_zscore / ts_min / ts_max / ts_argmin / ts_argmax / ts_rank / decay_linear / delay / delta on one column and ts_cov / ts_corr on two
// (Factor.ts_* / decay_linear / delay / delta; beyond the README => decision D-29).
//
// Columns are symbol-major [n_series][stride]; everything runs along one symbol's days and nothing crosses symbols.  The sample rule is
// rolling.hip's (D-21): a row is NULL unless every value of its window (of both columns for the pair ops) is non-null and finite, and
// so is a result that comes out NaN.  win[0 .. w) is the row's window, oldest to newest; every sum starts at 0.0 and adds it in
// ascending order.
//  windowed ops: xsec_window.h's walk on the column itself, in rl_window_kernel's static LDS.  The ordering ops (min, max, arg*, rank) are
//               the same O(w) direct scan with a compare in place of the add: no deque, no sorted structure.
//  pair ops:     two value arrays and one last[] (an entry is unusable if either column's is) in dynamic LDS sized by the window:
//               20 (255 + w) bytes, 25 580 at w = 1024.
//  delay, delta: two loads per row, no LDS (the shape of rl_momentum_kernel).
#include "xsec_window.h"

namespace {

enum TsOp { TS_SUM = 0, TS_STD = 1, TS_ZSCORE = 2, TS_MIN = 3, TS_MAX = 4, TS_ARGMIN = 5, TS_ARGMAX = 6, TS_RANK = 7, TS_DECAY = 8,
            TS_DELAY = 9, TS_DELTA = 10 };
enum TsPairOp { TSP_COV = 0, TSP_CORR = 1 };

// the result of one row from its window win[0 .. w), all usable; pct is rank's mode 1
template <int OP> __device__ __forceinline__ double ts_row(const double *win, int w, bool pct) {
    const double dw = (double)w;
    if (OP == TS_SUM) {
        return xw_sum(win, w);
    } else if (OP == TS_STD || OP == TS_ZSCORE) {
        const auto [mean, q2] = xw_mean_q2(win, w);
        const double sd = sqrt(q2 / (double)(w - 1));
        if (OP == TS_STD) return sd;
        return q2 != 0.0 ? (win[w - 1] - mean) / sd : pq_null();
    } else if (OP == TS_MIN || OP == TS_MAX || OP == TS_ARGMIN || OP == TS_ARGMAX) {
        double m = win[0];
        int at = 0;
        for (int k = 1; k < w; k++) {                           // strict compares: the oldest of equal extremes stays, -0 ties with +0
            const double v = win[k];
            const bool better = (OP == TS_MIN || OP == TS_ARGMIN) ? v < m : v > m;
            m = better ? v : m;
            at = better ? k : at;
        }
        return (OP == TS_MIN || OP == TS_MAX) ? m : (double)at;
    } else if (OP == TS_RANK) {
        const double x = win[w - 1];
        int less = 0, equal = 0;                                // equal counts the row's own day
        for (int k = 0; k < w; k++) {
            const double v = win[k];
            less += v < x;
            equal += v == x;
        }
        const double r = (double)(2 * less + equal + 1) * 0.5;
        return pct ? r / dw : r;
    } else {
        double acc = 0.0;
        for (int k = 0; k < w; k++) acc += (double)(k + 1) * win[k];
        return acc / (double)(w * (w + 1) / 2);
    }
}

template <int OP>
__global__ __launch_bounds__(XW_TILE) void ts_window_kernel(const double *x, Dims d, int w, int pct, int64_t chunks, int64_t total,
                                                            double *out) {
    __shared__ double val[XW_STAGE];
    __shared__ int last[XW_STAGE];          // index of the last unusable entry <= l, -1 without one
    __shared__ int wave_last[XW_TILE / 64];
    xw_walk<1>(val, last, wave_last, d, w, chunks, total,
        [&](int64_t s, int64_t g, double *v) {
            const bool inside = g >= 0 && g < d.len;
            v[0] = inside ? x[s * d.stride + g] : 0.0;
            return inside && xs_valid(v[0]);
        },
        [&](int64_t s, int64_t t, const double *win, int, bool usable) {
            double r = pq_null();
            if (usable) {
                r = ts_row<OP>(win, w, pct != 0);
                if (r != r) r = pq_null();
            }
            out[s * d.stride + t] = r;
        });
}

// the two-column ops.  Dynamic LDS: vx[M], vy[M], last[M]
template <int OP>
__global__ __launch_bounds__(XW_TILE) void ts_pair_kernel(const double *x, const double *y, Dims d, int w, int64_t chunks, int64_t total,
                                                          double *out) {
    extern __shared__ double ts_lds[];
    __shared__ int wave_last[XW_TILE / 64];
    int *last = (int *)(ts_lds + 2 * (size_t)(XW_TILE + w - 1));   // index of the last unusable entry <= l, -1 without one
    xw_walk<2>(ts_lds, last, wave_last, d, w, chunks, total,
        [&](int64_t s, int64_t g, double *v) {
            const bool inside = g >= 0 && g < d.len;
            v[0] = inside ? x[s * d.stride + g] : 0.0;
            v[1] = inside ? y[s * d.stride + g] : 0.0;
            return inside && xs_valid(v[0]) && xs_valid(v[1]);
        },
        [&](int64_t s, int64_t t, const double *wx, int M, bool usable) {
            const double *wy = wx + M;
            const double dw = (double)w;
            double r = pq_null();
            if (usable) {
                double sx = 0.0, sy = 0.0;
                for (int k = 0; k < w; k++) {
                    sx += wx[k];
                    sy += wy[k];
                }
                const double mx = sx / dw, my = sy / dw;
                double sxy = 0.0, sxx = 0.0, syy = 0.0;
                for (int k = 0; k < w; k++) {
                    const double dx = wx[k] - mx, dy = wy[k] - my;
                    sxy += dx * dy;
                    sxx += dx * dx;
                    syy += dy * dy;
                }
                if (OP == TSP_COV) r = sxy / (double)(w - 1);
                else if (sxx != 0.0 && syy != 0.0) r = sxy / (sqrt(sxx) * sqrt(syy));
                if (r != r) r = pq_null();
            }
            out[s * d.stride + t] = r;
        });
}

// delay: x[t - w]; delta: x[t] - x[t - w]
template <int OP>
__global__ __launch_bounds__(XW_TILE) void ts_lag_kernel(const double *x, Dims d, int64_t w, int64_t chunks, int64_t total, double *out) {
    xw_rows(d, chunks, total, [&](int64_t s, int64_t t) {
        const double *row = x + s * d.stride;
        double r = pq_null();
        if (t >= w) {
            const double b = row[t - w];
            if (OP == TS_DELAY) {
                if (b == b) r = b;                              // NULL is a NaN: it stays NULL; +-inf passes
            } else {
                const double a = row[t];
                if (xs_valid(a) && xs_valid(b)) {
                    r = a - b;
                    if (r != r) r = pq_null();
                }
            }
        }
        out[s * d.stride + t] = r;
    });
}

constexpr char TS_RAGGED[] = "pq_factor_ts / pq_factor_ts_pair (the column of a factor is [n_series][stride]): ragged batches are not supported";

} // namespace

extern "C" {

pq_status pq_factor_ts(pq_ctx *ctx, const pq_batch *b, const double *x, int32_t op, int64_t window, int32_t mode, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op >= TS_SUM && op <= TS_DELTA,
               "pq_factor_ts: op must be 0 (sum), 1 (std), 2 (zscore), 3 (min), 4 (max), 5 (argmin), 6 (argmax), 7 (rank), 8 (decay_linear), "
               "9 (delay) or 10 (delta)");
    PQ_REQUIRE(window >= 1 && window <= XW_MAX_W, "pq_factor_ts: window must be in [1, 1024]");
    PQ_REQUIRE((op != TS_STD && op != TS_ZSCORE) || window >= 2, "pq_factor_ts: std and zscore need window >= 2");
    PQ_REQUIRE(mode == 0 || (mode == 1 && op == TS_RANK), "pq_factor_ts: mode must be 0, or 1 (rank / window) for rank alone");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && out), "pq_factor_ts: null pointer");
    XwGrid g;
    PQ_TRY(xw_prepare(ctx, b, "pq_factor_ts cannot be recorded into a suite", TS_RAGGED, PQ_ERR_UNSUPPORTED, &g));
    if (g.total == 0) return PQ_OK;
    const Dims d = g.d;
    const XwSpan in = xw_span(x, xw_plane_bytes(d)), o = xw_span(out, xw_plane_bytes(d));
    PQ_TRY(xw_no_overlap(&o, 1, &in, 1, "pq_factor_ts: out must not overlap x", nullptr));
    const dim3 block(XW_TILE);
    hipStream_t st = ctx->stream;
    const int w = (int)window, pct = mode;
#define TS_WINDOWED(OP) \
    case OP: hipLaunchKernelGGL(ts_window_kernel<OP>, g.grid, block, 0, st, x, d, w, pct, g.chunks, g.total, out); break
    switch (op) {
    TS_WINDOWED(TS_SUM);
    TS_WINDOWED(TS_STD);
    TS_WINDOWED(TS_ZSCORE);
    TS_WINDOWED(TS_MIN);
    TS_WINDOWED(TS_MAX);
    TS_WINDOWED(TS_ARGMIN);
    TS_WINDOWED(TS_ARGMAX);
    TS_WINDOWED(TS_RANK);
    TS_WINDOWED(TS_DECAY);
    case TS_DELAY: hipLaunchKernelGGL(ts_lag_kernel<TS_DELAY>, g.grid, block, 0, st, x, d, window, g.chunks, g.total, out); break;
    default: hipLaunchKernelGGL(ts_lag_kernel<TS_DELTA>, g.grid, block, 0, st, x, d, window, g.chunks, g.total, out); break;
    }
#undef TS_WINDOWED
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_factor_ts_pair(pq_ctx *ctx, const pq_batch *b, const double *x, const double *y, int32_t op, int64_t window, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op == TSP_COV || op == TSP_CORR, "pq_factor_ts_pair: op must be 0 (cov) or 1 (corr)");
    PQ_REQUIRE(window >= 2 && window <= XW_MAX_W, "pq_factor_ts_pair: window must be in [2, 1024]");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && y && out), "pq_factor_ts_pair: null pointer");
    XwGrid g;
    PQ_TRY(xw_prepare(ctx, b, "pq_factor_ts_pair cannot be recorded into a suite", TS_RAGGED, PQ_ERR_UNSUPPORTED, &g));
    if (g.total == 0) return PQ_OK;
    const Dims d = g.d;
    const XwSpan ins[] = {xw_span(x, xw_plane_bytes(d)), xw_span(y, xw_plane_bytes(d))}, o = xw_span(out, xw_plane_bytes(d));
    PQ_TRY(xw_no_overlap(&o, 1, ins, 2, "pq_factor_ts_pair: out must not overlap x or y", nullptr));
    const dim3 block(XW_TILE);
    const int w = (int)window;
    const size_t M = (size_t)(XW_TILE + w - 1), lds = 2 * M * 8 + M * 4;
    if (op == TSP_COV) hipLaunchKernelGGL(ts_pair_kernel<TSP_COV>, g.grid, block, lds, ctx->stream, x, y, d, w, g.chunks, g.total, out);
    else hipLaunchKernelGGL(ts_pair_kernel<TSP_CORR>, g.grid, block, lds, ctx->stream, x, y, d, w, g.chunks, g.total, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
