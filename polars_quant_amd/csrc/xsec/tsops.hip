// xsec/tsops.hip -- the time-series operators that formulaic alphas are written in, along the days of every symbol: ts_sum / ts_std /
// ts_zscore / ts_min / ts_max / ts_argmin / ts_argmax / ts_rank / decay_linear / delay / delta on one column and ts_cov / ts_corr on two
// (Factor.ts_* / decay_linear / delay / delta; beyond the README => decision D-29).
//
// Columns are symbol-major [n_series][stride]; everything runs along one symbol's days and nothing crosses symbols.  The sample rule is
// rolling.hip's (D-21): a row is NULL unless every value of its window (of both columns for the pair ops) is non-null and finite, and
// so is a result that comes out NaN.  win[0 .. w) is the row's window, oldest to newest; every sum starts at 0.0 and adds it in
// ascending order.
//  windowed ops: the third user of xsec_window.h's stage, in the launch shape of rl_window_kernel: one workgroup of 256 threads per
//               (symbol, tile of 256 days), walked with a grid stride; the tile and a halo of window - 1 earlier days go into LDS with
//               loads coalesced along days, beside them last[] (xw_last_scan), so "is the whole window usable" is one compare.  Each
//               thread then evaluates its own row's window directly out of LDS: consecutive threads read consecutive 8-byte words at
//               every step (no bank conflict), and the order of the additions is the definition's.  The ordering ops (min, max, arg*,
//               rank) are the same O(w) direct scan with a compare in place of the add: no deque, no sorted structure.
//  pair ops:     two value arrays and one last[] (an entry is unusable if either column's is) in dynamic LDS sized by the window:
//               20 (255 + w) bytes, 25 580 at w = 1024.
//  delay, delta: two loads per row, no LDS (the shape of rl_momentum_kernel).
#include "xsec_window.h"

namespace {

constexpr int TS_TILE = XW_TILE;                                // days per workgroup = threads per workgroup
constexpr int TS_MAX_W = PQ_FACTOR_ROLLING_MAX_WINDOW;
constexpr int TS_STAGE = TS_TILE + TS_MAX_W - 1;                // staged entries at the widest window: 10 KiB of f64 + 5 KiB of i32

enum TsOp { TS_SUM = 0, TS_STD = 1, TS_ZSCORE = 2, TS_MIN = 3, TS_MAX = 4, TS_ARGMIN = 5, TS_ARGMAX = 6, TS_RANK = 7, TS_DECAY = 8,
            TS_DELAY = 9, TS_DELTA = 10 };
enum TsPairOp { TSP_COV = 0, TSP_CORR = 1 };

// the result of one row from its window win[0 .. w), all usable; pct is rank's mode 1
template <int OP> __device__ __forceinline__ double ts_row(const double *win, int w, bool pct) {
    const double dw = (double)w;
    if (OP == TS_SUM) {
        double sum = 0.0;
        for (int k = 0; k < w; k++) sum += win[k];
        return sum;
    } else if (OP == TS_STD || OP == TS_ZSCORE) {
        double sum = 0.0;
        for (int k = 0; k < w; k++) sum += win[k];
        const double mean = sum / dw;
        double q2 = 0.0;
        for (int k = 0; k < w; k++) {
            const double dv = win[k] - mean;
            q2 += dv * dv;
        }
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

// one workgroup per (symbol, tile of TS_TILE days); entry l of the staged stretch is day g0 + l, row t0 + i is entry i + w - 1 and its
// window is entries [i, i + w)
template <int OP>
__global__ __launch_bounds__(TS_TILE) void ts_window_kernel(const double *x, Dims d, int w, int pct, int64_t chunks, int64_t total,
                                                            double *out) {
    __shared__ double val[TS_STAGE];
    __shared__ int last[TS_STAGE];          // index of the last unusable entry <= l, -1 without one
    __shared__ int wave_last[TS_TILE / 64];
    const int tid = threadIdx.x, M = TS_TILE + w - 1;
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, w);
        const double *row = x + s * d.stride;
        for (int l = tid; l < M; l += TS_TILE) {
            const int64_t g = g0 + l;
            double v = 0.0;
            bool ok = false;
            if (g >= 0 && g < d.len) { v = row[g]; ok = xs_valid(v); }
            val[l] = v;
            last[l] = ok ? -1 : l;
        }
        xw_last_scan(last, M, wave_last);
        const int64_t t = t0 + tid;
        if (t < d.len) {
            const int e = tid + w - 1;
            double r = pq_null();
            if (e - last[e] >= w) {
                r = ts_row<OP>(val + tid, w, pct != 0);
                if (r != r) r = pq_null();
            }
            out[s * d.stride + t] = r;
        }
        __syncthreads();                                        // the next tile restages val / last
    }
}

// the two-column ops.  Dynamic LDS: vx[M], vy[M], last[M]
template <int OP>
__global__ __launch_bounds__(TS_TILE) void ts_pair_kernel(const double *x, const double *y, Dims d, int w, int64_t chunks, int64_t total,
                                                          double *out) {
    extern __shared__ double ts_lds[];
    __shared__ int wave_last[TS_TILE / 64];
    const int tid = threadIdx.x, M = TS_TILE + w - 1;
    double *vx = ts_lds, *vy = ts_lds + M;
    int *last = (int *)(ts_lds + 2 * (size_t)M);                // index of the last unusable entry <= l, -1 without one
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, w);
        const double *rx = x + s * d.stride, *ry = y + s * d.stride;
        for (int l = tid; l < M; l += TS_TILE) {
            const int64_t g = g0 + l;
            double a = 0.0, b = 0.0;
            bool ok = false;
            if (g >= 0 && g < d.len) { a = rx[g]; b = ry[g]; ok = xs_valid(a) && xs_valid(b); }
            vx[l] = a;
            vy[l] = b;
            last[l] = ok ? -1 : l;
        }
        xw_last_scan(last, M, wave_last);
        const int64_t t = t0 + tid;
        if (t < d.len) {
            const int e = tid + w - 1;
            const double *wx = vx + tid, *wy = vy + tid;
            const double dw = (double)w;
            double r = pq_null();
            if (e - last[e] >= w) {
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
        }
        __syncthreads();                                        // the next tile restages vx / vy / last
    }
}

// delay: x[t - w]; delta: x[t] - x[t - w].  One workgroup per (symbol, TS_TILE days), walked with a grid stride
template <int OP>
__global__ __launch_bounds__(TS_TILE) void ts_lag_kernel(const double *x, Dims d, int64_t w, int64_t chunks, int64_t total, double *out) {
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const auto [s, t0, g0] = xw_job(job, chunks, 1);        // nothing is staged: no halo
        const int64_t t = t0 + threadIdx.x;
        if (t >= d.len) continue;
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
    }
}

// what both entry points check after their own arguments; *run = false where there is nothing to launch
pq_status ts_prepare(pq_ctx *ctx, const pq_batch *b, const char *recorded, bool *run) {
    *run = false;
    if (ctx->rec) { pq_set_error("%s", recorded); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_ts / pq_factor_ts_pair (the column of a factor is [n_series][stride])");
    *run = b->len != 0 && b->n_series != 0;
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_factor_ts(pq_ctx *ctx, const pq_batch *b, const double *x, int32_t op, int64_t window, int32_t mode, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op >= TS_SUM && op <= TS_DELTA,
               "pq_factor_ts: op must be 0 (sum), 1 (std), 2 (zscore), 3 (min), 4 (max), 5 (argmin), 6 (argmax), 7 (rank), 8 (decay_linear), "
               "9 (delay) or 10 (delta)");
    PQ_REQUIRE(window >= 1 && window <= TS_MAX_W, "pq_factor_ts: window must be in [1, 1024]");
    PQ_REQUIRE((op != TS_STD && op != TS_ZSCORE) || window >= 2, "pq_factor_ts: std and zscore need window >= 2");
    PQ_REQUIRE(mode == 0 || (mode == 1 && op == TS_RANK), "pq_factor_ts: mode must be 0, or 1 (rank / window) for rank alone");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && out), "pq_factor_ts: null pointer");
    bool run;
    PQ_TRY(ts_prepare(ctx, b, "pq_factor_ts cannot be recorded into a suite", &run));
    if (!run) return PQ_OK;
    const Dims d = dims_of(b);
    // a workgroup reads a halo of days that another workgroup writes: the two [n_series][stride] columns must be disjoint
    const uintptr_t bytes = (uintptr_t)d.n * (uintptr_t)d.stride * 8;
    PQ_REQUIRE(xw_disjoint(xw_span(x, bytes), xw_span(out, bytes)), "pq_factor_ts: out must not overlap x");
    const XwGrid g = xw_grid(d);
    const dim3 block(TS_TILE);
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
    PQ_REQUIRE(window >= 2 && window <= TS_MAX_W, "pq_factor_ts_pair: window must be in [2, 1024]");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (x && y && out), "pq_factor_ts_pair: null pointer");
    bool run;
    PQ_TRY(ts_prepare(ctx, b, "pq_factor_ts_pair cannot be recorded into a suite", &run));
    if (!run) return PQ_OK;
    const Dims d = dims_of(b);
    // a workgroup reads a halo of days that another workgroup writes: out must be disjoint from both [n_series][stride] inputs
    const uintptr_t bytes = (uintptr_t)d.n * (uintptr_t)d.stride * 8;
    PQ_REQUIRE(xw_disjoint(xw_span(x, bytes), xw_span(out, bytes)) && xw_disjoint(xw_span(y, bytes), xw_span(out, bytes)),
               "pq_factor_ts_pair: out must not overlap x or y");
    const XwGrid g = xw_grid(d);
    const dim3 block(TS_TILE);
    const int w = (int)window;
    const size_t M = (size_t)(TS_TILE + w - 1), lds = 2 * M * 8 + M * 4;
    if (op == TSP_COV) hipLaunchKernelGGL(ts_pair_kernel<TSP_COV>, g.grid, block, lds, ctx->stream, x, y, d, w, g.chunks, g.total, out);
    else hipLaunchKernelGGL(ts_pair_kernel<TSP_CORR>, g.grid, block, lds, ctx->stream, x, y, d, w, g.chunks, g.total, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
