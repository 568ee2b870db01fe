// xsec/linear.hip -- the pooled OLS of the data-processing surface, linear(df, x_cols, y_col, pred_col, resid_col, return_stats):
// one regression y = a + sum_j b_j x_j over ALL rows of the columns, with the prediction and the residual column; README.md:165-240,
// README-only => decision D-24, DESIGN.md section 2.
//
// The three passes, the centred normal equations, the solve and the standard errors are D-17's (regress.hip): pass 1 n and the sums,
// pass 2 the packed triangle of the K + 1 columns x_0 .. x_{K-1}, y that xsec_ols.h factorises, pass 3 the squared residuals -- here
// of the residuals it writes, resid = y - pred with pred = a + sum_j b_j x_j (j ascending, from a).  The solve is xo_fit (xsec_ols.h) and
// the coefficient statistics are rg_coef_stats / rg_r2 (xsec_ttest.h), the functions regress.hip calls.  What differs is the reduction: D-17
// has one thread per (unit, block of 256 indices) and a serial combine per unit, and a pooled fit is ONE unit of up to 5e7 rows.
//
// Summation order (a function of the logical row index r = s * len + t alone: not of the grid, the CU count or the row pitch):
//  1. tile:    rows [k LN_TILE, (k + 1) LN_TILE) belong to tile k, one workgroup of 256 lanes.  Lane l adds the terms of rows
//              k LN_TILE + l + 256 i, i = 0 .. 15 ascending, from +0.0; a row that is no member (or lies behind the last row) adds +0.0,
//              which never changes a round-to-nearest sum that started at +0.0.
//  2. tree:    the 256 lane sums fold in a fixed tree (ln_fold): within each wave v[l] += v[l + o] for o = 32, 16, 8, 4, 2, 1 (shuffles),
//              then the four wave sums through LDS as (w0 + w2) + (w1 + w3).  One partial per accumulator and tile, ps[q][tile].
//  3. stage 2: one workgroup per accumulator: lane l adds the partials of tiles l + 256 i, i ascending, from +0.0 (LN_STAGE2 = 256
//              partials per step), and the 256 lane sums fold in the same tree.
// The member count rides along as one more f64 accumulator of pass 1 (sums of ones are exact in any order below 2^53).  No atomics.
// Loads are 8 bytes per lane on consecutive rows (a pitched [N, T] column is walked by (s, t), advanced by 256 rows without a division),
// xo_ahead(K + 1) rows ahead; the two output columns leave as streaming stores.
#include "xsec_ols.h"
#include "xsec_ttest.h"

namespace {

constexpr int LN_THREADS = 256, LN_WAVES = LN_THREADS / 64;
constexpr int LN_ROWS = 16;                       // rows per lane and tile
constexpr int LN_TILE = LN_THREADS * LN_ROWS;     // PQ_LINEAR_TILE
constexpr int LN_STAGE2 = LN_THREADS;             // PQ_LINEAR_STAGE2
constexpr int LN_AHEAD2 = 8;                      // partials loaded ahead per lane in stage 2
static_assert(LN_TILE == PQ_LINEAR_TILE && LN_STAGE2 == PQ_LINEAR_STAGE2, "pq_hip.h documents the tile constants");

enum LnPass { LN_P1 = 1, LN_P2 = 2, LN_P3 = 3 };

template <int K> struct LnNa {   // accumulators per pass: P1 the K + 1 column sums and the count, P2 the packed triangle, P3 the SSE
    static constexpr int P1 = K + 2, P2 = xo_tri(K + 1), P3 = 1;
};
constexpr int LN_MAX_NA = LnNa<XO_MAX_K>::P2;

struct LnIn {
    const double *x[XO_MAX_K];
    const double *y;
    int64_t rows, len, stride;   // rows = n_series * len logical rows; row r = s * len + t lies at s * stride + t
    int64_t step_s, step_t;      // 256 rows on: s += step_s, t += step_t, and one carry
};

// the fit's state in the workspace
struct LnState {
    int64_t *n;
    int32_t *ok;       // 1: solved
    double *mean;      // [K + 1]: xbar_0 .. xbar_{K-1}, ybar
    double *b;         // [K + 1]: b_0 .. b_{K-1}, intercept
    double *v;         // [K + 1]: diag(C^-1), then 1/n + xbar^T C^-1 xbar
    double *syy;
    double *sums;      // [LN_MAX_NA]: the pass's accumulators after stage 2
};

// the tree over the 256 lane sums; thread q < NA returns accumulator q's total (the other threads return 0.0)
template <int NA> __device__ __forceinline__ double ln_fold(double (&acc)[NA], double (*red)[LN_WAVES]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < NA; q++) acc[q] += __shfl_xor(acc[q], o, 64);   // lane l < o: v[l] + v[l + o]; the upper lanes mirror it
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NA; q++) red[q][wave] = acc[q];
    }
    __syncthreads();
    double tot = 0.0;
    if ((int)threadIdx.x < NA) tot = (red[threadIdx.x][0] + red[threadIdx.x][2]) + (red[threadIdx.x][1] + red[threadIdx.x][3]);
    return tot;
}

// stage 2, the lane's part: the partials p[l + 256 i] in ascending i from +0.0
__device__ __forceinline__ double ln_lane_sum(const double *p, int64_t ntile) {
    double a = 0.0;
    for (int64_t k0 = threadIdx.x; k0 < ntile; k0 += (int64_t)LN_STAGE2 * LN_AHEAD2) {
        double v[LN_AHEAD2];
#pragma unroll
        for (int i = 0; i < LN_AHEAD2; i++) {
            const int64_t k = k0 + (int64_t)i * LN_STAGE2;
            v[i] = k < ntile ? p[k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < LN_AHEAD2; i++) a += v[i];
    }
    return a;
}

// ---------------------------------------------------------------- passes
template <int K, int P, bool FLAT, bool OUT>
__global__ __launch_bounds__(LN_THREADS) void ln_pass_kernel(LnIn in, LnState st, double *ps, int64_t ntile, double *pred, double *resid) {
    constexpr int NA = P == LN_P1 ? LnNa<K>::P1 : (P == LN_P2 ? LnNa<K>::P2 : LnNa<K>::P3);
    __shared__ double red[NA][LN_WAVES];
    const int64_t tile = blockIdx.x;
    double mean[K + 1], b[K + 1];
#pragma unroll
    for (int j = 0; j <= K; j++) { mean[j] = 0.0; b[j] = 0.0; }
    bool ok = true;
    if (P == LN_P2) {
#pragma unroll
        for (int j = 0; j <= K; j++) mean[j] = st.mean[j];
    }
    if (P == LN_P3) {
        ok = *st.ok != 0;
#pragma unroll
        for (int j = 0; j <= K; j++) b[j] = st.b[j];
    }
    double acc[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) acc[q] = 0.0;
    int64_t r = tile * LN_TILE + threadIdx.x, s = 0, t = r;
    if (!FLAT) { s = r / in.len; t = r - s * in.len; }   // (rows > 0 here: a pitched batch is not empty)
    constexpr int B = xo_ahead(K + 1);
    static_assert(LN_ROWS % B == 0, "the rows of a lane are loaded in whole batches");
    if (P == LN_P3 && !ok) {   // no solution: NULL columns, a zero partial (without outputs the grid only writes its zeros: whether the
                               // fit solved is known on the device alone, and a fit without a solution is not the case to be fast in)
        if (OUT) {
            for (int i = 0; i < LN_ROWS; i++) {
                if (r < in.rows) {
                    const int64_t o = FLAT ? r : s * in.stride + t;
                    __builtin_nontemporal_store(pq_null(), pred + o);
                    __builtin_nontemporal_store(pq_null(), resid + o);
                }
                r += LN_THREADS;
                if (!FLAT) { s += in.step_s; t += in.step_t; if (t >= in.len) { t -= in.len; s += 1; } }
            }
        }
    } else {
#pragma unroll 1   // B rows of loads in flight per lane, not all 16: the registers go to occupancy
        for (int i0 = 0; i0 < LN_ROWS; i0 += B) {
            double yv[B], xv[B][K];
            int64_t off[B];
            bool in_rng[B];
#pragma unroll
            for (int k = 0; k < B; k++) {
                in_rng[k] = r < in.rows;
                const int64_t o = FLAT ? r : s * in.stride + t;
                off[k] = o;
                yv[k] = in_rng[k] ? in.y[o] : pq_null();
#pragma unroll
                for (int j = 0; j < K; j++) xv[k][j] = in_rng[k] ? in.x[j][o] : pq_null();
                r += LN_THREADS;
                if (!FLAT) { s += in.step_s; t += in.step_t; if (t >= in.len) { t -= in.len; s += 1; } }
            }
#pragma unroll
            for (int k = 0; k < B; k++) {
                bool xok = true;
#pragma unroll
                for (int j = 0; j < K; j++) xok = xok && xs_valid(xv[k][j]);
                const bool mem = xok && xs_valid(yv[k]);
                if (P == LN_P1) {
#pragma unroll
                    for (int j = 0; j < K; j++) acc[j] += mem ? xv[k][j] : 0.0;
                    acc[K] += mem ? yv[k] : 0.0;
                    acc[K + 1] += mem ? 1.0 : 0.0;
                }
                if (P == LN_P2) {
                    double d[K + 1];
#pragma unroll
                    for (int j = 0; j < K; j++) d[j] = xv[k][j] - mean[j];
                    d[K] = yv[k] - mean[K];
#pragma unroll
                    for (int j = 0; j <= K; j++)
#pragma unroll
                        for (int l = 0; l <= j; l++) {
                            const double pr = d[j] * d[l];
                            acc[xo_tri(j) + l] += mem ? pr : 0.0;
                        }
                }
                if (P == LN_P3) {
                    double p = b[K];
#pragma unroll
                    for (int j = 0; j < K; j++) p = p + b[j] * xv[k][j];
                    const double e = yv[k] - p, ee = e * e;
                    acc[0] += mem ? ee : 0.0;
                    if (OUT && in_rng[k]) {
                        __builtin_nontemporal_store(xok ? p : pq_null(), pred + off[k]);
                        __builtin_nontemporal_store(mem ? e : pq_null(), resid + off[k]);
                    }
                }
            }
        }
    }
    const double tot = ln_fold<NA>(acc, red);
    if ((int)threadIdx.x < NA) ps[(int64_t)threadIdx.x * ntile + tile] = tot;
}

// stage 2 after pass 1: workgroup q sums column q and the count; n and the K + 1 means
template <int K> __global__ __launch_bounds__(LN_THREADS) void ln_means_kernel(const double *ps, int64_t ntile, LnState st) {
    __shared__ double red[2][LN_WAVES];
    __shared__ double tot[2];
    double acc[2] = {ln_lane_sum(ps + (int64_t)blockIdx.x * ntile, ntile), ln_lane_sum(ps + (int64_t)(K + 1) * ntile, ntile)};
    const double v = ln_fold<2>(acc, red);
    if (threadIdx.x < 2) tot[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        st.mean[blockIdx.x] = tot[0] / tot[1];
        if (blockIdx.x == 0) *st.n = (int64_t)tot[1];
    }
}

// stage 2 of one accumulator per workgroup -> sums[q]
__global__ __launch_bounds__(LN_THREADS) void ln_sum_kernel(const double *ps, int64_t ntile, double *sums) {
    __shared__ double red[1][LN_WAVES];
    double acc[1] = {ln_lane_sum(ps + (int64_t)blockIdx.x * ntile, ntile)};
    const double v = ln_fold<1>(acc, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// after pass 2 (one thread): the triangle goes through xo_fit, as in rg_solve_kernel -- b, the intercept, diag(C^-1) and
// 1/n + xbar^T C^-1 xbar
template <int K> __global__ __launch_bounds__(64) void ln_solve_kernel(LnState st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    constexpr int NA = LnNa<K>::P2;
    double s[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) s[q] = st.sums[q];
    *st.syy = s[NA - 1];
    *st.ok = xo_fit<K>(s, *st.n, st.mean, st.mean + K, st.b, st.v, 1) ? 1 : 0;
}

// stage 2 after pass 3 and the statistics of rg_final_kernel (xsec_ttest.h) on n - K - 1 degrees of freedom.  Thread j <= K writes
// coefficient j.
template <int K>
__global__ __launch_bounds__(LN_THREADS) void ln_final_kernel(const double *ps, int64_t ntile, LnState st, double *coef, double *tst,
                                                              double *pv, double *r2, int64_t *n_out) {
    __shared__ double red[1][LN_WAVES];
    __shared__ double tot;
    double acc[1] = {ln_lane_sum(ps, ntile)};
    const double v = ln_fold<1>(acc, red);
    if (threadIdx.x == 0) tot = v;
    __syncthreads();
    const int j = threadIdx.x;
    if (j > K) return;
    const double sse = tot;
    const int64_t n = *st.n;
    const bool ok = *st.ok != 0;
    const double df = (double)(n - K - 1), s2 = sse / df, syy = ok ? *st.syy : 0.0;
    if (j == 0) {
        *n_out = n;
        *r2 = rg_r2(ok, sse, syy);
    }
    rg_coef_stats(ok, st.b + j, st.v + j, s2, df, coef + j, tst + j, pv + j);
}

struct LnOut {
    double *coef, *tst, *pv, *r2;
    int64_t *n;
    double *pred, *resid;
};

// workspace: n (i64) | ok (i32) | 3 (K + 1) + 1 + LN_MAX_NA f64: mean, b, v, syy, sums | tile partials [NA][ntile] (f64)
template <int K, bool FLAT, bool OUT>
pq_status ln_run(pq_ctx *ctx, const LnIn &in, const LnOut &out) {
    const int64_t ntile = in.rows > LN_TILE ? (in.rows + LN_TILE - 1) / LN_TILE : 1;   // at least one: an empty column still gets its zero sums
    constexpr int NS = 3 * (K + 1) + 1 + LN_MAX_NA;
    static_assert(LnNa<K>::P1 <= LnNa<K>::P2 && LnNa<K>::P3 <= LnNa<K>::P2, "every pass's partials fit the carve of pass 2");
    LnState st;
    double *ps;
    PQ_TRY(xs_ws_carve(ctx, "pq_linear", [&](XsWs &w) { w.take(st.n, 1).take(st.ok, 1).take(st.mean, NS).take(ps, (size_t)ntile * LnNa<K>::P2); }));
    st.b = st.mean + (K + 1); st.v = st.b + (K + 1); st.syy = st.v + (K + 1); st.sums = st.syy + 1;
    const dim3 gp((unsigned)ntile), blk(LN_THREADS);
    hipStream_t sm = ctx->stream;
    hipLaunchKernelGGL((ln_pass_kernel<K, LN_P1, FLAT, false>), gp, blk, 0, sm, in, st, ps, ntile, (double *)nullptr, (double *)nullptr);
    PQ_HIP_TRY(hipGetLastError());   // a launch that cannot be configured is reported before six more are enqueued
    hipLaunchKernelGGL(ln_means_kernel<K>, dim3(K + 1), blk, 0, sm, (const double *)ps, ntile, st);
    hipLaunchKernelGGL((ln_pass_kernel<K, LN_P2, FLAT, false>), gp, blk, 0, sm, in, st, ps, ntile, (double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(ln_sum_kernel, dim3(LnNa<K>::P2), blk, 0, sm, (const double *)ps, ntile, st.sums);
    hipLaunchKernelGGL(ln_solve_kernel<K>, dim3(1), dim3(64), 0, sm, st);
    hipLaunchKernelGGL((ln_pass_kernel<K, LN_P3, FLAT, OUT>), gp, blk, 0, sm, in, st, ps, ntile, out.pred, out.resid);
    hipLaunchKernelGGL(ln_final_kernel<K>, dim3(1), blk, 0, sm, (const double *)ps, ntile, st, out.coef, out.tst, out.pv, out.r2, out.n);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

template <int K> pq_status ln_layout(pq_ctx *ctx, const LnIn &in, const LnOut &out) {
    const bool flat = in.stride == in.len || in.rows == in.len;   // one series, or rows without padding: row r lies at r
    const bool outs = out.pred != nullptr;
    if (flat) return outs ? ln_run<K, true, true>(ctx, in, out) : ln_run<K, true, false>(ctx, in, out);
    return outs ? ln_run<K, false, true>(ctx, in, out) : ln_run<K, false, false>(ctx, in, out);
}

pq_status ln_dispatch(pq_ctx *ctx, int k, const LnIn &in, const LnOut &out) {
    return xo_with_k<XO_MAX_K>(k, [&](auto K) { return ln_layout<decltype(K)::value>(ctx, in, out); });
}

} // namespace

extern "C" pq_status pq_linear(pq_ctx *ctx, const pq_batch *b, const double *const *x, int32_t k, const double *y, double *coef,
                               double *t_stat, double *p_value, double *r2, int64_t *n, double *pred, double *resid) {
    PQ_TRY(pq_check(ctx, b));
    if (k < 1 || k > XO_MAX_K) { pq_set_error("pq_linear: k must be in [1, 8]"); return PQ_ERR_ARG; }
    if (ctx->rec) { pq_set_error("pq_linear cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("pq_linear: ragged batches are not supported"); return PQ_ERR_UNSUPPORTED; }
    const bool empty = b->n_series == 0 || b->len == 0;
    if (!empty && (!x || !y)) { pq_set_error("pq_linear: null pointer"); return PQ_ERR_ARG; }
    PQ_REQUIRE(coef && t_stat && p_value && r2 && n, "pq_linear: null output pointer");
    PQ_REQUIRE((pred == nullptr) == (resid == nullptr), "pq_linear: pred and resid are given together or not at all");
    LnIn in{};
    in.y = y;
    in.rows = empty ? 0 : b->n_series * b->len;
    in.len = empty ? 1 : b->len;
    in.stride = empty ? 1 : b->stride;
    in.step_s = LN_THREADS / in.len;
    in.step_t = LN_THREADS % in.len;
    for (int j = 0; j < k && !empty; j++) {
        if (!x[j]) { pq_set_error("pq_linear: null regressor pointer"); return PQ_ERR_ARG; }
        in.x[j] = x[j];
    }
    return ln_dispatch(ctx, k, in, LnOut{coef, t_stat, p_value, r2, n, empty ? nullptr : pred, empty ? nullptr : resid});
}
