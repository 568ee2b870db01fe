// xsec/sorts.hip -- cross-sectional quantile sorts, long-short legs, turnover, coverage and IC statistics
// (Factor.quantile / portfolio_sorts / long_short / factor_mimicking_portfolio / turnover / coverage / ir / ic_win_rate;
// README.md:1479-1487, :1535-1545, :1589-1599; README-only => decision D-15).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.
//  1. prep:      the day-sort stage of xsec_dev.h (also double_sort.hip's, clean.hip's and build.hip's): xs_prep_kernel, a tiled
//                transpose, turns the factor column into day-major key rows (+inf where the (factor, return) pair is not in the
//                cross-section) and counts each day's cross-section n.
//  2. label:     xsec_dev.h's sort-then-look-up pair with XsLabelOp.  Up to XS_LDS_MAX symbols one workgroup per day sorts its key row
//                in LDS (xs_load_sort_row: bitonic, keys only); wider cross-sections go through daysort.hip (rocPRIM's segmented radix
//                sort, keys only, in global memory).  Each symbol then finds its tie run [a, b) by binary searches of its own key in the
//                sorted row (xs_tie_run) -- m = a + b, so ties share a label and nothing depends on sort stability -- and writes one
//                uint8 label per cell, day-major.
// The cells stage, from day-major labels on, is defined here once for this file and double_sort.hip (D-31; interface in xsec_dev.h):
//  3. transpose: labels day-major -> symbol-major, 64 x 64 byte tiles.
//  4. aggregate: one thread per (day, block of 256 symbols), consecutive threads on consecutive days (coalesced); the per-cell sums
//                are D-12's order (ascending symbols inside a block, from 0.0), counts and "new member" counts are integers.  Up to 20
//                cells the accumulators are registers (<2 | 5 | 10 | 20>), above that LDS tiles of XS_CT cells, one column per lane
//                (robust.hip's group tiles), with blockIdx.z walking the tiles.  One thread per (day, cell) then adds the block sums in
//                ascending block order and writes mean / count / turnover; the single sorts' spread is one more row from the means.
//  5. summary:   one 64-lane workgroup per output row (the cells with their turnover, then the caller's spread rows); chunks of the
//                series are staged in LDS and summed by one lane in ascending day order (the stated sequential order), two-pass sample std.
#include "xsec_dev.h"

namespace {

struct XsRule {
    int32_t mode;    // 0: quantiles, 1: long / short
    int32_t q;       // number of quantiles (mode 0)
    int32_t min_n;   // a day with a smaller cross-section is labelled PQ_LABEL_OUT everywhere
    double top, bottom;
};

// the key of xs_prep_kernel: the factor, as it is, where the (factor, return) pair is valid
struct XsKey {
    const double *f, *r;
    __device__ void operator()(int64_t o, double (&k)[1]) const {
        const double a = f[o], b = r[o];
        if (xs_valid(a) & xs_valid(b)) k[0] = a; // &, not &&: both loads are issued before either test
    }
};

__device__ __forceinline__ uint8_t xs_label(int64_t m, int64_t nv, const XsRule &rule) {
    if (rule.mode == 0) return (uint8_t)((m * rule.q) / (2 * nv)); // floor(m Q / 2n) in integers: m < 2n => [0, Q)
    const double p = (double)m / (double)(2 * nv);
    if (p > 1.0 - rule.top) return 1;
    if (p < rule.bottom) return 0;
    return PQ_LABEL_MID;
}

// the operation of xsec_dev.h's sort-then-look-up pair: one sort, the symbol's label from its tie run (day-major)
struct XsLabelOp {
    static constexpr int MAX_STEPS = 1;
    const double *key;
    XsRule rule;
    uint8_t *lab;
    __host__ __device__ int steps() const { return 1; }
    __host__ __device__ const double *row(int) const { return key; }
    __device__ bool unsorted(int nv) const { return nv < rule.min_n; }
    __device__ void fill(int64_t i) const { lab[i] = PQ_LABEL_OUT; }
    template <bool PAD> __device__ void at(int, XsRow<PAD> S, int nv, int64_t i) const {
        const double k = key[i];
        lab[i] = k == xs_inf() ? (uint8_t)PQ_LABEL_OUT : xs_label(xs_tie_run(S, nv, k), nv, rule);
    }
};

// ---------------------------------------------------------------- the cells stage
constexpr int XS_CT = 32; // cells per LDS tile of the partial sums: 32 x 64 lanes x (8 + 4 + 4) bytes = 32 KiB of LDS

// day-major [len][n] labels -> symbol-major [n][ostride]
__global__ __launch_bounds__(256) void xs_label_transpose_kernel(const uint8_t *dm, int64_t n, int64_t len, uint8_t *sm, int64_t ostride) {
    __shared__ uint8_t tile[64][65];
    const int64_t t0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6; // 64 x 4
    for (int i = ly; i < 64; i += 4) {
        const int64_t t = t0 + i, s = s0 + lx;
        tile[i][lx] = (t < len && s < n) ? dm[t * n + s] : (uint8_t)PQ_LABEL_OUT;
    }
    __syncthreads();
    for (int i = ly; i < 64; i += 4) {
        const int64_t s = s0 + i, t = t0 + lx;
        if (s < n && t < len) sm[s * ostride + t] = tile[lx][i];
    }
}

// The partial sums, one thread per (day, block of 256 symbols): per cell the sum of the members' returns (ascending symbols, from 0.0),
// the member count and the count of new members.  Both kernels walk the block eight symbols s0 .. s0 + 7 (clamped to s_hi - 1) at a
// time, all loads issued before the first add, and apply one rule, whose loads are xs_cell_load: on day t symbol s is a member of cell
// l, and a new one when lp, its label the day before (PQ_LABEL_OUT before day 0), is another.  The comparison stays at the
// accumulation: made at the load it waits for every label before the first add (the <10> kernel took 0.173 ms against 0.154 at
// 10 000 x 5 040), and the eight loads stay a loop of the kernel (as a helper of their own they cost the register kernels 1 - 4 VGPRs).
constexpr int XS_B = 8;
__device__ __forceinline__ void xs_cell_load(const uint8_t *lab, int64_t lstride, const double *ret, int64_t rstride, int64_t t, int64_t s,
                                             int &l, int &lp, double &v) {
    l = lab[s * lstride + t];
    lp = t > 0 ? lab[s * lstride + t - 1] : PQ_LABEL_OUT;
    v = ret[s * rstride + t];
}

// C <= G cells in registers (static indices)
template <int G>
__global__ __launch_bounds__(64) void xs_cell_partial_reg_kernel(const uint8_t *lab, int64_t lstride, const double *ret, Dims d, int C,
                                                                 double *psum, int32_t *pcnt, int32_t *pnew) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    double sum[G];
    int cnt[G], nw[G];
#pragma unroll
    for (int g = 0; g < G; g++) { sum[g] = 0.0; cnt[g] = 0; nw[g] = 0; }
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += XS_B) {
        int l[XS_B], lp[XS_B];
        double v[XS_B];
#pragma unroll
        for (int k = 0; k < XS_B; k++) xs_cell_load(lab, lstride, ret, d.stride, t, s0 + k < s_hi ? s0 + k : s_hi - 1, l[k], lp[k], v[k]);
#pragma unroll
        for (int k = 0; k < XS_B; k++) {
            if (s0 + k >= s_hi) break;
#pragma unroll
            for (int g = 0; g < G; g++)
                if (l[k] == g) { sum[g] += v[k]; cnt[g] += 1; nw[g] += lp[k] != g; }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (g < C) {
            const int64_t o = ((int64_t)blockIdx.y * C + g) * d.len + t;
            psum[o] = sum[g]; pcnt[o] = cnt[g]; pnew[o] = nw[g];
        }
}

// more cells than fit registers: blockIdx.z = the tile of XS_CT cells, whose sums and counts live in LDS, one column per lane
__global__ __launch_bounds__(64) void xs_cell_partial_lds_kernel(const uint8_t *lab, int64_t lstride, const double *ret, Dims d, int C,
                                                                 double *psum, int32_t *pcnt, int32_t *pnew) {
    __shared__ double sum[XS_CT][64];
    __shared__ int cnt[XS_CT][64], nw[XS_CT][64];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    if (t >= d.len) return; // no workgroup barrier below: every lane only touches its own column
    const int c0 = (int)blockIdx.z * XS_CT, nc = C - c0 < XS_CT ? C - c0 : XS_CT;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    for (int j = 0; j < XS_CT; j++) { sum[j][lane] = 0.0; cnt[j][lane] = 0; nw[j][lane] = 0; }
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += XS_B) {
        int l[XS_B], lp[XS_B];
        double v[XS_B];
#pragma unroll
        for (int k = 0; k < XS_B; k++) xs_cell_load(lab, lstride, ret, d.stride, t, s0 + k < s_hi ? s0 + k : s_hi - 1, l[k], lp[k], v[k]);
#pragma unroll
        for (int k = 0; k < XS_B; k++) {
            if (s0 + k >= s_hi) break;
            const int j = l[k] - c0;
            if (j < 0 || j >= nc) continue; // another tile's cell, PQ_LABEL_MID or PQ_LABEL_OUT
            sum[j][lane] += v[k]; cnt[j][lane] += 1; nw[j][lane] += lp[k] != l[k];
        }
    }
    for (int j = 0; j < nc; j++) {
        const int64_t o = ((int64_t)blockIdx.y * C + c0 + j) * d.len + t;
        psum[o] = sum[j][lane]; pcnt[o] = cnt[j][lane]; pnew[o] = nw[j][lane];
    }
}

// one thread per (day, cell): block sums in ascending block order (from 0.0); mean, count, turnover
__global__ __launch_bounds__(64) void xs_cell_combine_kernel(const double *psum, const int32_t *pcnt, const int32_t *pnew, int64_t nblk,
                                                             int64_t len, int C, double *mean, int32_t *count, double *tov) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    if (t >= len) return;
    double s = 0.0;
    int64_t c = 0, nw = 0, cp = 0;
    for (int64_t k = 0; k < nblk; k++) {
        const int64_t o = (k * C + g) * len + t;
        s += psum[o]; c += pcnt[o]; nw += pnew[o];
        if (t > 0) cp += pcnt[o - 1];
    }
    mean[g * len + t] = c > 0 ? s / (double)c : pq_null();
    count[g * len + t] = (int32_t)c;
    tov[g * len + t] = (t > 0 && c > 0 && cp > 0) ? (double)nw / (double)c : pq_null();
}

// one 64-lane workgroup per row: rows 0 .. C-1 = the cells (mean_return, turnover), then the e0.n and the e1.n extra rows
__global__ __launch_bounds__(64) void xs_summary_kernel(const double *mean, const double *tov, XsRows e0, XsRows e1, int64_t len, int C,
                                                        double *summary) {
    __shared__ double buf[XS_CHUNK];
    const int g = blockIdx.x;
    const bool cell = g < C;
    const double *x = cell ? mean + g * len : (g < C + e0.n ? e0.x + (int64_t)(g - C) * len : e1.x + (int64_t)(g - C - e0.n) * len);
    double s, ss, ts = 0.0;
    int64_t n, nt = 0, pos;
    xs_seq<false>(x, len, 0.0, buf, s, n, pos);
    const double m = n > 0 ? s / (double)n : pq_null();
    xs_seq<true>(x, len, n > 0 ? m : 0.0, buf, ss, n, pos);
    if (cell) xs_seq<false>(tov + g * len, len, 0.0, buf, ts, nt, pos); // uniform across the workgroup
    if (threadIdx.x == 0) {
        const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : pq_null();
        double *o = summary + (int64_t)g * PQ_GROUP_SUMMARY_COLS;
        o[0] = (double)n;
        o[1] = m;
        o[2] = sd;
        o[3] = (n >= 2 && sd > 0.0) ? m / sd * sqrt(252.0) : pq_null();
        o[4] = (cell && nt > 0) ? ts / (double)nt : pq_null();
    }
}

// the single sorts' spread: mean[ng - 1] - mean[0], NULL where either is
__global__ __launch_bounds__(64) void xs_spread_kernel(const double *mean, int64_t len, int ng, double *spread) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    const double lo = mean[t], hi = mean[(int64_t)(ng - 1) * len + t];
    spread[t] = (pq_isnull(lo) || pq_isnull(hi)) ? pq_null() : hi - lo;
}

// n_days, mean, std, ir = mean / std (not annualised), win_rate = #(ic > 0) / n_days
__global__ __launch_bounds__(64) void xs_ic_stats_kernel(const double *ic, int64_t len, double *out) {
    __shared__ double buf[XS_CHUNK];
    double s, ss;
    int64_t n, pos, pos2;
    xs_seq<false>(ic, len, 0.0, buf, s, n, pos);
    const double m = n > 0 ? s / (double)n : 0.0;
    xs_seq<true>(ic, len, m, buf, ss, n, pos2);
    if (threadIdx.x == 0) {
        const bool ok = n >= 2;
        const double sd = ok ? sqrt(ss / (double)(n - 1)) : pq_null();
        out[0] = (double)n;
        out[1] = ok ? m : pq_null();
        out[2] = sd;
        out[3] = (ok && sd > 0.0) ? m / sd : pq_null();
        out[4] = ok ? (double)pos / (double)n : pq_null();
    }
}

// coverage: one thread per (day, block of 256 symbols) counts the valid factor values (integers: any order is exact)
__global__ __launch_bounds__(64) void xs_coverage_partial_kernel(const double *f, Dims d, int32_t *cnt) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    int c = 0;
    constexpr int B = 16;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double v[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1;
            v[k] = f[s * d.stride + t];
        }
#pragma unroll
        for (int k = 0; k < B; k++) c += (s0 + k < s_hi && xs_valid(v[k])) ? 1 : 0;
    }
    if (c) atomicAdd(&cnt[t], c);
}
__global__ __launch_bounds__(256) void xs_coverage_final_kernel(const int32_t *cnt, int64_t len, int64_t n, double *coverage) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < len) coverage[t] = n > 0 ? (double)cnt[t] / (double)n : pq_null();
}

} // namespace

// ---------------------------------------------------------------- host side of the cells stage (declared in xsec_dev.h)
XsCellsWs xs_cells_layout(XsWs &w, const Dims &d, int nkey, int ncell, bool caller_labels, const XsDaySort &plan) {
    const size_t cells = (size_t)d.len * (size_t)d.n, len = (size_t)d.len, part = (size_t)xs_nblk(d.n) * (size_t)ncell * len;
    XsCellsWs ws{nullptr, XsWs::pitch<double>(cells)};
    w.take(ws.key, cells, nkey).take(ws.nv, len).take(ws.ldm, cells).take(ws.lsm, caller_labels ? 0 : cells);
    w.take(ws.ps, part).take(ws.pc, part).take(ws.pn, part).take(ws.tail, plan.bytes);
    return ws;
}

pq_status xs_cells_stats(pq_ctx *ctx, const Dims &d, const XsCellsWs &ws, int ncell, uint8_t *labels, const double *ret, double *mean,
                         int32_t *count, double *tov) {
    const uint8_t *lsm = labels ? labels : ws.lsm;
    const int64_t lstride = labels ? d.stride : d.len, nblk = xs_nblk(d.n);
    const unsigned gx = (unsigned)((d.len + 63) / 64);
    if (d.n > 0)
        hipLaunchKernelGGL(xs_label_transpose_kernel, dim3(gx, (unsigned)((d.n + 63) / 64)), dim3(256), 0, ctx->stream,
                           (const uint8_t *)ws.ldm, d.n, d.len, (uint8_t *)lsm, lstride);
    // the accumulator form belongs to the cell count: registers while the cells fit them, LDS tiles above
    const auto partial = ncell <= 2 ? xs_cell_partial_reg_kernel<2> : ncell <= 5 ? xs_cell_partial_reg_kernel<5>
                       : ncell <= 10 ? xs_cell_partial_reg_kernel<10> : ncell <= 20 ? xs_cell_partial_reg_kernel<20>
                       : xs_cell_partial_lds_kernel;
    hipLaunchKernelGGL(partial, dim3(gx, (unsigned)nblk, ncell <= 20 ? 1u : (unsigned)((ncell + XS_CT - 1) / XS_CT)), dim3(64), 0,
                       ctx->stream, lsm, lstride, ret, d, ncell, ws.ps, ws.pc, ws.pn);
    hipLaunchKernelGGL(xs_cell_combine_kernel, dim3(gx, (unsigned)ncell), dim3(64), 0, ctx->stream, (const double *)ws.ps,
                       (const int32_t *)ws.pc, (const int32_t *)ws.pn, nblk, d.len, ncell, mean, count, tov);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status xs_cells_summary(pq_ctx *ctx, int64_t len, int ncell, const double *mean, const double *tov, XsRows e0, XsRows e1, double *summary) {
    hipLaunchKernelGGL(xs_summary_kernel, dim3((unsigned)(ncell + e0.n + e1.n)), dim3(64), 0, ctx->stream, mean, tov, e0, e1, len, ncell,
                       summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

// labels -> group statistics -> summary: the body shared by pq_factor_quantiles (ng = Q) and pq_factor_long_short (ng = 2)
static pq_status xs_groups(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, const XsRule &rule, int ng,
                           uint8_t *labels, double *mean, int32_t *count, double *tov, double *spread, double *summary) {
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    XsDaySort plan;
    PQ_TRY(xs_day_sort_plan(ctx, d, "factor sorts", &plan));
    XsCellsWs ws;
    PQ_TRY(xs_ws_carve(ctx, "factor sorts", [&](XsWs &w) { ws = xs_cells_layout(w, d, 1, ng, labels != nullptr, plan); }));
    if (d.n > 0) {
        PQ_HIP_TRY(hipMemsetAsync(ws.nv, 0, (size_t)d.len * 4, ctx->stream));
        hipLaunchKernelGGL((xs_prep_kernel<1, XsKey>), dim3((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32)), dim3(256), 0,
                           ctx->stream, XsKey{factor, fwd_return}, d, ws.key, (int64_t)ws.key_pitch, ws.nv);
        PQ_TRY(xs_sort_lookup(ctx, d, plan, ws.tail, XsLabelOp{ws.key, rule, ws.ldm}, ws.nv));
    }
    PQ_TRY(xs_cells_stats(ctx, d, ws, ng, labels, fwd_return, mean, count, tov));
    hipLaunchKernelGGL(xs_spread_kernel, dim3((unsigned)((d.len + 63) / 64)), dim3(64), 0, ctx->stream, (const double *)mean, d.len, ng,
                       spread);
    return xs_cells_summary(ctx, d.len, ng, mean, tov, XsRows{spread, 1}, XsRows{nullptr, 0}, summary);
}

extern "C" {

pq_status pq_factor_quantiles(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, int32_t n_quantiles,
                              uint8_t *labels, double *mean_return, int32_t *count, double *turnover, double *spread, double *summary) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(n_quantiles >= 2 && n_quantiles <= 20, "pq_factor_quantiles: n_quantiles must be in [2, 20]");
    PQ_REQUIRE((b->n_series == 0 || (factor && fwd_return)) && mean_return && count && turnover && spread && summary,
               "pq_factor_quantiles: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_quantiles cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_quantiles (a cross-section needs every symbol on every day)");
    const XsRule rule{0, n_quantiles, n_quantiles, 0.0, 0.0};
    return xs_groups(ctx, b, factor, fwd_return, rule, n_quantiles, labels, mean_return, count, turnover, spread, summary);
}

pq_status pq_factor_long_short(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, double top_pct,
                               double bottom_pct, uint8_t *labels, double *mean_return, int32_t *count, double *turnover, double *ls_return,
                               double *summary) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(top_pct > 0.0 && bottom_pct > 0.0 && top_pct + bottom_pct <= 1.0,
               "pq_factor_long_short: need 0 < top_pct, 0 < bottom_pct and top_pct + bottom_pct <= 1");
    PQ_REQUIRE((b->n_series == 0 || (factor && fwd_return)) && mean_return && count && turnover && ls_return && summary,
               "pq_factor_long_short: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_long_short cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_long_short (a cross-section needs every symbol on every day)");
    const XsRule rule{1, 0, 2, top_pct, bottom_pct};
    return xs_groups(ctx, b, factor, fwd_return, rule, 2, labels, mean_return, count, turnover, ls_return, summary);
}

pq_status pq_factor_coverage(pq_ctx *ctx, const pq_batch *b, const double *factor, double *coverage) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE((b->n_series == 0 || factor) && coverage, "pq_factor_coverage: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_coverage cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_coverage (a cross-section needs every symbol on every day)");
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    PQ_TRY(pq_ws_reserve(ctx, (size_t)d.len * 4));
    int32_t *cnt = (int32_t *)ctx->ws;
    PQ_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)d.len * 4, ctx->stream));
    if (d.n > 0)
        hipLaunchKernelGGL(xs_coverage_partial_kernel, dim3((unsigned)((d.len + 63) / 64), (unsigned)xs_nblk(d.n)),
                           dim3(64), 0, ctx->stream, factor, d, cnt);
    hipLaunchKernelGGL(xs_coverage_final_kernel, dim3((unsigned)((d.len + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t *)cnt,
                       d.len, d.n, coverage);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_ic_stats(pq_ctx *ctx, const double *ic, int64_t len, double *out) {
    PQ_REQUIRE(ctx && out && (len == 0 || ic), "pq_ic_stats: null pointer");
    PQ_REQUIRE(len >= 0, "pq_ic_stats: negative length");
    if (ctx->rec) { pq_set_error("pq_ic_stats cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(xs_ic_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, ic, len, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
