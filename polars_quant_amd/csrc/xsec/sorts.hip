// xsec/sorts.hip -- cross-sectional quantile sorts, long-short legs, turnover, coverage and IC statistics
// (Factor.quantile / portfolio_sorts / long_short / factor_mimicking_portfolio / turnover / coverage / ir / ic_win_rate;
// README.md:1479-1487, :1535-1545, :1589-1599; README-only => decision D-15).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.
//  1. prep:      the day-sort stage of xsec_dev.h (also clean.hip's and build.hip's): xs_prep_kernel, a tiled transpose, turns the
//                factor column into day-major key rows (+inf where the (factor, return) pair is not in the cross-section) and counts
//                each day's cross-section n.
//  2. label:     up to XS_LDS_MAX symbols one workgroup per day sorts its key row in LDS (xs_load_sort_row: bitonic, keys only); wider
//                cross-sections go through daysort.hip (rocPRIM's segmented radix sort, keys only, in global memory).  Each symbol then
//                finds its tie run [a, b) by binary searches of its own key in the sorted row (xs_tie_run) -- m = a + b, so ties share
//                a label and nothing depends on sort stability -- and writes one uint8 label per cell, day-major.
//  3. transpose: labels day-major -> symbol-major, 64 x 64 byte tiles.
//  4. aggregate: one thread per (day, block of 256 symbols), consecutive threads on consecutive days (coalesced); the per-group sums
//                are D-12's order (ascending symbols inside a block, from 0.0), counts and "new member" counts are integers.  A per-day
//                combine adds the block sums in ascending block order and writes mean / count / turnover / spread.
//  5. summary:   one 64-lane workgroup per output row; chunks of the series are staged in LDS and summed by one lane in ascending day
//                order (the stated sequential order), two-pass sample std.
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
    __device__ double operator()(int64_t o) const {
        const double a = f[o], b = r[o];
        return (xs_valid(a) & xs_valid(b)) ? a : xs_inf(); // &, not &&: both loads are issued before either test
    }
};

__device__ __forceinline__ uint8_t xs_label(int64_t m, int64_t nv, const XsRule &rule) {
    if (rule.mode == 0) return (uint8_t)((m * rule.q) / (2 * nv)); // floor(m Q / 2n) in integers: m < 2n => [0, Q)
    const double p = (double)m / (double)(2 * nv);
    if (p > 1.0 - rule.top) return 1;
    if (p < rule.bottom) return 0;
    return PQ_LABEL_MID;
}

// one workgroup per day, n <= XS_LDS_MAX: sort the day's keys in LDS, label every symbol (day-major)
__global__ __launch_bounds__(1024) void xs_label_lds_kernel(const double *key, const int32_t *n_valid, int64_t n, int P, XsRule rule,
                                                            uint8_t *lab) {
    extern __shared__ __align__(16) unsigned char xs_lds[];
    double *S = (double *)xs_lds;
    const int64_t t = blockIdx.x;
    const double *row = key + t * n;
    uint8_t *out = lab + t * n;
    const int tid = threadIdx.x, nthr = blockDim.x, nv = n_valid[t];
    if (nv < rule.min_n) { // uniform across the workgroup
        for (int s = tid; s < n; s += nthr) out[s] = PQ_LABEL_OUT;
        return;
    }
    xs_load_sort_row(S, row, n, P, tid, nthr);
    for (int s = tid; s < n; s += nthr) {
        const double k = row[s];
        out[s] = k == xs_inf() ? (uint8_t)PQ_LABEL_OUT : xs_label(xs_tie_run(XsRow<true>{S}, nv, k), nv, rule);
    }
}

// n > XS_LDS_MAX: the day's row was sorted by rocPRIM (sorted); label from the original row
__global__ __launch_bounds__(256) void xs_label_sorted_kernel(const double *key, const double *sorted, const int32_t *n_valid, int64_t n,
                                                              XsRule rule, uint8_t *lab) {
    const int64_t t = blockIdx.x;
    const double *row = key + t * n, *S = sorted + t * n;
    uint8_t *out = lab + t * n;
    const int nv = n_valid[t];
    for (int64_t s = threadIdx.x; s < n; s += 256) {
        const double k = row[s];
        out[s] = (nv < rule.min_n || k == xs_inf()) ? (uint8_t)PQ_LABEL_OUT : xs_label(xs_tie_run(XsRow<false>{S}, nv, k), nv, rule);
    }
}

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

// one thread per (day, block of 256 symbols): per group the sum of the members' returns (ascending symbols, from 0.0), the member count
// and the count of members that were not in the group the day before.  G >= ng groups live in registers (static indices).
template <int G>
__global__ __launch_bounds__(64) void xs_group_partial_kernel(const uint8_t *lab, int64_t lstride, const double *ret, Dims d, int ng,
                                                              double *psum, int32_t *pcnt, int32_t *pnew) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    double sum[G];
    int cnt[G], nw[G];
#pragma unroll
    for (int g = 0; g < G; g++) { sum[g] = 0.0; cnt[g] = 0; nw[g] = 0; }
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        int l[B], lp[B];
        double v[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1;
            l[k] = lab[s * lstride + t];
            lp[k] = t > 0 ? lab[s * lstride + t - 1] : PQ_LABEL_OUT;
            v[k] = ret[s * d.stride + t];
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
#pragma unroll
            for (int g = 0; g < G; g++)
                if (l[k] == g) { sum[g] += v[k]; cnt[g] += 1; nw[g] += lp[k] != g; }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (g < ng) {
            const int64_t o = ((int64_t)blockIdx.y * ng + g) * d.len + t;
            psum[o] = sum[g]; pcnt[o] = cnt[g]; pnew[o] = nw[g];
        }
}

// one thread per day: block sums in ascending block order (from 0.0); mean, count, turnover per group; top - bottom spread
__global__ __launch_bounds__(64) void xs_group_combine_kernel(const double *psum, const int32_t *pcnt, const int32_t *pnew, int64_t nblk,
                                                              int64_t len, int ng, double *mean, int32_t *count, double *tov,
                                                              double *spread) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    double lo = pq_null(), hi = pq_null();
    for (int g = 0; g < ng; g++) {
        double s = 0.0;
        int64_t c = 0, nw = 0, cp = 0;
        for (int64_t k = 0; k < nblk; k++) {
            const int64_t o = (k * ng + g) * len + t;
            s += psum[o]; c += pcnt[o]; nw += pnew[o];
            if (t > 0) cp += pcnt[o - 1];
        }
        const double m = c > 0 ? s / (double)c : pq_null();
        mean[g * len + t] = m;
        count[g * len + t] = (int32_t)c;
        tov[g * len + t] = (t > 0 && c > 0 && cp > 0) ? (double)nw / (double)c : pq_null();
        if (g == 0) lo = m;
        if (g == ng - 1) hi = m;
    }
    spread[t] = (pq_isnull(lo) || pq_isnull(hi)) ? pq_null() : hi - lo;
}

// one 64-lane workgroup per row: rows 0 .. ng-1 = the groups (mean_return[g], turnover[g]), row ng = the spread / long-short series
__global__ __launch_bounds__(64) void xs_summary_kernel(const double *mean, const double *tov, const double *spread, int64_t len, int ng,
                                                        double *summary) {
    __shared__ double buf[XS_CHUNK];
    const int g = blockIdx.x;
    const double *x = g < ng ? mean + g * len : spread;
    double s, ss, ts;
    int64_t n, nt, pos;
    xs_seq<false>(x, len, 0.0, buf, s, n, pos);
    const double m = n > 0 ? s / (double)n : pq_null();
    xs_seq<true>(x, len, n > 0 ? m : 0.0, buf, ss, n, pos);
    if (g < ng) xs_seq<false>(tov + g * len, len, 0.0, buf, ts, nt, pos);
    if (threadIdx.x == 0) {
        const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : pq_null();
        double *o = summary + (int64_t)g * PQ_GROUP_SUMMARY_COLS;
        o[0] = (double)n;
        o[1] = m;
        o[2] = sd;
        o[3] = (n >= 2 && sd > 0.0) ? m / sd * sqrt(252.0) : pq_null();
        o[4] = (g < ng && nt > 0) ? ts / (double)nt : pq_null();
    }
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

// labels -> group statistics -> summary: the body shared by pq_factor_quantiles (ng = Q) and pq_factor_long_short (ng = 2)
pq_status xs_groups(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, const XsRule &rule, int ng,
                    uint8_t *labels, double *mean, int32_t *count, double *tov, double *spread, double *summary) {
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const size_t cells = (size_t)d.len * (size_t)d.n, len = (size_t)d.len;
    const int64_t nblk = xs_nblk(d.n);
    XsDaySort plan;
    PQ_TRY(xs_day_sort_plan(ctx, d, "factor sorts", &plan));
    // workspace: keys (f64, day-major) | n per day (i32) | labels day-major (u8) | labels symbol-major (u8, when the caller passes
    // none) | block partials: sums (f64), counts, new members (i32) | wide: sorted keys (f64), offsets (u32), rocPRIM temp
    const size_t part = (size_t)nblk * (size_t)ng * len;
    const size_t o_cnt = xs_al(cells * 8), o_ldm = o_cnt + xs_al(len * 4), o_lsm = o_ldm + xs_al(cells),
                 o_ps = o_lsm + (labels ? 0 : xs_al(cells)), o_pc = o_ps + xs_al(part * 8), o_pn = o_pc + xs_al(part * 4),
                 o_srt = o_pn + xs_al(part * 4);
    PQ_TRY(pq_ws_reserve(ctx, o_srt + plan.bytes));
    unsigned char *w = (unsigned char *)ctx->ws;
    double *key = (double *)w;
    int32_t *nv = (int32_t *)(w + o_cnt);
    uint8_t *ldm = w + o_ldm;
    uint8_t *lsm = labels ? labels : w + o_lsm;
    const int64_t lstride = labels ? d.stride : d.len;
    double *psum = (double *)(w + o_ps);
    int32_t *pcnt = (int32_t *)(w + o_pc), *pnew = (int32_t *)(w + o_pn);
    if (d.n > 0) {
        PQ_HIP_TRY(hipMemsetAsync(nv, 0, len * 4, ctx->stream));
        hipLaunchKernelGGL(xs_prep_kernel<XsKey>, dim3((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32)), dim3(256), 0,
                           ctx->stream, XsKey{factor, fwd_return}, d, key, nv);
        if (!plan.wide) {
            const XsLds L = xs_lds_shape(d.n);
            PQ_HIP_TRY(hipFuncSetAttribute((const void *)xs_label_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
            hipLaunchKernelGGL(xs_label_lds_kernel, dim3((unsigned)d.len), dim3(L.nthr), L.bytes, ctx->stream, (const double *)key,
                               (const int32_t *)nv, d.n, L.P, rule, ldm);
        } else {
            const double *srt;
            PQ_TRY(xs_day_sort_wide(ctx, d, plan, w + o_srt, key, &srt));
            hipLaunchKernelGGL(xs_label_sorted_kernel, dim3((unsigned)d.len), dim3(256), 0, ctx->stream, (const double *)key, srt,
                               (const int32_t *)nv, d.n, rule, ldm);
        }
        hipLaunchKernelGGL(xs_label_transpose_kernel, dim3((unsigned)((d.len + 63) / 64), (unsigned)((d.n + 63) / 64)), dim3(256), 0,
                           ctx->stream, (const uint8_t *)ldm, d.n, d.len, lsm, lstride);
    }
    const dim3 gp((unsigned)((d.len + 63) / 64), (unsigned)nblk), gc((unsigned)((d.len + 63) / 64));
    if (ng <= 2)
        hipLaunchKernelGGL(xs_group_partial_kernel<2>, gp, dim3(64), 0, ctx->stream, (const uint8_t *)lsm, lstride, fwd_return, d, ng, psum,
                           pcnt, pnew);
    else if (ng <= 5)
        hipLaunchKernelGGL(xs_group_partial_kernel<5>, gp, dim3(64), 0, ctx->stream, (const uint8_t *)lsm, lstride, fwd_return, d, ng, psum,
                           pcnt, pnew);
    else if (ng <= 10)
        hipLaunchKernelGGL(xs_group_partial_kernel<10>, gp, dim3(64), 0, ctx->stream, (const uint8_t *)lsm, lstride, fwd_return, d, ng,
                           psum, pcnt, pnew);
    else
        hipLaunchKernelGGL(xs_group_partial_kernel<20>, gp, dim3(64), 0, ctx->stream, (const uint8_t *)lsm, lstride, fwd_return, d, ng,
                           psum, pcnt, pnew);
    hipLaunchKernelGGL(xs_group_combine_kernel, gc, dim3(64), 0, ctx->stream, (const double *)psum, (const int32_t *)pcnt,
                       (const int32_t *)pnew, nblk, d.len, ng, mean, count, tov, spread);
    hipLaunchKernelGGL(xs_summary_kernel, dim3((unsigned)(ng + 1)), dim3(64), 0, ctx->stream, (const double *)mean, (const double *)tov,
                       (const double *)spread, d.len, ng, summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // namespace

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
