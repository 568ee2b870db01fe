// xsec/attribution.hip -- the return attribution of holdings through the factor model (api.return_attribution, Factor.return_attribution;
// decision D-36): how much of every day's return of a book came from each style factor, each industry and the
// specific returns of Factor.pure_factor_return (D-32), and how much the model cannot see.  For a member of D-32's sample
// r = sum_j x_j f_j + f_g + u, so sum h r over the covered symbols is X . f + sum h u with X = B' h, risk.hip's first portfolio pass.
//
// Every day t in [0, len) is evaluated.  P books: the holdings alone (P = 1), or with a benchmark the portfolio, the benchmark and the
// active book a = h - b (P = 3).
//  pass:     at_pass_kernel<PC, FIRST>: 64 lanes = 64 consecutive days (every column load of a wave is 512 contiguous bytes), blockIdx.y =
//            the block of 256 symbols (rk_pf_pass1_kernel's shape).  Per book the K + 3 sums without an industry index -- h x_j, h u, the
//            unexplained and the realized h r -- and the three counts sit in registers under static indices (guarded unrolled loops over
//            the caps); the industry sums sit [book][g][lane] in LDS.  All of them do not fit at every G, so the pass runs over ranges of
//            at_chunk(P, G) industries; the registers and the counts belong to the first launch (FIRST), the later ones add their
//            industries only.  Every plane word is loaded once per (symbol, day) and used for all books; the loads of AT_AHEAD symbols
//            are issued before the first is used.  Block partials go to the workspace.
//  sum:      one thread per (day, cell) adds the partials in ascending block order from 0.0 (D-12's blocked sum); the count rows likewise.
//  day:      one thread per (day, book): the contributions c_j = X[j] f_j(t), the six totals and the NULL days.
//  summary:  one 64-lane workgroup per (book, series): xsec_ttest.h's summary row over the series' non-NULL days.
//  periods:  one thread per (book, series, period) adds the period's non-NULL days in ascending order from 0.0; the threads of series 0
//            also count the days whose total is not NULL.
// The operation order is D-36's, restated in tests/xsec_attribution_ref.py.
#include "xsec_ttest.h"
#include "xsec_window.h"

namespace {

constexpr int AT_MAX_K = PQ_REGRESS_MAX_K;
constexpr int AT_TOTALS = PQ_ATTRIBUTION_TOTALS;   // style, industry, specific, unexplained, total, realized
constexpr int AT_LDS_CELLS = 128;                  // (book, industry) pairs of [64]-lane f64 accumulators per workgroup: 64 KiB (wls.hip's WL_LDS_CELLS)
constexpr int AT_AHEAD = 4;                        // symbols whose loads are in flight before the first is used
static_assert(XS_BLOCK % AT_AHEAD == 0, "a block is walked in whole groups");

// industries per launch of the pass: as many as keep books * chunk within AT_LDS_CELLS (wl_chunk's rule: at least one, at most G)
inline int at_chunk(int books, int G) {
    const int c = AT_LDS_CELLS / books;
    return c > G ? G : c;
}

struct AtIn {
    const double *h, *b, *x[AT_MAX_K];   // b: the benchmark, read with PC = 3 only
    int32_t K;
    XsGroups grp;                        // null codes: every symbol in group 0 (G = 1)
    const double *u, *r;                 // r null: no next return
    Dims d;
};

// cells of one book: X_0 .. X_{K-1}, the G industry rows, then specific, unexplained, realized: NQ = K + G + 3 rows.  Block partials
// ps[block][book][NQ][len], counts pc[block][3][book][len] (held, uncovered, missing).  LDS: acc[book][g - g0][lane] for g in [g0, g0 + gc).
template <int PC, bool FIRST>
__global__ __launch_bounds__(64) void at_pass_kernel(AtIn in, int g0, int gc, double *ps, int32_t *pc) {
    extern __shared__ double at_acc[];
    const int lane = threadIdx.x;
    const int64_t len = in.d.len, t = (int64_t)blockIdx.x * 64 + lane;
    if (t >= len) return;
    const int K = in.K, G = in.grp.G, NQ = K + G + 3;
    for (int q = 0; q < PC * gc; q++) at_acc[q * 64 + lane] = 0.0;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < in.d.n ? s_lo + XS_BLOCK : in.d.n;
    double X[PC][AT_MAX_K], spec[PC], unex[PC], real[PC];
    int32_t nh[PC], nu[PC], nm[PC];
#pragma unroll
    for (int p = 0; p < PC; p++) {
#pragma unroll
        for (int j = 0; j < AT_MAX_K; j++) X[p][j] = 0.0;
        spec[p] = unex[p] = real[p] = 0.0;
        nh[p] = nu[p] = nm[p] = 0;
    }
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += AT_AHEAD) {
        double hv[AT_AHEAD], bv[AT_AHEAD], uv[AT_AHEAD], rv[AT_AHEAD], xv[AT_AHEAD][AT_MAX_K];
        int32_t gv[AT_AHEAD];
#pragma unroll
        for (int a = 0; a < AT_AHEAD; a++) {                    // a symbol past the block's end is held by no book
            const int64_t s = s0 + a, o = s * in.d.stride + t;
            const bool in_blk = s < s_hi;
            hv[a] = in_blk ? in.h[o] : 0.0;
            bv[a] = PC == 3 && in_blk ? in.b[o] : 0.0;
            uv[a] = in_blk ? in.u[o] : 0.0;
            rv[a] = in_blk && in.r ? in.r[o] : pq_null();
            gv[a] = in_blk && in.grp.codes ? in.grp.codes[in.grp.stride ? s * in.grp.stride + t : s] : 0;
#pragma unroll
            for (int j = 0; j < AT_MAX_K; j++) xv[a][j] = j < K && in_blk ? in.x[j][o] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < AT_AHEAD; a++) {
            const int32_t g = gv[a];
            bool covered = xs_valid(uv[a]) && g >= 0 && g < G;
#pragma unroll
            for (int j = 0; j < AT_MAX_K; j++) covered = covered && xs_valid(xv[a][j]);
            const bool r_ok = xs_valid(rv[a]);
            double v[PC];
            v[0] = hv[a];
            if (PC == 3) {
                v[1] = bv[a];
                v[2] = (xs_valid(hv[a]) ? hv[a] : 0.0) - (xs_valid(bv[a]) ? bv[a] : 0.0);
            }
#pragma unroll
            for (int p = 0; p < PC; p++) {
                const double w = v[p];
                if (!(xs_valid(w) && w != 0.0)) continue;
                if (covered) {
                    if (g >= g0 && g < g0 + gc) at_acc[(p * gc + (g - g0)) * 64 + lane] += w;
                }
                if (FIRST) {
                    nh[p]++;
                    if (covered) {
#pragma unroll
                        for (int j = 0; j < AT_MAX_K; j++)
                            if (j < K) X[p][j] += w * xv[a][j];
                        spec[p] += w * uv[a];
                    } else {
                        nu[p]++;
                        if (r_ok) unex[p] += w * rv[a];
                        else nm[p]++;
                    }
                    if (r_ok) real[p] += w * rv[a];
                }
            }
        }
    }
    const int64_t blk = blockIdx.y;
#pragma unroll
    for (int p = 0; p < PC; p++) {
        double *row = ps + ((blk * PC + p) * NQ) * len + t;
        for (int q = 0; q < gc; q++) row[(int64_t)(K + g0 + q) * len] = at_acc[(p * gc + q) * 64 + lane];
        if (FIRST) {
#pragma unroll
            for (int j = 0; j < AT_MAX_K; j++)
                if (j < K) row[(int64_t)j * len] = X[p][j];
            row[(int64_t)(K + G) * len] = spec[p];
            row[(int64_t)(K + G + 1) * len] = unex[p];
            row[(int64_t)(K + G + 2) * len] = real[p];
            pc[((blk * 3 + 0) * PC + p) * len + t] = nh[p];
            pc[((blk * 3 + 1) * PC + p) * len + t] = nu[p];
            pc[((blk * 3 + 2) * PC + p) * len + t] = nm[p];
        }
    }
}

// one thread per (day, cell q of the rows = P * NQ): the block sums in ascending block order from 0.0 -> X[q][len]; the threads of the
// first 3 * P cells also add the count row of the same index -> n_out[3][P][len]
__global__ __launch_bounds__(64) void at_sum_kernel(const double *ps, const int32_t *pc, int64_t nblk, int64_t len, int rows, int crows,
                                                    double *X, int32_t *n_out) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int q = blockIdx.y;
    if (t >= len) return;
    double s = 0.0;
    for (int64_t k = 0; k < nblk; k++) s += ps[(k * rows + q) * len + t];
    X[(int64_t)q * len + t] = s;
    if (q < crows) {
        int32_t n = 0;
        for (int64_t k = 0; k < nblk; k++) n += pc[(k * crows + q) * len + t];
        n_out[(int64_t)q * len + t] = n;
    }
}

// one thread per (day, book): c_j = X[j] f_j(t) where X[j] != 0 and 0.0 where it is 0 (an empty industry's NULL return does not matter);
// a NULL or non-finite f_j(t) that is needed and a day on which nothing is held make every f64 output of the book's day NULL
__global__ __launch_bounds__(64) void at_day_kernel(const double *X, const int32_t *n_out, const double *f, int64_t fr_stride, int64_t len,
                                                    int K, int G, int P, int has_r, double *exposure, double *contribution, double *totals) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int p = blockIdx.y, M = K + G, NQ = M + 3;
    if (t >= len) return;
    const double *Xp = X + (int64_t)p * NQ * len + t;
    bool nul = n_out[(int64_t)p * len + t] == 0;
    double style = 0.0, industry = 0.0;
    for (int j = 0; j < M; j++) {
        const double xj = Xp[(int64_t)j * len];
        double c = 0.0;
        if (xj != 0.0) {
            const double fj = f[(int64_t)j * fr_stride + t];
            nul = nul || !xs_valid(fj);
            c = xj * fj;
        }
        if (j < K) style += c;
        else industry += c;
    }
    const double spec = Xp[(int64_t)M * len], unex = Xp[(int64_t)(M + 1) * len], real = Xp[(int64_t)(M + 2) * len];
    const double total = ((style + industry) + spec) + unex;
    for (int j = 0; j < M; j++) {
        const int64_t o = ((int64_t)p * M + j) * len + t;
        const double xj = Xp[(int64_t)j * len];
        exposure[o] = nul ? pq_null() : rk_nan_null(xj);
        contribution[o] = nul ? pq_null() : (xj != 0.0 ? rk_nan_null(xj * f[(int64_t)j * fr_stride + t]) : 0.0);
    }
    double *tp = totals + (int64_t)p * AT_TOTALS * len + t;
    tp[0] = nul ? pq_null() : rk_nan_null(style);
    tp[len] = nul ? pq_null() : rk_nan_null(industry);
    tp[2 * len] = nul ? pq_null() : rk_nan_null(spec);
    tp[3 * len] = nul ? pq_null() : rk_nan_null(unex);
    tp[4 * len] = nul ? pq_null() : rk_nan_null(total);
    tp[5 * len] = nul || !has_r ? pq_null() : rk_nan_null(real);
}

// series q of book p: the M contribution rows, then the six totals
__device__ __forceinline__ const double *at_series(const double *contribution, const double *totals, int64_t len, int M, int p, int q) {
    return q < M ? contribution + ((int64_t)p * M + q) * len : totals + ((int64_t)p * AT_TOTALS + (q - M)) * len;
}

// one 64-lane workgroup per (book, series): D-17's summary row over the non-NULL days
__global__ __launch_bounds__(64) void at_summary_kernel(const double *contribution, const double *totals, int64_t len, int M, double *summary) {
    __shared__ double buf[XS_CHUNK];
    const int NS = M + AT_TOTALS, p = blockIdx.x / NS, q = blockIdx.x - p * NS;
    rg_summary_row(at_series(contribution, totals, len, M, p, q), len, buf, summary + (int64_t)blockIdx.x * RG_SUMMARY_COLS);
}

// one thread per (book, series, period): the sum over the period's non-NULL days, ascending from 0.0 -> psum[P][NS][S]; the threads of
// series M + 4 (total) also count those days -> pdays[P][S]
__global__ __launch_bounds__(64) void at_period_kernel(const double *contribution, const double *totals, int64_t len, int M, int P,
                                                       const int64_t *bounds, int64_t S, double *psum, int32_t *pdays) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x, NS = M + AT_TOTALS;
    if (i >= (int64_t)P * NS * S) return;
    const int64_t k = i % S, pq = i / S;
    const int p = (int)(pq / NS), q = (int)(pq - (int64_t)p * NS);
    const double *x = at_series(contribution, totals, len, M, p, q);
    double s = 0.0;
    int32_t n = 0;
    for (int64_t t = bounds[k]; t < bounds[k + 1]; t++) {
        const double v = x[t];
        if (v == v) { s += v; n++; }
    }
    psum[i] = s;
    if (q == M + 4) pdays[(int64_t)p * S + k] = n;
}

template <int PC>
pq_status at_pass(pq_ctx *ctx, const AtIn &in, int64_t nblk, double *ps, int32_t *pc) {
    const int G = in.grp.G, gc = at_chunk(PC, G);
    const dim3 grid((unsigned)((in.d.len + 63) / 64), (unsigned)nblk);
    const size_t lds = (size_t)PC * gc * 64 * 8;
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)at_pass_kernel<PC, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)at_pass_kernel<PC, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int g0 = 0; g0 < G; g0 += gc) {
        const int n = G - g0 < gc ? G - g0 : gc;
        if (g0 == 0) hipLaunchKernelGGL((at_pass_kernel<PC, true>), grid, dim3(64), lds, ctx->stream, in, g0, n, ps, pc);
        else hipLaunchKernelGGL((at_pass_kernel<PC, false>), grid, dim3(64), lds, ctx->stream, in, g0, n, ps, pc);
    }
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_return_attribution(pq_ctx *ctx, const pq_batch *b, const double *holdings, const double *benchmark_holdings,
                                const double *const *exposures, int32_t k, const int32_t *industry, int64_t group_stride, int32_t n_groups,
                                const double *factor_return, int64_t fr_stride, const double *specific_return, const double *next_return,
                                const int64_t *period_bounds, int64_t n_periods, double *exposure_out, double *contribution_out,
                                double *totals_out, int32_t *n_out, double *summary_out, double *period_sum_out, int32_t *period_days_out) {
    const char *what = "pq_return_attribution";
    auto refuse = [&](const char *text, pq_status s) { pq_set_error("%s: %s", what, text); return s; };
    PQ_TRY(pq_check(ctx, b));
    if (k < 0 || k > AT_MAX_K) return refuse("k must be in [0, 8]", PQ_ERR_ARG);
    AtIn in{};
    PQ_TRY(xs_groups_arg(what, b, industry, group_stride, n_groups, XsGroupsPolicy{XS_G_ALWAYS, "n_groups", "industry"}, &in.grp));
    if (ctx->rec) return refuse("cannot be recorded into a suite", PQ_ERR_UNSUPPORTED);
    if (b->offsets) return refuse("ragged batches are not supported", PQ_ERR_UNSUPPORTED);
    PQ_TRY(xs_groups_stride(what, b, industry != nullptr, group_stride));
    if (fr_stride < b->len) return refuse("fr_stride must be >= len", PQ_ERR_ARG);
    const int64_t S = n_periods;
    if (S < 0 || (S > 0) != (period_bounds != nullptr)) return refuse("period_bounds must be given exactly when n_periods > 0", PQ_ERR_ARG);
    for (int64_t i = 0; i <= S && S > 0; i++)
        if (period_bounds[i] < 0 || period_bounds[i] > b->len || (i > 0 && period_bounds[i] <= period_bounds[i - 1]))
            return refuse("period_bounds must be strictly ascending in [0, len]", PQ_ERR_ARG);
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    if (!(holdings && factor_return && specific_return && exposure_out && contribution_out && totals_out && n_out && summary_out) ||
        (k > 0 && !exposures) || (S > 0 && !(period_sum_out && period_days_out)))
        return refuse("null pointer", PQ_ERR_ARG);
    for (int j = 0; j < k; j++) {
        if (!exposures[j]) return refuse("null exposure pointer", PQ_ERR_ARG);
        in.x[j] = exposures[j];
    }
    in.h = holdings;
    in.b = benchmark_holdings;
    in.K = k;
    in.u = specific_return;
    in.r = next_return;
    in.d = dims_of(b);
    const Dims d = in.d;
    const int P = benchmark_holdings ? 3 : 1, G = n_groups, M = k + G, NQ = M + 3, NS = M + AT_TOTALS;
    const int64_t nblk = xs_nblk(d.n);
    if (!(nblk <= 65535 && S <= 0x7fffffffLL / 64 / (3 * NS))) return refuse("batch too large (n_series <= 16776960)", PQ_ERR_ARG);
    const uintptr_t plane = xw_plane_bytes(d), len = (uintptr_t)d.len;
    XwSpan ins[AT_MAX_K + 6], outs[7];
    int ni = 0, no = 0;
    ins[ni++] = xw_span(holdings, plane);
    if (benchmark_holdings) ins[ni++] = xw_span(benchmark_holdings, plane);
    for (int j = 0; j < k; j++) ins[ni++] = xw_span(in.x[j], plane);
    ins[ni++] = xw_span(specific_return, plane);
    if (next_return) ins[ni++] = xw_span(next_return, plane);
    ins[ni++] = xw_span(factor_return, (uintptr_t)M * (uintptr_t)fr_stride * 8);
    if (industry) ins[ni++] = xw_span(industry, (uintptr_t)d.n * (uintptr_t)(group_stride ? group_stride : 1) * 4);
    outs[no++] = xw_span(exposure_out, (uintptr_t)P * M * len * 8);
    outs[no++] = xw_span(contribution_out, (uintptr_t)P * M * len * 8);
    outs[no++] = xw_span(totals_out, (uintptr_t)P * AT_TOTALS * len * 8);
    outs[no++] = xw_span(n_out, (uintptr_t)3 * P * len * 4);
    outs[no++] = xw_span(summary_out, (uintptr_t)P * NS * RG_SUMMARY_COLS * 8);
    if (S > 0) {
        outs[no++] = xw_span(period_sum_out, (uintptr_t)P * NS * (uintptr_t)S * 8);
        outs[no++] = xw_span(period_days_out, (uintptr_t)P * (uintptr_t)S * 4);
    }
    PQ_TRY(xw_no_overlap(outs, no, ins, ni, "pq_return_attribution: an output must not overlap an input",
                         "pq_return_attribution: the outputs must not overlap each other"));
    // workspace: block partials ps [nblk][P][NQ][len] (f64) | X [P][NQ][len] | block counts pc [nblk][3][P][len] (i32) | the bounds (i64)
    double *ps, *X;
    int32_t *pc;
    int64_t *bd;
    PQ_TRY(xs_ws_carve(ctx, what, [&](XsWs &w) {
        w.take(ps, (size_t)nblk * P * NQ * len).take(X, (size_t)P * NQ * len).take(pc, (size_t)nblk * 3 * P * len).take(bd, (size_t)(S > 0 ? S + 1 : 0));
    }));
    hipStream_t st = ctx->stream;
    if (S > 0) {
        PQ_HIP_TRY(hipMemcpyAsync(bd, period_bounds, (size_t)(S + 1) * 8, hipMemcpyHostToDevice, st));
        PQ_HIP_TRY(hipStreamSynchronize(st));                  // the caller's array may go away with this call
    }
    if (P == 3) PQ_TRY(at_pass<3>(ctx, in, nblk, ps, pc));
    else PQ_TRY(at_pass<1>(ctx, in, nblk, ps, pc));
    const dim3 gd((unsigned)((d.len + 63) / 64));
    hipLaunchKernelGGL(at_sum_kernel, dim3(gd.x, (unsigned)(P * NQ)), dim3(64), 0, st, (const double *)ps, (const int32_t *)pc, nblk, d.len,
                       P * NQ, 3 * P, X, n_out);
    hipLaunchKernelGGL(at_day_kernel, dim3(gd.x, (unsigned)P), dim3(64), 0, st, (const double *)X, (const int32_t *)n_out, factor_return,
                       fr_stride, d.len, (int)k, G, P, next_return ? 1 : 0, exposure_out, contribution_out, totals_out);
    hipLaunchKernelGGL(at_summary_kernel, dim3((unsigned)(P * NS)), dim3(64), 0, st, (const double *)contribution_out,
                       (const double *)totals_out, d.len, M, summary_out);
    if (S > 0) {
        const int64_t cells = (int64_t)P * NS * S;
        hipLaunchKernelGGL(at_period_kernel, dim3((unsigned)((cells + 63) / 64)), dim3(64), 0, st, (const double *)contribution_out,
                           (const double *)totals_out, d.len, M, P, (const int64_t *)bd, S, period_sum_out, period_days_out);
    }
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
