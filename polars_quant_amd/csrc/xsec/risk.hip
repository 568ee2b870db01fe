// xsec/risk.hip -- the risk model that consumes the three series of Factor.pure_factor_return (D-32): the exponentially weighted
// covariance of the factor (and industry) returns, the specific variance of every symbol, and the predicted risk of a portfolio from
// the two (Factor.risk_model / Factor.portfolio_risk); decision D-33, DESIGN.md section 2.
//
// Everything is evaluated on `count` as-of days t_d = day0 + d * step only, and the model of day t reads rows t-w+1 .. t and nothing later.
//  rk_wcov:    the one arithmetic.  Over the entries k of two windows a, b (oldest to newest) whose day is >= 0, whose a[k] and b[k] are
//              both non-null and finite and whose weight om[k] > 0, ascending from 0.0 with every product rounded before it is added:
//              W = sum om, W2 = sum (om om), Sa = sum (om a), Sb = sum (om b), ma = Sa / W, mb = Sb / W, C = sum (om (a - ma)) (b - mb);
//              cov = C / (W - W2 / W) (unbiased) or C / W.  NULL below min_periods entries (below 2 when unbiased), where the
//              denominator is not > 0 and where the result is NaN.  With every weight 1.0 and a full window each step is
//              ts_pair_kernel<TSP_COV>'s (tsops.hip).
//  windowed:   xsec_window.h's staging -- a tile of days and a halo of w - 1 earlier ones in LDS, loads coalesced along days -- but not
//              xw_walk: a row here tests every entry itself, so there is no last-unusable scan, and thread i of a tile evaluates the
//              tile's i-th AS-OF day, which packs the live lanes of a step > 1 into the leading waves; a tile without an as-of day is
//              skipped before it stages anything.  A tile is XW_TILE days at step 1 and rk_tile_days(step, w) days beyond: as many as
//              hold XW_TILE as-of days, within RK_STAGE staged entries.  Days outside [0, len) are staged as NULL.  The weights are
//              staged once per workgroup; every lane reads the same word of them at each step (a broadcast).
//  cov:        one workgroup per (series j, chunk of RK_LCHUNK columns l <= j, tile): column j is staged once, then each column l of the
//              chunk is staged beside it and the pair evaluated once, stored to [d][j][l] and [d][l][j]; l = j runs on column j's own
//              staging.  (One workgroup per (j, tile) left the call waiting for row M - 1's M evaluations in series.)
//  specific:   the same kernel with the diagonal alone, stored [s][out_stride] by as-of day.
//  portfolio:  1. 64 lanes = 64 consecutive as-of days, blockIdx.y = the block of 256 symbols (regress.hip / wls.hip pass 1): the held and
//              uncovered counts, and the sums h x_j (j < K), h per industry and (h h) s^2, kept [row][lane] in LDS; block partials to the
//              context workspace.  2. one thread per (day, row) adds the partials in ascending block order from 0.0 (D-12's blocked
//              sum).  3. one thread per (day, row j): v_j = sum_l cov[j][l] X[l] over the rows with X[l] != 0, c_j = X[j] v_j.  4. one
//              thread per day: the NULL rules, the sums and the square root.
// The operation order is D-33's, restated in tests/xsec_risk_ref.py.
#include "xsec_window.h"

namespace {

constexpr int RK_MAX_SERIES = PQ_RISK_MAX_SERIES;
constexpr int RK_MAX_K = PQ_REGRESS_MAX_K;
static_assert(RK_MAX_SERIES == RK_MAX_K + XS_MAX_GROUPS, "the rows of D-32's coef block");

constexpr int RK_LCHUNK = 8;                                    // columns l per workgroup of the covariance: column j is restaged once per 8
constexpr int RK_STAGE = 2048;                                  // staged entries per column at a step > 1 (16 KiB), XW_STAGE at most at step 1

// days per tile: XW_TILE as-of days' worth, as far as the tile and its halo stay within RK_STAGE entries, and never below XW_TILE.  With
// XW_TILE days at every step a workgroup at step 20 would stage 256 + w - 1 entries per column for 13 live lanes.
inline int rk_tile_days(int64_t step, int w) {
    const int64_t want = (int64_t)XW_TILE * step, room = RK_STAGE - (w - 1);
    const int64_t td = want < room ? want : room;
    return td > XW_TILE ? (int)td : XW_TILE;
}

struct RkCov { double cov; int32_t n; };

__device__ __forceinline__ RkCov rk_wcov(const double *a, const double *b, const double *om, int w, int minp, bool unbiased) {
    double W = 0.0, W2 = 0.0, Sa = 0.0, Sb = 0.0;
    int32_t n = 0;
    for (int k = 0; k < w; k++) {
        const double av = a[k], bv = b[k], o = om[k];
        if (xs_valid(av) && xs_valid(bv) && o > 0.0) {
            W += o;
            W2 += o * o;
            Sa += o * av;
            Sb += o * bv;
            n++;
        }
    }
    RkCov r{pq_null(), n};
    if (n < minp || (unbiased && n < 2)) return r;
    const double ma = Sa / W, mb = Sb / W;
    double Cs = 0.0;
    for (int k = 0; k < w; k++) {
        const double av = a[k], bv = b[k], o = om[k];
        if (xs_valid(av) && xs_valid(bv) && o > 0.0) Cs += (o * (av - ma)) * (bv - mb);
    }
    const double den = unbiased ? W - W2 / W : W;
    if (!(den > 0.0)) return r;
    const double c = Cs / den;
    if (c == c) r.cov = c;
    return r;
}

// the as-of days d_lo .. d_lo + cnt - 1 (cnt <= XW_TILE, as td <= XW_TILE * step) that fall on the days [t0, t0 + td) of tile `tile`
struct RkTile { int64_t t0, d_lo; int cnt; };
__device__ __forceinline__ int64_t rk_days_before(const RkDays &a, int64_t t) {   // as-of days (of any d >= 0) on a day < t
    return t > a.day0 ? (t - a.day0 + a.step - 1) / a.step : 0;
}
__device__ __forceinline__ RkTile rk_tile(const RkDays &a, int64_t tile, int td) {
    const int64_t t0 = tile * td, lo = rk_days_before(a, t0), hi0 = rk_days_before(a, t0 + td), hi = hi0 < a.count ? hi0 : a.count;
    return RkTile{t0, lo, hi > lo ? (int)(hi - lo) : 0};
}

// val[0 .. td + w - 1) <- the days t0 - (w - 1) .. t0 + td - 1 of one series, NULL outside [0, len)
__device__ __forceinline__ void rk_stage(double *val, const double *col, int64_t len, int64_t t0, int td, int w) {
    const int Mw = td + w - 1;
    for (int l = threadIdx.x; l < Mw; l += XW_TILE) {
        const int64_t g = t0 - (w - 1) + l;
        val[l] = g >= 0 && g < len ? col[g] : pq_null();
    }
}

// DIAG = false: out[d][j][l] = out[d][l][j] = rk_wcov(f_j, f_l) for l <= j, n_out[d][j] the n of the diagonal; LDS va[Mw], vb[Mw], om[w],
//               Mw = td + w - 1.
// DIAG = true:  out[j * out_stride + d] = rk_wcov(f_j, f_j), n_out on the same layout; LDS va[Mw], om[w].
template <bool DIAG>
__global__ __launch_bounds__(XW_TILE) void rk_cov_kernel(const double *f, Dims d, const double *omega, int w, int minp, int unbiased, RkDays a,
                                                         int td, int64_t tile0, int64_t tiles, int64_t chunks, int64_t total, double *out,
                                                         int64_t out_stride, int32_t *n_out) {
    extern __shared__ double rk_lds[];
    const int tid = threadIdx.x, Mw = td + w - 1;
    double *va = rk_lds, *vb = DIAG ? va : va + Mw, *om = vb + Mw;
    for (int k = tid; k < w; k += XW_TILE) om[k] = omega[k];
    const int64_t M = d.n;
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        // job = (j, chunk c of the columns, tile); the chunks are laid out for row M - 1, a row j has those with c * RK_LCHUNK <= j
        const int64_t j = job / (chunks * tiles), rem = job - j * chunks * tiles, c = rem / tiles;
        const int64_t l_lo = DIAG ? j : c * RK_LCHUNK, l_hi = DIAG || l_lo + RK_LCHUNK - 1 > j ? j : l_lo + RK_LCHUNK - 1;
        if (l_lo > j) continue;                                 // (the same for every thread, as is the next)
        const RkTile tl = rk_tile(a, tile0 + (rem - c * tiles), td);
        if (tl.cnt == 0) continue;                              // no as-of day, no row work
        __syncthreads();                                        // the rows of the job before are done with va
        rk_stage(va, f + j * d.stride, d.len, tl.t0, td, w);
        const int64_t dd = tl.d_lo + tid;
        const bool live = tid < tl.cnt;
        const int off = live ? (int)(a.day0 + dd * a.step - tl.t0) : 0;   // the row's window is entries [off, off + w)
        for (int64_t l = l_lo; l <= l_hi; l++) {
            if (!DIAG && l > l_lo) __syncthreads();             // the rows of column l - 1 are done with vb
            if (l < j) rk_stage(vb, f + l * d.stride, d.len, tl.t0, td, w);
            __syncthreads();
            if (live) {
                const RkCov r = rk_wcov(va + off, (l < j ? vb : va) + off, om, w, minp, unbiased != 0);
                if (DIAG) {
                    out[j * out_stride + dd] = r.cov;
                    if (n_out) n_out[j * out_stride + dd] = r.n;
                } else {
                    out[(dd * M + j) * M + l] = r.cov;
                    out[(dd * M + l) * M + j] = r.cov;
                    if (l == j && n_out) n_out[dd * M + j] = r.n;
                }
            }
        }
    }
}

// ---------------------------------------------------------------- portfolio
struct RkPf {
    const double *h, *x[RK_MAX_K];
    int32_t K;
    XsGroups grp;          // null codes: every symbol in group 0 (G = 1)
    const double *sv;      // [n_series][sv_stride], by as-of day
    int64_t sv_stride;
    Dims d;
    RkDays a;
};

// accumulators [K + G + 1][lane] in LDS: X_0 .. X_{K-1}, the G industry rows, the specific sum; block partials ps[block][K + G + 1][count]
// and the counts pc[block][2][count] (held, uncovered)
__global__ __launch_bounds__(64) void rk_pf_pass1_kernel(RkPf in, double *ps, int32_t *pc) {
    extern __shared__ double rk_acc[];
    const int lane = threadIdx.x;
    const int64_t D = in.a.count, dd = (int64_t)blockIdx.x * 64 + lane;
    if (dd >= D) return;
    const int K = in.K, G = in.grp.G, NQ = K + G + 1;
    for (int q = 0; q < NQ; q++) rk_acc[q * 64 + lane] = 0.0;
    const int64_t t = in.a.day0 + dd * in.a.step;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < in.d.n ? s_lo + XS_BLOCK : in.d.n;
    int32_t nh = 0, nu = 0;
    for (int64_t s = s_lo; s < s_hi; s++) {
        const int64_t o = s * in.d.stride + t;
        const double h = in.h[o], s2 = in.sv[s * in.sv_stride + dd];
        const int32_t g = in.grp.codes ? in.grp.codes[in.grp.stride ? s * in.grp.stride + t : s] : 0;   // written out, as the test below
        double x[RK_MAX_K];
#pragma unroll
        for (int j = 0; j < RK_MAX_K; j++) x[j] = j < K ? in.x[j][o] : 0.0;
        if (!(xs_valid(h) && h != 0.0)) continue;
        nh++;
        bool covered = s2 >= 0.0 && g >= 0 && g < G;            // a NULL (or NaN) variance fails the compare; g: see XsGroups
#pragma unroll
        for (int j = 0; j < RK_MAX_K; j++) covered = covered && xs_valid(x[j]);
        if (!covered) { nu++; continue; }
#pragma unroll
        for (int j = 0; j < RK_MAX_K; j++)
            if (j < K) rk_acc[j * 64 + lane] += h * x[j];
        rk_acc[(K + g) * 64 + lane] += h;
        rk_acc[(K + G) * 64 + lane] += (h * h) * s2;
    }
    for (int q = 0; q < NQ; q++) ps[((int64_t)blockIdx.y * NQ + q) * D + dd] = rk_acc[q * 64 + lane];
    pc[((int64_t)blockIdx.y * 2 + 0) * D + dd] = nh;
    pc[((int64_t)blockIdx.y * 2 + 1) * D + dd] = nu;
}

// one thread per (as-of day, row q of the K + G + 1): the block sums in ascending block order from 0.0 -> X[q][count]; row 0's threads
// also add the counts -> n_out[2][count]
__global__ __launch_bounds__(64) void rk_pf_sum_kernel(const double *ps, const int32_t *pc, int64_t nblk, int64_t D, int NQ, double *X,
                                                       int32_t *n_out) {
    const int64_t dd = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int q = blockIdx.y;
    if (dd >= D) return;
    double s = 0.0;
    for (int64_t k = 0; k < nblk; k++) s += ps[(k * NQ + q) * D + dd];
    X[(int64_t)q * D + dd] = s;
    if (q == 0) {
        int32_t nh = 0, nu = 0;
        for (int64_t k = 0; k < nblk; k++) {
            nh += pc[(k * 2 + 0) * D + dd];
            nu += pc[(k * 2 + 1) * D + dd];
        }
        n_out[dd] = nh;
        n_out[D + dd] = nu;
    }
}

// one thread per (as-of day, row j of the M): c_j -> cw[j][count]; NULL where a covariance that the sum needs is NULL
__global__ __launch_bounds__(64) void rk_pf_contrib_kernel(const double *cov, const double *X, int64_t D, int M, double *cw) {
    const int64_t dd = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y;
    if (dd >= D) return;
    const double xj = X[(int64_t)j * D + dd];
    double c = 0.0;
    if (xj != 0.0) {
        const double *row = cov + (dd * M + j) * M;
        double v = 0.0;
        bool missing = false;
        for (int l = 0; l < M; l++) {
            const double xl = X[(int64_t)l * D + dd];
            if (xl != 0.0) {
                const double cv = row[l];
                missing = missing || pq_isnull(cv);
                v += cv * xl;
            }
        }
        c = missing ? pq_null() : xj * v;
    }
    cw[(int64_t)j * D + dd] = c;
}

// one thread per as-of day: the day's NULL rules, factor_var = sum_j c_j (ascending from 0.0), total and volatility
__global__ __launch_bounds__(64) void rk_pf_final_kernel(const double *X, const double *cw, const int32_t *n_out, int64_t D, int M,
                                                         double *exposure, double *contribution, double *risk) {
    const int64_t dd = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (dd >= D) return;
    bool nul = n_out[dd] == 0 || n_out[D + dd] > 0;
    double fv = 0.0;
    for (int j = 0; j < M; j++) {
        const double c = cw[(int64_t)j * D + dd];
        nul = nul || pq_isnull(c);
        fv += c;
    }
    for (int j = 0; j < M; j++) {
        const int64_t o = (int64_t)j * D + dd;
        exposure[o] = nul ? pq_null() : rk_nan_null(X[o]);
        contribution[o] = nul ? pq_null() : rk_nan_null(cw[o]);
    }
    const double sp = X[(int64_t)M * D + dd], tot = fv + sp;
    risk[dd] = nul ? pq_null() : rk_nan_null(fv);
    risk[D + dd] = nul ? pq_null() : rk_nan_null(sp);
    risk[2 * D + dd] = nul ? pq_null() : rk_nan_null(tot);
    risk[3 * D + dd] = nul || tot < 0.0 ? pq_null() : rk_nan_null(sqrt(tot));
}

// ---------------------------------------------------------------- host (the as-of days: rk_days, xsec_dev.h)
template <bool DIAG>
pq_status rk_windowed(const char *what, pq_ctx *ctx, const pq_batch *b, const double *f, const double *omega, int64_t window,
                      int64_t min_periods, int32_t unbiased, int64_t day0, int64_t step, int64_t count, double *out, int64_t out_stride,
                      int32_t *n_out) {
    char msg[256];
    auto refuse = [&](const char *text, pq_status s) { snprintf(msg, sizeof msg, "%s: %s", what, text); pq_set_error("%s", msg); return s; };
    PQ_TRY(pq_check(ctx, b));
    if (window < 1 || window > XW_MAX_W) return refuse("window must be in [1, 1024]", PQ_ERR_ARG);
    if (min_periods < 1 || min_periods > window) return refuse("min_periods must be in [1, window]", PQ_ERR_ARG);
    if (unbiased && min_periods < 2) return refuse("the unbiased estimate needs min_periods >= 2", PQ_ERR_ARG);
    if (!DIAG && b->n_series > RK_MAX_SERIES) return refuse("at most 264 series", PQ_ERR_ARG);
    RkDays a;
    PQ_TRY(rk_days(what, b->len, day0, step, count, &a));
    if (DIAG && out_stride < count) return refuse("out_stride must be >= count", PQ_ERR_ARG);
    const bool empty = count == 0 || b->len == 0 || b->n_series == 0;
    if (!empty && !(f && omega && out)) return refuse("null pointer", PQ_ERR_ARG);
    XwGrid g;
    snprintf(msg, sizeof msg, "%s cannot be recorded into a suite", what);
    char ragged[256];
    snprintf(ragged, sizeof ragged, "%s (the series are [n_series][stride]): ragged batches are not supported", what);
    PQ_TRY(xw_prepare(ctx, b, msg, ragged, PQ_ERR_UNSUPPORTED, &g));
    if (empty) return PQ_OK;
    const Dims d = g.d;
    const uintptr_t cells = DIAG ? (uintptr_t)d.n * (uintptr_t)out_stride : (uintptr_t)count * (uintptr_t)d.n * (uintptr_t)d.n,
                    ncells = DIAG ? cells : (uintptr_t)count * (uintptr_t)d.n;
    const XwSpan ins[] = {xw_span(f, xw_plane_bytes(d)), xw_span(omega, (uintptr_t)window * 8)};
    const XwSpan outs[] = {xw_span(out, cells * 8), xw_span(n_out, ncells * 4)};
    char vs_in[256], vs_out[256];
    snprintf(vs_in, sizeof vs_in, "%s: an output must not overlap the series or the weights", what);
    snprintf(vs_out, sizeof vs_out, "%s: the outputs must not overlap each other", what);
    PQ_TRY(xw_no_overlap(outs, n_out ? 2 : 1, ins, 2, vs_in, vs_out));
    const int w = (int)window, td = rk_tile_days(a.step, w);
    const int64_t tile0 = a.day0 / td, tiles = (a.day0 + (a.count - 1) * a.step) / td - tile0 + 1,
                  chunks = DIAG ? 1 : (d.n + RK_LCHUNK - 1) / RK_LCHUNK, total = d.n * chunks * tiles;
    const dim3 grid((unsigned)(total < (int64_t)1 << 20 ? total : (int64_t)1 << 20));
    const size_t Mw = (size_t)(td + w - 1), lds = ((DIAG ? 1 : 2) * Mw + (size_t)w) * 8;
    hipLaunchKernelGGL(rk_cov_kernel<DIAG>, grid, dim3(XW_TILE), lds, ctx->stream, f, d, omega, w, (int)min_periods, (int)unbiased, a, td, tile0,
                       tiles, chunks, total, out, out_stride, n_out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_risk_factor_cov(pq_ctx *ctx, const pq_batch *b, const double *f, const double *omega, int64_t window, int64_t min_periods,
                             int32_t unbiased, int64_t day0, int64_t step, int64_t count, double *cov_out, int32_t *n_out) {
    return rk_windowed<false>("pq_risk_factor_cov", ctx, b, f, omega, window, min_periods, unbiased, day0, step, count, cov_out, 0, n_out);
}

pq_status pq_risk_specific_var(pq_ctx *ctx, const pq_batch *b, const double *x, const double *omega, int64_t window, int64_t min_periods,
                               int32_t unbiased, int64_t day0, int64_t step, int64_t count, double *var_out, int64_t out_stride,
                               int32_t *n_out) {
    return rk_windowed<true>("pq_risk_specific_var", ctx, b, x, omega, window, min_periods, unbiased, day0, step, count, var_out, out_stride,
                             n_out);
}

pq_status pq_risk_portfolio(pq_ctx *ctx, const pq_batch *b, const double *holdings, const double *const *exposures, int32_t k,
                            const int32_t *industry, int64_t group_stride, int32_t n_groups, const double *cov, const double *specific_var,
                            int64_t sv_stride, int64_t day0, int64_t step, int64_t count, double *exposure_out, double *contribution_out,
                            double *risk_out, int32_t *n_out) {
    const char *what = "pq_risk_portfolio";
    PQ_TRY(pq_check(ctx, b));
    if (k < 0 || k > RK_MAX_K) { pq_set_error("%s: k must be in [0, 8]", what); return PQ_ERR_ARG; }
    RkPf in{};
    PQ_TRY(xs_groups_arg(what, b, industry, group_stride, n_groups, XsGroupsPolicy{XS_G_ALWAYS, "n_groups", "industry"}, &in.grp));
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", what); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", what); return PQ_ERR_UNSUPPORTED; }
    PQ_TRY(xs_groups_stride(what, b, industry != nullptr, group_stride));
    PQ_TRY(rk_days(what, b->len, day0, step, count, &in.a));
    if (sv_stride < count) { pq_set_error("%s: sv_stride must be >= count", what); return PQ_ERR_ARG; }
    if (count == 0) return PQ_OK;
    if (!(cov && exposure_out && contribution_out && risk_out && n_out)) { pq_set_error("%s: null pointer", what); return PQ_ERR_ARG; }
    if (b->n_series != 0 && (!holdings || !specific_var || (k > 0 && !exposures))) { pq_set_error("%s: null pointer", what); return PQ_ERR_ARG; }
    for (int j = 0; j < k && b->n_series != 0; j++) {
        if (!exposures[j]) { pq_set_error("%s: null exposure pointer", what); return PQ_ERR_ARG; }
        in.x[j] = exposures[j];
    }
    in.h = holdings;
    in.K = k;
    in.sv = specific_var;
    in.sv_stride = sv_stride;
    in.d = dims_of(b);
    const int M = k + n_groups, NQ = M + 1;
    const int64_t D = count, nblk = xs_nblk(in.d.n);
    // workspace: block partials ps [nblk][NQ][D] (f64) | X [NQ][D] | cw [M][D] | block counts pc [nblk][2][D] (i32)
    double *ps, *X, *cw;
    int32_t *pc;
    PQ_TRY(xs_ws_carve(ctx, what, [&](XsWs &w) {
        w.take(ps, (size_t)nblk * NQ * D).take(X, (size_t)NQ * D).take(cw, (size_t)M * D).take(pc, (size_t)nblk * 2 * D);
    }));
    const dim3 gd((unsigned)((D + 63) / 64)), gp(gd.x, (unsigned)nblk), gq(gd.x, (unsigned)NQ), gm(gd.x, (unsigned)M);
    const size_t lds = (size_t)NQ * 64 * 8;                     // at most 265 rows: 132.5 KiB of the CU's 160
    hipStream_t st = ctx->stream;
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)rk_pf_pass1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(rk_pf_pass1_kernel, gp, dim3(64), lds, st, in, ps, pc);
    hipLaunchKernelGGL(rk_pf_sum_kernel, gq, dim3(64), 0, st, (const double *)ps, (const int32_t *)pc, nblk, D, NQ, X, n_out);
    hipLaunchKernelGGL(rk_pf_contrib_kernel, gm, dim3(64), 0, st, cov, (const double *)X, D, M, cw);
    hipLaunchKernelGGL(rk_pf_final_kernel, gd, dim3(64), 0, st, (const double *)X, (const double *)cw, (const int32_t *)n_out, D, M,
                       exposure_out, contribution_out, risk_out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
