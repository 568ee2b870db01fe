// portfolio/weights.hip -- decision D-35: the backtest of GIVEN target weights -- signed, not normalised, NULL outside
// the day's universe, the remainder 1 - sum w in cash -- for up to eight portfolios a call: pq_factor_weights.  The definitions are in
// include/pq_hip.h; what is not said there is D-27's (portfolio_dev.h: the usable test, the held price, the days / seg tables, the chain).
//
// D-27's shape: the growth G(p, t) = c_k + sum over the members of w (h(s, t) / price[s][d_k]) is one pass of cross-sectional sums in
// D-12's order with the lanes of a wave on consecutive days, and the price word and the held-price walk of a (symbol, day) serve all P
// portfolios -- P separate calls would read the price plane P times.  Around it the light passes on the rebalance days (net, gross and the
// counts before it, the turnover after it), the chain per portfolio, the curve with the first day that is not > 0, and, when asked, the
// drifted holdings [n][stride] of one portfolio.
//
// Workspace: days (i32 [R]) | seg (i32 [len]) | block partials of net and gross (f64 [nblk][2][P][R]) and of the counts (i32 [nblk][3][P][R])
// | block partials of L (f64 [nblk][P][len]) | G (f64 [P][len]) | block partials of the turnover (f64 [nblk][P][R]) | B (f64 [P][R])
#include "../xsec/xsec_window.h"   // xw_no_overlap
#include "portfolio_dev.h"

namespace {

constexpr int PW_MAX = PQ_WEIGHTS_MAX_PORTFOLIOS;
constexpr int PW_NO_DAY = 0x7fffffff;   // first_nonpositive while the curve runs: above every day

struct PwArgs {
    const double *w[PW_MAX];  // per portfolio [n][ws], column k = rebalance k
    const double *price;      // [n][stride]
    const int32_t *days;      // [R], ascending
    const int32_t *seg;       // [len]: PfArgs::seg
    const double *net;        // [P][R]: sum of the members' weights
    const double *G;          // [P][len]
    Dims d;
    int64_t R, ws;
    int P;
};

// a weight that is held: non-null, finite and not 0 (a member also needs a usable price on d_k)
__device__ __forceinline__ bool pw_target(double w) { return xs_valid(w) && w != 0.0; }

// rebalance pass: one thread per (rebalance k, block of 256 symbols) -> per portfolio the block's net and gross weight of the members and
// the three counts (long, short, dropped).  The price of d_k is read once per symbol for all portfolios.
template <int PC> __global__ __launch_bounds__(64) void pw_rebalance_partial_kernel(PwArgs q, double *psum, int32_t *pcnt) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= q.R) return;
    const int64_t dk = q.days[k];
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double net[PC], gross[PC];
    int nl[PC], ns[PC], nd[PC];
#pragma unroll
    for (int p = 0; p < PC; p++) { net[p] = 0.0; gross[p] = 0.0; nl[p] = 0; ns[p] = 0; nd[p] = 0; }
    constexpr int B = PC <= 2 ? 8 : 2;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double p0[B], w[B][PC];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int64_t s = s0 + j < s_hi ? s0 + j : s_hi - 1;
            p0[j] = q.price[s * q.d.stride + dk];
#pragma unroll
            for (int p = 0; p < PC; p++) w[j][p] = p < q.P ? q.w[p][s * q.ws + k] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            const bool held = pf_usable(p0[j]);
#pragma unroll
            for (int p = 0; p < PC; p++) {
                if (!pw_target(w[j][p])) continue;
                if (held) {
                    net[p] += w[j][p];
                    gross[p] += fabs(w[j][p]);
                    if (w[j][p] > 0.0) nl[p] += 1; else ns[p] += 1;
                } else nd[p] += 1;
            }
        }
    }
    const int64_t pr = (int64_t)q.P * q.R;
#pragma unroll
    for (int p = 0; p < PC; p++)
        if (p < q.P) {
            const int64_t o = p * q.R + k;
            psum[(int64_t)blockIdx.y * 2 * pr + o] = net[p];
            psum[(int64_t)blockIdx.y * 2 * pr + pr + o] = gross[p];
            pcnt[(int64_t)blockIdx.y * 3 * pr + o] = nl[p];
            pcnt[(int64_t)blockIdx.y * 3 * pr + pr + o] = ns[p];
            pcnt[(int64_t)blockIdx.y * 3 * pr + 2 * pr + o] = nd[p];
        }
}

// one thread per cell: the block partials in ascending block order, from 0.0; fcells f64 cells and icells i32 cells (either may be 0)
__global__ __launch_bounds__(64) void pw_sum_blocks_kernel(const double *psum, int64_t fcells, const int32_t *pcnt, int64_t icells, int64_t nblk,
                                                           double *sum, int32_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i < fcells) {
        double s = 0.0;
        for (int64_t b = 0; b < nblk; b++) s += psum[b * fcells + i];
        sum[i] = s;
    }
    if (i < icells) {
        int32_t c = 0;
        for (int64_t b = 0; b < nblk; b++) c += pcnt[b * icells + i];
        cnt[i] = c;
    }
}

// growth pass, the hot one: one thread per (day, block of 256 symbols), the 64 lanes of a wave on 64 consecutive days -- a price load is 512
// contiguous bytes, the base price and the weights on d_k are one address for all the lanes of a segment.  Ascending symbols, the loads of B
// symbols issued before the first is used; the ratio h / price[s][d_k] is formed once per (symbol, day) and multiplied into the PC >= P
// accumulators, which sit in registers under static indices.
template <int PC> __global__ __launch_bounds__(64) void pw_growth_partial_kernel(PwArgs q, double *part) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= q.d.len) return;
    const int64_t k = q.seg[t];
    if (k < 0) return;
    const int64_t dk = q.days[k];
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double sum[PC];
#pragma unroll
    for (int p = 0; p < PC; p++) sum[p] = 0.0;
    constexpr int B = PC <= 2 ? 8 : 4;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double pt[B], p0[B], w[B][PC];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int64_t s = s0 + j < s_hi ? s0 + j : s_hi - 1;
            pt[j] = q.price[s * q.d.stride + t];
            p0[j] = q.price[s * q.d.stride + dk];
#pragma unroll
            for (int p = 0; p < PC; p++) w[j][p] = p < q.P ? q.w[p][s * q.ws + k] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            if (!pf_usable(p0[j])) continue;
            const double ratio = pf_held(q.price + (s0 + j) * q.d.stride, pt[j], t, dk) / p0[j];
#pragma unroll
            for (int p = 0; p < PC; p++)
                if (pw_target(w[j][p])) sum[p] += w[j][p] * ratio;
        }
    }
#pragma unroll
    for (int p = 0; p < PC; p++)
        if (p < q.P) part[((int64_t)blockIdx.y * q.P + p) * q.d.len + t] = sum[p];
}

// one thread per (portfolio, day): G = c_k + L, c_k = 1.0 - W_k the cash, L the block partials in ascending block order from 0.0; 1.0 up to d_0
__global__ __launch_bounds__(64) void pw_growth_combine_kernel(PwArgs q, const double *part, int64_t nblk, double *Gout) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x, cells = (int64_t)q.P * q.d.len;
    if (i >= cells) return;
    const int64_t p = i / q.d.len, t = i - p * q.d.len, k = q.seg[t];
    double g = 1.0;
    if (k >= 0) {
        double L = 0.0;
        for (int64_t b = 0; b < nblk; b++) L += part[b * cells + i];
        g = (1.0 - q.net[p * q.R + k]) + L;
    }
    Gout[i] = g;
}

// turnover pass: one thread per (rebalance k, block of 256 symbols) -> per portfolio the block's sum of |w_new - w_old|, w_old the weights of
// rebalance k - 1 drifted to d_k (0 at k = 0 and for a symbol that was not held), w_new those of rebalance k (0 for a non-member).  The two
// prices and the held-price walk are done once per symbol.
template <int PC> __global__ __launch_bounds__(64) void pw_turnover_partial_kernel(PwArgs q, double *part) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= q.R) return;
    const int64_t dk = q.days[k], dp = k > 0 ? q.days[k - 1] : dk, ko = k > 0 ? k - 1 : k;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double tau[PC], Gd[PC];
#pragma unroll
    for (int p = 0; p < PC; p++) { tau[p] = 0.0; Gd[p] = p < q.P ? q.G[(int64_t)p * q.d.len + dk] : 1.0; }
    constexpr int B = PC <= 2 ? 4 : 2;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double pn[B], po[B], wn[B][PC], wo[B][PC];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int64_t s = s0 + j < s_hi ? s0 + j : s_hi - 1;
            pn[j] = q.price[s * q.d.stride + dk];
            po[j] = q.price[s * q.d.stride + dp];
#pragma unroll
            for (int p = 0; p < PC; p++) {
                wn[j][p] = p < q.P ? q.w[p][s * q.ws + k] : 0.0;
                wo[j][p] = p < q.P ? q.w[p][s * q.ws + ko] : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            const bool m_new = pf_usable(pn[j]), m_old = k > 0 && pf_usable(po[j]);
            double ratio = 0.0;
            if (m_old) ratio = pf_held(q.price + (s0 + j) * q.d.stride, pn[j], dk, dp) / po[j];
#pragma unroll
            for (int p = 0; p < PC; p++) {
                const double w_new = m_new && pw_target(wn[j][p]) ? wn[j][p] : 0.0;
                double w_old = 0.0;
                if (m_old && pw_target(wo[j][p])) w_old = (wo[j][p] * ratio) / Gd[p];
                tau[p] += fabs(w_new - w_old);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < PC; p++)
        if (p < q.P) part[((int64_t)blockIdx.y * q.P + p) * q.R + k] = tau[p];
}

// first_nonpositive: PW_NO_DAY before the curve (INIT), and -1 where the curve left it there
template <bool INIT> __global__ __launch_bounds__(64) void pw_first_kernel(int32_t *first, int P) {
    const int p = threadIdx.x;
    if (p >= P) return;
    if (INIT) first[p] = PW_NO_DAY;
    else if (first[p] == PW_NO_DAY) first[p] = -1;
}

// one thread per (portfolio, day): pf_curve_kernel's value, and the smallest day whose value is not > 0 (<= 0 or NaN) by an integer minimum
__global__ __launch_bounds__(64) void pw_curve_kernel(PwArgs q, const double *Bv, double capital, double *value, int32_t *first) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (int64_t)q.P * q.d.len) return;
    const int64_t p = i / q.d.len, t = i - p * q.d.len, k = q.seg[t];
    double v;
    if (k < 0) v = (q.R > 0 && t == q.days[0]) ? Bv[p * q.R] : capital;
    else if (k + 1 < q.R && t == q.days[k + 1]) v = Bv[p * q.R + k + 1];
    else v = Bv[p * q.R + k] * q.G[i];
    value[i] = v;
    if (!(v > 0.0)) atomicMin(&first[p], (int32_t)t);
}

// holdings pass: workgroup = (symbol, 256 consecutive days), coalesced along the days.  0.0 before d_0 and for a non-member, the weight itself
// on a rebalance day, the drifted weight (w (h / price[s][d_k])) / G(p, t) in between; reads the weights wp and the finished G row Gp of one portfolio.
__global__ __launch_bounds__(256) void pw_holdings_kernel(PwArgs q, const double *wp, const double *Gp, int64_t tiles, double *out) {
    const int64_t s = blockIdx.x / tiles, t = (blockIdx.x - s * tiles) * 256 + threadIdx.x;
    if (t >= q.d.len) return;
    const double *row = q.price + s * q.d.stride, *w = wp + s * q.ws;
    const int64_t k = q.seg[t];
    int64_t kr = -1;   // the rebalance that day t is, if any
    if (k < 0) kr = q.R > 0 && t == q.days[0] ? 0 : -1;
    else if (k + 1 < q.R && t == q.days[k + 1]) kr = k + 1;
    const double pt = row[t];
    double h = 0.0;
    if (kr >= 0) {
        const double wk = w[kr];
        if (pw_target(wk) && pf_usable(pt)) h = wk;
    } else if (k >= 0) {
        const int64_t dk = q.days[k];
        const double wk = w[k], p0 = row[dk];
        if (pw_target(wk) && pf_usable(p0)) h = (wk * (pf_held(row, pt, t, dk) / p0)) / Gp[t];
    }
    out[s * q.d.stride + t] = h;
}

#define PW_LAUNCH_P(kern, grid, ...)                                                                       \
    do {                                                                                                   \
        if (P <= 1) hipLaunchKernelGGL(kern<1>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);              \
        else if (P <= 2) hipLaunchKernelGGL(kern<2>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);         \
        else hipLaunchKernelGGL(kern<PW_MAX>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);                \
    } while (0)

} // namespace

extern "C" {

pq_status pq_factor_weights(pq_ctx *ctx, const pq_batch *b, const double *const *weights, int32_t n_portfolios, int64_t w_stride,
                            const double *price, const int32_t *rebalance_days, int64_t n_rebalance, double cost_rate, double initial_capital,
                            double *value, double *turnover, double *exposure, int32_t *count, int32_t *first_nonpositive,
                            int32_t holdings_of, double *holdings_out) {
    const char *what = "pq_factor_weights";
    auto refuse = [&](const char *text, pq_status s) { pq_set_error("%s: %s", what, text); return s; };
    PQ_TRY(pq_check(ctx, b));
    if (n_portfolios < 1 || n_portfolios > PW_MAX) return refuse("n_portfolios must be in [1, 8] (PQ_WEIGHTS_MAX_PORTFOLIOS)", PQ_ERR_ARG);
    if (n_rebalance < 0) return refuse("n_rebalance must not be negative", PQ_ERR_ARG);
    if (w_stride < n_rebalance) return refuse("w_stride must be >= n_rebalance", PQ_ERR_ARG);
    if (!(cost_rate >= 0.0 && cost_rate < 1.0)) return refuse("cost_rate must be in [0, 1)", PQ_ERR_ARG);
    if (!(initial_capital > 0.0 && initial_capital <= 1.7976931348623157e308))
        return refuse("initial_capital must be positive and finite", PQ_ERR_ARG);
    if (holdings_of < -1 || holdings_of >= n_portfolios) return refuse("holdings_of must be -1 or a portfolio index", PQ_ERR_ARG);
    if ((holdings_of >= 0) != (holdings_out != nullptr)) return refuse("holdings_of and holdings_out go together", PQ_ERR_ARG);
    if (ctx->rec) return refuse("cannot be recorded into a suite", PQ_ERR_UNSUPPORTED);
    if (b->offsets) return refuse("ragged batches are not supported (a cross-section needs every symbol on every day)", PQ_ERR_UNSUPPORTED);
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int64_t R = n_rebalance, nblk = xs_nblk(d.n), tiles = (d.len + 255) / 256;
    const int P = n_portfolios;
    if (!(weights && price && value && first_nonpositive && (R == 0 || (rebalance_days && turnover && exposure && count))))
        return refuse("null pointer", PQ_ERR_ARG);
    for (int p = 0; p < P; p++)
        if (!weights[p]) return refuse("null weights pointer", PQ_ERR_ARG);
    if (!(d.len <= 0x7fffffffLL && nblk <= 65535 && (holdings_of < 0 || d.n <= 0x7fffffffLL / tiles)))
        return refuse("batch too large (len < 2^31, n_series <= 16776960, n_series * ceil(len / 256) < 2^31 with holdings)", PQ_ERR_ARG);
    PQ_TRY(pf_check_days(what, rebalance_days, R, 0, "0", d.len));
    const size_t len = (size_t)d.len, pr = (size_t)P * (size_t)R, pt = (size_t)P * len;
    XwSpan ins[PW_MAX + 1], outs[6];
    int ni = 0, no = 0;
    for (int p = 0; p < P; p++) ins[ni++] = xw_span(weights[p], (uintptr_t)d.n * (uintptr_t)w_stride * 8);
    ins[ni++] = xw_span(price, xw_plane_bytes(d));
    outs[no++] = xw_span(value, (uintptr_t)pt * 8);
    outs[no++] = xw_span(first_nonpositive, (uintptr_t)P * 4);
    if (R > 0) {
        outs[no++] = xw_span(turnover, (uintptr_t)pr * 8);
        outs[no++] = xw_span(exposure, (uintptr_t)pr * 16);
        outs[no++] = xw_span(count, (uintptr_t)pr * 12);
    }
    if (holdings_out) outs[no++] = xw_span(holdings_out, xw_plane_bytes(d));
    PQ_TRY(xw_no_overlap(outs, no, ins, ni, "pq_factor_weights: an output must not overlap an input",
                         "pq_factor_weights: the outputs must not overlap each other"));
    const std::vector<int32_t> host = pf_day_tables(rebalance_days, R, d.len);
    int32_t *days, *seg, *pc;
    double *pe, *pg, *G, *ptv, *Bv;
    PQ_TRY(xs_ws_carve(ctx, what, [&](XsWs &w) {
        w.take(days, (size_t)R).take(seg, len).take(pe, nblk * 2 * pr).take(pc, nblk * 3 * pr).take(pg, nblk * pt).take(G, pt);
        w.take(ptv, nblk * pr).take(Bv, pr);
    }));
    if (R > 0) PQ_HIP_TRY(hipMemcpyAsync(days, host.data(), (size_t)R * 4, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipMemcpyAsync(seg, host.data() + R, len * 4, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream)); // the table goes away with this call
    PwArgs q{};
    for (int p = 0; p < P; p++) q.w[p] = weights[p];
    q.price = price; q.days = days; q.seg = seg; q.net = exposure; q.G = G; q.d = d; q.R = R; q.ws = w_stride; q.P = P;
    hipStream_t st = ctx->stream;
    if (R > 0) {
        PW_LAUNCH_P(pw_rebalance_partial_kernel, pf_grid(R, nblk), q, pe, pc);
        hipLaunchKernelGGL(pw_sum_blocks_kernel, pf_grid((int64_t)(3 * pr)), dim3(64), 0, st, (const double *)pe, (int64_t)(2 * pr),
                           (const int32_t *)pc, (int64_t)(3 * pr), nblk, exposure, count);
        PW_LAUNCH_P(pw_growth_partial_kernel, pf_grid(d.len, nblk), q, pg);
        hipLaunchKernelGGL(pw_growth_combine_kernel, pf_grid((int64_t)pt), dim3(64), 0, st, q, (const double *)pg, nblk, G);
        PW_LAUNCH_P(pw_turnover_partial_kernel, pf_grid(R, nblk), q, ptv);
        hipLaunchKernelGGL(pw_sum_blocks_kernel, pf_grid((int64_t)pr), dim3(64), 0, st, (const double *)ptv, (int64_t)pr, (const int32_t *)nullptr,
                           (int64_t)0, nblk, turnover, (int32_t *)nullptr);
        const PfArgs c{nullptr, price, nullptr, days, seg, nullptr, G, nullptr, d, R, 0, P};
        hipLaunchKernelGGL(pf_chain_kernel, dim3((unsigned)P), dim3(64), 0, st, c, (const double *)turnover, cost_rate, initial_capital, Bv);
    }
    hipLaunchKernelGGL(pw_first_kernel<true>, dim3(1), dim3(64), 0, st, first_nonpositive, P);
    hipLaunchKernelGGL(pw_curve_kernel, pf_grid((int64_t)pt), dim3(64), 0, st, q, (const double *)Bv, initial_capital, value, first_nonpositive);
    hipLaunchKernelGGL(pw_first_kernel<false>, dim3(1), dim3(64), 0, st, first_nonpositive, P);
    if (holdings_out)
        hipLaunchKernelGGL(pw_holdings_kernel, dim3((unsigned)(d.n * tiles)), dim3(256), 0, st, q, weights[holdings_of],
                           (const double *)(G + (size_t)holdings_of * len), tiles, holdings_out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
