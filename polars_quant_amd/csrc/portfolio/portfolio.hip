// portfolio/portfolio.hip -- decision D-27: group portfolios that are re-formed on given rebalance days, hold their
// members in between and pay a fee on the traded value -- pq_factor_portfolio.  The definitions are in include/pq_hip.h.
//
// On prices the history needs no serial walk: a member bought on d_k at weight w is worth w * h(t) / p(d_k) on day t, so the growth
// G(g, t) of every group on every day is one pass of cross-sectional sums in D-12's order (blocks of 256 symbols, ascending symbols
// from 0.0, blocks in ascending order from 0.0), with the lanes of a wave on consecutive days.  Around it run light passes on the
// rebalance days only -- the sum of the weights A_k(g) and the member counts before it, the turnover after it -- and the chain over
// the rebalance days, the one sequential product, walks R values per group out of LDS.
//
// Workspace: days (i32 [R]) | seg (i32 [len]) | block partials of A (f64) and of the counts (i32), [nblk][ng][R] | A (f64 [ng][R]) |
// block partials of G (f64 [nblk][ng][len]) | G (f64 [ng][len]) | block partials of the turnover (f64 [nblk][ng][R]) | B (f64 [ng][R])
#include "portfolio_dev.h"   // pf_usable, PfArgs, pf_held, pf_chain_kernel, pf_grid, the day check and tables

namespace {

// the members of rebalance k: label (of day d_k - lag) < ng, usable price and weight on d_k
struct PfCell { int l; double p0, a; };
__device__ __forceinline__ PfCell pf_cell(const PfArgs &q, int64_t s, int64_t dk) {
    const int64_t o = s * q.d.stride + dk;
    return PfCell{q.labels[o - q.lag], q.price[o], q.weight ? q.weight[o] : 1.0};
}
__device__ __forceinline__ bool pf_member(const PfArgs &q, const PfCell &c) { return c.l < q.ng && pf_usable(c.p0) && pf_usable(c.a); }

// weight pass: one thread per (rebalance k, block of 256 symbols) -> per group the block's sum of the members' weights and their number
template <int G> __global__ __launch_bounds__(64) void pf_weight_partial_kernel(PfArgs q, double *psum, int32_t *pcnt) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= q.R) return;
    const int64_t dk = q.days[k];
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double sum[G];
    int cnt[G];
#pragma unroll
    for (int g = 0; g < G; g++) { sum[g] = 0.0; cnt[g] = 0; }
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        PfCell c[B];
#pragma unroll
        for (int j = 0; j < B; j++) c[j] = pf_cell(q, s0 + j < s_hi ? s0 + j : s_hi - 1, dk);
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            const bool mem = pf_member(q, c[j]);
#pragma unroll
            for (int g = 0; g < G; g++)
                if (mem && c[j].l == g) { sum[g] += c[j].a; cnt[g] += 1; }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (g < q.ng) {
            const int64_t o = ((int64_t)blockIdx.y * q.ng + g) * q.R + k;
            psum[o] = sum[g]; pcnt[o] = cnt[g];
        }
}

// one thread per cell of [ng][R]: the block partials in ascending block order, from 0.0 (pcnt / cnt null: sums only)
__global__ __launch_bounds__(64) void pf_sum_blocks_kernel(const double *psum, const int32_t *pcnt, int64_t nblk, int64_t cells, double *sum,
                                                           int32_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= cells) return;
    double s = 0.0;
    int32_t c = 0;
    for (int64_t b = 0; b < nblk; b++) {
        s += psum[b * cells + i];
        if (pcnt) c += pcnt[b * cells + i];
    }
    sum[i] = s;
    if (cnt) cnt[i] = c;
}

// growth pass: one thread per (day, block of 256 symbols), the 64 lanes of a wave on 64 consecutive days -- a price load is 512
// contiguous bytes, and the label, base price and weight on d_k are one address for all the lanes of a segment.  Ascending symbols,
// the loads of 8 symbols issued before the first is used; G >= ng accumulators in registers (static indices).  The price matrix is
// read once; the search back for a held price is a rarely taken branch, bounded by the segment.
template <int G> __global__ __launch_bounds__(64) void pf_growth_partial_kernel(PfArgs q, double *part) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= q.d.len) return;
    const int64_t k = q.seg[t];
    if (k < 0) return;
    const int64_t dk = q.days[k];
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double sum[G];
#pragma unroll
    for (int g = 0; g < G; g++) sum[g] = 0.0;
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        PfCell c[B];
        double p[B], A[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int64_t s = s0 + j < s_hi ? s0 + j : s_hi - 1;
            p[j] = q.price[s * q.d.stride + t];
            c[j] = pf_cell(q, s, dk);
        }
#pragma unroll
        for (int j = 0; j < B; j++) A[j] = q.A[(int64_t)(c[j].l < q.ng ? c[j].l : 0) * q.R + k];
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            if (!pf_member(q, c[j])) continue;
            const double h = pf_held(q.price + (s0 + j) * q.d.stride, p[j], t, dk);
            const double term = (c[j].a / A[j]) * (h / c[j].p0);
#pragma unroll
            for (int g = 0; g < G; g++)
                if (c[j].l == g) sum[g] += term;
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (g < q.ng) part[((int64_t)blockIdx.y * q.ng + g) * q.d.len + t] = sum[g];
}

// one thread per (group, day): the block partials in ascending block order; a group without members holds cash (1.0)
__global__ __launch_bounds__(64) void pf_growth_combine_kernel(PfArgs q, const double *part, int64_t nblk, double *Gout) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x, cells = (int64_t)q.ng * q.d.len;
    if (i >= cells) return;
    const int64_t g = i / q.d.len, t = i - g * q.d.len, k = q.seg[t];
    double s = 1.0;
    if (k >= 0 && q.count[g * q.R + k] > 0) {
        s = 0.0;
        for (int64_t b = 0; b < nblk; b++) s += part[b * cells + i];
    }
    Gout[i] = s;
}

// turnover pass: one thread per (rebalance k, block of 256 symbols) -> per group the block's sum of |w_new - w_old|, w_old the weights
// of rebalance k - 1 drifted to d_k (0 at k = 0 and for a symbol that was not held), w_new those of rebalance k (0 for a non-member)
template <int G> __global__ __launch_bounds__(64) void pf_turnover_partial_kernel(PfArgs q, double *part) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= q.R) return;
    const int64_t dk = q.days[k], dp = k > 0 ? q.days[k - 1] : dk;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < q.d.n ? s_lo + XS_BLOCK : q.d.n;
    double tau[G];
#pragma unroll
    for (int g = 0; g < G; g++) tau[g] = 0.0;
    constexpr int B = 4;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        PfCell c[B], o[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int64_t s = s0 + j < s_hi ? s0 + j : s_hi - 1;
            c[j] = pf_cell(q, s, dk);
            o[j] = pf_cell(q, s, dp);
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (s0 + j >= s_hi) break;
            const bool m_new = pf_member(q, c[j]), m_old = k > 0 && pf_member(q, o[j]);
            double w_new = 0.0, w_old = 0.0;
            if (m_new) w_new = c[j].a / q.A[(int64_t)c[j].l * q.R + k];
            if (m_old) {
                const double h = pf_held(q.price + (s0 + j) * q.d.stride, c[j].p0, dk, dp);
                w_old = (o[j].a / q.A[(int64_t)o[j].l * q.R + k - 1]) * (h / o[j].p0) / q.G[(int64_t)o[j].l * q.d.len + dk];
            }
#pragma unroll
            for (int g = 0; g < G; g++) tau[g] += fabs((m_new && c[j].l == g ? w_new : 0.0) - (m_old && o[j].l == g ? w_old : 0.0));
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (g < q.ng) part[((int64_t)blockIdx.y * q.ng + g) * q.R + k] = tau[g];
}

// one thread per (group, day): the capital before d_0, B_k on d_k, B_k G(g, t) on the days in between and after the last
__global__ __launch_bounds__(64) void pf_curve_kernel(PfArgs q, const double *Bv, double capital, double *value) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (int64_t)q.ng * q.d.len) return;
    const int64_t g = i / q.d.len, t = i - g * q.d.len, k = q.seg[t];
    double v;
    if (k < 0) v = (q.R > 0 && t == q.days[0]) ? Bv[g * q.R] : capital;
    else if (k + 1 < q.R && t == q.days[k + 1]) v = Bv[g * q.R + k + 1];
    else v = Bv[g * q.R + k] * q.G[i];
    value[i] = v;
}

#define PF_LAUNCH_G(kern, grid, ...)                                                                        \
    do {                                                                                                    \
        if (ng <= 2) hipLaunchKernelGGL(kern<2>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);              \
        else if (ng <= 5) hipLaunchKernelGGL(kern<5>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);         \
        else if (ng <= 10) hipLaunchKernelGGL(kern<10>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);       \
        else hipLaunchKernelGGL(kern<20>, grid, dim3(64), 0, ctx->stream, __VA_ARGS__);                     \
    } while (0)

} // namespace

extern "C" {

pq_status pq_factor_portfolio(pq_ctx *ctx, const pq_batch *b, const uint8_t *labels, int32_t n_groups, int32_t label_lag,
                              const double *price, const double *weight, const int32_t *rebalance_days, int64_t n_rebalance,
                              double cost_rate, double initial_capital, double *value, double *turnover, int32_t *count) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(n_groups >= 1 && n_groups <= 20, "pq_factor_portfolio: n_groups must be in [1, 20]");
    PQ_REQUIRE(label_lag >= 0, "pq_factor_portfolio: label_lag must not be negative");
    PQ_REQUIRE(cost_rate >= 0.0 && cost_rate < 1.0, "pq_factor_portfolio: cost_rate must be in [0, 1)");
    PQ_REQUIRE(initial_capital > 0.0 && initial_capital <= 1.7976931348623157e308,
               "pq_factor_portfolio: initial_capital must be positive and finite");
    PQ_REQUIRE(n_rebalance >= 0, "pq_factor_portfolio: n_rebalance must not be negative");
    PQ_REQUIRE((b->n_series == 0 || b->len == 0 || (labels && price)) && (b->len == 0 || value) &&
                   (n_rebalance == 0 || (rebalance_days && turnover && count)),
               "pq_factor_portfolio: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_portfolio cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_portfolio (a cross-section needs every symbol on every day)");
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int64_t R = n_rebalance, nblk = xs_nblk(d.n);
    const int ng = n_groups;
    PQ_REQUIRE(d.len <= 0x7fffffffLL && nblk <= 65535, "pq_factor_portfolio: batch too large (len < 2^31, n_series <= 16776960)");
    PQ_TRY(pf_check_days("pq_factor_portfolio", rebalance_days, R, label_lag, "label_lag", d.len));
    const std::vector<int32_t> host = pf_day_tables(rebalance_days, R, d.len);
    const size_t len = (size_t)d.len, gr = (size_t)ng * (size_t)R, gt = (size_t)ng * len;
    int32_t *days, *seg, *pc;
    double *pa, *A, *pg, *G, *pt, *Bv;
    PQ_TRY(xs_ws_carve(ctx, "pq_factor_portfolio", [&](XsWs &w) {
        w.take(days, (size_t)R).take(seg, len).take(pa, nblk * gr).take(pc, nblk * gr).take(A, gr).take(pg, nblk * gt).take(G, gt);
        w.take(pt, nblk * gr).take(Bv, gr);
    }));
    if (R > 0) PQ_HIP_TRY(hipMemcpyAsync(days, host.data(), (size_t)R * 4, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipMemcpyAsync(seg, host.data() + R, len * 4, hipMemcpyHostToDevice, ctx->stream));
    PQ_HIP_TRY(hipStreamSynchronize(ctx->stream)); // the table goes away with this call
    const PfArgs q{labels, price, weight, days, seg, A, G, count, d, R, (int)label_lag, ng};
    if (R > 0) {
        PF_LAUNCH_G(pf_weight_partial_kernel, pf_grid(R, nblk), q, pa, pc);
        hipLaunchKernelGGL(pf_sum_blocks_kernel, pf_grid((int64_t)gr), dim3(64), 0, ctx->stream, (const double *)pa, (const int32_t *)pc, nblk,
                           (int64_t)gr, A, count);
        PF_LAUNCH_G(pf_growth_partial_kernel, pf_grid(d.len, nblk), q, pg);
        hipLaunchKernelGGL(pf_growth_combine_kernel, pf_grid((int64_t)gt), dim3(64), 0, ctx->stream, q, (const double *)pg, nblk, G);
        PF_LAUNCH_G(pf_turnover_partial_kernel, pf_grid(R, nblk), q, pt);
        hipLaunchKernelGGL(pf_sum_blocks_kernel, pf_grid((int64_t)gr), dim3(64), 0, ctx->stream, (const double *)pt, (const int32_t *)nullptr,
                           nblk, (int64_t)gr, turnover, (int32_t *)nullptr);
        hipLaunchKernelGGL(pf_chain_kernel, dim3((unsigned)ng), dim3(64), 0, ctx->stream, q, (const double *)turnover, cost_rate, initial_capital, Bv);
    }
    hipLaunchKernelGGL(pf_curve_kernel, pf_grid((int64_t)gt), dim3(64), 0, ctx->stream, q, (const double *)Bv, initial_capital, value);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
