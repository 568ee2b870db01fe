// xsec/combine.hip -- K tested factors into the one score that the sorts and portfolio_backtest take: weights from the trailing window of
// the factors' IC series, and the weighted sum per (symbol, day) (Factor.combine; beyond the README => decision D-30).
//
//  weights:  ic is [K][len], one IC series per factor (pq_factor_ic's); w[K][len].  The window of day t is the `window` days
//            t - lag - window + 1 .. t - lag; row t is NULL in all K weights unless the whole window lies in [0, len) and all K * window
//            values are non-NULL (pq_rolling_ic's rule: a NaN or inf IC is a value).  method 0 ic: m_k = (sum ic_k) / window; 1 icir:
//            m_k / sd_k, sd_k = sqrt((sum (ic_k - m_k)^2) / (window - 1)), the row NULL unless every sd_k > 0; 2 max_icir: C^-1 m, C the
//            packed triangle of the centred cross-products over window - 1, solved by xsec_ols.h's L D L^T without an intercept, the row
//            NULL unless all K pivots pass XO_SINGULAR.  Every sum starts at 0.0 and adds the window in ascending day order; a weight that
//            comes out NaN makes the row NULL.  m_k and the squares are xw_mean / xw_mean_q2, the row code of ts_std and volatility and the
//            operation sequence of rolling_ic_kernel (factor.hip), so for ic / icir w_k[t] is pq_rolling_ic(ic_k, window) at day t - lag
//            bit for bit.
//            The fourth user of xsec_window.h: the walk sees one symbol whose K columns are the IC series, and the load of staged day g
//            reads day g - lag, so the row of day t finds its window where every other windowed kernel does.  Dynamic LDS, K (255 +
//            window) f64 and (255 + window) i32: 86 972 bytes at K = 8, window = 1024.  Templated on K and the method: every index of the
//            triangle and of L, D is static and nothing goes to scratch (combine.resources.txt).
//  combine:  out[s][t] = sum_k w_k[t] f_k[s][t] (k ascending from 0.0, product and sum rounded separately), over D[t] = sum_k |w_k[t]|
//            with normalize.  NULL unless all K cells are non-null and finite (D-19's common sample), and where a weight of the day is
//            NULL or NaN, where D[t] == 0 under normalize, and where the result is NaN.  Lanes lie along days, the unit-stride axis of
//            every column: a wave loads and stores 512 contiguous bytes per column and symbol (8-byte accesses: a row pitch may be odd).
//            A thread keeps the K weights and D of its day in registers down a strip of CB_STRIP symbols; the (strip, day tile) jobs are
//            walked with a grid stride.  No LDS.
#include "xsec_ols.h"
#include "xsec_window.h"

namespace {

constexpr int CB_MAX_K = XO_MAX_K;
constexpr int CB_STRIP = 16;                                    // symbols per job: the weights of a day are loaded once per strip
enum CbMethod { CB_IC = PQ_COMBINE_IC, CB_ICIR = PQ_COMBINE_ICIR, CB_MAX_ICIR = PQ_COMBINE_MAX_ICIR };

// LDS: column k at cb_lds + k * M, then last[M]
template <int K, int METHOD>
__global__ __launch_bounds__(XW_TILE) void cb_weights_kernel(const double *ic, Dims d, int w, int64_t lag, int64_t chunks, int64_t total,
                                                             double *out) {
    extern __shared__ double cb_lds[];
    __shared__ int wave_last[XW_TILE / 64];
    int *last = (int *)(cb_lds + (size_t)K * (XW_TILE + w - 1));    // index of the last unusable entry <= l, -1 without one
    xw_walk<K>(cb_lds, last, wave_last, d, w, chunks, total,
        [&](int64_t, int64_t g, double *v) {
            const int64_t day = g - lag;
            const bool inside = day >= 0 && day < d.len;
            bool ok = inside;
#pragma unroll
            for (int k = 0; k < K; k++) {
                v[k] = inside ? ic[k * d.len + day] : 0.0;
                ok = ok && !pq_isnull(v[k]);
            }
            return ok;
        },
        [&](int64_t, int64_t t, const double *win, int M, bool usable) {
            double r[K];
            bool ok = usable;
            if (usable) {
                if constexpr (METHOD == CB_IC) {
#pragma unroll
                    for (int k = 0; k < K; k++) r[k] = xw_mean(win + k * M, w);
                } else if constexpr (METHOD == CB_ICIR) {
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const auto [mean, q2] = xw_mean_q2(win + k * M, w);
                        const double sd = sqrt(q2 / (double)(w - 1));
                        ok = ok && sd > 0.0;
                        r[k] = mean / sd;
                    }
                } else {
                    constexpr int NA = xo_tri(K);
                    double mean[K], sq[NA];
#pragma unroll
                    for (int k = 0; k < K; k++) mean[k] = xw_mean(win + k * M, w);
#pragma unroll
                    for (int q = 0; q < NA; q++) sq[q] = 0.0;
                    for (int i = 0; i < w; i++) {
                        double dv[K];
#pragma unroll
                        for (int k = 0; k < K; k++) dv[k] = win[k * M + i] - mean[k];
#pragma unroll
                        for (int j = 0; j < K; j++)
#pragma unroll
                            for (int l = 0; l <= j; l++) sq[xo_tri(j) + l] += dv[j] * dv[l];
                    }
                    const double dof = (double)(w - 1);
#pragma unroll
                    for (int q = 0; q < NA; q++) sq[q] = sq[q] / dof;
                    double L[K][K], D[K], z[K];
                    ok = xo_ldl<K>(sq, L, D) == K;
                    xo_forward<K>(L, mean, K, z);
                    xo_back<K>(L, D, z, K, r);
                }
#pragma unroll
                for (int k = 0; k < K; k++) ok = ok && r[k] == r[k];    // a NaN weight: the row has none
            }
#pragma unroll
            for (int k = 0; k < K; k++) out[k * d.len + t] = ok ? r[k] : pq_null();
        });
}

struct CbIn { const double *f[CB_MAX_K]; };

template <int K>
__global__ __launch_bounds__(XW_TILE) void cb_combine_kernel(CbIn in, const double *wts, Dims d, int normalize, int64_t tiles, int64_t total,
                                                             double *out) {
    for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
        const int64_t strip = job / tiles, t = (job - strip * tiles) * XW_TILE + threadIdx.x;
        if (t >= d.len) continue;
        double wk[K], D = 0.0;
        bool wok = true;
#pragma unroll
        for (int k = 0; k < K; k++) {
            wk[k] = wts[k * d.len + t];
            wok = wok && wk[k] == wk[k];                        // NULL is a NaN
            D += fabs(wk[k]);
        }
        if (normalize) wok = wok && D != 0.0;
        const int64_t s0 = strip * CB_STRIP, s1 = s0 + CB_STRIP < d.n ? s0 + CB_STRIP : d.n;
#pragma unroll 4
        for (int64_t s = s0; s < s1; s++) {
            const int64_t o = s * d.stride + t;
            double f[K];
#pragma unroll
            for (int k = 0; k < K; k++) f[k] = in.f[k][o];
            bool ok = wok;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                ok = ok && xs_valid(f[k]);
                acc += wk[k] * f[k];
            }
            const double r = normalize ? acc / D : acc;
            out[o] = ok && r == r ? r : pq_null();
        }
    }
}

// f(std::integral_constant<int, m>) for a runtime method in [0, 2] (the entry point checks the range)
template <class F> void cb_with_method(int m, F &&f) {
    if (m == CB_IC) f(std::integral_constant<int, CB_IC>{});
    else if (m == CB_ICIR) f(std::integral_constant<int, CB_ICIR>{});
    else f(std::integral_constant<int, CB_MAX_ICIR>{});
}

} // namespace

extern "C" {

pq_status pq_factor_combine_weights(pq_ctx *ctx, const double *ic, int32_t k, int64_t len, int32_t method, int64_t window, int64_t lag,
                                    double *weights) {
    PQ_REQUIRE(ctx, "pq_factor_combine_weights: null context");
    PQ_REQUIRE(k >= 1 && k <= CB_MAX_K, "pq_factor_combine_weights: k must be in [1, 8]");
    PQ_REQUIRE(method >= CB_IC && method <= CB_MAX_ICIR, "pq_factor_combine_weights: method must be 0 (ic), 1 (icir) or 2 (max_icir)");
    const int64_t lo = method == CB_IC ? 1 : (method == CB_ICIR ? 2 : (int64_t)k + 1);
    PQ_REQUIRE(window >= lo && window <= XW_MAX_W,
               "pq_factor_combine_weights: window must be in [1, 1024], at least 2 for icir and at least k + 1 for max_icir");
    PQ_REQUIRE(lag >= 0 && lag <= XW_MAX_W, "pq_factor_combine_weights: lag must be in [0, 1024]");
    PQ_REQUIRE(len >= 0, "pq_factor_combine_weights: negative length");
    PQ_REQUIRE(len == 0 || (ic && weights), "pq_factor_combine_weights: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_combine_weights cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    if (len == 0) return PQ_OK;
    const uintptr_t bytes = (uintptr_t)k * (uintptr_t)len * 8;
    const XwSpan in = xw_span(ic, bytes), o = xw_span(weights, bytes);
    PQ_TRY(xw_no_overlap(&o, 1, &in, 1, "pq_factor_combine_weights: weights must not overlap ic", nullptr));
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    const Dims d{1, len, len, nullptr};
    const int64_t chunks = (len + XW_TILE - 1) / XW_TILE;
    const int w = (int)window;
    const size_t M = (size_t)(XW_TILE + w - 1), lds = (size_t)k * M * 8 + M * 4;
    pq_status st = PQ_OK;
    xo_with_k<CB_MAX_K>(k, [&](auto K) {
        cb_with_method(method, [&](auto METHOD) {
            auto kernel = cb_weights_kernel<decltype(K)::value, decltype(METHOD)::value>;
            if (lds > 48 * 1024) {                              // a launch with more than 64 KB needs the attribute
                const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) {
                    pq_set_error("pq_factor_combine_weights: hipFuncSetAttribute(%zu bytes of LDS): %s", lds, hipGetErrorString(e));
                    st = PQ_ERR_HIP;
                    return;
                }
            }
            hipLaunchKernelGGL(kernel, dim3((unsigned)chunks), dim3(XW_TILE), lds, ctx->stream, ic, d, w, lag, chunks, chunks, weights);
        });
    });
    PQ_TRY(st);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_factor_combine(pq_ctx *ctx, const pq_batch *b, const double *const *factors, int32_t k, const double *weights, int32_t normalize,
                            double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(k >= 1 && k <= CB_MAX_K, "pq_factor_combine: k must be in [1, 8]");
    if (ctx->rec) { pq_set_error("pq_factor_combine cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_combine (a factor column is [n_series][stride])");
    if (b->n_series == 0 || b->len == 0) return PQ_OK;
    PQ_REQUIRE(factors && weights && out, "pq_factor_combine: null pointer");
    const Dims d = dims_of(b);
    const uintptr_t colb = xw_plane_bytes(d) - (uintptr_t)(d.stride - d.len) * 8;   // a column without its last padding
    CbIn in{};
    XwSpan ins[CB_MAX_K + 1];
    for (int j = 0; j < k; j++) {
        PQ_REQUIRE(factors[j], "pq_factor_combine: null factor pointer");
        in.f[j] = factors[j];
        ins[j] = xw_span(factors[j], colb);
    }
    ins[k] = xw_span(weights, (uintptr_t)k * (uintptr_t)d.len * 8);
    const XwSpan o = xw_span(out, colb);
    PQ_TRY(xw_no_overlap(&o, 1, ins, k + 1, "pq_factor_combine: out must not overlap a factor or the weights", nullptr));
    const int64_t tiles = (d.len + XW_TILE - 1) / XW_TILE, strips = (d.n + CB_STRIP - 1) / CB_STRIP, total = tiles * strips;
    const dim3 grid((unsigned)(total < (int64_t)1 << 20 ? total : (int64_t)1 << 20));
    xo_with_k<CB_MAX_K>(k, [&](auto K) {
        hipLaunchKernelGGL(cb_combine_kernel<decltype(K)::value>, grid, dim3(XW_TILE), 0, ctx->stream, in, weights, d, normalize != 0 ? 1 : 0,
                           tiles, total, out);
    });
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
