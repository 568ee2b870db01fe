// xsec/wls.hip -- the weighted per-day cross-sectional regression of the next return on K style factors and G industry dummies
// (Factor.pure_factor_return); decision D-32, DESIGN.md section 2.
//
// Model on day t over the day's sample: r_i = g_{ind(i)} + sum_j b_j f_ij + e_i, minimising sum_i w_i e_i^2.  No separate intercept: the
// dummies span it, and without industries every symbol is in group 0, whose return is the intercept.  The dummy block is eliminated
// exactly (Frisch-Waugh): weighted demeaning within each industry, then D-17's K x K system on xsec_ols.h's xo_ldl / xo_forward /
// xo_back, used the way orth.hip uses them (xo_fit's intercept half has no counterpart here).  Columns are symbol-major
// [n_series][stride]; 64 lanes = 64 consecutive days (coalesced), blockIdx.y = the block of 256 symbols, every sum D-12's blocked sum.
//  1. pass 1:  per (day, industry) the member count, W = sum w and S[c] = sum (w x_c) of the columns c = r, f_0 .. f_{K-1}: K + 3
//              accumulator columns, kept [column][g][lane] in LDS as clean.hip's industry pass keeps its sums.  All of them do not fit
//              the CU's LDS at every G, so the pass runs over chunks of wl_chunk(K + 3, G) columns (the rule is there); each chunk's
//              block partials are combined per (day, industry) into the table tab[column][g][len] before the next chunk reuses them.
//  2. day:     n, G_t (industries with a member) and rbar = (sum_g S_g[r]) / (sum_g W_g), present g ascending; then the table's S
//              rows become the means m_g[c] = S_g[c] / W_g.
//  3. pass 2:  d_c = x_c - m_g[c] read from the table (coalesced over days); the packed triangle of D-17 on (w d_j) d_l, Srr, and Stot
//              on r - rbar, in registers (templated on K: every triangle index is static).
//  4. solve:   one thread per day: C = L D L^T, b, diag(C^-1); L and D are kept for the industry rows.
//  5. pass 3:  e = d_r - sum_j b_j d_j, SSE = sum (w e) e, and e -> resid on the sample's cells of solved days (NULL elsewhere).
//  6. final:   one thread per day: s^2 = SSE / (n - K - G_t), the factor rows, both R^2, n, G_t; one thread per (day, industry):
//              g_g = m_g[r] - sum_j b_j m_g[f_j], V_g = 1 / W_g + u^T D^-1 u with L u = m_g[f].  Then D-17's Fama-MacBeth rows.
// The operation order is D-32's, restated in tests/xsec_wls_ref.py.  With every weight 1.0 and one group each step is D-17's bit for bit.
#include "xsec_ols.h"
#include "xsec_ttest.h"

namespace {

constexpr int WL_LDS_CELLS = 128;    // (column, industry) pairs of [64]-lane f64 accumulators per pass-1 workgroup: 64 KiB of LDS

// columns of pass 1 per chunk: as many of the ncol as keep chunk * G within WL_LDS_CELLS, at least one.  So a workgroup's LDS is
// chunk * G * 512 B <= 64 KiB up to G = 128 (two workgroups per CU, more at small G) and G * 512 B <= 128 KiB beyond (one), and the
// block partials are chunk * G * nblk * len * 8 B <= 128 * nblk * len * 8 B: half an input column (a full one for G > 128).
inline int wl_chunk(int ncol, int G) {
    const int c = WL_LDS_CELLS / G;
    return c < 1 ? 1 : (c > ncol ? ncol : c);
}

struct WlIn {
    const double *f[XO_MAX_K];
    const double *r, *w;   // w null: every weight 1.0
    XsGroups grp;          // null codes: every symbol in group 0 (G = 1)
    Dims d;
};

// per-day state, [len] rows (b, v: [K]; L: [K (K - 1) / 2] packed by rows; D: [K]), and the (column, industry) table
struct WlDay {
    int32_t *n, *gt, *ok;
    double *rbar, *srr, *stot, *s2;
    double *b, *v, *L, *D;
    double *tab;           // [K + 3][G][len]: member count, W, then S (after wl_means_kernel: m) of r, f_0 .. f_{K-1}
};

enum WlTab { WL_CNT = 0, WL_W = 1, WL_R = 2, WL_F = 3 };

__device__ __forceinline__ int64_t wl_tab(const WlIn &in, int q, int g, int64_t t) { return ((int64_t)q * in.grp.G + g) * in.d.len + t; }

// the cells of one step of a (day, block) thread: B symbols loaded ahead, then their membership
template <int K, int B> struct WlCells {
    double r[B], f[B][K], w[B];
    int32_t g[B];
    __device__ __forceinline__ void load(const WlIn &in, int64_t s0, int64_t s_hi, int64_t t) {
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1, o = s * in.d.stride + t;
            r[k] = in.r[o];
#pragma unroll
            for (int j = 0; j < K; j++) f[k][j] = in.f[j][o];
            w[k] = in.w ? in.w[o] : 1.0;
            g[k] = in.grp.codes ? in.grp.at(s, t) : 0;
        }
    }
    __device__ __forceinline__ bool member(const WlIn &in, int k) const {
        bool mem = xs_valid(r[k]) && xs_valid(w[k]) && w[k] > 0.0 && in.grp.has(g[k]);
#pragma unroll
        for (int j = 0; j < K; j++) mem = mem && xs_valid(f[k][j]);
        return mem;
    }
};

// ---------------------------------------------------------------- pass 1
// the columns [c0, c1) of the K + 3; accumulators [c - c0][g][lane] in LDS (consecutive lanes on consecutive 8-byte words: no bank
// conflict whatever the codes), block partials ps[block][c - c0][g][len]
template <int K>
__global__ __launch_bounds__(64) void wl_pass1_kernel(WlIn in, int c0, int c1, double *ps) {
    extern __shared__ __align__(16) unsigned char wl_lds[];
    double *acc = (double *)wl_lds;
    const Dims d = in.d;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int lane = threadIdx.x, G = in.grp.G, nq = (c1 - c0) * G;
    for (int q = 0; q < nq; q++) acc[q * 64 + lane] = 0.0;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    constexpr int B = xo_ahead(K + 2);
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        WlCells<K, B> c;
        c.load(in, s0, s_hi, t);
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            if (!c.member(in, k)) continue;
            const double wv = c.w[k];
#pragma unroll
            for (int q = 0; q < K + 3; q++) {
                if (q < c0 || q >= c1) continue;
                const double v = q == WL_CNT ? 1.0 : (q == WL_W ? wv : (q == WL_R ? wv * c.r[k] : wv * c.f[k][q >= WL_F ? q - WL_F : 0]));
                acc[((q - c0) * G + c.g[k]) * 64 + lane] += v;
            }
        }
    }
    for (int q = 0; q < nq; q++) ps[((int64_t)blockIdx.y * nq + q) * d.len + t] = acc[q * 64 + lane];
}

// one thread per (day, industry): the chunk's block sums in ascending block order from 0.0 -> the table rows c0 .. c0 + nc - 1
__global__ __launch_bounds__(64) void wl_gsum_kernel(const double *ps, int64_t nblk, int64_t len, int G, int c0, int nc, double *tab) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (t >= len) return;
    for (int q = 0; q < nc; q++) {
        double s = 0.0;
        for (int64_t k = 0; k < nblk; k++) s += ps[((k * nc + q) * G + g) * len + t];
        tab[((int64_t)(c0 + q) * G + g) * len + t] = s;
    }
}

// one thread per day: n, G_t, and rbar over the present industries in ascending order from 0.0
__global__ __launch_bounds__(64) void wl_day_kernel(WlIn in, WlDay day) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= in.d.len) return;
    int32_t n = 0, gt = 0;
    double sw = 0.0, sr = 0.0;
    for (int g = 0; g < in.grp.G; g++) {
        const double c = day.tab[wl_tab(in, WL_CNT, g, t)];
        if (c > 0.0) {
            n += (int32_t)c;
            gt += 1;
            sw += day.tab[wl_tab(in, WL_W, g, t)];
            sr += day.tab[wl_tab(in, WL_R, g, t)];
        }
    }
    day.n[t] = n;
    day.gt[t] = gt;
    day.rbar[t] = sr / sw;
}

// one thread per (day, industry): S_g[c] -> m_g[c] = S_g[c] / W_g (after wl_day_kernel has read the S of r)
__global__ __launch_bounds__(64) void wl_means_kernel(WlIn in, int K, WlDay day) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (t >= in.d.len) return;
    const double W = day.tab[wl_tab(in, WL_W, g, t)];
    for (int c = 0; c <= K; c++) {
        const int64_t o = wl_tab(in, WL_R + c, g, t);
        day.tab[o] = day.tab[o] / W;
    }
}

// ---------------------------------------------------------------- passes 2 and 3
template <int K> struct WlNa {
    static constexpr int P2 = xo_tri(K + 1) + 1;   // D-17's triangle of f_0 .. f_{K-1}, r, then Stot
};

// P == 2: the triangle and Stot.  P == 3: SSE, and e -> resid where resid is given.
template <int K, int P>
__global__ __launch_bounds__(64) void wl_pass_kernel(WlIn in, WlDay day, double *ps, double *__restrict__ resid) {
    constexpr int NA = P == 2 ? WlNa<K>::P2 : 1;
    const Dims d = in.d;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const double rbar = P == 2 ? day.rbar[t] : 0.0;
    const bool ok = P == 3 && day.ok[t] != 0;
    double b[K];
#pragma unroll
    for (int j = 0; j < K; j++) b[j] = ok ? day.b[(int64_t)j * d.len + t] : 0.0;
    double acc[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) acc[q] = 0.0;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    constexpr int B = xo_ahead(K + 2);
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        WlCells<K, B> c;
        c.load(in, s0, s_hi, t);
        double mr[B], mf[B][K];   // the means of the cell's industry (of industry 0 for a cell outside [0, G): not a member)
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int g = c.g[k] >= 0 && c.g[k] < in.grp.G ? c.g[k] : 0;   // written out: through has() +2 VGPRs per instantiation (XsGroups)
            mr[k] = day.tab[wl_tab(in, WL_R, g, t)];
#pragma unroll
            for (int j = 0; j < K; j++) mf[k][j] = day.tab[wl_tab(in, WL_F + j, g, t)];
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            const bool mem = c.member(in, k);
            if (P == 3 && resid && !(mem && ok)) resid[(s0 + k) * d.stride + t] = pq_null();
            if (!mem) continue;
            const double wv = c.w[k], dr = c.r[k] - mr[k];
            double df[K];
#pragma unroll
            for (int j = 0; j < K; j++) df[j] = c.f[k][j] - mf[k][j];
            if (P == 2) {
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const double wd = wv * df[j];
#pragma unroll
                    for (int l = 0; l <= j; l++) acc[xo_tri(j) + l] += wd * df[l];
                    acc[xo_tri(K) + j] += wd * dr;
                }
                acc[xo_tri(K) + K] += (wv * dr) * dr;
                const double dt = c.r[k] - rbar;
                acc[NA - 1] += (wv * dt) * dt;
                continue;
            }
            double fit = 0.0;
#pragma unroll
            for (int j = 0; j < K; j++) fit += b[j] * df[j];
            const double e = dr - fit;
            acc[0] += (wv * e) * e;
            if (resid && ok) resid[(s0 + k) * d.stride + t] = e;
        }
    }
#pragma unroll
    for (int q = 0; q < NA; q++) ps[((int64_t)blockIdx.y * NA + q) * d.len + t] = acc[q];
}

// after pass 2, one thread per day: solved iff no pivot is singular and n >= K + G_t + 1; b, diag(C^-1), and L, D for the industry rows
template <int K>
__global__ __launch_bounds__(64) void wl_solve_kernel(const double *ps, int64_t nblk, int64_t len, WlDay day) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    constexpr int NA = WlNa<K>::P2;
    double s[NA];
    xo_combine<NA>(ps, nblk, len, t, s);
    day.srr[t] = s[xo_tri(K) + K];
    day.stot[t] = s[NA - 1];
    double L[K][K], D[K];
    const bool ok = xo_ldl<K>(s, L, D) == K && day.n[t] >= K + day.gt[t] + 1;
    day.ok[t] = ok ? 1 : 0;
    if (!ok) return;
    double z[K], b[K];
    xo_forward<K>(L, s + xo_tri(K), K, z);   // c = row K of the triangle
    xo_back<K>(L, D, z, K, b);
#pragma unroll
    for (int j = 0; j < K; j++) {
        day.b[(int64_t)j * len + t] = b[j];
        day.D[(int64_t)j * len + t] = D[j];
#pragma unroll
        for (int l = 0; l < j; l++) day.L[(int64_t)(j * (j - 1) / 2 + l) * len + t] = L[j][l];
        // (C^-1)_jj = sum_m (L^-1 e_j)_m^2 / D_m, m ascending from 0.0 (as xo_fit)
        double e[K], w[K];
#pragma unroll
        for (int m = 0; m < K; m++) e[m] = m == j ? 1.0 : 0.0;
        xo_forward<K>(L, e, K, w);
        double vj = 0.0;
#pragma unroll
        for (int m = 0; m < K; m++) vj += w[m] * w[m] / D[m];
        day.v[(int64_t)j * len + t] = vj;
    }
}

struct WlOut {
    double *coef, *tst, *pv, *r2;
    int32_t *n_obs, *n_present;
    double *resid, *summary;
};

// after pass 3, one thread per day: s^2 = SSE / df on df = n - K - G_t, the K factor rows, R^2 total and within, n and G_t
template <int K>
__global__ __launch_bounds__(64) void wl_final_kernel(const double *ps, int64_t nblk, int64_t len, WlDay day, WlOut out) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    double sse[1];
    xo_combine<1>(ps, nblk, len, t, sse);
    const int32_t n = day.n[t], gt = day.gt[t];
    out.n_obs[t] = n;
    out.n_present[t] = gt;
    const bool ok = day.ok[t] != 0;
    const double df = (double)(n - K - gt), s2 = sse[0] / df;
    day.s2[t] = s2;
    out.r2[t] = rg_r2(ok, sse[0], ok ? day.stot[t] : 0.0);
    out.r2[len + t] = rg_r2(ok, sse[0], ok ? day.srr[t] : 0.0);
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int64_t o = (int64_t)j * len + t;
        rg_coef_stats(ok, day.b + o, day.v + o, s2, df, out.coef + o, out.tst + o, out.pv + o);
    }
}

// one thread per (day, industry): rows K + g; NULL without a solution and on a day the industry has no member
template <int K>
__global__ __launch_bounds__(64) void wl_industry_kernel(WlIn in, WlDay day, WlOut out) {
    const int64_t len = in.d.len, t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (t >= len) return;
    const int64_t o = (int64_t)(K + g) * len + t;
    const bool ok = day.ok[t] != 0 && day.tab[wl_tab(in, WL_CNT, g, t)] > 0.0;
    if (!ok) { rg_coef_stats(false, nullptr, nullptr, 0.0, 0.0, out.coef + o, out.tst + o, out.pv + o); return; }
    double L[K][K], D[K], b[K], mf[K], u[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        b[j] = day.b[(int64_t)j * len + t];
        D[j] = day.D[(int64_t)j * len + t];
        mf[j] = day.tab[wl_tab(in, WL_F + j, g, t)];
#pragma unroll
        for (int l = 0; l < K; l++) L[j][l] = l < j ? day.L[(int64_t)(j * (j - 1) / 2 + l) * len + t] : (l == j ? 1.0 : 0.0);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < K; j++) s += b[j] * mf[j];
    const double gc = day.tab[wl_tab(in, WL_R, g, t)] - s;
    xo_forward<K>(L, mf, K, u);
    double q = 0.0;
#pragma unroll
    for (int m = 0; m < K; m++) q += u[m] * u[m] / D[m];
    const double vg = 1.0 / day.tab[wl_tab(in, WL_W, g, t)] + q;
    rg_coef_stats(true, &gc, &vg, day.s2[t], (double)(day.n[t] - K - day.gt[t]), out.coef + o, out.tst + o, out.pv + o);
}

template <int K>
pq_status wl_run(pq_ctx *ctx, const WlIn &in, const WlOut &out) {
    const Dims d = in.d;
    const int G = in.grp.G, NC = K + 3, chunk = wl_chunk(NC, G);
    const int64_t nblk = xs_nblk(d.n);
    const size_t len = (size_t)d.len;
    // workspace: n, G_t, ok (i32) | day rows (f64): rbar, srr, stot, s2, b [K], v [K], L [K (K - 1) / 2], D [K] | the table
    // [K + 3][G][len] | block partials: the larger of a pass-1 chunk [nblk][chunk][G][len] and pass 2's [nblk][NA][len]
    constexpr int NL = K * (K - 1) / 2;
    const size_t part = (size_t)nblk * len, p1 = part * (size_t)chunk * (size_t)G, p2 = part * (size_t)WlNa<K>::P2;
    WlDay day;
    double *ps;
    PQ_TRY(xs_ws_carve(ctx, "pq_xsec_regress_wls", [&](XsWs &w) {
        w.take(day.n, len).take(day.gt, len).take(day.ok, len).take(day.rbar, len).take(day.srr, len).take(day.stot, len).take(day.s2, len);
        // b, v, L and D are read `len` doubles apart, so their rows are carved unaligned from one aligned span
        w.take(day.b, (size_t)(3 * K + NL) * len).take(day.tab, (size_t)NC * G * len).take(ps, p1 > p2 ? p1 : p2);
    }));
    day.v = day.b + (size_t)K * len; day.L = day.b + (size_t)2 * K * len; day.D = day.b + (size_t)(2 * K + NL) * len;
    const dim3 gd((unsigned)((d.len + 63) / 64)), gp(gd.x, (unsigned)nblk), gg(gd.x, (unsigned)G);
    hipStream_t st = ctx->stream;
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)wl_pass1_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, chunk * G * 64 * 8));
    for (int c0 = 0; c0 < NC; c0 += chunk) {
        const int c1 = c0 + chunk < NC ? c0 + chunk : NC;
        hipLaunchKernelGGL(wl_pass1_kernel<K>, gp, dim3(64), (size_t)(c1 - c0) * G * 64 * 8, st, in, c0, c1, ps);
        hipLaunchKernelGGL(wl_gsum_kernel, gg, dim3(64), 0, st, (const double *)ps, nblk, d.len, G, c0, c1 - c0, day.tab);
    }
    hipLaunchKernelGGL(wl_day_kernel, gd, dim3(64), 0, st, in, day);
    hipLaunchKernelGGL(wl_means_kernel, gg, dim3(64), 0, st, in, K, day);
    hipLaunchKernelGGL((wl_pass_kernel<K, 2>), gp, dim3(64), 0, st, in, day, ps, (double *)nullptr);
    hipLaunchKernelGGL(wl_solve_kernel<K>, gd, dim3(64), 0, st, (const double *)ps, nblk, d.len, day);
    hipLaunchKernelGGL((wl_pass_kernel<K, 3>), gp, dim3(64), 0, st, in, day, ps, out.resid);
    hipLaunchKernelGGL(wl_final_kernel<K>, gd, dim3(64), 0, st, (const double *)ps, nblk, d.len, day, out);
    hipLaunchKernelGGL(wl_industry_kernel<K>, gg, dim3(64), 0, st, in, day, out);
    if (out.summary)
        hipLaunchKernelGGL(rg_summary_kernel, dim3((unsigned)(K + G)), dim3(64), 0, st, (const double *)out.coef, d.len, out.summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_xsec_regress_wls(pq_ctx *ctx, const pq_batch *b, const double *const *factors, int32_t k, const double *fwd_return,
                              const double *weight, const int32_t *group, int64_t group_stride, int32_t n_groups, double *coef,
                              double *t_stat, double *p_value, double *r2, int32_t *n_obs, int32_t *n_groups_present, double *resid,
                              double *summary) {
    const char *what = "pq_xsec_regress_wls";
    PQ_TRY(pq_check(ctx, b));
    if (k < 1 || k > XO_MAX_K) { pq_set_error("%s: k must be in [1, 8]", what); return PQ_ERR_ARG; }
    WlIn in{};
    PQ_TRY(xs_groups_arg(what, b, group, group_stride, n_groups, XsGroupsPolicy{XS_G_ALWAYS, "n_groups", "group"}, &in.grp));
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", what); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", what); return PQ_ERR_UNSUPPORTED; }
    PQ_TRY(xs_groups_stride(what, b, group != nullptr, group_stride));
    const bool empty = b->n_series == 0 || b->len == 0;
    if (!empty && (!factors || !fwd_return)) { pq_set_error("%s: null pointer", what); return PQ_ERR_ARG; }
    for (int j = 0; j < k && !empty; j++) {
        if (!factors[j]) { pq_set_error("%s: null factor pointer", what); return PQ_ERR_ARG; }
        in.f[j] = factors[j];
    }
    if (b->len != 0 && !(coef && t_stat && p_value && r2 && n_obs && n_groups_present)) {
        pq_set_error("%s: null output pointer", what);
        return PQ_ERR_ARG;
    }
    if (b->len == 0) return PQ_OK;
    in.r = fwd_return;
    in.w = weight;
    in.d = dims_of(b);
    const WlOut out{coef, t_stat, p_value, r2, n_obs, n_groups_present, resid, summary};
    return xo_with_k<XO_MAX_K>(k, [&](auto K) { return wl_run<decltype(K)::value>(ctx, in, out); });
}

} // extern "C"
