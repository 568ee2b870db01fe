// xsec/build.hip -- the README's general factor calculations: per-day rank, normalize, weighted, and the elementwise ratio and diff
// (Factor.rank / normalize / weighted / ratio / diff; README.md:1416-1421, :1438-1470; README-only => decision D-20).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.  Every output is a full [n_series][stride] f64
// column, NULL outside the day's sample.
//  rank family: D-15's day-sort stage (xsec_dev.h, daysort.hip) with the key "the factor where it is non-null and finite, +0 for -0" and
//               its sort-then-look-up pair with BdRankOp:
//               every symbol finds the tie run [a, b) of its own key (xs_tie_run) and overwrites its key by the finished value (rank,
//               reversed rank, pct or mid-rank position), still day-major; a second tiled transpose brings the values symbol-major, so the
//               final stores run along days, 256 contiguous bytes per half-wave.
//  minmax:      one thread per (day, block of 256 symbols), consecutive threads on consecutive days (coalesced), takes the block's min
//               and max; one thread per day combines them; the (day, block) pass runs once more and writes.
//  weighted:    the same three passes with the sum of the weights (D-12: members only, ascending symbols from 0.0, block sums in ascending
//               block order).  With groups every lane keeps G sums in LDS ([g][lane]: consecutive lanes on consecutive 8-byte words, so no
//               bank conflict whatever the codes), as D-16's industry sums do.
//  ratio, diff: one elementwise kernel with an op code, rows along days.
// The zscore of Factor.normalize is pq_factor_clean(standardize = 1) itself (clean.hip), not restated here.
#include "xsec_dev.h"

namespace {

enum BdRank { BD_RANK = 0, BD_PCT = 1, BD_MID = 2 };
enum BdOp { BD_RATIO = 0, BD_DIFF = 1, BD_RELDIFF = 2 };

// ---------------------------------------------------------------- rank family
// the key of xs_prep_kernel: the factor where it is valid, +0 for -0
struct BdKey {
    const double *f;
    __device__ void operator()(int64_t o, double (&k)[1]) const {
        const double x = f[o];
        if (xs_valid(x)) k[0] = x == 0.0 ? 0.0 : x;
    }
};

// m = a + b -> the average rank ((a + 1) + b) / 2 (a half-integer: exact), reversed as n + 1 - rank (exact), then one division
__device__ __forceinline__ double bd_value(int64_t m, int nv, int mode, int desc) {
    double r = (double)(m + 1) / 2.0;
    if (desc) r = (double)(nv + 1) - r;
    if (mode == BD_PCT) r = r / (double)nv;
    if (mode == BD_MID) r = (r - 0.5) / (double)nv;
    return r;
}

// the operation of xsec_dev.h's sort-then-look-up pair: one sort; every symbol replaces its key by its value (day-major, in place)
struct BdRankOp {
    static constexpr int MAX_STEPS = 1;
    double *key;
    int mode, desc;
    __host__ __device__ int steps() const { return 1; }
    __host__ __device__ const double *row(int) const { return key; }
    __device__ bool unsorted(int nv) const { return nv == 0; }
    __device__ void fill(int64_t i) const { key[i] = pq_null(); }
    template <bool PAD> __device__ void at(int, XsRow<PAD> S, int nv, int64_t i) const {
        const double k = key[i];
        key[i] = k == xs_inf() ? pq_null() : bd_value(xs_tie_run(S, nv, k), nv, mode, desc);
    }
};

// day-major [len][n] values -> symbol-major [n][stride]: 32 x 32 tiles, reads along symbols, stores along days
__global__ __launch_bounds__(256) void bd_transpose_kernel(const double *dm, int64_t n, int64_t len, double *out, int64_t stride) {
    __shared__ double tile[32][33];
    const int64_t t0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5; // 32 x 8
    for (int i = ly; i < 32; i += 8) {
        const int64_t t = t0 + i, s = s0 + lx;
        tile[i][lx] = (t < len && s < n) ? dm[t * n + s] : 0.0;
    }
    __syncthreads();
    for (int i = ly; i < 32; i += 8) {
        const int64_t s = s0 + i, t = t0 + lx;
        if (s < n && t < len) out[s * stride + t] = tile[lx][i];
    }
}

// ---------------------------------------------------------------- minmax
// one thread per (day, block of 256 symbols): the block's min and max over the valid values (-0 read as +0); +inf / -inf without one
template <bool WRITE>
__global__ __launch_bounds__(64) void bd_minmax_kernel(const double *f, Dims d, double *pmin, double *pmax, const double *dmin,
                                                       const double *dmax, double *out) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    double mn = xs_inf(), mx = -xs_inf();
    if (WRITE) { mn = dmin[t]; mx = dmax[t]; }
    const double range = mx - mn;
    const bool dead = WRITE && mx == mn;
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double x[B];
#pragma unroll
        for (int k = 0; k < B; k++) x[k] = f[(s0 + k < s_hi ? s0 + k : s_hi - 1) * d.stride + t];
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            const bool mem = xs_valid(x[k]);
            const double v = x[k] == 0.0 ? 0.0 : x[k];
            if (WRITE) {
                out[(s0 + k) * d.stride + t] = (mem && !dead) ? (v - mn) / range : pq_null();
            } else if (mem) {
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            }
        }
    }
    if (WRITE) return;
    const int64_t o = (int64_t)blockIdx.y * d.len + t;
    pmin[o] = mn;
    pmax[o] = mx;
}

__global__ __launch_bounds__(64) void bd_minmax_combine_kernel(const double *pmin, const double *pmax, int64_t nblk, int64_t len, double *dmin,
                                                               double *dmax) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    double mn = xs_inf(), mx = -xs_inf();
    for (int64_t k = 0; k < nblk; k++) {
        const double a = pmin[k * len + t], b = pmax[k * len + t];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    dmin[t] = mn;
    dmax[t] = mx;
}

// ---------------------------------------------------------------- weighted
struct BdW {
    const double *f, *w;
    XsGroups grp;         // null codes = one sum per day
    Dims d;
};

__device__ __forceinline__ bool bd_w_member(const BdW &in, double x, double w, int32_t g) {
    return xs_valid(x) && xs_valid(w) && (!in.grp.codes || (g >= 0 && g < in.grp.G));   // written out: see XsGroups::has
}

enum BdWPass { BD_W_SUM, BD_W_GSUM, BD_W_WRITE };

// one thread per (day, block of 256 symbols).  BD_W_SUM: the block's sum of w over the members, ascending symbols from 0.0 (D-12);
// BD_W_GSUM: one such sum per group, [g][lane] in LDS; BD_W_WRITE: (x w) / W with the day's (or the day's group's) W, NULL where W == 0
template <int P>
__global__ __launch_bounds__(64) void bd_weighted_kernel(BdW in, double *ps, const double *W, double *out) {
    extern __shared__ __align__(16) unsigned char bd_lds[];
    const Dims d = in.d;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int lane = threadIdx.x, G = in.grp.G;
    double *gs = (double *)bd_lds;
    if (P == BD_W_GSUM)
        for (int g = 0; g < G; g++) gs[g * 64 + lane] = 0.0;
    const bool grouped = in.grp.codes != nullptr;
    const double Wday = (P == BD_W_WRITE && !grouped) ? W[t] : 0.0;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    double a0 = 0.0;
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double x[B], w[B];
        int32_t g[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1, o = s * d.stride + t;
            x[k] = in.f[o];
            w[k] = in.w[o];
            g[k] = grouped ? in.grp.at(s, t) : 0;
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            const bool mem = bd_w_member(in, x[k], w[k], g[k]);
            if (P == BD_W_SUM) { if (mem) a0 += w[k]; continue; }
            if (P == BD_W_GSUM) { if (mem) gs[g[k] * 64 + lane] += w[k]; continue; }
            double v = pq_null();
            if (mem) {
                const double Ws = grouped ? W[(int64_t)g[k] * d.len + t] : Wday;
                if (Ws != 0.0) v = (x[k] * w[k]) / Ws;
            }
            out[(s0 + k) * d.stride + t] = v;
        }
    }
    if (P == BD_W_SUM) ps[(int64_t)blockIdx.y * d.len + t] = a0;
    if (P == BD_W_GSUM)
        for (int g = 0; g < G; g++) ps[((int64_t)blockIdx.y * G + g) * d.len + t] = gs[g * 64 + lane];
}

// one thread per (day, group): the block sums in ascending block order from 0.0 -> W [G][len] (G = 1 without groups)
__global__ __launch_bounds__(64) void bd_weighted_combine_kernel(const double *ps, int64_t nblk, int64_t len, int G, double *W) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (t >= len) return;
    double s = 0.0;
    for (int64_t k = 0; k < nblk; k++) s += ps[(k * G + g) * len + t];
    W[(int64_t)g * len + t] = s;
}

// ---------------------------------------------------------------- ratio / diff
// one workgroup per (series, 256 days), walked with a grid stride; NULL where either input is NULL, else plain IEEE-754
__global__ __launch_bounds__(256) void bd_binary_kernel(const double *a, const double *b, Dims d, int op, int64_t chunks, int64_t total,
                                                        double *out) {
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t s = w / chunks, t = (w - s * chunks) * 256 + threadIdx.x;
        if (t >= d.len) continue;
        const int64_t o = s * d.stride + t;
        const double x = a[o], y = b[o];
        double v;
        if (pq_isnull(x) || pq_isnull(y)) v = pq_null();
        else if (op == BD_RATIO) v = x / y;
        else if (op == BD_DIFF) v = x - y;
        else v = (x - y) / fabs(y);
        out[o] = v;
    }
}

} // namespace

extern "C" {

pq_status pq_factor_rank(pq_ctx *ctx, const pq_batch *b, const double *factor, int32_t mode, int32_t descending, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(mode >= BD_RANK && mode <= BD_MID, "pq_factor_rank: mode must be 0 (rank), 1 (pct) or 2 (mid-rank position)");
    PQ_REQUIRE(descending == 0 || descending == 1, "pq_factor_rank: descending must be 0 or 1");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (factor && out), "pq_factor_rank: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_rank cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_rank (a cross-section needs every symbol on every day)");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const size_t cells = (size_t)d.len * (size_t)d.n, len = (size_t)d.len;
    XsDaySort plan;
    PQ_TRY(xs_day_sort_plan(ctx, d, "pq_factor_rank", &plan));
    // workspace: keys, then values (f64, day-major) | n per day (i32) | wide: sorted keys (f64), offsets (u32), rocPRIM temp
    double *key;
    int32_t *nv;
    unsigned char *tail;
    PQ_TRY(xs_ws_carve(ctx, "pq_factor_rank", [&](XsWs &w) { w.take(key, cells).take(nv, len).take(tail, plan.bytes); }));
    hipStream_t st = ctx->stream;
    const dim3 gt((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32));
    PQ_HIP_TRY(hipMemsetAsync(nv, 0, len * 4, st));
    hipLaunchKernelGGL((xs_prep_kernel<1, BdKey>), gt, dim3(256), 0, st, BdKey{factor}, d, key, (int64_t)0, nv);
    PQ_TRY(xs_sort_lookup(ctx, d, plan, tail, BdRankOp{key, mode, descending}, nv));
    hipLaunchKernelGGL(bd_transpose_kernel, gt, dim3(256), 0, st, (const double *)key, d.n, d.len, out, d.stride);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_factor_minmax(pq_ctx *ctx, const pq_batch *b, const double *factor, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (factor && out), "pq_factor_minmax: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_minmax cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_minmax (a cross-section needs every symbol on every day)");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const size_t len = (size_t)d.len;
    const int64_t nblk = xs_nblk(d.n);
    // workspace: block partials min, max [nblk][len] | per-day min, max [len]
    double *pmin, *pmax, *dmin, *dmax;
    PQ_TRY(xs_ws_carve(ctx, "pq_factor_minmax", [&](XsWs &w) { w.take(pmin, nblk * len).take(pmax, nblk * len).take(dmin, len).take(dmax, len); }));
    const dim3 gp((unsigned)((d.len + 63) / 64), (unsigned)nblk), gd((unsigned)((d.len + 63) / 64));
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(bd_minmax_kernel<false>, gp, dim3(64), 0, st, factor, d, pmin, pmax, (const double *)nullptr, (const double *)nullptr,
                       (double *)nullptr);
    hipLaunchKernelGGL(bd_minmax_combine_kernel, gd, dim3(64), 0, st, (const double *)pmin, (const double *)pmax, nblk, d.len, dmin, dmax);
    hipLaunchKernelGGL(bd_minmax_kernel<true>, gp, dim3(64), 0, st, factor, d, (double *)nullptr, (double *)nullptr, (const double *)dmin,
                       (const double *)dmax, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_factor_weighted(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *weight, const int32_t *group,
                             int64_t group_stride, int32_t n_groups, double *out) {
    PQ_TRY(pq_check(ctx, b));
    XsGroups grp;
    PQ_TRY(xs_groups_arg("pq_factor_weighted", b, group, group_stride, n_groups, XsGroupsPolicy{XS_G_WITH_CODES, "n_groups", "group"}, &grp));
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (factor && weight && out), "pq_factor_weighted: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_weighted cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_weighted (a cross-section needs every symbol on every day)");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const size_t len = (size_t)d.len;
    const int G = group ? n_groups : 1;
    const int64_t nblk = xs_nblk(d.n);
    const BdW in{factor, weight, grp, d};
    // workspace: block partials [nblk][G][len] | W [G][len]
    double *ps, *W;
    PQ_TRY(xs_ws_carve(ctx, "pq_factor_weighted", [&](XsWs &w) { w.take(ps, (size_t)nblk * G * len).take(W, G * len); }));
    const dim3 gp((unsigned)((d.len + 63) / 64), (unsigned)nblk), gc((unsigned)((d.len + 63) / 64), (unsigned)G);
    hipStream_t st = ctx->stream;
    if (group) {
        const size_t lds = (size_t)G * 64 * 8;
        PQ_HIP_TRY(hipFuncSetAttribute((const void *)bd_weighted_kernel<BD_W_GSUM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(bd_weighted_kernel<BD_W_GSUM>, gp, dim3(64), lds, st, in, ps, (const double *)nullptr, (double *)nullptr);
    } else {
        hipLaunchKernelGGL(bd_weighted_kernel<BD_W_SUM>, gp, dim3(64), 0, st, in, ps, (const double *)nullptr, (double *)nullptr);
    }
    hipLaunchKernelGGL(bd_weighted_combine_kernel, gc, dim3(64), 0, st, (const double *)ps, nblk, d.len, G, W);
    hipLaunchKernelGGL(bd_weighted_kernel<BD_W_WRITE>, gp, dim3(64), 0, st, in, (double *)nullptr, (const double *)W, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_factor_binary(pq_ctx *ctx, const pq_batch *b, const double *a, const double *bcol, int32_t op, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(op >= BD_RATIO && op <= BD_RELDIFF, "pq_factor_binary: op must be 0 (a / b), 1 (a - b) or 2 ((a - b) / |b|)");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (a && bcol && out), "pq_factor_binary: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_binary cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_binary (the columns of a factor are [n_series][stride])");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int64_t chunks = (d.len + 255) / 256, total = chunks * d.n;
    const unsigned grid = (unsigned)(total < (int64_t)1 << 20 ? total : (int64_t)1 << 20);
    hipLaunchKernelGGL(bd_binary_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, bcol, d, op, chunks, total, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
