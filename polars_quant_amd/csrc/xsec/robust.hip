// xsec/robust.hip -- IC decay, sub-period and sub-group robustness tests: Factor.ic_decay / subsample_test / subgroup_test
// (README.md:1556-1565, :1607-1624; README-only => decision D-18).
//
// Columns are symbol-major [n_series][stride].  A "view" is one row of the result: a lag l (decay: the factor of day t against the
// return of day t + l - 1) or a group g (sub-group: D-12's cross-section of day t restricted to the symbols whose code is g).  Every
// view's daily IC is bit-identical to pq_factor_ic on the shifted / masked inputs, because the order of every rounded operation is D-12's:
//  * Pearson: one thread per (day, block of 256 symbols) sums its block in ascending symbol order from 0.0, members only, for a whole
//    tile of views at once -- decay: RB_LT lags in registers, the factor read once for the tile and the lag window of the return shared
//    through the caches (consecutive lanes read consecutive days); sub-group: RB_GT groups in LDS, one [group][lane] column per lane.
//    One thread per (view, day) then adds the block sums in ascending block order, as ic_combine_kernel does.
//  * Rank-IC, n_series <= XS_LDS_MAX: each day's valid factor keys and valid return keys are sorted once (xsec_dev.h's LDS bitonic sort
//    at its launch shape xs_lds_shape, the LDS half of D-15's day-sort stage; the key load and the searches are this file's), and every
//    symbol records its tie-run start a_s = #{valid keys of the day < its key}.  Ordering by a_s is ordering by value with ties kept,
//    on any subset of the day's valid keys.  Decay: per (day, lag) a histogram c[p] = #{members with a_s = p} and its exclusive scan E
//    give 2 rank_s = 2 E[a_s] + c[a_s] + 1 over the joint members.  Sub-group: the composite key g * 2^14 + a_s of every member is sorted
//    once per side and day; rank within the group = position - the group's first position, ties kept.  Ranks are half-integers, so the
//    five rank sums are exact in any order and D-12's closed form (xs_rank_corr, xsec_dev.h) gives the same bits as pq_factor_ic.
//  * Rank-IC, n_series > XS_LDS_MAX: pq_factor_ic per lag on shifted pointers (decay) or per group on a masked copy of the factor
//    (sub-group) -- bit-identical by definition.
//  * Summary rows: rg_summary_row (xsec_ttest.h), D-17's Fama-MacBeth rules; sub-periods are numpy.array_split's contiguous slices.
#include "xsec_ttest.h"

namespace {

constexpr int RB_MAX_VIEWS = 256;    // PQ_IC_DECAY_MAX_LAG, PQ_IC_MAX_GROUPS
constexpr int RB_LT = 8;             // lags per thread (Pearson decay)
constexpr int RB_GT = 32;            // groups per LDS tile (Pearson sub-group): 3 x 32 x 64 f64 = 48 KiB
constexpr double RB_KEY_G = 16384.0; // composite key g * 2^14 + a_s, a_s < n_series <= XS_LDS_MAX: exact in f64
constexpr int RB_THR = 512;          // threads of the per-day rank workgroups
constexpr int RB_WAVES = RB_THR / 64;

__device__ __forceinline__ bool rb_valid(double a, double b) { return xs_valid(a) && xs_valid(b); }

struct RbIn {
    const double *x, *y;   // factor, forward return
    XsGroups grp;          // sub-group codes (decay: none)
    Dims d;
    int V;                 // views: lags or groups (= grp.G)
};

// ---------------------------------------------------------------- Pearson
// decay, PASS 0: n, sum x, sum y; PASS 1: the centred sums given the means.  part: [L][nblk][len][3], means: [L][len][3]
template <int PASS>
__global__ __launch_bounds__(64) void rb_decay_partial_kernel(RbIn in, const double *means, double *part) {
    const double *x = in.x, *y = in.y;
    const Dims d = in.d;
    const int L = in.V;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int64_t nblk = gridDim.y;
    const int l0 = (int)blockIdx.z * RB_LT;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    bool on[RB_LT];
    double mx[RB_LT], my[RB_LT], a0[RB_LT], a1[RB_LT], a2[RB_LT];
#pragma unroll
    for (int j = 0; j < RB_LT; j++) {
        on[j] = l0 + j < L && t + l0 + j < d.len;    // the return of day t + l - 1 exists (l = l0 + j + 1)
        a0[j] = 0.0; a1[j] = 0.0; a2[j] = 0.0; mx[j] = 0.0; my[j] = 0.0;
        if (PASS == 1 && on[j]) {
            const double *m = means + ((int64_t)(l0 + j) * d.len + t) * 3;
            mx[j] = m[1]; my[j] = m[2];
        }
    }
    constexpr int B = 2;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double a[B], b[B][RB_LT];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1;
            a[k] = x[s * d.stride + t];
#pragma unroll
            for (int j = 0; j < RB_LT; j++) b[k][j] = on[j] ? y[s * d.stride + t + l0 + j] : xs_inf();
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
#pragma unroll
            for (int j = 0; j < RB_LT; j++)
                if (rb_valid(a[k], b[k][j])) {
                    if (PASS == 0) { a0[j] += 1.0; a1[j] += a[k]; a2[j] += b[k][j]; }
                    else { const double dx = a[k] - mx[j], dy = b[k][j] - my[j]; a0[j] += dx * dy; a1[j] += dx * dx; a2[j] += dy * dy; }
                }
        }
    }
#pragma unroll
    for (int j = 0; j < RB_LT; j++)
        if (l0 + j < L) {
            double *o = part + (((int64_t)(l0 + j) * nblk + blockIdx.y) * d.len + t) * 3;
            o[0] = a0[j]; o[1] = a1[j]; o[2] = a2[j];
        }
}

// sub-group: as above with the view = the symbol's code (codes outside [0, G) are unclassified); the group sums of the workgroup's tile
// of RB_GT groups live in LDS, one column per lane
template <int PASS>
__global__ __launch_bounds__(64) void rb_group_partial_kernel(RbIn in, const double *means, double *part) {
    const double *x = in.x, *y = in.y;
    const XsGroups grp = in.grp;
    const Dims d = in.d;
    const int G = in.V;
    __shared__ double acc[3][RB_GT][64];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    if (t >= d.len) return; // no workgroup barrier below: every lane only touches its own column
    const int64_t nblk = gridDim.y;
    const int g0 = (int)blockIdx.z * RB_GT, ng = G - g0 < RB_GT ? G - g0 : RB_GT;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    for (int j = 0; j < RB_GT; j++) { acc[0][j][lane] = 0.0; acc[1][j][lane] = 0.0; acc[2][j][lane] = 0.0; }
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double a[B], b[B];
        int c[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t s = s0 + k < s_hi ? s0 + k : s_hi - 1;
            a[k] = x[s * d.stride + t]; b[k] = y[s * d.stride + t];
            c[k] = grp.at(s, t);
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            const int j = c[k] - g0;
            if (j < 0 || j >= ng || !rb_valid(a[k], b[k])) continue;
            if (PASS == 0) { acc[0][j][lane] += 1.0; acc[1][j][lane] += a[k]; acc[2][j][lane] += b[k]; }
            else {
                const double *m = means + ((int64_t)(g0 + j) * d.len + t) * 3;
                const double dx = a[k] - m[1], dy = b[k] - m[2];
                acc[0][j][lane] += dx * dy; acc[1][j][lane] += dx * dx; acc[2][j][lane] += dy * dy;
            }
        }
    }
    for (int j = 0; j < ng; j++) {
        double *o = part + (((int64_t)(g0 + j) * nblk + blockIdx.y) * d.len + t) * 3;
        o[0] = acc[0][j][lane]; o[1] = acc[1][j][lane]; o[2] = acc[2][j][lane];
    }
}

// block sums of view blockIdx.y added in ascending block order from 0.0, then D-12's means (PASS 0) or IC (PASS 1)
template <int PASS>
__global__ __launch_bounds__(64) void rb_combine_kernel(const double *part, int64_t nblk, int64_t len, double *means, double *ic,
                                                        int32_t *n_valid) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x, v = blockIdx.y;
    if (t >= len) return;
    part += v * nblk * len * 3;
    means += v * len * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t k = 0; k < nblk; k++) {
        const double *o = part + (k * len + t) * 3;
        a0 += o[0]; a1 += o[1]; a2 += o[2];
    }
    if (PASS == 0) {
        means[t * 3] = a0;
        means[t * 3 + 1] = a0 > 0.0 ? a1 / a0 : 0.0;
        means[t * 3 + 2] = a0 > 0.0 ? a2 / a0 : 0.0;
        n_valid[v * len + t] = (int32_t)a0;
    } else {
        const double n = means[t * 3];
        ic[v * len + t] = (n >= 2.0 && a1 > 0.0 && a2 > 0.0) ? a0 / (sqrt(a1) * sqrt(a2)) : pq_null();
    }
}

// ---------------------------------------------------------------- Rank-IC, n_series <= XS_LDS_MAX
// #{S[i] < key} (UPPER: <= key) in the ascending row S[0 .. P), P a power of two
template <bool UPPER> __device__ __forceinline__ int rb_search(const double *S, int P, double key) {
    int lo = 0;
    for (int step = P >> 1; step > 0; step >>= 1) {
        const double v = S[xs_phys(lo + step - 1)];
        if (UPPER ? v <= key : v < key) lo += step;
    }
    if (lo == P - 1) {
        const double v = S[xs_phys(P - 1)];
        if (UPPER ? v <= key : v < key) lo = P;
    }
    return lo;
}

// one workgroup per (day, side): A[side][t][s] = a_s, the tie-run start of the symbol's key among the day's valid keys of that side
// (side 0 the factor, 1 the return), -1 where the key is not valid
__global__ __launch_bounds__(1024) void rb_tie_start_kernel(const double *x, const double *y, Dims d, int P, int32_t *A) {
    extern __shared__ __align__(16) unsigned char rb_lds[];
    double *S = (double *)rb_lds;
    const int64_t t = blockIdx.x;
    const double *col = (blockIdx.y ? y : x) + t;
    int32_t *out = A + ((int64_t)blockIdx.y * d.len + t) * d.n;
    const int tid = threadIdx.x, nthr = blockDim.x, n = (int)d.n;
    for (int i = tid; i < P; i += nthr) {
        double v = xs_inf();
        if (i < n) {
            v = col[(int64_t)i * d.stride];
            if (!xs_valid(v)) v = xs_inf();
        }
        S[xs_phys(i)] = v;
    }
    __syncthreads();
    xs_sort_lds(S, P, n, tid, nthr);
    for (int s = tid; s < n; s += nthr) {
        const double v = col[(int64_t)s * d.stride];
        out[s] = xs_valid(v) ? rb_search<false>(S, P, v) : -1;
    }
}

// in-place exclusive scan of cx[0 .. n) and cy[0 .. n) over the workgroup (RB_THR threads, a contiguous chunk per thread) -> the totals
__device__ void rb_scan2(int32_t *cx, int32_t *cy, int n, int32_t (&wsum)[2][RB_WAVES], int &tx, int &ty) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ch = (n + RB_THR - 1) / RB_THR;
    const int lo = tid * ch < n ? tid * ch : n, hi = lo + ch < n ? lo + ch : n;
    int sx = 0, sy = 0;
    for (int i = lo; i < hi; i++) { sx += cx[i]; sy += cy[i]; }
    int ix = sx, iy = sy;
    for (int o = 1; o < 64; o <<= 1) {
        const int ux = __shfl_up(ix, o, 64), uy = __shfl_up(iy, o, 64);
        if (lane >= o) { ix += ux; iy += uy; }
    }
    if (lane == 63) { wsum[0][w] = ix; wsum[1][w] = iy; }
    __syncthreads();
    int bx = 0, by = 0;
    tx = 0; ty = 0;
    for (int k = 0; k < RB_WAVES; k++) {
        if (k < w) { bx += wsum[0][k]; by += wsum[1][k]; }
        tx += wsum[0][k]; ty += wsum[1][k];
    }
    int ex = bx + ix - sx, ey = by + iy - sy;
    for (int i = lo; i < hi; i++) {
        const int vx = cx[i], vy = cy[i];
        cx[i] = ex; cy[i] = ey;
        ex += vx; ey += vy;
    }
    __syncthreads();
}

// the five rank sums (2 x ranks) of the workgroup -> D-12's closed form, by thread 0
__device__ double rb_rank_close(unsigned long long (&v)[5], int nv, unsigned long long (&red)[RB_WAVES][5]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 5; k++)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if ((tid & 63) == 0)
        for (int k = 0; k < 5; k++) red[tid >> 6][k] = v[k];
    __syncthreads();
    double out = pq_null();
    if (tid == 0) {
        for (int w = 1; w < RB_WAVES; w++)
            for (int k = 0; k < 5; k++) v[k] += red[w][k];
        out = xs_rank_corr(nv, v[0], v[1], v[2], v[3], v[4]);
    }
    __syncthreads(); // red is reused
    return out;
}

// decay, one workgroup per day t, every lag in turn: histograms of a_s over the joint members (factor of day t, return of day t + l - 1)
__global__ __launch_bounds__(RB_THR) void rb_decay_rank_kernel(const int32_t *A, Dims d, int L, double *ic, int32_t *n_valid) {
    extern __shared__ __align__(16) unsigned char rb_lds[];
    __shared__ int32_t wsum[2][RB_WAVES];
    __shared__ unsigned long long red[RB_WAVES][5];
    const int n = (int)d.n, tid = threadIdx.x;
    int32_t *cx = (int32_t *)rb_lds, *cy = cx + n;
    const int64_t t = blockIdx.x;
    const int32_t *ax = A + t * n;
    for (int l = 1; l <= L; l++) {
        const int64_t u = t + l - 1, o = (int64_t)(l - 1) * d.len + t;
        if (u >= d.len) { // uniform over the workgroup
            if (tid == 0) { ic[o] = pq_null(); n_valid[o] = 0; }
            continue;
        }
        const int32_t *ay = A + (d.len + u) * n;
        for (int i = tid; i < n; i += RB_THR) { cx[i] = 0; cy[i] = 0; }
        __syncthreads();
        for (int s = tid; s < n; s += RB_THR) {
            const int a = ax[s], b = ay[s];
            if (a >= 0 && b >= 0) { atomicAdd(&cx[a], 1); atomicAdd(&cy[b], 1); }
        }
        __syncthreads();
        int nv, nvy;
        rb_scan2(cx, cy, n, wsum, nv, nvy);
        unsigned long long v[5] = {0, 0, 0, 0, 0};
        for (int s = tid; s < n; s += RB_THR) {
            const int a = ax[s], b = ay[s];
            if (a < 0 || b < 0) continue;
            const int ea = cx[a], eb = cy[b];
            const unsigned long long rx = (unsigned)(2 * ea + ((a + 1 < n ? cx[a + 1] : nv) - ea) + 1),
                                     ry = (unsigned)(2 * eb + ((b + 1 < n ? cy[b + 1] : nv) - eb) + 1);
            v[0] += rx; v[1] += ry; v[2] += rx * rx; v[3] += ry * ry; v[4] += rx * ry;
        }
        const double r = rb_rank_close(v, nv, red);
        if (tid == 0) { ic[o] = r; n_valid[o] = nv; }
    }
}

// sub-group, one workgroup per day t: per side, the composite keys g * 2^14 + a_s of the members (valid pair, code in [0, G)) sorted in
// LDS; 2 x the rank within the group = 2 (lower - group start) + (upper - lower) + 1.  The factor side's ranks wait in R2 (day-major,
// read back by the thread that wrote them); the group sums are LDS atomics on exact integers.  (code, cstride, G), not XsGroups: see there.
__global__ __launch_bounds__(RB_THR) void rb_group_rank_kernel(const int32_t *A, const int32_t *code, int64_t cstride, Dims d, int G, int P,
                                                               int32_t *R2, double *ic, int32_t *n_valid) {
    extern __shared__ __align__(16) unsigned char rb_lds[];
    __shared__ unsigned long long gs[RB_MAX_VIEWS][5];
    __shared__ int gcnt[RB_MAX_VIEWS];
    double *S = (double *)rb_lds;
    const int n = (int)d.n, tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int32_t *ax = A + t * n, *ay = A + (d.len + t) * n;
    int32_t *r2 = R2 + t * n;
    for (int g = tid; g < G; g += RB_THR) {
        for (int k = 0; k < 5; k++) gs[g][k] = 0;
        gcnt[g] = 0;
    }
    for (int side = 0; side < 2; side++) {
        const int32_t *as = side ? ay : ax;
        for (int i = tid; i < P; i += RB_THR) {
            double key = xs_inf();
            if (i < n) {
                const int c = code[cstride ? (int64_t)i * cstride + t : i];
                if (ax[i] >= 0 && ay[i] >= 0 && c >= 0 && c < G) key = (double)c * RB_KEY_G + (double)as[i];
            }
            S[xs_phys(i)] = key;
        }
        __syncthreads();
        xs_sort_lds(S, P, n, tid, RB_THR);
        for (int s = tid; s < n; s += RB_THR) {
            const int c = code[cstride ? (int64_t)s * cstride + t : s];
            if (ax[s] < 0 || ay[s] < 0 || c < 0 || c >= G) continue;
            const double key = (double)c * RB_KEY_G + (double)as[s];
            const int lo = rb_search<false>(S, P, key), hi = rb_search<true>(S, P, key), g0 = rb_search<false>(S, P, (double)c * RB_KEY_G);
            const int rr = 2 * (lo - g0) + (hi - lo) + 1;
            if (side == 0) { r2[s] = rr; continue; }
            const unsigned long long rx = (unsigned)r2[s], ry = (unsigned)rr;
            atomicAdd(&gs[c][0], rx); atomicAdd(&gs[c][1], ry); atomicAdd(&gs[c][2], rx * rx); atomicAdd(&gs[c][3], ry * ry);
            atomicAdd(&gs[c][4], rx * ry); atomicAdd(&gcnt[c], 1);
        }
        __syncthreads();
    }
    for (int g = tid; g < G; g += RB_THR) {
        const int nv = gcnt[g];
        ic[(int64_t)g * d.len + t] = xs_rank_corr(nv, gs[g][0], gs[g][1], gs[g][2], gs[g][3], gs[g][4]);
        n_valid[(int64_t)g * d.len + t] = nv;
    }
}

// ---------------------------------------------------------------- wide rank fallbacks, summaries
// decay rows: NULL / 0 on the days t > len - l that have no return l - 1 days ahead
__global__ __launch_bounds__(256) void rb_decay_tail_kernel(int L, int64_t len, double *ic, int32_t *n_valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)L * len) return;
    const int64_t l = i / len + 1, t = i % len;
    if (t + l - 1 >= len) { ic[i] = pq_null(); n_valid[i] = 0; }
}

// out = the factor where code == g, NULL elsewhere (same layout)
__global__ __launch_bounds__(256) void rb_mask_kernel(const double *x, const int32_t *code, int64_t cstride, Dims d, int g, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n * d.len) return;
    const int64_t s = i / d.len, t = i % d.len, o = s * d.stride + t;
    out[o] = code[cstride ? s * cstride + t : s] == g ? x[o] : pq_null();
}

// one 64-lane workgroup per period p of numpy.array_split(range(len), P): the summary row of x over the period
__global__ __launch_bounds__(64) void rb_split_summary_kernel(const double *x, int64_t len, int32_t P, double *summary) {
    __shared__ double buf[XS_CHUNK];
    const int64_t p = blockIdx.x, q = len / P, r = len % P;
    const int64_t start = p * q + (p < r ? p : r), size = q + (p < r ? 1 : 0);
    rg_summary_row(x + start, size, buf, summary + p * RG_SUMMARY_COLS);
}

pq_status rb_args(pq_ctx *ctx, const pq_batch *b, const char *what, const double *factor, const double *ret, int32_t method, int32_t views,
                  const void *ic, const void *nv, const void *summary) {
    PQ_TRY(pq_check(ctx, b));
    if (ctx->rec) { pq_set_error("%s cannot be recorded into a suite", what); return PQ_ERR_UNSUPPORTED; }
    if (b->offsets) { pq_set_error("%s: ragged batches are not supported", what); return PQ_ERR_UNSUPPORTED; }
    if (method != 0 && method != 1) { pq_set_error("%s: method must be 0 (Pearson IC) or 1 (Spearman Rank-IC)", what); return PQ_ERR_ARG; }
    if (views < 1 || views > RB_MAX_VIEWS) { pq_set_error("%s: max_lag / n_groups must be in [1, 256]", what); return PQ_ERR_ARG; }
    if (!summary || (b->len > 0 && (!ic || !nv)) || (b->len > 0 && b->n_series > 0 && (!factor || !ret))) {
        pq_set_error("%s: null pointer", what);
        return PQ_ERR_ARG;
    }
    if (method == 1 && b->n_series > 100000) { pq_set_error("%s: Rank-IC supports at most 100000 series", what); return PQ_ERR_ARG; }
    return PQ_OK;
}

// the Pearson passes over the views: one thread per (day, block of 256 symbols, tile of views), then one per (view, day)
template <bool GROUP>
pq_status rb_pearson(pq_ctx *ctx, const RbIn &in, int tile, double *ic, int32_t *n_valid) {
    const Dims d = in.d;
    const int V = in.V;
    const int64_t nblk = xs_nblk(d.n);
    const dim3 gp((unsigned)((d.len + 63) / 64), (unsigned)nblk, (unsigned)((V + tile - 1) / tile));
    double *ps, *ms;
    PQ_TRY(xs_ws_carve(ctx, GROUP ? "pq_ic_subgroup" : "pq_ic_decay", [&](XsWs &w) { w.take(ps, (size_t)V * nblk * d.len * 3).take(ms, (size_t)V * d.len * 3); }));
    const dim3 gc((unsigned)((d.len + 63) / 64), (unsigned)V);
    hipStream_t st = ctx->stream;
    if (GROUP) hipLaunchKernelGGL(rb_group_partial_kernel<0>, gp, dim3(64), 0, st, in, (const double *)ms, ps);
    else hipLaunchKernelGGL(rb_decay_partial_kernel<0>, gp, dim3(64), 0, st, in, (const double *)ms, ps);
    hipLaunchKernelGGL(rb_combine_kernel<0>, gc, dim3(64), 0, st, (const double *)ps, nblk, d.len, ms, ic, n_valid);
    if (GROUP) hipLaunchKernelGGL(rb_group_partial_kernel<1>, gp, dim3(64), 0, st, in, (const double *)ms, ps);
    else hipLaunchKernelGGL(rb_decay_partial_kernel<1>, gp, dim3(64), 0, st, in, (const double *)ms, ps);
    hipLaunchKernelGGL(rb_combine_kernel<1>, gc, dim3(64), 0, st, (const double *)ps, nblk, d.len, ms, ic, n_valid);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

// workspace: A (tie-run starts of both sides, [2][len][n] int32) | `extra` further int32 (R2)
pq_status rb_tie_starts(pq_ctx *ctx, const Dims &d, const double *factor, const double *ret, size_t extra, int32_t *&A, int32_t *&rest) {
    PQ_TRY(xs_ws_carve(ctx, extra ? "pq_ic_subgroup" : "pq_ic_decay", [&](XsWs &w) { w.take(A, (size_t)2 * d.len * d.n).take(rest, extra); }));
    const XsLds sh = xs_lds_shape(d.n);
    PQ_HIP_TRY(hipFuncSetAttribute((const void *)rb_tie_start_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.bytes));
    hipLaunchKernelGGL(rb_tie_start_kernel, dim3((unsigned)d.len, 2), dim3(sh.nthr), sh.bytes, ctx->stream, factor, ret, d, sh.P, A);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status rb_summaries(pq_ctx *ctx, const double *ic, int64_t len, int V, double *summary) {
    hipLaunchKernelGGL(rg_summary_kernel, dim3((unsigned)V), dim3(64), 0, ctx->stream, ic, len, summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_ic_decay(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, int32_t method, int32_t max_lag,
                      double *ic, int32_t *n_valid, double *summary) {
    PQ_TRY(rb_args(ctx, b, "pq_ic_decay", factor, fwd_return, method, max_lag, ic, n_valid, summary));
    const Dims d = dims_of(b);
    const int L = max_lag;
    if (d.len > 0) {
        if (method == 0 || d.n == 0) {
            PQ_TRY(rb_pearson<false>(ctx, RbIn{factor, fwd_return, XsGroups{nullptr, 0, 0}, d, L}, RB_LT, ic, n_valid));
        } else if (d.n <= XS_LDS_MAX) {
            int32_t *A, *rest;
            PQ_TRY(rb_tie_starts(ctx, d, factor, fwd_return, 0, A, rest));
            const size_t lds = (size_t)2 * d.n * 4;
            PQ_HIP_TRY(hipFuncSetAttribute((const void *)rb_decay_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(rb_decay_rank_kernel, dim3((unsigned)d.len), dim3(RB_THR), lds, ctx->stream, (const int32_t *)A, d, L, ic, n_valid);
            PQ_HIP_TRY(hipGetLastError());
        } else { // wide: D-12's own Rank-IC on the shifted views
            for (int l = 1; l <= L && l <= d.len; l++) {
                pq_batch bl = *b;
                bl.len = d.len - l + 1;
                PQ_TRY(pq_factor_ic(ctx, &bl, factor, fwd_return + (l - 1), 1, ic + (int64_t)(l - 1) * d.len, n_valid + (int64_t)(l - 1) * d.len));
            }
            const int64_t cells = (int64_t)L * d.len;
            hipLaunchKernelGGL(rb_decay_tail_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, L, d.len, ic, n_valid);
            PQ_HIP_TRY(hipGetLastError());
        }
    } else {
        PQ_HIP_TRY(hipSetDevice(ctx->device));
    }
    return rb_summaries(ctx, ic, d.len, L, summary);
}

pq_status pq_ic_subgroup(pq_ctx *ctx, const pq_batch *b, const double *factor, const double *fwd_return, const int32_t *group,
                         int64_t group_stride, int32_t n_groups, int32_t method, double *ic, int32_t *n_valid, double *summary) {
    PQ_TRY(rb_args(ctx, b, "pq_ic_subgroup", factor, fwd_return, method, n_groups, ic, n_valid, summary));
    PQ_REQUIRE(b->len == 0 || b->n_series == 0 || group, "pq_ic_subgroup: null group pointer");
    XsGroups grp;   // the count is one of rb_args' views
    PQ_TRY(xs_groups_arg("pq_ic_subgroup", b, group, group_stride, n_groups, XsGroupsPolicy{XS_G_REQUIRED, "n_groups", "group"}, &grp));
    const Dims d = dims_of(b);
    const int G = n_groups;
    if (d.len > 0) {
        if (method == 0 || d.n == 0) {
            PQ_TRY(rb_pearson<true>(ctx, RbIn{factor, fwd_return, grp, d, G}, RB_GT, ic, n_valid));
        } else if (d.n <= XS_LDS_MAX) {
            int32_t *A, *R2;
            PQ_TRY(rb_tie_starts(ctx, d, factor, fwd_return, (size_t)d.len * d.n, A, R2));
            const XsLds sh = xs_lds_shape(d.n);   // the row's P and bytes; the workgroup is RB_THR threads whatever P
            PQ_HIP_TRY(hipFuncSetAttribute((const void *)rb_group_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.bytes));
            hipLaunchKernelGGL(rb_group_rank_kernel, dim3((unsigned)d.len), dim3(RB_THR), sh.bytes, ctx->stream, (const int32_t *)A, grp.codes,
                               grp.stride, d, G, sh.P, R2, ic, n_valid);
            PQ_HIP_TRY(hipGetLastError());
        } else { // wide: D-12's own Rank-IC on the factor masked to each group
            double *masked = nullptr;
            PQ_HIP_TRY(hipSetDevice(ctx->device));
            const size_t bytes = (size_t)d.n * d.stride * 8;
            if (hipMalloc(&masked, bytes) != hipSuccess) { pq_set_error("pq_ic_subgroup: hipMalloc(%zu) failed", bytes); return PQ_ERR_NOMEM; }
            pq_status st = PQ_OK;
            const int64_t cells = d.n * d.len;
            for (int g = 0; g < G && st == PQ_OK; g++) {
                hipLaunchKernelGGL(rb_mask_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, factor, grp.codes, grp.stride,
                                   d, g, masked);
                st = hipGetLastError() == hipSuccess ? PQ_OK : PQ_ERR_HIP;
                if (st != PQ_OK) pq_set_error("pq_ic_subgroup: mask launch failed");
                else st = pq_factor_ic(ctx, b, masked, fwd_return, 1, ic + (int64_t)g * d.len, n_valid + (int64_t)g * d.len);
            }
            const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipFree(masked);
            PQ_TRY(st);
            PQ_HIP_TRY(e1);
            PQ_HIP_TRY(e2);
        }
    } else {
        PQ_HIP_TRY(hipSetDevice(ctx->device));
    }
    return rb_summaries(ctx, ic, d.len, G, summary);
}

pq_status pq_series_split_summary(pq_ctx *ctx, const double *x, int64_t len, int32_t n_splits, double *summary) {
    PQ_REQUIRE(ctx, "pq_series_split_summary: null context");
    PQ_REQUIRE(len >= 1 && n_splits >= 1 && n_splits <= len, "pq_series_split_summary: need 1 <= n_splits <= len");
    PQ_REQUIRE(x && summary, "pq_series_split_summary: null pointer");
    if (ctx->rec) { pq_set_error("pq_series_split_summary cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rb_split_summary_kernel, dim3((unsigned)n_splits), dim3(64), 0, ctx->stream, x, len, n_splits, summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
