// xsec/xsec_dev.h -- helpers shared by the cross-sectional kernels: the summation block and its count (every file), the day-sort stage
// of D-15 (sorts.hip, double_sort.hip: D-31, clean.hip: D-16, build.hip: D-20, and its LDS half also robust.hip: D-18) -- the prep transpose to day-major keys,
// the LDS bitonic sort of one day's keys and its launch shape, the row accessor and the tie-run search on a sorted row, the
// sort-then-look-up kernel pair with its host dispatch (sorts.hip, double_sort.hip, build.hip), and the host interface of daysort.hip for
// rows too wide for LDS --, the host interface of the cells stage of sorts.hip (labels -> per-cell statistics -> summary; also
// double_sort.hip), D-12's rank closed form (robust.hip) and the sequential summaries (sorts.hip, xsec_ttest.h).  The OLS core of
// regress.hip (D-17) and orth.hip (D-19) is xsec_ols.h.  Host scaffolding of the entry points: xs_ws_carve reserves and binds a call's workspace
// from one description of its spans (XsWs, xsec_ws.h); XsGroups and xs_groups_arg are the group (industry) codes argument (fetch, membership, checks).
#pragma once
#include "../pq_dev.h"
#include "xsec_ws.h"

namespace {

constexpr int XS_BLOCK = 256;      // D-12 / D-15 summation block (symbols)
constexpr int XS_LDS_MAX = 16384;  // widest cross-section sorted in LDS: 16 384 f64 keys = 128 KiB of the CU's 160 KiB
constexpr int XS_CHUNK = 2048;     // days staged in LDS per step of the sequential summaries

__device__ __forceinline__ double xs_inf() { return __longlong_as_double(0x7FF0000000000000LL); }
__device__ __forceinline__ bool xs_valid(double v) { return !pq_isnull(v) && isfinite(v); }

// LDS rows carry one pad slot per 16 keys, so that the 16-key chunks of consecutive lanes start on different banks
__device__ __forceinline__ int xs_phys(int i) { return i + (i >> 4); }

// All-ascending bitonic network over S[0 .. P) (P = 2^p >= 16): the first stage of the merge of size k pairs i with its mirror
// i ^ (k-1), the later stages are half-cleaners i, i + j.  S[n .. P) holds +inf and keeps it (the larger key always goes to the
// larger index), so a pair or a 16-key chunk that only touches indices >= n changes nothing and is skipped.  Every stage whose pairs
// lie inside one aligned 16-key chunk runs in registers -- merges of 2 .. 16 keys entirely, and the last four stages (j = 8 .. 1) of
// every larger merge -- so a workgroup barrier is paid for each stage with j >= 16 and once per merge for the register pass: 65
// barriers instead of 105 at P = 16 384.
__device__ __forceinline__ void xs_cx(double &a, double &b) { // a <= b afterwards (keys are never NaN)
    const bool sw = b < a;
    const double lo = sw ? b : a, hi = sw ? a : b;
    a = lo; b = hi;
}
template <bool FULL> __device__ __forceinline__ void xs_chunk(double *S, int c) {
    double r[16];
#pragma unroll
    for (int m = 0; m < 16; m++) r[m] = S[xs_phys(c * 16 + m)];
    if (FULL) {
#pragma unroll
        for (int k = 2; k <= 16; k <<= 1) {
#pragma unroll
            for (int m = 0; m < 16; m++)
                if (!(m & (k >> 1))) xs_cx(r[m], r[m ^ (k - 1)]);
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1)
#pragma unroll
                for (int m = 0; m < 16; m++)
                    if (!(m & j)) xs_cx(r[m], r[m | j]);
        }
    } else {
#pragma unroll
        for (int j = 8; j > 0; j >>= 1)
#pragma unroll
            for (int m = 0; m < 16; m++)
                if (!(m & j)) xs_cx(r[m], r[m | j]);
    }
#pragma unroll
    for (int m = 0; m < 16; m++) S[xs_phys(c * 16 + m)] = r[m];
}
__device__ __forceinline__ void xs_sort_lds(double *S, int P, int n, int tid, int nthr) {
    const int nchunk = P >> 4;
    for (int c = tid; c < nchunk && c * 16 < n; c += nthr) xs_chunk<true>(S, c);
    __syncthreads();
    for (int k = 32; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 16; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (int q = tid; q < (P >> 1); q += nthr) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)); // grows with q
                if (i >= n) break;
                const int p = mirror ? (i ^ (k - 1)) : (i + j);
                if (p < n) {
                    const int pi = xs_phys(i), pp = xs_phys(p);
                    const double a = S[pi], b = S[pp];
                    if (b < a) { S[pi] = b; S[pp] = a; }
                }
            }
            __syncthreads();
        }
        for (int c = tid; c < nchunk && c * 16 < n; c += nthr) xs_chunk<false>(S, c);
        __syncthreads();
    }
}

// S[0 .. P) <- row[0 .. n) with a +inf tail, sorted ascending (one workgroup; S is an LDS row of xs_lds_shape(n).bytes)
__device__ __forceinline__ void xs_load_sort_row(double *S, const double *row, int64_t n, int P, int tid, int nthr) {
    for (int i = tid; i < P; i += nthr) S[xs_phys(i)] = i < n ? row[i] : xs_inf();
    __syncthreads();
    xs_sort_lds(S, P, (int)n, tid, nthr);
}

// [n][stride] columns -> NK day-major [len][n] key rows, `pitch` doubles apart, and n per day.  key(o, k) sets k[0 .. NK) to the keys of the
// cell at offset o = s * stride + t and leaves them +inf where the cell is not in the day's sample (the same sample for every row: it is
// counted on row 0); the callers differ only in it.  32 x 32 tiles, LDS rows padded to 33 words.
template <int NK, class Key>
__global__ __launch_bounds__(256) void xs_prep_kernel(Key key, Dims d, double *out, int64_t pitch, int32_t *n_valid) {
    __shared__ double tile[NK][32][33];
    __shared__ int cnt[32];
    const int64_t t0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5; // 32 x 8
    if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
    for (int i = ly; i < 32; i += 8) { // rows = symbols, lanes along days (coalesced reads)
        const int64_t s = s0 + i, t = t0 + lx;
        double k[NK];
#pragma unroll
        for (int j = 0; j < NK; j++) k[j] = xs_inf();
        if (s < d.n && t < d.len) key(s * d.stride + t, k);
#pragma unroll
        for (int j = 0; j < NK; j++) tile[j][i][lx] = k[j];
    }
    __syncthreads();
    for (int i = ly; i < 32; i += 8) { // rows = days, lanes along symbols (coalesced writes)
        const int64_t t = t0 + i, s = s0 + lx;
        if (t < d.len && s < d.n) {
#pragma unroll
            for (int j = 0; j < NK; j++) out[j * pitch + t * d.n + s] = tile[j][lx][i];
            if (tile[0][lx][i] != xs_inf()) atomicAdd(&cnt[i], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && t0 + threadIdx.x < d.len && cnt[threadIdx.x]) atomicAdd(&n_valid[t0 + threadIdx.x], cnt[threadIdx.x]);
}

// one sorted day: an LDS row indexed through xs_phys (PAD) or a plain global row
template <bool PAD> struct XsRow {
    const double *S;
    __device__ __forceinline__ double operator()(int i) const { return S[PAD ? xs_phys(i) : i]; }
};

// m = a + b for the tie run [a, b) of `key` in the ascending row S[0 .. nv) (key is one of its entries, -0 == +0): binary searches only,
// so a discrete factor's runs of thousands of equal keys cost O(log nv) per symbol, not O(run); the second search is skipped where the
// next entry already differs.  Ties share m and nothing depends on sort stability.
template <bool PAD> __device__ __forceinline__ int64_t xs_tie_run(XsRow<PAD> S, int nv, double key) {
    int lo = 0, hi = nv;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (S(mid) < key) lo = mid + 1; else hi = mid; }
    const int a = lo;
    int b = a + 1;
    if (b < nv && S(b) == key) {
        lo = b + 1; hi = nv;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (S(mid) <= key) lo = mid + 1; else hi = mid; }
        b = lo;
    }
    return (int64_t)a + (int64_t)b;
}

// The sort-then-look-up kernel pair: sort one day's key row, then let every symbol look itself up in the sorted row.  What is looked
// up and where it goes is the file's operation Op:
//   MAX_STEPS, steps()     1 .. 3 sorts per day, each followed by one look-up per symbol; steps() <= MAX_STEPS may depend on the call
//   row(step)              the day-major [len][n] key rows that step sorts
//   unsorted(nv)           the day is not sorted at all (uniform across the workgroup); fill(i) is what cell i = t * n + s gets then
//   at(step, S, nv, i)     the look-up of cell i in the sorted row S[0 .. nv); a later step may read what an earlier one wrote to cell i
// one workgroup per day, n <= XS_LDS_MAX: every step sorts its row in the same LDS row
template <class Op> __global__ __launch_bounds__(1024) void xs_sort_lds_kernel(Op op, const int32_t *n_valid, int64_t n, int P) {
    extern __shared__ __align__(16) unsigned char xs_lds[];
    double *S = (double *)xs_lds;
    const int64_t o = (int64_t)blockIdx.x * n;
    const int tid = threadIdx.x, nthr = blockDim.x, nv = n_valid[blockIdx.x];
    if (op.unsorted(nv)) {
        for (int s = tid; s < n; s += nthr) op.fill(o + s);
        return;
    }
#pragma unroll
    for (int step = 0; step < Op::MAX_STEPS; step++) {
        if (step >= op.steps()) break;
        if (step) __syncthreads(); // every search of the row before is done before the LDS row is loaded again
        xs_load_sort_row(S, op.row(step) + o, n, P, tid, nthr); // thread tid loads the cells tid, tid + nthr, ...: the ones it writes below
        for (int s = tid; s < n; s += nthr) op.at(step, XsRow<true>{S}, nv, o + s);
    }
}
// n > XS_LDS_MAX: step's rows were sorted by rocPRIM (sorted); one launch per step.  A day that is not sorted is filled by step 0 and
// left alone by the later steps.
template <class Op>
__global__ __launch_bounds__(256) void xs_sort_wide_kernel(Op op, int step, const double *sorted, const int32_t *n_valid, int64_t n) {
    const int64_t o = (int64_t)blockIdx.x * n;
    const int nv = n_valid[blockIdx.x];
    if (op.unsorted(nv)) {
        if (step == 0)
            for (int64_t s = threadIdx.x; s < n; s += 256) op.fill(o + s);
        return;
    }
    for (int64_t s = threadIdx.x; s < n; s += 256) op.at(step, XsRow<false>{sorted + o}, nv, o + s);
}

// Sequential statistics of a series x[0 .. len) over its non-NaN entries, in ascending order from 0.0.  SQ = false: count, sum and
// count of entries > 0; SQ = true: sum of (x - center)^2.  The 64 lanes stage XS_CHUNK terms at a time in LDS -- the entry (or its
// square deviation), +0.0 for a NaN entry -- and count in parallel (integers: any order); lane 0 adds the staged terms in order.
// A +0.0 term leaves the sum unchanged: it starts at +0.0, and a round-to-nearest sum that starts there is never -0.0.  Sum and
// counts are returned in every lane.
template <bool SQ>
__device__ void xs_seq(const double *x, int64_t len, double center, double *buf, double &acc, int64_t &n, int64_t &pos) {
    acc = 0.0;
    long long cn = 0, cp = 0;
    for (int64_t c0 = 0; c0 < len; c0 += XS_CHUNK) {
        const int64_t m = len - c0 < XS_CHUNK ? len - c0 : XS_CHUNK, m8 = (m + 7) & ~7LL;
        for (int64_t i0 = threadIdx.x; i0 < m8; i0 += 64 * 8) { // eight global loads in flight per lane
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int64_t i = i0 + k * 64;
                v[k] = i < m ? x[c0 + i] : __longlong_as_double(0x7FF8000000000000LL);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool ok = v[k] == v[k];
                cn += ok;
                if (!SQ) cp += v[k] > 0.0;
                const double dv = v[k] - center;
                if (i0 + k * 64 < m8) buf[i0 + k * 64] = ok ? (SQ ? dv * dv : v[k]) : 0.0;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int64_t i = 0; i < m8; i += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = buf[i + k];
#pragma unroll
                for (int k = 0; k < 8; k++) acc += v[k];
            }
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) { cn += __shfl_xor(cn, o, 64); cp += __shfl_xor(cp, o, 64); }
    n = cn; pos = cp;
    acc = __shfl(acc, 0, 64); // the next pass centres on the mean in every lane
}

// D-12's closed form: the correlation of nv ranks from the five integer sums of 2 x rank (x, y, x x, y y, x y); NULL below two members
// or where a side is constant.  csrc/factor.hip keeps its own copy (its files are hashed into the committed counter profile).
__device__ __forceinline__ double xs_rank_corr(int nv, unsigned long long sx, unsigned long long sy, unsigned long long sxx,
                                               unsigned long long syy, unsigned long long sxy) {
    if (nv < 2) return pq_null();
    const double nn = (double)nv, Sx = (double)sx / 2.0, Sy = (double)sy / 2.0, Sxx = (double)sxx / 4.0, Syy = (double)syy / 4.0,
                 Sxy = (double)sxy / 4.0;
    const double vx = nn * Sxx - Sx * Sx, vy = nn * Syy - Sy * Sy;
    return vx > 0.0 && vy > 0.0 ? (nn * Sxy - Sx * Sy) / (sqrt(vx) * sqrt(vy)) : pq_null();
}

// summation blocks over `span` indices, at least one (an empty span still gets its zero sums written)
inline int64_t xs_nblk(int64_t span) { return span > XS_BLOCK ? (span + XS_BLOCK - 1) / XS_BLOCK : 1; }
// `carve(XsWs &)` takes a call's spans in order: run on a null base to measure, then on ctx->ws to bind (one description, so they agree)
template <class F> pq_status xs_ws_carve(pq_ctx *ctx, const char *what, F &&carve) {
    XsWs measure{nullptr}, bind{nullptr};
    carve(measure);
    if (measure.bad) { pq_set_error("%s: the workspace does not fit size_t", what); return PQ_ERR_ARG; }
    PQ_TRY(pq_ws_reserve(ctx, measure.off));
    bind.base = (unsigned char *)ctx->ws;
    carve(bind);
    return PQ_OK;
}
constexpr int XS_MAX_GROUPS = PQ_IC_MAX_GROUPS;   // group (industry) codes: the one limit of every entry that takes them
// int32 codes, one per symbol (stride 0) or per cell, `stride` codes from symbol to symbol; outside [0, G): unclassified.  Null codes keep the
// file's meaning: group 0 (wls.hip, risk.hip) or no grouping (build.hip, clean.hip).  Kernels that compile to other code through the members keep
// the fetch or test written out (EXPERIMENTS.md): cl_member, bd_w_member, rk_pf_pass1_kernel, wl_pass_kernel's clamp, rb_group_rank / rb_mask_kernel.
struct XsGroups {
    const int32_t *codes; int64_t stride; int32_t G;
    __device__ __forceinline__ int32_t at(int64_t s, int64_t t) const { return codes[stride ? s * stride + t : s]; }
    __device__ __forceinline__ int32_t at_cell(int64_t o) const { return codes[o]; }   // codes on the columns' own stride: the cell at offset o
    __device__ __forceinline__ bool has(int32_t g) const { return g >= 0 && g < G; }
};
// The host checks, messages prefixed with `what` and worded with the entry's names for its count and codes.  XS_G_REQUIRED: the entry needs
// codes and checks the count itself (pq_ic_subgroup, in rb_args), the stride is checked whatever the pointer; XS_G_WITH_CODES: the count is checked
// with codes, ignored without (G = 0); XS_G_ALWAYS: checked always, 1 without codes, and the entry calls xs_groups_stride behind its own refusals.
enum XsGroupsCount { XS_G_REQUIRED, XS_G_WITH_CODES, XS_G_ALWAYS };
struct XsGroupsPolicy { XsGroupsCount mode; const char *count, *codes; };
inline pq_status xs_groups_stride(const char *what, const pq_batch *b, bool checked, int64_t stride) {
    if (!checked || stride == 0 || stride >= b->len) return PQ_OK;
    pq_set_error("%s: group_stride must be 0 ([n_series] codes) or >= len", what);
    return PQ_ERR_ARG;
}
inline pq_status xs_groups_arg(const char *what, const pq_batch *b, const int32_t *codes, int64_t stride, int32_t n_groups,
                               const XsGroupsPolicy &policy, XsGroups *out) {
    *out = XsGroups{codes, codes ? stride : 0, policy.mode == XS_G_WITH_CODES && !codes ? 0 : n_groups};
    if ((policy.mode == XS_G_ALWAYS || (policy.mode == XS_G_WITH_CODES && codes)) && (n_groups < 1 || n_groups > XS_MAX_GROUPS))
        pq_set_error("%s: %s must be in [1, %d]", what, policy.count, XS_MAX_GROUPS);
    else if (policy.mode == XS_G_ALWAYS && !codes && n_groups != 1)
        pq_set_error("%s: %s must be 1 without %s codes", what, policy.count, policy.codes);
    else return policy.mode == XS_G_ALWAYS ? PQ_OK : xs_groups_stride(what, b, codes || policy.mode == XS_G_REQUIRED, stride);
    return PQ_ERR_ARG;
}
// The as-of days of the risk entries (risk.hip: D-33, risk_solve.hip: D-34): day d = day0 + d * step, d = 0 .. count - 1, checked against the
// batch's length; *a gets a step that no kernel can overflow on (a lone day has no step)
struct RkDays { int64_t day0, step, count; };
inline pq_status rk_days(const char *what, int64_t len, int64_t day0, int64_t step, int64_t count, RkDays *a) {
    if (day0 < 0 || step < 1 || count < 0 || (count > 0 && (day0 >= len || (count - 1) > (len - 1 - day0) / step))) {
        pq_set_error("%s: the as-of days need day0 >= 0, step >= 1, count >= 0 and day0 + (count - 1) * step < len", what);
        return PQ_ERR_ARG;
    }
    *a = RkDays{day0, count > 1 ? step : 1, count};
    return PQ_OK;
}
__device__ __forceinline__ double rk_nan_null(double v) { return v == v ? v : pq_null(); }
} // namespace

// ---------------------------------------------------------------- host side of the day sort (daysort.hip)
// launch shape of a kernel that sorts one day of n <= XS_LDS_MAX keys in LDS: P = the power of two >= max(16, n), one thread per 16-key
// chunk clamped to 64 .. 1024, and the padded row's bytes
struct XsLds { int P, nthr; size_t bytes; };
inline XsLds xs_lds_shape(int64_t n) {
    int P = 16;
    while (P < n) P <<= 1;
    return XsLds{P, P / 16 < 64 ? 64 : (P / 16 > 1024 ? 1024 : P / 16), (size_t)(P + P / 16) * 8};
}
// n > XS_LDS_MAX: rocPRIM's segmented radix sort in global memory.  The caller appends one span of `bytes` unsigned char to its workspace
// (0 when !wide) and hands that tail's start to xs_day_sort_wide, which carves it: sorted keys (f64), segment offsets (u32), rocPRIM temp.
struct XsDaySort { bool wide; size_t tmp_bytes, bytes; };
// the width limits (PQ_ERR_ARG, the message prefixed with `who`) and rocPRIM's size query
pq_status xs_day_sort_plan(pq_ctx *ctx, const Dims &d, const char *who, XsDaySort *plan);
// sorts every day-major row of key[len][n] on ctx->stream; *sorted = the sorted rows (inside the tail)
pq_status xs_day_sort_wide(pq_ctx *ctx, const Dims &d, const XsDaySort &plan, unsigned char *tail, const double *key, const double **sorted);

namespace {
// the host side of the sort-then-look-up pair: one workgroup per day in LDS, or one rocPRIM sort and one look-up launch per step.
// `tail` is the wide tail of the caller's workspace, nv the n per day of xs_prep_kernel.
template <class Op>
pq_status xs_sort_lookup(pq_ctx *ctx, const Dims &d, const XsDaySort &plan, unsigned char *tail, const Op &op, const int32_t *nv) {
    const dim3 grid((unsigned)d.len);
    if (!plan.wide) {
        const XsLds L = xs_lds_shape(d.n);
        PQ_HIP_TRY(hipFuncSetAttribute((const void *)xs_sort_lds_kernel<Op>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
        hipLaunchKernelGGL(xs_sort_lds_kernel<Op>, grid, dim3(L.nthr), L.bytes, ctx->stream, op, nv, d.n, L.P);
        return PQ_OK;
    }
    for (int step = 0; step < op.steps(); step++) {
        const double *srt;
        PQ_TRY(xs_day_sort_wide(ctx, d, plan, tail, op.row(step), &srt));
        hipLaunchKernelGGL(xs_sort_wide_kernel<Op>, grid, dim3(256), 0, ctx->stream, op, step, srt, nv, d.n);
    }
    return PQ_OK;
}
} // namespace

// ---------------------------------------------------------------- host side of the cells stage (sorts.hip)
// workspace of a sort into cells: nkey key rows (f64, day-major, key_pitch doubles apart) | n per day (i32) | labels day-major (u8) |
// labels symbol-major (u8, only when the caller passes none) | block partials: sums (f64), counts, new members (i32) | the wide tail
// of xs_day_sort_plan
struct XsCellsWs { double *key; size_t key_pitch; int32_t *nv; uint8_t *ldm, *lsm; double *ps; int32_t *pc, *pn; unsigned char *tail; };
XsCellsWs xs_cells_layout(XsWs &w, const Dims &d, int nkey, int ncell, bool caller_labels, const XsDaySort &plan);
// day-major labels at ws.ldm (cells 0 .. ncell-1, PQ_LABEL_MID, PQ_LABEL_OUT) -> labels symbol-major (into `labels`, or the
// workspace) -> mean / count / turnover [ncell][len] of `ret`, on ctx->stream
pq_status xs_cells_stats(pq_ctx *ctx, const Dims &d, const XsCellsWs &ws, int ncell, uint8_t *labels, const double *ret, double *mean,
                         int32_t *count, double *tov);
// summary rows: the ncell cells (mean, turnover), then e0.n and e1.n rows of further [.][len] series without turnover
struct XsRows { const double *x; int n; };
pq_status xs_cells_summary(pq_ctx *ctx, int64_t len, int ncell, const double *mean, const double *tov, XsRows e0, XsRows e1, double *summary);
