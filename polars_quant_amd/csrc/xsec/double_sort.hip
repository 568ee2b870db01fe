// xsec/double_sort.hip -- two-way (double) portfolio sorts: a control A and a factor B sorted into a Qa x Qb grid of cells per day,
// independently or B inside each control bucket, with the cells' mean return / count / turnover, the spread along each axis and its
// average over the other (Factor.double_sort; beyond the README => decision D-31).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.  The stages are those of sorts.hip (D-15):
//  1. prep:      one tiled transpose writes two day-major key rows, A and B, with +inf outside the day's three-way sample (A, B and the
//                return all valid), and counts the sample's n.
//  2. label:     the day-sort stage of xsec_dev.h, two or three times.  Up to XS_LDS_MAX symbols one workgroup per day sorts one row at a
//                time in LDS (a row of 16 384 keys fills 136 KiB); wider cross-sections go through daysort.hip.  Sort 1 (A) leaves the
//                control label la in the day-major label row; sort 2 (B) gives m_B: the independent mode labels from it at once, the
//                dependent mode overwrites the B key with the composite key la * 2^18 + m_B (m_B < 2 n <= 200 000 < 2^18: exact in f64,
//                ordered by bucket first, ties of B kept as ties); sort 3 (composite) gives each bucket's key range [lo, hi) by two
//                binary searches and the tie run inside it, so m_{B|a} = a + b - 2 lo and n_a = hi - lo.  A thread only ever reads back
//                the label and the key cells it wrote itself.
//  3. transpose: labels day-major -> symbol-major, 64 x 64 byte tiles.
//  4. aggregate: one thread per (day, block of 256 symbols) as in D-15, but up to 100 cells do not fit registers: the sums and the two
//                integer counts of a tile of DS_CT cells live in LDS, one column per lane (robust.hip's group tiles), and blockIdx.z
//                walks the tiles.  One thread per (day, cell) then adds the block sums in ascending block order, one thread per day
//                writes the two spread tables.
//  5. summary:   D-15's rule per row (xs_seq), one 64-lane workgroup per row: the cells with their turnover, then the spread rows.
#include "xsec_dev.h"

namespace {

constexpr double DS_KEY_A = 262144.0; // composite key la * 2^18 + m_B
constexpr int DS_CT = 32;             // cells per aggregate tile: 32 x 64 lanes x (8 + 4 + 4) bytes = 32 KiB of LDS

struct DsRule {
    int32_t qa, qb;
    int32_t dep;     // 0: independent, 1: B sorted inside each control bucket
    int32_t min_n;   // a day with a smaller sample is labelled PQ_LABEL_OUT everywhere
};

// the keys of the prep kernel: A and B as they are where (A, B, return) are all valid
struct DsKeys {
    const double *a, *b, *r;
    __device__ void operator()(int64_t o, double &ka, double &kb) const {
        const double x = a[o], y = b[o], z = r[o];
        const bool ok = xs_valid(x) & xs_valid(y) & xs_valid(z); // &, not &&: the loads are issued before the tests
        ka = ok ? x : xs_inf();
        kb = ok ? y : xs_inf();
    }
};

// xs_prep_kernel with two key rows per day (the sample, and so n, is the same for both)
__global__ __launch_bounds__(256) void ds_prep_kernel(DsKeys key, Dims d, double *outA, double *outB, int32_t *n_valid) {
    __shared__ double tA[32][33], tB[32][33];
    __shared__ int cnt[32];
    const int64_t t0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5; // 32 x 8
    if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
    for (int i = ly; i < 32; i += 8) { // rows = symbols, lanes along days (coalesced reads)
        const int64_t s = s0 + i, t = t0 + lx;
        double ka = xs_inf(), kb = xs_inf();
        if (s < d.n && t < d.len) key(s * d.stride + t, ka, kb);
        tA[i][lx] = ka; tB[i][lx] = kb;
    }
    __syncthreads();
    for (int i = ly; i < 32; i += 8) { // rows = days, lanes along symbols (coalesced writes)
        const int64_t t = t0 + i, s = s0 + lx;
        const double ka = tA[lx][i], kb = tB[lx][i];
        if (t < d.len && s < d.n) {
            outA[t * d.n + s] = ka; outB[t * d.n + s] = kb;
            if (ka != xs_inf()) atomicAdd(&cnt[i], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && t0 + threadIdx.x < d.len && cnt[threadIdx.x]) atomicAdd(&n_valid[t0 + threadIdx.x], cnt[threadIdx.x]);
}

// first index of the ascending row S[0 .. nv) whose key is >= key
template <bool PAD> __device__ __forceinline__ int ds_lower(XsRow<PAD> S, int nv, double key) {
    int lo = 0, hi = nv;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (S(mid) < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// step 1, on the sorted A row: the control label
template <bool PAD> __device__ __forceinline__ uint8_t ds_control_label(XsRow<PAD> S, int nv, double k, const DsRule &rule) {
    return k == xs_inf() ? (uint8_t)PQ_LABEL_OUT : (uint8_t)((xs_tie_run(S, nv, k) * rule.qa) / (2 * (int64_t)nv));
}

// step 2, on the sorted B row: the cell label (independent) or la and the composite key (dependent); outside the sample the key stays +inf
template <bool PAD>
__device__ __forceinline__ void ds_factor_step(XsRow<PAD> S, int nv, double k, int la, const DsRule &rule, uint8_t &lab, double &ck) {
    lab = (uint8_t)la; ck = k;
    if (k == xs_inf()) return; // la is PQ_LABEL_OUT there
    const int64_t m = xs_tie_run(S, nv, k);
    if (rule.dep) ck = (double)la * DS_KEY_A + (double)m;
    else lab = (uint8_t)(la * rule.qb + (int)((m * rule.qb) / (2 * (int64_t)nv)));
}

// step 3, on the sorted composite row: bucket la is the key range [lo, hi); the tie run of ck lies inside it
template <bool PAD> __device__ __forceinline__ uint8_t ds_cell_label(XsRow<PAD> S, int nv, double ck, int la, const DsRule &rule) {
    if (ck == xs_inf()) return (uint8_t)PQ_LABEL_OUT;
    const int lo = ds_lower(S, nv, (double)la * DS_KEY_A), hi = ds_lower(S, nv, (double)(la + 1) * DS_KEY_A);
    const int64_t na = hi - lo;
    if (na < rule.qb) return (uint8_t)PQ_LABEL_MID;
    const int64_t m = xs_tie_run(S, nv, ck) - 2 * (int64_t)lo;
    return (uint8_t)(la * rule.qb + (int)((m * rule.qb) / (2 * na)));
}

// one workgroup per day, n <= XS_LDS_MAX: the two or three sorts in one LDS row, labels day-major.  keyB is overwritten with the
// composite keys in the dependent mode.
__global__ __launch_bounds__(1024) void ds_label_lds_kernel(const double *keyA, double *keyB, const int32_t *n_valid, int64_t n, int P,
                                                            DsRule rule, uint8_t *lab) {
    extern __shared__ __align__(16) unsigned char ds_lds[];
    double *S = (double *)ds_lds;
    const int64_t t = blockIdx.x;
    const double *rowA = keyA + t * n;
    double *rowB = keyB + t * n;
    uint8_t *out = lab + t * n;
    const int tid = threadIdx.x, nthr = blockDim.x, nv = n_valid[t];
    if (nv < rule.min_n) { // uniform across the workgroup
        for (int s = tid; s < n; s += nthr) out[s] = PQ_LABEL_OUT;
        return;
    }
    xs_load_sort_row(S, rowA, n, P, tid, nthr);
    for (int s = tid; s < n; s += nthr) out[s] = ds_control_label(XsRow<true>{S}, nv, rowA[s], rule);
    __syncthreads(); // every search of the A row is done before the row is loaded again
    xs_load_sort_row(S, rowB, n, P, tid, nthr);
    for (int s = tid; s < n; s += nthr) {
        uint8_t l;
        double ck;
        ds_factor_step(XsRow<true>{S}, nv, rowB[s], out[s], rule, l, ck);
        out[s] = l;
        if (rule.dep) rowB[s] = ck;
    }
    if (!rule.dep) return;
    __syncthreads();
    xs_load_sort_row(S, rowB, n, P, tid, nthr); // thread tid loads the cells tid, tid + nthr, ...: the ones it wrote above
    for (int s = tid; s < n; s += nthr) out[s] = ds_cell_label(XsRow<true>{S}, nv, rowB[s], out[s], rule);
}

// n > XS_LDS_MAX: the rows were sorted by rocPRIM; one kernel per step, each on the sorted rows of its step
template <int STEP>
__global__ __launch_bounds__(256) void ds_label_sorted_kernel(double *key, const double *sorted, const int32_t *n_valid, int64_t n,
                                                              DsRule rule, uint8_t *lab) {
    const int64_t t = blockIdx.x;
    double *row = key + t * n;
    const XsRow<false> S{sorted + t * n};
    uint8_t *out = lab + t * n;
    const int nv = n_valid[t];
    if (nv < rule.min_n) { // uniform across the workgroup; the later steps leave the day as step 1 labelled it
        if (STEP == 1)
            for (int64_t s = threadIdx.x; s < n; s += 256) out[s] = PQ_LABEL_OUT;
        return;
    }
    for (int64_t s = threadIdx.x; s < n; s += 256) {
        if (STEP == 1) out[s] = ds_control_label(S, nv, row[s], rule);
        else if (STEP == 2) {
            uint8_t l;
            double ck;
            ds_factor_step(S, nv, row[s], out[s], rule, l, ck);
            out[s] = l;
            if (rule.dep) row[s] = ck;
        } else out[s] = ds_cell_label(S, nv, row[s], out[s], rule);
    }
}

// day-major [len][n] labels -> symbol-major [n][ostride]
__global__ __launch_bounds__(256) void ds_label_transpose_kernel(const uint8_t *dm, int64_t n, int64_t len, uint8_t *sm, int64_t ostride) {
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

// one thread per (day, block of 256 symbols), blockIdx.z = the tile of DS_CT cells: per cell the sum of the members' returns (ascending
// symbols, from 0.0), the member count and the count of members that were not in the cell the day before; one LDS column per lane
__global__ __launch_bounds__(64) void ds_cell_partial_kernel(const uint8_t *lab, int64_t lstride, const double *ret, Dims d, int C,
                                                             double *psum, int32_t *pcnt, int32_t *pnew) {
    __shared__ double sum[DS_CT][64];
    __shared__ int cnt[DS_CT][64], nw[DS_CT][64];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    if (t >= d.len) return; // no workgroup barrier below: every lane only touches its own column
    const int c0 = (int)blockIdx.z * DS_CT, nc = C - c0 < DS_CT ? C - c0 : DS_CT;
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    for (int j = 0; j < DS_CT; j++) { sum[j][lane] = 0.0; cnt[j][lane] = 0; nw[j][lane] = 0; }
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
            const int j = l[k] - c0;
            if (j < 0 || j >= nc) continue; // another tile's cell, PQ_LABEL_MID or PQ_LABEL_OUT
            sum[j][lane] += v[k]; cnt[j][lane] += 1; nw[j][lane] += lp[k] != l[k];
        }
    }
    for (int j = 0; j < nc; j++) {
        const int64_t o = ((int64_t)blockIdx.y * C + c0 + j) * d.len + t;
        psum[o] = sum[j][lane]; pcnt[o] = cnt[j][lane]; pnew[o] = nw[j][lane];
    }
}

// one thread per (day, cell): block sums in ascending block order (from 0.0); mean, count, turnover
__global__ __launch_bounds__(64) void ds_cell_combine_kernel(const double *psum, const int32_t *pcnt, const int32_t *pnew, int64_t nblk,
                                                             int64_t len, int C, double *mean, int32_t *count, double *tov) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    if (t >= len) return;
    double s = 0.0;
    int64_t c = 0, nw = 0, cp = 0;
    for (int64_t k = 0; k < nblk; k++) {
        const int64_t o = (k * C + g) * len + t;
        s += psum[o]; c += pcnt[o]; nw += pnew[o];
        if (t > 0) cp += pcnt[o - 1];
    }
    mean[g * len + t] = c > 0 ? s / (double)c : pq_null();
    count[g * len + t] = (int32_t)c;
    tov[g * len + t] = (t > 0 && c > 0 && cp > 0) ? (double)nw / (double)c : pq_null();
}

// one thread per day: spread_factor[a] = mean[a][Qb - 1] - mean[a][0] and its average over a (ascending a, from 0.0, over Qa; NULL where
// any row is), spread_control[b] = mean[Qa - 1][b] - mean[0][b] and its average over b
__global__ __launch_bounds__(64) void ds_spread_kernel(const double *mean, int64_t len, int qa, int qb, double *sf, double *sc) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    double acc = 0.0;
    bool full = true;
    for (int a = 0; a < qa; a++) {
        const double lo = mean[(int64_t)(a * qb) * len + t], hi = mean[(int64_t)(a * qb + qb - 1) * len + t];
        const bool ok = !pq_isnull(lo) && !pq_isnull(hi);
        const double v = ok ? hi - lo : pq_null();
        sf[a * len + t] = v;
        if (ok) acc += v;
        full = full && ok;
    }
    sf[qa * len + t] = full ? acc / (double)qa : pq_null();
    acc = 0.0; full = true;
    for (int b = 0; b < qb; b++) {
        const double lo = mean[(int64_t)b * len + t], hi = mean[(int64_t)((qa - 1) * qb + b) * len + t];
        const bool ok = !pq_isnull(lo) && !pq_isnull(hi);
        const double v = ok ? hi - lo : pq_null();
        sc[b * len + t] = v;
        if (ok) acc += v;
        full = full && ok;
    }
    sc[qb * len + t] = full ? acc / (double)qb : pq_null();
}

// one 64-lane workgroup per row: rows 0 .. C-1 = the cells (mean_return, turnover), then the Qa + 1 rows of spread_factor, then the
// Qb + 1 rows of spread_control; D-15's columns
__global__ __launch_bounds__(64) void ds_summary_kernel(const double *mean, const double *tov, const double *sf, const double *sc,
                                                        int64_t len, int C, int nsf, double *summary) {
    __shared__ double buf[XS_CHUNK];
    const int g = blockIdx.x;
    const bool cell = g < C;
    const double *x = cell ? mean + g * len : (g < C + nsf ? sf + (int64_t)(g - C) * len : sc + (int64_t)(g - C - nsf) * len);
    double s, ss, ts = 0.0;
    int64_t n, nt = 0, pos;
    xs_seq<false>(x, len, 0.0, buf, s, n, pos);
    const double m = n > 0 ? s / (double)n : pq_null();
    xs_seq<true>(x, len, n > 0 ? m : 0.0, buf, ss, n, pos);
    if (cell) xs_seq<false>(tov + g * len, len, 0.0, buf, ts, nt, pos); // uniform across the workgroup
    if (threadIdx.x == 0) {
        const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : pq_null();
        double *o = summary + (int64_t)g * PQ_GROUP_SUMMARY_COLS;
        o[0] = (double)n;
        o[1] = m;
        o[2] = sd;
        o[3] = (n >= 2 && sd > 0.0) ? m / sd * sqrt(252.0) : pq_null();
        o[4] = (cell && nt > 0) ? ts / (double)nt : pq_null();
    }
}

pq_status ds_run(pq_ctx *ctx, const pq_batch *b, const double *control, const double *factor, const double *fwd_return,
                 const DsRule &rule, uint8_t *labels, double *mean, int32_t *count, double *tov, double *sf, double *sc, double *summary) {
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int C = rule.qa * rule.qb;
    const size_t cells = (size_t)d.len * (size_t)d.n, len = (size_t)d.len;
    const int64_t nblk = xs_nblk(d.n);
    XsDaySort plan;
    PQ_TRY(xs_day_sort_plan(ctx, d, "factor double sort", &plan));
    // workspace: A keys | B keys, then composite keys (f64, day-major) | n per day (i32) | labels day-major (u8) | labels symbol-major
    // (u8, when the caller passes none) | block partials: sums (f64), counts, new members (i32) | wide: sorted keys, offsets, rocPRIM temp
    const size_t part = (size_t)nblk * (size_t)C * len;
    const size_t o_kb = xs_al(cells * 8), o_cnt = o_kb + xs_al(cells * 8), o_ldm = o_cnt + xs_al(len * 4), o_lsm = o_ldm + xs_al(cells),
                 o_ps = o_lsm + (labels ? 0 : xs_al(cells)), o_pc = o_ps + xs_al(part * 8), o_pn = o_pc + xs_al(part * 4),
                 o_srt = o_pn + xs_al(part * 4);
    PQ_TRY(pq_ws_reserve(ctx, o_srt + plan.bytes));
    unsigned char *w = (unsigned char *)ctx->ws;
    double *keyA = (double *)w, *keyB = (double *)(w + o_kb);
    int32_t *nv = (int32_t *)(w + o_cnt);
    uint8_t *ldm = w + o_ldm;
    uint8_t *lsm = labels ? labels : w + o_lsm;
    const int64_t lstride = labels ? d.stride : d.len;
    double *psum = (double *)(w + o_ps);
    int32_t *pcnt = (int32_t *)(w + o_pc), *pnew = (int32_t *)(w + o_pn);
    if (d.n > 0) {
        PQ_HIP_TRY(hipMemsetAsync(nv, 0, len * 4, ctx->stream));
        hipLaunchKernelGGL(ds_prep_kernel, dim3((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32)), dim3(256), 0, ctx->stream,
                           DsKeys{control, factor, fwd_return}, d, keyA, keyB, nv);
        if (!plan.wide) {
            const XsLds L = xs_lds_shape(d.n);
            PQ_HIP_TRY(hipFuncSetAttribute((const void *)ds_label_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
            hipLaunchKernelGGL(ds_label_lds_kernel, dim3((unsigned)d.len), dim3(L.nthr), L.bytes, ctx->stream, (const double *)keyA, keyB,
                               (const int32_t *)nv, d.n, L.P, rule, ldm);
        } else {
            const double *srt;
            const dim3 g((unsigned)d.len);
            PQ_TRY(xs_day_sort_wide(ctx, d, plan, w + o_srt, keyA, &srt));
            hipLaunchKernelGGL(ds_label_sorted_kernel<1>, g, dim3(256), 0, ctx->stream, keyA, srt, (const int32_t *)nv, d.n, rule, ldm);
            PQ_TRY(xs_day_sort_wide(ctx, d, plan, w + o_srt, keyB, &srt));
            hipLaunchKernelGGL(ds_label_sorted_kernel<2>, g, dim3(256), 0, ctx->stream, keyB, srt, (const int32_t *)nv, d.n, rule, ldm);
            if (rule.dep) {
                PQ_TRY(xs_day_sort_wide(ctx, d, plan, w + o_srt, keyB, &srt));
                hipLaunchKernelGGL(ds_label_sorted_kernel<3>, g, dim3(256), 0, ctx->stream, keyB, srt, (const int32_t *)nv, d.n, rule,
                                   ldm);
            }
        }
        hipLaunchKernelGGL(ds_label_transpose_kernel, dim3((unsigned)((d.len + 63) / 64), (unsigned)((d.n + 63) / 64)), dim3(256), 0,
                           ctx->stream, (const uint8_t *)ldm, d.n, d.len, lsm, lstride);
    }
    const unsigned gx = (unsigned)((d.len + 63) / 64);
    hipLaunchKernelGGL(ds_cell_partial_kernel, dim3(gx, (unsigned)nblk, (unsigned)((C + DS_CT - 1) / DS_CT)), dim3(64), 0, ctx->stream,
                       (const uint8_t *)lsm, lstride, fwd_return, d, C, psum, pcnt, pnew);
    hipLaunchKernelGGL(ds_cell_combine_kernel, dim3(gx, (unsigned)C), dim3(64), 0, ctx->stream, (const double *)psum,
                       (const int32_t *)pcnt, (const int32_t *)pnew, nblk, d.len, C, mean, count, tov);
    hipLaunchKernelGGL(ds_spread_kernel, dim3(gx), dim3(64), 0, ctx->stream, (const double *)mean, d.len, rule.qa, rule.qb, sf, sc);
    hipLaunchKernelGGL(ds_summary_kernel, dim3((unsigned)(C + rule.qa + rule.qb + 2)), dim3(64), 0, ctx->stream, (const double *)mean,
                       (const double *)tov, (const double *)sf, (const double *)sc, d.len, C, rule.qa + 1, summary);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // namespace

extern "C" {

pq_status pq_factor_double_sort(pq_ctx *ctx, const pq_batch *b, const double *control, const double *factor, const double *fwd_return,
                                int32_t n_control, int32_t n_quantiles, int32_t mode, uint8_t *labels, double *mean_return,
                                int32_t *count, double *turnover, double *spread_factor, double *spread_control, double *summary) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(n_control >= 2 && n_control <= 10, "pq_factor_double_sort: n_control must be in [2, 10]");
    PQ_REQUIRE(n_quantiles >= 2 && n_quantiles <= 10, "pq_factor_double_sort: n_quantiles must be in [2, 10]");
    PQ_REQUIRE(mode == 0 || mode == 1, "pq_factor_double_sort: mode must be 0 (independent) or 1 (dependent)");
    PQ_REQUIRE((b->n_series == 0 || (control && factor && fwd_return)) && mean_return && count && turnover && spread_factor &&
                   spread_control && summary,
               "pq_factor_double_sort: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_double_sort cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_double_sort (a cross-section needs every symbol on every day)");
    const DsRule rule{n_control, n_quantiles, mode, mode ? n_control : (n_control > n_quantiles ? n_control : n_quantiles)};
    return ds_run(ctx, b, control, factor, fwd_return, rule, labels, mean_return, count, turnover, spread_factor, spread_control,
                  summary);
}

} // extern "C"
