// xsec/double_sort.hip -- two-way (double) portfolio sorts: a control A and a factor B sorted into a Qa x Qb grid of cells per day,
// independently or B inside each control bucket, with the cells' mean return / count / turnover, the spread along each axis and its
// average over the other (Factor.double_sort; beyond the README => decision D-31).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.  The stages are those of sorts.hip (D-15):
//  1. prep:      xs_prep_kernel<2, DsKeys>: one tiled transpose writes two day-major key rows, A and B, with +inf outside the day's
//                three-way sample (A, B and the return all valid), and counts the sample's n.
//  2. label:     xsec_dev.h's sort-then-look-up pair with DsLabelOp, two or three steps.  Up to XS_LDS_MAX symbols one workgroup per day
//                sorts one row at a time in LDS (a row of 16 384 keys fills 136 KiB); wider cross-sections go through daysort.hip.  Step 1
//                (A) leaves the control label la in the day-major label row; step 2 (B) gives m_B: the independent mode labels from it at
//                once, the dependent mode overwrites the B key with the composite key la * 2^18 + m_B (m_B < 2 n <= 200 000 < 2^18: exact
//                in f64, ordered by bucket first, ties of B kept as ties); step 3 (composite) gives each bucket's key range [lo, hi) by
//                two binary searches and the tie run inside it, so m_{B|a} = a + b - 2 lo and n_a = hi - lo.  A thread only ever reads
//                back the label and the key cells it wrote itself.
//  3. cells:     the cells stage of sorts.hip (xs_cells_stats) with Qa Qb cells: label transpose, per-cell mean / count / turnover.
//                One thread per day then writes the two spread tables.
//  4. summary:   xs_cells_summary: the cells with their turnover, then the rows of the two spread tables.
#include "xsec_dev.h"

namespace {

constexpr double DS_KEY_A = 262144.0; // composite key la * 2^18 + m_B

struct DsRule {
    int32_t qa, qb;
    int32_t dep;     // 0: independent, 1: B sorted inside each control bucket
    int32_t min_n;   // a day with a smaller sample is labelled PQ_LABEL_OUT everywhere
};

// the keys of xs_prep_kernel: A and B as they are where (A, B, return) are all valid
struct DsKeys {
    const double *a, *b, *r;
    __device__ void operator()(int64_t o, double (&k)[2]) const {
        const double x = a[o], y = b[o], z = r[o];
        if (xs_valid(x) & xs_valid(y) & xs_valid(z)) { k[0] = x; k[1] = y; } // &, not &&: the loads are issued before the tests
    }
};

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

// the operation of xsec_dev.h's sort-then-look-up pair: the steps above, labels day-major.  keyB is overwritten with the composite keys
// in the dependent mode.
struct DsLabelOp {
    static constexpr int MAX_STEPS = 3;
    const double *keyA;
    double *keyB;
    DsRule rule;
    uint8_t *lab;
    __host__ __device__ int steps() const { return rule.dep ? 3 : 2; }
    __host__ __device__ const double *row(int step) const { return step == 0 ? keyA : keyB; }
    __device__ bool unsorted(int nv) const { return nv < rule.min_n; }
    __device__ void fill(int64_t i) const { lab[i] = PQ_LABEL_OUT; }
    template <bool PAD> __device__ void at(int step, XsRow<PAD> S, int nv, int64_t i) const {
        if (step == 0) lab[i] = ds_control_label(S, nv, keyA[i], rule);
        else if (step == 1) {
            uint8_t l;
            double ck;
            ds_factor_step(S, nv, keyB[i], lab[i], rule, l, ck);
            lab[i] = l;
            if (rule.dep) keyB[i] = ck;
        } else lab[i] = ds_cell_label(S, nv, keyB[i], lab[i], rule);
    }
};

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

pq_status ds_run(pq_ctx *ctx, const pq_batch *b, const double *control, const double *factor, const double *fwd_return,
                 const DsRule &rule, uint8_t *labels, double *mean, int32_t *count, double *tov, double *sf, double *sc, double *summary) {
    if (b->len == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int C = rule.qa * rule.qb;
    XsDaySort plan;
    PQ_TRY(xs_day_sort_plan(ctx, d, "factor double sort", &plan));
    XsCellsWs ws; // key rows: A | B, then the composite keys
    PQ_TRY(xs_ws_carve(ctx, "factor double sort", [&](XsWs &w) { ws = xs_cells_layout(w, d, 2, C, labels != nullptr, plan); }));
    double *keyA = ws.key, *keyB = keyA + ws.key_pitch;
    if (d.n > 0) {
        PQ_HIP_TRY(hipMemsetAsync(ws.nv, 0, (size_t)d.len * 4, ctx->stream));
        hipLaunchKernelGGL((xs_prep_kernel<2, DsKeys>), dim3((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32)), dim3(256), 0,
                           ctx->stream, DsKeys{control, factor, fwd_return}, d, keyA, (int64_t)ws.key_pitch, ws.nv);
        PQ_TRY(xs_sort_lookup(ctx, d, plan, ws.tail, DsLabelOp{keyA, keyB, rule, ws.ldm}, ws.nv));
    }
    PQ_TRY(xs_cells_stats(ctx, d, ws, C, labels, fwd_return, mean, count, tov));
    hipLaunchKernelGGL(ds_spread_kernel, dim3((unsigned)((d.len + 63) / 64)), dim3(64), 0, ctx->stream, (const double *)mean, d.len,
                       rule.qa, rule.qb, sf, sc);
    return xs_cells_summary(ctx, d.len, C, mean, tov, XsRows{sf, rule.qa + 1}, XsRows{sc, rule.qb + 1}, summary);
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
