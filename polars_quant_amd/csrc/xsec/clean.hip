// xsec/clean.hip -- per-day cross-sectional factor cleaning: winsorize, size neutralization, industry neutralization, standardize
// (README.md:244-345 `clean`; README-only => decision D-16).
//
// Columns are symbol-major [n_series][stride]; a day's cross-section is a strided column.  Every step is a per-day statistic of the
// step before it, so the work is a chain of passes over the inputs; no intermediate [N, T] column is written.
//  1. bounds:   mad / percentile: D-15's day-sort stage (xsec_dev.h, daysort.hip) with the key "the factor where the symbol is in the
//               cross-section, -0 read as +0"; one thread reads the clip bounds off the sorted row.  MAD needs no second sort: the deviations
//               |S[i] - med| are two ascending runs (leftwards from the median and rightwards from it), and the k-th smallest of two
//               sorted runs is a binary search.  sigma: two blocked passes (mean, then squared deviations).
//  2. passes:   one thread per (day, block of 256 symbols), consecutive threads on consecutive days (coalesced); each recomputes the
//               value chain up to the step it sums (clip, residual, industry mean, standardize) from the inputs and the per-day
//               parameters of the earlier steps, and writes its block sums.  Industry sums keep G accumulators per thread in LDS.
//  3. combine:  one thread per day (per (day, industry) for the industry sums) adds the block sums in ascending block order from 0.0 and
//               writes the next per-day parameters.
//  4. write:    the pass body once more, writing the cleaned value (NULL outside the cross-section and on dead days) symbol-major.
#include "xsec_dev.h"

namespace {

enum ClWinsor { CL_WIN_NONE = 0, CL_WIN_MAD = 1, CL_WIN_SIGMA = 2, CL_WIN_PCT = 3 };

// pass kinds: what a (day, block) thread sums
enum ClPass {
    CL_COUNT,  // members only
    CL_SUM0,   // sigma: sum of the raw values
    CL_VAR0,   // sigma: sum of (x - mean)^2
    CL_CAP1,   // sum of the clipped values, sum of z
    CL_CAP2,   // sum of (x - xbar)(z - zbar), sum of (z - zbar)^2
    CL_IND,    // per industry: sum of the residuals, member count
    CL_STD1,   // sum of the industry-neutral residuals
    CL_STD2,   // sum of their squared deviations from the mean
    CL_WRITE,  // the cleaned value -> out
};

struct ClIn {
    const double *f, *z;    // z: null = size neutralization off
    XsGroups ind;           // the industry codes, on the batch's stride; null codes = industry neutralization off
    int32_t standardize;
    Dims d;
};

// per-day parameters, [len] each (gmean: [G][len])
struct ClDay {
    int32_t *n;
    double *lo, *hi;          // clip bounds (-inf / +inf: not clipped)
    double *m0;               // sigma: mean of the raw values
    double *xbar, *zbar, *beta;
    double *gmean;
    double *smean, *sstd;
};

__device__ __forceinline__ bool cl_member(const ClIn &in, double x, double z, int32_t g) {
    return xs_valid(x) && (!in.z || xs_valid(z)) && (!in.ind.codes || (g >= 0 && g < in.ind.G));   // written out: see XsGroups::has
}

// clip by comparisons: a value equal to a bound keeps its own bits (so -0 / +0 never depend on which bound is hit)
__device__ __forceinline__ double cl_clip(double x, double lo, double hi) {
    const double y = x < lo ? lo : x;
    return y > hi ? hi : y;
}

// the key of xs_prep_kernel: the factor where the symbol is in the cross-section, +0 for -0
struct ClKey {
    ClIn in;
    __device__ void operator()(int64_t o, double (&k)[1]) const {
        const double x = in.f[o];
        if (cl_member(in, x, in.z ? in.z[o] : 0.0, in.ind.codes ? in.ind.at_cell(o) : 0)) k[0] = x == 0.0 ? 0.0 : x;
    }
};

struct ClWin {
    int32_t mode;
    double c;          // mad: winsorize_n * 1.4826
    double qlo, qhi;   // percentile: p, 1 - p
};

// numpy's "linear" quantile, written in the D-16 order: h = q (n - 1), i = floor(h), g = h - i, S[i] + g (S[i+1] - S[i]) unless g == 0
template <bool PAD> __device__ double cl_quantile(XsRow<PAD> S, int nv, double q) {
    const double h = q * (double)(nv - 1);
    const int i = (int)floor(h);
    const double g = h - (double)i;
    return g == 0.0 ? S(i) : S(i) + g * (S(i + 1) - S(i));
}

// k-th smallest (from 0) of |S[i] - med| over S[0 .. nv): the run A (a = m entries, A[j] = |S[m-1-j] - med|) and the run B (B[j] =
// |S[m+j] - med|) are both ascending (m = the first index with S[i] >= med).  Find the smallest i with A[i] >= B[k-i]: then the k + 1
// smallest are A[0 .. i) and B[0 .. k+1-i), and the k-th is the larger of their last entries.
template <bool PAD> __device__ double cl_dev_kth(XsRow<PAD> S, int nv, int m, double med, int k) {
    const int a = m, b = nv - m;
    auto A = [&](int j) { return fabs(S(m - 1 - j) - med); };
    auto B = [&](int j) { return fabs(S(m + j) - med); };
    int lo = k + 1 - b > 0 ? k + 1 - b : 0, hi = k + 1 < a ? k + 1 : a;
    while (lo < hi) {
        const int i = (lo + hi) >> 1;
        if (A(i) < B(k - i)) lo = i + 1; else hi = i;
    }
    const int i = lo, j = k + 1 - lo;
    const double x = i > 0 ? A(i - 1) : 0.0, y = j > 0 ? B(j - 1) : 0.0;
    return x < y ? y : x;
}

template <bool PAD> __device__ double cl_median(XsRow<PAD> S, int nv) {
    return (nv & 1) ? S((nv - 1) / 2) : (S(nv / 2 - 1) + S(nv / 2)) * 0.5;
}

// clip bounds of one day from its ascending members S[0 .. nv)
template <bool PAD> __device__ void cl_bounds(XsRow<PAD> S, int nv, const ClWin &w, double &lo, double &hi) {
    lo = -xs_inf(); hi = xs_inf();
    if (nv < 2) return;
    if (w.mode == CL_WIN_PCT) {
        lo = cl_quantile(S, nv, w.qlo);
        hi = cl_quantile(S, nv, w.qhi);
        return;
    }
    const double med = cl_median(S, nv);
    int m = 0, r = nv;
    while (m < r) { const int mid = (m + r) >> 1; if (S(mid) < med) m = mid + 1; else r = mid; }
    const double mad = (nv & 1) ? cl_dev_kth(S, nv, m, med, (nv - 1) / 2)
                                : (cl_dev_kth(S, nv, m, med, nv / 2 - 1) + cl_dev_kth(S, nv, m, med, nv / 2)) * 0.5;
    if (mad != 0.0) { // MAD == 0: not clipped
        lo = med - w.c * mad;
        hi = med + w.c * mad;
    }
}

// one workgroup per day, n <= XS_LDS_MAX: sort the day's keys in LDS, one thread writes the bounds
__global__ __launch_bounds__(1024) void cl_bounds_lds_kernel(const double *key, int64_t n, int P, ClWin w, ClDay day) {
    extern __shared__ __align__(16) unsigned char cl_lds[];
    double *S = (double *)cl_lds;
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, nthr = blockDim.x, nv = day.n[t];
    if (nv >= 2) { // uniform across the workgroup
        const double *row = key + t * n;
        xs_load_sort_row(S, row, n, P, tid, nthr);
    }
    if (tid == 0) cl_bounds(XsRow<true>{S}, nv, w, day.lo[t], day.hi[t]);
}

// n > XS_LDS_MAX: the day-major rows were sorted by rocPRIM; one thread per day
__global__ __launch_bounds__(64) void cl_bounds_sorted_kernel(const double *sorted, int64_t n, int64_t len, ClWin w, ClDay day) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t < len) cl_bounds(XsRow<false>{sorted + t * n}, day.n[t], w, day.lo[t], day.hi[t]);
}

// one thread per (day, block of 256 symbols).  The value chain of one member, up to the step pass P sums:
// v1 = clip(x), v2 = (v1 - xbar) - beta (z - zbar) (size on), v3 = v2 - gmean[g] (industry on), v4 = (v3 - smean) / sstd (standardize)
// Block sums: members only, ascending symbols, from 0.0 (D-12).  CL_IND keeps G sums and uint16 counts per lane in LDS ([g][lane]:
// consecutive lanes on consecutive 8-byte words, so no bank conflict whatever the codes).
template <int P>
__global__ __launch_bounds__(64) void cl_pass_kernel(ClIn in, ClDay day, double *ps0, double *ps1, int32_t *pcnt, uint16_t *pgcnt,
                                                     double *out) {
    extern __shared__ __align__(16) unsigned char cl_lds[];
    const Dims d = in.d;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= d.len) return;
    const int lane = threadIdx.x, G = in.ind.G;
    double *gs = (double *)cl_lds;
    uint16_t *gc = (uint16_t *)(cl_lds + (size_t)G * 64 * 8);
    if (P == CL_IND)
        for (int g = 0; g < G; g++) { gs[g * 64 + lane] = 0.0; gc[g * 64 + lane] = 0; }
    const int nv = day.n[t];
    const double lo = day.lo[t], hi = day.hi[t];
    const double m0 = P == CL_VAR0 ? day.m0[t] : 0.0;
    const bool cap = in.z != nullptr, ind = in.ind.codes != nullptr, stdz = in.standardize != 0;
    const double xbar = cap && P >= CL_CAP2 ? day.xbar[t] : 0.0, zbar = cap && P >= CL_CAP2 ? day.zbar[t] : 0.0,
                 beta = cap && P >= CL_IND ? day.beta[t] : 0.0;
    const double smean = P >= CL_STD2 ? day.smean[t] : 0.0, sstd = P == CL_WRITE && stdz ? day.sstd[t] : 1.0;
    const bool dead = P == CL_WRITE && (nv < 2 || (stdz && sstd == 0.0));
    const int64_t s_lo = (int64_t)blockIdx.y * XS_BLOCK, s_hi = s_lo + XS_BLOCK < d.n ? s_lo + XS_BLOCK : d.n;
    double a0 = 0.0, a1 = 0.0;
    int cnt = 0;
    constexpr int B = 8;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += B) {
        double x[B], z[B];
        int32_t g[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int64_t o = (s0 + k < s_hi ? s0 + k : s_hi - 1) * d.stride + t;
            x[k] = in.f[o];
            z[k] = cap ? in.z[o] : 0.0;
            g[k] = ind ? in.ind.at_cell(o) : 0;
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            if (s0 + k >= s_hi) break;
            const bool mem = cl_member(in, x[k], z[k], g[k]);
            if (P == CL_WRITE) {
                if (!mem || dead) { out[(s0 + k) * d.stride + t] = pq_null(); continue; }
            } else if (!mem) {
                continue;
            }
            cnt += 1;
            if (P == CL_COUNT) continue;
            if (P == CL_SUM0) { a0 += x[k]; continue; }
            if (P == CL_VAR0) { const double e = x[k] - m0; a0 += e * e; continue; }
            double v = cl_clip(x[k], lo, hi);
            if (P == CL_CAP1) { a0 += v; a1 += z[k]; continue; }
            if (P == CL_CAP2) {
                const double dz = z[k] - zbar;
                a0 += (v - xbar) * dz;
                a1 += dz * dz;
                continue;
            }
            if (cap) v = (v - xbar) - beta * (z[k] - zbar);
            if (P == CL_IND) { gs[g[k] * 64 + lane] += v; gc[g[k] * 64 + lane] += 1; continue; }
            if (ind) v = v - day.gmean[(int64_t)g[k] * d.len + t];
            if (P == CL_STD1) { a0 += v; continue; }
            if (P == CL_STD2) { const double e = v - smean; a0 += e * e; continue; }
            if (stdz) v = (v - smean) / sstd;
            out[(s0 + k) * d.stride + t] = v;
        }
    }
    if (P == CL_WRITE) return;
    if (P == CL_IND) {
        for (int g = 0; g < G; g++) {
            const int64_t o = ((int64_t)blockIdx.y * G + g) * d.len + t;
            ps0[o] = gs[g * 64 + lane];
            pgcnt[o] = gc[g * 64 + lane];
        }
        return;
    }
    const int64_t o = (int64_t)blockIdx.y * d.len + t;
    ps0[o] = a0;
    ps1[o] = a1;
    pcnt[o] = cnt;
}

// one thread per day: block sums in ascending block order from 0.0 -> the parameters of step P
template <int P>
__global__ __launch_bounds__(64) void cl_combine_kernel(const double *ps0, const double *ps1, const int32_t *pcnt, int64_t nblk, int64_t len,
                                                        double wn, ClDay day) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= len) return;
    double s0 = 0.0, s1 = 0.0;
    int32_t n = 0;
    for (int64_t k = 0; k < nblk; k++) {
        const int64_t o = k * len + t;
        s0 += ps0[o]; s1 += ps1[o]; n += pcnt[o];
    }
    day.n[t] = n;
    const double dn = (double)n;
    if (P == CL_SUM0) day.m0[t] = s0 / dn;
    if (P == CL_VAR0) {
        const double sd = sqrt(s0 / (dn - 1.0));
        day.lo[t] = day.m0[t] - wn * sd;
        day.hi[t] = day.m0[t] + wn * sd;
    }
    if (P == CL_CAP1) { day.xbar[t] = s0 / dn; day.zbar[t] = s1 / dn; }
    if (P == CL_CAP2) day.beta[t] = s1 == 0.0 ? 0.0 : s0 / s1;
    if (P == CL_STD1) day.smean[t] = s0 / dn;
    if (P == CL_STD2) day.sstd[t] = sqrt(s0 / (dn - 1.0));
}

// one thread per (day, industry): the industry's block sums in ascending block order from 0.0, over its member count
__global__ __launch_bounds__(64) void cl_ind_combine_kernel(const double *ps, const uint16_t *pc, int64_t nblk, int64_t len, int G,
                                                            double *gmean) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (t >= len) return;
    double s = 0.0;
    int64_t c = 0;
    for (int64_t k = 0; k < nblk; k++) {
        const int64_t o = (k * G + g) * len + t;
        s += ps[o]; c += pc[o];
    }
    gmean[(int64_t)g * len + t] = c > 0 ? s / (double)c : pq_null();
}

__global__ __launch_bounds__(256) void cl_fill_kernel(double *p, int64_t m, double v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) p[i] = v;
}

} // namespace

extern "C" {

pq_status pq_factor_clean(pq_ctx *ctx, const pq_batch *b, const double *factor, int32_t winsorize, double winsorize_n, const double *cap_z,
                          const int32_t *industry, int32_t n_industries, int32_t standardize, double *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(winsorize >= CL_WIN_NONE && winsorize <= CL_WIN_PCT, "pq_factor_clean: winsorize must be 0 (none), 1 (mad), 2 (sigma) or 3 (percentile)");
    ClWin w{winsorize, 0.0, 0.0, 0.0};
    if (winsorize == CL_WIN_MAD || winsorize == CL_WIN_SIGMA)
        PQ_REQUIRE(winsorize_n >= 0.0 && winsorize_n < HUGE_VAL, "pq_factor_clean: winsorize_n must be finite and >= 0");
    if (winsorize == CL_WIN_MAD) w.c = winsorize_n * 1.4826;
    if (winsorize == CL_WIN_PCT) {
        const double p = winsorize_n / 100.0;
        PQ_REQUIRE(p >= 0.0 && p < 0.5, "pq_factor_clean: percentile winsorize needs 0 <= winsorize_n / 100 < 0.5");
        w.qlo = p;
        w.qhi = 1.0 - p;
    }
    XsGroups ind;   // no stride parameter: the codes lie on the batch's
    PQ_TRY(xs_groups_arg("pq_factor_clean", b, industry, b->stride, n_industries, XsGroupsPolicy{XS_G_WITH_CODES, "n_industries", "industry"}, &ind));
    PQ_REQUIRE(standardize == 0 || standardize == 1, "pq_factor_clean: standardize must be 0 or 1");
    PQ_REQUIRE((b->n_series == 0 || factor) && (b->n_series == 0 || b->len == 0 || out), "pq_factor_clean: null pointer");
    if (ctx->rec) { pq_set_error("pq_factor_clean cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_factor_clean (a cross-section needs every symbol on every day)");
    if (b->len == 0 || b->n_series == 0) return PQ_OK;
    const Dims d = dims_of(b);
    const int G = ind.G;
    const ClIn in{factor, cap_z, ind, standardize, d};
    const size_t cells = (size_t)d.len * (size_t)d.n, len = (size_t)d.len;
    const int64_t nblk = xs_nblk(d.n);
    const bool sorted = winsorize == CL_WIN_MAD || winsorize == CL_WIN_PCT;
    XsDaySort plan{};
    if (sorted) PQ_TRY(xs_day_sort_plan(ctx, d, "pq_factor_clean (mad / percentile winsorize)", &plan));
    // workspace: per-day n (i32) and 8 parameter rows (f64) | industry means [G][len] | block partials: 2 sums (f64) + count (i32) |
    // industry partials: sums (f64) + counts (u16) [nblk][G][len] | sorted modes: keys day-major (f64) | wide: sorted keys, offsets, rocPRIM temp
    const size_t part = (size_t)nblk * len, gpart = part * (size_t)G;
    ClDay day;
    double *ps0, *ps1, *gs, *key;
    int32_t *pc;
    uint16_t *gc;
    unsigned char *tail;
    PQ_TRY(xs_ws_carve(ctx, "pq_factor_clean", [&](XsWs &w) {
        w.take(day.n, len).take(day.lo, len).take(day.hi, len).take(day.m0, len).take(day.xbar, len).take(day.zbar, len);
        w.take(day.beta, len).take(day.smean, len).take(day.sstd, len).take(day.gmean, (size_t)G * len);
        w.take(ps0, part).take(ps1, part).take(pc, part).take(gs, gpart).take(gc, gpart).take(key, sorted ? cells : 0).take(tail, plan.bytes);
    }));
    const dim3 gp((unsigned)((d.len + 63) / 64), (unsigned)nblk), gd((unsigned)((d.len + 63) / 64)), g256((unsigned)((d.len + 255) / 256));
    const double wn = winsorize == CL_WIN_SIGMA ? winsorize_n : 0.0;
    hipStream_t st = ctx->stream;
#define CL_PASS(P)                                                                                                                      \
    do {                                                                                                                                \
        hipLaunchKernelGGL(cl_pass_kernel<P>, gp, dim3(64), 0, st, in, day, ps0, ps1, pc, (uint16_t *)nullptr, (double *)nullptr);   \
        hipLaunchKernelGGL(cl_combine_kernel<P>, gd, dim3(64), 0, st, (const double *)ps0, (const double *)ps1, (const int32_t *)pc, \
                           nblk, d.len, wn, day);                                                                                      \
    } while (0)
    // 1. clip bounds (+-inf: not clipped) and n
    if (!sorted) {
        hipLaunchKernelGGL(cl_fill_kernel, g256, dim3(256), 0, st, day.lo, d.len, -HUGE_VAL);
        hipLaunchKernelGGL(cl_fill_kernel, g256, dim3(256), 0, st, day.hi, d.len, HUGE_VAL);
    }
    if (winsorize == CL_WIN_SIGMA) {
        CL_PASS(CL_SUM0);
        CL_PASS(CL_VAR0);
    } else if (sorted) {
        PQ_HIP_TRY(hipMemsetAsync(day.n, 0, len * 4, st));
        hipLaunchKernelGGL((xs_prep_kernel<1, ClKey>), dim3((unsigned)((d.len + 31) / 32), (unsigned)((d.n + 31) / 32)), dim3(256), 0, st,
                           ClKey{in}, d, key, (int64_t)0, day.n);
        if (!plan.wide) {
            const XsLds L = xs_lds_shape(d.n);
            PQ_HIP_TRY(hipFuncSetAttribute((const void *)cl_bounds_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
            hipLaunchKernelGGL(cl_bounds_lds_kernel, dim3((unsigned)d.len), dim3(L.nthr), L.bytes, st, (const double *)key, d.n, L.P, w, day);
        } else {
            const double *srt;
            PQ_TRY(xs_day_sort_wide(ctx, d, plan, tail, key, &srt));
            hipLaunchKernelGGL(cl_bounds_sorted_kernel, gd, dim3(64), 0, st, srt, d.n, d.len, w, day);
        }
    }
    // 2. size neutralization
    if (cap_z) {
        CL_PASS(CL_CAP1);
        CL_PASS(CL_CAP2);
    }
    // 3. industry neutralization
    if (industry) {
        const size_t lds = (size_t)G * 64 * (8 + 2);
        PQ_HIP_TRY(hipFuncSetAttribute((const void *)cl_pass_kernel<CL_IND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(cl_pass_kernel<CL_IND>, gp, dim3(64), lds, st, in, day, gs, (double *)nullptr, (int32_t *)nullptr, gc,
                           (double *)nullptr);
        hipLaunchKernelGGL(cl_ind_combine_kernel, dim3(gd.x, (unsigned)G), dim3(64), 0, st, (const double *)gs, (const uint16_t *)gc, nblk,
                           d.len, G, day.gmean);
    }
    // 4. standardize; n for the write pass when no pass so far has counted it (the industry pass does not)
    if (standardize) {
        CL_PASS(CL_STD1);
        CL_PASS(CL_STD2);
    } else if (winsorize == CL_WIN_NONE && !cap_z) {
        CL_PASS(CL_COUNT);
    }
#undef CL_PASS
    hipLaunchKernelGGL(cl_pass_kernel<CL_WRITE>, gp, dim3(64), 0, st, in, day, (double *)nullptr, (double *)nullptr, (int32_t *)nullptr,
                       (uint16_t *)nullptr, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
