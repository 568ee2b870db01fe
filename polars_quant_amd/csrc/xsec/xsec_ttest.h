// xsec/xsec_ttest.h -- Student-t p-values and the sequential summary row (D-17), shared by regress.hip (Fama-MacBeth, ic_test) and
// robust.hip (D-18: IC decay, sub-period and sub-group tests).  Moved unchanged from regress.hip, whose header notes the method.  Also
// the coefficient statistics of a fit (coef / t / p and R^2 with their NULL rules), shared by regress.hip and linear.hip (D-24).
#pragma once
#include "xsec_dev.h"

namespace {

constexpr int RG_SUMMARY_COLS = 5;      // PQ_REGRESS_SUMMARY_COLS

// ---------------------------------------------------------------- Student-t p-value
struct Dd { double hi, lo; };
__device__ __forceinline__ Dd dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return Dd{s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ Dd dd_quick(double a, double b) {
    const double s = a + b;
    return Dd{s, b - (s - a)};
}
__device__ __forceinline__ Dd dd_add(Dd x, Dd y) {
    const Dd s = dd_two_sum(x.hi, y.hi);
    return dd_quick(s.hi, s.lo + (x.lo + y.lo));
}
__device__ __forceinline__ Dd dd_mul(Dd x, Dd y) {
    const double p = x.hi * y.hi, e = fma(x.hi, y.hi, -p);
    return dd_quick(p, e + (x.hi * y.lo + x.lo * y.hi));
}
__device__ __forceinline__ Dd dd_div(Dd x, Dd y) {
    const double q1 = x.hi / y.hi;
    const Dd p = dd_mul(y, Dd{q1, 0.0});
    const Dd r = dd_add(x, Dd{-p.hi, -p.lo});
    return dd_quick(q1, r.hi / y.hi);
}
__device__ __forceinline__ Dd dd_floor(Dd x) { return fabs(x.hi) < 1e-300 ? Dd{1e-300, 0.0} : x; }

// continued fraction of I_x(a, b) (Numerical Recipes' betacf, modified Lentz), x in double-double; a, b are multiples of 1/2 small
// enough that every numerator and denominator below is exact in f64
__device__ double rg_betacf(Dd x, double a, double b) {
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    const Dd one{1.0, 0.0};
    Dd c = one, d = dd_floor(dd_add(one, dd_div(dd_mul(x, Dd{-qab, 0.0}), Dd{qap, 0.0})));
    d = dd_div(one, d);
    Dd h = d;
    for (int m = 1; m <= 100000; m++) {
        const double m2 = 2.0 * m, dm = (double)m;
        Dd del{1.0, 0.0};
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const double num = half == 0 ? dm * (b - dm) : -(a + dm) * (qab + dm);
            const double den = half == 0 ? (qam + m2) * (a + m2) : (a + m2) * (qap + m2);
            const Dd aa = dd_div(dd_mul(x, Dd{num, 0.0}), Dd{den, 0.0});
            d = dd_floor(dd_add(dd_mul(d, aa), one));
            c = dd_floor(dd_add(dd_div(aa, c), one));
            d = dd_div(one, d);
            del = dd_mul(d, c);
            h = dd_mul(h, del);
        }
        if (fabs((del.hi - 1.0) + del.lo) < 1e-17) break;
    }
    return h.hi;
}

// log(Gamma(a + 1/2) / Gamma(a)), a >= 1/2: shift a up to >= 16, then 1/2 log a - 1/(8a) + 1/(192a^3) - 1/(640a^5) + 17/(14336a^7)
// - 31/(18432a^9) (error < 1e-17 there)
__device__ double rg_lgamma_half_ratio(double a) {
    double prod = 1.0;
    while (a < 16.0) {
        prod *= (a + 0.5) / a;
        a += 1.0;
    }
    const double ia = 1.0 / a, ia2 = ia * ia;
    const double s = ia * (-1.0 / 8 + ia2 * (1.0 / 192 + ia2 * (-1.0 / 640 + ia2 * (17.0 / 14336 + ia2 * (-31.0 / 18432)))));
    return 0.5 * log(a) + s - log(prod);
}

// two-sided Student-t p-value of t on df > 0 degrees of freedom: I_x(df/2, 1/2), x = df / (df + t^2), 1 - x = t^2 / (df + t^2)
// taken directly; 1 at t == 0 (or t^2 below the f64 range), 0 at |t| == inf
__device__ double rg_t_pvalue(double t, double df) {
    if (!isfinite(t)) return t == t ? 0.0 : pq_null();
    const double t2h = t * t;
    if (t2h == 0.0) return 1.0;
    if (!(t2h < HUGE_VAL)) return 0.0;
    const Dd t2{t2h, fma(t, t, -t2h)}, den = dd_add(Dd{df, 0.0}, t2);
    const Dd x = dd_div(Dd{df, 0.0}, den), y = dd_div(t2, den);
    const double a = 0.5 * df;
    const double e = a * -log1p(t2h / df) + 0.5 * log(y.hi) + rg_lgamma_half_ratio(a);   // log(x^a (1-x)^(1/2) / B(a, 1/2)) + log sqrt(pi)
    const double front = exp(e) / 1.7724538509055160273;                                   // / sqrt(pi)
    if (x.hi < (a + 1.0) / (a + 2.5)) return front * rg_betacf(x, a, 0.5) / a;
    return 1.0 - front * rg_betacf(y, 0.5, a) / 0.5;
}

// Coefficient j of a fit (xo_fit's b_j and v_j, read only where the fit solved) with s^2 = SSE / df: coef = b_j, se = sqrt(s^2 v_j),
// t = b_j / se, p on df; t and p are NULL where se == 0, and all three without a solution.  Shared by rg_final_kernel (regress.hip)
// and ln_final_kernel (linear.hip); where the three values go is the caller's.
__device__ __forceinline__ void rg_coef_stats(bool ok, const double *bj, const double *vj, double s2, double df, double *coef, double *tst,
                                              double *pv) {
    if (!ok) { *coef = pq_null(); *tst = pq_null(); *pv = pq_null(); return; }
    const double b = *bj, se = sqrt(s2 * *vj);
    *coef = b;
    const double t = se == 0.0 ? pq_null() : b / se;
    *tst = t;
    *pv = se == 0.0 ? pq_null() : rg_t_pvalue(t, df);
}
// R^2 = 1 - SSE / Syy; NULL without a solution or where the dependent column is constant
__device__ __forceinline__ double rg_r2(bool ok, double sse, double syy) { return ok && syy != 0.0 ? 1.0 - sse / syy : pq_null(); }

// Summary row of one series, one 64-lane workgroup: n_days, mean, std (ddof 1), t = mean / (std / sqrt(n_days)), p on n_days - 1, over
// the non-NaN days of x[0 .. len), ascending sequential sums from 0.0; o[0 .. RG_SUMMARY_COLS) is written by lane 0
__device__ __forceinline__ void rg_summary_row(const double *x, int64_t len, double *buf, double *o) {
    double s, ss;
    int64_t n, pos;
    xs_seq<false>(x, len, 0.0, buf, s, n, pos);
    const double m = n > 0 ? s / (double)n : 0.0;
    xs_seq<true>(x, len, m, buf, ss, n, pos);
    if (threadIdx.x == 0) {
        const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : 0.0;
        const bool ok = n >= 2 && sd != 0.0;
        o[0] = (double)n;
        o[1] = n > 0 ? m : pq_null();
        o[2] = ok ? sd : pq_null();
        const double t = ok ? m / (sd / sqrt((double)n)) : pq_null();
        o[3] = t;
        o[4] = ok ? rg_t_pvalue(t, (double)(n - 1)) : pq_null();
    }
}

// Fama-MacBeth summary, one 64-lane workgroup per coefficient row: the summary row over the non-NaN days of the row (the days with a
// solution)
__global__ __launch_bounds__(64) void rg_summary_kernel(const double *coef, int64_t len, double *summary) {
    __shared__ double buf[XS_CHUNK];
    rg_summary_row(coef + (int64_t)blockIdx.x * len, len, buf, summary + (int64_t)blockIdx.x * RG_SUMMARY_COLS);
}

} // namespace
