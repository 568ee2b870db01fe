// pattern.hip -- the 61 candlestick recognisers of src/talib/pattern.rs as ONE pass over OHLC.
// ROW shape: one (series, row) per thread; each thread builds the 5-candle window ending at its row,
// derives the per-candle predicates (pattern.rs:2067-2143) once, and evaluates every requested
// recogniser from them.  Int32 in {-100, 0, +100}; rows below a recogniser's look-back are 0.
// Reading OHLC once for all 61 outputs is the fused form SURVEY 8(a) prices at 276 B/row instead
// of 61 x 36 B/row.
#include "pq_dev.h"
#include <utility>

struct Cdl { // one candle; k = rows back from the current row
    double o, h, l, c;
    double body, us, ls, mx, mn;
    __device__ void set(double o_, double h_, double l_, double c_) {
        o = o_; h = h_; l = l_; c = c_;
        body = fabs(o - c);                             // :2077
        mn = fmin(o, c);                                // :2081
        mx = fmax(o, c);                                // :2085
        us = h - mx;                                    // :2089
        ls = mn - l;                                    // :2093
    }
    // The predicates are functions of the values above, written where a recogniser uses them: the compiler still computes each one once
    // (at its first use), but as fields set up front all 5 x 12 of them -- a scalar register pair each -- were live from the top of the
    // kernel, far more than the scalar register file holds.
    __device__ __forceinline__ bool bull() const { return c > o; }                       // :2069
    __device__ __forceinline__ bool bear() const { return c < o; }                       // :2073
    __device__ __forceinline__ bool lng() const { return body > 0.05 * (o + c) * 0.5; }  // :2097
    __device__ __forceinline__ bool sht() const { return body < 0.1 * (o + c) * 0.5; }   // :2101
    __device__ __forceinline__ bool doji() const { return body <= 0.005 * (o + c) * 0.5; } // :2105
    __device__ __forceinline__ bool lus() const { return us > 2.0 * body; }              // :2109
    __device__ __forceinline__ bool lds() const { return ls > 2.0 * body; }              // :2113
    __device__ __forceinline__ bool sus() const { return us < 0.5 * body; }              // :2117
    __device__ __forceinline__ bool sds() const { return ls < 0.5 * body; }              // :2121
    __device__ __forceinline__ bool vsus() const { return us < 0.1 * body; }             // :2125
    __device__ __forceinline__ bool vsds() const { return ls < 0.1 * body; }             // :2129
    __device__ __forceinline__ bool vlds() const { return ls > 3.0 * body; }             // :2133
    __device__ __forceinline__ bool maru() const { return lng() & vsus() & vsds(); }
};
__device__ __forceinline__ bool nearq(double a, double b, const Cdl &k) { return fabs(a - b) < 0.01 * (k.h + k.l) * 0.5; }   // :2137
__device__ __forceinline__ bool equalq(double a, double b, const Cdl &k) { return fabs(a - b) < 0.001 * (k.h + k.l) * 0.5; } // :2141
__device__ __forceinline__ int pm(bool up, bool dn) { return up ? 100 : (dn ? -100 : 0); }

// a = current row, b .. e = 1 .. 4 rows back.  Returns the recogniser's value; caller masks t < lookback.
// The conditions are combined with the NON-short-circuit & and | on purpose: with `&` every term becomes a branch on the
// execution mask (a wave leaves a condition chain only when all 64 lanes fail it), and half of the kernel's instructions
// were scalar mask / branch instructions; with & / | each comparison is one v_cmp + one scalar AND and the recogniser is
// straight-line code.
__device__ __forceinline__ int cdl_eval(int id, const Cdl &a, const Cdl &b, const Cdl &c, const Cdl &d, const Cdl &e, double pen,
                                        int *lookback) {
    switch (id) {
    case 0: *lookback = 2; // cdl2crows :10-40
        return (c.bull() & c.lng() & b.bear() & b.o > c.c & a.bear() & a.o > b.o & a.o < b.c & a.c > c.o & a.c < c.c) ? -100 : 0;
    case 1: *lookback = 2; // cdl3blackcrows :43-73
        return (c.bear() & c.lng() & b.bear() & b.lng() & a.bear() & a.lng() & b.o < c.o & b.o > c.c & a.o < b.o & a.o > b.c &
                b.c < c.c & a.c < b.c) ? -100 : 0;
    case 2: *lookback = 2; // cdl3inside :76-111
        return pm(c.bear() & c.lng() & b.bull() & b.c < c.o & b.o > c.c & a.bull() & a.c > c.o,
                  c.bull() & c.lng() & b.bear() & b.o < c.c & b.c > c.o & a.bear() & a.c < c.o);
    case 3: *lookback = 3; // cdl3linestrike :114-157
        return pm(d.bear() & c.bear() & b.bear() & c.c < d.c & b.c < c.c & c.o > d.c & c.o < d.o & b.o > c.c & b.o < c.o &
                      a.bull() & a.o < b.c & a.c > d.o,
                  d.bull() & c.bull() & b.bull() & c.c > d.c & b.c > c.c & c.o < d.c & c.o > d.o & b.o < c.c & b.o > c.o &
                      a.bear() & a.o > b.c & a.c < d.o);
    case 4: *lookback = 2; // cdl3outside :160-191
        return pm(c.bear() & b.bull() & b.o <= c.c & b.c >= c.o & a.bull() & a.c > b.c,
                  c.bull() & b.bear() & b.o >= c.c & b.c <= c.o & a.bear() & a.c < b.c);
    case 5: *lookback = 2; // cdl3starsinsouth :194-231
        return (c.bear() & c.lng() & c.lds() & b.bear() & b.l > c.l & b.c > c.c & a.bear() & a.sht() & a.h < b.h & a.l > b.l) ? 100 : 0;
    case 6: *lookback = 2; // cdl3whitesoldiers :234-265
        return (c.bull() & c.lng() & b.bull() & b.lng() & a.bull() & a.lng() & b.o > c.o & b.o <= c.c & a.o > b.o & a.o <= b.c &
                b.c > c.c & a.c > b.c) ? 100 : 0;
    case 7: *lookback = 2; // cdlabandonedbaby :268-306
        return pm(c.bear() & c.lng() & b.doji() & b.h < c.l & a.bull() & a.l > b.h,
                  c.bull() & c.lng() & b.doji() & b.l > c.h & a.bear() & a.h < b.l);
    case 8: *lookback = 2; // cdladvanceblock :309-342
        return (c.bull() & c.lng() & b.bull() & a.bull() & b.o > c.o & b.o <= c.c & a.o > b.o & a.o <= b.c & b.c > c.c &
                a.c > b.c & a.body < b.body) ? -100 : 0;
    case 9: *lookback = 0; // cdlbelthold :345-370
        return pm(a.bull() & a.lng() & a.vsds(), a.bear() & a.lng() & a.vsus());
    case 10: *lookback = 4; // cdlbreakaway :373-411
        return pm(e.bear() & e.lng() & d.bear() & d.o < e.c & c.c < d.c & a.bull() & a.c > d.o & a.c < e.c,
                  e.bull() & e.lng() & d.bull() & d.o > e.c & c.c > d.c & a.bear() & a.c < d.o & a.c > e.c);
    case 11: *lookback = 0; // cdlclosingmarubozu :414-439
        return pm(a.bull() & a.lng() & a.vsus(), a.bear() & a.lng() & a.vsds());
    case 12: *lookback = 3; // cdlconcealbabyswall :442-484
        return (d.bear() & d.lng() & d.vsus() & d.vsds() & c.bear() & c.lng() & c.vsus() & c.vsds() & c.c < d.c & b.bear() &
                b.h > c.c & a.bear() & a.lng() & a.o > b.h & a.c < c.l) ? 100 : 0;
    case 13: *lookback = 1; // cdlcounterattack :487-516
        return pm(b.bear() & b.lng() & a.bull() & a.lng() & nearq(a.c, b.c, a), b.bull() & b.lng() & a.bear() & a.lng() & nearq(a.c, b.c, a));
    case 14: *lookback = 1; // cdldarkcloudcover :519-550
        return (b.bull() & b.lng() & a.bear() & a.o > b.c & a.c < (b.c - (b.body * pen)) & a.c > b.o) ? -100 : 0;
    case 15: *lookback = 0; // cdldoji :553-575
        return a.doji() ? 100 : 0;
    case 16: { *lookback = 1; // cdldojistar :578-607
        double mid = (a.o + a.c) / 2.0;
        return pm(b.bear() & b.lng() & a.doji() & mid < b.c, b.bull() & b.lng() & a.doji() & mid > b.c); }
    case 17: *lookback = 0; // cdldragonflydoji :610-632
        return (a.doji() & a.lds() & a.vsus()) ? 100 : 0;
    case 18: *lookback = 1; // cdlengulfing :635-662
        return pm(b.bear() & a.bull() & a.o <= b.c & a.c >= b.o & (a.o < b.c | a.c > b.o),
                  b.bull() & a.bear() & a.o >= b.c & a.c <= b.o & (a.o > b.c | a.c < b.o));
    case 19: *lookback = 2; // cdleveningdojistar :665-700
        return (c.bull() & c.lng() & b.doji() & b.mn > c.c & a.bear() & a.c < (c.c - (c.body * pen))) ? -100 : 0;
    case 20: *lookback = 2; // cdleveningstar :703-736
        return (c.bull() & c.lng() & b.sht() & b.mn > c.c & a.bear() & a.c < (c.c - (c.body * pen))) ? -100 : 0;
    case 21: { *lookback = 2; // cdlgapsidesidewhite :739-774
        bool common = b.bull() & a.bull() & nearq(a.body, b.body, a) & nearq(a.o, b.o, a);
        return pm(c.bull() & b.o > c.c & common, c.bear() & b.c < c.c & common); }
    case 22: *lookback = 0; // cdlgravestonedoji :777-799
        return (a.doji() & a.lus() & a.vsds()) ? -100 : 0;
    case 23: *lookback = 1; // cdlhammer :802-829
        return (a.sht() & a.ls > (2.0 * a.body) & a.vsus() & b.bear()) ? 100 : 0;
    case 24: *lookback = 1; // cdlhangingman :832-859
        return (a.sht() & a.ls > (2.0 * a.body) & a.vsus() & b.bull()) ? -100 : 0;
    case 25: *lookback = 1; // cdlharami :862-893
        return pm(b.bear() & b.lng() & a.bull() & a.sht() & a.o > b.c & a.c < b.o, b.bull() & b.lng() & a.bear() & a.sht() & a.o < b.c & a.c > b.o);
    case 26: *lookback = 1; // cdlharamicross :896-926
        return pm(b.bear() & b.lng() & a.doji() & a.mx < b.o & a.mn > b.c, b.bull() & b.lng() & a.doji() & a.mx < b.c & a.mn > b.o);
    case 27: { *lookback = 0; // cdlhighwave :929-953
        bool m = a.sht() & a.lus() & a.lds();
        return pm(m & a.bull(), m & a.bear()); }
    case 28: { *lookback = 2; // cdlhikkake :956-984
        bool inside = b.h < c.h & b.l > c.l;
        return pm(inside & a.c > c.h & a.bull(), inside & a.c < c.l & a.bear()); }
    case 29: { *lookback = 3; // cdlhikkakemod :987-1018
        bool inside = c.h < d.h & c.l > d.l & b.h < c.h & b.l > c.l;
        return pm(inside & a.c > d.h & a.bull(), inside & a.c < d.l & a.bear()); }
    case 30: *lookback = 1; // cdlhomingpigeon :1021-1045
        return (b.bear() & b.lng() & a.bear() & a.sht() & a.o < b.o & a.c > b.c) ? 100 : 0;
    case 31: *lookback = 2; // cdlidentical3crows :1048-1080
        return (c.bear() & c.lng() & b.bear() & b.lng() & a.bear() & a.lng() & equalq(b.o, c.c, a) & equalq(a.o, b.c, a) &
                b.c < c.c & a.c < b.c) ? -100 : 0;
    case 32: *lookback = 1; // cdlinneck :1083-1108
        return (b.bear() & b.lng() & a.bull() & a.o < b.c & nearq(a.c, b.c, a)) ? -100 : 0;
    case 33: *lookback = 1; // cdlinvertedhammer :1111-1138
        return (a.sht() & a.us > (2.0 * a.body) & a.vsds() & b.bear()) ? 100 : 0;
    case 34: *lookback = 1; // cdlkicking :1141-1180
        return pm(b.bear() & b.maru() & a.bull() & a.maru() & a.o > b.o, b.bull() & b.maru() & a.bear() & a.maru() & a.o < b.o);
    case 35: { *lookback = 1; // cdlkickingbylength :1183-1226
        bool bk = b.bear() & b.maru() & a.bull() & a.maru() & a.o > b.o;
        bool sk = b.bull() & b.maru() & a.bear() & a.maru() & a.o < b.o;
        bool longer = a.body >= b.body;
        bool bl = bk & longer, sl = sk & longer;
        return pm(bl | (bk & !sl), sl | (sk & !bl)); }
    case 36: *lookback = 4; // cdlladderbottom :1229-1264
        return (e.bear() & e.lng() & d.bear() & d.c < e.c & c.bear() & c.c < d.c & b.bear() & b.lus() & a.bull() & a.o > b.o) ? 100 : 0;
    case 37: *lookback = 0; // cdllongleggeddoji :1267-1289
        return (a.doji() & a.lus() & a.lds()) ? 100 : 0;
    case 38: { *lookback = 0; // cdllongline :1292-1318
        bool m = a.lng() & a.sus() & a.sds();
        return pm(m & a.bull(), m & a.bear()); }
    case 39: { *lookback = 0; // cdlmarubozu :1321-1346
        bool m = a.maru();
        return pm(m & a.bull(), m & a.bear()); }
    case 40: *lookback = 1; // cdlmatchinglow :1349-1373
        return (b.bear() & b.lng() & a.bear() & equalq(a.c, b.c, a)) ? 100 : 0;
    case 41: *lookback = 4; // cdlmathold :1376-1413
        return (e.bull() & e.lng() & d.sht() & d.o > e.c & c.sht() & b.sht() & d.l > e.o & c.l > e.o & b.l > e.o & a.bull() &
                a.c > e.c) ? 100 : 0;
    case 42: *lookback = 2; // cdlmorningdojistar :1416-1451
        return (c.bear() & c.lng() & b.doji() & b.mx < c.c & a.bull() & a.c > (c.c + (c.body * pen))) ? 100 : 0;
    case 43: *lookback = 2; // cdlmorningstar :1454-1487
        return (c.bear() & c.lng() & b.sht() & b.mx < c.c & a.bull() & a.c > (c.c + (c.body * pen))) ? 100 : 0;
    case 44: *lookback = 1; // cdlonneck :1490-1516
        return (b.bear() & b.lng() & a.bull() & a.o < b.c & nearq(a.c, b.l, a)) ? -100 : 0;
    case 45: *lookback = 1; // cdlpiercing :1519-1550
        return (b.bear() & b.lng() & a.bull() & a.o < b.c & a.c > (b.c + (b.body * pen)) & a.c < b.o) ? 100 : 0;
    case 46: *lookback = 0; // cdlrickshawman :1553-1578
        return (a.doji() & a.lus() & a.lds() & nearq(a.us, a.ls, a)) ? 100 : 0;
    case 47: { *lookback = 4; // cdlrisefall3methods :1581-1644
        bool mid = d.sht() & c.sht() & b.sht() & d.h < e.h & c.h < e.h & b.h < e.h & d.l > e.l & c.l > e.l & b.l > e.l;
        return pm(e.bull() & e.lng() & mid & a.bull() & a.lng() & a.c > e.c, e.bear() & e.lng() & mid & a.bear() & a.lng() & a.c < e.c); }
    case 48: *lookback = 1; // cdlseparatinglines :1647-1676
        return pm(b.bear() & b.lng() & a.bull() & a.lng() & equalq(a.o, b.o, a), b.bull() & b.lng() & a.bear() & a.lng() & equalq(a.o, b.o, a));
    case 49: *lookback = 1; // cdlshootingstar :1679-1706
        return (a.sht() & a.us > (2.0 * a.body) & a.vsds() & b.bull()) ? -100 : 0;
    case 50: { *lookback = 0; // cdlshortline :1709-1735
        bool m = a.sht() & a.sus() & a.sds();
        return pm(m & a.bull(), m & a.bear()); }
    case 51: { *lookback = 0; // cdlspinningtop :1738-1763
        bool m = a.sht() & a.us > a.body & a.ls > a.body;
        return pm(m & a.bull(), m & a.bear()); }
    case 52: *lookback = 2; // cdlstalledpattern :1766-1794
        return (c.bull() & c.lng() & b.bull() & b.lng() & b.c > c.c & a.bull() & a.sht() & a.c > b.c & a.o > b.o & a.o <= b.c) ? -100 : 0;
    case 53: *lookback = 2; // cdlsticksandwich :1797-1828
        return (c.bear() & c.lng() & b.bull() & b.lng() & b.o > c.c & a.bear() & a.lng() & equalq(a.c, c.c, a)) ? 100 : 0;
    case 54: *lookback = 0; // cdltakuri :1831-1853
        return (a.doji() & a.vlds() & a.vsus()) ? 100 : 0;
    case 55: *lookback = 2; // cdltasukigap :1856-1891
        return pm(c.bull() & b.bull() & b.o > c.c & a.bear() & a.o > b.o & a.o < b.c & a.c > c.o & a.c < c.c,
                  c.bear() & b.bear() & b.o < c.c & a.bull() & a.o < b.o & a.o > b.c & a.c < c.o & a.c > c.c);
    case 56: { *lookback = 1; // cdlthrusting :1894-1919
        double midpoint = b.c + (b.body * 0.5);
        return (b.bear() & b.lng() & a.bull() & a.o < b.c & a.c > b.c & a.c < midpoint) ? -100 : 0; }
    case 57: { *lookback = 2; // cdltristar :1922-1961
        bool dj = c.doji() & b.doji() & a.doji();
        double m1 = (c.o + c.c) / 2.0, m2 = (b.o + b.c) / 2.0, m3 = (a.o + a.c) / 2.0;
        return pm(dj & m2 < m1 & m3 > m2, dj & m2 > m1 & m3 < m2); }
    case 58: *lookback = 2; // cdlunique3river :1964-1994
        return (c.bear() & c.lng() & b.bear() & b.l < c.l & b.c > b.l & b.o < c.o & b.o > c.c & a.bull() & a.sht() & a.c < b.c) ? 100 : 0;
    case 59: *lookback = 2; // cdlupsidegap2crows :1997-2024
        return (c.bull() & c.lng() & b.bear() & b.o > c.c & b.c > c.c & a.bear() & a.o > b.o & a.c > c.c & a.c < b.c) ? -100 : 0;
    case 60: *lookback = 2; // cdlxsidegap3methods :2027-2062
        return pm(c.bull() & b.bull() & b.o > c.c & a.bear() & a.o < b.c & a.o > b.o & a.c > c.o & a.c < c.c,
                  c.bear() & b.bear() & b.o < c.c & a.bull() & a.o > b.c & a.o < b.o & a.c < c.o & a.c > c.c);
    }
    *lookback = 0;
    return 0;
}

struct CdlArgs { // cdl_one_kernel: slot 0.  cdl_all_kernel: slot k belongs to recogniser k_cdl_order[k] (below), the k-th it evaluates
    const double *o, *h, *l, *c;
    int32_t *out[PQ_N_PATTERNS];
    double pen[PQ_N_PATTERNS];
};

__device__ __forceinline__ Cdl load_candle(const CdlArgs &a, int64_t base, int64_t q) {
    Cdl k;
    if (q >= 0) k.set(a.o[base + q], a.h[base + q], a.l[base + q], a.c[base + q]);
    else k.set(0.0, 0.0, 0.0, 0.0);
    return k;
}

// R consecutive rows per thread: the R + 4 candles they look at are loaded and classified once (instead of 5 per row), and
// each recogniser's R results leave as one 4R-byte store.  `vec`: the int32 rows are 4R-byte aligned (stride % R == 0).
// Measured at 5000 x 2520 (solo / suite step, one session, on the rolled form of rounds 2 - 6): R = 1 0.87 / 5.34 ms, R = 2 1.07 / 5.42,
// R = 4 2.41 / 6.28 (the classified candles of more rows cost more registers than the shared loads save) -- 0.87 ms is 3.75 GB at
// 4.3 TB/s, the non-temporal store ceiling.  Before the recognisers were made branch-free (see cdl_eval) the kernel took 1.4 ms solo.
// (R > 1 still compiles in the straight-line form below -- 99 - 104 VGPRs, no scratch at R = 2 -- and was not measured again.)
#ifndef PQ_CDL_R
#define PQ_CDL_R 1
#endif
constexpr int CDL_R = PQ_CDL_R;

// The order in which the all-patterns kernel evaluates and stores the recognisers: grouped by the oldest candle they read, deepest
// window first (a .. e, then a .. d, a .. c, a .. b, a alone), so that the raw values and predicate masks of e, d, c and b die group by
// group and the 5 x 12 predicate masks (one SGPR pair each) are never all live at once.
constexpr int k_cdl_order[PQ_N_PATTERNS] = {
    10, 36, 41, 47,                                                                                  // a .. e (look-back 4)
    3, 12, 29,                                                                                       // a .. d (3)
    0, 1, 2, 4, 5, 6, 7, 8, 19, 20, 21, 28, 31, 42, 43, 52, 53, 55, 57, 58, 59, 60,                  // a .. c (2)
    13, 14, 16, 18, 23, 24, 25, 26, 30, 32, 33, 34, 35, 40, 44, 45, 48, 49, 56,                      // a, b   (1)
    9, 11, 15, 17, 22, 27, 37, 38, 39, 46, 50, 51, 54};                                              // a      (0)
constexpr bool cdl_order_is_permutation() {
    bool seen[PQ_N_PATTERNS] = {};
    for (int id : k_cdl_order) {
        if (id < 0 || id >= PQ_N_PATTERNS || seen[id]) return false;
        seen[id] = true;
    }
    return true;
}
static_assert(cdl_order_is_permutation(), "k_cdl_order names every recogniser exactly once");

typedef __attribute__((address_space(1))) int pq_gint;
typedef __attribute__((address_space(1))) unsigned char pq_gbyte1;
// What one wave shares while it stores: rows0 = the series' first row + the wave's first row, in elements (wave-uniform, in scalar
// registers); lane_b = this lane's byte offset from there (32 bits).
struct CdlRows {
    int64_t rows0;
    unsigned lane_b;
    int64_t t0, slen;
    bool ge[CDL_R][5]; // ge[r][lb]: row t0 + r has lb rows before it
};
// The column pointers, CDL_PB at a time and one batch ahead: `cur` = the slots of the batch being evaluated, `nxt` = the batch after it,
// whose scalar loads (one s_load_dwordx8) are issued by the first recogniser of the current batch and waited for CDL_PB recognisers later.
// They are read from the kernel's first argument where it lies -- offset 0 of the kernarg segment -- through a pointer that is made opaque
// in front of every batch, which pins the loads there.  Read through the by-value argument, all 61 pointers were loaded at the top of the
// kernel: 122 scalar registers, which the allocator moved to vector lanes and back (212 lane moves); read at their use without the
// batch ahead, each batch of stores waited for its own load.
#ifndef PQ_CDL_PB
#define PQ_CDL_PB 4 // (8: one s_load_dwordx16 per batch, but 32 scalar registers of pointers: 80 lane moves against 48; 3.503 / 3.506 against 3.509 / 3.506 ms per step)
#endif
constexpr int CDL_PB = PQ_CDL_PB;
typedef __attribute__((address_space(4))) const CdlArgs pq_cdl_kargs;
struct CdlCols {
    pq_cdl_kargs *ka;
    int32_t *cur[CDL_PB], *nxt[CDL_PB];
    template <int K0>
    __device__ __forceinline__ void fetch() { // nxt = slots K0 .. K0 + CDL_PB - 1
        asm volatile("" : "+s"(ka));
#pragma unroll
        for (int j = 0; j < CDL_PB; j++) nxt[j] = K0 + j < PQ_N_PATTERNS ? ka->out[K0 + j] : nullptr;
    }
    template <int K>
    __device__ __forceinline__ void advance() { // in front of slot K
        if constexpr (K % CDL_PB == 0) {
#pragma unroll
            for (int j = 0; j < CDL_PB; j++) cur[j] = nxt[j];
            if constexpr (K + CDL_PB < PQ_N_PATTERNS) fetch<K + CDL_PB>();
        }
    }
};
// The K-th recogniser for the thread's R rows, evaluated and stored at once.  Its id is a constant: cdl_eval's switch and look-back fold,
// its column pointer and penetration are fixed kernel-argument offsets (consecutive slots in the order of use), and the store is the job
// kernel's form (pq_dev.h run_seq_lds): a wave-uniform 64-bit base in scalar registers -- two scalar adds per column -- plus the lane's
// 32-bit offset.
template <int K, bool ALL, bool VEC>
__device__ __forceinline__ void cdl_emit(const CdlArgs &a, CdlCols &cols, const Cdl (&w)[CDL_R + 4], const CdlRows &g) {
    constexpr int ID = k_cdl_order[K];
    cols.template advance<K>();
    int32_t *const col = cols.cur[K % CDL_PB];
    if (!ALL && col == nullptr) return; // wave-uniform
    int v[CDL_R];
#pragma unroll
    for (int r = 0; r < CDL_R; r++) { // row t0 + r: current candle w[CDL_R - 1 - r]
        int lb;
        const int x = cdl_eval(ID, w[CDL_R - 1 - r], w[CDL_R - r], w[CDL_R + 1 - r], w[CDL_R + 2 - r], w[CDL_R + 3 - r], a.pen[K], &lb);
        v[r] = g.ge[r][lb] ? x : 0;
    }
    const unsigned long long p = reinterpret_cast<unsigned long long>(col + g.rows0);
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
    asm("" : "+s"(lo), "+s"(hi)); // (opaque: otherwise base and lane offset are folded into one 64-bit vector address per store)
    unsigned off = g.lane_b;
    asm volatile("" : "+v"(off));
    pq_gint *dst = (pq_gint *)((pq_gbyte1 *)(((unsigned long long)hi << 32) | lo) + off);
#if PQ_EXP_NOSTORE_ON
    if (v[0] == 123456789) *dst = v[0];
#else
    if (VEC && (CDL_R == 1 || g.t0 + CDL_R <= g.slen)) {
        typedef int pq_irv __attribute__((ext_vector_type(CDL_R)));
        typedef __attribute__((address_space(1))) pq_irv pq_girv;
        pq_irv vv;
#pragma unroll
        for (int r = 0; r < CDL_R; r++) vv[r] = v[r];
        __builtin_nontemporal_store(vv, (pq_girv *)dst);
    } else {
#pragma unroll
        for (int r = 0; r < CDL_R; r++)
            if (g.t0 + r < g.slen) __builtin_nontemporal_store(v[r], dst + r);
    }
#endif
}
template <bool ALL, bool VEC, int... KS>
__device__ __forceinline__ void cdl_emit_all(const CdlArgs &a, CdlCols &cols, const Cdl (&w)[CDL_R + 4], const CdlRows &g, std::integer_sequence<int, KS...>) {
    // (the scheduling barrier keeps the recognisers apart: without it the scheduler moves all ~130 comparisons of the block in front of the
    //  first store, every mask is live at once, and the kernel spends 700 instructions moving scalar registers to vector lanes and back)
    ((cdl_emit<KS, ALL, VEC>(a, cols, w, g), __builtin_amdgcn_sched_barrier(0)), ...);
}

// ALL: every recogniser has an output column (the usual call): no per-recogniser test of its pointer -- 61 uniform branches per row,
// each the end of a scheduling region -- and one store form (VEC: the int32 rows are 4R-byte aligned).
// The 61 recognisers are expanded at compile time (cdl_emit_all over k_cdl_order): straight-line code, one store site per recogniser.
// Beside two 192-VGPR job waves one wave of this kernel fits on a SIMD (it needs <= 128 VGPRs and no scratch: pattern.resources.txt,
// tests/test_pattern_resources.py), 193 of them run in series per slot, and inside a suite step the kernel is bound by the length of one
// wave's instruction stream, not by its bytes.  As a `#pragma unroll` loop over a runtime id the compiler had kept all 61 results in
// registers (110 VGPRs) and a rolled loop of 8 x 8 stores that picked each value with a branch tree on the counter and loaded each column
// pointer, waited for, in front of its store.  <true, true> in the listing (hipcc -S, gfx950), before -> now: 1 522 -> 1 203 instructions
// (static; executed per wave about 2 700 -> 1 200), 127 -> 9 branches, 8 -> 61 store sites, 64 -> 16 scalar pointer loads per wave (none
// waited for at its store), 110 -> 82 VGPRs, 12 -> 48 lane moves of spilled scalar registers, no scratch.  Suite step at 5 000 x 2 520,
// parent and this form alternated, three runs each: 3.627 / 3.611 / 3.630 -> 3.500 / 3.492 / 3.500 ms (EXPERIMENTS.md).
template <bool ALL, bool VEC>
__global__ __launch_bounds__(ROW_BLOCK) void cdl_all_kernel(CdlArgs a, Dims d) {
    const int64_t s = blockIdx.y;
    const int64_t t0 = ((int64_t)blockIdx.x * ROW_BLOCK + threadIdx.x) * CDL_R;
    const int64_t slen = dims_len(d, s);
    if (t0 >= slen) return;
    const int64_t base = dims_base(d, s);
    // Issue priority beside the SEQ grids of a suite (whose long jobs raise their own).  Round 2: 1 (the kernel was only issued in the gaps
    // and became the critical path at 0; 3 cost +4 %).  Round 3: 0 -- its waves now sit beside two job waves on every SIMD (192-VGPR job
    // kernel) and advance all the time; at 0 they take what the job waves leave: 4.06 against 4.12 ms per step (2: 4.12, 3: 4.19).
    // On the straight-line form: 0 3.509 / 3.506, 1 3.502 / 3.507 ms per step -- no difference, 0 stays.
#ifndef PQ_CDL_PRIO
#define PQ_CDL_PRIO 0
#endif
    __builtin_amdgcn_s_setprio(PQ_CDL_PRIO);
    CdlCols cols;
    cols.ka = (pq_cdl_kargs *)__builtin_amdgcn_kernarg_segment_ptr();
    cols.template fetch<0>(); // (beside the candle loads)
    Cdl w[CDL_R + 4]; // w[k] = candle of row t0 + CDL_R - 1 - k
#pragma unroll
    for (int k = 0; k < CDL_R + 4; k++) {
        const int64_t q = t0 + CDL_R - 1 - k;
        w[k] = load_candle(a, base, q < slen ? q : slen - 1); // rows past the end (ragged last thread) are never stored
    }
    CdlRows g;
    const unsigned wave_row0 = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u); // (every lane of the wave holds the same value)
    g.rows0 = base + ((int64_t)blockIdx.x * ROW_BLOCK + wave_row0) * CDL_R;
    g.lane_b = (threadIdx.x & 63u) * (unsigned)(4 * CDL_R);
    g.t0 = t0;
    g.slen = slen;
#pragma unroll
    for (int r = 0; r < CDL_R; r++)
#pragma unroll
        for (int lb = 0; lb < 5; lb++) g.ge[r][lb] = t0 + r >= lb;
    cdl_emit_all<ALL, VEC>(a, cols, w, g, std::make_integer_sequence<int, PQ_N_PATTERNS>{});
}

__global__ __launch_bounds__(ROW_BLOCK) void cdl_one_kernel(CdlArgs a, int id, Dims d) {
    const int64_t s = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * ROW_BLOCK + threadIdx.x;
    if (t >= dims_len(d, s)) return;
    const int64_t base = dims_base(d, s);
    Cdl w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = load_candle(a, base, t - k);
    int lb;
    int v = cdl_eval(id, w[0], w[1], w[2], w[3], w[4], a.pen[0], &lb);
    a.out[0][base + t] = (t >= lb) ? v : 0;
}

static const char *const k_pattern_names[PQ_N_PATTERNS] = {
    "cdl2crows", "cdl3blackcrows", "cdl3inside", "cdl3linestrike", "cdl3outside", "cdl3starsinsouth",
    "cdl3whitesoldiers", "cdlabandonedbaby", "cdladvanceblock", "cdlbelthold", "cdlbreakaway",
    "cdlclosingmarubozu", "cdlconcealbabyswall", "cdlcounterattack", "cdldarkcloudcover", "cdldoji",
    "cdldojistar", "cdldragonflydoji", "cdlengulfing", "cdleveningdojistar", "cdleveningstar",
    "cdlgapsidesidewhite", "cdlgravestonedoji", "cdlhammer", "cdlhangingman", "cdlharami", "cdlharamicross",
    "cdlhighwave", "cdlhikkake", "cdlhikkakemod", "cdlhomingpigeon", "cdlidentical3crows", "cdlinneck",
    "cdlinvertedhammer", "cdlkicking", "cdlkickingbylength", "cdlladderbottom", "cdllongleggeddoji",
    "cdllongline", "cdlmarubozu", "cdlmatchinglow", "cdlmathold", "cdlmorningdojistar", "cdlmorningstar",
    "cdlonneck", "cdlpiercing", "cdlrickshawman", "cdlrisefall3methods", "cdlseparatinglines",
    "cdlshootingstar", "cdlshortline", "cdlspinningtop", "cdlstalledpattern", "cdlsticksandwich", "cdltakuri",
    "cdltasukigap", "cdlthrusting", "cdltristar", "cdlunique3river", "cdlupsidegap2crows",
    "cdlxsidegap3methods"};

#include <string.h>
extern "C" {

const char *pq_pattern_name(int32_t id) { return (id >= 0 && id < PQ_N_PATTERNS) ? k_pattern_names[id] : nullptr; }
int32_t pq_pattern_id(const char *name) {
    if (!name) return -1;
    for (int i = 0; i < PQ_N_PATTERNS; i++)
        if (strcmp(name, k_pattern_names[i]) == 0) return i;
    return -1;
}

struct CdlBlob {
    CdlArgs args;
    int id;
    pq_batch b;
};
static void cdl_launch_blob(const void *blob, hipStream_t stream);
static pq_status cdl_launch(pq_ctx *ctx, const pq_batch *b, const CdlArgs &args, int id) {
    if (b->n_series == 0 || b->len == 0) return PQ_OK;
    CdlBlob cb{args, id, *b};
    if (ctx->rec) {
        static_assert(sizeof(CdlBlob) <= sizeof(RowThunk::blob), "CdlBlob too large");
        RowThunk t;
        t.launch = &cdl_launch_blob;
        t.row_id = 0;
        t.blob_bytes = (int)sizeof cb;
        t.dims = dims_of(b);
        memcpy(t.blob, &cb, sizeof cb);
        t.n_reads = 4;
        t.reads[0] = args.o; t.reads[1] = args.h; t.reads[2] = args.l; t.reads[3] = args.c;
        t.n_writes = 0;
        for (int i = 0; i < PQ_N_PATTERNS; i++) if (args.out[i]) t.writes[t.n_writes++] = args.out[i];
        return rec_add_row(ctx, t);
    }
    cdl_launch_blob(&cb, ctx->stream);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}
static void cdl_launch_blob(const void *blob, hipStream_t stream) {
    const CdlBlob &cb = *reinterpret_cast<const CdlBlob *>(blob);
    const pq_batch *b = &cb.b;
    const CdlArgs &args = cb.args;
    const int id = cb.id;
    for (int64_t s0 = 0; s0 < b->n_series; s0 += 65535) {
        int64_t ns = b->n_series - s0 < 65535 ? b->n_series - s0 : 65535;
        CdlArgs a2 = args;
        int64_t off = b->offsets ? 0 : s0 * b->stride; // (a ragged slice keeps the column pointers: its offsets are absolute rows)
        a2.o += off; a2.h += off; a2.l += off; a2.c += off;
        for (int i = 0; i < PQ_N_PATTERNS; i++) if (a2.out[i]) a2.out[i] += off;
        dim3 grid((unsigned)((b->len + ROW_BLOCK - 1) / ROW_BLOCK), (unsigned)ns);
        Dims d{ns, b->len, b->stride, b->offsets ? b->offsets + s0 : nullptr};
        if (id < 0) {
            int vec = (b->stride % CDL_R) == 0 && !b->offsets;
            for (int i = 0; i < PQ_N_PATTERNS; i++)
                if (a2.out[i] && reinterpret_cast<uintptr_t>(a2.out[i]) % (4 * CDL_R)) vec = 0;
            const int64_t per_block = (int64_t)ROW_BLOCK * CDL_R;
            dim3 grid2((unsigned)((b->len + per_block - 1) / per_block), (unsigned)ns);
            bool all = true;
            for (int i = 0; i < PQ_N_PATTERNS; i++) all &= a2.out[i] != nullptr;
            if (all && vec) hipLaunchKernelGGL((cdl_all_kernel<true, true>), grid2, dim3(ROW_BLOCK), 0, stream, a2, d);
            else if (all) hipLaunchKernelGGL((cdl_all_kernel<true, false>), grid2, dim3(ROW_BLOCK), 0, stream, a2, d);
            else if (vec) hipLaunchKernelGGL((cdl_all_kernel<false, true>), grid2, dim3(ROW_BLOCK), 0, stream, a2, d);
            else hipLaunchKernelGGL((cdl_all_kernel<false, false>), grid2, dim3(ROW_BLOCK), 0, stream, a2, d);
        } else hipLaunchKernelGGL(cdl_one_kernel, grid, dim3(ROW_BLOCK), 0, stream, a2, id, d);
    }
}

pq_status pq_cdl(pq_ctx *ctx, const pq_batch *b, int32_t id, const double *o, const double *h, const double *l,
                 const double *c, double penetration, int32_t *out) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(o && h && l && c && out, "pq_cdl: null pointer");
    PQ_REQUIRE(id >= 0 && id < PQ_N_PATTERNS, "pq_cdl: pattern id out of range");
    CdlArgs a;
    memset(&a, 0, sizeof a);
    a.o = o; a.h = h; a.l = l; a.c = c;
    a.out[0] = out; a.pen[0] = penetration;
    return cdl_launch(ctx, b, a, id);
}

pq_status pq_cdl_all(pq_ctx *ctx, const pq_batch *b, const double *o, const double *h, const double *l,
                     const double *c, const double *penetrations, int32_t *const *outs) {
    PQ_TRY(pq_check(ctx, b));
    PQ_REQUIRE(o && h && l && c && penetrations && outs, "pq_cdl_all: null pointer");
    CdlArgs a;
    memset(&a, 0, sizeof a);
    a.o = o; a.h = h; a.l = l; a.c = c;
    for (int k = 0; k < PQ_N_PATTERNS; k++) { a.out[k] = outs[k_cdl_order[k]]; a.pen[k] = penetrations[k_cdl_order[k]]; }
    return cdl_launch(ctx, b, a, -1);
}

} // extern "C"
