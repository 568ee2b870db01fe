// report/report.hip -- the README's statistics report of `Backtest` (README.md:511-548, :627-640; README-only => decision D-22, DESIGN.md
// section 2): PQ_REPORT_COLS values per symbol from its total_value row, its closed-trade records and the shared benchmark, and the
// portfolio row built from those rows.
//
//  rp_symbol_kernel: one wavefront per symbol, four symbols per workgroup.  Lane k owns days k, k + 64, ...: a load instruction reads 512
//                    contiguous bytes, and the 64 partial sums of D-22's summation order are the lanes' own accumulators, folded by
//                    shuffles at the end.  The first pass forms the returns (the previous day comes from the lane below, across a tile
//                    edge from the last lane of the tile before), the running peak (a wave max-scan plus the carried peak), the under-water
//                    run lengths (a max-scan of "last day not under water", as rolling.hip marks unusable entries) and the first-moment
//                    sums; the second pass re-reads the row -- from L2, 20 KB a symbol -- for the centred sums.  Four tiles of loads are
//                    issued before the first is consumed.  The trade records follow in the same form, lane per trade.  Nothing of
//                    [N, T] is written.
//  rp_block_kernel / rp_total_kernel: the portfolio row.  One workgroup per block of 256 symbols stages the five summed columns in LDS
//                    and adds each in ascending symbol order (D-10's order); counts and extrema are reduced in any order.  One wave then
//                    adds the block records in ascending order and forms the ratios.
#include "../pq_dev.h"

namespace {

constexpr int RP_WAVES = 4;                                     // symbols per workgroup
constexpr int RP_UNROLL = 4;                                    // tiles of 64 days loaded ahead
constexpr int RP_BLOCK = 256;                                   // D-10's summation block (symbols)
constexpr double RP_SQRT252 = 15.874507866387544;               // sqrt(252.0), correctly rounded
constexpr double RP_RF = 0.03, RP_DAYS = 252.0;
constexpr long long RP_NONE = -(1LL << 62);                      // no candidate in an index reduction

__device__ __forceinline__ double rp_inf() { return __longlong_as_double(0x7FF0000000000000LL); }

// D-22's fold of the 64 partials: p[k] += p[k + s] for k < s, s = 32 .. 1; the result p[0] goes to every lane.  Lanes >= s add
// values that no lower lane reads again.
__device__ __forceinline__ double rp_fold(double p) {
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return __shfl(p, 0, 64);
}
__device__ __forceinline__ long long rp_isum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long rp_imax(long long v) {
    for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ double rp_dmax(double v) {
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ double rp_dmin(double v) {
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}
// inclusive max-scan over the wave, joined with the value carried from the tiles before; the new carry is the last lane's
__device__ __forceinline__ long long rp_scan_imax(long long v, long long &carry, int lane) {
    for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(v, o, 64); if (lane >= o && u > v) v = u; }
    v = carry > v ? carry : v;
    carry = __shfl(v, 63, 64);
    return v;
}
__device__ __forceinline__ double rp_scan_dmax(double v, double &carry, int lane) {
    for (int o = 1; o < 64; o <<= 1) { const double u = __shfl_up(v, o, 64); if (lane >= o && u > v) v = u; }
    v = carry > v ? carry : v;
    carry = __shfl(v, 63, 64);
    return v;
}
__device__ __forceinline__ double rp_div(double a, double b) { return b == 0.0 ? pq_null() : a / b; }

struct RpTrades {
    int32_t max_trades;
    const int32_t *count, *entry_day, *exit_day, *reason;      // count: nullable; the records: all or none
    const double *entry_price, *exit_price, *quantity, *pnl;
    double rate, min_commission;
};

// the daily return of one tile: the previous value is the lane below's, lane 0 takes the one carried across the tile edge
__device__ __forceinline__ double rp_return(double v, double &carry, int lane) {
    double pv = __shfl_up(v, 1, 64);
    if (lane == 0) pv = carry;
    carry = __shfl(v, 63, 64);
    return pv > 0.0 ? (v - pv) / pv : 0.0;
}

template <bool BENCH>
__global__ __launch_bounds__(RP_WAVES * 64) void rp_symbol_kernel(const double *tv, Dims d, double c0, const double *bm, RpTrades tr, double *report) {
    __shared__ double stage[RP_WAVES][PQ_REPORT_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * RP_WAVES + wave, T = d.len;
    if (s < d.n) {
        double *o = stage[wave];
        const double *row = tv + s * d.stride;
        const double dT = (double)T;
        // ---- pass 1: returns, peak, under-water runs, first moments
        double s_r = 0.0, s_b = 0.0, s_a = 0.0, s_neg = 0.0, maxdd = 0.0;
        long long n_pos = 0, n_neg = 0, n_ahead = 0, maxrun = 0, bad = 0, bbad = 0;
        double cv = c0, cb = 0.0, cpeak = c0;
        long long clast = -1;
        for (int64_t t0 = 0; t0 < T; t0 += 64 * RP_UNROLL) {
            double vv[RP_UNROLL], bb[RP_UNROLL];
#pragma unroll
            for (int u = 0; u < RP_UNROLL; u++) {
                const int64_t i = t0 + u * 64 + lane;
                vv[u] = i < T ? row[i] : 0.0;
                if (BENCH) bb[u] = i < T ? bm[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < RP_UNROLL; u++) {
                const int64_t i = t0 + u * 64 + lane;
                if (t0 + u * 64 >= T) break;                    // wave-uniform
                const bool act = i < T;
                const double v = vv[u];
                bad |= act && !isfinite(v);                     // NULL is a NaN
                double r = rp_return(v, cv, lane);                // every lane takes part in the shuffles
                if (!act) r = 0.0;
                const double peak = rp_scan_dmax(act ? v : -rp_inf(), cpeak, lane);
                const bool under = act && v < peak;
                const double dd = act ? (peak - v) / peak : 0.0;
                maxdd = dd > maxdd ? dd : maxdd;
                const long long last = rp_scan_imax(act && !under ? (long long)i : -1, clast, lane);
                const long long run = under ? (long long)i - last : 0;
                maxrun = run > maxrun ? run : maxrun;
                s_r += r;
                s_neg += r < 0.0 ? r * r : 0.0;
                n_pos += r > 0.0;
                n_neg += r < 0.0;
                if (BENCH) {
                    const double b = bb[u];
                    bbad |= act && !isfinite(b);
                    double rb = rp_return(b, cb, lane);
                    if (!act || i == 0) rb = 0.0;
                    const double a = r - rb;
                    s_b += rb;
                    s_a += a;
                    n_ahead += act && r > rb;
                }
            }
        }
        const double S_r = rp_fold(s_r), S_neg = rp_fold(s_neg);
        const double mean = S_r / dT;
        double S_b = 0.0, mean_b = 0.0, alpha = 0.0;
        if (BENCH) { S_b = rp_fold(s_b); mean_b = S_b / dT; alpha = rp_fold(s_a) / dT; }
        maxdd = rp_dmax(maxdd);
        maxrun = rp_imax(maxrun);
        n_pos = rp_isum(n_pos); n_neg = rp_isum(n_neg); n_ahead = rp_isum(n_ahead);
        bad = rp_imax(bad); bbad = rp_imax(bbad);
        // ---- pass 2: the centred sums, from the row again (L2)
        double q_r = 0.0, q_c = 0.0, q_b = 0.0, q_a = 0.0;
        cv = c0; cb = 0.0;
        for (int64_t t0 = 0; t0 < T; t0 += 64 * RP_UNROLL) {
            double vv[RP_UNROLL], bb[RP_UNROLL];
#pragma unroll
            for (int u = 0; u < RP_UNROLL; u++) {
                const int64_t i = t0 + u * 64 + lane;
                vv[u] = i < T ? row[i] : 0.0;
                if (BENCH) bb[u] = i < T ? bm[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < RP_UNROLL; u++) {
                const int64_t i = t0 + u * 64 + lane;
                if (t0 + u * 64 >= T) break;
                const bool act = i < T;
                const double r = rp_return(vv[u], cv, lane);
                const double dr = r - mean;
                q_r += act ? dr * dr : 0.0;
                if (BENCH) {
                    double rb = rp_return(bb[u], cb, lane);
                    if (i == 0) rb = 0.0;
                    const double db = rb - mean_b, da = (r - rb) - alpha;
                    q_c += act ? dr * db : 0.0;
                    q_b += act ? db * db : 0.0;
                    q_a += act ? da * da : 0.0;
                }
            }
        }
        const double Q_r = rp_fold(q_r);
        double Q_c = 0.0, Q_b = 0.0, Q_a = 0.0;
        if (BENCH) { Q_c = rp_fold(q_c); Q_b = rp_fold(q_b); Q_a = rp_fold(q_a); }
        // ---- the trades, lane per record
        const long long cnt = tr.count ? (long long)tr.count[s] : -1;
        const bool rec = tr.pnl && cnt >= 0 && cnt <= (long long)tr.max_trades;
        double gp = 0.0, gl = 0.0, s_cost = 0.0, s_rev = 0.0, f_in = 0.0, f_out = 0.0, maxw = -rp_inf(), minl = rp_inf();
        long long nw = 0, nl = 0, hw = 0, hl = 0, ht = 0, mc = 0, runw = 0, runl = 0, cw = -1, cl = -1;
        if (rec) {
            const int64_t rb0 = s * (int64_t)tr.max_trades;
            for (int64_t j0 = 0; j0 < cnt; j0 += 64) {
                const int64_t j = j0 + lane;
                const bool act = j < cnt;
                double pnl = 0.0, q = 0.0, ep = 0.0, xp = 0.0;
                long long hold = 0;
                int reason = 0;
                if (act) {
                    pnl = tr.pnl[rb0 + j]; q = tr.quantity[rb0 + j]; ep = tr.entry_price[rb0 + j]; xp = tr.exit_price[rb0 + j];
                    hold = (long long)tr.exit_day[rb0 + j] - (long long)tr.entry_day[rb0 + j];
                    reason = tr.reason[rb0 + j];
                }
                const bool win = act && pnl > 0.0, los = act && pnl < 0.0;
                gp += win ? pnl : 0.0;
                gl += los ? pnl : 0.0;
                nw += win; nl += los;
                hw += win ? hold : 0; hl += los ? hold : 0; ht += hold;
                maxw = win && pnl > maxw ? pnl : maxw;
                minl = los && pnl < minl ? pnl : minl;
                const double cost = q * ep, rev = q * xp;        // the engine's own cost and rev
                s_cost += cost;
                s_rev += rev;
                f_in += act ? fmax(cost * tr.rate, tr.min_commission) : 0.0;
                f_out += act ? fmax(rev * tr.rate, tr.min_commission) : 0.0;
                mc += reason == 2;
                const long long lw = rp_scan_imax(act && !win ? (long long)j : -1, cw, lane);
                const long long ll = rp_scan_imax(act && !los ? (long long)j : -1, cl, lane);
                const long long rw = win ? (long long)j - lw : 0, rl = los ? (long long)j - ll : 0;
                runw = rw > runw ? rw : runw;
                runl = rl > runl ? rl : runl;
            }
            gp = rp_fold(gp); gl = rp_fold(gl); s_cost = rp_fold(s_cost); s_rev = rp_fold(s_rev); f_in = rp_fold(f_in); f_out = rp_fold(f_out);
            maxw = rp_dmax(maxw); minl = rp_dmin(minl);
            nw = rp_isum(nw); nl = rp_isum(nl); hw = rp_isum(hw); hl = rp_isum(hl); ht = rp_isum(ht); mc = rp_isum(mc);
            runw = rp_imax(runw); runl = rp_imax(runl);
        }
        // ---- the row (every lane holds every value; lane 0 stages it)
        if (lane == 0) {
            const double NUL = pq_null();
            for (int k = 0; k < PQ_REPORT_COLS; k++) o[k] = 0.0;
            if (bad) {
                for (int k = 0; k < 15; k++) o[k] = NUL;
            } else {
                const double last = row[T - 1], tr_ = (last - c0) / c0;
                const double ann = tr_ > -1.0 ? pow(1.0 + tr_, RP_DAYS / dT) - 1.0 : -1.0;
                const double dof = T > 1 ? (double)(T - 1) : 1.0;
                const double vol = sqrt(Q_r / dof), avol = vol * RP_SQRT252;
                const double dden = sqrt(S_neg / dT) * RP_SQRT252;
                o[0] = last; o[1] = last - c0; o[2] = tr_; o[3] = ann; o[4] = mean; o[5] = maxdd; o[6] = (double)maxrun;
                o[7] = vol; o[8] = avol;
                o[9] = avol > 0.0 ? (ann - RP_RF) / avol : 0.0;
                o[10] = dden > 0.0 ? (ann - RP_RF) / dden : 0.0;
                o[11] = maxdd == 0.0 ? 0.0 : ann / maxdd;
                o[12] = (double)n_pos; o[13] = (double)n_neg; o[14] = (double)n_pos / dT;
            }
            o[15] = cnt >= 0 ? (double)cnt : NUL;
            if (!rec) {
                for (int k = 16; k < 38; k++) o[k] = NUL;
            } else {
                const double dn = (double)cnt, dw = (double)nw, dl = (double)nl;
                const double turnover = s_cost + s_rev, fees = f_in + f_out;
                o[16] = dw; o[17] = dl; o[18] = rp_div(dw, dn);
                o[19] = gp; o[20] = gl; o[21] = rp_div(gp, -gl); o[22] = rp_div(gp, dw); o[23] = rp_div(gl, dl);
                o[24] = nw ? maxw : NUL; o[25] = nl ? minl : NUL;
                o[26] = rp_div((double)hw, dw); o[27] = rp_div((double)hl, dl); o[28] = rp_div((double)ht, dn); o[29] = (double)ht;
                o[30] = (double)runw; o[31] = (double)runl;
                o[32] = turnover; o[33] = fees; o[34] = rp_div(fees, turnover);
                o[35] = rp_div(s_cost, dn); o[36] = cnt ? o[35] / c0 : NUL;
                o[37] = (double)mc;
                o[45] = (double)hw; o[46] = (double)hl; o[47] = s_cost;
            }
            if (!BENCH || bad || bbad) {
                for (int k = 38; k < 45; k++) o[k] = NUL;
            } else {
                const double b0 = bm[0], b1 = bm[T - 1];
                o[38] = b0 > 0.0 ? (b1 - b0) / b0 : 0.0;
                o[39] = o[2] - o[38];
                o[40] = alpha;
                o[41] = Q_b > 0.0 ? Q_c / Q_b : 0.0;
                const double sd = T > 1 ? sqrt(Q_a / (double)(T - 1)) : 0.0;
                o[42] = sd == 0.0 ? NUL : alpha / sd * RP_SQRT252;
                o[43] = (double)n_ahead; o[44] = (double)n_ahead / dT;
            }
        }
    }
    __syncthreads();
    if (s < d.n && lane < PQ_REPORT_COLS) report[s * PQ_REPORT_COLS + lane] = stage[wave][lane];
}

// ---- the portfolio row
enum { RB_GP = 0, RB_GL, RB_TURN, RB_FEES, RB_COST, RB_NSUM };   // the five columns summed in D-10's order: cols 19, 20, 32, 33, 47
struct RpBlock {
    double sum[RB_NSUM];
    double maxw, minl, best, worst;                             // -inf / +inf / -inf / +inf without a candidate
    long long n15, n16, n17, hold, mc, hw, hl, active, runw, runl, ibest, iworst, null15, null16;
};

__global__ __launch_bounds__(RP_BLOCK) void rp_block_kernel(const double *rep, int64_t n, RpBlock *blk) {
    __shared__ double col[RB_NSUM][RP_BLOCK];
    __shared__ RpBlock wv[RP_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = (int64_t)blockIdx.x * RP_BLOCK + tid;
    const bool act = s < n;
    const double *r = rep + (act ? s : 0) * PQ_REPORT_COLS;
    const bool t_ok = act && !pq_isnull(r[16]), c_ok = act && !pq_isnull(r[15]);
    col[RB_GP][tid] = t_ok ? r[19] : 0.0;
    col[RB_GL][tid] = t_ok ? r[20] : 0.0;
    col[RB_TURN][tid] = t_ok ? r[32] : 0.0;
    col[RB_FEES][tid] = t_ok ? r[33] : 0.0;
    col[RB_COST][tid] = t_ok ? r[47] : 0.0;
    RpBlock p{};
    p.n15 = rp_isum(c_ok ? (long long)r[15] : 0);
    p.active = rp_isum(c_ok && r[15] > 0.0);
    p.n16 = rp_isum(t_ok ? (long long)r[16] : 0);
    p.n17 = rp_isum(t_ok ? (long long)r[17] : 0);
    p.hold = rp_isum(t_ok ? (long long)r[29] : 0);
    p.mc = rp_isum(t_ok ? (long long)r[37] : 0);
    p.hw = rp_isum(t_ok ? (long long)r[45] : 0);
    p.hl = rp_isum(t_ok ? (long long)r[46] : 0);
    p.runw = rp_imax(t_ok ? (long long)r[30] : 0);
    p.runl = rp_imax(t_ok ? (long long)r[31] : 0);
    p.null15 = rp_imax(act && !c_ok);
    p.null16 = rp_imax(act && !t_ok);
    p.maxw = rp_dmax(t_ok && !pq_isnull(r[24]) ? r[24] : -rp_inf());
    p.minl = rp_dmin(t_ok && !pq_isnull(r[25]) ? r[25] : rp_inf());
    const bool ranked = act && !pq_isnull(r[2]);
    const double ret = ranked ? r[2] : 0.0;
    p.best = rp_dmax(ranked ? ret : -rp_inf());
    p.worst = rp_dmin(ranked ? ret : rp_inf());
    p.ibest = -rp_imax(ranked && ret == p.best ? -(long long)s : RP_NONE);   // the lowest index among the ties
    p.iworst = -rp_imax(ranked && ret == p.worst ? -(long long)s : RP_NONE);
    if (lane == 0) wv[wave] = p;
    __syncthreads();
    if (tid < RB_NSUM) {                                         // ascending symbol order, eight LDS reads in flight
        double acc = 0.0;
        const int m = n - (int64_t)blockIdx.x * RP_BLOCK < RP_BLOCK ? (int)(n - (int64_t)blockIdx.x * RP_BLOCK) : RP_BLOCK;
        int k = 0;
        for (; k + 8 <= m; k += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = col[tid][k + q];
#pragma unroll
            for (int q = 0; q < 8; q++) acc += v[q];
        }
        for (; k < m; k++) acc += col[tid][k];
        blk[blockIdx.x].sum[tid] = acc;
    }
    if (tid == 64) {                                             // another wave joins the four wave records
        RpBlock a = wv[0];
        for (int w = 1; w < RP_BLOCK / 64; w++) {
            const RpBlock &b = wv[w];
            a.n15 += b.n15; a.n16 += b.n16; a.n17 += b.n17; a.hold += b.hold; a.mc += b.mc; a.hw += b.hw; a.hl += b.hl; a.active += b.active;
            a.runw = b.runw > a.runw ? b.runw : a.runw; a.runl = b.runl > a.runl ? b.runl : a.runl;
            a.null15 |= b.null15; a.null16 |= b.null16;
            a.maxw = b.maxw > a.maxw ? b.maxw : a.maxw; a.minl = b.minl < a.minl ? b.minl : a.minl;
            if (b.best > a.best) { a.best = b.best; a.ibest = b.ibest; }      // waves ascend: a tie keeps the lower index
            if (b.worst < a.worst) { a.worst = b.worst; a.iworst = b.iworst; }
        }
        RpBlock *g = blk + blockIdx.x;
        g->maxw = a.maxw; g->minl = a.minl; g->best = a.best; g->worst = a.worst;
        g->n15 = a.n15; g->n16 = a.n16; g->n17 = a.n17; g->hold = a.hold; g->mc = a.mc; g->hw = a.hw; g->hl = a.hl; g->active = a.active;
        g->runw = a.runw; g->runl = a.runl; g->ibest = a.ibest; g->iworst = a.iworst; g->null15 = a.null15; g->null16 = a.null16;
    }
}

// one wave: lane k < RB_NSUM adds the block sums of column k in ascending order; lane 0 joins the rest and writes the row
__global__ __launch_bounds__(64) void rp_total_kernel(const RpBlock *blk, int64_t nblk, double c0, const double *curve, double *out) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    if (lane < RB_NSUM)
        for (int64_t k = 0; k < nblk; k++) acc += blk[k].sum[lane];
    const double gp = __shfl(acc, RB_GP, 64), gl = __shfl(acc, RB_GL, 64), turnover = __shfl(acc, RB_TURN, 64), fees = __shfl(acc, RB_FEES, 64),
                 cost = __shfl(acc, RB_COST, 64);
    if (lane != 0) return;
    RpBlock a = blk[0];
    for (int64_t k = 1; k < nblk; k++) {
        const RpBlock &b = blk[k];
        a.n15 += b.n15; a.n16 += b.n16; a.n17 += b.n17; a.hold += b.hold; a.mc += b.mc; a.hw += b.hw; a.hl += b.hl; a.active += b.active;
        a.runw = b.runw > a.runw ? b.runw : a.runw; a.runl = b.runl > a.runl ? b.runl : a.runl;
        a.null15 |= b.null15; a.null16 |= b.null16;
        a.maxw = b.maxw > a.maxw ? b.maxw : a.maxw; a.minl = b.minl < a.minl ? b.minl : a.minl;
        if (b.best > a.best) { a.best = b.best; a.ibest = b.ibest; }
        if (b.worst < a.worst) { a.worst = b.worst; a.iworst = b.iworst; }
    }
    const double NUL = pq_null();
    for (int k = 0; k < 15; k++) out[k] = curve[k];
    for (int k = 38; k < 45; k++) out[k] = curve[k];
    out[15] = a.null15 ? NUL : (double)a.n15;
    if (a.null15 || a.null16) {
        for (int k = 16; k < 38; k++) out[k] = NUL;
    } else {
        const double dn = (double)a.n15, dw = (double)a.n16, dl = (double)a.n17;
        out[16] = dw; out[17] = dl; out[18] = rp_div(dw, dn);
        out[19] = gp; out[20] = gl; out[21] = rp_div(gp, -gl); out[22] = rp_div(gp, dw); out[23] = rp_div(gl, dl);
        out[24] = a.n16 ? a.maxw : NUL; out[25] = a.n17 ? a.minl : NUL;
        out[26] = rp_div((double)a.hw, dw); out[27] = rp_div((double)a.hl, dl); out[28] = rp_div((double)a.hold, dn); out[29] = (double)a.hold;
        out[30] = (double)a.runw; out[31] = (double)a.runl;
        out[32] = turnover; out[33] = fees; out[34] = rp_div(fees, turnover);
        out[35] = rp_div(cost, dn); out[36] = a.n15 ? out[35] / c0 : NUL;
        out[37] = (double)a.mc;
    }
    out[45] = a.best == -rp_inf() ? NUL : (double)a.ibest;
    out[46] = a.worst == rp_inf() ? NUL : (double)a.iworst;
    out[47] = (double)a.active;
}

} // namespace

extern "C" {

pq_status pq_backtest_report(pq_ctx *ctx, const pq_batch *b, const double *total_value, double initial_capital, const double *benchmark,
                             const pq_lev_params *params, int32_t max_trades, const int32_t *trade_count, const int32_t *entry_day,
                             const int32_t *exit_day, const double *entry_price, const double *exit_price, const double *quantity,
                             const double *pnl, const int32_t *reason, double *report) {
    PQ_TRY(pq_check(ctx, b));
    const int nrec = (entry_day != nullptr) + (exit_day != nullptr) + (entry_price != nullptr) + (exit_price != nullptr) +
                     (quantity != nullptr) + (pnl != nullptr) + (reason != nullptr);
    PQ_REQUIRE(nrec == 0 || nrec == 7, "pq_backtest_report: pass all seven trade-record arrays or none");
    PQ_REQUIRE(nrec == 0 || trade_count, "pq_backtest_report: trade records need trade_count");
    PQ_REQUIRE(max_trades >= 0, "pq_backtest_report: max_trades < 0");
    PQ_REQUIRE(nrec == 0 || params, "pq_backtest_report: trade records need the engine's params (commission_rate, min_commission)");
    PQ_REQUIRE(initial_capital > 0.0 && initial_capital < (double)INFINITY, "pq_backtest_report: initial_capital must be positive and finite");
    PQ_REQUIRE(b->n_series == 0 || b->len == 0 || (total_value && report), "pq_backtest_report: null pointer");
    if (ctx->rec) { pq_set_error("pq_backtest_report cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_NO_RAGGED(b, "pq_backtest_report (total_value is [n_series][stride])");
    if (b->n_series == 0 || b->len == 0) return PQ_OK;
    RpTrades tr{};
    tr.max_trades = max_trades; tr.count = trade_count; tr.entry_day = entry_day; tr.exit_day = exit_day; tr.reason = reason;
    tr.entry_price = entry_price; tr.exit_price = exit_price; tr.quantity = quantity; tr.pnl = pnl;
    if (params) { tr.rate = params->commission_rate; tr.min_commission = params->min_commission; }
    const Dims d = dims_of(b);
    const dim3 grid((unsigned)((d.n + RP_WAVES - 1) / RP_WAVES)), block(RP_WAVES * 64);
    if (benchmark) hipLaunchKernelGGL(rp_symbol_kernel<true>, grid, block, 0, ctx->stream, total_value, d, initial_capital, benchmark, tr, report);
    else hipLaunchKernelGGL(rp_symbol_kernel<false>, grid, block, 0, ctx->stream, total_value, d, initial_capital, benchmark, tr, report);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

pq_status pq_report_portfolio(pq_ctx *ctx, int64_t n_symbols, const double *report, const double *curve_row, double initial_capital,
                              double *out) {
    PQ_REQUIRE(ctx, "pq_report_portfolio: null context");
    PQ_REQUIRE(n_symbols >= 1, "pq_report_portfolio: n_symbols must be >= 1");
    PQ_REQUIRE(report && curve_row && out, "pq_report_portfolio: null pointer");
    PQ_REQUIRE(initial_capital > 0.0 && initial_capital < (double)INFINITY, "pq_report_portfolio: initial_capital must be positive and finite");
    if (ctx->rec) { pq_set_error("pq_report_portfolio cannot be recorded into a suite"); return PQ_ERR_UNSUPPORTED; }
    PQ_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nblk = (n_symbols + RP_BLOCK - 1) / RP_BLOCK;
    PQ_TRY(pq_ws_reserve(ctx, (size_t)nblk * sizeof(RpBlock)));
    RpBlock *blk = (RpBlock *)ctx->ws;
    hipLaunchKernelGGL(rp_block_kernel, dim3((unsigned)nblk), dim3(RP_BLOCK), 0, ctx->stream, report, n_symbols, blk);
    hipLaunchKernelGGL(rp_total_kernel, dim3(1), dim3(64), 0, ctx->stream, (const RpBlock *)blk, nblk, initial_capital, curve_row, out);
    PQ_HIP_TRY(hipGetLastError());
    return PQ_OK;
}

} // extern "C"
