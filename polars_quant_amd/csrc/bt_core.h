// bt_core.h -- the backtest arithmetic that every engine shares, written once: one row of the pool (vectorized.rs:141-177), the running
// part of calculate_summary (metrics.rs:26-49), its second pass over a stored equity row and the closing of its eight values
// (metrics.rs:52-149).  The lane forms (ops_backtest.h), the wave forms (ops_backtest_wave.h), the sweep (sweep/sweep.hip) and the
// sequential tape (seq/sequential.hip) differ in how rows reach a lane and in how partial sums are combined, never in these lines.
// Every line keeps the reference's rounding order (-ffp-contract=off).  Counters stay with the caller, typed as the caller needs them.
#pragma once
#include "pq_dev.h"

// the daily return of metrics.rs:40-44 (and of the benchmark, :91-98)
__device__ __forceinline__ double bt_ret(double prev, double v) { return (prev > 0.0) ? (v - prev) / prev : 0.0; }

struct BtPool { // vectorized.rs:124-129
    double pos, avail, entry_cost;
    __device__ __forceinline__ void reset(double capital) { pos = 0.0; avail = capital; entry_cost = 0.0; }
    __device__ __forceinline__ double equity(double px) const { return avail + pos * px; } // :177, and :142 on an untouched row
};
// vectorized.rs:146-161 on a valid price with the pool flat; true: a position was opened (a pool that cannot afford a share stays as it is)
__device__ __forceinline__ bool bt_buy(BtPool &pl, double px, const pq_bt_params &prm) {
    const double exec = px + prm.buy_slippage;
    const double cur_eq = pl.avail + pl.pos * px;
    const double deploy = cur_eq * prm.position_size;
    const double qty = floor(deploy / exec);
    if (!(qty > 0.0)) return false;
    const double cost = qty * exec;
    const double fee = fmax(cost * prm.buy_commission_rate, prm.min_commission);
    pl.pos += qty;
    pl.avail -= cost + fee;
    pl.entry_cost = pl.pos * px;
    return true;
}
// vectorized.rs:162-175 on a valid price with the pool long; true: the round trip was a win
__device__ __forceinline__ bool bt_sell(BtPool &pl, double px, const pq_bt_params &prm) {
    const double exec = px - prm.sell_slippage;
    const double revenue = pl.pos * exec;
    const double fee = fmax(revenue * prm.sell_commission_rate, prm.min_commission);
    const double net = revenue - fee;
    const bool win = net > pl.entry_cost;
    pl.avail += net;
    pl.pos = 0.0;
    return win;
}

struct BtRun { // calculate_summary's first pass (metrics.rs:21-49)
    double max_eq, max_dd, prev_eq, ret_sum;
    __device__ __forceinline__ void reset(double capital) { max_eq = capital; max_dd = 0.0; prev_eq = capital; ret_sum = 0.0; }
    __device__ __forceinline__ double add(double eq) { // the row's daily return
        if (eq > max_eq) max_eq = eq;
        const double dd = (max_eq > 0.0) ? (max_eq - eq) / max_eq : 0.0;
        if (dd > max_dd) max_dd = dd;
        const double r = bt_ret(prev_eq, eq);
        ret_sum += r;
        prev_eq = eq;
        return r;
    }
};

__device__ __forceinline__ void bt_summary_zero(double *sm) { // metrics.rs:17-19: no rows
#pragma unroll
    for (int k = 0; k < PQ_SUMMARY_COLS; k++) sm[k] = 0.0;
}

// metrics.rs:52-149 once the sums are known: T rows (> 0), vs / bvs / cvs the squared deviations of the daily returns, of the benchmark's
// and their products, b0 / b1 the benchmark's first and last row (read only where has_bench).
template <class I>
__device__ __forceinline__ void bt_summary_close(double T, double capital, double last_eq, double max_dd, double vs, double bvs, double cvs,
                                                 I trades, I wins, bool has_bench, double b0, double b1, double *sm) {
    const double DAYS = 252.0, RF = 0.03;
    const double total_return = (last_eq - capital) / capital;                                 // :52
    const double ann = (total_return > -1.0) ? pow(1.0 + total_return, DAYS / T) - 1.0 : -1.0; // :54-58
    const double dof = fmax(T - 1.0, 1.0);                                                     // :61
    const double var = vs / dof;
    const double vol = sqrt(var) * sqrt(DAYS);                                                 // :69
    const double sharpe = (vol > 0.0) ? (ann - RF) / vol : 0.0;                                // :71-75
    const double win_rate = (trades > 0) ? (double)wins / (double)trades : 0.0;
    double alpha = 0.0, beta = 0.0;
    if (has_bench) {                                                                           // :86-140
        const double bvar = bvs / dof, cov = cvs / dof;
        if (bvar > 0.0) beta = cov / bvar;
        const double btr = bt_ret(b0, b1);
        const double bann = (btr > -1.0) ? pow(1.0 + btr, DAYS / T) - 1.0 : -1.0;
        alpha = ann - (RF + beta * (bann - RF));
    }
    sm[0] = ann; sm[1] = max_dd; sm[2] = alpha; sm[3] = beta; sm[4] = sharpe;
    sm[5] = fmax(total_return, 0.0); sm[6] = win_rate; sm[7] = (double)trades;                 // :142-149
}

// The serial second pass and the close, for a lane that has its T equity rows in memory (`eqr`) and the first pass behind it; `bm`: the
// lane's benchmark rows or nullptr.  Every sum runs left to right over the rows, as the reference's does.
template <class I>
__device__ __forceinline__ void bt_summary_finish(const double *eqr, const double *bm, int64_t T, double capital, const BtRun &run, I trades,
                                                  I wins, double *sm) {
    if (T == 0) { bt_summary_zero(sm); return; }
    const double mean = run.ret_sum / (double)T;
    double vs = 0.0, bvs = 0.0, cvs = 0.0, pe = capital;
    for (int64_t i = 0; i < T; i++) { // metrics.rs:63-67
        const double e = eqr[i];
        const double dlt = bt_ret(pe, e) - mean;
        vs += dlt * dlt;
        pe = e;
    }
    if (bm) { // metrics.rs:86-116: the benchmark's mean return, its variance, the covariance
        double pb = bm[0], bs = 0.0;
        for (int64_t i = 0; i < T; i++) { const double bv = bm[i]; bs += bt_ret(pb, bv); pb = bv; }
        const double bmean = bs / (double)T;
        pb = bm[0];
        for (int64_t i = 0; i < T; i++) {
            const double bv = bm[i];
            const double dlt = bt_ret(pb, bv) - bmean;
            bvs += dlt * dlt;
            pb = bv;
        }
        pb = bm[0]; pe = capital;
        for (int64_t i = 0; i < T; i++) {
            const double bv = bm[i], e = eqr[i];
            const double br = bt_ret(pb, bv), r = bt_ret(pe, e);
            cvs += (r - mean) * (br - bmean);
            pb = bv; pe = e;
        }
    }
    bt_summary_close((double)T, capital, run.prev_eq, run.max_dd, vs, bvs, cvs, trades, wins, bm != nullptr, bm ? bm[0] : 0.0,
                     bm ? bm[T - 1] : 0.0, sm);
}
