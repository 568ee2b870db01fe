"""Decision D-22 restated in numpy: the statistics report of `Backtest`, one row of 48 f64 per symbol, and the
portfolio row.  Written from the decision's text, not from the kernel; imports nothing from oracle/.

Sums S(x) run in the decision's one order: 64 partials -- partial k starts at +0.0 and adds x[k], x[k + 64], ... ascending -- folded
p[k] += p[k + s] (k < s) for s = 32, 16, 8, 4, 2, 1; the result is p[0].  A sum "over winners" runs over the trade index with +0.0 in
the place of every other trade."""
import numpy as np

NULL_BITS = np.uint64(0x7FF80000504E554C)
NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]
COLS = 48
SQRT252 = float(np.sqrt(252.0))
RF = 0.03
NAMES = ("final_value", "total_pnl", "total_return", "annualized_return", "mean_daily_return", "max_drawdown", "max_drawdown_days",
         "daily_volatility", "annualized_volatility", "sharpe", "sortino", "calmar", "positive_days", "negative_days", "daily_win_rate",
         "total_trades", "winning_trades", "losing_trades", "win_rate", "gross_profit", "gross_loss", "profit_factor", "avg_win",
         "avg_loss", "max_win", "max_loss", "avg_hold_win", "avg_hold_loss", "avg_hold", "total_hold_days", "max_consecutive_wins",
         "max_consecutive_losses", "turnover", "total_fees", "fee_ratio", "avg_trade_amount", "capital_use", "margin_calls",
         "benchmark_return", "excess_return", "alpha_daily", "beta", "information_ratio", "days_ahead", "ahead_rate",
         "best_symbol_index", "worst_symbol_index", "active_symbols")
C = {k: i for i, k in enumerate(NAMES)}
CURVE, TRADES, BENCH = slice(0, 15), slice(16, 38), slice(38, 45)
TRADE_FIELDS = ("entry_day", "exit_day", "entry_price", "exit_price", "quantity", "pnl", "reason")


def isnull(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64) == NULL_BITS


def S(x):
    """the decision's sum of a 1-D series"""
    x = np.asarray(x, dtype=np.float64)
    p = np.zeros(64)
    for k in range(64):
        acc = np.float64(0.0)
        for val in x[k::64]:
            acc = acc + val
        p[k] = acc
    for s in (32, 16, 8, 4, 2, 1):
        p[:s] = p[:s] + p[s:2 * s]
    return float(p[0])


def longest_run(flags):
    """longest run of consecutive True: a max-scan of the index of the last False at or before each entry"""
    flags = np.asarray(flags, dtype=bool)
    if flags.size == 0:
        return 0
    idx = np.arange(flags.size)
    last = np.maximum.accumulate(np.where(flags, -1, idx))
    return int(np.max(np.where(flags, idx - last, 0)))


def div(a, b):
    return NULL if b == 0 else a / b


def returns(v, first_base):
    """r[i] = (v[i] - v[i-1]) / v[i-1], the base of r[0] being first_base; 0.0 where the base is <= 0"""
    base = np.concatenate([[first_base], v[:-1]])
    with np.errstate(all="ignore"):
        return np.where(base > 0.0, (v - base) / base, 0.0)


def report_row(v, c0, bench=None, trades=None, trade_count=None, max_trades=0, commission_rate=0.0003, min_commission=5.0, ann=None):
    """one symbol.  trades: {field: 1-D arrays of max_trades entries} or None; `ann` replaces column 3 in the three ratios that follow
    it (the device's own pow)"""
    v = np.asarray(v, dtype=np.float64)
    T = v.size
    o = np.zeros(COLS)
    ok = bool(np.isfinite(v).all())
    r = mean = None
    if not ok:
        o[CURVE] = NULL
    else:
        r = returns(v, c0)
        peak, m = np.empty(T), c0
        for i in range(T):
            m = v[i] if v[i] > m else m
            peak[i] = m
        tr = (v[-1] - c0) / c0
        a3 = float(np.float64(1.0 + tr) ** np.float64(252.0 / T)) - 1.0 if tr > -1.0 else -1.0
        mean = S(r) / T
        dv = r - mean
        vol = float(np.sqrt(S(dv * dv) / max(T - 1, 1)))
        avol = vol * SQRT252
        dden = float(np.sqrt(S(np.where(r < 0.0, r * r, 0.0)) / T)) * SQRT252
        maxdd = float(np.max((peak - v) / peak))
        o[0], o[1], o[2], o[3], o[4], o[5] = v[-1], v[-1] - c0, tr, a3, mean, maxdd
        o[6] = longest_run(v < peak)
        o[7], o[8] = vol, avol
        a = a3 if ann is None else ann
        o[9] = (a - RF) / avol if avol > 0.0 else 0.0
        o[10] = (a - RF) / dden if dden > 0.0 else 0.0
        o[11] = 0.0 if maxdd == 0.0 else a / maxdd
        o[12], o[13] = np.sum(r > 0.0), np.sum(r < 0.0)
        o[14] = o[12] / T
    # ---- trades
    if trade_count is None:
        o[15] = NULL
        o[TRADES] = NULL
    else:
        cnt = int(trade_count)
        o[15] = cnt
        if trades is None or cnt > max_trades:
            o[TRADES] = NULL
        else:
            f = {k: np.asarray(trades[k])[:cnt] for k in TRADE_FIELDS}
            pnl, q, ep, xp = (f[k].astype(np.float64) for k in ("pnl", "quantity", "entry_price", "exit_price"))
            hold = f["exit_day"].astype(np.int64) - f["entry_day"].astype(np.int64)
            win, los = pnl > 0.0, pnl < 0.0
            nw, nl = int(win.sum()), int(los.sum())
            gp, gl = S(np.where(win, pnl, 0.0)), S(np.where(los, pnl, 0.0))
            hw, hl, ht = int(hold[win].sum()), int(hold[los].sum()), int(hold.sum())
            cost, rev = q * ep, q * xp
            s_cost = S(cost)
            turnover = s_cost + S(rev)
            fees = S(np.maximum(cost * commission_rate, min_commission)) + S(np.maximum(rev * commission_rate, min_commission))
            o[16], o[17], o[18] = nw, nl, div(float(nw), float(cnt))
            o[19], o[20], o[21], o[22], o[23] = gp, gl, div(gp, -gl), div(gp, float(nw)), div(gl, float(nl))
            o[24] = pnl[win].max() if nw else NULL
            o[25] = pnl[los].min() if nl else NULL
            o[26], o[27], o[28], o[29] = div(float(hw), float(nw)), div(float(hl), float(nl)), div(float(ht), float(cnt)), ht
            o[30], o[31] = longest_run(win), longest_run(los)
            o[32], o[33], o[34] = turnover, fees, div(fees, turnover)
            o[35] = div(s_cost, float(cnt))
            o[36] = o[35] / c0 if cnt else NULL
            o[37] = int((f["reason"] == 2).sum())
            o[45], o[46], o[47] = hw, hl, s_cost
    # ---- benchmark
    b = None if bench is None else np.asarray(bench, dtype=np.float64)
    if b is None or not ok or not np.isfinite(b).all():
        o[BENCH] = NULL
    else:
        rb = returns(b, b[0])
        rb[0] = 0.0
        al = r - rb
        alpha, mean_b = S(al) / T, S(rb) / T
        db = rb - mean_b
        varb = S(db * db)
        o[38] = (b[-1] - b[0]) / b[0] if b[0] > 0.0 else 0.0
        o[39] = o[2] - o[38]
        o[40] = alpha
        o[41] = S((r - mean) * db) / varb if varb > 0.0 else 0.0
        da = al - alpha
        sd = float(np.sqrt(S(da * da) / (T - 1))) if T > 1 else 0.0
        o[42] = NULL if sd == 0.0 else alpha / sd * SQRT252
        o[43] = np.sum(r > rb)
        o[44] = o[43] / T
    return o


def report(v, c0, bench=None, trades=None, trade_count=None, max_trades=0, commission_rate=0.0003, min_commission=5.0, ann=None):
    """[N, T] -> [N, 48]; trades {field: [N, max_trades]}, trade_count [N], ann [N] or None"""
    v = np.asarray(v, dtype=np.float64)
    return np.stack([report_row(v[s], c0, bench, None if trades is None else {k: np.asarray(trades[k])[s] for k in TRADE_FIELDS},
                                None if trade_count is None else trade_count[s], max_trades, commission_rate, min_commission,
                                None if ann is None else float(ann[s])) for s in range(v.shape[0])])


def block_sum(x):
    """D-10's order: blocks of 256 symbols, ascending inside a block, block sums in ascending order, both from +0.0"""
    total = np.float64(0.0)
    for lo in range(0, len(x), 256):
        bs = np.float64(0.0)
        for val in x[lo:lo + 256]:
            bs = bs + val
        total = total + bs
    return float(total)


def portfolio_row(rep, curve_row, c0):
    """rep [N, 48], curve_row [48] = report_row of the portfolio_value series on c0 * N, c0 = one symbol's capital"""
    rep = np.asarray(rep, dtype=np.float64)
    o = np.zeros(COLS)
    o[CURVE], o[BENCH] = curve_row[CURVE], curve_row[BENCH]
    no_count, no_trades = isnull(rep[:, 15]).any(), isnull(rep[:, 16]).any()
    o[15] = NULL if no_count else rep[:, 15].sum()
    if no_count or no_trades:
        o[TRADES] = NULL
    else:
        isum = lambda c: float(int(rep[:, c].astype(np.int64).sum()))
        cnt, nw, nl, ht, hw, hl = (isum(c) for c in (15, 16, 17, 29, 45, 46))
        gp, gl, turnover, fees, s_cost = (block_sum(rep[:, c]) for c in (19, 20, 32, 33, 47))
        o[16], o[17], o[18] = nw, nl, div(nw, cnt)
        o[19], o[20], o[21], o[22], o[23] = gp, gl, div(gp, -gl), div(gp, nw), div(gl, nl)
        wins, losses = rep[:, 24][~isnull(rep[:, 24])], rep[:, 25][~isnull(rep[:, 25])]
        o[24] = wins.max() if wins.size else NULL
        o[25] = losses.min() if losses.size else NULL
        o[26], o[27], o[28], o[29] = div(hw, nw), div(hl, nl), div(ht, cnt), ht
        o[30], o[31] = rep[:, 30].max(), rep[:, 31].max()
        o[32], o[33], o[34] = turnover, fees, div(fees, turnover)
        o[35] = div(s_cost, cnt)
        o[36] = o[35] / c0 if cnt else NULL
        o[37] = isum(37)
    ranked = np.flatnonzero(~isnull(rep[:, 2]))
    if ranked.size:
        ret = rep[ranked, 2]
        o[45] = ranked[np.flatnonzero(ret == ret.max())[0]]      # ties: the lowest index
        o[46] = ranked[np.flatnonzero(ret == ret.min())[0]]
    else:
        o[45] = o[46] = NULL
    o[47] = int((rep[:, 15] > 0).sum())                         # a NULL count is no trade
    return o
