"""not-gpu: the numpy restatement of decision D-22 (tests/backtest_report_ref.py) against a table worked out by hand, against independent
numpy / plain-Python computations, and on the NULL rules.  No GPU and no library."""
import math

import numpy as np

import backtest_report_ref as R

NAN = float("nan")


def close(got, exp, rel=1e-12):
    return abs(got - exp) <= rel * max(abs(exp), 1e-300)


# ---- the hand table: c0 = 1000, six days, three trades (win, zero, loss), a six-day benchmark; commission 0.001, minimum 2
V = [1000.0, 1100.0, 990.0, 990.0, 1188.0, 1069.2]       # r     = 0, +.1, -.1, 0, +.2, -.1          S(r) = .1, mean = 1/60
B = [100.0, 105.0, 105.0, 94.5, 94.5, 103.95]            # rb    = 0, +.05, 0, -.1, 0, +.1           S(rb) = .05, mean_b = 1/120
#                                                          peak  = 1000, 1100, 1100, 1100, 1188, 1188: under water on days 2, 3 and 5
#                                                          dd    = 0, 0, .1, .1, 0, .1
#                                                          a     = r - rb = 0, .05, -.1, .1, .2, -.2  S(a) = .05, alpha = 1/120
TR = dict(entry_day=[0, 2, 3, 0], exit_day=[2, 3, 5, 0], entry_price=[10.0, 12.0, 12.0, 0.0], exit_price=[12.0, 12.0, 11.0, 0.0],
          quantity=[100.0, 100.0, 200.0, 0.0], pnl=[190.0, 0.0, -210.0, 0.0], reason=[1, 1, 2, 0])
# amounts in: 1000, 1200, 2400 = 4600; out: 1200, 1200, 2200 = 4600; fees in: max(1, 2), max(1.2, 2), 2.4 = 6.4; out: 2, 2, 2.2 = 6.2
ANN = math.pow(1.0692, 42.0) - 1.0                       # 252 / 6 = 42
VOL = math.sqrt(246.0 / 3600.0 / 5.0)                    # 60 (r - mean) = -1, 5, -7, -1, 11, -7: squares 1 + 25 + 49 + 1 + 121 + 49 = 246
DOWN = math.sqrt(0.02 / 6.0) * math.sqrt(252.0)          # min(r, 0)^2 = .01 + .01
SD_A = math.sqrt(1470.0 / 14400.0 / 5.0)                 # 120 (a - alpha) = -1, 5, -13, 11, 23, -25: squares sum to 1470
HAND = {
    "final_value": 1069.2, "total_pnl": 69.2, "total_return": 0.0692, "annualized_return": ANN, "mean_daily_return": 1.0 / 60.0,
    "max_drawdown": 0.1, "max_drawdown_days": 2, "daily_volatility": VOL, "annualized_volatility": VOL * math.sqrt(252.0),
    "sharpe": (ANN - 0.03) / (VOL * math.sqrt(252.0)), "sortino": (ANN - 0.03) / DOWN, "calmar": ANN / 0.1,
    "positive_days": 2, "negative_days": 2, "daily_win_rate": 1.0 / 3.0,
    "total_trades": 3, "winning_trades": 1, "losing_trades": 1, "win_rate": 1.0 / 3.0, "gross_profit": 190.0, "gross_loss": -210.0,
    "profit_factor": 190.0 / 210.0, "avg_win": 190.0, "avg_loss": -210.0, "max_win": 190.0, "max_loss": -210.0,
    "avg_hold_win": 2.0, "avg_hold_loss": 2.0, "avg_hold": 5.0 / 3.0, "total_hold_days": 5,
    "max_consecutive_wins": 1, "max_consecutive_losses": 1,             # the pnl == 0 trade in between is neither
    "turnover": 9200.0, "total_fees": 12.6, "fee_ratio": 12.6 / 9200.0, "avg_trade_amount": 4600.0 / 3.0, "capital_use": 4.6 / 3.0,
    "margin_calls": 1,
    "benchmark_return": 0.0395, "excess_return": 0.0692 - 0.0395, "alpha_daily": 1.0 / 120.0,
    # 60 (r - mean) x 120 (rb - mean_b) = (-1)(-1) + 5 5 + (-7)(-1) + (-1)(-13) + 11 (-1) + (-7) 11 = -42 over 7200;
    # 120 (rb - mean_b) = -1, 5, -1, -13, -1, 11: squares sum to 318 over 14400
    "beta": (-42.0 / 7200.0) / (318.0 / 14400.0),
    "information_ratio": (1.0 / 120.0) / SD_A * math.sqrt(252.0),
    "days_ahead": 3, "ahead_rate": 0.5,                                 # r > rb on days 1, 3 and 4
    "best_symbol_index": 2, "worst_symbol_index": 2, "active_symbols": 4600.0,   # in a symbol row: hold days of winners, of losers, S(q ep)
}
EXACT = {"final_value", "max_drawdown_days", "positive_days", "negative_days", "total_trades", "winning_trades", "losing_trades",
         "gross_profit", "gross_loss", "avg_win", "avg_loss", "max_win", "max_loss", "avg_hold_win", "avg_hold_loss", "total_hold_days",
         "max_consecutive_wins", "max_consecutive_losses", "turnover", "margin_calls", "days_ahead", "ahead_rate", "best_symbol_index",
         "worst_symbol_index", "active_symbols"}


def hand_row():
    return R.report_row(V, 1000.0, B, TR, 3, 4, commission_rate=0.001, min_commission=2.0)


def test_hand_table_every_column():
    row = hand_row()
    assert set(HAND) == set(R.NAMES) and len(R.NAMES) == R.COLS == 48
    for k, name in enumerate(R.NAMES):
        if name in EXACT:
            assert row[k] == HAND[name], (name, row[k], HAND[name])
        else:
            assert close(row[k], HAND[name], 1e-11), (name, row[k], HAND[name])   # decimal inputs: .1 is not a binary fraction


def test_names_match_the_package_table():
    from polars_quant_amd._spec import REPORT_COLS, REPORT_SECTIONS, REPORT_TRADE_FIELDS
    assert tuple(REPORT_COLS) == R.NAMES and tuple(REPORT_TRADE_FIELDS) == R.TRADE_FIELDS
    assert len(REPORT_SECTIONS) == 13 and sorted(c for _, cs in REPORT_SECTIONS for c in cs) == sorted(R.NAMES[:45])


def test_header_declares_the_report():
    import re
    from pathlib import Path
    txt = (Path(__file__).resolve().parent.parent / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define\s+PQ_REPORT_COLS\s+48\b", txt)
    assert re.search(r"pq_status\s+pq_backtest_report\s*\(", txt) and re.search(r"pq_status\s+pq_report_portfolio\s*\(", txt)


def test_sum_order_is_the_partials_then_the_fold():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300) * 10.0 ** rng.integers(-8, 8, 300)
    p = [0.0] * 64
    for i, val in enumerate(x):                                          # ascending i: partial i % 64 takes x[i] in its own order
        p[i % 64] += float(val)
    for s in (32, 16, 8, 4, 2, 1):
        for k in range(s):
            p[k] += p[k + s]
    assert R.S(x) == p[0]
    assert R.S([]) == 0.0 and R.S([-0.0]) == 0.0 and math.copysign(1.0, R.S([-0.0])) == 1.0
    assert R.S([1e16, 1.0] + [0.0] * 62 + [-1e16]) == 1.0               # 1e16 - 1e16 in partial 0, then + 1.0 in the fold


def walks(n, T, seed):
    rng = np.random.default_rng(seed)
    return 1000.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((n, T)), axis=1)), 50.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T)))


def run_loop(flags):
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best


def test_cross_checks_on_random_walks():
    v, b = walks(6, 300, 2)
    rng = np.random.default_rng(3)
    for s in range(6):
        m = 40
        days = np.sort(rng.choice(300, 2 * m, replace=False))
        pnl = np.round(rng.standard_normal(m) * 100.0)
        pnl[rng.random(m) < 0.3] = 0.0
        tr = dict(entry_day=days[0::2], exit_day=days[1::2], entry_price=rng.uniform(3, 30, m), exit_price=rng.uniform(3, 30, m),
                  quantity=100.0 * rng.integers(1, 40, m), pnl=pnl, reason=rng.integers(1, 3, m))
        row = R.report_row(v[s], 1000.0, b, tr, m, m)
        peak = np.maximum.accumulate(np.maximum(v[s], 1000.0))
        r = np.diff(np.concatenate([[1000.0], v[s]])) / np.concatenate([[1000.0], v[s][:-1]])
        rb = np.concatenate([[0.0], np.diff(b) / b[:-1]])
        assert row[5] == np.max((peak - v[s]) / peak)
        assert close(row[7], np.std(r, ddof=1)) and close(row[4], np.mean(r)) and close(row[40], np.mean(r - rb))
        cov = np.cov(r, rb, ddof=1)
        assert close(row[41], cov[0, 1] / cov[1, 1])
        assert close(row[42], np.mean(r - rb) / np.std(r - rb, ddof=1) * math.sqrt(252.0), 1e-10)
        assert row[6] == run_loop(v[s] < peak) and row[30] == run_loop(pnl > 0) and row[31] == run_loop(pnl < 0)
        assert row[12] == np.sum(r > 0) and row[13] == np.sum(r < 0) and row[43] == np.sum(r > rb)
        fees = [max(q * p * 0.0003, 5.0) for q, p in zip(tr["quantity"], tr["entry_price"])]
        fees += [max(q * p * 0.0003, 5.0) for q, p in zip(tr["quantity"], tr["exit_price"])]
        assert close(row[33], math.fsum(fees))
        assert R.S(np.maximum(tr["quantity"] * tr["entry_price"] * 0.0003, 5.0)) + R.S(np.maximum(tr["quantity"] * tr["exit_price"] * 0.0003, 5.0)) == row[33]
        assert all(max(float(q) * float(p) * 0.0003, 5.0) == f for q, p, f in zip(tr["quantity"], tr["entry_price"], fees))
        assert row[29] == int(np.sum(tr["exit_day"] - tr["entry_day"])) and row[37] == np.sum(tr["reason"] == 2)


def test_null_rules():
    nul = lambda a: R.isnull(a)
    row = R.report_row(V, 1000.0, None, {k: np.zeros(4) for k in R.TRADE_FIELDS}, 0, 4)          # no trades, no benchmark
    assert nul(row[[18, 21, 22, 23, 24, 25, 26, 27, 28, 34, 35, 36]]).all() and (row[[15, 16, 17, 19, 20, 29, 30, 31, 32, 33, 37]] == 0).all()
    assert nul(row[R.BENCH]).all() and not nul(row[R.CURVE]).any() and (row[45:] == 0).all()
    win = {**TR, "pnl": [190.0, 5.0, 7.0, 0.0]}
    row = R.report_row(V, 1000.0, B, win, 3, 4)                                                    # winners only
    assert nul(row[[21, 23, 25, 27]]).all() and not nul(row[[18, 22, 24, 26, 28, 34, 35, 36]]).any() and row[30] == 3 and row[31] == 0
    row = R.report_row(V, 1000.0, B, TR, 5, 4)                                                     # trade_count > max_trades
    assert nul(row[R.TRADES]).all() and row[15] == 5 and (row[45:] == 0).all() and not nul(row[R.CURVE]).any()
    row = R.report_row(V, 1000.0, B, None, 3, 4)                                                   # no record arrays
    assert nul(row[R.TRADES]).all() and row[15] == 3
    assert nul(R.report_row(V, 1000.0, B)[15:38]).all()                                            # no trade_count either
    for bad in (NAN, R.NULL, float("inf")):
        v = list(V); v[3] = bad
        row = R.report_row(v, 1000.0, B, TR, 3, 4)
        assert nul(row[R.CURVE]).all() and nul(row[R.BENCH]).all() and row[15] == 3 and row[19] == 190.0
    b = list(B); b[2] = NAN
    row = R.report_row(V, 1000.0, b, TR, 3, 4)
    assert nul(row[R.BENCH]).all() and not nul(row[R.CURVE]).any()
    row = R.report_row([1010.0], 1000.0, [7.0])                                                    # T = 1
    assert close(row[2], 0.01) and close(row[3], 1.01 ** 252 - 1.0) and row[7] == 0.0 and row[9] == 0.0 and row[6] == 0 and row[5] == 0.0
    assert row[38] == 0.0 and row[41] == 0.0 and nul(row[42]) and row[43] == 1 and row[44] == 1.0
    row = R.report_row([0.0, 5.0], 1000.0)                                                         # a base of 0: that day's return is 0
    assert row[2] == -0.995 and row[12] == 0 and row[13] == 1 and row[4] == -0.5
    row = R.report_row([5.0, 0.0], 1000.0)                                                         # total return -1
    assert row[2] == -1.0 and row[3] == -1.0 and row[13] == 2 and row[5] == 1.0
    row = R.report_row([1000.0] * 5, 1000.0, [3.0] * 5)                                            # flat against constant
    assert row[41] == 0.0 and nul(row[42]) and row[9] == 0.0 and row[10] == 0.0 and row[11] == 0.0


def test_portfolio_row_by_hand():
    rep = np.zeros((3, 48))
    # total return: a tie for the best between symbols 0 and 2; symbol 1 has a NULL curve
    rep[:, 2] = [0.25, R.NULL, 0.25]
    rep[1, 0:15] = R.NULL
    #            n   win lose            gp     gl                       maxw  minl  hold          streaks      turn   fees          mc
    rep[0, 15:38] = [4, 3, 1, 0.75, 300.0, -50.0, 6.0, 100.0, -50.0, 150.0, -50.0, 2.0, 4.0, 2.5, 10, 3, 1, 8000.0, 16.0, 0.002, 1000.0, 1.0, 1]
    rep[1, 15:38] = [0, 0, 0, R.NULL, 0.0, 0.0, R.NULL, R.NULL, R.NULL, R.NULL, R.NULL, R.NULL, R.NULL, R.NULL, 0, 0, 0, 0.0, 0.0, R.NULL, R.NULL, R.NULL, 0]
    rep[2, 15:38] = [2, 0, 2, 0.0, 0.0, -30.0, 0.0, R.NULL, -15.0, R.NULL, -20.0, R.NULL, 3.0, 3.0, 6, 0, 2, 2000.0, 8.0, 0.004, 500.0, 0.5, 0]
    rep[:, 45], rep[:, 46], rep[:, 47] = [6, 0, 0], [4, 0, 6], [4000.0, 0.0, 1000.0]
    curve = np.arange(100.0, 148.0)
    row = R.portfolio_row(rep, curve, 1000.0)
    assert (row[0:15] == curve[0:15]).all() and (row[38:45] == curve[38:45]).all()
    exp = {15: 6, 16: 3, 17: 3, 18: 0.5, 19: 300.0, 20: -80.0, 21: 3.75, 22: 100.0, 23: -80.0 / 3.0, 24: 150.0, 25: -50.0,
           26: 2.0, 27: 10.0 / 3.0, 28: 16.0 / 6.0, 29: 16, 30: 3, 31: 2, 32: 10000.0, 33: 24.0, 34: 0.0024, 35: 5000.0 / 6.0,
           36: 5000.0 / 6.0 / 1000.0, 37: 1, 45: 0, 46: 0, 47: 2}
    for k, e in exp.items():
        assert row[k] == e, (R.NAMES[k], row[k], e)
    rep[2, 16:38] = R.NULL                                               # symbol 2's records were cut short
    rep[2, 45:] = 0.0
    row = R.portfolio_row(rep, curve, 1000.0)
    assert R.isnull(row[16:38]).all() and row[15] == 6 and row[47] == 2 and row[45] == 0
    rep[[0, 2], 2] = [0.1, 0.3]
    row = R.portfolio_row(rep, curve, 1000.0)
    assert row[45] == 2 and row[46] == 0
    x = np.arange(1.0, 601.0) * 0.1                                      # D-10's order: blocks of 256, then the block sums
    blocks = [sum(x[lo:lo + 256].tolist(), 0.0) for lo in (0, 256, 512)]
    assert R.block_sum(x) == sum(blocks, 0.0)
