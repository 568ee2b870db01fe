"""Test-side scalar restatement of the sweep kernel's algorithm (csrc/sweep/sweep.hip, decision D-25) for ONE (symbol, parameter set):
the rule on the two line values of rows t - 1 and t, the scan of vectorized.rs:124-194 on the signal of the row, and calculate_summary
(metrics.rs:7-152) as two streaming walks -- walk 1: sum of returns, peak, drawdown, trades, wins; walk 2: the same state machine again
for the squared deviations and the covariance, in the same left-to-right order.  It holds no signal and no equity array.

Independent of the HIP kernels and of the C oracle; plain Python floats are IEEE doubles and never contracted.
"""
from __future__ import annotations

import math

NAN = float("nan")
DEFAULTS = dict(initial_capital=100000.0, buy_slippage=0.0, sell_slippage=0.0, buy_commission_rate=0.0003,
                sell_commission_rate=0.0003, min_commission=5.0, position_size=1.0)   # vectorized.rs:38
DAYS, RF = 252.0, 0.03


class _Lane:
    def __init__(self, c):
        self.pa = self.pb = NAN          # row 0 never signals: a NaN compares false
        self.pos, self.avail, self.entry_cost, self.prev_eq = 0.0, c["initial_capital"], 0.0, c["initial_capital"]
        self.trades = self.wins = 0

    def step(self, c, rule, k0, k1, xa, xb, px):
        """one row: the rule, then the scan -> (equity of the row, its return against the previous row)"""
        if rule == 1:   # band (oracle/backtest.c:271-278); a NULL is a NaN
            buy, sell = self.pa < k0 and xa >= k0, self.pa > k1 and xa <= k1
        else:           # cross (oracle/backtest.c:263-270)
            buy, sell = self.pa <= self.pb and xa > xb, self.pa >= self.pb and xa < xb
        self.pa, self.pb = xa, xb
        if px > 0.0:    # a NaN (a NULL is one) or non-positive price leaves the state untouched (:141-144)
            if buy and self.pos == 0.0:
                ex = px + c["buy_slippage"]
                qty = float(math.floor((self.avail + self.pos * px) * c["position_size"] / ex))
                if qty > 0.0:
                    cost = qty * ex
                    fee = max(cost * c["buy_commission_rate"], c["min_commission"])
                    self.pos += qty
                    self.avail -= cost + fee
                    self.entry_cost = self.pos * px
                    self.trades += 1
            elif sell and self.pos > 0.0:
                revenue = self.pos * (px - c["sell_slippage"])
                net = revenue - max(revenue * c["sell_commission_rate"], c["min_commission"])
                if net > self.entry_cost:
                    self.wins += 1
                self.avail += net
                self.pos = 0.0
        eq = self.avail + self.pos * px
        r = (eq - self.prev_eq) / self.prev_eq if self.prev_eq > 0.0 else 0.0
        self.prev_eq = eq
        return eq, r


def _bench_ret(bench, t):
    pb = bench[t - 1] if t > 0 else bench[0]
    return (bench[t] - pb) / pb if pb > 0.0 else 0.0


def sweep_cell(price, line_a, line_b, rule, k0=0.0, k1=0.0, bench=None, **costs):
    """price, line_a, line_b (and bench): sequences of T floats -> the 8 summary values (SUMMARY_KEYS order) as a list"""
    c = {**DEFAULTS, **costs}
    T = len(price)
    if T == 0:
        return [0.0] * 8
    price, line_a, line_b = [float(x) for x in price], [float(x) for x in line_a], [float(x) for x in line_b]
    bench = None if bench is None else [float(x) for x in bench]
    cap = c["initial_capital"]
    # walk 1
    st = _Lane(c)
    max_eq, max_dd, ret_sum, bsum = cap, 0.0, 0.0, 0.0
    for t in range(T):
        eq, r = st.step(c, rule, k0, k1, line_a[t], line_b[t], price[t])
        if eq > max_eq:
            max_eq = eq
        dd = (max_eq - eq) / max_eq if max_eq > 0.0 else 0.0
        if dd > max_dd:
            max_dd = dd
        ret_sum += r
        if bench is not None:
            bsum += _bench_ret(bench, t)
    last_eq, trades, wins = st.prev_eq, st.trades, st.wins
    mean, bmean = ret_sum / T, bsum / T
    # walk 2: the same deterministic state machine again
    st = _Lane(c)
    vs = bv = cv = 0.0
    for t in range(T):
        _eq, r = st.step(c, rule, k0, k1, line_a[t], line_b[t], price[t])
        d = r - mean
        vs += d * d
        if bench is not None:
            db = _bench_ret(bench, t) - bmean
            bv += db * db
            cv += d * db
    total_return = (last_eq - cap) / cap
    ann = math.pow(1.0 + total_return, DAYS / T) - 1.0 if total_return > -1.0 else -1.0
    dof = max(T - 1.0, 1.0)
    vol = math.sqrt(vs / dof) * math.sqrt(DAYS) if vs == vs else NAN
    sharpe = (ann - RF) / vol if vol > 0.0 else 0.0
    win_rate = wins / trades if trades > 0 else 0.0
    alpha = beta = 0.0
    if bench is not None:
        bvar, cov = bv / dof, cv / dof
        if bvar > 0.0:
            beta = cov / bvar
        btr = (bench[T - 1] - bench[0]) / bench[0] if bench[0] > 0.0 else 0.0
        bann = math.pow(1.0 + btr, DAYS / T) - 1.0 if btr > -1.0 else -1.0
        alpha = ann - (RF + beta * (bann - RF))
    return [ann, max_dd, alpha, beta, sharpe, max(total_return, 0.0) if total_return == total_return else NAN, win_rate, float(trades)]
