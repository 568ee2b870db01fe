"""ParameterSweep -- a grid of strategy parameters backtested in one launch (decision D-25 in DESIGN.md).

`Strategy` + `api.backtest_vectorized` backtest ONE parameter set per call: two [N, T] signal columns written and read back, and every
moving average recomputed for every pair it takes part in.  A sweep computes every distinct indicator column ("line") once with the
existing indicator call and hands the lines and a table of parameter sets -- rule 0: cross(lines[a], lines[b]), rule 1:
band(lines[a], k0, k1), the rules of `Strategy.ma` / `.macd` / `.rsi` -- to pq_backtest_sweep, whose lanes are the parameter sets.  The
result is the [P, N, 8] summary (SUMMARY_KEYS order) and nothing else: no signal or equity column exists.

The grid builders (ma_grid, macd_grid, rsi_grid) are pure host code; like strategy.py this module holds no arithmetic of its own.
"""
from __future__ import annotations

import numpy as np

from . import api as _api
from ._spec import BT_DEFAULTS, SUMMARY_KEYS
from .strategy import _MA

RULE_CROSS, RULE_BAND = 0, 1


def _ints(xs, what):
    out = [int(x) for x in np.atleast_1d(np.asarray(xs)).tolist()]
    if not out or any(x != y for x, y in zip(out, np.atleast_1d(np.asarray(xs)).tolist())):
        raise ValueError(f"{what} must be a non-empty list of integers")
    return out


def ma_grid(fast_periods, slow_periods):
    """-> (periods, rules, params): the distinct periods (ascending: line j is MA(periods[j])), the SWEEP_PARAM_DTYPE table and the
    {"fast", "slow"} columns of the P pairs with fast < slow, fast-major in the order given"""
    fasts, slows = _ints(fast_periods, "fast_periods"), _ints(slow_periods, "slow_periods")
    pairs = [(f, s) for f in dict.fromkeys(fasts) for s in dict.fromkeys(slows) if f < s]
    periods = sorted({p for pair in pairs for p in pair})
    line = {p: j for j, p in enumerate(periods)}
    rules = np.zeros(len(pairs), dtype=_api.SWEEP_PARAM_DTYPE)
    rules["rule"] = RULE_CROSS
    rules["a"] = [line[f] for f, _ in pairs]
    rules["b"] = [line[s] for _, s in pairs]
    params = {"fast": np.array([f for f, _ in pairs], dtype=np.int64), "slow": np.array([s for _, s in pairs], dtype=np.int64)}
    return periods, rules, params


def macd_grid(fast_periods, slow_periods, signal_periods):
    """-> (triples, rules, params): the P = #{(fast, slow): fast < slow} x #signal triples (fast, slow, signal), fast-major; set i
    crosses lines 2 i (the MACD line) and 2 i + 1 (its signal line)"""
    fasts, slows, sigs = (_ints(x, w) for x, w in ((fast_periods, "fast_periods"), (slow_periods, "slow_periods"),
                                                    (signal_periods, "signal_periods")))
    triples = [(f, s, g) for f in dict.fromkeys(fasts) for s in dict.fromkeys(slows) if f < s for g in dict.fromkeys(sigs)]
    rules = np.zeros(len(triples), dtype=_api.SWEEP_PARAM_DTYPE)
    rules["rule"] = RULE_CROSS
    rules["a"] = 2 * np.arange(len(triples))
    rules["b"] = 2 * np.arange(len(triples)) + 1
    params = {k: np.array([t[j] for t in triples], dtype=np.int64) for j, k in enumerate(("fast", "slow", "signal"))}
    return triples, rules, params


def rsi_grid(periods, oversold, overbought):
    """-> (periods, rules, params): one line per distinct period (in the order given); the P = #periods x #oversold x #overbought sets,
    period-major, then oversold, then overbought"""
    ps = list(dict.fromkeys(_ints(periods, "periods")))
    lo = [float(x) for x in np.atleast_1d(np.asarray(oversold, dtype=np.float64))]
    hi = [float(x) for x in np.atleast_1d(np.asarray(overbought, dtype=np.float64))]
    sets = [(j, p, l, h) for j, p in enumerate(ps) for l in lo for h in hi]
    rules = np.zeros(len(sets), dtype=_api.SWEEP_PARAM_DTYPE)
    rules["rule"] = RULE_BAND
    rules["a"] = [s[0] for s in sets]
    rules["b"] = rules["a"]
    rules["k0"] = [s[2] for s in sets]
    rules["k1"] = [s[3] for s in sets]
    params = {"period": np.array([s[1] for s in sets], dtype=np.int64), "oversold": np.array([s[2] for s in sets]),
              "overbought": np.array([s[3] for s in sets])}
    return ps, rules, params


class SweepResult:
    """params: dict of [P] arrays (one entry per parameter set); summary: device [P, N, 8] in SUMMARY_KEYS order"""

    def __init__(self, params, summary):
        self.params = params
        self.summary = summary

    def metric(self, name):
        """-> [P, N] view of one summary column"""
        if name not in SUMMARY_KEYS:
            raise KeyError(f"metric must be one of {SUMMARY_KEYS}")
        return self.summary[..., SUMMARY_KEYS.index(name)]

    def best(self, metric="sharpe_ratio", maximize=True):
        """per symbol the parameter set with the largest (smallest) metric -> (index [N] int64, value [N]); a NaN ranks last, and a
        symbol whose every cell is NaN gets index 0 and a NaN value"""
        import torch
        m = self.metric(metric)
        if m.shape[0] == 0:
            raise ValueError("best() of an empty grid")
        worst = float("-inf") if maximize else float("inf")
        key = torch.where(torch.isnan(m), torch.full_like(m, worst), m)
        idx = key.argmax(dim=0) if maximize else key.argmin(dim=0)
        idx = torch.where(torch.isnan(m).all(dim=0), torch.zeros_like(idx), idx)
        return idx, m.gather(0, idx.unsqueeze(0))[0]


class ParameterSweep:
    def __init__(self, df, benchmark=None, **costs):
        """df: the dict / frame of [N, T] columns `Strategy` takes; benchmark: None, [T] or [N, T]; costs: VectorizedBacktester's
        (initial_capital, buy_slippage, sell_slippage, buy_commission_rate, sell_commission_rate, min_commission, position_size)"""
        unknown = set(costs) - set(BT_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown cost parameters {sorted(unknown)}; known: {sorted(BT_DEFAULTS)}")
        self.df, self.benchmark, self.costs = df, benchmark, costs

    def run(self, lines, rules, params=None, price_col="close"):
        """caller-built lines (a list of [N, T] columns or one [L, N, T] array) and rules (api.sweep_params) -> SweepResult"""
        tab = _api.sweep_params(rules)
        if params is None:
            params = {k: tab[k].copy() for k in ("rule", "a", "b", "k0", "k1")}
        summ = _api.backtest_sweep(self.df[price_col], lines, tab, benchmark=self.benchmark, **self.costs)
        return SweepResult(params, summ)

    def ma(self, fast_periods, slow_periods, ma_type="sma", price_col="close"):
        """the grid of `Strategy.ma` crosses: every pair with fast < slow; each distinct period is computed once"""
        if ma_type not in _MA:
            raise ValueError(f"ma_type must be one of {sorted(_MA)}")
        periods, rules, params = ma_grid(fast_periods, slow_periods)
        x = self.df[price_col]
        lines = [_api.call(_MA[ma_type], x, timeperiod=p)[0] for p in periods]
        return self.run(lines, rules, params, price_col)

    def macd(self, fast_periods, slow_periods, signal_periods, price_col="close"):
        """the grid of `Strategy.macd` crosses: two lines (MACD, signal) per parameter set"""
        triples, rules, params = macd_grid(fast_periods, slow_periods, signal_periods)
        x = self.df[price_col]
        lines = []
        for f, s, g in triples:
            m, sg, _h = _api.call("macd", x, fastperiod=f, slowperiod=s, signalperiod=g)
            lines += [m, sg]
        return self.run(lines, rules, params, price_col)

    def rsi(self, periods, oversold, overbought, price_col="close"):
        """the grid of `Strategy.rsi` bands: one line per period, period x oversold x overbought parameter sets"""
        ps, rules, params = rsi_grid(periods, oversold, overbought)
        x = self.df[price_col]
        lines = [_api.call("rsi", x, timeperiod=p)[0] for p in ps]
        return self.run(lines, rules, params, price_col)
