"""ParameterSweep -- a grid of strategy parameters backtested in one launch (decision D-25 in DESIGN.md).

`Strategy` + `api.backtest_vectorized` backtest ONE parameter set per call: two [N, T] signal columns written and read back, and every
moving average recomputed for every pair it takes part in.  A sweep computes every distinct indicator column ("line") once with the
existing indicator call and hands the lines and a table of parameter sets -- rule 0: cross(lines[a], lines[b]), rule 1:
band(lines[a], k0, k1), the rules of `Strategy.ma` / `.macd` / `.rsi` -- to pq_backtest_sweep, whose lanes are the parameter sets.  The
result is the [P, N, 8] summary (SUMMARY_KEYS order) and nothing else: no signal or equity column exists.

`bband`, `stoch`, `cci`, `adx`, `breakout`, `reversion` and `grid` go through pq_backtest_sweep_rules, whose table has a third column
index c (-1: the price) and the rules 2 channel, 3 breakout, 4 channel around a scaled base line, 5 cross in zones, 6 cross with
strength (include/pq_hip.h).  Not covered: `ma`'s trend / slope / distance filters, `volume`, `gap`, `pattern`, `trend`.

Walk-forward analysis (decision D-26): every method takes `windows`, an integer [W, 2] array of row ranges [t0, t1).  The lines are
still computed once over the full history -- a window of a causal indicator is a warmed-up indicator -- and pq_backtest_sweep_windows
backtests every window in the same launch: summary[w] is [P, N, 8] and bit for bit the sweep of the rows [t0, t1) alone (flat and
fully in cash at t0, row t0 never signals).  `walk_forward_windows` lays out rolling or anchored train / test folds,
`ParameterSweep.walk_forward` runs one sweep launch over the 2 F windows and one pq_sweep_select launch, which picks per fold and symbol
the best set of the train window and reads that set's result in the test window -> `WalkForwardResult`.

The grid builders (ma_grid, macd_grid, rsi_grid, bband_grid, ...) and walk_forward_windows are pure host code; like strategy.py this
module holds no arithmetic of its own.
"""
from __future__ import annotations

import numpy as np

from . import api as _api
from ._spec import BT_DEFAULTS, SUMMARY_KEYS
from .strategy import _MA

RULE_CROSS, RULE_BAND = 0, 1
RULE_CHANNEL, RULE_BREAKOUT, RULE_SCALED_CHANNEL, RULE_CROSS_ZONES, RULE_CROSS_STRENGTH = 2, 3, 4, 5, 6
PRICE = -1   # column c of a rule: the price column itself


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


def _floats(xs):
    return [float(x) for x in np.atleast_1d(np.asarray(xs, dtype=np.float64))]


def _rule_table(rule, a, b=None, c=None, k0=None, k1=None):
    tab = np.zeros(len(a), dtype=_api.SWEEP_RULE_DTYPE)
    tab["rule"] = rule
    tab["a"] = a
    tab["b"] = a if b is None else b
    tab["c"] = PRICE if c is None else c
    if k0 is not None:
        tab["k0"] = k0
    if k1 is not None:
        tab["k1"] = k1
    return tab


def _band_grid(periods, lower, upper):
    """one line per distinct period (in the order given), period x lower x upper sets -> (periods, SWEEP_RULE_DTYPE table, the sets)"""
    ps = list(dict.fromkeys(_ints(periods, "periods")))
    sets = [(j, p, l, h) for j, p in enumerate(ps) for l in lower for h in upper]
    tab = _rule_table(RULE_BAND, [s[0] for s in sets], c=0, k0=[s[2] for s in sets], k1=[s[3] for s in sets])
    return ps, tab, sets


def bband_grid(periods, nbdevs):
    """-> (pairs, rules, params): the P = #periods x #nbdevs pairs (period, nbdev), period-major; set i owns lines 2 i (the lower band)
    and 2 i + 1 (the upper band) of bbands(x, period, nbdev, nbdev) and trades the price against them (rule 2, c = -1)"""
    pairs = [(p, d) for p in dict.fromkeys(_ints(periods, "periods")) for d in dict.fromkeys(_floats(nbdevs))]
    i = np.arange(len(pairs))
    rules = _rule_table(RULE_CHANNEL, 2 * i, 2 * i + 1)
    params = {"period": np.array([p for p, _ in pairs], dtype=np.int64), "nbdev": np.array([d for _, d in pairs], dtype=np.float64)}
    return pairs, rules, params


def stoch_grid(fastk_periods, slowk_periods, slowd_periods, oversold, overbought):
    """-> (triples, rules, params): the distinct (fastk, slowk, slowd) triples -- triple j owns lines 2 j (%K) and 2 j + 1 (%D) -- and the
    P = #triples x #oversold x #overbought sets, fastk outermost: %K crossing %D, gated by the zones of %K (rule 5, c = a)"""
    fk, sk, sd = (list(dict.fromkeys(_ints(x, w))) for x, w in ((fastk_periods, "fastk_periods"), (slowk_periods, "slowk_periods"),
                                                                 (slowd_periods, "slowd_periods")))
    triples = [(f, k, d) for f in fk for k in sk for d in sd]
    sets = [(j, t, l, h) for j, t in enumerate(triples) for l in _floats(oversold) for h in _floats(overbought)]
    k = np.array([2 * s[0] for s in sets], dtype=np.int64)
    rules = _rule_table(RULE_CROSS_ZONES, k, k + 1, k, [s[2] for s in sets], [s[3] for s in sets])
    params = {name: np.array([s[1][j] for s in sets], dtype=np.int64) for j, name in enumerate(("fastk_period", "slowk_period", "slowd_period"))}
    params["oversold"], params["overbought"] = np.array([s[2] for s in sets]), np.array([s[3] for s in sets])
    return triples, rules, params


def cci_grid(periods, oversold, overbought):
    """-> (periods, rules, params): like rsi_grid, one CCI line per distinct period"""
    ps, rules, sets = _band_grid(periods, _floats(oversold), _floats(overbought))
    params = {"period": np.array([s[1] for s in sets], dtype=np.int64), "oversold": np.array([s[2] for s in sets]),
              "overbought": np.array([s[3] for s in sets])}
    return ps, rules, params


def adx_grid(periods, thresholds):
    """-> (periods, rules, params): period j owns lines 3 j (plus_dm), 3 j + 1 (minus_dm) and 3 j + 2 (adx); the P = #periods x
    #thresholds sets, period-major: plus_dm crossing minus_dm while adx > threshold (rule 6)"""
    ps = list(dict.fromkeys(_ints(periods, "periods")))
    sets = [(j, p, th) for j, p in enumerate(ps) for th in _floats(thresholds)]
    k = np.array([3 * s[0] for s in sets], dtype=np.int64)
    rules = _rule_table(RULE_CROSS_STRENGTH, k, k + 1, k + 2, [s[2] for s in sets])
    params = {"period": np.array([s[1] for s in sets], dtype=np.int64), "threshold": np.array([s[2] for s in sets])}
    return ps, rules, params


def breakout_grid(periods, close_is_price=True):
    """-> (periods, rules, params): period j owns lines 2 j (rolling_min(low)) and 2 j + 1 (rolling_max(high)); the close breaks out of
    the previous row's channel (rule 3).  The close is the price column (c = -1) or, with close_is_price=False, one more line after
    the channels"""
    ps = list(dict.fromkeys(_ints(periods, "periods")))
    j = np.arange(len(ps))
    rules = _rule_table(RULE_BREAKOUT, 2 * j, 2 * j + 1, PRICE if close_is_price else 2 * len(ps))
    return ps, rules, {"period": np.array(ps, dtype=np.int64)}


def reversion_grid(periods, thresholds):
    """-> (periods, rules, params): one z-score line per distinct period; the P = #periods x #thresholds sets, period-major, are the
    band (-threshold, +threshold)"""
    ths = _floats(thresholds)
    ps = list(dict.fromkeys(_ints(periods, "periods")))
    sets = [(j, p, th) for j, p in enumerate(ps) for th in ths]
    rules = _rule_table(RULE_BAND, [s[0] for s in sets], c=0, k0=[-s[2] for s in sets], k1=[s[2] for s in sets])
    params = {"period": np.array([s[1] for s in sets], dtype=np.int64), "threshold": np.array([s[2] for s in sets])}
    return ps, rules, params


def grid_grid(base_periods, grid_pcts):
    """-> (periods, rules, params): one SMA base line per distinct period; the P = #periods x #grid_pcts sets, period-major, trade the
    price against base x (1 - pct %) and base x (1 + pct %) (rule 4, c = -1); the factors are `Strategy.grid`'s expressions"""
    ps = list(dict.fromkeys(_ints(base_periods, "base_periods")))
    sets = [(j, p, pct) for j, p in enumerate(ps) for pct in _floats(grid_pcts)]
    rules = _rule_table(RULE_SCALED_CHANNEL, [s[0] for s in sets], k0=[1.0 - s[2] / 100.0 for s in sets], k1=[1.0 + s[2] / 100.0 for s in sets])
    params = {"base_period": np.array([s[1] for s in sets], dtype=np.int64), "grid_pct": np.array([s[2] for s in sets])}
    return ps, rules, params


def _fits(n_lines, what):
    if n_lines > _api.SWEEP_MAX_LINES:
        raise ValueError(f"{what}: the grid needs {n_lines} lines, a sweep takes {_api.SWEEP_MAX_LINES} at the most")


def walk_forward_windows(n_rows, train, test, step=None, anchored=False):
    """-> int64 [F, 2, 2]: fold k trains on the rows [k step, k step + train) -- anchored: [0, k step + train) -- and tests on the `test`
    rows after them; [k, 0] is the train range [t0, t1), [k, 1] the test range.  step defaults to `test` (the test windows tile the
    rows); only folds whose test window is complete are kept"""
    step = test if step is None else step
    n_rows, train, test, step = (int(x) for x in (n_rows, train, test, step))
    if train < 1 or test < 1 or step < 1:
        raise ValueError(f"train, test and step must be positive, not {train}, {test}, {step}")
    folds = []
    k = 0
    while k * step + train + test <= n_rows:
        t = k * step + train
        folds.append(((0 if anchored else k * step, t), (t, t + test)))
        k += 1
    if not folds:
        raise ValueError(f"{n_rows} rows hold no fold of {train} train and {test} test rows")
    return np.array(folds, dtype=np.int64)


class SweepResult:
    """params: dict of [P] arrays (one entry per parameter set); summary: device [P, N, 8] in SUMMARY_KEYS order -- of a windowed sweep
    [W, P, N, 8], with `windows` the int64 [W, 2] row ranges (None otherwise)"""

    def __init__(self, params, summary, windows=None):
        self.params = params
        self.summary = summary
        self.windows = windows

    def metric(self, name):
        """-> [P, N] ([W, P, N]) view of one summary column"""
        if name not in SUMMARY_KEYS:
            raise KeyError(f"metric must be one of {SUMMARY_KEYS}")
        return self.summary[..., SUMMARY_KEYS.index(name)]

    def best(self, metric="sharpe_ratio", maximize=True):
        """per symbol (and window) the parameter set with the largest (smallest) metric -> (index [N] int64, value [N]), of a windowed
        sweep both [W, N]; a NaN ranks last, and a symbol whose every cell is NaN gets index 0 and a NaN value"""
        import torch
        m = self.metric(metric)
        ax = m.dim() - 2                # the parameter axis of [P, N] or [W, P, N]
        if m.shape[ax] == 0:
            raise ValueError("best() of an empty grid")
        worst = float("-inf") if maximize else float("inf")
        key = torch.where(torch.isnan(m), torch.full_like(m, worst), m)
        idx = key.argmax(dim=ax) if maximize else key.argmin(dim=ax)
        idx = torch.where(torch.isnan(m).all(dim=ax), torch.zeros_like(idx), idx)
        return idx, m.gather(ax, idx.unsqueeze(ax)).squeeze(ax)


class WalkForwardResult:
    """params: dict of [P] arrays; folds: int64 [F, 2, 2] (walk_forward_windows); summary: device [2 F, P, N, 8], window 2 k the train
    and 2 k + 1 the test range of fold k; chosen: device [F, N] int32, per fold and symbol the best set of the train window;
    in_sample / out_of_sample: device [F, N, 8], that set's summary in the train / test window"""

    def __init__(self, params, folds, summary, chosen, in_sample, out_of_sample):
        self.params, self.folds, self.summary = params, folds, summary
        self.chosen, self.in_sample, self.out_of_sample = chosen, in_sample, out_of_sample

    def metric(self, name, which="out"):
        """-> [F, N] view of one column of the out-of-sample (which="out") or in-sample (which="in") summary"""
        if name not in SUMMARY_KEYS:
            raise KeyError(f"metric must be one of {SUMMARY_KEYS}")
        if which not in ("in", "out"):
            raise ValueError("which must be 'in' or 'out'")
        return (self.out_of_sample if which == "out" else self.in_sample)[..., SUMMARY_KEYS.index(name)]

    def chosen_params(self):
        """-> dict of [F, N] host arrays: the parameters of the chosen sets"""
        idx = self.chosen.cpu().numpy()
        return {k: np.asarray(v)[idx] for k, v in self.params.items()}


class ParameterSweep:
    def __init__(self, df, benchmark=None, **costs):
        """df: the dict / frame of [N, T] columns `Strategy` takes; benchmark: None, [T] or [N, T]; costs: VectorizedBacktester's
        (initial_capital, buy_slippage, sell_slippage, buy_commission_rate, sell_commission_rate, min_commission, position_size)"""
        unknown = set(costs) - set(BT_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown cost parameters {sorted(unknown)}; known: {sorted(BT_DEFAULTS)}")
        self.df, self.benchmark, self.costs = df, benchmark, costs

    def run(self, lines, rules, params=None, price_col="close", windows=None):
        """caller-built lines (a list of [N, T] columns or one [L, N, T] array) and rules (api.sweep_params) -> SweepResult; windows:
        an integer [W, 2] array of row ranges [t0, t1), each backtested on its own in the same launch (every method takes it)"""
        tab = _api.sweep_params(rules)
        if params is None:
            params = {k: tab[k].copy() for k in ("rule", "a", "b", "k0", "k1")}
        win = None if windows is None else _api.sweep_windows(windows)
        summ = _api.backtest_sweep(self.df[price_col], lines, tab, benchmark=self.benchmark, windows=win, **self.costs)
        return SweepResult(params, summ, win)

    def ma(self, fast_periods, slow_periods, ma_type="sma", price_col="close", windows=None):
        """the grid of `Strategy.ma` crosses: every pair with fast < slow; each distinct period is computed once"""
        if ma_type not in _MA:
            raise ValueError(f"ma_type must be one of {sorted(_MA)}")
        periods, rules, params = ma_grid(fast_periods, slow_periods)
        x = self.df[price_col]
        lines = [_api.call(_MA[ma_type], x, timeperiod=p)[0] for p in periods]
        return self.run(lines, rules, params, price_col, windows)

    def macd(self, fast_periods, slow_periods, signal_periods, price_col="close", windows=None):
        """the grid of `Strategy.macd` crosses: two lines (MACD, signal) per parameter set"""
        triples, rules, params = macd_grid(fast_periods, slow_periods, signal_periods)
        x = self.df[price_col]
        lines = []
        for f, s, g in triples:
            m, sg, _h = _api.call("macd", x, fastperiod=f, slowperiod=s, signalperiod=g)
            lines += [m, sg]
        return self.run(lines, rules, params, price_col, windows)

    def rsi(self, periods, oversold, overbought, price_col="close", windows=None):
        """the grid of `Strategy.rsi` bands: one line per period, period x oversold x overbought parameter sets"""
        ps, rules, params = rsi_grid(periods, oversold, overbought)
        x = self.df[price_col]
        lines = [_api.call("rsi", x, timeperiod=p)[0] for p in ps]
        return self.run(lines, rules, params, price_col, windows)

    # ---- the rules with a third column (pq_backtest_sweep_rules) ---------------------------------------------------------------------
    def run_rules(self, lines, rules, params=None, price_col="close", windows=None):
        """caller-built lines and rules (api.sweep_rules: rule / a / b / c / k0 / k1, c = -1 for the price) -> SweepResult"""
        tab = _api.sweep_rules(rules)
        if params is None:
            params = {k: tab[k].copy() for k in tab.dtype.names}
        win = None if windows is None else _api.sweep_windows(windows)
        summ = _api.backtest_sweep_rules(self.df[price_col], lines, tab, benchmark=self.benchmark, windows=win, **self.costs)
        return SweepResult(params, summ, win)

    def bband(self, periods, nbdevs, price_col="close", windows=None):
        """the grid of `Strategy.bband`: the price against the Bollinger bands of every (period, nbdev)"""
        pairs, rules, params = bband_grid(periods, nbdevs)
        _fits(2 * len(pairs), "bband")
        x = self.df[price_col]
        lines = []
        for p, d in pairs:
            up, _mid, lo = _api.call("bbands", x, timeperiod=p, nbdevup=d, nbdevdn=d)
            lines += [lo, up]
        return self.run_rules(lines, rules, params, price_col, windows)

    def stoch(self, fastk_periods, slowk_periods, slowd_periods, oversold, overbought, price_col="close", windows=None):
        """the grid of `Strategy.stoch`: %K and %D once per period triple, every (oversold, overbought) zone pair on them"""
        triples, rules, params = stoch_grid(fastk_periods, slowk_periods, slowd_periods, oversold, overbought)
        _fits(2 * len(triples), "stoch")
        lines = []
        for f, k, d in triples:
            lines += list(_api.call("stoch", self.df["high"], self.df["low"], self.df["close"], fastk_period=f, slowk_period=k, slowd_period=d))
        return self.run_rules(lines, rules, params, price_col, windows)

    def cci(self, periods, oversold, overbought, price_col="close", windows=None):
        """the grid of `Strategy.cci` bands: one line per period"""
        ps, rules, params = cci_grid(periods, oversold, overbought)
        _fits(len(ps), "cci")
        lines = [_api.call("cci", self.df["high"], self.df["low"], self.df["close"], timeperiod=p)[0] for p in ps]
        return self.run_rules(lines, rules, params, price_col, windows)

    def adx(self, periods, thresholds, price_col="close", windows=None):
        """the grid of `Strategy.adx`: plus_dm, minus_dm and adx once per period, every threshold on them"""
        ps, rules, params = adx_grid(periods, thresholds)
        _fits(3 * len(ps), "adx")
        h, l, c = self.df["high"], self.df["low"], self.df["close"]
        lines = []
        for p in ps:
            lines += [_api.call("plus_dm", h, l, timeperiod=p)[0], _api.call("minus_dm", h, l, timeperiod=p)[0],
                      _api.call("adx", h, l, c, timeperiod=p)[0]]
        return self.run_rules(lines, rules, params, price_col, windows)

    def breakout(self, periods, price_col="close", windows=None):
        """the grid of `Strategy.breakout`: the Donchian channel of every period; the signal is taken on the close whatever the price
        column of the backtest is"""
        close_is_price = price_col == "close"
        ps, rules, params = breakout_grid(periods, close_is_price)
        _fits(2 * len(ps) + (0 if close_is_price else 1), "breakout")
        lines = []
        for p in ps:
            lines += [_api.call("rolling_min", self.df["low"], window=p)[0], _api.call("rolling_max", self.df["high"], window=p)[0]]
        if not close_is_price:
            lines.append(self.df["close"])
        return self.run_rules(lines, rules, params, price_col, windows)

    def reversion(self, periods, thresholds, price_col="close", windows=None):
        """the grid of `Strategy.reversion`: one z-score line per period, every threshold on it"""
        ps, rules, params = reversion_grid(periods, thresholds)
        _fits(len(ps), "reversion")
        x = self.df[price_col]
        lines = []
        for p in ps:
            up, mid, _lo = _api.call("bbands", x, timeperiod=p, nbdevup=1.0, nbdevdn=1.0)
            lines.append(_api.zscore(x, up, mid))
        return self.run_rules(lines, rules, params, price_col, windows)

    def grid(self, base_periods, grid_pcts, price_col="close", windows=None):
        """the grid of `Strategy.grid`: one SMA base line per period, every percentage around it"""
        ps, rules, params = grid_grid(base_periods, grid_pcts)
        _fits(len(ps), "grid")
        x = self.df[price_col]
        lines = [_api.call("sma", x, timeperiod=p)[0] for p in ps]
        return self.run_rules(lines, rules, params, price_col, windows)

    # ---- walk-forward analysis (D-26) -------------------------------------------------------------------------------------------------
    _RULES = ("run", "run_rules", "ma", "macd", "rsi", "bband", "stoch", "cci", "adx", "breakout", "reversion", "grid")

    def walk_forward(self, rule, *grid_args, train, test, step=None, anchored=False, metric="sharpe_ratio", maximize=True, **grid_kwargs):
        """rule: the name of a method above ("ma", "stoch", ...), grid_args / grid_kwargs: its arguments.  Lays out the folds of
        walk_forward_windows over the rows of the price column, sweeps the grid over all 2 F train and test windows in one launch and,
        in a second one, picks per fold and symbol the set with the best `metric` in the train window -> WalkForwardResult"""
        if rule not in self._RULES:
            raise ValueError(f"rule must be one of {self._RULES}")
        if metric not in SUMMARY_KEYS:
            raise KeyError(f"metric must be one of {SUMMARY_KEYS}")
        if "windows" in grid_kwargs:
            raise TypeError("walk_forward lays out its own windows")
        n_rows = _api._shape(self.df[grid_kwargs.get("price_col", "close")])[-1]
        folds = walk_forward_windows(n_rows, train, test, step, anchored)
        F = len(folds)
        res = getattr(self, rule)(*grid_args, windows=folds.reshape(2 * F, 2), **grid_kwargs)
        chosen, ins, outs = _api.sweep_select(res.summary, 2 * np.arange(F), 2 * np.arange(F) + 1, metric, maximize)
        return WalkForwardResult(res.params, folds, res.summary, chosen, ins, outs)
