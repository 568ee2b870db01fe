"""Factor -- both halves of the README's `Factor` class.  The general factor calculations ratio / diff / weighted / normalize / rank
(README.md:1416-1421, :1438-1470; decision D-20) build the [N, T] factor columns; the evaluation half consumes
them (README.md:1429-1430, :1480-1482, :1626-1634): per-day cross-sectional IC, Rank-IC and their rolling mean / information ratio
(decision D-12, oracle/backtest.c), and quantile sorts, long-short legs, turnover, coverage and IC statistics (decision D-15), and the
regressions and significance tests ic_test / factor_return / fama_macbeth / time_series_regression (decision D-17), and the robustness
tests ic_decay / subsample_test / subgroup_test (decision D-18), and the multi-factor orthogonalization / neutralization Factor().clean
(decision D-19).  The common technical factors moving_average / momentum / volatility / skewness / relative_strength
(README.md:1423-1426, :1472-1477; decision D-21) roll along the days of every symbol, and so do the two-column ones rolling_regression /
rolling_beta / idiosyncratic_volatility (decision D-28: rolling-window OLS).  The time-series operators of factor construction ts_sum /
ts_std / ts_zscore / ts_min / ts_max / ts_argmin / ts_argmax / ts_rank / decay_linear / delay / delta / ts_cov / ts_corr (decision
D-29, beyond the README) are the windowed operators that formulaic alphas are written in.  README-only in the reference.  Inputs are [N, T] arrays (symbol-major, like every other column of this package): the
factor and the forward return of every symbol on every day.
`clean` is the README's factor cleaning step that comes before the evaluation (decision D-16).
`portfolio_backtest` (decision D-27, beyond the README) holds the groups of the sorts as portfolios: rebalance days, weights, drift and
a fee on the traded value, as value curves with the backtest report's statistics; it takes the factor and the PRICE of every symbol.
`combine` (decision D-30, beyond the README) is the step between the two: K tested factors into the one score that `portfolio_backtest`
takes, by equal, trailing-IC, trailing-ICIR or max-IR weights that only use ICs already known on the day the weight is used.
`double_sort` (decision D-31, beyond the README) is the two-way sort that follows a factor's single sort: a control (size, another
factor) times the factor, independent or dependent, with the cells' returns and the bucket-averaged spread along each axis.
`risk_model` and `portfolio_risk` (decision D-33, beyond the README) consume the three series of `pure_factor_return` (decision D-32):
the exponentially weighted covariance of the factor and industry returns and the specific variance of every symbol on the rebalance
days, and from the two the predicted variance of a portfolio with its exposures and each factor's contribution.
`optimal_portfolio` (decision D-34, beyond the README) is the step after them: the minimum-variance, tangency or mean-variance weights
under that model on every rebalance day, from Sigma^-1 v through the factor structure (Sigma itself is never built).
`weights_backtest` (decision D-35, beyond the README) holds such weights -- signed, the remainder in cash -- between the rebalance days:
the value curve with turnover and costs, and the drifted daily holdings that `portfolio_risk` reads.
"""
from __future__ import annotations

import torch

from . import api as _api

IC_METHODS = {"pearson": 0, "spearman": 1}


def _stack_factor_returns(d):
    """pure_factor_return's dict -> (its factor_return rows stacked with industry_return (or intercept) into the [K + G, T] block, its
    specific_return or None): the one stacking of risk_model and return_attribution"""
    rest = d["industry_return"] if "industry_return" in d else d["intercept"]
    fr, rest = (_api._to_device(x)[0] for x in (d["factor_return"], rest))
    return torch.cat([fr, rest.to(fr.device)]), d.get("specific_return")


class Factor:
    def __init__(self):
        # Factor().clean (D-19) is bound per instance, the way the README calls it (`factor = Factor(); factor.clean(df, ...)`).  The
        # class itself carries no `clean` attribute: the package's public-surface contract keeps `Factor.clean` off the class so that it
        # is never taken for the module-level single-factor `clean` (D-16).
        self.clean = self._clean_factors

    # ---- D-20: the general factor calculations (README.md:1416-1421, :1438-1470); every result is a device f64 [N, T] column
    def ratio(self, a, b):
        """-> a / b; NULL where either is NULL, otherwise plain IEEE-754 (a zero divisor gives inf or nan)"""
        return _api.factor_binary(a, b, _api.BINARY_OPS["ratio"])

    def diff(self, a, b, normalize=False):
        """-> a - b, or (a - b) / |b| with normalize=True; NULL where either is NULL"""
        return _api.factor_binary(a, b, _api.BINARY_OPS["reldiff" if normalize else "diff"])

    def weighted(self, factor, weight, group=None):
        """-> (factor * weight) / W per day, W the sum of the weights over the symbols whose factor and weight are both non-null and
        finite; with group (integer codes [N] or [N, T], negative = unclassified, at most 256 groups) W is the sum over the symbol's
        group on that day.  NULL outside the sample and where W == 0"""
        return _api.factor_weighted(factor, weight, group)

    def normalize(self, factor, method="zscore"):
        """per day over the non-null finite symbols: "zscore" (x - mean) / sample std (clean(factor, standardize=True) itself),
        "minmax" (x - min) / (max - min) (the day NULL where max == min), "quantile" (average rank - 0.5) / n, in (0, 1)"""
        return _api.factor_normalize(factor, method)

    def rank(self, factor, ascending=True, pct=False):
        """per day over the non-null finite symbols: the average rank in 1 .. n (ties share the mean of their positions; -0 ties with
        +0), ascending=False: n + 1 - rank, pct=True: divided by n; NULL outside the day's sample"""
        return _api.factor_rank(factor, _api.RANK_MODES["pct" if pct else "rank"], not ascending)

    # ---- D-21: the common technical factors (README.md:1423-1426, :1472-1477), along the days of every symbol; a row without its full
    # sample is NULL, so is a result that comes out NaN; 1 <= window <= 1024
    def moving_average(self, factor, window=20):
        """-> the mean of the last `window` days, NULL unless all of them are non-null and finite"""
        return _api.factor_rolling(factor, _api.ROLLING_OPS["mean"], window)

    def momentum(self, factor, window=20, skip=0):
        """-> (a - b) / b with a = x[t - skip], b = x[t - skip - window] (skip=21, window=231: the usual "12-1" form); NULL unless both
        are non-null and finite; returns(x, period=window) itself at skip=0, a zero base gives inf"""
        return _api.factor_rolling(factor, _api.ROLLING_OPS["momentum"], window, skip)

    def volatility(self, factor, window=20):
        """-> the sample std (ddof 1) of the last `window` period-1 simple returns (window >= 2, not annualised); NULL unless the
        window + 1 prices are non-null and finite and every return is finite; 0.0 over a constant stretch"""
        return _api.factor_rolling(factor, _api.ROLLING_OPS["volatility"], window)

    def skewness(self, factor, window=20):
        """-> the population skewness m3 / m2^1.5 (scipy.stats.skew(bias=True)) of the last `window` period-1 simple returns
        (window >= 3), on volatility's sample; NULL where m2 == 0 (a constant stretch)"""
        return _api.factor_rolling(factor, _api.ROLLING_OPS["skewness"], window)

    def relative_strength(self, factor, window=14):
        """-> 100 G / (G + L) over the last `window` day-to-day differences, G the sum of the rises and L of the falls (the
        simple-average form, no warm-up memory); NULL unless the window + 1 values are non-null and finite, and where G + L == 0"""
        return _api.factor_rolling(factor, _api.ROLLING_OPS["relative_strength"], window)

    # ---- D-28: rolling-window OLS of the returns on K regressors (1 <= K <= 4, each [N, T] or a [T] series shared by every symbol, e.g.
    # the market return), one fit per (symbol, day) over the last `window` days; a row is NULL unless every value of its window is
    # non-null and finite, and where the window is singular; K + 2 <= window <= 1024
    def rolling_regression(self, returns, factors, window=60):
        """-> {"beta": [K, N, T], "alpha", "resid_std", "r_squared", "resid": [N, T]}: the slopes, the intercept, the residual std
        sqrt(sse / (window - K - 1)), R^2 (NULL where the returns are constant over the window) and the residual of the window's last
        day"""
        return _api.factor_rolling_regress(returns, factors, window)

    def rolling_beta(self, returns, market, window=60):
        """-> [N, T]: the slope of the rolling OLS of the returns on one regressor, [N, T] or a [T] market series"""
        return _api.factor_rolling_regress(returns, [market], window, outputs=("beta",))["beta"][0]

    def idiosyncratic_volatility(self, returns, factors, window=60):
        """-> [N, T]: the residual std of the rolling OLS of the returns on the factors (not annualised)"""
        return _api.factor_rolling_regress(returns, factors, window, outputs=("resid_std",))["resid_std"]

    # ---- D-29: the time-series operators of factor construction, along the days of every symbol over the last `window` days (oldest to
    # newest); a row is NULL unless every value of its window is non-null and finite, so is a result that comes out NaN;
    # 1 <= window <= 1024; every result is a device f64 [N, T] column, so -rank(ts_corr(open, volume, 10)) never leaves the device
    def ts_sum(self, x, window):
        """-> the sum of the last `window` days (moving_average times the window, before its division)"""
        return _api.factor_ts(x, _api.TS_OPS["sum"], window)

    def ts_std(self, x, window):
        """-> the sample std (ddof 1) of the last `window` days (window >= 2); on period-1 returns this is volatility"""
        return _api.factor_ts(x, _api.TS_OPS["std"], window)

    def ts_zscore(self, x, window):
        """-> (today's value - the window's mean) / ts_std (window >= 2); NULL over a constant stretch"""
        return _api.factor_ts(x, _api.TS_OPS["zscore"], window)

    def ts_min(self, x, window):
        """-> the smallest value of the last `window` days"""
        return _api.factor_ts(x, _api.TS_OPS["min"], window)

    def ts_max(self, x, window):
        """-> the largest value of the last `window` days"""
        return _api.factor_ts(x, _api.TS_OPS["max"], window)

    def ts_argmin(self, x, window):
        """-> where the window's minimum lies: the 0-based offset from the window's OLDEST day, 0 .. window - 1, as f64 (numpy.argmin
        of the window; ties go to the oldest day, -0 ties with +0)"""
        return _api.factor_ts(x, _api.TS_OPS["argmin"], window)

    def ts_argmax(self, x, window):
        """-> where the window's maximum lies: the 0-based offset from the window's OLDEST day, 0 .. window - 1, as f64 (numpy.argmax
        of the window; ties go to the oldest day); window - 1 - ts_argmax is "days since the high" """
        return _api.factor_ts(x, _api.TS_OPS["argmax"], window)

    def ts_rank(self, x, window, pct=False):
        """-> the average rank of today's value among the last `window` days, 1 .. window (ties share the mean of their positions:
        pandas rolling(window).rank(method="average")), pct=True: divided by the window"""
        return _api.factor_ts(x, _api.TS_OPS["rank"], window, 1 if pct else 0)

    def decay_linear(self, x, window):
        """-> the linearly weighted mean of the last `window` days, weights 1 (oldest) .. window (today) over window (window + 1) / 2"""
        return _api.factor_ts(x, _api.TS_OPS["decay_linear"], window)

    def delay(self, x, periods=1):
        """-> x[t - periods], NULL for t < periods and where that value is NULL or NaN (+-inf passes); 1 <= periods <= 1024"""
        return _api.factor_ts(x, _api.TS_OPS["delay"], periods)

    def delta(self, x, periods=1):
        """-> x[t] - x[t - periods], NULL unless both are non-null and finite; 1 <= periods <= 1024"""
        return _api.factor_ts(x, _api.TS_OPS["delta"], periods)

    def ts_cov(self, x, y, window):
        """-> the sample covariance (ddof 1) of x and y over the last `window` days (window >= 2); NULL unless both columns are
        non-null and finite on every day of the window"""
        return _api.factor_ts_pair(x, y, _api.TS_PAIR_OPS["cov"], window)

    def ts_corr(self, x, y, window):
        """-> the Pearson correlation of x and y over the last `window` days (window >= 2), on ts_cov's sample; NULL where either
        column is constant over the window"""
        return _api.factor_ts_pair(x, y, _api.TS_PAIR_OPS["corr"], window)

    def ic(self, factor, next_return):
        """-> (ic [T], n_valid [T]): Pearson correlation across symbols, per day"""
        return _api.factor_ic(factor, next_return, 0)

    def rank_ic(self, factor, next_return):
        """-> (rank_ic [T], n_valid [T]): Spearman correlation (average ranks) across symbols, per day"""
        return _api.factor_ic(factor, next_return, 1)

    def rolling_ic(self, factor, next_return, window=60, rank=False):
        """-> {"rolling_ic": [T], "rolling_ir": [T]} of the (rank) IC series"""
        ic, _ = _api.factor_ic(factor, next_return, 1 if rank else 0)
        m, ir = _api.rolling_ic(ic, window)
        return {"rolling_ic": m, "rolling_ir": ir}

    # ---- D-15: quantile sorts, long-short legs, turnover, coverage and IC statistics (README.md:1479-1487, :1535-1545, :1589-1599)
    def quantile(self, factor, next_return, n_quantiles=5):
        """-> {"mean_return", "count", "turnover": [Q, T], "spread": [T], "summary": [Q + 1, 5]} (bucket 0 = lowest factor values)"""
        return _api.factor_quantiles(factor, next_return, n_quantiles)

    def portfolio_sorts(self, factor, next_return, n_quantiles=5):
        """-> {"quantile", "mean_return", "std_return", "sharpe"}: one row per bucket plus a last row (quantile -1) for the
        top-minus-bottom spread"""
        s = _api.factor_quantiles(factor, next_return, n_quantiles)["summary"]
        q = torch.tensor(list(range(int(n_quantiles))) + [-1], dtype=torch.int32, device=s.device)
        return {"quantile": q, "mean_return": s[:, 1], "std_return": s[:, 2], "sharpe": s[:, 3]}

    def long_short(self, factor, next_return, top_pct=0.2, bottom_pct=0.2):
        """-> {"mean_return", "count", "turnover": [2, T] (short, long), "ls_return": [T], "summary": [3, 5]}"""
        return _api.factor_long_short(factor, next_return, top_pct, bottom_pct)

    def factor_mimicking_portfolio(self, factor, next_return, top_pct=0.3, bottom_pct=0.3):
        """-> {"long_return", "short_return", "ls_return"}: [T] each"""
        r = _api.factor_long_short(factor, next_return, top_pct, bottom_pct)
        return {"long_return": r["mean_return"][1], "short_return": r["mean_return"][0], "ls_return": r["ls_return"]}

    def turnover(self, factor, next_return, n_quantiles=5):
        """-> [Q, T]: share of each bucket's members that were not in it the day before"""
        return _api.factor_quantiles(factor, next_return, n_quantiles)["turnover"]

    def coverage(self, factor):
        """-> [T]: share of the symbols with a non-null finite factor value"""
        return _api.factor_coverage(factor)

    def ir(self, factor, next_return, rank=False):
        """-> mean / sample std of the (rank) IC series over its non-null days (not annualised; nan below 2 days or at std 0)"""
        ic, _ = _api.factor_ic(factor, next_return, 1 if rank else 0)
        return float(_api.ic_stats(ic)[3])

    def ic_win_rate(self, factor, next_return, rank=False):
        """-> share of the non-null days with a positive (rank) IC (nan below 2 days)"""
        ic, _ = _api.factor_ic(factor, next_return, 1 if rank else 0)
        return float(_api.ic_stats(ic)[4])

    # ---- D-31: the two-way (double) sort: does the factor survive controlling for size, or for another factor?
    def double_sort(self, control, factor, next_return, n_control=2, n_quantiles=3, dependent=True):
        """the symbols of each day in Qa = n_control buckets of `control` times Qb = n_quantiles buckets of `factor` (2 x 3: the
        size / value grid); dependent=True sorts the factor inside each control bucket, False both over the whole day.
        -> {"mean_return", "count", "turnover": [Qa, Qb, T], "spread": [Qa, T] (top - bottom factor bucket inside control bucket a),
        "spread_avg": [T] (their average: the HML-style series), "control_spread": [Qb, T], "control_spread_avg": [T] (the same
        along the control axis), "summary": {"cells": [Qa, Qb, 5], "spread": [Qa + 1, 5], "control_spread": [Qb + 1, 5]} (last row:
        the average)}; every tensor is a view of the call's buffers"""
        r = _api.factor_double_sort(control, factor, next_return, n_control, n_quantiles, dependent)
        qa, qb = int(n_control), int(n_quantiles)
        T = r["mean_return"].shape[1]
        s = r["summary"]
        return {"mean_return": r["mean_return"].view(qa, qb, T), "count": r["count"].view(qa, qb, T),
                "turnover": r["turnover"].view(qa, qb, T),
                "spread": r["spread_factor"][:qa], "spread_avg": r["spread_factor"][qa],
                "control_spread": r["spread_control"][:qb], "control_spread_avg": r["spread_control"][qb],
                "summary": {"cells": s[:qa * qb].view(qa, qb, s.shape[1]), "spread": s[qa * qb:qa * qb + qa + 1],
                            "control_spread": s[qa * qb + qa + 1:]}}

    # ---- D-27: the sorts' groups as portfolios that are held between rebalance days, with weights, drift and a fee on the traded value
    def portfolio_backtest(self, factor, price, n_quantiles=5, top_pct=None, bottom_pct=None, rebalance=20, start=0, weight=None, lag=0,
                           cost_rate=0.001, initial_capital=1_000_000.0, benchmark=None):
        """factor, price (and weight, e.g. the market cap; None: equal weights) [N, T].  The groups are the quantile buckets of the
        factor (0 = lowest values) or, with top_pct / bottom_pct, the two legs (0 = short, 1 = long), sorted per day over the symbols
        with a valid factor and a non-null finite price; a member also needs a price > 0.  rebalance: an interval in days (the
        rebalance days are start, start + rebalance, ...) or a sequence of day indices; a rebalance on day d uses the labels of day
        d - lag.  -> {"value": [G, T], "turnover": [G, R], "count": [G, R], "rebalance_days": [R], "daily_return": [G, T],
        "ls_return": [T] (top group minus bottom group, two long-only curves), "statistics": {name: [G]}, the curve columns of the
        backtest report and, with a benchmark [T], its benchmark columns}"""
        from ._spec import REPORT_COLS
        if (top_pct is None) != (bottom_pct is None):
            raise ValueError("top_pct and bottom_pct go together")
        T = _api._shape(price)[-1]
        if hasattr(rebalance, "__index__"):
            if int(rebalance) < 1:
                raise ValueError(f"rebalance must be an interval of at least one day or a sequence of days, not {rebalance!r}")
            rebalance = range(int(start), T, int(rebalance))
        if top_pct is None:
            groups = int(n_quantiles)
            lab = _api.factor_quantiles(factor, price, groups, labels=True)["labels"]
        else:
            groups = 2
            lab = _api.factor_long_short(factor, price, top_pct, bottom_pct, labels=True)["labels"]
        out = _api.factor_portfolio(lab, price, groups, list(rebalance), weight, lag, cost_rate, initial_capital)
        value = out["value"]
        (daily,) = _api.call("returns", value, period=1)
        out["daily_return"] = daily
        out["ls_return"] = _api.factor_binary(daily[groups - 1:], daily[:1], _api.BINARY_OPS["diff"])[0]
        rep = _api.backtest_report(value, initial_capital, benchmark)
        cols = list(range(15)) + (list(range(38, 45)) if benchmark is not None else [])
        out["statistics"] = {REPORT_COLS[c]: rep[:, c] for c in cols}
        return out

    # ---- D-30: K tested factors into the one score that quantile / long_short / portfolio_backtest take
    def combine(self, factors, next_return=None, method="icir", window=60, lag=1, rank=False, weights=None, normalize=True):
        """factors: a list of K [N, T] arrays or one [K, N, T] array (1 <= K <= 8), taken as given: standardise them first
        (Factor.normalize, clean), or the weights mix their scales.  -> {"composite": [N, T], "weights": [K, T], "ic": [K, T] or None}.
        composite[s, t] = sum_k weights[k, t] * factors[k][s, t], with normalize divided by sum_k |weights[k, t]|; NULL unless all K
        factors are non-null and finite there and the day has its K weights.  method "equal": weight 1.0 on every day (no
        next_return); "ic" / "icir" / "max_icir": from the daily IC (rank=True: Rank-IC) of each factor against next_return, over the
        `window` days that end at day t - lag: the mean IC, mean / sample std, and C^-1 mean with C the sample covariance of the K IC
        series (window >= 1 / 2 / K + 1; a day is NULL unless its window is complete and holds no NULL IC).  weights= ([K] or [K, T])
        replaces the method; next_return must then be left out.
        Look-ahead: the IC of day d uses the return that follows day d, so it is known only once that return is.  With an h-day forward
        return (next_return[s, d] = the return over days d .. d + h) pass lag >= h: the weights of day t then use ICs up to day t - h
        only.  lag=0 lets day t weigh itself by a return that is not known on day t."""
        methods = ("equal",) + tuple(_api.COMBINE_METHODS)
        if weights is None and method not in methods:
            raise ValueError(f"method must be one of {methods}, not {method!r}")
        if weights is not None and next_return is not None:
            raise ValueError("weights replaces the method: leave next_return out")
        from_ic = weights is None and method != "equal"
        if from_ic and next_return is None:
            raise ValueError(f"method {method!r} needs next_return")
        cols, (n, T) = _api._combine_args(factors, weights)
        K = len(cols)
        if from_ic:
            _api._combine_weight_args(K, _api.COMBINE_METHODS[method], window, lag)
            if _api._shape(next_return) != (n, T):
                raise ValueError(f"next_return must have the factors' shape {(n, T)}, not {_api._shape(next_return)}")
        cols = [_api._to_device(c)[0] for c in cols]            # uploaded once for the ICs and the composite
        dev = cols[0].device
        ic = None
        if from_ic:
            r = _api._to_device(next_return)[0]
            ic = torch.stack([_api.factor_ic(c, r, 1 if rank else 0)[0] for c in cols])
            w = _api.factor_combine_weights(ic, _api.COMBINE_METHODS[method], window, lag)
        elif weights is None:
            w = torch.ones((K, T), dtype=torch.float64, device=dev)
        else:
            w = _api.combine_weight_rows(weights, K, T, dev)
        return {"composite": _api.factor_combine(cols, w, normalize), "weights": w, "ic": ic}

    # ---- D-17: regressions and significance tests (README.md:1521-1600)
    def ic_test(self, factor, next_return, method="pearson"):
        """-> {"ic", "n_valid", "t_stat", "p_value"}: [T] each; t = ic sqrt((n - 2) / (1 - ic^2)), two-sided p on n - 2 degrees of
        freedom (method "pearson": IC, "spearman": Rank-IC)"""
        if method not in IC_METHODS:
            raise ValueError(f"method must be 'pearson' or 'spearman', not {method!r}")
        ic, nv = _api.factor_ic(factor, next_return, IC_METHODS[method])
        t, p = _api.corr_t_test(ic, nv)
        return {"ic": ic, "n_valid": nv, "t_stat": t, "p_value": p}

    def factor_return(self, factor, next_return):
        """-> {"factor_return", "intercept", "t_stat", "p_value", "r_squared", "n"}: [T] each, the per-day cross-sectional OLS of the
        next return on the factor with an intercept (t and p of the slope)"""
        r = _api.xsec_regress([factor], next_return, summary=False)
        return {"factor_return": r["coef"][0], "intercept": r["coef"][1], "t_stat": r["t_stat"][0], "p_value": r["p_value"][0],
                "r_squared": r["r_squared"], "n": r["n"]}

    def fama_macbeth(self, factors, next_return):
        """factors: a list of [N, T] arrays or one [K, N, T] array -> {"mean_coef", "std_coef", "t_stat", "p_value", "n_days"}: [K + 1]
        each (the intercept last), over the days with a solution, and "daily": {"coef", "t_stat", "p_value": [K + 1, T], "r_squared",
        "n": [T]}, the per-day cross-sectional regressions"""
        r = _api.xsec_regress(factors, next_return, summary=True)
        s = r.pop("summary")
        return {"mean_coef": s[:, 1], "std_coef": s[:, 2], "t_stat": s[:, 3], "p_value": s[:, 4], "n_days": s[:, 0], "daily": r}

    # ---- D-32: weighted cross-sectional regression with industry dummies
    def pure_factor_return(self, factors, next_return, weight=None, industry=None, specific_return=False):
        """The per-day weighted regression of the next return on K style factors and the industry dummies (no separate intercept).
        factors: a list of [N, T] arrays or one [K, N, T] array; weight [N, T] (e.g. sqrt(cap); None: equal); industry int codes [N] or
        [N, T] (negative = unclassified, G = max code + 1 <= 256; None: no industries, and "intercept" replaces "industry_return").
        -> {"factor_return", "t_stat", "p_value": [K, T]; "industry_return", "industry_t_stat", "industry_p_value": [G, T] (or
        "intercept", "intercept_t_stat", "intercept_p_value": [T]); "r_squared", "r_squared_within", "n", "n_industries": [T];
        "summary": {"factor" / "industry" (or "intercept"): {"mean_coef", "std_coef", "t_stat", "p_value", "n_days"}}, the
        Fama-MacBeth rows; with specific_return=True "specific_return" [N, T], the residual (NULL outside the day's sample)}"""
        r = _api.xsec_regress_wls(factors, next_return, weight, industry, summary=True, resid=specific_return)
        K = len(factors) if isinstance(factors, (list, tuple)) else _api._shape(factors)[0]
        s = r["summary"]

        def fm(rows):
            return {"mean_coef": rows[:, 1], "std_coef": rows[:, 2], "t_stat": rows[:, 3], "p_value": rows[:, 4], "n_days": rows[:, 0]}
        out = {"factor_return": r["coef"][:K], "t_stat": r["t_stat"][:K], "p_value": r["p_value"][:K]}
        if industry is not None:
            out.update({"industry_return": r["coef"][K:], "industry_t_stat": r["t_stat"][K:], "industry_p_value": r["p_value"][K:]})
            summ = {"factor": fm(s[:K]), "industry": fm(s[K:])}
        else:
            out.update({"intercept": r["coef"][K], "intercept_t_stat": r["t_stat"][K], "intercept_p_value": r["p_value"][K]})
            summ = {"factor": fm(s[:K]), "intercept": fm(s[K:])}
        out.update({"r_squared": r["r_squared"], "r_squared_within": r["r_squared_within"], "n": r["n"],
                    "n_industries": r["n_industries"], "summary": summ})
        if specific_return:
            out["specific_return"] = r["resid"]
        return out

    # ---- D-36: which factor, industry and specific returns the return of a book came from
    def return_attribution(self, holdings, exposures, returns, industry=None, next_return=None, benchmark=None, periods=None):
        """holdings [N, T] (weights or values; NULL or 0: not held) or the dict of weights_backtest(..., holdings=p), whose "holdings"
        is taken; exposures the K factors of the regression (a list of [N, T] arrays or one [K, N, T] array), industry its codes;
        returns: the dict of pure_factor_return(..., specific_return=True), or a pair (factor_return [K + G, T], specific_return
        [N, T]); next_return [N, T] (optional): the return that was regressed; benchmark (optional): a second [N, T] book or such a dict,
        which gives the three books portfolio, benchmark, active (= h - b) instead of one; periods: an int, read as
        numpy.array_split(range(T), periods) like subsample_test, or S + 1 explicit day bounds strictly ascending in [0, T].
        -> {"exposure", "contribution": [P, M, T]; "style", "industry", "specific", "unexplained", "total", "realized": [P, T];
        "n_held", "n_uncovered", "n_missing": [P, T] (int32); "summary": [P, M + 6, 5] (n_days, mean, std, t_stat, p_value of the M
        contributions and the six totals over their non-NULL days); with periods "period_sum": [P, M + 6, S], "period_days": [P, S],
        "period_bounds": [S + 1]}.  total = style + industry + specific + unexplained; a held symbol that lacks an exposure, an
        industry or a specific return is uncovered, its h r is the unexplained part (n_missing: it has no next return either); on a
        day without uncovered symbols total equals realized up to rounding.  A book's day is NULL where nothing is held and where a
        factor return that a non-zero exposure needs is NULL.  The period sums are arithmetic, not geometrically linked.
        Alignment: row t pairs the holdings at the close of day t with the return from t to t + 1, which is pure_factor_return's
        convention (it regresses the NEXT return on the exposures of day t): pass the same exposures, industry and next_return.
        Look-ahead: pure_factor_return regresses the NEXT return, so its row t -- and the attribution of day t -- is known one day
        later (risk_model's note)."""
        def book(x, what):
            if isinstance(x, dict):
                if "holdings" not in x:
                    raise ValueError(f"the {what} dict has no \"holdings\": call weights_backtest(..., holdings=p)")
                return x["holdings"]
            return x
        if isinstance(returns, dict):
            fr, sr = _stack_factor_returns(returns)
            if sr is None:
                raise ValueError("returns has no specific_return: call pure_factor_return(..., specific_return=True)")
        elif isinstance(returns, (list, tuple)) and len(returns) == 2:
            fr, sr = returns
        else:
            raise ValueError("returns must be pure_factor_return's dict or a pair (factor_return [K + G, T], specific_return [N, T])")
        return _api.return_attribution(book(holdings, "holdings"), exposures, fr, sr, industry, next_return,
                                       None if benchmark is None else book(benchmark, "benchmark"), periods)

    # ---- D-33: the risk model on pure_factor_return's three series, and the predicted risk of a portfolio from it
    def risk_model(self, factor_returns, specific_returns=None, window=252, halflife=None, min_periods=None, start=None, step=1,
                   unbiased=True, specific_window=None, specific_halflife=None):
        """factor_returns: an [M, T] array, or the dict that pure_factor_return returns -- its factor_return rows are then stacked with
        industry_return (or intercept) into the [K + G, T] block, and specific_return is taken from it where it is there and
        specific_returns is not given.  Exponentially weighted (halflife in days; None: equal weights) over the last `window` days, on
        the as-of days start, start + step, ... (start=None: window - 1, the first day with a full window); min_periods=None:
        max(2, window // 2); the specific_* arguments default to the factor ones (and the specific min_periods to max(2,
        specific_window // 2) where min_periods is not given).
        -> {"factor_cov": [D, M, M], "specific_var": [N, D] (if specific returns were given), "n": [D, M] (int32, the days behind each
        factor variance), "days": [D] (int64, the as-of days), "day0", "step"}.  Pairwise-complete: entry [j, l] uses the days on which
        both series are non-null and finite (an unsolved day is NULL in every row, a day without a member in that industry's), so the
        matrix need not be positive semi-definite.  NULL below min_periods days.
        Look-ahead: the model of as-of day t reads the rows t - window + 1 .. t and nothing later.  pure_factor_return regresses the
        NEXT return, so its row t, and the model "as of t", is known one day later: shift with Factor.delay where that matters."""
        sr = specific_returns
        if isinstance(factor_returns, dict):
            factor_returns, own = _stack_factor_returns(factor_returns)
            if sr is None:
                sr = own
        window = int(window)
        sw = window if specific_window is None else int(specific_window)
        shl = halflife if specific_halflife is None else specific_halflife
        mp = max(2, window // 2) if min_periods is None else min_periods
        smp = max(2, sw // 2) if min_periods is None else min_periods
        w = _api.risk_weights(window, halflife)
        ws = _api.risk_weights(sw, shl)
        T = _api._shape(factor_returns)[-1]
        day0 = window - 1 if start is None else start
        if sr is not None and _api._shape(sr)[-1] != T:
            raise ValueError(f"specific_returns must have the factor returns' {T} days, not {_api._shape(sr)}")
        cov, n = _api.risk_factor_cov(factor_returns, w, mp, day0, step, None, unbiased, counts=True)
        D = cov.shape[0]
        out = {"factor_cov": cov}
        if sr is not None:
            out["specific_var"] = _api.risk_specific_var(sr, ws, smp, day0, step, D, unbiased)
        out.update({"n": n, "days": int(day0) + int(step) * torch.arange(D, dtype=torch.int64, device=cov.device), "day0": int(day0),
                    "step": int(step)})
        return out

    def portfolio_risk(self, holdings, exposures, model, industry=None):
        """holdings [N, T] (weights or values; NULL or 0: not held), exposures the K factors of the regression (a list of [N, T] arrays
        or one [K, N, T] array), industry its codes, model the dict of risk_model (with its specific_var) -> {"exposure",
        "contribution": [M, D], "factor_var", "specific_var", "total_var", "volatility": [D], "n_held", "n_uncovered": [D] (int32)} on
        the model's as-of days: total_var = X' F X + sum h^2 s^2, contribution[j] = X_j (F X)_j.  A day is NULL where nothing is held,
        where a held symbol lacks an exposure, an industry or a specific variance (n_uncovered counts them), and where a covariance
        that the product needs is NULL.  The covariances are pairwise-complete and need not be positive semi-definite: volatility is
        NULL where total_var < 0.  Not annualised."""
        if "specific_var" not in model:
            raise ValueError("the model has no specific_var: pass specific returns to risk_model")
        return _api.risk_portfolio(holdings, exposures, model["factor_cov"], model["specific_var"], industry, model["day0"], model["step"])

    # ---- D-34: the portfolio that the risk model itself chooses
    def optimal_portfolio(self, exposures, model, alpha=None, industry=None, objective="min_variance", risk_aversion=1.0):
        """The minimum-variance, tangency or mean-variance portfolio under the model Sigma = B F B' + diag(s^2) on each of its as-of days.
        exposures, industry and model are portfolio_risk's; alpha [N, T] is the expected return of every symbol.  objective:
        "min_variance" (minimise w' Sigma w subject to 1' w = 1): w = y_1 / q_11; "max_sharpe" (alpha needed): w = y_a / q_1a, NULL where
        q_1a is not > 0; "mean_variance" (alpha needed; maximise a' w - (risk_aversion / 2) w' Sigma w subject to 1' w = 1):
        w = (y_a - g y_1) / risk_aversion with g = (q_1a - risk_aversion) / q_11.  Here y_v = Sigma^-1 v and q_uv = u' Sigma^-1 v come
        from one api.risk_solve call with the right-hand sides [ones] or [ones, alpha]; Sigma is never built.
        -> {"weights": [N, D], "predicted_var": [D] (w' Sigma w, from the same q: not a second pass), "expected_return": [D] (a' w, NULL
        without alpha), "n_universe", "n_uncovered": [D] (int32), "days": [D] (int64)}.  A symbol that lacks an exposure, an industry, a
        specific variance or an alpha on a day gets a NULL weight (n_uncovered counts those whose alpha is there); a day is NULL where no
        symbol is left, where a covariance that the system needs is NULL and where the system is singular.
        The weights sum to 1 and are unconstrained in sign: long-only or box constraints need an iterative solver and are not covered.
        Not annualised.  Look-ahead: pure_factor_return regresses the NEXT return, so a model "as of t" from its series is known one day
        later (risk_model's note)."""
        if objective not in ("min_variance", "max_sharpe", "mean_variance"):
            raise ValueError(f"objective must be 'min_variance', 'max_sharpe' or 'mean_variance', not {objective!r}")
        if alpha is None and objective != "min_variance":
            raise ValueError(f"objective {objective!r} needs alpha")
        lam = float(risk_aversion)
        if not (0.0 < lam < float("inf")):
            raise ValueError(f"risk_aversion must be finite and > 0, not {risk_aversion!r}")
        if "specific_var" not in model:
            raise ValueError("the model has no specific_var: pass specific returns to risk_model")
        if alpha is None:       # (the vector of ones as an array: it tells the days where there is no exposure either)
            T = int(model["day0"]) + max(int(_api._shape(model["factor_cov"])[0]) - 1, 0) * int(model["step"]) + 1
            first = next(iter(exposures), None) if isinstance(exposures, (list, tuple)) else (None if exposures is None else exposures[0])
            rhs = [None] if first is not None else [torch.ones((_api._shape(model["specific_var"])[0], T), dtype=torch.float64)]
        else:
            rhs = [None, alpha]
        y, q, n = _api.risk_solve(rhs, exposures, model["factor_cov"], model["specific_var"], industry, model["day0"], model["step"])
        null = torch.from_numpy(_api.np.full(1, _api.NULL)).to(y.device)[0]   # (a tensor copy keeps NULL's payload)
        nn = lambda v: torch.where(torch.isnan(v), null, v)   # noqa: E731
        q11 = q[0, 0]
        if objective == "min_variance":
            w, var = y[0] / q11, 1.0 / q11
            ret = q[1, 0] / q11 if alpha is not None else torch.full_like(q11, float("nan"))
        else:
            q1a, qaa = q[1, 0], q[1, 1]
            if objective == "max_sharpe":
                bad = ~(q1a > 0.0)
                w, var, ret = y[1] / q1a, qaa / (q1a * q1a), qaa / q1a
                w, var, ret = torch.where(bad, null, w), torch.where(bad, null, var), torch.where(bad, null, ret)
            else:
                lt = torch.full((), lam, dtype=torch.float64, device=y.device)   # a device divisor: a true division, no reciprocal
                gam = (q1a - lt) / q11
                w = (y[1] - gam * y[0]) / lt
                ret = (qaa - gam * q1a) / lt
                var = ((qaa - (2.0 * gam) * q1a) + (gam * gam) * q11) / (lt * lt)
        D = q.shape[2]
        days = int(model["day0"]) + int(model["step"]) * torch.arange(D, dtype=torch.int64, device=y.device)
        return {"weights": nn(w), "predicted_var": nn(var), "expected_return": nn(ret), "n_universe": n[0], "n_uncovered": n[1],
                "days": days}

    # ---- D-35: what given weights would have earned -- signed, with cash, with turnover and costs
    def weights_backtest(self, weights, price, days=None, lag=0, cost_rate=0.001, initial_capital=1_000_000.0, benchmark=None,
                         holdings=None):
        """weights: one [N, R] array, a list of P such arrays or one [P, N, R] array (1 <= P <= 8), column k the target weights of
        rebalance k -- or the dict that optimal_portfolio returns, whose "weights" and "days" are then taken.  price [N, T]; days [R]: the
        day each column is known.  The trade day of column k is days[k] + lag; trailing columns whose trade day is >= T are dropped, and
        the returned "rebalance_days" shows the days that were used.  The weights are signed and need not sum to one: the remainder is
        cash (negative under leverage), a NULL, NaN or infinite weight is not held, and a target without a usable price on its trade day
        is dropped (n_dropped counts them, the weight stays in cash).  Holdings drift with their prices, every rebalance pays cost_rate
        on the traded value; no borrow or financing rate is charged on the short leg or on negative cash.
        -> {"value": [P, T], "turnover", "net", "gross": [P, R], "n_long", "n_short", "n_dropped": [P, R] (int32), "first_nonpositive":
        [P] (int32), "rebalance_days": [R], "daily_return": [P, T], "statistics": {name: [P]}, the curve columns of the backtest report
        and, with a benchmark [T], its benchmark columns} and, with holdings=p, "holdings": [N, T], portfolio p's drifted weights on
        every day -- what portfolio_risk(holdings=...) takes.  first_nonpositive is the first day whose value is not > 0 (-1: none): a
        signed, levered book can be ruined, and the curve and the statistics after that day mean nothing.
        Look-ahead: pure_factor_return regresses the NEXT return, so a model "as of t" from its series, and a portfolio built from it,
        is known one day later (risk_model's note): trade it with lag=1."""
        from ._spec import REPORT_COLS
        if isinstance(weights, dict):
            if days is None:
                days = weights["days"]
            weights = weights["weights"]
        if days is None:
            raise ValueError("days is needed: the day each column of weights is known (optimal_portfolio's dict carries its own)")
        if not hasattr(lag, "__index__") or int(lag) < 0:
            raise ValueError(f"lag must be a non-negative number of days, not {lag!r}")
        d = days.cpu().numpy() if isinstance(days, torch.Tensor) else _api.np.asarray(days)
        if d.size and d.dtype.kind not in "iu":
            raise ValueError("days must hold integer day indices")
        d = d.reshape(-1).astype(_api.np.int64) + int(lag)
        T = _api._shape(price)[-1]
        stacked = not isinstance(weights, (list, tuple))
        cols = [weights] if stacked else list(weights)
        for c in cols:
            if _api._shape(c)[-1:] != (d.size,):
                raise ValueError(f"weights must have one column per day: {d.size}, not {_api._shape(c)}")
        keep = d.size
        while keep and d[keep - 1] >= T:
            keep -= 1
        if keep < d.size:
            cols = [c[..., :keep] for c in cols]
        out = _api.factor_weights(cols[0] if stacked else cols, price, d[:keep], cost_rate, initial_capital, holdings)
        value = out["value"]
        (daily,) = _api.call("returns", value, period=1)
        out["daily_return"] = daily
        rep = _api.backtest_report(value, initial_capital, benchmark)
        cols = list(range(15)) + (list(range(38, 45)) if benchmark is not None else [])
        out["statistics"] = {REPORT_COLS[c]: rep[:, c] for c in cols}
        return out

    def time_series_regression(self, factors, returns):
        """factors: a list of [N, T] or [T] arrays (a [T] series, e.g. a market return, is shared by every symbol) or one [K, N, T]
        array -> {"coefficient", "t_stat", "p_value": [N, K + 1] (the intercept last), "r_squared", "n_obs": [N]}, one OLS per symbol
        over its days"""
        r = _api.ts_regress(factors, returns)
        return {"coefficient": r["coef"], "t_stat": r["t_stat"], "p_value": r["p_value"], "r_squared": r["r_squared"],
                "n_obs": r["n_obs"]}

    # ---- D-18: IC decay, sub-period and sub-group robustness tests (README.md:1556-1565, :1607-1624)
    def ic_decay(self, factor, next_return, max_lag=10, method="pearson"):
        """-> {"lag", "ic", "std_ic", "t_stat", "p_value", "n_days"}: [max_lag] each, over the non-null days of the IC of the factor of
        day t against the return of day t + lag - 1 (lag 1 = the ordinary IC), and "daily": {"ic", "n_valid": [max_lag, T]}"""
        r = _api.ic_decay(factor, next_return, max_lag, _method(method))
        s = r.pop("summary")
        lag = torch.arange(1, s.shape[0] + 1, dtype=torch.int32, device=s.device)
        return {"lag": lag, "ic": s[:, 1], "std_ic": s[:, 2], "t_stat": s[:, 3], "p_value": s[:, 4], "n_days": s[:, 0], "daily": r}

    def subsample_test(self, factor, next_return, n_splits=3, method="pearson", dates=None):
        """-> {"period", "start", "end", "mean_ic", "std_ic", "t_stat", "p_value", "n_days"}: [n_splits] each, the daily IC summarised
        over numpy.array_split(range(T), n_splits) (start / end: inclusive day indices); with dates (length T), also "start_date" /
        "end_date" lists"""
        m = _method(method)
        T = _api._ic_pair_args(factor, next_return, m)[1]
        start, end = _api.split_periods(T, n_splits)
        if dates is not None and len(dates) != T:
            raise ValueError(f"dates must have one entry per day ({T}), not {len(dates)}")
        ic, _ = _api.factor_ic(factor, next_return, m)
        s = _api.series_split_summary(ic, n_splits)
        p = torch.arange(len(start), dtype=torch.int64, device=s.device)   # the bounds of split_periods, built on the device (no copy)
        q, rem = divmod(T, len(start))
        first = p * q + p.clamp(max=rem)
        out = {"period": p.to(torch.int32), "start": first, "end": first + (q - 1) + (p < rem), "mean_ic": s[:, 1], "std_ic": s[:, 2],
               "t_stat": s[:, 3], "p_value": s[:, 4], "n_days": s[:, 0]}
        if dates is not None:
            out["start_date"] = [dates[int(i)] for i in start]
            out["end_date"] = [dates[int(i)] for i in end]
        return out

    def subgroup_test(self, factor, next_return, group, method="pearson"):
        """group: integer codes [N] or [N, T] (e.g. industries; negative = unclassified, at most 256 groups) -> {"group", "mean_ic",
        "std_ic", "t_stat", "p_value", "n_days"}: [G] each (G = max code + 1), and "daily": {"ic", "n_valid": [G, T]}, the per-day IC
        within each group"""
        r = _api.ic_subgroup(factor, next_return, group, _method(method))
        s = r.pop("summary")
        g = torch.arange(s.shape[0], dtype=torch.int32, device=s.device)
        return {"group": g, "mean_ic": s[:, 1], "std_ic": s[:, 2], "t_stat": s[:, 3], "p_value": s[:, 4], "n_days": s[:, 0], "daily": r}

    # ---- D-19: multi-factor orthogonalization and neutralization (README.md:1495-1519); reached as Factor().clean
    def _clean_factors(self, factors, method="orthogonalize", inplace=False):
        """Factor().clean(factors, method="orthogonalize", inplace=False).  factors: a list of K [N, T] arrays or one [K, N, T] array
        (2 <= K <= 8), in order of priority.  Per day, over the symbols whose K factors are all non-null and finite: "orthogonalize" (sequential Gram-Schmidt) keeps factor 0 as it is and replaces factor k
        by its OLS residual on factors 0 .. k-1 -> [K, N, T]; "neutralize" gives the residual of each factor 1 .. K-1 on factor 0 alone
        -> [K - 1, N, T].  NULL outside the day's sample and where the regression has no solution.  inplace=True (orthogonalize only,
        factors a device float64 [K, N, T] tensor) rewrites rows 1 .. K-1 of factors and returns it."""
        if method not in _api.ORTH_MODES:
            raise ValueError(f"method must be 'orthogonalize' or 'neutralize', not {method!r}")
        mode = _api.ORTH_MODES[method]
        cols, _ = _api._orth_args(factors, mode)
        if not inplace:
            return _api.factor_orthogonalize(factors, mode, keep_first=mode == 0)
        if mode != 0:
            raise ValueError("inplace=True is only for method='orthogonalize'")
        if not (isinstance(factors, torch.Tensor) and factors.is_cuda and factors.dtype == torch.float64 and factors.dim() == 3
                and (factors.shape[2] <= 1 or factors.stride(2) == 1)):
            raise ValueError("inplace=True needs one device float64 [K, N, T] tensor with unit stride along days")
        _api.factor_orthogonalize(factors, 0, out=[factors[j] for j in range(1, len(cols))])
        return factors


def _method(method):
    if method not in IC_METHODS:
        raise ValueError(f"method must be 'pearson' or 'spearman', not {method!r}")
    return IC_METHODS[method]


def clean(factor, winsorize=None, winsorize_n=None, neutralize_market_cap=False, cap=None, neutralize_industry=False, industry=None,
          standardize=False, log_cap=True):
    """README `clean(df, col, winsorize, winsorize_n, neutralize_market_cap, cap_col, neutralize_industry, industry_col, standardize)`
    (README.md:244-345) on arrays instead of columns: factor and cap [N, T], industry integer codes [N] or [N, T] (negative =
    unclassified).  Per day and in the README's order: winsorize ("mad" / "sigma" / "percentile"; winsorize_n=None picks 3.0 / 3.0 /
    1.0), size neutralization (OLS residual on log(cap), or on cap with log_cap=False), industry neutralization (minus the industry mean,
    after the size step), standardize.  -> device tensor [N, T]; NULL outside the day's cross-section.  Decision D-16, DESIGN.md section 2."""
    if neutralize_market_cap and cap is None:
        raise ValueError("neutralize_market_cap=True needs cap")
    if neutralize_industry and industry is None:
        raise ValueError("neutralize_industry=True needs industry")
    return _api.factor_clean(factor, winsorize, winsorize_n, cap if neutralize_market_cap else None, log_cap,
                             industry if neutralize_industry else None, standardize)
