"""Test-side restatement of decision D-29 in numpy: the time-series operators ts_sum / ts_std / ts_zscore /
ts_min / ts_max / ts_argmin / ts_argmax / ts_rank / decay_linear / delay / delta and the two-column ts_cov / ts_corr along the days of
every symbol of an [N, T] column.

Independent of the HIP kernel: every sum is an explicit loop over the window offset that starts at 0.0 and adds whole [N, T] slices in
ascending day order (never np.sum / np.mean / np.std / np.corrcoef, whose pairwise order differs), the ordering ops are loops over the
offset with elementwise compares, and every other step is one elementwise IEEE operation in the stated order.  So the GPU results are
compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)
from xsec_rolling_ref import finish, shift, window_all, window_sum

OPS = ("sum", "std", "zscore", "min", "max", "argmin", "argmax", "rank", "decay_linear", "delay", "delta")
PAIR_OPS = ("cov", "corr")
MIN_WINDOW = {"sum": 1, "std": 2, "zscore": 2, "min": 1, "max": 1, "argmin": 1, "argmax": 1, "rank": 1, "decay_linear": 1, "delay": 1,
              "delta": 1, "cov": 2, "corr": 2}
MAX_WINDOW = 1024
ORDERING = ("min", "max", "argmin", "argmax", "rank")


def day(v, w, k):
    """-> win[k] of every row: the value of day t - (w - 1 - k), 0.0 before the series"""
    return shift(v, w - 1 - k, 0.0)


def sq_dev(v, m, w):
    """sum of (win[k] - m)^2 in ascending k from 0.0, m the row's own mean"""
    q2 = np.zeros(v.shape)
    for k in range(w):
        e = day(v, w, k) - m
        q2 = q2 + e * e
    return q2


def ts(x, op, window, mode=0):
    x = np.asarray(x, dtype=np.float64)
    w = int(window)
    assert op in OPS and MIN_WINDOW[op] <= w <= MAX_WINDOW and (mode == 0 or (mode == 1 and op == "rank"))
    dw = float(w)
    with np.errstate(all="ignore"):
        if op == "delay":
            b = shift(x, w, NULL)
            return np.where(np.isnan(b), NULL, b)
        if op == "delta":
            b = shift(x, w, NULL)
            return finish(x - b, valid(x) & valid(b))
        ok = valid(x)
        full = window_all(ok, w)
        v = np.where(ok, x, 0.0)
        if op == "sum":
            return finish(window_sum(v, w), full)
        if op in ("std", "zscore"):
            m = window_sum(v, w) / dw
            q2 = sq_dev(v, m, w)
            sd = np.sqrt(q2 / float(w - 1))
            if op == "std":
                return finish(sd, full)
            return finish((v - m) / sd, full & (q2 != 0.0))
        if op == "decay_linear":
            acc = np.zeros(x.shape)
            for k in range(w):
                acc = acc + float(k + 1) * day(v, w, k)
            return finish(acc / float(w * (w + 1) // 2), full)
        if op == "rank":
            less, equal = np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape, dtype=np.int64)
            for k in range(w):
                c = day(v, w, k)
                less += c < v
                equal += c == v
            r = (2 * less + equal + 1).astype(np.float64) * 0.5
            return finish(r / dw if mode == 1 else r, full)
        m, at = day(v, w, 0), np.zeros(x.shape)
        for k in range(1, w):                       # strict compares: of equal extremes the oldest stays
            c = day(v, w, k)
            better = c < m if op in ("min", "argmin") else c > m
            m = np.where(better, c, m)
            at = np.where(better, float(k), at)
        return finish(m if op in ("min", "max") else at, full)


def ts_pair(x, y, op, window):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = int(window)
    assert op in PAIR_OPS and x.shape == y.shape and MIN_WINDOW[op] <= w <= MAX_WINDOW
    dw = float(w)
    ok = valid(x) & valid(y)
    full = window_all(ok, w)
    a, b = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    with np.errstate(all="ignore"):
        mx, my = window_sum(a, w) / dw, window_sum(b, w) / dw
        sxy, sxx, syy = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape)
        for k in range(w):
            dx, dy = day(a, w, k) - mx, day(b, w, k) - my
            sxy = sxy + dx * dy
            sxx = sxx + dx * dx
            syy = syy + dy * dy
        if op == "cov":
            return finish(sxy / float(w - 1), full)
        return finish(sxy / (np.sqrt(sxx) * np.sqrt(syy)), full & (sxx != 0.0) & (syy != 0.0))


def ts_sum(x, window):
    return ts(x, "sum", window)


def ts_std(x, window):
    return ts(x, "std", window)


def ts_zscore(x, window):
    return ts(x, "zscore", window)


def ts_min(x, window):
    return ts(x, "min", window)


def ts_max(x, window):
    return ts(x, "max", window)


def ts_argmin(x, window):
    return ts(x, "argmin", window)


def ts_argmax(x, window):
    return ts(x, "argmax", window)


def ts_rank(x, window, pct=False):
    return ts(x, "rank", window, 1 if pct else 0)


def decay_linear(x, window):
    return ts(x, "decay_linear", window)


def delay(x, periods=1):
    return ts(x, "delay", periods)


def delta(x, periods=1):
    return ts(x, "delta", periods)


def ts_cov(x, y, window):
    return ts_pair(x, y, "cov", window)


def ts_corr(x, y, window):
    return ts_pair(x, y, "corr", window)
