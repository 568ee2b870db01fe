"""Test-side restatement of decision D-21 in numpy: the rolling technical factors moving_average / momentum /
volatility / skewness / relative_strength along the days of every symbol of an [N, T] column.

Independent of the HIP kernel: every sum is an explicit loop over the window offset that starts at 0.0 and adds whole [N, T] slices in
ascending day order (never np.sum / np.mean / np.std, whose pairwise order differs), and every other step is one elementwise IEEE
operation in the stated order.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)

OPS = ("mean", "momentum", "volatility", "skewness", "relative_strength")
MIN_WINDOW = {"mean": 1, "momentum": 1, "volatility": 2, "skewness": 3, "relative_strength": 1}
MAX_WINDOW = 1024


def shift(a, k, fill):
    """-> b with b[:, t] = a[:, t - k], `fill` where t < k"""
    out = np.full(a.shape, fill, dtype=a.dtype)
    if k < a.shape[1]:
        out[:, k:] = a[:, :a.shape[1] - k]
    return out


def finish(v, full):
    """NULL where the sample is incomplete or the value came out NaN"""
    return np.where(full & ~np.isnan(v), v, NULL)


def window_sum(term, w):
    """sum of term[t - w + 1 .. t], from 0.0 in ascending day order"""
    acc = np.zeros(term.shape)
    for k in range(w - 1, -1, -1):
        acc = acc + shift(term, k, 0.0)
    return acc


def window_all(ok, w):
    full = np.ones(ok.shape, dtype=bool)
    for k in range(w):
        full &= shift(ok, k, False)
    return full


def derived(x, kind):
    """-> (series, usable): r[j] = (x[j] - x[j-1]) / x[j-1] where both days are valid and r is finite, or d[j] = x[j] - x[j-1] where
    both days are valid; 0.0 elsewhere"""
    ok = valid(x) & shift(valid(x), 1, False)
    prev = shift(x, 1, 0.0)
    with np.errstate(all="ignore"):
        v = x - prev
        if kind == "r":
            v = v / prev
            ok = ok & np.isfinite(v)
    return np.where(ok, v, 0.0), ok


def rolling(x, op, window, skip=0):
    x = np.asarray(x, dtype=np.float64)
    w = int(window)
    assert op in OPS and MIN_WINDOW[op] <= w <= MAX_WINDOW and skip >= 0 and (skip == 0 or op == "momentum")
    dw = float(w)
    with np.errstate(all="ignore"):
        if op == "mean":
            ok = valid(x)
            return finish(window_sum(np.where(ok, x, 0.0), w) / dw, window_all(ok, w))
        if op == "momentum":
            a, b = shift(x, skip, NULL), shift(x, skip + w, NULL)
            return finish((a - b) / b, valid(a) & valid(b))
        if op == "relative_strength":
            d, ok = derived(x, "d")
            G = window_sum(np.where(d > 0.0, d, 0.0), w)
            L = window_sum(np.where(d < 0.0, -d, 0.0), w)
            den = G + L
            return finish((100.0 * G) / den, window_all(ok, w) & (den != 0.0))
        r, ok = derived(x, "r")
        full = window_all(ok, w)
        m = window_sum(r, w) / dw
        q2, q3 = np.zeros(x.shape), np.zeros(x.shape)
        for k in range(w - 1, -1, -1):          # the deviation of day t - k from the mean of row t's window
            e = shift(r, k, 0.0) - m
            sq = e * e
            q2 = q2 + sq
            q3 = q3 + sq * e
        if op == "volatility":
            return finish(np.sqrt(q2 / float(w - 1)), full)
        m2, m3 = q2 / dw, q3 / dw
        return finish(m3 / (m2 * np.sqrt(m2)), full & (m2 != 0.0))


def moving_average(x, window=20):
    return rolling(x, "mean", window)


def momentum(x, window=20, skip=0):
    return rolling(x, "momentum", window, skip)


def volatility(x, window=20):
    return rolling(x, "volatility", window)


def skewness(x, window=20):
    return rolling(x, "skewness", window)


def relative_strength(x, window=14):
    return rolling(x, "relative_strength", window)
