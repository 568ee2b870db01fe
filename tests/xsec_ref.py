"""Test-side restatement of decision D-15 in numpy / scipy: quantile and long-short labels, per-group
mean return / count / turnover, the top-minus-bottom series, the summary rows, coverage and IC statistics.

Independent of the HIP kernels: ranks come from scipy.stats.rankdata (average ranks, m = 2R - 1), the blocked cross-sectional sums
are explicit ascending loops over symbols (vectorised over days, members only), and the sequential statistics are Python float loops
in ascending day order.  Every value is exact integer arithmetic or a correctly rounded IEEE operation in the stated order, so the
GPU results are compared bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.stats import rankdata

NULL_BITS = 0x7FF80000504E554C
NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]
LABEL_OUT, LABEL_MID = 255, 254
BLOCK = 256
ANN = 252.0


def isnull(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64) == np.uint64(NULL_BITS)


def valid(x):
    x = np.asarray(x, dtype=np.float64)
    return ~isnull(x) & np.isfinite(x)


def label_day(f, r, mode, q=0, top=0.0, bottom=0.0):
    """one day's cross-section: f, r [N] -> uint8 labels [N]"""
    f, r = np.asarray(f, dtype=np.float64), np.asarray(r, dtype=np.float64)
    ok = valid(f) & valid(r)
    n = int(ok.sum())
    out = np.full(f.shape[0], LABEL_OUT, dtype=np.uint8)
    if n < (q if mode == 0 else 2):
        return out
    R = rankdata(f[ok], method="average")          # half-integers, exact
    m = (2.0 * R - 1.0).astype(np.int64)           # = a + b for the tie run [a, b)
    if mode == 0:
        lab = (m * q) // (2 * n)
    else:
        p = m.astype(np.float64) / np.float64(2 * n)
        lab = np.where(p > np.float64(1.0) - np.float64(top), 1, np.where(p < np.float64(bottom), 0, LABEL_MID))
    out[ok] = lab.astype(np.uint8)
    return out


def labels(factor, ret, mode, q=0, top=0.0, bottom=0.0, days=None):
    """[N, T] -> uint8 [N, len(days)] (all days when days is None)"""
    days = range(factor.shape[1]) if days is None else days
    return np.stack([label_day(factor[:, t], ret[:, t], mode, q, top, bottom) for t in days], axis=1) if len(days) else \
        np.zeros((factor.shape[0], 0), dtype=np.uint8)


def group_sums(lab, ret, ng, lab_prev=None):
    """lab, ret [N, D] (lab_prev [N, D] or None) -> block-ordered sums [ng, D], counts [ng, D], new members [ng, D]"""
    N, D = lab.shape
    g = np.arange(ng)[:, None]
    total = np.zeros((ng, D))
    cnt = np.zeros((ng, D), dtype=np.int64)
    new = np.zeros((ng, D), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, N, BLOCK):
            blk = np.zeros((ng, D))
            for s in range(b0, min(b0 + BLOCK, N)):
                mem = lab[s][None, :] == g
                blk = np.where(mem, blk + ret[s][None, :], blk)
                cnt += mem
                if lab_prev is not None:
                    new += mem & (lab_prev[s][None, :] != g)
            total = total + blk
    return total, cnt, new


def sample_days(days, T):
    """the days a restatement of `days` needs: each day t together with t - 1 (for turnover), sorted"""
    need = set()
    for t in days:
        need.add(int(t))
        if t > 0:
            need.add(int(t) - 1)
    return sorted(x for x in need if 0 <= x < T)


def groups(factor, ret, mode, q=0, top=0.0, bottom=0.0, days=None):
    """D-15 per-day outputs on `days` (all when None) -> dict: labels [N, D], mean_return / count / turnover [ng, D], spread [D]"""
    factor, ret = np.asarray(factor, dtype=np.float64), np.asarray(ret, dtype=np.float64)
    N, T = factor.shape
    days = list(range(T)) if days is None else [int(t) for t in days]
    need = sample_days(days, T)
    col = {t: i for i, t in enumerate(need)}
    L = labels(factor, ret, mode, q, top, bottom, need)
    ng = q if mode == 0 else 2
    cur = L[:, [col[t] for t in days]]
    prev = np.stack([L[:, col[t - 1]] if t > 0 else np.full(N, LABEL_OUT, np.uint8) for t in days], axis=1) if days else cur
    rr = ret[:, days]
    total, cnt, new = group_sums(cur, rr, ng, prev)
    _, cnt_prev, _ = group_sums(prev, rr, ng)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, total / np.maximum(cnt, 1), NULL)
        first = np.array([t == 0 for t in days])[None, :]
        tov = np.where(~first & (cnt > 0) & (cnt_prev > 0), new / np.maximum(cnt, 1), NULL)
        lo, hi = mean[0], mean[ng - 1]
        spread = np.where(isnull(lo) | isnull(hi), NULL, hi - lo)
    return {"labels": cur, "mean_return": mean, "count": cnt.astype(np.int32), "turnover": tov, "spread": spread}


def _seq(x, center=None):
    s, n, pos = 0.0, 0, 0
    for v in np.asarray(x, dtype=np.float64).tolist():
        if v != v:
            continue
        if center is None:
            s += v
            pos += v > 0.0
        else:
            d = v - center
            s += d * d
        n += 1
    return s, n, pos


def summary_row(x, tov=None):
    """n_days, mean_return, std_return, sharpe, mean_turnover of one series over its non-null days"""
    s, n, _ = _seq(x)
    m = s / n if n > 0 else NULL
    ss, _, _ = _seq(x, m if n > 0 else 0.0)
    sd = math.sqrt(ss / (n - 1)) if n >= 2 else NULL
    sharpe = m / sd * math.sqrt(ANN) if (n >= 2 and sd > 0.0) else NULL
    mt = NULL
    if tov is not None:
        ts, nt, _ = _seq(tov)
        mt = ts / nt if nt > 0 else NULL
    return [float(n), m, sd, sharpe, mt]


def summary(res):
    """[ng + 1, 5] from groups(...) over ALL days"""
    ng = res["mean_return"].shape[0]
    rows = [summary_row(res["mean_return"][g], res["turnover"][g]) for g in range(ng)]
    rows.append(summary_row(res["spread"]))
    return np.array(rows, dtype=np.float64)


def coverage(factor):
    factor = np.asarray(factor, dtype=np.float64)
    N = factor.shape[0]
    if N == 0:
        return np.full(factor.shape[1], NULL)
    return valid(factor).sum(axis=0).astype(np.float64) / np.float64(N)


def ic_stats(ic):
    """n_days, mean, std, ir, win_rate of an IC series over its non-null days"""
    s, n, pos = _seq(ic)
    if n < 2:
        return np.array([float(n), NULL, NULL, NULL, NULL])
    m = s / n
    ss, _, _ = _seq(ic, m)
    sd = math.sqrt(ss / (n - 1))
    return np.array([float(n), m, sd, m / sd if sd > 0.0 else NULL, pos / n])
