"""Test-side restatement of decision D-36 in numpy: the return attribution of holdings through the factor model.

Independent of the HIP kernels: every cross-sectional sum goes through xsec_clean_ref.bsum (D-12's blocked sum) with the products
rounded first, the totals are explicit loops over the rows in ascending order from 0.0, the summary rows are xsec_regress_ref's
sequential fm_summary and the period sums explicit loops over the days; every other step is one elementwise IEEE operation in the
stated order.  No kernel is called and no numpy.linalg.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)
from xsec_regress_ref import fm_summary

MAX_K = 8
MAX_G = 256
TOTALS = ("style", "industry", "specific", "unexplained", "total", "realized")


def nan_null(v):
    return np.where(np.isnan(v), NULL, v)


def books(holdings, benchmark=None):
    """the P books [P, N, T]: the holdings alone, or the portfolio, the benchmark and the active book a = h - b, where a holding that
    is not valid counts as 0.0"""
    h = np.asarray(holdings, dtype=np.float64)
    if benchmark is None:
        return h[None]
    b = np.asarray(benchmark, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = np.where(valid(h), h, 0.0) - np.where(valid(b), b, 0.0)
    return np.stack([h, b, a])


def check_bounds(bounds, T):
    b = np.asarray(bounds, dtype=np.int64).reshape(-1)
    assert b.size >= 2 and b[0] >= 0 and b[-1] <= T and (np.diff(b) > 0).all(), "bounds: S + 1 day indices strictly ascending in [0, T]"
    return b


def attribution(holdings, exposures, factor_return, specific_return, industry=None, G=1, next_return=None, benchmark=None, bounds=None):
    """holdings [N, T], exposures a list of K [N, T], factor_return [K + G, T], specific_return [N, T], industry [N] or [N, T] codes or
    None (G = 1), next_return [N, T] or None, benchmark [N, T] or None, bounds S + 1 day indices or None
    -> dict(exposure, contribution [P, M, T], totals [P, 6, T], n [3, P, T] int32, summary [P, M + 6, 5] and, with bounds, period_sum
    [P, M + 6, S], period_days [P, S] int32)"""
    B = books(holdings, benchmark)
    P, N, T = B.shape
    xs = [np.asarray(x, dtype=np.float64) for x in exposures]
    K = len(xs)
    M = K + G
    assert K <= MAX_K and 1 <= G <= MAX_G and (industry is not None or G == 1)
    f = np.asarray(factor_return, dtype=np.float64)
    u = np.asarray(specific_return, dtype=np.float64)
    assert f.shape == (M, T) and u.shape == (N, T)
    r = None if next_return is None else np.asarray(next_return, dtype=np.float64)
    covered = valid(u)
    for x in xs:
        covered = covered & valid(x)
    if industry is None:
        g = np.zeros((N, T), dtype=np.int64)
    else:
        ind = np.asarray(industry).astype(np.int64)
        g = ind if ind.ndim == 2 else np.broadcast_to(ind[:, None], (N, T))
        covered = covered & (g >= 0) & (g < G)
    r_ok = np.zeros((N, T), dtype=bool) if r is None else valid(r)
    rr = np.zeros((N, T)) if r is None else r
    n = np.zeros((3, P, T), dtype=np.int32)
    expo, contrib = np.zeros((P, M, T)), np.zeros((P, M, T))
    totals = np.zeros((P, 6, T))
    with np.errstate(all="ignore"):
        for p in range(P):
            h = B[p]
            held = valid(h) & (h != 0.0)
            mem, unc = held & covered, held & ~covered
            n[0, p], n[1, p], n[2, p] = held.sum(axis=0), unc.sum(axis=0), (unc & ~r_ok).sum(axis=0)
            X = np.zeros((M, T))
            for j in range(K):
                X[j] = bsum(h * xs[j], mem)
            for gg in range(G):
                X[K + gg] = bsum(h, mem & (g == gg))
            spec = bsum(h * u, mem)
            unex = bsum(h * rr, unc & r_ok)
            real = bsum(h * rr, held & r_ok)
            live = X != 0.0
            c = np.where(live, X * f, 0.0)
            nul = (n[0, p] == 0) | (live & ~valid(f)).any(axis=0)
            style, indu = np.zeros(T), np.zeros(T)
            for j in range(K):
                style = style + c[j]
            for gg in range(G):
                indu = indu + c[K + gg]
            total = ((style + indu) + spec) + unex
            rows = np.stack([style, indu, spec, unex, total, real])
            rows = nan_null(rows)
            if r is None:
                rows[5] = NULL
            expo[p] = np.where(nul[None], NULL, nan_null(X))
            contrib[p] = np.where(nul[None], NULL, nan_null(c))
            totals[p] = np.where(nul[None], NULL, rows)
    series = np.concatenate([contrib, totals], axis=1)                  # [P, M + 6, T]
    out = {"exposure": expo, "contribution": contrib, "totals": totals, "n": n,
           "summary": np.stack([fm_summary(series[p]) for p in range(P)])}
    if bounds is not None:
        b = check_bounds(bounds, T)
        S = b.size - 1
        psum = np.zeros((P, M + 6, S))
        pdays = np.zeros((P, S), dtype=np.int32)
        for p in range(P):
            for q in range(M + 6):
                row = series[p, q].tolist()
                for k in range(S):
                    s, cnt = 0.0, 0
                    for t in range(int(b[k]), int(b[k + 1])):           # the period's non-NULL days, ascending from 0.0
                        v = row[t]
                        if v == v:
                            s += v
                            cnt += 1
                    psum[p, q, k] = s
                    if q == M + 4:
                        pdays[p, k] = cnt
        out["period_sum"], out["period_days"] = psum, pdays
    return out
