"""Test-side restatement of decision D-33 in numpy: the weighted covariance of two windows (rk_wcov), the factor
covariance matrix and the specific variances on the as-of days, and the predicted risk of a portfolio from the two.

Independent of the HIP kernels: every sum of a window is an explicit loop over the window offset that starts at 0.0 and adds the
sample's entries in ascending day order (vectorised over the series and the as-of days, never np.cov / np.sum / np.average), the
cross-sectional sums go through xsec_clean_ref.bsum (D-12's blocked sum), the matrix-vector product is a loop over its columns in
ascending order, and every other step is one elementwise IEEE operation in the stated order.  So the GPU results are compared bit for
bit.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)

MAX_WINDOW = 1024
MAX_SERIES = 264


def weights(window, halflife=None):
    """api.risk_weights"""
    if halflife is None:
        return np.ones(window)
    return 0.5 ** ((window - 1 - np.arange(window, dtype=np.float64)) / float(halflife))


def as_of_days(day0, step, count):
    return int(day0) + int(step) * np.arange(int(count), dtype=np.int64)


def wcov(A, B, om, days, min_periods, unbiased=True):
    """rk_wcov of the rows of A against the rows of B (A [..., T] and B [..., T] broadcast over their leading axes) on every as-of day
    -> (cov [..., D], n [..., D] int32)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    om = np.asarray(om, dtype=np.float64)
    days = np.asarray(days, dtype=np.int64)
    w = len(om)
    assert 1 <= w <= MAX_WINDOW and 1 <= min_periods <= w and (min_periods >= 2 or not unbiased)
    shape = np.broadcast_shapes(A.shape[:-1], B.shape[:-1]) + (len(days),)

    def col(X, k):
        """win[k] of every as-of day: the value of day t - (w - 1 - k), NULL before day 0"""
        t = days - (w - 1 - k)
        return np.where(t >= 0, X[..., np.clip(t, 0, None)], NULL)

    W, W2, Sa, Sb = (np.zeros(shape) for _ in range(4))
    n = np.zeros(shape, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(w):
            o = float(om[k])
            if not o > 0.0:
                continue
            a, b = col(A, k), col(B, k)
            ok = valid(a) & valid(b)
            W = np.where(ok, W + o, W)
            W2 = np.where(ok, W2 + o * o, W2)
            Sa = np.where(ok, Sa + o * a, Sa)
            Sb = np.where(ok, Sb + o * b, Sb)
            n = n + ok
        ma, mb = Sa / W, Sb / W
        C = np.zeros(shape)
        for k in range(w):
            o = float(om[k])
            if not o > 0.0:
                continue
            a, b = col(A, k), col(B, k)
            ok = valid(a) & valid(b)
            C = np.where(ok, C + (o * (a - ma)) * (b - mb), C)
        den = W - W2 / W if unbiased else W
        cov = C / den
        good = (n >= min_periods) & ((n >= 2) | (not unbiased)) & (den > 0.0) & ~np.isnan(cov)
    return np.where(good, cov, NULL), n.astype(np.int32)


def factor_cov(F, om, days, min_periods, unbiased=True):
    """F [M, T] -> (cov [D, M, M], n [D, M]): entry [d][j][l], l <= j, is rk_wcov(f_j, f_l) with f_j as a, mirrored to [d][l][j]"""
    F = np.asarray(F, dtype=np.float64)
    M = F.shape[0]
    assert M <= MAX_SERIES
    full, n = wcov(F[:, None, :], F[None, :, :], om, days, min_periods, unbiased)      # [j, l, d]
    low = np.tril(np.ones((M, M), dtype=bool))[:, :, None]
    sym = np.where(low, full, np.swapaxes(full, 0, 1))
    return np.ascontiguousarray(np.moveaxis(sym, 2, 0)), np.ascontiguousarray(n[np.arange(M), np.arange(M)].T)


def specific_var(X, om, days, min_periods, unbiased=True):
    """X [N, T] -> (var [N, D], n [N, D])"""
    return wcov(X, X, om, days, min_periods, unbiased)


def nan_null(v):
    return np.where(np.isnan(v), NULL, v)


def portfolio(H, exposures, cov, sv, days, industry=None, G=1):
    """H [N, T], exposures a list of K [N, T], cov [D, K + G, K + G], sv [N, D], industry [N] or [N, T] codes or None (G = 1)
    -> dict(exposure, contribution [M, D], risk [4, D] (factor_var, specific_var, total_var, volatility), n [2, D] int32)"""
    H = np.asarray(H, dtype=np.float64)
    days = np.asarray(days, dtype=np.int64)
    cov, sv = np.asarray(cov, dtype=np.float64), np.asarray(sv, dtype=np.float64)
    N, D, K = H.shape[0], len(days), len(exposures)
    M = K + G
    assert cov.shape == (D, M, M) and sv.shape == (N, D) and (industry is not None or G == 1)
    h = H[:, days]
    xs = [np.asarray(x, dtype=np.float64)[:, days] for x in exposures]
    held = valid(h) & (h != 0.0)
    with np.errstate(all="ignore"):
        covered = sv >= 0.0                                     # NULL, NaN and negative variances fail
        for x in xs:
            covered = covered & valid(x)
        if industry is None:
            g = np.zeros((N, D), dtype=np.int64)
        else:
            ind = np.asarray(industry).astype(np.int64)
            g = ind[:, days] if ind.ndim == 2 else np.broadcast_to(ind[:, None], (N, D))
            covered = covered & (g >= 0) & (g < G)
        n = np.stack([held.sum(axis=0), (held & ~covered).sum(axis=0)]).astype(np.int32)
        mem = held & covered
        X = np.zeros((M, D))
        for j in range(K):
            X[j] = bsum(h * xs[j], mem)
        for gg in range(G):
            X[K + gg] = bsum(h, mem & (g == gg))
        S = bsum((h * h) * sv, mem)
        live = X != 0.0
        v = np.zeros((M, D))
        missing = np.zeros((M, D), dtype=bool)
        for l in range(M):                                      # v_j = sum_l cov[j][l] X[l] over ascending l with X[l] != 0
            cv = cov[:, :, l].T                                 # [j, d]
            use = live & live[l][None, :]
            v = np.where(use, v + cv * X[l][None, :], v)
            missing = missing | (use & isnull(cv))
        c = np.where(live, np.where(missing, NULL, X * v), 0.0)
        nul = (n[0] == 0) | (n[1] > 0) | isnull(c).any(axis=0)
        fv = np.zeros(D)
        for j in range(M):
            fv = fv + c[j]
        tot = fv + S
        vol = np.where(tot < 0.0, NULL, np.sqrt(tot))
    risk = np.where(nul[None, :], NULL, nan_null(np.stack([fv, S, tot, vol])))
    return {"exposure": np.where(nul[None, :], NULL, nan_null(X)), "contribution": np.where(nul[None, :], NULL, nan_null(c)), "risk": risk,
            "n": n}
