"""Test-side restatement of decision D-28 in numpy: the rolling-window OLS y = a + sum_j b_j x_j over the last
`window` days of every symbol of [N, T] columns -- rolling beta, alpha, residual std, R^2 and the residual of the window's last day.

Independent of the HIP kernel: every sum is an explicit loop over the window offset that starts at 0.0 and adds whole [N, T] slices in
ascending day order (xsec_rolling_ref.window_sum's way, never np.sum), and the L D L^T factorisation, the substitutions and the
intercept are written out element by element in the order of xsec_regress_ref.regress_units (D-17) with n = window, vectorised over
the rows.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_regress_ref import SINGULAR, _forward
from xsec_rolling_ref import MAX_WINDOW, shift, window_all, window_sum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)

MAX_K = 4
OUTPUTS = ("beta", "alpha", "resid_std", "r_squared", "resid")


def rolling_regress(y, xs, window):
    """y [N, T]; xs: K regressors, each [N, T] or a [T] series shared by every symbol -> {"beta": [K, N, T], "alpha", "resid_std",
    "r_squared", "resid": [N, T]}"""
    y = np.asarray(y, dtype=np.float64)
    K, w = len(xs), int(window)
    assert y.ndim == 2 and 1 <= K <= MAX_K and K + 2 <= w <= MAX_WINDOW
    cols = [np.broadcast_to(np.asarray(x, dtype=np.float64), y.shape) for x in xs] + [y]      # x_0 .. x_{K-1}, y
    ok = np.ones(y.shape, dtype=bool)
    for c in cols:
        ok &= valid(c)
    full = window_all(ok, w)                     # all K + 1 values valid on each of the w days; false for t < w - 1
    z = [np.where(ok, c, 0.0) for c in cols]     # (what a row without its sample computes is thrown away)
    dw = float(w)
    zero = np.zeros(y.shape)
    with np.errstate(all="ignore"):
        # pass 1: the K + 1 sums and means
        mean = [window_sum(c, w) / dw for c in z]
        # pass 2: the centred products d_j d_l (l <= j) of the K + 1 columns; row K holds d_j d_y and d_y d_y
        S = [[zero for _ in range(j + 1)] for j in range(K + 1)]
        for k in range(w - 1, -1, -1):           # day t - k of row t's window, ascending days
            dv = [shift(z[c], k, 0.0) - mean[c] for c in range(K + 1)]
            for j in range(K + 1):
                for l in range(j + 1):
                    S[j][l] = S[j][l] + dv[j] * dv[l]
        syy = S[K][K]
        # C = L D L^T by rows (D-17's order and singular rule)
        L = [[np.ones(y.shape) if j == k else zero for k in range(K)] for j in range(K)]
        W = [[zero for _ in range(K)] for _ in range(K)]
        D = [None] * K
        solved = full.copy()
        for j in range(K):
            for k in range(j):
                t = S[j][k]
                for m in range(k):
                    t = t - W[j][m] * L[k][m]
                W[j][k] = t
                L[j][k] = t / D[k]
            d = S[j][j]
            for m in range(j):
                d = d - W[j][m] * L[j][m]
            D[j] = d
            solved &= d > SINGULAR * S[j][j]
        zz = _forward(L, [S[K][j] for j in range(K)])
        b = [None] * K
        for j in range(K - 1, -1, -1):
            t = zero
            for m in range(j + 1, K):
                t = t + L[m][j] * b[m]
            b[j] = zz[j] / D[j] - t
        sa = zero
        for j in range(K):
            sa = sa + b[j] * mean[j]
        alpha = mean[K] - sa
        # pass 3: the residuals
        sse, e = zero, zero
        for k in range(w - 1, -1, -1):
            fit = zero
            for j in range(K):
                fit = fit + b[j] * (shift(z[j], k, 0.0) - mean[j])
            e = (shift(z[K], k, 0.0) - mean[K]) - fit
            sse = sse + e * e
        resid_std = np.sqrt(sse / float(w - K - 1))
        r2 = 1.0 - sse / syy
        has_r2 = syy != 0.0
        # a row with a NaN result has none at all
        num = ~np.isnan(alpha) & ~np.isnan(resid_std) & ~np.isnan(e) & (~has_r2 | ~np.isnan(r2))
        for j in range(K):
            num &= ~np.isnan(b[j])
        good = solved & num
    return {"beta": np.stack([np.where(good, bj, NULL) for bj in b]), "alpha": np.where(good, alpha, NULL),
            "resid_std": np.where(good, resid_std, NULL), "r_squared": np.where(good & has_r2, r2, NULL),
            "resid": np.where(good, e, NULL)}
