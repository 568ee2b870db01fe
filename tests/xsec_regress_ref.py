"""Test-side restatement of decision D-17 in numpy / scipy: the per-day cross-sectional OLS (factor_return,
fama_macbeth), the per-symbol time-series OLS (time_series_regression) and the correlation t-test (ic_test).

Independent of the HIP kernels: the blocked sums are xsec_clean_ref.bsum (explicit ascending loops over each block of 256 indices,
members only), and the L D L^T factorisation, the substitutions and the standard errors are written out element by element in D-17's
order, vectorised over the units (days or symbols).  So coef / t / R^2 / n and the Fama-MacBeth mean / std / t are compared bit for bit.
p-values come from scipy.special.stdtr, never from the device's formula.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.special import stdtr

from xsec_clean_ref import bsum
from xsec_ref import NULL, _seq, isnull, valid  # noqa: F401  (isnull: re-exported for the tests)

MAX_K = 8
SINGULAR = 1e-12


def t_pvalue(t, df):
    """two-sided Student-t p-value, NaN where t is NaN"""
    t, df = np.asarray(t, dtype=np.float64), np.asarray(df, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(t), np.nan, 2.0 * stdtr(df, -np.abs(t)))


def _forward(L, v):
    """z_m = v_m - sum_{i < m} L[m][i] z_i, the sum ascending from 0.0 (L unit lower-triangular; arrays over the units)"""
    K = len(v)
    z = [None] * K
    for m in range(K):
        s = np.zeros_like(v[0])
        for i in range(m):
            s = s + L[m][i] * z[i]
        z[m] = v[m] - s
    return z


def regress_units(F, r, mem):
    """D-17 on units along the last axis: F [K, I, U] factors, r [I, U] returns, mem [I, U] the sample (I = the summation index, in
    blocks of 256) -> dict: coef / t / p [K + 1, U] (row K = the intercept), r2 [U], n [U] (int32)"""
    F = np.asarray(F, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    K, _, U = F.shape
    n = mem.sum(axis=0).astype(np.int32)
    dn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        rbar = bsum(r, mem) / dn
        fbar = [bsum(F[j], mem) / dn for j in range(K)]
        dr = r - rbar
        df = [F[j] - fbar[j] for j in range(K)]
        Cm = [[bsum(df[j] * df[l], mem) if l <= j else None for l in range(K)] for j in range(K)]
        c = [bsum(df[j] * dr, mem) for j in range(K)]
        srr = bsum(dr * dr, mem)
        # C = L D L^T by rows; W[j][k] = the numerator of L[j][k] (= L[j][k] D[k] before rounding)
        L = [[np.ones(U) if j == k else np.zeros(U) for k in range(K)] for j in range(K)]
        W = [[np.zeros(U) for _ in range(K)] for _ in range(K)]
        D = [None] * K
        ok = n >= K + 2
        for j in range(K):
            for k in range(j):
                w = Cm[j][k]
                for m in range(k):
                    w = w - W[j][m] * L[k][m]
                W[j][k] = w
                L[j][k] = w / D[k]
            d = Cm[j][j]
            for m in range(j):
                d = d - W[j][m] * L[j][m]
            D[j] = d
            ok &= d > SINGULAR * Cm[j][j]
        z = _forward(L, c)
        b = [None] * K
        for j in range(K - 1, -1, -1):
            t = np.zeros(U)
            for m in range(j + 1, K):
                t = t + L[m][j] * b[m]
            b[j] = z[j] / D[j] - t
        sa = np.zeros(U)
        for j in range(K):
            sa = sa + b[j] * fbar[j]
        a = rbar - sa
        V = []
        for j in range(K):
            w = _forward(L, [np.full(U, 1.0 if m == j else 0.0) for m in range(K)])
            vj = np.zeros(U)
            for m in range(K):
                vj = vj + w[m] * w[m] / D[m]
            V.append(vj)
        w = _forward(L, fbar)
        q = np.zeros(U)
        for m in range(K):
            q = q + w[m] * w[m] / D[m]
        V.append(1.0 / dn + q)
        fit = np.zeros_like(r)
        for j in range(K):
            fit = fit + b[j] * df[j]
        e = dr - fit
        sse = bsum(e * e, mem)
        dof = (n - K - 1).astype(np.float64)
        s2 = sse / dof
        coef = np.array(b + [a])
        se = np.sqrt(s2 * np.array(V))
        tt = np.where(se == 0.0, NULL, coef / se)
        pp = np.where(se == 0.0, NULL, t_pvalue(tt, dof))
        r2 = np.where(ok & (srr != 0.0), 1.0 - sse / srr, NULL)
    coef = np.where(ok, coef, NULL)
    tt = np.where(ok, tt, NULL)
    pp = np.where(ok, pp, NULL)
    return {"coef": coef, "t": tt, "p": pp, "r2": r2, "n": n}


def _factor_stack(factors, shape):
    """list of [N, T] (or [T]: one series for every symbol) -> [K, N, T]"""
    return np.stack([np.broadcast_to(np.asarray(f, dtype=np.float64), shape) for f in factors])


def sample(F, r):
    mem = valid(r)
    for f in F:
        mem = mem & valid(f)
    return mem


def xsec_regress(factors, ret):
    """per-day cross-sectional regression: factors list of [N, T], ret [N, T] -> regress_units over the symbols, units = days"""
    r = np.asarray(ret, dtype=np.float64)
    F = _factor_stack(factors, r.shape)
    return regress_units(F, r, sample(F, r))


def ts_regress(factors, ret):
    """per-symbol time-series regression: factors list of [N, T] or [T], ret [N, T] -> coef / t / p [N, K + 1], r2 / n [N]"""
    r = np.asarray(ret, dtype=np.float64)
    F = _factor_stack(factors, r.shape)
    out = regress_units(np.ascontiguousarray(F.transpose(0, 2, 1)), np.ascontiguousarray(r.T), sample(F, r).T)
    return {"coef": out["coef"].T, "t": out["t"].T, "p": out["p"].T, "r2": out["r2"], "n": out["n"]}


def fm_summary(coef):
    """Fama-MacBeth summary of coef [K + 1, T] -> [K + 1, 5]: n_days, mean, std (ddof 1), t = mean / (std / sqrt(n_days)), p on
    n_days - 1, over the non-NaN days of each row (sequential sums from 0.0 in day order, two-pass std)"""
    rows = []
    for x in np.asarray(coef, dtype=np.float64):
        s, n, _ = _seq(x)
        m = s / n if n > 0 else NULL
        sd = math.sqrt(_seq(x, m)[0] / (n - 1)) if n >= 2 else 0.0
        if n < 2 or sd == 0.0:
            rows.append([float(n), m, NULL, NULL, NULL])
            continue
        t = m / (sd / math.sqrt(n))
        rows.append([float(n), m, sd, t, float(t_pvalue(t, n - 1))])
    return np.array(rows)


def corr_t_test(corr, n_valid):
    """t = corr sqrt((n - 2) / (1 - corr corr)), p on n - 2; NULL where corr is NaN, n < 3 or 1 - corr^2 == 0"""
    r = np.asarray(corr, dtype=np.float64)
    n = np.asarray(n_valid).astype(np.int64)
    with np.errstate(all="ignore"):
        den = 1.0 - r * r
        dof = (n - 2).astype(np.float64)
        t = r * np.sqrt(dof / den)
        bad = np.isnan(r) | (n < 3) | (den == 0.0)
        t = np.where(bad, NULL, t)
        p = np.where(bad, NULL, t_pvalue(t, dof))
    return t, p
