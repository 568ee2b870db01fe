"""Test-side restatement of decision D-32 in numpy / scipy: the weighted per-day cross-sectional regression of
the next return on K style factors and G industry dummies (Factor.pure_factor_return).

Independent of the HIP kernels: every sum is xsec_clean_ref.bsum (explicit ascending loops over each block of 256 symbol indices,
members only; a per-industry sum is the same loop restricted to the industry's members), and the within-industry demeaning, the
L D L^T factorisation, the substitutions and the standard errors are written out element by element in D-32's order, vectorised over
the days.  So coef / t / both R^2 / n / G_t / resid and the Fama-MacBeth n / mean / std / t are compared bit for bit.  p-values come
from scipy.special.stdtr, never from the device's formula.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (isnull: re-exported for the tests)
from xsec_regress_ref import SINGULAR, _forward, fm_summary, t_pvalue  # noqa: F401  (fm_summary: re-exported)

MAX_K = 8
MAX_G = 256


def bsums(cols, mem):
    """bsum of several [N, T] columns over one sample, in one walk of the blocks (the columns side by side along the day axis)"""
    T = mem.shape[1]
    out = bsum(np.concatenate(cols, axis=1), np.concatenate([mem] * len(cols), axis=1))
    return [out[k * T:(k + 1) * T] for k in range(len(cols))]


def sample(F, r, w, ind, G):
    mem = valid(r) & valid(w) & (ind >= 0) & (ind < G)
    with np.errstate(invalid="ignore"):
        mem &= w > 0.0
    for f in F:
        mem = mem & valid(f)
    return mem


def wls(factors, ret, weight=None, industry=None, n_groups=None):
    """D-32: factors list of [N, T] (or [K, N, T]), ret [N, T], weight [N, T] or None (1.0), industry int codes [N] or [N, T] or None
    (one group; its row is the intercept), n_groups (default max code + 1) -> dict: coef / t / p [K + G, T] (factors, then
    industries), r2 [2, T] (total, within), n / gt [T] (int32), ok [T] (bool: the day solved), resid [N, T]"""
    r = np.asarray(ret, dtype=np.float64)
    N, T = r.shape
    F = np.stack([np.asarray(f, dtype=np.float64) for f in factors]) if len(factors) else np.zeros((0, N, T))
    K = F.shape[0]
    w = np.ones((N, T)) if weight is None else np.asarray(weight, dtype=np.float64)
    if industry is None:
        ind, G = np.zeros((N, T), dtype=np.int64), 1
    else:
        ind = np.asarray(industry, dtype=np.int64)
        if ind.ndim == 1:
            ind = np.repeat(ind[:, None], T, axis=1)
        G = n_groups if n_groups is not None else (max(int(ind.max()) + 1, 1) if ind.size else 1)
    mem = sample(F, r, w, ind, G)
    days = np.arange(T)[None, :]
    with np.errstate(all="ignore"):
        # pass 1: per (day, industry) the member count, W = sum w and S[c] = sum (w x_c), the product rounded first
        X = [r] + [F[j] for j in range(K)]
        WX = [w] + [w * x for x in X]
        cnt = np.zeros((G, T), dtype=np.int64)
        Wg = np.zeros((G, T))
        Sg = np.zeros((K + 1, G, T))
        for g in range(G):
            mg = mem & (ind == g)
            cnt[g] = mg.sum(axis=0)
            s = bsums(WX, mg)
            Wg[g] = s[0]
            for c in range(K + 1):
                Sg[c, g] = s[1 + c]
        M = Sg / Wg[None]                                   # m_g[c]; NaN for an industry without a member
        present = cnt > 0
        n = cnt.sum(axis=0).astype(np.int32)
        gt = present.sum(axis=0).astype(np.int32)
        sw, sr = np.zeros(T), np.zeros(T)
        for g in range(G):                                  # present industries, ascending, from 0.0
            sw = np.where(present[g], sw + Wg[g], sw)
            sr = np.where(present[g], sr + Sg[0, g], sr)
        rbar = sr / sw
        # pass 2: the cross-products of the within-industry deviations
        gi = np.clip(ind, 0, G - 1)
        dr = r - M[0][gi, days]
        df = [F[j] - M[1 + j][gi, days] for j in range(K)]
        wd = [w * df[j] for j in range(K)]
        dt = r - rbar
        terms = [wd[j] * df[l] for j in range(K) for l in range(j + 1)] + [wd[j] * dr for j in range(K)] + [(w * dr) * dr, (w * dt) * dt]
        s = bsums(terms, mem)
        Cm = [[s[j * (j + 1) // 2 + l] if l <= j else None for l in range(K)] for j in range(K)]
        c = s[K * (K + 1) // 2:K * (K + 1) // 2 + K]
        srr, stot = s[-2], s[-1]
        # C = L D L^T by rows (D-17); W2[j][k] = the numerator of L[j][k]
        L = [[np.ones(T) if j == k else np.zeros(T) for k in range(K)] for j in range(K)]
        W2 = [[np.zeros(T) for _ in range(K)] for _ in range(K)]
        D = [None] * K
        ok = n >= K + gt + 1
        for j in range(K):
            for k in range(j):
                x = Cm[j][k]
                for m in range(k):
                    x = x - W2[j][m] * L[k][m]
                W2[j][k] = x
                L[j][k] = x / D[k]
            d = Cm[j][j]
            for m in range(j):
                d = d - W2[j][m] * L[j][m]
            D[j] = d
            ok &= d > SINGULAR * Cm[j][j]
        z = _forward(L, c)
        b = [None] * K
        for j in range(K - 1, -1, -1):
            x = np.zeros(T)
            for m in range(j + 1, K):
                x = x + L[m][j] * b[m]
            b[j] = z[j] / D[j] - x
        V = []
        for j in range(K):
            u = _forward(L, [np.full(T, 1.0 if m == j else 0.0) for m in range(K)])
            vj = np.zeros(T)
            for m in range(K):
                vj = vj + u[m] * u[m] / D[m]
            V.append(vj)
        # industry returns g_g = m_g[r] - sum_j b_j m_g[f_j], V_g = 1 / W_g + sum_m u_m u_m / D_m with L u = m_g[f]
        gcoef = []
        for g in range(G):
            sa = np.zeros(T)
            for j in range(K):
                sa = sa + b[j] * M[1 + j, g]
            gcoef.append(M[0, g] - sa)
            u = _forward(L, [M[1 + j, g] for j in range(K)])
            q = np.zeros(T)
            for m in range(K):
                q = q + u[m] * u[m] / D[m]
            V.append(1.0 / Wg[g] + q)
        # pass 3
        fit = np.zeros_like(r)
        for j in range(K):
            fit = fit + b[j] * df[j]
        e = dr - fit
        sse = bsum((w * e) * e, mem)
        dof = (n - K - gt).astype(np.float64)
        s2 = sse / dof
        coef = np.array(b + gcoef)
        se = np.sqrt(s2 * np.array(V))
        tt = np.where(se == 0.0, NULL, coef / se)
        pp = np.where(se == 0.0, NULL, t_pvalue(tt, dof))
        r2 = np.array([np.where(ok & (stot != 0.0), 1.0 - sse / stot, NULL), np.where(ok & (srr != 0.0), 1.0 - sse / srr, NULL)])
    live = np.concatenate([np.broadcast_to(ok, (K, T)), present & ok[None, :]])
    return {"coef": np.where(live, coef, NULL), "t": np.where(live, tt, NULL), "p": np.where(live, pp, NULL), "r2": r2, "n": n, "gt": gt,
            "ok": ok, "resid": np.where(mem & ok[None, :], e, NULL)}
