"""Test-side restatement of decision D-34 in numpy: y_r = Sigma^-1 v_r under the factor risk model of D-33,
Sigma = B F B^T + diag(s^2), through the factor structure -- the moments A = B^T diag(q) B and p_r = B^T diag(q) v_r with q = 1 / s^2,
the M x M system (I + F A) u = F p on the active rows, and y = q (v - B u) -- with the matrix v_r^T Sigma^-1 v_q, and the three
portfolios that Factor.optimal_portfolio forms from them.

Independent of the HIP kernels and in the definition's order: the cross-sectional sums go through xsec_clean_ref.bsum (D-12's blocked
sum), the products F A and F p are loops over the inner index in ascending order from 0.0, the LU with partial pivoting and the back
substitution are explicit loops over the columns and rows (one elementwise IEEE operation per step, vectorised only across entries that
do not depend on each other), and nothing calls numpy.linalg.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)
from xsec_risk_ref import as_of_days, nan_null  # noqa: F401

MAX_RHS = 4
MAX_M = 128


def lu_solve(S, C):
    """[S | C] (S [m, m], C [m, R]) by in-place LU with partial pivoting -> u [m, R], or None where a pivot is 0, NaN or infinite.
    At column c the pivot is the first row >= c with the largest |S[., c]| (a NaN never displaces an entry)."""
    S, C = np.array(S, dtype=np.float64), np.array(C, dtype=np.float64)
    m = S.shape[0]
    with np.errstate(all="ignore"):
        for c in range(m):
            best = c
            for i in range(c + 1, m):
                if abs(S[i, c]) > abs(S[best, c]):
                    best = i
            if best != c:
                S[[c, best]] = S[[best, c]]
                C[[c, best]] = C[[best, c]]
            piv = S[c, c]
            if not (piv != 0.0 and np.isfinite(piv)):
                return None
            for i in range(c + 1, m):
                mu = S[i, c] / piv
                S[i, c + 1:] = S[i, c + 1:] - mu * S[c, c + 1:]
                C[i] = C[i] - mu * C[c]
        u = np.zeros_like(C)
        for a in range(m - 1, -1, -1):
            s = np.zeros(C.shape[1])
            for b in range(a + 1, m):
                s = s + S[a, b] * u[b]
            u[a] = (C[a] - s) / S[a, a]
    return u


def moments(v, xs, q, U, g, G):
    """-> (A [D, M, M], p [R, D, M]): the blocked sums of the definition"""
    K, R, D = len(xs), len(v), q.shape[1]
    M = K + G
    A, p = np.zeros((D, M, M)), np.zeros((R, D, M))
    with np.errstate(all="ignore"):
        qx = [q * x for x in xs]
        for j in range(K):
            for l in range(j + 1):
                A[:, j, l] = A[:, l, j] = bsum(qx[j] * xs[l], U)
            for r in range(R):
                p[r, :, j] = bsum(qx[j] * v[r], U)
        for gg in range(G):
            mem = U & (g == gg)
            for j in range(K):
                A[:, K + gg, j] = A[:, j, K + gg] = bsum(qx[j], mem)
            A[:, K + gg, K + gg] = bsum(q, mem)
            for r in range(R):
                p[r, :, K + gg] = bsum(q * v[r], mem)
    return A, p


def solve(rhs, exposures, cov, sv, days, industry=None, G=1):
    """rhs: a list of R [N, T] arrays or None (ones); exposures: a list of K [N, T]; cov [D, K + G, K + G]; sv [N, D]; industry [N] or [N, T]
    codes or None (G = 1) -> dict(y [R, N, D], quad [R, R, D], n [2, D] int32 (|U|, uncovered), null [D] bool, u [R, D, M], cond [D])"""
    days = np.asarray(days, dtype=np.int64)
    cov, sv = np.asarray(cov, dtype=np.float64), np.asarray(sv, dtype=np.float64)
    N, D = sv.shape
    K, R = len(exposures), len(rhs)
    M = K + G
    assert 1 <= R <= MAX_RHS and 1 <= M <= MAX_M and cov.shape == (D, M, M) and D == len(days) and (industry is not None or G == 1)
    xs = [np.asarray(x, dtype=np.float64)[:, days] for x in exposures]
    v = [np.ones((N, D)) if a is None else np.asarray(a, dtype=np.float64)[:, days] for a in rhs]
    if industry is None:
        g = np.zeros((N, D), dtype=np.int64)
    else:
        ind = np.asarray(industry).astype(np.int64)
        g = ind[:, days] if ind.ndim == 2 else np.broadcast_to(ind[:, None], (N, D))
    with np.errstate(all="ignore"):
        given = np.ones((N, D), dtype=bool)
        for a in v:
            given &= valid(a)
        covered = (sv > 0.0) & (g >= 0) & (g < G)               # NULL, NaN, zero and negative variances fail
        for x in xs:
            covered &= valid(x)
        U = given & covered
        n = np.stack([U.sum(axis=0), (given & ~covered).sum(axis=0)]).astype(np.int32)
        q = 1.0 / sv
        A, p = moments(v, xs, q, U, g, G)
        ufull = np.zeros((R, D, M))
        active = np.zeros((D, M), dtype=bool)
        null = n[0] == 0
        cond = np.full(D, np.nan)
        for d in range(D):
            J = [j for j in range(M) if A[d, j, j] > 0.0]
            active[d, J] = True
            if null[d]:
                continue
            m = len(J)
            F = cov[d][np.ix_(J, J)]
            if isnull(F).any():
                null[d] = True
                continue
            Aj = A[d][np.ix_(J, J)]
            S, C = np.zeros((m, m)), np.zeros((m, R))
            for c in range(m):                                  # over ascending c from 0.0
                S = S + F[:, c][:, None] * Aj[c][None, :]
                C = C + F[:, c][:, None] * p[:, d, J[c]][None, :]
            for a in range(m):
                S[a, a] = S[a, a] + 1.0
            u = lu_solve(S, C)
            if u is None or not np.isfinite(u).all():
                null[d] = True
                continue
            cond[d] = np.linalg.cond(S) if m else 1.0           # (reported to the tests, not used)
            ufull[:, d, J] = u.T
        yraw = np.full((R, N, D), np.nan)
        gc = np.clip(g, 0, G - 1)
        for r in range(R):
            e = np.zeros((N, D))
            for j in range(K):
                e = np.where(active[:, j][None, :], e + xs[j] * ufull[r, :, j][None, :], e)
            e = e + np.take_along_axis(ufull[r][:, K:], gc.T, axis=1).T
            yraw[r] = q * (v[r] - e)
        live = U & ~null[None, :]
        y = np.where(live[None], nan_null(yraw), NULL)
        quad = np.full((R, R, D), NULL)
        for r in range(R):
            for l in range(r + 1):
                quad[r, l] = quad[l, r] = np.where(null, NULL, nan_null(bsum(v[r] * yraw[l], live)))
    return {"y": y, "quad": quad, "n": n, "null": null, "u": ufull, "cond": cond}


OBJECTIVES = ("min_variance", "max_sharpe", "mean_variance")


def optimal(y, quad, objective, risk_aversion=1.0):
    """Factor.optimal_portfolio's elementwise step: rhs 0 is the vector of ones, rhs 1 (where given) alpha
    -> (weights [N, D], predicted_var [D], expected_return [D])"""
    lam = float(risk_aversion)
    with np.errstate(all="ignore"):
        q11 = quad[0, 0]
        if objective == "min_variance":
            w, var = y[0] / q11[None, :], 1.0 / q11
            ret = quad[1, 0] / q11 if len(y) > 1 else np.full_like(q11, NULL)
        else:
            q1a, qaa = quad[1, 0], quad[1, 1]
            if objective == "max_sharpe":
                w, var, ret = y[1] / q1a[None, :], qaa / (q1a * q1a), qaa / q1a
                bad = ~(q1a > 0.0)
                w, var, ret = np.where(bad[None, :], NULL, w), np.where(bad, NULL, var), np.where(bad, NULL, ret)
            else:
                gam = (q1a - lam) / q11
                w = (y[1] - gam[None, :] * y[0]) / lam
                ret = (qaa - gam * q1a) / lam
                var = ((qaa - (2.0 * gam) * q1a) + (gam * gam) * q11) / (lam * lam)
    return nan_null(w), nan_null(var), nan_null(ret)
