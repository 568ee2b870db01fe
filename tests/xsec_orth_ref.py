"""Test-side restatement of decision D-19 in numpy: multi-factor orthogonalization (sequential Gram-Schmidt) and
neutralization of K [N, T] factors, per day.

Independent of the HIP kernels: the blocked sums are xsec_clean_ref.bsum (explicit ascending loops over each block of 256 symbols,
members only), and the L D L^T factorisation, the substitutions and the residual are written out element by element in D-17's order
(tests/xsec_regress_ref.regress_units, which does not return the residual), vectorised over the days.  So the residuals are compared
bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum
from xsec_ref import NULL, isnull, valid  # noqa: F401  (isnull: re-exported for the tests)

MAX_K = 8
SINGULAR = 1e-12
MODES = ("orthogonalize", "neutralize")


def joint(F):
    """F [K, N, T] -> the per-day sample [N, T]: every factor non-null and finite"""
    mem = valid(F[0])
    for f in F[1:]:
        mem = mem & valid(f)
    return mem


def _residual(dr, df, b):
    """D-17's pass 3: e = dr - fit, fit = 0.0; fit += b_j df_j for ascending j"""
    fit = np.zeros_like(dr)
    for j in range(len(b)):
        fit = fit + b[j] * df[j]
    return dr - fit


def regress_residual(Fx, y, mem):
    """D-17 on days: regressors Fx [k, N, T], response y [N, T], sample mem [N, T] -> (e [N, T] before masking, ok [T]): the residual of
    y on the regressors with an intercept, and whether D-17 has coefficients (n >= k + 2, every pivot D_j > 1e-12 C[j][j])"""
    k = len(Fx)
    U = y.shape[1]
    n = mem.sum(axis=0)
    dn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        ybar = bsum(y, mem) / dn
        fbar = [bsum(Fx[j], mem) / dn for j in range(k)]
        dr = y - ybar
        df = [Fx[j] - fbar[j] for j in range(k)]
        Cm = [[bsum(df[j] * df[m], mem) if m <= j else None for m in range(k)] for j in range(k)]
        c = [bsum(df[j] * dr, mem) for j in range(k)]
        L = [[np.ones(U) if j == m else np.zeros(U) for m in range(k)] for j in range(k)]
        W = [[np.zeros(U) for _ in range(k)] for _ in range(k)]
        D = [None] * k
        ok = n >= k + 2
        for j in range(k):
            for m in range(j):
                w = Cm[j][m]
                for i in range(m):
                    w = w - W[j][i] * L[m][i]
                W[j][m] = w
                L[j][m] = w / D[m]
            d = Cm[j][j]
            for i in range(j):
                d = d - W[j][i] * L[j][i]
            D[j] = d
            ok &= d > SINGULAR * Cm[j][j]
        z = [None] * k
        for m in range(k):
            s = np.zeros(U)
            for i in range(m):
                s = s + L[m][i] * z[i]
            z[m] = c[m] - s
        b = [None] * k
        for j in range(k - 1, -1, -1):
            t = np.zeros(U)
            for m in range(j + 1, k):
                t = t + L[m][j] * b[m]
            b[j] = z[j] / D[j] - t
        e = _residual(dr, df, b)
    return e, ok


def orthogonalize(factors, method="orthogonalize"):
    """D-19: factors [K, N, T] (or a list of K [N, T]) -> [K - 1, N, T], row j the residual of factor j + 1: on factors 0 .. j
    (orthogonalize) or on factor 0 alone (neutralize), over the day's joint sample; NULL outside it and where D-17 has no coefficients"""
    assert method in MODES
    F = np.stack([np.asarray(f, dtype=np.float64) for f in factors])
    K = F.shape[0]
    assert 2 <= K <= MAX_K
    mem = joint(F)
    out = []
    for k in range(1, K):
        Fx = F[:k] if method == "orthogonalize" else F[:1]
        e, ok = regress_residual(Fx, F[k], mem)
        out.append(np.where(mem & ok[None, :], e, NULL))
    return np.stack(out)


def clean_full(factors, method="orthogonalize"):
    """Factor().clean's result: orthogonalize -> [K, N, T] (row 0 factor 0 unchanged), neutralize -> [K - 1, N, T]"""
    F = np.stack([np.asarray(f, dtype=np.float64) for f in factors])
    e = orthogonalize(F, method)
    return np.concatenate([F[:1], e]) if method == "orthogonalize" else e
