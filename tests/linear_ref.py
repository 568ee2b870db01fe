"""Test-side restatement of decision D-24 in numpy / scipy: linear(), the pooled OLS y = a + sum_j b_j x_j over all
rows of the columns, with its prediction and residual columns (csrc/xsec/linear.hip).

Independent of the HIP kernels.  The summation order is D-24's, written as array operations (psum): the logical rows (an [N, T] column
is its reshape(-1)) in tiles of TILE = 4096; inside a tile lane l of 256 adds rows l + 256 i, i = 0 .. 15 ascending, from +0.0 -- a row
that is no member adds +0.0 --; the 256 lane sums fold by halving inside each group of 64 (v[l] + v[l + o], o = 32 .. 1) and the four
group sums as (w0 + w2) + (w1 + w3); the tile partials are summed the same way, lane l taking partials l + 256 i.  The L D L^T
factorisation, the substitutions and the standard errors are D-17's element by element (xsec_regress_ref.py states them vectorised
over its units and has no solve of its own to import; its forward substitution is used).  So coef / t / R^2 / n / pred / resid are
compared bit for bit; p-values come from scipy.special.stdtr, never from the device's formula.
"""
from __future__ import annotations

import numpy as np

from xsec_ref import NULL, isnull, valid  # noqa: F401  (isnull: re-exported for the tests)
from xsec_regress_ref import SINGULAR, _forward, t_pvalue

MAX_K = 8
LANES = 256                # lanes of a tile
ROWS = 16                  # rows per lane and tile
TILE = LANES * ROWS        # api.LINEAR_TILE
STAGE2 = LANES             # api.LINEAR_STAGE2


def _fold(v):
    """the fixed tree over the last axis of 256 lane sums"""
    v = v.reshape(v.shape[:-1] + (4, 64))
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    w = v[..., 0]
    return (w[..., 0] + w[..., 2]) + (w[..., 1] + w[..., 3])


def _lane_sums(z, per):
    """z [m] -> [ceil(m / per / 256) or 1, 256]: lane l of group g adds z[g per 256 + l + 256 i], i = 0 .. per - 1 ascending, from +0.0"""
    g = max(1, -(-z.size // (per * LANES)))
    buf = np.zeros(g * per * LANES)
    buf[:z.size] = z
    buf = buf.reshape(g, per, LANES)
    a = np.zeros((g, LANES))
    for i in range(per):
        a = a + buf[:, i, :]
    return a


def psum(terms, mem):
    """D-24's sum of terms [M] over the members mem [M] -> f64 scalar"""
    with np.errstate(all="ignore"):
        z = np.where(mem, terms, 0.0).reshape(-1)
    part = _fold(_lane_sums(z, ROWS))                        # one partial per tile
    steps = max(1, -(-part.size // STAGE2))
    return _fold(_lane_sums(part, steps)[0])


def linear(xs, y):
    """xs: K columns (a list, or one [K, ...] array), y: a column, all [M] or [N, T] -> dict: coef / t / p [K + 1] (slopes first, the
    intercept last), r2 (f64 scalar), n (int), pred / resid in y's shape"""
    y = np.asarray(y, dtype=np.float64)
    shape = y.shape
    yv = y.reshape(-1)
    X = [np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]
    K = len(X)
    assert 1 <= K <= MAX_K and all(x.shape == yv.shape for x in X)
    xok = np.ones(yv.shape, dtype=bool)
    for x in X:
        xok &= valid(x)
    mem = xok & valid(yv)
    n = int(mem.sum())
    f = np.float64
    nul = np.full(K + 1, NULL)
    none = {"coef": nul, "t": nul.copy(), "p": nul.copy(), "r2": f(NULL), "n": n, "pred": np.full(shape, NULL), "resid": np.full(shape, NULL)}
    with np.errstate(all="ignore"):
        dn = f(n)
        cols = X + [yv]                                      # the K + 1 columns of the triangle: x_0 .. x_{K-1}, y
        mean = [psum(c, mem) / dn for c in cols]
        d = [c - m for c, m in zip(cols, mean)]
        S = [[psum(d[j] * d[l], mem) for l in range(j + 1)] for j in range(K + 1)]
        Cm, c, syy = S, S[K][:K], S[K][K]
        # C = L D L^T by rows; W[j][k] = the numerator of L[j][k]
        L = [[f(1.0) if j == k else f(0.0) for k in range(K)] for j in range(K)]
        W = [[f(0.0) for _ in range(K)] for _ in range(K)]
        D = [None] * K
        ok = n >= K + 2
        for j in range(K):
            for k in range(j):
                w = Cm[j][k]
                for m in range(k):
                    w = w - W[j][m] * L[k][m]
                W[j][k] = w
                L[j][k] = w / D[k]
            dj = Cm[j][j]
            for m in range(j):
                dj = dj - W[j][m] * L[j][m]
            D[j] = dj
            ok = ok and bool(dj > SINGULAR * Cm[j][j])
        if not ok:
            return none
        z = _forward(L, c)
        b = [None] * K
        for j in range(K - 1, -1, -1):
            t = f(0.0)
            for m in range(j + 1, K):
                t = t + L[m][j] * b[m]
            b[j] = z[j] / D[j] - t
        sa = f(0.0)
        for j in range(K):
            sa = sa + b[j] * mean[j]
        a = mean[K] - sa
        V = []
        for j in range(K):
            w = _forward(L, [f(1.0 if m == j else 0.0) for m in range(K)])
            vj = f(0.0)
            for m in range(K):
                vj = vj + w[m] * w[m] / D[m]
            V.append(vj)
        w = _forward(L, mean[:K])
        q = f(0.0)
        for m in range(K):
            q = q + w[m] * w[m] / D[m]
        V.append(f(1.0) / dn + q)
        p = np.full(yv.shape, a)
        for j in range(K):
            p = p + b[j] * X[j]
        e = yv - p
        sse = psum(e * e, mem)
        dof = f(n - K - 1)
        s2 = sse / dof
        coef = np.array(b + [a], dtype=np.float64)
        se = np.sqrt(s2 * np.array(V, dtype=np.float64))
        tt = np.where(se == 0.0, NULL, coef / se)
        pp = np.where(se == 0.0, NULL, t_pvalue(tt, dof))
        r2 = f(1.0) - sse / syy if syy != 0.0 else f(NULL)
        pred = np.where(xok, p, NULL).reshape(shape)
        resid = np.where(mem, e, NULL).reshape(shape)
    return {"coef": coef, "t": tt, "p": pp, "r2": r2, "n": n, "pred": pred, "resid": resid}
