"""Test-side restatement of decision D-30 in numpy: the combination weights of K factors from the trailing window
of their IC series (ic / icir / max_icir) and the composite, the weighted sum of the K factors per (symbol, day).

Independent of the HIP kernels: every sum is an explicit loop over the window offset (or over k) that starts at 0.0 and adds whole arrays
in ascending order (never np.sum / np.mean / np.std / np.cov / np.linalg, whose order differs), the L D L^T solve is written element by
element in D-17's order (as tests/xsec_regress_ref.py does), and every other step is one elementwise IEEE operation in the stated order.
So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)
from xsec_rolling_ref import shift, window_all, window_sum
from xsec_ts_ref import day, sq_dev

METHODS = ("ic", "icir", "max_icir")
MAX_K = 8
MAX_WINDOW = MAX_LAG = 1024
SINGULAR = 1e-12


def min_window(method, K):
    return {"ic": 1, "icir": 2, "max_icir": K + 1}[method]


def weights(ic, method, window, lag):
    """ic [K, T] (or [T]) -> w [K, T]: the weights of day t from the days t - lag - window + 1 .. t - lag"""
    ic = np.asarray(ic, dtype=np.float64)
    ic = ic.reshape(1, -1) if ic.ndim == 1 else ic
    K, T = ic.shape
    w = int(window)
    assert method in METHODS and 1 <= K <= MAX_K and min_window(method, K) <= w <= MAX_WINDOW and 0 <= lag <= MAX_LAG
    dw = float(w)
    late = shift(ic, int(lag), NULL)                            # late[:, t] = ic[:, t - lag]: row t is the plain trailing window of `late`
    ok = ~isnull(late)
    full = window_all(ok.all(axis=0, keepdims=True), w)         # [1, T]: all K * window values
    v = np.where(ok, late, 0.0)
    with np.errstate(all="ignore"):
        m = [window_sum(v[k:k + 1], w) / dw for k in range(K)]
        if method == "ic":
            r = m
        elif method == "icir":
            sd = [np.sqrt(sq_dev(v[k:k + 1], m[k], w) / float(w - 1)) for k in range(K)]
            for k in range(K):
                full = full & (sd[k] > 0.0)
            r = [m[k] / sd[k] for k in range(K)]
        else:
            Cm = [[np.zeros((1, T)) if l <= j else None for l in range(K)] for j in range(K)]
            for i in range(w):
                dv = [day(v[k:k + 1], w, i) - m[k] for k in range(K)]
                for j in range(K):
                    for l in range(j + 1):
                        Cm[j][l] = Cm[j][l] + dv[j] * dv[l]
            dof = float(w - 1)
            Cm = [[Cm[j][l] / dof if l <= j else None for l in range(K)] for j in range(K)]
            # C = L D L^T by rows; W[j][k] = the numerator of L[j][k] (xsec_regress_ref.regress_units, without the intercept)
            L = [[np.ones((1, T)) if j == k else np.zeros((1, T)) for k in range(K)] for j in range(K)]
            W = [[np.zeros((1, T)) for _ in range(K)] for _ in range(K)]
            D = [None] * K
            for j in range(K):
                for k in range(j):
                    x = Cm[j][k]
                    for q in range(k):
                        x = x - W[j][q] * L[k][q]
                    W[j][k] = x
                    L[j][k] = x / D[k]
                d = Cm[j][j]
                for q in range(j):
                    d = d - W[j][q] * L[j][q]
                D[j] = d
                full = full & (d > SINGULAR * Cm[j][j])
            z = [None] * K
            for q in range(K):
                s = np.zeros((1, T))
                for i in range(q):
                    s = s + L[q][i] * z[i]
                z[q] = m[q] - s
            r = [None] * K
            for j in range(K - 1, -1, -1):
                t = np.zeros((1, T))
                for q in range(j + 1, K):
                    t = t + L[q][j] * r[q]
                r[j] = z[j] / D[j] - t
        r = np.concatenate(r, axis=0)
        full = full & ~np.isnan(r).any(axis=0, keepdims=True)
    return np.where(full, r, NULL)


def composite(factors, w, normalize=True):
    """factors [K, N, T] (or a list of K [N, T]), w [K, T] (or [K]: the same on every day) -> [N, T]"""
    F = np.asarray(factors, dtype=np.float64)
    K, N, T = F.shape
    w = np.asarray(w, dtype=np.float64)
    w = np.repeat(w.reshape(K, 1), T, axis=1) if w.ndim == 1 else w
    assert w.shape == (K, T)
    ok = ~np.isnan(w).any(axis=0)                               # NULL is a NaN
    with np.errstate(all="ignore"):
        D = np.zeros(T)
        for k in range(K):
            D = D + np.abs(w[k])
        if normalize:
            ok = ok & (D != 0.0)
        mem = np.broadcast_to(ok, (N, T)).copy()
        acc = np.zeros((N, T))
        for k in range(K):
            mem &= valid(F[k])
            acc = acc + w[k] * F[k]
        r = acc / D if normalize else acc
    return np.where(mem & ~np.isnan(r), r, NULL)
