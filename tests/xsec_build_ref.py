"""Test-side restatement of decision D-20 in numpy: the per-day rank, normalize and weighted columns and the
elementwise ratio and diff of [N, T] factors.

Independent of the HIP kernels: the ranks sort each day's members with np.sort and read the tie run of every key off the sorted values
with np.searchsorted, the weight sums are the explicit blocked loops of xsec_clean_ref.bsum (D-12: blocks of 256 symbols, members only,
ascending from 0.0, block sums in ascending order), zscore is xsec_clean_ref.clean itself, and every other step is an elementwise IEEE
operation in the stated order.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

import xsec_clean_ref as CR
from xsec_ref import NULL, isnull, valid  # noqa: F401  (re-exported for the tests)

RANK_MODES = ("rank", "pct", "quantile")
METHODS = ("zscore", "minmax", "quantile")


def rank_day(x, mode="rank", descending=False):
    """one day: x [N] -> [N]; the members are the valid entries, -0 ties with +0, the tie run of a key in the ascending sort is [a, b)
    and rank = ((a + 1) + b) / 2; descending: n + 1 - rank; "pct": / n; "quantile": (rank - 0.5) / n"""
    x = np.asarray(x, dtype=np.float64)
    mem = valid(x)
    out = np.full(x.shape, NULL)
    n = int(mem.sum())
    if n == 0:
        return out
    k = np.where(x[mem] == 0.0, 0.0, x[mem])
    S = np.sort(k)
    a = np.searchsorted(S, k, side="left").astype(np.float64)
    b = np.searchsorted(S, k, side="right").astype(np.float64)
    r = ((a + 1.0) + b) / 2.0
    if descending:
        r = (float(n) + 1.0) - r
    if mode == "pct":
        r = r / float(n)
    elif mode == "quantile":
        r = (r - 0.5) / float(n)
    out[mem] = r
    return out


def rank(factor, mode="rank", descending=False):
    f = np.asarray(factor, dtype=np.float64)
    if f.shape[1] == 0:
        return np.full(f.shape, NULL)
    return np.stack([rank_day(f[:, t], mode, descending) for t in range(f.shape[1])], axis=1)


def minmax(factor):
    """(x - min) / (max - min) over each day's members, -0 read as +0; the whole day NULL where max == min"""
    f = np.asarray(factor, dtype=np.float64)
    mem = valid(f)
    k = np.where(f == 0.0, 0.0, f)
    with np.errstate(all="ignore"):
        mn = np.where(mem, k, np.inf).min(axis=0, initial=np.inf)
        mx = np.where(mem, k, -np.inf).max(axis=0, initial=-np.inf)
        v = (k - mn) / (mx - mn)
    return np.where(mem & (mx != mn)[None, :], v, NULL)


def normalize(factor, method="zscore"):
    if method == "zscore":
        return CR.clean(factor, standardize=True)
    if method == "minmax":
        return minmax(factor)
    if method == "quantile":
        return rank(factor, "quantile")
    raise ValueError(method)


def weighted(factor, weight, group=None, n_groups=None):
    """(x w) / W: W the D-12 blocked sum of w over the day's members (factor and weight valid, and with group a code in [0, G)), per
    group with group; NULL outside the sample and where W == 0"""
    f, w = np.asarray(factor, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    N, D = f.shape
    mem = valid(f) & valid(w)
    with np.errstate(all="ignore"):
        if group is None:
            W = np.broadcast_to(CR.bsum(w, mem)[None, :], (N, D))
        else:
            g = np.asarray(group, dtype=np.int64)
            if g.ndim == 1:
                g = np.repeat(g[:, None], D, axis=1)
            if n_groups is None:
                n_groups = max(int(g.max()) + 1, 1) if g.size else 1
            mem &= (g >= 0) & (g < n_groups)
            Wg = np.zeros((n_groups, D))
            for c in range(n_groups):
                Wg[c] = CR.bsum(w, mem & (g == c))
            W = Wg[np.clip(g, 0, n_groups - 1), np.arange(D)[None, :]]
        v = (f * w) / W
    return np.where(mem & (W != 0.0), v, NULL)


def binary(a, b, op="ratio"):
    """op "ratio": a / b, "diff": a - b, "reldiff": (a - b) / |b|; NULL where either input is NULL, otherwise plain IEEE-754"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        v = a / b if op == "ratio" else (a - b if op == "diff" else (a - b) / np.abs(b))
    return np.where(isnull(a) | isnull(b), NULL, v)
