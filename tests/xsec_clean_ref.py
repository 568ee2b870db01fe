"""Test-side restatement of decision D-16 in numpy: per-day winsorize, size neutralization, industry
neutralization and standardize of an [N, T] factor.

Independent of the HIP kernels: the order statistics sort each day's members with np.sort and read the stated formulas off the sorted
values (the MAD sorts the deviations a second time), the blocked cross-sectional sums are explicit ascending loops over the symbols of
each block of 256 (vectorised over days and blocks, members only), and every other step is an elementwise IEEE operation in the stated
order.  So the GPU results are compared bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from xsec_ref import BLOCK, NULL, isnull, valid  # noqa: F401  (isnull: re-exported for the tests)

WINSORIZE = {None: 0, "mad": 1, "sigma": 2, "percentile": 3}
MAD_SCALE = 1.4826
INF = float("inf")


def bsum(v, mem):
    """D-12 blocked sum over the members of each column: v, mem [N, D] -> [D].  Blocks of 256 symbol indices, ascending inside a
    block from 0.0, block sums added in ascending block order from 0.0."""
    v = np.asarray(v, dtype=np.float64)
    N, D = v.shape
    nb = max(1, -(-N // BLOCK))
    pad = nb * BLOCK - N
    vv = np.concatenate([v, np.zeros((pad, D))]).reshape(nb, BLOCK, D)
    mm = np.concatenate([np.asarray(mem, dtype=bool), np.zeros((pad, D), dtype=bool)]).reshape(nb, BLOCK, D)
    blk = np.zeros((nb, D))
    with np.errstate(all="ignore"):
        for j in range(BLOCK):
            blk = np.where(mm[:, j], blk + vv[:, j], blk)
        total = np.zeros(D)
        for k in range(nb):
            total = total + blk[k]
    return total


def median_sorted(S):
    n = len(S)
    return float(S[(n - 1) // 2]) if n % 2 else (float(S[n // 2 - 1]) + float(S[n // 2])) * 0.5


def quantile_sorted(S, q):
    """numpy's "linear" method in the D-16 order: h = q (n - 1), i = floor(h), g = h - i, S[i] + g (S[i+1] - S[i]) unless g == 0"""
    h = q * float(len(S) - 1)
    i = math.floor(h)
    g = h - float(i)
    return float(S[i]) if g == 0.0 else float(S[i]) + g * (float(S[i + 1]) - float(S[i]))


def order_bounds(x, winsorize, winsorize_n):
    """one day's members x (1-D) -> dict(med, mad, lo, hi) for "mad", (lo, hi) for "percentile"; -inf / +inf when not clipped"""
    x = np.asarray(x, dtype=np.float64)
    S = np.sort(np.where(x == 0.0, 0.0, x))          # -0 is read as +0
    out = {"lo": -INF, "hi": INF}
    if len(S) < 2:
        return out
    if winsorize == "percentile":
        p = winsorize_n / 100.0
        out["lo"], out["hi"] = quantile_sorted(S, p), quantile_sorted(S, 1.0 - p)
        return out
    med = median_sorted(S)
    mad = median_sorted(np.sort(np.abs(S - med)))
    out["med"], out["mad"] = med, mad
    if mad != 0.0:
        c = winsorize_n * MAD_SCALE
        out["lo"], out["hi"] = med - c * mad, med + c * mad
    return out


def members(factor, z=None, industry=None, n_industries=None):
    m = valid(factor)
    if z is not None:
        m &= valid(z)
    if industry is not None:
        m &= (industry >= 0) & (industry < n_industries)
    return m


def clean(factor, winsorize=None, winsorize_n=None, z=None, industry=None, n_industries=None, standardize=False, parts=False):
    """D-16 on [N, D] columns (every day is independent, so any subset of days may be passed).  z: the regressor as the C entry point
    receives it (already logged); industry: int codes [N, D] (or [N]), unclassified outside [0, n_industries) (default max + 1).
    -> out [N, D] (with parts=True: a dict of the per-day intermediates as well)"""
    f = np.asarray(factor, dtype=np.float64)
    N, D = f.shape
    if winsorize_n is None:
        winsorize_n = {None: 0.0, "mad": 3.0, "sigma": 3.0, "percentile": 1.0}[winsorize]
    if industry is not None:
        industry = np.asarray(industry, dtype=np.int64)
        if industry.ndim == 1:
            industry = np.repeat(industry[:, None], D, axis=1)
        if n_industries is None:
            n_industries = max(int(industry.max()) + 1, 1) if industry.size else 1
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
    mem = members(f, z, industry, n_industries)
    n = mem.sum(axis=0)
    dn = n.astype(np.float64)
    info = {"n": n}
    with np.errstate(all="ignore"):
        lo, hi = np.full(D, -INF), np.full(D, INF)
        if winsorize in ("mad", "percentile"):
            for t in range(D):
                b = order_bounds(f[mem[:, t], t], winsorize, winsorize_n)
                lo[t], hi[t] = b["lo"], b["hi"]
        elif winsorize == "sigma":
            m0 = bsum(f, mem) / dn
            d0 = f - m0
            sd0 = np.sqrt(bsum(d0 * d0, mem) / (dn - 1.0))
            lo, hi = m0 - winsorize_n * sd0, m0 + winsorize_n * sd0
        info["lo"], info["hi"] = lo, hi
        x = np.where(f < lo, lo, f)
        x = np.where(x > hi, hi, x)
        e = x
        if z is not None:
            xbar, zbar = bsum(x, mem) / dn, bsum(z, mem) / dn
            dz = z - zbar
            sxz, szz = bsum((x - xbar) * dz, mem), bsum(dz * dz, mem)
            beta = np.where(szz == 0.0, 0.0, sxz / np.where(szz == 0.0, 1.0, szz))
            e = (x - xbar) - beta * (z - zbar)
            info["beta"] = beta
        if industry is not None:
            gmean = np.zeros((n_industries, D))
            for g in range(n_industries):
                mg = mem & (industry == g)
                cg = mg.sum(axis=0)
                gmean[g] = np.where(cg > 0, bsum(e, mg) / np.maximum(cg, 1).astype(np.float64), NULL)
            gi = np.clip(industry, 0, n_industries - 1)
            e = e - gmean[gi, np.arange(D)[None, :]]
            info["gmean"] = gmean
        dead = n < 2
        if standardize:
            sm = bsum(e, mem) / dn
            de = e - sm
            ss = np.sqrt(bsum(de * de, mem) / (dn - 1.0))
            e = (e - sm) / ss
            dead = dead | (ss == 0.0)
        out = np.where(mem & ~dead[None, :], e, NULL)
    return (out, info) if parts else out
