"""Test-side restatement of decision D-18: IC decay, sub-period and sub-group robustness tests.

Independent of the HIP kernels: every daily IC comes from the CPU oracle's D-12 restatement (oracle.factor_ic, C) on shifted or masked
numpy arrays, which is what D-18 defines the rows to be.  The summary rows follow D-17's Fama-MacBeth rules with xsec_ref's sequential
sums, and p-values come from scipy.special.stdtr (xsec_regress_ref.t_pvalue), never from the device's formula.
"""
from __future__ import annotations

import math

import numpy as np

from xsec_ref import NULL, _seq, isnull, valid  # noqa: F401  (re-exported for the tests)
from xsec_regress_ref import t_pvalue


def _oracle():
    from oracle import pq_oracle
    return pq_oracle


def summary_row(x):
    """n_days, mean, std (ddof 1), t = mean / (std / sqrt(n_days)), p on n_days - 1 over the non-NaN entries of x (sums in order from
    0.0, two-pass std); mean NULL at 0 days, std / t / p NULL below 2 days or at std 0"""
    s, n, _ = _seq(x)
    m = s / n if n > 0 else 0.0
    ss = _seq(x, m)[0]
    sd = math.sqrt(ss / (n - 1)) if n >= 2 else 0.0
    if n < 2 or sd == 0.0:
        return [float(n), m if n > 0 else NULL, NULL, NULL, NULL]
    t = m / (sd / math.sqrt(n))
    return [float(n), m, sd, t, float(t_pvalue(t, n - 1))]


def summaries(rows):
    return np.array([summary_row(np.asarray(r, dtype=np.float64)) for r in rows], dtype=np.float64).reshape(-1, 5)


def ic_decay(factor, ret, max_lag, method=0):
    """-> ic [L, T], n_valid [L, T], summary [L, 5]: row l - 1 = D-12 IC of factor[:, :T - l + 1] vs ret[:, l - 1:], NULL / 0 beyond"""
    f = np.asarray(factor, dtype=np.float64)
    r = np.asarray(ret, dtype=np.float64)
    T = f.shape[1]
    ic = np.full((max_lag, T), NULL)
    nv = np.zeros((max_lag, T), np.int32)
    for l in range(1, max_lag + 1):
        m = T - l + 1
        if m <= 0:
            continue
        ic[l - 1, :m], nv[l - 1, :m] = _oracle().factor_ic(np.ascontiguousarray(f[:, :m]), np.ascontiguousarray(r[:, l - 1:]), method)
    return ic, nv, summaries(ic)


def group_codes(group, shape):
    g = np.asarray(group)
    return np.broadcast_to(g[:, None] if g.ndim == 1 else g, shape)


def ic_subgroup(factor, ret, group, method=0):
    """-> ic [G, T], n_valid [G, T], summary [G, 5]: row g = D-12 IC of where(code == g, factor, NaN) vs ret (G = max code + 1)"""
    f = np.asarray(factor, dtype=np.float64)
    r = np.asarray(ret, dtype=np.float64)
    codes = group_codes(group, f.shape)
    G = max(int(codes.max()) + 1 if codes.size else 1, 1)
    T = f.shape[1]
    ic = np.full((G, T), NULL)
    nv = np.zeros((G, T), np.int32)
    for g in range(G):
        if T:
            ic[g], nv[g] = _oracle().factor_ic(np.where(codes == g, f, np.nan), r, method)
    return ic, nv, summaries(ic)


def split_periods(T, n_splits):
    parts = np.array_split(np.arange(T), n_splits)
    return np.array([p[0] for p in parts], np.int64), np.array([p[-1] for p in parts], np.int64)


def series_split_summary(x, n_splits):
    x = np.asarray(x, dtype=np.float64)
    start, end = split_periods(len(x), n_splits)
    return summaries([x[a:b + 1] for a, b in zip(start, end)]) if n_splits else np.zeros((0, 5))
