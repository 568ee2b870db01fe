"""Inputs for the tests of decision D-32 (the weighted cross-sectional regression with industry dummies), shared by
tests/test_factor_wls_ref.py and tests/test_factor_wls_gpu.py: random panels with holes, and the constructed days that exercise one NULL
rule each."""
from __future__ import annotations

import numpy as np

from xsec_ref import NULL

# the constructed days; the first three have no solution, every other one solves
KINDS = ("short", "const", "collinear", "empty", "badw", "badcode", "perfect")
UNSOLVED = ("short", "const", "collinear")
SPECIAL_MIN_N = 64
H16 = np.array([[1.0]])
while H16.shape[0] < 16:                                     # Sylvester: rows 1 .. 15 have mean 0 and are mutually orthogonal
    H16 = np.block([[H16, H16], [H16, -H16]])


def panel(K, N, T, G, seed, holes=0.03, weights=True, codes="2d"):
    """-> F [K, N, T], r [N, T], w [N, T] or None, ind ([N] / [N, T] int32, or None with codes=None; then G must be 1).  r = an
    industry effect + sum_j 0.1 (j + 1) f_j + noise; holes: that share of NULL cells (and some NaN / inf) in every column, weights that
    are 0, negative, NaN and NULL, codes -1 and G"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, N, T))
    ind1 = rng.integers(0, G, N)
    ind = np.repeat(ind1[:, None], T, axis=1)
    if codes == "2d":                                        # some symbols change industry on some days
        move = rng.random((N, T)) < 0.1
        ind = np.where(move, rng.integers(0, G, (N, T)), ind)
    else:
        ind = ind1
    gam = 0.5 * rng.standard_normal(G)
    r = gam[ind if ind.ndim == 2 else ind[:, None]] + (0.1 * np.arange(1, K + 1)[:, None, None] * F).sum(0) + 0.5 * rng.standard_normal((N, T))
    w = np.exp(0.5 * rng.standard_normal((N, T))) if weights else None
    if holes:
        F[rng.random((K, N, T)) < holes / 2] = NULL
        F[rng.random((K, N, T)) < holes / 4] = np.nan
        r[rng.random((N, T)) < holes] = NULL
        r[rng.random((N, T)) < holes / 3] = np.inf
        if w is not None:
            for v in (0.0, -1.5, np.nan, NULL, np.inf):
                w[rng.random((N, T)) < holes / 3] = v
        for v in (-1, G, -2**31, 2**31 - 1):
            ind = np.where(rng.random(ind.shape) < holes / 3, v, ind)
    ind = ind.astype(np.int32)
    return F, r, w, (None if codes is None else ind)


def put_special(F, r, w, ind, G, day_of, seed):
    """overwrites day t = day_of[kind] of the panel (N >= 64, ind [N, T]; w may be None: the weights are then 1.0 and "badw" is not
    available) with a clean day of 2 .. 4 industries (codes s % min(G, 4)) that meets exactly one NULL rule:
      short      n = K + G_t: the first K + G_t symbols only                                   -> no solution
      const      f_0 = 0.5 * code, dyadic weights: constant inside every industry, C_00 = 0    -> no solution
      collinear  f_{K-1} = f_0 (K >= 2)                                                          -> no solution
      empty      industry 1 has no member (G >= 2): its rows NULL, G_t one less, the rest solved
      badw       weights 0, -1, NaN, NULL, +inf on symbols 0 .. 4: not members
      badcode    codes -1 and G on symbols 0, 1: not members
      perfect    16 symbols in each of min(G, 2) industries, f_j = a row of the 16 x 16 Hadamard matrix, weights 2.0,
                 r = g + sum_j b_j f_j on dyadic numbers: every sum is exact, SSE = 0, so t and p are NULL and coef is kept"""
    rng = np.random.default_rng(seed)
    K, N, _ = F.shape
    g2 = min(G, 4)
    code = np.arange(N) % g2
    for kind, t in day_of.items():
        F[:, :, t] = rng.standard_normal((K, N))
        r[:, t] = 0.3 * code + (0.1 * np.arange(1, K + 1)[:, None] * F[:, :, t]).sum(0) + 0.5 * rng.standard_normal(N)
        ind[:, t] = code
        if w is not None:
            w[:, t] = rng.choice([0.5, 1.0, 2.0], N)
        if kind == "short":
            r[K + g2:, t] = NULL
        elif kind == "const":
            F[0, :, t] = 0.5 * code
        elif kind == "collinear":
            assert K >= 2
            F[K - 1, :, t] = F[0, :, t]
        elif kind == "empty":
            assert G >= 2
            r[code == 1, t] = NULL
        elif kind == "badw":
            w[:5, t] = [0.0, -1.0, np.nan, NULL, np.inf]
        elif kind == "badcode":
            ind[0, t], ind[1, t] = -1, G
        elif kind == "perfect":
            s = np.arange(N)
            ind[:, t] = np.where(s < 16, 0, min(G, 2) - 1)
            r[32:, t] = NULL
            F[:, :, t] = H16[1:K + 1][:, s % 16]
            bj = 0.25 * np.arange(1, K + 1) - 1.0
            r[:32, t] = np.array([0.5, -1.5])[ind[:32, t]] + (bj[:, None] * F[:, :32, t]).sum(0)
            if w is not None:
                w[:, t] = 2.0
        else:
            raise KeyError(kind)


def kinds_for(K, G, weights):
    return [k for k in KINDS if not (k == "collinear" and K < 2) and not (k == "empty" and G < 2) and not (k == "badw" and not weights)]
