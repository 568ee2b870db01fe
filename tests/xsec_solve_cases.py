"""Shared inputs of the D-34 tests (tests/test_factor_solve_ref.py, tests/test_factor_solve_gpu.py): the hand-derived example, a dense
model for the comparison with numpy.linalg.solve, and panels with holes whose model is the risk entries' own output."""
from __future__ import annotations

import functools

import numpy as np

from xsec_ref import NULL

W = 8                                                        # the risk window of the panels' models


def hand():
    """Four symbols, K = 1, two industries, s^2 = (1/2, 1/2, 1/4, 1/4), an indefinite integer F; rhs: ones and alpha = (1, 2, -1, 0)"""
    x = np.array([[1.0], [2.0], [-1.0], [-1.0]])
    alpha = np.array([[1.0], [2.0], [-1.0], [0.0]])
    ind = np.array([0, 0, 1, 1], dtype=np.int32)
    F = np.array([[[-1.0, 1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0]]])
    sv = np.array([[0.5], [0.5], [0.25], [0.25]])
    return x, alpha, ind, F, sv


@functools.lru_cache(maxsize=None)
def dense(N, K, G, seed=0):
    """one day of a full model: F the sample covariance of 260 days of N(0, 0.01^2) returns, s in [0.01, 0.03], every industry present;
    -> (X [K, N, 1], alpha [N, 1], ind [N], F [1, M, M], sv [N, 1], B [N, M])"""
    rng = np.random.default_rng(100_000 * N + 1000 * K + G + seed)
    X = rng.normal(0.0, 1.0, (K, N, 1))
    ind = rng.integers(0, G, N).astype(np.int32)
    ind[:G] = np.arange(G)
    F = np.cov(rng.normal(0.0, 0.01, (260, K + G)).T).reshape(1, K + G, K + G)
    s = rng.uniform(0.01, 0.03, (N, 1))
    alpha = rng.normal(0.0, 1.0, (N, 1))
    B = np.concatenate([X[:, :, 0].T, np.eye(G)[ind]], axis=1)
    for a in (X, ind, F, alpha, B):
        a.setflags(write=False)
    return X, alpha, ind, F, s * s, B


@functools.lru_cache(maxsize=None)
def panel(N, K, G, codes, D, step=1, seed=0):
    """factor series [K + G, T] and specific returns [N, T] for a model of window W, exposures [K, N, T], two rhs columns a, b [N, T] and
    codes (None, "1d": [N], "2d": [N, T]); T holds D as-of days from day W - 1.  Holes: NULLs in every column, symbol 1 never has a
    variance, [N, T] codes leave [0, G) on a few cells."""
    rng = np.random.default_rng(1000 * N + 100 * K + G + D + seed)
    day0 = W - 1
    T = day0 + (D - 1) * step + 1
    M = K + G
    F = rng.normal(0.0, 0.01, (M, T))
    F[rng.random((M, T)) < 0.01] = NULL
    E = rng.normal(0.0, 0.02, (N, T))
    E[rng.random((N, T)) < 0.02] = NULL
    if N > 2:
        E[1] = NULL
    X = rng.normal(0.0, 1.0, (K, N, T))
    X[rng.random((K, N, T)) < 0.02] = NULL
    a = np.round(rng.normal(0.0, 1.0, (N, T)), 3)
    b = rng.normal(0.5, 1.0, (N, T))
    if N > 2:
        a[rng.random((N, T)) < 0.05] = NULL
        b[rng.random((N, T)) < 0.05] = NULL
        a[0, :] = np.where(np.arange(T) % 5 == 0, np.inf, a[0])
    ind = None
    if codes is not None:
        ind = (np.arange(N) % G).astype(np.int32)
        if codes == "2d":
            ind = np.repeat(ind[:, None], T, axis=1)
            r = rng.random((N, T))
            ind[r < 0.02] = -1
            ind[r > 0.98] = G
    for arr in (F, E, X, a, b, ind):
        if arr is not None:
            arr.setflags(write=False)
    return {"F": F, "E": E, "X": X, "a": a, "b": b, "ind": ind, "day0": day0, "T": T}
