"""Test-side restatement of decision D-35 in numpy: the backtest of GIVEN target weights -- signed, not normalised,
NULL outside the day's universe, the remainder in cash -- with drift, turnover, a fee on the traded value, the first day of ruin and the
drifted holdings of one portfolio.

Independent of the HIP kernels: explicit loops over the rebalance days and over the days of a segment for the held price, the drifted
weights and the curve, in the definition's order, every cross-sectional sum D-12's blocked sum through xsec_clean_ref.bsum (blocks of 256 symbols, ascending from 0.0,
block sums ascending from 0.0), the chain a Python float loop.  Every value is a correctly rounded IEEE operation in the stated order, so
the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from xsec_clean_ref import bsum

NULL_BITS = 0x7FF80000504E554C
NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]
MAX_PORTFOLIOS = 8


def isnull(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) == np.uint64(NULL_BITS)


def valid(x):
    x = np.asarray(x, dtype=np.float64)
    return ~isnull(x) & np.isfinite(x)


def usable(x):
    """a price that can be held: non-null, finite and > 0"""
    with np.errstate(invalid="ignore"):
        return valid(x) & (np.asarray(x, dtype=np.float64) > 0.0)


def target(w):
    """a weight that is held: non-null, finite and != 0"""
    return valid(w) & (np.asarray(w, dtype=np.float64) != 0.0)


def check_days(days, T):
    days = [int(d) for d in days]
    if any(b <= a for a, b in zip(days, days[1:])):
        raise ValueError("rebalance days must be strictly ascending")
    if any(d < 0 or d >= T for d in days):
        raise ValueError("rebalance day outside [0, len)")
    return days


def blocked(terms, mem):
    """terms, mem [N, ...] -> [...]: D-12's blocked sum over the symbols, every trailing cell on its own (one walk of the blocks)"""
    shape = terms.shape[1:]
    return bsum(terms.reshape(terms.shape[0], -1), np.broadcast_to(mem, terms.shape).reshape(terms.shape[0], -1)).reshape(shape)


def weights(weights, price, rebalance_days, cost_rate=0.001, initial_capital=1_000_000.0, holdings_of=None):
    """weights: a list of P [N, R] arrays (or one [N, R] / [P, N, R] array), price f64 [N, T] -> {"value": [P, T], "turnover", "net",
    "gross": [P, R], "n_long", "n_short", "n_dropped": int32 [P, R], "first_nonpositive": int32 [P], "holdings": [N, T] (if asked)}"""
    price = np.asarray(price, dtype=np.float64)
    N, T = price.shape
    days = check_days(rebalance_days, T)
    R = len(days)
    if not isinstance(weights, (list, tuple)):
        weights = np.asarray(weights, dtype=np.float64)
        weights = [weights] if weights.ndim == 2 else list(weights)
    P = len(weights)
    if not 1 <= P <= MAX_PORTFOLIOS:
        raise ValueError("1..8 portfolios")
    W = np.stack([np.asarray(w, dtype=np.float64).reshape(N, R) for w in weights], axis=1)      # [N, P, R]
    c, c0 = float(cost_rate), float(initial_capital)
    if R == 0:                                                                                  # never invested: the capital, in cash
        out = {"value": np.full((P, T), c0), "turnover": np.zeros((P, 0)), "net": np.zeros((P, 0)), "gross": np.zeros((P, 0)),
               "n_long": np.zeros((P, 0), dtype=np.int32), "n_short": np.zeros((P, 0), dtype=np.int32),
               "n_dropped": np.zeros((P, 0), dtype=np.int32), "first_nonpositive": np.full(P, -1, dtype=np.int32)}
        if holdings_of is not None:
            out["holdings"] = np.zeros((N, T))
        return out
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # the rebalance days: targets, members, dropped; net, gross and the cash
        base = price[:, days]                                                                   # [N, R]
        tgt = target(W)
        mem = tgt & usable(base)[:, None, :]
        Wm = np.where(mem, W, 0.0)
        n_long, n_short, n_dropped = (mem & (Wm > 0.0)).sum(axis=0), (mem & (Wm < 0.0)).sum(axis=0), (tgt & ~mem).sum(axis=0)
        net, gross = blocked(Wm, mem), blocked(np.abs(Wm), mem)                                 # [P, R]
        cash = 1.0 - net
        # h(s, t) / price[s][d_k] on the days that segment k owns (d_k < t <= d_{k+1}, the last to T - 1): one walk per symbol and
        # day, shared by the portfolios
        seg = np.full(T, -1)
        ratio = np.ones((N, T))
        for k, d in enumerate(days):
            end = days[k + 1] if k + 1 < R else T - 1
            held = base[:, k].copy()
            for t in range(d + 1, end + 1):
                held = np.where(usable(price[:, t]), price[:, t], held)
                ratio[:, t] = held / base[:, k]                                                 # divide first, then multiply
                seg[t] = k
        own = seg >= 0
        ks = np.where(own, seg, 0)
        rel = np.where(mem[:, :, ks], Wm[:, :, ks] * ratio[:, None, :], 0.0)                    # [N, P, T]
        growth = np.where(own[None, :], cash[:, ks] + blocked(rel, mem[:, :, ks]), 1.0)         # [P, T]: c_k + L
        # turnover over ALL symbols against the weights of the rebalance before, drifted to d_k
        w_old = np.zeros((N, P, R))
        for k in range(1, R):
            d = days[k]
            w_old[:, :, k] = np.where(mem[:, :, k - 1], (Wm[:, :, k - 1] * ratio[:, None, d]) / growth[None, :, d], 0.0)
        turnover = blocked(np.abs(Wm - w_old), np.ones((N, 1, 1), dtype=bool)) if R else np.zeros((P, 0))
        # the chain and the curve, a Python float loop per portfolio
        value = np.full((P, T), c0)
        for p in range(P):
            B = c0
            for k, d in enumerate(days):
                end = days[k + 1] if k + 1 < R else T - 1
                Pk = c0 if k == 0 else B * float(growth[p, d])
                B = Pk * (1.0 - c * float(turnover[p, k]))
                value[p, d] = B
                for t in range(d + 1, end + 1):
                    if t < end or k + 1 == R:
                        value[p, t] = B * float(growth[p, t])
        first = np.array([int(np.nonzero(~(v > 0.0))[0][0]) if (~(v > 0.0)).any() else -1 for v in value], dtype=np.int32)
        out = {"value": value, "turnover": turnover, "net": net, "gross": gross, "n_long": n_long.astype(np.int32),
               "n_short": n_short.astype(np.int32), "n_dropped": n_dropped.astype(np.int32), "first_nonpositive": first}
        if holdings_of is not None:
            p = int(holdings_of)
            hold = np.where(own[None, :], rel[:, p, :] / growth[p][None, :], 0.0)               # (w (h / p0)) / G in between
            for k, d in enumerate(days):
                hold[:, d] = Wm[:, p, k]                                                        # the weight itself on d_k
            out["holdings"] = hold
    return out
