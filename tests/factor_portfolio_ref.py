"""Test-side restatement of decision D-27 in numpy: the value curves, turnover and member counts of group
portfolios that are re-formed on given rebalance days, hold their members in between (every holding drifts with its price) and pay a
fee on the traded value.

Independent of the HIP kernels: the cross-sectional sums are explicit loops over blocks of 256 symbols and, inside a block, over
ascending symbols from 0.0 (vectorised over the days of a segment only), the blocks are added in ascending order from 0.0, and the
chain over the rebalance days is a Python float loop.  Every value is a correctly rounded IEEE operation in the stated order, so the
GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

NULL_BITS = 0x7FF80000504E554C
NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]
LABEL_OUT, LABEL_MID = 255, 254
BLOCK = 256


def isnull(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64) == np.uint64(NULL_BITS)


def valid(x):
    x = np.asarray(x, dtype=np.float64)
    return ~isnull(x) & np.isfinite(x)


def usable(x):
    """non-null, finite and > 0: a price that can be held, a weight that counts"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return valid(x) & (x > 0.0)


def block_sum(terms):
    """terms [N, ...] -> [...]: blocks of 256 rows, ascending rows inside a block from 0.0, blocks added in ascending order from 0.0"""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.zeros(terms.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, terms.shape[0], BLOCK):
            blk = np.zeros(terms.shape[1:])
            for s in range(b0, min(b0 + BLOCK, terms.shape[0])):
                blk = blk + terms[s]
            total = total + blk
    return total


def check_days(days, T, label_lag):
    days = [int(d) for d in days]
    if any(b <= a for a, b in zip(days, days[1:])):
        raise ValueError("rebalance days must be strictly ascending")
    if any(d < label_lag or d >= T for d in days):
        raise ValueError("rebalance day outside [label_lag, len)")
    return days


def portfolio(labels, price, n_groups, rebalance_days, weight=None, label_lag=0, cost_rate=0.0, initial_capital=1_000_000.0):
    """labels uint8 [N, T], price (and weight) f64 [N, T] -> {"value": [G, T], "turnover": [G, R], "count": int32 [G, R]}"""
    labels = np.asarray(labels, dtype=np.uint8)
    price = np.asarray(price, dtype=np.float64)
    N, T = price.shape
    G = int(n_groups)
    days = check_days(rebalance_days, T, label_lag)
    R = len(days)
    c, c0 = float(cost_rate), float(initial_capital)
    value = np.full((G, T), c0)
    turnover = np.zeros((G, R))
    count = np.zeros((G, R), dtype=np.int32)
    gcol = np.arange(G)[None, :]
    B = [c0] * G                      # B_{k-1} per group
    prev = None                       # the segment before: in-group flags, weights, base prices, growth and held price on its last day
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k, d in enumerate(days):
            end = days[k + 1] if k + 1 < R else T - 1
            lab = labels[:, d - label_lag].astype(np.int64)
            p0 = price[:, d]
            mem = (lab < G) & usable(p0)
            a = np.ones(N)
            if weight is not None:
                a = np.asarray(weight, dtype=np.float64)[:, d]
                mem &= usable(a)
            ing = mem[:, None] & (lab[:, None] == gcol)                      # [N, G]
            count[:, k] = ing.sum(axis=0)
            A = block_sum(np.where(ing, a[:, None], 0.0))                    # [G]
            w = np.where(mem, a / A[np.where(mem, lab, 0)], 0.0)             # [N]
            # turnover against the drifted weights of the segment before
            w_new = np.where(ing, w[:, None], 0.0)
            w_old = np.zeros((N, G))
            if prev is not None:
                drift = prev["w"] * (prev["held"] / prev["p0"])              # divide first, then multiply
                w_old = np.where(prev["ing"], (drift[:, None] / prev["growth"][None, :]), 0.0)
            tau = block_sum(np.abs(w_new - w_old))                           # [G]
            turnover[:, k] = tau
            for g in range(G):
                P = c0 if k == 0 else B[g] * float(prev["growth"][g])
                B[g] = P * (1.0 - c * float(tau[g]))
                value[g, d] = B[g]
            # the days the segment owns: d < t <= end
            held = p0.copy()
            growth = np.ones(G)
            for t in range(d + 1, end + 1):
                held = np.where(usable(price[:, t]), price[:, t], held)
                rel = w * (held / p0)
                growth = np.where(count[:, k] > 0, block_sum(np.where(ing, rel[:, None], 0.0)), 1.0)
                if t < end or k + 1 == R:
                    for g in range(G):
                        value[g, t] = B[g] * float(growth[g])
            prev ={"ing": ing, "w": w, "p0": p0, "held": held, "growth": growth}
    return {"value": value, "turnover": turnover, "count": count}
