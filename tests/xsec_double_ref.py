"""Test-side restatement of decision D-31 in numpy, built on tests/xsec_ref.py: the two-way (double) sort of a
control A and a factor B into Qa x Qb cells, independent or dependent, the cells' mean return / count / turnover, the two spread tables
and the summary rows.

The labels are D-15 applied twice (xsec_ref.label_day on masked copies), which is how the dependent rule is defined; the sums and the
sequential statistics are xsec_ref's own, so every value is exact integer arithmetic or a correctly rounded IEEE operation in the stated
order and the GPU results are compared bit for bit.
"""
from __future__ import annotations

import numpy as np

import xsec_ref as X

NULL, LABEL_OUT, LABEL_MID = X.NULL, X.LABEL_OUT, X.LABEL_MID


def sample(a, b, r):
    return X.valid(a) & X.valid(b) & X.valid(r)


def label_day(a, b, r, qa, qb, dependent):
    """one day: control a, factor b, return r [N] -> uint8 cell labels [N] (la * qb + lb, LABEL_MID, LABEL_OUT)"""
    a, b, r = (np.asarray(x, dtype=np.float64) for x in (a, b, r))
    ok = sample(a, b, r)
    n = int(ok.sum())
    out = np.full(a.shape[0], LABEL_OUT, dtype=np.uint8)
    if n < (qa if dependent else max(qa, qb)):
        return out
    la = X.label_day(np.where(ok, a, NULL), r, 0, qa)            # LABEL_OUT outside the sample
    if not dependent:
        lb = X.label_day(np.where(ok, b, NULL), r, 0, qb)
        out[ok] = la[ok] * qb + lb[ok]
        return out
    for g in range(qa):
        mem = la == g
        lb = X.label_day(np.where(mem, b, NULL), r, 0, qb)       # all LABEL_OUT where the bucket has fewer than qb members
        out[mem] = np.where(lb[mem] == LABEL_OUT, LABEL_MID, g * qb + lb[mem])
    return out


def labels(control, factor, ret, qa, qb, dependent, days=None):
    days = range(factor.shape[1]) if days is None else days
    return np.stack([label_day(control[:, t], factor[:, t], ret[:, t], qa, qb, dependent) for t in days], axis=1) if len(days) else \
        np.zeros((factor.shape[0], 0), dtype=np.uint8)


def _spread(mean, lo_rows, hi_rows):
    """rows hi - lo (NULL where either is) and, last, their sum in ascending row order from 0.0 over the row count (NULL where any is)"""
    D = mean.shape[1]
    k = len(lo_rows)
    out = np.full((k + 1, D), NULL)
    acc = np.zeros(D)
    full = np.ones(D, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (lo, hi) in enumerate(zip(lo_rows, hi_rows)):
            ok = ~X.isnull(mean[lo]) & ~X.isnull(mean[hi])
            v = np.where(ok, mean[hi] - mean[lo], NULL)
            out[i] = v
            acc = np.where(ok, acc + v, acc)
            full &= ok
        out[k] = np.where(full, acc / np.float64(k), NULL)
    return out


def groups(control, factor, ret, qa, qb, dependent, days=None):
    """D-31 per-day outputs on `days` (all when None) -> dict: labels [N, D], mean_return / count / turnover [qa * qb, D],
    spread_factor [qa + 1, D], spread_control [qb + 1, D]"""
    control, factor, ret = (np.asarray(x, dtype=np.float64) for x in (control, factor, ret))
    N, T = factor.shape
    C = qa * qb
    days = list(range(T)) if days is None else [int(t) for t in days]
    need = X.sample_days(days, T)
    col = {t: i for i, t in enumerate(need)}
    L = labels(control, factor, ret, qa, qb, dependent, need)
    cur = L[:, [col[t] for t in days]]
    prev = np.stack([L[:, col[t - 1]] if t > 0 else np.full(N, LABEL_OUT, np.uint8) for t in days], axis=1) if days else cur
    rr = ret[:, days]
    total, cnt, new = X.group_sums(cur, rr, C, prev)
    _, cnt_prev, _ = X.group_sums(prev, rr, C)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, total / np.maximum(cnt, 1), NULL)
        first = np.array([t == 0 for t in days], dtype=bool)[None, :]
        tov = np.where(~first & (cnt > 0) & (cnt_prev > 0), new / np.maximum(cnt, 1), NULL)
    sf = _spread(mean, [a * qb for a in range(qa)], [a * qb + qb - 1 for a in range(qa)])
    sc = _spread(mean, list(range(qb)), [(qa - 1) * qb + b for b in range(qb)])
    return {"labels": cur, "mean_return": mean, "count": cnt.astype(np.int32), "turnover": tov, "spread_factor": sf,
            "spread_control": sc}


def summary(res):
    """[C + qa + qb + 2, 5] from groups(...) over ALL days: the cells with their turnover, the spread_factor rows, the spread_control rows"""
    rows = [X.summary_row(m, t) for m, t in zip(res["mean_return"], res["turnover"])]
    rows += [X.summary_row(x) for x in res["spread_factor"]]
    rows += [X.summary_row(x) for x in res["spread_control"]]
    return np.array(rows, dtype=np.float64).reshape(-1, 5)
