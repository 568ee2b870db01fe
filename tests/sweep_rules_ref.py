"""Test-side scalar restatement of ONE cell of pq_backtest_sweep_rules (csrc/sweep/sweep.hip, decision D-25) for all seven rules, and the
shared inputs and oracle reference of test_sweep_rules_ref.py (CPU) and test_sweep_rules_gpu.py.

The restatement evaluates the rule row by row on plain Python floats (`rule_signals`) and runs the scan and the two summary walks of
tests/sweep_ref.py on the result.  It is independent of the HIP kernels and of the C oracle.

The reference (`oracle_signals`, `oracle_cells`) is the C oracle: oracle.cross_signals / band_signals / channel_signals, the gates and the
scale as plain numpy comparisons, and oracle.backtest for the summary.
"""
from __future__ import annotations

import struct

import numpy as np

import sweep_ref as R

CROSS, BAND, CHANNEL, BREAKOUT, SCALED, ZONES, STRENGTH = range(7)
USES_B = (CROSS, CHANNEL, BREAKOUT, ZONES, STRENGTH)
USES_C = (CHANNEL, BREAKOUT, SCALED, ZONES, STRENGTH)
NULL_BITS = 0x7FF80000504E554C                                        # include/pq_hip.h PQ_NULL_BITS
NULL = struct.unpack("<d", struct.pack("<Q", NULL_BITS))[0]
EXACT, TOL = (1, 5, 6, 7), (0, 2, 3, 4)                                # test_backtest_wave_gpu.check_summary


def is_null(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] == NULL_BITS


def rule_signals(rule, la, lb, lc, k0, k1):
    """la, lb, lc: T floats each (lines[a], lines[b], col[c]) -> (buy, sell): two lists of T bools; row 0 never signals"""
    T = len(la)
    buy, sell = [False] * T, [False] * T
    if rule == SCALED:      # one rounded multiply each, NULL where the base is; then the channel
        lo = [x if is_null(x) else x * k0 for x in la]
        hi = [x if is_null(x) else x * k1 for x in la]
    else:
        lo, hi = la, lb
    for i in range(1, T):
        a0, a1, b0, b1, c0, c1 = la[i - 1], la[i], lb[i - 1], lb[i], lc[i - 1], lc[i]
        if rule == BAND:
            buy[i], sell[i] = a0 < k0 and a1 >= k0, a0 > k1 and a1 <= k1
        elif rule in (CHANNEL, SCALED):
            # a NULL anywhere refuses both sides; a non-NULL NaN only fails the comparisons it takes part in
            if any(is_null(x) for x in (c1, c0, lo[i], hi[i], lo[i - 1], hi[i - 1])):
                continue
            buy[i], sell[i] = c1 < lo[i] and c0 >= lo[i - 1], c1 > hi[i] and c0 <= hi[i - 1]
        elif rule == BREAKOUT:
            if is_null(c1) or is_null(lo[i - 1]) or is_null(hi[i - 1]):
                continue
            buy[i], sell[i] = c1 > hi[i - 1], c1 < lo[i - 1]
        else:               # cross (a NULL is a NaN: it compares false), alone or gated by col[c] of the row
            b, s = a0 <= b0 and a1 > b1, a0 >= b0 and a1 < b1
            if rule == ZONES:
                b, s = b and c1 < k0, s and c1 > k1
            elif rule == STRENGTH:
                b, s = b and c1 > k0, s and c1 > k0
            buy[i], sell[i] = b, s
    return buy, sell


def sweep_rule_cell(price, la, lb, lc, rule, k0=0.0, k1=0.0, bench=None, **costs):
    """the 8 summary values of one (symbol, parameter set): rule_signals, then the scan and the two walks of sweep_ref.sweep_cell.

    sweep_ref's lane evaluates its own cross rule inside `step`; the lane below hands that rule two values per row which make it take
    exactly the precomputed decision (a row with both signals buys from a flat position and sells from a long one -- what the scan does
    with both set), so sweep_ref.sweep_cell runs unedited."""
    f = lambda xs: [float(x) for x in xs]
    buy, sell = rule_signals(int(rule), f(la), f(lb), f(lc), float(k0), float(k1))

    class Lane(R._Lane):
        def __init__(self, c):
            super().__init__(c)
            self.t = 0

        def step(self, c, _rule, _k0, _k1, _xa, _xb, px):
            b, s = buy[self.t], sell[self.t]
            self.t += 1
            if b and s:
                b, s = self.pos == 0.0, self.pos > 0.0
            self.pa = self.pb = 0.0
            return super().step(c, 0, 0.0, 0.0, 1.0 if b else 0.0, 1.0 if s else 0.0, px)

    saved, R._Lane = R._Lane, Lane
    try:
        return R.sweep_cell(price, [0.0] * len(price), [0.0] * len(price), 0, bench=bench, **costs)
    finally:
        R._Lane = saved


# ---- the oracle reference -------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_signals(oracle, price, lines, q):
    """the [N, T] buy / sell columns of one parameter set (a row of a SWEEP_RULE_DTYPE table) from the oracle's rule functions"""
    rule, k0, k1 = int(q["rule"]), float(q["k0"]), float(q["k1"])
    a = lines[q["a"]]
    b = lines[q["b"]] if rule in USES_B else None
    c = (price if q["c"] < 0 else lines[q["c"]]) if rule in USES_C else None
    if rule == BAND:
        return oracle.band_signals(a, k0, k1)
    if rule in (CHANNEL, BREAKOUT):
        return oracle.channel_signals(c, a, b, rule - CHANNEL)
    if rule == SCALED:
        null = bits(a) == NULL_BITS
        return oracle.channel_signals(c, np.where(null, a, a * k0), np.where(null, a, a * k1), 0)
    buy, sell = oracle.cross_signals(a, b)
    with np.errstate(invalid="ignore"):
        if rule == ZONES:
            buy, sell = buy & (c < k0), sell & (c > k1)
        elif rule == STRENGTH:
            buy, sell = buy & (c > k0), sell & (c > k0)
    return buy.astype(np.uint8), sell.astype(np.uint8)


def rule_key(q):
    rule = int(q["rule"])
    return (rule, int(q["a"]), int(q["b"]) if rule in USES_B else -9, int(q["c"]) if rule in USES_C else -9,
            float(q["k0"]) if rule not in (CROSS, CHANNEL, BREAKOUT) else 0.0, float(q["k1"]) if rule in (BAND, SCALED, ZONES) else 0.0)


def oracle_cells(oracle, price, lines, tab, benchmark=None, **costs):
    """-> [P, N, 8]: the oracle's summary of every parameter set (equal sets are computed once)"""
    memo = {}
    out = []
    for q in tab:
        key = rule_key(q)
        if key not in memo:
            memo[key] = oracle.backtest(price, *oracle_signals(oracle, price, lines, q), benchmark=benchmark, **costs)[3].reshape(price.shape[0], 8)
        out.append(memo[key])
    return np.stack(out)


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------
def near_price(j, L):
    """lines come in two families: j % 7 < 4 moves around the price (channels, crosses), the others around 50 (bands, gates)"""
    return j % 7 < 4


def make_lines(close, L):
    """L columns for the [N, T] close: the price family is close x (1 + a few percent of a slow wave), so the price and these lines cross
    each other often; the other family oscillates around 50 like test_sweep_gpu.make_lines"""
    N, T = close.shape
    t = np.arange(T, dtype=np.float64)[None, :]
    n = np.arange(N, dtype=np.float64)[:, None]
    base = np.where(np.isfinite(close) & (close > 0), close, 50.0)
    out = []
    for j in range(L):
        if near_price(j, L):
            out.append(base * (1.0 + 0.004 * (j % 5 - 2) + 0.03 * np.sin(0.9 / (1.0 + 0.37 * (j % 11)) * t + 1.3 * j + 0.7 * n)))
        else:
            out.append(50.0 + 30.0 * np.sin(0.9 / (1.0 + 0.37 * (j % 11)) * t + 1.3 * j + 0.7 * n) + 5.0 * np.cos(0.31 * t * (1 + j % 3) + n))
    return out


def add_nulls(lines, N):
    """NULL lead-ins of different lengths (an indicator's warm-up) and interior NULLs, in place"""
    for j, l in enumerate(lines):
        l[:, : 3 * (j % 9) + (j % 2)] = NULL
        l[j % N, 100 + (j % 40): 104 + (j % 40) + 2 * (j % 5)] = NULL
    return lines


def make_table(dtype, P, L, rule=None):
    """P parameter sets over L >= 7 lines: all seven rules mixed inside every wavefront (rule=None) or one rule throughout; c = -1 and
    c >= 0 both occur under every rule that reads c; a field a rule does not use holds an index far out of range"""
    pf = [j for j in range(L) if near_price(j, L)]
    of = [j for j in range(L) if not near_price(j, L)]
    tab = np.zeros(P, dtype=dtype)
    for i in range(P):
        r = i % 7 if rule is None else rule
        u = i // 7 if rule is None else i
        q = tab[i]
        q["rule"] = r
        q["b"] = q["c"] = 10 ** 6                          # unused unless set below
        if r == CROSS:
            fam, v = (pf, u // 2) if u % 2 == 0 else (of, u // 2)
            q["a"], q["b"] = fam[v % len(fam)], fam[(v // len(fam) + 1) % len(fam)]
        elif r == BAND:
            q["a"], q["k0"], q["k1"] = of[u % len(of)], 30.0 + 5.0 * (u // 3 % 4), 70.0 - 5.0 * (u // 12 % 3)
        elif r in (CHANNEL, BREAKOUT):
            q["a"], q["b"] = pf[u % len(pf)], pf[(u // 4 + 1) % len(pf)]
            q["c"] = -1 if u % 3 else pf[(u // 3 + 2) % len(pf)]
        elif r == SCALED:
            q["a"], q["k0"], q["k1"] = pf[u % len(pf)], 1.0 - (1 + u // 4 % 3) / 100.0, 1.0 + (1 + u // 12 % 4) / 100.0
            q["c"] = -1 if u % 2 else pf[(u // 2 + 1) % len(pf)]
        else:
            q["a"], q["b"] = pf[u % len(pf)], pf[(u // 4 + 1) % len(pf)]
            q["c"] = of[u % len(of)] if u % 4 else -1      # -1: the price itself is the gate column
            level = 50.0 if q["c"] >= 0 else 13.0       # gen_ohlcv closes run from 8 to 27
            q["k0"], q["k1"] = level * (1.1 - 0.05 * (u // 4 % 3)), level * (0.9 + 0.05 * (u // 12 % 2))
            if r == STRENGTH:
                q["k0"] = level * (0.8 + 0.1 * (u // 4 % 3))
    return tab


def nan_in_hi_case(oracle, close):
    """-> (lo, hi_nan, hi_null, rows): a channel around a line that the close keeps crossing; per symbol `rows` holds the first row where
    the close buys.  There hi is a non-NULL NaN in hi_nan and the NULL in hi_null: the buy of that row must still fire against hi_nan
    and is refused against hi_null."""
    base = make_lines(close, 1)[0]
    lo, hi = base * 0.985, base * 1.015
    lo[:, :5] = NULL
    hi[:, :3] = NULL
    buy, _sell = oracle.channel_signals(close, lo, hi, 0)
    hi_nan, hi_null = hi.copy(), hi.copy()
    rows = []
    for n in range(close.shape[0]):
        (w,) = np.nonzero(buy[n])
        assert len(w), "every symbol needs a buy for this case"
        rows.append(int(w[0]))
        hi_nan[n, w[0]] = np.nan
        hi_null[n, w[0]] = NULL
    return lo, hi_nan, hi_null, rows
