"""Known answers for tests/strategy_ref.py, the numpy reference of the rule kernels of csrc/strategy.hip (definitions:
include/pq_hip.h, the comment block above pq_gate_signals).  Every expected column below is written out by hand.  Each series holds a
firing row, a row that fails ONLY because a strict comparison meets equality, a NULL row and row 0; the ragged variants put a row
that would fire, had it a predecessor, at the start of a range.  tests/test_strategy_rules_gpu.py runs the same table on the GPU."""
import numpy as np
import pytest

import strategy_ref as R

N = R.NULL
NI = R.NULL_I32
INF = np.inf
f = lambda *v: np.array(v, dtype=np.float64)
u = lambda *v: np.array(v, dtype=np.uint8)
i32 = lambda *v: np.array(v, dtype=np.int32)

_A = i32(100, 0, 200, -100, 0, -100)      # pattern_any: this column is on both sides
_MA = dict(ma0=f(3, 3, 3, 2, 3, N, 3, 1), ma1=f(2, 3, 2, 2, 2, 2, 2, 2), ma2=f(1, 1, 1, 1, 1, 1, 1, 3))
_VOL = dict(volume=f(9, 9, 3, 9, 9, 9, N, 9), avg_volume=f(2, 2, 2, 2, 2, 2, 2, N), close=f(1, 2, 3, 3, 2, N, 3, 4))
_GAP = dict(open=f(9, 9, 8, 1, 2, N, 9, 9), high=f(4, 4, 4, 4, 4, 4, N, 1), low=f(4, 4, 4, 4, 4, 4, 4, 1))
_G3 = dict(a=f(1, 2, 2, N, 3, 4, 3), buy_in=u(1, 1, 1, 1, 1, 1, 1), sell_in=u(0, 1, 0, 0, 0, 0, 3))

# (id, rule, columns, parameters, ranges or None, expected outputs).  NaN in an expected f64 column: "a NaN, whichever".
KATS = [
    # zones: row 1 a == k0 (no buy), row 4 a == k1 (no sell), row 2 NULL, inputs 2 and 255 count as set and come out as 1
    ("gate0", "gate0", dict(a=f(10, 20, N, 90, 80, 15), buy_in=u(1, 1, 1, 1, 0, 2), sell_in=u(0, 1, 1, 255, 1, 1)),
     dict(mode=0, k0=20.0, k1=80.0), None, (u(1, 0, 0, 0, 0, 1), u(0, 0, 0, 1, 0, 0))),
    # strength: row 1 a == k0 closes both sides
    ("gate1", "gate1", dict(a=f(30, 25, N, 26, 10), buy_in=u(1, 1, 1, 0, 1), sell_in=u(0, 1, 1, 1, 1)),
     dict(mode=1, k0=25.0, k1=0.0), None, (u(1, 0, 0, 0, 0), u(0, 0, 0, 1, 0))),
    # above a column: row 1 a == c, row 2 a NULL, row 3 c NULL; the sells pass through (as 0 / 1)
    ("gate2", "gate2", dict(a=f(5, 3, N, 4, 7, 2), c=f(4, 3, 1, N, 6, 9), buy_in=u(1, 1, 1, 1, 255, 1), sell_in=u(1, 0, 1, 0, 2, 0)),
     dict(mode=2, k0=0.0, k1=0.0), None, (u(1, 0, 0, 0, 1, 0), u(1, 0, 1, 0, 1, 0))),
    # rising: row 0 has no predecessor, row 2 a[i] == a[i-1], row 3 NULL, row 4 looks back at the NULL
    ("gate3", "gate3", _G3, dict(mode=3, k0=0.0, k1=0.0), None, (u(0, 1, 0, 0, 0, 1, 0), u(0, 1, 0, 0, 0, 0, 1))),
    # ... row 5 (4 > 3) starts the second range: no predecessor, no buy
    ("gate3-ragged", "gate3", _G3, dict(mode=3, k0=0.0, k1=0.0), [(0, 5), (5, 7)], (u(0, 1, 0, 0, 0, 0, 0), u(0, 1, 0, 0, 0, 0, 1))),
    # distance: row 1 a - c = 1 == |c| * k0 with c < 0 (without the |.| it would be 1 > -1); rows 2, 3 NULL
    ("gate4", "gate4", dict(a=f(6, -3, N, 5, 1, -5), c=f(4, -4, 1, N, 4, -4), buy_in=u(1, 1, 1, 1, 1, 1), sell_in=u(0, 1, 0, 1, 0, 0)),
     dict(mode=4, k0=0.25, k1=0.0), None, (u(1, 0, 0, 0, 0, 0), u(0, 1, 0, 1, 0, 0))),
    # row 1 upper NULL -> NULL; row 2 price NULL -> a NaN; row 3 upper == mid == price -> 0 / 0; rows 4, 5 upper == mid -> +-inf
    ("zscore", "zscore", dict(price=f(3, 5, N, 4, 3, 1), upper=f(5, N, 6, 4, 2, 4), mid=f(1, 2, 3, 4, 2, 4)), {}, None,
     (f(0.5, N, np.nan, np.nan, INF, -INF),)),
    ("scale_band", "scale_band", dict(base=f(10, N, INF, -INF, 0, -3)), dict(f_lo=0.5, f_hi=2.0), None,
     (f(5, N, INF, -INF, 0, -1.5), f(20, N, INF, -INF, 0, -6))),
    ("scale_band-zero", "scale_band", dict(base=f(INF, -INF, 2, N)), dict(f_lo=0.0, f_hi=1.0), None,
     (f(np.nan, np.nan, 0, N), f(INF, -INF, 2, N))),
    # row 2 volume == multiplier * average, row 3 close == close[i-1], rows 5..7 NULLs; row 4 the down day
    ("volume_surge", "volume_surge", _VOL, dict(multiplier=1.5), None, (u(0, 1, 0, 0, 0, 0, 0, 0), u(0, 0, 0, 0, 1, 0, 0, 0))),
    ("volume_surge-ragged", "volume_surge", _VOL, dict(multiplier=1.5), [(0, 1), (1, 8)], (u(0, 0, 0, 0, 0, 0, 0, 0), u(0, 0, 0, 0, 1, 0, 0, 0))),
    # f_up = 2 and f_dn = 0.5 are powers of two: row 2 open == high[i-1] * f_up, row 4 open == low[i-1] * f_dn; row 7 looks back at a NULL high
    ("gap", "gap", _GAP, dict(f_up=2.0, f_dn=0.5), None, (u(0, 1, 0, 0, 0, 0, 1, 0), u(0, 0, 0, 1, 0, 0, 0, 0))),
    ("gap-ragged", "gap", _GAP, dict(f_up=2.0, f_dn=0.5), [(0, 1), (1, 8)], (u(0, 0, 0, 0, 0, 0, 1, 0), u(0, 0, 0, 1, 0, 0, 0, 0))),
    # +-200 never fire, +100 in a bearish column does not sell, -100 in a bullish one does not buy, NULL_I32 is nothing
    ("pattern_any", "pattern_any", dict(bull0=_A, bull1=i32(0, 0, 100, 0, -200, NI), bear0=i32(-100, 100, 0, 0, -200, 0), bear1=_A),
     dict(nb=2, ns=2), None, (u(1, 0, 1, 0, 0, 0), u(1, 0, 0, 1, 0, 1))),
    # row 0 in order but no predecessor; rows 1, 3 two equal averages; row 5 NULL; rows 2, 4, 6 the first bar back in order; row 7 reversed
    ("ma_stack", "ma_stack", _MA, dict(n=3), None, (u(0, 0, 1, 0, 1, 0, 1, 0), u(0, 0, 0, 0, 0, 0, 0, 1))),
    ("ma_stack-ragged", "ma_stack", _MA, dict(n=3), [(0, 2), (2, 8)], (u(0, 0, 0, 0, 1, 0, 1, 0), u(0, 0, 0, 0, 0, 0, 0, 1))),
]


def assert_kat(tag, got, exp):
    assert len(got) == len(exp), tag
    for k, (g, e) in enumerate(zip(got, exp)):
        if e.dtype == np.uint8:
            assert g.dtype == np.uint8 and g.tolist() == e.tolist(), (tag, k, g.tolist(), e.tolist())
        else:
            nan = np.isnan(e) & ~R.isnull(e)
            assert np.isnan(g[nan]).all() and (R.bits(g)[~nan] == R.bits(e)[~nan]).all(), (tag, k, g.tolist(), e.tolist())


@pytest.mark.parametrize("kat", KATS, ids=[k[0] for k in KATS])
def test_known_answers(kat):
    tag, rule, cols, prm, ranges, exp = kat
    assert max(len(c) for c in cols.values()) <= 8
    got = R.ref_case(dict(rule=rule, cols=cols, params=prm), ranges)
    assert_kat(tag, got, exp)
    if ranges is None:      # the same series as one row of an [N, T] array, between two other series
        cols2 = {k: np.stack([c[::-1], c, c[::-1]]) for k, c in cols.items()}
        got2 = R.ref_case(dict(rule=rule, cols=cols2, params=prm), None)
        assert_kat(tag + "[N, T]", [g[1] for g in got2], exp)


def test_every_rule_and_mode_has_known_answers_with_both_sides_firing():
    assert {k[1] for k in KATS} == set(R.RULES)
    for rule in R.RULES:
        exp = [k[5] for k in KATS if k[1] == rule and k[4] is None]
        if exp[0][0].dtype == np.uint8 and not rule.startswith("gate"):
            assert any(e[0].any() for e in exp) and any(e[1].any() for e in exp), rule
    for tag, rule, cols, prm, ranges, exp in KATS:      # a ragged answer differs from the plain one exactly at a range start
        if ranges is not None:
            plain = next(k[5] for k in KATS if k[1] == rule and k[4] is None and k[2] is cols)
            diff = np.flatnonzero((plain[0] != exp[0]) | (plain[1] != exp[1]))
            assert len(diff) == 1 and diff[0] in [lo for lo, _ in ranges], tag


def test_refusals_and_empty_columns():
    with pytest.raises(ValueError):
        R.gate_signals(f(1), None, 5, 0, 0, u(1), u(1))
    with pytest.raises(ValueError):
        R.gate_signals(f(1), None, -1, 0, 0, u(1), u(1))
    for mode in (2, 4):
        with pytest.raises(ValueError):
            R.gate_signals(f(1), None, mode, 0, 0, u(1), u(1))
    for n in (1, 17):
        with pytest.raises(ValueError):
            R.ma_stack_signals([f(1, 2)] * n)
    b, s = R.pattern_any_signals([], [], shape=(2, 3))
    assert b.shape == (2, 3) and not b.any() and not s.any()
    for fn in (lambda: R.zscore(f(), f(), f()), lambda: R.scale_band(f(), 1.0, 2.0), lambda: R.gap_signals(f(), f(), f(), 1.0, 1.0)):
        assert all(o.size == 0 for o in fn())


def test_padding_and_guard_rows_are_not_series():
    """a pitched layout is the flat column with ranges: padding (1e300 / 0xFF) is neither read as a predecessor nor written"""
    lay = R.regular_layout(3, 5, 7)
    rng = np.random.default_rng(1)
    for rule in R.RULES:
        case = R.gen_case(rule, rng, lay, p_null=0.0, p_nan=0.0)
        live = R.live_of(lay)
        outs = R.ref_case(case, R.ranges_of(lay), shape=(lay["size"],))
        dense = {k: c[: 3 * 7].reshape(3, 7)[:, :5] for k, c in case["cols"].items()}
        outs2 = R.ref_case(dict(case, cols=dense), None, shape=(3, 5))
        for o, o2 in zip(outs, outs2):
            assert not o[~live].any()
            assert (o[: 3 * 7].reshape(3, 7)[:, :5] == o2).all(), rule


def test_randomised_run_fires_for_every_rule():
    """The precondition of the randomised GPU test, on the reference alone: over its cases every rule and mode produces set buys
    and sells (or finite and NULL values): zeros against zeros would prove nothing."""
    count = {r: np.zeros(2, dtype=np.int64) for r in R.RULES}
    rows = 0
    for case, lay in R.random_cases():
        outs = R.ref_case(case, R.ranges_of(lay), shape=(lay["size"],))
        count[case["rule"]] += R.firing(case, outs)
        rows += int(R.live_of(lay).sum())
    assert rows > 100_000
    for r, c in count.items():
        assert c[0] >= 50, (r, c)
        assert c[1] >= 50 or r in ("gate2", "gate3", "gate4"), (r, c)      # (their sells pass through: counted, not gated)
    assert all(count[r][1] >= 50 for r in ("gate2", "gate3", "gate4"))
