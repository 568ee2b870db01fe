"""not-gpu: the numpy restatement of decision D-21 (tests/xsec_rolling_ref.py: moving_average, momentum, volatility, skewness,
relative_strength) against hand-derived tables and against independent code (pandas rolling, scipy.stats.skew, plain numpy loops), the
bit identities D-21 states, and the public surface of the feature: method names and defaults, the argument errors that must come
before any device work, the C declaration."""
import inspect
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import xsec_rolling_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL
INF, NAN = np.inf, np.nan


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same(got, exp):
    assert (bits(got) == bits(exp)).all(), (got, exp)


def row(*v):
    return np.array([v], dtype=np.float64)


# ---------------------------------------------------------------- hand-derived tables
def test_moving_average_hand_table():
    # w = 3: rows 0, 1 warm up; the NULL of day 2 empties rows 2, 3, 4; 4 + 5 + 6 = 15, 5 + 6 + 9 = 20
    same(R.moving_average(row(1, 2, NULL, 4, 5, 6, 9), 3), row(NULL, NULL, NULL, NULL, NULL, 5.0, float(Fraction(20, 3))))
    # w = 2: a zero is a value like any other, +inf and NaN are outside
    same(R.moving_average(row(0, 2, 4, INF, 1, 1, 1, NAN), 2), row(NULL, 1.0, 3.0, NULL, NULL, 1.0, 1.0, NULL))
    same(R.moving_average(row(3, -INF, 5), 1), row(3.0, NULL, 5.0))
    # ascending order from 0.0: (0.0 + 1e16) + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    same(R.moving_average(row(1e16, 1, 1, 1e16), 3), row(NULL, NULL, 1e16 / 3.0, (2.0 + 1e16) / 3.0))


def test_momentum_hand_table():
    x = row(2, 4, NULL, 8, 0, 0, 1)
    # t = 3: (8 - 4) / 4; t = 5: (0 - 8) / 8; t = 6: (1 - 0) / 0 = +inf passes; t = 2, 4: one end NULL
    same(R.momentum(x, 2), row(NULL, NULL, NULL, 1.0, NULL, -1.0, INF))
    # skip = 1: row t holds the skip = 0 value of row t - 1
    same(R.momentum(x, 2, skip=1), row(NULL, NULL, NULL, NULL, 1.0, NULL, -1.0))
    same(R.momentum(x, 2, skip=5), np.full((1, 7), NULL))                             # skip + window >= T
    same(R.momentum(row(0, 5, 0, NAN, 7, -INF, 3), 2), row(NULL, NULL, NULL, NULL, INF, NULL, float(Fraction(-4, 7))))  # 0 / 0 -> NULL
    same(R.momentum(row(3, 4, 6), 1), row(NULL, float(Fraction(1, 3)), 0.5))


def test_volatility_and_skewness_hand_table():
    # prices 1 1 1 4 4 4 4: r = -, 0, 0, 3, 0, 0, 0.  w = 3, rows 3 .. 5 hold the returns {0, 0, 3} in three orders: m = 1,
    # e = {-1, -1, 2}, sum e^2 = 6, sum e^3 = 6; volatility sqrt(6 / 2), skewness (6 / 3) / ((6 / 3) sqrt(6 / 3)); row 6 is constant
    x = row(1, 1, 1, 4, 4, 4, 4)
    v, g = math.sqrt(3.0), 2.0 / (2.0 * math.sqrt(2.0))
    same(R.volatility(x, 3), row(NULL, NULL, NULL, v, v, v, 0.0))
    same(R.skewness(x, 3), row(NULL, NULL, NULL, g, g, g, NULL))
    # w = 2 on 1 2 3 6 6 6: r = -, 1, 1/2, 1, 0, 0 -> rows 2, 3: m = 3/4, e = +-1/4, v = 1/8; row 4: m = 1/2, v = 1/2; row 5 constant
    same(R.volatility(row(1, 2, 3, 6, 6, 6), 2), row(NULL, NULL, math.sqrt(0.125), math.sqrt(0.125), math.sqrt(0.5), 0.0))
    # a negative skew: returns {0, 0, -1/2}: m = -1/6 is inexact, so only the sign and the symmetry are read off
    s = R.skewness(row(2, 2, 2, 1, 1, 1), 3)
    assert (s[0, 3:5] < 0).all() and R.isnull(s[0, :3]).all()
    np.testing.assert_allclose(s[0, 3:], -g, rtol=1e-14)


def test_relative_strength_hand_table():
    # d = -, 2, -1, 0, 0, 3, -, -.  w = 2: row 2: G = 2, L = 1 -> 200 / 3; row 3: G = 0, L = 1 -> 0; row 4: flat -> NULL; row 5: 100
    x = row(1, 3, 2, 2, 2, 5, NULL, 1)
    same(R.relative_strength(x, 2), row(NULL, NULL, float(Fraction(200, 3)), 0.0, NULL, 100.0, NULL, NULL))
    same(R.relative_strength(x, 1), row(NULL, 100.0, 0.0, NULL, NULL, 100.0, NULL, NULL))
    # a zero price is a value: d = -, -3, 0, 1 -> w = 3: G = 1, L = 3 -> 25
    same(R.relative_strength(row(3, 0, 0, 1), 3), row(NULL, NULL, NULL, 25.0))


# day 2 of 1 .. 8 replaced: which rows lose their sample at w = 2 (besides the warm-up rows).  mean reads days t-1 .. t, the others
# days t-2 .. t, momentum only its two ends; row 5 is the first whose window lies wholly behind the bad day.
@pytest.mark.parametrize("bad", [NULL, NAN, INF, -INF], ids=["null", "nan", "+inf", "-inf"])
def test_invalid_cell_inside_at_the_edge_and_outside_the_window(bad):
    x = row(1, 2, 3, 4, 5, 6, 7, 8)
    x[0, 2] = bad
    nulls = {"mean": [0, 2, 3], "momentum": [0, 1, 2, 4], "volatility": [0, 1, 2, 3, 4], "skewness": [0, 1, 2, 3, 4, 5],
             "relative_strength": [0, 1, 2, 3, 4]}
    for op, rows in nulls.items():
        w = 3 if op == "skewness" else 2
        got = R.rolling(x, op, w)
        assert np.flatnonzero(R.isnull(got[0])).tolist() == rows, (op, got)
        assert not np.isnan(got[~R.isnull(got)]).any()


def test_zero_price_inside_the_window():
    x = row(1, 2, 0, 4, 5, 6, 7, 8)
    same(R.moving_average(x, 2), row(NULL, 1.5, 1.0, 2.0, 4.5, 5.5, 6.5, 7.5))
    same(R.momentum(x, 2)[0, :5], [NULL, NULL, -1.0, 1.0, INF])
    v = R.volatility(x, 2)                      # r[2] = -1 is finite, r[3] = 4 / 0 is not: rows 3 and 4 lose their sample
    assert np.flatnonzero(R.isnull(v[0])).tolist() == [0, 1, 3, 4]
    same(v[0, 2], math.sqrt(2.0))               # r = {1, -1}: m = 0, sum e^2 = 2
    assert np.flatnonzero(R.isnull(R.skewness(x, 3)[0])).tolist() == [0, 1, 2, 3, 4, 5]
    same(R.relative_strength(x, 2), row(NULL, NULL, float(Fraction(100, 3)), float(Fraction(400, 6)), 100.0, 100.0, 100.0, 100.0))


def test_constant_stretch():
    x = row(5, 5, 5, 5, 5, 5)
    same(R.volatility(x, 3), row(NULL, NULL, NULL, 0.0, 0.0, 0.0))
    same(R.skewness(x, 3), np.full((1, 6), NULL))
    same(R.relative_strength(x, 3), np.full((1, 6), NULL))
    same(R.momentum(x, 3), row(NULL, NULL, NULL, 0.0, 0.0, 0.0))
    same(R.moving_average(x, 3), row(NULL, NULL, 5.0, 5.0, 5.0, 5.0))


def test_window_longer_than_the_series_and_empty_columns():
    x = row(1, 2, 3)
    for op in R.OPS:
        same(R.rolling(x, op, 3 if op in ("mean", "momentum") else 4), row(NULL, NULL, NULL) if op != "mean" else row(NULL, NULL, 2.0))
        assert R.rolling(np.empty((0, 4)), op, 3).shape == (0, 4) and R.rolling(np.empty((2, 0)), op, 3).shape == (2, 0)


# ---------------------------------------------------------------- independent code
RTOL = ATOL = 1e-10       # sums of at most 60 well-scaled terms: rounding stays near 60 * 2^-53 * |e / sigma|^3 ~ 1e-12 even for g1


@pytest.fixture(scope="module")
def walk():
    """a positive random walk with holes: exp(cumsum(0.02 N(0, 1)))"""
    rng = np.random.default_rng(21)
    x = np.exp(np.cumsum(0.02 * rng.standard_normal((4, 260)), axis=1))
    x[1, 100] = NULL
    x[2, 50] = NAN
    x[3, 7] = INF
    return x


def clean(x):
    return np.where(R.valid(x), x, NAN)


@pytest.mark.parametrize("w", [5, 20, 60])
def test_against_pandas_scipy_and_plain_loops(walk, w):
    pd = pytest.importorskip("pandas")
    skew = pytest.importorskip("scipy.stats").skew
    x = walk
    ops = {op: R.rolling(x, op, w) for op in R.OPS}
    for s in range(x.shape[0]):
        ser = pd.Series(clean(x[s]))
        ret = ser.diff() / ser.shift(1)
        exp = {"mean": ser.rolling(w).mean().to_numpy(), "volatility": ret.rolling(w).std(ddof=1).to_numpy()}
        c, r = clean(x[s]), ret.to_numpy()
        exp["momentum"] = np.full(x.shape[1], NAN)
        exp["momentum"][w:] = (c[w:] - c[:-w]) / c[:-w]
        exp["skewness"] = np.full(x.shape[1], NAN)
        exp["relative_strength"] = np.full(x.shape[1], NAN)
        for t in range(w, x.shape[1]):
            exp["skewness"][t] = skew(r[t - w + 1:t + 1], bias=True)
            d = np.diff(c[t - w:t + 1])
            g, l = d[d > 0].sum(), -d[d < 0].sum()
            exp["relative_strength"][t] = 100.0 * g / (g + l) if not np.isnan(d).any() else NAN
        for op in R.OPS:
            got = ops[op][s]
            live = ~np.isnan(exp[op])
            assert (R.isnull(got) == ~live).all(), (op, s)
            np.testing.assert_allclose(got[live], exp[op][live], rtol=RTOL, atol=ATOL, err_msg=f"{op} w={w} symbol {s}")
            assert live[w:].sum() > (x.shape[1] - w) // 2


# ---------------------------------------------------------------- the bit identities of D-21
@pytest.mark.parametrize("w", [1, 5, 20])
def test_momentum_is_the_simple_return_of_period_w(walk, w):
    x = walk.copy()
    x[0, 30] = 0.0
    exp = np.full(x.shape, NULL)
    with np.errstate(all="ignore"):
        v = (x[:, w:] - x[:, :-w]) / x[:, :-w]
    exp[:, w:] = np.where(R.valid(x[:, w:]) & R.valid(x[:, :-w]) & ~np.isnan(v), v, NULL)
    same(R.momentum(x, w), exp)
    assert np.isinf(R.momentum(x, w)[0, 30 + w])


def test_moving_average_of_one_day_is_the_column(walk):
    x = walk.copy()
    x[0, 3] = 0.0
    same(R.moving_average(x, 1), np.where(R.valid(x), x, NULL))
    same(R.moving_average(row(-0.0, 2.0), 1), row(0.0, 2.0))      # the sum starts at +0.0, and +0.0 + -0.0 is +0.0


# ---------------------------------------------------------------- the public surface
def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import api
    F = pq.Factor
    want = {"moving_average": [("factor", None), ("window", 20)], "momentum": [("factor", None), ("window", 20), ("skip", 0)],
            "volatility": [("factor", None), ("window", 20)], "skewness": [("factor", None), ("window", 20)],
            "relative_strength": [("factor", None), ("window", 14)]}
    for name, params in want.items():
        sig = inspect.signature(getattr(F, name))
        assert list(sig.parameters) == ["self"] + [p for p, _ in params], name
        for p, default in params[1:]:
            assert sig.parameters[p].default == default, (name, p)
    assert not hasattr(F, "clean")
    assert api.ROLLING_OPS == {"mean": 0, "momentum": 1, "volatility": 2, "skewness": 3, "relative_strength": 4}
    assert api.ROLLING_MAX_WINDOW == 1024 == R.MAX_WINDOW
    assert {name: api.ROLLING_MIN_WINDOW[code] for name, code in api.ROLLING_OPS.items()} == R.MIN_WINDOW
    assert callable(api.factor_rolling)
    raw = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define\s+PQ_FACTOR_ROLLING_MAX_WINDOW\s+1024\b", raw)
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"pq_status\s+pq_factor_rolling\s*\(([^)]*)\)", txt)
    assert decl, "pq_factor_rolling is not declared"
    assert [re.findall(r"\w+", a)[-1] for a in decl.group(1).split(",")] == ["pq_ctx", "pq_batch", "x", "op", "window", "skip", "out"]
    assert [re.findall(r"\w+", a)[-2] for a in decl.group(1).split(",")[3:6]] == ["int32_t", "int64_t", "int64_t"]
    assert "xsec/rolling.hip" in (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()


ONES = np.ones((3, 40))


@pytest.mark.parametrize("call, msg", [
    (lambda f: f.moving_average(np.ones(40)), r"must be \[N, T\]"),
    (lambda f: f.volatility(np.ones((2, 3, 40))), r"must be \[N, T\]"),
    (lambda f: f.moving_average(ONES, 0), "window"),
    (lambda f: f.relative_strength(ONES, 1025), "window"),
    (lambda f: f.momentum(ONES, True), "window"),
    (lambda f: f.skewness(ONES, 2.5), "window"),
    (lambda f: f.volatility(ONES, 1), "window"),
    (lambda f: f.skewness(ONES, 2), "window"),
    (lambda f: f.momentum(ONES, 5, skip=-1), "skip"),
    (lambda f: f.momentum(ONES, 5, skip=1.0), "skip"),
    (lambda f: f.momentum(ONES, 5, skip=False), "skip"),
])
def test_argument_errors_raise_before_device_work(call, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    with pytest.raises(ValueError, match=msg):
        call(pq.Factor())


def test_api_codes_raise_before_device_work():
    from polars_quant_amd import api
    with pytest.raises(ValueError, match="skip"):
        api.factor_rolling(ONES, api.ROLLING_OPS["mean"], 5, skip=1)
    for bad in (lambda: api.factor_rolling(ONES, 5, 5), lambda: api.factor_rolling(ONES, -1, 5), lambda: api.factor_rolling(ONES, True, 5),
                lambda: api.factor_rolling(ONES, api.ROLLING_OPS["volatility"], 5, skip=2)):
        with pytest.raises(ValueError):
            bad()
