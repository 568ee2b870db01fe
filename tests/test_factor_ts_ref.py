"""not-gpu: the numpy restatement of decision D-29 (tests/xsec_ts_ref.py: ts_sum, ts_std, ts_zscore, ts_min, ts_max, ts_argmin,
ts_argmax, ts_rank, decay_linear, delay, delta, ts_cov, ts_corr) against hand-derived tables and against independent code (pandas
rolling, scipy.stats.rankdata, numpy.argmax / average per window), the bit identities that tie it to D-21 and D-28, the public surface
of the feature -- tables, method names and defaults, the argument errors that must come before any device work, the C declarations --
and the register / scratch figures of csrc/xsec/tsops.hip."""
import importlib
import inspect
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import xsec_rolling_ref as RL
import xsec_rolling_regress_ref as RR
import xsec_ts_ref as R

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
# w = 3 windows: [2 1 2] [1 2 3] [2 3 3] [3 3 0] [3 0 -0] [0 -0 0]: a tie for the maximum, a tie that includes today, a +-0 pair
TIES = row(2, 1, 2, 3, 3, 0.0, -0.0, 0.0)


def test_argmax_argmin_the_oldest_tie_wins():
    same(R.ts_argmax(TIES, 3), row(NULL, NULL, 0, 2, 1, 0, 0, 0))
    same(R.ts_argmin(TIES, 3), row(NULL, NULL, 1, 0, 0, 2, 1, 0))      # [3 0 -0]: -0 < 0 is false, the older +0 stays
    same(R.ts_argmax(row(4, 4, 4, 4), 4), row(NULL, NULL, NULL, 0))
    same(R.ts_argmax(row(7, 3, 9), 1), row(0, 0, 0))


def test_min_max_hand_table():
    same(R.ts_max(TIES, 3), row(NULL, NULL, 2, 3, 3, 3, 3, 0.0))
    same(R.ts_min(TIES, 3), row(NULL, NULL, 1, 1, 2, 0.0, 0.0, 0.0))  # of the +-0 tie the oldest stays, bit for bit
    same(R.ts_min(row(-0.0, 0.0, 5), 2), row(NULL, -0.0, 0.0))
    same(R.ts_max(row(-0.0, 0.0, 5), 2), row(NULL, -0.0, 5))


def test_rank_with_ties():
    # [2 1 2]: one value below today's 2 and two equal to it: (2 + 2 + 1) / 2 = 2.5; [3 0 -0]: -0 == 0, (0 + 2 + 1) / 2; [0 -0 0]: 2
    same(R.ts_rank(TIES, 3), row(NULL, NULL, 2.5, 3, 2.5, 1, 1.5, 2))
    same(R.ts_rank(TIES, 3, pct=True), row(NULL, NULL, 2.5 / 3.0, 1.0, 2.5 / 3.0, 1.0 / 3.0, 0.5, 2.0 / 3.0))
    same(R.ts_rank(TIES, 1), np.ones((1, 8)))
    same(R.ts_rank(row(5, 5, 5, 5), 4, pct=True), row(NULL, NULL, NULL, 2.5 / 4.0))


def test_sum_and_decay_linear_hand_table():
    x = row(1, 2, 3, 4)
    same(R.ts_sum(x, 3), row(NULL, NULL, 6, 9))
    # weights 1 2 3 over 6: (1 + 4 + 9) / 6, (2 + 6 + 12) / 6
    same(R.decay_linear(x, 3), row(NULL, NULL, float(Fraction(14, 6)), float(Fraction(20, 6))))
    same(R.decay_linear(x, 1), x)
    same(R.decay_linear(row(6, 6, 6), 3), row(NULL, NULL, 6))
    # ascending order from 0.0: (0.0 + 1e16) + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    same(R.ts_sum(row(1e16, 1, 1, 1e16), 3), row(NULL, NULL, 1e16, 2.0 + 1e16))
    same(R.ts_sum(row(-0.0, 2.0), 1), row(0.0, 2.0))                  # the sum starts at +0.0


def test_std_and_zscore_hand_table():
    # [5 5 5]: q2 = 0, std 0, zscore NULL; [5 5 2]: mean 4, deviations 1 1 -2, q2 = 6, std sqrt(6 / 2), z = (2 - 4) / sqrt(3)
    x = row(5, 5, 5, 2)
    same(R.ts_std(x, 3), row(NULL, NULL, 0.0, math.sqrt(3.0)))
    same(R.ts_zscore(x, 3), row(NULL, NULL, NULL, -2.0 / math.sqrt(3.0)))
    # w = 2 on 1 3: mean 2, q2 = 2, std sqrt(2), z = 1 / sqrt(2)
    same(R.ts_zscore(row(1, 3, 3), 2), row(NULL, 1.0 / math.sqrt(2.0), NULL))


def test_cov_and_corr_hand_table():
    x = row(1, 2, 3, 4, 4, 4, 7)
    # [1 2 3]: deviations -1 0 1, sxx = 2, cov = 1; [2 3 4] the same; [3 4 4]: mean 11/3 is inexact, only read off below; [4 4 4] constant
    c = R.ts_cov(x, x, 3)
    same(c[0, :4], [NULL, NULL, 1.0, 1.0])
    same(c[0, 5], 0.0)
    for y, sign in ((x, 1.0), (-x, -1.0)):
        r = R.ts_corr(x, y, 3)
        assert R.isnull(r[0, [0, 1, 5]]).all() and not R.isnull(r[0, [2, 3, 4, 6]]).any()
        np.testing.assert_allclose(r[0, [2, 3, 4, 6]], sign, rtol=5e-16, atol=0)     # two roots, a product, a division: 4 x 2^-53
    live = ~R.isnull(R.ts_corr(x, x, 3))
    same(R.ts_corr(x, -x, 3)[live], -R.ts_corr(x, x, 3)[live])
    # a constant y alone: syy == 0
    assert R.isnull(R.ts_corr(x, np.full(x.shape, 2.0), 3)).all() and (R.ts_cov(x, np.full(x.shape, 2.0), 3)[0, 2:] == 0.0).all()
    # exact: x = 1 2 3, y = 2 1 0 -> sxy = -2, sxx = syy = 2 -> cov -1
    same(R.ts_cov(row(1, 2, 3), row(2, 1, 0), 3), row(NULL, NULL, -1.0))


def test_delay_and_delta_hand_table():
    x = row(1, 2, NULL, 4, INF, NAN, -0.0, 8)
    same(R.delay(x), row(NULL, 1, 2, NULL, 4, INF, NULL, -0.0))       # +inf passes, NaN does not, -0 is copied
    same(R.delay(x, 2), row(NULL, NULL, 1, 2, NULL, 4, INF, NULL))
    same(R.delta(x), row(NULL, 1, NULL, NULL, NULL, NULL, NULL, 8))
    same(R.delta(x, 3), row(NULL, NULL, NULL, 3, NULL, NULL, -4, NULL))
    same(R.delay(x, 8), np.full((1, 8), NULL))
    same(R.delta(x, 9), np.full((1, 8), NULL))


# day 2 of 1 .. 8 replaced: every windowed op at w = 2 loses rows 2 and 3 (besides the warm-up row), delay 1 loses row 3 unless the cell
# is +-inf, delta 1 rows 2 and 3
@pytest.mark.parametrize("bad", [NULL, NAN, INF, -INF], ids=["null", "nan", "+inf", "-inf"])
def test_invalid_cell_inside_at_the_edge_and_outside_the_window(bad):
    x = row(1, 2, 3, 4, 5, 6, 7, 8)
    x[0, 2] = bad
    y = row(3, 1, 4, 1, 5, 9, 2, 6)
    for op in R.OPS[:9]:
        for mode in ((0, 1) if op == "rank" else (0,)):
            got = R.ts(x, op, 2, mode)
            assert np.flatnonzero(R.isnull(got[0])).tolist() == [0, 2, 3], (op, got)
            assert not np.isnan(got[~R.isnull(got)]).any()
    assert np.flatnonzero(R.isnull(R.delay(x)[0])).tolist() == ([0] if np.isinf(bad) else [0, 3])
    assert np.flatnonzero(R.isnull(R.delta(x)[0])).tolist() == [0, 2, 3]
    for op in R.PAIR_OPS:
        for a, b in ((x, y), (y, x)):
            assert np.flatnonzero(R.isnull(R.ts_pair(a, b, op, 2)[0])).tolist() == [0, 2, 3], op


def test_a_nan_result_is_null():
    """a sum of finite terms can overflow to +-inf (which passes) but never to NaN; a weighted one can: 2 * 1.7e308 - 3 * 1.7e308"""
    big = row(0, 1.7e308, -1.7e308, 1.7e308)
    same(R.ts_sum(big, 2), row(NULL, 1.7e308, 0.0, 0.0))
    same(R.ts_sum(row(1.7e308, 1.7e308, 1.0), 2), row(NULL, INF, 1.7e308 + 1.0))
    same(R.decay_linear(big, 3), row(NULL, NULL, NULL, NULL))          # 0 + inf - inf, and -1.7e308 + inf ... -inf + inf
    # sum = inf, mean = inf, deviations -inf, q2 = inf, std inf; zscore (x - inf) / inf = NaN -> NULL
    two = row(1.7e308, 1.7e308)
    assert np.isinf(R.ts_std(two, 2)[0, 1]) and R.isnull(R.ts_zscore(two, 2)).all()


def test_window_longer_than_the_series_and_empty_columns():
    x, y = row(1, 2, 3), row(3, 1, 2)
    for op in R.OPS:
        assert R.isnull(R.ts(x, op, 4)).all(), op
        assert not R.isnull(R.ts(x, op, 3 if op not in ("delay", "delta") else 2)[0, 2]), op
        assert R.ts(np.empty((0, 4)), op, 3).shape == (0, 4) and R.ts(np.empty((2, 0)), op, 3).shape == (2, 0)
    for op in R.PAIR_OPS:
        assert R.isnull(R.ts_pair(x, y, op, 4)).all() and not R.isnull(R.ts_pair(x, y, op, 3)[0, 2])
        assert R.ts_pair(np.empty((0, 4)), np.empty((0, 4)), op, 3).shape == (0, 4)


# ---------------------------------------------------------------- independent code
RTOL = ATOL = 1e-10       # test_factor_rolling_ref.py's: sums of at most 60 well-scaled terms


@pytest.fixture(scope="module")
def walk():
    """D-21's positive random walk with holes, exp(cumsum(0.02 N(0, 1))), and a second one for the pair ops, with a hole of its own"""
    rng = np.random.default_rng(21)
    x = np.exp(np.cumsum(0.02 * rng.standard_normal((4, 260)), axis=1))
    x[1, 100] = NULL
    x[2, 50] = NAN
    x[3, 7] = INF
    y = np.exp(np.cumsum(0.02 * rng.standard_normal((4, 260)), axis=1))
    y[0, 200] = NULL
    return x, y


def clean(x):
    return np.where(R.valid(x), x, NAN)


FLOATING = ("sum", "std", "zscore", "decay_linear", "cov", "corr")


def pandas_per_window(pd, how, w, c, other=None):
    """pandas' rolling std / cov / corr of every window of c taken on its own: the windows are the columns of a frame of w rows, and the
    frame's last row is read.  Slid along the whole series instead, pandas' moments are online sums that add the entering and remove the
    leaving day; that leaves an ABSOLUTE error near 1e-15 in the second moments, and against a window variance of 1e-8 .. 1e-4 (two to
    five days of a 2 % walk) a relative one of 1e-7 .. 1e-11 in std and corr: measured on these inputs against numpy.std / corrcoef
    window by window, pandas slid 5.4e-7 (std, relative) and 1.1e-6 (corr) at w = 2 and 2.9e-11 / 2.5e-11 at w = 5, the restatement
    0 / 4.4e-16 and 0 / 3.3e-16.  On a window of its own nothing leaves the sums, and pandas is as good as its formula."""
    from numpy.lib.stride_tricks import sliding_window_view
    frame = lambda v: pd.DataFrame(sliding_window_view(v, w).T.copy())
    roll = frame(c).rolling(w)
    res = roll.std(ddof=1) if how == "std" else getattr(roll, how)(frame(other), **({"ddof": 1} if how == "cov" else {}))
    return np.concatenate([np.full(w - 1, NAN), res.iloc[-1].to_numpy()])


@pytest.mark.parametrize("w", [2, 5, 20, 60])
def test_against_pandas_scipy_and_numpy(walk, w):
    pd = pytest.importorskip("pandas")
    rankdata = pytest.importorskip("scipy.stats").rankdata
    x, y = walk
    T = x.shape[1]
    got = {op: R.ts(x, op, w) for op in R.OPS}
    got["rank_pct"] = R.ts(x, "rank", w, 1)
    weights = np.arange(1.0, w + 1.0)
    for s in range(x.shape[0]):
        c = clean(x[s])
        ser = pd.Series(c)
        roll = ser.rolling(w)
        exp = {"sum": roll.sum(), "min": roll.min(), "max": roll.max(), "rank": roll.rank(method="average"),
               "rank_pct": roll.rank(method="average", pct=True)}
        exp = {k: v.to_numpy() for k, v in exp.items()}
        exp["std"] = pandas_per_window(pd, "std", w, c)
        exp["zscore"] = (c - roll.mean().to_numpy()) / exp["std"]
        passes = np.where(R.isnull(x[s]), NAN, x[s])                   # delay hands +-inf on
        exp["delay"] = pd.Series(passes).shift(w).to_numpy()
        exp["delta"] = np.full(T, NAN)
        exp["delta"][w:] = c[w:] - c[:-w]
        for op in ("argmin", "argmax", "decay_linear", "rank_scipy"):
            exp[op] = np.full(T, NAN)
        for t in range(w - 1, T):
            win = c[t - w + 1:t + 1]
            if np.isnan(win).any():
                continue
            exp["argmin"][t], exp["argmax"][t] = np.argmin(win), np.argmax(win)
            exp["decay_linear"][t] = np.average(win, weights=weights)
            exp["rank_scipy"][t] = rankdata(win, method="average")[-1]
        got["rank_scipy"] = got["rank"]
        for op, e in exp.items():
            g = got[op][s]
            live = ~np.isnan(e)
            assert (R.isnull(g) == ~live).all(), (op, s)
            if op in FLOATING:
                np.testing.assert_allclose(g[live], e[live], rtol=RTOL, atol=ATOL, err_msg=f"{op} w={w} symbol {s}")
            elif op == "rank_pct":                                     # pandas divides the same half-integer by the same count
                np.testing.assert_allclose(g[live], e[live], rtol=1e-15, atol=0, err_msg=f"{op} w={w} symbol {s}")
            else:
                assert (g[live] == e[live]).all(), (op, w, s)
            assert live[w:].sum() > (T - w) // 2, (op, s)


@pytest.mark.parametrize("w", [2, 5, 20, 60])
@pytest.mark.parametrize("op", R.PAIR_OPS)
def test_pair_ops_against_pandas(walk, op, w):
    """pandas' rolling cov / corr of every window on its own (pandas_per_window), x the D-21 walk.  The second column is the second
    walk with alternating signs, chosen from the reference's own error: pandas evaluates the numerator as E[xy] - E[x] E[y] on the
    uncentred values, so its absolute error is about 6 u |E[x] E[y]| (u = 2^-53: the products, the two means, the difference), and
    against a two-day covariance dx dy / 4 a relative one of 24 u (|E[x]| / |dx|) (|E[y]| / |dy|).  The walk fixes the first ratio, up
    to 2.4e4 on its smallest moves; a second column at a level of 1 that moves by 2 % has the same, and pandas is then good to 8.5e-8
    only (measured: up to 2.9e-9 from the exact +-1 of two days, which the restatement returns within 4.4e-16).  With alternating
    signs |E[y]| / |dy| is at most 0.015, the bound 1.8e-13, and the rest of the 1e-10 is left to pandas' variances.  The input
    property is asserted below; the tolerance and the windows are those of the other floating results."""
    pd = pytest.importorskip("pandas")
    x, y = walk
    y = y * np.where(np.arange(y.shape[1]) % 2 == 0, 1.0, -1.0)       # a NULL becomes another NaN: outside the sample either way
    cx, cy = clean(x), clean(y)
    with np.errstate(all="ignore"):
        level_over_move = [np.abs(c[:, 1:] + c[:, :-1]) / (2.0 * np.abs(c[:, 1:] - c[:, :-1])) for c in (cx, cy)]
        apriori = 24.0 * 2.0 ** -53 * np.nanmax(level_over_move[0] * level_over_move[1])
    print(f"pandas' numerator at w = 2 is good to {apriori:.3g} on these inputs")
    assert apriori <= 0.1 * RTOL
    got = R.ts_pair(x, y, op, w)
    for s in range(x.shape[0]):
        e = pandas_per_window(pd, op, w, cx[s], cy[s])
        live = ~np.isnan(e)
        assert (R.isnull(got[s]) == ~live).all(), s
        assert live[w:].sum() > (x.shape[1] - w) // 2, s
        print(f"{op} w={w} symbol {s}: max |restatement - pandas| = {np.abs(got[s][live] - e[live]).max():.3g}")
        np.testing.assert_allclose(got[s][live], e[live], rtol=RTOL, atol=ATOL, err_msg=f"{op} w={w} symbol {s}")


# ---------------------------------------------------------------- identities on the restatement
@pytest.mark.parametrize("w", [1, 2, 5, 20, 60])
def test_sum_over_w_is_the_moving_average(walk, w):
    x, _ = walk
    s = R.ts_sum(x, w)
    assert (~R.isnull(s)).sum() > x.size // 2
    same(np.where(R.isnull(s), NULL, s / float(w)), RL.moving_average(x, w))


@pytest.mark.parametrize("w", [2, 5, 20, 60])
def test_std_of_the_returns_is_the_volatility(walk, w):
    x = np.exp(np.cumsum(0.02 * np.random.default_rng(29).standard_normal((4, 260)), axis=1))      # the plain walk
    r = RL.momentum(x, 1)
    v = RL.volatility(x, w)
    assert R.isnull(r[:, 0]).all() and not R.isnull(v[:, w:]).any()
    same(R.ts_std(r, w), v)


@pytest.mark.parametrize("w", [3, 5, 20, 60])
def test_corr_squared_is_the_r_squared_of_the_one_regressor_fit(walk, w):
    x, y = walk
    c = R.ts_corr(x, y, w)
    r2 = RR.rolling_regress(y, [x], w)["r_squared"]
    live = ~R.isnull(c)
    assert (live == ~R.isnull(r2)).all() and live.sum() > x.size // 2
    np.testing.assert_allclose(c[live] * c[live], r2[live], rtol=0, atol=1e-10)


def test_ts_pair_is_symmetric_and_cov_with_itself_is_the_variance(walk):
    x, y = walk
    for op in R.PAIR_OPS:
        same(R.ts_pair(x, y, op, 20), R.ts_pair(y, x, op, 20))
    s = R.ts_std(x, 20)
    v = R.ts_cov(x, x, 20)
    live = ~R.isnull(v)
    assert (live == ~R.isnull(s)).all()
    same(np.sqrt(v[live]), s[live])


# ---------------------------------------------------------------- the public surface
def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    F = pq.Factor
    want = {"ts_sum": [("x", None), ("window", None)], "ts_std": [("x", None), ("window", None)], "ts_zscore": [("x", None), ("window", None)],
            "ts_min": [("x", None), ("window", None)], "ts_max": [("x", None), ("window", None)], "ts_argmin": [("x", None), ("window", None)],
            "ts_argmax": [("x", None), ("window", None)], "ts_rank": [("x", None), ("window", None), ("pct", False)],
            "decay_linear": [("x", None), ("window", None)], "delay": [("x", None), ("periods", 1)], "delta": [("x", None), ("periods", 1)],
            "ts_cov": [("x", None), ("y", None), ("window", None)], "ts_corr": [("x", None), ("y", None), ("window", None)]}
    for name, params in want.items():
        sig = inspect.signature(getattr(F, name))
        assert list(sig.parameters) == ["self"] + [p for p, _ in params], name
        for p, default in params:
            assert sig.parameters[p].default == (inspect.Parameter.empty if default is None else default), (name, p)
        assert getattr(F, name).__doc__, name
    assert tuple(sorted(api.TS_OPS, key=api.TS_OPS.get)) == R.OPS and sorted(api.TS_OPS.values()) == list(range(len(R.OPS)))
    assert tuple(sorted(api.TS_PAIR_OPS, key=api.TS_PAIR_OPS.get)) == R.PAIR_OPS and api.TS_PAIR_OPS == {"cov": 0, "corr": 1}
    assert api.TS_MIN_WINDOW == R.MIN_WINDOW and api.ROLLING_MAX_WINDOW == R.MAX_WINDOW
    assert inspect.signature(api.factor_ts).parameters["mode"].default == 0
    assert list(inspect.signature(api.factor_ts_pair).parameters) == ["x", "y", "op", "window"]
    assert "D-29" in (importlib.import_module("polars_quant_amd.factor").__doc__ or "")
    raw = (ROOT / "include" / "pq_hip.h").read_text()
    assert "D-29" in raw
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {"pq_factor_ts": ["pq_ctx *", "const pq_batch *", "const double *x", "int32_t op", "int64_t window", "int32_t mode", "double *out"],
              "pq_factor_ts_pair": ["pq_ctx *", "const pq_batch *", "const double *x", "const double *y", "int32_t op", "int64_t window",
                                    "double *out"]}
    for fn, params in protos.items():
        decl = re.search(rf"pq_status\s+{fn}\s*\(([^)]*)\)", txt)
        assert decl, f"{fn} is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, fn
    assert re.search(r"^factor_ts\s+i\s+pBpilip$", _lib._SIGNATURES, flags=re.M)
    assert re.search(r"^factor_ts_pair\s+i\s+pBppilp$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/tsops.hip" in mk and mk.count("xsec/tsops.resources.txt") == 1


ONES = np.ones((3, 40))


@pytest.mark.parametrize("call, msg", [
    (lambda f, a: a.factor_ts(ONES, 11, 5), "op"),
    (lambda f, a: a.factor_ts(ONES, -1, 5), "op"),
    (lambda f, a: a.factor_ts(ONES, True, 5), "op"),
    (lambda f, a: a.factor_ts(ONES, "sum", 5), "op"),
    (lambda f, a: a.factor_ts(ONES, 1.0, 5), "op"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, 1.0, 5), "op"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, 2, 5), "op"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, False, 5), "op"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["sum"], True), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["sum"], 5.0), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["sum"], 0), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["max"], 1025), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["std"], 1), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["zscore"], 1), "window"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, a.TS_PAIR_OPS["cov"], 1), "window"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, a.TS_PAIR_OPS["corr"], 1), "window"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, a.TS_PAIR_OPS["corr"], 1025), "window"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, a.TS_PAIR_OPS["corr"], True), "window"),
    (lambda f, a: a.factor_ts_pair(ONES, ONES, a.TS_PAIR_OPS["corr"], 2.0), "window"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["sum"], 5, 1), "mode"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["argmax"], 5, mode=1), "mode"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["rank"], 5, 2), "mode"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["rank"], 5, -1), "mode"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["rank"], 5, True), "mode"),
    (lambda f, a: a.factor_ts(ONES, a.TS_OPS["rank"], 5, 1.0), "mode"),
    (lambda f, a: a.factor_ts(np.ones(40), a.TS_OPS["sum"], 5), r"must be \[N, T\]"),
    (lambda f, a: a.factor_ts_pair(ONES, np.ones((3, 41)), a.TS_PAIR_OPS["corr"], 5), "shape"),
    (lambda f, a: a.factor_ts_pair(ONES, np.ones(40), a.TS_PAIR_OPS["cov"], 5), "shape"),
    (lambda f, a: f.ts_sum(ONES, 0), "window"),
    (lambda f, a: f.ts_std(ONES, 1), "window"),
    (lambda f, a: f.ts_zscore(ONES, 1), "window"),
    (lambda f, a: f.ts_min(ONES, 1025), "window"),
    (lambda f, a: f.ts_max(ONES, 2.5), "window"),
    (lambda f, a: f.ts_argmin(ONES, True), "window"),
    (lambda f, a: f.ts_argmax(ONES, -3), "window"),
    (lambda f, a: f.ts_rank(ONES, 0, pct=True), "window"),
    (lambda f, a: f.decay_linear(ONES, 1025), "window"),
    (lambda f, a: f.delay(ONES, 0), "window"),
    (lambda f, a: f.delta(ONES, 1025), "window"),
    (lambda f, a: f.ts_cov(ONES, ONES, 1), "window"),
    (lambda f, a: f.ts_corr(ONES, np.ones((4, 40)), 10), "shape"),
    (lambda f, a: f.ts_corr(np.ones((2, 3, 40)), np.ones((2, 3, 40)), 10), r"must be \[N, T\]"),
])
def test_argument_errors_raise_before_device_work(call, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(pq.Factor(), api)


# ---------------------------------------------------------------- the kernels' resources
def test_no_instantiation_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/tsops.hip (tsops.resources.txt, from hipcc's kernel-resource-usage
    remarks): the windowed kernel once per op 0 .. 8, the lag kernel for delay and delta, the pair kernel for cov and corr, none with
    scratch or a spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "tsops.resources.txt"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    found = re.findall(r"Function Name: \S*?(ts_\w+?_kernel)ILi(\d+)E\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [("ts_window_kernel", k) for k in range(9)] + [("ts_lag_kernel", 9), ("ts_lag_kernel", 10)] + [("ts_pair_kernel", 0), ("ts_pair_kernel", 1)]
    assert sorted((k, int(g)) for k, g, *_ in found) == sorted(want)
    for k, g, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, g, vgprs, scratch, occ, spill)
