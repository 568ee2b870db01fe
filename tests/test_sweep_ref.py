"""not-gpu: the scalar restatement of the sweep kernel's algorithm (tests/sweep_ref.py: rule + scan + two-walk streaming summary, no
equity array) against the C oracle's signals + backtest, and the host-only grid builders of polars_quant_amd/sweep.py."""
import itertools

import numpy as np
import pytest

import sweep_ref as R

SEED = 0x5EED0003
EXACT, TOL = (1, 5, 6, 7), (0, 2, 3, 4)     # test_backtest_wave_gpu.check_summary
PERIODS = (3, 5, 8, 13, 21, 34)
BANDS = ((20.0, 80.0), (30.0, 70.0), (40.0, 60.0), (45.0, 55.0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(got, exp, tag):
    """EXACT columns bit for bit, the others at the project's rtol = 1e-12 / atol = 1e-13; -> whether every column has the same bits"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert np.isfinite(exp).all(), tag
    for k in EXACT:
        assert (bits(got[..., k]) == bits(exp[..., k])).all(), (tag, "exact column", k)
    for k in TOL:
        np.testing.assert_allclose(got[..., k], exp[..., k], rtol=1e-12, atol=1e-13, err_msg=f"{tag} column {k}")
    return bool((bits(got) == bits(exp)).all())


@pytest.fixture(scope="module")
def data(oracle):
    d = oracle.gen_ohlcv(SEED, 9, 300, 0)
    close = d["close"]
    sma = {p: oracle.call("sma", close, timeperiod=p)[0] for p in PERIODS}
    (rsi,) = oracle.call("rsi", close, timeperiod=14)
    return close, sma, rsi, d["open"]


def test_cross_cells_match_the_oracle(oracle, data):
    close, sma, _rsi, _bench = data
    pairs = list(itertools.combinations(PERIODS, 2))
    assert len(pairs) == 15
    exp = np.stack([oracle.backtest(close, *oracle.cross_signals(sma[f], sma[s]))[3] for f, s in pairs])       # [15, 9, 8]
    got = np.array([[R.sweep_cell(close[n], sma[f][n], sma[s][n], 0) for n in range(9)] for f, s in pairs])
    same = check(got, exp, "cross")
    print("cross: every column bit-identical to the oracle:", same)
    # a grid where nothing trades proves nothing
    assert (exp[..., 7] >= 2).mean() >= 0.9
    assert ((exp[..., 6] > 0) & (exp[..., 6] < 1)).mean() >= 0.8


def test_band_cells_match_the_oracle(oracle, data):
    close, _sma, rsi, _bench = data
    exp = np.stack([oracle.backtest(close, *oracle.band_signals(rsi, lo, hi))[3] for lo, hi in BANDS])          # [4, 9, 8]
    got = np.array([[R.sweep_cell(close[n], rsi[n], rsi[n], 1, lo, hi) for n in range(9)] for lo, hi in BANDS])
    same = check(got, exp, "band")
    print("band: every column bit-identical to the oracle:", same)
    assert (exp[..., 7] >= 1).any()


def test_benchmark_costs_and_invalid_prices_match_the_oracle(oracle, data):
    close, sma, _rsi, bench = data
    costs = dict(initial_capital=5000.0, buy_slippage=0.01, sell_slippage=0.02, min_commission=20.0, position_size=0.5)
    price = close.copy()
    price[2, 100:105] = oracle.NULL
    price[5, 7] = -1.0
    a, b = sma[5], sma[21]
    exp = oracle.backtest(price, *oracle.cross_signals(a, b), benchmark=bench, **costs)[3]
    got = np.array([R.sweep_cell(price[n], a[n], b[n], 0, bench=bench[n], **costs) for n in range(9)])
    ok = ~np.isnan(exp).any(axis=1)
    assert ok.sum() == 8 and not ok[2]                       # the NULL prices make the oracle's row NaN, and ours
    assert np.isnan(got[2]).any()
    check(got[ok], exp[ok], "benchmark + costs")
    assert (exp[ok][:, 3] != 0).all()                         # a beta was computed
    assert R.sweep_cell([], [], [], 0) == [0.0] * 8           # no rows: zeros (metrics.rs:17-19)


def test_ma_grid_keeps_fast_below_slow_and_shares_lines():
    from polars_quant_amd import api, sweep
    fasts, slows = range(5, 55, 5), range(20, 220, 20)
    periods, rules, params = sweep.ma_grid(fasts, slows)
    want = [(f, s) for f in fasts for s in slows if f < s]
    assert list(zip(params["fast"].tolist(), params["slow"].tolist())) == want and len(want) == 90
    assert periods == sorted(set(fasts) | set(slows)) and len(periods) == 18           # 20 and 40 are one line each
    assert rules.dtype == api.SWEEP_PARAM_DTYPE and rules.dtype.itemsize == 32
    assert (rules["rule"] == 0).all()
    assert [periods[j] for j in rules["a"]] == [f for f, _ in want] and [periods[j] for j in rules["b"]] == [s for _, s in want]
    # a period that no pair uses is no line
    periods, rules, params = sweep.ma_grid([10, 50], [20, 30])
    assert periods == [10, 20, 30] and len(rules) == 2
    with pytest.raises(ValueError):
        sweep.ma_grid([], [20])
    with pytest.raises(ValueError):
        sweep.ma_grid([2.5], [20])


def test_rsi_and_macd_grids():
    from polars_quant_amd import sweep
    ps, rules, params = sweep.rsi_grid([14, 7], [20, 30], [70, 75, 80])
    assert ps == [14, 7] and len(rules) == 2 * 2 * 3
    assert (rules["rule"] == 1).all() and rules["a"].tolist() == [0] * 6 + [1] * 6
    assert params["period"].tolist() == [14] * 6 + [7] * 6
    assert list(zip(rules["k0"][:6].tolist(), rules["k1"][:6].tolist())) == [(lo, hi) for lo in (20.0, 30.0) for hi in (70.0, 75.0, 80.0)]
    assert (params["oversold"] == rules["k0"]).all() and (params["overbought"] == rules["k1"]).all()
    triples, rules, params = sweep.macd_grid([8, 12, 30], [26, 30], [9, 5])
    assert triples == [(8, 26, 9), (8, 26, 5), (8, 30, 9), (8, 30, 5), (12, 26, 9), (12, 26, 5), (12, 30, 9), (12, 30, 5)]
    assert rules["a"].tolist() == list(range(0, 16, 2)) and rules["b"].tolist() == list(range(1, 16, 2)) and (rules["rule"] == 0).all()
    assert [params[k].tolist() for k in ("fast", "slow", "signal")] == [list(c) for c in zip(*triples)]


def test_sweep_params_from_columns():
    from polars_quant_amd import api
    tab = api.sweep_params({"rule": [0, 1], "a": [1, 0], "b": [0, 0], "k0": [0.0, 30.0], "k1": [0.0, 70.0]})
    assert tab.dtype == api.SWEEP_PARAM_DTYPE and tab["k1"].tolist() == [0.0, 70.0] and tab["_pad"].tolist() == [0, 0]
    assert api.sweep_params(tab) is not None and len(api.sweep_params(tab)) == 2
    with pytest.raises(ValueError):
        api.sweep_params({"rule": [0, 1], "a": [0]})
    with pytest.raises(ValueError):
        api.sweep_params({"rule": [0], "a": [0], "period": [14]})
