"""not-gpu: the scalar restatement of one cell of pq_backtest_sweep_rules for all seven rules (tests/sweep_rules_ref.py) against the C
oracle's signals + backtest, the host-only grid builders of polars_quant_amd/sweep.py for bband / stoch / cci / adx / breakout /
reversion / grid, api.sweep_rules, and -- on the oracle alone -- that the grids test_sweep_rules_gpu.py uses trade."""
import os
import re

import numpy as np
import pytest

import sweep_rules_ref as S

SEED = 0x5EED0003
N, T, L = 9, 300, 7
RULE_DTYPE = np.dtype([("rule", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("k0", "<f8"), ("k1", "<f8")])


def check(got, exp, tag):
    """EXACT columns bit for bit, the others at the project's rtol = 1e-12 / atol = 1e-13"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert np.isfinite(exp).all(), tag
    for k in S.EXACT:
        assert (S.bits(got[..., k]) == S.bits(exp[..., k])).all(), (tag, "exact column", k)
    for k in S.TOL:
        np.testing.assert_allclose(got[..., k], exp[..., k], rtol=1e-12, atol=1e-13, err_msg=f"{tag} column {k}")


def ref_cells(price, lines, tab, bench=None, **costs):
    out = []
    for q in tab:
        col = lambda j: price if j < 0 else lines[j]
        a = lines[q["a"]]
        b = lines[q["b"]] if q["rule"] in S.USES_B else a
        c = col(q["c"]) if q["rule"] in S.USES_C else a
        out.append([S.sweep_rule_cell(price[n], a[n], b[n], c[n], q["rule"], q["k0"], q["k1"], bench=None if bench is None else bench[n], **costs)
                    for n in range(price.shape[0])])
    return np.array(out)


@pytest.fixture(scope="module")
def data(oracle):
    d = oracle.gen_ohlcv(SEED, N, T, 0)
    lines = S.add_nulls(S.make_lines(d["close"], L), N)
    return d, d["close"], lines


def test_null_is_the_abi_null(oracle):
    assert S.bits(np.array([S.NULL]))[0] == S.bits(np.array([oracle.NULL]))[0] == S.NULL_BITS
    assert S.is_null(float(oracle.NULL)) and not S.is_null(float("nan"))


def test_every_rule_matches_the_oracle(oracle, data):
    """all seven rules mixed in one table, c = -1 and c >= 0, NULL lead-ins and interior NULLs in the lines"""
    _d, close, lines = data
    tab = S.make_table(RULE_DTYPE, 42, L)
    assert sorted(set(tab["rule"].tolist())) == list(range(7))
    for r in S.USES_C:
        cs = tab["c"][tab["rule"] == r]
        assert (cs == -1).any() and (cs >= 0).any(), r
    exp = S.oracle_cells(oracle, close, lines, tab)
    check(ref_cells(close, lines, tab), exp, "mixed")
    for r in range(7):       # a rule that never trades proves nothing
        assert (exp[tab["rule"] == r][..., 7] >= 1).mean() >= 0.5, r


def test_benchmark_costs_and_invalid_prices(oracle, data):
    d, close, lines = data
    costs = dict(initial_capital=5000.0, buy_slippage=0.01, sell_slippage=0.02, min_commission=20.0, position_size=0.5)
    price = close.copy()
    price[2, 100:105] = oracle.NULL      # a NULL price is also a NULL p of the channel rules (c = -1)
    price[5, 7] = -1.0
    tab = S.make_table(RULE_DTYPE, 21, L)
    exp = S.oracle_cells(oracle, price, lines, tab, benchmark=d["open"], **costs)
    got = ref_cells(price, lines, tab, bench=d["open"], **costs)
    ok = ~np.isnan(exp).any(axis=2)
    assert not ok[:, 2].any() and ok[:, [0, 1, 3, 4, 5, 6, 7, 8]].all()
    assert np.isnan(got[:, 2]).any(axis=1).all()
    check(got[ok], exp[ok], "benchmark + costs")


def test_a_nan_in_hi_does_not_refuse_the_buy(oracle, data):
    """ChannelSigOp<0> tests the other side's column for the NULL, not for a NaN: with a non-NULL NaN in hi the buy of that row fires,
    with a NULL there it does not"""
    _d, close, lines = data
    lo, hi_nan, hi_null, rows = S.nan_in_hi_case(oracle, close)
    ls = [lo, hi_nan, hi_null]
    tab = np.zeros(2, dtype=RULE_DTYPE)
    tab["rule"], tab["a"], tab["b"], tab["c"] = S.CHANNEL, 0, [1, 2], -1
    for n, i in enumerate(rows):
        f = lambda x: [float(v) for v in x[n]]
        assert S.rule_signals(S.CHANNEL, f(lo), f(hi_nan), f(close), 0.0, 0.0)[0][i]
        assert not S.rule_signals(S.CHANNEL, f(lo), f(hi_null), f(close), 0.0, 0.0)[0][i]
        assert oracle.channel_signals(close, lo, hi_nan, 0)[0][n, i] == 1 and oracle.channel_signals(close, lo, hi_null, 0)[0][n, i] == 0
    exp = S.oracle_cells(oracle, close, ls, tab)
    check(ref_cells(close, ls, tab), exp, "NaN in hi")
    assert (S.bits(exp[0]) != S.bits(exp[1])).any() and (exp[..., 7] >= 1).all()
    # the same through the scaled channel: a NaN base is a NaN lo and hi, never a NULL
    base = close.copy()
    base[:, 50] = np.nan
    tab4 = np.zeros(1, dtype=RULE_DTYPE)
    tab4["rule"], tab4["a"], tab4["c"], tab4["k0"], tab4["k1"] = S.SCALED, 0, -1, 0.99, 1.01
    check(ref_cells(close, [base], tab4), S.oracle_cells(oracle, close, [base], tab4), "NaN base")


# ---- the grid builders ----------------------------------------------------------------------------------------------------------------
def test_bband_and_grid_grids():
    from polars_quant_amd import api, sweep
    pairs, rules, params = sweep.bband_grid([10, 20, 10], [1.0, 1.5, 2.0])
    assert pairs == [(p, d) for p in (10, 20) for d in (1.0, 1.5, 2.0)]
    assert rules.dtype == api.SWEEP_RULE_DTYPE and (rules["rule"] == 2).all() and (rules["c"] == -1).all()
    assert rules["a"].tolist() == [0, 2, 4, 6, 8, 10] and rules["b"].tolist() == [1, 3, 5, 7, 9, 11]
    assert params["period"].tolist() == [10] * 3 + [20] * 3 and params["nbdev"].tolist() == [1.0, 1.5, 2.0] * 2
    ps, rules, params = sweep.grid_grid([10, 20], [1, 2, 5])
    assert ps == [10, 20] and (rules["rule"] == 4).all() and (rules["c"] == -1).all() and rules["a"].tolist() == [0] * 3 + [1] * 3
    # the doubles of Strategy.grid
    assert rules["k0"].tolist() == [1.0 - g / 100.0 for g in (1.0, 2.0, 5.0)] * 2 and rules["k1"].tolist() == [1.0 + g / 100.0 for g in (1.0, 2.0, 5.0)] * 2
    assert params["base_period"].tolist() == [10] * 3 + [20] * 3 and params["grid_pct"].tolist() == [1.0, 2.0, 5.0] * 2
    for bad in ([], [2.5]):
        with pytest.raises(ValueError):
            sweep.bband_grid(bad, [2.0])
        with pytest.raises(ValueError):
            sweep.grid_grid(bad, [2.0])


def test_stoch_and_adx_grids():
    from polars_quant_amd import sweep
    triples, rules, params = sweep.stoch_grid([5, 9], [3], [3, 5], [20, 30], [70, 80])
    assert triples == [(5, 3, 3), (5, 3, 5), (9, 3, 3), (9, 3, 5)] and len(rules) == 16
    want = [(j, lo, hi) for j in range(4) for lo in (20.0, 30.0) for hi in (70.0, 80.0)]
    assert (rules["rule"] == 5).all()
    assert rules["a"].tolist() == [2 * w[0] for w in want] and rules["b"].tolist() == [2 * w[0] + 1 for w in want]
    assert rules["c"].tolist() == rules["a"].tolist()                                    # the zones are %K's
    assert rules["k0"].tolist() == [w[1] for w in want] and rules["k1"].tolist() == [w[2] for w in want]
    assert [params[k].tolist() for k in ("fastk_period", "slowk_period", "slowd_period")] == [[triples[w[0]][j] for w in want] for j in range(3)]
    assert (params["oversold"] == rules["k0"]).all() and (params["overbought"] == rules["k1"]).all()
    ps, rules, params = sweep.adx_grid([7, 14], [15, 20, 25])
    assert ps == [7, 14] and (rules["rule"] == 6).all()
    assert rules["a"].tolist() == [0] * 3 + [3] * 3 and rules["b"].tolist() == [1] * 3 + [4] * 3 and rules["c"].tolist() == [2] * 3 + [5] * 3
    assert rules["k0"].tolist() == [15.0, 20.0, 25.0] * 2 and params["period"].tolist() == [7] * 3 + [14] * 3
    assert (params["threshold"] == rules["k0"]).all()
    for bad in ([], [2.5]):
        with pytest.raises(ValueError):
            sweep.stoch_grid(bad, [3], [3], [20], [80])
        with pytest.raises(ValueError):
            sweep.stoch_grid([5], bad, [3], [20], [80])
        with pytest.raises(ValueError):
            sweep.stoch_grid([5], [3], bad, [20], [80])
        with pytest.raises(ValueError):
            sweep.adx_grid(bad, [25])


def test_cci_reversion_and_breakout_grids():
    from polars_quant_amd import sweep
    ps, rules, params = sweep.cci_grid([14, 20, 14], [-100, -50], [50, 100])
    assert ps == [14, 20] and len(rules) == 8 and (rules["rule"] == 1).all() and rules["a"].tolist() == [0] * 4 + [1] * 4
    assert list(zip(rules["k0"][:4].tolist(), rules["k1"][:4].tolist())) == [(lo, hi) for lo in (-100.0, -50.0) for hi in (50.0, 100.0)]
    assert params["period"].tolist() == [14] * 4 + [20] * 4 and (params["oversold"] == rules["k0"]).all() and (params["overbought"] == rules["k1"]).all()
    ps, rules, params = sweep.reversion_grid([10, 20], [1.0, 1.5, 2.0])
    assert ps == [10, 20] and (rules["rule"] == 1).all() and rules["a"].tolist() == [0] * 3 + [1] * 3
    assert rules["k0"].tolist() == [-1.0, -1.5, -2.0] * 2 and rules["k1"].tolist() == [1.0, 1.5, 2.0] * 2
    assert params["threshold"].tolist() == [1.0, 1.5, 2.0] * 2 and params["period"].tolist() == [10] * 3 + [20] * 3
    ps, rules, params = sweep.breakout_grid([5, 10, 20, 55])
    assert ps == [5, 10, 20, 55] and (rules["rule"] == 3).all() and (rules["c"] == -1).all()
    assert rules["a"].tolist() == [0, 2, 4, 6] and rules["b"].tolist() == [1, 3, 5, 7] and params["period"].tolist() == ps
    _ps, rules, _params = sweep.breakout_grid([5, 10], close_is_price=False)
    assert rules["c"].tolist() == [4, 4]                                                 # the close as one more line
    for bad in ([], [2.5]):
        for grid in (lambda x: sweep.cci_grid(x, [-100], [100]), lambda x: sweep.reversion_grid(x, [2.0]), sweep.breakout_grid):
            with pytest.raises(ValueError):
                grid(bad)


def test_a_grid_beyond_the_line_limit_is_refused_on_the_host():
    """before any device work: the frame is never touched"""
    import polars_quant_amd as pq
    from polars_quant_amd import api

    class Untouched(dict):
        def __getitem__(self, k):
            raise AssertionError("the frame was read")
    sw = pq.ParameterSweep(Untouched())
    many = list(range(2, 2 + api.SWEEP_MAX_LINES + 1))
    for call in (lambda: sw.bband(many[:129], [1.0, 1.5]), lambda: sw.stoch(many[:257], [3], [3], [20], [80]), lambda: sw.cci(many, [-100], [100]),
                 lambda: sw.adx(many[:171], [25]), lambda: sw.breakout(many[:257]), lambda: sw.breakout(many[:256], price_col="open"),
                 lambda: sw.reversion(many, [2.0]), lambda: sw.grid(many, [5.0])):
        with pytest.raises(ValueError, match="lines"):
            call()


def test_sweep_rules_from_columns():
    from polars_quant_amd import api
    assert api.SWEEP_RULE_DTYPE == RULE_DTYPE and api.SWEEP_RULE_DTYPE.itemsize == 32 and api.SWEEP_RULE_DTYPE.names == ("rule", "a", "b", "c", "k0", "k1")
    assert [api.SWEEP_RULE_DTYPE.fields[k][1] for k in api.SWEEP_RULE_DTYPE.names] == [api.SWEEP_PARAM_DTYPE.fields[k][1] for k in api.SWEEP_PARAM_DTYPE.names]
    tab = api.sweep_rules({"rule": [2, 6], "a": [1, 0], "b": [0, 1], "c": [-1, 2], "k0": [0.0, 25.0]})
    assert tab.dtype == api.SWEEP_RULE_DTYPE and tab["c"].tolist() == [-1, 2] and tab["k1"].tolist() == [0.0, 0.0]
    assert len(api.sweep_rules(tab)) == 2
    with pytest.raises(ValueError):
        api.sweep_rules({"rule": [0, 1], "a": [0]})
    with pytest.raises(ValueError):
        api.sweep_rules({"rule": [0], "a": [0], "period": [14]})
    with pytest.raises(ValueError):
        api.sweep_rules(np.zeros(2, dtype=api.SWEEP_PARAM_DTYPE))      # the other table: its fourth field is padding, not c
    # the surface the issue leaves alone
    assert api.SWEEP_PARAM_DTYPE.names == ("rule", "a", "b", "_pad", "k0", "k1")


# ---- the grids of test_sweep_rules_gpu.py, on the oracle alone -------------------------------------------------------------------------
def test_the_gpu_grids_trade_and_the_gates_bite(oracle):
    d = oracle.gen_ohlcv(SEED, 9, 300, 0)
    o, h, l, c = d["open"], d["high"], d["low"], d["close"]
    trades = lambda sig: oracle.backtest(c, *sig)[3][:, 7]
    share = {}
    cells = []
    for p in (10, 20):
        for dev in (1.0, 1.5, 2.0):
            up, _mid, lo = oracle.call("bbands", c, timeperiod=p, nbdevup=dev, nbdevdn=dev)
            cells.append(trades(oracle.channel_signals(c, lo, up, 0)))
    share["bband"] = (np.array(cells) >= 1).mean()
    cells, differs = [], False
    with np.errstate(invalid="ignore"):
        for fk in (5, 9):
            k, dd = oracle.call("stoch", h, l, c, fastk_period=fk, slowk_period=3, slowd_period=3)
            buy, sell = oracle.cross_signals(k, dd)
            for lo in (20.0, 30.0):
                for hi in (70.0, 80.0):
                    gated = (buy & (k < lo)).astype(np.uint8), (sell & (k > hi)).astype(np.uint8)
                    cells.append(trades(gated))
                    differs |= bool((S.bits(oracle.backtest(c, *gated)[3]) != S.bits(oracle.backtest(c, buy, sell)[3])).any())
        share["stoch"] = (np.array(cells) >= 1).mean()
        assert differs, "stoch: the zones change no cell"
        cells, differs = [], False
        for p in (7, 14):
            (pdm,), (mdm,), (adx,) = (oracle.call("plus_dm", h, l, timeperiod=p), oracle.call("minus_dm", h, l, timeperiod=p),
                                     oracle.call("adx", h, l, c, timeperiod=p))
            buy, sell = oracle.cross_signals(pdm, mdm)
            for th in (15.0, 20.0, 25.0):
                gated = (buy & (adx > th)).astype(np.uint8), (sell & (adx > th)).astype(np.uint8)
                cells.append(trades(gated))
                differs |= bool((S.bits(oracle.backtest(c, *gated)[3]) != S.bits(oracle.backtest(c, buy, sell)[3])).any())
        share["adx"] = (np.array(cells) >= 1).mean()
        assert differs, "adx: the strength gate changes no cell"
    cells = []
    for p in (14, 20):
        (cci,) = oracle.call("cci", h, l, c, timeperiod=p)
        cells += [trades(oracle.band_signals(cci, lo, hi)) for lo in (-100.0, -50.0) for hi in (50.0, 100.0)]
    share["cci"] = (np.array(cells) >= 1).mean()
    cells = [trades(oracle.channel_signals(c, oracle.call("rolling_min", l, window=p)[0], oracle.call("rolling_max", h, window=p)[0], 1)) for p in (5, 10, 20, 55)]
    share["breakout"] = (np.array(cells) >= 1).mean()
    cells = []
    for p in (10, 20):
        up, mid, _lo = oracle.call("bbands", c, timeperiod=p, nbdevup=1.0, nbdevdn=1.0)
        z = np.where(S.bits(up) == S.NULL_BITS, up, (c - mid) / (up - mid))
        cells += [trades(oracle.band_signals(z, -th, th)) for th in (1.0, 1.5, 2.0)]
    share["reversion"] = (np.array(cells) >= 1).mean()
    cells = []
    for p in (10, 20):
        (base,) = oracle.call("sma", c, timeperiod=p)
        null = S.bits(base) == S.NULL_BITS
        for g in (1.0, 2.0, 5.0):
            cells.append(trades(oracle.channel_signals(c, np.where(null, base, base * (1.0 - g / 100.0)), np.where(null, base, base * (1.0 + g / 100.0)), 0)))
    share["grid"] = (np.array(cells) >= 1).mean()
    print({k: round(float(v), 2) for k, v in share.items()})
    assert all(v >= 0.9 for v in share.values()), share
    assert {k: round(float(v), 2) for k, v in share.items()} == dict(bband=1.0, stoch=1.0, cci=1.0, adx=1.0, breakout=0.97, reversion=1.0, grid=0.93)


def test_no_sweep_instantiation_uses_scratch():
    """The build writes the register / scratch figures of every instantiation of the sweep kernel (csrc/sweep/sweep.resources.txt, from
    hipcc's kernel-resource-usage remarks): seven rules and the generic one, each with and without a benchmark, none with scratch or a
    spilled VGPR, all at two waves per SIMD."""
    path = os.path.join(os.path.dirname(__file__), "..", "polars_quant_amd", "csrc", "sweep", "sweep.resources.txt")
    if not os.path.exists(path):
        pytest.skip("sweep.resources.txt not built (make -C polars_quant_amd/csrc)")
    found = re.findall(r"Function Name: \S*sweep_kernelILi(n?\d)ELb([01])E\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", open(path).read())
    assert sorted((r, b) for r, b, *_ in found) == sorted((r, b) for r in ("n1", "0", "1", "2", "3", "4", "5", "6") for b in "01")
    for r, b, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0 and int(occ) >= 2 and int(vgprs) <= 256, (r, b, vgprs, scratch, occ, spill)
