"""-m gpu: pq_backtest_sweep_rules (csrc/sweep/sweep.hip, decision D-25) -- every cell of a parameter grid over all seven rules against the
CPU oracle (sweep_rules_ref.oracle_cells: oracle.cross / band / channel_signals, the gates and the scale as numpy comparisons,
oracle.backtest), with test_backtest_wave_gpu.check_summary: max_drawdown, max_profit, win_rate and total_trades BIT FOR BIT,
annualized_return / alpha / beta / sharpe (the device pow) at rtol 1e-12 / atol 1e-13.

Tables: one that mixes the seven rules inside every wavefront (the generic instantiation of the kernel) and seven with one rule
throughout (the instantiation of that rule).  Shapes as in test_sweep_gpu.py: a partial wavefront after a full one and a second workgroup
per symbol (P = 65, 257), the row tile R and its neighbours, and one case whose R is below the cap (79 lines)."""
import numpy as np
import pytest

import sweep_rules_ref as S
from test_backtest_wave_gpu import EXACT, bits, check_summary, special_prices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SEED = 0x5EED0003
TABLES = ["mixed", 0, 1, 2, 3, 4, 5, 6]


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()
    return pq


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C")).cuda()


def table(P, L, which):
    from polars_quant_amd import api
    return S.make_table(api.SWEEP_RULE_DTYPE, P, L, None if which == "mixed" else which)


def run(price, lines, tab, **kw):
    from polars_quant_amd import api
    got = api.backtest_sweep_rules(dev(price), [dev(l) for l in lines], tab, **kw)
    assert tuple(got.shape) == (len(tab), price.shape[0], 8) and got.stride() == (8, 8 * len(tab), 1)   # a view of [N, P, 8]
    return got.cpu().numpy()


def check_cells(got, exp, tag):
    P, N, _ = exp.shape
    check_summary(got.reshape(P * N, 8), exp.reshape(P * N, 8), tag)


def row_tile(L):
    from polars_quant_amd import api
    R = api.SWEEP_ROW_TILE(L)
    assert R >= 7 and R % 2 == 1
    return R


_inputs = {}


def inputs(oracle, N, T, L):
    """the close and the lines of a shape, computed once and never changed"""
    if (N, T, L) not in _inputs:
        close = oracle.gen_ohlcv(SEED, N, T, 0)["close"]
        lines = S.make_lines(close, L)
        for a in [close] + lines:
            a.setflags(write=False)
        _inputs[(N, T, L)] = close, lines
    return _inputs[(N, T, L)]


@pytest.mark.parametrize("Tk", ["1", "2", "R", "R+1", "3R+5"])
@pytest.mark.parametrize("P", [65, 257])
@pytest.mark.parametrize("which", TABLES)
def test_tables_and_shapes(pq, oracle, which, P, Tk):
    N, L = 3, 7
    R = row_tile(L)
    T = {"1": 1, "2": 2, "R": R, "R+1": R + 1, "3R+5": 3 * R + 5}[Tk]
    close, lines = inputs(oracle, N, T, L)
    tab = table(P, L, which)
    if which == "mixed":
        assert all((tab["rule"][w: w + 64] == r).any() for w in range(0, P - 63, 64) for r in range(7))   # every rule in every full wavefront
        assert all(((tab["c"] == -1) & (tab["rule"] == r)).any() and ((tab["c"] >= 0) & (tab["c"] < L) & (tab["rule"] == r)).any() for r in S.USES_C)
    exp = S.oracle_cells(oracle, close, lines, tab)
    check_cells(run(close, lines, tab), exp, f"{which} P={P} T={T}")
    if Tk == "3R+5":     # not vacuous
        assert (exp[..., 7] >= 1).mean() >= 0.5, (exp[..., 7] >= 1).mean()


def test_79_lines(pq, oracle):
    N, L, P = 3, 79, 65
    R = row_tile(L)
    assert R < row_tile(7)
    close, lines = inputs(oracle, N, 3 * R + 5, L)
    tab = table(P, L, "mixed")
    for f in ("a", "b", "c"):      # every other set reads the last lines instead of the first (70 = 0 mod 7: the same family of lines)
        tab[f][(tab[f] >= 0) & (tab[f] < 7) & (np.arange(P) % 2 == 1)] += 70
    assert tab["a"].max() >= 70 and tab["a"].min() < 7
    check_cells(run(close, lines, tab), S.oracle_cells(oracle, close, lines, tab), "L=79")


@pytest.mark.parametrize("which", TABLES)
def test_special_series(pq, oracle, which):
    """flat, interior / leading NULL, NaN, non-positive and every-third-row-NULL prices (which are also the p of the channel rules where
    c = -1); lines with NULL lead-ins of different lengths and interior NULLs; without and with a benchmark"""
    N, T, L, P = 9, 300, 7, 65
    d, price = special_prices(oracle, N, T)
    lines = S.add_nulls(S.make_lines(price, L), N)
    tab = table(P, L, which)
    exp = S.oracle_cells(oracle, price, lines, tab)
    check_cells(run(price, lines, tab), exp, f"special {which}")
    assert np.isfinite(exp).all()
    bench = d["open"]
    exp = S.oracle_cells(oracle, price, lines, tab, benchmark=bench)
    got = run(price, lines, tab, benchmark=dev(bench))
    check_cells(got, exp, f"special {which} + benchmark")
    nan = np.isnan(exp).any(axis=2)
    assert nan[:, [2, 3, 4, 7]].all() and not nan[:, [0, 1, 5, 6, 8]].any() and (np.isnan(got).any(axis=2) == nan).all()


@pytest.mark.parametrize("uniform", [True, False])
def test_a_nan_in_hi_does_not_refuse_the_buy(pq, oracle, uniform):
    """rule 2 against hi with a non-NULL NaN on the row of a buy (it fires) and with the NULL there (it does not); in a table of rule 2
    alone and next to other rules; also rule 4 on a base with a NaN"""
    from polars_quant_amd import api
    close = oracle.gen_ohlcv(SEED, 9, 300, 0)["close"]
    lo, hi_nan, hi_null, rows = S.nan_in_hi_case(oracle, close)
    base = close.copy()
    base[:, 50] = np.nan
    lines = [lo, hi_nan, hi_null, base]
    tab = np.zeros(2 if uniform else 4, dtype=api.SWEEP_RULE_DTYPE)
    tab["rule"], tab["a"], tab["c"] = S.CHANNEL, 0, -1
    tab["b"][:2] = [1, 2]
    if not uniform:
        tab["rule"][2:] = [S.SCALED, S.CROSS]
        tab["a"][2:], tab["b"][2:], tab["k0"][2], tab["k1"][2] = [3, 0], [0, 1], 0.99, 1.01
    for bench in (None, oracle.gen_ohlcv(SEED, 9, 300, 0)["open"]):
        exp = S.oracle_cells(oracle, close, lines, tab, benchmark=bench)
        got = run(close, lines, tab, **({} if bench is None else {"benchmark": dev(bench)}))
        check_cells(got, exp, "NaN in hi")
        assert (exp[:2, :, 7] >= 1).all() and (bits(got[0]) != bits(got[1])).any()
    buy_nan, buy_null = oracle.channel_signals(close, lo, hi_nan, 0)[0], oracle.channel_signals(close, lo, hi_null, 0)[0]
    assert all(buy_nan[n, i] == 1 and buy_null[n, i] == 0 for n, i in enumerate(rows))


def test_cross_and_band_equal_backtest_sweep_and_tables_permute(pq, oracle):
    from polars_quant_amd import api
    N, L, P = 3, 7, 130
    T = 3 * row_tile(L) + 5
    d = oracle.gen_ohlcv(SEED, N, T, 0)
    close, lines = inputs(oracle, N, T, L)
    bench = dev(d["open"])
    new = np.concatenate([table(P // 2, L, 0), table(P // 2, L, 1)])
    old = np.zeros(P, dtype=api.SWEEP_PARAM_DTYPE)
    for k in ("rule", "a", "b", "k0", "k1"):
        old[k] = new[k]
    old["b"][old["rule"] == 1] = 0       # pq_backtest_sweep ignores b under the band rule as well
    for tabs in ((new, old), (new[: P // 2], old[: P // 2]), (new[P // 2:], old[P // 2:])):   # mixed, all cross, all band
        a = run(close, lines, tabs[0], benchmark=bench)
        b = api.backtest_sweep(dev(close), [dev(l) for l in lines], tabs[1], benchmark=bench).cpu().numpy()
        assert (bits(a) == bits(b)).all()
    mixed = table(P, L, "mixed")
    base = run(close, lines, mixed, benchmark=bench)
    perm = np.random.default_rng(7).permutation(P)
    assert (bits(run(close, lines, mixed[perm], benchmark=bench)) == bits(base[perm])).all()


def test_refusals(pq, oracle):
    from polars_quant_amd import api
    N, T, L, P = 3, 60, 7, 65
    close, lines = inputs(oracle, N, T, L)
    price, dl = dev(close), [dev(l) for l in lines]
    tab = table(P, L, "mixed")
    bad = [(0, "rule", 7), (0, "rule", -1)]
    bad += [(r, "a", v) for r in range(7) for v in (-1, L)]
    bad += [(r, "b", v) for r in S.USES_B for v in (-1, L)]
    bad += [(r, "c", v) for r in S.USES_C for v in (-2, L)]
    for r, field, v in bad:
        t2 = tab.copy()
        i = 35 + r               # make_table: set i has rule i % 7
        assert t2["rule"][i] == r
        t2[field][i] = v
        out = torch.full((N, P, 8), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(pq.PqError):
            api.backtest_sweep_rules(price, dl, t2, out=out)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), ("nothing may be launched", r, field, v)
    # a field that a rule does not use may hold anything (make_table puts 10 ** 6 there; -7 is no better)
    t2 = tab.copy()
    t2["b"][~np.isin(t2["rule"], S.USES_B)] = -7
    t2["c"][~np.isin(t2["rule"], S.USES_C)] = -7
    assert (bits(api.backtest_sweep_rules(price, dl, t2).cpu().numpy()) == bits(api.backtest_sweep_rules(price, dl, tab).cpu().numpy())).all()
    # pq_backtest_sweep keeps its two rules
    old = np.zeros(3, dtype=api.SWEEP_PARAM_DTYPE)
    old["rule"][1] = 2
    with pytest.raises(pq.PqError):
        api.backtest_sweep(price, dl, old)
    assert tuple(api.backtest_sweep_rules(price, dl, tab[:0]).shape) == (0, N, 8)
    z = api.backtest_sweep_rules(price[:, :0], [l[:, :0] for l in dl], tab, out=torch.full((N, P, 8), 7.0, dtype=torch.float64, device="cuda"))
    assert tuple(z.shape) == (P, N, 8) and (z == 0).all()


# ---- the seven methods against the loops they replace -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(pq, oracle):
    d = oracle.gen_ohlcv(SEED, 9, 300, 0)
    return {k: dev(d[k]) for k in ("open", "high", "low", "close", "volume")}


def against_the_loop(pq, df, res, strategy_args, P):
    """res: the SweepResult; strategy_args(i) -> (method name, kwargs) of set i -> the sweep's [P, 9, 8] summary"""
    from polars_quant_amd import api
    assert tuple(res.summary.shape) == (P, 9, 8)
    got = res.summary.cpu().numpy()
    strat = pq.Strategy()
    for i in range(P):
        name, kw = strategy_args(i)
        sig = getattr(strat, name)(df, **kw)
        loop = api.backtest_vectorized(df["close"], sig["buy_signal"], sig["sell_signal"], want_curves=False)[3].cpu().numpy()
        for k in EXACT:
            assert (bits(got[i, :, k]) == bits(loop[:, k])).all(), (name, kw, k)
        np.testing.assert_allclose(got[i], loop, rtol=1e-12, atol=1e-13, err_msg=f"{name} {kw}")
    assert (got[..., 7] >= 1).mean() >= 0.9, (got[..., 7] >= 1).mean()
    return got


def test_bband(pq, frame):
    res = pq.ParameterSweep(frame).bband((10, 20), (1.0, 1.5, 2.0))
    against_the_loop(pq, frame, res, lambda i: ("bband", dict(period=int(res.params["period"][i]), nbdev=float(res.params["nbdev"][i]))), 6)


def ungated_differs(pq, frame, got, lines):
    """at least one cell of the gated sweep differs from the plain cross of the same lines"""
    from polars_quant_amd import api
    plain = api.backtest_sweep(frame["close"], lines, {"rule": [0], "a": [0], "b": [1]}).cpu().numpy()[0]
    return any((bits(g) != bits(plain)).any() for g in got)


def test_stoch(pq, frame):
    from polars_quant_amd import api
    res = pq.ParameterSweep(frame).stoch((5, 9), 3, 3, (20, 30), (70, 80))
    pr = res.params
    got = against_the_loop(pq, frame, res, lambda i: ("stoch", dict(fastk_period=int(pr["fastk_period"][i]), slowk_period=int(pr["slowk_period"][i]),
                                                                   slowd_period=int(pr["slowd_period"][i]), oversold=float(pr["oversold"][i]),
                                                                   overbought=float(pr["overbought"][i]))), 8)
    kd = list(api.call("stoch", frame["high"], frame["low"], frame["close"], fastk_period=5, slowk_period=3, slowd_period=3))
    assert pr["fastk_period"][:4].tolist() == [5] * 4 and ungated_differs(pq, frame, got[:4], kd)


def test_cci(pq, frame):
    res = pq.ParameterSweep(frame).cci((14, 20), (-100, -50), (50, 100))
    pr = res.params
    against_the_loop(pq, frame, res, lambda i: ("cci", dict(period=int(pr["period"][i]), oversold=float(pr["oversold"][i]),
                                                            overbought=float(pr["overbought"][i]))), 8)


def test_adx(pq, frame):
    from polars_quant_amd import api
    res = pq.ParameterSweep(frame).adx((7, 14), (15, 20, 25))
    pr = res.params
    got = against_the_loop(pq, frame, res, lambda i: ("adx", dict(period=int(pr["period"][i]), threshold=float(pr["threshold"][i]))), 6)
    dm = [api.call(nm, frame["high"], frame["low"], timeperiod=7)[0] for nm in ("plus_dm", "minus_dm")]
    assert pr["period"][:3].tolist() == [7] * 3 and ungated_differs(pq, frame, got[:3], dm)


def test_breakout(pq, frame):
    from polars_quant_amd import api
    res = pq.ParameterSweep(frame).breakout((5, 10, 20, 55))
    got = against_the_loop(pq, frame, res, lambda i: ("breakout", dict(period=int(res.params["period"][i]))), 4)
    # a backtest on another price column: the signal is still taken on the close, which then travels as one more line
    other = pq.ParameterSweep(frame).breakout((5, 10, 20, 55), price_col="open").summary.cpu().numpy()
    strat = pq.Strategy()
    for i, p in enumerate((5, 10, 20, 55)):
        sig = strat.breakout(frame, period=p)
        loop = api.backtest_vectorized(frame["open"], sig["buy_signal"], sig["sell_signal"], want_curves=False)[3].cpu().numpy()
        check_summary(other[i], loop, f"breakout on the open, period {p}")
    assert (bits(other) != bits(got)).any()


def test_reversion(pq, frame):
    res = pq.ParameterSweep(frame).reversion((10, 20), (1.0, 1.5, 2.0))
    pr = res.params
    against_the_loop(pq, frame, res, lambda i: ("reversion", dict(period=int(pr["period"][i]), threshold=float(pr["threshold"][i]))), 6)


def test_grid(pq, frame):
    res = pq.ParameterSweep(frame).grid((10, 20), (1, 2, 5))
    pr = res.params
    against_the_loop(pq, frame, res, lambda i: ("grid", dict(base_period=int(pr["base_period"][i]), grid_pct=float(pr["grid_pct"][i]))), 6)


def test_run_rules_and_the_line_limit(pq, frame, oracle):
    from polars_quant_amd import api
    close_h = frame["close"].cpu().numpy()
    lines = S.make_lines(close_h, 7)
    tab = table(20, 7, "mixed")
    res = pq.ParameterSweep(frame).run_rules([dev(l) for l in lines], tab)
    check_cells(res.summary.cpu().numpy(), S.oracle_cells(oracle, close_h, lines, tab), "run_rules")
    assert sorted(res.params) == sorted(api.SWEEP_RULE_DTYPE.names) and res.params["c"].tolist() == tab["c"].tolist()
    sw = pq.ParameterSweep(frame)
    many = list(range(2, 2 + api.SWEEP_MAX_LINES + 1))
    for call in (lambda: sw.bband(many[:129], [1.0, 1.5]), lambda: sw.stoch(many[:257], [3], [3], [20], [80]), lambda: sw.cci(many, [-100], [100]),
                 lambda: sw.adx(many[:171], [25]), lambda: sw.breakout(many[:257]), lambda: sw.reversion(many, [2.0]), lambda: sw.grid(many, [5.0])):
        with pytest.raises(ValueError, match="lines"):
            call()
