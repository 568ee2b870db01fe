"""-m gpu: pq_backtest_sweep (csrc/sweep/sweep.hip, decision D-25) -- every cell of a parameter grid against the CPU oracle's
signals + backtest (oracle/backtest.c:263-278, :65-104, :7-61), with test_backtest_wave_gpu.check_summary: max_drawdown, max_profit,
win_rate and total_trades BIT FOR BIT, annualized_return / alpha / beta / sharpe (the device pow) at rtol 1e-12 / atol 1e-13.

Shapes are the smallest at which the kernel takes another path: a partial / full / several wavefronts and a second workgroup per symbol
(P around 64 and 256), the row tile R = api.SWEEP_ROW_TILE(n_lines) and its neighbours (one tile, a one-row last tile, several tiles),
1 .. 256 lines (256 lines: a smaller R, and four wavefronts needed to carry a tile whatever P is)."""
import numpy as np
import pytest

from test_backtest_wave_gpu import EXACT, bits, check_summary, special_prices

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SEED = 0x5EED0003


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()
    return pq


def make_lines(N, T, L):
    """L oscillating columns around 50 that cross each other and the band thresholds often (the kernel does not care what a line means)"""
    t = np.arange(T, dtype=np.float64)[None, :]
    n = np.arange(N, dtype=np.float64)[:, None]
    return [50.0 + 30.0 * np.sin(0.9 / (1.0 + 0.37 * (j % 11)) * t + 1.3 * j + 0.7 * n) + 5.0 * np.cos(0.31 * t * (1 + j % 3) + n) for j in range(L)]


def make_table(api, P, L):
    """cross and band rules mixed inside every wavefront, some a == b (a cross of a line with itself never signals)"""
    i = np.arange(P)
    tab = np.zeros(P, dtype=api.SWEEP_PARAM_DTYPE)
    tab["rule"] = (i % 3 == 2).astype(np.int32)
    tab["a"] = (i * 7 + 1) % L
    tab["b"] = (i * 3 + i // L) % L
    tab["k0"] = 30.0 + 5.0 * (i % 4)
    tab["k1"] = 70.0 - 5.0 * (i % 3)
    if P > 5:
        tab["b"][5] = tab["a"][5]
        tab["rule"][5] = 0
    return tab


def oracle_cells(oracle, price, lines, tab, benchmark=None, **costs):
    """-> [P, N, 8]: the oracle's summary of every parameter set (equal sets are computed once)"""
    memo = {}
    out = []
    for q in tab:
        key = (int(q["rule"]), int(q["a"]), int(q["b"]) if q["rule"] == 0 else -1, float(q["k0"]), float(q["k1"]))
        if key not in memo:
            sig = (oracle.cross_signals(lines[q["a"]], lines[q["b"]]) if q["rule"] == 0
                   else oracle.band_signals(lines[q["a"]], float(q["k0"]), float(q["k1"])))
            memo[key] = oracle.backtest(price, *sig, benchmark=benchmark, **costs)[3].reshape(price.shape[0], 8)
        out.append(memo[key])
    return np.stack(out)


def run(api, price, lines, tab, **kw):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got = api.backtest_sweep(dev(price), [dev(l) for l in lines], tab, **kw)
    assert tuple(got.shape) == (len(tab), price.shape[0], 8) and got.stride() == (8, 8 * len(tab), 1)   # a view of [N, P, 8]
    return got.cpu().numpy()


def check_cells(got, exp, tag):
    P, N, _ = exp.shape
    check_summary(got.reshape(P * N, 8), exp.reshape(P * N, 8), tag)


def case(pq, oracle, N, P, L, T, tag):
    from polars_quant_amd import api
    price = oracle.gen_ohlcv(SEED, N, T, 0)["close"]
    lines, tab = make_lines(N, T, L), make_table(api, P, L)
    exp = oracle_cells(oracle, price, lines, tab)
    got = run(api, price, lines, tab)
    check_cells(got, exp, tag)
    return got, exp, tab


def row_tile(L):
    from polars_quant_amd import api
    R = api.SWEEP_ROW_TILE(L)
    assert R >= 7 and R % 2 == 1      # odd: the pitch of a line in LDS
    return R


@pytest.mark.parametrize("N", [1, 3, 9])
def test_symbols(pq, oracle, N):
    got, exp, tab = case(pq, oracle, N, 65, 7, row_tile(7) + 1, f"N={N}")
    # not vacuous: most cells trade, and the cross of a line with itself never does
    assert (exp[tab["a"] != tab["b"], :, 7] >= 2).mean() > 0.9
    assert (got[5, :, 7] == 0).all() and tab["a"][5] == tab["b"][5]


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130, 200, 257])   # 257: a second workgroup per symbol
def test_parameter_sets(pq, oracle, P):
    case(pq, oracle, 3, P, 7, 3 * row_tile(7) + 5, f"P={P}")


@pytest.mark.parametrize("L", [1, 2, 7, 33, 79, 256])            # 79: R < the cap; 256: R = 15 and four wavefronts carry a tile
def test_lines(pq, oracle, L):
    R = row_tile(L)
    case(pq, oracle, 3 if L < 256 else 1, 65, L, (R + 1) if L < 79 else 3 * R + 5, f"L={L}")


@pytest.mark.parametrize("Tk", ["1", "2", "R-1", "R", "R+1", "3R+5"])
def test_rows(pq, oracle, Tk):
    R = row_tile(7)
    T = {"1": 1, "2": 2, "R-1": R - 1, "R": R, "R+1": R + 1, "3R+5": 3 * R + 5}[Tk]
    case(pq, oracle, 3, 65, 7, T, f"T={T}")


def test_row_tile_is_sized_from_the_lines(pq):
    from polars_quant_amd import api
    tiles = [api.SWEEP_ROW_TILE(L) for L in (1, 18, 78, 79, 256, api.SWEEP_MAX_LINES)]
    assert tiles == sorted(tiles, reverse=True) and tiles[0] > tiles[-1] >= 7
    assert api.SWEEP_ROW_TILE(0) == 0 and api.SWEEP_ROW_TILE(api.SWEEP_MAX_LINES + 1) == 0
    assert api.SWEEP_MAX_LINES >= 256


def test_special_series(pq, oracle):
    """flat, interior / leading NULL, NaN, non-positive and every-third-row-NULL prices; lines with leading NULLs of different lengths
    (MA warm-up) and interior NULLs"""
    from polars_quant_amd import api
    N, T, L, P = 9, 300, 7, 65
    d, price = special_prices(oracle, N, T)
    lines = make_lines(N, T, L)
    for j, l in enumerate(lines):
        l[:, : 3 * j + (j % 2)] = oracle.NULL
        l[j % N, 100 + j: 104 + 2 * j] = oracle.NULL
    tab = make_table(api, P, L)
    # without a benchmark a NaN equity row only turns the variance NaN, which the comparison `vol > 0` maps to a sharpe of 0 ...
    exp = oracle_cells(oracle, price, lines, tab)
    check_cells(run(api, price, lines, tab), exp, "special")
    assert np.isfinite(exp).all() and (exp[:, [2, 3, 4, 7], 4] == 0).all()
    # ... with one the covariance makes alpha and beta NaN: a NULL or NaN price is a NaN row in the oracle's summary and in the kernel's
    bench = d["open"]
    exp = oracle_cells(oracle, price, lines, tab, benchmark=bench)
    got = run(api, price, lines, tab, benchmark=torch.from_numpy(bench).cuda())
    check_cells(got, exp, "special + benchmark")
    nan = np.isnan(exp).any(axis=2)
    assert nan[:, [2, 3, 4, 7]].all() and not nan[:, [0, 1, 5, 6, 8]].any() and (np.isnan(got).any(axis=2) == nan).all()


COSTS = {"poor": dict(initial_capital=5.0), "min-commission": dict(min_commission=500.0),
         "slippage": dict(buy_slippage=0.05, sell_slippage=0.03), "half": dict(position_size=0.5)}


@pytest.mark.parametrize("name", list(COSTS))
def test_costs(pq, oracle, name):
    from polars_quant_amd import api
    N, T, L, P = 3, 158, 7, 65
    price = oracle.gen_ohlcv(SEED, N, T, 0)["close"]
    lines, tab = make_lines(N, T, L), make_table(api, P, L)
    exp = oracle_cells(oracle, price, lines, tab, **COSTS[name])
    got = run(api, price, lines, tab, **COSTS[name])
    check_cells(got, exp, name)
    base = oracle_cells(oracle, price, lines, tab)
    if name == "poor":
        assert (exp[..., 7] == 0).all() and (got[..., 7] == 0).all()      # a buy that cannot afford one share is not a trade
    else:
        assert (bits(exp) != bits(base)).any()                             # the cost changes the result


def test_benchmark(pq, oracle):
    from polars_quant_amd import api
    N, T, L, P = 3, 158, 7, 65
    d = oracle.gen_ohlcv(SEED, N, T, 0)
    price, per = d["close"], d["open"]
    shared = np.ascontiguousarray(per[1])
    lines, tab = make_lines(N, T, L), make_table(api, P, L)
    none = run(api, price, lines, tab)
    assert (none[..., 2:4] == 0).all()
    g_shared = run(api, price, lines, tab, benchmark=torch.from_numpy(shared).cuda())
    g_repl = run(api, price, lines, tab, benchmark=torch.from_numpy(np.tile(shared, (N, 1))).cuda())
    g_per = run(api, price, lines, tab, benchmark=torch.from_numpy(per).cuda())
    assert (bits(g_shared) == bits(g_repl)).all()
    check_cells(g_repl, oracle_cells(oracle, price, lines, tab, benchmark=np.tile(shared, (N, 1))), "shared benchmark")
    check_cells(g_per, oracle_cells(oracle, price, lines, tab, benchmark=per), "per-symbol benchmark")
    assert (g_per[..., 3] != 0).mean() > 0.8 and (bits(g_per[:, 0]) != bits(g_shared[:, 0])).any()
    for k in (1, 5, 6, 7):                                      # the benchmark touches alpha and beta only
        assert (bits(g_per[..., k]) == bits(none[..., k])).all()


def test_position_independence(pq, oracle):
    from polars_quant_amd import api
    N, T, L, P = 3, 158, 7, 130
    d = oracle.gen_ohlcv(SEED, N, T, 0)
    price, bench = d["close"], d["open"]
    lines, tab = make_lines(N, T, L), make_table(api, P, L)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    base = run(api, price, lines, tab, benchmark=dev(bench))
    perm = np.random.default_rng(7).permutation(P)
    assert (bits(run(api, price, lines, tab[perm], benchmark=dev(bench))) == bits(base[perm])).all()
    dup = np.concatenate([tab[:70], tab[3:4], tab[3:4], tab[70:]])
    g = run(api, price, lines, dup, benchmark=dev(bench))
    assert (bits(g[70]) == bits(base[3])).all() and (bits(g[71]) == bits(base[3])).all() and (bits(g[72:]) == bits(base[70:])).all()
    # columns on a row pitch > T whose padding is NaN
    stride = T + 10

    def padded(x):
        buf = torch.full((N, stride), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :T] = dev(x)
        return buf[:, :T]
    got = api.backtest_sweep(padded(price), [padded(l) for l in lines], tab, benchmark=padded(bench)).cpu().numpy()
    assert (bits(got) == bits(base)).all()


def test_against_the_loop_it_replaces(pq, oracle):
    """ParameterSweep.ma against Strategy.ma + api.backtest_vectorized(want_curves=False) per pair: the EXACT columns bit for bit, the
    others at 1e-12 (the four-wave summary of the wave backtest sums in a different fixed order)"""
    from polars_quant_amd import api
    periods = (3, 5, 8, 13, 21, 34)
    close = torch.from_numpy(oracle.gen_ohlcv(SEED, 9, 300, 0)["close"]).cuda()
    df = {"close": close}
    res = pq.ParameterSweep(df).ma(periods, periods)
    assert tuple(res.summary.shape) == (15, 9, 8) and len(res.params["fast"]) == 15
    got = res.summary.cpu().numpy()
    for i, (f, s) in enumerate(zip(res.params["fast"].tolist(), res.params["slow"].tolist())):
        assert f < s
        sig = pq.Strategy().ma(df, fast_period=f, slow_period=s)
        loop = api.backtest_vectorized(close, sig["buy_signal"], sig["sell_signal"], want_curves=False)[3].cpu().numpy()
        for k in EXACT:
            assert (bits(got[i, :, k]) == bits(loop[:, k])).all(), (f, s, k)
        np.testing.assert_allclose(got[i], loop, rtol=1e-12, atol=1e-13)
    assert (got[..., 7] >= 2).mean() >= 0.9
    assert (bits(res.metric("total_trades").cpu().numpy()) == bits(got[..., 7])).all()


def test_rsi_and_macd_sweeps(pq, oracle):
    close_h = oracle.gen_ohlcv(SEED, 9, 300, 0)["close"]
    sw = pq.ParameterSweep({"close": torch.from_numpy(close_h).cuda()})
    res = sw.rsi([14, 7], [20.0, 30.0, 40.0], [60.0, 70.0])
    assert tuple(res.summary.shape) == (12, 9, 8)
    got = res.summary.cpu().numpy()
    for i in range(12):
        (r,) = oracle.call("rsi", close_h, timeperiod=int(res.params["period"][i]))
        sig = oracle.band_signals(r, float(res.params["oversold"][i]), float(res.params["overbought"][i]))
        check_summary(got[i], oracle.backtest(close_h, *sig)[3], f"rsi set {i}")
    res = sw.macd([5, 12], [12, 26], [9])
    assert tuple(res.summary.shape) == (3, 9, 8)
    got = res.summary.cpu().numpy()
    for i in range(3):
        sig = oracle.macd_cross_signals(close_h, *(int(res.params[k][i]) for k in ("fast", "slow", "signal")))
        check_summary(got[i], oracle.backtest(close_h, *sig)[3], f"macd set {i}")


def test_refusals_and_empty_shapes(pq, oracle):
    from polars_quant_amd import api
    N, T, L, P = 3, 60, 7, 65
    price = torch.from_numpy(oracle.gen_ohlcv(SEED, N, T, 0)["close"]).cuda()
    lines = [torch.from_numpy(l).cuda() for l in make_lines(N, T, L)]
    tab = make_table(api, P, L)
    for field, bad in (("a", L), ("a", -1), ("b", L), ("rule", 2)):
        t2 = tab.copy()
        t2[field][40] = bad
        t2["rule"][40] = 0 if field != "rule" else bad
        out = torch.full((N, P, 8), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(pq.PqError):
            api.backtest_sweep(price, lines, t2, out=out)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), "nothing may be launched"
    t2 = tab.copy()
    t2["rule"][:] = 1
    t2["b"][:] = 10 ** 6                                           # a band rule does not look at b
    api.backtest_sweep(price, lines, t2)
    empty = api.backtest_sweep(price, lines, tab[:0])
    assert tuple(empty.shape) == (0, N, 8)
    with pytest.raises(pq.PqError):
        api.backtest_sweep(price.reshape(1, -1), [l.reshape(1, -1) for l in lines], tab, offsets=[0, T, 2 * T, 3 * T])
    with pytest.raises(pq.PqError):
        api.backtest_sweep(price, lines * 80, tab)                 # more lines than fit
    # no rows: zeros (metrics.rs:17-19)
    z = api.backtest_sweep(price[:, :0], [l[:, :0] for l in lines], tab, out=torch.full((N, P, 8), 7.0, dtype=torch.float64, device="cuda"))
    assert tuple(z.shape) == (P, N, 8) and (z == 0).all()


def test_best_ranks_nan_last(pq, oracle):
    from polars_quant_amd.sweep import SweepResult
    s = torch.zeros((4, 3, 8), dtype=torch.float64, device="cuda")
    s[:, :, 4] = torch.tensor([[1.0, float("nan"), float("nan")], [float("nan"), -2.0, float("nan")], [3.0, -1.0, float("nan")],
                               [2.0, float("nan"), float("nan")]], dtype=torch.float64)
    res = SweepResult({"k": np.arange(4)}, s)
    idx, val = res.best()
    assert idx.tolist() == [2, 2, 0] and val[:2].tolist() == [3.0, -1.0] and bool(torch.isnan(val[2]))
    idx, val = res.best(maximize=False)
    assert idx.tolist() == [0, 1, 0] and val[:2].tolist() == [1.0, -2.0] and bool(torch.isnan(val[2]))
    # on a sweep: against a benchmark the symbols with a NULL or NaN price have NaN alphas only
    d, price = special_prices(oracle, 9, 300)
    res = pq.ParameterSweep({"close": torch.from_numpy(price).cuda()}, benchmark=torch.from_numpy(d["open"]).cuda()).run(
        [torch.from_numpy(l).cuda() for l in make_lines(9, 300, 3)], {"rule": [0, 0, 1], "a": [0, 1, 2], "b": [1, 2, 0], "k0": [0, 0, 35.0], "k1": [0, 0, 65.0]})
    idx, val = res.best("alpha")
    m = res.metric("alpha").cpu().numpy()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    dead = np.isnan(m).all(axis=0)
    assert dead.tolist() == [n in (2, 3, 4, 7) for n in range(9)] and (np.isnan(m).any(axis=0) == dead).all()
    assert (idx[dead] == 0).all() and np.isnan(val[dead]).all()
    assert (val[~dead] == m[:, ~dead].max(axis=0)).all() and (m[idx, np.arange(9)][~dead] == val[~dead]).all()
