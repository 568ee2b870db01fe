"""-m gpu: the statistics report of `Backtest` (D-22, csrc/report/report.hip) against the numpy restatement in tests/backtest_report_ref.py.

Every column is compared bitwise on the uint64 view, with D-22's one exception: annualized_return goes through the device's pow and is
held to |g - e| <= 1e-12 max(|e|, 1); sharpe, sortino and calmar, which only subtract and divide after it, are compared bitwise against
the restatement evaluated from the GPU's own column 3.  Before a comparison, the restatement's output is checked for non-NULL values
in every column group the case is there to exercise.

Every comparison prints the largest scaled error of the tolerance-held column before it asserts (pytest -s shows the lines); the bound
is the one of tests/tolerance.py."""
import ctypes as C

import numpy as np
import pytest

import backtest_report_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C0 = 100000.0
KW = dict(leverage=2.0, slippage=0.001, interest_rate=0.06, commission_rate=0.0003, min_commission=5.0)
FEE = dict(commission_rate=KW["commission_rate"], min_commission=KW["min_commission"])


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(name, got, exp):
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def same_rows(name, got, make_exp):
    """got [N, 48] from the GPU; make_exp(ann) -> the restatement with column 3 of the GPU in the ratios after it"""
    got = np.asarray(got)
    exp = make_exp(got[:, 3])
    g3, e3 = got[:, 3], exp[:, 3]
    same(name + " (NULLs of annualized_return)", R.isnull(g3).astype(np.float64), R.isnull(e3).astype(np.float64))
    live = ~R.isnull(e3)
    err = np.abs(g3[live] - e3[live]) / np.maximum(np.abs(e3[live]), 1.0)
    print(f"{name}: annualized_return max scaled error {err.max() if err.size else 0.0:.3e} over {err.size} rows")
    assert (err <= 1e-12).all(), (name, err.max())
    keep = [c for c in range(got.shape[1]) if c != 3]
    same(name, got[:, keep], exp[:, keep])
    return exp


def engine(pq, n, T, seed, max_trades=64, p=0.08, bench=True):
    """the engine's own curves and records on a random walk with random signals"""
    from polars_quant_amd import api
    rng = np.random.default_rng(seed)
    price = 20.0 * np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))
    buy, sell = (rng.random((n, T)) < p).astype(np.uint8), (rng.random((n, T)) < p).astype(np.uint8)
    bm = 3000.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T))) if bench else None
    r = api.backtest_leveraged(dev(price), dev(buy), dev(sell), None if bm is None else dev(bm), max_trades, initial_capital=C0, **KW)
    host = dict(total_value=r["total_value"].cpu().numpy(), trade_count=r["trade_count"].cpu().numpy(),
                trades={k: v.cpu().numpy() for k, v in r["trades"].items()}, summary=r["summary"].cpu().numpy(), bench=bm)
    return r, host


def engine_report(pq, r, h, max_trades=64):
    from polars_quant_amd import api
    got = api.backtest_report(r["total_value"], C0, None if h["bench"] is None else dev(h["bench"]), r["trades"], r["trade_count"],
                              max_trades, **KW)
    return got, lambda ann: R.report(h["total_value"], C0, h["bench"], h["trades"], h["trade_count"], max_trades, ann=ann, **FEE)


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 8193])
def test_engine_rows_every_length(pq, T):
    """N = 3: one tile, the tile edge, two tiles and their edge, several unrolled steps, and a row longer than the engine's wave form"""
    width = 512 if T > 1000 else 64                                      # wide enough for every record of the long rows
    r, h = engine(pq, 3, T, 100 + T, max_trades=width, p=0.3 if T < 200 else 0.08)   # frequent signals: a short row still has winners and losers
    got, make = engine_report(pq, r, h, width)
    exp = make(None)
    assert not R.isnull(exp[:, R.CURVE]).any() and not R.isnull(exp[:, 38:42]).any() and not R.isnull(exp[:, 43:45]).any()
    assert R.isnull(exp[:, 42]).all() == (T == 1)                        # information_ratio needs two days
    if T >= 63:
        assert (h["trade_count"] <= width).all() and not R.isnull(exp[:, 16]).any() and (exp[:, 16] > 0).any() and (exp[:, 17] > 0).any()
        assert (~R.isnull(exp[:, [18, 21, 22, 23, 34, 36]])).all(axis=1).any()
    if T >= 127:
        assert (exp[:, 6] > 0).all() and (exp[:, 5] > 0).all()
    exp = same_rows(f"T = {T}", got.cpu().numpy(), make)
    if T >= 2:                                                           # the sanity link to the engine's own summary (another order)
        for col, k in ((3, 0), (5, 1), (41, 3)):
            e = h["summary"][:, k]
            assert (np.abs(exp[:, col] - e) <= 1e-12 * np.maximum(np.abs(e), 1.0)).all(), (col, exp[:, col], e)


def records(n, width, counts, seed, all_margin=False):
    """hand-built records: pnl with zeros and both signs, amounts on both sides of the minimum commission (q p 0.0003 against 5.0)"""
    rng = np.random.default_rng(seed)
    t = dict(entry_day=np.zeros((n, width), np.int32), exit_day=np.zeros((n, width), np.int32), reason=np.zeros((n, width), np.int32),
             entry_price=np.zeros((n, width)), exit_price=np.zeros((n, width)), quantity=np.zeros((n, width)), pnl=np.zeros((n, width)))
    for s, c in enumerate(counts):
        m = min(c, width)
        days = np.sort(rng.choice(5000, size=2 * m, replace=False)).astype(np.int32)
        t["entry_day"][s, :m], t["exit_day"][s, :m] = days[0::2], days[1::2]
        t["quantity"][s, :m] = 100.0 * rng.integers(1, 40, m)
        t["entry_price"][s, :m] = rng.uniform(3.0, 30.0, m)
        t["exit_price"][s, :m] = t["entry_price"][s, :m] * rng.uniform(0.8, 1.25, m)
        pnl = t["quantity"][s, :m] * (t["exit_price"][s, :m] - t["entry_price"][s, :m]) - 11.0
        pnl[rng.random(m) < 0.1] = 0.0
        t["pnl"][s, :m] = pnl
        t["reason"][s, :m] = 2 if all_margin else rng.integers(1, 3, m)
    return t


def curves(n, T, seed):
    rng = np.random.default_rng(seed)
    return 1000.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((n, T)), axis=1))


def direct(pq, v, c0, bench=None, trades=None, counts=None, **fee):
    from polars_quant_amd import api
    got = api.backtest_report(dev(v), c0, None if bench is None else dev(bench), None if trades is None else {k: dev(a) for k, a in trades.items()},
                              None if counts is None else dev(np.asarray(counts, np.int32)), **fee)
    width = 0 if trades is None else trades["pnl"].shape[1]
    f = {**FEE, **fee}
    return got.cpu().numpy(), lambda ann: R.report(v, c0, bench, trades, counts, width, ann=ann, **f)


def test_record_counts_and_truncation(pq):
    """0, 1, 63, 64, 65 and max_trades records, and trade_count = max_trades + 1: the tile edge of the trade loop and the NULL rules"""
    width, counts = 80, [0, 1, 63, 64, 65, 80, 81]
    t = records(len(counts), width, counts, 5)
    got, make = direct(pq, curves(len(counts), 70, 6), 1000.0, None, t, counts)
    exp = make(None)
    assert R.isnull(exp[0, [18, 21, 22, 23, 24, 25, 26, 27, 28, 34, 35, 36]]).all() and (exp[0, [15, 16, 17, 19, 20, 29, 32, 33, 37]] == 0).all()
    assert not R.isnull(exp[2:6, R.TRADES]).any() and R.isnull(exp[6, R.TRADES]).all() and exp[6, 15] == 81
    assert R.isnull(exp[:, R.BENCH]).all()
    cost = t["quantity"] * t["entry_price"] * 0.0003
    assert (cost[2, :63] > 5.0).any() and (cost[2, :63] < 5.0).any()      # the minimum commission binds on some trades only
    same_rows("record counts", got, make)


def test_streaks_zero_pnl_and_margin_calls(pq):
    n, width = 5, 130
    t = records(n, width, [130, 130, 130, 3, 0], 8)
    t["pnl"][0, 50:80] = 7.5                                             # a win streak across the 64-trade tile edge
    t["pnl"][0, 49] = t["pnl"][0, 80] = -1.0
    t["pnl"][1, :] = np.abs(t["pnl"][1, :]) + 1.0
    t["pnl"][1, 60:70] = -3.0                                            # a loss streak across it, with a pnl == 0 trade inside
    t["pnl"][1, 64] = 0.0
    t["pnl"][2, :] = np.abs(t["pnl"][2, :]) + 1.0                        # winners only
    t["reason"][3, :3] = 2                                               # all trades margin calls
    counts = [130, 130, 130, 3, 0]
    got, make = direct(pq, curves(n, 40, 9), 1000.0, None, t, counts, commission_rate=0.001, min_commission=2.0)
    exp = make(None)
    assert exp[0, 30] >= 30 and exp[1, 31] == 5 and exp[1, 30] == 60 and exp[2, 30] == 130 and exp[2, 17] == 0
    assert R.isnull(exp[2, [21, 23, 25, 27]]).all() and not R.isnull(exp[2, [18, 22, 24, 26, 28]]).any()
    assert exp[3, 37] == 3 and exp[3, 15] == 3
    same_rows("streaks", got, make)


def edge_curves(T=200, c0=1000.0):
    rng = np.random.default_rng(12)
    wob = lambda: 0.5 * rng.random(T)
    v = np.empty((9, T))
    v[0] = 990.0 - wob(); v[0, 63], v[0, 64] = 1100.0, 1200.0            # peaks on the last row of a tile and the first of the next
    v[1] = 990.0 - wob(); v[1, 60] = 1500.0; v[1, 196:] = 1600.0 + np.arange(4)   # under water over days 61 .. 195: three tiles
    v[2] = 1010.0 + np.arange(T); v[2, 11:] = 1015.0 - wob()[11:]        # a run that ends on the last day
    v[3] = 999.0 - wob()                                                 # never above c0: every day under water
    v[4] = 1000.0 + np.cumsum(rng.random(T))                             # never falls
    v[5] = 1000.0 + np.cumsum(rng.standard_normal(T)); v[5, 77] = np.nan
    v[6] = 1000.0 + np.cumsum(rng.standard_normal(T)); v[6, 128] = R.NULL
    v[7] = c0                                                            # flat: no return at all
    v[8] = 1000.0 + np.cumsum(rng.standard_normal(T)); v[8, 5] = np.inf
    return v


def test_curve_edges(pq):
    v = edge_curves()
    T = v.shape[1]
    rng = np.random.default_rng(13)
    walk = 50.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T)))
    zero = walk.copy(); zero[100] = 0.0
    for name, bench in (("no benchmark", None), ("a walk", walk), ("a zero in the benchmark", zero), ("a constant benchmark", np.full(T, 42.0))):
        got, make = direct(pq, v, 1000.0, bench)
        exp = make(None)
        assert exp[0, 6] > 64 and exp[1, 6] == 135 and exp[2, 6] == T - 11 and exp[3, 6] == T and exp[4, 6] == 0 and exp[4, 5] == 0 and exp[4, 11] == 0
        assert R.isnull(exp[[5, 6, 8]][:, R.CURVE]).all() and R.isnull(exp[[5, 6, 8]][:, R.BENCH]).all() and not R.isnull(exp[:5, R.CURVE]).any()
        assert R.isnull(exp[:, 15:38]).all()                             # no trade_count: 15 is NULL too
        if bench is None:
            assert R.isnull(exp[:, R.BENCH]).all()
        else:
            assert not R.isnull(exp[:5, 38:42]).any()
        if name == "a constant benchmark":
            assert (exp[:5, 41] == 0).all() and not R.isnull(exp[:5, 42]).any() and R.isnull(exp[7, 42])    # flat against constant: no deviation
        if name == "a walk":
            assert (exp[:5, 41] != 0).all()
        same_rows(f"curve edges, {name}", got, make)
    bad = walk.copy(); bad[3] = np.nan
    got, make = direct(pq, v[:5], 1000.0, bad)
    assert R.isnull(make(None)[:, R.BENCH]).all()
    same_rows("a NaN in the benchmark", got, make)


def test_row_pitch_through_the_abi(pq):
    """stride = len + 3: rows read at the batch's pitch, the report written dense, the padding of the input untouched"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, LevParams, check as ok, lib
    from polars_quant_amd._spec import LEV_DEFAULTS
    n, T = 5, 131
    v = curves(n, T, 21)
    buf = torch.full((n, T + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = dev(v)
    out = torch.full((n + 1, R.COLS), -77.0, dtype=torch.float64, device="cuda")
    prm = LevParams(**LEV_DEFAULTS)
    vp = C.c_void_p
    ok(lib().pq_backtest_report(api.ctx(), C.byref(Batch(n, T, T + 3)), vp(buf.data_ptr()), C.c_double(1000.0), None, C.byref(prm), 0,
                                *[None] * 8, vp(out.data_ptr())))
    got = out.cpu().numpy()
    assert (got[n] == -77.0).all(), "wrote past the last row"
    exp = same_rows("pitch", got[:n], lambda ann: R.report(v, 1000.0, ann=ann))
    assert not R.isnull(exp[:, R.CURVE]).any()


def test_refusals(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, LevParams, check as ok, lib
    from polars_quant_amd._spec import LEV_DEFAULTS
    n, T = 4, 30
    v = curves(n, T, 22)
    t = records(n, 8, [3, 3, 3, 3], 23)
    with pytest.raises(ValueError, match="benchmark"):
        api.backtest_report(v, 1000.0, np.ones(T + 1))
    with pytest.raises(ValueError, match="one shape"):
        api.backtest_report(v, 1000.0, None, {**t, "pnl": t["pnl"][:, :7]}, np.full(n, 3))
    with pytest.raises(ValueError, match="trade_count"):
        api.backtest_report(v, 1000.0, None, t)
    with pytest.raises(ValueError, match="initial_capital"):
        api.backtest_report(v, 0.0)
    with pytest.raises(ValueError, match="report"):
        api.report_portfolio(np.zeros((3, 47)), np.zeros(48), 1000.0)
    vd = dev(v)
    out = torch.full((n, R.COLS), 7.0, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    prm, vp = LevParams(**LEV_DEFAULTS), C.c_void_p
    with pytest.raises(pq.PqError, match="ragged") as e:
        ok(lib().pq_backtest_report(api.ctx(), C.byref(Batch(3, n * T - 25, n * T, vp(off.data_ptr()))), vp(vd.data_ptr()), C.c_double(1000.0),
                                    None, C.byref(prm), 0, *[None] * 8, vp(out.data_ptr())))
    assert "pq status 5:" in str(e.value)                                 # PQ_ERR_UNSUPPORTED
    cnt = dev(np.full(n, 3, np.int32))
    with pytest.raises(pq.PqError, match="all seven") as e:
        ok(lib().pq_backtest_report(api.ctx(), C.byref(Batch(n, T, T)), vp(vd.data_ptr()), C.c_double(1000.0), None, C.byref(prm), 8,
                                    vp(cnt.data_ptr()), vp(cnt.data_ptr()), *[None] * 6, vp(out.data_ptr())))
    assert "pq status 1:" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote"


@pytest.mark.parametrize("n", [1, 2, 256, 257, 513])
def test_portfolio_row(pq, n):
    """one block, the block edge, two blocks and a tail; at 257 the records are cut short (max_trades = 2) and 16-37 are NULL"""
    from polars_quant_amd import api
    T, width = 130, 2 if n == 257 else 64
    r, h = engine(pq, n, T, 300 + n, max_trades=width)
    got, make = engine_report(pq, r, h, width)
    rows = same_rows(f"rows, N = {n}", got.cpu().numpy(), make)
    pv = api.portfolio_metrics(r["total_value"], C0 * n, dev(h["bench"]))[:, 0].contiguous()
    curve = api.backtest_report(pv.reshape(1, -1), C0 * n, dev(h["bench"]))
    crow = same_rows(f"curve row, N = {n}", curve.cpu().numpy(), lambda ann: R.report(pv.cpu().numpy()[None], C0 * n, h["bench"], ann=ann))[0]
    exp = R.portfolio_row(rows, crow, C0)
    assert not R.isnull(exp[R.CURVE]).any() and not R.isnull(exp[R.BENCH]).any() and not R.isnull(exp[45:]).any() and exp[47] >= 1
    if n == 257:
        assert (h["trade_count"] > width).any() and R.isnull(exp[R.TRADES]).all() and exp[15] == h["trade_count"].sum()
    else:
        assert not R.isnull(exp[R.TRADES]).any() and exp[16] > 0 and exp[17] > 0
    port = api.report_portfolio(got, curve[0], C0).cpu().numpy()
    same(f"portfolio row, N = {n}", port, R.portfolio_row(got.cpu().numpy(), curve[0].cpu().numpy(), C0))


def test_portfolio_ties_and_null_returns(pq):
    """best / worst: the lowest index among equal returns, across waves and blocks; a symbol with a NULL return is skipped"""
    from polars_quant_amd import api
    n = 600
    rep = np.zeros((n, R.COLS))
    rep[:, 2] = 0.01
    rep[[70, 300, 599], 2] = 0.5
    rep[[130, 257], 2] = -0.5
    rep[[0, 69], 2] = R.NULL
    rep[0, 0:15] = R.NULL
    rep[:, 15:38] = R.NULL
    exp = R.portfolio_row(rep, np.arange(48.0), 1000.0)
    assert exp[45] == 70 and exp[46] == 130 and R.isnull(exp[15:38]).all() and exp[47] == 0
    same("ties", api.report_portfolio(rep, np.arange(48.0), 1000.0).cpu().numpy(), exp)
    rep[:, 2] = R.NULL
    exp = R.portfolio_row(rep, np.arange(48.0), 1000.0)
    assert R.isnull(exp[45:47]).all()
    same("no ranked symbol", api.report_portfolio(rep, np.arange(48.0), 1000.0).cpu().numpy(), exp)


def frames(n, T, seed):
    rng = np.random.default_rng(seed)
    syms = [f"S{k}" for k in range(n)]
    dates = [f"d{t:04d}" for t in range(T)]
    price = 20.0 * np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))
    mk = lambda a: {"date": dates, **{s: a[k] for k, s in enumerate(syms)}}
    buy, sell = (rng.random((n, T)) < 0.1).astype(np.uint8), (rng.random((n, T)) < 0.1).astype(np.uint8)
    bench = {"date": dates, "IDX": 3000.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T)))}
    return syms, mk(price), mk(buy), mk(sell), bench


@pytest.mark.parametrize("with_bench", [False, True])
def test_backtest_statistics_and_summaries(pq, with_bench, capsys):
    from polars_quant_amd._spec import REPORT_SECTIONS
    syms, price, buy, sell, bench = frames(4, 200, 31)
    bt = pq.Backtest(price, buy, sell, initial_capital=C0, benchmark=bench if with_bench else None, max_trades=16, **KW)
    with pytest.raises(RuntimeError):
        bt.statistics()
    bt.run()
    st = bt.statistics()
    assert bt.statistics() is not st and bt._report()[0] is bt._report()[0]          # computed once, handed out as fresh dicts
    bm = bench["IDX"] if with_bench else None
    tv, tr, cnt = bt._r["total_value"], bt._r["trades"], bt._r["trade_count"]
    got = np.stack([st["symbols"][k] for k in R.NAMES[:45]], axis=1)
    assert not np.isnan(got[:, :15]).any() and (cnt > 0).all() and np.isnan(got[:, 38:45]).all() != with_bench
    unnull = lambda a: np.where(R.isnull(a), np.nan, a)
    renull = lambda a: np.where(np.isnan(a), R.NULL, a)
    exp = same_rows("statistics, symbols", renull(got), lambda ann: R.report(tv, C0, bm, tr, cnt, 16, ann=ann, **FEE)[:, :45])
    for k, s in enumerate(syms):
        one = bt.get_stock_statistics(s)
        assert list(one) == list(R.NAMES[:45])
        np.testing.assert_array_equal(np.array(list(one.values())), got[k])
    pv = bt._metrics[:, 0]
    full = R.report(tv, C0, bm, tr, cnt, 16, ann=got[:, 3], **FEE)
    full[:, 3] = got[:, 3]
    port = np.array([st["portfolio"][k] for k in R.NAMES])
    crow = R.report(pv[None], C0 * 4, bm, ann=port[3:4])[0]
    assert abs(port[3] - crow[3]) <= 1e-12 * max(abs(crow[3]), 1.0)
    crow[3] = port[3]
    same("statistics, portfolio", renull(port), R.portfolio_row(full, crow, C0))
    assert st["best_symbol"] == syms[int(port[45])] and st["worst_symbol"] == syms[int(port[46])]
    assert st["best_symbol"] == syms[int(np.argmax(exp[:, 2]))] and st["worst_symbol"] == syms[int(np.argmin(exp[:, 2]))]
    capsys.readouterr()
    bt.summary()
    lines = capsys.readouterr().out.splitlines()
    m = bt._metrics
    assert lines[0] == f"symbols: 4  days: 200  trades: {int(cnt.sum())}"
    assert lines[1] == f"final portfolio value: {m[-1, 0]:.2f}  cumulative return: {m[-1, 4]:.4f} %"
    text = "\n".join(lines[2:])
    for k, (title, _) in enumerate(REPORT_SECTIONS, 1):
        assert (f"[{k}] {title}" in text) == (with_bench or title != "benchmark comparison"), title
    assert len(REPORT_SECTIONS) == 13 and f"best_symbol: {st['best_symbol']}" in text and "sortino:" in text
    one = bt.get_stock_summary(syms[1])
    assert one.startswith("annualized_return: ") and "sharpe_ratio: " in one and "[5] trade statistics" in one and "max_consecutive_wins:" in one
    assert one.splitlines()[:8] == [f"{k}: {v:.6g}" for k, v in zip(pq.api.SUMMARY_KEYS, bt._r["summary"][1])]
