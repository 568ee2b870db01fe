"""-m gpu: the lane-per-symbol backtest kernels (csrc/ops_backtest.h over csrc/bt_core.h) against the CPU oracle.

Every direct call with len <= 8192 takes the wave-per-symbol form, so these cases force the lane forms with PQ_BT_LANE_FORM and reach
each of them: backtest_body<false,false> (signals as inputs), BtMacdOp (all three curves, tiled) and backtest_body<true,false> (summary
only), LevOp (row pitch a multiple of 8, tiled) and lev_backtest_kernel (any other pitch).  The inputs are the special series of
test_backtest_wave_gpu.py (flat, NULL, NaN and non-positive rows) at lengths that leave a ragged last tile, fit one tile and are one
or two rows.  Curves, trade records and the exact summary columns are compared BIT FOR BIT, the four tolerance columns at 1e-12 / 1e-13.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_backtest_wave_gpu import EXACT, TOL, bits, check_summary, pq, same_bits, special_prices  # noqa: F401  (pq: a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
N = 24
LENS = [1, 2, 65, 777]
LEV_KW = dict(leverage=3.0, interest_rate=0.5, margin_call_threshold=0.6)


@pytest.fixture
def lane_form(pq, monkeypatch):
    from polars_quant_amd import api
    monkeypatch.setenv("PQ_BT_LANE_FORM", "1")
    api.backtest_wave_stats(reset=True)
    yield
    assert api.backtest_wave_stats()[0] == 0, "the wave form must not have run"


@functools.lru_cache(maxsize=None)
def inputs(oracle, T):
    """prices, benchmark and the signals of each density: made once per length, shared by the cases, never written to"""
    d, price = special_prices(oracle, N, T)
    rng = np.random.default_rng(T)
    sig = {dens: ((rng.random(price.shape) < dens).astype(np.uint8), (rng.random(price.shape) < dens).astype(np.uint8)) for dens in (0.05, 0.3, 1.0)}
    for a in (price, d["open"], *(s for p in sig.values() for s in p)):
        a.setflags(write=False)
    return price, d["open"], sig


@functools.lru_cache(maxsize=None)
def lev_expected(oracle, T, with_bench, max_trades):
    price, bench, sig = inputs(oracle, T)
    return oracle.backtest_leveraged(price, *sig[0.3], benchmark=bench[0].copy() if with_bench else None, max_trades=max_trades, **LEV_KW)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("T", LENS)
@pytest.mark.parametrize("dens", [0.05, 1.0])
def test_vectorized_lane_form(pq, oracle, lane_form, T, dens):
    from polars_quant_amd import api
    price, bench, sig = inputs(oracle, T)
    buy, sell = sig[dens]
    cases = [(dict(), bench), (dict(), None), (dict(buy_slippage=0.01, sell_slippage=0.02, position_size=0.5, min_commission=1.0), bench)]
    if dens == 1.0:
        cases.append((dict(initial_capital=30.0), bench))  # a pool that cannot afford a share: buy signals that are no events
    for kw, bm in cases:
        epos, ecash, eeq, es = oracle.backtest(price, buy, sell, benchmark=bm, **kw)
        for curves in (True, False):
            pos, cash, eq, s = api.backtest_vectorized(dev(price), dev(buy), dev(sell), benchmark=None if bm is None else dev(bm),
                                                       want_curves=curves, **kw)
            tag = (T, dens, tuple(kw), bm is not None, curves)
            if curves:
                for nm, g, e in (("position", pos, epos), ("cash", cash, ecash), ("equity", eq, eeq)):
                    ok = same_bits(g.cpu().numpy(), e)
                    assert ok.all(), (tag, nm, np.argwhere(~ok)[:4].tolist())
            else:
                assert pos is None and cash is None and eq is None
            check_summary(s.cpu().numpy(), es, tag)
        if "initial_capital" in kw:
            assert (es[:, 7] == 0).any(), "some pool must be unable to afford a share"


@pytest.mark.parametrize("T", LENS)
def test_macd_cross_lane_forms(pq, oracle, lane_form, T):
    from polars_quant_amd import api
    price, _, _ = inputs(oracle, T)
    ebuy, esell = oracle.macd_cross_signals(price)
    for kw in (dict(), dict(initial_capital=30.0), dict(buy_slippage=0.01, sell_slippage=0.02, position_size=0.5, min_commission=1.0)):
        epos, ecash, eeq, es = oracle.backtest(price, ebuy, esell, **kw)
        pos, cash, eq, s = api.backtest_macd_cross(dev(price), **kw)                          # BtMacdOp
        for nm, g, e in (("position", pos, epos), ("cash", cash, ecash), ("equity", eq, eeq)):
            ok = same_bits(g.cpu().numpy(), e)
            assert ok.all(), (T, kw, nm, np.argwhere(~ok)[:4].tolist())
        check_summary(s.cpu().numpy(), es, (T, tuple(kw), "tiled"))
        _, _, _, s2 = api.backtest_macd_cross(dev(price), want_curves=False, **kw)            # backtest_body<true, false>
        check_summary(s2.cpu().numpy(), es, (T, tuple(kw), "summary only"))
        assert same_bits(s2.cpu().numpy(), s.cpu().numpy()).all(), (T, kw)


def leveraged_pitched(price, buy, sell, bench, pitch, max_trades, **kw):
    """pq_backtest_leveraged on columns of row pitch `pitch` >= T (api.backtest_leveraged packs its inputs: its pitch is T itself)"""
    from polars_quant_amd._lib import Batch, LevParams, check, lib
    from polars_quant_amd.api import ctx
    from polars_quant_amd._spec import LEV_DEFAULTS, TRADE_FIELDS
    n, T = price.shape

    def pitched(a, dtype):
        t = torch.zeros((n, pitch), dtype=dtype, device="cuda")
        t[:, :T] = dev(a)
        return t
    p, bu, se = pitched(price, torch.float64), pitched(buy, torch.uint8), pitched(sell, torch.uint8)
    cash, sv, tv = (torch.zeros((n, pitch), dtype=torch.float64, device="cuda") for _ in range(3))
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    tr = {k: torch.zeros((n, max_trades), dtype=torch.int32 if k in ("entry_day", "exit_day", "reason") else torch.float64, device="cuda")
          for k in TRADE_FIELDS}
    summ = torch.empty((n, 8), dtype=torch.float64, device="cuda")
    bm = None if bench is None else dev(bench)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    prm = LevParams(**{**LEV_DEFAULTS, **kw})
    check(lib().pq_backtest_leveraged(ctx(0), C.byref(Batch(n, T, pitch)), vp(p), vp(bu), vp(se), vp(bm), C.byref(prm), vp(cash), vp(sv), vp(tv),
                                      max_trades, vp(cnt), *[vp(tr[k]) for k in ("entry_day", "exit_day", "entry_price", "exit_price", "quantity",
                                                                                "pnl", "pnl_pct", "reason")], vp(summ)))
    return dict(cash=cash[:, :T], stock_value=sv[:, :T], total_value=tv[:, :T], trade_count=cnt, trades=tr, summary=summ)


@pytest.mark.parametrize("T", LENS)
@pytest.mark.parametrize("form", ["tiled", "odd-pitch"])
def test_leveraged_lane_forms(pq, oracle, lane_form, T, form):
    """tiled: pitch a multiple of 8 -> LevOp; odd-pitch: the packed columns of api.backtest_leveraged, pitch T (1, 2, 65, 777: none a
    multiple of 8) -> lev_backtest_kernel"""
    from polars_quant_amd import api
    price, bench, sig = inputs(oracle, T)
    buy, sell = sig[0.3]
    for with_bench in (True, False):
        bm = bench[0].copy() if with_bench else None
        for max_trades in (64, 3, 0):   # room for 64 records, fewer records than trades, no record arrays
            e = lev_expected(oracle, T, with_bench, max_trades or 64)
            if form == "tiled":
                g = leveraged_pitched(price, buy, sell, bm, (T + 7) // 8 * 8, max_trades, **LEV_KW)
            else:
                g = api.backtest_leveraged(dev(price), dev(buy), dev(sell), benchmark=None if bm is None else dev(bm), max_trades=max_trades,
                                           **LEV_KW)
            tag = (T, form, with_bench, max_trades)
            for k in ("cash", "stock_value", "total_value"):
                ok = same_bits(g[k].cpu().numpy(), e[k])
                assert ok.all(), (tag, k, np.argwhere(~ok)[:4].tolist())
            assert (g["trade_count"].cpu().numpy() == e["trade_count"]).all(), tag
            if max_trades:
                for k, v in e["trades"].items():
                    gv = g["trades"][k].cpu().numpy()
                    assert (gv == v).all() if v.dtype == np.int32 else same_bits(gv, v).all(), (tag, k)
            check_summary(g["summary"].cpu().numpy(), e["summary"], tag)
    if T == 777:
        e = lev_expected(oracle, T, True, 64)
        assert (e["trades"]["reason"] == 2).any(), "the margin-call path must be exercised"
        assert e["trade_count"].max() > 3, "max_trades = 3 must be fewer records than trades"
