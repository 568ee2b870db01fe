"""BASELINE config 5 (5000 symbols x 2520 days, MACD-cross signals, leverage 2): the statistics report of `Backtest` (D-22) next to the
engine it reports on, in the same run and with the same event timing -- pq_backtest_leveraged alone (preallocated outputs),
pq_backtest_report on the engine's curves and records, pq_report_portfolio, and Backtest.statistics() end to end from the tensors
run() kept.  Prints the report's rate over the bytes it has to read once (the total_value column and the seven record arrays)."""
import sys; sys.path.insert(0, ".")
import ctypes as C
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import api
from polars_quant_amd._lib import Batch, LevParams, check, lib
from polars_quant_amd._spec import LEV_DEFAULTS
from oracle import pq_oracle as oracle

N, T, MT, C0 = 5000, 2520, 64, 1e5
d = oracle.gen_ohlcv(0x5EED0002, N, T, 0)
close = torch.from_numpy(d["close"]).cuda()
buy, sell = api.macd_cross_signals(close)
bench = close[0].clone()
kw = dict(leverage=2.0, slippage=0.001)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


r = api.backtest_leveraged(close, buy, sell, bench, MT, **kw)
outs = [torch.empty((N, T), dtype=torch.float64, device="cuda") for _ in range(3)]
cnt, sm = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.empty((N, 8), dtype=torch.float64, device="cuda")
prm, b, h = LevParams(**{**LEV_DEFAULTS, **kw}), Batch(N, T, T), api.ctx(0)
vp = lambda t: C.c_void_p(t.data_ptr())
rec = [r["trades"][k] for k in ("entry_day", "exit_day", "entry_price", "exit_price", "quantity", "pnl", "pnl_pct", "reason")]
ms_engine = timed(lambda: check(lib().pq_backtest_leveraged(h, C.byref(b), vp(close), vp(buy), vp(sell), vp(bench), C.byref(prm), *[vp(t) for t in outs],
                                                            MT, vp(cnt), *[vp(t) for t in rec], vp(sm))))
rep = torch.empty((N, 48), dtype=torch.float64, device="cuda")
rec7 = [r["trades"][k] for k in ("entry_day", "exit_day", "entry_price", "exit_price", "quantity", "pnl", "reason")]
ms_report = timed(lambda: check(lib().pq_backtest_report(h, C.byref(b), vp(r["total_value"]), C0, vp(bench), C.byref(prm), MT, vp(r["trade_count"]),
                                                         *[vp(t) for t in rec7], vp(rep))))
pv = api.portfolio_metrics(r["total_value"], C0 * N, bench)[:, 0].contiguous()
curve = api.backtest_report(pv.reshape(1, -1), C0 * N, bench)
port = torch.empty(48, dtype=torch.float64, device="cuda")
ms_port = timed(lambda: check(lib().pq_report_portfolio(h, N, vp(rep), vp(curve), C0, vp(port))))
ms_api = timed(lambda: api.backtest_report(r["total_value"], C0, bench, r["trades"], r["trade_count"], **kw))

syms = [f"S{k}" for k in range(N)]
frame = lambda a: {"date": list(range(T)), **{s: a[k] for k, s in enumerate(syms)}}
bt = pq.Backtest(frame(d["close"]), frame(buy.cpu().numpy()), frame(sell.cpu().numpy()), benchmark={"date": list(range(T)), "B": d["close"][0]},
                 max_trades=MT, **kw)
bt.run()


def stats():
    bt._stats = None
    return bt.statistics()


ms_stats = timed(stats, warm=2, reps=5)
st = stats()
byt = 8 * N * T + (3 * 4 + 4 * 8) * int(torch.clamp(r["trade_count"], max=MT).sum())
print(f"pq_backtest_leveraged alone {ms_engine:.3f} ms | pq_backtest_report {ms_report:.3f} ms ({byt / ms_report / 1e6:.0f} GB/s over {byt / 1e6:.0f} MB read once; "
      f"{ms_report / ms_engine:.2f} x the engine) | through api.backtest_report {ms_api:.3f} ms | pq_report_portfolio {ms_port:.3f} ms | "
      f"Backtest.statistics() end to end {ms_stats:.3f} ms")
print(f"trades={int(r['trade_count'].sum())}  portfolio sharpe={st['portfolio']['sharpe']:.4f}  best={st['best_symbol']}  worst={st['worst_symbol']}")
