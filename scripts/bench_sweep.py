"""ParameterSweep (D-25, pq_backtest_sweep) on BASELINE config 3: 5 000 symbols x 2 520 days of synthetic.py data, the SMA grid fasts
5..50 step 5 x slows 20..200 step 20 with fast < slow (90 pairs over 18 distinct periods), device-resident close.  Device-event times
after a warm-up (the Python call included) over a window of at least half a second: the sweep launch on ready lines, the computation of
the 18 lines, and -- in the same run -- the loop the sweep replaces, `Strategy.ma` + `api.backtest_vectorized(want_curves=False)` per
pair, as it stands; then max_drawdown / max_profit / win_rate / total_trades of the two compared bit for bit on all 450 000 cells and the
largest relative difference of the other four columns."""
import sys; sys.path.insert(0, ".")
import json, math
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import api, sweep
from polars_quant_amd.synthetic import gen_ohlcv
N, T = 5000, 2520
close = torch.from_numpy(gen_ohlcv(0x5EED0002, N, T, 0)["close"]).cuda()
df = {"close": close}
fasts, slows = list(range(5, 55, 5)), list(range(20, 220, 20))
periods, rules, params = sweep.ma_grid(fasts, slows)
P = len(rules)
def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    reps = max(3, min(400, math.ceil(500.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, reps
make_lines = lambda: [api.call("sma", close, timeperiod=p)[0] for p in periods]
lines = make_lines()
lines_ms, lines_reps = timed(make_lines)
sweep_ms, sweep_reps = timed(lambda: api.backtest_sweep(close, lines, rules))
both_ms, both_reps = timed(lambda: pq.ParameterSweep(df).ma(fasts, slows))
strat = pq.Strategy()
def loop(keep=None):
    for i, (f, s) in enumerate(zip(params["fast"].tolist(), params["slow"].tolist())):
        sig = strat.ma(df, fast_period=f, slow_period=s)
        summ = api.backtest_vectorized(close, sig["buy_signal"], sig["sell_signal"], want_curves=False)[3]
        if keep is not None: keep[i] = summ
loop_ms, loop_reps = timed(loop)
print(f"{N} x {T}, {P} SMA pairs over {len(periods)} lines (row tile {api.SWEEP_ROW_TILE(len(periods))})")
print(f"sweep launch on ready lines   {sweep_ms:9.3f} ms ({sweep_reps} reps)  {N * P * T / sweep_ms / 1e6:8.2f} G cell-rows/s")
print(f"the {len(periods)} SMA lines              {lines_ms:9.3f} ms ({lines_reps} reps)")
print(f"ParameterSweep.ma (both)      {both_ms:9.3f} ms ({both_reps} reps)")
print(f"loop of Strategy.ma + backtest_vectorized(want_curves=False), {P} pairs {loop_ms:9.3f} ms ({loop_reps} reps) = "
      f"{loop_ms / both_ms:.1f} x ParameterSweep.ma, {loop_ms / sweep_ms:.1f} x the sweep launch")
got = pq.ParameterSweep(df).ma(fasts, slows).summary
ref = torch.empty((P, N, 8), dtype=torch.float64, device="cuda")
loop(ref)
g, r = got.cpu().numpy(), ref.cpu().numpy()
exact = {k: bool((g[..., j].view(np.uint64) == r[..., j].view(np.uint64)).all()) for j, k in enumerate(pq.SUMMARY_KEYS) if j in (1, 5, 6, 7)}
with np.errstate(invalid="ignore", divide="ignore"):
    rel = {k: float(np.nanmax(np.abs(g[..., j] - r[..., j]) / np.maximum(np.abs(r[..., j]), 1e-300))) for j, k in enumerate(pq.SUMMARY_KEYS) if j in (0, 2, 3, 4)}
print(f"bitwise equal to the loop on {P * N} cells: {exact}; largest relative difference of the others: {rel}; "
      f"mean trades per cell {g[..., 7].mean():.1f}")
print(json.dumps({"bench": "sweep", "n": N, "t": T, "pairs": P, "lines": len(periods), "sweep_ms": round(sweep_ms, 3), "lines_ms": round(lines_ms, 3),
                  "parameter_sweep_ma_ms": round(both_ms, 3), "loop_ms": round(loop_ms, 3), "exact_columns_bitwise": all(exact.values()),
                  "max_rel_diff": max(rel.values())}))
