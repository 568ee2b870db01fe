"""Walk-forward sweep (D-26, pq_backtest_sweep_windows + pq_sweep_select) on BASELINE config 3: 5 000 symbols x 2 520 days of synthetic.py
data, the 90-pair SMA grid of bench_sweep.py (18 lines, computed once over the full history), rolling folds of 504 train + 126 test rows:
16 folds, 32 windows, about 4 x the rows of a plain sweep.  Device-event times after a warm-up (the Python calls included) over a window
of at least half a second: the two launches (the windowed sweep, the selection), and -- in the same run -- the loop they replace: one
api.backtest_sweep per window on row slices of the price and of every line (views, no copy) plus torch argmax / gather per fold; then
the two compared bit for bit."""
import sys; sys.path.insert(0, ".")
import json, math
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import api, sweep
from polars_quant_amd.synthetic import gen_ohlcv
N, T, TRAIN, TEST = 5000, 2520, 504, 126
METRIC = pq.SUMMARY_KEYS.index("sharpe_ratio")
close = torch.from_numpy(gen_ohlcv(0x5EED0002, N, T, 0)["close"]).cuda()
fasts, slows = list(range(5, 55, 5)), list(range(20, 220, 20))
periods, rules, params = sweep.ma_grid(fasts, slows)
P = len(rules)
lines = [api.call("sma", close, timeperiod=p)[0] for p in periods]
folds = pq.walk_forward_windows(T, TRAIN, TEST)
F = len(folds)
windows = folds.reshape(2 * F, 2)
train, test = 2 * np.arange(F), 2 * np.arange(F) + 1
def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    reps = max(3, min(400, math.ceil(500.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, reps
out = torch.empty((2 * F, N, P, 8), dtype=torch.float64, device="cuda")
def launches():
    summ = api.backtest_sweep(close, lines, rules, windows=windows, out=out)
    return (summ,) + api.sweep_select(summ, train, test, METRIC)
def loop():
    summ = [api.backtest_sweep(close[:, t0:t1], [l[:, t0:t1] for l in lines], rules) for t0, t1 in windows.tolist()]
    chosen, ins, outs = [], [], []
    for k in range(F):
        m = summ[2 * k][..., METRIC]
        idx = torch.where(torch.isnan(m), torch.full_like(m, float("-inf")), m).argmax(dim=0)
        idx = torch.where(torch.isnan(m).all(dim=0), torch.zeros_like(idx), idx)
        g = idx[None, :, None].expand(1, -1, 8)
        chosen.append(idx); ins.append(summ[2 * k].gather(0, g)[0]); outs.append(summ[2 * k + 1].gather(0, g)[0])
    return torch.stack(summ), torch.stack(chosen), torch.stack(ins), torch.stack(outs)
sweep_ms, sweep_reps = timed(lambda: api.backtest_sweep(close, lines, rules, windows=windows, out=out))
both_ms, both_reps = timed(launches)
loop_ms, loop_reps = timed(loop)
plain_ms, plain_reps = timed(lambda: api.backtest_sweep(close, lines, rules))
rows = int((windows[:, 1] - windows[:, 0]).sum())
print(f"{N} x {T}, {P} SMA pairs over {len(periods)} lines, {F} folds of {TRAIN} + {TEST} rows = {2 * F} windows, {rows} rows ({rows / T:.2f} x the history)")
print(f"windowed sweep launch             {sweep_ms:9.3f} ms ({sweep_reps} reps)  {N * P * rows / sweep_ms / 1e6:8.2f} G cell-rows/s")
print(f"windowed sweep + select           {both_ms:9.3f} ms ({both_reps} reps)")
print(f"loop of {2 * F} sweeps + argmax / gather {loop_ms:9.3f} ms ({loop_reps} reps) = {loop_ms / both_ms:.2f} x the two launches")
print(f"plain sweep of the whole history  {plain_ms:9.3f} ms ({plain_reps} reps)  {N * P * T / plain_ms / 1e6:8.2f} G cell-rows/s")
got, ref = launches(), loop()
same = [bool((a.cpu().numpy().view(np.uint64 if a.dtype == torch.float64 else a.cpu().numpy().dtype) ==
              b.cpu().numpy().view(np.uint64 if b.dtype == torch.float64 else b.cpu().numpy().dtype)).all())
        for a, b in ((got[0], ref[0]), (got[1].long(), ref[1]), (got[2], ref[2]), (got[3], ref[3]))]
print(f"bitwise equal to the loop (summary, chosen, in-sample, out-of-sample): {same}; distinct chosen sets {len(torch.unique(got[1]))}")
print(json.dumps({"bench": "sweep_windows", "n": N, "t": T, "pairs": P, "folds": F, "windows": 2 * F, "window_rows": rows,
                  "windowed_sweep_ms": round(sweep_ms, 3), "two_launches_ms": round(both_ms, 3), "loop_ms": round(loop_ms, 3),
                  "loop_over_launches": round(loop_ms / both_ms, 3), "plain_sweep_ms": round(plain_ms, 3), "bitwise_equal_to_the_loop": all(same)}))
