"""The seven ParameterSweep methods of pq_backtest_sweep_rules (D-25) on BASELINE config 3: 5 000 symbols x 2 520 days of synthetic.py
OHLCV, device resident.  For each of bband / stoch / cci / adx / breakout / reversion / grid a representative grid is timed three ways
in the same run -- the sweep launch on ready lines, the method end to end (its lines computed once + the launch), and the loop it
replaces, `Strategy.x` + `api.backtest_vectorized(want_curves=False)` per parameter set -- with device events after a warm-up (the Python
calls included) over a window of at least half a second.  Then max_drawdown / max_profit / win_rate / total_trades of the sweep and the
loop are compared bit for bit on every cell, and the largest relative difference of the other four columns is printed.  One JSON line
per method and one for the run."""
import sys; sys.path.insert(0, ".")
import json, math
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import api
from polars_quant_amd.synthetic import gen_ohlcv
N, T = 5000, 2520
d = gen_ohlcv(0x5EED0002, N, T, 0)
df = {k: torch.from_numpy(d[k]).cuda() for k in ("open", "high", "low", "close", "volume")}
close = df["close"]
GRIDS = {   # method -> (arguments of ParameterSweep.method, the Strategy keyword of each SweepResult.params column)
    "bband": (((10, 15, 20, 30, 50), (1.0, 1.5, 2.0, 2.5)), {"period": "period", "nbdev": "nbdev"}),
    "stoch": (((5, 9, 14), 3, 3, (10, 20, 30), (70, 80, 90)), {k: k for k in ("fastk_period", "slowk_period", "slowd_period", "oversold", "overbought")}),
    "cci": (((10, 14, 20, 30), (-150, -100, -50), (50, 100, 150)), {"period": "period", "oversold": "oversold", "overbought": "overbought"}),
    "adx": (((7, 10, 14, 20, 28), (15, 20, 25, 30)), {"period": "period", "threshold": "threshold"}),
    "breakout": (((5, 10, 20, 30, 55, 100),), {"period": "period"}),
    "reversion": (((10, 20, 30, 50), (1.0, 1.5, 2.0, 2.5)), {"period": "period", "threshold": "threshold"}),
    "grid": (((10, 20, 50), (1, 2, 3, 5, 8)), {"base_period": "base_period", "grid_pct": "grid_pct"}),
}
def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    reps = max(3, min(400, math.ceil(500.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, reps
class Capture(pq.ParameterSweep):
    """keeps the lines and the table a method hands to the launch, so the launch can be timed on ready lines"""
    def run_rules(self, lines, rules, params=None, price_col="close"):
        self.kept = (lines, api.sweep_rules(rules))
        return super().run_rules(lines, rules, params, price_col)
strat = pq.Strategy()
rows = []
for name, (args, keys) in GRIDS.items():
    cap = Capture(df)
    res = getattr(cap, name)(*args)
    lines, tab = cap.kept
    P, n_lines = len(tab), len(lines)
    kw = [{keys[k]: (int(v[i]) if v.dtype.kind == "i" else float(v[i])) for k, v in res.params.items()} for i in range(P)]
    def loop(keep=None):
        for i in range(P):
            sig = getattr(strat, name)(df, **kw[i])
            summ = api.backtest_vectorized(close, sig["buy_signal"], sig["sell_signal"], want_curves=False)[3]
            if keep is not None: keep[i] = summ
    launch_ms, launch_reps = timed(lambda: api.backtest_sweep_rules(close, lines, tab))
    del lines, cap
    method_ms, method_reps = timed(lambda: getattr(pq.ParameterSweep(df), name)(*args))
    loop_ms, loop_reps = timed(loop)
    ref = torch.empty((P, N, 8), dtype=torch.float64, device="cuda")
    loop(ref)
    g, r = res.summary.cpu().numpy(), ref.cpu().numpy()
    exact = all(bool((g[..., j].view(np.uint64) == r[..., j].view(np.uint64)).all()) for j in (1, 5, 6, 7))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = max(float(np.nanmax(np.abs(g[..., j] - r[..., j]) / np.maximum(np.abs(r[..., j]), 1e-300))) for j in (0, 2, 3, 4))
    row = {"bench": "sweep_rules", "method": name, "n": N, "t": T, "sets": P, "lines": n_lines,
           "rule": int(tab["rule"][0]), "launch_ms": round(launch_ms, 3), "method_ms": round(method_ms, 3), "loop_ms": round(loop_ms, 3),
           "loop_over_method": round(loop_ms / method_ms, 2), "exact_columns_bitwise": exact, "max_rel_diff": rel,
           "mean_trades": round(float(g[..., 7].mean()), 1)}
    rows.append(row)
    print(f"{name:9s} rule {row['rule']}  {P:3d} sets over {row['lines']:2d} lines: launch {launch_ms:8.3f} ms ({launch_reps} reps)  method {method_ms:8.3f} ms "
          f"({method_reps} reps)  loop {loop_ms:8.3f} ms ({loop_reps} reps) = {loop_ms / method_ms:.1f} x the method; exact columns bitwise {exact}, "
          f"others within {rel:.1e}, {row['mean_trades']} trades per cell")
    print(json.dumps(row))
    del res, ref, g, r
    torch.cuda.empty_cache()
print(json.dumps({"bench": "sweep_rules", "n": N, "t": T, "methods": len(rows), "all_exact": all(r["exact_columns_bitwise"] for r in rows),
                  "slowest_ratio": min(r["loop_over_method"] for r in rows)}))
