"""BASELINE config 4: 10000 symbols x 5040 days, the time-series operators of D-29 (Factor.ts_sum / ts_rank / ts_argmax / decay_linear /
ts_corr) at windows 20 / 60 / 252 on device-resident columns.  Every case is called REPS times after a warm-up, each call between its
own pair of device events (the Python call included); the minimum and the median are printed.  In the same process and on the same
bytes: Factor.moving_average at the same window as the yardstick (ts_sum does the same loads and additions), and at window 20 the torch
formulation a user would write today for ts_rank and ts_argmax (unfold + comparison / argmax; no NULL handling).  Bit parity with the
numpy restatement (tests/xsec_ts_ref.py) on a sample of symbols."""
import statistics
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import Factor
import xsec_ts_ref as R
N, T, REPS = 10000, 5040, 7
g = torch.Generator(device="cuda"); g.manual_seed(1)
def column():
    x = torch.exp(torch.cumsum(0.02 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g), dim=1))
    x[torch.rand((N, T), device="cuda", generator=g) < 0.001] = float("nan")
    return x
x, y = column(), column()
fac = Factor()
def timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return min(ms), statistics.median(ms)
WINDOWS = (20, 60, 252)
METHODS = (("ts_sum", "sum"), ("ts_rank", "rank"), ("ts_argmax", "argmax"), ("decay_linear", "decay_linear"), ("ts_corr", "corr"))
def torch_rank(w):
    win = x.unfold(1, w, 1)                            # [N, T - w + 1, w], a view
    last = win[..., -1:]
    return ((win < last).sum(-1) * 2 + (win == last).sum(-1) + 1) * 0.5
def torch_argmax(w):
    return x.unfold(1, w, 1).argmax(-1).to(torch.float64)
cases = []
for w in WINDOWS:
    cases.append((f"moving_average({w}) [yardstick]", 2, lambda w=w: fac.moving_average(x, w)))
    for name, op in METHODS:
        cases.append((f"{name}({w})", 3 if op == "corr" else 2, (lambda name=name, w=w: getattr(fac, name)(x, y, w)) if op == "corr"
                      else (lambda name=name, w=w: getattr(fac, name)(x, w))))
cases += [("torch unfold rank(20)", 2, lambda: torch_rank(20)), ("torch unfold argmax(20)", 2, lambda: torch_argmax(20))]
cells = N * T
res = {}
for name, ncols, fn in cases:
    lo, med = timed(fn)
    res[name] = (lo, med)
    print(f"{name:34s} min {lo:8.3f} ms  median {med:8.3f} ms  {ncols*8*cells/med/1e6:7.0f} GB/s over the bytes floor (median)", flush=True)
for w in WINDOWS:
    print(f"ts_sum({w}) / moving_average({w}): {res[f'ts_sum({w})'][1] / res[f'moving_average({w}) [yardstick]'][1]:.3f}x (medians)")
for name in ("rank", "argmax"):
    print(f"torch unfold {name}(20) / ts_{name}(20): {res[f'torch unfold {name}(20)'][1] / res[f'ts_{name}(20)'][1]:.1f}x (medians)")
# parity on sampled symbols (the ops run along days, so whole rows are compared)
rows = [0, 1, 777, 4999, 5000, 9999]
xs, ys = x[rows].cpu().numpy(), y[rows].cpu().numpy()
ok = True
for name, op in METHODS:
    for w in WINDOWS:
        got = (getattr(fac, name)(x, y, w) if op == "corr" else getattr(fac, name)(x, w))[rows].cpu().numpy()
        exp = R.ts_pair(xs, ys, op, w) if op == "corr" else R.ts(xs, op, w)
        ok &= not bool((got.view(np.uint64) != exp.view(np.uint64)).any())
print(f"parity on {len(rows)} sampled symbols (every op and window): {ok}")
