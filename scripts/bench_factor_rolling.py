"""BASELINE config 4: 10000 symbols x 5040 days, the rolling technical factors of D-21 (Factor.moving_average / momentum / volatility /
skewness / relative_strength) at windows 20 / 60 / 252 on a device-resident price column, next to two yardsticks from the unchanged code
in the same run and on the same bytes: pq.SMA(x, 20) as a direct call (the TA-Lib moving average: one column in, one out) and Factor.diff
(D-20's elementwise kernel: two columns in, one out).  Device-event times after a warm-up (the Python call included), the rate over the
bytes floor (16 B per cell: the column read once, the output written once), the ratio of moving_average(20) to SMA(20), and a bit-parity
check against the numpy restatement (tests/xsec_rolling_ref.py) on a sample of symbols."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import Factor
import xsec_rolling_ref as R
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(1)
x = torch.exp(torch.cumsum(0.02 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g), dim=1))
clean = x.clone()                                    # SMA refuses nothing here, but it is timed on the column without holes
x[torch.rand((N, T), device="cuda", generator=g) < 0.001] = float("nan")
fac = Factor()
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
WINDOWS = (20, 60, 252)
METHODS = (("moving_average", "mean"), ("momentum", "momentum"), ("volatility", "volatility"), ("skewness", "skewness"),
           ("relative_strength", "relative_strength"))
cases = [(f"{name}({w})", 2, (lambda name=name, w=w: getattr(fac, name)(x, w))) for name, _ in METHODS for w in WINDOWS]
cases += [("momentum(231, skip=21)", 2, lambda: fac.momentum(x, 231, 21)),
          ("moving_average(20), no holes", 2, lambda: fac.moving_average(clean, 20)),
          ("SMA(20) direct call", 2, lambda: pq.SMA(clean, 20)),
          ("Factor.diff (D-20)", 3, lambda: fac.diff(x, clean))]
ms_of = {}
for name, ncols, fn in cases:
    ms, _ = timed(fn)
    ms_of[name] = ms
    print(f"{name:30s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {ncols*8*cells/ms/1e6:7.0f} GB/s over the bytes floor", flush=True)
print(f"moving_average(20) / SMA(20): {ms_of['moving_average(20), no holes'] / ms_of['SMA(20) direct call']:.2f}x "
      f"(with holes: {ms_of['moving_average(20)'] / ms_of['SMA(20) direct call']:.2f}x)")
# parity on sampled symbols (the ops run along days, so whole rows are compared)
rows = [0, 1, 777, 4999, 5000, 9999]
xs = x[rows].cpu().numpy()
ok = True
for name, op in METHODS:
    for w in WINDOWS:
        got = getattr(fac, name)(x, w)[rows].cpu().numpy()
        ok &= not bool((got.view(np.uint64) != R.rolling(xs, op, w).view(np.uint64)).any())
got = fac.momentum(x, 231, 21)[rows].cpu().numpy()
ok &= not bool((got.view(np.uint64) != R.rolling(xs, "momentum", 231, 21).view(np.uint64)).any())
print(f"parity on {len(rows)} sampled symbols (every op and window): {ok}")
