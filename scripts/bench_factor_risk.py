"""BASELINE config 4: 10000 symbols x 5040 days, the risk model of D-33 on device-resident inputs: api.risk_specific_var on the [N, T]
specific returns and api.risk_factor_cov on M = 39 and M = 264 series of T days, each at step 1 (every day from the first full window)
and step 20 (252 rebalance days), w = 252 with a half-life of 90, and api.risk_portfolio at K = 8, G = 31 on the 252 days.  Medians of
7 device-event times after a warm-up (the Python call included).  In the same run, never against the new code itself: api.factor_ts
`std` at the same shape and window -- the same LDS walk on one column, one LDS word per entry and pass where the risk row reads two and
compares, so about 2 x is expected at step 1; the ratio is printed -- and the loop the calls replace: torch.cov(aweights=) /
a weighted variance per as-of day on NaN-free inputs, over a sample of days, scaled to all of them (marked "scaled").  Then bit parity
with the numpy restatement (tests/xsec_risk_ref.py) on sampled symbols and days.
--one: only two step-1 calls of risk_specific_var, for a kernel trace."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
N, T, W, HL, K, G31 = 10000, 5040, 252, 90.0, 8, 31
g = torch.Generator(device="cuda"); g.manual_seed(1)
x = 0.02 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
om = api.risk_weights(W, HL)
if "--one" in sys.argv:
    for _ in range(2):
        api.risk_specific_var(x, om, W // 2, day0=W - 1)
    torch.cuda.synchronize()
    sys.exit(0)
def timed(fn, reps=7):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))
STEPS = ((1, W - 1), (20, 19))                      # (step, day0): 4789 days from the first full window; the 252 days 19, 39, ...
std = timed(lambda: api.factor_ts(x, api.TS_OPS["std"], W))
print(f"factor_ts std [N, T] w={W}                      {std:9.3f} ms  ({N * T} rows)")
for step, day0 in STEPS:
    D = (T - 1 - day0) // step + 1
    ms = timed(lambda: api.risk_specific_var(x, om, W // 2, day0=day0, step=step))
    print(f"risk_specific_var [N, T] step={step:2d} D={D:4d}          {ms:9.3f} ms  x{ms / std:5.2f} of std; per row x{ms / (N * D) / (std / (N * T)):5.2f}")
xh = x.clone()
xh[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
ms = timed(lambda: api.risk_specific_var(xh, om, W // 2, day0=W - 1))
print(f"risk_specific_var, 1 % NaN cells, step= 1            {ms:9.3f} ms  x{ms / std:5.2f} of std")
f = 0.01 * torch.randn((264, T), dtype=torch.float64, device="cuda", generator=g)
std_m = {M: timed(lambda: api.factor_ts(f[:M], api.TS_OPS["std"], W)) for M in (39, 264)}
for M in (39, 264):
    for step, day0 in STEPS:
        D = (T - 1 - day0) // step + 1
        ms = timed(lambda: api.risk_factor_cov(f[:M], om, W // 2, day0=day0, step=step))
        print(f"risk_factor_cov M={M:3d} step={step:2d} D={D:4d}              {ms:9.3f} ms  ({M * (M + 1) // 2 * D} pairs; std of the {M} rows: {std_m[M]:.3f} ms)")
# the portfolio on the model of the 252 days
step, day0 = STEPS[1]
M = K + G31
cov = api.risk_factor_cov(f[:M], om, W // 2, day0=day0, step=step)
sv = api.risk_specific_var(x, om, 2, day0=day0, step=step)
ind = torch.randint(0, G31, (N,), device="cuda", generator=g, dtype=torch.int32)
expo = [torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g) for _ in range(K)]
h = torch.rand((N, T), dtype=torch.float64, device="cuda", generator=g)
h[torch.rand((N, T), device="cuda", generator=g) < 0.5] = 0.0
ms = timed(lambda: api.risk_portfolio(h, expo, cov, sv, ind, day0, step))
print(f"risk_portfolio K={K} G={G31} D={cov.shape[0]}                    {ms:9.3f} ms")
# the loops the calls replace, on a sample of as-of days
omd = torch.from_numpy(om).cuda()
days = list(range(W - 1, T, (T - W) // 8))[:8]
for M in (39, 264):
    ms = timed(lambda: [torch.cov(f[:M, t - W + 1:t + 1], aweights=omd) for t in days], 3)
    for step, day0 in STEPS:
        D = (T - 1 - day0) // step + 1
        print(f"torch.cov(aweights) M={M:3d}: {ms:8.2f} ms for {len(days)} days -> {ms * D / len(days):10.1f} ms scaled to the {D} days of step {step}")
def wvar(t):
    win = x[:, t - W + 1:t + 1]
    m = (win * omd).sum(dim=1, keepdim=True) / omd.sum()
    return ((win - m) ** 2 * omd).sum(dim=1) / (omd.sum() - (omd * omd).sum() / omd.sum())
ms = timed(lambda: [wvar(t) for t in days], 3)
for step, day0 in STEPS:
    D = (T - 1 - day0) // step + 1
    print(f"torch weighted variance [N, w]: {ms:8.2f} ms for {len(days)} days -> {ms * D / len(days):10.1f} ms scaled to the {D} days of step {step}")
# parity on sampled symbols and days
import xsec_risk_ref as R
rows = [0, 1, 255, 256, 5000, N - 1]
dd = np.array([W - 1, 1000, 2519, 2520, 4000, T - 1])
di = torch.from_numpy(dd - (W - 1)).cuda()
got = api.risk_specific_var(xh, om, W // 2, day0=W - 1)
exp, _ = R.specific_var(xh[rows].cpu().numpy(), om, dd, W // 2)
ok = bool((got[rows][:, di].cpu().numpy().view(np.uint64) == exp.view(np.uint64)).all())
gc = api.risk_factor_cov(f[:39], om, W // 2, day0=W - 1)
ec, _ = R.factor_cov(f[:39].cpu().numpy(), om, dd, W // 2)
ok &= bool((gc[di].cpu().numpy().view(np.uint64) == ec.view(np.uint64)).all())
print(f"parity on sampled symbols and days (specific_var with 1 % NaN; factor_cov M = 39): {ok}")
