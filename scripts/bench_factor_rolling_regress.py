"""BASELINE config 4: 10000 symbols x 5040 days, the rolling-window OLS of D-28 (Factor.rolling_beta / idiosyncratic_volatility /
rolling_regression) at windows 20 / 60 / 252 on device-resident return columns: K = 1 with a [T] market series and K = 3 with [N, T]
factors, each with one output and with all five.  In the same run and on the same shape: Factor.volatility at the same windows as the
yardstick (D-21's windowed kernel: one column, two passes), and the host method the K = 1 call replaces -- sliding sums by torch.cumsum
(beta = (Sxy - Sx Sy / w) / (Sxx - Sx Sx / w)), which has another rounding order, so the largest deviation of its beta from the kernel's
is reported.  Device-event times after a warm-up (the Python call included), the rate over the bytes floor ((the [N, T] inputs + the
output planes) x 8 B per cell), and a bit-parity check against the numpy restatement (tests/xsec_rolling_regress_ref.py) on a sample
of symbols."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import Factor, api
import xsec_rolling_regress_ref as R
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(28)
rnd = lambda *s: torch.randn(s, dtype=torch.float64, device="cuda", generator=g)   # noqa: E731
mkt = 0.01 * rnd(T)
facs = [0.01 * rnd(N, T) for _ in range(3)]
y = (0.5 + rnd(N, 1)) * mkt + 0.3 * facs[0] - 0.2 * facs[1] + 0.1 * facs[2] + 0.015 * rnd(N, T)
y[torch.rand((N, T), device="cuda", generator=g) < 0.001] = float("nan")
price = torch.exp(torch.cumsum(torch.nan_to_num(y), dim=1))
fac = Factor()
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
def cumsum_beta(w):
    """the K = 1 slope from sliding sums: four cumulative sums, window sums as differences"""
    yy = torch.nan_to_num(y)
    def win(c):
        out = c.clone()
        out[..., w:] -= c[..., :-w]
        return out
    sx, sxx = win(torch.cumsum(mkt, 0)), win(torch.cumsum(mkt * mkt, 0))
    sy, sxy = win(torch.cumsum(yy, 1)), win(torch.cumsum(yy * mkt, 1))
    return (sxy - sx * sy / w) / (sxx - sx * sx / w)
cells = N * T
WINDOWS = (20, 60, 252)
cases = []                                           # (name, [N, T] planes moved at least, call)
for w in WINDOWS:
    cases += [(f"rolling_beta(K=1 series, {w})", 2, lambda w=w: fac.rolling_beta(y, mkt, w)),
              (f"rolling_regression(K=1 series, {w})", 6, lambda w=w: fac.rolling_regression(y, [mkt], w)),
              (f"idiosyncratic_volatility(K=3, {w})", 5, lambda w=w: fac.idiosyncratic_volatility(y, facs, w)),
              (f"rolling_regression(K=3, {w})", 11, lambda w=w: fac.rolling_regression(y, facs, w)),
              (f"Factor.volatility({w}) (D-21)", 2, lambda w=w: fac.volatility(price, w)),
              (f"cumsum sliding sums, K=1 beta ({w})", 2, lambda w=w: cumsum_beta(w))]
for name, planes, fn in cases:
    ms, _ = timed(fn)
    print(f"{name:40s} {ms:9.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {planes*8*cells/ms/1e6:7.0f} GB/s over the bytes floor", flush=True)
for w in WINDOWS:
    kb, hb = fac.rolling_beta(y, mkt, w), cumsum_beta(w)
    have = ~torch.isnan(kb)
    dev = (kb - hb)[have].abs().max().item()
    print(f"cumsum beta against the kernel, window {w}: largest deviation {dev:.3g} (largest |beta| {kb[have].abs().max().item():.3g})")
# parity on sampled symbols (the fits run along days, so whole rows are compared)
rows = [0, 1, 777, 4999, 5000, 9999]
yh, mh, fh = y[rows].cpu().numpy(), mkt.cpu().numpy(), [f[rows].cpu().numpy() for f in facs]
ok = True
for w in WINDOWS:
    for xs_d, xs_h in (([mkt], [mh]), (facs, fh)):
        got, exp = api.factor_rolling_regress(y, xs_d, w), R.rolling_regress(yh, xs_h, w)
        for k in R.OUTPUTS:
            ok &= not bool((got[k][..., rows, :].cpu().numpy().view(np.uint64) != exp[k].view(np.uint64)).any())
print(f"parity on {len(rows)} sampled symbols (K = 1 and K = 3, every window and output): {ok}")
