"""BASELINE config 4: 10000 symbols x 5040 days, the regressions and t-tests of D-17: ic_test (Pearson IC + t-test), factor_return
(K = 1), fama_macbeth at K = 3 and K = 8, and time_series_regression at K = 3 with [T] series factors and with [N, T] factors, all on
device-resident inputs.  Device-event times after a warm-up (the Python call included), bytes moved by a shape-based model over the
measured time, and a bit-parity check of coef / t / R^2 / n against the numpy restatement (tests/xsec_regress_ref.py) on sampled days
(cross-sectional) and sampled symbols (time-series)."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import Factor, api
import xsec_regress_ref as R
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(1)
F = torch.randn((8, N, T), dtype=torch.float64, device="cuda", generator=g)
r = 0.1 * F[0] - 0.05 * F[1] + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
S = torch.randn((3, T), dtype=torch.float64, device="cuda", generator=g)     # market-like [T] series
fac = Factor()
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
# bytes floor (per call): each [N, T] input column read once (8 B/cell); the passes re-read them (IC 2 passes, regressions 3), so the
# rate over this floor is below the achieved traffic.  [T] series and the per-day / per-symbol outputs are negligible.
fs = [F[j] for j in range(8)]
cases = [("ic_test", 2, lambda: fac.ic_test(F[0], r)),
         ("factor_return K=1", 2, lambda: fac.factor_return(F[0], r)),
         ("fama_macbeth K=3", 4, lambda: fac.fama_macbeth(fs[:3], r)),
         ("fama_macbeth K=8", 9, lambda: fac.fama_macbeth(fs, r)),
         ("ts_regression K=3 [T]", 1, lambda: fac.time_series_regression([S[0], S[1], S[2]], r)),
         ("ts_regression K=3 [N,T]", 4, lambda: fac.time_series_regression(fs[:3], r))]
for name, ncols, fn in cases:
    ms, _ = timed(fn)
    print(f"{name:24s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {ncols*8*cells/ms/1e6:7.0f} GB/s over the bytes floor")
# parity on sampled days / symbols
days = [0, 1, 1000, 2519, 2520, 4000, 5039]
ok = True
for K in (3, 8):
    got = api.xsec_regress(fs[:K], r)
    exp = R.xsec_regress([f[:, days].cpu().numpy() for f in fs[:K]], r[:, days].cpu().numpy())
    for k, e in (("coef", "coef"), ("t_stat", "t"), ("r_squared", "r2")):
        gk = got[k][..., days].cpu().numpy()
        ok &= bool((gk.view(np.uint64) == exp[e].view(np.uint64)).all())
    ok &= bool((got["n"][days].cpu().numpy() == exp["n"]).all())
syms = [0, 1, 4999, 9999]
got = api.ts_regress([S[0], fs[1], S[2]], r)
exp = R.ts_regress([S[0].cpu().numpy(), fs[1][syms].cpu().numpy(), S[2].cpu().numpy()], r[syms].cpu().numpy())
for k, e in (("coef", "coef"), ("t_stat", "t"), ("r_squared", "r2")):
    ok &= bool((got[k][syms].cpu().numpy().view(np.uint64) == exp[e].view(np.uint64)).all())
ok &= bool((got["n_obs"][syms].cpu().numpy() == exp["n"]).all())
print(f"parity on {len(days)} sampled days (K = 3, 8) and {len(syms)} sampled symbols (time-series K = 3): {ok}")
