"""BASELINE config 4: 10000 symbols x 5040 days, the general factor calculations of D-20 (Factor.rank / normalize / weighted / ratio /
diff) on device-resident inputs, next to two yardsticks from the unchanged code in the same run: Factor().quantile(f, r, 5) (D-15: the
same prep and day sort as the rank family) and clean(f, standardize=True) (D-16: the bytes of the sort-free methods).  Device-event times
after a warm-up (the Python call included), the rate over the bytes floor (each input column read once, the output written once), and a
bit-parity check against the numpy restatement (tests/xsec_build_ref.py) on sampled days."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import Factor
import xsec_build_ref as R
N, T, G = 10000, 5040, 31
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
f[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
w = torch.exp(torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g) + 10.0)
r = 0.1 * torch.nan_to_num(f) + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
grp = torch.randint(0, G, (N,), device="cuda", generator=g)
fac = Factor()
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
# (name, columns of the bytes floor, call)
cases = [("rank", 2, lambda: fac.rank(f)),
         ("rank descending pct", 2, lambda: fac.rank(f, ascending=False, pct=True)),
         ("normalize quantile", 2, lambda: fac.normalize(f, "quantile")),
         ("normalize zscore", 2, lambda: fac.normalize(f, "zscore")),
         ("normalize minmax", 2, lambda: fac.normalize(f, "minmax")),
         ("weighted", 3, lambda: fac.weighted(f, w)),
         (f"weighted, {G} groups", 3, lambda: fac.weighted(f, w, grp)),
         ("ratio", 3, lambda: fac.ratio(f, w)),
         ("diff normalize", 3, lambda: fac.diff(f, w, normalize=True)),
         ("quantile Q=5 (D-15)", 2, lambda: fac.quantile(f, r, 5)),
         ("clean standardize (D-16)", 2, lambda: pq.clean(f, standardize=True))]
for name, ncols, fn in cases:
    ms, _ = timed(fn)
    print(f"{name:28s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {ncols*8*cells/ms/1e6:7.0f} GB/s over the bytes floor", flush=True)
# parity on sampled days
days = [0, 1, 1000, 2519, 2520, 4000, 5039]
fs, ws, gs = f[:, days].cpu().numpy(), w[:, days].cpu().numpy(), grp.cpu().numpy()
def eq(got, exp, nan_ok=False):
    got = got[:, days].cpu().numpy()
    d = got.view(np.uint64) != exp.view(np.uint64)
    if nan_ok: d &= ~(np.isnan(got) & np.isnan(exp) & ~R.isnull(got) & ~R.isnull(exp))
    return not bool(d.any())
ok = eq(fac.rank(f), R.rank(fs)) and eq(fac.rank(f, ascending=False, pct=True), R.rank(fs, "pct", True))
ok &= all(eq(fac.normalize(f, m), R.normalize(fs, m)) for m in R.METHODS)
ok &= eq(fac.weighted(f, w), R.weighted(fs, ws)) and eq(fac.weighted(f, w, grp), R.weighted(fs, ws, gs, G))
ok &= eq(fac.ratio(f, w), R.binary(fs, ws, "ratio"), True) and eq(fac.diff(f, w, normalize=True), R.binary(fs, ws, "reldiff"), True)
print(f"parity on {len(days)} sampled days (every method): {ok}")
