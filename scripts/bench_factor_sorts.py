"""BASELINE config 4: 10000 symbols x 5040 days, quantile sorts / long-short legs / coverage / IC statistics (D-15) next to Rank-IC,
all in one run on the same device-resident inputs.  Device-event times after a warm-up, bytes moved by a shape-based model over the
measured time, and a bit-parity check against the numpy restatement (tests/xsec_ref.py) on a sample of adjacent day pairs."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
import xsec_ref as X
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r = 0.1 * f + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
# bytes model (algorithmic, per call): the sorts read factor + return (16 B/cell), write + read day-major keys (16), write + read
# day-major labels (2), write + read symbol-major labels (2), read the return again (8): 44 B/cell; coverage reads the factor (8)
models = {"quantiles": 44 * cells, "long_short": 44 * cells, "coverage": 8 * cells, "rank_ic": 16 * cells}
ms_r, (ic, nv) = timed(lambda: api.factor_ic(f, r, 1))
ms_q5, q5 = timed(lambda: api.factor_quantiles(f, r, 5))
ms_q10, _ = timed(lambda: api.factor_quantiles(f, r, 10))
ms_ls, ls = timed(lambda: api.factor_long_short(f, r, 0.2, 0.2))
ms_c, cov = timed(lambda: api.factor_coverage(f))
ms_s, st = timed(lambda: api.ic_stats(ic))
for name, ms, b in (("Rank-IC", ms_r, models["rank_ic"]), ("quantiles(5)", ms_q5, models["quantiles"]),
                    ("quantiles(10)", ms_q10, models["quantiles"]), ("long_short", ms_ls, models["long_short"]),
                    ("coverage", ms_c, models["coverage"])):
    print(f"{name:14s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {b/ms/1e6:7.0f} GB/s (model)")
print(f"{'ic_stats':14s} {ms_s:8.3f} ms  ({T} days)")
# parity on a sample of adjacent day pairs
days = [1, 2, 1000, 2519, 2520, 4000, 5039]
need = X.sample_days(days, T)
fs, rs = f[:, need].cpu().numpy(), r[:, need].cpu().numpy()
local = [need.index(t) for t in days]
ok = True
for mode, q, got, key in ((0, 5, api.factor_quantiles(f, r, 5, labels=True), "spread"), (1, 0, api.factor_long_short(f, r, 0.2, 0.2, labels=True), "ls_return")):
    exp = X.groups(fs, rs, mode, q, 0.2, 0.2, days=local)
    ok &= bool((got["labels"][:, days].cpu().numpy() == exp["labels"]).all())
    for k in ("count", "mean_return", "turnover"):
        ok &= bool((got[k][:, days].cpu().numpy().view(np.int64 if k != "count" else np.int32) ==
                    np.asarray(exp[k]).view(np.int64 if k != "count" else np.int32)).all())
    ok &= bool((got[key][days].cpu().numpy().view(np.int64) == exp["spread"].view(np.int64)).all())
ok &= bool((cov.cpu().numpy().view(np.int64) == X.coverage(f.cpu().numpy()).view(np.int64)).all())
ok &= bool((st.cpu().numpy().view(np.int64) == X.ic_stats(ic.cpu().numpy()).view(np.int64)).all())
print(f"parity on {len(days)} sampled days (+ previous days), coverage and ic_stats: {ok}")
