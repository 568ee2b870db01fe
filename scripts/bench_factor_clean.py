"""BASELINE config 4: 10000 symbols x 5040 days, per-day factor cleaning (D-16): each winsorize mode alone, size neutralization alone,
industry neutralization alone (31 industries), standardize alone, and the README's full pipeline (mad + log cap + industry +
standardize), all on the same device-resident inputs.  Device-event times after a warm-up, bytes moved by a shape-based model over the
measured time, and a bit-parity check of the full pipeline against the numpy restatement (tests/xsec_clean_ref.py) on sampled days."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
import xsec_clean_ref as R
N, T, G = 10000, 5040, 31
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
f[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
cap = torch.exp(torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g) + 10.0)
ind = torch.randint(0, G, (N,), device="cuda", generator=g)
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
# bytes floor (per call): the kernels read the factor (8 B/cell), z (8) and the industry codes (4) when those steps are on, once each,
# and write the output (8) once; the passes re-read the columns, so the rate over this floor is below the achieved traffic
def floor(cap_on, ind_on):
    return (8 + (8 if cap_on else 0) + (4 if ind_on else 0) + 8) * cells
cases = [("mad", "mad", None, None, False), ("sigma", "sigma", None, None, False), ("percentile", "percentile", None, None, False),
         ("cap only", None, cap, None, False), ("industry only", None, None, ind, False), ("standardize only", None, None, None, True),
         ("full pipeline", "mad", cap, ind, True)]
for name, mode, c, i, std in cases:
    ms, _ = timed(lambda: api.factor_clean(f, mode, None, c, True, i, std))
    b = floor(c is not None, i is not None)
    print(f"{name:17s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {b/ms/1e6:7.0f} GB/s over the bytes floor")
# parity of the full pipeline on sampled days
days = [0, 1, 1000, 2519, 2520, 4000, 5039]
out = api.factor_clean(f, "mad", None, cap, True, ind, True)
exp = R.clean(f[:, days].cpu().numpy(), "mad", None, torch.log(cap[:, days]).cpu().numpy(), ind.cpu().numpy(), None, True)
ok = bool((out[:, days].cpu().numpy().view(np.uint64) == exp.view(np.uint64)).all())
print(f"parity of the full pipeline on {len(days)} sampled days: {ok}")
