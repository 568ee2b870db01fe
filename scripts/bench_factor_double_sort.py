"""BASELINE config 4: 10000 symbols x 5040 days, the two-way sort (D-31) at 2 x 3 and 5 x 5, independent and dependent, next to the loop
of single sorts it replaces, in one run on the same device-resident inputs.  dependent loop: one api.factor_quantiles call for the
control's labels, then one per control bucket on a torch.where-masked factor; independent loop: two label calls, then the cell sums and
counts by a torch scatter_add over the cells (no turnover, no summary: less than the call computes).  Each figure is the median of 7
calls timed one by one with device events after a warm-up, the two sides alternating; min and max are the spread.  Ends with a
bit-parity check against the numpy restatement (tests/xsec_double_ref.py) on a sample of adjacent day pairs."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
import xsec_double_ref as D
import xsec_ref as X
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(1)
a = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
f = 0.5 * a + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r = 0.1 * f + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
NULL = torch.tensor(X.NULL, dtype=torch.float64, device="cuda")
def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)
def loop_dependent(qa, qb):
    la = api.factor_quantiles(a, r, qa, labels=True)["labels"]
    return [api.factor_quantiles(torch.where(la == k, f, NULL), r, qb) for k in range(qa)]
def loop_independent(qa, qb):
    la = api.factor_quantiles(a, r, qa, labels=True)["labels"]
    lb = api.factor_quantiles(f, r, qb, labels=True)["labels"]
    cell = la.to(torch.int64) * qb + lb.to(torch.int64)          # inputs without nulls: every label is a bucket
    s = torch.zeros((qa * qb, T), dtype=torch.float64, device="cuda").scatter_add_(0, cell, r)
    c = torch.zeros((qa * qb, T), dtype=torch.float64, device="cuda").scatter_add_(0, cell, torch.ones_like(r))
    return s / c
def fmt(ts):
    return f"{np.median(ts):8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"
for qa, qb in ((2, 3), (5, 5)):
    for dependent in (True, False):
        call = lambda: api.factor_double_sort(a, f, r, qa, qb, dependent)
        loop = (lambda: loop_dependent(qa, qb)) if dependent else (lambda: loop_independent(qa, qb))
        call(); loop(); torch.cuda.synchronize()
        tc, tl = [], []
        for _ in range(7):
            tc.append(once(call)); tl.append(once(loop))
        print(f"{qa} x {qb} {'dependent  ' if dependent else 'independent'}  double_sort {fmt(tc)}   loop {fmt(tl)}   "
              f"loop / call {np.median(tl) / np.median(tc):.2f}", flush=True)
# parity on a sample of adjacent day pairs
days = [1, 2, 1000, 2519, 2520, 5039]
need = X.sample_days(days, T)
cols = [x[:, need].cpu().numpy() for x in (a, f, r)]
local = [need.index(t) for t in days]
ok = True
for dependent in (True, False):
    got = api.factor_double_sort(a, f, r, 5, 5, dependent, labels=True)
    exp = D.groups(*cols, 5, 5, dependent, days=local)
    ok &= bool((got["labels"][:, days].cpu().numpy() == exp["labels"]).all())
    for k in ("count", "mean_return", "turnover", "spread_factor", "spread_control"):
        v = np.int32 if k == "count" else np.int64
        ok &= bool((got[k][:, days].cpu().numpy().view(v) == np.ascontiguousarray(exp[k]).view(v)).all())
print(f"parity on {len(days)} sampled days (+ previous days), 5 x 5, both modes: {ok}")
