"""BASELINE config 4: 10000 symbols x 5040 days, linear() of D-24: the pooled OLS over all M = 50.4 million rows at K = 1 / 3 / 8, with
and without the two output columns, on device-resident inputs.  Device-event times after a warm-up (the Python call included) over a
window of at least half a second; the bytes that must move -- three passes over the K + 1 input columns and two output columns,
(3 (K + 1) + 2) 8 M, or 3 (K + 1) 8 M without outputs -- over the measured time as a fraction of the achievable HBM bandwidth
(6.3 TB/s); in the same run ts_regress at K = 3 with [N, T] factors (the same bytes in the same three passes, without the outputs) and
the time of two [N, T] column stores; and a bit-parity check of coef / t / R^2 / n / pred / resid at K = 1 on all rows against the numpy
restatement (tests/linear_ref.py)."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import math
import numpy as np, torch
from polars_quant_amd import api
import linear_ref as R
N, T = 10000, 5040
HBM = 6.3e12   # achievable bytes/s
g = torch.Generator(device="cuda"); g.manual_seed(1)
F = torch.randn((8, N, T), dtype=torch.float64, device="cuda", generator=g)
r = 0.1 * F[0] - 0.05 * F[1] + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
fs = [F[j] for j in range(8)]
M = N * T
def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    reps = max(5, min(400, math.ceil(500.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, reps
ms_of = {}
for K in (1, 3, 8):
    for outputs in (True, False):
        nbytes = (3 * (K + 1) + (2 if outputs else 0)) * 8 * M
        ms, reps = timed(lambda: api.linear(fs[:K], r, outputs=outputs))
        ms_of[K, outputs] = ms
        print(f"linear K={K} outputs={str(outputs):5s} {ms:8.3f} ms ({reps} reps)  {nbytes/1e9:6.2f} GB  {nbytes/ms/1e9:6.2f} TB/s = "
              f"{100*nbytes/(ms*1e-3)/HBM:5.1f} % of {HBM/1e12} TB/s")
ts, reps = timed(lambda: api.ts_regress(fs[:3], r))
nb = 3 * 4 * 8 * M
print(f"ts_regress K=3 [N,T]       {ts:8.3f} ms ({reps} reps)  {nb/1e9:6.2f} GB  {nb/ts/1e9:6.2f} TB/s = {100*nb/(ts*1e-3)/HBM:5.1f} %")
p, q = torch.empty((N, T), dtype=torch.float64, device="cuda"), torch.empty((N, T), dtype=torch.float64, device="cuda")
st, reps = timed(lambda: (p.fill_(1.0), q.fill_(1.0)))
print(f"two [N,T] column stores    {st:8.3f} ms ({reps} reps)  {2*8*M/st/1e9:6.2f} TB/s")
print(f"linear K=3 with outputs {ms_of[3, True]:.3f} ms against ts_regress + two stores {ts + st:.3f} ms; without outputs "
      f"{ms_of[3, False]:.3f} ms against ts_regress {ts:.3f} ms")
# parity at K = 1 on all rows, as [N, T] and (the same logical rows) as one flat column
got = api.linear([fs[0]], r)
flat = api.linear([fs[0].reshape(-1)], r.reshape(-1))
exp = R.linear([fs[0].cpu().numpy()], r.cpu().numpy())
ok = True
for k, e in (("coef", "coef"), ("t_stat", "t"), ("r_squared", "r2"), ("pred", "pred"), ("resid", "resid")):
    ev = np.asarray(exp[e]).reshape(-1).view(np.uint64)
    for res in (got, flat):
        ok &= bool((res[k].cpu().numpy().reshape(-1).view(np.uint64) == ev).all())
ok &= int(got["n"]) == exp["n"] == int(flat["n"])
print(f"parity of coef / t / R^2 / n / pred / resid at K = 1 on {M} rows ([N, T] and flat): {ok}")
