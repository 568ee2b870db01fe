"""BASELINE config 4: 10000 symbols x 5040 days, the quantile portfolios of D-27 (Q = 5; rebalance every 21 days and every day; equal
and cap weights; fee 0.001) next to Factor.quantile(Q = 5) and to a torch host loop over the rebalance days (gather, index_add and a
cumulative chain) that computes the same curves on the same device-resident inputs.  Device-event means after a warm-up; the growth
pass's bytes floor is the price matrix read once at the 6.3 TB/s the project measures HBM to achieve.  `--passes` runs the four
portfolio calls alone, for a kernel trace of the passes (the pf_* kernels)."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import torch
from polars_quant_amd import api
N, T, Q, FEE, C0 = 10000, 5040, 5, 0.001, 1_000_000.0
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
price = 20.0 * torch.exp(torch.cumsum(0.02 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g), dim=1))
cap = price * torch.exp(torch.randn((N, 1), dtype=torch.float64, device="cuda", generator=g))
labels = api.factor_quantiles(f, price, Q, labels=True)["labels"]
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
def loop(days, weight):
    """the host loop a user writes today: per rebalance day a gather of the labels, base prices and weights, index_add sums per group,
    the segment's price ratios, and the chain of the capital over the rebalance days (clean prices: no held-price search)"""
    value = torch.full((Q, T), C0, dtype=torch.float64, device="cuda")
    B = torch.full((Q,), C0, dtype=torch.float64, device="cuda")
    prev = None
    for k, d in enumerate(days):
        end = days[k + 1] if k + 1 < len(days) else T - 1
        lab, p0 = labels[:, d].long(), price[:, d]
        a = weight[:, d] if weight is not None else torch.ones(N, dtype=torch.float64, device="cuda")
        mem = (lab < Q) & (p0 > 0) & (a > 0)
        idx = torch.where(mem, lab, Q)
        A = torch.zeros(Q + 1, dtype=torch.float64, device="cuda").index_add_(0, idx, a)
        w = torch.where(mem, a / A[idx], 0.0)
        wn, wo_old = w, None
        if prev is not None:
            w_old = torch.where(prev["mem"], prev["w"] * (p0 / prev["p0"]) / prev["G"][prev["idx"]], 0.0)
            same = idx == prev["idx"]
            wn, wo_old = torch.where(same, (w - w_old).abs(), w), torch.where(same, 0.0, w_old)
            B = B * prev["G"][:Q]
        tau = torch.zeros(Q + 1, dtype=torch.float64, device="cuda").index_add_(0, idx, wn)
        if prev is not None:
            tau.index_add_(0, prev["idx"], wo_old)
        B = B * (1.0 - FEE * tau[:Q])
        value[:, d] = B
        G = torch.zeros((Q + 1, end - d), dtype=torch.float64, device="cuda").index_add_(0, idx, w[:, None] * (price[:, d + 1:end + 1] / p0[:, None]))
        has = torch.zeros(Q + 1, dtype=torch.float64, device="cuda").index_add_(0, idx, torch.ones_like(w)) > 0
        G = torch.where(has[:, None], G, 1.0)
        last = end if k + 1 == len(days) else end - 1
        value[:, d + 1:last + 1] = B[:, None] * G[:Q, :last - d]
        prev = {"w": w, "p0": p0, "idx": idx, "mem": mem, "G": G[:, -1] if end > d else torch.ones(Q + 1, dtype=torch.float64, device="cuda")}
    return value
cases = [(f"rebalance {step:2d}, {'cap' if w is not None else 'equal'} weights", list(range(0, T, step)), w)
         for step in (21, 1) for w in (None, cap)]
floor_ms = N * T * 8 / 6.3e12 * 1e3
print(f"growth pass bytes floor: {N * T * 8 / 1e6:.0f} MB of prices once at 6.3 TB/s = {floor_ms:.3f} ms")
for name, days, w in cases:
    ms, out = timed(lambda: api.factor_portfolio(labels, price, Q, days, w, 0, FEE, C0))
    print(f"portfolio, {name}: {ms:8.3f} ms  (R = {len(days)}; {ms / floor_ms:5.1f} x the growth pass's floor)")
    if "--passes" in sys.argv:
        continue
    ms_loop, ref = timed(lambda: loop(days, w), reps=1)
    err = float(((out["value"] - ref).abs() / ref.abs()).max())
    print(f"    torch host loop: {ms_loop:10.1f} ms = {ms_loop / ms:7.1f} x; largest relative difference of the curves {err:.2e}")
if "--passes" not in sys.argv:
    ms_q, _ = timed(lambda: api.factor_quantiles(f, price, Q))
    print(f"Factor.quantile(Q = {Q}) on the same inputs: {ms_q:8.3f} ms")
