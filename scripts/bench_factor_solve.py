"""BASELINE config 4: 10000 symbols x 5040 days, portfolio construction from the risk model (D-34) on device-resident inputs:
api.risk_solve at K = 8, G = 31 (M = 39) with R = 1 (ones) and R = 2 (ones, alpha), on the 252 rebalance days of step 20 and on every
day from the first full window, on a model that is risk_factor_cov's and risk_specific_var's own output (w = 252, half-life 90).
Medians of 7 device-event times after a warm-up (the Python call included), with the bytes that must move -- (K + R + 2) N D 8 in
(exposures, right-hand sides, the variance, the codes counted as a column), R N D 8 out -- and the fraction of 6.3 TB/s they reach.
In the same run, for the loop the call replaces: a batched torch Woodbury over the 252 days (B gathered per day, bmm, one batched
linalg.solve; scaled to every day), and the dense torch.linalg.solve of Sigma = B F B' + diag(s^2) on three sampled days, scaled.
Then bit parity with the numpy restatement (tests/xsec_solve_ref.py) on three days, and Factor.optimal_portfolio's three objectives.
--one R STEP: only two calls of risk_solve at that R and step, for a kernel trace (the split between the passes)."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import polars_quant_amd as pq
from polars_quant_amd import api
N, T, W, HL, K, G = 10000, 5040, 252, 90.0, 8, 31
M = K + G
g = torch.Generator(device="cuda"); g.manual_seed(1)
rnd = lambda *s: torch.randn(s, dtype=torch.float64, device="cuda", generator=g)   # noqa: E731
om = api.risk_weights(W, HL)
resid, f = 0.02 * rnd(N, T), 0.01 * rnd(M, T)
expo = [rnd(N, T) for _ in range(K)]
alpha = 0.001 * rnd(N, T)
ind = torch.randint(0, G, (N,), device="cuda", generator=g, dtype=torch.int32)
STEPS = ((20, 19), (1, W - 1))                      # (step, day0): the 252 days 19, 39, ...; 4789 days from the first full window
models = {}
for step, day0 in STEPS:
    models[step] = (api.risk_factor_cov(f, om, 20, day0=day0, step=step), api.risk_specific_var(resid, om, 20, day0=day0, step=step), day0)
del resid
def timed(fn, reps=7):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))
def rhs_of(R):
    return [None, alpha][:R]
if "--one" in sys.argv:
    R, step = int(sys.argv[sys.argv.index("--one") + 1]), int(sys.argv[sys.argv.index("--one") + 2])
    cov, sv, day0 = models[step]
    for _ in range(2):
        api.risk_solve(rhs_of(R), expo, cov, sv, ind, day0, step)
    torch.cuda.synchronize()
    sys.exit(0)
for step, day0 in STEPS:
    cov, sv, _ = models[step]
    D = cov.shape[0]
    for R in (1, 2):
        ms = timed(lambda: api.risk_solve(rhs_of(R), expo, cov, sv, ind, day0, step))
        b_in, b_out = (K + R + 2) * N * D * 8, R * N * D * 8
        print(f"risk_solve K={K} G={G} R={R} step={step:2d} D={D:4d}   {ms:9.3f} ms   in {b_in / 1e6:8.1f} MB out {b_out / 1e6:7.1f} MB "
              f"-> {(b_in + b_out) / ms / 1e9:6.3f} TB/s = {(b_in + b_out) / ms / 1e9 / 6.3 * 100:5.1f} % of 6.3 TB/s")
# the batched torch Woodbury on the 252 days
step, day0 = STEPS[0]
cov, sv, _ = models[step]
D = cov.shape[0]
days = day0 + step * torch.arange(D, device="cuda")
onehot = torch.nn.functional.one_hot(ind.long(), G).to(torch.float64)
def woodbury(R):
    B = torch.cat([torch.stack([x[:, days] for x in expo], dim=2), onehot[:, None, :].expand(N, D, G)], dim=2).permute(1, 0, 2)   # [D, N, M]
    v = torch.stack([torch.ones((N, D), dtype=torch.float64, device="cuda"), alpha[:, days]][:R], dim=2).permute(1, 0, 2)          # [D, N, R]
    q = (1.0 / sv).T[:, :, None]                                                                                                  # [D, N, 1]
    Bq = B * q
    A, p = Bq.transpose(1, 2) @ B, Bq.transpose(1, 2) @ v
    u = torch.linalg.solve(torch.eye(M, dtype=torch.float64, device="cuda") + cov @ A, cov @ p)
    return q * (v - B @ u)
for R in (1, 2):
    ms = timed(lambda: woodbury(R), 3)
    D1 = models[1][0].shape[0]
    print(f"torch batched Woodbury R={R} D={D}: {ms:9.2f} ms -> {ms * D1 / D:10.1f} ms scaled to the {D1} days of step 1")
yw = woodbury(2).permute(2, 1, 0)
y, quad, n = api.risk_solve(rhs_of(2), expo, cov, sv, ind, day0, step)
print(f"risk_solve against the torch Woodbury: worst deviation {float(((y - yw).abs().amax(dim=1) / yw.abs().amax(dim=1)).max()):.3g} of max|y| per day")
del yw
# the dense solve on three sampled days
sample = [0, D // 2, D - 1]
def dense(d, R):
    B = torch.cat([torch.stack([x[:, days[d]] for x in expo], dim=1), onehot], dim=1)
    Sigma = B @ cov[d] @ B.T + torch.diag(sv[:, d])
    v = torch.stack([torch.ones(N, dtype=torch.float64, device="cuda"), alpha[:, days[d]]][:R], dim=1)
    return torch.linalg.solve(Sigma, v)
for R in (1, 2):
    ms = timed(lambda: [dense(d, R) for d in sample], 3)
    for st, _ in STEPS:
        Dn = models[st][0].shape[0]
        print(f"torch dense linalg.solve R={R}: {ms:9.2f} ms for {len(sample)} days -> {ms * Dn / len(sample):12.1f} ms scaled to the {Dn} days of step {st}")
yd = dense(sample[1], 2)
print(f"risk_solve against the dense solve on day {sample[1]}: worst deviation "
      f"{float(((y[:, :, sample[1]].T - yd).abs().amax(dim=0) / yd.abs().amax(dim=0)).max()):.3g} of max|y|")
# parity on three days, and the Factor method
import xsec_solve_ref as S
di = torch.tensor(sample, device="cuda")
at = lambda x: x[:, days[di]].cpu().numpy()   # noqa: E731  (the three days as a panel of their own)
exp = S.solve([None, at(alpha)], [at(x) for x in expo], cov[di].cpu().numpy(), sv[:, di].cpu().numpy(), np.arange(len(sample)),
              ind.cpu().numpy(), G)
dd = di
bits = lambda a: np.ascontiguousarray(a).view(np.uint64)   # noqa: E731
ok = bool((bits(y[:, :, dd].cpu().numpy()) == bits(exp["y"])).all() and (bits(quad[:, :, dd].cpu().numpy()) == bits(exp["quad"])).all()
          and (n[:, dd].cpu().numpy() == exp["n"]).all())
print(f"parity with the restatement on the days {sample} (y, quad, n): {ok}")
model = {"factor_cov": cov, "specific_var": sv, "day0": day0, "step": step}
for obj in ("min_variance", "max_sharpe", "mean_variance"):
    ms = timed(lambda: pq.Factor().optimal_portfolio(expo, model, alpha, ind, obj, 5.0))
    print(f"Factor.optimal_portfolio {obj:13s} D={D}: {ms:9.3f} ms")
