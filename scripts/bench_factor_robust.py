"""BASELINE config 4: 10000 symbols x 5040 days, the robustness tests of D-18 against the host loops they replace, on device-resident
inputs: ic_decay (max_lag = 10) vs a loop of Factor.ic / rank_ic on shifted views, subgroup_test (31 groups) vs a loop of Factor.ic /
rank_ic on the masked factor, and subsample_test (n_splits = 3) vs Factor.ic plus one summary per period.  Device-event times after a
warm-up (the Python call included), and bit parity of the fused rows against the loop's rows on sampled lags / groups."""
import sys; sys.path.insert(0, ".")
import torch
from polars_quant_amd import Factor, api
N, T, L, G, P = 10000, 5040, 10, 31, 3
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r = 0.05 * f + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
r[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
code = torch.randint(0, G, (N,), device="cuda", generator=g, dtype=torch.int32)
code[code == 3] = -1                                                   # one group unclassified
fac = Factor()
NAN = torch.tensor(float("nan"), dtype=torch.float64, device="cuda")


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def bits(x):
    return x.contiguous().view(torch.int64)


ok = True
for method in ("pearson", "spearman"):
    ic1 = fac.ic if method == "pearson" else fac.rank_ic
    ms_f, out = timed(lambda: fac.ic_decay(f, r, max_lag=L, method=method))
    ms_l, loop = timed(lambda: [ic1(f[:, :T - l + 1], r[:, l - 1:]) for l in range(1, L + 1)])
    print(f"ic_decay L={L} {method:9s} fused {ms_f:8.3f} ms   loop {ms_l:8.3f} ms   x{ms_l / ms_f:5.2f}")
    for l in (1, 2, 5, 10):
        ok &= bool(torch.equal(bits(out["daily"]["ic"][l - 1, :T - l + 1]), bits(loop[l - 1][0])))
        ok &= bool(torch.equal(out["daily"]["n_valid"][l - 1, :T - l + 1], loop[l - 1][1]))
    ms_f, out = timed(lambda: fac.subgroup_test(f, r, code, method=method))
    ms_l, loop = timed(lambda: [ic1(torch.where(code[:, None] == k, f, NAN), r) for k in range(G)])
    print(f"subgroup G={G} {method:9s} fused {ms_f:8.3f} ms   loop {ms_l:8.3f} ms   x{ms_l / ms_f:5.2f}")
    for k in (0, 3, 17, G - 1):
        ok &= bool(torch.equal(bits(out["daily"]["ic"][k]), bits(loop[k][0])))
        ok &= bool(torch.equal(out["daily"]["n_valid"][k], loop[k][1]))
    start, end = api.split_periods(T, P)

    def sub_loop():
        ic, _ = ic1(f, r)
        return [api.series_split_summary(ic[a:b + 1], 1) for a, b in zip(start.tolist(), end.tolist())]
    ms_f, out = timed(lambda: fac.subsample_test(f, r, n_splits=P, method=method))
    ms_l, loop = timed(sub_loop)
    print(f"subsample P={P} {method:9s} fused {ms_f:8.3f} ms   loop {ms_l:8.3f} ms   x{ms_l / ms_f:5.2f}")
    for p in range(P):
        ok &= bool(torch.equal(bits(out["mean_ic"][p]), bits(loop[p][0, 1])))
print(f"bit parity of the fused rows against the loops on sampled lags / groups / periods: {ok}")
