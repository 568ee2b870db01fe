"""BASELINE config 4: 10000 symbols x 5040 days, the weighted cross-sectional regression with industry dummies of D-32
(api.xsec_regress_wls / Factor.pure_factor_return) at K = 3 and 8, G = 1 (no codes) and 31 ([N] codes), with and without weights, with
and without the residual column, all on device-resident inputs.  Medians of 7 device-event times after a warm-up (the Python call
included).  In the same run: api.xsec_regress (D-17) at the same K, with the ratio to it next to the ratio of the bytes moved --
(K + 2 columns + 4-byte codes) x the passes over the cells (3 + the extra chunks of pass 1, which reads every column again) + the
residual store, against (K + 1) x 3 --, and the loop the call replaces: torch.linalg.lstsq, batched over a subset of days, on the
sqrt(w)-scaled [F | dummies] design of NaN-free inputs, scaled to all days (marked "scaled").  Then bit parity of coef / t / R^2 / n /
resid with the numpy restatement (tests/xsec_wls_ref.py) on sampled days.
--one: only two calls of the K = 8, G = 31 weighted case with the residual, for a kernel trace of the passes."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
N, T, G31 = 10000, 5040, 31
g = torch.Generator(device="cuda"); g.manual_seed(1)
F = torch.randn((8, N, T), dtype=torch.float64, device="cuda", generator=g)
ind = torch.randint(0, G31, (N,), device="cuda", generator=g, dtype=torch.int32)
r = 0.1 * F[0] - 0.05 * F[1] + 0.02 * ind[:, None] + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
w = torch.exp(0.5 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g))
clean_r = r.clone()
r[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
fs = [F[j] for j in range(8)]
if "--one" in sys.argv:
    for _ in range(2):
        api.xsec_regress_wls(fs, r, w, ind, resid=True)
    torch.cuda.synchronize()
    sys.exit(0)
def timed(fn, reps=7):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))
cells = N * T
def chunks(K, G):                      # launches of pass 1: ceil((K + 3) / clamp(128 / G, 1, K + 3))
    c = max(1, min(K + 3, 128 // G))
    return -(-(K + 3) // c)
base = {}
for K in (3, 8):
    base[K] = timed(lambda: api.xsec_regress(fs[:K], r))
    print(f"xsec_regress K={K}                         {base[K]:8.3f} ms  {(K + 1) * 3 * 8 * cells / base[K] / 1e6:7.0f} GB/s over its 3 passes")
for K in (3, 8):
    for G in (1, 31):
        for wt in (False, True):
            for res in (False, True):
                ms = timed(lambda: api.xsec_regress_wls(fs[:K], r, w if wt else None, ind if G > 1 else None, resid=res))
                passes = 2 + chunks(K, G)
                per_cell = (8 * (K + 1) + (8 if wt else 0)) * passes + (8 if res else 0)     # [N] codes: 4 B per symbol, negligible
                byte_ratio = per_cell / ((K + 1) * 3 * 8)
                print(f"wls K={K} G={G:2d} weights={int(wt)} resid={int(res)}   {ms:8.3f} ms  {per_cell * cells / ms / 1e6:7.0f} GB/s over "
                      f"{passes} passes  x{ms / base[K]:5.2f} of xsec_regress (bytes x{byte_ratio:4.2f})")
# the loop it replaces, on a subset of days
days = list(range(0, T, T // 8))[:8]
for K, G in ((3, 31), (8, 31)):
    dm = torch.nn.functional.one_hot(ind.long(), G).to(torch.float64)                        # [N, G]
    def loop(dev):
        sw = torch.sqrt(w[:, days].T.to(dev))[:, :, None]                                    # [D, N, 1]
        A = torch.cat([torch.stack([f[:, days].T for f in fs[:K]], dim=2).to(dev), dm.to(dev)[None].expand(len(days), N, G)], dim=2) * sw
        return torch.linalg.lstsq(A, clean_r[:, days].T.to(dev)[:, :, None] * sw).solution
    try:
        ms, where = timed(lambda: loop("cuda"), 3), "device"
    except Exception as e:                                                                    # no batched device lstsq in this build
        import time
        print(f"torch.linalg.lstsq on the device: {type(e).__name__}; timing the host's")
        t0 = time.perf_counter(); loop("cpu"); ms, where = (time.perf_counter() - t0) * 1e3, "host"
    print(f"torch.linalg.lstsq ({where}) K={K} G={G}: {ms:8.2f} ms for {len(days)} days -> {ms * T / len(days):10.1f} ms scaled to {T} days")
# parity on sampled days
import xsec_wls_ref as R
days = [0, 1, 1000, 2519, 2520, 4000, 5039]
ok = True
for K in (3, 8):
    got = api.xsec_regress_wls(fs[:K], r, w, ind, resid=True)
    exp = R.wls([f[:, days].cpu().numpy() for f in fs[:K]], r[:, days].cpu().numpy(), w[:, days].cpu().numpy(), ind.cpu().numpy(), G31)
    r2 = torch.stack([got["r_squared"], got["r_squared_within"]])
    for gk, e in ((got["coef"], "coef"), (got["t_stat"], "t"), (r2, "r2"), (got["resid"], "resid")):
        ok &= bool((gk[..., days].cpu().numpy().view(np.uint64) == exp[e].view(np.uint64)).all())
    ok &= bool((got["n"][days].cpu().numpy() == exp["n"]).all()) and bool((got["n_industries"][days].cpu().numpy() == exp["gt"]).all())
print(f"parity on {len(days)} sampled days (K = 3, 8; G = 31, weights, resid): {ok}")
