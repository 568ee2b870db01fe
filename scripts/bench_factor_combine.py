"""BASELINE config 4: 10000 symbols x 5040 days, the composite of K factors under per-day weights (D-30: api.factor_combine) and the
weights from the factors' IC series (api.factor_combine_weights: ic / icir / max_icir at windows 20 / 60 / 252), on device-resident
columns.  usage: bench_factor_combine.py [K ...] (default 2 3 8; one K per process keeps each GPU step under a time limit of its own).
Every case is called REPS times after a warm-up, each call between its own pair of device events (the Python call included); the
minimum and the median are printed.  In the same process, per K:
  * the traffic floor: a device-to-device copy that moves what the combine kernel moves, (K + 1) N T 8 bytes in all -- (K + 1) N T / 2
    doubles read and as many written;
  * the torch expression a user would write: stack, validity mask, weighted sum, divide.
Bit parity with the numpy restatement (tests/xsec_combine_ref.py) on a sample of symbols, and of every weights case."""
import statistics
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import api
import xsec_combine_ref as R
N, T, REPS = 10000, 5040, 7
KS = [int(a) for a in sys.argv[1:]] or [2, 3, 8]
WINDOWS = (20, 60, 252)
g = torch.Generator(device="cuda"); g.manual_seed(1)
def column():
    x = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
    x[torch.rand((N, T), device="cuda", generator=g) < 0.001] = float("nan")
    return x
def timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return min(ms), statistics.median(ms)
def torch_combine(fs, w):
    F = torch.stack(fs)                                 # [K, N, T]
    ok = torch.isfinite(F).all(0)                       # NULL is a NaN
    acc = (w[:, None, :] * F).sum(0)
    return torch.where(ok, acc / w.abs().sum(0), torch.full_like(acc, float("nan")))
rows = [0, 1, 15, 16, 777, 4999, 5000, 9999]
for K in KS:
    fs = [column() for _ in range(K)]
    ic = 0.03 + 0.05 * torch.randn((K, T), dtype=torch.float64, device="cuda", generator=g)
    w = api.factor_combine_weights(ic, api.COMBINE_METHODS["icir"], 60, 1)
    traffic = (K + 1) * N * T * 8
    src = torch.randn(traffic // 16, dtype=torch.float64, device="cuda", generator=g)
    dst = torch.empty_like(src)
    res = {}
    cases = [("copy of the combine's traffic", lambda: dst.copy_(src)),
             ("factor_combine normalize", lambda: api.factor_combine(fs, w, True)),
             ("factor_combine plain sum", lambda: api.factor_combine(fs, w, False)),
             ("torch stack / mask / sum / divide", lambda: torch_combine(fs, w))]
    for name, fn in cases:
        lo, med = res[name] = timed(fn)
        print(f"K={K} {name:36s} min {lo:8.3f} ms  median {med:8.3f} ms  {traffic/med/1e6:7.0f} GB/s of (K + 1) N T 8 bytes (median)", flush=True)
    copy, comb, tor = (res[n][1] for n in ("copy of the combine's traffic", "factor_combine normalize", "torch stack / mask / sum / divide"))
    print(f"K={K} factor_combine reaches {100.0 * copy / comb:.1f} % of the copy's bandwidth; the torch expression takes {tor / comb:.1f}x its time")
    for method, code in api.COMBINE_METHODS.items():
        for win in WINDOWS:
            if win < api.combine_min_window(code, K):
                continue
            lo, med = timed(lambda: api.factor_combine_weights(ic, code, win, 1))
            got = api.factor_combine_weights(ic, code, win, 1).cpu().numpy()
            same = not bool((got.view(np.uint64) != R.weights(ic.cpu().numpy(), method, win, 1).view(np.uint64)).any())
            print(f"K={K} factor_combine_weights {method:8s} window {win:3d}  min {lo:8.3f} ms  median {med:8.3f} ms  parity {same}", flush=True)
    wn = w.cpu().numpy()
    Fs = np.stack([f[rows].cpu().numpy() for f in fs])
    ok = True
    for normalize in (True, False):
        got = api.factor_combine(fs, w, normalize)[rows].cpu().numpy()
        ok &= not bool((got.view(np.uint64) != R.composite(Fs, wn, normalize).view(np.uint64)).any())
    print(f"K={K} parity of the composite on {len(rows)} sampled symbols (both normalize values): {ok}", flush=True)
    del fs, src, dst
    torch.cuda.empty_cache()
