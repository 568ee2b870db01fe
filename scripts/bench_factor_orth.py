"""BASELINE config 4: 10000 symbols x 5040 days, multi-factor orthogonalization and neutralization of D-19 (Factor().clean(factors,
method)): orthogonalize and neutralize at K = 3 and K = 8, and orthogonalize K = 3 in place, on device-resident inputs, next to
fama_macbeth at the same K on the same inputs (D-17: the same passes with one more column read).  Device-event times after a warm-up
(the Python call included), the rate over the bytes floor (each input column read once, each residual column written once), and a
bit-parity check against the numpy restatement (tests/xsec_orth_ref.py) on sampled days."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from polars_quant_amd import Factor
import xsec_orth_ref as O
N, T = 10000, 5040
g = torch.Generator(device="cuda"); g.manual_seed(1)
F = torch.randn((8, N, T), dtype=torch.float64, device="cuda", generator=g)
for k in range(1, 8):
    F[k] += 0.3 * F[k - 1]                                                  # correlated factors
F[torch.rand((8, N, T), device="cuda", generator=g) < 0.01] = float("nan")
r = 0.1 * F[0] + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
X3 = F[:3].clone()                                                          # rewritten by the in-place case
fac = Factor()
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): out = fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, out
cells = N * T
# bytes floor (per call): each input column read once and each residual column written once (K + K - 1 columns, 8 B/cell).  The kernel
# reads the inputs in 3 passes, and out-of-place orthogonalize also copies factor 0 into row 0 of its result.
cases = [("orthogonalize K=3", 5, lambda: fac.clean(F[:3], method="orthogonalize")),
         ("orthogonalize K=3 in place", 5, lambda: fac.clean(X3, method="orthogonalize", inplace=True)),
         ("neutralize K=3", 5, lambda: fac.clean(F[:3], method="neutralize")),
         ("orthogonalize K=8", 15, lambda: fac.clean(F, method="orthogonalize")),
         ("neutralize K=8", 15, lambda: fac.clean(F, method="neutralize")),
         ("fama_macbeth K=3 (D-17)", 4, lambda: fac.fama_macbeth(F[:3], r)),
         ("fama_macbeth K=8 (D-17)", 9, lambda: fac.fama_macbeth(F, r))]
for name, ncols, fn in cases:
    ms, _ = timed(fn)
    print(f"{name:28s} {ms:8.3f} ms  {cells/ms/1e6:7.2f} G cells/s  {ncols*8*cells/ms/1e6:7.0f} GB/s over the bytes floor")
# parity on sampled days
days = [0, 1, 1000, 2519, 2520, 4000, 5039]
ok = True
for K in (3, 8):
    Fs = F[:K][:, :, days].cpu().numpy()
    for method in O.MODES:
        got = fac.clean(F[:K], method=method)[..., days].cpu().numpy()
        ok &= bool((got.view(np.uint64) == O.clean_full(Fs, method).view(np.uint64)).all())
X = F[:3].clone()
fac.clean(X, method="orthogonalize", inplace=True)
ok &= bool((X[..., days].cpu().numpy().view(np.uint64) == O.clean_full(F[:3][:, :, days].cpu().numpy()).view(np.uint64)).all())
print(f"parity on {len(days)} sampled days (K = 3, 8, both methods, and in place): {ok}")
