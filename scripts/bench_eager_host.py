"""Host cost of an eager call: three wrappers of polars_quant_amd.api on a [4, 64] device tensor at the recommended row pitch, where the
launch and the kernel are negligible and the Python path (conversion, marshalling, ctypes) dominates.  Per case 300 warm-up calls, then
2 000 calls with one stream synchronise at the end; microseconds per call, with and without that synchronise.  Prints one JSON object.
Compare two trees by running the script from each in alternating fresh processes (EXPERIMENTS.md)."""
import sys; sys.path.insert(0, ".")
import json, time
import torch
from polars_quant_amd import api

g = torch.Generator().manual_seed(1)
x = (50.0 + torch.randn((4, 64), dtype=torch.float64, generator=g).cumsum(1)).cuda()
buy = (torch.rand((4, 64), generator=g) < 0.3).to(torch.uint8).cuda()
sell = (torch.rand((4, 64), generator=g) < 0.3).to(torch.uint8).cuda()
cases = {"call_sma": lambda: api.call("sma", x, timeperiod=30), "factor_rank": lambda: api.factor_rank(x),
         "backtest_vectorized": lambda: api.backtest_vectorized(x, buy, sell, want_curves=False)}
out = {}
for name, fn in cases.items():
    for _ in range(300): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2000): fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out[name + "_us"] = round((t2 - t0) / 2000 * 1e6, 2)
    out[name + "_enqueue_us"] = round((t1 - t0) / 2000 * 1e6, 2)
print(json.dumps(out))
