"""Solo replay time of the cdl_all task at 5000 x 2520 (run on the GPU box; scripts/exp_solo.py covers the SEQ tasks only).
PQ_LIB_PATH selects an A/B library."""
import sys; sys.path.insert(0, ".")
import torch
from polars_quant_amd.suite import Suite
from oracle import pq_oracle as oracle
N, T = 5000, 2520
d = oracle.gen_ohlcv(0x5EED0002, N, T, 0)
st = Suite(N, T, "cuda")
g = {}
for k, v in d.items():
    buf = torch.zeros((N, st.stride), dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(v).cuda()
    g[k] = buf[:, :T]
st.record(g, ["cdl_all"])
for _ in range(3): st.run()
torch.cuda.synchronize()
ts = []
for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): st.run()
    e1.record(); e1.synchronize()
    ts.append(e0.elapsed_time(e1) / 10)
print("cdl_all solo ms per replay:", " ".join(f"{t:.4f}" for t in ts), "min", f"{min(ts):.4f}")
