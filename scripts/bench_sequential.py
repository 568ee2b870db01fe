"""SequentialBacktester's engine (D-23, pq_backtest_sequential): T = 2520 periods, A = 500 assets, about 8 orders per period, replayed
as B = 1 / 256 / 2048 tapes in one launch.  Every tape has its own orders (a sweep over strategies); preallocated outputs, event-timed
mean of 10 launches after 3.  Prints ms per launch and orders matched per second.  One tape is ONE wavefront walking a serial chain:
its time is a latency, not a rate, and is reported as such.  Before timing, tape 0 is compared bit for bit with the restatement in
tests/seq_ref.py."""
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import ctypes as C
import numpy as np, torch
from polars_quant_amd import api
from polars_quant_amd._lib import SeqParams, check, lib
from polars_quant_amd._spec import SEQ_DEFAULTS
import seq_ref as R

T, A, PER = 2520, 500, 8
NB = (1, 256, 2048)
rng = np.random.default_rng(0x5E9)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def tapes(B):
    """B tapes of Poisson(PER) orders per period over random assets: 55 % buys, 45 % sells, 1 .. 49 shares each"""
    counts = rng.poisson(PER, (B, T))
    n = int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64)
    rows = np.stack([off[b * T:b * T + T + 1] for b in range(B)])
    asset = rng.integers(0, A, n).astype(np.int32)
    qty = rng.integers(1, 50, n).astype(np.float64) * np.where(rng.random(n) < 0.55, 1.0, -1.0)
    price = rng.uniform(5.0, 60.0, A)[asset] * (1.0 + 0.05 * rng.standard_normal(n)).clip(0.5)
    return rows, asset, qty, price


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


vp = lambda t: C.c_void_p(t.data_ptr())
prm, h = SeqParams(**SEQ_DEFAULTS), api.ctx(0)
bench = torch.from_numpy(3000.0 * np.cumprod(1.0 + 0.01 * rng.standard_normal(T))).cuda()
for B in NB:
    rows, asset, qty, price = tapes(B)
    d = [torch.from_numpy(x).cuda() for x in (rows, asset, qty, price)]
    out = api.backtest_sequential(*d, A, bench)
    torch.cuda.synchronize()
    ref = R.run_lanes(rows[0], asset, qty, price, A)
    assert (out["equity"][0].cpu().numpy().view(np.uint64) == ref["equity"].view(np.uint64)).all(), "tape 0 differs from the restatement"
    n = len(asset)
    ms = timed(lambda: check(lib().pq_backtest_sequential(h, B, T, A, *[vp(t) for t in d], n, vp(bench), C.byref(prm), 1, vp(out["equity"]),
                                                          vp(out["cash"]), vp(out["position"]), vp(out["counts"]), vp(out["summary"]))))
    kind = "latency of one wavefront" if B == 1 else "throughput"
    print(f"B = {B:5d} tapes ({n} orders, tape 0: {ref['trades']} buys filled, {ref['outcomes']['sell_filled']} sells filled): "
          f"{ms:.3f} ms per launch, {n / ms / 1e3:.2f} M orders/s ({kind})")
