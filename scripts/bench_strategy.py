"""A Strategy in front of the backtest, two ways (README.md:862-994 -> VectorizedBacktester): the stochastic strategy -- STOCH, its %K / %D
cross (pq_cross_signals), the oversold / overbought zones (pq_gate_signals) -- followed by pq_backtest_vectorized over 5000 x 2520:
  eager   four C-ABI calls, one launch (or more) each
  suite   the same four calls recorded once (pq_suite_begin / end) and replayed: the signal columns stay on the device between the
          indicator job, the rule kernels and the wave-per-symbol backtest, and the launches are a recorded plan
Eager against recorded, column by column: the signal columns, position, cash, equity and summary columns 1, 5, 6, 7 (max_drawdown,
max_profit, win_rate, total_trades) are compared BIT FOR BIT ("exact_columns_identical"); summary columns 0, 2, 3, 4 (annualized
return, alpha, beta, sharpe: ordered sums) get their largest relative difference -- a recorded backtest runs the one-wave kernel, an
eager one the four-wave kernel, and the two add the daily returns in different orders (tests/test_strategy_rules_gpu.py).  The last
field repeats the comparison with the eager backtest forced to one wave (PQ_BT_WAVES=1): the same kernel on both sides.
Prints one JSON object (profiles/r07_bench_strategy.json)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, ".")
import torch

from polars_quant_amd import api
from polars_quant_amd._lib import Batch, BtParams, check, lib
from polars_quant_amd._spec import BT_DEFAULTS
from polars_quant_amd.synthetic import gen_ohlcv

N, T = 5000, 2520
PITCH = (T + 15) // 16 * 16
d = gen_ohlcv(0x5EED0002, N, T, 0)
dev = torch.device("cuda")
col = {}
for k in ("high", "low", "close"):
    buf = torch.zeros((N, PITCH), dtype=torch.float64, device=dev)
    buf[:, :T] = torch.from_numpy(d[k]).to(dev)
    col[k] = buf
f64 = lambda: torch.empty((N, PITCH), dtype=torch.float64, device=dev)
u8 = lambda: torch.zeros((N, PITCH), dtype=torch.uint8, device=dev)
k_, d_, b0, s0, b1, s1 = f64(), f64(), u8(), u8(), u8(), u8()
pos, cash, eq, summ = f64(), f64(), f64(), torch.empty((N, 8), dtype=torch.float64, device=dev)
L, h, b, prm = lib(), api.ctx(0), Batch(N, T, PITCH), BtParams(**BT_DEFAULTS)
P = lambda t: C.c_void_p(t.data_ptr())


def calls():
    check(L.pq_stoch(h, C.byref(b), P(col["high"]), P(col["low"]), P(col["close"]), 5, 3, 0, 3, 0, P(k_), P(d_)))
    check(L.pq_cross_signals(h, C.byref(b), P(k_), P(d_), P(b0), P(s0)))
    check(L.pq_gate_signals(h, C.byref(b), P(k_), None, 0, C.c_double(20.0), C.c_double(80.0), P(b0), P(s0), P(b1), P(s1)))
    check(L.pq_backtest_vectorized(h, C.byref(b), P(col["close"]), P(b1), P(s1), None, C.byref(prm), P(pos), P(cash), P(eq), P(summ)))


def t_event(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


SUMMARY_KEYS = ("annualized_return", "max_drawdown", "alpha", "beta", "sharpe_ratio", "max_profit", "win_rate", "total_trades")
EXACT, SUMS = (1, 5, 6, 7), (0, 2, 3, 4)
NAMED = (("slowk", k_), ("slowd", d_), ("cross_buy", b0), ("cross_sell", s0), ("buy", b1), ("sell", s1), ("position", pos), ("cash", cash), ("equity", eq))


def snapshot():
    torch.cuda.synchronize()
    return {nm: t[:, :T].clone() for nm, t in NAMED}, summ.clone()


def same_bits(a, r):
    return torch.equal(a.view(torch.int64), r.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, r)


def compare(ref, got):
    """-> (names of the columns that differ in some bit, exact columns identical, largest relative difference of the sum columns)"""
    differing = [nm for nm in ref[0] if not same_bits(got[0][nm], ref[0][nm])]
    differing += [f"summary.{SUMMARY_KEYS[k]}" for k in range(8) if not same_bits(got[1][:, k].contiguous(), ref[1][:, k].contiguous())]
    exact = not any(nm in differing for nm in list(ref[0]) + [f"summary.{SUMMARY_KEYS[k]}" for k in EXACT])
    a, r = got[1][:, list(SUMS)], ref[1][:, list(SUMS)]
    ok = torch.isfinite(a) & torch.isfinite(r) & (r != 0)
    rel = float(((a - r).abs() / r.abs())[ok].max()) if bool(ok.any()) else 0.0
    return differing, exact, rel


eager_ms = t_event(calls)
ref = snapshot()
os.environ["PQ_BT_WAVES"] = "1"          # the eager backtest as the one-wave kernel: what a recording runs
calls()
ref_one_wave = snapshot()
del os.environ["PQ_BT_WAVES"]
check(L.pq_suite_begin(h, C.byref(b)))
calls()
suite = C.c_void_p()
check(L.pq_suite_end(h, C.byref(suite)))
for _, t in NAMED:
    t.fill_(-1.0 if t.dtype == torch.float64 else 7)
summ.fill_(-1.0)
suite_ms = t_event(lambda: check(L.pq_suite_run(h, suite)))
got = snapshot()
check(L.pq_suite_destroy(h, suite))
differing, exact, rel = compare(ref, got)
differing1, _, _ = compare(ref_one_wave, got)
print(json.dumps({"workload": f"Strategy.stoch -> VectorizedBacktester, {N} x {T}", "eager_ms": eager_ms, "recorded_suite_ms": suite_ms,
                  "identical_results": not differing, "exact_columns_identical": exact, "differing_columns": differing,
                  "summary_sum_columns_max_rel_diff": rel, "identical_to_one_wave_eager": not differing1,
                  "differing_columns_one_wave_eager": differing1, "trades_total": float(summ[:, 7].sum())}, indent=1))
