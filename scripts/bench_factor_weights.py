"""D-35's measurements: 5 000 symbols x 5 040 days, a rebalance every 20 days (R = 252), fee 0.001, clean
random-walk prices, long-short weights with a gross of 1.5.
  (a) api.factor_weights at P = 1 against api.factor_portfolio with one group and equal weights on the same prices and days
  (b) P = 8 in one call against eight P = 1 calls
  (d) the call with and without holdings_of (the holdings pass alone is the difference; the kernel trace has it exactly)
Every call sits between its own device events, the Python call included; medians of 9 calls after a warm-up, the variants alternating,
and the whole comparison three times over, so that the spread between rounds can be read beside each difference.
`--passes` runs the weights calls alone, for a kernel trace of the passes (the pw_* kernels; (c) is pw_growth_partial_kernel's time
against the bytes printed here).  `--tree PATH` imports the package from another checkout and times api.factor_portfolio alone: the
yardstick of (a) on the parent commit."""
import statistics
import sys

tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else "."
sys.path.insert(0, tree)
import torch  # noqa: E402
from polars_quant_amd import api  # noqa: E402

N, T, STEP, FEE, C0 = 5000, 5040, 20, 0.001, 1_000_000.0
days = list(range(0, T, STEP))
R = len(days)
g = torch.Generator(device="cuda"); g.manual_seed(1)
price = 20.0 * torch.exp(torch.cumsum(0.02 * torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g), dim=1))
labels = torch.zeros((N, T), dtype=torch.uint8, device="cuda")


def weights(P):
    w = torch.randn((P, N, R), dtype=torch.float64, device="cuda", generator=g)
    return w * (1.5 / w.abs().sum(dim=1, keepdim=True))


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def rounds(variants, reps=9, n_rounds=3):
    """{name: fn} -> prints per round the median ms of each variant, the calls of the variants alternating"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for r in range(n_rounds):
        ms = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                ms[k].append(once(fn))
        print("    round %d: " % r + "; ".join(f"{k} {statistics.median(v):7.3f} ms (min {min(v):.3f})" for k, v in ms.items()))


def portfolio():
    return api.factor_portfolio(labels, price, 1, days, None, 0, FEE, C0)


if "--tree" in sys.argv:
    print(f"yardstick: api.factor_portfolio of the tree {tree}, one group, equal weights, N = {N}, T = {T}, R = {R}")
    rounds({"factor_portfolio": portfolio})
    sys.exit(0)

w1, w8 = weights(1), weights(8)
plane, partials = N * T * 8, ((N + 255) // 256) * T * 8
print(f"N = {N}, T = {T}, R = {R}; growth pass lower bound: the price plane once {plane / 1e6:.1f} MB + the partials "
      f"{partials / 1e6:.2f} MB per portfolio = {(plane + partials) / 6.3e12 * 1e3:.4f} ms at 6.3 TB/s (P = 1), "
      f"{(plane + 8 * partials) / 6.3e12 * 1e3:.4f} ms (P = 8); holdings pass: {2 * plane / 1e6:.1f} MB = {2 * plane / 6.3e12 * 1e3:.4f} ms")
if "--passes" in sys.argv:
    for _ in range(3):
        api.factor_weights(w1[0], price, days, FEE, C0)
        api.factor_weights(w8, price, days, FEE, C0)
        api.factor_weights(w8, price, days, FEE, C0, holdings_of=0)
    torch.cuda.synchronize()
    sys.exit(0)
print("(a) P = 1 against pq_factor_portfolio with one group:")
rounds({"factor_weights P=1": lambda: api.factor_weights(w1[0], price, days, FEE, C0), "factor_portfolio G=1": portfolio})
print("(b) P = 8 in one call against eight P = 1 calls:")
rounds({"one call P=8": lambda: api.factor_weights(w8, price, days, FEE, C0),
        "eight calls P=1": lambda: [api.factor_weights(w8[p], price, days, FEE, C0) for p in range(8)]})
print("(d) with and without the holdings pass:")
rounds({"P=1": lambda: api.factor_weights(w1[0], price, days, FEE, C0),
        "P=1 + holdings": lambda: api.factor_weights(w1[0], price, days, FEE, C0, holdings_of=0),
        "P=8": lambda: api.factor_weights(w8, price, days, FEE, C0),
        "P=8 + holdings": lambda: api.factor_weights(w8, price, days, FEE, C0, holdings_of=7)})
one = api.factor_weights(w8, price, days, FEE, C0)
sep = torch.cat([api.factor_weights(w8[p], price, days, FEE, C0)["value"] for p in range(8)])
print("P = 8 in one call and eight calls agree bit for bit:", bool((one["value"].view(torch.int64) == sep.view(torch.int64)).all()),
      "; first_nonpositive:", one["first_nonpositive"].tolist())
