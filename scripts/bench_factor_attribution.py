"""D-36's measurements: 10 000 symbols x 5 040 days, K = 8 exposures, G = 31 industries ([N] codes), random
holdings, exposures and returns with 1 % NULL cells; api.return_attribution with one book (P = 1) and with a benchmark (P = 3) against
  (a) api.risk_portfolio at step = 1 on the same holdings, exposures and codes: it reads h, the K exposures and the codes in the same
      lane shape (and a specific variance in place of the specific return), so it is the yardstick of the pass
  (b) the torch loop that the call replaces: K + 3 masked nansums over the planes and an index_add_ by industry, for one book
Every call sits between its own device events, the Python call included; medians of 9 calls after a warm-up, the variants alternating,
and the whole comparison three times over, so that the spread between rounds can be read beside each difference.  The bytes that must
move are (the books' planes + K + u + r) N T 8 B plus the codes.  `--passes` runs the attribution calls alone, for a kernel trace."""
import statistics
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402
from polars_quant_amd import api  # noqa: E402

N, T, K, G = 10_000, 5040, 8, 31
g = torch.Generator(device="cuda"); g.manual_seed(36)
f64 = dict(dtype=torch.float64, device="cuda")
NULL = torch.from_numpy(api.np.full(1, api.NULL)).cuda()[0]


def plane(scale, holes=0.01):
    x = scale * torch.randn((N, T), generator=g, **f64)
    return torch.where(torch.rand((N, T), generator=g, device="cuda") < holes, NULL, x)


h, b = plane(1.0 / N), plane(1.0 / N).abs()
xs = [plane(1.0) for _ in range(K)]
u, r = plane(0.02), plane(0.03)
codes = torch.randint(0, G, (N,), generator=g, device="cuda")
fr = 0.01 * torch.randn((K + G, T), generator=g, **f64)
cov = torch.eye(K + G, **f64).expand(T, K + G, K + G).contiguous()
sv = u.abs()


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def rounds(variants, nbytes, reps=9, n_rounds=3):
    """{name: fn} -> prints per round the median ms of each variant (and TB/s where nbytes names it), the calls alternating"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for rnd in range(n_rounds):
        ms = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                ms[k].append(once(fn))
        print("    round %d: " % rnd + "; ".join(
            f"{k} {statistics.median(v):8.3f} ms (min {min(v):.3f}" + (f", {nbytes[k] / statistics.median(v) / 1e9:.2f} TB/s" if k in nbytes else "") + ")"
            for k, v in ms.items()))


def attribution(P):
    return api.return_attribution(h, xs, fr, u, codes, next_return=r, benchmark=b if P == 3 else None)


def torch_loop():
    """one book: K + 3 masked nansums and an index_add_ by industry"""
    covered = torch.isfinite(u)
    for x in xs:
        covered &= torch.isfinite(x)
    held = torch.isfinite(h)
    hm = torch.where(held & covered, h, 0.0)
    out = [(hm * x).nansum(dim=0) for x in xs]
    out.append((hm * u).nansum(dim=0))
    out.append((torch.where(held & ~covered, h, 0.0) * r).nansum(dim=0))
    out.append((torch.where(held, h, 0.0) * r).nansum(dim=0))
    out.append(torch.zeros((G, T), **f64).index_add_(0, codes, hm))
    return out


pb = N * T * 8
nbytes = {"attribution P=1": (1 + K + 2) * pb + N * 4, "attribution P=3": (2 + K + 2) * pb + N * 4, "risk_portfolio step=1": (1 + K + 1) * pb + N * 4}
print(f"N = {N}, T = {T}, K = {K}, G = {G}; bytes that must move: P = 1 {nbytes['attribution P=1'] / 1e9:.2f} GB, "
      f"P = 3 {nbytes['attribution P=3'] / 1e9:.2f} GB, risk_portfolio {nbytes['risk_portfolio step=1'] / 1e9:.2f} GB")
if "--passes" in sys.argv:
    for _ in range(3):
        attribution(1)
        attribution(3)
    torch.cuda.synchronize()
    sys.exit(0)
print("(a) against api.risk_portfolio at step = 1 on the same planes:")
rounds({"attribution P=1": lambda: attribution(1), "attribution P=3": lambda: attribution(3),
        "risk_portfolio step=1": lambda: api.risk_portfolio(h, xs, cov, sv, codes)}, nbytes)
print("(b) against the torch loop that the call replaces (one book):")
rounds({"attribution P=1": lambda: attribution(1), "torch loop": torch_loop}, nbytes, reps=5, n_rounds=2)
