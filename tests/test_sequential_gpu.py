"""-m gpu: pq_backtest_sequential (decision D-23, csrc/seq/sequential.hip) against the restatements of tests/seq_ref.py.

equity, cash, position, trades and wins are compared with run_lanes bit for bit on the uint64 view.  The summary is compared with the
oracle's calculate_summary of the GPU's own equity row (rtol 1e-12, atol 1e-13: the rule of tests/test_gpu_parity.py); the worst error
is printed before it is asserted.  In every randomised case with at least 100 orders the restatement must first show each of the four
outcomes (buy filled / rejected, sell filled / rejected) at least 8 times."""
import numpy as np
import pytest

import seq_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EXACT = dict(buy_commission_rate=2.0 ** -12, sell_commission_rate=2.0 ** -12, buy_slippage=1 / 64, sell_slippage=3 / 64)
WAVES = 4                                   # tapes per workgroup while 4 * 24 * A <= 64 KiB (A <= 682)


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from polars_quant_amd import api
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(name, got, exp):
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.argwhere(bits(got) != bits(exp))
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def pack(tapes):
    """tapes with their own offsets -> one order array and absolute offsets [B, T + 1]"""
    offs, base = [], 0
    for off, a, _, _ in tapes:
        offs.append(off + base)
        base += len(a)
    cat = lambda k, dt: np.concatenate([t[k] for t in tapes]).astype(dt)
    return np.stack(offs), cat(1, np.int32), cat(2, np.float64), cat(3, np.float64)


def launch(api, off, a, q, p, A, bench=None, params=None):
    r = api.backtest_sequential(off, a, q, p, A, bench, params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def covered(name, ref, n_orders):
    if n_orders >= 100:
        assert all(v >= 8 for v in ref["outcomes"].values()), (name, ref["outcomes"])


def check(api, oracle, name, tapes, A, params=None, bench=None, literal=None):
    """every tape against run_lanes; literal = "exact": equity also equals run_literal bitwise; "bound": within D-23's bound"""
    B = len(tapes)
    plist = [params or {}] * B if not isinstance(params, list) else params
    got = launch(api, *pack(tapes), A, bench, plist if isinstance(params, list) else params)
    worst = 0.0
    for b, tape in enumerate(tapes):
        prm = {**R.DEFAULTS, **plist[b]}
        ref = R.run_lanes(*tape, A, prm)
        covered(f"{name}[{b}]", ref, len(tape[1]))
        same(f"{name}[{b}] equity", got["equity"][b], ref["equity"])
        same(f"{name}[{b}] cash", got["cash"][b], ref["cash"])
        same(f"{name}[{b}] position", got["position"][b], ref["position"])
        assert (int(got["counts"][b, 0]), int(got["counts"][b, 1])) == (ref["trades"], ref["wins"]), (name, b)
        exp = oracle.summary(got["equity"][b], bench, prm["initial_capital"], ref["trades"], ref["wins"])
        err = np.abs(got["summary"][b] - exp) / (1e-13 + 1e-12 * np.abs(exp))
        worst = max(worst, float(err.max()))
        if literal:
            lit = R.run_literal(*tape, A, prm)
            same(f"{name}[{b}] cash (literal)", got["cash"][b], lit["cash"])
            same(f"{name}[{b}] position (literal)", got["position"][b], lit["position"])
            assert (ref["trades"], ref["wins"]) == (lit["trades"], lit["wins"])
            if literal == "exact":
                same(f"{name}[{b}] equity (literal)", got["equity"][b], lit["equity"])
            else:
                V = np.abs(ref["equity"] - ref["cash"])
                bound = 2.0 * A * 2.0 ** -53 * (np.abs(ref["cash"]) + V)
                diff = np.abs(got["equity"][b] - lit["equity"])
                print(f"{name}[{b}]: worst |gpu - literal| {diff.max():.3e}, bound there {bound[diff.argmax()]:.3e}")
                assert (diff <= bound).all(), (name, b, diff.max())
    print(f"{name}: worst summary error {worst:.3e} of the tolerance (rtol 1e-12, atol 1e-13)")
    assert worst <= 1.0, (name, worst)
    return got


def bench_series(T, seed=7):
    rng = np.random.default_rng(seed)
    return 3000.0 * np.cumprod(1.0 + 0.01 * rng.standard_normal(T))


@pytest.mark.parametrize("name", sorted(R.KATS))
def test_known_answers(api, name):
    """the hand-derived numbers of tests/seq_ref.py, on the device"""
    periods, A, prm, exp = R.KATS[name]
    got = launch(api, *R.tape_of(periods), A, None, prm)
    for k in ("equity", "cash", "position"):
        same(f"{name} {k}", got[k][0], exp[k])
    assert got["counts"][0].tolist() == [exp["trades"], exp["wins"]]


@pytest.mark.parametrize("A", [1, 63, 64, 65, 130])
def test_asset_counts(api, oracle, A):
    """partials of 1 to 3 terms and the fold; with and without a benchmark"""
    T = 65
    tape = R.random_tape(300 + A, T, A, 8)
    check(api, oracle, f"A={A}", [tape], A, literal="bound")
    check(api, oracle, f"A={A} benchmark", [tape], A, bench=bench_series(T))


def test_orders_per_period(api, oracle):
    """0, 1, 64, 65 and 130 orders in the periods of one tape: the 64-order chunk, its edge, and a chunk that starts mid-period"""
    counts = [0, 1, 64, 65, 130, 0, 0, 130, 1, 65, 64, 1, 0]
    tape = R.random_tape(41, len(counts), 65, counts)
    check(api, oracle, "orders per period", [tape], 65, literal="bound")


def test_tape_without_orders(api, oracle):
    T = 70
    none = (np.zeros(T + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    got = check(api, oracle, "no orders", [none], 5, bench=bench_series(T))
    assert (got["equity"] == 100000.0).all() and got["counts"].tolist() == [[0, 0]]
    # an empty tape beside a busy one, sharing a workgroup
    check(api, oracle, "no orders + busy", [none, R.random_tape(42, T, 5, 8)], 5)


@pytest.mark.parametrize("T", [1, 2, 64, 65, 130])
def test_period_counts(api, oracle, T):
    """the 64-period store buffer and its tail"""
    check(api, oracle, f"T={T}", [R.random_tape(500 + T, T, 7, 8)], 7, bench=bench_series(T) if T > 2 else None)


@pytest.mark.parametrize("B", [1, WAVES, WAVES + 1])
def test_tapes_per_workgroup(api, oracle, B):
    """tapes of very different order counts in one workgroup (a barrier in the walk would hang or corrupt) and an idle tail wave"""
    T, A = 66, 65
    means = [0.2, 24, 2, 8, 40]
    tapes = [R.random_tape(600 + b, T, A, means[b]) for b in range(B)]
    check(api, oracle, f"B={B}", tapes, A, bench=bench_series(T))


def test_one_tape_per_workgroup_above_the_plain_lds_size(api, oracle):
    """A = 2100: 50 400 B a tape, no two fit 64 KiB, so each of the 3 tapes takes a workgroup of its own"""
    T, A = 40, 2100
    tapes = [R.random_tape(700 + b, T, A, 12) for b in range(3)]
    check(api, oracle, "A=2100", tapes, A, literal="bound")


def test_too_many_assets_is_an_argument_error(api):
    from polars_quant_amd import PqError
    T, A = 3, 6145
    tape = R.tape_of([[(0, 1.0, 10.0)], [], [(6144, 1.0, 10.0)]])
    dev = torch.device("cuda")
    out = dict(equity=torch.full((1, T), -7.0, dtype=torch.float64, device=dev), cash=torch.full((1, T), -7.0, dtype=torch.float64, device=dev),
               position=torch.full((1, A), -7.0, dtype=torch.float64, device=dev), counts=torch.full((1, 2), -7, dtype=torch.int64, device=dev),
               summary=torch.full((1, 8), -7.0, dtype=torch.float64, device=dev))
    with pytest.raises(PqError, match="n_assets"):
        api.backtest_sequential(*tape, A, out=out)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out.values())
    # the cap itself is served: one wave with 147 456 B of LDS
    A = 6144
    got = launch(api, *tape, A)
    ref = R.run_lanes(*tape, A)
    same("A=6144 equity", got["equity"][0], ref["equity"])
    same("A=6144 position", got["position"][0], ref["position"])


def test_two_tapes_share_one_order_array(api, oracle):
    """one tape under two parameter sets: both rows of period_offsets point at the same orders"""
    T, A = 65, 9
    off, a, q, p = R.random_tape(43, T, A, 8)
    plist = [dict(initial_capital=100000.0), dict(initial_capital=25000.0, buy_slippage=0.05, sell_slippage=0.02, buy_commission_rate=0.001,
                                                  sell_commission_rate=0.002, minimum_commission_fee=1.0)]
    got = launch(api, np.stack([off, off]), a, q, p, A, bench_series(T), plist)
    for b, prm in enumerate(plist):
        ref = R.run_lanes(off, a, q, p, A, prm)
        covered(f"shared[{b}]", ref, len(a))
        same(f"shared[{b}] equity", got["equity"][b], ref["equity"])
        same(f"shared[{b}] cash", got["cash"][b], ref["cash"])
        same(f"shared[{b}] position", got["position"][b], ref["position"])
        assert got["counts"][b].tolist() == [ref["trades"], ref["wins"]]
        exp = oracle.summary(got["equity"][b], bench_series(T), prm["initial_capital"], ref["trades"], ref["wins"])
        np.testing.assert_allclose(got["summary"][b], exp, rtol=1e-12, atol=1e-13)
    assert not (got["cash"][0] == got["cash"][1]).all()


@pytest.mark.parametrize("A", [5, 65, 130])
def test_exact_tapes_equal_the_literal_order(api, oracle, A):
    """prices and slippages in 1/64, integer quantities <= 400, rates 2^-12, fee 5, c0 = 1e5: every product and sum is exact, so the
    device's equity equals the ascending-id valuation bit for bit, with ascending and with shuffled id assignment"""
    tapes = [R.random_tape(200 + A, 130, A, 8, exact=True, shuffle_ids=s) for s in (False, True)]
    check(api, oracle, f"exact A={A}", tapes, A, params=EXACT, literal="exact")


def test_defensive_clamps(api):
    """an offset outside [0, n_orders] is clamped, a decreasing pair is an empty period, an asset id outside [0, A) is skipped"""
    _, a, q, p = R.tape_of([[(0, 10.0, 50.0), (7, 5.0, 20.0), (-1, 5.0, 20.0), (1, 4.0, 30.0), (1, -2.0, 35.0), (0, -3.0, 55.0)]])
    off = np.array([-5, 2, 4, 3, 5, 99], dtype=np.int64)
    got = launch(api, off, a, q, p, 2)
    ref = R.run_lanes(off, a, q, p, 2)
    # [0, 2): a buy and a skipped id; [2, 4): a skipped id and a buy; [4, 3): empty; [3, 5): that buy again and a sell; [5, 6): a sell
    assert ref["trades"] == 3 and ref["outcomes"]["sell_filled"] == 2 and sum(ref["outcomes"].values()) == 5
    for k in ("equity", "cash", "position"):
        same(f"clamps {k}", got[k][0], ref[k])
    assert got["counts"][0].tolist() == [ref["trades"], ref["wins"]]


def ma_strategy(prices, fast=3, slow=8):
    """a small moving-average strategy over the columns of `prices` {name: [T]}: buy 50 when the fast mean crosses above the slow one,
    sell 50 when it crosses below; the callback sees the period index only"""
    def cb(ctx, t):
        if t < slow:
            return
        for name, px in prices.items():
            f, s = px[t - fast + 1:t + 1].mean(), px[t - slow + 1:t + 1].mean()
            f0, s0 = px[t - fast:t].mean(), px[t - slow:t].mean()
            if f > s and f0 <= s0:
                ctx.buy(name, 50.0, float(px[t]))
            elif f < s and f0 >= s0:
                ctx.sell(name, 50.0, float(px[t]))
    return cb


def test_surface(api, oracle):
    import polars_quant_amd as pq
    from polars_quant_amd._spec import SUMMARY_KEYS
    T = 150
    rng = np.random.default_rng(9)
    prices = {k: 40.0 * (j + 1) * np.cumprod(1.0 + 0.02 * rng.standard_normal(T)) for j, k in enumerate(("AAA", "BBB", "CCC"))}
    cb = ma_strategy(prices)
    bench = bench_series(T)
    bt = pq.SequentialBacktester(prices["AAA"], benchmark={"b": bench}, initial_capital=50000.0, buy_slippage=0.01)
    positions, capital, summary = bt.run(cb)
    many = bt.run_many([cb])
    tape = pq.OrderTape.record(cb, T)
    assert tape.n_orders >= 10 and sorted(tape.assets) == ["AAA", "BBB", "CCC"]
    ref = R.run_lanes(tape.period_offsets, tape.asset, tape.quantity, tape.price, 3, bt.params)
    assert ref["outcomes"]["buy_filled"] >= 3 and ref["outcomes"]["sell_filled"] >= 3
    eq = np.asarray(capital["equity"], dtype=np.float64)
    assert eq.shape == (T,) and len(positions) == 0
    same("run equity", eq, ref["equity"])
    same("run_many equity", many["equity"][0], eq)
    same("run_many position", many["position"][0], ref["position"])
    assert many["assets"] == tape.assets and (int(many["trades"][0]), int(many["wins"][0])) == (ref["trades"], ref["wins"])
    assert list(summary) == SUMMARY_KEYS and summary == many["summary"][0]
    exp = oracle.summary(eq, bench, 50000.0, ref["trades"], ref["wins"])
    np.testing.assert_allclose([summary[k] for k in SUMMARY_KEYS], exp, rtol=1e-12, atol=1e-13)
    assert summary["beta"] != 0.0
    # a benchmark of another length is not used (metrics.rs:86): alpha and beta are 0
    short = pq.SequentialBacktester(prices["AAA"], benchmark=bench[:-1], initial_capital=50000.0, buy_slippage=0.01)
    _, cap2, s2 = short.run(cb)
    same("equity without the benchmark", np.asarray(cap2["equity"], dtype=np.float64), eq)
    assert s2["alpha"] == 0.0 and s2["beta"] == 0.0 and s2["sharpe_ratio"] == summary["sharpe_ratio"]


def test_run_many_renumbers_into_one_universe(api):
    """two tapes with different first-seen orders and one set of overriding parameters, replayed in one launch"""
    import polars_quant_amd as pq

    def cb1(ctx, t):
        ctx.buy("x", 10.0, 20.0 + t)
        ctx.buy("y", 5.0, 30.0)
        if t % 3 == 2:
            ctx.sell("x", 12.0, 21.0 + t)

    def cb2(ctx, t):
        ctx.buy("y", 7.0, 31.0 + t)
        ctx.buy("z", 2.0, 50.0)
        if t % 2:
            ctx.sell("y", 3.0, 33.0 + t)
    T = 20
    bt = pq.SequentialBacktester(np.zeros(T))
    t2 = pq.OrderTape.record(cb2, T)
    r = bt.run_many([cb1, t2], params=[{}, dict(initial_capital=3000.0, minimum_commission_fee=0.0)])
    assert r["assets"] == ["x", "y", "z"] and r["equity"].shape == (2, T) and r["position"].shape == (2, 3)
    t1 = pq.OrderTape.record(cb1, T, assets=r["assets"])
    t2u = pq.OrderTape.record(cb2, T, assets=r["assets"])
    for b, (tape, prm) in enumerate(((t1, {}), (t2u, dict(initial_capital=3000.0, minimum_commission_fee=0.0)))):
        ref = R.run_lanes(tape.period_offsets, tape.asset, tape.quantity, tape.price, 3, prm)
        same(f"run_many[{b}] equity", r["equity"][b], ref["equity"])
        same(f"run_many[{b}] cash", r["cash"][b], ref["cash"])
        same(f"run_many[{b}] position", r["position"][b], ref["position"])
        assert (int(r["trades"][b]), int(r["wins"][b])) == (ref["trades"], ref["wins"])
