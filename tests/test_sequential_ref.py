"""not-gpu: decision D-23 (the SequentialBacktester engine on an order tape) -- the two restatements of tests/seq_ref.py against known
answers derived by hand, against each other on random tapes, and the host side of the feature: OrderContext, OrderTape and the public
names.  tests/test_sequential_gpu.py holds the kernel to run_lanes bit for bit."""
import inspect

import numpy as np
import pytest

import seq_ref as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("fn", [R.run_literal, R.run_lanes], ids=["literal", "lanes"])
@pytest.mark.parametrize("name", sorted(R.KATS))
def test_known_answers(name, fn):
    periods, A, prm, exp = R.KATS[name]
    r = fn(*R.tape_of(periods), A, prm)
    for k in ("equity", "cash", "position"):
        assert (bits(r[k]) == bits(exp[k])).all(), (name, k, r[k], exp[k])
    assert (r["trades"], r["wins"]) == (exp["trades"], exp["wins"]), name


def test_known_answers_cover_every_outcome():
    seen = {k: 0 for k in ("buy_filled", "buy_rejected", "sell_filled", "sell_rejected")}
    for periods, A, prm, _ in R.KATS.values():
        for k, v in R.run_lanes(*R.tape_of(periods), A, prm)["outcomes"].items():
            seen[k] += v
    assert all(v >= 1 for v in seen.values()), seen


def test_orders_outside_the_rule_do_nothing():
    """a NaN or non-positive price, a NaN or zero quantity: not even the board moves"""
    nan = float("nan")
    periods = [[(0, 10.0, 50.0)], [(0, 5.0, nan), (0, 5.0, 0.0), (0, -5.0, -1.0), (0, nan, 70.0), (0, 0.0, 70.0)]]
    r = R.run_lanes(*R.tape_of(periods), 1)
    assert r["equity"].tolist() == [99995.0, 99995.0] and r["trades"] == 1
    assert sum(r["outcomes"].values()) == 1


def test_order_context_filters():
    import polars_quant_amd as pq
    nan = float("nan")
    ctx = pq.OrderContext()
    for p in (nan, 0.0, -1.0):
        ctx.buy("a", 1.0, p)
        ctx.sell("a", 1.0, p)
    for q in (nan, 0.0, -1.0):
        ctx.buy("a", q, 10.0)
        ctx.sell("a", q, 10.0)
    assert ctx.pending_orders == []
    ctx.buy("a", 2.0, 10.0)
    ctx.sell("b", 3.0, 11.0)
    assert ctx.pending_orders == [("a", 2.0, 10.0), ("b", -3.0, 11.0)]


def test_record_offsets_with_empty_periods():
    from polars_quant_amd import OrderTape

    def cb(ctx, t):
        if t == 1:
            ctx.buy("x", 1.0, 10.0)
            ctx.buy("y", 2.0, 20.0)
        if t == 4:
            ctx.sell("y", 1.0, 21.0)
            ctx.buy("z", 1.0, float("nan"))          # filtered: z is never numbered
    tape = OrderTape.record(cb, 6)
    assert tape.period_offsets.tolist() == [0, 0, 2, 2, 2, 3, 3] and tape.period_offsets.dtype == np.int64
    assert tape.assets == ["x", "y"] and tape.asset.tolist() == [0, 1, 1] and tape.asset.dtype == np.int32
    assert tape.quantity.tolist() == [1.0, 2.0, -1.0] and tape.price.tolist() == [10.0, 20.0, 21.0]
    assert tape.n_periods == 6 and tape.n_orders == 3
    fixed = OrderTape.record(cb, 6, assets=["y", "w", "x"])
    assert fixed.assets == ["y", "w", "x"] and fixed.asset.tolist() == [2, 0, 0]
    with pytest.raises(ValueError):
        OrderTape.record(cb, 6, assets=["x"])


def test_record_keeps_the_orders_before_an_exception():
    from polars_quant_amd import OrderTape

    def cb(ctx, t):
        ctx.buy("x", 1.0, 10.0 + t)
        if t == 1:
            raise RuntimeError("strategy bug")
        ctx.sell("x", 1.0, 11.0 + t)
    tape = OrderTape.record(cb, 3)
    assert tape.period_offsets.tolist() == [0, 2, 3, 5]
    assert tape.quantity.tolist() == [1.0, -1.0, 1.0, 1.0, -1.0]


@pytest.mark.parametrize("bad", [
    dict(period_offsets=[0, 2, 1, 3]),                   # decreasing
    dict(period_offsets=[1, 2, 3]),                      # does not start at 0
    dict(period_offsets=[0, 1, 2]),                      # does not end at the order count
    dict(asset=[0, 1, 2]),                               # id == len(assets)
    dict(asset=[0, -1, 1]),
    dict(quantity=[1.0, 2.0]),                           # ragged arrays
])
def test_tape_validation(bad):
    from polars_quant_amd import OrderTape
    kw = dict(assets=["a", "b"], period_offsets=[0, 1, 3], asset=[0, 1, 1], quantity=[1.0, 2.0, -1.0], price=[5.0, 6.0, 7.0])
    OrderTape(**kw)
    with pytest.raises(ValueError):
        OrderTape(**{**kw, **bad})


@pytest.mark.parametrize("A", [1, 5, 65, 130])
def test_literal_against_lanes_on_random_tapes(A):
    """cash, positions, trades and wins do not depend on the valuation's order; equity differs by at most
    2 A 2^-53 (|cash| + V): two orderings of at most A positive terms (each within (A - 1) 2^-53 V of the exact sum) plus the final
    add, whose rounding moves by at most 2^-53 of |cash| + V more than the difference of its operands"""
    tape = R.random_tape(100 + A, 130, A, 8)
    lit, lan = R.run_literal(*tape, A), R.run_lanes(*tape, A)
    assert all(v >= 8 for v in lan["outcomes"].values()), lan["outcomes"]
    assert (bits(lit["cash"]) == bits(lan["cash"])).all() and (bits(lit["position"]) == bits(lan["position"])).all()
    assert (lit["trades"], lit["wins"]) == (lan["trades"], lan["wins"])
    V = np.abs(lan["equity"] - lan["cash"])
    bound = 2.0 * A * 2.0 ** -53 * (np.abs(lan["cash"]) + V)
    diff = np.abs(lit["equity"] - lan["equity"])
    print(f"A = {A}: worst |literal - lanes| {diff.max():.3e}, bound there {bound[diff.argmax()]:.3e}")
    assert (diff <= bound).all()


@pytest.mark.parametrize("A", [5, 65, 130])
def test_exact_tapes_do_not_depend_on_the_order(A):
    """prices and slippages in 1/64, integer quantities <= 400, rates 2^-12, fee 5: every product and sum is exact, so ascending-id and
    lane-order valuation agree bit for bit, under either id assignment"""
    prm = dict(buy_commission_rate=2.0 ** -12, sell_commission_rate=2.0 ** -12, buy_slippage=1 / 64, sell_slippage=3 / 64)
    for shuffle in (False, True):
        tape = R.random_tape(200 + A, 130, A, 8, exact=True, shuffle_ids=shuffle)
        lit, lan = R.run_literal(*tape, A, prm), R.run_lanes(*tape, A, prm)
        assert all(v >= 8 for v in lan["outcomes"].values()), lan["outcomes"]
        assert (bits(lit["equity"]) == bits(lan["equity"])).all()


def test_public_names():
    import polars_quant_amd as pq
    from polars_quant_amd._spec import SEQ_DEFAULTS
    assert callable(pq.OrderContext().buy) and callable(pq.OrderContext().sell)
    sig = inspect.signature(pq.SequentialBacktester.__init__)
    assert list(sig.parameters)[1:] == ["historical_data", "benchmark", "initial_capital", "buy_slippage", "sell_slippage",
                                        "buy_commission_rate", "sell_commission_rate", "minimum_commission_fee"]
    assert {k: sig.parameters[k].default for k in SEQ_DEFAULTS} == SEQ_DEFAULTS
    assert sig.parameters["benchmark"].default is None
    assert list(inspect.signature(pq.OrderContext.buy).parameters)[1:] == ["target_asset", "target_quantity", "execution_price"]
    assert list(inspect.signature(pq.OrderContext.sell).parameters)[1:] == ["target_asset", "target_quantity", "execution_price"]
    assert callable(pq.SequentialBacktester.run) and callable(pq.SequentialBacktester.run_many)
    from polars_quant_amd._lib import SeqParams
    assert [f for f, _ in SeqParams._fields_] == list(SEQ_DEFAULTS)


def test_empty_run_needs_no_gpu():
    """T == 0: no launch, empty summary, empty curve"""
    import polars_quant_amd as pq
    positions, capital, summary = pq.SequentialBacktester([]).run(lambda ctx, t: ctx.buy("x", 1.0, 1.0))
    assert len(capital["equity"]) == 0 and summary == {} and len(positions) == 0
