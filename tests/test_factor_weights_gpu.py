"""-m gpu: the backtest of given target weights, signed and with cash (D-35, csrc/portfolio/weights.hip) against the numpy restatement in
tests/factor_weights_ref.py.  Every comparison of value, turnover, net, gross, the counts, first_nonpositive and the holdings is bitwise,
through api.factor_weights; property (i) is checked against api.factor_portfolio on the device, and the chain optimal_portfolio ->
weights_backtest -> portfolio_risk end to end."""
import ctypes as C

import numpy as np
import pytest

import factor_weights_ref as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(1, 5), (2, 3), (37, 50), (300, 131), (520, 70)]   # (300, 131): two blocks, three waves of days; (520, 70): three blocks
COUNTS = [1, 2, 3, 8]                                        # the size classes <1>, <2>, <8> and the first count above <2>
KEYS = ("n_long", "n_short", "n_dropped", "net", "gross", "turnover", "value", "first_nonpositive")
C0 = 1_000_000.0
NULL = W.NULL


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def same(name, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    if exp.dtype == np.float64:
        g, e = np.ascontiguousarray(got, dtype=np.float64).view(np.uint64), np.ascontiguousarray(exp).view(np.uint64)
    else:
        g, e = got.astype(np.int64), exp.astype(np.int64)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def host(t):
    return t.cpu().numpy()


def schedules(T):
    """tests/test_factor_portfolio_gpu.py's: every day, every 5 and 21 days, a single day, d_0 > 0, the last day = T - 1, an irregular
    list, an interval longer than T"""
    irregular = sorted({0, 1, 2, T // 3, T // 3 + 1, T // 2, T - 2, T - 1} & set(range(T)))
    return {"daily": list(range(T)), "every5": list(range(0, T, 5)), "every21": list(range(0, T, 21)), "single": [T // 2],
            "late_start": list(range(min(3, T - 1), T, 4)), "ends_on_last": sorted({0, T // 2, T - 1}), "irregular": irregular,
            "longer_than_T": list(range(0, T, T + 7))}


def make(n, T, R, P, seed, dirty=True):
    """prices on a random walk (dirty: 5 % NULL and some NaN, 0 and negative cells); P weight arrays [n, R], long-short with a gross
    between 0.5 and 3 (so some cells are > 1 and the cash is negative), dirty: NULL, NaN, +-inf and 0.0 cells"""
    rng = np.random.default_rng(seed)
    price = 20.0 * np.exp(np.cumsum(0.03 * rng.standard_normal((n, T)), axis=1))
    if dirty:
        price[rng.random((n, T)) < 0.05] = NULL
        price[rng.random((n, T)) < 0.01] = np.nan
        price[rng.random((n, T)) < 0.01] = 0.0
        price[rng.random((n, T)) < 0.01] *= -1.0
    ws = []
    for p in range(P):
        w = rng.standard_normal((n, R))
        w *= rng.uniform(0.5, 3.0, (1, R)) / np.maximum(np.abs(w).sum(axis=0, keepdims=True), 1e-300)
        if n <= 2:
            w[0] = 1.5                                           # a cell > 1
        if dirty:
            for bad in (NULL, np.nan, np.inf, -np.inf, 0.0):
                w[rng.random((n, R)) < 0.03] = bad
        ws.append(w)
    return ws, price


def to_dev(a, pitch=None):
    n, T = a.shape
    if pitch is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf[:, :T]


def check(ws, price, days, cost=0.003, hold=None, pitch=None, wpitch=None, tag=""):
    from polars_quant_amd import api
    got = api.factor_weights([to_dev(w, wpitch) for w in ws], to_dev(price, pitch), days, cost, C0, hold)
    torch.cuda.synchronize()
    exp = W.weights(ws, price, days, cost, C0, hold)
    tag = f"{tag} {price.shape} P={len(ws)} R={len(days)} cost={cost} hold={hold} pitch={pitch} wpitch={wpitch}"
    for k in KEYS:
        same(f"{k} {tag}", host(got[k]), exp[k])
    same("rebalance_days " + tag, host(got["rebalance_days"]), np.asarray(days, dtype=np.int32))
    assert ("holdings" in got) == (hold is not None)
    if hold is not None:
        same("holdings " + tag, host(got["holdings"]), exp["holdings"])
    return got, exp


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_and_portfolio_count(pq, shape, P):
    """dirty prices and weights; the schedule, the cost rate and holdings_of (none, 0, P - 1) rotate over the cases"""
    n, T = shape
    i = SHAPES.index(shape) * len(COUNTS) + COUNTS.index(P)
    names = sorted(schedules(T))
    days = schedules(T)[names[i % len(names)]]
    ws, price = make(n, T, len(days), P, 100 + i)
    check(ws, price, days, (0.0, 0.003)[(i // 3) % 2], (None, 0, P - 1)[i % 3], tag=names[i % len(names)])


@pytest.mark.parametrize("name", sorted(schedules(131)))
def test_every_rebalance_schedule(pq, name):
    n, T, P = 300, 131, 3
    days = schedules(T)[name]
    ws, price = make(n, T, len(days), P, 7)
    check(ws, price, days, 0.003, P - 1, tag=name)


@pytest.mark.parametrize("P,hold", [(1, 0), (2, None), (8, 7)])
def test_pitched_inputs(pq, P, hold):
    n, T = 300, 131
    days = list(range(1, T, 21))
    ws, price = make(n, T, len(days), P, 11)
    check(ws, price, days, 0.003, hold, pitch=144, wpitch=len(days) + 3, tag="pitched")
    check(ws, price, days, 0.0, hold, pitch=133, wpitch=None, tag="odd price pitch")
    # host arrays, one stacked [P, N, R] array and weights on different pitches (made dense) are the same call
    from polars_quant_amd import api
    exp = W.weights(ws, price, days, 0.003, C0, hold)
    mixed = [to_dev(w, len(days) + (j % 2)) for j, w in enumerate(ws)]
    for arg in (np.stack(ws) if P > 1 else ws[0], mixed):
        got = api.factor_weights(arg, price, np.asarray(days), 0.003, C0, hold)
        for k in KEYS:
            same(k, host(got[k]), exp[k])


def test_a_suspended_symbol_a_dropped_target_and_an_empty_rebalance(pq):
    n, T, P = 37, 50, 2
    days = [0, 10, 20, 30, 40]
    ws, price = make(n, T, len(days), P, 21, dirty=False)
    price[3, 1:21] = NULL                    # held from day 0, no price through segment 0 and on days 10 and 20: dropped there
    price[5, 11:20] = np.nan                 # suspended inside segment 1, back on its last day
    ws[0][:, 2] = NULL                       # portfolio 0 holds nothing from day 20 to day 30: all cash
    got, exp = check(ws, price, days, 0.003, 0, tag="suspended")
    assert exp["n_dropped"][1].tolist() == [0, 1, 1, 0, 0] and (exp["n_long"][0, 2], exp["n_short"][0, 2]) == (0, 0)
    assert exp["value"][0, 21] == exp["value"][0, 29] == exp["value"][0, 20] and (exp["holdings"][:, 20:30] == 0.0).all()


def test_a_ruined_book(pq):
    """a levered short whose price quadruples wipes the first book out (what the curve does after that day means nothing and is only
    compared); the second survives"""
    n, T = 37, 50
    days = [0, 10, 20]
    ws, price = make(n, T, len(days), 2, 31, dirty=False)
    price[0] = np.concatenate([np.full(5, 10.0), np.linspace(10.0, 40.0, 10), np.full(T - 15, 40.0)])
    ws[0][0] = -3.0
    got, exp = check(ws, price, days, 0.003, 0, tag="ruined")
    assert 5 < exp["first_nonpositive"][0] < 15 and exp["first_nonpositive"][1] == -1
    assert exp["value"][0, exp["first_nonpositive"][0]] <= 0.0 and (exp["value"][0, :exp["first_nonpositive"][0]] > 0.0).all()


@pytest.mark.parametrize("n,members", [(64, 64), (520, 512)])
def test_property_i_on_the_device(pq, n, members):
    """2^m members, clean prices, equal weights 1 / 2^m: value and turnover are api.factor_portfolio's (one group) bit for bit"""
    from polars_quant_amd import api
    T, days = 131, [0, 9, 10, 33, 100, 130]
    rng = np.random.default_rng(6)
    price = 20.0 * np.exp(np.cumsum(0.03 * rng.standard_normal((n, T)), axis=1))
    labels = np.full((n, T), api.LABEL_OUT, dtype=np.uint8)
    w = np.full((n, len(days)), NULL)
    for k, d in enumerate(days):
        who = rng.permutation(n)[:members]
        labels[who, d] = 0
        w[who, k] = 1.0 / members
    got = api.factor_weights(w, price, days, 0.003, C0)
    exp = api.factor_portfolio(labels, price, 1, days, None, 0, 0.003, C0)
    torch.cuda.synchronize()
    same("value", host(got["value"]), host(exp["value"]))
    same("turnover", host(got["turnover"]), host(exp["turnover"]))
    same("count", host(got["n_long"]), host(exp["count"]))
    assert (host(got["net"]) == 1.0).all() and (host(got["n_dropped"]) == 0).all()


def test_optimal_portfolio_to_weights_backtest_to_portfolio_risk(pq):
    """the chain end to end: the minimum-variance weights of every second day are traded, their drifted holdings priced by the same
    model: on each rebalance day the holdings are the weights themselves and their risk is predicted_var within D-34's 1e-11"""
    from polars_quant_amd import api
    N, K, G, D, step = 300, 3, 7, 20, 2
    T = D * step
    rng = np.random.default_rng(3)
    X = rng.standard_normal((K, N, T))
    ind = rng.integers(0, G, N).astype(np.int32)
    F = np.cov(rng.normal(0.0, 0.01, (260, K + G)).T)
    sv = rng.uniform(0.01, 0.03, (N, D)) ** 2
    price = 20.0 * np.exp(np.cumsum(0.03 * rng.standard_normal((N, T)), axis=1))
    bench = 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T)))
    fac = pq.Factor()
    m = {"factor_cov": torch.from_numpy(np.repeat(F[None], D, axis=0)).cuda(), "specific_var": to_dev(sv), "day0": 0, "step": step}
    cols, gd = [to_dev(x) for x in X], torch.from_numpy(ind)
    opt = fac.optimal_portfolio(cols, m, industry=gd)
    res = fac.weights_backtest(opt, price, cost_rate=0.002, benchmark=bench, holdings=0)
    torch.cuda.synchronize()
    days = list(range(0, T, step))
    w = host(opt["weights"])
    assert host(opt["days"]).tolist() == days and not W.isnull(w).any()
    exp = W.weights([w], price, days, 0.002, C0, 0)
    for k in KEYS:
        same(k, host(res[k]), exp[k])
    same("holdings", host(res["holdings"]), exp["holdings"])
    assert (host(res["n_dropped"]) == 0).all() and host(res["rebalance_days"]).tolist() == days
    same("the holdings of a rebalance day are the weights", host(res["holdings"])[:, days], w)
    risk = fac.portfolio_risk(res["holdings"], cols, m, gd)
    tot, pv = host(risk["total_var"]), host(opt["predicted_var"])
    assert (host(risk["n_uncovered"]) == 0).all() and (host(risk["n_held"]) == N).all() and not W.isnull(tot).any()
    dev = np.abs(tot - pv) / pv
    print(f"portfolio_risk of the holdings against predicted_var: worst deviation {dev.max():.3g}")
    assert (dev <= 1e-11).all()
    # daily_return and statistics are what portfolio_backtest adds: returns on value, then the report with the benchmark columns
    from polars_quant_amd._spec import REPORT_COLS
    (daily,) = api.call("returns", res["value"], period=1)
    same("daily_return", host(res["daily_return"]), host(daily))
    rep = host(api.backtest_report(res["value"], C0, bench))
    assert list(res["statistics"]) == [REPORT_COLS[c] for c in list(range(15)) + list(range(38, 45))]
    for c, (name, col) in zip(list(range(15)) + list(range(38, 45)), res["statistics"].items()):
        same("statistics " + name, host(col), rep[:, c])
    # lag: the trade days move, trailing columns whose trade day is >= T are dropped
    lagged = fac.weights_backtest(opt["weights"], price, days=np.asarray(days), lag=3, cost_rate=0.002)
    kept = [d + 3 for d in days if d + 3 < T]
    assert host(lagged["rebalance_days"]).tolist() == kept and len(kept) == D - 1
    same("lagged value", host(lagged["value"]), W.weights([w[:, :len(kept)]], price, kept, 0.002, C0)["value"])
    assert "holdings" not in lagged


def raw_buffers(P, n, T, R, stride):
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    return {"value": torch.full((P, T), 7.0, **f64), "turnover": torch.full((P, max(R, 1)), 7.0, **f64),
            "exposure": torch.full((2, P, max(R, 1)), 7.0, **f64), "count": torch.full((3, P, max(R, 1)), 77, **i32),
            "first": torch.full((P,), 77, **i32), "holdings": torch.full((n, stride), 7.0, **f64)}


def test_empty_and_no_rebalance_calls(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    ws, price = make(37, 50, 2, 3, 51)
    got = api.factor_weights([w[:, :0] for w in ws], price, [], holdings_of=2)                  # R = 0: never invested
    exp = W.weights([w[:, :0] for w in ws], price, [], 0.001, C0, 2)
    for k in KEYS:
        same("R = 0 " + k, host(got[k]), exp[k])
    same("R = 0 holdings", host(got["holdings"]), np.zeros((37, 50)))
    same("R = 0 value", host(got["value"]), np.full((3, 50), C0))
    got = api.factor_weights([w[:0] for w in ws], price[:0], [0, 9], holdings_of=0)             # N = 0: cash
    same("N = 0 value", host(got["value"]), np.full((3, 50), C0))
    same("N = 0 turnover", host(got["turnover"]), np.zeros((3, 2)))
    assert (host(got["first_nonpositive"]) == -1).all() and got["holdings"].shape == (0, 50) and (host(got["n_dropped"]) == 0).all()
    got = api.factor_weights(np.zeros((37, 0)), price[:, :0], [])                               # T = 0
    assert got["value"].shape == (1, 0) and got["turnover"].shape == (1, 0)
    # the C entry itself: R = 0 writes the capital, -1 and 0.0; an empty batch returns without touching anything
    n, T = 37, 50
    p = to_dev(price)
    wd = [to_dev(w) for w in ws]
    wp = (C.c_void_p * 3)(*[w.data_ptr() for w in wd])
    o = raw_buffers(3, n, T, 0, T)
    api._call("pq_factor_weights", p.device, Batch(n, T, T), wp, 3, 2, p, None, 0, 0.001, C0, o["value"], None, None, None, o["first"], 1,
              o["holdings"])
    torch.cuda.synchronize()
    same("C entry R = 0 value", host(o["value"]), np.full((3, T), C0))
    assert host(o["first"]).tolist() == [-1] * 3 and (host(o["holdings"]) == 0.0).all()
    for batch in (Batch(0, T, T), Batch(n, 0, 0)):
        o = raw_buffers(3, n, T, 2, T)
        api._call("pq_factor_weights", p.device, batch, wp, 3, 2, p, np.array([0, 9], dtype=np.int32), 2, 0.001, C0, o["value"], o["turnover"],
                  o["exposure"], o["count"], o["first"], 1, o["holdings"])
        torch.cuda.synchronize()
        assert (host(o["value"]) == 7.0).all() and (host(o["first"]) == 77).all() and (host(o["holdings"]) == 7.0).all()


def test_refusals_of_the_c_entry(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    n, T, P, R = 37, 50, 2, 2
    ws, price = make(n, T, R, P, 61)
    p = to_dev(price)
    dev = p.device
    wd = [to_dev(w) for w in ws]
    days = np.array([1, 9], dtype=np.int32)
    o = raw_buffers(P, n, T, R, T)

    def call(batch=None, weights=wd, n_p=P, ws_=R, price=p, days=days, R_=R, cost=0.003, cap=C0, value=o["value"], turnover=o["turnover"],
             exposure=o["exposure"], count=o["count"], first=o["first"], hold_of=1, hold=o["holdings"]):
        wp = None if weights is None else (C.c_void_p * len(weights))(*[None if w is None else w.data_ptr() for w in weights])
        api._call("pq_factor_weights", dev, batch or Batch(n, T, T), wp, n_p, ws_, price, days, R_, cost, cap, value, turnover, exposure,
                  count, first, hold_of, hold)

    for change, match in ((dict(n_p=0), "n_portfolios"), (dict(n_p=9), "n_portfolios"), (dict(R_=-1), "n_rebalance"),
                          (dict(ws_=1), "w_stride"), (dict(cost=-0.001), "cost_rate"), (dict(cost=1.0), "cost_rate"),
                          (dict(cost=float("nan")), "cost_rate"), (dict(cap=0.0), "initial_capital"), (dict(cap=float("inf")), "initial_capital"),
                          (dict(cap=float("nan")), "initial_capital"), (dict(hold_of=2), "holdings_of"), (dict(hold_of=-2), "holdings_of"),
                          (dict(hold_of=-1), "go together"), (dict(hold=None), "go together"),
                          (dict(days=np.array([9, 9], dtype=np.int32)), "ascending"), (dict(days=np.array([9, 8], dtype=np.int32)), "ascending"),
                          (dict(days=np.array([1, T], dtype=np.int32)), "outside"), (dict(days=np.array([-1, 3], dtype=np.int32)), "outside"),
                          (dict(weights=None), "null pointer"), (dict(weights=[wd[0], None]), "null weights"), (dict(price=None), "null pointer"),
                          (dict(days=None), "null pointer"), (dict(value=None), "null pointer"), (dict(turnover=None), "null pointer"),
                          (dict(exposure=None), "null pointer"), (dict(count=None), "null pointer"), (dict(first=None), "null pointer"),
                          (dict(hold=p), "overlap an input"), (dict(value=wd[1]), "overlap an input"),
                          (dict(turnover=o["value"]), "overlap each other"), (dict(exposure=o["turnover"]), "overlap each other")):
        with pytest.raises(pq.PqError, match=match):
            call(**change)
    ragged, _offsets = api.ragged_batch(np.array([0, T, 2 * T]), dev)
    with pytest.raises(pq.PqError, match="ragged"):
        call(batch=ragged)
    api._call("pq_suite_begin", None, api.ctx(dev.index), Batch(n, T, T))
    try:
        with pytest.raises(pq.PqError, match="recorded"):
            call()
    finally:
        api._call("pq_suite_abort", None, api.ctx(dev.index))
    torch.cuda.synchronize()
    for k, fill in (("value", 7.0), ("turnover", 7.0), ("exposure", 7.0), ("count", 77), ("first", 77), ("holdings", 7.0)):
        assert (host(o[k]) == fill).all(), f"a refused call wrote to {k}"
    call()                                                                       # the context computes again
    torch.cuda.synchronize()
    exp = W.weights(ws, price, [1, 9], 0.003, C0, 1)
    same("after the refusals: value", host(o["value"]), exp["value"])
    same("after the refusals: holdings", host(o["holdings"]), exp["holdings"])
