"""-m gpu: group portfolios with rebalancing, weights, drift and costs (D-27, csrc/portfolio/portfolio.hip) against the numpy
restatement in tests/factor_portfolio_ref.py.  Every comparison of value, turnover and count is bitwise, through api.factor_portfolio."""
import numpy as np
import pytest

import backtest_report_ref as R
import factor_portfolio_ref as P
import xsec_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(1, 5), (2, 3), (37, 50), (300, 131), (520, 70)]   # (300, 131): two blocks, three waves of days; (520, 70): three blocks
GROUPS = [2, 3, 5, 6, 10, 11, 20]                            # every instantiation and the first count above each
C0 = 1_000_000.0


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


def schedules(T):
    """name -> rebalance days: every day, every 5 and 21 days, a single day, d_0 > 0, the last day = T - 1, an irregular list, an
    interval longer than T"""
    irregular = sorted({0, 1, 2, T // 3, T // 3 + 1, T // 2, T - 2, T - 1} & set(range(T)))
    return {"daily": list(range(T)), "every5": list(range(0, T, 5)), "every21": list(range(0, T, 21)), "single": [T // 2],
            "late_start": list(range(min(3, T - 1), T, 4)), "ends_on_last": sorted({0, T // 2, T - 1}), "irregular": irregular,
            "longer_than_T": list(range(0, T, T + 7))}


def make(n, T, ng, seed, weights, dirty=True):
    """prices on a random walk (dirty: 5 % NULL and some NaN, 0 and negative cells), random labels with PQ_LABEL_MID / PQ_LABEL_OUT
    among them, weights with NULL / 0 / negative / inf cells"""
    rng = np.random.default_rng(seed)
    price = 20.0 * np.exp(np.cumsum(0.03 * rng.standard_normal((n, T)), axis=1))
    if dirty:
        price[rng.random((n, T)) < 0.05] = P.NULL
        price[rng.random((n, T)) < 0.01] = np.nan
        price[rng.random((n, T)) < 0.01] = 0.0
        price[rng.random((n, T)) < 0.01] *= -1.0
    lab = rng.integers(0, ng + 2, (n, T))
    labels = np.where(lab == ng, P.LABEL_MID, np.where(lab == ng + 1, P.LABEL_OUT, lab)).astype(np.uint8)
    weight = None
    if weights:
        weight = np.exp(rng.standard_normal((n, T)))
        for bad in (P.NULL, 0.0, -1.5, np.inf):
            weight[rng.random((n, T)) < 0.02] = bad
    return labels, price, weight


def to_dev(a, pitch=None):
    n, T = a.shape
    if pitch is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = torch.full((n, pitch), 7, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    buf[:, :T] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf[:, :T]


def check(labels, price, weight, ng, days, lag=0, cost=0.0, pitch=None, tag=""):
    from polars_quant_amd import api
    got = api.factor_portfolio(to_dev(labels, pitch), to_dev(price, pitch), ng, days, None if weight is None else to_dev(weight, pitch),
                               lag, cost, C0)
    torch.cuda.synchronize()
    exp = P.portfolio(labels, price, ng, days, weight, lag, cost, C0)
    tag = f"{tag} {price.shape} ng={ng} R={len(days)} lag={lag} cost={cost} weights={weight is not None} pitch={pitch}"
    same("count " + tag, got["count"].cpu().numpy(), exp["count"])
    same("turnover " + tag, got["turnover"].cpu().numpy(), exp["turnover"])
    same("value " + tag, got["value"].cpu().numpy(), exp["value"])
    same("rebalance_days " + tag, got["rebalance_days"].cpu().numpy(), np.asarray(days, dtype=np.int32))
    return exp


@pytest.mark.parametrize("ng", GROUPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_and_group_count(pq, shape, ng):
    """dirty prices, random labels; the schedule, the weights, label_lag and the cost rate rotate over the cases"""
    n, T = shape
    i = SHAPES.index(shape) * len(GROUPS) + GROUPS.index(ng)
    labels, price, weight = make(n, T, ng, 100 + i, weights=i % 2 == 1)
    names = sorted(schedules(T))
    lag = (i // 2) % 2
    days = sorted({max(d, lag) for d in schedules(T)[names[i % len(names)]]})
    check(labels, price, weight, ng, days, lag, (0.0, 0.003)[(i // 3) % 2], tag=names[i % len(names)])


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("name", sorted(schedules(131)))
def test_every_rebalance_schedule(pq, name, weights):
    n, T, ng = 300, 131, 5
    labels, price, weight = make(n, T, ng, 7, weights)
    check(labels, price, weight, ng, schedules(T)[name], 0, 0.003, tag=name)


@pytest.mark.parametrize("lag,cost", [(0, 0.0), (1, 0.003)])
def test_pitched_inputs(pq, lag, cost):
    n, T, ng = 300, 131, 3
    labels, price, weight = make(n, T, ng, 11, True)
    check(labels, price, weight, ng, list(range(1, T, 21)), lag, cost, pitch=144, tag="pitched")
    check(labels, price, None, ng, list(range(1, T, 5)), lag, cost, pitch=133, tag="odd pitch")


def test_a_suspended_symbol_and_a_day_without_members(pq):
    """a symbol without a price through a whole segment (and on the rebalance day that ends it) keeps its last price; a group that is
    empty on a rebalance day sits in cash until the next one and pays to come back"""
    n, T, ng = 37, 50, 3
    labels, price, weight = make(n, T, ng, 21, True, dirty=False)
    days = [0, 10, 20, 30, 40]
    labels[:, 0] = 1                         # symbol 3 is held from day 0 ...
    price[3, 1:21] = P.NULL                  # ... and has no price on days 1 .. 20: segment 0 whole, day 10 and day 20 included
    price[5, 11:20] = np.nan                 # suspended inside segment 1, back on its last day
    labels[labels[:, 20] == 2, 20] = 0       # group 2 has no member on day 20
    exp = check(labels, price, weight, ng, days, 0, 0.003, tag="suspended")
    assert exp["count"][2, 2] == 0 and exp["count"][2, 3] > 0 and exp["turnover"][2, 2] > 0.0 and abs(exp["turnover"][2, 3] - 1.0) < 1e-12
    assert exp["value"][2, 21] == exp["value"][2, 29] == exp["value"][2, 20]
    check(labels, price, None, ng, days, 0, 0.0, tag="suspended, equal weights")


@pytest.mark.parametrize("shape", [(37, 50), (300, 131)])
def test_the_labels_of_the_sorts_are_taken_without_a_copy(pq, shape):
    from polars_quant_amd import api
    n, T = shape
    rng = np.random.default_rng(5)
    _, price, weight = make(n, T, 5, 31, True)
    factor = rng.standard_normal((n, T))
    factor[rng.random((n, T)) < 0.05] = X.NULL
    pitch = 144 if T > 100 else 64
    fd, pd, wd = to_dev(factor, pitch), to_dev(price, pitch), to_dev(weight, pitch)
    for got, ng in ((api.factor_quantiles(fd, pd, 5, labels=True), 5), (api.factor_long_short(fd, pd, 0.3, 0.2, labels=True), 2)):
        lab = got["labels"]
        assert api._labels_on_pitch(lab, api._xsec_inputs([pd])[1], lab.device, (n, T)) is lab
        ref_lab = X.labels(factor, price, 0 if ng == 5 else 1, 5, 0.3, 0.2)
        same("labels", lab.cpu().numpy(), ref_lab)
        days = list(range(1, T, 5))
        res = api.factor_portfolio(lab, pd, ng, days, wd, 1, 0.003, C0)
        exp = P.portfolio(ref_lab, price, ng, days, weight, 1, 0.003, C0)
        for k in ("count", "turnover", "value"):
            same(f"{k} ng={ng}", res[k].cpu().numpy(), exp[k])


def test_host_inputs_and_foreign_label_layouts(pq):
    from polars_quant_amd import api
    labels, price, weight = make(37, 50, 5, 41, True)
    exp = P.portfolio(labels, price, 5, [0, 7, 30], weight, 0, 0.003, C0)
    for lab in (labels, torch.from_numpy(labels), torch.from_numpy(labels).cuda(), torch.from_numpy(labels.T.copy()).cuda().T):
        got = api.factor_portfolio(lab, price, 5, np.array([0, 7, 30]), weight, cost_rate=0.003)
        for k in ("count", "turnover", "value"):
            same(k, got[k].cpu().numpy(), exp[k])
    with pytest.raises(ValueError):
        api.factor_portfolio(labels[:, :-1], price, 5, [0])
    with pytest.raises(ValueError):
        api.factor_portfolio(labels.astype(np.int32), price, 5, [0])
    with pytest.raises(ValueError):
        api.factor_portfolio(labels, price, 5, [0.5])


def test_empties(pq):
    from polars_quant_amd import api
    labels, price, weight = make(37, 50, 4, 51, True)
    got = api.factor_portfolio(labels, price, 4, [])                                   # R = 0
    assert got["turnover"].shape == (4, 0) and got["count"].shape == (4, 0) and got["rebalance_days"].shape == (0,)
    same("R = 0", got["value"].cpu().numpy(), np.full((4, 50), C0))
    got = api.factor_portfolio(labels[:0], price[:0], 4, [0, 9], weight[:0], cost_rate=0.003)   # N = 0: cash
    exp = P.portfolio(labels[:0], price[:0], 4, [0, 9], weight[:0], 0, 0.003, C0)
    same("N = 0 value", got["value"].cpu().numpy(), exp["value"])
    same("N = 0 value is the capital", got["value"].cpu().numpy(), np.full((4, 50), C0))
    same("N = 0 turnover", got["turnover"].cpu().numpy(), np.zeros((4, 2)))
    same("N = 0 count", got["count"].cpu().numpy(), np.zeros((4, 2), dtype=np.int32))
    got = api.factor_portfolio(labels[:, :0], price[:, :0], 4, [])                     # T = 0
    assert got["value"].shape == (4, 0) and got["turnover"].shape == (4, 0)


def test_refusals(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    n, T = 37, 50
    labels, price, weight = make(n, T, 5, 61, True)
    good = dict(n_groups=5, rebalance_days=[1, 9], label_lag=1, cost_rate=0.003, initial_capital=C0)
    for change, match in ((dict(n_groups=0), "n_groups"), (dict(n_groups=21), "n_groups"), (dict(label_lag=-1), "label_lag"),
                          (dict(cost_rate=-0.001), "cost_rate"), (dict(cost_rate=1.0), "cost_rate"), (dict(cost_rate=float("nan")), "cost_rate"),
                          (dict(initial_capital=0.0), "initial_capital"), (dict(initial_capital=-1.0), "initial_capital"),
                          (dict(initial_capital=float("inf")), "initial_capital"), (dict(initial_capital=float("nan")), "initial_capital"),
                          (dict(rebalance_days=[9, 9]), "ascending"), (dict(rebalance_days=[9, 8]), "ascending"),
                          (dict(rebalance_days=[1, T]), "outside"), (dict(rebalance_days=[-1, 3]), "outside"),
                          (dict(rebalance_days=[0, 3]), "outside")):          # day 0 < label_lag 1
        with pytest.raises(pq.PqError, match=match):
            api.factor_portfolio(labels, price, **{**good, **change})
    # what the Python layer cannot send: a negative count, null pointers, a ragged batch, a recording context
    lab, p = to_dev(labels), to_dev(price)
    dev = p.device
    b = Batch(n, T, T)
    days = np.array([1, 9], dtype=np.int32)
    val = torch.empty((5, T), dtype=torch.float64, device=dev)
    tov = torch.empty((5, 2), dtype=torch.float64, device=dev)
    cnt = torch.empty((5, 2), dtype=torch.int32, device=dev)

    def call(batch=b, labels=lab, price=p, days=days, R=2, value=val, turnover=tov, count=cnt):
        api._call("pq_factor_portfolio", dev, batch, labels, 5, 1, price, None, days, R, 0.003, C0, value, turnover, count)

    with pytest.raises(pq.PqError, match="n_rebalance"):
        call(R=-1)
    for null in ("labels", "price", "days", "value", "turnover", "count"):
        with pytest.raises(pq.PqError, match="null pointer"):
            call(**{null: None})
    ragged, _offsets = api.ragged_batch(np.array([0, T, 2 * T]), dev)
    with pytest.raises(pq.PqError, match="ragged"):
        call(batch=ragged)
    api._call("pq_suite_begin", None, api.ctx(dev.index), b)
    try:
        with pytest.raises(pq.PqError, match="recorded"):
            call()
    finally:
        api._call("pq_suite_abort", None, api.ctx(dev.index))
    call()                                                                       # the context computes again
    torch.cuda.synchronize()
    same("after the refusals", val.cpu().numpy(), P.portfolio(labels, price, 5, [1, 9], None, 1, 0.003, C0)["value"])


def report_matches(name, got, value, bench):
    """got: {column name: [G]} of the GPU; the restatement of D-22 on `value`, annualized_return (the device's pow) within D-22's 1e-12"""
    cols = list(range(15)) + (list(range(38, 45)) if bench is not None else [])
    assert list(got) == [R.NAMES[c] for c in cols]
    g = {k: v.cpu().numpy() for k, v in got.items()}
    exp = R.report(value, C0, bench, ann=g["annualized_return"])
    for c in cols:
        if c == 3:
            live = ~R.isnull(exp[:, 3])
            same(name + " NULLs of annualized_return", R.isnull(g["annualized_return"]), R.isnull(exp[:, 3]))
            err = np.abs(g["annualized_return"][live] - exp[live, 3]) / np.maximum(np.abs(exp[live, 3]), 1.0)
            assert (err <= 1e-12).all(), (name, err.max())
        else:
            same(f"{name} {R.NAMES[c]}", g[R.NAMES[c]], exp[:, c])


@pytest.mark.parametrize("legs", [False, True])
def test_portfolio_backtest_end_to_end(pq, legs):
    from polars_quant_amd import api
    n, T = 300, 131
    rng = np.random.default_rng(71)
    _, price, weight = make(n, T, 5, 72, True)
    factor = rng.standard_normal((n, T))
    factor[rng.random((n, T)) < 0.05] = X.NULL
    bench = 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(T)))
    kw = dict(top_pct=0.3, bottom_pct=0.2) if legs else dict(n_quantiles=5)
    ng = 2 if legs else 5
    res = pq.Factor().portfolio_backtest(factor, price, rebalance=21, start=2, weight=weight, lag=1, cost_rate=0.002, benchmark=bench if legs else None,
                                         **kw)
    torch.cuda.synchronize()
    lab = X.labels(factor, price, 1 if legs else 0, 5, 0.3, 0.2)
    days = list(range(2, T, 21))
    exp = P.portfolio(lab, price, ng, days, weight, 1, 0.002, C0)
    for k in ("count", "turnover", "value"):
        same(k, res[k].cpu().numpy(), exp[k])
    same("rebalance_days", res["rebalance_days"].cpu().numpy(), np.asarray(days, dtype=np.int32))
    report_matches("statistics", res["statistics"], exp["value"], bench if legs else None)
    rep = api.backtest_report(res["value"], C0, bench if legs else None).cpu().numpy()
    for name, col in res["statistics"].items():
        same("statistics are the report's " + name, col.cpu().numpy(), rep[:, R.C[name]])
    (daily,) = api.call("returns", res["value"], period=1)
    same("daily_return", res["daily_return"].cpu().numpy(), daily.cpu().numpy())
    d = daily.cpu().numpy()
    with np.errstate(invalid="ignore"):
        diff = np.where(R.isnull(d[ng - 1]) | R.isnull(d[0]), P.NULL, d[ng - 1] - d[0])
    same("ls_return", res["ls_return"].cpu().numpy(), diff)
    # an explicit list of days is the same call
    again = pq.Factor().portfolio_backtest(factor, price, rebalance=days, weight=weight, lag=1, cost_rate=0.002, **kw)
    same("explicit days", again["value"].cpu().numpy(), exp["value"])
