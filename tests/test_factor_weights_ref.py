"""not-gpu: the numpy restatement of decision D-35 (tests/factor_weights_ref.py) against answers derived by hand, one case per rule, its
two properties (bitwise agreement with D-27's restatement, linearity), an independent day-by-day share accounting, the argument checks
of api.factor_weights that need no device, and the register / scratch figures of csrc/portfolio/weights.hip."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import factor_portfolio_ref as P
import factor_weights_ref as W

ROOT = Path(__file__).resolve().parent.parent
NULL = W.NULL


def run(weights, price, days, cost_rate=0.0, initial_capital=1000.0, holdings_of=None):
    ws = [np.asarray(w, dtype=np.float64) for w in weights]
    return W.weights(ws, np.asarray(price, dtype=np.float64), days, cost_rate, initial_capital, holdings_of)


def same(got, exp, what=""):
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} cells differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {exp[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- the surface
def test_the_surface():
    """the restatement has something to restate: without the feature this fails"""
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    assert list(inspect.signature(api.factor_weights).parameters) == ["weights", "price", "rebalance_days", "cost_rate", "initial_capital",
                                                                      "holdings_of"]
    sig = inspect.signature(pq.Factor.weights_backtest)
    assert list(sig.parameters) == ["self", "weights", "price", "days", "lag", "cost_rate", "initial_capital", "benchmark", "holdings"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, 0, 0.001, 1_000_000.0, None, None]
    doc, adoc = " ".join(pq.Factor.weights_backtest.__doc__.split()), " ".join(api.factor_weights.__doc__.split())
    assert "are dropped" in doc and "one day later" in doc and "means nothing" in adoc and "mean nothing" in doc
    assert api.WEIGHTS_MAX_PORTFOLIOS == W.MAX_PORTFOLIOS == 8
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define PQ_WEIGHTS_MAX_PORTFOLIOS 8\b", txt)
    decl = re.search(r"pq_status\s+pq_factor_weights\s*\(([^)]*)\)", txt)
    assert decl, "pq_factor_weights is not declared"
    assert [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")] == [
        "pq_ctx *", "const pq_batch *", "const double *const *weights", "int32_t n_portfolios", "int64_t w_stride", "const double *price",
        "const int32_t *rebalance_days", "int64_t n_rebalance", "double cost_rate", "double initial_capital", "double *value",
        "double *turnover", "double *exposure", "int32_t *count", "int32_t *first_nonpositive", "int32_t holdings_of",
        "double *holdings_out"]
    assert re.search(r"^factor_weights\s+i\s+pBpilpplddpppppip$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "portfolio/weights.hip" in mk and mk.count("portfolio/weights.resources.txt") == 1
    assert "polars_quant_amd/csrc/portfolio/weights.resources.txt" in (ROOT / ".gitignore").read_text().split()


# ---------------------------------------------------------------- by hand
def test_hand_derived_dyadic_example():
    """Two symbols, prices (4, 8) -> (8, 4) -> (8, 2), rebalances on days 0 and 1, fee 1/4, capital 1000.
    k = 0: w = (1/2, -1/4): net 1/4, gross 3/4, cash 3/4; nothing held before: tau_0 = 1/2 + 1/4 = 3/4; B_0 = 1000 (1 - 3/16) = 812.5.
    day 1: G = 3/4 + 1/2 (8 / 4) - 1/4 (4 / 8) = 0.75 + 1.0 - 0.125 = 1.625; P_1 = 812.5 * 1.625 = 1320.3125.
    k = 1: w = (1/4, 1/2): net 3/4, gross 3/4, cash 1/4; drifted w_old = (1.0 / 1.625, -0.125 / 1.625) = (8/13, -1/13);
    tau_1 = |1/4 - 8/13| + |1/2 + 1/13| = 19/52 + 15/26 = 49/52; B_1 = 1320.3125 (1 - tau_1 / 4).
    day 2: G = 1/4 + 1/4 (8 / 8) + 1/2 (2 / 4) = 0.75; value = 0.75 B_1; holdings (0.25 / 0.75, 0.25 / 0.75) = (1/3, 1/3)."""
    r = run([[[0.5, 0.25], [-0.25, 0.5]]], [[4.0, 8.0, 8.0], [8.0, 4.0, 2.0]], [0, 1], cost_rate=0.25, holdings_of=0)
    assert r["net"].tolist() == [[0.25, 0.75]] and r["gross"].tolist() == [[0.75, 0.75]]
    assert r["n_long"].tolist() == [[1, 2]] and r["n_short"].tolist() == [[1, 0]] and r["n_dropped"].tolist() == [[0, 0]]
    tau1 = (0.0 + abs(0.25 - 1.0 / 1.625)) + abs(0.5 - (-0.125 / 1.625))
    assert r["turnover"].tolist() == [[0.75, tau1]] and abs(tau1 - 49.0 / 52.0) < 1e-15
    B1 = (812.5 * 1.625) * (1.0 - 0.25 * tau1)
    assert 812.5 * 1.625 == 1320.3125
    assert r["value"].tolist() == [[812.5, B1, B1 * 0.75]]
    assert r["holdings"].tolist() == [[0.5, 0.25, 0.25 / 0.75], [-0.25, 0.5, 0.25 / 0.75]]
    assert r["first_nonpositive"].tolist() == [-1]
    # without a fee and with one rebalance the curve is the capital times G
    r = run([[[0.5], [-0.25]]], [[4.0, 8.0], [8.0, 4.0]], [0])
    assert r["value"].tolist() == [[1000.0, 1625.0]] and r["turnover"].tolist() == [[0.75]]


# ---------------------------------------------------------------- one case per rule
def test_a_dropped_target_stays_in_cash():
    # s1 has no price on day 0: it is counted as dropped, its 1/2 stays in cash: G = (1 - 1/4) + 1/4 * 2 = 1.25
    r = run([[[0.25], [0.5]]], [[2.0, 4.0], [NULL, 8.0]], [0], holdings_of=0)
    assert r["n_long"].tolist() == [[1]] and r["n_dropped"].tolist() == [[1]] and r["net"].tolist() == [[0.25]]
    assert r["turnover"].tolist() == [[0.25]] and r["value"].tolist() == [[1000.0, 1250.0]]
    assert r["holdings"].tolist() == [[0.25, 0.5 / 1.25], [0.0, 0.0]]
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert run([[[0.25], [0.5]]], [[2.0, 4.0], [bad, 8.0]], [0])["n_dropped"].tolist() == [[1]]


def test_null_nan_inf_and_zero_weights_are_not_held():
    w = [[0.5], [NULL], [np.nan], [np.inf], [-np.inf], [0.0], [-0.0]]
    r = run([w], [[1.0, 2.0]] * 7, [0])
    assert r["n_long"].tolist() == [[1]] and r["n_short"].tolist() == [[0]] and r["n_dropped"].tolist() == [[0]]
    assert r["net"].tolist() == [[0.5]] and r["gross"].tolist() == [[0.5]] and r["value"].tolist() == [[1000.0, 1500.0]]


def test_a_suspended_member_keeps_its_held_price():
    # s0 has no usable price on days 1 and 2 (NULL, then 0): G = 1/2 + 1/2 * 1 there; on day 3 it trades at 3x
    r = run([[[0.5]]], [[2.0, NULL, 0.0, 6.0]], [0])
    assert r["value"].tolist() == [[1000.0, 1000.0, 1000.0, 2000.0]]
    # ... and across the next rebalance day its drifted weight uses the held price: w_old = (1/2 * (4 / 2)) / 1.5
    r = run([[[0.5, 0.5]]], [[2.0, 4.0, NULL, 8.0]], [0, 2], holdings_of=0)
    assert r["n_dropped"].tolist() == [[0, 1]] and r["turnover"].tolist() == [[0.5, abs(0.0 - 1.0 / 1.5)]]
    assert r["value"].tolist() == [[1000.0, 1500.0, 1500.0, 1500.0]]          # sold at the held price, then all cash
    assert r["holdings"].tolist() == [[0.5, 1.0 / 1.5, 0.0, 0.0]]


def test_an_empty_member_set_is_all_cash():
    r = run([[[NULL, 0.5]]], [[2.0, 4.0, 4.0, 8.0]], [0, 2])
    assert r["net"].tolist() == [[0.0, 0.5]] and r["turnover"].tolist() == [[0.0, 0.5]]
    assert r["value"].tolist() == [[1000.0, 1000.0, 1000.0, 1500.0]]


def test_no_rebalance_at_all():
    r = run([np.zeros((2, 0)), np.zeros((2, 0))], [[1.0, 2.0, 3.0]] * 2, [], holdings_of=1)
    assert r["value"].tolist() == [[1000.0] * 3] * 2 and r["first_nonpositive"].tolist() == [-1, -1]
    assert r["holdings"].tolist() == [[0.0] * 3] * 2
    assert all(r[k].shape == (2, 0) for k in ("turnover", "net", "gross", "n_long", "n_short", "n_dropped"))


def test_a_late_start_and_a_rebalance_on_the_last_day():
    r = run([[[1.0, 0.5]]], [[1.0, 2.0, 4.0, 8.0]], [1, 3], cost_rate=0.25, holdings_of=0)
    # the capital up to day 1; B_0 = 1000 (1 - 1/4) = 750; day 2: 1500; day 3: P = 750 * 4 = 3000, w_old = (1 * 4) / 4 = 1, tau = 1/2
    assert r["value"].tolist() == [[1000.0, 750.0, 1500.0, 3000.0 * (1.0 - 0.25 * 0.5)]]
    assert r["holdings"].tolist() == [[0.0, 1.0, 1.0, 0.5]]
    assert r["turnover"].tolist() == [[1.0, 0.5]]


def test_a_ruined_book_and_its_first_nonpositive_day():
    # short 2x a stock that doubles: G = 3 - 2 * 2 = -1 on day 2; the second portfolio survives; the third is NaN from day 3 on
    price = [[1.0, 1.25, 2.0, 1.0], [1.0, 1.0, 1.0, 1.0]]
    r = run([[[-2.0], [0.0]], [[-0.25], [0.0]], [[-1.0], [0.0]]], price, [0])
    assert r["value"][0].tolist() == [1000.0, 500.0, -1000.0, 1000.0] and r["value"][1].tolist() == [1000.0, 937.5, 750.0, 1000.0]
    assert r["first_nonpositive"].tolist() == [2, -1, 2]                        # the third: G = 2 - 2 = 0 on day 2
    assert r["net"].tolist() == [[-2.0], [-0.25], [-1.0]] and r["gross"].tolist() == [[2.0], [0.25], [1.0]]
    # after a wipe-out at a rebalance day the drifted weights divide by G = 0: the NaN stays, and is found
    r = run([[[-1.0, -1.0], [0.0, 0.0]]], price, [0, 2])
    assert r["first_nonpositive"].tolist() == [2] and np.isnan(r["value"][0, 3]) and not W.isnull(r["value"]).any()


def test_holdings_on_and_between_the_rebalance_days():
    price = [[4.0, 8.0, 8.0, 4.0], [8.0, 4.0, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0]]
    r = run([[[0.5, 0.25], [-0.25, 0.5], [NULL, NULL]]], price, [0, 2], holdings_of=0)
    h = r["holdings"]
    assert h[:, 0].tolist() == [0.5, -0.25, 0.0] and h[:, 2].tolist() == [0.25, 0.5, 0.0]
    assert h[:, 1].tolist() == [1.0 / 1.625, -0.125 / 1.625, 0.0]
    assert h[:, 3].tolist() == [0.125 / (0.25 + (0.0 + 0.125 + 0.5)), 0.5 / (0.25 + (0.0 + 0.125 + 0.5)), 0.0]
    # net exposure plus cash over G is one: the holdings and the cash weight sum to 1
    assert h[:, 1].sum() + 0.75 / 1.625 == 1.0


def test_bad_arguments_of_the_restatement():
    for days in ([1, 1], [2, 1], [3], [-1]):
        with pytest.raises(ValueError):
            run([np.zeros((1, len(days)))], [[1.0, 1.0, 1.0]], days)
    with pytest.raises(ValueError):
        run([np.zeros((1, 1))] * 9, [[1.0, 1.0, 1.0]], [0])


# ---------------------------------------------------------------- the two properties
def clean_prices(n, T, seed):
    rng = np.random.default_rng(seed)
    return 20.0 * np.exp(np.cumsum(0.03 * rng.standard_normal((n, T)), axis=1))


@pytest.mark.parametrize("n,members", [(64, 64), (520, 512)])
def test_property_i_equal_dyadic_weights_are_d27_bit_for_bit(n, members):
    """2^m members with clean prices and equal weights 1 / 2^m: W_k = 1.0 and c_k = 0.0 exactly, every step is pq_factor_portfolio's"""
    T, days = 70, [0, 9, 10, 33, 69]
    price = clean_prices(n, T, 5)
    labels = np.full((n, T), P.LABEL_OUT, dtype=np.uint8)
    w = np.full((n, len(days)), NULL)
    rng = np.random.default_rng(6)
    for k, d in enumerate(days):                                # other members at every rebalance
        who = rng.permutation(n)[:members]
        labels[who, d] = 0
        w[who, k] = 1.0 / members
    exp = P.portfolio(labels, price, 1, days, None, 0, 0.003, 1_000_000.0)
    got = W.weights([w], price, days, 0.003, 1_000_000.0)
    assert (got["net"] == 1.0).all() and (got["n_long"] == members).all() and (got["n_long"] == exp["count"]).all()
    same(got["turnover"], exp["turnover"], "turnover")
    same(got["value"], exp["value"], "value")


def dyadic_case(n, T, seed):
    """weights that are multiples of 1/64 in [-1, 1], base prices that are powers of two and later prices that are small multiples of
    1/4 of them: every ratio, product and partial sum is a multiple of 2^-8 below 2^12, so every operation of L, W and G is exact"""
    rng = np.random.default_rng(seed)
    w = rng.integers(-64, 65, (n, 1)) / 64.0
    w[rng.random((n, 1)) < 0.1] = NULL
    base = 2.0 ** rng.integers(-2, 4, (n, 1))
    price = base * (rng.integers(1, 13, (n, T)) / 4.0)
    price[:, :1] = base
    return w, price


@pytest.mark.parametrize("n,T", [(37, 9), (300, 5)])
def test_property_ii_linearity(n, T):
    """Doubling every weight doubles net, gross and turnover[.][0] (= gross_0) exactly and leaves the counts; on the dyadic case, with one
    rebalance, no fee and capital 1.0 the curve is G itself and G - 1.0 doubles exactly.  Later turnovers and the chain are not linear
    (the drifted weights divide by G) and are not pinned."""
    w, price = dyadic_case(n, T, 11)
    a = W.weights([w, 2.0 * w], price, [0], 0.0, 1.0)
    for k in ("net", "gross", "turnover"):
        same(a[k][1], 2.0 * a[k][0], k)
    for k in ("n_long", "n_short", "n_dropped"):
        assert (a[k][0] == a[k][1]).all()
    same(a["value"][1] - 1.0, 2.0 * (a["value"][0] - 1.0), "G - 1")
    assert len(set(a["value"][0].tolist())) > 2
    # and on ordinary inputs the exposures still double exactly
    rng = np.random.default_rng(12)
    w, price = rng.standard_normal((n, 2)), clean_prices(n, T, 13)
    b = W.weights([w, 2.0 * w], price, [0, T // 2], 0.001, 1000.0)
    same(b["net"][1], 2.0 * b["net"][0], "net")
    same(b["gross"][1], 2.0 * b["gross"][0], "gross")
    same(b["turnover"][1, 0], 2.0 * b["turnover"][0, 0], "turnover_0")


# ---------------------------------------------------------------- against plain share accounting
def share_accounting(w, price, days, cost, capital):
    """day by day in shares: at a rebalance the book is valued at the day's prices, the fee is cost times the traded value -- the sum of
    |target value - held value| with the targets sized on the pre-trade value --, and the new shares are w B / price with the rest in cash"""
    N, T = price.shape
    shares, cash = np.zeros(N), capital
    value = np.full(T, capital)
    k = 0
    for t in range(T):
        v = cash + float(np.sum(shares * price[:, t]))
        if k < len(days) and t == days[k]:
            traded = float(np.sum(np.abs(w[:, k] * v - shares * price[:, t])))
            v -= cost * traded
            shares = w[:, k] * v / price[:, t]
            cash = v - float(np.sum(shares * price[:, t]))
            k += 1
        value[t] = v
    return value


SHARE_TOL = 1e-13   # 64 x the worst relative deviation measured on the development host (3.88e-16), rounded up to a power of ten


@pytest.mark.parametrize("N,T,R", [(40, 60, 6), (300, 131, 7)])
def test_against_share_accounting(N, T, R):
    """Long-short weights with gross <= 2 and clean prices: the closed form (growth per segment, the chain) against shares and cash carried
    day by day.  Measured on the development host: the worst relative deviation of value is 3.65e-16 at (40, 60, 6) and 3.88e-16 at
    (300, 131, 7); allowed: 64 x the larger, rounded up to a power of ten (D-28's convention)."""
    rng = np.random.default_rng(100 + N)
    price = clean_prices(N, T, 200 + N)
    days = sorted(rng.choice(np.arange(1, T - 1), R, replace=False).tolist())
    w = rng.standard_normal((N, R))
    w *= rng.uniform(0.5, 2.0, R) / np.abs(w).sum(axis=0)
    got = W.weights([w], price, days, 0.002, 1_000_000.0)
    assert (got["gross"] <= 2.0 + 1e-12).all() and (got["n_short"] > 0).all() and (got["n_dropped"] == 0).all()
    exp = share_accounting(w, price, days, 0.002, 1_000_000.0)
    dev = float(np.max(np.abs(got["value"][0] - exp) / np.abs(exp)))
    print(f"share accounting {(N, T, R)}: worst relative deviation {dev:.3g}")
    assert dev <= SHARE_TOL


# ---------------------------------------------------------------- api.factor_weights' checks that need no device
ONES = np.ones((6, 10))
W2 = np.zeros((6, 2))


@pytest.mark.parametrize("call, msg", [
    (lambda a: a.factor_weights(np.zeros(6), ONES, [0, 1]), r"weights must be one \[N, R\] array"),
    (lambda a: a.factor_weights(np.zeros((1, 1, 6, 2)), ONES, [0, 1]), r"weights must be one \[N, R\] array"),
    (lambda a: a.factor_weights([], ONES, [0, 1]), "number of portfolios"),
    (lambda a: a.factor_weights([W2] * 9, ONES, [0, 1]), "number of portfolios"),
    (lambda a: a.factor_weights(np.zeros((9, 6, 2)), ONES, [0, 1]), "number of portfolios"),
    (lambda a: a.factor_weights(W2, np.ones(10), [0, 1]), r"price must be \[N, T\]"),
    (lambda a: a.factor_weights(W2, ONES, [0.5, 1.0]), "integer day indices"),
    (lambda a: a.factor_weights(W2, ONES, [0, 10]), r"must lie in \[0, T\)"),
    (lambda a: a.factor_weights(W2, ONES, [-1, 3]), r"must lie in \[0, T\)"),
    (lambda a: a.factor_weights(W2, ONES, [3, 3]), "strictly ascending"),
    (lambda a: a.factor_weights(W2, ONES, [4, 3]), "strictly ascending"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1, 2]), "weights 0 must be"),
    (lambda a: a.factor_weights([W2, np.zeros((5, 2))], ONES, [0, 1]), "weights 1 must be"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], cost_rate=-0.001), "cost_rate"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], cost_rate=1.0), "cost_rate"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], cost_rate=float("nan")), "cost_rate"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], initial_capital=0.0), "initial_capital"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], initial_capital=float("inf")), "initial_capital"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], initial_capital=float("nan")), "initial_capital"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], holdings_of=1), "holdings_of"),
    (lambda a: a.factor_weights([W2, W2], ONES, [0, 1], holdings_of=-1), "holdings_of"),
    (lambda a: a.factor_weights(W2, ONES, [0, 1], holdings_of=0.0), "holdings_of"),
])
def test_argument_refusals_without_a_device(call, msg):
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(api)


def test_factor_method_refusals_without_a_device():
    import polars_quant_amd as pq
    fac = pq.Factor()
    with pytest.raises(ValueError, match="days is needed"):
        fac.weights_backtest(W2, ONES)
    with pytest.raises(ValueError, match="lag"):
        fac.weights_backtest(W2, ONES, [0, 1], lag=-1)
    with pytest.raises(ValueError, match="integer day indices"):
        fac.weights_backtest(W2, ONES, [0.0, 1.0])
    with pytest.raises(ValueError, match="one column per day"):
        fac.weights_backtest(W2, ONES, [0, 1, 2])
    with pytest.raises(ValueError, match="strictly ascending"):
        fac.weights_backtest({"weights": W2, "days": np.array([3, 3])}, ONES)
    with pytest.raises(ValueError, match="holdings_of"):
        fac.weights_backtest(W2, ONES, [0, 1], holdings=2)


# ---------------------------------------------------------------- the kernels' resources
def test_no_kernel_uses_scratch():
    """The build writes the register / scratch figures of csrc/portfolio/weights.hip (weights.resources.txt, from hipcc's
    kernel-resource-usage remarks): the rebalance, growth and turnover passes in their size classes <1>, <2>, <8>, the two ends of
    first_nonpositive, the plain kernels and D-27's chain, none with scratch or a spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "portfolio" / "weights.resources.txt"
    if not path.exists():
        pytest.skip("csrc/portfolio/weights.resources.txt is not built")
    found = re.findall(r"Function Name: \S*?\d+(p[wf]_\w+?_kernel)(?:IL[ib](\d+)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [(k, c) for k in ("pw_rebalance_partial_kernel", "pw_growth_partial_kernel", "pw_turnover_partial_kernel") for c in ("1", "2", "8")]
    want += [("pw_first_kernel", "0"), ("pw_first_kernel", "1")]
    want += [(k, "") for k in ("pw_sum_blocks_kernel", "pw_growth_combine_kernel", "pw_curve_kernel", "pw_holdings_kernel", "pf_chain_kernel")]
    assert sorted((k, c) for k, c, *_ in found) == sorted(want)
    for k, c, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, c, vgprs, scratch, occ, spill)
