"""not-gpu: the numpy restatement of decision D-27 (tests/factor_portfolio_ref.py) against answers derived by hand, one consistency
check against the restatement of D-15 (tests/xsec_ref.py), and the register / scratch figures of csrc/portfolio/portfolio.hip."""
import os
import re

import numpy as np
import pytest

import factor_portfolio_ref as P
import xsec_ref as X

OUT = P.LABEL_OUT


def run(labels, price, n_groups, days, **kw):
    kw.setdefault("initial_capital", 1000.0)
    return P.portfolio(np.asarray(labels, dtype=np.uint8), np.asarray(price, dtype=np.float64), n_groups, days, **kw)


def test_the_api_and_the_method_exist():
    """the restatement has something to restate: without the feature this fails"""
    from polars_quant_amd import api
    from polars_quant_amd.factor import Factor
    assert callable(api.factor_portfolio) and callable(Factor.portfolio_backtest)


def test_two_symbols_equal_weights_one_price_doubles():
    r = run([[0, 0, 0], [0, 0, 0]], [[10.0, 20.0, 20.0], [5.0, 5.0, 5.0]], 1, [0])
    # w = 0.5 each; G(1) = 0.5 * (20 / 10) + 0.5 * (5 / 5) = 1.5
    assert r["value"].tolist() == [[1000.0, 1500.0, 1500.0]]
    assert r["turnover"].tolist() == [[1.0]] and r["count"].tolist() == [[2]]


def test_the_first_rebalance_pays_the_fee_on_the_whole_capital():
    r = run([[0, 0, 0], [0, 0, 0]], [[10.0, 20.0, 20.0], [5.0, 5.0, 5.0]], 1, [0], cost_rate=0.25)
    # tau_0 = 1: B_0 = 1000 * (1 - 0.25 * 1) = 750
    assert r["value"].tolist() == [[750.0, 1125.0, 1125.0]]
    r = run([[0, 0, 0], [0, 0, 0]], [[10.0, 20.0, 20.0], [5.0, 5.0, 5.0]], 1, [0], cost_rate=0.001, initial_capital=1_000_000.0)
    assert r["value"][0, 0] == 1_000_000.0 * (1.0 - 0.001 * 1.0)


def test_a_null_price_is_carried_through_the_segment():
    r = run([[0, 0, 0, 0], [0, 0, 0, 0]], [[10.0, P.NULL, np.nan, 30.0], [5.0, 5.0, 0.0, 5.0]], 1, [0])
    # day 1: s0 keeps 10 -> G = 1; day 2: NaN and 0 are not usable either -> G = 1; day 3: 0.5 * 3 + 0.5 * 1 = 2
    assert r["value"].tolist() == [[1000.0, 1000.0, 1000.0, 2000.0]]


def test_an_empty_group_sits_in_cash_and_pays_to_enter():
    labels = [[0, 0, 1, 1], [0, 0, 0, 0]]
    price = [[10.0, 10.0, 10.0, 20.0], [5.0, 5.0, 5.0, 5.0]]
    r = run(labels, price, 2, [0, 2], cost_rate=0.25)
    # group 1: empty on day 0 (tau = 0, cash), buys s0 on day 2 (tau = 1): 1000, 1000, 750, 750 * (20 / 10)
    # group 0: s0 and s1 at 0.5 (tau = 1: 750); on day 2 s0 leaves, s1 goes from 0.5 to 1 (tau = 0.5 + 0.5): 750 * 0.75, flat after
    assert r["value"].tolist() == [[750.0, 750.0, 562.5, 562.5], [1000.0, 1000.0, 750.0, 1500.0]]
    assert r["turnover"].tolist() == [[1.0, 1.0], [0.0, 1.0]]
    assert r["count"].tolist() == [[2, 1], [0, 1]]


def test_unchanged_membership_trades_the_drift_only():
    r = run([[0, 0], [0, 0]], [[10.0, 30.0], [10.0, 10.0]], 1, [0, 1], cost_rate=0.5)
    # G(1) = 0.5 * 3 + 0.5 * 1 = 2; drifted weights 1.5 / 2 = 0.75 and 0.5 / 2 = 0.25 against 0.5 and 0.5: tau_1 = 0.5
    # B_0 = 1000 * (1 - 0.5) = 500; P_1 = 500 * 2 = 1000; B_1 = 1000 * (1 - 0.5 * 0.5) = 750
    assert r["turnover"].tolist() == [[1.0, 0.5]]
    assert r["value"].tolist() == [[500.0, 750.0]]


def test_cap_weights_drop_a_zero_and_a_null_weight():
    price = [[10.0, 20.0], [10.0, 10.0], [10.0, 1000.0], [10.0, 1000.0], [10.0, 1000.0], [10.0, 1000.0]]
    weight = [[3.0, 9.0], [1.0, 9.0], [0.0, 9.0], [P.NULL, 9.0], [-1.0, 9.0], [np.inf, 9.0]]
    r = run(np.zeros((6, 2)), price, 1, [0], weight=np.array(weight))
    # A = 4: w = 0.75 and 0.25; G(1) = 0.75 * 2 + 0.25 * 1 = 1.75
    assert r["count"].tolist() == [[2]] and r["turnover"].tolist() == [[1.0]]
    assert r["value"].tolist() == [[1000.0, 1750.0]]


def test_label_lag_reads_the_labels_of_the_day_before():
    r = run([[0, OUT, OUT], [OUT, 0, 0]], [[1.0, 2.0, 4.0], [1.0, 1.0, 1.0]], 1, [1], label_lag=1)
    # the rebalance of day 1 uses the labels of day 0: s0 alone, bought at 2, worth 4 on day 2
    assert r["count"].tolist() == [[1]]
    assert r["value"].tolist() == [[1000.0, 1000.0, 2000.0]]


def test_days_before_the_first_rebalance_hold_the_capital():
    r = run([[0, 0, 0, 0]], [[1.0, 2.0, 4.0, 6.0]], 1, [2], cost_rate=0.25)
    assert r["value"].tolist() == [[1000.0, 1000.0, 750.0, 1125.0]]
    r = run([[0, 0, 0, 0]], [[1.0, 2.0, 4.0, 6.0]], 3, [])
    assert r["value"].tolist() == [[1000.0] * 4] * 3 and r["turnover"].shape == (3, 0) and r["count"].shape == (3, 0)


def test_labels_outside_the_groups_belong_to_none():
    r = run([[P.LABEL_MID, 0], [OUT, 0], [2, 0], [1, 0]], [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 3.0]], 2, [0])
    assert r["count"].tolist() == [[0], [1]]
    assert r["value"].tolist() == [[1000.0, 1000.0], [1000.0, 3000.0]]


def test_bad_rebalance_days_are_refused():
    for days, lag in (([1, 1], 0), ([2, 1], 0), ([3], 0), ([-1], 0), ([0], 1)):
        with pytest.raises(ValueError):
            run([[0, 0, 0]], [[1.0, 1.0, 1.0]], 1, days, label_lag=lag)


def daily_rebalance_gap(n, T, q, seed):
    """largest |value[g][t + 1] / value[g][t] - 1 - mean_return[g][t]| over the days on which the bucket has members"""
    rng = np.random.default_rng(seed)
    price = 50.0 * np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))
    factor = rng.standard_normal((n, T))
    factor[rng.random((n, T)) < 0.05] = X.NULL
    nxt = np.full((n, T), X.NULL)
    nxt[:, :-1] = price[:, 1:] / price[:, :-1] - 1.0
    ref = X.groups(factor, nxt, 0, q)
    got = P.portfolio(ref["labels"], price, q, range(T), cost_rate=0.0)
    assert (got["count"] == ref["count"]).all()
    step = got["value"][:, 1:] / got["value"][:, :-1] - 1.0
    has = ref["count"][:, :-1] > 0
    assert has.sum() > q * (T - 1) // 2
    return float(np.abs(step - ref["mean_return"][:, :-1])[has].max())


def test_daily_rebalance_without_costs_is_the_quantile_mean_return():
    """Two restatements of one quantity: with a rebalance every day, equal weights and no fee, the portfolio of a bucket grows by the
    mean of its members' price ratios, and D-15's mean_return is the mean of their next-day simple returns.  They differ by rounding
    alone (the mean of p1 / p0 - 1 against the mean of p1 / p0, minus 1, and the curve's own product and quotient).  Measured on the
    CPU: the largest absolute difference is 3.51e-16 on (37, 50) and 4.93e-16 on (300, 131); the bound is 8 x the larger of the two."""
    gaps = [daily_rebalance_gap(37, 50, 5, 1), daily_rebalance_gap(300, 131, 5, 2)]
    print(gaps)
    assert max(gaps) <= 8 * 4.93e-16


def test_no_portfolio_kernel_uses_scratch():
    """The build writes the register / scratch figures of every kernel of csrc/portfolio/portfolio.hip (portfolio.resources.txt, from
    hipcc's kernel-resource-usage remarks): the three per-group passes in their four instantiations and the four plain kernels, none
    with scratch or a spilled VGPR."""
    path = os.path.join(os.path.dirname(__file__), "..", "polars_quant_amd", "csrc", "portfolio", "portfolio.resources.txt")
    if not os.path.exists(path):
        pytest.skip("portfolio.resources.txt not built (make -C polars_quant_amd/csrc)")
    found = re.findall(r"Function Name: \S*?(pf_\w+?_kernel)(?:ILi(\d+)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", open(path).read())
    want = [(k, g) for k in ("pf_weight_partial_kernel", "pf_growth_partial_kernel", "pf_turnover_partial_kernel")
            for g in ("2", "5", "10", "20")]
    want += [(k, "") for k in ("pf_sum_blocks_kernel", "pf_growth_combine_kernel", "pf_chain_kernel", "pf_curve_kernel")]
    assert sorted((k, g) for k, g, *_ in found) == sorted(want)
    for k, g, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, g, vgprs, scratch, occ, spill)
