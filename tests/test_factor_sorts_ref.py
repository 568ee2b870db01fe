"""not-gpu: known answers of the D-15 restatement (tests/xsec_ref.py) on tiny hand-derived tables, and the public surface of the
quantile-sort / long-short / coverage / IC-statistics feature (C ABI declarations, Factor methods)."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
from scipy.stats import rankdata

import xsec_ref as X

ROOT = Path(__file__).resolve().parent.parent
OUT, MID = X.LABEL_OUT, X.LABEL_MID


def col(*v):
    return np.array(v, dtype=np.float64)[:, None]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_tie_across_a_bucket_edge_shares_the_upper_bucket():
    # 10 symbols, Q = 5: positions 0..9 map to buckets 0 0 1 1 2 2 3 3 4 4; the two 5.0s occupy [3, 5): m = 8, 8 * 5 // 20 = 2
    f = col(10, 9, 8, 7, 6, 5, 5, 3, 2, 1)
    r = col(*range(10)) / 8.0
    lab = X.labels(f, r, 0, 5)[:, 0]
    assert lab.tolist() == [4, 4, 3, 3, 2, 2, 2, 1, 0, 0]
    res = X.groups(f, r, 0, 5)
    assert res["count"][:, 0].tolist() == [2, 1, 3, 2, 2]
    assert res["mean_return"][2, 0] == (4 + 5 + 6) / 8.0 / 3
    assert res["spread"][0] == (0 + 1) / 8.0 / 2 - (8 + 9) / 8.0 / 2
    assert X.isnull(res["turnover"]).all()            # day 0


def test_day_with_fewer_symbols_than_quantiles_is_out_everywhere():
    f = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, X.NULL], [4.0, 4.0], [5.0, 5.0]])
    r = np.zeros_like(f)
    lab = X.labels(f, r, 0, 5)
    assert lab[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert (lab[:, 1] == OUT).all()                    # n = 4 < Q = 5
    res = X.groups(f, r, 0, 5)
    assert (res["count"][:, 1] == 0).all() and X.isnull(res["mean_return"][:, 1]).all() and X.isnull(res["spread"][1])


def test_null_return_removes_a_valid_factor_from_the_cross_section():
    f = col(1, 2, 3, 4, 5)
    r = col(0.1, X.NULL, 0.3, np.nan, 0.5)
    lab = X.labels(f, r, 0, 3)[:, 0]
    assert lab[1] == OUT and lab[3] == OUT
    assert lab[[0, 2, 4]].tolist() == [0, 1, 2]        # n = 3: m = 1, 3, 5 -> 3m // 6 = 0, 1, 2
    assert X.groups(f, r, 0, 3)["count"][:, 0].tolist() == [1, 1, 1]


def test_infinite_factor_values_are_not_in_the_cross_section():
    f = col(-np.inf, 1, 2, np.inf, 3, 4)
    lab = X.labels(f, np.ones_like(f), 0, 2)[:, 0]
    assert lab.tolist() == [OUT, 0, 0, OUT, 1, 1]


def test_signed_zeros_are_one_tie_run():
    f = col(0.0, -0.0, 1.0, -0.0, 2.0)
    # sorted: three zeros at [0, 3) -> m = 3; 1.0 -> m = 7; 2.0 -> m = 9; n = 5, Q = 2: 2m // 10
    assert X.labels(f, np.ones_like(f), 0, 2)[:, 0].tolist() == [0, 0, 1, 0, 1]
    assert X.labels(f, np.ones_like(f), 0, 5)[:, 0].tolist() == [1, 1, 3, 1, 4]


def test_long_short_legs_that_cover_the_whole_cross_section():
    f = col(5, 4, 3, 2, 1)
    # n = 5: m = 1, 3, 5, 7, 9 -> p = 0.1 .. 0.9; top = bottom = 0.5: the median (p = 0.5) is in neither leg
    assert X.labels(f, np.ones_like(f), 1, 0, 0.5, 0.5)[:, 0].tolist() == [1, 1, MID, 0, 0]
    f4 = col(4, 3, 2, 1)
    assert X.labels(f4, np.ones_like(f4), 1, 0, 0.3, 0.7)[:, 0].tolist() == [1, 0, 0, 0]
    assert X.labels(f4, np.ones_like(f4), 1, 0, 0.2, 0.2)[:, 0].tolist() == [1, MID, MID, 0]
    one = col(1.0, X.NULL)
    assert (X.labels(one, np.ones_like(one), 1, 0, 0.5, 0.5) == OUT).all()   # n = 1 < 2


def test_turnover_across_a_day_with_an_empty_bucket():
    # Q = 2, four symbols.  Day 0: distinct values; day 1: a constant factor -> m = 4 for all, 2 * 4 // 8 = 1: bucket 0 empty;
    # day 2: distinct again, in the opposite order from day 0
    f = np.array([[1.0, 7.0, 4.0], [2.0, 7.0, 3.0], [3.0, 7.0, 2.0], [4.0, 7.0, 1.0]])
    r = np.array([[0.5, 0.25, 1.0], [0.25, 0.5, 2.0], [1.0, 0.75, 4.0], [2.0, 1.0, 8.0]])
    res = X.groups(f, r, 0, 2)
    assert res["labels"].tolist() == [[0, 1, 1], [0, 1, 1], [1, 1, 0], [1, 1, 0]]
    assert res["count"].tolist() == [[2, 0, 2], [2, 4, 2]]
    tov = res["turnover"]
    assert X.isnull(tov[:, 0]).all()
    assert X.isnull(tov[0, 1]) and tov[1, 1] == 2 / 4          # bucket 0 empty on day 1; two newcomers in bucket 1
    assert X.isnull(tov[0, 2]) and tov[1, 2] == 0 / 2          # bucket 0 was empty the day before; bucket 1 kept symbols 0, 1
    assert X.isnull(res["mean_return"][0, 1]) and X.isnull(res["spread"][1])
    assert res["mean_return"][1, 2] == (1.0 + 2.0) / 2 and res["spread"][2] == 1.5 - 6.0 and res["spread"][0] == 1.5 - 0.375
    s = X.summary(res)
    assert s.shape == (3, 5)
    assert s[0, 0] == 2 and s[0, 1] == (0.375 + 6.0) / 2       # bucket 0 on days 0 and 2
    assert X.isnull(s[0, 4])                                    # no non-null turnover day
    assert s[1, 4] == (0.5 + 0.0) / 2 and X.isnull(s[2, 4])
    m = (1.125 + -4.5) / 2                                     # spread on days 0 and 2
    assert s[2, 0] == 2 and bits(s[2, 1]) == bits(m)
    assert s[2, 2] > 0.0 and bits(s[2, 3]) == bits(m / s[2, 2] * math.sqrt(252.0))


def test_block_order_of_the_cross_sectional_sum():
    # 600 symbols in one bucket: block sums of 256 / 256 / 88 symbols added in ascending order differ from a flat sum
    rng = np.random.default_rng(7)
    r = (rng.standard_normal(600) * 10.0 ** rng.integers(-8, 8, 600))[:, None]
    lab = np.zeros((600, 1), dtype=np.uint8)
    total, cnt, _ = X.group_sums(lab, r, 1)
    blocks = []
    for b0 in range(0, 600, 256):
        s = 0.0
        for v in r[b0:b0 + 256, 0].tolist():
            s += v
        blocks.append(s)
    expect = 0.0
    for s in blocks:
        expect += s
    assert bits(total[0, 0]) == bits(expect) and cnt[0, 0] == 600


def test_coverage_and_ic_stats():
    f = np.array([[1.0, X.NULL, np.nan], [np.inf, 2.0, 3.0], [1.0, 1.0, 1.0], [0.0, X.NULL, 1.0]])
    assert X.coverage(f).tolist() == [0.75, 0.5, 0.75]
    st = X.ic_stats(np.array([0.1, X.NULL, -0.05, 0.2, np.nan]))
    m = (0.1 + -0.05 + 0.2) / 3
    sd = (((0.1 - m) * (0.1 - m) + (-0.05 - m) * (-0.05 - m) + (0.2 - m) * (0.2 - m)) / 2) ** 0.5
    assert st[0] == 3 and st[1] == m and st[2] == sd and st[3] == m / sd and st[4] == 2 / 3
    one = X.ic_stats(np.array([0.3, X.NULL]))
    assert one[0] == 1 and X.isnull(one[1:]).all()
    flat = X.ic_stats(np.array([0.25, 0.25, 0.25]))
    assert flat[2] == 0.0 and X.isnull(flat[3]) and flat[4] == 1.0


def test_c_abi_declares_the_new_entry_points():
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    for fn in ("pq_factor_quantiles", "pq_factor_long_short", "pq_factor_coverage", "pq_ic_stats"):
        assert re.search(r"\b" + fn + r"\s*\(", txt), fn
    for k, v in (("PQ_LABEL_OUT", 255), ("PQ_LABEL_MID", 254), ("PQ_GROUP_SUMMARY_COLS", 5)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", txt), k


def test_factor_class_has_the_evaluation_methods():
    import polars_quant_amd as pq
    for m in ("quantile", "portfolio_sorts", "long_short", "factor_mimicking_portfolio", "turnover", "coverage", "ir", "ic_win_rate"):
        assert callable(getattr(pq.Factor, m, None)), m
    from polars_quant_amd import api
    for f in ("factor_quantiles", "factor_long_short", "factor_coverage", "ic_stats"):
        assert callable(getattr(api, f, None)), f


@pytest.mark.parametrize("q", [3, 7, 13])
def test_label_day_against_rankdata(q):
    """label_day's quantile buckets = floor((2 rank - 1) Q / (2 n_valid)) with scipy's average ranks over the valid pairs, in exact
    rationals, on tied and NULL-bearing days; every label is LABEL_OUT on a day with n_valid < Q"""
    rng = np.random.default_rng(q)
    for n, levels in ((40, 0), (40, 4), (257, 9), (600, 3), (q + 1, 2), (q, 0), (q - 1, 0)):
        f = rng.integers(-levels, levels + 1, n).astype(np.float64) if levels else rng.standard_normal(n)
        f[(f == 0.0) & (rng.random(n) < 0.5)] = -0.0
        r = rng.standard_normal(n)
        if n > 2 * q:
            f[rng.random(n) < 0.1] = X.NULL
            f[rng.random(n) < 0.05] = np.nan
            f[rng.random(n) < 0.03] = np.inf
            r[rng.random(n) < 0.05] = X.NULL
            r[rng.random(n) < 0.03] = -np.inf
        ok = np.isfinite(f) & np.isfinite(r)
        nv = int(ok.sum())
        lab = X.label_day(f, r, 0, q)
        assert (lab[~ok] == OUT).all()
        if nv < q:
            assert (lab == OUT).all()
            continue
        rank = rankdata(f[ok], method="average")
        exp = [math.floor(Fraction(int(2 * R - 1)) * q / (2 * nv)) for R in rank]
        assert lab[ok].tolist() == exp, (n, levels)
        if not levels:      # distinct values: every bucket is used
            assert set(exp) == set(range(q)), n
