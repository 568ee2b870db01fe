"""not-gpu: decision D-18 (IC decay, sub-period and sub-group tests).  The public surface and its argument checks, which run before any
device work, and the restatement in tests/xsec_robust_ref.py pinned against hand-derived answers, scipy.stats.pearsonr / spearmanr per
day and scipy.stats.ttest_1samp for the summary rows."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

import xsec_robust_ref as R

ROOT = Path(__file__).resolve().parent.parent


def data(n, T, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, T))
    r = 0.1 * f + rng.standard_normal((n, T))
    r[rng.random((n, T)) < 0.05] = R.NULL
    f[rng.random((n, T)) < 0.03] = np.nan
    return f, r


# ---------------------------------------------------------------- public surface
def test_factor_methods_and_signatures():
    import polars_quant_amd as pq
    F = pq.Factor
    sig = lambda m: [(p.name, p.default) for p in inspect.signature(getattr(F, m)).parameters.values()][1:]
    e = inspect.Parameter.empty
    assert sig("ic_decay") == [("factor", e), ("next_return", e), ("max_lag", 10), ("method", "pearson")]
    assert sig("subsample_test") == [("factor", e), ("next_return", e), ("n_splits", 3), ("method", "pearson"), ("dates", None)]
    assert sig("subgroup_test") == [("factor", e), ("next_return", e), ("group", e), ("method", "pearson")]
    from polars_quant_amd import api
    for name in ("ic_decay", "ic_subgroup", "series_split_summary", "split_periods"):
        assert callable(getattr(api, name)), name


def test_header_declares_the_new_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pq_hip.h").read_text(), flags=re.S)
    for sym in ("pq_ic_decay", "pq_ic_subgroup", "pq_series_split_summary"):
        assert re.search(rf"\b{sym}\s*\(", txt), sym
    for macro, v in (("PQ_IC_DECAY_MAX_LAG", 256), ("PQ_IC_MAX_GROUPS", 256), ("PQ_IC_SUMMARY_COLS", 5)):
        assert re.search(rf"#define {macro} {v}\b", txt), macro


BAD_CALLS = [
    ("ic_decay", dict(max_lag=0)),
    ("ic_decay", dict(max_lag=257)),
    ("ic_decay", dict(max_lag=2.5)),
    ("ic_decay", dict(method="kendall")),
    ("subsample_test", dict(n_splits=0)),
    ("subsample_test", dict(n_splits=9)),
    ("subsample_test", dict(method="rank")),
    ("subsample_test", dict(dates=["a", "b"])),
    ("subgroup_test", dict(group=np.full(5, 256))),
    ("subgroup_test", dict(group=np.zeros(4, np.int32))),
    ("subgroup_test", dict(group=np.zeros((5, 3), np.int32))),
    ("subgroup_test", dict(group=np.zeros(5))),
    ("subgroup_test", dict(group=np.zeros(5, np.int32), method=None)),
]


@pytest.mark.parametrize("name,kw", BAD_CALLS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD_CALLS)])
def test_argument_errors_need_no_device(name, kw):
    """every argument error is a ValueError raised before any device work (without a GPU, device work raises PqError instead)"""
    import polars_quant_amd as pq
    f, r = data(5, 8, 1)
    kw = dict(kw)
    args = (f, r, kw.pop("group")) if name == "subgroup_test" else (f, r)
    with pytest.raises(ValueError):
        getattr(pq.Factor(), name)(*args, **kw)


@pytest.mark.parametrize("call", ["ic_decay", "ic_subgroup"])
def test_shape_errors_need_no_device(call):
    from polars_quant_amd import api
    f, r = data(5, 8, 2)
    extra = (np.zeros(5, np.int32),) if call == "ic_subgroup" else ()
    with pytest.raises(ValueError):
        getattr(api, call)(f, r[:, :7], *extra)
    with pytest.raises(ValueError):
        getattr(api, call)(f[0], r[0], *extra)
    with pytest.raises(ValueError):
        api.series_split_summary(np.zeros(4), 5)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("method", [0, 1])
def test_factor_equal_to_the_return_k_days_ahead(method):
    n, T, k = 30, 20, 3
    rng = np.random.default_rng(3)
    full = rng.standard_normal((n, T + k))
    f, r = full[:, k - 1:k - 1 + T].copy(), full[:, :T].copy()
    ic, nv, summ = R.ic_decay(f, r, k + 1, method)
    assert np.abs(ic[k - 1, :T - k + 1] - 1.0).max() < 1e-14
    assert (nv[k - 1, :T - k + 1] == n).all() and (nv[k - 1, T - k + 1:] == 0).all() and R.isnull(ic[k - 1, T - k + 1:]).all()
    assert summ[k - 1, 0] == T - k + 1 and abs(summ[k - 1, 1] - 1.0) < 1e-14


def test_two_group_day_by_hand():
    f = np.array([[1.0], [2.0], [3.0], [1.0], [2.0], [3.0], [5.0]])
    r = np.array([[1.0], [2.0], [4.0], [3.0], [2.0], [1.0], [9.0]])
    codes = np.array([0, 0, 0, 1, 1, 1, -1])
    ic, nv, summ = R.ic_subgroup(f, r, codes, 1)
    assert np.abs(ic[:, 0] - [1.0, -1.0]).max() < 1e-15 and nv[:, 0].tolist() == [3, 3]
    ic, nv, _ = R.ic_subgroup(f, r, codes, 0)
    assert abs(ic[0, 0] - stats.pearsonr([1, 2, 3], [1, 2, 4])[0]) < 1e-15 and abs(ic[1, 0] + 1.0) < 1e-15
    assert summ[:, 0].tolist() == [1.0, 1.0] and R.isnull(summ[:, 2]).all()   # one day: std / t / p NULL


def test_every_day_its_own_period():
    f, r = data(20, 9, 4)
    ic, _ = R._oracle().factor_ic(f, r, 0)
    s = R.series_split_summary(ic, 9)
    assert s[:, 0].tolist() == [1.0] * 9
    assert s[:, 1].tolist() == ic.tolist()
    assert R.isnull(s[:, 2:]).all()
    start, end = R.split_periods(9, 9)
    assert start.tolist() == end.tolist() == list(range(9))


def test_lag_above_t_is_an_empty_row():
    f, r = data(10, 4, 5)
    ic, nv, summ = R.ic_decay(f, r, 6, 0)
    assert R.isnull(ic[4:]).all() and (nv[4:] == 0).all()
    assert summ[4:, 0].tolist() == [0.0, 0.0] and R.isnull(summ[4:, 1:]).all()
    assert R.isnull(ic[3, 1:]).all() and not R.isnull(ic[3, 0])


@pytest.mark.parametrize("method", [0, 1])
def test_restatement_against_scipy(method):
    n, T, L = 60, 25, 4
    f, r = data(n, T, 6)
    ic, nv, summ = R.ic_decay(f, r, L, method)
    corr = stats.pearsonr if method == 0 else stats.spearmanr
    for l in range(1, L + 1):
        for t in range(T - l + 1):
            x, y = f[:, t], r[:, t + l - 1]
            m = R.valid(x) & R.valid(y)
            assert nv[l - 1, t] == m.sum()
            assert abs(ic[l - 1, t] - corr(x[m], y[m])[0]) < 1e-12
        row = ic[l - 1, :T - l + 1]
        tt = stats.ttest_1samp(row, 0.0)
        assert summ[l - 1, 0] == T - l + 1 and abs(summ[l - 1, 1] - row.mean()) < 1e-15
        assert abs(summ[l - 1, 2] - row.std(ddof=1)) < 1e-14
        assert abs(summ[l - 1, 3] - tt.statistic) < 1e-11 * abs(tt.statistic) + 1e-13
        assert abs(summ[l - 1, 4] - tt.pvalue) < 1e-11 * tt.pvalue + 1e-300
    codes = np.random.default_rng(7).integers(-1, 3, n)
    ic, nv, summ = R.ic_subgroup(f, r, codes, method)
    for g in range(3):
        for t in range(T):
            m = R.valid(f[:, t]) & R.valid(r[:, t]) & (codes == g)
            assert nv[g, t] == m.sum()
            assert abs(ic[g, t] - corr(f[m, t], r[m, t])[0]) < 1e-12
        tt = stats.ttest_1samp(ic[g], 0.0)
        assert abs(summ[g, 3] - tt.statistic) < 1e-11 * abs(tt.statistic) + 1e-13
