"""not-gpu: known answers of the D-16 restatement (tests/xsec_clean_ref.py) on tiny hand-derived days, the restatement against numpy's
own median / quantile / least squares, and the public surface of factor cleaning (pq.clean, api.factor_clean, the C declaration);
argument errors are raised before any device work."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_clean_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL


def col(*v):
    return np.array(v, dtype=np.float64)[:, None]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# README.md:277-282: factor [1.5, 2.3, 10.0, 1.8, 2.1], market caps, industries 金融 / 科技 / 金融 / 科技 / 消费 -> codes 0 1 0 1 2
README_F = col(1.5, 2.3, 10.0, 1.8, 2.1)
README_CAP = col(100.0, 200.0, 150.0, 300.0, 250.0)
README_IND = np.array([0, 1, 0, 1, 2])


def test_readme_known_answer_mad():
    b = R.order_bounds(README_F[:, 0], "mad", 3.0)
    assert b["med"] == 2.1
    assert b["mad"] == abs(1.8 - 2.1) and abs(b["mad"] - 0.3) < 1e-15
    c = 3.0 * 1.4826
    assert b["lo"] == 2.1 - c * b["mad"] and b["hi"] == 2.1 + c * b["mad"]
    assert abs(b["hi"] - 3.43434) < 1e-5 and abs(b["lo"] - 0.76566) < 1e-5
    out = R.clean(README_F, "mad")[:, 0]
    assert out[2] == b["hi"]                                    # only 10.0 is clipped
    assert bits(out[[0, 1, 3, 4]]).tolist() == bits(README_F[[0, 1, 3, 4], 0]).tolist()


def test_readme_single_member_industry_is_exactly_zero():
    out = R.clean(README_F, "mad", industry=README_IND)[:, 0]
    assert out[4] == 0.0                                        # industry 2 holds only the fifth symbol
    hi = R.order_bounds(README_F[:, 0], "mad", 3.0)["hi"]
    assert out[0] == 1.5 - (1.5 + hi) / 2 and out[2] == hi - (1.5 + hi) / 2
    assert out[1] == 2.3 - (2.3 + 1.8) / 2 and out[3] == 1.8 - (2.3 + 1.8) / 2
    z = np.log(README_CAP)
    full = R.clean(README_F, "mad", z=z, industry=README_IND, standardize=True)[:, 0]
    assert not R.isnull(full).any()
    assert abs(full.mean()) < 1e-15 and abs(full.std(ddof=1) - 1.0) < 1e-15


def test_median_odd_and_even():
    assert R.order_bounds([5.0, 1.0, 3.0], "mad", 3.0)["med"] == 3.0
    b = R.order_bounds([4.0, 1.0, 3.0, 2.0], "mad", 3.0)
    assert b["med"] == 2.5 and b["mad"] == 1.0                  # deviations 1.5 0.5 0.5 1.5
    b = R.order_bounds([1.0, 2.0, 4.0, 8.0, 100.0], "mad", 1.0)
    assert b["med"] == 4.0 and b["mad"] == 3.0                  # deviations 3 2 0 4 96
    assert b["lo"] == 4.0 - 1.4826 * 3.0 and b["hi"] == 4.0 + 1.4826 * 3.0


def test_zero_mad_day_is_not_clipped():
    f = col(1.0, 1.0, 1.0, 1.0, 50.0)
    b = R.order_bounds(f[:, 0], "mad", 3.0)
    assert b["mad"] == 0.0 and b["lo"] == -np.inf and b["hi"] == np.inf
    assert R.clean(f, "mad")[:, 0].tolist() == [1.0, 1.0, 1.0, 1.0, 50.0]


def test_percentile_bounds():
    f = col(*range(11))                                         # 0 .. 10
    assert R.clean(f, "percentile", 0.0)[:, 0].tolist() == list(range(11))   # p = 0: min and max
    b = R.order_bounds(f[:, 0], "percentile", 5.0)              # h = 0.05 * 10 = 0.5
    assert b["lo"] == 0.0 + 0.5 * (1.0 - 0.0) and b["hi"] == 9.0 + (0.95 * 10 - 9.0) * (10.0 - 9.0)
    assert R.clean(f, "percentile", 5.0)[[0, 5, 10], 0].tolist() == [b["lo"], 5.0, b["hi"]]
    b = R.order_bounds([3.0, 1.0, 2.0, 4.0, 5.0], "percentile", 25.0)   # h = 1.0 and 3.0: g = 0
    assert (b["lo"], b["hi"]) == (2.0, 4.0)


def test_sigma_bounds():
    f = col(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0)
    m = 1.0
    sd = ((9 * (0.0 - m) * (0.0 - m) + (10.0 - m) * (10.0 - m)) / 9) ** 0.5
    out = R.clean(f, "sigma", 2.0)[:, 0]
    assert out[9] == m + 2.0 * sd and (out[:9] == 0.0).all()


def test_zero_regressor_variance_leaves_the_centred_factor():
    f = col(1.0, 2.0, 6.0)
    out = R.clean(f, z=col(5.0, 5.0, 5.0))[:, 0]
    assert out.tolist() == [1.0 - 3.0, 2.0 - 3.0, 6.0 - 3.0]


def test_size_residual_is_orthogonal_to_the_regressor():
    f = col(1.0, 2.0, 4.0, 8.0)
    z = col(1.0, 2.0, 3.0, 4.0)
    out, info = R.clean(f, z=z, parts=True)
    assert info["beta"][0] == (-1.5 * -3.75 + -0.5 * -2.75 + 0.5 * -0.75 + 1.5 * 3.25) / 5.0
    assert abs(out[:, 0] @ (z[:, 0] - 2.5)) < 1e-14 and abs(out[:, 0].sum()) < 1e-14


def test_constant_day_under_standardize_and_small_days_are_null():
    f = np.array([[2.0, 1.0, 7.0], [2.0, NULL, 8.0], [2.0, np.nan, 9.0]])
    out = R.clean(f, standardize=True)
    assert R.isnull(out[:, 0]).all()                            # std 0
    assert R.isnull(out[:, 1]).all()                            # n = 1
    assert out[:, 2].tolist() == [-1.0, 0.0, 1.0]
    assert R.isnull(R.clean(f)[:, 1]).all()                     # n = 1 without standardize too
    assert R.clean(f)[:, 0].tolist() == [2.0, 2.0, 2.0]


def test_cross_section_rules():
    f = col(1.0, 2.0, np.inf, 4.0, 5.0, 6.0, -np.inf)
    cap = col(1.0, 0.0, 1.0, -2.0, 1.0, NULL, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.log(cap)
    out = R.clean(f, z=z)[:, 0]
    assert R.isnull(out[[1, 2, 3, 5, 6]]).all()                 # log of cap <= 0, infinite factors, null cap
    assert out[0] == 1.0 - 3.0 and out[4] == 5.0 - 3.0          # both members at z = log 1 = 0: Szz = 0, beta = 0
    ind = np.array([0, -1, 0, 1, 1, 5, 0])
    out = R.clean(f, industry=ind, n_industries=2)[:, 0]
    assert R.isnull(out[[1, 2, 5, 6]]).all()                    # negative code, inf factor, code >= n_industries
    assert out[[0, 3, 4]].tolist() == [0.0, -0.5, 0.5]


def test_blocked_sum_order():
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(600) * 10.0 ** rng.integers(-8, 8, 600))[:, None]
    mem = rng.random((600, 1)) < 0.8
    blocks = []
    for b0 in range(0, 600, 256):
        s = 0.0
        for i in range(b0, min(b0 + 256, 600)):
            if mem[i, 0]:
                s += float(v[i, 0])
        blocks.append(s)
    expect = 0.0
    for s in blocks:
        expect += s
    assert bits(R.bsum(v, mem)[0]) == bits(expect)


def test_restatement_against_numpy():
    rng = np.random.default_rng(11)
    N, D = 301, 9
    f = rng.standard_normal((N, D)) * 2.0 + 0.5
    f[rng.random((N, D)) < 0.05] = NULL
    z = rng.standard_normal((N, D))
    for t in range(D):
        x = f[R.valid(f[:, t]), t]
        med = np.median(x)
        assert abs(R.order_bounds(x, "mad", 3.0)["med"] - med) <= 1e-15 * abs(med) + 1e-300
        assert abs(R.order_bounds(x, "mad", 3.0)["mad"] - np.median(np.abs(x - med))) <= 1e-14
        for wn in (0.0, 1.0, 2.5, 10.0, 49.9):
            b = R.order_bounds(x, "percentile", wn)
            q = np.quantile(x, [wn / 100.0, 1.0 - wn / 100.0], method="linear")
            assert abs(b["lo"] - q[0]) <= 1e-14 and abs(b["hi"] - q[1]) <= 1e-14
    out = R.clean(f, z=z)
    for t in range(D):
        m = R.valid(f[:, t])
        A = np.stack([np.ones(m.sum()), z[m, t]], axis=1)
        coef, *_ = np.linalg.lstsq(A, f[m, t], rcond=None)
        np.testing.assert_allclose(out[m, t], f[m, t] - A @ coef, rtol=0, atol=1e-12)
        assert R.isnull(out[~m, t]).all()
    st = R.clean(f, standardize=True)
    for t in range(D):
        m = R.valid(f[:, t])
        np.testing.assert_allclose(st[m, t], (f[m, t] - f[m, t].mean()) / f[m, t].std(ddof=1), rtol=0, atol=1e-12)


def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import api
    assert callable(pq.clean) and callable(api.factor_clean)
    params = list(inspect.signature(pq.clean).parameters)
    assert params[:8] == ["factor", "winsorize", "winsorize_n", "neutralize_market_cap", "cap", "neutralize_industry", "industry",
                          "standardize"]
    assert not hasattr(pq.Factor, "clean")                     # README's Factor.clean is orthogonalization, not this
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    decl = re.search(r"pq_status\s+pq_factor_clean\s*\(([^)]*)\)", txt)
    assert decl, "pq_factor_clean is not declared"
    names = [re.findall(r"\w+", a)[-1] for a in decl.group(1).split(",")]
    assert names == ["pq_ctx", "pq_batch", "factor", "winsorize", "winsorize_n", "cap_z", "industry", "n_industries", "standardize", "out"]
    assert "xsec/clean.hip" in (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()


@pytest.mark.parametrize("kw, msg", [
    (dict(winsorize="median"), "winsorize must be"),
    (dict(winsorize="percentile", winsorize_n=50.0), "percentile"),
    (dict(winsorize="percentile", winsorize_n=-1.0), "percentile"),
    (dict(winsorize="mad", winsorize_n=-1.0), "winsorize_n"),
    (dict(winsorize="sigma", winsorize_n=float("nan")), "winsorize_n"),
    (dict(neutralize_market_cap=True), "needs cap"),
    (dict(neutralize_industry=True), "needs industry"),
    (dict(neutralize_industry=True, industry=np.array([0, 1, 256])), "industry codes"),
    (dict(neutralize_industry=True, industry=np.array([0.5, 1.0, 2.0])), "integer"),
    (dict(neutralize_industry=True, industry=np.array([0j, 1j, 2j])), "integer"),
])
def test_argument_errors_raise_before_device_work(kw, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    with pytest.raises(ValueError, match=msg):
        pq.clean(np.ones((3, 4)), **kw)
