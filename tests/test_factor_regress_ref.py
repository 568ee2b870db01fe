"""not-gpu: known answers of the D-17 restatement (tests/xsec_regress_ref.py) on hand-derived days, the restatement against scipy's and
numpy's own regressions and t-tests, and the public surface of the regressions (Factor.ic_test / factor_return / fama_macbeth /
time_series_regression, api.xsec_regress / ts_regress / corr_t_test, the C declarations); argument errors are raised before any device
work."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

import xsec_regress_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL


def col(*v):
    return np.array(v, dtype=np.float64)[:, None]


def test_public_surface():
    from polars_quant_amd import api
    from polars_quant_amd.factor import Factor
    sig = {name: list(inspect.signature(getattr(Factor, name)).parameters) for name in
           ("ic_test", "factor_return", "fama_macbeth", "time_series_regression")}
    assert sig == {"ic_test": ["self", "factor", "next_return", "method"], "factor_return": ["self", "factor", "next_return"],
                   "fama_macbeth": ["self", "factors", "next_return"], "time_series_regression": ["self", "factors", "returns"]}
    assert inspect.signature(Factor.ic_test).parameters["method"].default == "pearson"
    assert not hasattr(Factor, "clean")
    for fn in ("xsec_regress", "ts_regress", "corr_t_test"):
        assert callable(getattr(api, fn))
    assert api.REGRESS_MAX_K == 8 and api.REGRESS_SUMMARY_COLS == 5
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pq_hip.h").read_text(), flags=re.S)
    assert re.search(r"pq_status pq_xsec_regress\(pq_ctx \*, const pq_batch \*, const double \*const \*factors, int32_t k, const double "
                     r"\*fwd_return, double \*coef,\s+double \*t_stat, double \*p_value, double \*r2, int32_t \*n_obs, double \*summary\);", hdr)
    assert re.search(r"pq_status pq_ts_regress\(pq_ctx \*, const pq_batch \*, const double \*const \*factors, int32_t k, uint32_t "
                     r"series_mask, const double \*ret,\s+double \*coef, double \*t_stat, double \*p_value, double \*r2, int32_t \*n_obs\);", hdr)
    assert re.search(r"pq_status pq_corr_t_test\(pq_ctx \*, const double \*corr, const int32_t \*n_valid, int64_t len, double \*t_stat, "
                     r"double \*p_value\);", hdr)
    assert re.search(r"#define PQ_REGRESS_MAX_K 8\b", hdr) and re.search(r"#define PQ_REGRESS_SUMMARY_COLS 5\b", hdr)


# ---- hand-derived days (dyadic data: every sum, mean and product below is exact)
def test_k1_slope_is_sfr_over_sff_exactly():
    f = col(1.0, 2.0, 3.0, 4.0, 6.0)
    r = col(0.5, 0.25, 1.0, 0.75, 1.5)
    out = R.xsec_regress([f], r)
    fb, rb = 16.0 / 5, 4.0 / 5
    sff = float(((f[:, 0] - fb) ** 2).sum())
    sfr = float(((f[:, 0] - fb) * (r[:, 0] - rb)).sum())
    assert out["coef"][0, 0] == sfr / sff
    assert out["coef"][1, 0] == rb - (sfr / sff) * fb
    assert out["n"][0] == 5
    assert 0.0 < out["r2"][0] < 1.0 and 0.0 < out["p"][0, 0] < 1.0


def test_perfect_fit_keeps_coef_and_nulls_t_and_p():
    f = col(1.0, 2.0, 3.0, 5.0)
    r = 0.5 * f + 0.25
    out = R.xsec_regress([f], r)
    assert out["coef"][0, 0] == 0.5 and out["coef"][1, 0] == 0.25
    assert out["r2"][0] == 1.0
    assert R.isnull(out["t"][:, 0]).all() and R.isnull(out["p"][:, 0]).all()


def test_collinear_factors_null_the_day():
    f0 = col(1.0, 2.0, 3.0, 4.0, 5.0)
    out = R.xsec_regress([f0, 2.0 * f0], col(1.0, 0.0, 2.0, 1.0, 3.0))
    for k in ("coef", "t", "p"):
        assert R.isnull(out[k][:, 0]).all(), k
    assert R.isnull(out["r2"][0]) and out["n"][0] == 5
    const = R.xsec_regress([np.full((5, 1), 3.0)], col(1.0, 0.0, 2.0, 1.0, 3.0))   # C[0][0] == 0
    assert R.isnull(const["coef"][:, 0]).all()


def test_sample_size_threshold_is_k_plus_2():
    f0, f1 = col(1.0, 2.0, 4.0, 7.0), col(0.5, -1.0, 2.0, 1.0)
    r = col(1.0, 3.0, 2.0, 5.0)
    for K in (1, 2):
        fs = [f0, f1][:K]
        small = R.xsec_regress([f[:K + 1] for f in fs], r[:K + 1])
        assert R.isnull(small["coef"]).all() and R.isnull(small["r2"]).all() and small["n"][0] == K + 1
        ok = R.xsec_regress([f[:K + 2] for f in fs], r[:K + 2])
        assert not R.isnull(ok["coef"]).any() and ok["n"][0] == K + 2


def test_constant_returns_null_r_squared():
    out = R.xsec_regress([col(1.0, 2.0, 3.0, 5.0)], np.full((4, 1), 0.75))
    assert out["coef"][0, 0] == 0.0 and out["coef"][1, 0] == 0.75
    assert R.isnull(out["r2"][0]) and R.isnull(out["t"][:, 0]).all()


def test_sample_excludes_null_nan_inf_in_any_column():
    f = col(1.0, 2.0, NULL, 4.0, 5.0, 6.0, np.inf)
    g = col(0.5, np.nan, 1.0, 2.0, 1.5, 3.0, 1.0)
    r = col(1.0, 2.0, 3.0, -np.inf, 0.5, 2.5, 1.0)
    out = R.xsec_regress([f, g], r)
    ref = R.xsec_regress([f[[0, 4, 5]], g[[0, 4, 5]]], r[[0, 4, 5]])
    assert out["n"][0] == 3 and R.isnull(out["coef"]).all() and R.isnull(ref["coef"]).all()
    out1 = R.xsec_regress([f], r)
    ref1 = R.xsec_regress([f[[0, 1, 4, 5]]], r[[0, 1, 4, 5]])
    assert out1["n"][0] == 4 and np.array_equal(out1["coef"].view(np.uint64), ref1["coef"].view(np.uint64))


def pivot_table(K, seed, n=40):
    """K factors and a return [n, K + 2] on which the first singular pivot of C = L D L^T sits at every position in turn -> day 0:
    f_0 constant (pivot 0 is 0); day j, 1 <= j < K: f_j = 2 f_{j-1} + 3 (pivot j is rounding noise behind j healthy ones, and every
    pivot after it is computed from that noise); day K: every factor scaled by 1e160, so C[0][0] overflows and the later pivots are
    NaN; day K + 1: untouched.  Every symbol is a member on every day."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, n, K + 2))
    r = (0.1 * np.arange(1, K + 1)[:, None, None] * F).sum(0) + 0.5 * rng.standard_normal((n, K + 2))
    F[0, :, 0] = 0.375
    for j in range(1, K):
        F[j, :, j] = 2.0 * F[j - 1, :, j] + 3.0
    F[:, :, K] *= 1e160
    return F, r


@pytest.mark.parametrize("K", [3, 8])
def test_failing_pivot_at_every_position(K):
    """a day is solved only when all K pivots pass: NULL coefficients on the days whose pivot 0 .. K-1 fails (an interior failure leaves
    later pivots that may well pass on their own) and on the overflow day, a solution on the untouched day"""
    F, r = pivot_table(K, 60 + K)
    out = R.xsec_regress(list(F), r)
    assert (out["n"] == 40).all()
    for k in ("coef", "t", "p"):
        assert R.isnull(out[k][:, :K + 1]).all(), k
    assert R.isnull(out["r2"][:K + 1]).all()
    assert np.isfinite(out["coef"][:, K + 1]).all() and np.isfinite(out["t"][:, K + 1]).all() and np.isfinite(out["r2"][K + 1])
    ts = R.ts_regress([f.T for f in F], r.T)                      # the same table with the days as symbols
    assert R.isnull(ts["coef"][:K + 1]).all() and np.isfinite(ts["coef"][K + 1]).all() and (ts["n"] == 40).all()


# ---- against scipy / numpy
def test_k1_against_linregress():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((400, 6))
    r = 0.3 * f + rng.standard_normal((400, 6))
    out = R.xsec_regress([f], r)
    for t in range(6):
        lr = stats.linregress(f[:, t], r[:, t])
        np.testing.assert_allclose(out["coef"][0, t], lr.slope, rtol=1e-12)
        np.testing.assert_allclose(out["coef"][1, t], lr.intercept, rtol=1e-12)
        np.testing.assert_allclose(out["coef"][0, t] / out["t"][0, t], lr.stderr, rtol=1e-12)
        np.testing.assert_allclose(out["coef"][1, t] / out["t"][1, t], lr.intercept_stderr, rtol=1e-12)
        np.testing.assert_allclose(out["r2"][t], lr.rvalue ** 2, rtol=1e-12)
        np.testing.assert_allclose(out["p"][0, t], lr.pvalue, rtol=1e-12)


@pytest.mark.parametrize("K", range(1, 9))
def test_against_lstsq_and_inverse_normal_equations(K):
    rng = np.random.default_rng(10 + K)
    n, T = 300, 4
    F = rng.standard_normal((K, n, T))
    r = (np.arange(1, K + 1)[:, None, None] * 0.1 * F).sum(0) + rng.standard_normal((n, T))
    out = R.xsec_regress(list(F), r)
    for t in range(T):
        X = np.column_stack([F[j][:, t] for j in range(K)] + [np.ones(n)])
        beta, res, _, _ = np.linalg.lstsq(X, r[:, t], rcond=None)
        s2 = res[0] / (n - K - 1)
        se = np.sqrt(np.diag(np.linalg.inv(X.T @ X)) * s2)
        np.testing.assert_allclose(out["coef"][:, t], beta, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(out["coef"][:, t] / out["t"][:, t], se, rtol=1e-10)
        np.testing.assert_allclose(out["p"][:, t], 2 * stats.t.sf(np.abs(beta / se), n - K - 1), rtol=1e-9)
        rc = r[:, t] - r[:, t].mean()
        np.testing.assert_allclose(out["r2"][t], 1.0 - res[0] / (rc @ rc), rtol=1e-10)


@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_time_series_form_against_lstsq(K):
    """per-symbol OLS on the symbol's sample, with [T] series at j = 0 and j = K - 1 (one with NULL days) among [N, T] factors"""
    rng = np.random.default_rng(40 + K)
    N, T = 5, 700
    cols = [rng.standard_normal((N, T)) for _ in range(K)]
    cols[0] = rng.standard_normal(T)
    cols[K - 1] = rng.standard_normal(T) + 0.5 * cols[0]
    r = sum(0.1 * (j + 1) * np.broadcast_to(c, (N, T)) for j, c in enumerate(cols)) + rng.standard_normal((N, T))
    cols[0][::13] = NULL
    cols[2][3, ::7] = np.nan
    r[1, ::5] = NULL
    r[4, 3] = np.inf
    out = R.ts_regress(cols, r)
    for s in range(N):
        Xs = np.column_stack([np.broadcast_to(c, (N, T))[s] for c in cols] + [np.ones(T)])
        ok = np.isfinite(Xs).all(axis=1) & np.isfinite(r[s])
        X, y = Xs[ok], r[s][ok]
        n = len(y)
        beta, res, _, _ = np.linalg.lstsq(X, y, rcond=None)
        s2 = res[0] / (n - K - 1)
        se = np.sqrt(np.diag(np.linalg.inv(X.T @ X)) * s2)
        assert out["n"][s] == n, s
        np.testing.assert_allclose(out["coef"][s], beta, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(out["coef"][s] / out["t"][s], se, rtol=1e-10)
        np.testing.assert_allclose(out["p"][s], 2 * stats.t.sf(np.abs(beta / se), n - K - 1), rtol=1e-9)
        yc = y - y.mean()
        np.testing.assert_allclose(out["r2"][s], 1.0 - res[0] / (yc @ yc), rtol=1e-10)


def test_ill_conditioned_day_against_mpmath():
    """K = 5 with two factors correlated at rho ~ 0.999 and one of mean 1e6, sd 1: the slopes against the exact least-squares solution of
    the same f64 data (mpmath, 50 digits) within 1e-14 * kappa_2(C) * |b|_inf, C the centred cross-product matrix"""
    import mpmath
    rng = np.random.default_rng(21)
    n, K = 400, 5
    F = rng.standard_normal((K, n))
    F[1] = 0.999 * F[0] + np.sqrt(1.0 - 0.999 ** 2) * F[1]
    F[2] = 1e6 + F[2]
    r = 0.3 * F[0] - 0.2 * F[1] + 0.05 * (F[2] - 1e6) + 0.1 * F[3] - 0.4 * F[4] + 0.5 * rng.standard_normal(n)
    out = R.xsec_regress([f[:, None] for f in F], r[:, None])
    with mpmath.workdps(50):
        cols = [[mpmath.mpf(float(v)) for v in f] for f in F]
        ys = [mpmath.mpf(float(v)) for v in r]
        means = [mpmath.fsum(c) / n for c in cols]
        ybar = mpmath.fsum(ys) / n
        dc = [[v - m for v in c] for c, m in zip(cols, means)]
        dy = [v - ybar for v in ys]
        C = mpmath.matrix(K, K)
        c = mpmath.matrix(K, 1)
        for j in range(K):
            c[j] = mpmath.fsum(a * b for a, b in zip(dc[j], dy))
            for k in range(K):
                C[j, k] = mpmath.fsum(a * b for a, b in zip(dc[j], dc[k]))
        b = mpmath.lu_solve(C, c)
        exact = np.array([float(b[j]) for j in range(K)])
        sv = mpmath.svd_r(C, compute_uv=False)
        kappa = float(max(sv) / min(sv))
    got = out["coef"][:K, 0]
    err = float(np.abs(got - exact).max())
    ratio = err / (kappa * float(np.abs(exact).max()))
    assert kappa > 1e3, kappa
    assert ratio <= 1e-14, f"|db|_inf / (kappa_2(C) |b|_inf) = {ratio:.3e} (kappa {kappa:.3e}, |db|_inf {err:.3e})"


def test_time_series_form_transposes_the_units():
    rng = np.random.default_rng(3)
    N, T = 5, 600
    mkt = rng.standard_normal(T)
    g = rng.standard_normal((N, T))
    r = 1.2 * mkt + 0.5 * g + rng.standard_normal((N, T))
    r[1, ::7] = NULL
    out = R.ts_regress([mkt, g], r)
    assert out["coef"].shape == (N, 3) and out["r2"].shape == (N,)
    for s in range(N):
        one = R.xsec_regress([mkt[:, None], g[s][:, None]], r[s][:, None])
        assert np.array_equal(out["coef"][s].view(np.uint64), one["coef"][:, 0].view(np.uint64))
        assert out["n"][s] == one["n"][0]
    assert out["n"][1] == T - len(range(0, T, 7))


def test_fama_macbeth_summary_against_ttest_1samp():
    rng = np.random.default_rng(8)
    coef = rng.standard_normal((3, 40)) * 0.1 + np.array([[0.05], [-0.02], [0.0]])
    coef[1, 5] = NULL
    coef[2, ::3] = NULL
    s = R.fm_summary(coef)
    for j in range(3):
        x = coef[j][~R.isnull(coef[j])]
        tt = stats.ttest_1samp(x, 0.0)
        assert s[j, 0] == len(x)
        np.testing.assert_allclose(s[j, 1], x.mean(), rtol=1e-13)
        np.testing.assert_allclose(s[j, 2], x.std(ddof=1), rtol=1e-13)
        np.testing.assert_allclose(s[j, 3], tt.statistic, rtol=1e-12)
        np.testing.assert_allclose(s[j, 4], tt.pvalue, rtol=1e-11)
    few = R.fm_summary(np.array([[NULL, 0.5, NULL], [NULL, NULL, NULL], [0.25, 0.25, 0.25]]))
    assert few[0, 0] == 1 and few[0, 1] == 0.5 and R.isnull(few[0, 2:]).all()
    assert few[1, 0] == 0 and R.isnull(few[1, 1:]).all()
    assert few[2, 1] == 0.25 and R.isnull(few[2, 2:]).all()     # std == 0


def test_ic_test_against_pearsonr():
    rng = np.random.default_rng(9)
    for n in (3, 4, 30, 500):
        f = rng.standard_normal(n)
        r = 0.2 * f + rng.standard_normal(n)
        ic = np.corrcoef(f, r)[0, 1]
        t, p = R.corr_t_test(np.array([ic]), np.array([n]))
        np.testing.assert_allclose(p[0], stats.pearsonr(f, r).pvalue, rtol=1e-9)
        np.testing.assert_allclose(t[0], ic * np.sqrt((n - 2) / (1 - ic * ic)), rtol=0)
    t, p = R.corr_t_test(np.array([np.nan, 0.5, 1.0, -1.0, 0.0]), np.array([10, 2, 10, 10, 10]))
    assert R.isnull(t[:4]).all() and R.isnull(p[:4]).all()
    assert t[4] == 0.0 and p[4] == 1.0


# ---- argument errors before any device work
def test_argument_errors():
    from polars_quant_amd import api
    from polars_quant_amd.factor import Factor
    f = np.zeros((4, 6))
    with pytest.raises(ValueError, match="1..8"):
        api.xsec_regress([], f)
    with pytest.raises(ValueError, match="1..8"):
        api.ts_regress([f] * 9, f)
    with pytest.raises(ValueError, match="1..8"):
        Factor().fama_macbeth(np.zeros((9, 4, 6)), f)
    with pytest.raises(ValueError, match="shape"):
        api.xsec_regress([np.zeros((4, 5))], f)
    with pytest.raises(ValueError, match="shape"):
        api.xsec_regress([np.zeros(6)], f)              # a [T] series only in the time-series form
    with pytest.raises(ValueError, match="shape"):
        api.ts_regress([np.zeros(5)], f)
    with pytest.raises(ValueError, match=r"\[N, T\]"):
        api.xsec_regress([f], np.zeros(6))
    with pytest.raises(ValueError, match="method"):
        Factor().ic_test(f, f, method="kendall")
