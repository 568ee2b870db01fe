"""not-gpu: the numpy restatement of decision D-33 (tests/xsec_risk_ref.py: the weighted covariance of two windows, the factor
covariance and specific variance on as-of days, the portfolio's predicted risk) against an example derived by hand, one constructed
window per NULL rule, numpy.cov(aweights=) on fully valid windows, bit for bit against the restatement of ts_cov (tests/xsec_ts_ref.py)
under unit weights, its invariances (doubled weights, exact symmetry, the diagonal against the specific variance), the portfolio's hand
example and NULL rules; the public surface, the argument refusals that need no device, and the register / scratch figures of
csrc/xsec/risk.hip.

The tolerance against numpy.cov: the restatement and numpy sum in different orders.  Measured on this file's own inputs (M = 3 and
M = 39 series of N(0, 0.01^2), w = 252, half-life 90 and equal weights, ddof 1 and 0, three as-of days each), the worst deviation is
9.7e-16 of sqrt(var_j var_l); 64 times that (6.2e-14), rounded up to a power of ten, is the bound 1e-13 (D-28's and D-32's convention)."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_risk_ref as R
import xsec_ts_ref as RTS

ROOT = Path(__file__).resolve().parents[1]
NUMPY_COV_TOL = 1e-13
NULL = R.NULL


def same(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.dtype == np.int32:
        assert (got == exp).all(), (what, got, exp)
        return
    got, exp = got.astype(np.float64), exp.astype(np.float64)
    assert (got.view(np.uint64) == exp.view(np.uint64)).all(), (what, got, exp)


def panel(M, T, seed, holes=0.03):
    rng = np.random.default_rng(seed)
    F = rng.normal(0.0, 0.01, (M, T))
    if holes:
        F[rng.random((M, T)) < holes] = NULL
    return F


# ---------------------------------------------------------------- by hand
A3, B3, OM3 = np.array([[1.0, 3.0, 4.0]]), np.array([[2.0, 2.0, -2.0]]), np.array([1.0, 1.0, 2.0])


def test_hand_derived_example():
    """om = (1, 1, 2), a = (1, 3, 4), b = (2, 2, -2): W = 4, W2 = 6, Sa = 12, Sb = 0, ma = 3, mb = 0.
    C = 1 (-2)(2) + 1 (0)(2) + 2 (1)(-2) = -8, C_aa = 4 + 0 + 2 = 6.  Biased: cov = -8 / 4 = -2, var = 6 / 4 = 1.5.
    Unbiased: den = 4 - 6 / 4 = 2.5, cov = -3.2, var = 2.4.  All dyadic up to the last division."""
    days = [2]
    c, n = R.wcov(A3, B3, OM3, days, 1, unbiased=False)
    assert c[0, 0] == -2.0 and n[0, 0] == 3
    assert R.wcov(A3, A3, OM3, days, 1, unbiased=False)[0][0, 0] == 1.5
    assert R.wcov(A3, B3, OM3, days, 2)[0][0, 0] == -8.0 / 2.5
    assert R.wcov(A3, A3, OM3, days, 3)[0][0, 0] == 6.0 / 2.5
    cov, nd = R.factor_cov(np.concatenate([A3, B3]), OM3, days, 2, unbiased=False)
    assert cov[0].tolist() == [[1.5, -2.0], [-2.0, 4.0]] and nd.tolist() == [[3, 3]]      # C_bb = 4 + 4 + 2 * 4 = 16 at mb = 0


def test_one_window_per_null_rule():
    days = [2]
    # n < min_periods (a NULL and a NaN and an inf each drop their entry; a zero weight drops its)
    for bad in (NULL, float("nan"), float("inf"), -float("inf")):
        a = np.array([[1.0, bad, 4.0]])
        c, n = R.wcov(a, B3, OM3, days, 3)
        assert R.isnull(c).all() and n[0, 0] == 2
        c, n = R.wcov(a, B3, OM3, days, 2)
        assert not R.isnull(c).any() and n[0, 0] == 2
        c2, n2 = R.wcov(B3, a, OM3, days, 2)                  # the pair's sample, whichever side the hole is on
        same(c2, c)
        same(n2, n)
    c, n = R.wcov(A3, B3, [1.0, 0.0, 2.0], days, 3)
    assert R.isnull(c).all() and n[0, 0] == 2
    # unbiased and n < 2 (min_periods >= 2 says the same); biased: one entry gives the variance 0
    one = np.array([[NULL, NULL, 4.0]])
    assert R.isnull(R.wcov(one, one, OM3, days, 2)[0]).all()
    c, n = R.wcov(one, one, OM3, days, 1, unbiased=False)
    assert c[0, 0] == 0.0 and n[0, 0] == 1
    # the denominator is not > 0: W = 1 + 1e-20 = 1, W2 = 1, den = 0
    c, n = R.wcov(A3, B3, [0.0, 1e-20, 1.0], days, 2)
    assert R.isnull(c).all() and n[0, 0] == 2
    # the result is NaN: the products overflow to +inf and -inf
    a = np.array([[1e308, -1e308, 1e308, -1e308]])
    b = np.array([[1e308, 1e308, -1e308, -1e308]])
    assert R.isnull(R.wcov(a, b, np.ones(4), [3], 4)[0]).all()
    # +-inf passes
    big = np.array([[1e200, -1e200, 1e200]])
    assert R.wcov(big, big, np.ones(3), days, 3)[0][0, 0] == float("inf")
    assert R.wcov(big, -big, np.ones(3), days, 3)[0][0, 0] == -float("inf")


def test_a_window_that_reaches_before_day_0():
    """as of day 1 with w = 3: entry 0 is day -1 and is skipped; entries 1, 2 are days 0, 1 under the weights 1, 2"""
    c, n = R.wcov(A3, B3, OM3, [1], 2, unbiased=False)
    # om = (1, 2) on a = (1, 3), b = (2, 2): W = 3, Sa = 7, ma = 7 / 3; b is constant, so C = 0 up to rounding of (b - mb) = 0 exactly
    assert n[0, 0] == 2 and c[0, 0] == 0.0
    c, n = R.wcov(A3, A3, OM3, [0, 1, 2], 2, unbiased=False)
    assert n.tolist() == [[1, 2, 3]] and R.isnull(c[0, 0]) and c[0, 2] == 1.5
    # the same windows cut by hand
    same(c[0, 1], R.wcov(A3[:, :2], A3[:, :2], OM3[1:], [1], 2, unbiased=False)[0][0, 0])


# ---------------------------------------------------------------- against numpy.cov
def numpy_cov_deviation(M, halflife, unbiased, seed):
    w, T = 252, 300
    F = panel(M, T, seed, holes=0.0)
    om = R.weights(w, halflife)
    days = [251, 270, 299]
    cov, n = R.factor_cov(F, om, days, w, unbiased)
    assert (n == w).all()
    worst = 0.0
    for d, t in enumerate(days):
        ref = np.cov(F[:, t - w + 1:t + 1], aweights=om, ddof=1 if unbiased else 0).reshape(M, M)
        sd = np.sqrt(np.diag(ref))
        worst = max(worst, float((np.abs(cov[d] - ref) / np.outer(sd, sd)).max()))
    return worst


@pytest.mark.parametrize("M", [3, 39])
@pytest.mark.parametrize("halflife", [90, None])
@pytest.mark.parametrize("unbiased", [True, False])
def test_against_numpy_cov(M, halflife, unbiased):
    worst = numpy_cov_deviation(M, halflife, unbiased, 1000 + M)
    print(f"M={M} halflife={halflife} unbiased={unbiased}: worst deviation {worst:.3e} of sqrt(var_j var_l)")
    assert worst <= NUMPY_COV_TOL, worst


# ---------------------------------------------------------------- ts_cov, bit for bit
@pytest.mark.parametrize("w", [2, 5, 64])
def test_unit_weights_equal_the_ts_cov_restatement(w):
    """om = 1, unbiased, min_periods = w: every step is ts_cov's; rows without a full valid window are NULL in both"""
    T, holes = (150, 0.03) if w <= 5 else (300, 0.003)
    X, Y = panel(4, T, 7 + w, holes), panel(4, T, 70 + w, holes)
    X[0, 10] = float("inf")
    Y[1, 20] = float("nan")
    got, n = R.wcov(X, Y, np.ones(w), np.arange(T), w)
    exp = RTS.ts_cov(X, Y, w)
    assert (~R.isnull(exp)).sum() > T // 2 and R.isnull(exp).sum() > 4 * (w - 1)
    same(got, exp, f"ts_cov w={w}")
    assert ((n == w) == ~R.isnull(exp)).all()


# ---------------------------------------------------------------- invariances
def test_doubled_weights_symmetry_and_the_diagonal():
    M, T, w = 6, 120, 40
    F = panel(M, T, 5)
    F[2] = NULL                                                # a fully NULL series
    om = R.weights(w, 15.0)
    om[3] = om[17] = 0.0
    days = R.as_of_days(5, 7, 16)
    cov, n = R.factor_cov(F, om, days, 10)
    assert not R.isnull(cov[-1, 0, 1]) and R.isnull(cov[:, 2, :]).all() and R.isnull(cov[0]).all()
    cov2, n2 = R.factor_cov(F, 2.0 * om, days, 10)
    same(cov2, cov, "doubled weights")
    same(n2, n)
    # one evaluation per unordered pair, f_j (the row) as a: the matrix is exactly symmetric by construction
    full, _ = R.wcov(F[:, None, :], F[None, :, :], om, days, 10)           # every ordered pair evaluated on its own: [j, l, d]
    same(cov, np.swapaxes(cov, 1, 2), "the matrix is exactly symmetric")
    low = np.tril(np.ones((M, M), dtype=bool))
    same(np.moveaxis(full, 2, 0)[:, low], cov[:, low], "the triangle is rk_wcov(f_j, f_l)")
    # swapping the arguments changes no bit where om (a - ma) is exact -- equal (or dyadic) weights: then every product commutes.  Under
    # general weights (om (a - ma)) (b - mb) and (om (b - mb)) (a - ma) round differently, which is why the matrix is mirrored.
    unit, _ = R.wcov(F[:, None, :], F[None, :, :], 4.0 * (om > 0), days, 10)
    same(unit, np.swapaxes(unit, 0, 1), "cov(a, b) == cov(b, a) under equal weights")
    ok = ~R.isnull(full)
    assert (np.abs(full - np.swapaxes(full, 0, 1))[ok] <= 1e-13 * np.abs(full[ok]).max()).all()
    var, nv = R.specific_var(F, om, days, 10)
    same(var, np.diagonal(cov, axis1=1, axis2=2).T, "the diagonal")
    same(nv, n.T)
    b, _ = R.factor_cov(F, om, days, 10, unbiased=False)
    ok = ~R.isnull(cov)
    assert (np.abs(b[ok]) <= np.abs(cov[ok])).all() and (b[ok] != cov[ok]).any()


# ---------------------------------------------------------------- the portfolio
def hand_portfolio():
    """K = 1, two industries, four symbols, one day.  h = (0.5, 0.25, 0.25, -0.5), x = (2, -2, 4, 1), codes (0, 0, 1, 1),
    s^2 = (0.25, 1, 4, 0.5).  X = (1 - 0.5 + 1 - 0.5, 0.75, -0.25) = (1, 0.75, -0.25).
    F = [[4, 1, 0], [1, 2, -1], [0, -1, 8]]: F X = (4.75, 2.75, -2.75); c = (4.75, 2.0625, 0.6875), factor_var = 7.5.
    specific = 0.25 * 0.25 + 0.0625 * 1 + 0.0625 * 4 + 0.25 * 0.5 = 0.5; total = 8, vol = sqrt(8)."""
    H = np.array([[0.5], [0.25], [0.25], [-0.5]])
    X = np.array([[2.0], [-2.0], [4.0], [1.0]])
    ind = np.array([0, 0, 1, 1])
    sv = np.array([[0.25], [1.0], [4.0], [0.5]])
    F = np.array([[[4.0, 1.0, 0.0], [1.0, 2.0, -1.0], [0.0, -1.0, 8.0]]])
    return H, X, ind, sv, F


def test_portfolio_hand_example():
    H, X, ind, sv, F = hand_portfolio()
    out = R.portfolio(H, [X], F, sv, [0], ind, 2)
    assert out["exposure"][:, 0].tolist() == [1.0, 0.75, -0.25]
    assert out["contribution"][:, 0].tolist() == [4.75, 2.0625, 0.6875]
    assert out["risk"][:, 0].tolist() == [7.5, 0.5, 8.0, np.sqrt(8.0)]
    assert out["n"][:, 0].tolist() == [4, 0]
    # without codes: G = 1 and row K is the net weight
    out = R.portfolio(H, [X], F[:, :2, :2], sv, [0])
    assert out["exposure"][:, 0].tolist() == [1.0, 0.5]
    assert out["contribution"][:, 0].tolist() == [1.0 * (4.0 + 0.5), 0.5 * (1.0 + 1.0)]
    # K = 0: the industries alone
    out = R.portfolio(H, [], F[:, 1:, 1:], sv, [0], ind, 2)
    assert out["exposure"][:, 0].tolist() == [0.75, -0.25] and out["risk"][0, 0] == 0.75 * 1.75 + -0.25 * -2.75


def test_portfolio_null_rules():
    H, X, ind, sv, F = hand_portfolio()
    base = R.portfolio(H, [X], F, sv, [0], ind, 2)

    def all_null(out, n):
        assert R.isnull(out["exposure"]).all() and R.isnull(out["contribution"]).all() and R.isnull(out["risk"]).all()
        assert out["n"][:, 0].tolist() == n
    # nothing held: NULL and 0 holdings are not held
    all_null(R.portfolio(np.array([[0.0], [NULL], [-0.0], [float("inf")]]), [X], F, sv, [0], ind, 2), [0, 0])
    # an uncovered held symbol: an exposure, a code, a variance
    x2 = X.copy()
    x2[1, 0] = NULL
    all_null(R.portfolio(H, [x2], F, sv, [0], ind, 2), [4, 1])
    for code in (-1, 2):
        all_null(R.portfolio(H, [X], F, sv, [0], np.array([0, 0, code, code]), 2), [4, 2])
    for bad in (NULL, -0.5, float("nan")):
        s2 = sv.copy()
        s2[3, 0] = bad
        all_null(R.portfolio(H, [X], F, s2, [0], ind, 2), [4, 1])
    # ... but not where the symbol is not held
    h2, s2 = H.copy(), sv.copy()
    h2[3, 0], s2[3, 0] = 0.0, NULL
    out = R.portfolio(h2, [X], F, s2, [0], ind, 2)
    assert out["n"][:, 0].tolist() == [3, 0] and not R.isnull(out["risk"]).any()
    # a covariance that the product needs is NULL
    f2 = F.copy()
    f2[0, 0, 2] = f2[0, 2, 0] = NULL
    all_null(R.portfolio(H, [X], f2, sv, [0], ind, 2), [4, 0])
    # ... and one that it does not need, because an exposure is 0: industry 1 nets to 0 with h = (.., 0.5, -0.5)
    h3 = np.array([[0.5], [0.25], [0.5], [-0.5]])
    f3 = F.copy()
    f3[0, 2, :] = f3[0, :, 2] = NULL
    out = R.portfolio(h3, [X], f3, sv, [0], ind, 2)
    assert out["exposure"][:, 0].tolist() == [2.0, 0.75, 0.0] and out["contribution"][2, 0] == 0.0
    assert out["contribution"][:2, 0].tolist() == [2.0 * (8.0 + 0.75), 0.75 * (2.0 + 1.5)] and not R.isnull(out["risk"]).any()
    # a negative total: the volatility alone is NULL
    f4 = F.copy()
    f4[0, 0, 0] = -40.0
    out = R.portfolio(H, [X], f4, sv, [0], ind, 2)
    assert out["risk"][2, 0] == base["risk"][2, 0] - 44.0 and R.isnull(out["risk"][3, 0]) and not R.isnull(out["risk"][:3]).any()
    assert not R.isnull(out["exposure"]).any()


def test_portfolio_blocked_sums_over_two_blocks():
    """300 symbols: the exposures are block sums added in block order, not one running sum"""
    rng = np.random.default_rng(3)
    N, T = 300, 4
    H, X = rng.normal(0, 1, (N, T)), rng.normal(0, 1, (N, T))
    sv = rng.random((N, 2))
    F = np.broadcast_to(np.eye(2), (2, 2, 2)).copy()
    out = R.portfolio(H, [X], F, sv, [1, 3])
    for d, t in enumerate((1, 3)):
        blocks = []
        for lo in (0, 256):
            s = 0.0
            for i in range(lo, min(lo + 256, N)):
                s += H[i, t] * X[i, t]
            blocks.append(s)
        assert out["exposure"][0, d] == (0.0 + blocks[0]) + blocks[1]


# ---------------------------------------------------------------- the surface
def test_the_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    assert list(inspect.signature(api.risk_weights).parameters) == ["window", "halflife"]
    windowed = ["weights", "min_periods", "day0", "step", "count", "unbiased", "counts"]
    assert list(inspect.signature(api.risk_factor_cov).parameters) == ["series"] + windowed
    assert list(inspect.signature(api.risk_specific_var).parameters) == ["x"] + windowed
    sig = inspect.signature(api.risk_factor_cov)
    assert [sig.parameters[k].default for k in windowed[2:]] == [0, 1, None, True, False]
    assert list(inspect.signature(api.risk_portfolio).parameters) == ["holdings", "exposures", "cov", "specific_var", "industry", "day0",
                                                                      "step"]
    assert api.RISK_MAX_SERIES == 264
    sig = inspect.signature(pq.Factor.risk_model)
    assert list(sig.parameters) == ["self", "factor_returns", "specific_returns", "window", "halflife", "min_periods", "start", "step",
                                    "unbiased", "specific_window", "specific_halflife"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, 252, None, None, None, 1, True, None, None]
    assert list(inspect.signature(pq.Factor.portfolio_risk).parameters) == ["self", "holdings", "exposures", "model", "industry"]
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define PQ_RISK_MAX_SERIES \(PQ_REGRESS_MAX_K \+ PQ_IC_MAX_GROUPS\)", txt)
    want = {
        "pq_risk_factor_cov": ["pq_ctx *", "const pq_batch *", "const double *f", "const double *omega", "int64_t window",
                               "int64_t min_periods", "int32_t unbiased", "int64_t day0", "int64_t step", "int64_t count",
                               "double *cov_out", "int32_t *n_out"],
        "pq_risk_specific_var": ["pq_ctx *", "const pq_batch *", "const double *x", "const double *omega", "int64_t window",
                                 "int64_t min_periods", "int32_t unbiased", "int64_t day0", "int64_t step", "int64_t count",
                                 "double *var_out", "int64_t out_stride", "int32_t *n_out"],
        "pq_risk_portfolio": ["pq_ctx *", "const pq_batch *", "const double *holdings", "const double *const *exposures", "int32_t k",
                              "const int32_t *industry", "int64_t group_stride", "int32_t n_groups", "const double *cov",
                              "const double *specific_var", "int64_t sv_stride", "int64_t day0", "int64_t step", "int64_t count",
                              "double *exposure_out", "double *contribution_out", "double *risk_out", "int32_t *n_out"]}
    for name, args in want.items():
        decl = re.search(r"pq_status\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert decl, f"{name} is not declared"
        assert [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in decl.group(1).split(",")] == args, name
    assert re.search(r"^risk_factor_cov\s+i\s+pBppllilllpp$", _lib._SIGNATURES, flags=re.M)
    assert re.search(r"^risk_specific_var\s+i\s+pBppllilllplp$", _lib._SIGNATURES, flags=re.M)
    assert re.search(r"^risk_portfolio\s+i\s+pBppiplippllllpppp$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/risk.hip" in mk and mk.count("xsec/risk.resources.txt") == 1
    assert "polars_quant_amd/csrc/xsec/risk.resources.txt" in (ROOT / ".gitignore").read_text().split()


def test_risk_weights():
    from polars_quant_amd import api
    w = api.risk_weights(5, 2.0)
    assert w.dtype == np.float64 and w.tolist() == [0.25, 0.5 ** 1.5, 0.5, 0.5 ** 0.5, 1.0]
    assert api.risk_weights(3).tolist() == [1.0, 1.0, 1.0]
    same(api.risk_weights(252, 90), R.weights(252, 90))


ONES = np.ones((6, 10))
W4 = np.ones(4)
COV = np.zeros((3, 2, 2))
SV = np.zeros((6, 3))
CODES = np.zeros(6, dtype=np.int32)


@pytest.mark.parametrize("call, msg", [
    (lambda a: a.risk_weights(0), "window must be"),
    (lambda a: a.risk_weights(1025), "window must be"),
    (lambda a: a.risk_weights(2.0), "window must be"),
    (lambda a: a.risk_weights(5, 0.0), "halflife"),
    (lambda a: a.risk_weights(5, float("inf")), "halflife"),
    (lambda a: a.risk_factor_cov(ONES, np.ones((2, 2)), 2), "one-dimensional"),
    (lambda a: a.risk_factor_cov(ONES, np.ones(0), 2), "window"),
    (lambda a: a.risk_factor_cov(ONES, np.ones(1025), 2), "window"),
    (lambda a: a.risk_factor_cov(ONES, [1.0, float("nan")], 2), "finite"),
    (lambda a: a.risk_factor_cov(ONES, [1.0, float("inf")], 2), "finite"),
    (lambda a: a.risk_factor_cov(ONES, [1.0, -1.0], 2), "finite and >= 0"),
    (lambda a: a.risk_factor_cov(ONES, [0.0, 0.0], 2), "at least one > 0"),
    (lambda a: a.risk_factor_cov(ONES, W4, 1), "min_periods must be in 2..4"),
    (lambda a: a.risk_factor_cov(ONES, W4, 0, unbiased=False), "min_periods must be in 1..4"),
    (lambda a: a.risk_factor_cov(ONES, W4, 5), "min_periods must be in"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2.0), "min_periods must be an integer"),
    (lambda a: a.risk_factor_cov(np.ones((265, 3)), W4, 2), "at most 264"),
    (lambda a: a.risk_factor_cov(np.ones((2, 3, 4)), W4, 2), r"must be \[M, T\]"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2, day0=-1), "day0 >= 0"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2, step=0), "step >= 1"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2, day0=0.5), "day0 must be an integer"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2, day0=3, step=3, count=4), "count must be in 0..3"),
    (lambda a: a.risk_factor_cov(ONES, W4, 2, count=-1), "count must be"),
    (lambda a: a.risk_specific_var(ONES, W4, 1), "min_periods must be in 2..4"),
    (lambda a: a.risk_specific_var(ONES, W4, 2, day0=10, count=1), "count must be in 0..0"),
    (lambda a: a.risk_specific_var(ONES, [0.0], 1, unbiased=False), "at least one > 0"),
    (lambda a: a.risk_portfolio(np.ones(10), [ONES], COV, SV), r"holdings must be \[N, T\]"),
    (lambda a: a.risk_portfolio(ONES, [np.ones((6, 9))], COV, SV), "exposure 0"),
    (lambda a: a.risk_portfolio(ONES, [ONES] * 9, COV, SV), "number of exposures"),
    (lambda a: a.risk_portfolio(ONES, [ONES], np.zeros((3, 2, 3)), SV), r"cov must be \[D, M, M\]"),
    (lambda a: a.risk_portfolio(ONES, [ONES], np.zeros((3, 3, 3)), SV), "no industry codes"),
    (lambda a: a.risk_portfolio(ONES, None, COV, SV), "no industry codes"),
    (lambda a: a.risk_portfolio(ONES, [ONES], np.zeros((3, 1, 1)), SV, CODES), "K = 1 exposures and G industries"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, np.full(6, 1)), "K = 1 exposures and G industries"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, np.zeros(6)), "integer codes"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, np.zeros(5, dtype=np.int32)), "industry must be"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, np.zeros((6, 4))), "specific_var must be"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, day0=8), "do not fit"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, step=5), "do not fit"),
    (lambda a: a.risk_portfolio(ONES, [ONES], COV, SV, step=0), "step >= 1"),
])
def test_argument_refusals_without_a_device(call, msg):
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(api)


def test_factor_method_refusals_without_a_device():
    import polars_quant_amd as pq
    fac = pq.Factor()
    with pytest.raises(ValueError, match="window must be"):
        fac.risk_model(ONES, window=0)
    with pytest.raises(ValueError, match="halflife"):
        fac.risk_model(ONES, window=4, halflife=-1.0)
    with pytest.raises(ValueError, match="min_periods must be in 2..4"):
        fac.risk_model(ONES, window=4, min_periods=5)
    with pytest.raises(ValueError, match="specific_returns must have"):
        fac.risk_model(ONES, np.ones((3, 9)), window=4)
    with pytest.raises(ValueError, match="no specific_var"):
        fac.portfolio_risk(ONES, [ONES], {"factor_cov": COV, "day0": 0, "step": 1})


# ---------------------------------------------------------------- the kernels' resources
def test_no_kernel_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/risk.hip (risk.resources.txt, from hipcc's kernel-resource-usage
    remarks): the windowed kernel's two instantiations and the four portfolio kernels, none with scratch or a spilled VGPR (DESIGN.md
    D-33)."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "risk.resources.txt"
    if not path.exists():
        pytest.skip("csrc/xsec/risk.resources.txt is not built")
    found = re.findall(r"Function Name: \S*?\d+(rk_\w+?_kernel)(?:ILb(\d)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [("rk_cov_kernel", "0"), ("rk_cov_kernel", "1"), ("rk_pf_pass1_kernel", ""), ("rk_pf_sum_kernel", ""),
            ("rk_pf_contrib_kernel", ""), ("rk_pf_final_kernel", "")]
    assert sorted((k, b) for k, b, *_ in found) == sorted(want)
    for k, b, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, b, vgprs, scratch, occ, spill)
