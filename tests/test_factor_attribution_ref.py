"""not-gpu: the numpy restatement of decision D-36 (tests/xsec_attribution_ref.py) against an answer derived by hand, one case per rule,
its properties (the identity total = realized through D-32's own regression, exact doubling, active = portfolio - benchmark on dyadic
data), the chain to D-35's value curve, the argument checks of api.return_attribution that need no device, and the register / scratch
figures of csrc/xsec/attribution.hip."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import factor_weights_ref as W
import xsec_attribution_ref as A
import xsec_wls_ref as WLS

ROOT = Path(__file__).resolve().parent.parent
NULL = A.NULL
INF = float("inf")
STYLE, INDUSTRY, SPECIFIC, UNEXPLAINED, TOTAL, REALIZED = range(6)


def col(*v):
    """one day: a column [N, 1]"""
    return np.array(v, dtype=np.float64)[:, None]


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
    assert list(inspect.signature(api.return_attribution).parameters) == [
        "holdings", "exposures", "factor_return", "specific_return", "industry", "next_return", "benchmark", "periods"]
    sig = inspect.signature(pq.Factor.return_attribution)
    assert list(sig.parameters) == ["self", "holdings", "exposures", "returns", "industry", "next_return", "benchmark", "periods"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [None] * 4
    doc = " ".join(pq.Factor.return_attribution.__doc__.split())
    assert "holdings at the close of day t with the return from t to t + 1" in doc and "one day later" in doc
    assert api.ATTRIBUTION_TOTALS == A.TOTALS
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define PQ_ATTRIBUTION_TOTALS 6\b", txt)
    decl = re.search(r"pq_status\s+pq_return_attribution\s*\(([^)]*)\)", txt)
    assert decl, "pq_return_attribution is not declared"
    assert [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")] == [
        "pq_ctx *", "const pq_batch *", "const double *holdings", "const double *benchmark_holdings", "const double *const *exposures",
        "int32_t k", "const int32_t *industry", "int64_t group_stride", "int32_t n_groups", "const double *factor_return",
        "int64_t fr_stride", "const double *specific_return", "const double *next_return", "const int64_t *period_bounds",
        "int64_t n_periods", "double *exposure_out", "double *contribution_out", "double *totals_out", "int32_t *n_out",
        "double *summary_out", "double *period_sum_out", "int32_t *period_days_out"]
    assert re.search(r"^return_attribution\s+i\s+pBpppipliplppplppppppp$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/attribution.hip" in mk and mk.count("xsec/attribution.resources.txt") == 1
    assert "polars_quant_amd/csrc/xsec/attribution.resources.txt" in (ROOT / ".gitignore").read_text().split()
    src = (ROOT / "polars_quant_amd" / "csrc" / "xsec" / "attribution.hip").read_text()
    assert "rg_summary_row(" in src and "rg_t_pvalue" not in src, "the summary goes through xsec_ttest.h's shared row, no second copy"


# ---------------------------------------------------------------- by hand
H3, B3 = col(1 / 2, 1 / 4, 1 / 4), col(1 / 4, 1 / 4, 1 / 2)
X3, G3 = col(1.0, -1 / 2, NULL), np.array([0, 1, 0])
F3, U3, R3 = col(1 / 8, 1 / 4, -1 / 8), col(1 / 8, -1 / 8, 0.0), col(1 / 2, -5 / 16, 1 / 8)


def test_hand_derived_dyadic_example():
    """DESIGN.md D-36's example.  Three symbols A, B, C on one day, K = 1, industries (0, 1, 0); style return 1/8, industry returns
    (1/4, -1/8); exposures (1, -1/2, NULL): C is uncovered; specific returns (1/8, -1/8, .); so r_A = 1/8 + 1/4 + 1/8 = 1/2,
    r_B = -1/16 - 1/8 - 1/8 = -5/16, and r_C = 1/8 is given.
    portfolio h = (1/2, 1/4, 1/4): X = (1/2 - 1/8, 1/2, 1/4) = (3/8, 1/2, 1/4), c = (3/64, 1/8, -1/32), style 3/64, industry 3/32,
      specific 1/16 - 1/32 = 1/32, unexplained 1/4 * 1/8 = 1/32, total 13/64 = realized 1/4 - 5/64 + 1/32.
    benchmark b = (1/4, 1/4, 1/2): X = (1/8, 1/4, 1/4), c = (1/64, 1/16, -1/32), style 1/64, industry 1/32, specific 0, unexplained
      1/16, total 7/64 = realized 1/8 - 5/64 + 1/16.
    active a = (1/4, 0, -1/4): B is not held; X = (1/4, 1/4, 0), c = (1/32, 1/16, 0), style 1/32, industry 1/16, specific 1/32,
      unexplained -1/32, total 3/32 = 13/64 - 7/64 = realized 1/8 - 1/32."""
    o = A.attribution(H3, [X3], F3, U3, G3, 2, R3, B3, bounds=[0, 1])
    same(o["exposure"][:, :, 0], [[3 / 8, 1 / 2, 1 / 4], [1 / 8, 1 / 4, 1 / 4], [1 / 4, 1 / 4, 0.0]])
    same(o["contribution"][:, :, 0], [[3 / 64, 1 / 8, -1 / 32], [1 / 64, 1 / 16, -1 / 32], [1 / 32, 1 / 16, 0.0]])
    same(o["totals"][:, :, 0], [[3 / 64, 3 / 32, 1 / 32, 1 / 32, 13 / 64, 13 / 64], [1 / 64, 1 / 32, 0.0, 1 / 16, 7 / 64, 7 / 64],
                                [1 / 32, 1 / 16, 1 / 32, -1 / 32, 3 / 32, 3 / 32]])
    assert o["n"][:, :, 0].tolist() == [[3, 3, 2], [1, 1, 1], [0, 0, 0]]
    same(o["summary"][0, 3 + TOTAL], [1.0, 13 / 64, NULL, NULL, NULL])                 # one day: a mean, no deviation
    same(o["period_sum"][:, :, 0], np.concatenate([o["contribution"], o["totals"]], axis=1)[:, :, 0])
    assert o["period_days"].tolist() == [[1], [1], [1]]
    one = A.attribution(H3, [X3], F3, U3, G3, 2, R3)
    for k in ("exposure", "contribution", "totals", "n", "summary"):
        same(one[k][0] if k != "n" else one[k][:, 0], o[k][0] if k != "n" else o[k][:, 0], k)   # P = 1 is book 0 of P = 3


# ---------------------------------------------------------------- one case per rule
def test_an_empty_industry_with_a_null_return_does_not_matter():
    f = col(1 / 8, 1 / 4, -1 / 8, NULL)                                                # a third industry without a member: D-32 writes NULL
    o = A.attribution(H3, [X3], f, U3, G3, 3, R3)
    same(o["contribution"][0, :, 0], [3 / 64, 1 / 8, -1 / 32, 0.0])
    same(o["totals"][0, :, 0], [3 / 64, 3 / 32, 1 / 32, 1 / 32, 13 / 64, 13 / 64])


@pytest.mark.parametrize("bad", [NULL, float("nan"), INF, -INF])
def test_a_null_factor_return_that_is_needed_nulls_the_day_of_that_book(bad):
    f = col(1 / 8, 1 / 4, bad)                                                         # industry 1: held by h and b (symbol B), not by a
    o = A.attribution(H3, [X3], f, U3, G3, 2, R3, B3)
    for k in ("exposure", "contribution", "totals"):
        assert A.isnull(o[k][:2]).all(), k
    same(o["totals"][2, :, 0], [1 / 32, 1 / 16, 1 / 32, -1 / 32, 3 / 32, 3 / 32])
    assert o["n"][:, :, 0].tolist() == [[3, 3, 2], [1, 1, 1], [0, 0, 0]]              # the counts do not depend on it


def test_a_day_on_which_nothing_is_held_is_null():
    h = np.concatenate([H3, col(0.0, NULL, INF), H3], axis=1)
    rep = lambda v: np.repeat(v, 3, axis=1)   # noqa: E731
    o = A.attribution(h, [rep(X3)], rep(F3), rep(U3), G3, 2, rep(R3), bounds=[0, 2, 3])
    assert o["n"][:, 0].tolist() == [[3, 0, 3], [1, 0, 1], [0, 0, 0]]
    for k in ("exposure", "contribution", "totals"):
        assert A.isnull(o[k][0, :, 1]).all() and not A.isnull(o[k][0, :, [0, 2]]).any(), k
    same(o["summary"][0, 3 + TOTAL], [2.0, 13 / 64, NULL, NULL, NULL])   # two equal days: std 0, no t
    same(o["period_sum"][0, 3 + TOTAL], [13 / 64, 13 / 64])
    assert o["period_days"].tolist() == [[1, 1]]


def test_uncovered_with_and_without_next_return():
    with_r = A.attribution(H3, [X3], F3, U3, G3, 2, R3)
    no_r = A.attribution(H3, [X3], F3, U3, G3, 2, None)
    part = A.attribution(H3, [X3], F3, U3, G3, 2, col(1 / 2, -5 / 16, NULL))
    assert with_r["n"][:, 0, 0].tolist() == [3, 1, 0] and no_r["n"][:, 0, 0].tolist() == [3, 1, 1] == part["n"][:, 0, 0].tolist()
    same(no_r["totals"][0, :, 0], [3 / 64, 3 / 32, 1 / 32, 0.0, 11 / 64, NULL])        # nothing to explain with; realized NULL
    same(part["totals"][0, :, 0], [3 / 64, 3 / 32, 1 / 32, 0.0, 11 / 64, 11 / 64])     # realized leaves the missing symbol out
    # each way of being uncovered: the exposure (above), the code, the specific return
    for g, u in (([0, 1, 2], col(1 / 8, -1 / 8, 0.0)), ([0, 1, -1], col(1 / 8, -1 / 8, 0.0)), ([0, 1, 0], col(1 / 8, -1 / 8, NULL))):
        o = A.attribution(H3, [col(1.0, -1 / 2, 1.0)], F3, u, np.array(g), 2, R3)
        assert o["n"][:, 0, 0].tolist() == [3, 1, 0]
        same(o["totals"][0, :, 0], with_r["totals"][0, :, 0])


def test_k_0_and_g_1_without_codes():
    """no exposure, no codes: the one row is the net weight times the intercept"""
    o = A.attribution(H3, [], col(1 / 4), col(1 / 8, -1 / 8, 1 / 2), None, 1, col(3 / 8, 1 / 8, 3 / 4))
    same(o["exposure"][0, :, 0], [1.0])
    same(o["totals"][0, :, 0], [0.0, 1 / 4, 1 / 16 - 1 / 32 + 1 / 8, 0.0, 1 / 4 + 5 / 32, 3 / 16 + 1 / 32 + 3 / 16])
    assert o["summary"].shape == (1, 7, 5)


def test_codes_per_day():
    """[N, T] codes: symbol B changes industry on day 1"""
    rep = lambda v: np.repeat(v, 2, axis=1)   # noqa: E731
    g = np.array([[0, 0], [1, 0], [0, 0]])
    o = A.attribution(rep(H3), [rep(X3)], rep(F3), rep(U3), g, 2, rep(R3))
    same(o["exposure"][0], [[3 / 8, 3 / 8], [1 / 2, 3 / 4], [1 / 4, 0.0]])
    same(o["contribution"][0], [[3 / 64, 3 / 64], [1 / 8, 3 / 16], [-1 / 32, 0.0]])
    static = A.attribution(rep(H3), [rep(X3)], rep(F3), rep(U3), g[:, 0], 2, rep(R3))
    same(static["exposure"][0, :, 0], o["exposure"][0, :, 0])


def test_bad_arguments_of_the_restatement():
    for bounds in ([0], [1, 1], [0, 2], [-1, 1], [1, 0]):
        with pytest.raises(AssertionError):
            A.attribution(H3, [X3], F3, U3, G3, 2, R3, bounds=bounds)
    with pytest.raises(AssertionError):
        A.attribution(H3, [X3], F3, U3, None, 2, R3)


# ---------------------------------------------------------------- the model's data: D-32's own regression of r
def model(N, T, K, G, seed, holes=True):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((N, T)) for _ in range(K)]
    ind = rng.integers(0, G, N)
    ind[:G] = np.arange(G) if N >= G else ind[:G]
    r = 0.02 * rng.standard_normal((N, T))
    for x in xs:
        r = r + 0.005 * rng.standard_normal(T)[None, :] * x
    if holes:                                                   # on every third day, so that days without an uncovered symbol remain
        third = (np.arange(T) % 3 == 0)[None, :]
        r[(rng.random((N, T)) < 0.02) & third] = NULL
        if K:
            xs[0][(rng.random((N, T)) < 0.02) & third] = NULL
    fit = WLS.wls(xs, r, None, ind, G)
    h = rng.standard_normal((N, T)) / N
    h[rng.random((N, T)) < 0.3] = 0.0
    return xs, ind, r, fit, h


IDENTITY_BOUND = 1e-13      # 64 x the worst figure measured on the host (2.5e-16 at (40, 30, 2, 3), 1.7e-16 at (700, 40, 8, 31)), rounded up to a power of ten


@pytest.mark.parametrize("shape", [(40, 30, 2, 3), (700, 40, 8, 31)])
def test_property_i_total_equals_realized_without_uncovered_symbols(shape):
    """r = sum x_j f_j + f_g + u on D-32's sample, with f and u from tests/xsec_wls_ref's own regression of r: on the days without an
    uncovered symbol total equals realized up to rounding, relative to sum |h r|"""
    N, T, K, G = shape
    xs, ind, r, fit, h = model(N, T, K, G, 36)
    o = A.attribution(h, xs, fit["coef"], fit["resid"], ind, G, r)
    days = (o["n"][1, 0] == 0) & ~A.isnull(o["totals"][0, TOTAL])
    assert days.sum() >= 1 and (o["n"][1, 0] > 0).any(), "both kinds of day occur"
    scale = np.where(A.valid(h) & A.valid(r), np.abs(h * np.where(A.valid(r), r, 0.0)), 0.0).sum(axis=0)
    err = np.abs(o["totals"][0, TOTAL] - o["totals"][0, REALIZED])[days] / scale[days]
    print(f"identity at {shape}: worst |total - realized| / sum |h r| = {err.max():.3e} over {int(days.sum())} days")
    assert err.max() <= IDENTITY_BOUND
    # and with every hole closed, on every day
    xs, ind, r, fit, h = model(N, T, K, G, 37, holes=False)
    o = A.attribution(h, xs, fit["coef"], fit["resid"], ind, G, r)
    assert (o["n"][1:] == 0).all()
    err = np.abs(o["totals"][0, TOTAL] - o["totals"][0, REALIZED]) / np.abs(h * r).sum(axis=0)
    print(f"identity at {shape}, clean: {err.max():.3e}")
    assert err.max() <= IDENTITY_BOUND


def test_property_ii_doubling_the_holdings_doubles_every_output_bit_for_bit():
    """any input: products and sums scale by a power of two exactly; the counts, n_days, t and p do not change"""
    N, T, K, G = 300, 12, 3, 5
    xs, ind, r, fit, h = model(N, T, K, G, 38)
    b = np.roll(h, 7, axis=0)
    h[0, 0], h[1, 0], b[2, 0] = NULL, INF, float("nan")
    bounds = [0, 5, 12]
    o1 = A.attribution(h, xs, fit["coef"], fit["resid"], ind, G, r, b, bounds)
    o2 = A.attribution(2.0 * h, xs, fit["coef"], fit["resid"], ind, G, r, 2.0 * b, bounds)
    for k in ("exposure", "contribution", "totals", "period_sum"):
        same(o2[k], 2.0 * o1[k], k)
    same(o2["summary"][..., 1:3], 2.0 * o1["summary"][..., 1:3], "mean, std")
    same(o2["summary"][..., [0, 3, 4]], o1["summary"][..., [0, 3, 4]], "n_days, t, p")
    assert (o2["n"] == o1["n"]).all() and (o2["period_days"] == o1["period_days"]).all()


def dyadic(N, T, K, G, seed):
    """holdings in 1/64 up to 1, exposures in 1/64 up to 2, returns in 1/64 up to 1: a product h x is a multiple of 2^-12 below 2, a sum
    of N <= 1024 of them a multiple of 2^-12 below 2^11 (23 bits), X f a multiple of 2^-18 below 2^11 (29 bits) and a sum of at most 264
    rows below 2^20 (38 bits): every partial sum is exact in f64's 53"""
    rng = np.random.default_rng(seed)
    q = lambda lo, hi, *s: rng.integers(lo, hi + 1, s) / 64.0   # noqa: E731
    return (q(-64, 64, N, T), q(-64, 64, N, T), [q(-128, 128, N, T) for _ in range(K)], rng.integers(0, G, N), q(-64, 64, K + G, T),
            q(-64, 64, N, T), q(-64, 64, N, T))


def test_property_ii_the_active_book_is_portfolio_minus_benchmark_on_dyadic_data():
    N, T, K, G = 700, 9, 8, 31
    h, b, xs, ind, f, u, r = dyadic(N, T, K, G, 39)
    h[5, 1], b[6, 1], xs[0][7, 2], u[8, 3], r[9, 4] = NULL, INF, NULL, NULL, NULL      # an invalid holding counts as 0.0 in the active book
    o = A.attribution(h, xs, f, u, ind, G, r, b, [0, 4, 9])
    assert not A.isnull(o["totals"][:, :5]).any()
    for k in ("exposure", "contribution", "totals", "period_sum"):
        same(o[k][2], o[k][0] - o[k][1], k)
    assert (o["n"][0, 2] <= o["n"][0, 0] + o["n"][0, 1]).all()


# ---------------------------------------------------------------- the chain to D-35
CHAIN_BOUND = 1e-13         # 64 x the worst figure measured on the host (2.3e-16), rounded up to a power of ten


def test_chain_realized_is_the_growth_of_d35s_value_curve():
    """zero cost, clean prices, next_return = price[t + 1] / price[t] - 1: realized[t] of the drifted holdings is value[t + 1] /
    value[t] - 1 on the days from the first rebalance on that are not followed by a rebalance"""
    rng = np.random.default_rng(40)
    N, T = 50, 40
    price = 10.0 * np.cumprod(1.0 + 0.02 * rng.standard_normal((N, T)), axis=1)
    days = np.array([2, 9, 10, 25])
    w = rng.standard_normal((N, len(days))) / N
    bt = W.weights([w], price, days, 0.0, 1000.0, holdings_of=0)
    nxt = np.full((N, T), NULL)
    nxt[:, :-1] = price[:, 1:] / price[:, :-1] - 1.0
    o = A.attribution(bt["holdings"], [], np.zeros((1, T)), np.zeros((N, T)), None, 1, nxt)
    v = bt["value"][0]
    t = np.array([t for t in range(days[0], T - 1) if t + 1 not in days])
    got, want = o["totals"][0, REALIZED][t], v[t + 1] / v[t] - 1.0
    err = np.abs(got - want).max()
    print(f"chain: worst |realized - (value[t + 1] / value[t] - 1)| = {err:.3e} over {len(t)} days")
    assert err <= CHAIN_BOUND
    assert (o["n"][1:] == 0).all() and o["totals"][0, REALIZED][-1] == 0.0             # all covered; the last day has no next return


# ---------------------------------------------------------------- refusals that need no device
ONES = np.ones((6, 10))
FR = np.ones((3, 10))           # K = 1, G = 2
CODES = np.array([0, 1, 0, 1, 0, 1])


@pytest.mark.parametrize("call, msg", [
    (lambda a: a.return_attribution(np.ones(10), [ONES], FR, ONES, CODES), r"holdings must be \[N, T\]"),
    (lambda a: a.return_attribution(ONES, [ONES] * 9, FR, ONES, CODES), "number of exposures"),
    (lambda a: a.return_attribution(ONES, [np.ones((6, 9))], FR, ONES, CODES), "exposure 0 must have"),
    (lambda a: a.return_attribution(ONES, np.ones((6, 10)), FR, ONES, CODES), "exposures must be a list"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, None, CODES), "specific_return is needed"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, np.ones((5, 10)), CODES), "specific_return must have"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, next_return=np.ones((6, 11))), "next_return must have"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, benchmark=np.ones(10)), "benchmark must have"),
    (lambda a: a.return_attribution(ONES, [ONES], np.ones((3, 9)), ONES, CODES), r"factor_return must be \[K \+ G, T\]"),
    (lambda a: a.return_attribution(ONES, [ONES], np.ones(10), ONES, CODES), r"factor_return must be \[K \+ G, T\]"),
    (lambda a: a.return_attribution(ONES, [ONES], np.ones((2, 10)), ONES, CODES), "the codes are < G"),
    (lambda a: a.return_attribution(ONES, [ONES], np.ones((1, 10)), ONES, CODES), "the codes are < G"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, None), "no industry codes"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES.astype(np.float64)), "integer codes"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES[:5]), r"industry must be \[N\] or \[N, T\]"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=0), "n_splits"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=11), "n_splits"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=[0]), "day bounds"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=[0.0, 5.0]), "day bounds"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=[0, 11]), "strictly ascending"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=[-1, 5]), "strictly ascending"),
    (lambda a: a.return_attribution(ONES, [ONES], FR, ONES, CODES, periods=[3, 3]), "strictly ascending"),
])
def test_argument_refusals_without_a_device(call, msg):
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(api)


def test_factor_method_refusals_without_a_device():
    import polars_quant_amd as pq
    fac = pq.Factor()
    with pytest.raises(ValueError, match='no "holdings"'):
        fac.return_attribution({"value": ONES}, [ONES], (FR, ONES), CODES)
    with pytest.raises(ValueError, match='benchmark dict has no "holdings"'):
        fac.return_attribution(ONES, [ONES], (FR, ONES), CODES, benchmark={})
    with pytest.raises(ValueError, match="returns must be"):
        fac.return_attribution(ONES, [ONES], FR, CODES)
    with pytest.raises(ValueError, match="n_splits"):
        fac.return_attribution(ONES, [ONES], (FR, ONES), CODES, periods=0)


def test_the_period_bounds_of_an_int_are_array_split():
    from polars_quant_amd import api
    for T, n in ((10, 1), (10, 3), (10, 10), (131, 7)):
        parts = np.array_split(np.arange(T), n)
        assert api._attribution_bounds(T, n).tolist() == [int(p[0]) for p in parts] + [T]
    assert api._attribution_bounds(10, None) is None
    assert api._attribution_bounds(10, [2, 5, 10]).tolist() == [2, 5, 10]


# ---------------------------------------------------------------- the kernels' resources
def test_no_kernel_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/attribution.hip (attribution.resources.txt, from hipcc's
    kernel-resource-usage remarks): the pass in its book classes <1> and <3>, each as the first launch and as a later one, and the
    four plain kernels, none with scratch or a spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "attribution.resources.txt"
    if not path.exists():
        pytest.skip("csrc/xsec/attribution.resources.txt is not built")
    found = re.findall(r"Function Name: \S*?\d+(at_\w+?_kernel)(?:ILi(\d+)ELb([01])E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [("at_pass_kernel", pc, first) for pc in ("1", "3") for first in ("0", "1")]
    want += [(k, "", "") for k in ("at_sum_kernel", "at_day_kernel", "at_summary_kernel", "at_period_kernel")]
    assert sorted((k, c, f) for k, c, f, *_ in found) == sorted(want)
    for k, c, f, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, c, f, vgprs, scratch, occ, spill)
