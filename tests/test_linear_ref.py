"""not-gpu: the D-24 restatement (tests/linear_ref.py) against an independent computation, on hand-checkable cases, on the cases
without a solution and on the membership rules; the public surface of linear() (pq.linear, api.linear, the C declaration).

Tolerance of the independent comparison: the centred normal equations in np.longdouble (sums by np.sum, Gaussian elimination) on
well-conditioned data without holes (regressors of unit spread on offsets up to 100, noise of the size of the signal), M in
{K + 2, 1 000, 300 000} x K in {1, 3, 8}.  Worst relative deviation of coef and R^2 measured on this data: 1.78e-14 (a slope at K = 1,
M = 1 000; R^2 stays below 6e-16); allowed: 16 x that = 2.85e-13, which covers another libm or BLAS and nothing else."""
import inspect
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import linear_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL

MEASURED = 1.78e-14     # worst relative deviation of coef / R^2 from the longdouble solution over the nine cases below
ALLOWED = 16 * MEASURED


def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import api
    assert list(inspect.signature(pq.linear).parameters) == ["df", "x_cols", "y_col", "pred_col", "resid_col", "return_stats"]
    par = inspect.signature(pq.linear).parameters
    assert (par["pred_col"].default, par["resid_col"].default, par["return_stats"].default) == ("pred", "resid", False)
    assert list(inspect.signature(api.linear).parameters) == ["xs", "y", "outputs"] and inspect.signature(api.linear).parameters["outputs"].default is True
    assert api.LINEAR_TILE == R.TILE and api.LINEAR_STAGE2 == R.STAGE2
    assert (api.LINEAR_STAGE2 + 1) * api.LINEAR_TILE + 5 < 8_000_000
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pq_hip.h").read_text(), flags=re.S)
    assert re.search(r"pq_status pq_linear\(pq_ctx \*, const pq_batch \*, const double \*const \*x, int32_t k, const double \*y, double "
                     r"\*coef, double \*t_stat,\s+double \*p_value, double \*r2, int64_t \*n, double \*pred, double \*resid\);", hdr)
    assert re.search(rf"#define PQ_LINEAR_TILE {R.TILE}\b", hdr) and re.search(rf"#define PQ_LINEAR_STAGE2 {R.STAGE2}\b", hdr)


def test_argument_errors_need_no_device():
    from polars_quant_amd import api
    import polars_quant_amd as pq
    y = np.zeros(5)
    with pytest.raises(ValueError):
        api.linear([], y)
    with pytest.raises(ValueError):
        api.linear([y] * 9, y)
    with pytest.raises(ValueError):
        api.linear([np.zeros(4)], y)
    with pytest.raises(ValueError):
        api.linear([np.zeros((1, 1, 5))], np.zeros((1, 1, 5)))
    with pytest.raises(TypeError):
        pq.linear(y, ["x"], "y")


# ---- the restatement against the longdouble normal equations
def well_conditioned(K, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K, M)) * rng.uniform(0.5, 2.0, (K, 1)) + rng.uniform(-100.0, 100.0, (K, 1))
    beta = rng.uniform(0.5, 2.0, K) * rng.choice([-1.0, 1.0], K)
    sig = beta @ X
    y = 3.0 + sig + np.std(sig - sig.mean()) * rng.standard_normal(M) if M > K + 2 else 3.0 + sig + rng.standard_normal(M)
    return X, y


def longdouble_ols(X, y):
    """coef (slopes, intercept) and R^2 by the centred normal equations in np.longdouble"""
    ld = np.longdouble
    X, y = X.astype(ld), y.astype(ld)
    K = X.shape[0]
    xm, ym = X.mean(axis=1), y.mean()
    D, dy = X - xm[:, None], y - ym
    A, c = D @ D.T, D @ dy
    A, c = A.copy(), c.copy()
    for j in range(K):                                   # Gaussian elimination with partial pivoting
        p = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, p]], c[[j, p]] = A[[p, j]], c[[p, j]]
        for i in range(j + 1, K):
            m = A[i, j] / A[j, j]
            A[i, j:] -= m * A[j, j:]
            c[i] -= m * c[j]
    b = np.zeros(K, dtype=ld)
    for j in range(K - 1, -1, -1):
        b[j] = (c[j] - A[j, j + 1:] @ b[j + 1:]) / A[j, j]
    a = ym - b @ xm
    e = y - (a + b @ X)
    return np.append(b, a), 1 - (e @ e) / (dy @ dy)


DEVIATION_CASES = [(K, M) for K in (1, 3, 8) for M in (K + 2, 1_000, 300_000)]


def deviation(K, M):
    X, y = well_conditioned(K, M, 1000 * K + M % 997)
    out = R.linear(list(X), y)
    coef, r2 = longdouble_ols(X, y)
    assert out["n"] == M
    dc = float(np.max(np.abs((out["coef"].astype(np.longdouble) - coef) / coef)))
    dr = float(abs((np.longdouble(out["r2"]) - r2) / r2))
    return dc, dr


@pytest.mark.parametrize("K,M", DEVIATION_CASES)
def test_restatement_against_longdouble_normal_equations(K, M):
    dc, dr = deviation(K, M)
    print(f"K={K} M={M}: coef {dc:.3e} R^2 {dr:.3e} (allowed {ALLOWED:.3e})")
    assert dc <= ALLOWED and dr <= ALLOWED


# ---- hand-checkable cases
def test_readme_example_market_cap_on_return():
    x = np.array([1000.0, 1100.0, 1050.0, 1200.0])
    y = np.array([0.02, 0.01, -0.005, 0.03])
    out = R.linear([x], y)
    slope = Fraction(31, 350000)                           # Sxy / Sxx = 1.9375 / 21875
    icpt = Fraction(11, 800) - slope * Fraction(2175, 2)   # ybar - slope xbar
    r2 = Fraction(375390625, 1462890625)                   # Sxy^2 / (Sxx Syy) = 3.75390625 / 14.62890625
    for exp, quoted in ((slope, 8.857142857e-05), (icpt, -0.08257142857), (r2, 0.25660881175)):
        assert abs(float(exp) - quoted) <= 1e-9 * abs(quoted)
    assert abs(out["coef"][0] - float(slope)) <= 1e-12 * float(slope)
    assert abs(out["coef"][1] - float(icpt)) <= 1e-12 * abs(float(icpt))
    assert abs(out["r2"] - float(r2)) <= 1e-12 * float(r2)
    assert out["n"] == 4
    np.testing.assert_allclose(out["pred"] + out["resid"], y, rtol=0, atol=1e-17)


@pytest.mark.parametrize("K", [1, 2])
def test_perfect_integer_fit_is_exact(K):
    x0 = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0]) * 3 + 10     # orthogonal centred columns, dyadic means
    x1 = np.array([-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0]) * 2 - 6
    xs, beta = ([x0], [2.0]) if K == 1 else ([x0, x1], [2.0, -0.5])
    y = 3.0 + sum(b * x for b, x in zip(beta, xs))
    out = R.linear(xs, y)
    assert out["coef"].tolist() == beta + [3.0]
    assert out["r2"] == 1.0 and out["n"] == 8
    assert (out["resid"] == 0.0).all() and (out["pred"] == y).all()
    assert R.isnull(out["t"]).all() and R.isnull(out["p"]).all()            # se == 0


def test_constant_y():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(40)
    out = R.linear([x], np.full(40, 0.375))
    assert out["coef"][0] == 0.0 and out["coef"][1] == 0.375
    assert R.isnull(out["r2"]) and R.isnull(out["t"]).all() and R.isnull(out["p"]).all()
    assert (out["pred"] == 0.375).all() and (out["resid"] == 0.0).all()


# ---- no solution
def assert_no_solution(out, n, shape):
    for k in ("coef", "t", "p"):
        assert R.isnull(out[k]).all(), k
    assert R.isnull(out["r2"]) and out["n"] == n
    assert out["pred"].shape == shape and R.isnull(out["pred"]).all() and R.isnull(out["resid"]).all()


@pytest.mark.parametrize("K", [1, 3, 8])
def test_no_solution_with_k_plus_1_members(K):
    rng = np.random.default_rng(K)
    X, y = rng.standard_normal((K, K + 4)), rng.standard_normal(K + 4)
    y[K + 1:] = NULL
    assert_no_solution(R.linear(list(X), y), K + 1, (K + 4,))
    y[K + 1] = 0.5
    assert not R.isnull(R.linear(list(X), y)["coef"]).any()      # K + 2 members solve


def test_no_solution_collinear_constant_and_empty():
    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, 64).astype(np.float64)
    y = rng.standard_normal(64)
    assert_no_solution(R.linear([x, rng.standard_normal(64), 2.0 * x], y), 64, (64,))
    assert_no_solution(R.linear([np.full(64, 2.5)], y), 64, (64,))
    assert_no_solution(R.linear([rng.standard_normal(64), np.full(64, -1.0)], y), 64, (64,))
    assert_no_solution(R.linear([np.zeros(0)], np.zeros(0)), 0, (0,))
    assert_no_solution(R.linear([np.zeros((0, 7))], np.zeros((0, 7))), 0, (0, 7))


# ---- membership
def test_membership():
    rng = np.random.default_rng(11)
    M = 50
    x0, x1 = rng.standard_normal(M), rng.standard_normal(M) + 4.0
    y = 1.0 + 0.5 * x0 - 0.25 * x1 + 0.1 * rng.standard_normal(M)
    y[3], y[4], y[5] = NULL, np.nan, np.inf
    x0[10], x1[11], x0[12] = NULL, np.nan, -np.inf
    out = R.linear([x0, x1], y)
    assert out["n"] == M - 6
    for i in (3, 4, 5):                                    # valid x, invalid y: a prediction, no residual
        assert np.isfinite(out["pred"][i]) and R.isnull(out["resid"][i])
    for i in (10, 11, 12):                                 # one invalid x_j: neither
        assert R.isnull(out["pred"][i]) and R.isnull(out["resid"][i])
    keep = np.ones(M, dtype=bool)
    keep[[3, 4, 5, 10, 11, 12]] = False
    assert np.isfinite(out["pred"][keep]).all() and np.isfinite(out["resid"][keep]).all()
    coef, r2 = longdouble_ols(np.stack([x0[keep], x1[keep]]), y[keep])      # the fit is the fit of the members
    assert np.max(np.abs((out["coef"] - coef) / coef)) < 1e-12 and abs(out["r2"] - r2) < 1e-12
    p3 = out["coef"][2] + out["coef"][0] * x0[3] + out["coef"][1] * x1[3]   # from a, j ascending
    assert out["pred"][3] == p3


def test_sse_is_the_sum_of_the_written_residuals():
    X, y = well_conditioned(3, 9000, 77)
    out = R.linear(list(X), y)
    mem = np.ones(9000, dtype=bool)
    sse = R.psum(out["resid"] * out["resid"], mem)
    syy = R.psum((y - R.psum(y, mem) / 9000.0) ** 2, mem)
    assert out["r2"] == 1.0 - sse / syy


# ---- the definition depends on the logical row index only
@pytest.mark.parametrize("shape", [(37, 50), (3, 4099), (300, 131)])
def test_matrix_equals_its_flat_column(shape):
    rng = np.random.default_rng(shape[1])
    X = rng.standard_normal((2,) + shape) + 3.0
    y = 0.5 * X[0] - X[1] + rng.standard_normal(shape)
    y[rng.random(shape) < 0.05] = NULL
    a, b = R.linear(list(X), y), R.linear([x.reshape(-1) for x in X], y.reshape(-1))
    for k in ("coef", "t", "r2", "pred", "resid"):
        assert (np.asarray(a[k]).reshape(-1).view(np.uint64) == np.asarray(b[k]).reshape(-1).view(np.uint64)).all(), k
    assert a["n"] == b["n"] and a["pred"].shape == shape


def test_psum_first_tile_by_hand():
    """psum is a sum (close to the left-to-right one), and on one tile it is the lane sums folded in D-24's tree, written out here"""
    rng = np.random.default_rng(3)
    z = rng.standard_normal(3 * R.TILE + 17) * 1e8 + 0.1
    mem = np.ones(z.size, dtype=bool)
    seq = 0.0
    for v in z.tolist():
        seq += v
    s = R.psum(z, mem)
    assert abs(s - seq) <= 1e-9 * abs(seq)
    lanes = z[:R.TILE].reshape(R.ROWS, R.LANES)           # the first tile by hand: lane sums, then the tree
    a = np.zeros(R.LANES)
    for i in range(R.ROWS):
        a = a + lanes[i]
    w = []
    for g in range(4):
        v = a[64 * g:64 * g + 64]
        while v.size > 1:
            v = v[:v.size // 2] + v[v.size // 2:]
        w.append(v[0])
    assert R.psum(z[:R.TILE], mem[:R.TILE]) == (w[0] + w[2]) + (w[1] + w[3])
