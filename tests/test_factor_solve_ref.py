"""not-gpu: the numpy restatement of decision D-34 (tests/xsec_solve_ref.py: y = Sigma^-1 v through the factor structure, the quad
matrix, the three portfolios) against an example derived by hand, one constructed day per NULL rule, numpy.linalg.solve on the dense
Sigma = B F B^T + diag(s^2), and the properties of the portfolios; the public surface, the argument refusals that need no device, and
the register / scratch figures of csrc/xsec/risk_solve.hip.

The tolerance against the dense solve: the restatement and LAPACK solve different systems in different orders.  Measured on this
file's own inputs ((N, K, G) = (40, 2, 3), (300, 3, 4), (700, 8, 31), (700, 8, 64); F the sample covariance of 260 days of
N(0, 0.01^2) returns, s in [0.01, 0.03], v = ones and a normal vector), the worst deviation is 2.7e-14 of max |y| (cond(S) <= 210);
64 times that (1.7e-12), rounded up to a power of ten, is the bound 1e-11 (D-28's convention)."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_solve_cases as cases
import xsec_solve_ref as S

ROOT = Path(__file__).resolve().parents[1]
DENSE_TOL = 1e-11
NULL = S.NULL


def same(got, exp, what=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert (got.view(np.uint64) == exp.view(np.uint64)).all(), (what, got, exp)


# ---------------------------------------------------------------- by hand
def test_hand_derived_example():
    """x = (1, 2, -1, -1), industries (0, 0, 1, 1), s^2 = (1/2, 1/2, 1/4, 1/4): q = (2, 2, 4, 4).
    A[0][0] = 2 + 8 + 4 + 4 = 18, A[0][g] = (2 + 4, -4 - 4) = (6, -8), A[g][g] = (4, 8): A = [[18, 6, -8], [6, 4, 0], [-8, 0, 8]].
    F = [[-1, 1, -1], [1, 1, 1], [-1, 1, -1]] (indefinite): F A = [[-4, -2, 0], [16, 10, 0], [-4, -2, 0]], S = I + F A =
    [[-3, -2, 0], [16, 11, 0], [-4, -2, 1]] (the leading 2 x 2 block has determinant -1).
    v = ones: p = (6 - 8, 4, 8) = (-2, 4, 8), F p = (-2, 10, -2); u = (2, -2, 2); y_i = q_i (1 - 2 x_i - u_g) = (2, -2, 4, 4).
    alpha = (1, 2, -1, 0): p = (2 + 8 + 4 + 0, 2 + 4, -4 + 0) = (14, 6, -4), F p = (-4, 16, -4); u = (12, -16, 12);
    y_i = q_i (alpha_i - 12 x_i - u_g) = (10, -12, -4, 0).
    quad: 1'y_1 = 8, 1'y_a = alpha'y_1 = -6, alpha'y_a = 10 - 24 + 4 + 0 = -10.  Every intermediate value is a small integer, so
    the floating-point result is exact."""
    x, alpha, ind, F, sv = cases.hand()
    out = S.solve([None, alpha], [x], F, sv, [0], ind, 2)
    assert out["n"].tolist() == [[4], [0]] and not out["null"][0]
    assert out["u"][:, 0].tolist() == [[2.0, -2.0, 2.0], [12.0, -16.0, 12.0]]
    assert out["y"][:, :, 0].tolist() == [[2.0, -2.0, 4.0, 4.0], [10.0, -12.0, -4.0, 0.0]]
    assert out["quad"][:, :, 0].tolist() == [[8.0, -6.0], [-6.0, -10.0]]
    # the portfolios: min variance w = y_1 / 8 with variance 1 / 8; tangency w = y_a / -6 is NULL (q_1a is not > 0);
    # mean-variance at lambda = 2: gamma = (-6 - 2) / 8 = -1, w = (y_a + y_1) / 2 = (6, -7, 0, 2)
    w, var, ret = S.optimal(out["y"], out["quad"], "min_variance")
    assert w[:, 0].tolist() == [0.25, -0.25, 0.5, 0.5] and var[0] == 0.125 and ret[0] == -0.75
    w, var, ret = S.optimal(out["y"], out["quad"], "max_sharpe")
    assert S.isnull(w).all() and S.isnull(var).all() and S.isnull(ret).all()
    w, var, ret = S.optimal(out["y"], out["quad"], "mean_variance", 2.0)
    assert w[:, 0].tolist() == [6.0, -7.0, 0.0, 2.0] and w[:, 0].sum() == 1.0
    assert ret[0] == (-10.0 - 6.0) / 2.0 and var[0] == (-10.0 - 12.0 + 8.0) / 4.0


# ---------------------------------------------------------------- one day per NULL rule
def null_rule_case():
    """N = 12, K = 2, G = 3 on six days from one full model: 0 as it is; 1 nothing in U; 2 a NULL covariance between two active rows;
    3 industry 2 without a member and its covariances NULL; 4 factor 1 zero on all of U and its covariances NULL; 5 uncovered symbols"""
    N, K, G, D = 12, 2, 3, 6
    X1, alpha1, ind, F1, sv1, _ = cases.dense(N, K, G, seed=7)
    X = np.repeat(X1, D, axis=2)
    alpha = np.repeat(alpha1, D, axis=1)
    ind = np.repeat(np.array(ind)[:, None], D, axis=1)
    F = np.repeat(F1, D, axis=0)
    sv = np.repeat(sv1, D, axis=1)
    sv[:, 1] = NULL
    F[2, 0, K + 1] = F[2, K + 1, 0] = NULL
    ind[ind[:, 3] == 2, 3] = 0
    F[3, K + 2, :] = F[3, :, K + 2] = NULL
    X[1, :, 4] = 0.0
    F[4, 1, :] = F[4, :, 1] = NULL
    X[0, 0, 5] = NULL
    ind[1, 5] = G
    ind[2, 5] = -1
    sv[3, 5], sv[4, 5], sv[5, 5], sv[6, 5] = NULL, 0.0, -1e-9, float("nan")
    alpha[7, 5] = NULL
    return X, alpha, ind, F, sv, K, G


def test_one_day_per_null_rule():
    X, alpha, ind, F, sv, K, G = null_rule_case()
    N, D = sv.shape
    out = S.solve([None, alpha], list(X), F, sv, np.arange(D), ind, G)
    y, quad, n, u = out["y"], out["quad"], out["n"], out["u"]
    assert out["null"].tolist() == [False, True, True, False, False, False]
    assert n.tolist() == [[N, 0, N, N, N, N - 8], [0, N, 0, 0, 0, 7]]     # (symbol 7's alpha is missing: neither in U nor uncovered)
    for d in (1, 2):
        assert S.isnull(y[:, :, d]).all() and S.isnull(quad[:, :, d]).all()
    for d in (0, 3, 4, 5):
        assert not S.isnull(quad[:, :, d]).any()
    assert not S.isnull(y[:, :, [0, 3, 4]]).any()
    assert (u[:, 3, K + 2] == 0.0).all() and (u[:, 3, :K + 2] != 0.0).all()          # the absent industry takes no part
    assert (u[:, 4, 1] == 0.0).all() and (u[:, 4, 0] != 0.0).all()                    # nor does the zero factor
    assert S.isnull(y[:, :8, 5]).all() and not S.isnull(y[:, 8:, 5]).any()
    # the days with a row less are the smaller model's days
    keep = [j for j in range(K + G) if j != K + 2]
    small = S.solve([None, alpha[:, 3:4]], [x[:, 3:4] for x in X], F[3:4][:, keep][:, :, keep], sv[:, 3:4], [0], ind[:, 3], G - 1)
    same(small["y"][:, :, 0], y[:, :, 3], "without the absent industry")
    small = S.solve([None, alpha[:, 4:5]], [X[0][:, 4:5]], F[4:5][:, [0, 2, 3, 4]][:, :, [0, 2, 3, 4]], sv[:, 4:5], [0], ind[:, 4], G)
    same(small["y"][:, :, 0], y[:, :, 4], "without the zero factor")


def test_a_zero_pivot_makes_the_day_null():
    """K = 0, one group, four symbols with s^2 = 1/4: A = 16, and F = -1/16 gives S = 1 + F A = 0 exactly; F = -1/8 gives S = -1"""
    sv = np.full((4, 2), 0.25)
    F = np.array([[[-1.0 / 16.0]], [[-1.0 / 8.0]]])
    out = S.solve([None], [], F, sv, [0, 1])
    assert out["null"].tolist() == [True, False] and out["n"].tolist() == [[4, 4], [0, 0]]
    assert S.isnull(out["y"][0, :, 0]).all() and S.isnull(out["quad"][0, 0, 0])
    assert out["y"][0, :, 1].tolist() == [-4.0] * 4 and out["quad"][0, 0, 1] == -16.0   # u = -2 / -1 = 2, y = 4 (1 - 2)
    assert S.lu_solve(np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([[2.0], [3.0]])).tolist() == [[3.0], [2.0]]   # the pivot swap
    assert S.lu_solve(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones((2, 1))) is None
    assert S.lu_solve(np.array([[float("nan"), 1.0], [1.0, 1.0]]), np.ones((2, 1))) is None


# ---------------------------------------------------------------- against the dense solve
DENSE = [(40, 2, 3), (300, 3, 4), (700, 8, 31), (700, 8, 64)]


@pytest.fixture(scope="module")
def dense_runs():
    runs = {}
    for N, K, G in DENSE:
        X, alpha, ind, F, sv, B = cases.dense(N, K, G)
        out = S.solve([None, alpha], list(X), F, sv, [0], ind, G)
        runs[(N, K, G)] = (out, B @ F[0] @ B.T + np.diag(sv[:, 0]), alpha[:, 0])
    return runs


@pytest.mark.parametrize("N,K,G", DENSE)
def test_against_the_dense_solve(dense_runs, N, K, G):
    out, Sigma, alpha = dense_runs[(N, K, G)]
    assert not out["null"][0] and out["n"].tolist() == [[N], [0]]
    for r, v in enumerate((np.ones(N), alpha)):
        ref = np.linalg.solve(Sigma, v)
        dev = np.abs(out["y"][r, :, 0] - ref).max() / np.abs(ref).max()
        print(f"N={N} K={K} G={G} rhs {r}: deviation {dev:.3g} of max|y|, cond(S) = {out['cond'][0]:.4g}")
        assert dev <= DENSE_TOL
        for l, u in enumerate((np.ones(N), alpha)):
            assert abs(out["quad"][r, l, 0] - u @ ref) <= DENSE_TOL * np.abs(u) @ np.abs(ref)


@pytest.mark.parametrize("N,K,G", DENSE)
def test_properties_of_the_portfolios(dense_runs, N, K, G):
    out, Sigma, alpha = dense_runs[(N, K, G)]
    y, quad = out["y"], out["quad"]
    same(quad, quad.transpose(1, 0, 2), "quad is exactly symmetric")
    w, var, _ = S.optimal(y, quad, "min_variance")
    w = w[:, 0]
    assert abs(w.sum() - 1.0) <= DENSE_TOL * np.abs(w).max()
    assert abs(w @ Sigma @ w - 1.0 / quad[0, 0, 0]) <= DENSE_TOL * (1.0 / quad[0, 0, 0]) and var[0] == 1.0 / quad[0, 0, 0]
    for lam in (1.0, 7.5):
        w, var, ret = S.optimal(y, quad, "mean_variance", lam)
        w = w[:, 0]
        assert abs(w.sum() - 1.0) <= DENSE_TOL * np.abs(w).max()
        kkt = alpha - lam * (Sigma @ w)                         # proportional to the vector of ones
        assert np.abs(kkt - kkt.mean()).max() <= DENSE_TOL * max(np.abs(alpha).max(), lam * np.abs(Sigma @ w).max())
        assert abs(var[0] - w @ Sigma @ w) <= DENSE_TOL * abs(var[0]) and abs(ret[0] - alpha @ w) <= DENSE_TOL * np.abs(w).max()
    w, var, ret = S.optimal(y, quad, "max_sharpe")
    if quad[1, 0, 0] > 0.0:
        w = w[:, 0]
        assert abs(w.sum() - 1.0) <= DENSE_TOL * np.abs(w).max()
        g = Sigma @ w                                           # Sigma w proportional to alpha
        k = (g @ alpha) / (alpha @ alpha)
        assert np.abs(g - k * alpha).max() <= DENSE_TOL * np.abs(g).max()
    else:
        assert S.isnull(w).all()


def test_blocked_sums_of_the_moments():
    """the moments are D-12's blocked sums: 300 symbols are two blocks"""
    N = 300
    X, alpha, ind, F, sv, _ = cases.dense(N, 3, 4)
    q = 1.0 / sv
    A, p = S.moments([np.ones((N, 1)), alpha], list(X), q, np.ones((N, 1), dtype=bool), np.array(ind)[:, None], 4)
    blocks = []
    for lo in (0, 256):
        s = 0.0
        for i in range(lo, min(lo + 256, N)):
            s += (q[i, 0] * X[2, i, 0]) * X[1, i, 0]
        blocks.append(s)
    assert A[0, 2, 1] == (0.0 + blocks[0]) + blocks[1] and A[0, 1, 2] == A[0, 2, 1]
    assert (A[0, 3:, 3:] == np.diag(np.diag(A[0, 3:, 3:]))).all()


# ---------------------------------------------------------------- the surface
def test_the_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    assert list(inspect.signature(api.risk_solve).parameters) == ["rhs", "exposures", "cov", "specific_var", "industry", "day0", "step"]
    sig = inspect.signature(pq.Factor.optimal_portfolio)
    assert list(sig.parameters) == ["self", "exposures", "model", "alpha", "industry", "objective", "risk_aversion"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, "min_variance", 1.0]
    doc = pq.Factor.optimal_portfolio.__doc__
    assert "unconstrained in sign" in doc and "one day" in doc
    assert api.RISK_SOLVE_MAX_RHS == S.MAX_RHS == 4 and api.RISK_SOLVE_MAX_M == S.MAX_M == 128
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define PQ_RISK_SOLVE_MAX_RHS 4\b", txt) and re.search(r"#define PQ_RISK_SOLVE_MAX_M 128\b", txt)
    decl = re.search(r"pq_status\s+pq_risk_solve\s*\(([^)]*)\)", txt)
    assert decl, "pq_risk_solve is not declared"
    assert [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in decl.group(1).split(",")] == [
        "pq_ctx *", "const pq_batch *", "const double *const *rhs", "int32_t n_rhs", "const double *const *exposures", "int32_t k",
        "const int32_t *industry", "int64_t group_stride", "int32_t n_groups", "const double *cov", "const double *specific_var",
        "int64_t sv_stride", "int64_t day0", "int64_t step", "int64_t count", "double *const *y_out", "int64_t out_stride",
        "double *quad_out", "int32_t *n_out"]
    assert re.search(r"^risk_solve\s+i\s+pBpipiplippllllplpp$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/risk_solve.hip" in mk and mk.count("xsec/risk_solve.resources.txt") == 1
    assert "polars_quant_amd/csrc/xsec/risk_solve.resources.txt" in (ROOT / ".gitignore").read_text().split()


ONES = np.ones((6, 10))
COV = np.zeros((3, 2, 2))
SV = np.ones((6, 3))
CODES = np.zeros(6, dtype=np.int32)


@pytest.mark.parametrize("call, msg", [
    (lambda a: a.risk_solve(ONES, [ONES], COV, SV), "rhs must be a list"),
    (lambda a: a.risk_solve([], [ONES], COV, SV), "rhs must be a list"),
    (lambda a: a.risk_solve([None] * 5, [ONES], COV, SV), "rhs must be a list"),
    (lambda a: a.risk_solve([None], None, np.zeros((3, 1, 1)), SV), "nothing tells the days"),
    (lambda a: a.risk_solve([np.ones(10)], [ONES], COV, SV), r"must be \[N, T\]"),
    (lambda a: a.risk_solve([ONES, np.ones((6, 9))], [ONES], COV, SV), "rhs 1"),
    (lambda a: a.risk_solve([None], [ONES, np.ones((5, 10))], np.zeros((3, 3, 3)), SV), "exposure 1"),
    (lambda a: a.risk_solve([None], [ONES] * 9, COV, SV), "number of exposures"),
    (lambda a: a.risk_solve([None], [ONES], np.zeros((3, 2, 3)), SV), r"cov must be \[D, M, M\]"),
    (lambda a: a.risk_solve([None], [ONES], np.zeros((3, 3, 3)), SV), "no industry codes"),
    (lambda a: a.risk_solve([None], [ONES], COV, SV, np.full(6, 1)), "K = 1 exposures and G industries"),
    (lambda a: a.risk_solve([None], [ONES], COV, SV, np.zeros(6)), "integer codes"),
    (lambda a: a.risk_solve([None], [ONES], COV, SV, np.zeros(5, dtype=np.int32)), "industry must be"),
    (lambda a: a.risk_solve([None], [ONES], COV, np.zeros((6, 4))), "specific_var must be"),
    (lambda a: a.risk_solve([None], [ONES], COV, SV, day0=8), "do not fit"),
    (lambda a: a.risk_solve([None], [ONES], COV, SV, step=0), "step >= 1"),
    (lambda a: a.risk_solve([None], [ONES], np.zeros((3, 129, 129)), SV, CODES), "at most 128"),
])
def test_argument_refusals_without_a_device(call, msg):
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(api)


def test_factor_method_refusals_without_a_device():
    import polars_quant_amd as pq
    fac = pq.Factor()
    model = {"factor_cov": COV, "specific_var": SV, "day0": 0, "step": 1}
    with pytest.raises(ValueError, match="objective must be"):
        fac.optimal_portfolio([ONES], model, objective="long_only")
    with pytest.raises(ValueError, match="needs alpha"):
        fac.optimal_portfolio([ONES], model, objective="max_sharpe")
    with pytest.raises(ValueError, match="needs alpha"):
        fac.optimal_portfolio([ONES], model, objective="mean_variance")
    with pytest.raises(ValueError, match="risk_aversion"):
        fac.optimal_portfolio([ONES], model, ONES, objective="mean_variance", risk_aversion=0.0)
    with pytest.raises(ValueError, match="no specific_var"):
        fac.optimal_portfolio([ONES], {"factor_cov": COV, "day0": 0, "step": 1})


# ---------------------------------------------------------------- the kernels' resources
def test_no_kernel_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/risk_solve.hip (risk_solve.resources.txt, from hipcc's
    kernel-resource-usage remarks): the two instantiations of the moments kernel, the two sums, the solve and the output pass, none
    with scratch or a spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "risk_solve.resources.txt"
    if not path.exists():
        pytest.skip("csrc/xsec/risk_solve.resources.txt is not built")
    found = re.findall(r"Function Name: \S*?\d+(rs_\w+?_kernel)(?:ILb(\d)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [("rs_moments_kernel", "0"), ("rs_moments_kernel", "1"), ("rs_sum_kernel", ""), ("rs_solve_kernel", ""),
            ("rs_output_kernel", ""), ("rs_quad_kernel", "")]
    assert sorted((k, b) for k, b, *_ in found) == sorted(want)
    for k, b, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, b, vgprs, scratch, occ, spill)
