"""not-gpu: the numpy restatement of decision D-28 (tests/xsec_rolling_regress_ref.py: rolling-window OLS) against answers derived by
hand, against numpy.linalg.lstsq window by window, and bit for bit against the restatement of D-17 (tests/xsec_regress_ref.py) where
the window is the whole history; the public surface, the argument refusals that need no device, and the register / scratch figures of
csrc/xsec/rolling_regress.hip."""
import inspect
import os
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_regress_ref as G
import xsec_rolling_regress_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL


def same(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    assert (got.view(np.uint64) == exp.view(np.uint64)).all(), (got, exp)


def all_null(out, cols=slice(None)):
    return all(R.isnull(out[k][..., cols]).all() for k in R.OUTPUTS)


# ---------------------------------------------------------------- answers derived by hand
X8 = np.array([[1.0, 2.0, 4.0, 3.0, 5.0, 7.0, 6.0, 8.0], [3.0, -1.0, 0.0, 2.0, 9.0, 4.0, 4.0, 5.0]])


def test_an_exact_line():
    """y = 2 x + 1 on small integers, window 4: sums of four integers divided by 4.0 are exact, so are the centred products; c = 2 C,
    b = c / C = 2, alpha = ybar - 2 xbar = 1, every residual 0"""
    out = R.rolling_regress(2.0 * X8 + 1.0, [X8], 4)
    assert all_null(out, slice(0, 3))
    for k, v in (("alpha", 1.0), ("resid_std", 0.0), ("r_squared", 1.0), ("resid", 0.0)):
        assert (out[k][:, 3:] == v).all(), k
    assert out["beta"].shape == (1, 2, 8) and (out["beta"][0][:, 3:] == 2.0).all()


def test_a_constant_regressor_is_singular():
    """C = 0: the pivot 0 > 1e-12 * 0 fails"""
    x = X8.copy()
    x[0, 2:6] = 5.0                       # the window of row 5 of symbol 0 alone
    out = R.rolling_regress(X8[::-1] * X8, [x], 4)
    assert all_null(out, slice(0, 3))
    for k in R.OUTPUTS:
        nul = R.isnull(out[k][..., 3:])
        assert nul[..., 0, 2].all() and nul.sum() == nul[..., 0, 2].size, k


def test_a_constant_return():
    """Syy = 0: c = 0, so beta = 0 / C = 0, alpha = ybar, every residual 0 -- and R^2 alone is NULL"""
    out = R.rolling_regress(np.full(X8.shape, 7.0), [X8], 4)
    assert (out["beta"][0][:, 3:] == 0.0).all() and (out["alpha"][:, 3:] == 7.0).all()
    assert (out["resid_std"][:, 3:] == 0.0).all() and (out["resid"][:, 3:] == 0.0).all()
    assert R.isnull(out["r_squared"]).all()


def test_collinear_regressors_are_singular():
    """x_1 = 2 x_0 on integers: D_1 = 4 C00 - (2 C00) * 2 = 0 exactly"""
    assert all_null(R.rolling_regress(X8[::-1] * X8, [X8, 2.0 * X8], 4))
    assert not R.isnull(R.rolling_regress(X8[::-1] * X8, [X8, X8 * X8], 4)["beta"][:, :, 3:]).any()


@pytest.mark.parametrize("col", [0, 1, 2])
@pytest.mark.parametrize("bad", [np.nan, NULL, np.inf, -np.inf])
def test_an_invalid_cell_nulls_exactly_its_windows(col, bad):
    """day d of one column of symbol 1 (a [T] series at col 1: of every symbol) -> rows d .. d + window - 1"""
    rng = np.random.default_rng(3)
    n, T, w, d = 3, 40, 5, 11
    cols = [rng.standard_normal((n, T)), rng.standard_normal(T), rng.standard_normal((n, T))]   # x_0, x_1 (a series), y
    if col == 1:
        cols[1][d] = bad
    else:
        cols[col][1, d] = bad
    out = R.rolling_regress(cols[2], cols[:2], w)
    exp = np.zeros((n, T), dtype=bool)
    exp[:, :w - 1] = True
    exp[slice(None) if col == 1 else 1, d:d + w] = True
    for k in R.OUTPUTS:
        assert (R.isnull(out[k]) == exp).all(), k


def test_a_nan_result_nulls_the_row():
    """1e200-sized deviations: the centred products overflow, b = inf / inf"""
    x = X8 * 1e200
    out = R.rolling_regress(x[::-1].copy(), [x], 4)
    assert all_null(out)


# ---------------------------------------------------------------- numpy.linalg.lstsq, window by window
def lstsq_windows(y, xs, w):
    n, T = y.shape
    K = len(xs)
    X = [np.broadcast_to(x, y.shape) for x in xs]
    out = {"beta": np.full((K, n, T), np.nan), **{k: np.full((n, T), np.nan) for k in R.OUTPUTS[1:]}}
    for s in range(n):
        for t in range(w - 1, T):
            A = np.column_stack([x[s, t - w + 1:t + 1] for x in X] + [np.ones(w)])
            yy = y[s, t - w + 1:t + 1]
            coef = np.linalg.lstsq(A, yy, rcond=None)[0]
            e = yy - A @ coef
            out["beta"][:, s, t], out["alpha"][s, t] = coef[:K], coef[K]
            out["resid_std"][s, t] = np.sqrt(e @ e / (w - K - 1))
            out["r_squared"][s, t] = 1.0 - e @ e / ((yy - yy.mean()) @ (yy - yy.mean()))
            out["resid"][s, t] = e[-1]
    return out


LSTSQ_BOUND = 1e-11


def test_against_lstsq():
    """Well-conditioned inputs (independent N(0, 1) regressors, one of them a [T] series, y = 0.3 + sum_j (j + 1) x_j / 2 + 0.5 N(0, 1)),
    K = 1, 2, 3, windows 20 and 60, 4 symbols x 90 days.  The deviation of an output is max |restatement - lstsq| / max |lstsq| over its
    cells.  Measured on these inputs: the largest deviation over the cases and the five outputs is 2.61e-14 (alpha at K = 3, window 60;
    the two differ only in rounding order); the bound is 64 x that = 1.67e-12, rounded up to a power of ten: 1e-11."""
    rng = np.random.default_rng(28)
    n, T = 4, 90
    worst = 0.0
    for K in (1, 2, 3):
        xs = [rng.standard_normal(T) if j == 0 else rng.standard_normal((n, T)) for j in range(K)]
        y = 0.3 + sum(0.5 * (j + 1) * np.broadcast_to(x, (n, T)) for j, x in enumerate(xs)) + 0.5 * rng.standard_normal((n, T))
        for w in (20, 60):
            got, exp = R.rolling_regress(y, xs, w), lstsq_windows(y, xs, w)
            for k in R.OUTPUTS:
                g, e = got[k][..., w - 1:], exp[k][..., w - 1:]
                assert not R.isnull(g).any() and R.isnull(got[k][..., :w - 1]).all()
                dev = float(np.abs(g - e).max() / np.abs(e).max())
                print(f"K={K} w={w} {k}: {dev:.3g}")
                worst = max(worst, dev)
    print(f"largest deviation {worst:.3g}")
    assert worst <= LSTSQ_BOUND


# ---------------------------------------------------------------- D-17 where the window is the whole history
@pytest.mark.parametrize("K, T", [(1, 3), (1, 200), (2, 37), (3, 256), (4, 100)])
def test_the_last_column_is_the_time_series_regression(K, T):
    """T <= 256 (one summation block of D-17), no invalid cell, window = T: the one full window is D-17's sample, in D-17's order"""
    rng = np.random.default_rng(100 * K + T)
    n = 6
    xs = [rng.standard_normal(T) if j == 1 else rng.standard_normal((n, T)) for j in range(K)]
    y = rng.standard_normal((n, T))
    y[0] = 1.5                                            # Syy == 0: R^2 NULL on both sides
    if K >= 2:
        xs[0][1] = 2.0                                    # a constant regressor: singular on both sides
    got, exp = R.rolling_regress(y, xs, T), G.ts_regress(xs, y)
    assert all_null(got, slice(0, T - 1))
    same(got["beta"][:, :, -1].T, exp["coef"][:, :K])
    same(got["alpha"][:, -1], exp["coef"][:, K])
    same(got["r_squared"][:, -1], exp["r2"])
    assert R.isnull(exp["r2"][0]) and not R.isnull(exp["coef"][0]).any() and R.isnull(exp["coef"][1]).all() == (K >= 2)
    assert not R.isnull(exp["coef"][2:]).any()


# ---------------------------------------------------------------- the public surface
def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    F = pq.Factor
    want = {"rolling_regression": ["returns", "factors", "window"], "rolling_beta": ["returns", "market", "window"],
            "idiosyncratic_volatility": ["returns", "factors", "window"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(F, name))
        assert list(sig.parameters) == ["self"] + params, name
        assert sig.parameters["window"].default == 60
    assert callable(api.factor_rolling_regress)
    assert inspect.signature(api.factor_rolling_regress).parameters["outputs"].default == R.OUTPUTS
    assert api.ROLLING_REGRESS_MAX_K == 4 == R.MAX_K and api.ROLLING_REGRESS_OUTPUTS == R.OUTPUTS
    raw = (ROOT / "include" / "pq_hip.h").read_text()
    assert re.search(r"#define\s+PQ_ROLLING_REGRESS_MAX_K\s+4\b", raw)
    assert "D-28" in raw and "README.md:231" in raw
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"pq_status\s+pq_factor_rolling_regress\s*\(([^)]*)\)", txt)
    assert decl, "pq_factor_rolling_regress is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["pq_ctx *", "const pq_batch *", "const double *const *x", "int32_t n_x", "uint32_t series_mask", "const double *y",
                    "int64_t window", "double *beta", "double *alpha", "double *resid_std", "double *r_squared", "double *resid"]
    assert re.search(r"^factor_rolling_regress\s+i\s+pBpiuplppppp$", _lib._SIGNATURES, flags=re.M)
    assert "xsec/rolling_regress.hip" in (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()


Y = np.ones((3, 40))
S = np.ones(40)


@pytest.mark.parametrize("call, msg", [
    (lambda f, a: a.factor_rolling_regress(S, [S], 5), r"must be \[N, T\]"),
    (lambda f, a: a.factor_rolling_regress(Y, [np.ones((3, 41))], 5), "shape"),
    (lambda f, a: a.factor_rolling_regress(Y, [np.ones(39)], 5), "shape"),
    (lambda f, a: a.factor_rolling_regress(Y, np.ones((3, 40)), 5), r"\[K, N, T\]"),
    (lambda f, a: a.factor_rolling_regress(Y, [], 5), "number of regressors"),
    (lambda f, a: a.factor_rolling_regress(Y, [Y] * 5, 20), "number of regressors"),
    (lambda f, a: a.factor_rolling_regress(Y, np.ones((5, 3, 40)), 20), "number of regressors"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], 2), "window"),
    (lambda f, a: a.factor_rolling_regress(Y, [S, Y, Y, Y], 5), "window"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], 1025), "window"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], 20.0), "window"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], True), "window"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], 20, outputs=()), "outputs"),
    (lambda f, a: a.factor_rolling_regress(Y, [S], 20, outputs=("beta", "t_stat")), "outputs"),
    (lambda f, a: f.rolling_regression(Y, [S], 2), "window"),
    (lambda f, a: f.rolling_beta(Y, S, 2), "window"),
    (lambda f, a: f.rolling_beta(Y, np.ones(41)), "shape"),
    (lambda f, a: f.idiosyncratic_volatility(Y, [S, Y], 3), "window"),
    (lambda f, a: f.idiosyncratic_volatility(Y, [Y] * 5), "number of regressors"),
])
def test_argument_errors_raise_before_device_work(call, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(pq.Factor(), api)


# ---------------------------------------------------------------- the kernel's resources
def test_no_instantiation_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/rolling_regress.hip (rolling_regress.resources.txt, from hipcc's
    kernel-resource-usage remarks): the windowed kernel in its four instantiations K = 1 .. 4, none with scratch or a spilled VGPR
    (templated on K, every index of the L D L^T arrays is static)."""
    path = os.path.join(os.path.dirname(__file__), "..", "polars_quant_amd", "csrc", "xsec", "rolling_regress.resources.txt")
    if not os.path.exists(path):
        pytest.skip("rolling_regress.resources.txt not built (make -C polars_quant_amd/csrc)")
    found = re.findall(r"Function Name: \S*?(rr_\w+?_kernel)(?:ILi(\d+)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", open(path).read())
    assert sorted((k, g) for k, g, *_ in found) == [("rr_window_kernel", str(K)) for K in (1, 2, 3, 4)]
    for k, g, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, g, vgprs, scratch, occ, spill)
