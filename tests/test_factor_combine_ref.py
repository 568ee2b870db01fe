"""not-gpu: the numpy restatement of decision D-30 (tests/xsec_combine_ref.py: the ic / icir / max_icir combination weights and the
composite) against the CPU oracle's rolling_ic shifted by the lag (bit for bit), against hand-derived tables, and against the sample
covariance solved in np.longdouble; the public surface of the feature -- tables, the signature and defaults of Factor.combine, the
argument errors that must come before any device work, the C declarations -- and the register / scratch figures of
csrc/xsec/combine.hip.

Tolerance of the max_icir comparison: w = C^-1 m with C the sample covariance (ddof 1) of the window and m its mean, both by np.sum in
np.longdouble, solved by Gaussian elimination with partial pivoting in np.longdouble (numpy.linalg has no longdouble solve), on
well-conditioned IC series without holes: independent normal draws of size 0.05, K in {1, 3, 8} x window in {K + 1, 20, 252}, 40 rows
each.  The deviation of a row is max_k |w_k - ref_k| / max_k |ref_k|: a single weight can cancel to nearly zero, the row's largest
cannot.  Worst deviation measured on this data: 9.79e-12 (K = 8 at window = 9, where eight degrees of freedom leave the 8 x 8 matrix C
nearly singular; K = 3 at window = 4 1.28e-12 for the same reason; the seven longer windows stay below 4e-14); allowed: 16 x that."""
import importlib
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_combine_ref as R
from xsec_rolling_ref import shift

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL
INF, NAN = np.inf, np.nan

MEASURED = 9.79e-12     # worst row deviation of the max_icir weights from the longdouble solution over the nine cases below
ALLOWED = 16 * MEASURED


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same(got, exp):
    assert np.shape(got) == np.shape(exp) and (bits(got) == bits(exp)).all(), (got, exp)


def ic_series(K, T, seed, holes=True):
    rng = np.random.default_rng(seed)
    ic = 0.03 + 0.05 * rng.standard_normal((K, T))
    if holes and T > 8:
        ic[rng.integers(0, K, 3), rng.integers(0, T, 3)] = NULL
    return ic


# ---------------------------------------------------------------- ic / icir are rolling_ic read lag days earlier
@pytest.mark.parametrize("lag", [0, 1, 5])
@pytest.mark.parametrize("window", [1, 2, 20])
def test_ic_and_icir_are_the_oracles_rolling_ic_shifted_by_the_lag(window, lag):
    from oracle import pq_oracle as oracle
    T = 300
    for K in (1, 3):
        ic = ic_series(K, T, 10 * window + lag + K)
        roll = [oracle.rolling_ic(np.ascontiguousarray(ic[k]), window) for k in range(K)]
        mean = shift(np.stack([m for m, _ in roll]), lag, NULL)
        ir = shift(np.stack([r for _, r in roll]), lag, NULL)
        for method, exp in (("ic", mean), ("icir", ir)):
            if window < R.min_window(method, K):
                continue
            got = R.weights(ic, method, window, lag)
            row = ~R.isnull(exp).any(axis=0)                    # a row has its K weights or none
            assert row[window + lag:].sum() > (T - window - lag) // 2 and not row[:window + lag - 1].any()
            same(got[:, row], exp[:, row])
            assert R.isnull(got[:, ~row]).all()
            if K == 1:
                same(got, exp)


@pytest.mark.parametrize("method", R.METHODS)
def test_the_restatement_is_causal_and_the_lag_is_a_shift(method):
    """what tests/test_factor_combine_gpu.py shares one reference by: the weights of a series are the first rows of the weights of any
    longer one, and the weights at a lag are the weights at lag 0 moved by it"""
    K, T, w = 3, 90, 6
    ic = ic_series(K, T, 77)
    ic[1, 40], ic[2, 50] = INF, NAN
    base = R.weights(ic, method, w, 0)
    assert (~R.isnull(base[:, w:])).sum() > base[:, w:].size // 2 and R.isnull(base[:, w:]).any()
    for lag in (0, 1, 5, 89, 90, 200):
        moved = shift(base, lag, NULL)
        same(R.weights(ic, method, w, lag), moved)
        for n in (1, w + lag - 1, w + lag, 41, 89):
            if 1 <= n <= T:
                same(R.weights(ic[:, :n], method, w, lag), moved[:, :n])


# ---------------------------------------------------------------- hand-derived tables
IC2 = np.array([[1, 3, 5, NULL, 2, 4, 9], [2, 2, 6, 1, 1, 3, 0]], dtype=np.float64)


def test_weights_hand_table_k2_window2_lag1():
    """row t reads days t - 2 and t - 1: rows 0, 1 lie before the series, rows 4, 5 hold the NULL of day 3"""
    same(R.weights(IC2, "ic", 2, 1), [[NULL, NULL, 2, 4, NULL, NULL, 3], [NULL, NULL, 2, 4, NULL, NULL, 2]])
    # (1 3): mean 2, q2 = 2, sd sqrt(2); (2 2): sd 0 -> the row is NULL in both; (3 5) (2 6): 4 / sqrt(2), 4 / sqrt(8); (2 4) (1 3)
    r2, r8 = math.sqrt(2.0), math.sqrt(8.0)
    same(R.weights(IC2, "icir", 2, 1), [[NULL, NULL, NULL, 4 / r2, NULL, NULL, 3 / r2], [NULL, NULL, NULL, 4 / r8, NULL, NULL, 2 / r2]])
    # lag 0 reads days t - 1 and t; lag 5 leaves one row
    same(R.weights(IC2, "ic", 2, 0), [[NULL, 2, 4, NULL, NULL, 3, 6.5], [NULL, 2, 4, NULL, NULL, 2, 1.5]])
    same(R.weights(IC2, "ic", 2, 5), [[NULL] * 6 + [2.0], [NULL] * 6 + [2.0]])
    same(R.weights(IC2, "ic", 2, 6), np.full((2, 7), NULL))
    same(R.weights(IC2[1], "ic", 1, 1), [[NULL, 2, 2, 6, 1, 1, 3]])


def test_max_icir_hand_table():
    # K = 1: mean / variance.  (1 3): 2 / 2; (3 5): 4 / 2; a constant window has no pivot
    same(R.weights([1, 3, 5, 5, 5], "max_icir", 2, 0), [[NULL, 1.0, 2.0, NULL, NULL]])
    # K = 2, window 3: ic0 = 1 2 3, ic1 = 1 0 2: means 2 1, deviations (-1 0 1) (0 -1 1), C = [[1, .5], [.5, 1]]; D = 1, .75; L10 = .5;
    # z = 2, 1 - .5 * 2 = 0; w1 = 0 / .75, w0 = 2 / 1 - .5 * 0
    same(R.weights([[1, 2, 3], [1, 0, 2]], "max_icir", 3, 0), [[NULL, NULL, 2.0], [NULL, NULL, 0.0]])
    # two proportional series: the second pivot is 0
    assert R.isnull(R.weights([[1, 2, 4, 3], [2, 4, 8, 6]], "max_icir", 3, 0)).all()
    assert not R.isnull(R.weights([[1, 2, 4, 3], [2, 4, 8, 6]], "icir", 3, 0)[:, 2:]).any()


def test_a_nan_weight_makes_the_row_null_and_an_inf_ic_is_a_value():
    ic = np.array([[1, INF, 2, 3, -INF, INF, 1, 2], [1, 2, 3, 4, 5, 6, 7, 8]], dtype=np.float64)
    got = R.weights(ic, "ic", 2, 0)
    assert R.isnull(got[:, 0]).all() and got[0, 1] == INF and got[0, 4] == -INF and got[1, 4] == 4.5
    assert R.isnull(got[:, 5]).all() and got[0, 7] == 1.5       # -inf + inf: NaN in factor 0 takes factor 1's weight with it
    ic[0, 1] = NAN                                              # a NaN that is not NULL is a value too, and its mean is NaN
    assert R.isnull(R.weights(ic, "ic", 2, 0)[:, 1:3]).all()


def test_composite_hand_table():
    w = np.array([[1, NULL, 0], [-3, 2, 0]], dtype=np.float64)
    f = np.array([[[1, 2, 3], [NULL, 1, 1]], [[2, 2, 2], [1, INF, 4]]], dtype=np.float64)
    # day 0: D = 4, 1 * 1 - 3 * 2 = -5; symbol 1 lacks factor 0.  day 1: a NULL weight.  day 2: D = 0
    same(R.composite(f, w, True), [[-1.25, NULL, NULL], [NULL, NULL, NULL]])
    same(R.composite(f, w, False), [[-5.0, NULL, 0.0], [NULL, NULL, 0.0]])
    same(R.composite(f, [1.0, -3.0], True), [[-1.25, -1.0, -0.75], [NULL, NULL, -2.75]])
    same(R.composite(f[:1], [[2.0, -2.0, NAN]], True), [[1.0, -2.0, NULL], [NULL, -1.0, NULL]])
    same(R.composite(f[:1], [[2.0, -2.0, INF]], True), [[1.0, -2.0, NULL], [NULL, -1.0, NULL]])     # inf / inf
    assert R.composite(np.empty((2, 0, 3)), w).shape == (0, 3) and R.composite(np.empty((2, 4, 0)), np.empty((2, 0))).shape == (4, 0)


# ---------------------------------------------------------------- max_icir against the longdouble solution
def longdouble_max_ir(X):
    """C^-1 m of the window X [K, w]: sample covariance and mean in np.longdouble, Gaussian elimination with partial pivoting"""
    ld = np.longdouble
    X = X.astype(ld)
    K, w = X.shape
    m = X.sum(axis=1) / ld(w)
    d = X - m[:, None]
    A = np.array([[(d[j] * d[l]).sum() / ld(w - 1) for l in range(K)] for j in range(K)], dtype=ld)
    b = m.copy()
    for c in range(K):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        for r in range(c + 1, K):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(K, dtype=ld)
    for r in range(K - 1, -1, -1):
        x[r] = (b[r] - (A[r, r + 1:] * x[r + 1:]).sum()) / A[r, r]
    return x


DEVIATION_CASES = [(K, w) for K in (1, 3, 8) for w in (K + 1, 20, 252)]


def deviation(K, window):
    rows = 40
    T = window + rows - 1
    ic = 0.05 * np.random.default_rng(1000 * K + window).standard_normal((K, T))
    got = R.weights(ic, "max_icir", window, 0)
    assert not R.isnull(got[:, window - 1:]).any() and R.isnull(got[:, :window - 1]).all()
    worst = 0.0
    for t in range(window - 1, T):
        ref = longdouble_max_ir(ic[:, t - window + 1:t + 1])
        worst = max(worst, float(np.max(np.abs(got[:, t].astype(np.longdouble) - ref)) / np.max(np.abs(ref))))
    return worst


@pytest.mark.parametrize("K,window", DEVIATION_CASES)
def test_max_icir_against_the_longdouble_covariance_solve(K, window):
    dev = deviation(K, window)
    print(f"K={K} window={window}: worst row deviation {dev:.3e} (allowed {ALLOWED:.3e})")
    assert dev <= ALLOWED


def test_max_icir_is_icir_scaled_for_one_factor_and_solves_its_system():
    """K = 1: C^-1 m = m / var = icir / sd; K = 3: C w reproduces m"""
    ic = ic_series(3, 120, 5, holes=False)
    one = R.weights(ic[0], "max_icir", 20, 1)
    ir = R.weights(ic[0], "icir", 20, 1)
    m = R.weights(ic[0], "ic", 20, 1)
    live = ~R.isnull(one)
    assert (live == ~R.isnull(ir)).all() and live[0, 21:].all()
    np.testing.assert_allclose(one[live], ir[live] ** 2 / m[live], rtol=1e-13)
    w = R.weights(ic, "max_icir", 20, 0)
    for t in (19, 60, 119):
        win = ic[:, t - 19:t + 1]
        np.testing.assert_allclose(np.cov(win) @ w[:, t], win.mean(axis=1), rtol=1e-11)


# ---------------------------------------------------------------- the public surface
def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    sig = inspect.signature(pq.Factor.combine)
    want = [("factors", None), ("next_return", "None"), ("method", "icir"), ("window", 60), ("lag", 1), ("rank", False), ("weights", "None"),
            ("normalize", True)]
    assert list(sig.parameters) == ["self"] + [p for p, _ in want]
    for p, default in want:
        d = sig.parameters[p].default
        assert (d is inspect.Parameter.empty) if default is None else (d is None if default == "None" else d == default), p
    doc = pq.Factor.combine.__doc__
    assert "lag >= h" in doc and "standardise" in doc
    assert tuple(sorted(api.COMBINE_METHODS, key=api.COMBINE_METHODS.get)) == R.METHODS and sorted(api.COMBINE_METHODS.values()) == [0, 1, 2]
    assert all(api.combine_min_window(api.COMBINE_METHODS[m], K) == R.min_window(m, K) for m in R.METHODS for K in range(1, 9))
    assert api.COMBINE_MAX_LAG == R.MAX_LAG == api.ROLLING_MAX_WINDOW and api.REGRESS_MAX_K == R.MAX_K
    assert list(inspect.signature(api.factor_combine_weights).parameters) == ["ic", "method", "window", "lag"]
    assert list(inspect.signature(api.factor_combine).parameters) == ["factors", "weights", "normalize"]
    assert inspect.signature(api.factor_combine).parameters["normalize"].default is True
    assert "D-30" in (importlib.import_module("polars_quant_amd.factor").__doc__ or "")
    raw = (ROOT / "include" / "pq_hip.h").read_text()
    assert "D-30" in raw
    for nm, v in (("PQ_COMBINE_IC", 0), ("PQ_COMBINE_ICIR", 1), ("PQ_COMBINE_MAX_ICIR", 2)):
        assert re.search(rf"^#define {nm} {v}$", raw, flags=re.M), nm
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {"pq_factor_combine_weights": ["pq_ctx *", "const double *ic", "int32_t k", "int64_t len", "int32_t method", "int64_t window",
                                            "int64_t lag", "double *weights"],
              "pq_factor_combine": ["pq_ctx *", "const pq_batch *", "const double *const *factors", "int32_t k", "const double *weights",
                                    "int32_t normalize", "double *out"]}
    for fn, params in protos.items():
        decl = re.search(rf"pq_status\s+{fn}\s*\(([^)]*)\)", txt)
        assert decl, f"{fn} is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, fn
    assert re.search(r"^factor_combine_weights\s+i\s+ppilillp$", _lib._SIGNATURES, flags=re.M)
    assert re.search(r"^factor_combine\s+i\s+pBpipip$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/combine.hip" in mk and mk.count("xsec/combine.resources.txt") == 1
    assert "polars_quant_amd/csrc/xsec/combine.resources.txt" in (ROOT / ".gitignore").read_text().split()


ONES = np.ones((3, 40))
IC3 = np.ones((3, 40))


@pytest.mark.parametrize("call, msg", [
    (lambda f, a: f.combine([ONES, ONES], ONES, method="mean"), "method"),
    (lambda f, a: f.combine([ONES, ONES], ONES, method=1), "method"),
    (lambda f, a: f.combine([ONES, ONES]), "next_return"),
    (lambda f, a: f.combine([ONES, ONES], method="ic"), "next_return"),
    (lambda f, a: f.combine([ONES, ONES], method="max_icir"), "next_return"),
    (lambda f, a: f.combine([ONES, ONES], ONES, weights=[1.0, 2.0]), "weights"),
    (lambda f, a: f.combine([ONES, ONES], ONES, method="equal", weights=np.ones((2, 40))), "weights"),
    (lambda f, a: f.combine([ONES, ONES], weights=[1.0, 2.0, 3.0]), "weights"),
    (lambda f, a: f.combine([ONES, ONES], weights=np.ones((2, 39))), "weights"),
    (lambda f, a: f.combine([ONES, ONES], np.ones((3, 41))), "next_return"),
    (lambda f, a: f.combine([ONES, np.ones((3, 41))], ONES), "shape"),
    (lambda f, a: f.combine([ONES] * 9, ONES), "number of factors"),
    (lambda f, a: f.combine([], method="equal"), "number of factors"),
    (lambda f, a: f.combine(np.ones((3, 40)), method="equal"), r"\[K, N, T\]"),
    (lambda f, a: f.combine([ONES, ONES], ONES, window=1), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, method="max_icir", window=2), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, method="ic", window=0), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, window=1025), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, window=20.0), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, window=True), "window"),
    (lambda f, a: f.combine([ONES, ONES], ONES, lag=-1), "lag"),
    (lambda f, a: f.combine([ONES, ONES], ONES, lag=1025), "lag"),
    (lambda f, a: f.combine([ONES, ONES], ONES, lag=1.0), "lag"),
    (lambda f, a: a.factor_combine_weights(IC3, 3, 20, 1), "method"),
    (lambda f, a: a.factor_combine_weights(IC3, "icir", 20, 1), "method"),
    (lambda f, a: a.factor_combine_weights(IC3, True, 20, 1), "method"),
    (lambda f, a: a.factor_combine_weights(IC3, 2, 3, 1), "window"),
    (lambda f, a: a.factor_combine_weights(IC3, 1, 1, 1), "window"),
    (lambda f, a: a.factor_combine_weights(IC3, 0, 1025, 1), "window"),
    (lambda f, a: a.factor_combine_weights(IC3, 0, 20, -1), "lag"),
    (lambda f, a: a.factor_combine_weights(IC3, 0, 20, 1025), "lag"),
    (lambda f, a: a.factor_combine_weights(np.ones((9, 40)), 0, 20, 1), "number of factors"),
    (lambda f, a: a.factor_combine_weights(np.ones((2, 3, 40)), 0, 20, 1), r"\[K, T\]"),
    (lambda f, a: a.factor_combine([ONES, ONES], np.ones(3)), "weights"),
    (lambda f, a: a.factor_combine([ONES, ONES], np.ones((2, 41))), "weights"),
    (lambda f, a: a.factor_combine([ONES, np.ones(40)], np.ones(2)), "shape"),
    (lambda f, a: a.factor_combine([np.ones(40)], np.ones(1)), r"must be \[N, T\]"),
])
def test_argument_errors_raise_before_device_work(call, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(pq.Factor(), api)


# ---------------------------------------------------------------- the kernels' resources
def test_no_instantiation_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/combine.hip (combine.resources.txt, from hipcc's
    kernel-resource-usage remarks): the weights kernel once per (K, method), the combine kernel once per K, none with scratch or a
    spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "combine.resources.txt"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    found = re.findall(r"Function Name: \S*?(cb_\w+?_kernel)ILi(\d+)E(?:Li(\d+)E)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+"
                       r"Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [("cb_weights_kernel", K, m) for K in range(1, 9) for m in range(3)] + [("cb_combine_kernel", K, -1) for K in range(1, 9)]
    assert sorted((k, int(K), int(m) if m else -1) for k, K, m, *_ in found) == sorted(want)
    for k, K, m, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, K, m, vgprs, scratch, occ, spill)
