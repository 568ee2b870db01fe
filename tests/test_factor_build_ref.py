"""not-gpu: the numpy restatement of decision D-20 (tests/xsec_build_ref.py: rank, normalize, weighted, ratio, diff) against
hand-derived tables and against independent code (scipy.stats.rankdata, pandas.Series.rank, plain numpy), and the public surface of the
feature: method names and defaults, the argument errors that must come before any device work, the C declarations."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_build_ref as R

ROOT = Path(__file__).resolve().parent.parent
NULL = R.NULL


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same(got, exp):
    assert (bits(got) == bits(exp)).all(), (got, exp)


# ---------------------------------------------------------------- hand-derived tables
# one day of five symbols: a tie pair (2.0, 2.0) and a NULL; members 3.0, 2.0, 2.0, -1.0 -> sorted -1, 2, 2, 3
DAY = np.array([[3.0], [2.0], [NULL], [2.0], [-1.0]])


def test_rank_hand_table():
    same(R.rank(DAY), [[4.0], [2.5], [NULL], [2.5], [1.0]])                           # tie run [1, 3): ((1 + 1) + 3) / 2 = 2.5
    same(R.rank(DAY, descending=True), [[1.0], [2.5], [NULL], [2.5], [4.0]])          # n + 1 - rank, n = 4
    same(R.rank(DAY, "pct"), [[1.0], [0.625], [NULL], [0.625], [0.25]])
    same(R.rank(DAY, "pct", True), [[0.25], [0.625], [NULL], [0.625], [1.0]])
    same(R.rank(DAY, "quantile"), [[0.875], [0.5], [NULL], [0.5], [0.125]])           # (rank - 0.5) / 4


def test_rank_signed_zeros_tie_and_non_finite_values_are_outside():
    x = np.array([[0.0], [-0.0], [np.inf], [np.nan], [-np.inf], [1.0]])
    same(R.rank(x), [[1.5], [1.5], [NULL], [NULL], [NULL], [3.0]])
    same(R.rank(np.full((3, 2), NULL)), np.full((3, 2), NULL))                        # a day without members


def test_minmax_hand_table():
    same(R.minmax(DAY), [[1.0], [0.75], [NULL], [0.75], [0.0]])                       # (x + 1) / 4
    same(R.minmax(np.array([[2.0], [NULL], [2.0]])), [[NULL], [NULL], [NULL]])        # max == min: the whole day NULL
    same(R.minmax(np.array([[5.0], [NULL]])), [[NULL], [NULL]])                       # a day of one member
    same(R.minmax(np.array([[-0.0], [0.0], [4.0]])), [[0.0], [0.0], [1.0]])           # -0 is read as +0


def test_zscore_is_clean_standardize():
    import xsec_clean_ref as CR
    rng = np.random.default_rng(2)
    f = rng.standard_normal((40, 6))
    f[3, 2] = NULL
    same(R.normalize(f, "zscore"), CR.clean(f, standardize=True))
    z = R.normalize(DAY, "zscore")[:, 0]
    m = np.array([3.0, 2.0, 2.0, -1.0])
    np.testing.assert_allclose(z[[0, 1, 3, 4]], (m - m.mean()) / m.std(ddof=1), rtol=0, atol=1e-15)
    assert R.isnull(z[2])


def test_weighted_hand_tables():
    x = np.array([[3.0], [2.0], [NULL], [2.0], [-1.0]])
    w = np.array([[1.0], [2.0], [5.0], [NULL], [1.0]])
    same(R.weighted(x, w), [[0.75], [1.0], [NULL], [NULL], [-0.25]])                  # W = 1 + 2 + 1 = 4
    # two groups: codes 0, 1, 0, 1, -1 (unclassified) -> W0 = 1 + 3 = 4, W1 = 2 + 6 = 8
    x = np.array([[2.0], [4.0], [6.0], [8.0], [1.0]])
    w = np.array([[1.0], [2.0], [3.0], [6.0], [9.0]])
    g = np.array([0, 1, 0, 1, -1])
    same(R.weighted(x, w, g), [[0.5], [1.0], [4.5], [6.0], [NULL]])
    # a group whose weights cancel: W == 0 -> NULL, the other group untouched
    w2 = np.array([[1.0], [2.0], [-1.0], [6.0], [9.0]])
    same(R.weighted(x, w2, g), [[NULL], [1.0], [NULL], [6.0], [NULL]])
    same(R.weighted(x, w2), [[2.0 / 17.0], [8.0 / 17.0], [-6.0 / 17.0], [48.0 / 17.0], [9.0 / 17.0]])


def test_binary_hand_table():
    a = np.array([[6.0, NULL, 1.0, 0.0, -3.0]])
    b = np.array([[3.0, 2.0, 0.0, 0.0, NULL]])
    r = R.binary(a, b, "ratio")
    same(r[0, [0, 1, 2, 4]], [2.0, NULL, np.inf, NULL])
    assert np.isnan(r[0, 3]) and not R.isnull(r[0, 3])                                # 0 / 0: an IEEE NaN, not a NULL
    same(R.binary(a, b, "diff"), [[3.0, NULL, 1.0, 0.0, NULL]])
    same(R.binary(np.array([[1.0, 5.0]]), np.array([[-4.0, 2.0]]), "reldiff"), [[1.25, 1.5]])


# ---------------------------------------------------------------- independent code
def table(seed, n=300, T=9, discrete=False):
    rng = np.random.default_rng(seed)
    f = rng.integers(-2, 3, (n, T)).astype(np.float64) if discrete else rng.standard_normal((n, T))
    f[rng.random((n, T)) < 0.05] = NULL
    return rng, f


@pytest.mark.parametrize("discrete", [False, True])
def test_rank_equals_scipy_rankdata_and_pandas_pct(discrete):
    import pandas as pd
    from scipy.stats import rankdata
    _, f = table(5, discrete=discrete)
    for desc in (False, True):
        r, p = R.rank(f, "rank", desc), R.rank(f, "pct", desc)
        for t in range(f.shape[1]):
            m = R.valid(f[:, t])
            x = f[m, t] if not desc else -f[m, t]
            assert (r[m, t] == rankdata(x, method="average")).all()
            assert (p[m, t] == pd.Series(f[m, t]).rank(pct=True, ascending=not desc).to_numpy()).all()
            assert R.isnull(r[~m, t]).all() and R.isnull(p[~m, t]).all()


def test_quantile_is_a_mid_rank_position_inside_the_unit_interval():
    _, f = table(6, discrete=True)
    q, r = R.normalize(f, "quantile"), R.rank(f)
    m = R.valid(f)
    n = m.sum(axis=0)[None, :].repeat(f.shape[0], 0)
    assert ((q[m] > 0.0) & (q[m] < 1.0)).all()
    assert (q[m] == (r[m] - 0.5) / n[m]).all()


@pytest.mark.parametrize("n", [37, 256, 700])
def test_minmax_and_weighted_against_plain_numpy(n):
    """within rounding everywhere; exactly where one block holds the whole day (n <= 256: the blocked sum is the plain ascending sum)"""
    rng, f = table(n, n=n)
    w = np.exp(rng.standard_normal(f.shape))
    w[rng.random(f.shape) < 0.05] = NULL
    g = rng.integers(-1, 4, n)
    mm, wt, wg = R.minmax(f), R.weighted(f, w), R.weighted(f, w, g)
    for t in range(f.shape[1]):
        m = R.valid(f[:, t])
        x = f[m, t]
        assert (mm[m, t] == (x - x.min()) / (x.max() - x.min())).all() and R.isnull(mm[~m, t]).all()
        mw = m & R.valid(w[:, t])
        W = 0.0
        for v in w[mw, t]:
            W += v
        exp = f[mw, t] * w[mw, t] / (W if n <= 256 else np.sum(w[mw, t]))
        if n <= 256:
            assert (wt[mw, t] == exp).all()
        else:
            np.testing.assert_allclose(wt[mw, t], exp, rtol=1e-13, atol=0)
        assert R.isnull(wt[~mw, t]).all()
        for c in range(4):
            mg = mw & (g == c)
            np.testing.assert_allclose(wg[mg, t], f[mg, t] * w[mg, t] / np.sum(w[mg, t]), rtol=1e-13, atol=0)
            np.testing.assert_allclose(np.sum(wg[mg, t] / f[mg, t]), 1.0, rtol=0, atol=1e-12)
        assert R.isnull(wg[~mw | (g < 0), t]).all()


def test_descending_mid_rank_equals_scipy_rankdata():
    """rank(f, "quantile", True), which only pq_factor_rank's C ABI reaches: ((n + 1 - rank) - 0.5) / n, the mid-rank position of the
    descending order -- scipy's average rank of the negated keys, one subtraction and one division"""
    from scipy.stats import rankdata
    for discrete in (False, True):
        _, f = table(7, discrete=discrete)
        f[f == 0.0] = np.where(np.arange(int((f == 0.0).sum())) % 2 == 0, -0.0, 0.0)
        q = R.rank(f, "quantile", True)
        for t in range(f.shape[1]):
            m = R.valid(f[:, t])
            same(q[m, t], (rankdata(-f[m, t], method="average") - 0.5) / float(m.sum()))
            assert R.isnull(q[~m, t]).all()


def test_weighted_with_n_groups_below_the_largest_code():
    """codes >= n_groups, negative codes and the extreme int32 values are in no group: a plain per-group Python loop (n <= 256: the
    blocked sum is the plain ascending sum)"""
    rng, f = table(8, n=200, T=5)
    w = np.exp(rng.standard_normal(f.shape))
    w[rng.random(f.shape) < 0.05] = NULL
    kinds = np.array(list(range(-3, 9)) + [-2 ** 31, 2 ** 31 - 1], dtype=np.int64)
    for G, shape in ((4, (200,)), (4, (200, 5)), (1, (200, 5))):
        g = rng.choice(kinds, shape)
        got = R.weighted(f, w, g, G)
        g2 = np.broadcast_to(g[:, None] if g.ndim == 1 else g, f.shape)
        exp = np.full(f.shape, NULL)
        for t in range(f.shape[1]):
            for c in range(G):
                mem = [s for s in range(f.shape[0]) if g2[s, t] == c and R.valid(f[s, t]) and R.valid(w[s, t])]
                W = 0.0
                for s in mem:
                    W += w[s, t]
                for s in mem:
                    exp[s, t] = (f[s, t] * w[s, t]) / W
        same(got, exp)
        assert R.isnull(got[(g2 < 0) | (g2 >= G)]).all() and not R.isnull(got[g2 == 0]).all()


def test_minmax_subnormal_range_against_fractions():
    """members m * 2^-1074 over a range of 1 and of 1 000 units: the quotient is the correctly rounded m / range, in exact rationals"""
    from fractions import Fraction
    sub = 5e-324
    rng = np.random.default_rng(9)
    f = np.stack([np.where(rng.random(60) < 0.5, 0.0, sub), rng.integers(0, 1001, 60) * sub], axis=1)
    f[:3, 0] = -0.0, sub, NULL
    f[:2, 1] = 0.0, 1000 * sub
    got = R.minmax(f)
    for t in range(f.shape[1]):
        mem = [s for s in range(60) if R.valid(f[s, t])]
        lo, hi = min(Fraction(f[s, t]) for s in mem), max(Fraction(f[s, t]) for s in mem)
        assert hi > lo
        for s in mem:
            assert got[s, t] == float((Fraction(f[s, t]) - lo) / (hi - lo)), (s, t)
    assert R.isnull(got[2, 0]) and set(got[[0, 1], 0]) == {0.0, 1.0} and got[1, 1] == 1.0


# ---------------------------------------------------------------- the public surface
def test_public_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import api
    F = pq.Factor
    sig = {name: inspect.signature(getattr(F, name)) for name in ("rank", "normalize", "weighted", "ratio", "diff")}
    assert list(sig["rank"].parameters) == ["self", "factor", "ascending", "pct"]
    assert sig["rank"].parameters["ascending"].default is True and sig["rank"].parameters["pct"].default is False
    assert list(sig["normalize"].parameters) == ["self", "factor", "method"] and sig["normalize"].parameters["method"].default == "zscore"
    assert list(sig["weighted"].parameters) == ["self", "factor", "weight", "group"] and sig["weighted"].parameters["group"].default is None
    assert list(sig["ratio"].parameters) == ["self", "a", "b"]
    assert list(sig["diff"].parameters) == ["self", "a", "b", "normalize"] and sig["diff"].parameters["normalize"].default is False
    assert not hasattr(F, "clean")
    for fn in ("factor_rank", "factor_normalize", "factor_weighted", "factor_binary"):
        assert callable(getattr(api, fn))
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pq_hip.h").read_text(), flags=re.S)
    want = {"pq_factor_rank": ["pq_ctx", "pq_batch", "factor", "mode", "descending", "out"],
            "pq_factor_minmax": ["pq_ctx", "pq_batch", "factor", "out"],
            "pq_factor_weighted": ["pq_ctx", "pq_batch", "factor", "weight", "group", "group_stride", "n_groups", "out"],
            "pq_factor_binary": ["pq_ctx", "pq_batch", "a", "b", "op", "out"]}
    for name, args in want.items():
        decl = re.search(r"pq_status\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert decl, f"{name} is not declared"
        assert [re.findall(r"\w+", a)[-1] for a in decl.group(1).split(",")] == args
    assert "xsec/build.hip" in (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()


ONES = np.ones((3, 4))


@pytest.mark.parametrize("call, msg", [
    (lambda f: f.normalize(ONES, "robust"), "method must be"),
    (lambda f: f.normalize(ONES, None), "method must be"),
    (lambda f: f.rank(np.ones(4)), r"must be \[N, T\]"),
    (lambda f: f.weighted(ONES, np.ones((3, 5))), "shape"),
    (lambda f: f.weighted(ONES, ONES, np.array([0, 1, 256])), "group codes"),
    (lambda f: f.weighted(ONES, ONES, np.full((3, 4), 300)), "group codes"),
    (lambda f: f.weighted(ONES, ONES, np.array([0.5, 1.0, 2.0])), "integer"),
    (lambda f: f.weighted(ONES, ONES, np.array([0, 1])), r"group must be \[N\]"),
    (lambda f: f.ratio(ONES, np.ones((4, 3))), "shape"),
    (lambda f: f.diff(ONES, np.ones((3, 5)), normalize=True), "shape"),
])
def test_argument_errors_raise_before_device_work(call, msg):
    """on a machine without a GPU any device work raises PqError; these raise ValueError first"""
    import polars_quant_amd as pq
    with pytest.raises(ValueError, match=msg):
        call(pq.Factor())


def test_api_codes_raise_before_device_work():
    from polars_quant_amd import api
    for bad in (lambda: api.factor_rank(ONES, 3), lambda: api.factor_rank(ONES, 2, True), lambda: api.factor_binary(ONES, ONES, 3),
                lambda: api.factor_binary(ONES, ONES, -1)):
        with pytest.raises(ValueError):
            bad()
