"""-m gpu: the regressions and t-tests of D-17 (csrc/xsec/regress.hip) against the numpy restatement in tests/xsec_regress_ref.py.
coef / intercept / t / R^2 / n and the Fama-MacBeth n_days / mean / std / t are compared bit for bit; p-values against
scipy.special.stdtr within |dp| <= 1e-11 p + 1e-300."""
import numpy as np
import pytest

import xsec_regress_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(37, 50), (300, 131), (2, 3), (1, 5)]
KS = [1, 2, 3, 8]
TS_SHAPES = [(37, 50), (20, 600), (300, 131), (2, 3), (1, 5)]


def cases(shapes):
    """every shape at every K of KS; the K between them (the fit of xsec_ols.h is instantiated for 1 .. 8) at (37, 50) only"""
    return [pytest.param(s, K, id=f"{s[0]}x{s[1]}-{K}") for K in KS for s in shapes] + \
           [pytest.param((37, 50), K, id=f"37x50-{K}") for K in (4, 5, 6, 7)]


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def same(name, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    g = got.astype(np.float64).view(np.uint64) if got.dtype != np.int32 else got
    e = exp.astype(np.float64).view(np.uint64) if exp.dtype != np.int32 else exp.astype(np.int32)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def close_p(name, got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, name
    gn, en = np.isnan(got), np.isnan(exp)
    assert (gn == en).all(), f"{name}: NaN / NULL pattern differs"
    assert (R.isnull(got) == R.isnull(exp)).all(), f"{name}: NULL pattern differs"
    g, e = got[~gn], exp[~en]
    err = np.abs(g - e) - (1e-11 * e + 1e-300)
    assert (err <= 0).all(), f"{name}: worst |dp| excess {err.max()!r}"


def to_dev(a, pitch=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1 or pitch is None:
        return torch.from_numpy(a).cuda()
    n, T = a.shape
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(a).cuda()
    return buf[:, :T]


def make(K, n, T, seed, special=True):
    """K factors and a return [n, T]; special: NULL / NaN / inf holes, and (where the shape allows) a singular day, a day with only
    K + 1 members, a day with exactly K + 2, a perfect-fit day and a constant-return day"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, n, T))
    r = (0.1 * np.arange(1, K + 1)[:, None, None] * F).sum(0) + 0.5 * rng.standard_normal((n, T))
    if special:
        F[rng.random((K, n, T)) < 0.03] = R.NULL
        F[rng.random((K, n, T)) < 0.02] = np.nan
        r[rng.random((n, T)) < 0.03] = R.NULL
        r[rng.random((n, T)) < 0.01] = np.inf
        if T >= 6 and n >= K + 3:
            F[K - 1, :, 0] = F[0, :, 0] if K > 1 else 2.5             # singular: collinear (constant at K = 1)
            r[K + 1:, 1] = R.NULL                                      # n = K + 1
            r[K + 2:, 2] = R.NULL                                      # n = K + 2 (when the first K + 2 are members)
            F[:, :K + 2, 2] = rng.integers(-4, 5, (K, K + 2))
            r[:K + 2, 2] = rng.integers(-4, 5, K + 2)
            Fi = rng.integers(-8, 9, (K, n)).astype(np.float64)        # perfect fit on integers
            F[:, :, 3] = Fi
            r[:, 3] = 0.5 + (0.25 * Fi).sum(0)
            r[:, 4] = 0.375                                            # constant returns
    return F, r


def check_xsec(pq, F, r, pitch=None, summary=True):
    from polars_quant_amd import api
    K = F.shape[0]
    got = api.xsec_regress([to_dev(f, pitch) for f in F], to_dev(r, pitch), summary=summary)
    exp = R.xsec_regress(list(F), r)
    tag = f"K={K} {r.shape} pitch={pitch}"
    same(f"coef {tag}", got["coef"].cpu().numpy(), exp["coef"])
    same(f"t {tag}", got["t_stat"].cpu().numpy(), exp["t"])
    same(f"r2 {tag}", got["r_squared"].cpu().numpy(), exp["r2"])
    same(f"n {tag}", got["n"].cpu().numpy(), exp["n"])
    close_p(f"p {tag}", got["p_value"].cpu().numpy(), exp["p"])
    if summary:
        s = got["summary"].cpu().numpy()
        es = R.fm_summary(exp["coef"])
        same(f"summary {tag}", s[:, :4], es[:, :4])
        close_p(f"summary p {tag}", s[:, 4], es[:, 4])
    return got, exp


def check_ts(pq, cols, r, pitch=None):
    """ts_regress on factor columns cols ([N, T] or a [T] series each) and returns r [N, T] against the restatement"""
    from polars_quant_amd import api
    got = api.ts_regress([to_dev(c, pitch) for c in cols], to_dev(r, pitch))
    exp = R.ts_regress(cols, r)
    ser = "".join("s" if np.ndim(c) == 1 else "m" for c in cols)
    tag = f"ts K={len(cols)} {r.shape} factors={ser} pitch={pitch}"
    same(f"coef {tag}", got["coef"].cpu().numpy(), exp["coef"])
    same(f"t {tag}", got["t_stat"].cpu().numpy(), exp["t"])
    same(f"r2 {tag}", got["r_squared"].cpu().numpy(), exp["r2"])
    same(f"n {tag}", got["n_obs"].cpu().numpy(), exp["n"])
    close_p(f"p {tag}", got["p_value"].cpu().numpy(), exp["p"])
    return got, exp


@pytest.mark.parametrize("shape,K", cases(SHAPES))
def test_xsec_regress_bitwise(pq, shape, K):
    n, T = shape
    F, r = make(K, n, T, 100 * K + n + T)
    got, exp = check_xsec(pq, F, r)
    if T >= 6 and n >= K + 3:    # the forced days really are what they claim
        assert R.isnull(exp["coef"][:, 0]).all() and R.isnull(exp["coef"][:, 1]).all()
        assert exp["n"][1] <= K + 1


@pytest.mark.parametrize("K", [1, 3])
def test_xsec_regress_odd_pitch_and_clean_data(pq, K):
    F, r = make(K, 41, 77, 7 + K, special=False)
    check_xsec(pq, F, r, pitch=83)
    F, r = make(K, 300, 131, 9 + K)
    check_xsec(pq, F, r, pitch=139)


@pytest.mark.parametrize("shape,K", cases(TS_SHAPES))
def test_ts_regress_bitwise(pq, shape, K):
    n, T = shape
    F, r = make(K, n, T, 7 * K + n + T)
    rng = np.random.default_rng(K + T)
    cols = [F[j] for j in range(K)]
    mkt = rng.standard_normal(T)
    mkt[rng.random(T) < 0.05] = R.NULL
    cols[0] = mkt                                          # a [T] series shared by every symbol
    if K >= 3:
        cols[2] = rng.standard_normal(T)
    if n >= 2 and T >= 3:
        r[1, 2:] = R.NULL                                  # a symbol with too few days
    for pitch in (None, T + 5):
        check_ts(pq, cols, r, pitch)


def test_factor_methods(pq):
    from polars_quant_amd import api
    F, r = make(3, 300, 131, 77)
    fac = pq.Factor()
    fr = fac.factor_return(F[0], r)
    exp = R.xsec_regress([F[0]], r)
    same("factor_return", fr["factor_return"].cpu().numpy(), exp["coef"][0])
    same("intercept", fr["intercept"].cpu().numpy(), exp["coef"][1])
    same("factor_return t", fr["t_stat"].cpu().numpy(), exp["t"][0])
    same("factor_return r2", fr["r_squared"].cpu().numpy(), exp["r2"])
    same("factor_return n", fr["n"].cpu().numpy(), exp["n"])
    fm = fac.fama_macbeth(torch.from_numpy(F), r)
    exp = R.xsec_regress(list(F), r)
    es = R.fm_summary(exp["coef"])
    for j, k in enumerate(("n_days", "mean_coef", "std_coef", "t_stat")):
        same(f"fama_macbeth {k}", fm[k].cpu().numpy(), es[:, j])
    close_p("fama_macbeth p", fm["p_value"].cpu().numpy(), es[:, 4])
    same("fama_macbeth daily coef", fm["daily"]["coef"].cpu().numpy(), exp["coef"])
    tsr = fac.time_series_regression([F[0], F[1][0]], r)
    exp = R.ts_regress([F[0], F[1][0]], r)
    same("time_series_regression", tsr["coefficient"].cpu().numpy(), exp["coef"])
    same("time_series_regression n", tsr["n_obs"].cpu().numpy(), exp["n"])
    for method in ("pearson", "spearman"):
        it = fac.ic_test(F[0], r, method=method)
        ic, nv = api.factor_ic(F[0], r, 0 if method == "pearson" else 1)
        same(f"ic_test {method} ic", it["ic"].cpu().numpy(), ic.cpu().numpy())
        et, ep = R.corr_t_test(ic.cpu().numpy(), nv.cpu().numpy())
        same(f"ic_test {method} t", it["t_stat"].cpu().numpy(), et)
        close_p(f"ic_test {method} p", it["p_value"].cpu().numpy(), ep)


def test_corr_t_test_edges(pq):
    from polars_quant_amd import api
    corr = np.array([np.nan, R.NULL, 0.5, 0.5, 1.0, -1.0, 0.0, -0.25])
    n = np.array([10, 10, 2, 3, 10, 10, 10, 40], dtype=np.int32)
    t, p = api.corr_t_test(to_dev(corr), torch.from_numpy(n).cuda())
    et, ep = R.corr_t_test(corr, n)
    same("corr t", t.cpu().numpy(), et)
    close_p("corr p", p.cpu().numpy(), ep)
    assert p.cpu().numpy()[6] == 1.0


def test_pvalue_grid_against_stdtr(pq):
    """df in {1, 2, 3, 5, 10, 100, 1000, 5039, 1e5}, |t| in [0, 50] (t = 0 -> p = 1), through the correlation form"""
    from polars_quant_amd import api
    from scipy.special import stdtr
    dfs = [1, 2, 3, 5, 10, 100, 1000, 5039, 100000]
    ts = np.concatenate([[0.0, 1e-9, 1e-4], np.linspace(0.0, 50.0, 2001)[1:], [1.7, 1.73, 1.75, 1.8, 2.0, 3.0]])
    df = np.repeat(np.array(dfs, dtype=np.float64), len(ts))
    tt = np.tile(ts, len(dfs)) * np.tile([1.0, -1.0], len(df) // 2 + 1)[:len(df)]
    corr = tt / np.sqrt(df + tt * tt)
    nv = (df + 2).astype(np.int32)
    t, p = api.corr_t_test(to_dev(corr), torch.from_numpy(nv).cuda())
    t, p = t.cpu().numpy(), p.cpu().numpy()
    exp = 2.0 * stdtr(df, -np.abs(t))
    err = np.abs(p - exp) - (1e-11 * exp + 1e-300)
    i = int(np.argmax(err))
    assert (err <= 0).all(), f"df={df[i]} t={t[i]!r}: p={p[i]!r} stdtr={exp[i]!r}"
    assert (p[t == 0.0] == 1.0).all() and (t == 0.0).sum() >= len(dfs)


def test_full_size_config4_fama_macbeth_k3(pq):
    """config 4 (10 000 x 5 040), K = 3, every day bit for bit (the restatement runs in slices of days)"""
    from polars_quant_amd import api
    N, T, K = 10000, 5040, 3
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    Fd = torch.randn((K, N, T), dtype=torch.float64, device="cuda", generator=g)
    rd = 0.05 * Fd[0] - 0.02 * Fd[2] + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
    rd[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
    got = api.xsec_regress([Fd[j] for j in range(K)], rd)
    F, r = Fd.cpu().numpy(), rd.cpu().numpy()
    coef, tst, pv, r2, n = (got[k].cpu().numpy() for k in ("coef", "t_stat", "p_value", "r_squared", "n"))
    for t0 in range(0, T, 630):
        sl = slice(t0, t0 + 630)
        exp = R.xsec_regress([F[j][:, sl] for j in range(K)], r[:, sl])
        same(f"coef days {t0}", coef[:, sl], exp["coef"])
        same(f"t days {t0}", tst[:, sl], exp["t"])
        same(f"r2 days {t0}", r2[sl], exp["r2"])
        same(f"n days {t0}", n[sl], exp["n"])
        close_p(f"p days {t0}", pv[:, sl], exp["p"])
    es = R.fm_summary(coef)
    s = got["summary"].cpu().numpy()
    same("summary", s[:, :4], es[:, :4])
    close_p("summary p", s[:, 4], es[:, 4])
