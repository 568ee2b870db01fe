"""-m gpu: quantile sorts, long-short legs, turnover, coverage and IC statistics (D-15, csrc/xsec/sorts.hip) against the numpy
restatement in tests/xsec_ref.py.  Every comparison is bitwise: labels, counts, means, turnover, spread / long-short series and the
summary rows."""
import ctypes as C

import numpy as np
import pytest

import xsec_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QS = [2, 5, 10, 20]
LS = [(0.2, 0.2), (0.3, 0.3), (0.5, 0.5), (0.1, 0.4)]
SHAPES = [(37, 50), (300, 131), (1, 5), (2, 3)]


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
    if exp.dtype == np.float64:
        g, e = got.astype(np.float64).view(np.uint64), exp.view(np.uint64)
    else:
        g, e = got.astype(np.int64), exp.astype(np.int64)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def make(kind, n, T, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, T))
    r = 0.1 * f + rng.standard_normal((n, T)) * 0.02
    if kind == "nulls":            # 5 % null factors, 5 % null returns, some NaN returns
        f[rng.random((n, T)) < 0.05] = X.NULL
        r[rng.random((n, T)) < 0.05] = X.NULL
        r[rng.random((n, T)) < 0.02] = np.nan
    elif kind == "discrete":       # tie runs of about n / 3
        f = rng.integers(-1, 2, (n, T)).astype(np.float64)
        f[(f == 0) & (rng.random((n, T)) < 0.5)] = -0.0
    elif kind == "special":        # a constant day, a day with one pair, an all-null day, +-inf, signed zeros
        if T >= 4:
            f[:, 0] = 3.5
            r[1:, 1] = X.NULL
            f[:, 2] = X.NULL
            f[: n // 2, 3] = -0.0
            f[n // 2:, 3] = 0.0
        f[rng.random((n, T)) < 0.03] = np.inf
        f[rng.random((n, T)) < 0.03] = -np.inf
    return f, r


def to_dev(a, pitch=None):
    n, T = a.shape
    if pitch is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = torch.full((n, pitch), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(a).cuda()
    return buf[:, :T]


def check_groups(pq, f, r, mode, q=0, top=0.0, bottom=0.0, pitch=None):
    from polars_quant_amd import api
    fd, rd = to_dev(f, pitch), to_dev(r, pitch)
    if mode == 0:
        got = api.factor_quantiles(fd, rd, q, labels=True)
        key = "spread"
    else:
        got = api.factor_long_short(fd, rd, top, bottom, labels=True)
        key = "ls_return"
    torch.cuda.synchronize()
    exp = X.groups(f, r, mode, q, top, bottom)
    tag = f"mode{mode} q{q} top{top} bottom{bottom} {f.shape} pitch={pitch}"
    same("labels " + tag, got["labels"].cpu().numpy(), exp["labels"])
    same("count " + tag, got["count"].cpu().numpy(), exp["count"])
    same("mean_return " + tag, got["mean_return"].cpu().numpy(), exp["mean_return"])
    same("turnover " + tag, got["turnover"].cpu().numpy(), exp["turnover"])
    same(key + " " + tag, got[key].cpu().numpy(), exp["spread"])
    same("summary " + tag, got["summary"].cpu().numpy(), X.summary(exp))
    return got


@pytest.mark.parametrize("kind", ["plain", "nulls", "discrete", "special"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_quantiles_bitwise(pq, shape, kind):
    n, T = shape
    f, r = make(kind, n, T, 11 + n + T)
    for q in QS:
        check_groups(pq, f, r, 0, q)


@pytest.mark.parametrize("kind", ["plain", "nulls", "discrete", "special"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_long_short_bitwise(pq, shape, kind):
    n, T = shape
    f, r = make(kind, n, T, 23 + n + T)
    for top, bottom in LS:
        check_groups(pq, f, r, 1, 0, top, bottom)


def test_odd_row_pitch(pq):
    """batch stride > len (and odd): inputs read and labels written at the inputs' pitch"""
    f, r = make("nulls", 300, 131, 5)
    got = check_groups(pq, f, r, 0, 5, pitch=139)
    assert got["labels"].stride(0) == 139
    check_groups(pq, f, r, 1, 0, 0.3, 0.3, pitch=139)


def test_heavily_discrete_factor_long_tie_runs(pq):
    """a three-valued factor over 3 000 symbols: tie runs of about 1 000 entries per day"""
    rng = np.random.default_rng(3)
    f = rng.integers(-1, 2, (3000, 24)).astype(np.float64)
    f[f == 0] = np.where(rng.random(int((f == 0).sum())) < 0.5, -0.0, 0.0)
    r = np.round(rng.standard_normal((3000, 24)), 2)
    for q in (2, 5, 20):
        check_groups(pq, f, r, 0, q)
    check_groups(pq, f, r, 1, 0, 0.2, 0.2)


@pytest.mark.parametrize("n", [16385, 20000])
def test_wide_cross_section_segmented_sort(pq, n):
    """n_series > 16384: the segmented radix sort path, with ties and signed zeros"""
    rng = np.random.default_rng(n)
    T = 8
    f = rng.standard_normal((n, T))
    f[:, 1] = np.round(f[:, 1] * 2.0) / 2.0                 # a discrete day
    f[:, 2] = np.where(rng.random(n) < 0.5, -0.0, 0.0)     # all signed zeros: one tie run
    f[rng.random((n, T)) < 0.02] = X.NULL
    r = rng.standard_normal((n, T)) * 0.01
    r[rng.random((n, T)) < 0.02] = np.nan
    check_groups(pq, f, r, 0, 5)
    check_groups(pq, f, r, 0, 20)
    check_groups(pq, f, r, 1, 0, 0.1, 0.4)


def test_config4_full_size(pq):
    """10 000 x 5 040: per-day counts against Rank-IC's n_valid, 10 adjacent day pairs bitwise, summary from the day series"""
    from polars_quant_amd import api
    N, T = 10000, 5040
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
    r = 0.1 * f + torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
    r[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
    _, nv = api.factor_ic(f, r, 1)
    days = [1, 2, 777, 1500, 2519, 2520, 3333, 4000, 5038, 5039]
    need = X.sample_days(days, T)
    fs, rs = f[:, need].cpu().numpy(), r[:, need].cpu().numpy()
    local = [need.index(t) for t in days]
    for mode, q, top, bottom in ((0, 5, 0, 0), (0, 10, 0, 0), (1, 0, 0.2, 0.2)):
        got = api.factor_quantiles(f, r, q, labels=True) if mode == 0 else api.factor_long_short(f, r, top, bottom, labels=True)
        key = "spread" if mode == 0 else "ls_return"
        cnt = got["count"].cpu().numpy()
        if mode == 0:
            same(f"count sum q{q}", cnt.sum(axis=0), nv.cpu().numpy())
        exp = X.groups(fs, rs, mode, q, top, bottom, days=local)
        same("labels", got["labels"][:, days].cpu().numpy(), exp["labels"])
        for k in ("count", "mean_return", "turnover"):
            same(f"{k} mode{mode}", got[k][:, days].cpu().numpy(), exp[k])
        same(key, got[key][days].cpu().numpy(), exp["spread"])
        mean, tov, spr = got["mean_return"].cpu().numpy(), got["turnover"].cpu().numpy(), got[key].cpu().numpy()
        rows = [X.summary_row(mean[i], tov[i]) for i in range(mean.shape[0])] + [X.summary_row(spr)]
        same("summary", got["summary"].cpu().numpy(), np.array(rows))


def test_coverage_and_ic_stats(pq):
    from polars_quant_amd import api
    for shape in SHAPES + [(300, 131)]:
        f, r = make("special", *shape, 9)
        f2, _ = make("nulls", *shape, 10)
        for ff in (f, f2):
            same(f"coverage {shape}", api.factor_coverage(to_dev(ff)).cpu().numpy(), X.coverage(ff))
            for method in (0, 1):
                ic, _ = api.factor_ic(to_dev(ff), to_dev(r), method)
                same(f"ic_stats {shape} {method}", api.ic_stats(ic).cpu().numpy(), X.ic_stats(ic.cpu().numpy()))
    same("ic_stats flat", api.ic_stats(torch.full((4,), 0.25, dtype=torch.float64, device="cuda")).cpu().numpy(),
         X.ic_stats(np.full(4, 0.25)))


def test_factor_methods(pq):
    f, r = make("nulls", 300, 131, 17)
    fac = pq.Factor()
    exp = X.groups(f, r, 0, 5)
    s = X.summary(exp)
    q = fac.quantile(f, r)
    same("quantile", q["mean_return"].cpu().numpy(), exp["mean_return"])
    ps = fac.portfolio_sorts(f, r)
    assert ps["quantile"].cpu().tolist() == [0, 1, 2, 3, 4, -1]
    for i, k in ((1, "mean_return"), (2, "std_return"), (3, "sharpe")):
        same("portfolio_sorts " + k, ps[k].cpu().numpy(), s[:, i])
    same("turnover", fac.turnover(f, r).cpu().numpy(), exp["turnover"])
    ls = X.groups(f, r, 1, 0, 0.2, 0.2)
    same("long_short", fac.long_short(f, r)["ls_return"].cpu().numpy(), ls["spread"])
    fm = X.groups(f, r, 1, 0, 0.3, 0.3)
    got = fac.factor_mimicking_portfolio(f, r)
    same("fmp long", got["long_return"].cpu().numpy(), fm["mean_return"][1])
    same("fmp short", got["short_return"].cpu().numpy(), fm["mean_return"][0])
    same("fmp ls", got["ls_return"].cpu().numpy(), fm["spread"])
    same("coverage", fac.coverage(f).cpu().numpy(), X.coverage(f))
    for rank in (False, True):
        ic, _ = fac.rank_ic(f, r) if rank else fac.ic(f, r)
        st = X.ic_stats(ic.cpu().numpy())
        same("ir", np.float64(fac.ir(f, r, rank=rank)), st[3])
        same("ic_win_rate", np.float64(fac.ic_win_rate(f, r, rank=rank)), st[4])


def test_argument_errors_launch_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check, lib
    L = lib()
    n, T = 40, 30
    f, r = make("plain", n, T, 1)
    fd, rd = to_dev(f), to_dev(r)
    for bad_q in (1, 21):
        with pytest.raises(pq.PqError, match="n_quantiles"):
            api.factor_quantiles(fd, rd, bad_q)
    for top, bottom in ((0.6, 0.5), (0.0, 0.2), (0.2, -0.1)):
        with pytest.raises(pq.PqError, match="top_pct"):
            api.factor_long_short(fd, rd, top, bottom)
    h = api.ctx()
    vp = C.c_void_p
    b = Batch(n, T, T)
    mean = torch.full((2, T), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((2, T), 7, dtype=torch.int32, device="cuda")
    tov, spr, summ = mean.clone(), mean[0].clone(), torch.full((3, 5), 7.0, dtype=torch.float64, device="cuda")
    cov = mean[0].clone()
    ic5 = torch.full((5,), 7.0, dtype=torch.float64, device="cuda")
    outs = [vp(t.data_ptr()) for t in (mean, cnt, tov, spr, summ)]
    check(L.pq_suite_begin(h, C.byref(b)))
    try:
        with pytest.raises(pq.PqError, match="recorded"):
            check(L.pq_factor_quantiles(h, C.byref(b), vp(fd.data_ptr()), vp(rd.data_ptr()), C.c_int32(2), None, *outs))
        with pytest.raises(pq.PqError, match="recorded"):
            check(L.pq_factor_long_short(h, C.byref(b), vp(fd.data_ptr()), vp(rd.data_ptr()), C.c_double(0.2), C.c_double(0.2), None, *outs))
        with pytest.raises(pq.PqError, match="recorded"):
            check(L.pq_factor_coverage(h, C.byref(b), vp(fd.data_ptr()), vp(cov.data_ptr())))
        with pytest.raises(pq.PqError, match="recorded"):
            check(L.pq_ic_stats(h, vp(spr.data_ptr()), C.c_int64(T), vp(ic5.data_ptr())))
    finally:
        check(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    with pytest.raises(pq.PqError, match="ragged"):
        check(L.pq_factor_quantiles(h, C.byref(rb), vp(fd.data_ptr()), vp(rd.data_ptr()), C.c_int32(2), None, *outs))
    with pytest.raises(pq.PqError, match="ragged"):
        check(L.pq_factor_long_short(h, C.byref(rb), vp(fd.data_ptr()), vp(rd.data_ptr()), C.c_double(0.2), C.c_double(0.2), None, *outs))
    with pytest.raises(pq.PqError, match="ragged"):
        check(L.pq_factor_coverage(h, C.byref(rb), vp(fd.data_ptr()), vp(cov.data_ptr())))
    torch.cuda.synchronize()
    for name, t, v in (("mean", mean, 7.0), ("count", cnt, 7), ("turnover", tov, 7.0), ("spread", spr, 7.0), ("summary", summ, 7.0),
                       ("coverage", cov, 7.0), ("ic_stats", ic5, 7.0)):
        assert bool((t == v).all()), f"{name} was written by a refused call"
    # the context computes again after the refusals
    check_groups(pq, f, r, 0, 2)
