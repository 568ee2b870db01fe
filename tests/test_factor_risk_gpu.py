"""-m gpu: the risk model of D-33 (csrc/xsec/risk.hip) against the numpy restatement in tests/xsec_risk_ref.py.  Covariances,
variances, counts, exposures, contributions and the four risk rows (the volatility too: sqrt is correctly rounded) are compared bit
for bit, on buffers prefilled with a sentinel and 16 cells longer than the call may write; nothing beyond and no pitch cell may change.
Also: pq_factor_ts_pair's op 0 bit for bit under unit weights, the invariances on the device (doubled weights, the exactly symmetric
matrix, the diagonal against pq_risk_specific_var), the portfolio's NULL-rule days at the lanes 0, 63 and 64 on covariances and
variances that are the two calls' own outputs, the refusals of the three C entry points, empty batches, and the Factor methods' views."""
import ctypes as C
import functools

import numpy as np
import pytest

import xsec_risk_ref as R
import xsec_wls_cases as wls_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 7.0
ISENT = 77
TAIL = 16
NULL = R.NULL
BOUNDARY_DAYS = (0, 63, 64, 255, 256)


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


def to_dev(a, pitch=None):
    a = np.array(a, dtype=np.float64)                       # (a copy: the shared cases are read-only)
    if pitch is None:
        return torch.from_numpy(a).cuda()
    n, T = a.shape
    buf = torch.full((n, pitch), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(a).cuda()
    return buf[:, :T]


def host(t):
    return t.cpu().numpy()


def f64_buf(cells):
    return torch.full((cells + TAIL,), SENTINEL, dtype=torch.float64, device="cuda")


def i32_buf(cells):
    return torch.full((cells + TAIL,), ISENT, dtype=torch.int32, device="cuda")


def untouched(name, buf, used):
    sent = ISENT if buf.dtype == torch.int32 else SENTINEL
    assert bool((buf[used:] == sent).all()), f"{name}: written beyond its end"


# ---------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def series(M, T, seed=0, holes=0.03, bad=True):
    """M series of T days: N(0, 0.01^2) with 3 % NULLs and (bad, from 64 cells) a few +-inf and NaN cells (invalid); from M = 2 the last
    series is valid only on the tile-boundary days 0, 63, 64, 255, 256, from M = 3 series 1 is NULL throughout"""
    rng = np.random.default_rng(10_000 * M + T + seed)
    F = rng.normal(0.0, 0.01, (M, T))
    F[rng.random((M, T)) < holes] = NULL
    for v in (float("inf"), -float("inf"), float("nan")) if bad and M * T >= 64 else ():
        F[rng.integers(0, M, 2), rng.integers(0, T, 2)] = v
    if M >= 2:
        keep = [t for t in BOUNDARY_DAYS if t < T]
        row = np.full(T, NULL)
        row[keep] = rng.normal(0.0, 0.01, len(keep))
        F[M - 1] = row
    if M >= 3:
        F[1] = NULL
    F.setflags(write=False)
    return F


def omega(w, zeros=True):
    """a half-life of a third of the window, with zeros in it where the window has room for them"""
    om = R.weights(w, max(w / 3.0, 1.0))
    if zeros and w >= 5:
        om[[1, w // 2, w - 2]] = 0.0
    return om


def fit(T, day0, step):
    return 0 if day0 >= T else (T - 1 - day0) // step + 1


def cov_raw(F, om, minp, unbiased, day0, step, D, pitch=None, counts=True):
    """pq_risk_factor_cov on sentinel-filled buffers -> (cov [D, M, M], n [D, M]) as device views"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    M, T = F.shape
    fd, od = to_dev(F, pitch), to_dev(om)
    cov, n = f64_buf(D * M * M), (i32_buf(D * M) if counts else None)
    api._call("pq_risk_factor_cov", fd.device, Batch(M, T, pitch or T), fd, od, len(om), minp, 1 if unbiased else 0, day0, step, D, cov, n)
    torch.cuda.synchronize()
    untouched("cov", cov, D * M * M)
    if pitch:
        assert bool((fd.as_strided((M, pitch - T), (pitch, 1), T) == SENTINEL).all()), "the input's pitch cells changed"
    if counts:
        untouched("n", n, D * M)
    return cov[:D * M * M].view(D, M, M), (n[:D * M].view(D, M) if counts else None)


def var_raw(X, om, minp, unbiased, day0, step, D, pitch=None, out_stride=None, counts=True):
    """pq_risk_specific_var on sentinel-filled buffers, the output on a pitch of its own -> device views (var [N, D], n [N, D])"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    N, T = X.shape
    os_ = D + 3 if out_stride is None else out_stride
    xd, od = to_dev(X, pitch), to_dev(om)
    var, n = f64_buf(N * os_), (i32_buf(N * os_) if counts else None)
    api._call("pq_risk_specific_var", xd.device, Batch(N, T, pitch or T), xd, od, len(om), minp, 1 if unbiased else 0, day0, step, D, var,
              os_, n)
    torch.cuda.synchronize()
    untouched("var", var, N * os_)
    grid = var[:N * os_].view(N, os_)
    assert bool((grid[:, D:] == SENTINEL).all()), "var: pitch cells written"
    ng = None
    if counts:
        untouched("n", n, N * os_)
        ng = n[:N * os_].view(N, os_)
        assert bool((ng[:, D:] == ISENT).all()), "n: pitch cells written"
        ng = ng[:, :D]
    return grid[:, :D], ng


# ---------------------------------------------------------------- the windowed kernels at every T, window, min_periods and step class
# (T, w, min_periods: "lo" = 1 biased / 2 unbiased or "w", day0, step, count or None = every day that fits, M of the covariance, N of
# the variance).  T on both sides of the tile of 256 days; w = 1 (biased only), w > T, a halo wider than a tile (w = 257, 300); step 1,
# odd, 64 and 300; one as-of day.  A tile is 256 days at step 1 and min(256 step, 2048 - (w - 1)) days beyond (rk_tile_days), so the
# last three rows are step > 1 over several tiles: three tiles of 768 days, three of 1 749 (the staging's limit), and a step of 5 000
# whose middle tile of 2 044 days has no as-of day.
WINDOWED = [
    (1, 1, "lo", 0, 1, None, 1, 1),
    (1, 2, "lo", 0, 1, None, 2, 3),
    (255, 5, "w", 0, 1, None, 39, 3),
    (255, 1, "lo", 0, 3, None, 2, 1),
    (256, 64, "lo", 7, 1, None, 2, 300),
    (257, 257, "lo", 0, 3, None, 39, 3),
    (257, 5, "lo", 256, 1, 1, 1, 1),
    (300, 300, "w", 0, 1, None, 2, 3),
    (300, 2, "lo", 5, 64, None, 39, 1),
    (300, 64, "lo", 0, 300, None, 1, 300),
    (600, 64, "w", 7, 1, None, 2, 300),
    (600, 257, "w", 0, 3, None, 2, 3),
    (600, 300, "lo", 5, 64, None, 39, 300),
    (600, 5, "w", 0, 300, None, 1, 1),
    (600, 300, "lo", 0, 300, None, 2, 3),
    (600, 64, "lo", 0, 520, None, 39, 3),
    (2300, 300, "lo", 0, 3, None, 2, 3),
    (4000, 300, "lo", 5, 64, None, 2, 3),
    (5001, 5, "lo", 0, 5000, None, 2, 3),
]
WINDOWED_IDS = [f"T{T}-w{w}-{mp}-{d0}+{st}x{c}" for T, w, mp, d0, st, c, _, _ in WINDOWED]


def windowed_args(T, w, mp, day0, step, count):
    """-> unbiased, min_periods, D, the weights, the as-of days, and series' arguments: with min_periods = w only a window without a hole
    and without a zero weight has a result, so those cases get weights without zeros and series with 0.3 / w holes and no inf / NaN"""
    unbiased = w >= 2
    minp = w if mp == "w" else (2 if unbiased else 1)
    D = fit(T, day0, step) if count is None else count
    kw = dict(holes=min(0.03, 0.3 / w), bad=False) if mp == "w" else {}
    return unbiased, minp, D, omega(w, zeros=mp != "w"), R.as_of_days(day0, step, D), kw


@pytest.mark.parametrize("T,w,mp,day0,step,count,M,N", WINDOWED, ids=WINDOWED_IDS)
def test_factor_cov_at_every_window_class(pq, T, w, mp, day0, step, count, M, N):
    unbiased, minp, D, om, days, kw = windowed_args(T, w, mp, day0, step, count)
    F = series(M, T, **kw)
    exp, en = R.factor_cov(F, om, days, minp, unbiased)
    cov, n = cov_raw(F, om, minp, unbiased, day0, step, D, pitch=T + 5)
    same("cov", host(cov), exp)
    same("n", host(n), en)
    if w <= T and days[-1] > 0 and (mp == "w" or M == 39):
        assert not R.isnull(exp).all(), "the restatement has no covariance at all"
    same("cov without counts", host(cov_raw(F, om, minp, unbiased, day0, step, D, counts=False)[0]), exp)


@pytest.mark.parametrize("T,w,mp,day0,step,count,M,N", WINDOWED, ids=WINDOWED_IDS)
def test_specific_var_at_every_window_class(pq, T, w, mp, day0, step, count, M, N):
    unbiased, minp, D, om, days, kw = windowed_args(T, w, mp, day0, step, count)
    X = series(N, T, seed=1, **kw)
    exp, en = R.specific_var(X, om, days, minp, unbiased)
    var, n = var_raw(X, om, minp, unbiased, day0, step, D, pitch=T + 5)
    same("var", host(var), exp)
    same("n", host(n), en)
    if w <= T and days[-1] > 0 and (mp == "w" or N == 300):
        assert not R.isnull(exp).all(), "the restatement has no variance at all"
    same("var without counts, dense", host(var_raw(X, om, minp, unbiased, day0, step, D, out_stride=D, counts=False)[0]), exp)


@pytest.mark.timeout(120)
def test_factor_cov_at_the_widest_matrix(pq):
    """M = 264 (D-32's whole coef block) at T = 70, w = 20: every row of the triangle, 34 980 pairs per as-of day"""
    M, T, w = 264, 70, 20
    F = series(M, T)
    om = omega(w)
    D = fit(T, 0, 3)
    exp, en = R.factor_cov(F, om, R.as_of_days(0, 3, D), 5)
    cov, n = cov_raw(F, om, 5, True, 0, 3, D, pitch=T + 5)
    same("cov", host(cov), exp)
    same("n", host(n), en)
    assert (~R.isnull(exp[-1])).sum() > M * M // 2


# ---------------------------------------------------------------- the cross-checks on the device
@pytest.mark.parametrize("w", [2, 64])
def test_unit_weights_equal_pq_factor_ts_pair(pq, w):
    """om = 1.0, unbiased, min_periods = w, step 1: every step is ts_pair_kernel<TSP_COV>'s, so op 0 bit for bit -- every pair of the
    matrix, and the variance against ts_cov(x, x)"""
    from polars_quant_amd import api
    M, T = 3, 300
    rng = np.random.default_rng(w)
    F = rng.normal(0.0, 0.01, (M, T))
    F[rng.random((M, T)) < 0.004] = NULL
    F[0, 100] = float("inf")
    cov, n = cov_raw(F, np.ones(w), w, True, 0, 1, T)
    var, _ = var_raw(F, np.ones(w), w, True, 0, 1, T)
    cov, fd = host(cov), to_dev(F)
    for j in range(M):
        for l in range(M):
            ts = host(api.factor_ts_pair(fd[j:j + 1], fd[l:l + 1], api.TS_PAIR_OPS["cov"], w))[0]
            assert (~R.isnull(ts)).sum() > T // 5
            same(f"cov[{j}][{l}] against ts_cov", cov[:, j, l], ts)
        same(f"var[{j}] against ts_cov", host(var)[j], cov[:, j, j])


def test_doubled_weights_symmetry_and_the_diagonal_on_the_device(pq):
    M, T, w, day0, step = 39, 300, 64, 2, 3
    F, om = series(M, T), omega(w)
    D = fit(T, day0, step)
    cov, n = cov_raw(F, om, 10, True, day0, step, D)
    cov2, n2 = cov_raw(F, 2.0 * om, 10, True, day0, step, D)
    same("doubled weights", host(cov2), host(cov))
    same("doubled weights: n", host(n2), host(n))
    same("symmetry", host(cov), host(cov).transpose(0, 2, 1))
    var, nv = var_raw(F, om, 10, True, day0, step, D)
    same("the diagonal", host(var), np.diagonal(host(cov), axis1=1, axis2=2).T)
    same("the diagonal's n", host(nv), host(n).T)
    assert (~R.isnull(host(cov))).sum() > D * M * M // 2


# ---------------------------------------------------------------- the portfolio
PF_W = 8


@functools.lru_cache(maxsize=None)
def pf_case(N, K, G, codes, D, step=1, seed=0):
    """factor series [K + G, T], specific returns [N, T], holdings, exposures [K, N, T], codes; T holds D as-of days from day PF_W - 1.
    About a third of the symbols are held (the others 0 or NULL); what would leave a held symbol uncovered sits on symbols that are not
    held, except on a few days."""
    rng = np.random.default_rng(1000 * N + 100 * K + G + D + seed)
    day0 = PF_W - 1
    T = day0 + (D - 1) * step + 1
    M = K + G
    F = rng.normal(0.0, 0.01, (M, T))
    F[rng.random((M, T)) < 0.02] = NULL
    E = rng.normal(0.0, 0.02, (N, T))
    E[rng.random((N, T)) < 0.03] = NULL
    H = np.round(rng.normal(0.0, 1.0, (N, T)), 3)
    r = rng.random((N, T))
    H[r < 0.35] = 0.0
    H[r > 0.7] = NULL
    if N > 2:
        E[1] = NULL                                          # never a specific variance: not held
        H[1] = 0.0
    X = rng.normal(0.0, 1.0, (K, N, T))
    idle = ~(R.valid(H) & (H != 0.0))
    for j in range(K):
        X[j][idle & (rng.random((N, T)) < 0.2)] = NULL
    ind = None
    if codes is not None:
        ind = rng.integers(0, G, (N, T) if codes == "2d" else (N,)).astype(np.int32)
        if codes == "2d":
            ind[idle & (rng.random((N, T)) < 0.1)] = -1
            ind[idle & (rng.random((N, T)) < 0.1)] = G
    if K and D > 8 and N > 8:                                # a day with a held symbol whose exposure is NULL
        s = int(np.flatnonzero(~idle[:, day0 + 5 * step])[0])
        X[K - 1, s, day0 + 5 * step] = NULL
    for a in (F, E, H, X, ind):
        if a is not None:
            a.setflags(write=False)
    return F, E, H, X, ind, day0, T


def pf_model(F, E, day0, step, D):
    """the two calls' own outputs (device tensors, the variance on a pitch of D + 3) and their restatement"""
    om = omega(PF_W, zeros=False)
    days = R.as_of_days(day0, step, D)
    cov, _ = cov_raw(F, om, 2, True, day0, step, D)
    var, _ = var_raw(E, om, 2, True, day0, step, D)
    ecov, esv = R.factor_cov(F, om, days, 2)[0], R.specific_var(E, om, days, 2)[0]
    same("the model's cov", host(cov), ecov)
    same("the model's var", host(var), esv)
    return cov, var, ecov, esv, days


def pf_raw(H, X, ind, G, cov, var, day0, step, D, pitch=None, gpitch=None):
    """pq_risk_portfolio on sentinel-filled buffers; cov and var are device tensors (var a [N, D] view on its own pitch)"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    N, T = H.shape
    K, M = len(X), len(X) + G
    stride = pitch or T
    hd, xd = to_dev(H, pitch), [to_dev(x, pitch) for x in X]
    gd, gs = None, 0
    if ind is not None and ind.ndim == 1:
        gd = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    elif ind is not None:
        gs = gpitch or stride
        gd = torch.full((N, gs), 3, dtype=torch.int32, device="cuda")
        gd[:, :T] = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    expo, contrib, risk, n = f64_buf(M * D), f64_buf(M * D), f64_buf(4 * D), i32_buf(2 * D)
    ptrs = (C.c_void_p * max(K, 1))(*[x.data_ptr() for x in xd])
    api._call("pq_risk_portfolio", hd.device, Batch(N, T, stride), hd, ptrs, K, gd, gs, G, cov.contiguous(), var,
              var.stride(0) if N > 1 else D, day0, step, D, expo, contrib, risk, n)
    torch.cuda.synchronize()
    for name, buf, used in (("exposure", expo, M * D), ("contribution", contrib, M * D), ("risk", risk, 4 * D), ("n", n, 2 * D)):
        untouched(name, buf, used)
    return {"exposure": host(expo[:M * D]).reshape(M, D), "contribution": host(contrib[:M * D]).reshape(M, D),
            "risk": host(risk[:4 * D]).reshape(4, D), "n": host(n[:2 * D]).reshape(2, D)}


def pf_check(tag, got, exp, min_days=1):
    assert (~R.isnull(exp["risk"][3])).sum() >= min_days, f"{tag}: the restatement has {(~R.isnull(exp['risk'][3])).sum()} days with a volatility"
    for k in ("n", "exposure", "contribution", "risk"):
        same(f"{k} {tag}", got[k], exp[k])


PORTFOLIOS = [(1, 0, 1, None, 1, 1), (255, 1, 7, "1d", 63, 1), (256, 3, 7, "2d", 64, 2), (257, 8, 256, "1d", 65, 1),
              (600, 3, 1, None, 130, 1), (600, 1, 256, "2d", 65, 3), (257, 0, 7, "2d", 1, 1), (255, 8, 1, None, 64, 1)]


@pytest.mark.parametrize("N,K,G,codes,D,step", PORTFOLIOS, ids=[f"N{N}-K{K}-G{G}-{c}-D{D}+{s}" for N, K, G, c, D, s in PORTFOLIOS])
def test_portfolio_at_every_size_class(pq, N, K, G, codes, D, step):
    """N on both sides of the block of 256 symbols and of two blocks, D on both sides of the 64 as-of days of a workgroup, every K and G
    class with [N] and [N, T] codes on a pitch of their own; covariances and variances are the two calls' own outputs"""
    F, E, H, X, ind, day0, T = pf_case(N, K, G, codes, D, step)
    if N == 1:
        H = np.full((1, T), 0.5)
    cov, var, ecov, esv, days = pf_model(F, E, day0, step, D)
    exp = R.portfolio(H, list(X), ecov, esv, days, ind, G)
    got = pf_raw(H, list(X), ind, G, cov, var, day0, step, D, pitch=T + 5, gpitch=T + 9)
    pf_check(f"N={N} K={K} G={G} D={D}", got, exp, min_days=min(D, 3) if N != 600 or K != 1 else 0)


@pytest.mark.parametrize("rot", [0, 3])
def test_portfolio_null_rule_days_at_lanes_0_63_64(pq, rot):
    """the constructed as-of days: nothing held, an uncovered symbol (an exposure, a code, a variance), a needed NULL covariance, a NULL
    covariance that is not needed because its exposure is 0, and a negative total; three of the six on the as-of days 0, 63 and 64 (the
    first and last lane of a workgroup and the first of the next), the others on 1, 62 and 65; the second rotation swaps the halves"""
    N, K, G, D = 300, 3, 7, 130
    F, E, H, X, ind, day0, T = pf_case(N, K, G, "2d", D, 1, seed=rot)
    H, X, ind = H.copy(), X.copy(), ind.copy()
    cov, var, ecov, esv, days = pf_model(F, E, day0, 1, D)
    cov, var, ecov, esv = cov.clone(), var.clone(), ecov.copy(), esv.copy()
    kinds = ["empty", "uncovered", "null_cov", "unneeded", "negative", "variance"]
    kinds = kinds[rot:] + kinds[:rot]
    day_of = dict(zip(kinds, [0, 63, 64, 1, 62, 65]))
    held = lambda d: np.flatnonzero(R.valid(H[:, day0 + d]) & (H[:, day0 + d] != 0.0))   # noqa: E731

    def poke(dev, ref, idx, v):
        ref[idx] = v
        dev[idx] = torch.from_numpy(np.array(v, dtype=np.float64)).cuda()   # (a tensor copy keeps NULL's payload)
    d = day_of["empty"]
    H[:, day0 + d] = np.where(np.arange(N) % 2 == 0, 0.0, NULL)
    d = day_of["uncovered"]
    s = held(d)
    X[1, s[0], day0 + d] = NULL
    ind[s[1], day0 + d] = G
    ind[s[2], day0 + d] = -1
    d = day_of["variance"]
    s = held(d)
    poke(var, esv, (int(s[0]), d), NULL)
    poke(var, esv, (int(s[1]), d), -1e-9)
    d = day_of["null_cov"]
    poke(cov, ecov, (d, 2, K + 1), NULL)
    d = day_of["unneeded"]
    X[0, :, day0 + d] = 0.0                                  # X[0] = 0 exactly: row and column 0 are never read
    for l in range(K + G):
        poke(cov, ecov, (d, 0, l), NULL)
        poke(cov, ecov, (d, l, 0), NULL)
    d = day_of["negative"]
    poke(cov, ecov, (d, K, K), -1e6)
    exp = R.portfolio(H, list(X), ecov, esv, days, ind, G)
    n, risk = exp["n"], exp["risk"]
    assert n[:, day_of["empty"]].tolist() == [0, 0] and n[1, day_of["uncovered"]] == 3 and n[1, day_of["variance"]] == 2
    for k in ("empty", "uncovered", "variance", "null_cov"):
        assert R.isnull(risk[:, day_of[k]]).all() and R.isnull(exp["exposure"][:, day_of[k]]).all(), k
    assert n[1, day_of["null_cov"]] == 0 and n[0, day_of["null_cov"]] > 0
    d = day_of["unneeded"]
    assert not R.isnull(risk[:, d]).any() and exp["exposure"][0, d] == 0.0 and exp["contribution"][0, d] == 0.0
    d = day_of["negative"]
    assert risk[2, d] < 0.0 and R.isnull(risk[3, d]) and not R.isnull(risk[:3, d]).any()
    got = pf_raw(H, list(X), ind, G, cov, var, day0, 1, D, pitch=T + 3)
    pf_check(f"special days rot={rot}", got, exp, min_days=60)


# ---------------------------------------------------------------- the C entry points' refusals and empty batches
def test_windowed_refusals_write_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    M, T, w = 3, 40, 5
    F = series(M, T)
    fd, od = to_dev(F), to_dev(omega(w))
    b = Batch(M, T, T)
    for name, extra, cells in (("pq_risk_factor_cov", (), 8 * M * M), ("pq_risk_specific_var", (8,), M * 8)):
        out, n = f64_buf(cells), i32_buf(M * 8)

        def status(bb=b, f=fd, om=od, win=w, minp=2, unb=1, day0=0, step=5, count=8, out_=out, n_=n, extra_=extra):
            s = api._call(name, fd.device, bb, f, om, win, minp, unb, day0, step, count, out_, *extra_, n_, checked=False)
            return s, L.pq_last_error().decode()
        bad = [(dict(win=0), "window must be in [1, 1024]"), (dict(win=1025), "window must be"), (dict(minp=0), "min_periods must be"),
               (dict(minp=6), "min_periods must be"), (dict(minp=1), "min_periods >= 2"), (dict(day0=-1), "as-of days"),
               (dict(step=0), "as-of days"), (dict(count=-1), "as-of days"), (dict(count=9), "as-of days"), (dict(day0=40, count=1), "as-of days"),
               (dict(day0=5, step=2 ** 62, count=2), "as-of days"), (dict(f=None), "null pointer"), (dict(om=None), "null pointer"),
               (dict(out_=None), "null pointer"), (dict(out_=fd), "must not overlap the series"), (dict(out_=od, count=0), None),
               (dict(out_=od, count=1, win=5), "must not overlap the series or the weights")]
        if extra:
            bad += [(dict(extra_=(7,)), "out_stride")]
        else:
            bad += [(dict(bb=Batch(265, T, T)), "at most 264")]
        for kw, msg in bad:
            s, err = status(**kw)
            if msg is None:
                assert s == 0, (name, kw.keys(), s, err)
                continue
            assert s == 1 and msg in err and name in err, (name, kw.keys(), s, err)                 # PQ_ERR_ARG
        s, err = status(out_=out, n_=out.view(torch.int32))
        assert s == 1 and "must not overlap each other" in err, (s, err)
        off = torch.tensor([0, 10, 25, M * T], dtype=torch.int64, device="cuda")
        s, err = status(bb=Batch(3, M * T - 25, M * T, C.c_void_p(off.data_ptr())), count=1)
        assert s == 5 and "ragged" in err and name in err, (s, err)                                  # PQ_ERR_UNSUPPORTED
        assert L.pq_suite_begin(h, C.byref(b)) == 0
        try:
            s, err = status()
            assert s == 5 and "recorded" in err and name in err, (s, err)
        finally:
            assert L.pq_suite_abort(h) == 0
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((n == ISENT).all()), f"{name}: a refused call wrote"
        s, err = status(minp=1, unb=0)                                                               # biased: min_periods 1 passes
        assert s == 0, err
        s, err = status()                                                                            # the context computes again
        assert s == 0, err
        torch.cuda.synchronize()
        days = R.as_of_days(0, 5, 8)
        if extra:
            same("var after the refusals", host(out[:cells]).reshape(M, 8), R.specific_var(F, omega(w), days, 2)[0])
        else:
            same("cov after the refusals", host(out[:cells]).reshape(8, M, M), R.factor_cov(F, omega(w), days, 2)[0])
        # the empty batches: PQ_OK, nothing launched, no pointer needed
        for bb, cnt in ((Batch(0, T, T), 3), (Batch(M, 0, 0), 0), (b, 0)):
            assert api._call(name, fd.device, bb, None, None, w, 2, 1, 0, 1, cnt, None, *extra, None, checked=False) == 0


def test_portfolio_refusals_write_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    N, K, G, D = 40, 2, 3, 9
    F, E, H, X, ind, day0, T = pf_case(N, K, G, "1d", D)
    cov, var, ecov, esv, days = pf_model(F, E, day0, 1, D)
    M = K + G
    hd, xd = to_dev(H), [to_dev(x) for x in X]
    gd = torch.from_numpy(np.array(ind)).cuda()
    outs = [f64_buf(M * D), f64_buf(M * D), f64_buf(4 * D), i32_buf(2 * D)]
    b = Batch(N, T, T)
    cv, sv = cov.contiguous(), var

    def status(bb=b, h_=hd, cols=xd, k=K, g_=gd, gs=0, G_=G, cov_=cv, sv_=sv, svs=None, day0_=day0, step=1, count=D, outs_=outs, ptrs=True):
        p = (C.c_void_p * max(len(cols), 1))(*[None if c is None else c.data_ptr() for c in cols]) if ptrs else None
        s = api._call("pq_risk_portfolio", hd.device, bb, h_, p, k, g_, gs, G_, cov_, sv_, sv.stride(0) if svs is None else svs, day0_, step,
                      count, *outs_, checked=False)
        return s, L.pq_last_error().decode()
    bad = [(dict(k=-1), "k must be in [0, 8]"), (dict(k=9), "k must"), (dict(G_=0), "n_groups"), (dict(G_=257), "n_groups"),
           (dict(g_=None), "n_groups must be 1"), (dict(g_=torch.zeros((N, T), dtype=torch.int32, device="cuda"), gs=T - 1), "group_stride"),
           (dict(gs=-1), "group_stride"), (dict(svs=D - 1), "sv_stride"), (dict(day0_=-1), "as-of days"), (dict(step=0), "as-of days"),
           (dict(count=-1), "as-of days"), (dict(day0_=day0 + 1), "as-of days"), (dict(h_=None), "null pointer"),
           (dict(ptrs=False), "null pointer"), (dict(cols=[xd[0], None]), "null exposure"), (dict(cov_=None), "null pointer"),
           (dict(sv_=None), "null pointer")] + [(dict(outs_=outs[:j] + [None] + outs[j + 1:]), "null pointer") for j in range(4)]
    for kw, msg in bad:
        s, err = status(**kw)
        assert s == 1 and msg in err and "pq_risk_portfolio" in err, (kw.keys(), s, err)               # PQ_ERR_ARG
    off = torch.tensor([0, 10, 25, N * T], dtype=torch.int64, device="cuda")
    s, err = status(bb=Batch(3, N * T - 25, N * T, C.c_void_p(off.data_ptr())))
    assert s == 5 and "ragged" in err, (s, err)                                                    # PQ_ERR_UNSUPPORTED
    assert L.pq_suite_begin(h, C.byref(b)) == 0
    try:
        s, err = status()
        assert s == 5 and "recorded" in err, (s, err)
    finally:
        assert L.pq_suite_abort(h) == 0
    torch.cuda.synchronize()
    assert all(bool((o == (ISENT if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs), "a refused call wrote"
    s, err = status(count=0, outs_=[None] * 4, cov_=None)                                          # no as-of day: nothing launched
    assert s == 0, err
    s, err = status()                                                                              # the context computes again
    assert s == 0, err
    torch.cuda.synchronize()
    exp = R.portfolio(H, list(X), ecov, esv, days, ind, G)
    same("risk after the refusals", host(outs[2][:4 * D]).reshape(4, D), exp["risk"])
    same("n after the refusals", host(outs[3][:2 * D]).reshape(2, D), exp["n"])


def test_empty_batches_through_the_api(pq):
    from polars_quant_amd import api
    w = api.risk_weights(4, 2.0)
    for shape in ((0, 30), (3, 0)):
        z = torch.empty((shape[0], 32), dtype=torch.float64, device="cuda")[:, :shape[1]]   # (on an even pitch)
        cov, n = api.risk_factor_cov(z, w, 2, counts=True)
        D = 30 if shape[1] else 0
        assert tuple(cov.shape) == (D, shape[0], shape[0]) and tuple(n.shape) == (D, shape[0])
        var = api.risk_specific_var(z, w, 2)
        assert tuple(var.shape) == (shape[0], D)
    x = to_dev(series(3, 30))
    assert tuple(api.risk_factor_cov(x, w, 2, day0=30).shape) == (0, 3, 3)
    assert tuple(api.risk_factor_cov(x, w, 2, count=0).shape) == (0, 3, 3)
    # no symbol: every as-of day holds nothing
    z = torch.empty((0, 30), dtype=torch.float64, device="cuda")
    out = api.risk_portfolio(z, [z], torch.zeros((5, 2, 2), dtype=torch.float64, device="cuda"),
                             torch.empty((0, 5), dtype=torch.float64, device="cuda"), day0=3, step=2)
    assert R.isnull(host(out["volatility"])).all() and R.isnull(host(out["exposure"])).all() and tuple(out["exposure"].shape) == (2, 5)
    assert (host(out["n_held"]) == 0).all() and (host(out["n_uncovered"]) == 0).all()
    out = api.risk_portfolio(x, None, torch.zeros((0, 1, 1)), torch.zeros((3, 0)))
    assert tuple(out["volatility"].shape) == (0,) and tuple(out["contribution"].shape) == (1, 0)


# ---------------------------------------------------------------- the api and the Factor methods
def test_the_api_on_pitched_and_host_inputs(pq):
    """the Python entries on a pitched device tensor, a host array and a one-row series; count, day0 and step; the weights as given"""
    from polars_quant_amd import api
    M, T, w = 5, 130, 20
    F = series(M, T)
    om = api.risk_weights(w, 7.0)
    exp, en = R.factor_cov(F, om, R.as_of_days(19, 10, 12), 5)
    for x in (to_dev(F, 136), np.array(F)):
        cov, n = api.risk_factor_cov(x, om, 5, day0=19, step=10, counts=True)
        same("cov", host(cov), exp)
        same("n", host(n), en)
        var, nv = api.risk_specific_var(x, om, 5, day0=19, step=10, count=7, counts=True)
        same("var", host(var), np.diagonal(exp, axis1=1, axis2=2).T[:, :7])
        same("var n", host(nv), en.T[:, :7])
    b = host(api.risk_factor_cov(np.array(F[0]), om, 5, unbiased=False))
    same("one series, biased, every day", b[:, 0, 0], R.specific_var(F[:1], om, np.arange(T), 5, unbiased=False)[0][0])


def test_the_factor_methods_are_views_of_the_calls(pq):
    from polars_quant_amd import api
    K, G, N, T = 3, 7, 300, 300
    Fx, r, wt, ind = wls_cases.panel(K, N, T, G, 4242, codes="1d")
    ind = np.where((ind >= 0) & (ind < G), ind, -1).astype(np.int32)
    cols, rd, wd, gd = [to_dev(f) for f in Fx], to_dev(r), to_dev(wt), torch.from_numpy(ind)
    fac = pq.Factor()
    reg = fac.pure_factor_return(cols, rd, wd, gd, specific_return=True)
    model = fac.risk_model(reg, window=60, halflife=20.0, step=20, specific_window=40, specific_halflife=10.0)
    assert set(model) == {"factor_cov", "specific_var", "n", "days", "day0", "step"}
    assert model["day0"] == 59 and model["step"] == 20
    days = R.as_of_days(59, 20, 13)
    assert host(model["days"]).tolist() == days.tolist() and model["days"].dtype == torch.int64
    block = np.concatenate([host(reg["factor_return"]), host(reg["industry_return"])])
    resid = host(reg["specific_return"])
    ecov, en = R.factor_cov(block, R.weights(60, 20.0), days, 30)
    esv, _ = R.specific_var(resid, R.weights(40, 10.0), days, 20)
    same("factor_cov", host(model["factor_cov"]), ecov)
    same("n", host(model["n"]), en)
    same("specific_var", host(model["specific_var"]), esv)
    assert (~R.isnull(ecov)).sum() > ecov.size // 2 and (~R.isnull(esv)).sum() > esv.size // 2
    raw = api.risk_factor_cov(torch.cat([reg["factor_return"], reg["industry_return"]]), api.risk_weights(60, 20.0), 30, 59, 20)
    same("the raw call", host(raw), host(model["factor_cov"]))
    # holdings: a third of the covered symbols, equal weights summing to 1 on every as-of day
    rng = np.random.default_rng(5)
    H = np.where(rng.random((N, T)) < 0.3, 1.0, 0.0)
    covered = np.zeros((N, T), dtype=bool)
    covered[:, days] = ~R.isnull(esv) & (ind >= 0)[:, None]
    for f in Fx:
        covered &= R.valid(f)
    H = np.where(covered, H, 0.0)
    H = H / np.maximum(H.sum(axis=0, keepdims=True), 1.0)
    out = fac.portfolio_risk(to_dev(H), cols, model, gd)
    assert set(out) == {"exposure", "contribution", "factor_var", "specific_var", "total_var", "volatility", "n_held", "n_uncovered"}
    exp = R.portfolio(H, list(Fx), ecov, esv, days, ind, G)
    same("exposure", host(out["exposure"]), exp["exposure"])
    same("contribution", host(out["contribution"]), exp["contribution"])
    for j, k in enumerate(("factor_var", "specific_var", "total_var", "volatility")):
        same(k, host(out[k]), exp["risk"][j])
    same("n_held", host(out["n_held"]), exp["n"][0])
    same("n_uncovered", host(out["n_uncovered"]), exp["n"][1])
    assert not R.isnull(exp["risk"][3]).any() and (exp["n"][1] == 0).all()
    # an [M, T] array and explicit specific returns; no specific returns: no specific_var, and portfolio_risk says so
    m2 = fac.risk_model(block, resid, window=60, halflife=20.0, step=20, specific_window=40, specific_halflife=10.0)
    same("from arrays: factor_cov", host(m2["factor_cov"]), ecov)
    same("from arrays: specific_var", host(m2["specific_var"]), esv)
    m3 = fac.risk_model(block, window=60, halflife=20.0, step=20)
    assert "specific_var" not in m3
    with pytest.raises(ValueError, match="no specific_var"):
        fac.portfolio_risk(to_dev(H), cols, m3, gd)
    # without industries the intercept row closes the block
    reg1 = fac.pure_factor_return(cols, rd, wd)
    m4 = fac.risk_model(reg1, window=60, step=60)
    block1 = np.concatenate([host(reg1["factor_return"]), host(reg1["intercept"])[None, :]])
    same("with the intercept", host(m4["factor_cov"]), R.factor_cov(block1, np.ones(60), R.as_of_days(59, 60, 5), 30)[0])
