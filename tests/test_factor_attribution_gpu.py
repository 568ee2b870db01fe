"""-m gpu: the return attribution of D-36 (csrc/xsec/attribution.hip) against the numpy restatement in tests/xsec_attribution_ref.py.
Every output -- exposures, contributions, the six totals, the three counts, the summary rows, the period sums and days -- is compared
bit for bit (the summary's p-value as D-17 compares it: the restatement takes it from scipy, never from the device's formula), on buffers prefilled with a sentinel and 16 cells longer than the call may write; nothing beyond and no pitch cell may
change.  The sizes reach every branch: one symbol, one day, the blocks' and the waves' edges, K = 0 and 8, no codes, [N] and [N, T]
codes, 256 industries with one book (two launches of the pass) and both sides of the chunking boundary with three books.  Also: the
refusals of the C entry point, the empty calls, the Python entries on pitched and host inputs, and the whole chain pure_factor_return ->
risk_model -> optimal_portfolio -> weights_backtest -> return_attribution with the identity total = realized."""
import ctypes as C
import functools

import numpy as np
import pytest

import xsec_attribution_ref as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 7.0
ISENT = 77
TAIL = 16
NULL = A.NULL
INF = float("inf")
IDENTITY_BOUND = 1e-13      # tests/test_factor_attribution_ref.py: 64 x the worst error of the restatement, rounded up to a power of ten


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
def case(N, T, K, G, codes, seed=0):
    """holdings and a benchmark with NULL, NaN, +-inf and 0.0 cells, exposures, specific and next returns with holes, factor returns with
    NULL and infinite cells, codes -1 and G among the valid ones; symbol 0 of every block of 256 is uncovered on every day (its first
    exposure, or without exposures its specific return, is NULL).  G None: no codes."""
    rng = np.random.default_rng(1_000_003 * N + 1009 * T + 17 * K + (G or 0) + seed)
    Gn = G or 1
    h, b = rng.standard_normal((N, T)) / 8.0, np.abs(rng.standard_normal((N, T))) / 8.0
    for v in (NULL, float("nan"), INF, -INF, 0.0, 0.0, 0.0):
        h[rng.random((N, T)) < 0.03] = v
        b[rng.random((N, T)) < 0.03] = v
    xs = [rng.standard_normal((N, T)) for _ in range(K)]
    u, r = 0.02 * rng.standard_normal((N, T)), 0.03 * rng.standard_normal((N, T))
    for a in xs + [u, r]:
        a[rng.random((N, T)) < 0.02] = NULL
        a[rng.random((N, T)) < 0.005] = float("nan")
        a[rng.random((N, T)) < 0.005] = INF
    (xs[0] if K else u)[::256] = NULL
    f = 0.01 * rng.standard_normal((K + Gn, T))
    f[(rng.random((K + Gn, T)) < 0.02) & (np.arange(T) % 4 == 1)[None, :]] = NULL       # on every fourth day: the other days keep their books
    if T >= 3:
        f[0, 1], f[-1, 2] = INF, float("nan")
    ind = None
    if G is not None:
        ind = rng.integers(0, G, N if codes == "1d" else (N, T))
        for v in (-1, G, -2**31, 2**31 - 1):
            ind = np.where(rng.random(ind.shape) < 0.01, v, ind)
        ind = ind.astype(np.int32)
    out = (h, b, tuple(xs), u, r, f, ind)
    for a in (h, b, u, r, f) + tuple(xs) + ((ind,) if ind is not None else ()):
        a.setflags(write=False)
    return out


def bounds_of(T, periods):
    """None; an int: numpy.array_split's bounds; "days": T singletons; "uneven": periods of 1, many and many days that leave day 0 and
    the last day out (T >= 4)"""
    if periods is None:
        return None
    if periods == "days":
        return list(range(T + 1))
    if periods == "uneven":
        return [1, 2, T // 2, T - 1]
    return [0] + np.cumsum([len(p) for p in np.array_split(np.arange(T), periods)]).tolist()


def raw(c, G, bench=True, next_return=True, bounds=None, pitch=None, gpitch=None, fpitch=None):
    """pq_return_attribution on sentinel-filled buffers -> dict of host arrays in the restatement's shapes"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    h, b, xs, u, r, f, ind = c
    N, T = h.shape
    K, Gn = len(xs), G or 1
    M, P = K + Gn, 3 if bench else 1
    NS, S = M + 6, 0 if bounds is None else len(bounds) - 1
    stride = pitch or T
    planes = [to_dev(a, pitch) for a in (h, b, u, r) + xs]
    hd, bd, ud, rd, xd = planes[0], planes[1], planes[2], planes[3], planes[4:]
    fd = to_dev(f, fpitch)
    gd, gs = None, 0
    if ind is not None:
        if ind.ndim == 1:
            gd = torch.from_numpy(np.array(ind)).cuda()
        else:
            gs = gpitch or T
            gd = torch.full((N, gs), -5, dtype=torch.int32, device="cuda")
            gd[:, :T] = torch.from_numpy(np.array(ind)).cuda()
    bp = np.asarray(bounds, dtype=np.int64) if S else None
    outs = {"exposure": f64_buf(P * M * T), "contribution": f64_buf(P * M * T), "totals": f64_buf(P * 6 * T), "n": i32_buf(3 * P * T),
            "summary": f64_buf(P * NS * 5), "period_sum": f64_buf(P * NS * S) if S else None, "period_days": i32_buf(P * S) if S else None}
    ptrs = (C.c_void_p * max(K, 1))(*[x.data_ptr() for x in xd])
    api._call("pq_return_attribution", hd.device, Batch(N, T, stride), hd, bd if bench else None, ptrs, K, gd, gs, Gn, fd, fpitch or T, ud,
              rd if next_return else None, bp, S, *outs.values())
    torch.cuda.synchronize()
    shapes = {"exposure": (P, M, T), "contribution": (P, M, T), "totals": (P, 6, T), "n": (3, P, T), "summary": (P, NS, 5),
              "period_sum": (P, NS, S), "period_days": (P, S)}
    got = {}
    for k, buf in outs.items():
        if buf is None:
            continue
        cells = int(np.prod(shapes[k]))
        untouched(k, buf, cells)
        got[k] = host(buf[:cells]).reshape(shapes[k])
    if pitch:
        for p in planes:
            assert bool((p.as_strided((N, pitch - T), (pitch, 1), T) == SENTINEL).all()), "an input's pitch cells changed"
    return got


def expected(c, G, bench=True, next_return=True, bounds=None):
    h, b, xs, u, r, f, ind = c
    return A.attribution(h, list(xs), f, u, ind, G or 1, r if next_return else None, b if bench else None, bounds)


def close_p(name, got, exp):
    """D-17's comparison of a p-value: the device's continued fraction against the restatement's scipy.special.stdtr, the same NULL
    pattern and |dp| <= 1e-11 p"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, name
    assert (A.isnull(got) == A.isnull(exp)).all() and (np.isnan(got) == np.isnan(exp)).all(), f"{name}: NULL pattern differs"
    ok = ~np.isnan(exp)
    err = np.abs(got[ok] - exp[ok]) - (1e-11 * exp[ok] + 1e-300)
    assert (err <= 0).all(), f"{name}: worst |dp| excess {err.max()!r}"


def same_summary(name, got, exp):
    """n_days, mean, std and t bit for bit; the p-value as D-17 compares it"""
    same(name, np.asarray(got)[..., :4], np.asarray(exp)[..., :4])
    close_p(f"{name}: p", np.asarray(got)[..., 4], np.asarray(exp)[..., 4])


def check(tag, got, exp):
    assert set(got) == set(exp), (tag, sorted(got), sorted(exp))
    for k in exp:
        (same_summary if k == "summary" else same)(f"{tag}: {k}", got[k], exp[k])


# N, T, K, G (None: no codes), codes, benchmark, next_return, periods, pitch, group pitch, factor-return pitch
SIZES = [
    (1, 1, 0, None, None, False, True, 1, None, None, None),            # one symbol, one day, nothing but the intercept
    (1, 131, 1, 3, "2d", True, True, "days", None, None, None),         # one symbol; T singleton periods
    (255, 63, 1, 3, "1d", True, True, "days", None, None, None),        # one block short of full, one wave short of full
    (256, 64, 8, 31, "2d", True, True, "uneven", 80, 96, 70),           # exactly one block and one wave; every pitch larger than T
    (257, 65, 1, 256, "1d", False, True, 1, None, None, None),          # 256 industries, one book: two launches of 128
    (256, 1, 8, 129, "2d", False, False, None, None, None, None),       # one day; 129 industries: 128 + 1; no next return
    (257, 65, 0, 42, "2d", True, True, None, None, None, None),         # three books at the chunking boundary: 42 industries, one launch
    (257, 65, 1, 43, "1d", True, False, "uneven", 72, None, None),      # ... and 43: two launches
    (300, 64, 8, None, None, True, True, 3, None, None, None),          # K = 8 without codes
    (700, 131, 8, 31, "1d", True, True, "uneven", 144, None, 136),      # three blocks, three waves, the benchmark's size class
    (700, 65, 0, 3, "2d", False, True, 2, None, 80, None),              # K = 0 with codes on their own pitch
]


@pytest.mark.parametrize("N,T,K,G,codes,bench,nxt,periods,pitch,gpitch,fpitch", SIZES,
                         ids=[f"N{s[0]}-T{s[1]}-K{s[2]}-G{s[3]}-{s[4]}-P{3 if s[5] else 1}" for s in SIZES])
def test_every_output_bit_for_bit_at_every_size_class(pq, N, T, K, G, codes, bench, nxt, periods, pitch, gpitch, fpitch):
    c = case(N, T, K, G, codes)
    bounds = bounds_of(T, periods)
    exp = expected(c, G, bench, nxt, bounds)
    got = raw(c, G, bench, nxt, bounds, pitch, gpitch, fpitch)
    check(f"N={N} T={T} K={K} G={G}", got, exp)
    if N >= 255:                                                        # the case reaches the rules it is there for
        assert (exp["n"][1] > 0).any() and (exp["n"][0] > exp["n"][1]).any()
        if T > 1:
            nul = A.isnull(exp["totals"][0, 4])
            assert (~nul).any()
            if nxt:
                assert (exp["n"][2] > 0).any() and (exp["n"][2] < exp["n"][1]).any()


def test_the_hand_derived_example_on_the_device(pq):
    col = lambda *v: np.array(v, dtype=np.float64)[:, None]   # noqa: E731
    c = (col(1 / 2, 1 / 4, 1 / 4), col(1 / 4, 1 / 4, 1 / 2), (col(1.0, -1 / 2, NULL),), col(1 / 8, -1 / 8, 0.0), col(1 / 2, -5 / 16, 1 / 8),
         col(1 / 8, 1 / 4, -1 / 8), np.array([0, 1, 0], dtype=np.int32))
    got = raw(c, 2, bounds=[0, 1])
    same("totals", got["totals"][:, :, 0], [[3 / 64, 3 / 32, 1 / 32, 1 / 32, 13 / 64, 13 / 64], [1 / 64, 1 / 32, 0.0, 1 / 16, 7 / 64, 7 / 64],
                                             [1 / 32, 1 / 16, 1 / 32, -1 / 32, 3 / 32, 3 / 32]])
    assert got["n"][:, :, 0].tolist() == [[3, 3, 2], [1, 1, 1], [0, 0, 0]]
    check("the example", got, expected(c, 2, bounds=[0, 1]))


def test_doubled_holdings_double_every_output_on_the_device(pq):
    h, b, xs, u, r, f, ind = case(300, 70, 3, 5, "1d")
    one = raw((h, b, xs, u, r, f, ind), 5, bounds=[0, 30, 70])
    two = raw((2.0 * h, 2.0 * b, xs, u, r, f, ind), 5, bounds=[0, 30, 70])
    for k in ("exposure", "contribution", "totals", "period_sum"):
        same(k, two[k], 2.0 * one[k])
    same("mean, std", two["summary"][..., 1:3], 2.0 * one["summary"][..., 1:3])
    same("n_days, t, p", two["summary"][..., [0, 3, 4]], one["summary"][..., [0, 3, 4]])
    same("n", two["n"], one["n"])
    same("period_days", two["period_days"], one["period_days"])


# ---------------------------------------------------------------- refusals and empty calls
def test_refusals_write_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, ctx = lib(), api.ctx()
    N, T, K, G = 40, 20, 2, 3
    c = case(N, T, K, G, "1d")
    h, b, xs, u, r, f, ind = c
    M, P, S = K + G, 3, 2
    NS = M + 6
    hd, bd, ud, rd, xd, fd = to_dev(h), to_dev(b), to_dev(u), to_dev(r), [to_dev(x) for x in xs], to_dev(f)
    gd = torch.from_numpy(np.array(ind)).cuda()
    outs = [f64_buf(P * M * T), f64_buf(P * M * T), f64_buf(P * 6 * T), i32_buf(3 * P * T), f64_buf(P * NS * 5), f64_buf(P * NS * S),
            i32_buf(P * S)]
    bb = Batch(N, T, T)
    bounds = [0, 7, T]

    def status(bb=bb, h_=hd, b_=bd, cols=xd, k=K, g_=gd, gs=0, G_=G, f_=fd, frs=T, u_=ud, r_=rd, bounds_=bounds, S_=S, outs_=outs, ptrs=True):
        p = (C.c_void_p * max(len(cols), 1))(*[None if x is None else x.data_ptr() for x in cols]) if ptrs else None
        bp = None if bounds_ is None else np.asarray(bounds_, dtype=np.int64)
        s = api._call("pq_return_attribution", hd.device, bb, h_, b_, p, k, g_, gs, G_, f_, frs, u_, r_, bp, S_, *outs_, checked=False)
        return s, L.pq_last_error().decode()
    bad = [(dict(k=-1), "k must be in [0, 8]"), (dict(k=9), "k must"), (dict(G_=0), "n_groups"), (dict(G_=257), "n_groups"),
           (dict(g_=None), "n_groups must be 1"), (dict(g_=torch.zeros((N, T), dtype=torch.int32, device="cuda"), gs=T - 1), "group_stride"),
           (dict(gs=-1), "group_stride"), (dict(frs=T - 1), "fr_stride"), (dict(S_=-1), "period_bounds"), (dict(bounds_=None), "period_bounds"),
           (dict(S_=0), "period_bounds"), (dict(bounds_=[0, 0, T]), "strictly ascending"), (dict(bounds_=[-1, 7, T]), "strictly ascending"),
           (dict(bounds_=[0, 7, T + 1]), "strictly ascending"), (dict(bounds_=[7, 3, T]), "strictly ascending"),
           (dict(h_=None), "null pointer"), (dict(ptrs=False), "null pointer"), (dict(cols=[xd[0], None]), "null exposure"),
           (dict(f_=None), "null pointer"), (dict(u_=None), "null pointer")]
    bad += [(dict(outs_=outs[:j] + [None] + outs[j + 1:]), "null pointer") for j in range(7)]
    # an output on an input, and two outputs on each other
    bad += [(dict(outs_=[hd] + outs[1:]), "must not overlap an input"), (dict(outs_=outs[:2] + [fd] + outs[3:]), "must not overlap an input"),
            (dict(outs_=outs[:4] + [ud] + outs[5:]), "must not overlap an input"), (dict(outs_=outs[:5] + [rd] + outs[6:]), "must not overlap an input"),
            (dict(outs_=[outs[1]] + outs[1:]), "must not overlap each other"), (dict(outs_=outs[:5] + [outs[4]] + outs[6:]), "must not overlap each other")]
    for kw, msg in bad:
        s, err = status(**kw)
        assert s == 1 and msg in err and "pq_return_attribution" in err, (kw.keys(), s, err)            # PQ_ERR_ARG
    off = torch.tensor([0, 10, 25, N * T], dtype=torch.int64, device="cuda")
    s, err = status(bb=Batch(3, N * T - 25, N * T, C.c_void_p(off.data_ptr())), bounds_=None, S_=0)
    assert s == 5 and "ragged" in err, (s, err)                                                        # PQ_ERR_UNSUPPORTED
    assert L.pq_suite_begin(ctx, C.byref(bb)) == 0
    try:
        s, err = status()
        assert s == 5 and "recorded" in err, (s, err)
    finally:
        assert L.pq_suite_abort(ctx) == 0
    torch.cuda.synchronize()
    assert all(bool((o == (ISENT if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs), "a refused call wrote"
    assert bool((hd == to_dev(h)).logical_or(hd != hd).all()), "a refused call wrote to an input"
    for kw in (dict(bb=Batch(0, T, T)), dict(bb=Batch(N, 0, 0), bounds_=None, S_=0, frs=0)):           # nothing launched, nothing needed
        s, err = status(h_=None, b_=None, f_=None, u_=None, r_=None, outs_=[None] * 7, ptrs=False, **kw)
        assert s == 0, err
    s, err = status()                                                                                  # the context computes again
    assert s == 0, err
    torch.cuda.synchronize()
    exp = expected(c, G, bounds=bounds)
    same("totals after the refusals", host(outs[2][:P * 6 * T]).reshape(P, 6, T), exp["totals"])
    same("period_days after the refusals", host(outs[6][:P * S]).reshape(P, S), exp["period_days"])


def test_empty_calls_through_the_api(pq):
    from polars_quant_amd import api
    for n, T in ((0, 30), (3, 0)):
        z = torch.empty((n, 32), dtype=torch.float64, device="cuda")[:, :T]
        f = torch.zeros((3, T), dtype=torch.float64, device="cuda")             # K = 1, G = 2
        out = api.return_attribution(z, [z], f, z, torch.ones(n, dtype=torch.int64), next_return=z, benchmark=z,
                                     periods=None if T == 0 else 4)
        assert tuple(out["exposure"].shape) == (3, 3, T) == tuple(out["contribution"].shape)
        assert tuple(out["total"].shape) == (3, T) and tuple(out["n_held"].shape) == (3, T) and tuple(out["summary"].shape) == (3, 9, 5)
        assert A.isnull(host(out["total"])).all() and A.isnull(host(out["exposure"])).all() and (host(out["n_held"]) == 0).all()
        s = host(out["summary"])
        assert (s[..., 0] == 0.0).all() and A.isnull(s[..., 1:]).all()
        if T:
            assert tuple(out["period_sum"].shape) == (3, 9, 4) and (host(out["period_sum"]) == 0.0).all()
            assert (host(out["period_days"]) == 0).all() and host(out["period_bounds"]).tolist() == [0, 8, 16, 23, 30]


# ---------------------------------------------------------------- the api and the Factor method
def test_the_api_on_pitched_and_host_inputs(pq):
    from polars_quant_amd import api
    N, T, K, G = 257, 65, 2, 5
    c = case(N, T, K, G, "2d")
    h, b, xs, u, r, f, ind = (np.array(c[0]), np.array(c[1]), [np.array(x) for x in c[2]], np.array(c[3]), np.array(c[4]), np.array(c[5]),
                              np.where((c[6] >= 0) & (c[6] < G), c[6], -1))       # (the api sizes G by the largest code: the others become -1)
    exp = expected(c, G, bounds=[0, 22, 44, 65])
    for dev in (lambda a: to_dev(a, 80), np.array):
        out = api.return_attribution(dev(h), [dev(x) for x in xs], dev(f), dev(u), np.array(ind), next_return=dev(r), benchmark=dev(b), periods=3)
        assert set(out) == {"exposure", "contribution", "style", "industry", "specific", "unexplained", "total", "realized", "n_held",
                            "n_uncovered", "n_missing", "summary", "period_sum", "period_days", "period_bounds"}
        same("exposure", host(out["exposure"]), exp["exposure"])
        same("contribution", host(out["contribution"]), exp["contribution"])
        for j, k in enumerate(A.TOTALS):
            same(k, host(out[k]), exp["totals"][:, j])
        for j, k in enumerate(("n_held", "n_uncovered", "n_missing")):
            same(k, host(out[k]), exp["n"][j])
        same_summary("summary", host(out["summary"]), exp["summary"])
        same("period_sum", host(out["period_sum"]), exp["period_sum"])
        same("period_days", host(out["period_days"]), exp["period_days"])
        assert host(out["period_bounds"]).tolist() == [0, 22, 44, 65]
    one = api.return_attribution(h, np.stack(xs), f, u, torch.from_numpy(np.array(ind)))               # P = 1, a stacked [K, N, T] array
    e1 = expected(c, G, bench=False, next_return=False)
    assert "period_sum" not in one and tuple(one["total"].shape) == (1, T)
    same("P = 1: total", host(one["total"]), e1["totals"][:, 4])
    assert A.isnull(host(one["realized"])).all()
    row = api.return_attribution(h[:1], None, f[K:K + 1], u[:1])                                       # one series, K = 0, no codes
    same("one row", host(row["total"]), A.attribution(h[:1], [], f[K:K + 1], u[:1])["totals"][:, 4])


def test_the_chain_from_the_regression_to_the_attribution(pq):
    """pure_factor_return -> risk_model -> optimal_portfolio -> weights_backtest(holdings=0) -> return_attribution on clean data: every
    held symbol is covered, nothing is missing, and total equals realized within the identity bound on every day with a book"""
    rng = np.random.default_rng(36)
    N, T, K, G = 120, 200, 2, 4
    xs = [rng.standard_normal((N, T)) for _ in range(K)]
    ind = np.arange(N) % G
    r = 0.02 * rng.standard_normal((N, T)) + 0.01 * rng.standard_normal((G, T))[ind]
    for x in xs:
        r = r + 0.005 * rng.standard_normal(T)[None, :] * x
    price = np.empty((N, T))
    price[:, 0] = 10.0
    price[:, 1:] = 10.0 * np.cumprod(1.0 + r[:, :-1], axis=1)                                          # r[t] leads from price[t] to price[t + 1]
    nxt = np.concatenate([price[:, 1:] / price[:, :-1] - 1.0, r[:, -1:]], axis=1)
    cols, rd, gd = [to_dev(x) for x in xs], to_dev(nxt), torch.from_numpy(ind)
    fac = pq.Factor()
    reg = fac.pure_factor_return(cols, rd, None, gd, specific_return=True)
    model = fac.risk_model(reg, window=60, halflife=20.0, step=20)
    opt = fac.optimal_portfolio(cols, model, industry=gd)
    bt = fac.weights_backtest(opt, to_dev(price), lag=1, cost_rate=0.0, holdings=0)
    bench = torch.full((N, T), 1.0 / N, dtype=torch.float64, device="cuda")
    out = fac.return_attribution(bt, cols, reg, gd, next_return=rd, benchmark=bench, periods=4)
    first = int(host(bt["rebalance_days"])[0])
    assert first == 60 and tuple(out["total"].shape) == (3, T)
    n_held, n_unc, n_miss = (host(out[k]) for k in ("n_held", "n_uncovered", "n_missing"))
    assert (n_miss == 0).all() and (n_unc == 0).all()
    assert (n_held[0, :first] == 0).all() and (n_held[0, first:] == N).all() and (n_held[1] == N).all()
    total, realized = host(out["total"]), host(out["realized"])
    assert A.isnull(total[0, :first]).all() and not A.isnull(total[0, first:]).any() and not A.isnull(total[1:]).any()
    H = np.stack([host(bt["holdings"]), np.full((N, T), 1.0 / N)])
    H = np.concatenate([H, (H[0] - H[1])[None]])
    scale = np.abs(H * nxt[None]).sum(axis=1)
    live = ~A.isnull(total)
    err = np.abs(total - realized)[live] / scale[live]
    print(f"chain: worst |total - realized| / sum |h r| = {err.max():.3e} over {int(live.sum())} (book, day) cells")
    assert err.max() <= IDENTITY_BOUND
    # the call is the restatement on the device's own regression, bit for bit
    block = np.concatenate([host(reg["factor_return"]), host(reg["industry_return"])])
    exp = A.attribution(H[0], xs, block, host(reg["specific_return"]), ind, G, nxt, H[1], [0, 50, 100, 150, 200])
    same("total", total, exp["totals"][:, 4])
    same("contribution", host(out["contribution"]), exp["contribution"])
    same_summary("summary", host(out["summary"]), exp["summary"])
    same("period_sum", host(out["period_sum"]), exp["period_sum"])
    assert host(out["period_days"]).tolist() == [[0, 40, 50, 50], [50] * 4, [50] * 4]
    with pytest.raises(ValueError, match="no specific_return"):
        fac.return_attribution(bt, cols, fac.pure_factor_return(cols, rd, None, gd), gd)
