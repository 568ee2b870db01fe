"""-m gpu: portfolio construction from the risk model, D-34 (csrc/xsec/risk_solve.hip), against the numpy restatement in
tests/xsec_solve_ref.py.  y, quad and n are compared bit for bit, on buffers prefilled with a sentinel and 16 cells longer than the
call may write, with pitched inputs; nothing beyond and no pitch cell may change.  The covariances and variances are the outputs of
pq_risk_factor_cov and pq_risk_specific_var themselves (with their holes).  Also: the NULL-rule days at the lanes 0, 63 and 64, the
refusals of the C entry point, empty batches, Factor.optimal_portfolio's three objectives, and the cross-check of the minimum-variance
weights with Factor.portfolio_risk (within the tolerance of tests/test_factor_solve_ref.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import xsec_risk_ref as R
import xsec_solve_cases as cases
import xsec_solve_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 7.0
ISENT = 77
TAIL = 16
NULL = S.NULL
DENSE_TOL = 1e-11                                            # tests/test_factor_solve_ref.py


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


# ---------------------------------------------------------------- the model and the raw call
@functools.lru_cache(maxsize=None)
def model(N, K, G, codes, D, step=1, seed=0):
    """a panel and its model: the two risk entries' own outputs on the device (the variance on a pitch of D + 3), equal to their
    restatement bit for bit -> (panel, cov, var, ecov, esv, days)"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    p = cases.panel(N, K, G, codes, D, step, seed)
    om = R.weights(cases.W, cases.W / 3.0)
    days = R.as_of_days(p["day0"], step, D)
    M, T = p["F"].shape
    cov = torch.full((D, M, M), SENTINEL, dtype=torch.float64, device="cuda")
    var = torch.full((N, D + 3), SENTINEL, dtype=torch.float64, device="cuda")
    fd, ed, od = to_dev(p["F"]), to_dev(p["E"]), to_dev(om)
    api._call("pq_risk_factor_cov", fd.device, Batch(M, T, T), fd, od, cases.W, 2, 1, p["day0"], step, D, cov, None)
    api._call("pq_risk_specific_var", fd.device, Batch(N, T, T), ed, od, cases.W, 2, 1, p["day0"], step, D, var, D + 3, None)
    torch.cuda.synchronize()
    var = var[:, :D]
    ecov, esv = R.factor_cov(p["F"], om, days, 2)[0], R.specific_var(p["E"], om, days, 2)[0]
    same("the model's cov", host(cov), ecov)
    same("the model's var", host(var), esv)
    return p, cov, var, ecov, esv, days


def rhs_of(p, spec):
    """'1': the vector of ones (NULL pointer), 'a' / 'b': the panel's columns"""
    return [None if c == "1" else p[c] for c in spec]


def solve_raw(rhs, X, ind, G, cov, var, day0, step, D, N, T, pitch=None, gpitch=None):
    """pq_risk_solve on sentinel-filled buffers; cov and var are device tensors (var an [N, D] view on its own pitch); y on a pitch of
    D + 5"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    K, R_ = len(X), len(rhs)
    stride = pitch or T
    vd = [None if v is None else to_dev(v, pitch) for v in rhs]
    xd = [to_dev(x, pitch) for x in X]
    gd, gs = None, 0
    if ind is not None and ind.ndim == 1:
        gd = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    elif ind is not None:
        gs = gpitch or stride
        gd = torch.full((N, gs), 3, dtype=torch.int32, device="cuda")
        gd[:, :T] = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    ys = D + 5
    ybuf = [f64_buf(N * ys) for _ in range(R_)]
    quad, n = f64_buf(R_ * R_ * D), i32_buf(2 * D)
    rp = (C.c_void_p * R_)(*[None if v is None else v.data_ptr() for v in vd])
    xp = (C.c_void_p * max(K, 1))(*[x.data_ptr() for x in xd])
    yp = (C.c_void_p * R_)(*[y.data_ptr() for y in ybuf])
    api._call("pq_risk_solve", cov.device, Batch(N, T, stride), rp, R_, xp, K, gd, gs, G, cov.contiguous(), var,
              var.stride(0) if N > 1 else D, day0, step, D, yp, ys, quad, n)
    torch.cuda.synchronize()
    y = np.empty((R_, N, D))
    for r, buf in enumerate(ybuf):
        assert bool((buf[N * ys:] == SENTINEL).all()), "y: written beyond its end"
        full = host(buf[:N * ys]).reshape(N, ys)
        assert (full[:, D:] == SENTINEL).all(), "y: its pitch cells changed"
        y[r] = full[:, :D]
    assert bool((quad[R_ * R_ * D:] == SENTINEL).all()) and bool((n[2 * D:] == ISENT).all()), "quad / n: written beyond their end"
    if pitch:
        for t in [v for v in vd if v is not None] + xd:
            assert bool((t.as_strided((N, pitch - T), (pitch, 1), T) == SENTINEL).all()), "an input's pitch cells changed"
    return {"y": y, "quad": host(quad[:R_ * R_ * D]).reshape(R_, R_, D), "n": host(n[:2 * D]).reshape(2, D)}


def check(tag, got, exp, min_days=1):
    live = (~exp["null"]).sum()
    assert live >= min_days, f"{tag}: the restatement solves {live} days"
    for k in ("n", "quad", "y"):
        same(f"{k} {tag}", got[k], exp[k])


SHAPES = [(1, 0, 1, None, 1, 1, "a"), (5, 1, 1, None, 63, 1, "1"), (255, 3, 4, "1d", 64, 3, "1a"), (256, 8, 31, "2d", 65, 1, "a1b1"),
          (257, 3, 4, "2d", 130, 1, "1a"), (600, 8, 120, "1d", 2, 1, "1a"), (600, 0, 1, None, 65, 3, "b"), (257, 1, 1, None, 64, 1, "ab"),
          (300, 8, 31, "1d", 66, 1, "1")]


@pytest.mark.parametrize("N,K,G,codes,D,step,spec", SHAPES, ids=[f"N{N}-K{K}-G{G}-{c}-D{D}+{s}-{r}" for N, K, G, c, D, s, r in SHAPES])
def test_solve_at_every_size_class(pq, N, K, G, codes, D, step, spec):
    """N on both sides of the block of 256 symbols and of two blocks, D on both sides of the 64 as-of days of a workgroup, every K and G
    class up to M = 128 (the cap, and the moments pass in chunks of one column), one, two and four right-hand sides with and without
    the vector of ones, [N] and [N, T] codes on a pitch of their own"""
    p, cov, var, ecov, esv, days = model(N, K, G, codes, D, step)
    rhs = rhs_of(p, spec)
    if N == 1:
        rhs = [np.full((1, p["T"]), 0.5)]
    exp = S.solve(rhs, list(p["X"]), ecov, esv, days, p["ind"], G)
    got = solve_raw(rhs, list(p["X"]), p["ind"], G, cov, var, p["day0"], step, D, N, p["T"], pitch=p["T"] + 5, gpitch=p["T"] + 9)
    check(f"N={N} K={K} G={G} D={D} rhs={spec}", got, exp, min_days=min(D, 2))
    if (K, G) == (8, 120):
        assert exp["u"].shape[2] == 128 and (exp["u"][0, 0] != 0.0).all(), "every one of the 128 rows takes part"


@pytest.mark.parametrize("rot", [0, 3])
def test_null_rule_days_at_lanes_0_63_64(pq, rot):
    """the constructed as-of days: nothing in U, uncovered symbols (an exposure, a code, a variance that is NULL, zero or negative), a
    NULL covariance between two active rows, an industry without a member whose covariances are NULL, a factor that is zero on all of
    U whose covariances are NULL, and an rhs without a valid cell; three of the six on the as-of days 0, 63 and 64, the others on 1, 62
    and 65; the second rotation swaps the halves"""
    N, K, G, D = 300, 3, 7, 130
    p, cov, var, ecov, esv, days = model(N, K, G, "2d", D, 1, seed=rot)
    day0, T = p["day0"], p["T"]
    X, a, ind = p["X"].copy(), p["a"].copy(), p["ind"].copy()
    cov, var, ecov, esv = cov.clone(), var.clone(), ecov.copy(), esv.copy()
    kinds = ["empty", "uncovered", "null_cov", "absent", "zero_factor", "no_rhs"]
    kinds = kinds[rot:] + kinds[:rot]
    day_of = dict(zip(kinds, [0, 63, 64, 1, 62, 65]))

    def poke(dev, ref, idx, v):
        ref[idx] = v
        dev[idx] = torch.from_numpy(np.array(v, dtype=np.float64)).cuda()   # (a tensor copy keeps NULL's payload)
    d = day_of["empty"]
    for s in range(N):
        poke(var, esv, (s, d), NULL if s % 2 else 0.0)
    d = day_of["uncovered"]
    X[1, 10, day0 + d] = NULL
    ind[11, day0 + d] = G
    ind[12, day0 + d] = -1
    poke(var, esv, (13, d), NULL)
    poke(var, esv, (14, d), 0.0)
    poke(var, esv, (15, d), -1e-9)
    d = day_of["null_cov"]
    poke(cov, ecov, (d, 2, K + 1), NULL)
    d = day_of["absent"]
    ind[ind[:, day0 + d] == 4, day0 + d] = 5
    for l in range(K + G):
        poke(cov, ecov, (d, K + 4, l), NULL)
        poke(cov, ecov, (d, l, K + 4), NULL)
    d = day_of["zero_factor"]
    X[0, :, day0 + d] = 0.0
    for l in range(K + G):
        poke(cov, ecov, (d, 0, l), NULL)
        poke(cov, ecov, (d, l, 0), NULL)
    d = day_of["no_rhs"]
    a[:, day0 + d] = np.where(np.arange(N) % 2 == 0, NULL, np.inf)
    rhs = [None, a]
    exp = S.solve(rhs, list(X), ecov, esv, days, ind, G)
    n, null = exp["n"], exp["null"]
    for k in ("empty", "null_cov", "no_rhs"):
        assert null[day_of[k]] and S.isnull(exp["quad"][:, :, day_of[k]]).all() and S.isnull(exp["y"][:, :, day_of[k]]).all(), k
    assert n[0, day_of["empty"]] == 0 and n[1, day_of["empty"]] > 0 and n[:, day_of["no_rhs"]].tolist() == [0, 0]
    for k in ("uncovered", "absent", "zero_factor"):
        assert not null[day_of[k]] and not S.isnull(exp["quad"][:, :, day_of[k]]).any(), k
    d = day_of["uncovered"]
    assert S.isnull(exp["y"][0, 10:16, d]).all() and n[1, d] >= 6 - S.isnull(a[10:16, day0 + d]).sum()
    assert (exp["u"][:, day_of["absent"], K + 4] == 0.0).all() and (exp["u"][:, day_of["zero_factor"], 0] == 0.0).all()
    got = solve_raw(rhs, list(X), ind, G, cov, var, day0, 1, D, N, T, pitch=T + 3)
    check(f"special days rot={rot}", got, exp, min_days=60)


def test_a_zero_pivot_and_the_hand_example(pq):
    """S = 1 + F A = 0 exactly on day 0 (tests/test_factor_solve_ref.py); the hand-derived example's integers"""
    sv = torch.full((4, 2), 0.25, dtype=torch.float64, device="cuda")
    F = torch.tensor([[[-1.0 / 16.0]], [[-1.0 / 8.0]]], dtype=torch.float64, device="cuda")
    got = solve_raw([None], [], None, 1, F, sv, 0, 1, 2, 4, 2)
    exp = S.solve([None], [], host(F), host(sv), [0, 1])
    assert exp["null"].tolist() == [True, False]
    check("zero pivot", got, exp)
    x, alpha, ind, F, sv = cases.hand()
    got = solve_raw([None, alpha], [x], ind, 2, to_dev(F), to_dev(sv), 0, 1, 1, 4, 1)
    assert got["y"][:, :, 0].tolist() == [[2.0, -2.0, 4.0, 4.0], [10.0, -12.0, -4.0, 0.0]]
    assert got["quad"][:, :, 0].tolist() == [[8.0, -6.0], [-6.0, -10.0]] and got["n"].tolist() == [[4], [0]]


# ---------------------------------------------------------------- the C entry point's refusals and empty batches
def test_refusals_write_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    N, K, G, D = 40, 2, 3, 9
    p, cov, var, ecov, esv, days = model(N, K, G, "1d", D)
    day0, T, M = p["day0"], p["T"], K + G
    ad, xd = to_dev(p["a"]), [to_dev(x) for x in p["X"]]
    gd = torch.from_numpy(np.array(p["ind"])).cuda()
    ys = [f64_buf(N * D), f64_buf(N * D)]
    quad, n = f64_buf(4 * D), i32_buf(2 * D)
    b = Batch(N, T, T)
    cv = cov.contiguous()

    def status(bb=b, rhs=(None, ad), R_=2, cols=xd, k=K, g_=gd, gs=0, G_=G, cov_=cv, sv_=var, svs=None, day0_=day0, step=1, count=D,
               ys_=ys, os_=D, quad_=quad, n_=n, rptr=True, xptr=True, yptr=True):
        rp = (C.c_void_p * 4)(*[None if v is None else v.data_ptr() for v in rhs]) if rptr else None
        xp = (C.c_void_p * 9)(*[None if c is None else c.data_ptr() for c in cols]) if xptr else None
        yp = (C.c_void_p * 4)(*[None if y is None else y.data_ptr() for y in ys_]) if yptr else None
        s = api._call("pq_risk_solve", ad.device, bb, rp, R_, xp, k, g_, gs, G_, cov_, sv_, var.stride(0) if svs is None else svs, day0_,
                      step, count, yp, os_, quad_, n_, checked=False)
        return s, L.pq_last_error().decode()
    bad = [(dict(R_=0), "n_rhs must be in [1, 4]"), (dict(R_=5), "n_rhs must"), (dict(k=-1), "k must be in [0, 8]"), (dict(k=9), "k must"),
           (dict(G_=0), "n_groups"), (dict(G_=257), "n_groups"), (dict(g_=None), "n_groups must be 1"),
           (dict(g_=torch.zeros((N, T), dtype=torch.int32, device="cuda"), gs=T - 1), "group_stride"), (dict(gs=-1), "group_stride"),
           (dict(svs=D - 1), "sv_stride"), (dict(os_=D - 1), "out_stride"), (dict(day0_=-1), "as-of days"), (dict(step=0), "as-of days"),
           (dict(count=-1), "as-of days"), (dict(day0_=day0 + 1), "as-of days"), (dict(rptr=False), "null pointer"),
           (dict(xptr=False), "null pointer"), (dict(yptr=False), "null pointer"), (dict(cols=[xd[0], None]), "null exposure"),
           (dict(ys_=[ys[0], None]), "null output"), (dict(cov_=None), "null pointer"), (dict(sv_=None), "null pointer"),
           (dict(quad_=None), "null pointer"), (dict(n_=None), "null pointer"), (dict(ys_=[ys[0], ad]), "must not overlap an input"),
           (dict(ys_=[ys[0], xd[1]]), "must not overlap an input"), (dict(quad_=cv), "must not overlap an input"),
           (dict(ys_=[ys[0], ys[0]]), "must not overlap each other"), (dict(n_=quad.view(torch.int32)), "must not overlap each other")]
    for kw, msg in bad:
        s, err = status(**kw)
        assert s == 1 and msg in err and "pq_risk_solve" in err, (kw.keys(), s, err)                    # PQ_ERR_ARG
    s, err = status(G_=127, g_=gd)                                                                     # M = 129
    assert s == 5 and "128" in err and "PQ_RISK_SOLVE_MAX_M" in err, (s, err)                          # PQ_ERR_UNSUPPORTED
    off = torch.tensor([0, 10, 25, N * T], dtype=torch.int64, device="cuda")
    s, err = status(bb=Batch(3, N * T - 25, N * T, C.c_void_p(off.data_ptr())))
    assert s == 5 and "ragged" in err, (s, err)
    assert L.pq_suite_begin(h, C.byref(b)) == 0
    try:
        s, err = status()
        assert s == 5 and "recorded" in err, (s, err)
    finally:
        assert L.pq_suite_abort(h) == 0
    torch.cuda.synchronize()
    assert all(bool((o == (ISENT if o.dtype == torch.int32 else SENTINEL)).all()) for o in ys + [quad, n]), "a refused call wrote"
    # the empty batches: PQ_OK, nothing launched, no pointer needed
    for bb, cnt in ((b, 0), (Batch(0, T, T), D), (Batch(N, 0, 0), 0)):
        s, err = status(bb=bb, count=cnt, rptr=False, xptr=False, yptr=False, cov_=None, sv_=None, quad_=None, n_=None, g_=None, G_=1)
        assert s == 0, err
    torch.cuda.synchronize()
    assert all(bool((o == (ISENT if o.dtype == torch.int32 else SENTINEL)).all()) for o in ys + [quad, n]), "an empty call wrote"
    s, err = status()                                                                                  # the context computes again
    assert s == 0, err
    torch.cuda.synchronize()
    exp = S.solve([None, p["a"]], list(p["X"]), ecov, esv, days, p["ind"], G)
    same("quad after the refusals", host(quad[:4 * D]).reshape(2, 2, D), exp["quad"])
    same("y after the refusals", host(ys[1][:N * D]).reshape(N, D), exp["y"][1])


def test_empty_batches_through_the_api(pq):
    from polars_quant_amd import api
    z = torch.empty((0, 30), dtype=torch.float64, device="cuda")
    y, quad, n = api.risk_solve([None, z], [z], torch.zeros((5, 2, 2), dtype=torch.float64, device="cuda"),
                                torch.empty((0, 5), dtype=torch.float64, device="cuda"), day0=3, step=2)
    assert tuple(y.shape) == (2, 0, 5) and S.isnull(host(quad)).all() and tuple(quad.shape) == (2, 2, 5) and (host(n) == 0).all()
    x = to_dev(np.ones((3, 30)))
    y, quad, n = api.risk_solve([x], None, torch.zeros((0, 1, 1)), torch.zeros((3, 0)))
    assert tuple(y.shape) == (1, 3, 0) and tuple(quad.shape) == (1, 1, 0) and tuple(n.shape) == (2, 0)


# ---------------------------------------------------------------- the api and the Factor method
@pytest.fixture(scope="module")
def api_case(pq):
    N, K, G, D, step = 300, 3, 7, 20, 3
    p, cov, var, ecov, esv, days = model(N, K, G, "1d", D, step)
    rhs = [None, p["a"]]
    return p, cov, var, days, S.solve(rhs, list(p["X"]), ecov, esv, days, p["ind"], G), (N, K, G, D, step)


def test_the_api_on_pitched_and_host_inputs(pq, api_case):
    from polars_quant_amd import api
    p, cov, var, days, exp, (N, K, G, D, step) = api_case
    T = p["T"]
    for conv in (lambda v: to_dev(v, T + 6), np.array):
        y, quad, n = api.risk_solve([None, conv(p["a"])], [conv(x) for x in p["X"]], cov, var, np.array(p["ind"]), p["day0"], step)
        same("y", host(y), exp["y"])
        same("quad", host(quad), exp["quad"])
        same("n", host(n), exp["n"])
    y, quad, n = api.risk_solve([None], np.array(p["X"]), host(cov), host(var), torch.from_numpy(np.array(p["ind"])), p["day0"], step)
    one = S.solve([None], list(p["X"]), host(cov), host(var), days, p["ind"], G)
    same("ones alone, one [K, N, T] array: y", host(y), one["y"])
    same("ones alone: quad", host(quad), one["quad"])


@pytest.mark.parametrize("objective,lam", [("min_variance", 1.0), ("max_sharpe", 1.0), ("mean_variance", 1.0), ("mean_variance", 7.5)])
def test_optimal_portfolio_objectives(pq, api_case, objective, lam):
    p, cov, var, days, exp, (N, K, G, D, step) = api_case
    m = {"factor_cov": cov, "specific_var": var, "day0": p["day0"], "step": step}
    gd = torch.from_numpy(np.array(p["ind"]))
    out = pq.Factor().optimal_portfolio([to_dev(x) for x in p["X"]], m, to_dev(p["a"]), gd, objective, lam)
    assert set(out) == {"weights", "predicted_var", "expected_return", "n_universe", "n_uncovered", "days"}
    w, v, r = S.optimal(exp["y"], exp["quad"], objective, lam)
    same("weights", host(out["weights"]), w)
    same("predicted_var", host(out["predicted_var"]), v)
    same("expected_return", host(out["expected_return"]), r)
    same("n_universe", host(out["n_universe"]), exp["n"][0])
    same("n_uncovered", host(out["n_uncovered"]), exp["n"][1])
    assert host(out["days"]).tolist() == days.tolist() and out["days"].dtype == torch.int64
    assert (~S.isnull(v)).sum() >= (D // 2 if objective != "max_sharpe" else 1)


def test_min_variance_without_alpha_and_portfolio_risk(pq):
    """step = 1, day0 = 0: feeding the minimum-variance weights to Factor.portfolio_risk gives total_var = predicted_var within the
    dense-solve tolerance on the days where nothing is uncovered (a NULL weight is not held)"""
    N, K, G, D = 300, 3, 7, 40
    p = cases.panel(N, K, G, "1d", D)
    rng = np.random.default_rng(3)
    X = np.where(S.isnull(p["X"]), 0.25, p["X"])[:, :, :D]      # every exposure there: nothing uncovered but symbol 1's variance
    F = np.cov(rng.normal(0.0, 0.01, (260, K + G)).T)
    cov = to_dev(np.repeat(F[None], D, axis=0))
    sv = rng.uniform(0.01, 0.03, (N, D)) ** 2
    sv[1, D // 2:] = NULL
    var = to_dev(sv)
    fac = pq.Factor()
    m = {"factor_cov": cov, "specific_var": var, "day0": 0, "step": 1}
    cols, gd = [to_dev(x) for x in X], torch.from_numpy(np.array(p["ind"]))
    out = fac.optimal_portfolio(cols, m, industry=gd)
    exp = S.solve([None], list(X), host(cov), sv, np.arange(D), p["ind"], G)
    w, v, r = S.optimal(exp["y"], exp["quad"], "min_variance")
    same("weights", host(out["weights"]), w)
    same("predicted_var", host(out["predicted_var"]), v)
    assert S.isnull(host(out["expected_return"])).all() and not S.isnull(v).any()
    assert exp["n"][1].tolist() == [0] * (D // 2) + [1] * (D - D // 2)
    risk = fac.portfolio_risk(out["weights"], cols, m, gd)
    tot, pv = host(risk["total_var"]), host(out["predicted_var"])
    assert (host(risk["n_uncovered"]) == 0).all() and not S.isnull(tot).any()
    dev = np.abs(tot - pv) / pv
    print(f"portfolio_risk against predicted_var: worst deviation {dev.max():.3g}")
    assert (dev <= DENSE_TOL).all()
    wsum = np.where(S.isnull(w), 0.0, w).sum(axis=0)
    assert (np.abs(wsum - 1.0) <= DENSE_TOL * np.abs(np.where(S.isnull(w), 0.0, w)).max(axis=0)).all()
