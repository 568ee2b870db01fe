"""-m gpu: linear(), the pooled OLS of D-24 (csrc/xsec/linear.hip), against the numpy restatement in tests/linear_ref.py, through
api.linear, pq.linear and the C entry point.  coef / t / R^2 / n / pred / resid are compared bit for bit; p-values against
scipy.special.stdtr within |dp| <= 1e-11 p + 1e-300.  Sizes sit on both sides of every boundary of the reduction: the wave (64), the
tile (api.LINEAR_TILE) and the second stage's step (api.LINEAR_STAGE2 tiles)."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import linear_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from polars_quant_amd import api as _api  # noqa: E402  (constants only: the library is loaded by the fixture)

TILE, STAGE2 = _api.LINEAR_TILE, _api.LINEAR_STAGE2
README_R2 = float(Fraction(375390625, 1462890625))   # Sxy^2 / (Sxx Syy) of the README's market_cap -> return example, 0.25660881175


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd import api
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    assert (R.TILE, R.STAGE2) == (TILE, STAGE2), "the restatement sums in other tiles than the library"
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


@functools.lru_cache(maxsize=None)
def make(K, shape, seed, holes=False):
    """K regressors and y in `shape` ((M,) or (N, T)): unit spread on offsets, noise of the signal's size; holes: 3 % NULL and 2 % NaN in
    x, 3 % NULL and 1 % inf in y.  The arrays are shared between the tests: nobody writes into them."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K,) + shape) + rng.uniform(-10.0, 10.0, (K,) + (1,) * len(shape))
    y = 0.5 + (0.25 * np.arange(1, K + 1).reshape((K,) + (1,) * len(shape)) * X).sum(0) + K * 0.5 * rng.standard_normal(shape)
    if holes:
        X[rng.random(X.shape) < 0.03] = R.NULL
        X[rng.random(X.shape) < 0.02] = np.nan
        y[rng.random(shape) < 0.03] = R.NULL
        y[rng.random(shape) < 0.01] = np.inf
    return X, y


def compare(tag, got, exp, outputs=True):
    """an api.linear result against a linear_ref.linear result"""
    same(f"coef {tag}", got["coef"].cpu().numpy(), exp["coef"])
    same(f"t {tag}", got["t_stat"].cpu().numpy(), exp["t"])
    same(f"r2 {tag}", got["r_squared"].cpu().numpy().reshape(1), np.asarray(exp["r2"]).reshape(1))
    assert got["n"].dtype == torch.int64 and got["n"].dim() == 0 and got["r_squared"].dim() == 0
    assert int(got["n"]) == exp["n"], f"n {tag}: {int(got['n'])} vs {exp['n']}"
    close_p(f"p {tag}", got["p_value"].cpu().numpy(), exp["p"])
    if outputs:
        same(f"pred {tag}", got["pred"].cpu().numpy(), exp["pred"])
        same(f"resid {tag}", got["resid"].cpu().numpy(), exp["resid"])
    else:
        assert "pred" not in got and "resid" not in got


def check(pq, X, y, tag, surface=True):
    """X [K, ...], y on the host -> api.linear with and without the output columns and (surface) pq.linear on device columns, against
    the restatement (computed once)"""
    from polars_quant_amd import api
    exp = R.linear(list(X), y)
    dx, dy = [to_dev(x) for x in X], to_dev(y)
    got = api.linear(dx, dy)
    compare(tag, got, exp)
    compare(tag + " outputs=False", api.linear(dx, dy, outputs=False), exp, outputs=False)
    if surface:
        cols = {f"x{j}": d for j, d in enumerate(dx)}
        cols["y"] = dy
        out, (coefs, r2) = pq.linear(cols, [f"x{j}" for j in range(len(dx))], "y", return_stats=True)
        same(f"pq pred {tag}", out["pred"].cpu().numpy(), exp["pred"])
        same(f"pq resid {tag}", out["resid"].cpu().numpy(), exp["resid"])
        same(f"pq coef {tag}", np.array(coefs), np.append(exp["coef"][-1:], exp["coef"][:-1]))
        same(f"pq r2 {tag}", np.array([r2]), np.asarray(exp["r2"]).reshape(1))
    return got, exp


# ---- sizes
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_small_sizes(pq, K):
    for M in (0, 1, K + 1, K + 2, 63, 64, 65):
        X, y = make(K, (M,), 100 * K + M)
        got, exp = check(pq, X, y, f"K={K} M={M}")
        assert R.isnull(exp["coef"]).all() == (M < K + 2)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("M", [TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_tile_sizes(pq, K, M):
    X, y = make(K, (M,), K + M)
    check(pq, X, y, f"K={K} M={M}")


def test_second_stage_step(pq):
    M = (STAGE2 + 1) * TILE + 5
    assert M < 8_000_000
    X, y = make(1, (M,), 31)
    check(pq, X, y, f"K=1 M={M}", surface=False)


# ---- pitch
def abi_linear(xs, y, pred=None, resid=None):
    """pq_linear on device views of one pitch (xs, y: [N, T] views or [M] columns) -> (coef, t, p, r2, n) tensors; pred / resid: the
    caller's buffers on that pitch"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    vp = C.c_void_p
    n, T = (1, y.shape[0]) if y.dim() == 1 else y.shape
    b = Batch(n, T, T if y.dim() == 1 else y.stride(0))
    K = len(xs)
    ptrs = (vp * K)(*[x.data_ptr() for x in xs])
    f64 = dict(dtype=torch.float64, device="cuda")
    coef, t, p, r2 = torch.empty(K + 1, **f64), torch.empty(K + 1, **f64), torch.empty(K + 1, **f64), torch.empty((), **f64)
    nn = torch.empty((), dtype=torch.int64, device="cuda")
    ok(lib().pq_linear(api.ctx(), C.byref(b), ptrs, C.c_int32(K), vp(y.data_ptr()), vp(coef.data_ptr()), vp(t.data_ptr()),
                       vp(p.data_ptr()), vp(r2.data_ptr()), vp(nn.data_ptr()), vp(pred.data_ptr()) if pred is not None else None,
                       vp(resid.data_ptr()) if resid is not None else None))
    torch.cuda.synchronize()
    return coef, t, p, r2, nn


@pytest.mark.parametrize("shape,pitch", [((37, 50), 64), ((300, 131), 136)])
@pytest.mark.parametrize("K", [1, 3])
def test_pitched_matrix_equals_its_flat_column(pq, shape, pitch, K):
    from polars_quant_amd import api
    X, y = make(K, shape, pitch + K, holes=True)
    n, T = shape
    flat = api.linear([to_dev(x.reshape(-1)) for x in X], to_dev(y.reshape(-1)))
    compare(f"flat {shape}", flat, R.linear([x.reshape(-1) for x in X], y.reshape(-1)))
    dx, dy = [to_dev(x, pitch) for x in X], to_dev(y, pitch)
    got = api.linear(dx, dy)                                           # the public call keeps the pitch of its inputs
    assert got["pred"].shape == shape and got["pred"].stride(0) == pitch
    pred = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    resid = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    coef, t, p, r2, nn = abi_linear(dx, dy, pred, resid)               # the entry point on buffers whose padding is watched
    for name, a, b_, c in (("coef", got["coef"], coef, flat["coef"]), ("t", got["t_stat"], t, flat["t_stat"]),
                           ("p", got["p_value"], p, flat["p_value"]), ("r2", got["r_squared"].reshape(1), r2.reshape(1), flat["r_squared"].reshape(1))):
        same(f"{name} api {shape}", a.cpu().numpy(), c.cpu().numpy())
        same(f"{name} abi {shape}", b_.cpu().numpy(), c.cpu().numpy())
    assert int(got["n"]) == int(nn) == int(flat["n"])
    for name, a, b_ in (("pred", got["pred"], pred), ("resid", got["resid"], resid)):
        same(f"{name} api {shape}", a.cpu().numpy().reshape(-1), flat[name].cpu().numpy())
        same(f"{name} abi {shape}", b_[:, :T].cpu().numpy().reshape(-1), flat[name].cpu().numpy())
        assert bool((b_[:, T:] == 7.0).all()), f"{name}: the padding was written"
    for d in dx + [dy]:
        assert bool((d._base[:, T:] == 7.0).all()), "an input's padding was written"


# ---- holes
@pytest.mark.parametrize("K", [1, 3, 8])
def test_holes(pq, K):
    X, y = make(K, (3 * TILE + 17,), 7 * K, holes=True)
    got, exp = check(pq, X, y, f"holes K={K}", surface=K == 3)
    assert 0 < exp["n"] < y.size and R.isnull(exp["resid"]).sum() > R.isnull(exp["pred"]).sum() > 0


def test_a_tile_without_members_and_members_in_the_last_tile_only(pq):
    X, y = make(2, (3 * TILE + 17,), 19, holes=True)
    y1 = y.copy()
    y1[TILE:2 * TILE] = R.NULL                                         # tile 1: a zero-count partial
    got, exp = check(pq, X, y1, "empty tile", surface=False)
    assert R.isnull(exp["resid"][TILE:2 * TILE]).all() and not R.isnull(exp["pred"][TILE:2 * TILE]).all()
    X, y = make(1, (3 * TILE + 17,), 23)
    y2 = y.copy()
    y2[:3 * TILE] = np.nan                                             # members only in the ragged last tile
    got, exp = check(pq, X, y2, "last tile only", surface=False)
    assert exp["n"] == 17 and not R.isnull(exp["coef"]).any()
    x2 = X.copy()
    x2[:, :3 * TILE] = R.NULL                                          # ... and no prediction in front of it either
    got, exp = check(pq, x2, y, "last tile only, x", surface=False)
    assert exp["n"] == 17 and R.isnull(exp["pred"][:3 * TILE]).all()


# ---- special cases
def test_hand_checkable_cases(pq):
    x = np.array([1000.0, 1100.0, 1050.0, 1200.0])
    y = np.array([0.02, 0.01, -0.005, 0.03])
    got, exp = check(pq, x[None], y, "README example")
    c = got["coef"].cpu().numpy()
    assert abs(c[0] - 31 / 350000) <= 1e-12 * 31 / 350000 and abs(c[1] + 0.08257142857142857) <= 1e-12 * 0.0826
    assert abs(float(got["r_squared"]) - README_R2) <= 1e-12 * 0.2566
    x0 = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0]) * 3 + 10
    x1 = np.array([-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0]) * 2 - 6
    got, exp = check(pq, np.stack([x0, x1]), 3.0 + 2.0 * x0 - 0.5 * x1, "perfect integer fit")
    assert got["coef"].cpu().tolist() == [2.0, -0.5, 3.0] and float(got["r_squared"]) == 1.0
    assert R.isnull(got["t_stat"].cpu().numpy()).all() and R.isnull(got["p_value"].cpu().numpy()).all()
    assert bool((got["resid"] == 0.0).all())
    rng = np.random.default_rng(5)
    got, exp = check(pq, rng.standard_normal((1, 40)), np.full(40, 0.375), "constant y")
    assert got["coef"].cpu().tolist() == [0.0, 0.375] and R.isnull(got["r_squared"].cpu().numpy())


def test_no_solution_cases(pq):
    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, 64).astype(np.float64)
    y = rng.standard_normal(64)
    cases = [("collinear", np.stack([x, rng.standard_normal(64), 2.0 * x]), y), ("constant x", np.full((1, 64), 2.5), y),
             ("constant x1", np.stack([rng.standard_normal(64), np.full(64, -1.0)]), y),
             ("empty matrix", np.zeros((1, 0, 7)), np.zeros((0, 7))), ("empty rows", np.zeros((2, 5, 0)), np.zeros((5, 0)))]
    for K in (1, 3, 8):
        Xk, yk = rng.standard_normal((K, K + 4)), rng.standard_normal(K + 4)
        yk[K + 1:] = R.NULL
        cases.append((f"n = K + 1, K={K}", Xk, yk))
    for tag, X, yy in cases:
        got, exp = check(pq, X, yy, tag)
        for k in ("coef", "t_stat", "p_value", "r_squared", "pred", "resid"):
            assert R.isnull(got[k].cpu().numpy()).all(), (tag, k)
        assert int(got["n"]) == exp["n"]


def test_membership(pq):
    X, y = make(2, (50,), 11)
    X, y = X.copy(), y.copy()
    y[3], y[4], y[5] = R.NULL, np.nan, np.inf
    X[0, 10], X[1, 11], X[0, 12] = R.NULL, np.nan, -np.inf
    got, exp = check(pq, X, y, "membership")
    pred, resid = got["pred"].cpu().numpy(), got["resid"].cpu().numpy()
    assert int(got["n"]) == 44
    assert np.isfinite(pred[[3, 4, 5]]).all() and R.isnull(resid[[3, 4, 5]]).all()
    assert R.isnull(pred[[10, 11, 12]]).all() and R.isnull(resid[[10, 11, 12]]).all()


# ---- the pq.linear surface
def test_pq_linear_containers(pq):
    X, y = make(2, (300,), 41, holes=True)
    exp = R.linear(list(X), y)
    stats = ([float(exp["coef"][2]), float(exp["coef"][0]), float(exp["coef"][1])], float(exp["r2"]))
    host = {"a": X[0], "b": X[1], "ret": y, "other": np.arange(300)}
    out, (coefs, r2) = pq.linear(host, ["a", "b"], "ret", return_stats=True)          # numpy in, numpy out, a new dict
    assert list(out) == ["a", "b", "ret", "other", "pred", "resid"] and "pred" not in host and out["a"] is host["a"]
    assert isinstance(out["pred"], np.ndarray) and out["pred"].dtype == np.float64
    same("numpy pred", out["pred"], exp["pred"])
    same("numpy resid", out["resid"], exp["resid"])
    assert isinstance(coefs, list) and all(type(c) is float for c in coefs) and type(r2) is float
    assert (coefs, r2) == stats                                                       # the intercept FIRST
    dev = {k: to_dev(v) for k, v in host.items() if k != "other"}
    out = pq.linear(dev, ["a", "b"], "ret", pred_col="fit", resid_col="eps")          # device in, device out; no stats: the dict alone
    assert isinstance(out, dict) and list(out) == ["a", "b", "ret", "fit", "eps"] and out["fit"].is_cuda
    same("device pred", out["fit"].cpu().numpy(), exp["pred"])
    same("device resid", out["eps"].cpu().numpy(), exp["resid"])
    Xm, ym = make(1, (37, 50), 43, holes=True)                                        # [N, T] columns
    out = pq.linear({"x": Xm[0], "y": ym}, "x", "y")
    em = R.linear(list(Xm), ym)
    same("matrix pred", out["pred"], em["pred"])
    same("matrix resid", out["resid"], em["resid"])
    out, (coefs, r2) = pq.linear({"x": np.full(10, 1.0), "y": np.arange(10.0)}, ["x"], "y", return_stats=True)
    assert len(coefs) == 2 and all(c != c for c in coefs) and r2 != r2                # no solution: nan


def test_pq_linear_polars(pq):
    pl = pytest.importorskip("polars")
    df = pl.DataFrame({"date": ["2024-01-01", "2024-01-02", "2024-01-03", "2024-01-04", "2024-01-05"],
                       "market_cap": [1000.0, 1100.0, 1050.0, 1200.0, 1150.0], "return": [0.02, 0.01, -0.005, 0.03, None]})
    out, (coefs, r2) = pq.linear(df, x_cols=["market_cap"], y_col="return", return_stats=True)
    assert out.columns == ["date", "market_cap", "return", "pred", "resid"] and out.height == 5
    assert out["pred"].dtype == pl.Float64 and out["resid"].dtype == pl.Float64
    assert out["pred"].null_count() == 0 and out["resid"].is_null().to_list() == [False, False, False, False, True]
    assert abs(coefs[1] - 31 / 350000) <= 1e-12 * 31 / 350000 and abs(coefs[0] + 0.08257142857142857) <= 1e-12 * 0.0826
    assert abs(r2 - README_R2) <= 1e-12 * 0.2566
    assert out["pred"][4] == coefs[0] + coefs[1] * 1150.0
    out2 = pq.linear(df, ["market_cap"], "return", resid_col="market_neutral_return")
    assert out2.columns[-2:] == ["pred", "market_neutral_return"]


def test_pq_linear_pyarrow(pq):
    pa = pytest.importorskip("pyarrow")
    tab = pa.table({"market_cap": [1000.0, 1100.0, 1050.0, 1200.0, 1150.0, None], "return": [0.02, 0.01, -0.005, 0.03, None, 0.5],
                    "date": ["a", "b", "c", "d", "e", "f"]})
    out, (coefs, r2) = pq.linear(tab, ["market_cap"], "return", pred_col="fit", return_stats=True)
    assert out.column_names == ["market_cap", "return", "date", "fit", "resid"] and out.num_rows == 6
    assert out.column("fit").type == pa.float64() and out.column("resid").type == pa.float64()
    assert out.column("fit").is_null().to_pylist() == [False] * 5 + [True]                   # a null x: no prediction
    assert out.column("resid").is_null().to_pylist() == [False] * 4 + [True, True]           # a null y or x: no residual
    assert abs(coefs[1] - 31 / 350000) <= 1e-12 * 31 / 350000 and abs(coefs[0] + 0.08257142857142857) <= 1e-12 * 0.0826
    assert abs(r2 - README_R2) <= 1e-12 * 0.2566
    assert out.column("fit")[4].as_py() == coefs[0] + coefs[1] * 1150.0


# ---- ABI refusals
def test_abi_refusals(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    L, h, vp = lib(), api.ctx(), C.c_void_p
    M = 100
    X, y = make(1, (M,), 3)
    dx, dy = to_dev(X[0]), to_dev(y)
    f64 = dict(dtype=torch.float64, device="cuda")
    stat = torch.full((4, 16), 7.0, **f64)
    nn = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    cols = torch.full((2, M), 7.0, **f64)
    ptrs = (vp * 9)(*[dx.data_ptr()] * 9)

    def call(bb, k):
        ok(L.pq_linear(h, C.byref(bb), ptrs, C.c_int32(k), vp(dy.data_ptr()), vp(stat[0].data_ptr()), vp(stat[1].data_ptr()),
                       vp(stat[2].data_ptr()), vp(stat[3].data_ptr()), vp(nn.data_ptr()), vp(cols[0].data_ptr()), vp(cols[1].data_ptr())))

    b = Batch(1, M, M)
    for k in (0, 9):
        with pytest.raises(pq.PqError, match="k must be") as e:
            call(b, k)
        assert "pq status 1:" in str(e.value)                         # PQ_ERR_ARG
        assert b"k must be" in L.pq_last_error()
    ok(L.pq_suite_begin(h, C.byref(b)))
    try:
        with pytest.raises(pq.PqError, match="recorded") as e:
            call(b, 1)
        assert "pq status 5:" in str(e.value)                         # PQ_ERR_UNSUPPORTED
        assert b"recorded" in L.pq_last_error()
    finally:
        ok(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, M], dtype=torch.int64, device="cuda")
    rb = Batch(3, M - 25, M, vp(off.data_ptr()))
    with pytest.raises(pq.PqError, match="ragged") as e:
        call(rb, 1)
    assert "pq status 5:" in str(e.value)
    assert b"ragged" in L.pq_last_error()
    torch.cuda.synchronize()
    assert bool((stat == 7.0).all()) and int(nn) == 7 and bool((cols == 7.0).all()), "a refused call wrote"
    call(b, 1)                                                        # the context computes again after the refusals
    torch.cuda.synchronize()
    exp = R.linear(list(X), y)
    same("coef after refusals", stat[0, :2].cpu().numpy(), exp["coef"])
    same("pred after refusals", cols[0].cpu().numpy(), exp["pred"])
    assert int(nn) == M
