"""-m gpu: the rolling-window OLS (D-28, csrc/xsec/rolling_regress.hip) against the numpy restatement in
tests/xsec_rolling_regress_ref.py.  Every comparison is bitwise on the uint64 view: D-28 stores NULL wherever a row has no result, so no
cell is left to the hardware's NaN bits.

Before the GPU is asked, every case of the parity grid is checked on the restatement's output: at least a quarter of the rows beyond
the warm-up are non-NULL, so no case passes on columns of NULLs alone."""
import ctypes as C

import numpy as np
import pytest

import xsec_regress_ref as G
import xsec_rolling_regress_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 256                    # days per workgroup (RR_TILE)
GRID_CAP = 1 << 20            # workgroups per launch; above it the kernel walks its (symbol, tile) jobs with a grid stride
NULL = R.NULL


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def same(name, got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def same_all(name, got, exp, outputs=R.OUTPUTS):
    assert sorted(got) == sorted(outputs), (name, sorted(got))
    for k in outputs:
        same(f"{name} {k}", got[k].cpu().numpy(), exp[k])


def make(n, T, K, seed, series=()):
    """-> (y [n, T], xs): independent N(0, 1) regressors ([T] for the indices in `series`), y = 0.3 + sum_j (j + 1) x_j / 2 + 0.5 N(0, 1)"""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(T) if j in series else rng.standard_normal((n, T)) for j in range(K)]
    y = 0.3 + 0.5 * rng.standard_normal((n, T))
    for j, x in enumerate(xs):
        y = y + 0.5 * (j + 1) * np.broadcast_to(x, (n, T))
    return y, xs


def to_dev(a, pitch=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if a.ndim == 1 or pitch is None:
        return t.cuda()
    n, T = a.shape
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = t.cuda()
    return buf[:, :T]


def run(y, xs, w, pitch=None, outputs=R.OUTPUTS):
    from polars_quant_amd import api
    return api.factor_rolling_regress(to_dev(y, pitch), [to_dev(x, pitch) for x in xs], w, outputs=outputs)


def enough_rows(exp, w, name):
    """the condition on the input that makes the case worth comparing, on the restatement's output alone"""
    assert all(R.isnull(exp[k][..., :w - 1]).all() for k in R.OUTPUTS)
    beyond = ~R.isnull(exp["alpha"][:, w - 1:])
    assert beyond.size and 4 * int(beyond.sum()) >= beyond.size, f"badly chosen input: {name} is mostly NULL"
    assert (~R.isnull(exp["beta"][:, :, w - 1:])).all(axis=0).sum() == beyond.sum()


# ---------------------------------------------------------------- the parity grid
WINDOWS = ("min", 20, 257, 1024)
FORMS = [(1, ()), (1, (0,)), (2, (1,)), (3, (0,)), (4, (1, 3))]          # (K, which regressors are [T] series)


@pytest.mark.parametrize("K, series", FORMS, ids=[f"K{k}-series{''.join(map(str, s)) or 'none'}" for k, s in FORMS])
@pytest.mark.parametrize("window", WINDOWS)
def test_parity_grid(pq, K, series, window):
    """N = 5.  Short windows (K + 2 and 20) on T = 257, one full tile and one row, with isolated invalid cells in different columns at
    days 0, 255, 256 = T - 1; window 257 on T = 773 (the halo is longer than a tile) and 1024 on T = 1283, with at most one invalid
    cell per symbol (day 0 of symbol 0, a late day of symbol 1) and three clean symbols.  Each at the odd row pitch T and a padded one."""
    w = K + 2 if window == "min" else window
    n, T = 5, {257: 773, 1024: 1283}.get(w, 257)
    y, xs = make(n, T, K, 1000 * K + w + len(series), series)
    cols = [xs[j] for j in range(K) if j not in series] + [y]     # the [n, T] columns
    if w <= 20:
        y[0, 0] = np.nan
        cols[0][1, 255] = NULL
        y[2, 256] = np.nan
        cols[len(cols) // 2][3, T - 1] = np.nan
        if series:
            xs[series[0]][255] = np.nan                 # a series' cell is every symbol's
    else:
        y[0, 0] = np.nan
        cols[0][1, T - 10] = NULL
    exp = R.rolling_regress(y, xs, w)
    name = f"K={K} series={series} w={w} T={T}"
    enough_rows(exp, w, name)
    assert R.isnull(exp["alpha"][:, w - 1:]).any()
    for pitch in (T, T + 16 - T % 16):
        got = run(y, xs, w, pitch)
        same_all(f"{name} pitch={pitch}", got, exp)
        assert got["alpha"].stride(0) == pitch and got["beta"].stride(1) == pitch


# ---------------------------------------------------------------- further cases
@pytest.mark.parametrize("T", [255, 256, 512, 513])
def test_day_tiles(pq, T):
    y, xs = make(5, T, 1, T)
    xs[0][1, [min(TILE, T) - 1, T - 1]] = NULL            # the last day of the first tile and of the series
    exp = R.rolling_regress(y, xs, 20)
    enough_rows(exp, 20, f"T={T}")
    same_all(f"T={T}", run(y, xs, 20), exp)


def test_series_as_long_as_the_window(pq):
    """T < window: all NULL; T == window: one row"""
    for K, series in ((1, ()), (3, (1,))):
        w = 24
        for T, rows in ((w - 1, 0), (w, 1), (w + 1, 2)):
            y, xs = make(4, T, K, 10 * K + T, series)
            exp = R.rolling_regress(y, xs, w)
            assert int((~R.isnull(exp["alpha"])).sum()) == 4 * rows and not R.isnull(exp["alpha"][:, w - 1:]).any()
            same_all(f"K={K} T={T} w={w}", run(y, xs, w), exp)
    y, xs = make(3, 5, 1, 5)
    exp = R.rolling_regress(y, xs, 1024)
    assert R.isnull(exp["resid"]).all()
    same_all("T=5 w=1024", run(y, xs, 1024), exp)


def test_singular_constant_and_infinite_cells(pq):
    """a constant regressor (singular: every output NULL), a constant return (Syy == 0: R^2 alone NULL), +inf and -inf entries
    (unusable, like NaN), two collinear regressors, and deviations whose products overflow (a NaN result: the row NULL)"""
    n, T, w = 7, 300, 20
    y, xs = make(n, T, 2, 77, series=(1,))
    xs[0][0, 40:80] = 1.25                      # rows 59 .. 79 of symbol 0 see a constant x_0
    y[1, 100:160] = -2.5                        # rows 119 .. 159 of symbol 1 see a constant y
    xs[0][2, 200] = np.inf
    y[3, 256] = -np.inf
    xs[0][4] = 3.0 * xs[1] - 1.0                # collinear with the series wherever that is exact enough; singular or not, the same bits
    xs[0][5] = xs[0][5] * 1e200
    y[5] = y[5] * 1e200
    exp = R.rolling_regress(y, xs, w)
    for k in R.OUTPUTS:
        assert R.isnull(exp[k][..., 0, 59:80]).all() and R.isnull(exp[k][..., 2, 200:220]).all() and R.isnull(exp[k][..., 3, 256:276]).all()
        assert R.isnull(exp[k][..., 5, :]).all()
        assert not R.isnull(exp[k][..., 6, w - 1:]).any()
    assert R.isnull(exp["r_squared"][1, 119:160]).all() and (exp["beta"][0, 1, 119:160] == 0.0).all()
    assert not R.isnull(exp["alpha"][1, 119:160]).any()
    same_all("special cells", run(y, xs, w), exp)
    same_all("special cells, padded", run(y, xs, w, 304), exp)


def test_output_subsets(pq):
    """each single output alone, and all five, give the same bits; an output that is not requested is not allocated"""
    y, xs = make(5, 300, 3, 9, series=(2,))
    y[0, 17] = np.nan
    exp = R.rolling_regress(y, xs, 30)
    same_all("all five", run(y, xs, 30), exp)
    for k in R.OUTPUTS:
        same_all(f"{k} alone", run(y, xs, 30, outputs=(k,)), exp, (k,))
    same_all("two", run(y, xs, 30, outputs=("resid", "beta")), exp, ("beta", "resid"))
    same_all("a name, not a tuple", run(y, xs, 30, outputs="alpha"), exp, ("alpha",))


def raw(L, h, b, xs, mask, y, w, outs):
    """pq_factor_rolling_regress on device tensors (None: a NULL pointer) -> its status"""
    vp = C.c_void_p

    def ptr(t):
        return None if t is None else vp(t.data_ptr())
    arr = (vp * max(len(xs), 1))(*[x.data_ptr() for x in xs])
    return L.pq_factor_rolling_regress(h, C.byref(b), arr, C.c_int32(len(xs)), C.c_uint32(mask), ptr(y), C.c_int64(w), *[ptr(o) for o in outs])


def test_null_pointers_leave_buffers_alone(pq):
    """through the C ABI: an output whose pointer is NULL is not written -- its buffer keeps the sentinel --, and no written output
    touches its row padding"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    L, h = lib(), api.ctx()
    n, T, pitch, w = 6, 300, 304, 20
    y, xs = make(n, T, 2, 31, series=(0,))
    y[2, 100] = NULL
    exp = R.rolling_regress(y, xs, w)
    yd, xd = to_dev(y, pitch), [to_dev(x, pitch) for x in xs]
    b = Batch(n, T, pitch)
    for keep in ((0,), (1, 3), (2, 4), (0, 1, 2, 3, 4)):
        bufs = [torch.full((2, n, pitch) if k == 0 else (n, pitch), -77.0, dtype=torch.float64, device="cuda") for k in range(5)]
        ok(raw(L, h, b, xd, 0b01, yd, w, [bufs[k] if k in keep else None for k in range(5)]))
        torch.cuda.synchronize()
        for k, name in enumerate(R.OUTPUTS):
            if k in keep:
                same(f"{name} of {keep}", bufs[k][..., :T].cpu().numpy(), exp[name])
                assert bool((bufs[k][..., T:] == -77.0).all()), f"{name} wrote into the row padding"
            else:
                assert bool((bufs[k] == -77.0).all()), f"{name} was written though its pointer was NULL"


def test_more_jobs_than_the_grid(pq):
    """more (symbol, tile) jobs than the launch has workgroups: the grid stride restages the LDS tile"""
    n, T, w = GRID_CAP + 3, 4, 3
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((n, T)), rng.standard_normal((n, T))
    x[n - 2, 1] = NULL
    y[3, 0] = np.nan
    got = run(y, [x], w)
    for part in (slice(0, 1000), slice(n - 1000, n)):
        exp = R.rolling_regress(y[part], [x[part]], w)
        assert 4 * int((~R.isnull(exp["alpha"][:, w - 1:])).sum()) >= exp["alpha"][:, w - 1:].size
        same_all(f"symbols {part}", {k: v[..., part, :] for k, v in got.items()}, exp)


def test_refusals_launch_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    n, T, w = 40, 30, 5
    y, xs = make(n + 1, T, 2, 1, series=(1,))
    # every pointer of a refused call lies inside a buffer of this test, with room for the column it stands for
    cells = n * T
    yd, x0 = to_dev(y), to_dev(xs[0])                         # n + 1 rows: the columns of the batch are rows 0 .. n-1
    pool = torch.full((cells + T,), 7.0, dtype=torch.float64, device="cuda")
    x1 = pool[cells - 1:cells - 1 + T]                        # the series: its first cell is the last of a column at pool[0]
    x1.copy_(to_dev(xs[1]))
    pool2 = torch.full((3 * cells,), 7.0, dtype=torch.float64, device="cuda")     # beta [2][n][T], and alpha from beta's last cell on
    keep, keep_pool = yd.clone(), pool.clone()
    outs = [torch.full((2, n, T) if k == 0 else (n, T), 7.0, dtype=torch.float64, device="cuda") for k in range(5)]
    b = Batch(n, T, T)

    def status(bb=b, xs_=(x0, x1), mask=0b10, y_=yd, w_=w, outs_=outs):
        r = raw(L, h, bb, list(xs_), mask, y_, w_, outs_)
        return r, L.pq_last_error().decode()

    yflat = yd.reshape(-1)
    bad = [
        (dict(outs_=[outs[0], yd, None, None, None]), "overlap an input"),                     # alpha == y
        (dict(outs_=[None, None, yflat[T:], None, None]), "overlap an input"),                 # resid_std = y shifted by one row
        (dict(outs_=[None, None, None, yflat[1:], None]), "overlap an input"),                 # r_squared = y shifted by one cell
        (dict(outs_=[None, x0, None, None, None]), "overlap an input"),                        # alpha == x_0
        (dict(outs_=[outs[0], None, None, None, pool]), "overlap an input"),                   # the last cell of resid is the series' first
        (dict(outs_=[outs[0], outs[1], outs[1], None, None]), "two outputs"),                  # the same column twice
        (dict(outs_=[pool2, pool2[2 * cells - 1:], None, None, None]), "two outputs"),         # alpha starts in beta's last cell
        (dict(w_=3), "window"),                                                                # K + 1
        (dict(w_=1025), "window"),
        (dict(xs_=()), "n_x"),
        (dict(xs_=(x0,) * 5, mask=0), "n_x"),
        (dict(mask=0b100), "series_mask"),
    ]
    for kw, msg in bad:
        r, err = status(**kw)
        assert r == 1 and msg in err, (kw.keys(), r, err)                                      # PQ_ERR_ARG
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    r, err = status(bb=Batch(3, n * T - 25, n * T, C.c_void_p(off.data_ptr())))
    assert r == 1 and "ragged" in err, (r, err)
    assert L.pq_suite_begin(h, C.byref(b)) == 0
    try:
        r, err = status()
        assert r == 5 and "recorded" in err, (r, err)                                          # PQ_ERR_UNSUPPORTED
    finally:
        assert L.pq_suite_abort(h) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs + [pool2]) and bool((yd == keep).all()) and bool((pool == keep_pool).all()), \
        "a refused call wrote"
    r, err = status()                                                                          # the context computes again
    assert r == 0, err
    exp = R.rolling_regress(y[:n], [xs[0][:n], xs[1]], w)
    for k, name in enumerate(R.OUTPUTS):
        same(name, outs[k].cpu().numpy(), exp[name])


def test_empty_batches(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    for shape in ((0, 5), (4, 0)):
        b = Batch(shape[0], shape[1], shape[1])
        assert L.pq_factor_rolling_regress(h, C.byref(b), None, C.c_int32(1), C.c_uint32(0), None, C.c_int64(3), None, None, None, None,
                                           None) == 0                                           # PQ_OK, nothing launched
        z = torch.empty(shape, dtype=torch.float64, device="cuda")
        out = api.factor_rolling_regress(z, [z, z], 4)
        assert tuple(out["beta"].shape) == (2,) + shape and all(tuple(out[k].shape) == shape for k in R.OUTPUTS[1:])


def test_the_factor_methods_are_the_call(pq):
    from polars_quant_amd import api
    y, xs = make(5, 300, 2, 12, series=(0,))
    y[1, 33] = np.nan
    yd, xd = to_dev(y), [to_dev(x) for x in xs]
    F = pq.Factor()
    exp = R.rolling_regress(y, xs[:1], 60)
    beta = F.rolling_beta(yd, xd[0])
    same("rolling_beta", beta.cpu().numpy(), api.factor_rolling_regress(yd, xd[:1], 60)["beta"][0].cpu().numpy())
    same("rolling_beta against the restatement", beta.cpu().numpy(), exp["beta"][0])
    exp = R.rolling_regress(y, xs, 60)
    ivol = F.idiosyncratic_volatility(yd, xd)
    same("idiosyncratic_volatility", ivol.cpu().numpy(), api.factor_rolling_regress(yd, xd, 60)["resid_std"].cpu().numpy())
    same("idiosyncratic_volatility against the restatement", ivol.cpu().numpy(), exp["resid_std"])
    same_all("rolling_regression", F.rolling_regression(yd, xd), exp)
    assert beta.is_cuda and ivol.is_cuda and tuple(beta.shape) == tuple(ivol.shape) == (5, 300)


def test_the_whole_history_is_the_time_series_regression(pq):
    """T = 200 = window: the last column is api.ts_regress's coef and r_squared on the same data, bit for bit"""
    from polars_quant_amd import api
    n, T = 6, 200
    y, xs = make(n, T, 3, 200, series=(1,))
    y[0] = 1.5                                  # Syy == 0
    xs[0][1] = 2.0                              # singular
    yd, xd = to_dev(y), [to_dev(x) for x in xs]
    got = api.factor_rolling_regress(yd, xd, T)
    ts = api.ts_regress(xd, yd)
    coef, r2 = ts["coef"].cpu().numpy(), ts["r_squared"].cpu().numpy()
    assert R.isnull(r2[0]) and R.isnull(coef[1]).all() and not R.isnull(coef[2:]).any() and not R.isnull(r2[2:]).any()
    same("beta", got["beta"][:, :, -1].cpu().numpy().T, coef[:, :3])
    same("alpha", got["alpha"][:, -1].cpu().numpy(), coef[:, 3])
    same("r_squared", got["r_squared"][:, -1].cpu().numpy(), r2)
    same("against D-17's restatement", coef, G.ts_regress(xs, y)["coef"])
