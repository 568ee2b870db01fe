"""-m gpu: the rolling technical factors moving_average / momentum / volatility / skewness / relative_strength (D-21,
csrc/xsec/rolling.hip) against the numpy restatement in tests/xsec_rolling_ref.py.  Every comparison is bitwise on the uint64 view: D-21
stores every NaN result as NULL, so no cell is left to the hardware's NaN bits.

Before the GPU is compared, every (op, window) case is checked on the restatement's output: at least half of the rows beyond the
warm-up are non-NULL, and in the `special` inputs at least one of them is NULL -- so no case passes on a column of NULLs alone."""
import ctypes as C

import numpy as np
import pytest

import xsec_rolling_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 256                    # days per workgroup of the windowed kernel (RL_TILE)
GRID_CAP = 1 << 20            # workgroups per launch; above it the kernels walk their (symbol, tile) jobs with a grid stride
CODES = {"mean": 0, "momentum": 1, "volatility": 2, "skewness": 3, "relative_strength": 4}


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


def make(kind, n, T, w, seed, sprinkle=True):
    """`plain`: the positive random walk exp(cumsum(0.02 N(0, 1))) without an invalid cell.  `special`: NULL / NaN / +inf / -inf / 0.0
    cells at a combined rate of 1 / (4 (w + 1)), a NULL on the first day of symbol 0 (the first full window of every op holds it), one
    constant stretch of w + 2 days, and single NULLs on the last day of a tile, the first day of the next and the far edge of its halo.
    sprinkle=False (series of a few days, where a chance cell more would leave no majority of full samples): the NULL on the first day
    of symbol 0 and a zero price on the last day of symbol 1 only"""
    rng = np.random.default_rng(seed)
    x = np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))
    if kind == "special" and n and T:
        u = rng.random((n, T)) * (4.0 * (w + 1))
        for k, v in enumerate((R.NULL, np.nan, np.inf, -np.inf, 0.0)):
            if sprinkle:
                x[(u >= k * 0.2) & (u < (k + 1) * 0.2)] = v
        x[0, 0] = R.NULL
        if not sprinkle and n > 1:
            x[1, T - 1] = 0.0
        if T >= 8 * (w + 2):
            x[n - 1, T // 2:T // 2 + w + 2] = 1.25
        if T > TILE + w and n > 1:
            x[1, [TILE - 1, TILE, TILE + w]] = R.NULL
    return x


def cases_for(windows, skips=(0,)):
    out = []
    for op in R.OPS:
        for w in windows:
            if w < R.MIN_WINDOW[op]:
                continue
            out += [(op, w, s) for s in (skips if op == "momentum" else (0,))]
    return out


class BadInput(AssertionError):
    pass


def reference(x, kind, cases):
    """the restatement of every case, after the condition on the input that makes the case worth comparing"""
    exp = {}
    for op, w, skip in cases:
        e = R.rolling(x, op, w, skip)
        warm = w - 1 if op == "mean" else w + skip
        beyond = R.isnull(e[:, warm:])
        if beyond.size:
            if 2 * int((~beyond).sum()) < beyond.size:
                raise BadInput(f"badly chosen input: {op} w={w} skip={skip} {x.shape} {kind} is mostly NULL")
            if kind == "special" and not beyond.any():
                raise BadInput(f"badly chosen input: {op} w={w} skip={skip} {x.shape} has no NULL beyond the warm-up")
        assert R.isnull(e[:, :warm]).all()
        exp[op, w, skip] = e
    return exp


def make_for(kind, n, T, w, seed, cases, **kw):
    """an input that meets the condition for every case, and its references.  With five symbols and a window of hundreds of days a
    single sprinkled cell empties a third of a symbol's rows, so whether half of the rows keep their sample is up to the draw: the draw
    is repeated (on the restatement's output alone, before the GPU is asked) until it does"""
    err = None
    for k in range(32):
        x = make(kind, n, T, w, seed + 7919 * k, **kw)
        try:
            return x, reference(x, kind, cases)
        except BadInput as e:
            err = e
    raise err


def call(pq, xd, op, w, skip=0):
    F = pq.Factor()
    if op == "momentum":
        return F.momentum(xd, w, skip)
    return getattr(F, {"mean": "moving_average"}.get(op, op))(xd, w)


def to_dev(a, pitch=None):
    n, T = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if pitch is None:
        return t.cuda()
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = t.cuda()
    return buf[:, :T]


def check(pq, x, kind, cases, xd=None, tag="", exp=None):
    exp = reference(x, kind, cases) if exp is None else exp
    xd = to_dev(x) if xd is None else xd
    got = None
    for op, w, skip in cases:
        got = call(pq, xd, op, w, skip)
        same(f"{op} w={w} skip={skip} {x.shape} {kind} {tag}", got.cpu().numpy(), exp[op, w, skip])
    return got


SHAPES = [((1, 1), "plain"), ((1, 5), "plain"), ((37, 50), "plain"), ((37, 50), "special"), ((300, 131), "plain"), ((300, 131), "special")]


@pytest.mark.parametrize("shape, kind", SHAPES, ids=[f"{n}x{t}-{k}" for (n, t), k in SHAPES])
def test_every_op_bitwise(pq, shape, kind):
    """each op's minimum window, 2, 3 and 20 (longer than the series on the short shapes: all NULL), momentum with skip 0, 1, 21 and
    with skip + window >= T.  The one- and five-day series have no room for an invalid cell beside a majority of full samples; with
    invalid cells they are test_series_as_long_as_the_window's."""
    n, T = shape
    for w in (1, 2, 3, 20):
        x = make(kind, n, T, w, 100 * w + n + T)
        check(pq, x, kind, cases_for((w,), skips=(0, 1, 21, max(T - w, 0), T + 5)))


@pytest.mark.parametrize("w", [2, 3, 20])
def test_series_as_long_as_the_window(pq, w):
    """T = w, w + 1, w + 2: no full sample, the first one, the first two"""
    for T in (w, w + 1, w + 2):
        for kind in ("plain", "special"):
            check(pq, make(kind, 3, T, w, 7 * w + T, sprinkle=False), kind, cases_for((w,), skips=(0, 1)))


@pytest.mark.parametrize("T", [255, 256, 257, 515, 1023, 1024, 1025, 2051])
def test_day_tiles(pq, T):
    """the 256-day tiles around their edges (tile - 1, tile, tile + 1, 2 tile + 3 and the long series), windows shorter than, equal to
    and longer than a tile, with NULLs on the last day of a tile, the first day of the next and the far edge of its halo"""
    windows = [20] + ([255, 256, 257] if T >= 1023 else []) + ([1024] if T == 2051 else [])
    for w in windows:
        for kind in ("plain", "special"):
            cases = cases_for((w,), skips=(0, 21))
            x, exp = make_for(kind, 5, T, w, T + w, cases)
            check(pq, x, kind, cases, exp=exp)


def test_window_longer_than_the_series(pq):
    """the longest window with one full sample (the last day), one day more (all NULL), and the cap"""
    x = make("plain", 5, 300, 20, 3)
    xd = to_dev(x)
    for op in R.OPS:
        for w, last_day in ((300 if op == "mean" else 299, True), (301, False), (1024, False)):
            got = call(pq, xd, op, w).cpu().numpy()
            same(f"{op} w={w}", got, R.rolling(x, op, w))
            assert R.isnull(got[:, :-1]).all() and (~R.isnull(got[:, -1])).all() == last_day and R.isnull(got[:, -1]).all() != last_day


def test_more_jobs_than_the_grid(pq):
    """more (symbol, tile) jobs than the launch has workgroups: the grid stride restages the LDS tile"""
    n, T = GRID_CAP + 3, 3
    x = make("plain", n, T, 2, 5)
    x[n - 2, 1] = R.NULL
    xd = to_dev(x)
    for op, w in (("mean", 2), ("momentum", 1), ("volatility", 2), ("relative_strength", 1), ("relative_strength", 2)):
        same(f"{op} w={w} {n} symbols", call(pq, xd, op, w).cpu().numpy(), R.rolling(x, op, w))


@pytest.mark.parametrize("pitch", [51, 64])
def test_row_pitch(pq, pitch):
    """batch stride > len, odd and a multiple of 16 elements: the input read and the output written at the input's pitch"""
    x = make("special", 37, 50, 3, pitch)
    got = check(pq, x, "special", cases_for((3,), skips=(0, 1)), to_dev(x, pitch), tag=f"pitch {pitch}")
    assert got.stride(0) == pitch


def test_caller_owned_out_keeps_its_padding(pq):
    """through the C ABI, out prefilled with a sentinel: columns [T, pitch) are never written"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    L, h, vp = lib(), api.ctx(), C.c_void_p
    n, T, pitch = 37, 300, 304
    x = make("special", n, T, 20, 11)
    xd = to_dev(x, pitch)
    b = Batch(n, T, pitch)
    for op, w, skip in cases_for((20,), skips=(3,)):
        out = torch.full((n, pitch), -77.0, dtype=torch.float64, device="cuda")
        ok(L.pq_factor_rolling(h, C.byref(b), vp(xd.data_ptr()), C.c_int32(CODES[op]), C.c_int64(w), C.c_int64(skip), vp(out.data_ptr())))
        same(f"{op} into a caller's column", out[:, :T].cpu().numpy(), R.rolling(x, op, w, skip))
        assert bool((out[:, T:] == -77.0).all()), f"{op} wrote into the row padding"


def test_refusals_launch_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    L, h, vp = lib(), api.ctx(), C.c_void_p
    n, T = 40, 30
    x = make("plain", n + 1, T, 5, 1)
    buf = to_dev(x)                                   # n + 1 rows: x = rows 0 .. n-1, the shifted out = rows 1 .. n
    keep = buf.clone()
    out = torch.full((n, T), 7.0, dtype=torch.float64, device="cuda")
    b = Batch(n, T, T)
    xp, op_ = buf.data_ptr(), out.data_ptr()

    def roll(bb, code, w, skip=0, src=xp, dst=op_):
        ok(L.pq_factor_rolling(h, C.byref(bb), vp(src), C.c_int32(code), C.c_int64(w), C.c_int64(skip), vp(dst)))

    for args, msg in (((5, 5), "op"), ((-1, 5), "op"), ((0, 0), "window"), ((0, 1025), "window"), ((2, 1), "window"), ((3, 2), "window"),
                      ((1, 5, -1), "skip"), ((0, 5, 1), "skip"), ((4, 5, 2), "skip")):
        with pytest.raises(pq.PqError, match=msg) as e:
            roll(b, *args)
        assert "pq status 1:" in str(e.value)                         # PQ_ERR_ARG
    for code in range(5):
        for dst in (xp, xp + T * 8, xp + 8):                          # out == x, x shifted by one row, by one cell
            with pytest.raises(pq.PqError, match="overlap") as e:
                roll(b, code, 5, dst=dst)
            assert "pq status 1:" in str(e.value)
    ok(L.pq_suite_begin(h, C.byref(b)))
    try:
        for code in range(5):
            with pytest.raises(pq.PqError, match="recorded") as e:
                roll(b, code, 5)
            assert "pq status 5:" in str(e.value)                     # PQ_ERR_UNSUPPORTED
    finally:
        ok(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    for code in range(5):
        with pytest.raises(pq.PqError, match="ragged") as e:
            roll(rb, code, 5)
        assert "pq status 5:" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == keep).all()), "a refused call wrote"
    check(pq, x, "plain", cases_for((5,)))                            # the context computes again after the refusals


def test_empty_batches(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    for shape in ((0, 5), (4, 0)):
        z = torch.empty(shape, dtype=torch.float64, device="cuda")
        for op in R.OPS:
            out = call(pq, z, op, 3)
            assert tuple(out.shape) == shape and out.dtype == torch.float64
        b = Batch(shape[0], shape[1], shape[1])
        ok(lib().pq_factor_rolling(api.ctx(), C.byref(b), None, C.c_int32(2), C.c_int64(3), C.c_int64(0), None))   # PQ_OK, nothing launched


@pytest.mark.parametrize("w", [1, 5, 20])
def test_momentum_is_returns_on_the_device(pq, w):
    """Factor.momentum(x, w) is pq.returns(x, period=w) bit for bit wherever that is not NaN -- zero bases (+-inf) included.  The one
    difference is D-21's `valid`: over a finite base an infinite x[t] gives returns +-inf, and momentum NULL"""
    x = make("special", 300, 131, w, 40 + w)
    xd = to_dev(x)
    mom = pq.Factor().momentum(xd, w).cpu().numpy()
    ret = pq.returns(xd, period=w).cpu().numpy()
    num, fin = ~np.isnan(ret), np.isfinite(x)
    assert num.sum() > x.size // 2 and np.isinf(ret[num & fin]).any() and (num & ~fin).any()
    same("momentum against returns", mom[num & fin], ret[num & fin])
    assert R.isnull(mom[num & ~fin]).all()
    same("momentum against the restatement", mom, R.momentum(x, w))


def test_output_feeds_the_evaluation_half(pq):
    """the column stays on the device: Factor.ic on it equals Factor.ic on a copy that went through the host"""
    x = make("special", 300, 131, 5, 9)
    xd = to_dev(x)
    F = pq.Factor()
    mom = F.momentum(xd, 5)
    vol = F.volatility(xd, 5)
    assert mom.is_cuda and vol.is_cuda and mom.dtype == torch.float64
    fwd = F.momentum(xd, 1)
    for name, col in (("momentum", mom), ("volatility", vol)):
        ic, nv = F.ic(col, fwd)
        ic2, nv2 = F.ic(col.cpu().numpy(), fwd.cpu().numpy())
        same(f"ic of {name}", ic.cpu().numpy(), ic2.cpu().numpy())
        assert bool((nv == nv2).all()) and int(nv.max()) > 150
