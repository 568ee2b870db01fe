"""-m gpu: the time-series operators ts_sum / ts_std / ts_zscore / ts_min / ts_max / ts_argmin / ts_argmax / ts_rank / decay_linear /
delay / delta and ts_cov / ts_corr (D-29, csrc/xsec/tsops.hip) against the numpy restatement in tests/xsec_ts_ref.py.  Every comparison
is bitwise on the uint64 view: D-29 stores every NaN result as NULL, so no cell is left to the hardware's NaN bits, and the device uses
the function set that makes the restatement exact on the host (IEEE add, mul, div, sqrt; integer counts).

Before the GPU is compared, every (op, window) case is checked on the restatement's output: at least half of the rows beyond the
warm-up are non-NULL, in the `special` inputs at least one of them is NULL, and for the ordering ops (rank, argmin, argmax) at least one
non-NULL row has a tie -- so no case passes on a column of NULLs or on tie-free data alone."""
import ctypes as C

import numpy as np
import pytest

import xsec_build_ref as B
import xsec_rolling_ref as RL
import xsec_ts_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 256                    # days per workgroup of the windowed kernels (TS_TILE)
GRID_CAP = 1 << 20            # workgroups per launch; above it the kernels walk their (symbol, tile) jobs with a grid stride
CODES = {op: k for k, op in enumerate(R.OPS)}
PAIR_CODES = {op: k for k, op in enumerate(R.PAIR_OPS)}
CORE = ("sum", "rank", "argmax", "decay_linear", "corr")
LAGS = ("delay", "delta")


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


def walk(rng, n, T):
    return np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))


def make(kind, n, T, w, seed, sprinkle=True, ties=True):
    """-> (x, y).  `plain`: two positive random walks exp(cumsum(0.02 N(0, 1))) without an invalid cell.  `special`: in each column
    NULL / NaN / +inf / -inf / 0.0 cells at a combined rate of 1 / (4 (w + 1)), in x a NULL on the first day of symbol 0 (the first full
    window of every op holds it), one constant stretch of w + 2 days (another one in y), and single NULLs on the last day of a tile, the
    first day of the next and the far edge of its halo (in y one day inside each of them, on the same symbol: at the longest windows a
    symbol with one such cell has no full window left).  sprinkle=False (series of a few days, where a chance
    cell more would leave no majority of full samples): the NULL on the first day of symbol 0 and a zero on the last day of symbol 1
    only.  ties (both kinds, x only): a stretch of one repeated value above the walk (equal maxima; today's value met again in its
    window) and a +0 / -0 pair below it (equal minima that differ in their bits; on another symbol where the series has few days)"""
    rng = np.random.default_rng(seed)
    x, y = walk(rng, n, T), walk(rng, n, T)
    if kind == "special" and n and T:
        for col in (x, y):
            u = rng.random((n, T)) * (4.0 * (w + 1))
            for k, v in enumerate((R.NULL, np.nan, np.inf, -np.inf, 0.0)):
                if sprinkle:
                    col[(u >= k * 0.2) & (u < (k + 1) * 0.2)] = v
        x[0, 0] = R.NULL
        if not sprinkle and n > 1:
            x[1, T - 1] = 0.0
        if T >= 8 * (w + 2):
            x[n - 1, T // 2:T // 2 + w + 2] = 1.25
            y[0, T // 4:T // 4 + w + 2] = 0.75
        if T > TILE + w and n > 1:
            x[1, [TILE - 1, TILE, TILE + w]] = R.NULL
            y[1, [TILE - 2, TILE + 1, TILE + w - 1]] = R.NULL
    if ties and n and T >= 2:
        s, few = min(2, n - 1), T < max(16, w + 8)              # few days: the pair ends the series, so that a full window holds it
        a = 0 if few else T - 8
        x[s, a:a + (2 if few else 3)] = 3.0
        z = s if not few or n < 4 else 3
        b = a + 4 if not few else (T - 2 if T >= 4 or z != s else None)
        if b is not None:
            x[z, b], x[z, b + 1] = 0.0, -0.0
    return x, y


def cases_for(windows, ops=R.PAIR_OPS + R.OPS):
    """(op, window, mode): rank in both modes; the pair ops first, whose sample is the hardest to draw"""
    out = []
    for op in ops:
        for w in windows:
            if w >= R.MIN_WINDOW[op]:
                out += [(op, w, m) for m in ((0, 1) if op == "rank" else (0,))]
    return out


class BadInput(AssertionError):
    pass


def has_tie(x, e, op, w):
    """is there a non-NULL row whose window holds its extreme twice (arg*), or today's value twice (rank)"""
    v = np.where(R.valid(x), x, 0.0)
    ref = v if op == "rank" else R.ts(x, "min" if op == "argmin" else "max", w)
    cnt = np.zeros(x.shape, dtype=np.int64)
    for k in range(w):
        cnt += R.day(v, w, k) == ref
    return bool(((cnt > 1) & ~R.isnull(e)).any())


def reference(x, y, kind, cases):
    """the restatement of every case, after the conditions on the input that make the case worth comparing"""
    exp = {}
    for op, w, mode in cases:
        e = R.ts_pair(x, y, op, w) if op in R.PAIR_OPS else R.ts(x, op, w, mode)
        warm = w if op in LAGS else w - 1
        beyond = R.isnull(e[:, warm:])
        if beyond.size:
            if 2 * int((~beyond).sum()) < beyond.size:
                raise BadInput(f"badly chosen input: {op} w={w} {x.shape} {kind} is mostly NULL")
            if kind == "special" and not beyond.any():
                raise BadInput(f"badly chosen input: {op} w={w} {x.shape} has no NULL beyond the warm-up")
            if op in ("rank", "argmin", "argmax") and w >= 2 and not has_tie(x, e, op, w):
                raise BadInput(f"badly chosen input: {op} w={w} {x.shape} {kind} has no tie in a full window")
        assert R.isnull(e[:, :warm]).all()
        exp[op, w, mode] = e
    return exp


def make_for(kind, n, T, w, seed, cases, **kw):
    """an input that meets the conditions for every case, and its references.  With a few symbols and a window of hundreds of days a
    single sprinkled cell empties a third of a symbol's rows, so whether half of the rows keep their sample is up to the draw: the draw
    is repeated (on the restatement's output alone, before the GPU is asked) until it does"""
    err = None
    for k in range(32):
        x, y = make(kind, n, T, w, seed + 7919 * k, **kw)
        try:
            return x, y, reference(x, y, kind, cases)
        except BadInput as e:
            err = e
    raise err


def call(pq, xd, yd, op, w, mode=0):
    F = pq.Factor()
    if op in R.PAIR_OPS:
        return getattr(F, "ts_" + op)(xd, yd, w)
    if op == "rank":
        return F.ts_rank(xd, w, pct=bool(mode))
    return getattr(F, op if op in ("decay_linear", "delay", "delta") else "ts_" + op)(xd, w)


def to_dev(a, pitch=None):
    n, T = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if pitch is None:
        return t.cuda()
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = t.cuda()
    return buf[:, :T]


def check(pq, x, y, exp, cases, pitch=None, tag=""):
    xd, yd = to_dev(x, pitch), to_dev(y, pitch)
    got = None
    for op, w, mode in cases:
        got = call(pq, xd, yd, op, w, mode)
        same(f"{op} w={w} mode={mode} {x.shape} {tag}", got.cpu().numpy(), exp[op, w, mode])
    return got


SHAPES = [((1, 1), "plain"), ((1, 5), "plain"), ((37, 50), "plain"), ((37, 50), "special"), ((300, 131), "plain"), ((300, 131), "special")]


@pytest.mark.parametrize("shape, kind", SHAPES, ids=[f"{n}x{t}-{k}" for (n, t), k in SHAPES])
def test_every_op_bitwise(pq, shape, kind):
    """each op's minimum window, 2, 3 and 20 (longer than the series on the short shapes: all NULL), rank in both modes"""
    n, T = shape
    for w in (1, 2, 3, 20):
        cases = cases_for((w,))
        x, y, exp = make_for(kind, n, T, w, 100 * w + n + T, cases)
        check(pq, x, y, exp, cases, tag=kind)


@pytest.mark.parametrize("w", [2, 3, 20])
def test_series_as_long_as_the_window(pq, w):
    """T = w, w + 1, w + 2: one full sample (none for delay and delta), two, three"""
    for T in (w, w + 1, w + 2):
        for kind in ("plain", "special"):
            cases = cases_for((w,))
            x, y, exp = make_for(kind, 6, T, w, 7 * w + T, cases, sprinkle=False)
            check(pq, x, y, exp, cases, tag=kind)


@pytest.mark.parametrize("T", [255, 256, 257, 515, 1023, 1025, 2051])
def test_day_tiles(pq, T):
    """the 256-day tiles around their edges (tile - 1, tile, tile + 1, 2 tile + 3 and the long series), windows shorter than, equal to
    and longer than a tile up to the cap (a halo over four tiles, the pair kernel's largest LDS stretch), with NULLs on the last day of
    a tile, the first day of the next and the far edge of its halo.  sum, rank, argmax, decay_linear and corr at every point, every op
    at T = 257 and 2051"""
    windows = [20] + ([255, 256, 257] if T >= 1023 else []) + ([1024] if T == 2051 else [])
    ops = R.PAIR_OPS + R.OPS if T in (257, 2051) else CORE[::-1]
    for w in windows:
        for kind in ("plain", "special"):
            cases = cases_for((w,), ops)
            x, y, exp = make_for(kind, 4, T, w, T + w, cases)
            check(pq, x, y, exp, cases, tag=kind)


def test_window_against_the_series_length(pq):
    """the longest window with one full sample (the last day), one day more (all NULL), and the cap"""
    x, y = make("plain", 5, 300, 20, 3)
    xd, yd = to_dev(x), to_dev(y)
    for op in R.OPS + R.PAIR_OPS:
        for w, last_day in ((299 if op in LAGS else 300, True), (301, False), (1024, False)):
            got = call(pq, xd, yd, op, w).cpu().numpy()
            same(f"{op} w={w}", got, R.ts_pair(x, y, op, w) if op in R.PAIR_OPS else R.ts(x, op, w))
            assert R.isnull(got[:, :-1]).all() and (~R.isnull(got[:, -1])).all() == last_day and R.isnull(got[:, -1]).all() != last_day


def test_more_jobs_than_the_grid(pq):
    """more (symbol, tile) jobs than the launch has workgroups: the grid stride restages the LDS tile"""
    n, T = GRID_CAP + 3, 3
    x, y = make("plain", n, T, 2, 5)
    x[n - 2, 1] = R.NULL
    y[n - 1, 2] = R.NULL
    xd, yd = to_dev(x), to_dev(y)
    same(f"rank w=2 {n} symbols", call(pq, xd, yd, "rank", 2).cpu().numpy(), R.ts_rank(x, 2))
    same(f"corr w=2 {n} symbols", call(pq, xd, yd, "corr", 2).cpu().numpy(), R.ts_corr(x, y, 2))
    same(f"delta w=2 {n} symbols", call(pq, xd, yd, "delta", 2).cpu().numpy(), R.delta(x, 2))


@pytest.mark.parametrize("pitch", [51, 64])
def test_row_pitch(pq, pitch):
    """batch stride > len, odd and a multiple of 16 elements: the inputs read (both on the same pitch) and the output written at it"""
    cases = cases_for((3,))
    x, y, exp = make_for("special", 37, 50, 3, pitch, cases)
    got = check(pq, x, y, exp, cases, pitch=pitch, tag=f"pitch {pitch}")
    assert got.stride(0) == pitch


def raw(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import check as ok, lib
    L, h, vp = lib(), api.ctx(), C.c_void_p

    def ts(b, code, w, mode, src, dst):
        ok(L.pq_factor_ts(h, C.byref(b), vp(src), C.c_int32(code), C.c_int64(w), C.c_int32(mode), vp(dst)))

    def pair(b, code, w, sx, sy, dst):
        ok(L.pq_factor_ts_pair(h, C.byref(b), vp(sx), vp(sy), C.c_int32(code), C.c_int64(w), vp(dst)))

    return L, h, ok, ts, pair


def test_caller_owned_out_keeps_its_padding(pq):
    """through the C ABI, out prefilled with a sentinel: columns [T, pitch) are never written"""
    from polars_quant_amd._lib import Batch
    _, _, _, ts, pair = raw(pq)
    n, T, pitch = 37, 300, 304
    cases = cases_for((20,))
    x, y, exp = make_for("special", n, T, 20, 11, cases)
    xd, yd = to_dev(x, pitch), to_dev(y, pitch)
    b = Batch(n, T, pitch)
    for op, w, mode in cases:
        out = torch.full((n, pitch), -77.0, dtype=torch.float64, device="cuda")
        if op in R.PAIR_OPS:
            pair(b, PAIR_CODES[op], w, xd.data_ptr(), yd.data_ptr(), out.data_ptr())
        else:
            ts(b, CODES[op], w, mode, xd.data_ptr(), out.data_ptr())
        same(f"{op} mode={mode} into a caller's column", out[:, :T].cpu().numpy(), exp[op, w, mode])
        assert bool((out[:, T:] == -77.0).all()), f"{op} wrote into the row padding"


def test_refusals_launch_nothing(pq):
    from polars_quant_amd._lib import Batch
    L, h, ok, ts, pair = raw(pq)
    vp = C.c_void_p
    n, T = 40, 30
    x, y = make("plain", n + 1, T, 5, 1)
    buf, ybuf = to_dev(x), to_dev(y)                  # n + 1 rows: x = rows 0 .. n-1, the shifted out = rows 1 .. n
    keep, ykeep = buf.clone(), ybuf.clone()
    out = torch.full((n, T), 7.0, dtype=torch.float64, device="cuda")
    b = Batch(n, T, T)
    xp, yp, op_ = buf.data_ptr(), ybuf.data_ptr(), out.data_ptr()

    def refused(msg, status, fn, *args):
        with pytest.raises(pq.PqError, match=msg) as e:
            fn(*args)
        assert f"pq status {status}:" in str(e.value)

    for (code, w, mode), msg in (((11, 5, 0), "op"), ((-1, 5, 0), "op"), ((0, 0, 0), "window"), ((4, 1025, 0), "window"), ((9, 0, 0), "window"),
                                 ((1, 1, 0), "window"), ((2, 1, 0), "window"), ((0, 5, 1), "mode"), ((6, 5, 1), "mode"), ((7, 5, 2), "mode"),
                                 ((7, 5, -1), "mode"), ((10, 5, 1), "mode")):
        refused(msg, 1, ts, b, code, w, mode, xp, op_)                       # PQ_ERR_ARG
    for (code, w), msg in (((2, 5), "op"), ((-1, 5), "op"), ((0, 1), "window"), ((1, 1), "window"), ((1, 1025), "window")):
        refused(msg, 1, pair, b, code, w, xp, yp, op_)
    for code in CODES.values():
        refused("null pointer", 1, ts, b, code, 5, 0, None, op_)
        refused("null pointer", 1, ts, b, code, 5, 0, xp, None)
        for dst in (xp, xp + T * 8, xp + 8):                                 # out == x, x shifted by one row, by one cell
            refused("overlap", 1, ts, b, code, 5, 0, xp, dst)
    for code in PAIR_CODES.values():
        for args in ((None, yp, op_), (xp, None, op_), (xp, yp, None)):
            refused("null pointer", 1, pair, b, code, 5, *args)
        for dst in (xp, xp + T * 8, xp + 8):
            refused("overlap", 1, pair, b, code, 5, xp, yp, dst)             # out over x
            refused("overlap", 1, pair, b, code, 5, yp, xp, dst)             # out over y
    ok(L.pq_suite_begin(h, C.byref(b)))
    try:
        for code in CODES.values():
            refused("recorded", 5, ts, b, code, 5, 0, xp, op_)               # PQ_ERR_UNSUPPORTED
        for code in PAIR_CODES.values():
            refused("recorded", 5, pair, b, code, 5, xp, yp, op_)
    finally:
        ok(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    for code in CODES.values():
        refused("ragged", 5, ts, rb, code, 5, 0, xp, op_)
    for code in PAIR_CODES.values():
        refused("ragged", 5, pair, rb, code, 5, xp, yp, op_)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == keep).all()) and bool((ybuf == ykeep).all()), "a refused call wrote"
    cases = cases_for((5,))
    check(pq, x, y, reference(x, y, "plain", cases), cases)                  # the context computes again after the refusals


def test_empty_batches(pq):
    from polars_quant_amd._lib import Batch
    _, _, _, ts, pair = raw(pq)
    for shape in ((0, 5), (4, 0)):
        z = torch.empty(shape, dtype=torch.float64, device="cuda")
        for op in R.OPS + R.PAIR_OPS:
            out = call(pq, z, z.clone(), op, 3)
            assert tuple(out.shape) == shape and out.dtype == torch.float64
        b = Batch(shape[0], shape[1], shape[1])
        ts(b, CODES["std"], 3, 0, None, None)                                # PQ_OK, nothing launched
        pair(b, PAIR_CODES["corr"], 3, None, None, None)


@pytest.mark.parametrize("w", [1, 5, 20])
def test_sum_over_w_is_the_moving_average_on_the_device(pq, w):
    x, _ = make("special", 300, 131, w, 60 + w)
    xd = to_dev(x)
    F = pq.Factor()
    s, ma = F.ts_sum(xd, w), F.moving_average(xd, w)
    # an elementwise division of two tensors: by a Python scalar torch multiplies with the reciprocal, which is another rounding
    q = torch.div(s, torch.full_like(s, float(w))).cpu().numpy()
    s, ma = s.cpu().numpy(), ma.cpu().numpy()
    live = ~R.isnull(s)
    assert (live == ~R.isnull(ma)).all() and live.sum() > x.size // 2 and (~live[:, w:]).any()
    same("ts_sum / w against moving_average", q[live], ma[live])


@pytest.mark.parametrize("w", [2, 5, 20])
def test_std_of_the_returns_is_the_volatility_on_the_device(pq, w):
    x, _ = make("plain", 300, 131, w, 70 + w, ties=False)
    xd = to_dev(x)
    F = pq.Factor()
    vol = F.volatility(xd, w).cpu().numpy()
    std = F.ts_std(pq.returns(xd, period=1), w).cpu().numpy()
    assert not R.isnull(vol[:, w:]).any()
    same("ts_std of the returns against volatility", std, vol)
    same("volatility against the restatement", vol, RL.volatility(x, w))


@pytest.mark.parametrize("d", [1, 5, 130])
def test_delay_is_a_bit_copy(pq, d):
    x, _ = make("plain", 300, 131, 5, 80 + d)
    got = pq.Factor().delay(to_dev(x), d).cpu().numpy()
    assert R.isnull(got[:, :d]).all() and (np.signbit(x) & (x == 0.0)).any()          # the -0.0 of the tie pair is copied as it is
    same("delay against the shifted column", got[:, d:], x[:, :-d])
    same("delay by its default of one day", pq.Factor().delay(to_dev(x)).cpu().numpy(), R.delay(x))


def test_end_to_end_on_the_device(pq):
    """-rank(ts_corr(open, volume, 10)) never leaves the device: Factor.rank(-ts_corr) equals the composition of the two restatements
    bit for bit, and Factor.ic on that column equals Factor.ic on a copy that went through the host"""
    o, v = make("special", 300, 131, 10, 29)
    od, vd = to_dev(o), to_dev(v)
    F = pq.Factor()
    corr = F.ts_corr(od, vd, 10)
    col = F.rank(-corr)
    assert corr.is_cuda and col.is_cuda and col.dtype == torch.float64
    exp = B.rank(-R.ts_corr(o, v, 10))
    assert (~R.isnull(exp[:, 9:])).sum() > exp[:, 9:].size // 2 and R.isnull(exp[:, 9:]).any()
    same("rank(-ts_corr)", col.cpu().numpy(), exp)
    fwd = F.momentum(od, 1)
    ic, nv = F.ic(col, fwd)
    ic2, nv2 = F.ic(col.cpu().numpy(), fwd.cpu().numpy())
    same("ic of rank(-ts_corr)", ic.cpu().numpy(), ic2.cpu().numpy())
    assert bool((nv == nv2).all()) and int(nv.max()) > 150
