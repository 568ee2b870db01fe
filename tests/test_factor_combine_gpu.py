"""-m gpu: the combination weights and the composite of K factors (D-30, csrc/xsec/combine.hip) against the numpy restatement in
tests/xsec_combine_ref.py.  Every comparison is bitwise on the uint64 view: D-30 stores every NaN result as NULL, so no cell is left to
the hardware's NaN bits, and the device uses the function set that makes the restatement exact on the host (IEEE add, mul, div, sqrt).

The weights' reference is computed once per (method, K, window, kind) on the longest series at lag 0 and shared: the restatement is
causal (the weights of a series are the first rows of the weights of any longer one) and takes the lag as a shift of its input, so the
reference of a shorter series and of a lag is a slice and a shift of that one; tests/test_factor_combine_ref.py pins both properties
on the restatement itself.  Before the GPU is compared, every case is checked on the restatement's output: at least half of the rows
(cells) beyond the warm-up are non-NULL, and in the `special` inputs at least one of them is NULL -- so no case passes on NULLs alone.
Two kinds of case cannot hold a NULL beside a majority of results and are compared without that second condition: a series with fewer
than two rows beyond the warm-up, and a composite of a single cell."""
import ctypes as C

import numpy as np
import pytest

import factor_portfolio_ref as P
import xsec_combine_ref as R
import xsec_ref as X
from xsec_rolling_ref import shift

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 256                    # days per workgroup of the weights kernel (XW_TILE) and per job of the combine kernel
NULL = R.NULL
LAGS = (0, 1, 5)
CODES = {m: k for k, m in enumerate(R.METHODS)}


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


def to_dev(a, pitch=None):
    n, T = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if pitch is None:
        return t.cuda()
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = t.cuda()
    return buf[:, :T]


# ---------------------------------------------------------------- weights
def lengths(w, lag):
    """no full row, exactly one, and both edges of the 256-day tile"""
    return sorted({1, w + lag - 1, w + lag, 255, 256, 257, 256 + w} - {0})


def make_ic(kind, K, T, w, seed):
    """K IC series of independent normal draws of size 0.05 around 0.03.  `special`, in IC-day terms: a NULL on the last day of a tile
    and on the first day of the next (the last tile edge whose w + 1 dead rows leave a majority of results in every series that holds
    it; at the longest window there is none, and one NULL kills a quarter of the rows of the longest series instead), and for windows
    up to 20 a NaN, a +inf, a -inf and a 0.0 value, each in another factor"""
    rng = np.random.default_rng(seed)
    ic = 0.03 + 0.05 * rng.standard_normal((K, T))
    if kind == "special":
        if w <= 20:
            e = TILE
            ic[0, e - 1], ic[K - 1, e] = NULL, NULL
            for j, (d, v) in enumerate(((40, np.nan), (90, np.inf), (140, -np.inf), (190, 0.0))):
                ic[j % K, d] = v
        else:
            ic[K // 2, T - 64] = NULL
    return ic


def weights_reference(kind, method, K, w):
    """-> (ic, reference at lag 0) on the longest series of the case"""
    T = 256 + w + max(LAGS)
    ic = make_ic(kind, K, T, w, 1000 * K + w + (7 if kind == "special" else 0))
    return ic, R.weights(ic, method, w, 0)


def windows(method, K):
    return (R.min_window(method, K), 20, 1024)


WEIGHT_CASES = [(m, K, w) for m in R.METHODS for K in (1, 2, 3, 8) for w in windows(m, K)]


@pytest.mark.parametrize("method, K, w", WEIGHT_CASES, ids=[f"{m}-K{K}-w{w}" for m, K, w in WEIGHT_CASES])
def test_weights_bitwise(pq, method, K, w):
    from polars_quant_amd import api
    for kind in ("plain", "special"):
        ic, ref0 = weights_reference(kind, method, K, w)
        icd = torch.from_numpy(ic).cuda()
        for lag in LAGS:
            ref = shift(ref0, lag, NULL)
            for T in lengths(w, lag):
                exp = ref[:, :T]
                warm = w + lag - 1
                beyond = R.isnull(exp[:, warm:]).any(axis=0)
                assert R.isnull(exp[:, :warm]).all()
                if beyond.size:
                    assert 2 * int((~beyond).sum()) >= beyond.size, f"badly chosen input: {kind} T={T} lag={lag} is mostly NULL"
                    if kind == "plain":
                        assert not beyond.any()
                    elif beyond.size >= 2:
                        assert beyond.any(), f"badly chosen input: special T={T} lag={lag} has no NULL beyond the warm-up"
                got = api.factor_combine_weights(icd[:, :T].contiguous(), CODES[method], w, lag)
                assert got.is_cuda and tuple(got.shape) == (K, T)
                same(f"{method} K={K} w={w} lag={lag} T={T} {kind}", got.cpu().numpy(), exp)


@pytest.mark.parametrize("w", [1, 2, 20, 1024])
def test_ic_and_icir_are_rolling_ic_on_the_device(pq, w):
    """device weights for ic / icir against device api.rolling_ic shifted by the lag, K = 1 with NULL ICs (every row) and K = 3 (the
    rows that have their weights)"""
    from polars_quant_amd import api
    T = 256 + w + 40
    for K in (1, 3):
        rng = np.random.default_rng(31 * w + K)
        ic = 0.03 + 0.05 * rng.standard_normal((K, T))
        ic[K - 1, [TILE - 1, TILE]] = NULL
        ic[0, T - 20] = NULL
        icd = torch.from_numpy(ic).cuda()
        roll = [api.rolling_ic(icd[k], w) for k in range(K)]
        mean = np.stack([m.cpu().numpy() for m, _ in roll])
        ir = np.stack([r.cpu().numpy() for _, r in roll])
        for lag in LAGS:
            for method, series in (("ic", mean), ("icir", ir)):
                if w < R.min_window(method, K):
                    continue
                exp = shift(series, lag, NULL)
                got = api.factor_combine_weights(icd, CODES[method], w, lag).cpu().numpy()
                row = ~R.isnull(exp).any(axis=0)
                assert row.sum() >= 10 and (~row[w + lag:]).any()
                same(f"{method} K={K} w={w} lag={lag}: rows with weights", got[:, row], exp[:, row])
                assert R.isnull(got[:, ~row]).all()
                if K == 1:
                    same(f"{method} w={w} lag={lag}: every row", got, exp)


# ---------------------------------------------------------------- composite
def make_factors(kind, K, N, T, seed):
    """-> (factors [K, N, T], weights [K, T]).  `plain`: standard normal factors, weights of either sign.  `special`: NULL / NaN / +inf /
    -inf / 0.0 cells at a combined rate of 2.5 % per factor, a NULL in the last cell of factor 0, and from eight days on one day with
    a NULL weight, one with a NaN weight and one whose weights are all 0.0 (D == 0)"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, N, T))
    W = rng.standard_normal((K, T))
    if kind == "special":
        u = rng.random((K, N, T)) * 200.0
        for j, v in enumerate((NULL, np.nan, np.inf, -np.inf, 0.0)):
            F[(u >= j) & (u < j + 1)] = v
        if N * T >= 2:
            F[0, N - 1, T - 1] = NULL
        if T >= 8:
            W[K - 1, T // 3] = NULL
            W[0, T // 3 + 1] = np.nan
            W[:, T // 2] = 0.0
            W[0, T // 2] = -0.0
    return F, W


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 3, 257])
def test_composite_bitwise(pq, N, K):
    """one symbol, a remainder of the 16-symbol strip and seventeen strips; days at both sides of a wave and of the 256-day job; dense columns
    and a row pitch larger than T (odd at even T)"""
    from polars_quant_amd import api
    for T in (1, 63, 64, 65, 257):
        for kind in ("plain", "special"):
            F, W = make_factors(kind, K, N, T, 100 * K + N + T)
            Wd = torch.from_numpy(W).cuda()
            for normalize in (True, False):
                exp = R.composite(F, W, normalize)
                nul = R.isnull(exp)
                assert 2 * int((~nul).sum()) >= nul.size, f"badly chosen input: {kind} {F.shape} is mostly NULL"
                assert not (kind == "plain" and nul.any()) and (kind == "plain" or N * T < 2 or nul.any())
                for pitch in (None, T + 3):
                    cols = [to_dev(F[k], pitch) for k in range(K)]
                    got = api.factor_combine(cols, Wd, normalize)
                    assert got.is_cuda and tuple(got.shape) == (N, T) and (pitch is None or N == 1 or got.stride(0) == pitch)
                    same(f"K={K} {N}x{T} {kind} normalize={normalize} pitch={pitch}", got.cpu().numpy(), exp)


def test_weights_of_one_value_per_factor_are_the_broadcast_rows(pq):
    from polars_quant_amd import api
    K, N, T = 3, 37, 70
    F, _ = make_factors("special", K, N, T, 5)
    w = np.array([0.5, -2.0, 1.25])
    rows = np.repeat(w[:, None], T, axis=1)
    for normalize in (True, False):
        exp = R.composite(F, rows, normalize)
        for given in (w, list(w), torch.from_numpy(w), torch.from_numpy(w).cuda()):
            same("[K] weights", api.factor_combine(F, given, normalize).cpu().numpy(), exp)
        same("[K, T] weights", api.factor_combine(list(F), rows, normalize).cpu().numpy(), exp)
    out = pq.Factor().combine(F, weights=w)
    same("Factor.combine(weights=[K]) composite", out["composite"].cpu().numpy(), R.composite(F, rows, True))
    same("Factor.combine(weights=[K]) weights", out["weights"].cpu().numpy(), rows)
    assert out["ic"] is None
    eq = pq.Factor().combine(list(F), method="equal", normalize=False)
    same("equal weights", eq["composite"].cpu().numpy(), R.composite(F, np.ones(K), False))
    same("equal weights are ones", eq["weights"].cpu().numpy(), np.ones((K, T)))


# ---------------------------------------------------------------- the chain
def market(n, T, K, seed):
    """K standardised factors that each carry a little of the next return, the return and a price"""
    rng = np.random.default_rng(seed)
    ret = 0.02 * rng.standard_normal((n, T))
    F = np.stack([rng.standard_normal((n, T)) + (4.0 + k) * ret / 0.02 * 0.1 for k in range(K)])
    price = 20.0 * np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))
    return F, ret, price


@pytest.mark.parametrize("method", R.METHODS)
def test_causality(pq, method):
    """next_return replaced from day d on (d inside the second tile): the weights and the composite of every day t < d + lag are
    unchanged bit for bit, through Factor.combine"""
    n, T, K, d = 40, 600, 3, 300
    F, ret, _ = market(n, T, K, 11)
    other = ret.copy()
    other[:, d:] = 0.02 * np.random.default_rng(12).standard_normal((n, T - d))
    Fd = torch.from_numpy(F).cuda()
    for lag in (1, 5):
        for rank in (False, True):
            a = pq.Factor().combine(Fd, ret, method=method, window=20, lag=lag, rank=rank)
            b = pq.Factor().combine(Fd, other, method=method, window=20, lag=lag, rank=rank)
            known = d + lag
            wa, wb = a["weights"].cpu().numpy(), b["weights"].cpu().numpy()
            assert tuple(wa.shape) == (K, T) and tuple(a["ic"].shape) == (K, T)
            assert not R.isnull(wa[:, 19 + lag:]).any() and R.isnull(wa[:, :19 + lag]).all()
            same(f"weights before day {known}", wa[:, :known], wb[:, :known])
            same(f"composite before day {known}", a["composite"].cpu().numpy()[:, :known], b["composite"].cpu().numpy()[:, :known])
            assert (wa[:, known] != wb[:, known]).all(), "the first day that may know the new return does"


def test_end_to_end_into_portfolio_backtest(pq):
    """Factor.combine -> portfolio_backtest on the device against the host chain of the reference modules: the oracle's IC, the
    restatement's weights and composite, xsec_ref's labels, factor_portfolio_ref's portfolios"""
    from oracle import pq_oracle as oracle
    n, T, K = 40, 300, 3
    F, ret, price = market(n, T, K, 21)
    F[1, 5, 100] = NULL
    res = pq.Factor().combine(list(F), ret, method="icir", window=60, lag=1)
    ic = np.stack([oracle.factor_ic(np.ascontiguousarray(F[k]), ret, 0)[0] for k in range(K)])
    same("ic", res["ic"].cpu().numpy(), ic)
    w = R.weights(ic, "icir", 60, 1)
    comp = R.composite(F, w, True)
    assert not R.isnull(w[:, 60:]).any() and (~R.isnull(comp[:, 60:])).sum() > comp[:, 60:].size // 2 and R.isnull(comp[5, 100])
    same("weights", res["weights"].cpu().numpy(), w)
    same("composite", res["composite"].cpu().numpy(), comp)
    assert res["composite"].is_cuda
    bt = pq.Factor().portfolio_backtest(res["composite"], price, n_quantiles=5, rebalance=21, start=61, lag=1, cost_rate=0.002)
    torch.cuda.synchronize()
    days = list(range(61, T, 21))
    exp = P.portfolio(X.labels(comp, price, 0, 5, 0.0, 0.0), price, 5, days, None, 1, 0.002, 1_000_000.0)
    for k in ("count", "turnover", "value"):
        g = bt[k].cpu().numpy()
        if k == "count":
            assert (g == exp[k]).all() and int(g.min()) >= 1
        else:
            same(k, g, exp[k])


# ---------------------------------------------------------------- the surface
def raw(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import check as ok, lib
    L, h, vp = lib(), api.ctx(), C.c_void_p

    def weights(ic, k, n, method, w, lag, out):
        ok(L.pq_factor_combine_weights(h, vp(ic), C.c_int32(k), C.c_int64(n), C.c_int32(method), C.c_int64(w), C.c_int64(lag), vp(out)))

    def combine(b, ptrs, k, wts, normalize, out):
        arr = (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None
        ok(L.pq_factor_combine(h, C.byref(b), arr, C.c_int32(k), vp(wts), C.c_int32(normalize), vp(out)))

    return L, h, ok, weights, combine


def test_value_errors_come_before_device_work(pq):
    ones = torch.ones((3, 40), dtype=torch.float64, device="cuda")
    F = pq.Factor()
    for msg, call in (("method", lambda: F.combine([ones, ones], ones, method="mean")),
                      ("next_return", lambda: F.combine([ones, ones])),
                      ("next_return", lambda: F.combine([ones, ones], method="max_icir")),
                      ("weights", lambda: F.combine([ones, ones], ones, weights=[1.0, 1.0])),
                      ("window", lambda: F.combine([ones, ones], ones, method="max_icir", window=2)),
                      ("lag", lambda: F.combine([ones, ones], ones, lag=-1))):
        with pytest.raises(ValueError, match=msg):
            call()


def test_refusals_launch_nothing(pq):
    from polars_quant_amd._lib import Batch
    L, h, ok, weights, combine = raw(pq)
    vp = C.c_void_p
    K, n, T = 3, 40, 30
    F, W = make_factors("plain", K + 1, n, T, 1)
    fbuf = torch.from_numpy(F).cuda()                     # K + 1 planes: factors = planes 0 .. K-1, a shifted out = plane 1 ..
    icbuf = torch.from_numpy(np.ascontiguousarray(W)).cuda()     # [K + 1][T]: ic = rows 0 .. K-1
    fkeep, ickeep = fbuf.clone(), icbuf.clone()
    out = torch.full((n, T), 7.0, dtype=torch.float64, device="cuda")
    wout = torch.full((K, T), 7.0, dtype=torch.float64, device="cuda")
    b = Batch(n, T, T)
    fp = [fbuf[k].data_ptr() for k in range(K)]
    icp, wp, op_ = icbuf.data_ptr(), wout.data_ptr(), out.data_ptr()

    def refused(msg, status, fn, *args):
        with pytest.raises(pq.PqError, match=msg) as e:
            fn(*args)
        assert f"pq status {status}:" in str(e.value)

    for (k, method, w, lag), msg in (((0, 0, 5, 1), "k must"), ((9, 0, 5, 1), "k must"), ((K, 3, 5, 1), "method"), ((K, -1, 5, 1), "method"),
                                     ((K, 0, 0, 1), "window"), ((K, 0, 1025, 1), "window"), ((K, 1, 1, 1), "window"), ((K, 2, K, 1), "window"),
                                     ((K, 0, 5, -1), "lag"), ((K, 0, 5, 1025), "lag")):
        refused(msg, 1, weights, icp, k, T, method, w, lag, wp)                       # PQ_ERR_ARG
    refused("negative length", 1, weights, icp, K, -1, 0, 5, 1, wp)
    refused("null pointer", 1, weights, None, K, T, 0, 5, 1, wp)
    refused("null pointer", 1, weights, icp, K, T, 0, 5, 1, None)
    for dst in (icp, icp + T * 8, icp + 8):                                           # weights == ic, shifted by one row, by one value
        refused("overlap", 1, weights, icp, K, T, 0, 5, 1, dst)
    refused("k must", 1, combine, b, fp, 0, icp, 1, op_)
    refused("k must", 1, combine, b, fp + fp + fp, 9, icp, 1, op_)
    refused("null pointer", 1, combine, b, None, K, icp, 1, op_)
    refused("null pointer", 1, combine, b, fp, K, None, 1, op_)
    refused("null pointer", 1, combine, b, fp, K, icp, 1, None)
    refused("null factor pointer", 1, combine, b, fp[:2] + [None], K, icp, 1, op_)
    for dst in (fp[0], fp[1], fp[K - 1] + 8, fp[0] + T * 8, icp, icp + 8):            # out over a factor, over the weights
        refused("overlap", 1, combine, b, fp, K, icp, 1, dst)
    ok(L.pq_suite_begin(h, C.byref(b)))
    try:
        refused("recorded", 5, weights, icp, K, T, 0, 5, 1, wp)                       # PQ_ERR_UNSUPPORTED
        refused("recorded", 5, combine, b, fp, K, icp, 1, op_)
    finally:
        ok(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    refused("ragged", 5, combine, rb, fp, K, icp, 1, op_)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((wout == 7.0).all()) and bool((fbuf == fkeep).all()) and bool((icbuf == ickeep).all()), \
        "a refused call wrote"
    # the context computes again after the refusals, into a caller's column whose padding stays
    pitch = T + 4
    cols = [to_dev(F[k], pitch) for k in range(K)]
    dst = torch.full((n, pitch), -77.0, dtype=torch.float64, device="cuda")
    combine(Batch(n, T, pitch), [c.data_ptr() for c in cols], K, icp, 1, dst.data_ptr())
    same("into a caller's column", dst[:, :T].cpu().numpy(), R.composite(F[:K], W[:K], True))
    assert bool((dst[:, T:] == -77.0).all()), "the combine kernel wrote into the row padding"
    weights(icp, K, T, 1, 5, 1, wp)
    same("weights after the refusals", wout.cpu().numpy(), R.weights(W[:K], "icir", 5, 1))


def test_empty_batches(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    _, _, _, weights, combine = raw(pq)
    weights(None, 3, 0, 0, 5, 1, None)                                               # PQ_OK, nothing launched
    assert tuple(api.factor_combine_weights(torch.empty((3, 0), dtype=torch.float64, device="cuda"), 0, 5, 1).shape) == (3, 0)
    for shape in ((0, 5), (4, 0)):
        combine(Batch(shape[0], shape[1], shape[1]), None, 2, None, 1, None)
        z = torch.empty(shape, dtype=torch.float64, device="cuda")
        out = api.factor_combine([z, z.clone()], np.ones(2))
        assert tuple(out.shape) == shape and out.dtype == torch.float64 and out.is_cuda
