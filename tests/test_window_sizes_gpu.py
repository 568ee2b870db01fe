"""The window walk (csrc/xsec/xsec_window.h) under each of its users, the combination weights and the composite (D-30,
csrc/xsec/combine.hip) and the group portfolios (D-27, csrc/portfolio/portfolio.hip) at every size class and dispatch branch, bit for bit
against the numpy restatements (xsec_rolling_ref, xsec_ts_ref, xsec_rolling_regress_ref, xsec_combine_ref, factor_portfolio_ref), with the
helpers of the feature test modules.  No comparison has a tolerance: float columns are compared on their uint64 view, counts exactly.

The case tables are module-level.  Every case is built by a cached function that runs the restatement and asserts the conditions on the
input before anything is returned, so a device comparison never sees an input that was not checked; test_tables_on_the_cpu (not marked
gpu) walks every table through these functions alone.

Where each branch is reached (the failure tags name op, window, K, lag and shape):

| branch (never reached before)                    | case                                                                           |
|--------------------------------------------------|--------------------------------------------------------------------------------|
| xw_last_scan, runs of C = ceil((255 + w) / 256)  | SCAN_WINDOWS: C = 1 [w1], 2 [w2, w257], 3 [w258, w513], 4 [w514, w769],        |
|   entries per thread: C = 3 and C = 4; an        |   5 [w770, w1024].  One symbol per staged entry p of scan_positions(w): 0,     |
|   unusable entry at a chosen place of a thread's |   M - 1, the first and last entry of the run of thread 1, 17, 63, 64, 65, 128, |
|   run, of a wave's 64 runs, of the clamped tail  |   191, 192, 255 and the entry before it, the first entry of the last run (the  |
|   (lo = hi = M: the threads behind the last run) |   threads behind it scan nothing); scan_pairs(w): two entries closer than w in |
|                                                  |   different waves, further apart than w, both in one run                       |
| ... under rl_window_kernel (the day itself; the  | test_mark_scan[moving_average-*], [volatility-*]                               |
|   return-based load: entries p and p + 1)        |                                                                                |
| ... under ts_window_kernel (static LDS) and      | test_mark_scan[ts_sum-*], [ts_rank-*], [ts_corr-*] (the cell in y only)        |
|   ts_pair_kernel (dynamic LDS)                   |                                                                                |
| ... under rr_window_kernel's written-out walk,   | test_mark_scan[rolling_regress_k1-*] (the cell in y), [rolling_regress_k4-*]   |
|   K = 1 and K = 4 with a [T] series regressor    |   (a per-symbol regressor or y; of a pair one each), [rolling_regress_k4_      |
|                                                  |   series-*] (the series' cell is every symbol's)                               |
| ... under cb_weights_kernel, the staged day      | test_mark_scan_combine[w*]: K = 2, ic, lag 0 and 3, one launch per entry of    |
|   shifted by the lag                             |   scan_positions_thin(w), the NULL in the second series                        |
| cb_weights_kernel<K, METHOD>, K = 4 .. 7         | test_weights_every_k[ic / icir / max_icir - K4 .. K7 - minimum window, 20,     |
|   (twelve instantiations)                        |   1024]: test_factor_combine_gpu's inputs, lengths, lags and conditions        |
| dynamic LDS of (8 K + 4)(255 + w) bytes between  |   [*-K5-w1024] 56 276, [*-K6-w1024] 66 508, [*-K7-w1024] 76 740 bytes          |
|   46 044 and 86 972                              |                                                                                |
| the host's test lds > 48 KiB in front of         | test_weights_lds_thresholds: 49 148 / 49 192 [K5-w862, K5-w863], 49 096 /      |
|   hipFuncSetAttribute; 64 KiB                    |   49 164 [K8-w467, K8-w468]; 65 520 / 65 572 [K6-w1005, K6-w1006], 65 484 /    |
|                                                  |   65 552 [K8-w708, K8-w709]; max_icir                                          |
| lag of a whole tile or more (up to 1024)         | test_weights_long_lag[lag255, lag256, lag257, lag1024], K = 3, w = 20          |
| cb_combine_kernel<K>, K = 2, 4, 5, 6, 7; N a     | test_composite_strips_and_tiles[K2, K4 .. K7]: N = 15, 16, 17, 32, 33, T =     |
|   multiple of CB_STRIP = 16 and either side of   |   255, 256, 513; (33, 513) is 3 strips x 3 tiles                               |
|   one; the (strip, tile) decode with both > 2    |                                                                                |
| cb_combine_kernel's grid stride (jobs > 2^20)    | test_composite_more_jobs_than_the_grid: N = 16 * 2^20 + 17, T = 1              |
| pf_chain_kernel's second and third LDS pass and  | test_portfolio_chain_across_passes[R1023 .. R2049, R2100], with and without    |
|   the B carried between them                     |   weights, one case at label_lag 2                                             |
| symbol batches of 8 / 8 / 4, blocks of 256, day  | test_portfolio_edges: N = 7, 8, 9, 255, 256, 257, 512; T = 63, 64, 65, 128,    |
|   waves of 64 of the weight / growth / turnover  |   129; ng = 2, 5, 20                                                           |
|   passes                                         |                                                                                |
| label_lag above 1, label index 0                 | test_portfolio_label_lag[lag2-*, lag5-*]: first rebalance day = lag, lag + 1   |

The input conditions of the mark scan.  The series ends with the examined tile (T = t0 + 256), whose row i is staged entry i + w - 1 with
the window of entries i .. i + w - 1.  A cell at entry p therefore leaves rows p - w + 1 .. p of the tile NULL, and at w >= 257 a cell
with 255 <= p <= w - 1 covers all 256 rows: the position lists hold such entries at every window from 257 on but 258 (2 symbols at
w = 257, 3 at 513, 7 at 514, 12 at 769, 10 at 770, 15 at 1024, for an op that marks the day itself).  Those symbols check that the
mark reaches every row of the tile, and no choice of values gives them a non-NULL row in it.  For the same reason the non-NULL share of
the rows beyond the warm-up is a property of the position list, not of the draw: 0.99 at w = 1 and 2, 0.57 at 257, 0.56 at 258, 0.45 at
513, 0.38 at 514, 0.34 at 769, 0.38 at 770 and 0.33 at 1024 for every op of test_mark_scan (from w = 257 on 0.42 .. 0.75 over the
launches of one window and lag in test_mark_scan_combine).  What is asserted, on the restatement alone and before the device is asked:
 - the restatement's NULL mask is exactly the mask derived from (p, w, op) by reach_mask, for every symbol;
 - every single-cell symbol has a NULL row in the tile, and a non-NULL one unless its cell covers the tile, which is decided from (p, w);
 - at least half of the rows beyond the warm-up are non-NULL up to w = 258, and at least a quarter from w = 513 on (the bar that
   test_factor_rolling_regress_gpu's parity grid sets for its long windows)."""
import functools

import numpy as np
import pytest

import factor_portfolio_ref as P
import test_factor_combine_gpu as CB
import test_factor_portfolio_gpu as PF
import test_factor_rolling_regress_gpu as RG
import xsec_combine_ref as CR
import xsec_rolling_ref as RL
import xsec_rolling_regress_ref as RR
import xsec_ts_ref as TS

torch = pytest.importorskip("torch")

TILE = 256                    # days per workgroup of the windowed kernels (XW_TILE)
GRID_CAP = 1 << 20            # workgroups per launch; above it the kernels walk their jobs with a grid stride
STRIP = 16                    # symbols per job of the combine kernel (CB_STRIP)
NULL = RL.NULL
isnull = RL.isnull
same = CB.same


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


# ---------------------------------------------------------------- 1. the mark scan
SCAN_WINDOWS = [1, 2, 257, 258, 513, 514, 769, 770, 1024]       # both ends of every C class
SCAN_THREADS = (1, 17, 63, 64, 65, 128, 191, 192, 255)
SCAN_THIN = (1, 64, 192)
# op -> (minimum window, extra: the warm-up is w - 1 + extra rows and a cell at day d reaches rows d .. d + w - 1 + extra)
SCAN_OPS = {"moving_average": (1, 0), "volatility": (2, 1), "ts_sum": (1, 0), "ts_rank": (1, 0), "ts_corr": (2, 0),
            "rolling_regress_k1": (3, 0), "rolling_regress_k4": (6, 0), "rolling_regress_k4_series": (6, 0)}
SCAN_CASES = [(op, w) for op in SCAN_OPS for w in SCAN_WINDOWS if w >= SCAN_OPS[op][0]]
SCAN_LAGS = (0, 3)


def scan_geometry(w, lag=0):
    """-> (M staged entries, C entries per thread, t0 the first tile whose halo lies wholly inside the series, T = t0 + TILE, the day
    whose value staged entry 0 holds)"""
    M = TILE - 1 + w
    t0 = TILE * -(-(w - 1 + lag) // TILE)
    return M, -(-M // TILE), t0, t0 + TILE, t0 - (w - 1) - lag


def scan_positions(w, threads=SCAN_THREADS):
    M, C = scan_geometry(w)[:2]
    pos = {0, M - 1, (M - 1) // C * C}                           # ... and the first entry of the last non-empty run
    for k in threads:
        if k * C < M:                                            # thread k's run [kC, min(kC + C, M)) is not empty
            pos |= {k * C - 1, k * C, min(k * C + C, M) - 1}
    return sorted(p for p in pos if 0 <= p < M)


def scan_positions_thin(w):
    return scan_positions(w, SCAN_THIN)


def scan_pairs(w):
    M, C = scan_geometry(w)[:2]
    a = 64 * C - 1                                               # the last entry of wave 0
    out = [(a, min(a + w - 1, M - 1))] if w >= 2 else []         # closer than w apart, the second in a later wave
    out.append((3, 3 + w + 100))                                 # further apart than w: 100 rows between them keep their window
    if C >= 2:
        out.append((100 * C, 100 * C + C - 1))                   # the first and last entry of thread 100's run
    return out


def scan_symbols(w):
    """-> (the cells of every symbol as tuples of staged entries, the number of single-cell symbols in front)"""
    pos = scan_positions(w)
    return [(p,) for p in pos] + scan_pairs(w), len(pos)


# the tables reach what the branch table names (checked at import, with or without a GPU)
assert sorted({scan_geometry(w)[1] for w in SCAN_WINDOWS}) == [1, 2, 3, 4, 5]
assert all(scan_geometry(w)[1] != scan_geometry(w + 1)[1] for w in (1, 257, 513, 769)) and scan_geometry(1024)[3] == 1280
assert all(15 <= len(scan_symbols(w)[0]) <= 32 and 7 <= len(scan_positions_thin(w)) <= 12 for w in SCAN_WINDOWS)
assert all(set(scan_positions_thin(w)) <= set(scan_positions(w)) for w in SCAN_WINDOWS)
for _w in SCAN_WINDOWS:
    _M, _C = scan_geometry(_w)[:2]
    for _a, _b in scan_pairs(_w):
        assert 0 <= _a < _b < _M
    _far = [(a, b) for a, b in scan_pairs(_w) if b - a > _w]
    _near = [(a, b) for a, b in scan_pairs(_w) if b - a < _w and a // _C // 64 != b // _C // 64]
    _run = [(a, b) for a, b in scan_pairs(_w) if a // _C == b // _C]
    assert len(_far) == 1 and len(_near) == (_w >= 2) and len(_run) == (_C >= 2)


def reach_mask(cells, T, w, day0, extra=0, lag=0):
    """the rows without a result, from the geometry alone: the warm-up, and for a cell at staged entry p (day day0 + p of the input) the
    rows whose window holds it"""
    null = np.zeros(T, dtype=bool)
    null[:w - 1 + extra + lag] = True
    for p in cells:
        d = day0 + p + lag
        null[d:d + w + extra] = True
    return null


def walk(rng, n, T):
    return np.exp(np.cumsum(0.02 * rng.standard_normal((n, T)), axis=1))


def scan_conditions(tag, exp, null, w, warm, extra, t0, singles):
    """exp: {name: [n, T] or [K, n, T]} of the restatement, null [n, T] from reach_mask; singles: the staged entry of each single-cell symbol, which
    makes the entries p .. p + extra unusable"""
    for name, e in exp.items():
        assert (isnull(e) == np.broadcast_to(null, e.shape)).all(), f"{tag} {name}: the restatement's NULL rows are not the cell's reach"
    live = ~null[:, warm:]
    assert (2 if w <= 258 else 4) * int(live.sum()) >= live.size, f"badly chosen input: {tag} is mostly NULL ({live.mean():.3f})"
    for s, p in enumerate(singles):
        tile = null[s, t0:t0 + TILE]
        # rows p - w + 1 .. p + extra hold every row of the tile (behind the warm-up, which volatility's reaches into the tile at t0 = w - 1)
        covered = p - w + 1 <= max(0, warm - t0) and p + extra >= TILE - 1
        assert tile.any() and tile.all() == covered, f"badly chosen input: {tag} symbol {s}, entry {p}"


@functools.lru_cache(maxsize=None)
def scan_case(op, w):
    """-> (device inputs as numpy, expected {name: array}, null [n, T])"""
    extra = SCAN_OPS[op][1]
    M, C, t0, T, g0 = scan_geometry(w)
    symbols, n_single = scan_symbols(w)
    if op == "rolling_regress_k4_series":
        symbols, n_single = [(w + 150,)] * 3, 3                    # one cell of the series is every symbol's: rows 151 .. 255 of the tile
    n = len(symbols)
    rng = np.random.default_rng(1000 * list(SCAN_OPS).index(op) + w)
    null = np.stack([reach_mask(cells, T, w, g0, extra) for cells in symbols])
    days = [[g0 + p for p in cells] for cells in symbols]
    if op in ("moving_average", "volatility", "ts_sum", "ts_rank"):
        x = walk(rng, n, T)
        for s, ds in enumerate(days):
            x[s, ds] = NULL
        e = (RL.rolling(x, "mean" if op == "moving_average" else op, w) if op in ("moving_average", "volatility")
             else TS.ts(x, op[3:], w))
        inputs, exp = (x,), {op: e}
    elif op == "ts_corr":
        x, y = walk(rng, n, T), walk(rng, n, T)
        for s, ds in enumerate(days):
            y[s, ds] = NULL
        inputs, exp = (x, y), {op: TS.ts_pair(x, y, "corr", w)}
    else:
        K = 1 if op.endswith("k1") else 4
        y, xs = RG.make(n, T, K, int(rng.integers(1 << 30)), series=() if K == 1 else (1,))
        own = [j for j in range(K) if K > 1 and j != 1]                 # the per-symbol regressors
        for s, ds in enumerate(days):
            if op == "rolling_regress_k4_series":
                xs[1][ds] = NULL
            else:                                                  # K = 4: even symbols in a regressor (of a pair, the first cell), odd in y
                for i, d in enumerate(ds):
                    col = xs[own[(s // 2) % len(own)]] if K > 1 and s % 2 == 0 and i == 0 else y
                    col[s, d] = NULL
        inputs, exp = (y, *xs), RR.rolling_regress(y, xs, w)
    scan_conditions(f"{op} w={w}", exp, null, w, w - 1 + extra, extra, t0, [cells[0] for cells in symbols[:n_single]])
    return inputs, exp, null


def scan_device(pq, op, w, inputs):
    from polars_quant_amd import api
    F = pq.Factor()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs]
    if op.startswith("rolling_regress"):
        return {k: v.cpu().numpy() for k, v in api.factor_rolling_regress(dev[0], dev[1:], w).items()}
    got = getattr(F, op)(*dev, w)
    return {op: got.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("op, w", SCAN_CASES, ids=[f"{op}-w{w}" for op, w in SCAN_CASES])
def test_mark_scan(pq, op, w):
    """one launch: a symbol per staged entry of the examined tile, a few with two cells"""
    inputs, exp, null = scan_case(op, w)
    got = scan_device(pq, op, w, inputs)
    assert sorted(got) == sorted(exp)
    for name, e in exp.items():
        same(f"{op} w={w} {name}", got[name], e)
        assert (isnull(got[name]) == np.broadcast_to(null, e.shape)).all(), f"{op} w={w} {name}: NULL rows"


@functools.lru_cache(maxsize=None)
def scan_combine_case(w, lag):
    """-> [(staged entry, ic [2, T], expected weights [2, T], null [T])]: K = 2, method ic, the NULL in the second series on the day that
    staged entry p of the examined tile reads (lag days before the day it stands for)"""
    M, C, t0, T, day0 = scan_geometry(w, lag)
    assert day0 >= 0 and T == t0 + TILE
    out = []
    for p in scan_positions_thin(w):
        ic = 0.03 + 0.05 * np.random.default_rng(7000 + 10 * w + lag + 100000 * p).standard_normal((2, T))
        ic[1, day0 + p] = NULL
        out.append((p, ic, CR.weights(ic, "ic", w, lag), reach_mask((p,), T, w, day0, 0, lag)))
    tag = f"combine weights w={w} lag={lag}"
    exp = {f"entry {p} series {k}": np.stack([o[2][k] for o in out]) for k in (0, 1)}
    scan_conditions(tag, exp, np.stack([o[3] for o in out]), w, w - 1 + lag, 0, t0, [o[0] for o in out])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w", SCAN_WINDOWS, ids=[f"w{w}" for w in SCAN_WINDOWS])
def test_mark_scan_combine(pq, w):
    """cb_weights_kernel: one symbol of K series, so one launch per staged entry; lag 3 shifts the day an entry reads"""
    from polars_quant_amd import api
    for lag in SCAN_LAGS:
        for p, ic, exp, null in scan_combine_case(w, lag):
            got = api.factor_combine_weights(torch.from_numpy(ic).cuda(), CB.CODES["ic"], w, lag).cpu().numpy()
            same(f"combine weights w={w} lag={lag} entry {p}", got, exp)
            assert (isnull(got) == null[None, :]).all(), f"combine weights w={w} lag={lag} entry {p}: NULL rows"


# ---------------------------------------------------------------- 2. combine
WEIGHT_KS = (4, 5, 6, 7)
WEIGHT_CASES = [(m, K, w) for m in CR.METHODS for K in WEIGHT_KS for w in CB.windows(m, K)]
LDS_CASES = [(5, 862), (5, 863), (8, 467), (8, 468), (6, 1005), (6, 1006), (8, 708), (8, 709)]      # (K, w), pairs around 48 and 64 KiB
LONG_LAGS = [255, 256, 257, 1024]
COMPOSITE_KS = (2, 4, 5, 6, 7)
COMPOSITE_NS = (15, 16, 17, 32, 33)
COMPOSITE_TS = (255, 256, 513)
KINDS = ("plain", "special")


def weights_lds(K, w):
    return (8 * K + 4) * (TILE - 1 + w)


assert len(WEIGHT_CASES) == 36 and [weights_lds(K, 1024) for K in (5, 6, 7)] == [56276, 66508, 76740]
assert [weights_lds(K, w) for K, w in LDS_CASES] == [49148, 49192, 49096, 49164, 65520, 65572, 65484, 65552]
assert all((weights_lds(*a) <= lim) and (weights_lds(*b) > lim)
           for a, b, lim in zip(LDS_CASES[::2], LDS_CASES[1::2], (48 << 10, 48 << 10, 64 << 10, 64 << 10)))


def weight_conditions(tag, kind, exp, warm):
    """test_factor_combine_gpu.test_weights_bitwise's, on the rows beyond `warm`"""
    beyond = isnull(exp[:, warm:]).any(axis=0)
    assert isnull(exp[:, :warm]).all()
    if beyond.size:
        assert 2 * int((~beyond).sum()) >= beyond.size, f"badly chosen input: {tag} is mostly NULL"
        if kind == "plain":
            assert not beyond.any()
        elif beyond.size >= 2:
            assert beyond.any(), f"badly chosen input: {tag} has no NULL beyond the warm-up"


@functools.lru_cache(maxsize=None)
def weights_case(method, K, w):
    """test_weights_bitwise's inputs -> [(kind, ic, [(lag, T, expected)])]: one reference per kind, on the longest series at lag 0"""
    out = []
    for kind in KINDS:
        ic, ref0 = CB.weights_reference(kind, method, K, w)
        runs = []
        for lag in CB.LAGS:
            ref = RL.shift(ref0, lag, NULL)
            for T in CB.lengths(w, lag):
                exp = ref[:, :T]
                weight_conditions(f"{method} K={K} w={w} {kind} T={T} lag={lag}", kind, exp, w + lag - 1)
                runs.append((lag, T, exp))
        out.append((kind, ic, runs))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("method, K, w", WEIGHT_CASES, ids=[f"{m}-K{K}-w{w}" for m, K, w in WEIGHT_CASES])
def test_weights_every_k(pq, method, K, w):
    from polars_quant_amd import api
    for kind, ic, runs in weights_case(method, K, w):
        icd = torch.from_numpy(ic).cuda()
        for lag, T, exp in runs:
            got = api.factor_combine_weights(icd[:, :T].contiguous(), CB.CODES[method], w, lag)
            assert got.is_cuda and tuple(got.shape) == (K, T)
            same(f"{method} K={K} w={w} lag={lag} T={T} {kind}", got.cpu().numpy(), exp)


@functools.lru_cache(maxsize=None)
def lds_case(K, w):
    T = TILE + w + 1
    ic = CB.make_ic("plain", K, T, w, 50 * K + w)
    exp = CR.weights(ic, "max_icir", w, 0)
    weight_conditions(f"max_icir K={K} w={w} T={T}", "plain", exp, w - 1)
    return ic, exp


@pytest.mark.gpu
@pytest.mark.parametrize("K, w", LDS_CASES, ids=[f"K{K}-w{w}" for K, w in LDS_CASES])
def test_weights_lds_thresholds(pq, K, w):
    """the last window whose dynamic LDS fits 48 KiB (64 KiB) and the first that does not, at two K each; max_icir, the heaviest row"""
    from polars_quant_amd import api
    ic, exp = lds_case(K, w)
    got = api.factor_combine_weights(torch.from_numpy(ic).cuda(), CB.CODES["max_icir"], w, 0)
    same(f"max_icir K={K} w={w} lds={weights_lds(K, w)}", got.cpu().numpy(), exp)


@functools.lru_cache(maxsize=None)
def long_lag_case(lag):
    K, w = 3, 20
    T = TILE + w + lag + 1
    out = []
    for kind in KINDS:
        ic = CB.make_ic(kind, K, T, w, 300 + lag + (7 if kind == "special" else 0))
        for method in CR.METHODS:
            exp = CR.weights(ic, method, w, lag)
            weight_conditions(f"{method} K={K} w={w} lag={lag} T={T} {kind}", kind, exp, w + lag - 1)
            out.append((kind, method, ic, exp))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lag", LONG_LAGS, ids=[f"lag{lag}" for lag in LONG_LAGS])
def test_weights_long_lag(pq, lag):
    """the staged day a tile less one, a tile, a tile and one, four tiles behind the day it stands for"""
    from polars_quant_amd import api
    for kind, method, ic, exp in long_lag_case(lag):
        got = api.factor_combine_weights(torch.from_numpy(ic).cuda(), CB.CODES[method], 20, lag)
        same(f"{method} K=3 w=20 lag={lag} {kind}", got.cpu().numpy(), exp)


def composite_grid(K):
    """(N, T, kind) for every N and T; the kind alternates along N, along T and along K"""
    k = COMPOSITE_KS.index(K)
    return [(N, T, KINDS[(k + i + j) % 2]) for i, N in enumerate(COMPOSITE_NS) for j, T in enumerate(COMPOSITE_TS)]


for _K in COMPOSITE_KS:
    _g = composite_grid(_K)
    assert len(_g) == 15 and all({kind for N, T, kind in _g if N == n} == set(KINDS) for n in COMPOSITE_NS)
    assert all({kind for N, T, kind in _g if T == t} == set(KINDS) for t in COMPOSITE_TS)
assert {n % STRIP for n in COMPOSITE_NS} == {15, 0, 1} and -(-33 // STRIP) == 3 and -(-513 // TILE) == 3


def composite_conditions(tag, kind, exp):
    """test_factor_combine_gpu.test_composite_bitwise's"""
    nul = isnull(exp)
    assert 2 * int((~nul).sum()) >= nul.size, f"badly chosen input: {tag} is mostly NULL"
    assert not (kind == "plain" and nul.any()) and (kind == "plain" or nul.any())


@functools.lru_cache(maxsize=None)
def composite_case(K):
    """-> [(N, T, kind, factors, weights, {normalize: expected})]"""
    out = []
    for N, T, kind in composite_grid(K):
        F, W = CB.make_factors(kind, K, N, T, 100 * K + N + T)
        exp = {}
        for normalize in (True, False):
            exp[normalize] = CR.composite(F, W, normalize)
            composite_conditions(f"K={K} {N}x{T} {kind} normalize={normalize}", kind, exp[normalize])
        out.append((N, T, kind, F, W, exp))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K", COMPOSITE_KS, ids=[f"K{K}" for K in COMPOSITE_KS])
def test_composite_strips_and_tiles(pq, K):
    """a remainder of 15, none and one on one and two strips of 16 symbols; a tile less one day, one tile, two tiles and a day; normalize
    on and off, dense columns and the row pitch T + 3"""
    from polars_quant_amd import api
    for N, T, kind, F, W, exp in composite_case(K):
        Wd = torch.from_numpy(W).cuda()
        for pitch in (None, T + 3):
            cols = [CB.to_dev(F[k], pitch) for k in range(K)]
            for normalize in (True, False):
                got = api.factor_combine(cols, Wd, normalize)
                assert got.is_cuda and tuple(got.shape) == (N, T) and (pitch is None or got.stride(0) == pitch)
                same(f"K={K} {N}x{T} {kind} normalize={normalize} pitch={pitch}", got.cpu().numpy(), exp[normalize])


STRIDE_N = STRIP * GRID_CAP + 17
STRIDE_NULLS = (3, STRIP * GRID_CAP + 5, STRIDE_N - 1)           # in the first strip, in the first strip of the second step, in the last
assert -(-STRIDE_N // STRIP) == GRID_CAP + 2 and STRIDE_NULLS[1] // STRIP == GRID_CAP and STRIDE_NULLS[2] // STRIP == GRID_CAP + 1


@functools.lru_cache(maxsize=None)
def stride_case():
    """N = 16 * 2^20 + 17 symbols on one day: 2^20 + 2 strips, so two jobs fall to the second step of the grid stride, the last a strip
    of one symbol"""
    rng = np.random.default_rng(77)
    F = rng.standard_normal((1, STRIDE_N, 1))
    F[0, list(STRIDE_NULLS), 0] = NULL
    W = np.array([[-0.75]])
    exp = {}
    for normalize in (True, False):
        e = CR.composite(F, W, normalize)
        nul = isnull(e)
        assert np.flatnonzero(nul).tolist() == list(STRIDE_NULLS)
        exp[normalize] = e
    return F, W, exp


@pytest.mark.gpu
def test_composite_more_jobs_than_the_grid(pq):
    """more (strip, tile) jobs than the launch has workgroups; the whole column is compared"""
    from polars_quant_amd import api
    F, W, exp = stride_case()
    col = torch.from_numpy(F[0]).cuda()
    Wd = torch.from_numpy(W).cuda()
    for normalize in (True, False):
        got = api.factor_combine([col], Wd, normalize)
        assert tuple(got.shape) == (STRIDE_N, 1)
        same(f"K=1 {STRIDE_N}x1 normalize={normalize}", got.cpu().numpy(), exp[normalize])
        del got
    del col
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 3. factor_portfolio
CHAIN = 1024                  # rebalances per LDS pass of the chain (PF_CHAIN)
CHAIN_N, CHAIN_T, CHAIN_NG, COST = 37, 2100, 3, 0.003
# (R, first day, weights, label_lag): both sides of one and two passes on consecutive days from day 5, the daily schedule from day 0
CHAIN_CASES = [(R, 5, wts, 0) for R in (1023, 1024, 1025, 2048, 2049) for wts in (False, True)] + \
              [(2100, 0, False, 0), (2100, 0, True, 0), (1025, 5, True, 2)]
# (N, T, ng, schedule, weights): the batches of 8, 8 and 4 symbols, the blocks of 256, the waves of 64 days
EDGE_CASES = [(7, 63, 2, "every5", False), (7, 64, 5, "irregular", True), (8, 64, 5, "every5", False), (8, 65, 2, "irregular", True),
              (9, 65, 2, "every5", False), (9, 128, 5, "irregular", True), (255, 128, 20, "every5", False), (255, 129, 5, "irregular", True),
              (256, 129, 2, "every5", False), (256, 63, 20, "irregular", True), (257, 63, 5, "every5", False),
              (257, 64, 20, "irregular", True), (512, 65, 20, "every5", False), (512, 128, 2, "irregular", True)]
LAG_CASES = [(lag, lag + late, wts) for lag in (2, 5) for late, wts in ((0, False), (1, True))]      # (label_lag, first day, weights)
LAG_N, LAG_T, LAG_NG = 300, 131, 5

assert {-(-c[0] // CHAIN) for c in CHAIN_CASES} == {1, 2, 3} and {c[0] % CHAIN for c in CHAIN_CASES} >= {1023, 0, 1}
assert all(c[1] + c[0] <= CHAIN_T and c[1] >= c[3] for c in CHAIN_CASES) and any(c[3] == 2 for c in CHAIN_CASES)
assert {c[0] for c in EDGE_CASES} == {7, 8, 9, 255, 256, 257, 512} and {c[1] for c in EDGE_CASES} == {63, 64, 65, 128, 129}
assert {c[2] for c in EDGE_CASES} == {2, 5, 20} and all(len({c[1] for c in EDGE_CASES if c[0] == n}) == 2 for n in (7, 8, 9, 255, 256, 257, 512))
assert all({c[k] for c in EDGE_CASES if c[0] == n} == set(v) for n in (7, 512) for k, v in ((3, ("every5", "irregular")), (4, (False, True))))


def chain_days(R, first):
    return list(range(first, first + R))


@functools.lru_cache(maxsize=None)
def chain_case(R, first, weights, lag):
    labels, price, weight = PF.make(CHAIN_N, CHAIN_T, CHAIN_NG, 900 + R + lag, weights)
    days = chain_days(R, first)
    exp = P.portfolio(labels, price, CHAIN_NG, days, weight, lag, COST, PF.C0)
    v = exp["value"]
    assert np.isfinite(v).all() and (v > 0.0).all(), f"badly chosen input: R={R} the value leaves (0, inf)"
    assert (exp["turnover"][:, 1:] > 0.0).any(axis=0).all()        # 1 - cost_rate tau is not 1 on any rebalance day after the first
    return labels, price, weight, days, exp


def portfolio_device(labels, price, weight, ng, days, lag, exp, tag):
    from polars_quant_amd import api
    got = api.factor_portfolio(PF.to_dev(labels), PF.to_dev(price), ng, days, None if weight is None else PF.to_dev(weight), lag, COST, PF.C0)
    torch.cuda.synchronize()
    tag = f"{tag} {price.shape} ng={ng} R={len(days)} lag={lag} weights={weight is not None}"
    for k in ("count", "turnover", "value"):
        PF.same(f"{k} {tag}", got[k].cpu().numpy(), exp[k])
    PF.same(f"rebalance_days {tag}", got["rebalance_days"].cpu().numpy(), np.asarray(days, dtype=np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("R, first, weights, lag", CHAIN_CASES, ids=[f"R{c[0]}-{'weights' if c[2] else 'equal'}-lag{c[3]}" for c in CHAIN_CASES])
def test_portfolio_chain_across_passes(pq, R, first, weights, lag):
    """R rebalances on consecutive days: the chain's LDS passes of 1024 with one step less, exactly, one more; two passes and three"""
    labels, price, weight, days, exp = chain_case(R, first, weights, lag)
    portfolio_device(labels, price, weight, CHAIN_NG, days, lag, exp, "chain")


@functools.lru_cache(maxsize=None)
def edge_case(N, T, ng, schedule, weights):
    """PF.make's dirty table; on the second rebalance day the members of the last group are moved to group 0, so that day has an empty
    group at every N"""
    labels, price, weight = PF.make(N, T, ng, 40 * N + T + ng, weights)
    days = PF.schedules(T)[schedule]
    labels[labels[:, days[1]] == ng - 1, days[1]] = 0
    exp = P.portfolio(labels, price, ng, days, weight, 0, COST, PF.C0)
    cnt = exp["count"]
    assert (cnt.max(axis=1) >= 1).all(), f"badly chosen input: {N}x{T} ng={ng} {schedule}: a group never has a member"
    assert cnt[ng - 1, 1] == 0 and (N < 8 or (cnt == 0).any())
    return labels, price, weight, days, exp


@pytest.mark.gpu
@pytest.mark.parametrize("N, T, ng, schedule, weights", EDGE_CASES, ids=[f"n{c[0]}-T{c[1]}-ng{c[2]}-{c[3]}" for c in EDGE_CASES])
def test_portfolio_edges(pq, N, T, ng, schedule, weights):
    labels, price, weight, days, exp = edge_case(N, T, ng, schedule, weights)
    portfolio_device(labels, price, weight, ng, days, 0, exp, schedule)


@functools.lru_cache(maxsize=None)
def lag_case(lag, first, weights):
    labels, price, weight = PF.make(LAG_N, LAG_T, LAG_NG, 60 + 10 * lag + first, weights)
    days = list(range(first, LAG_T, 7))
    exp = P.portfolio(labels, price, LAG_NG, days, weight, lag, COST, PF.C0)
    assert (exp["count"] >= 1).all() and days[0] - lag in (0, 1)
    return labels, price, weight, days, exp


@pytest.mark.gpu
@pytest.mark.parametrize("lag, first, weights", LAG_CASES, ids=[f"lag{c[0]}-first{c[1]}" for c in LAG_CASES])
def test_portfolio_label_lag(pq, lag, first, weights):
    """the labels of day d - label_lag: the first rebalance reads label index 0, or 1"""
    labels, price, weight, days, exp = lag_case(lag, first, weights)
    portfolio_device(labels, price, weight, LAG_NG, days, lag, exp, "label_lag")


# ---------------------------------------------------------------- the tables, without a GPU
def test_tables_on_the_cpu():
    """builds every input of every table above, runs its restatement and asserts the input conditions (inside the case functions)"""
    for op, w in SCAN_CASES:
        inputs, exp, null = scan_case(op, w)
        assert all(a.shape[-1] == scan_geometry(w)[3] for a in inputs) and null.shape == inputs[0].shape
    for w in SCAN_WINDOWS:
        for lag in SCAN_LAGS:
            assert len(scan_combine_case(w, lag)) == len(scan_positions_thin(w))
    for case in WEIGHT_CASES:
        assert [kind for kind, _, _ in weights_case(*case)] == list(KINDS)
    for K, w in LDS_CASES:
        assert lds_case(K, w)[1].shape == (K, TILE + w + 1)
    for lag in LONG_LAGS:
        assert len(long_lag_case(lag)) == 6
    for K in COMPOSITE_KS:
        assert len(composite_case(K)) == 15
    assert stride_case()[2][True].shape == (STRIDE_N, 1)
    for case in CHAIN_CASES:
        assert chain_case(*case)[4]["turnover"].shape == (CHAIN_NG, case[0])
    for case in EDGE_CASES:
        assert edge_case(*case)[4]["value"].shape == (case[2], case[1])
    for case in LAG_CASES:
        assert lag_case(*case)[4]["value"].shape == (LAG_NG, LAG_T)
