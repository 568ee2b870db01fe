"""-m gpu: the walk-forward sweep (csrc/sweep/sweep.hip, decision D-26) -- pq_backtest_sweep_windows, pq_sweep_select and
ParameterSweep.walk_forward.

Window w of a windowed sweep is BIT FOR BIT the plain sweep of contiguous copies of the rows [t0, t1) (the same arithmetic, the same
device pow, no contraction: no tolerance), and -- independently of the old kernel -- the CPU oracle's summary of the sliced arrays under
check_summary (max_drawdown, max_profit, win_rate, total_trades bit for bit, the others at rtol 1e-12 / atol 1e-13).  The selection is
compared bit for bit with test_sweep_windows_ref.select_ref.

Shapes: N <= 9 symbols, T <= 3 R + 5 rows (R = api.SWEEP_ROW_TILE(L)); window lengths 1, 2, R - 1, R, R + 1 and 3 R + 5, starts 0, 1, odd
offsets, windows ending at T, overlapping, identical and empty ones; W in {1, 2, 7}, P in {1, 65, 257} (257: a second workgroup per
symbol and window), L in {7, 79}."""
import ctypes as C

import numpy as np
import pytest

import sweep_rules_ref as S
import test_sweep_gpu as G
import test_sweep_rules_gpu as RG
from test_backtest_wave_gpu import bits, special_prices
from test_sweep_windows_ref import select_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SEED = 0x5EED0003
dev = RG.dev


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()
    return pq


_data = {}


def data(oracle, N, T, L):
    """close, per-symbol benchmark and the lines of a shape, computed once and never changed"""
    if (N, T, L) not in _data:
        d = oracle.gen_ohlcv(SEED, N, T, 0)
        close, bench = d["close"], d["open"]
        lines = S.make_lines(close, L)
        for a in [close, bench] + lines:
            a.setflags(write=False)
        _data[(N, T, L)] = close, bench, lines
    return _data[(N, T, L)]


def windowed(price, lines, tab, windows, benchmark=None, **kw):
    """-> [W, P, N, 8] host array of api.backtest_sweep_rules(..., windows=); checks that it is the permuted view of [W, N, P, 8]"""
    from polars_quant_amd import api
    got = api.backtest_sweep_rules(dev(price), [dev(l) for l in lines], tab, windows=np.asarray(windows, dtype=np.int64),
                                   **({} if benchmark is None else {"benchmark": dev(benchmark)}), **kw)
    W, P, N = len(windows), len(tab), price.shape[0]
    assert tuple(got.shape) == (W, P, N, 8) and got.stride() == (8 * N * P, 8, 8 * P, 1)
    return got.cpu().numpy()


def sliced(price, lines, tab, t0, t1, benchmark=None, **kw):
    """the plain sweep on contiguous copies of the rows [t0, t1) of every column -> [P, N, 8]; of no rows: zeros (metrics.rs:17-19)"""
    if t0 == t1:
        return np.zeros((len(tab), price.shape[0], 8))
    cut = lambda x: np.ascontiguousarray(x[..., t0:t1])
    return RG.run(cut(price), [cut(l) for l in lines], tab, **({} if benchmark is None else {"benchmark": dev(cut(benchmark))}), **kw)


def assert_windows_equal_slices(price, lines, tab, windows, benchmark, tag):
    got = windowed(price, lines, tab, windows, benchmark)
    for w, (t0, t1) in enumerate(windows):
        exp = sliced(price, lines, tab, t0, t1, benchmark)
        assert (bits(got[w]) == bits(exp)).all(), (tag, w, (t0, t1), np.argwhere(bits(got[w]) != bits(exp))[:3].tolist())
    return got


def window_lists(R, T):
    """two lists of seven windows: (a) the lengths 3 R + 5 ([0, T) itself), 1, 2, R - 1, R, R + 1 at the starts 0, 1, odd offsets and ending
    at T, all overlapping; (b) two identical windows, an empty one between two live ones, an empty one at T, one row ending at T"""
    a = [(0, T), (1, 2), (7, 9), (T - (R - 1), T), (0, R), (13, 13 + R + 1), (1, T)]
    b = [(5, 5 + R + 1), (5, 5 + R + 1), (20, 20), (0, 2), (T - 1, T), (T, T), (3, 3 + 2 * R)]
    return a, b


# ---- 1. bit for bit with the plain sweep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bench", [False, True], ids=["plain", "bench"])
@pytest.mark.parametrize("which", RG.TABLES)
def test_every_table_equals_the_plain_sweep_of_the_slices(pq, oracle, which, with_bench):
    N, L, P = 3, 7, 65
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, lines = data(oracle, N, T, L)
    tab = RG.table(P, L, which)
    for k, wins in enumerate(window_lists(R, T)):
        assert sorted({t1 - t0 for t0, t1 in wins} & {1, 2, R - 1, R, R + 1, T}) == ([1, 2, R - 1, R, R + 1, T] if k == 0 else [1, 2, R + 1])
        got = assert_windows_equal_slices(close, lines, tab, wins, bench if with_bench else None, f"{which} list {k}")
        if k == 0:      # not vacuous: the long windows trade, and the benchmark reaches alpha and beta
            assert (got[0, ..., 7] >= 1).mean() >= 0.5 and (got[6, ..., 7] >= 1).mean() >= 0.5
            assert ((got[0, ..., 3] != 0).mean() > 0.4) == with_bench
        else:           # the empty windows are zeros (metrics.rs:17-19), between live ones
            assert (got[2] == 0).all() and (got[5] == 0).all() and (got[1, ..., 7] >= 1).any() and (got[6, ..., 7] >= 1).any()
            assert (bits(got[0]) == bits(got[1])).all()


@pytest.mark.parametrize("L", [7, 79])
@pytest.mark.parametrize("P", [1, 65, 257])
@pytest.mark.parametrize("W", [1, 2, 7])
def test_window_counts_parameter_sets_and_lines(pq, oracle, W, P, L):
    N = 3
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, lines = data(oracle, N, T, L)
    tab = RG.table(P, L, "mixed")
    if L == 79:         # every other set reads the last lines (70 = 0 mod 7: the same family)
        for f in ("a", "b", "c"):
            tab[f][(tab[f] >= 0) & (tab[f] < 7) & (np.arange(P) % 2 == 1)] += 70
    a, b = window_lists(R, T)
    wins = {1: [a[5]], 2: [a[3], b[2]], 7: a}[W]          # one odd start; one ending at T and an empty one; the seven of list (a)
    assert_windows_equal_slices(close, lines, tab, wins, bench, f"W={W} P={P} L={L}")


def test_the_two_rule_table_and_a_shared_benchmark(pq, oracle):
    """api.backtest_sweep(windows=) (the pq_sweep_param table: cross and band) against api.backtest_sweep on the slices, with one [T]
    benchmark shared by all symbols; a rule beyond 1 stays refused"""
    from polars_quant_amd import api
    N, L, P = 3, 7, 130
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, _ = data(oracle, N, T, L)
    lines, tab = G.make_lines(N, T, L), G.make_table(api, P, L)
    shared = np.ascontiguousarray(bench[1])
    wins, _b = window_lists(R, T)
    got = api.backtest_sweep(dev(close), [dev(l) for l in lines], tab, benchmark=dev(shared), windows=wins)
    assert tuple(got.shape) == (7, P, N, 8)
    got = got.cpu().numpy()
    for w, (t0, t1) in enumerate(wins):
        exp = G.run(api, close[:, t0:t1], [l[:, t0:t1] for l in lines], tab, benchmark=dev(np.ascontiguousarray(shared[t0:t1])))
        assert (bits(got[w]) == bits(exp)).all(), w
    bad = tab.copy()
    bad["rule"][3] = 2
    with pytest.raises(pq.PqError, match="rule"):
        api.backtest_sweep(dev(close), [dev(l) for l in lines], bad, windows=wins)


# ---- 2. against the CPU oracle, independently of the old kernel -------------------------------------------------------------------------
def test_windows_against_the_oracle(pq, oracle):
    from polars_quant_amd import api
    N, L, P = 9, 7, 65
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, rlines = data(oracle, N, T, L)
    wins = [(0, R + 1), (1, R + 2), (37, 37 + R + 1), (T - (R + 1), T)]
    # the two-rule table on the oscillating lines of test_sweep_gpu: most cells trade at least twice inside a window of R + 1 rows
    lines, tab = G.make_lines(N, T, L), G.make_table(api, P, L)
    got = api.backtest_sweep(dev(close), [dev(l) for l in lines], tab, windows=wins).cpu().numpy()
    exp = np.stack([G.oracle_cells(oracle, np.ascontiguousarray(close[:, t0:t1]), [np.ascontiguousarray(l[:, t0:t1]) for l in lines], tab)
                    for t0, t1 in wins])
    assert (exp[:, tab["a"] != tab["b"], :, 7] >= 2).mean() > 0.9, (exp[:, tab["a"] != tab["b"], :, 7] >= 2).mean()
    for w in range(len(wins)):
        G.check_cells(got[w], exp[w], f"two rules, window {wins[w]}")
    assert (bits(exp[0]) != bits(exp[1])).any() and (bits(exp[0]) != bits(exp[2])).any()      # the windows differ
    # all seven rules, mixed, with a per-symbol benchmark
    tab = RG.table(P, L, "mixed")
    got = windowed(close, rlines, tab, wins, bench)
    for w, (t0, t1) in enumerate(wins):
        cut = lambda x: np.ascontiguousarray(x[:, t0:t1])
        exp_w = S.oracle_cells(oracle, cut(close), [cut(l) for l in rlines], tab, benchmark=cut(bench))
        RG.check_cells(got[w], exp_w, f"seven rules, window {(t0, t1)}")
        assert (exp_w[..., 7] >= 1).mean() >= 0.5


# ---- 3. row t0 - 1 is not read --------------------------------------------------------------------------------------------------------
def test_a_cross_between_rows_t0_minus_1_and_t0_is_not_seen(pq, oracle):
    """lines[0] crosses lines[1] exactly between rows t0 - 1 and t0 and never again: the window [t0, t1) does not trade, the window
    that starts one row earlier buys on row t0.  The same for the breakout rule, whose channel is row t - 1's: the only low `hi` is
    at row t0 - 1."""
    from polars_quant_amd import api
    N, T, t0, t1 = 3, 60, 23, 51
    close = oracle.gen_ohlcv(SEED, N, T, 0)["close"]
    up = np.where(np.arange(T) >= t0, 1.0, -1.0)[None, :].repeat(N, 0)           # -1 up to row t0 - 1, +1 from row t0 on
    zero = np.zeros((N, T))
    hi = np.full((N, T), 1e9)
    hi[:, t0 - 1] = 0.0                                                          # the close (> 0) breaks out of row t0 - 1's channel only
    lo = np.full((N, T), -1e9)
    lines = [up, zero, lo, hi]
    tab = np.zeros(2, dtype=api.SWEEP_RULE_DTYPE)
    tab["rule"], tab["a"], tab["b"], tab["c"] = [S.CROSS, S.BREAKOUT], [0, 2], [1, 3], -1
    wins = [(t0, t1), (t0 - 1, t1), (0, T), (t0, t0 + 1), (t0 + 1, t1)]
    exp = np.stack([S.oracle_cells(oracle, np.ascontiguousarray(close[:, a:b]), [np.ascontiguousarray(l[:, a:b]) for l in lines], tab) for a, b in wins])
    assert (exp[[0, 3, 4], ..., 7] == 0).all() and (exp[[1, 2], ..., 7] == 1).all()    # the oracle on the slices says the same
    got = assert_windows_equal_slices(close, lines, tab, wins, None, "cross at t0")
    assert (got[..., 7] == exp[..., 7]).all()
    for w in range(len(wins)):
        RG.check_cells(got[w], exp[w], f"cross at t0, window {wins[w]}")
    # the two-rule entry point reads no row t0 - 1 either
    old = np.zeros(1, dtype=api.SWEEP_PARAM_DTYPE)
    old["a"], old["b"] = 0, 1
    g2 = api.backtest_sweep(dev(close), [dev(l) for l in lines], old, windows=wins).cpu().numpy()
    assert (bits(g2[:, 0]) == bits(got[:, 0])).all()


@pytest.mark.parametrize("which", ["mixed", 3])
def test_null_and_nan_rows_at_the_window_edges(pq, oracle, which):
    """special_prices: symbol 2 is NULL on rows T/3 .. T/3 + 4, symbol 4 is NaN on row T/2, symbol 7 is NULL on every third row, symbol 3
    starts with NULLs; the lines carry NULL lead-ins and interior NULLs.  Windows whose rows t0 - 1, t0 and t1 - 1 are such rows, against
    the plain sweep of the slices, bit for bit with the NaN cells included, and against the oracle"""
    N, L, P = 9, 7, 65
    T = 3 * RG.row_tile(L) + 5
    d, price = special_prices(oracle, N, T)
    a, h = T // 3, T // 2
    assert bits(price[2, a: a + 5]).tolist() == [S.NULL_BITS] * 5 and np.isnan(price[4, h]) and bits(price[7, 0]) == S.NULL_BITS
    lines = S.add_nulls(S.make_lines(price, L), N)
    bench = d["open"]
    tab = RG.table(P, L, which)
    wins = [(a + 1, h + 1),       # NULL at t0 - 1 and t0 (symbol 2), NaN at t1 - 1 (symbol 4)
            (a, a + 5),           # NULL rows only (symbol 2)
            (a + 5, h),           # NULL at t0 - 1, NaN just behind the window
            (h, T),               # NaN at t0
            (h + 1, T),           # NaN at t0 - 1: symbol 4 is clean inside
            (1, 3 * 13 + 1),      # symbol 7: NULL at t0 - 1 and at t1 - 1
            (0, T)]
    got = windowed(price, lines, tab, wins, bench)
    for w, (t0, t1) in enumerate(wins):
        cut = lambda x: np.ascontiguousarray(x[:, t0:t1])
        exp = sliced(price, lines, tab, t0, t1, bench)
        assert (bits(got[w]) == bits(exp)).all(), (w, np.argwhere(bits(got[w]) != bits(exp))[:3].tolist())
        RG.check_cells(got[w], S.oracle_cells(oracle, cut(price), [cut(l) for l in lines], tab, benchmark=cut(bench)), f"special, window {(t0, t1)}")
    assert np.isnan(got[3][:, 4]).any() and np.isfinite(got[4][:, 4]).all()        # the NaN of row h reaches window (h, T) only


# ---- 4. the selection -------------------------------------------------------------------------------------------------------------------
def select(summary, train, test, metric, maximize):
    from polars_quant_amd import api
    chosen, ins, outs = api.sweep_select(summary, train, test, metric, maximize)
    F, N = len(train), summary.shape[2]
    assert chosen.dtype == torch.int32 and tuple(chosen.shape) == (F, N) and tuple(ins.shape) == tuple(outs.shape) == (F, N, 8)
    return chosen.cpu().numpy(), ins.cpu().numpy(), outs.cpu().numpy()


def assert_select(summary, train, test, col, maximize, tag):
    from polars_quant_amd._spec import SUMMARY_KEYS
    got = select(summary, train, test, SUMMARY_KEYS[col], maximize)
    exp = select_ref(summary.cpu().numpy(), train, test, col, maximize)
    assert (got[0] == exp[0]).all(), (tag, np.argwhere(got[0] != exp[0])[:3].tolist())
    assert (bits(got[1]) == bits(exp[1])).all() and (bits(got[2]) == bits(exp[2])).all(), tag
    return exp


@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
def test_select_on_a_windowed_summary(pq, oracle, P):
    from polars_quant_amd import api
    N, L = 9, 7
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, lines = data(oracle, N, T, L)
    wins = [(0, R), (R, R + 30), (20, 20 + R), (20 + R, T), (0, 2 * R), (2 * R, T)]
    summ = api.backtest_sweep_rules(dev(close), [dev(l) for l in lines], RG.table(P, L, "mixed"), benchmark=dev(bench), windows=wins)
    train, test = [0, 2, 4, 0], [1, 3, 5, 5]                       # train window 0 serves two folds
    for col in range(8):
        for maximize in (True, False):
            exp = assert_select(summ, train, test, col, maximize, f"P={P} col={col} max={maximize}")
            if col == 7 and maximize and P >= 63:                   # total_trades: ties, and a choice that moves
                m = summ.cpu().numpy()[train, :, :, 7]                                  # [F, P, N]
                assert ((m == m.max(axis=1, keepdims=True)).sum(axis=1) >= 2).any(), "no (fold, symbol) maximum is a tie"
                assert len(set(exp[0].ravel().tolist())) >= 3 and (exp[0] != 0).any()
    # an integer column works like its name
    a, b = select(summ, train, test, 4, True), select(summ, train, test, "sharpe_ratio", True)
    assert (a[0] == b[0]).all() and (bits(a[2]) == bits(b[2])).all()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
def test_select_on_nans_and_infinities(pq, P):
    W, N = 4, 9
    rng = np.random.default_rng(P)
    s = rng.integers(-3, 4, size=(W, P, N, 8)).astype(np.float64)          # small integers: ties everywhere
    s[rng.random(s.shape) < 0.2] = np.nan
    s[rng.random(s.shape) < 0.05] = np.inf
    s[rng.random(s.shape) < 0.05] = -np.inf
    s[1, :, 3, :] = np.nan                                                 # all-NaN (f, s) columns: index 0
    s[2, :, 5, 4] = np.nan
    s[0, :, 0, :] = -np.inf                                                # a column of ties at the worst value of a maximum
    if P > 1:
        s[0, : P - 1, 1, :] = np.nan                                       # the only number is the last set
        s[0, P - 1, 1, :] = -7.0
    summ = torch.from_numpy(np.ascontiguousarray(s.transpose(0, 2, 1, 3))).cuda().permute(0, 2, 1, 3)      # the view a sweep returns
    train, test = [0, 1, 2, 1, 3], [1, 2, 3, 0, 3]
    for col in range(8):
        for maximize in (True, False):
            exp = assert_select(summ, train, test, col, maximize, f"P={P} col={col} max={maximize}")
            assert (exp[0][[1, 3], 3] == 0).all() and (exp[0][0, 0] == 0)
            if P > 1:
                assert exp[0][0, 1] == P - 1
    # a contiguous [W, P, N, 8] tensor is taken as well (copied into the kernel's layout)
    a = select(summ.contiguous(), train, test, 2, True)
    assert (a[0] == select_ref(s, train, test, 2, True)[0]).all()


# ---- 5. walk_forward against the loop it replaces ----------------------------------------------------------------------------------------
def loop_reference(pq, frame, res_params, lines, tab, folds, metric_col, maximize, runner):
    """lines on the full history, sliced per window; one plain sweep per window; torch argmax / gather"""
    summaries = []
    for t0, t1 in folds.reshape(-1, 2).tolist():
        df = {k: v[:, t0:t1].contiguous() for k, v in frame.items()}
        summaries.append(getattr(pq.ParameterSweep(df), runner)([l[:, t0:t1].contiguous() for l in lines], tab).summary)
    chosen, ins, outs = [], [], []
    for k in range(len(folds)):
        tr, te = summaries[2 * k], summaries[2 * k + 1]
        m = tr[..., metric_col]
        key = torch.where(torch.isnan(m), torch.full_like(m, float("-inf") if maximize else float("inf")), m)
        idx = key.argmax(dim=0) if maximize else key.argmin(dim=0)
        idx = torch.where(torch.isnan(m).all(dim=0), torch.zeros_like(idx), idx)
        g = idx[None, :, None].expand(1, -1, 8)
        chosen.append(idx)
        ins.append(tr.gather(0, g)[0])
        outs.append(te.gather(0, g)[0])
    return torch.stack(summaries), torch.stack(chosen), torch.stack(ins), torch.stack(outs)


def assert_walk_forward(pq, wf, ref, folds, distinct):
    from polars_quant_amd._spec import SUMMARY_KEYS
    summaries, chosen, ins, outs = ref
    F = len(folds)
    assert (wf.folds == folds).all() and tuple(wf.summary.shape) == (2 * F,) + tuple(summaries.shape[1:])
    assert (bits(wf.summary.cpu().numpy()) == bits(summaries.cpu().numpy())).all()
    assert (wf.chosen.cpu().numpy() == chosen.cpu().numpy()).all()
    assert (bits(wf.in_sample.cpu().numpy()) == bits(ins.cpu().numpy())).all()
    assert (bits(wf.out_of_sample.cpu().numpy()) == bits(outs.cpu().numpy())).all()
    for k, name in enumerate(SUMMARY_KEYS):
        assert (bits(wf.metric(name).cpu().numpy()) == bits(outs[..., k].cpu().numpy())).all()
        assert (bits(wf.metric(name, which="in").cpu().numpy()) == bits(ins[..., k].cpu().numpy())).all()
    cp = wf.chosen_params()
    assert sorted(cp) == sorted(wf.params)
    for name, v in cp.items():
        assert v.shape == tuple(chosen.shape) and (v == np.asarray(wf.params[name])[chosen.cpu().numpy()]).all()
    assert len(set(chosen.cpu().numpy().ravel().tolist())) >= distinct       # the choice moves between folds and symbols


@pytest.mark.parametrize("anchored", [False, True])
def test_walk_forward_ma(pq, oracle, anchored):
    from polars_quant_amd import api, sweep
    d = oracle.gen_ohlcv(SEED, 9, 300, 0)
    frame = {k: dev(d[k]) for k in ("open", "high", "low", "close", "volume")}
    periods = (3, 5, 8, 13, 21, 34)
    wf = pq.ParameterSweep(frame).walk_forward("ma", periods, periods, train=100, test=50, anchored=anchored)
    folds = sweep.walk_forward_windows(300, 100, 50, anchored=anchored)
    assert len(folds) == 4 and isinstance(wf, pq.WalkForwardResult)
    ps, tab, params = sweep.ma_grid(periods, periods)
    lines = [api.call("sma", frame["close"], timeperiod=p)[0] for p in ps]
    ref = loop_reference(pq, frame, params, lines, tab, folds, 4, True, "run")
    assert_walk_forward(pq, wf, ref, folds, 3)
    assert sorted(wf.params) == ["fast", "slow"] and (wf.chosen_params()["fast"] < wf.chosen_params()["slow"]).all()


def test_walk_forward_stoch(pq, oracle):
    from polars_quant_amd import api, sweep
    d = oracle.gen_ohlcv(SEED, 9, 300, 0)
    frame = {k: dev(d[k]) for k in ("open", "high", "low", "close", "volume")}
    args = ((5, 9), 3, 3, (20, 30), (70, 80))
    wf = pq.ParameterSweep(frame).walk_forward("stoch", *args, train=120, test=40, step=60, metric="max_drawdown", maximize=False)
    folds = sweep.walk_forward_windows(300, 120, 40, step=60)
    assert len(folds) == 3
    triples, tab, params = sweep.stoch_grid(*args)
    lines = []
    for f, k, dd in triples:
        lines += list(api.call("stoch", frame["high"], frame["low"], frame["close"], fastk_period=f, slowk_period=k, slowd_period=dd))
    ref = loop_reference(pq, frame, params, lines, tab, folds, 1, False, "run_rules")
    assert_walk_forward(pq, wf, ref, folds, 2)
    with pytest.raises(ValueError, match="rule"):
        pq.ParameterSweep(frame).walk_forward("nope", train=10, test=5)
    with pytest.raises(KeyError):
        pq.ParameterSweep(frame).walk_forward("ma", (3, 5), (8, 13), train=100, test=50, metric="nope")
    with pytest.raises(ValueError, match="no fold"):
        pq.ParameterSweep(frame).walk_forward("ma", (3, 5), (8, 13), train=280, test=50)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(pq, oracle):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, BtParams, check, lib
    from polars_quant_amd._spec import BT_DEFAULTS
    N, T, L, P = 3, 60, 7, 65
    close, _bench, lines = data(oracle, N, T, L)
    price, dl = dev(close), [dev(l) for l in lines]
    tab = RG.table(P, L, "mixed")

    def untouched(call, match):
        out = torch.full((2, N, P, 8), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(pq.PqError, match=match):
            call(out)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), "nothing may be launched"
    for bad in ((-1, 5), (0, T + 1), (9, 8)):                                  # t0 < 0, t1 > len, t0 > t1: the message names window 1
        untouched(lambda out: api.backtest_sweep_rules(price, dl, tab, windows=[(0, 10), bad], out=out), "window 1")
    bad_tab = tab.copy()
    bad_tab["a"][35] = L                                                       # the table is still checked (sw_run's checks)
    untouched(lambda out: api.backtest_sweep_rules(price, dl, bad_tab, windows=[(0, 10), (5, 20)], out=out), "parameter set 35")
    with pytest.raises(pq.PqError):
        api.backtest_sweep_rules(price, dl * 80, tab, windows=[(0, 10)])      # more lines than fit
    # n_windows < 0 and a grid beyond 2^31 - 1 blocks, through the C ABI (the table is not read before the size is known to be sane)
    Lb, h, vp = lib(), api.ctx(0), C.c_void_p
    b, prm = Batch(N, T, T), BtParams(**BT_DEFAULTS)
    dtab = torch.from_numpy(tab.view(np.uint8).reshape(P, 32)).cuda()
    ptrs = (vp * L)(*[m.data_ptr() for m in dl])
    one = np.array([[0, 10]], dtype=np.int64)

    def raw(out, n_windows):
        check(Lb.pq_backtest_sweep_windows(h, C.byref(b), vp(price.data_ptr()), ptrs, C.c_int32(L), vp(dtab.data_ptr()), C.c_int64(P),
                                           vp(one.ctypes.data), C.c_int64(n_windows), None, C.c_int64(0), C.byref(prm), vp(out.data_ptr())))
    untouched(lambda out: raw(out, -1), "n_windows")
    untouched(lambda out: raw(out, (2 ** 31 - 1) // N + 1), "2\\^31")
    out = torch.full((2, N, P, 8), 7.0, dtype=torch.float64, device="cuda")
    raw(out, 0)                                                                # no window: nothing is written
    raw(out[1:], 1)
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (bits(out[1].cpu().numpy()) == bits(windowed(close, lines, tab, one)[0].transpose(1, 0, 2))).all()
    # a recording context
    check(Lb.pq_suite_begin(h, C.byref(b)))
    try:
        untouched(lambda out: api.backtest_sweep_rules(price, dl, tab, windows=[(0, 10), (5, 20)], out=out), "recorded")
        with pytest.raises(pq.PqError, match="recorded"):
            api.sweep_select(torch.zeros((2, P, N, 8), dtype=torch.float64, device="cuda"), [0], [1], "alpha")
    finally:
        check(Lb.pq_suite_abort(h))
    # ragged batches
    with pytest.raises(pq.PqError):
        api.backtest_sweep(price.reshape(1, -1), [l.reshape(1, -1) for l in dl], G.make_table(api, P, L), offsets=[0, T, 2 * T, 3 * T], windows=[(0, 10)])
    # empty shapes
    assert tuple(api.backtest_sweep_rules(price, dl, tab, windows=np.zeros((0, 2), dtype=np.int64)).shape) == (0, P, N, 8)
    assert tuple(api.backtest_sweep_rules(price, dl, tab[:0], windows=[(0, 10)]).shape) == (1, 0, N, 8)
    z = api.backtest_sweep_rules(price[:, :0], [l[:, :0] for l in dl], tab, windows=[(0, 0), (0, 0)], out=torch.full((2, N, P, 8), 7.0, dtype=torch.float64, device="cuda"))
    assert tuple(z.shape) == (2, P, N, 8) and (z == 0).all()
    with pytest.raises(ValueError, match="windows"):
        api.backtest_sweep_rules(price, dl, tab, windows=[0, 10])
    # pq_sweep_select
    summ = torch.zeros((3, P, N, 8), dtype=torch.float64, device="cuda")
    for kw, match in ((dict(train=[0], test=[1], metric=8), "metric_col"), (dict(train=[0], test=[1], metric=-1), "metric_col"),
                      (dict(train=[3], test=[1], metric=0), "fold 0"), (dict(train=[0, 1], test=[1, -1], metric=0), "fold 1")):
        with pytest.raises(pq.PqError, match=match):
            api.sweep_select(summ, **kw)
    with pytest.raises(pq.PqError, match="parameter set"):
        api.sweep_select(summ[:, :0], [0], [1], "alpha")
    with pytest.raises(KeyError):
        api.sweep_select(summ, [0], [1], "nope")
    with pytest.raises(ValueError):
        api.sweep_select(summ, [0, 1], [1], "alpha")
    chosen, ins, outs = api.sweep_select(summ, [], [], "alpha")                # no fold: empty results
    assert tuple(chosen.shape) == (0, N) and tuple(ins.shape) == tuple(outs.shape) == (0, N, 8)


# ---- 7. unchanged paths -----------------------------------------------------------------------------------------------------------------
def test_unchanged_paths_and_best_per_window(pq, oracle):
    from polars_quant_amd import api
    from polars_quant_amd.sweep import SweepResult
    N, L, P = 9, 7, 65
    R = RG.row_tile(L)
    T = 3 * R + 5
    close, bench, lines = data(oracle, N, T, L)
    tab = RG.table(P, L, "mixed")
    price, dl = dev(close), [dev(l) for l in lines]
    # windows=None: the tensor of the plain call, and of the one window [0, T)
    plain = api.backtest_sweep_rules(price, dl, tab, benchmark=dev(bench))
    none = api.backtest_sweep_rules(price, dl, tab, benchmark=dev(bench), windows=None)
    assert tuple(none.shape) == (P, N, 8) and none.stride() == (8, 8 * P, 1) and (bits(none.cpu().numpy()) == bits(plain.cpu().numpy())).all()
    RG.check_cells(plain.cpu().numpy(), S.oracle_cells(oracle, close, lines, tab, benchmark=bench), "the plain sweep")
    sw = pq.ParameterSweep({"close": price}, benchmark=dev(bench))
    res = sw.run_rules(dl, tab)
    assert res.windows is None and (bits(res.summary.cpu().numpy()) == bits(plain.cpu().numpy())).all()
    # best() on [P, N, 8] is what it was
    idx, val = res.best("alpha")
    m = res.metric("alpha")
    assert tuple(idx.shape) == (N,) and idx.dtype == torch.int64 and (idx == m.argmax(dim=0)).all() and (val == m.max(dim=0).values).all()
    G.test_best_ranks_nan_last(pq, oracle)
    # best() on [W, P, N, 8] is best() per window
    wins = [(0, T), (3, R), (R, T), (0, T)]
    rw = sw.run_rules(dl, tab, windows=wins)
    assert (rw.windows == np.array(wins)).all() and tuple(rw.summary.shape) == (4, P, N, 8)
    assert (bits(rw.summary[0].cpu().numpy()) == bits(plain.cpu().numpy())).all()
    nan_summary = rw.summary.clone()
    nan_summary[1, :, 2, 4] = float("nan")
    nan_summary[2, ::2, :, 4] = float("nan")
    for summ in (rw.summary, nan_summary):
        for metric, maximize in (("sharpe_ratio", True), ("sharpe_ratio", False), ("total_trades", True)):
            idx, val = SweepResult(rw.params, summ, rw.windows).best(metric, maximize)
            assert tuple(idx.shape) == tuple(val.shape) == (4, N)
            for w in range(4):
                i1, v1 = SweepResult(rw.params, summ[w]).best(metric, maximize)
                assert (idx[w] == i1).all() and (bits(val[w].cpu().numpy()) == bits(v1.cpu().numpy())).all()
    with pytest.raises(ValueError):
        SweepResult({}, rw.summary[:, :0]).best()
