"""-m gpu: what the wrappers of polars_quant_amd.api do at the edges of their marshalling -- an empty batch (N = 0, T = 0) and the
optional inputs (benchmark, cap, industry, group, out, trades) given and left out.  The outcomes of the empty calls and the
shapes / dtypes / devices / container kinds of everything returned were recorded from the binding before it got its one call path
(tests/golden/api_edges.json); the non-empty calls are also compared bit for bit with the same call made through the raw lib()
symbol with hand-built ctypes arguments."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden" / "api_edges.json"
N, T, PITCH = 3, 17, 32          # the odd T keeps the input's width and the row pitch apart


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from polars_quant_amd import api
    return api


def describe(r):
    if r is None or isinstance(r, (bool, int, float, str)):
        return r
    if isinstance(r, torch.Tensor):
        return ["tensor", list(r.shape), str(r.dtype), str(r.device)]
    if isinstance(r, np.ndarray):
        return ["ndarray", list(r.shape), str(r.dtype)]
    if isinstance(r, dict):
        return {"dict": {k: describe(v) for k, v in r.items()}}
    if isinstance(r, (tuple, list)):
        return {type(r).__name__: [describe(v) for v in r]}
    return ["object", type(r).__name__]


def outcome(fn):
    from polars_quant_amd._lib import PqError
    try:
        return {"returns": describe(fn())}
    except (PqError, ValueError, TypeError) as e:     # a refusal: its type and message are what the test pins
        if isinstance(e, PqError) and str(e).startswith(("pq status 2:", "pq status 4:")):
            raise       # PQ_ERR_HIP / PQ_ERR_NOMEM is no refusal of the arguments: nothing more goes to the device
        return {"raises": type(e).__name__, "message": str(e)}


def empty_cases(api, n, t):
    """name -> call, every input an all-zero device tensor of n symbols and t days"""
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
    x, u8, i32 = z(n, t), z(n, t, dt=torch.uint8), z(n, t, dt=torch.int32)
    s = z(t)
    rule = {"rule": [0], "a": [0], "b": [1]}
    return {
        "count_nulls": lambda: api.count_nulls(x),
        "call_sma": lambda: api.call("sma", x, timeperiod=3),
        "call_macd": lambda: api.call("macd", x),
        "cdl": lambda: api.cdl("cdlengulfing", x, x, x, x),
        "cdl_all": lambda: api.cdl_all(x, x, x, x, names=["cdldoji", "cdlharami"]),
        "backtest_vectorized": lambda: api.backtest_vectorized(x, u8, u8),
        "backtest_vectorized_no_curves": lambda: api.backtest_vectorized(x, u8, u8, want_curves=False),
        "backtest_macd_cross": lambda: api.backtest_macd_cross(x),
        "macd_cross_signals": lambda: api.macd_cross_signals(x),
        "factor_ic": lambda: api.factor_ic(x, x),
        "rolling_ic": lambda: api.rolling_ic(s, 3),
        "factor_quantiles": lambda: api.factor_quantiles(x, x, labels=True),
        "factor_long_short": lambda: api.factor_long_short(x, x),
        "factor_coverage": lambda: api.factor_coverage(x),
        "ic_stats": lambda: api.ic_stats(s),
        "factor_clean": lambda: api.factor_clean(x, winsorize="mad", cap=x + 1.0, industry=z(n, dt=torch.int64), standardize=True),
        "xsec_regress": lambda: api.xsec_regress([x, x], x),
        "ts_regress": lambda: api.ts_regress([x, s], x),
        "corr_t_test": lambda: api.corr_t_test(s, z(t, dt=torch.int32)),
        "linear": lambda: api.linear([x, x], x),
        "factor_orthogonalize": lambda: api.factor_orthogonalize([x, x]),
        "ic_decay": lambda: api.ic_decay(x, x, max_lag=2),
        "ic_subgroup": lambda: api.ic_subgroup(x, x, z(n, dt=torch.int64)),
        "factor_rank": lambda: api.factor_rank(x),
        "factor_minmax": lambda: api.factor_normalize(x, "minmax"),
        "factor_weighted": lambda: api.factor_weighted(x, x, group=z(n, t, dt=torch.int64)),
        "factor_binary": lambda: api.factor_binary(x, x),
        "factor_rolling": lambda: api.factor_rolling(x, 0, 3),
        "series_split_summary": lambda: api.series_split_summary(s, 1),
        "cross_signals": lambda: api.cross_signals(x, x),
        "band_signals": lambda: api.band_signals(x, 0.0, 1.0),
        "channel_signals": lambda: api.channel_signals(x, x, x, 0),
        "gate_signals": lambda: api.gate_signals(u8, u8, x, 0, c=x),
        "zscore": lambda: api.zscore(x, x, x),
        "scale_band": lambda: api.scale_band(x, 0.9, 1.1),
        "volume_surge_signals": lambda: api.volume_surge_signals(x, x, x, 2.0),
        "gap_signals": lambda: api.gap_signals(x, x, x, 0.01, 0.01),
        "pattern_any_signals": lambda: api.pattern_any_signals([i32], [i32]),
        "ma_stack_signals": lambda: api.ma_stack_signals([x, x, x]),
        "backtest_leveraged": lambda: api.backtest_leveraged(x, u8, u8),
        "portfolio_metrics": lambda: api.portfolio_metrics(x, 1e5),
        "backtest_report": lambda: api.backtest_report(x, 1e5),
        "backtest_sequential": lambda: api.backtest_sequential(z(n, t + 1, dt=torch.int64), z(0, dt=torch.int32), z(0), z(0), 4),
        "backtest_sweep": lambda: api.backtest_sweep(x, [x, x], rule),
        "backtest_sweep_rules": lambda: api.backtest_sweep_rules(x, [x, x], rule),
    }


# ---- the non-empty calls: with and without their optional inputs, through the wrapper and through the raw symbol

def P(t):
    return C.c_void_p(t.data_ptr())


def pitched(a, dtype=torch.float64):
    """a host [n, t] array as a device view at the row pitch PITCH, which the wrappers use in place"""
    a = np.asarray(a)
    buf = torch.zeros((a.shape[0], PITCH), dtype=dtype, device="cuda")
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dtype)
    return buf[:, :a.shape[1]]


def dense(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def make_data():
    rng = np.random.default_rng(0xED6E)
    price = 50.0 + rng.normal(size=(N, T)).cumsum(axis=1)
    return dict(price=price, buy=rng.random((N, T)) < 0.3, sell=rng.random((N, T)) < 0.3, bench=100.0 + rng.normal(size=T).cumsum(),
                f=rng.normal(size=(3, N, T)), cap=np.exp(rng.normal(size=(N, T)) + 10.0), w=rng.random((N, T)) + 0.5,
                industry=np.array([0, 1, 0]), group=rng.integers(0, 2, size=(N, T)))


@pytest.fixture(scope="module")
def data():
    return make_data()


def raw_ctx(api):
    from polars_quant_amd._lib import lib
    L = lib()

    def ck(st):
        assert st == 0, L.pq_last_error().decode()
    return L, api.ctx(0), ck


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    v = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return bool((a.contiguous().view(v) == b.contiguous().view(v)).all())


def walk_equal(got, exp):
    if isinstance(exp, dict):
        assert isinstance(got, dict) and list(got) == list(exp)
        return all(walk_equal(got[k], exp[k]) for k in exp)
    if isinstance(exp, (tuple, list)):
        assert type(got) is type(exp) and len(got) == len(exp)
        return all(walk_equal(g, e) for g, e in zip(got, exp))
    if exp is None:
        return got is None
    return same_bits(got, exp)


def _bt_vectorized(api, d, with_opt):
    from polars_quant_amd._lib import Batch, BtParams
    from polars_quant_amd._spec import BT_DEFAULTS
    L, h, ck = raw_ctx(api)
    p, bu, se = pitched(d["price"]), dense(d["buy"], torch.uint8), dense(d["sell"], torch.uint8)
    bm = dense(d["bench"]) if with_opt else None
    got = api.backtest_vectorized(p, bu, se, benchmark=bm)
    pc = p.contiguous()
    bmc = bm[None, :].expand(N, T).contiguous() if with_opt else None
    pos, cash, eq = (torch.empty((N, T), dtype=torch.float64, device="cuda") for _ in range(3))
    summ = torch.empty((N, 8), dtype=torch.float64, device="cuda")
    b, prm = Batch(N, T, T), BtParams(**BT_DEFAULTS)
    ck(L.pq_backtest_vectorized(h, C.byref(b), P(pc), P(bu), P(se), P(bmc) if with_opt else None, C.byref(prm), P(pos), P(cash), P(eq),
                                P(summ)))
    return got, (pos, cash, eq, summ)


def _lev_raw(api, d, with_opt):
    from polars_quant_amd._lib import Batch, LevParams
    from polars_quant_amd._spec import LEV_DEFAULTS, TRADE_FIELDS
    L, h, ck = raw_ctx(api)
    p, bu, se = dense(d["price"]), dense(d["buy"], torch.uint8), dense(d["sell"], torch.uint8)
    bm = dense(d["bench"]) if with_opt else None
    mk = lambda: torch.empty((N, T), dtype=torch.float64, device="cuda")
    cash, sv, tv = mk(), mk(), mk()
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    tr = {k: torch.zeros((N, 64), dtype=torch.int32 if k in ("entry_day", "exit_day", "reason") else torch.float64, device="cuda")
          for k in TRADE_FIELDS}
    summ = torch.empty((N, 8), dtype=torch.float64, device="cuda")
    b, prm = Batch(N, T, T), LevParams(**LEV_DEFAULTS)
    ck(L.pq_backtest_leveraged(h, C.byref(b), P(p), P(bu), P(se), P(bm) if with_opt else None, C.byref(prm), P(cash), P(sv), P(tv),
                               C.c_int32(64), P(cnt), *[P(tr[k]) for k in TRADE_FIELDS], P(summ)))
    return (p, bu, se, bm), dict(cash=cash, stock_value=sv, total_value=tv, trade_count=cnt, trades=tr, summary=summ)


def _bt_leveraged(api, d, with_opt):
    (p, bu, se, bm), exp = _lev_raw(api, d, with_opt)
    return api.backtest_leveraged(p, bu, se, benchmark=bm), exp


def _bt_report(api, d, with_opt):
    from polars_quant_amd._lib import Batch, LevParams
    from polars_quant_amd._spec import LEV_DEFAULTS, REPORT_COLS, REPORT_TRADE_FIELDS
    L, h, ck = raw_ctx(api)
    (_p, _bu, _se, bm), lev = _lev_raw(api, d, True)
    tv = lev["total_value"]
    got = api.backtest_report(tv, 1e5, benchmark=bm, trades=lev["trades"], trade_count=lev["trade_count"]) if with_opt else \
        api.backtest_report(tv, 1e5)
    out = torch.empty((N, len(REPORT_COLS)), dtype=torch.float64, device="cuda")
    b, prm = Batch(N, T, T), LevParams(**LEV_DEFAULTS)
    rec = [P(lev["trades"][k]) if with_opt else None for k in REPORT_TRADE_FIELDS]
    ck(L.pq_backtest_report(h, C.byref(b), P(tv), C.c_double(1e5), P(bm) if with_opt else None, C.byref(prm),
                            C.c_int32(64 if with_opt else 0), P(lev["trade_count"]) if with_opt else None, *rec, P(out)))
    return got, out


def _factor_clean(api, d, with_opt):
    from polars_quant_amd._lib import Batch
    L, h, ck = raw_ctx(api)
    f, cap = pitched(d["f"][0]), pitched(d["cap"])
    got = api.factor_clean(f, winsorize="mad", cap=cap, industry=d["industry"], standardize=True) if with_opt else \
        api.factor_clean(f, winsorize="mad", standardize=True)
    z = torch.empty_strided(f.shape, f.stride(), dtype=torch.float64, device="cuda")
    torch.log(cap, out=z)
    ib = torch.empty((N, PITCH), dtype=torch.int32, device="cuda")
    ib[:, :T] = torch.from_numpy(d["industry"]).to(device="cuda", dtype=torch.int32)[:, None]
    out = torch.empty((N, PITCH), dtype=torch.float64, device="cuda")
    b = Batch(N, T, PITCH)
    ck(L.pq_factor_clean(h, C.byref(b), P(f), C.c_int32(1), C.c_double(3.0), P(z) if with_opt else None, P(ib) if with_opt else None,
                         C.c_int32(2 if with_opt else 0), C.c_int32(1), P(out)))
    return got, out[:, :T]


def _factor_weighted(api, d, with_opt):
    from polars_quant_amd._lib import Batch
    L, h, ck = raw_ctx(api)
    f, w = pitched(d["f"][0]), pitched(d["w"])
    got = api.factor_weighted(f, w, group=d["group"] if with_opt else None)
    g = pitched(d["group"], torch.int32)
    out = torch.empty((N, PITCH), dtype=torch.float64, device="cuda")
    b = Batch(N, T, PITCH)
    ck(L.pq_factor_weighted(h, C.byref(b), P(f), P(w), P(g) if with_opt else None, C.c_int64(PITCH if with_opt else 0),
                            C.c_int32(int(d["group"].max()) + 1 if with_opt else 0), P(out)))
    return got, out[:, :T]


def _factor_orth(api, d, with_opt):
    from polars_quant_amd._lib import Batch
    L, h, ck = raw_ctx(api)
    fs = [pitched(d["f"][k]) for k in range(3)]
    outs = [pitched(np.zeros((N, T))) for _ in range(2)]
    got = api.factor_orthogonalize(fs, out=outs if with_opt else None)
    if with_opt:
        assert isinstance(got, list) and all(g is o for g, o in zip(got, outs))
    exp = [pitched(np.zeros((N, T))) for _ in range(2)]
    fp = (C.c_void_p * 3)(*[t.data_ptr() for t in fs])
    op = (C.c_void_p * 2)(*[t.data_ptr() for t in exp])
    b = Batch(N, T, PITCH)
    ck(L.pq_factor_orthogonalize(h, C.byref(b), fp, C.c_int32(3), C.c_int32(0), op))
    return got, exp if with_opt else torch.stack(exp)


def _bt_sweep(api, d, with_opt, rules=False):
    from polars_quant_amd._lib import Batch, BtParams
    from polars_quant_amd._spec import BT_DEFAULTS
    L, h, ck = raw_ctx(api)
    p, lines = pitched(d["price"]), [pitched(d["price"] + k) for k in (0.5, -0.5)]
    if rules:       # a breakout of the price from the channel (lines[1], lines[0]), and a band
        tab = api.sweep_rules({"rule": [3, 1], "a": [1, 0], "b": [0, 0], "c": [-1, 0], "k0": [0.0, 45.0], "k1": [0.0, 55.0]})
    else:
        tab = api.sweep_params({"rule": [0, 1], "a": [0, 0], "b": [1, 0], "k0": [0.0, 45.0], "k1": [0.0, 55.0]})
    wrapper, entry = (api.backtest_sweep_rules, "pq_backtest_sweep_rules") if rules else (api.backtest_sweep, "pq_backtest_sweep")
    bm = dense(d["bench"]) if with_opt else None
    mine = torch.empty((N, 2, 8), dtype=torch.float64, device="cuda") if with_opt else None
    got = wrapper(p, lines, tab, benchmark=bm, out=mine)
    if with_opt:
        assert got.data_ptr() == mine.data_ptr()
    out = torch.empty((N, 2, 8), dtype=torch.float64, device="cuda")
    dtab = torch.from_numpy(tab.view(np.uint8).reshape(2, 32)).to("cuda")
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in lines])
    b, prm = Batch(N, T, PITCH), BtParams(**BT_DEFAULTS)
    ck(getattr(L, entry)(h, C.byref(b), P(p), ptrs, C.c_int32(2), P(dtab), C.c_int64(2), P(bm) if with_opt else None, C.c_int64(0),
                         C.byref(prm), P(out)))
    return got, out.permute(1, 0, 2)


def _bt_sweep_rules(api, d, with_opt):
    return _bt_sweep(api, d, with_opt, rules=True)


def _portfolio_metrics(api, d, with_opt):
    from polars_quant_amd._lib import Batch
    L, h, ck = raw_ctx(api)
    tv, bm = pitched(1000.0 * d["price"]), dense(d["bench"]) if with_opt else None
    got = api.portfolio_metrics(tv, 3e5, benchmark=bm)
    tvc = tv.contiguous()
    out = torch.zeros((T, 10), dtype=torch.float64, device="cuda")
    b = Batch(N, T, T)
    ck(L.pq_portfolio_metrics(h, C.byref(b), P(tvc), C.c_double(3e5), P(bm) if with_opt else None, P(out)))
    return got, out


def _bt_sequential(api, d, with_opt):
    """three tapes over one list of 20 orders on 4 assets, two parameter sets short of one per tape: one dict for all"""
    from polars_quant_amd._lib import SeqParams
    from polars_quant_amd._spec import SEQ_DEFAULTS
    L, h, ck = raw_ctx(api)
    rng = np.random.default_rng(0x5E9)
    A, n_orders = 4, 20
    off = np.sort(rng.integers(0, n_orders + 1, size=(N, T + 1)), axis=1)
    off[:, 0], off[:, -1] = 0, n_orders
    asset = rng.integers(0, A, size=n_orders).astype(np.int32)
    qty = rng.integers(1, 50, size=n_orders) * rng.choice([1.0, 1.0, -1.0], size=n_orders)
    px = 20.0 + 5.0 * rng.random(n_orders)
    prm = {"buy_slippage": 0.001}
    shapes = dict(equity=((N, T), torch.float64), cash=((N, T), torch.float64), position=((N, A), torch.float64),
                  counts=((N, 2), torch.int64), summary=((N, 8), torch.float64))
    mk = lambda: {k: torch.zeros(shp, dtype=dt, device="cuda") for k, (shp, dt) in shapes.items()}
    mine = mk() if with_opt else None
    got = api.backtest_sequential(off, asset, qty, px, A, benchmark=d["bench"] if with_opt else None, params=prm, out=mine)
    if with_opt:
        assert all(got[k] is mine[k] for k in shapes)
    exp = mk()
    o_d, a_d, q_d, p_d = dense(off, torch.int64), dense(asset, torch.int32), dense(qty), dense(px)
    bm = dense(d["bench"]) if with_opt else None
    sp = (SeqParams * 1)(SeqParams(**{**SEQ_DEFAULTS, **prm}))
    ck(L.pq_backtest_sequential(h, C.c_int64(N), C.c_int64(T), C.c_int32(A), P(o_d), P(a_d), P(q_d), P(p_d), C.c_int64(n_orders),
                                P(bm) if with_opt else None, sp, C.c_int64(1), *[P(exp[k]) for k in shapes]))
    return got, exp


OPTIONAL = {"backtest_vectorized": _bt_vectorized, "backtest_leveraged": _bt_leveraged, "backtest_report": _bt_report,
            "factor_clean": _factor_clean, "factor_weighted": _factor_weighted, "factor_orthogonalize": _factor_orth,
            "backtest_sweep": _bt_sweep, "backtest_sweep_rules": _bt_sweep_rules, "portfolio_metrics": _portfolio_metrics,
            "backtest_sequential": _bt_sequential}


def record(api, data):
    """everything tests/golden/api_edges.json holds: this function was run on the binding as it stood before the one call path and
    its result dumped as JSON"""
    rec = {}
    for tag, (n, t) in (("N=0", (0, 5)), ("T=0", (3, 0))):
        for name, fn in empty_cases(api, n, t).items():
            rec[f"{name}[{tag}]"] = outcome(fn)
    for name, fn in OPTIONAL.items():
        for with_opt in (False, True):
            rec[f"{name}[{'with' if with_opt else 'without'}]"] = {"returns": describe(fn(api, data, with_opt)[0])}
    torch.cuda.synchronize()
    return rec


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("tag,n,t", [("N=0", 0, 5), ("T=0", 3, 0)])
def test_empty_batches_behave_as_recorded(api, golden, tag, n, t):
    cases = empty_cases(api, n, t)
    assert sorted(f"{k}[{tag}]" for k in cases) == sorted(k for k in golden if k.endswith(f"[{tag}]"))
    got = {f"{k}[{tag}]": outcome(fn) for k, fn in cases.items()}
    torch.cuda.synchronize()
    bad = {k: (v, golden[k]) for k, v in got.items() if v != golden[k]}
    assert not bad, bad


@pytest.mark.parametrize("with_opt", [False, True], ids=["without", "with"])
@pytest.mark.parametrize("name", sorted(OPTIONAL))
def test_optional_inputs_match_the_raw_call(api, golden, data, name, with_opt):
    got, exp = OPTIONAL[name](api, data, with_opt)
    torch.cuda.synchronize()
    assert {"returns": describe(got)} == golden[f"{name}[{'with' if with_opt else 'without'}]"]
    assert walk_equal(got, exp)
