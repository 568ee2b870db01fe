"""-m gpu: the seven rule kernels of csrc/strategy.hip, called through the C ABI with an explicit Batch, against the numpy reference
tests/strategy_ref.py (written from include/pq_hip.h) -- eager and recorded into a suite.

Every output buffer is filled with the poison byte 0xA5 first, padding and a guard tail included: after a call the rows of the batch
equal the reference BIT FOR BIT (signals; f64 columns too, up to the NaN an operation produces -- strategy_ref.same_f64) and every
other byte still holds the poison.  Input padding holds 1e300 / 0xFF, so a row read from it would show.

The recorded chains settle an old finding (profiles/r04-r06_bench_strategy.json: "identical_results": false for stoch -> backtest):
with PQ_BT_WAVES=1 on both sides a replay equals the eager calls in every bit, all eight summary columns included; without it a
recorded backtest runs the one-wave kernel and an eager one the four-wave kernel, whose summary sums (columns 0, 2, 3, 4) are ordered
differently -- those columns are held to the project's 1e-12 bound against the oracle, everything else stays bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import strategy_ref as R
from test_strategy_ref import KATS, assert_kat

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = 0xA5
RAGGED = [0, 1, 1, 4, 260, 517, 520]       # a one-row group, an empty one, groups that straddle a 256-row block
LOOKBACK = ("gate3", "volume_surge", "gap", "ma_stack")


class Env:
    def __init__(self, pq):
        from polars_quant_amd import api
        from polars_quant_amd._lib import Batch, check, lib
        self.pq, self.L, self.h, self.Batch, self.check = pq, lib(), api.ctx(0), Batch, check
        self.keep = []

    def batch(self, lay):
        off = None
        if lay["offsets"] is not None:
            off = torch.from_numpy(np.asarray(lay["offsets"], dtype=np.int64)).cuda()
            self.keep = [off]
        return self.Batch(lay["n"], lay["len"], lay["stride"], None if off is None else off.data_ptr())


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    return Env(pq)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_list(ts):
    return (C.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])


def out_dtypes(rule):
    return {"zscore": (np.float64,), "scale_band": (np.float64, np.float64)}.get(rule, (np.uint8, np.uint8))


def poisoned(size, dtype):
    return torch.full((size * np.dtype(dtype).itemsize,), POISON, dtype=torch.uint8, device="cuda")


def as_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def launch(env, b, case, ins, outs):
    """one C-ABI call; ins: {name: device tensor or None}, outs: device tensors.  -> status"""
    L, h, r, p, bb = env.L, env.h, case["rule"], case["params"], C.byref(b)
    if r.startswith("gate"):
        return L.pq_gate_signals(h, bb, P(ins.get("a")), P(ins.get("c")), p["mode"], C.c_double(p["k0"]), C.c_double(p["k1"]),
                                 P(ins.get("buy_in")), P(ins.get("sell_in")), P(outs[0]), P(outs[1]))
    if r == "zscore":
        return L.pq_zscore(h, bb, P(ins.get("price")), P(ins.get("upper")), P(ins.get("mid")), P(outs[0]))
    if r == "scale_band":
        return L.pq_scale_band(h, bb, P(ins.get("base")), C.c_double(p["f_lo"]), C.c_double(p["f_hi"]), P(outs[0]), P(outs[1]))
    if r == "volume_surge":
        return L.pq_volume_surge_signals(h, bb, P(ins.get("volume")), P(ins.get("avg_volume")), P(ins.get("close")), C.c_double(p["multiplier"]),
                                         P(outs[0]), P(outs[1]))
    if r == "gap":
        return L.pq_gap_signals(h, bb, P(ins.get("open")), P(ins.get("high")), P(ins.get("low")), C.c_double(p["f_up"]), C.c_double(p["f_dn"]),
                                P(outs[0]), P(outs[1]))
    if r == "pattern_any":
        bull = None if p.get("bull_list_null") else ptr_list([ins.get(f"bull{k}") for k in range(p["nb"])])
        bear = None if p.get("bear_list_null") else ptr_list([ins.get(f"bear{k}") for k in range(p["ns"])])
        return L.pq_pattern_any_signals(h, bb, bull, p["nb"], bear, p["ns"], P(outs[0]), P(outs[1]))
    if r == "ma_stack":
        mas = None if p.get("list_null") else ptr_list([ins.get(f"ma{k}") for k in range(p["n"])])
        return L.pq_ma_stack_signals(h, bb, mas, p["n"], P(outs[0]), P(outs[1]))
    raise KeyError(r)


def upload(case):
    return {k: torch.from_numpy(np.ascontiguousarray(c)).cuda() for k, c in case["cols"].items()}


def run_gpu(env, case, lay):
    """the call on poisoned outputs -> host arrays of lay['size'] elements"""
    ins, b = upload(case), env.batch(lay)
    dts = out_dtypes(case["rule"])
    outs = [poisoned(lay["size"], dt) for dt in dts]
    env.check(launch(env, b, case, ins, outs))
    torch.cuda.synchronize()
    for k, t in ins.items():       # the inputs are read only
        assert (as_host(t, np.uint8) == np.ascontiguousarray(case["cols"][k]).view(np.uint8)).all(), (case["rule"], k, "input changed")
    return [as_host(t, dt) for t, dt in zip(outs, dts)]


def assert_matches(tag, case, lay, got, exp=None):
    """rows of the batch equal the reference, everything else still holds the poison"""
    live = R.live_of(lay)
    exp = R.ref_case(case, R.ranges_of(lay), shape=(lay["size"],)) if exp is None else exp
    carrier = R.carrier_of(case)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert (g.view(np.uint8).reshape(lay["size"], -1)[~live] == POISON).all(), (tag, k, "a byte outside the batch was written")
        if g.dtype == np.uint8:
            bad = np.flatnonzero((g != e) & live)
        else:
            bad = np.flatnonzero(~R.same_f64(g, e, carrier) & live)
        assert len(bad) == 0, (tag, "output", k, "rows", bad[:5].tolist(), g[bad[:5]].tolist(), e[bad[:5]].tolist())
    return exp


def check_case(env, tag, case, lay):
    return assert_matches(tag, case, lay, run_gpu(env, case, lay))


def case_for(rule, rng, lay):
    n_cols = {"pattern_any": (3, 2), "ma_stack": 3}.get(rule)
    return R.gen_case(rule, rng, lay, n_cols=n_cols)


# ---- known answers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kat", KATS, ids=[k[0] for k in KATS])
def test_known_answers_on_the_gpu(env, kat):
    """the hand-written table of test_strategy_ref.py, each series as a batch of its own (ragged where the table gives ranges)"""
    tag, rule, cols, prm, ranges, exp = kat
    T = len(next(iter(cols.values())))
    lay = R.regular_layout(1, T) if ranges is None else R.ragged_layout([0] + [hi for _, hi in ranges])
    pad = lambda c: np.concatenate([c, np.full(R.GUARD, 77, dtype=c.dtype)])
    case = dict(rule=rule, cols={k: pad(c) for k, c in cols.items()}, params=prm)
    got = run_gpu(env, case, lay)
    assert_kat(tag, [g[:T] for g in got], exp)
    assert_matches(tag, case, lay, got)


# ---- row blocks, series split, pitch, ragged -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 255), (3, 256), (3, 257), (2, 513)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_blocks(env, shape):
    rng = np.random.default_rng(shape[1])
    lay = R.regular_layout(*shape)
    for rule in R.RULES:
        check_case(env, (rule, shape), case_for(rule, rng, lay), lay)


def formula_case(rule, lay):
    """inputs that are a function of (series, row): a series computed from another series' base is wrong"""
    n, T = lay["n"], lay["len"]
    s, t = np.divmod(np.arange(lay["size"]), lay["stride"])
    v = lambda j, m=7: ((s * (2 * j + 1) + t * 5 + j) % m).astype(np.float64)      # (2j + 1 and m are coprime below)
    sig = lambda j: ((s + t + j) % 3 != 0).astype(np.uint8)
    pat = lambda j: np.array([-200, -100, 0, 100, 200], dtype=np.int32)[(s * (j + 1) + t + j) % 5]
    if rule.startswith("gate"):
        mode = int(rule[4])
        return dict(rule=rule, cols=dict(a=v(0) - 3.0, c=v(1) - 3.0, buy_in=sig(0), sell_in=sig(1)), params=dict(mode=mode, k0=(0.0, 0.0, 0.0, 0.0, 0.25)[mode], k1=0.0))
    cols, prm = {
        "zscore": (dict(price=v(0), upper=v(1) + 1.0, mid=v(2)), {}),
        "scale_band": (dict(base=v(0, 11)), dict(f_lo=0.97, f_hi=1.03)),
        "volume_surge": (dict(volume=v(0), avg_volume=v(1, 5), close=v(2, 3)), dict(multiplier=1.5)),
        "gap": (dict(open=v(0), high=v(1), low=v(2)), dict(f_up=1.0, f_dn=1.0)),
        "pattern_any": (dict(bull0=pat(0), bull1=pat(1), bear0=pat(2)), dict(nb=2, ns=1)),
        "ma_stack": (dict(ma0=v(0, 4), ma1=v(1, 4)), dict(n=2)),
    }[rule]
    return dict(rule=rule, cols=cols, params=prm)


@pytest.mark.parametrize("n", [65535, 65536, 65541])
def test_series_split_over_grid_y_and_z(env, n):
    """grid.y holds at most 65535 series, grid.z the rest: the last series is written, and from its own rows"""
    lay = R.regular_layout(n, 3)
    for rule in (R.RULES if n == 65541 else ("gate3", "gap", "ma_stack")):
        case = formula_case(rule, lay)
        got = run_gpu(env, case, lay)
        exp = assert_matches((rule, n), case, lay, got)
        fired = R.firing(case, exp)
        assert fired[0] > n // 20, (rule, fired)       # the formula fires in every part of the batch
        last = [e[(n - 6) * 3: n * 3] for e in exp]
        assert any(x.any() for x in last), (rule, "nothing to see in the series behind the split")


@pytest.mark.parametrize("stride", [302, 304, 312])
def test_row_pitch(env, stride):
    """T = 301 at a larger pitch; u8 and i32 columns use the same stride in elements"""
    rng = np.random.default_rng(stride)
    lay = R.regular_layout(5, 301, stride)
    for rule in R.RULES:
        case = case_for(rule, rng, lay)
        pad = ~R.live_of(lay)
        for c in case["cols"].values():
            assert (c[pad] == (R.PAD_F64 if c.dtype == np.float64 else R.PAD_U8 if c.dtype == np.uint8 else R.PAD_I32)).all()
        check_case(env, (rule, stride), case, lay)


def plant_group_starts(case, lay):
    """make the first row of every group fire IF it read the last row of the group before it; -> those rows"""
    c, r = case["cols"], case["rule"]
    starts = sorted({int(lo) for lo, hi in R.ranges_of(lay) if lo > 0 and hi > lo})
    for lo in starts:
        if r == "gate3":
            c["a"][lo - 1], c["a"][lo], c["buy_in"][lo] = 1.0, 2.0, 1
        elif r == "volume_surge":
            c["close"][lo - 1], c["close"][lo], c["volume"][lo], c["avg_volume"][lo] = 1.0, 2.0, 10.0, 1.0
        elif r == "gap":
            c["high"][lo - 1], c["open"][lo] = 2.0, 2.0 * case["params"]["f_up"] + 1.0
        elif r == "ma_stack":
            for k in range(case["params"]["n"]):
                c[f"ma{k}"][lo - 1], c[f"ma{k}"][lo] = 1.0, float(-k)
    return starts


def test_ragged_groups(env):
    rng = np.random.default_rng(520)
    lay = R.ragged_layout(RAGGED)
    assert (lay["n"], lay["len"], lay["stride"]) == (6, 257, 520)
    for rule in R.RULES:
        case = case_for(rule, rng, lay)
        if rule in LOOKBACK:
            starts = plant_group_starts(case, lay)
            assert starts == [1, 4, 260, 517]
            alone = R.ref_case(case, R.ranges_of(lay))[0]
            joined = R.ref_case(case, [(0, lay["stride"])])[0]        # the concatenated rows as ONE series: it looks back
            assert (joined[starts] == 1).all() and (alone[starts] == 0).all(), rule
        check_case(env, (rule, "ragged"), case, lay)


# ---- values ---------------------------------------------------------------------------------------------------------------------------

def test_special_values_in_every_input_column(env):
    """NULL, NaN, +inf, -inf (one series each) at rows 0, 1, T - 1 and a random row of each input column in turn"""
    T, specials = 37, (R.NULL, np.nan, np.inf, -np.inf)
    lay = R.regular_layout(len(specials), T, 40)
    rng = np.random.default_rng(37)
    for rule in R.RULES:
        base = case_for(rule, rng, lay)
        for name, col in base["cols"].items():
            if col.dtype != np.float64:
                continue
            cols = {k: c.copy() for k, c in base["cols"].items()}
            for s, val in enumerate(specials):
                for t in (0, 1, T - 1, int(rng.integers(2, T - 1))):
                    cols[name][s * 40 + t] = val
            check_case(env, (rule, name), dict(base, cols=cols), lay)


def test_ties_infinities_and_wide_signal_bytes(env):
    f, u = (lambda *v: np.array(v, dtype=np.float64)), (lambda *v: np.array(v, dtype=np.uint8))

    def run(rule, cols, prm):
        T = len(next(iter(cols.values())))
        lay = R.regular_layout(1, T)
        pad = lambda c: np.concatenate([c, np.full(R.GUARD, 77, dtype=c.dtype)])
        case = dict(rule=rule, cols={k: pad(c) for k, c in cols.items()}, params=prm)
        got = run_gpu(env, case, lay)
        assert_matches(rule, case, lay, got)
        return [g[:T] for g in got]

    (z,) = run("zscore", dict(price=f(3, 1, 2, -np.inf, 5), upper=f(2, 2, 2, 3, np.inf), mid=f(2, 2, 2, 1, 1)), {})
    assert z[0] == np.inf and z[1] == -np.inf and np.isnan(z[2]) and z[3] == -np.inf and z[4] == 0.0
    lo, hi = run("scale_band", dict(base=f(np.inf, -np.inf, 3, R.NULL)), dict(f_lo=0.0, f_hi=-1.0))
    assert np.isnan(lo[0]) and np.isnan(lo[1]) and not R.isnull(lo[:2]).any() and lo[2] == 0.0 and R.isnull(lo[3])
    assert hi[0] == -np.inf and hi[1] == np.inf and hi[2] == -3.0 and R.isnull(hi[3])
    for mode, k0 in ((0, 5.0), (1, 0.0), (2, 0.0), (3, 0.0), (4, 0.0)):      # 2 and 255 count as set and come out as 1
        b, s = run(f"gate{mode}", dict(a=f(1, 2, 3, 4), c=f(0, 0, 0, 0), buy_in=u(2, 255, 0, 128), sell_in=u(255, 2, 0, 1)), dict(mode=mode, k0=k0, k1=0.0))
        assert b.tolist() == ([1, 1, 0, 1] if mode != 3 else [0, 1, 0, 1]) and s.tolist() == [1, 1, 0, 1], mode
    b, s = run("gate0", dict(a=f(-np.inf, np.inf, 5, 5), buy_in=u(1, 1, 1, 1), sell_in=u(1, 1, 1, 1)), dict(mode=0, k0=5.0, k1=5.0))
    assert b.tolist() == [1, 0, 0, 0] and s.tolist() == [0, 1, 0, 0]
    b, s = run("volume_surge", dict(volume=f(3, 3, np.inf, 4), avg_volume=f(2, 2, np.inf, 2), close=f(1, 2, 3, 3)), dict(multiplier=1.5))
    assert b.tolist() == [0, 0, 0, 0] and s.tolist() == [0, 0, 0, 0]        # 3 == 1.5 * 2; inf > inf is false; equal closes
    b, s = run("gap", dict(open=f(0, 8, 2, np.inf, -np.inf), high=f(4, 4, np.inf, np.inf, 1), low=f(4, 4, 1, -np.inf, -np.inf)), dict(f_up=2.0, f_dn=0.5))
    assert b.tolist() == [0, 0, 0, 0, 0] and s.tolist() == [0, 0, 0, 0, 0]  # 8 == 4 * 2, 2 == 4 * 0.5, inf > inf, -inf < -inf


def test_gates_in_place(env):
    """buy == buy_in and sell == sell_in give what fresh outputs give; modes 2, 3, 4 hand the sells through"""
    rng = np.random.default_rng(11)
    for lay in (R.regular_layout(3, 301, 304), R.ragged_layout(RAGGED)):
        for mode in range(5):
            case = R.gen_case(f"gate{mode}", rng, lay)
            fresh = run_gpu(env, case, lay)
            exp = assert_matches(("fresh", mode), case, lay, fresh)
            ins, b = upload(case), env.batch(lay)
            env.check(launch(env, b, case, ins, [ins["buy_in"], ins["sell_in"]]))
            torch.cuda.synchronize()
            live = R.live_of(lay)
            for k, nm in enumerate(("buy_in", "sell_in")):
                g = ins[nm].cpu().numpy()
                assert (g[live] == fresh[k][live]).all(), (mode, nm)
                assert (g[~live] == case["cols"][nm][~live]).all(), (mode, nm, "padding written")
            if mode >= 2:
                assert (exp[1][live] == (case["cols"]["sell_in"][live] != 0)).all() and (fresh[1][live] == exp[1][live]).all(), mode


# ---- column counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts", [(0, 0), (1, 0), (0, 1), (16, 16), (3, 3)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_pattern_any_column_counts(env, counts):
    rng = np.random.default_rng(sum(counts))
    for lay in (R.regular_layout(3, 257, 260), R.ragged_layout(RAGGED)):
        case = R.gen_case("pattern_any", rng, lay, n_cols=counts)
        for c in case["cols"].values():      # +-100 rare enough that 16 columns leave rows without a signal
            dull = (rng.random(c.shape) < 0.8) & R.live_of(lay)
            c[dull] = rng.choice(np.array([-200, 0, 200], dtype=np.int32), c.shape)[dull]
        if counts == (3, 3):
            case["cols"]["bear1"] = case["cols"]["bull2"]      # one column on both sides
        got = run_gpu(env, case, lay)
        exp = assert_matches(("pattern_any", counts), case, lay, got)
        live = R.live_of(lay)
        if counts == (0, 0):
            assert not got[0][live].any() and not got[1][live].any()       # zeros written over the poison
        else:
            for k, side in enumerate(("bull", "bear")):
                if counts[k]:
                    assert 0 < exp[k][live].sum() < live.sum(), (side, counts)
                else:
                    assert not got[k][live].any()
        bear = [case["cols"][f"bear{k}"] for k in range(counts[1])]
        bull = [case["cols"][f"bull{k}"] for k in range(counts[0])]
        if bear:      # +100 in a bearish column does not sell, +-200 fires nothing
            only_plus = np.all([c != -100 for c in bear], axis=0) & np.any([c == 100 for c in bear], axis=0) & live
            assert only_plus.any() and not got[1][only_plus].any()
        if bull:
            only_200 = np.all([np.abs(c) == 200 for c in bull], axis=0) & live
            assert not got[0][only_200].any()


@pytest.mark.parametrize("n", [2, 3, 16])
def test_ma_stack_column_counts(env, n):
    """a NULL in ANY column breaks the order on its row; the first later row where the order holds again fires"""
    rng = np.random.default_rng(n)
    for lay in (R.regular_layout(3, 257, 260), R.ragged_layout(RAGGED)):
        case = R.gen_case("ma_stack", rng, lay, n_cols=n)
        check_case(env, ("ma_stack", n, "random"), case, lay)
    T = 3 * n + 2
    lay = R.regular_layout(2, T)
    cols = {f"ma{k}": np.full(lay["size"], float(n - k)) for k in range(n)}      # series 0 in bullish order on every row, series 1 bearish
    for k in range(n):
        cols[f"ma{k}"][T: 2 * T] = float(k)
        cols[f"ma{k}"][3 * k + 1] = R.NULL                                        # column k is NULL on row 3k + 1 of series 0 ...
        cols[f"ma{k}"][T + 3 * k + 1] = R.NULL                                    # ... and of series 1
    case = dict(rule="ma_stack", cols=cols, params=dict(n=n))
    got = run_gpu(env, case, lay)
    assert_matches(("ma_stack", n, "nulls"), case, lay, got)
    fire = np.zeros(T, dtype=np.uint8)
    fire[[3 * k + 2 for k in range(n)]] = 1
    assert got[0][:T].tolist() == fire.tolist() and not got[1][:T].any()
    assert got[1][T: 2 * T].tolist() == fire.tolist() and not got[0][T: 2 * T].any()


# ---- refusals, empty batches ----------------------------------------------------------------------------------------------------------

def refusal_cases(lay, rng):
    """(tag, case, names of inputs passed as NULL, which outputs are NULL, batch override, message)"""
    out = []
    for rule in R.RULES:
        n_cols = {"pattern_any": (2, 2), "ma_stack": 2}.get(rule)
        case = R.gen_case(rule, rng, lay, n_cols=n_cols)
        if rule.startswith("gate"):
            case["cols"].setdefault("c", case["cols"]["a"].copy())
        msg = "null column" if rule in ("pattern_any", "ma_stack") else "null pointer"
        for name in case["cols"]:
            if name == "c" and case["params"]["mode"] not in (2, 4):
                continue
            m = "second column" if name == "c" else msg
            out.append((f"{rule}: {name} NULL", case, (name,), (), None, m))
        for k in range(len(out_dtypes(rule))):
            out.append((f"{rule}: output {k} NULL", case, (), (k,), None, "null pointer"))
        out.append((f"{rule}: stride < len", case, (), (), (lay["n"], lay["len"], lay["len"] - 1), "bad batch"))
        if rule == "gate0":
            for mode in (-1, 5):
                out.append((f"gate mode {mode}", dict(case, params=dict(case["params"], mode=mode)), (), (), None, "mode must be"))
        if rule == "pattern_any":
            big = R.gen_case(rule, rng, lay, n_cols=(17, 17))
            out.append(("pattern_any: 17 bullish", dict(big, params=dict(nb=17, ns=1)), (), (), None, "at most 16"))
            out.append(("pattern_any: 17 bearish", dict(big, params=dict(nb=1, ns=17)), (), (), None, "at most 16"))
            out.append(("pattern_any: -1 bullish", dict(big, params=dict(nb=-1, ns=1)), (), (), None, "at most 16"))
            out.append(("pattern_any: bullish list NULL", dict(case, params=dict(case["params"], bull_list_null=True)), (), (), None, "null pointer"))
            out.append(("pattern_any: bearish list NULL", dict(case, params=dict(case["params"], bear_list_null=True)), (), (), None, "null pointer"))
        if rule == "ma_stack":
            big = R.gen_case(rule, rng, lay, n_cols=17)
            out.append(("ma_stack: n = 1", dict(big, params=dict(n=1)), (), (), None, "2 .. 16"))
            out.append(("ma_stack: n = 17", dict(big, params=dict(n=17)), (), (), None, "2 .. 16"))
            out.append(("ma_stack: list NULL", dict(case, params=dict(n=2, list_null=True)), (), (), None, "null pointer"))
    return out


def test_refusals_write_nothing_and_leave_the_context_usable(env):
    rng = np.random.default_rng(99)
    lay = R.regular_layout(3, 40, 48)
    n_refused = 0
    for tag, case, null_ins, null_outs, bshape, msg in refusal_cases(lay, rng):
        ins = upload(case)
        for nm in null_ins:
            ins[nm] = None
        dts = out_dtypes(case["rule"])
        outs = [poisoned(lay["size"], dt) for dt in dts]
        b = env.batch(lay) if bshape is None else env.Batch(*bshape, None)
        with pytest.raises(env.pq.PqError, match=msg):
            env.check(launch(env, b, case, ins, [None if k in null_outs else t for k, t in enumerate(outs)]))
        torch.cuda.synchronize()
        for t in outs:
            assert (t.cpu().numpy() == POISON).all(), (tag, "a refused call wrote")
        n_refused += 1
    assert n_refused > 60
    # the refusals are refused while a suite is being recorded too, and record nothing
    b = env.batch(lay)
    env.check(env.L.pq_suite_begin(env.h, C.byref(b)))
    try:
        case = R.gen_case("gate2", rng, lay)
        ins = upload(case)
        ins["c"] = None
        with pytest.raises(env.pq.PqError, match="second column"):
            env.check(launch(env, b, case, ins, [poisoned(lay["size"], np.uint8)] * 2))
    finally:
        env.check(env.L.pq_suite_abort(env.h))
    for rule in R.RULES:      # ... and a valid call afterwards works
        check_case(env, (rule, "after the refusals"), case_for(rule, rng, lay), lay)


def test_empty_batches_touch_nothing(env):
    rng = np.random.default_rng(5)
    full = R.regular_layout(3, 40, 48)
    for rule in R.RULES:
        case = case_for(rule, rng, full)
        ins = upload(case)
        for shape in ((0, 40, 48), (3, 0, 48), (0, 0, 0)):
            outs = [poisoned(full["size"], dt) for dt in out_dtypes(rule)]
            env.check(launch(env, env.Batch(*shape, None), case, ins, outs))
            torch.cuda.synchronize()
            for t in outs:
                assert (t.cpu().numpy() == POISON).all(), (rule, shape)
    lay = R.ragged_layout([0, 0, 0])            # a ragged batch of empty groups
    case = case_for("gap", rng, lay)
    assert_matches("empty groups", case, lay, run_gpu(env, case, lay))


# ---- randomised ----------------------------------------------------------------------------------------------------------------------

def test_randomised_cases(env):
    """150 seeded cases: random rule and mode, N in 1..40, T in 1..600, a random pitch or ragged offsets, 2 % NULLs, 2 % NaNs,
    quantised values.  The reference fires for every rule over the run (asserted here and, on the CPU, in test_strategy_ref.py)."""
    count = {r: np.zeros(2, dtype=np.int64) for r in R.RULES}
    n = 0
    for case, lay in R.random_cases():
        exp = check_case(env, ("random", n, case["rule"], lay["n"], lay["len"], lay["stride"], lay["offsets"] is not None), case, lay)
        count[case["rule"]] += R.firing(case, exp)
        n += 1
    assert n == R.RANDOM_CASES == 150
    for r, c in count.items():
        assert c[0] >= 50 and c[1] >= 50, (r, c)


# ---- recorded chains ------------------------------------------------------------------------------------------------------------------

EXACT, TOL = (1, 5, 6, 7), (0, 2, 3, 4)
CHAIN_LAYOUTS = {"70x301": lambda: R.regular_layout(70, 301), "66x306": lambda: R.regular_layout(66, 306),
                 "70x301-pitch-304": lambda: R.regular_layout(70, 301, 304), "ragged-40-groups": None}


def ragged_chain_layout():
    rng = np.random.default_rng(40)
    lens = rng.integers(1, 401, 40)
    lens[:7] = [1, 2, 255, 256, 257, 400, 33]
    return R.ragged_layout(np.concatenate([[0], np.cumsum(lens)]))


class Chain:
    """the recorded workload: inputs, every intermediate and output column, and the calls -- made eagerly or between
    pq_suite_begin / pq_suite_end, they are the same code"""
    F64 = ("k", "d", "m5", "m10", "m20", "t1", "t2", "bb_u", "bb_m", "bb_l", "z", "lo", "hi", "pos1", "cash1", "eq1", "pos2", "cash2", "eq2")
    U8 = ("b0", "s0", "b1", "s1", "b2", "s2", "b3", "s3", "b4", "s4", "b5", "s5", "b6", "s6", "b7", "s7", "b8", "s8")
    I32 = ("p0", "p1", "p2")
    PATTERNS = ("cdlengulfing", "cdlhikkake", "cdl3outside")

    def __init__(self, env, oracle, lay):
        from polars_quant_amd._lib import BtParams
        from polars_quant_amd._spec import BT_DEFAULTS
        self.env, self.lay, self.live = env, lay, R.live_of(lay)
        self.prm = BtParams(**BT_DEFAULTS)
        ranges = R.ranges_of(lay)
        d = oracle.gen_ohlcv(0x5EED0070, lay["n"], lay["len"], 0)
        self.host = {}
        for nm in ("open", "high", "low", "close", "volume"):
            col = np.full(lay["size"], R.PAD_F64)
            for s, (lo, hi) in enumerate(ranges):
                col[lo:hi] = d[nm][s, : hi - lo]
            self.host[nm] = col
        self.host["vavg"] = np.where(self.live, np.roll(self.host["volume"], 3), R.PAD_F64)      # "the average": the volume three rows earlier
        rng = np.random.default_rng(7)
        for nm in ("rb", "rs"):      # signal INPUTS (no recorded call writes them): the gate that reads them depends on its column c alone
            self.host[nm] = np.where(self.live, rng.random(lay["size"]) < 0.5, R.PAD_U8).astype(np.uint8)
        self.inp = {k: torch.from_numpy(v).cuda() for k, v in self.host.items()}
        self.buf = {k: poisoned(lay["size"], np.float64).view(torch.float64) for k in self.F64}
        self.buf.update({k: poisoned(lay["size"], np.uint8) for k in self.U8})
        self.buf.update({k: poisoned(lay["size"], np.int32).view(torch.int32) for k in self.I32})
        self.buf.update({k: poisoned(lay["n"] * 8, np.float64).view(torch.float64) for k in ("summ1", "summ2")})
        self.b = env.batch(lay)
        self.keep = list(env.keep)

    def poison(self):
        for t in self.buf.values():
            t.view(torch.uint8).fill_(POISON)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in self.buf.items()}

    def calls(self):
        L, h, bb, ck, i, o = self.env.L, self.env.h, C.byref(self.b), self.env.check, self.inp, self.buf
        dbl = C.c_double
        # 1. the stochastic strategy of scripts/bench_strategy.py: %K / %D cross, zones (fresh outputs), backtest
        ck(L.pq_stoch(h, bb, P(i["high"]), P(i["low"]), P(i["close"]), 5, 3, 0, 3, 0, P(o["k"]), P(o["d"])))
        ck(L.pq_cross_signals(h, bb, P(o["k"]), P(o["d"]), P(o["b0"]), P(o["s0"])))
        ck(L.pq_gate_signals(h, bb, P(o["k"]), None, 0, dbl(20.0), dbl(80.0), P(o["b0"]), P(o["s0"]), P(o["b1"]), P(o["s1"])))
        ck(L.pq_backtest_vectorized(h, bb, P(i["close"]), P(o["b1"]), P(o["s1"]), None, C.byref(self.prm), P(o["pos1"]), P(o["cash1"]), P(o["eq1"]), P(o["summ1"])))
        # 2. three averages, their stack, three gates IN PLACE (above m20, 0.1 % above m10, m5 rising), a second backtest
        for nm, per in (("m5", 5), ("m10", 10), ("m20", 20)):
            ck(L.pq_sma(h, bb, P(i["close"]), per, P(o[nm])))
        ck(L.pq_ma_stack_signals(h, bb, ptr_list([o["m5"], o["m10"], o["m20"]]), 3, P(o["b2"]), P(o["s2"])))
        ck(L.pq_gate_signals(h, bb, P(i["close"]), P(o["m20"]), 2, dbl(0.0), dbl(0.0), P(o["b2"]), P(o["s2"]), P(o["b2"]), P(o["s2"])))
        ck(L.pq_gate_signals(h, bb, P(i["close"]), P(o["m10"]), 4, dbl(0.001), dbl(0.0), P(o["b2"]), P(o["s2"]), P(o["b2"]), P(o["s2"])))
        ck(L.pq_gate_signals(h, bb, P(o["m5"]), None, 3, dbl(0.0), dbl(0.0), P(o["b2"]), P(o["s2"]), P(o["b2"]), P(o["s2"])))
        ck(L.pq_backtest_vectorized(h, bb, P(i["close"]), P(o["b2"]), P(o["s2"]), None, C.byref(self.prm), P(o["pos2"]), P(o["cash2"]), P(o["eq2"]), P(o["summ2"])))
        # 3. three recognisers, any-of (p1 on both sides)
        for nm, pat in zip(self.I32, self.PATTERNS):
            ck(L.pq_cdl(h, bb, self.env.pq.PATTERN_NAMES.index(pat), P(i["open"]), P(i["high"]), P(i["low"]), P(i["close"]), dbl(0.3), P(o[nm])))
        ck(L.pq_pattern_any_signals(h, bb, ptr_list([o["p0"], o["p1"]]), 2, ptr_list([o["p1"], o["p2"]]), 2, P(o["b3"]), P(o["s3"])))
        # 4. Bollinger bands, z-score, band rule
        ck(L.pq_bbands(h, bb, P(i["close"]), 20, dbl(2.0), dbl(2.0), P(o["bb_u"]), P(o["bb_m"]), P(o["bb_l"])))
        ck(L.pq_zscore(h, bb, P(i["close"]), P(o["bb_u"]), P(o["bb_m"]), P(o["z"])))
        ck(L.pq_band_signals(h, bb, P(o["z"]), dbl(-1.0), dbl(1.0), P(o["b4"]), P(o["s4"])))
        # 5. percentage bands around an average, channel reversion
        ck(L.pq_scale_band(h, bb, P(o["m20"]), dbl(0.97), dbl(1.03), P(o["lo"]), P(o["hi"])))
        ck(L.pq_channel_signals(h, bb, P(i["close"]), P(o["lo"]), P(o["hi"]), 0, P(o["b5"]), P(o["s5"])))
        # 6. the rules that read the inputs alone
        ck(L.pq_volume_surge_signals(h, bb, P(i["volume"]), P(i["vavg"]), P(i["close"]), dbl(1.1), P(o["b6"]), P(o["s6"])))
        ck(L.pq_gap_signals(h, bb, P(i["open"]), P(i["high"]), P(i["low"]), dbl(0.995), dbl(1.005), P(o["b7"]), P(o["s7"])))
        # 7. a gate whose ONLY recorded dependency is its column c, two jobs deep: dropped from the thunk's reads, the gate would
        #    replay in the first phase, before c is written
        ck(L.pq_sma(h, bb, P(i["close"]), 7, P(o["t1"])))
        ck(L.pq_sma(h, bb, P(o["t1"]), 7, P(o["t2"])))
        ck(L.pq_gate_signals(h, bb, P(i["close"]), P(o["t2"]), 2, dbl(0.0), dbl(0.0), P(i["rb"]), P(i["rs"]), P(o["b8"]), P(o["s8"])))


def run_chain(env, oracle, lay, tag):
    """eager against two replays of the recording -> (eager snapshot, chain)"""
    ch = Chain(env, oracle, lay)
    ch.poison()
    ch.calls()
    eager = ch.snapshot()
    live = ch.live
    for k in Chain.U8:      # not zeros against zeros: every signal column fires, and the gates cut something
        assert eager[k][live].max() == 1 and eager[k][live].sum() > 0, (tag, k)
    assert eager["b1"][live].sum() < eager["b0"][live].sum() and eager["b8"][live].sum() < ch.host["rb"][live].sum()
    L, h = env.L, env.h
    env.check(L.pq_suite_begin(h, C.byref(ch.b)))
    try:
        ch.calls()
    except Exception:
        L.pq_suite_abort(h)
        raise
    suite = C.c_void_p()
    env.check(L.pq_suite_end(h, C.byref(suite)))
    try:
        nph, nseq, nrow = C.c_int32(), C.c_int32(), C.c_int32()
        env.check(L.pq_suite_info(suite, C.byref(nph), C.byref(nseq), C.byref(nrow)))
        # averages -> stack -> gate 2 -> gate 4 -> gate 3 (each in place on the signals of the one before) -> backtest: six phases deep
        assert nph.value >= 6, nph.value
        for rep in range(2):
            ch.poison()
            env.check(L.pq_suite_run(h, suite))
            got = ch.snapshot()
            for k in Chain.F64 + Chain.U8 + Chain.I32:
                g, e = got[k].view(np.uint8).reshape(lay["size"], -1)[live], eager[k].view(np.uint8).reshape(lay["size"], -1)[live]
                bad = np.flatnonzero((g != e).any(axis=1))
                assert len(bad) == 0, (tag, "replay", rep, "column", k, "differs from the eager call at rows", bad[:5].tolist())
            for k in ("summ1", "summ2"):
                g, e = got[k].reshape(-1, 8), eager[k].reshape(-1, 8)
                for col in EXACT:
                    assert (R.bits(g[:, col]) == R.bits(e[:, col])).all(), (tag, "replay", rep, k, "summary column", col)
            last = got
    finally:
        env.check(L.pq_suite_destroy(h, suite))
    return eager, last, ch


def oracle_summary(oracle, ch, eager, buy, sell):
    out = np.zeros((ch.lay["n"], 8))
    for s, (lo, hi) in enumerate(R.ranges_of(ch.lay)):
        if hi > lo:
            out[s] = oracle.backtest(ch.host["close"][lo:hi], eager[buy][lo:hi], eager[sell][lo:hi])[3]
    return out


@pytest.mark.parametrize("layout", list(CHAIN_LAYOUTS))
def test_recorded_chains_equal_the_eager_calls(env, oracle, layout, monkeypatch):
    """Signals, intermediates, position / cash / equity and summary columns 1, 5, 6, 7 bit for bit; columns 0, 2, 3, 4 of both sides
    within 1e-12 of the oracle run on the eager signals (a recorded backtest runs the one-wave kernel, an eager one four waves)."""
    monkeypatch.delenv("PQ_BT_WAVES", raising=False)
    lay = ragged_chain_layout() if CHAIN_LAYOUTS[layout] is None else CHAIN_LAYOUTS[layout]()
    eager, replay, ch = run_chain(env, oracle, lay, layout)
    for summ, buy, sell in (("summ1", "b1", "s1"), ("summ2", "b2", "s2")):
        es = oracle_summary(oracle, ch, eager, buy, sell)
        nonempty = np.array([hi > lo for lo, hi in R.ranges_of(lay)])
        ok = ~np.isnan(es).any(axis=1) & nonempty
        assert ok.sum() > lay["n"] // 2 and es[ok, 7].sum() > 0
        for side, got in (("eager", eager), ("replay", replay)):
            g = got[summ].reshape(-1, 8)
            for col in EXACT:
                assert (R.bits(g[ok, col]) == R.bits(es[ok, col])).all(), (layout, side, summ, col)
            for col in TOL:
                np.testing.assert_allclose(g[ok, col], es[ok, col], rtol=1e-12, atol=1e-13, err_msg=f"{layout} {side} {summ} column {col}")


@pytest.mark.parametrize("layout", list(CHAIN_LAYOUTS))
def test_recorded_chains_one_wave_on_both_sides_every_bit(env, oracle, layout, monkeypatch):
    """PQ_BT_WAVES=1 for the eager calls AND the recording: the same backtest kernel on both sides, so all eight summary columns are
    equal in every bit.  This is what decides that the profiles' mismatch is the kernel form and not the recorded order."""
    monkeypatch.setenv("PQ_BT_WAVES", "1")
    lay = ragged_chain_layout() if CHAIN_LAYOUTS[layout] is None else CHAIN_LAYOUTS[layout]()
    eager, replay, ch = run_chain(env, oracle, lay, layout)
    for k in ("summ1", "summ2"):
        g, e = replay[k].reshape(-1, 8), eager[k].reshape(-1, 8)
        nonempty = np.array([hi > lo for lo, hi in R.ranges_of(lay)])
        for col in range(8):
            bad = np.flatnonzero((R.bits(g[:, col]) != R.bits(e[:, col])) & nonempty)
            assert len(bad) == 0, (layout, k, "summary column", col, "series", bad[:5].tolist(), g[bad[:3], col].tolist(), e[bad[:3], col].tolist())
