"""-m gpu: a metamorphic matrix over the entry points of polars_quant_amd/api.py -- the result of a call must not depend on how its
arguments are laid out.  For every entry point and shape the BASELINE is the call with every argument a dense contiguous device tensor;
it is compared once with the reference that the entry point's own suite uses (the anchor: the matrix cannot pass on a uniformly wrong
answer), and then the call is repeated under each layout assignment and every output is compared with the baseline: shapes and dtypes
equal, bits equal on the integer view (so a NULL equals only a NULL), inner stride 1.

Entry points and the layout helper each one goes through:

| entry point                                                         | helper                                                          |
|---------------------------------------------------------------------|-----------------------------------------------------------------|
| call (ema 1 input, midprice 2, atr 3, ad 4, macd; [T] inputs), cdl, cdl_all | _to_device, _same_layout, _batch(lone_dense)            |
| backtest_vectorized, backtest_leveraged, cross / channel / gate_signals     | _to_device, contiguous(), _batch(dense=True)            |
| backtest_report                                                     | its own stride check, _batch(lone_dense)                        |
| factor_ic                                                           | _to_device, contiguous(), _batch(dense=True)                    |
| factor_quantiles, factor_long_short, factor_double_sort, ic_decay   | _xsec_inputs (_same_layout, _batch); labels out on the pitch    |
| ic_subgroup, factor_weighted                                        | _xsec_inputs, _codes_on_pitch                                   |
| factor_portfolio                                                    | _xsec_inputs, _labels_on_pitch                                  |
| factor_clean (log_cap on / off, industry [N] / [N, T])              | _same_layout, _batch, _codes_on_pitch(spread)                   |
| xsec_regress, ts_regress, factor_rolling_regress ([T] series among the columns) | _regress_upload (_same_layout, _batch of the LAST)  |
| linear                                                              | _same_layout, _batch of the LAST                                |
| factor_orthogonalize (with and without out= on the batch pitch), factor_combine | _same_layout, _batch                                |
| factor_rank, factor_normalize, factor_binary, factor_rolling, factor_ts, factor_ts_pair | _build_call (_xsec_inputs)                  |
| backtest_sweep (price, lines, [n, T] benchmark)                     | _same_layout, _batch; the benchmark keeps its own stride        |

Layouts of one [n, T] float64 argument, each a view into a larger device buffer whose other cells hold poison (one run with the NULL
pattern, one with +inf: a cell read as data beyond T changes an output in one of the two), the live cells flush against it:
D dense; P pitch rs(T) (T + 16 where rs(T) == T); Q pitch rs(T) + 16; O odd pitch (T + 1 or T + 2); B pitch P, base one element off;
X the transpose of a [T, n] tensor; H host numpy in C order; F host numpy in Fortran order; for n = 1 also R2 = row 1 of a [3, rs(T)]
matrix and R3 = [1, 1:2, :T] of a [2, 3, rs(T) + 16] tensor.  A [T] series: D, S = x[::2], H.  uint8 arguments (labels, buy, sell): D, P,
X, H; integer codes [n, T]: D, P, H; codes [n]: D, H.  A layout that an argument's kind does not have is replaced by its nearest one.
After every call the whole backing buffer of every device argument is compared with a pristine copy.

Assignments per entry point: every layout for all arguments; every layout first with the others dense; dense first with every layout
last; and the mixed rows (P, Q, O, ...) and, for one row, (R2, D, R3, ...) cycled over the arguments.

Shapes: (1, 37), (1, 48), (3, 37), (3, 48), (2, 1), (3, 0), (0, 5); a refusal must be the same refusal under every layout.  On an empty
batch nothing is launched and outputs may be left unwritten, so there shapes, dtypes and refusals are compared, not bits.  atr, ema and
macd also run at (1, 1100) and (3, 1100) under PQ_WT_ALL=1, where the layout decides between the wave-per-symbol form, the 16-byte
tiled body and the 8-byte form: the bits agree, and wt_stats shows that some assignments took the wave form and some did not.

The anchor's bound: the entry points' own suites hold the references bit for bit (or to tests/tolerance.py); here the reference only has
to tell a right baseline from a wrong one, at shapes those suites do not run, and some references take a host log or pow where the
device takes its own (factor_clean's log of the cap, the report's annualisation), which differ in the last bits and are then amplified
by a regression.  2^-53 is 1.1e-16; the amplification of a least-squares residual at these sizes stays below 1e6: relative 1e-7, absolute
1e-9 on values of order 1.  NULL masks and integer outputs are compared exactly.
"""
import itertools
import types
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import backtest_report_ref as RP                      # noqa: E402
import factor_portfolio_ref as PF                     # noqa: E402
import linear_ref as LN                               # noqa: E402
import strategy_ref as SR                             # noqa: E402
import sweep_ref as SW                                # noqa: E402
import xsec_build_ref as XB                           # noqa: E402
import xsec_clean_ref as XC                           # noqa: E402
import xsec_combine_ref as CB                         # noqa: E402
import xsec_double_ref as XD                          # noqa: E402
import xsec_orth_ref as XO                            # noqa: E402
import xsec_ref as X                                  # noqa: E402
import xsec_regress_ref as RG                         # noqa: E402
import xsec_robust_ref as RB                          # noqa: E402
import xsec_rolling_ref as RL                         # noqa: E402
import xsec_rolling_regress_ref as RR                 # noqa: E402
import xsec_ts_ref as TS                              # noqa: E402
from oracle import pq_oracle as O                     # noqa: E402
from parity_util import NULL_BITS                     # noqa: E402

NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]
SEED = 0x1A70075
GUARD = 16                                            # poison cells in front of and behind every view (128 bytes: the base stays aligned)
POISON = {"null": NULL_BITS, "inf": 0x7FF0000000000000}
POISON_U8 = {"null": 1, "inf": 255}                   # a live signal / group 1; LABEL_OUT
POISON_CODE = {"null": 0, "inf": 1}                   # valid codes both
SENT = -7.25e300
SHAPES = [(1, 37), (1, 48), (3, 37), (3, 48), (2, 1), (3, 0), (0, 5)]
ALLOWED = {"f8": ("D", "P", "Q", "O", "B", "X", "H", "F", "R2", "R3"), "u8": ("D", "P", "X", "H"), "code2": ("D", "P", "H"),
           "code1": ("D", "H"), "ser": ("D", "S", "H")}
RTOL, ATOL = 1e-7, 1e-9


def rs(T):
    return (T + 15) // 16 * 16


def even_pitch(T):
    return rs(T) if rs(T) != T else T + 16


def fit(kind, L):
    """the layout of ALLOWED[kind] nearest to L"""
    if L in ALLOWED[kind]:
        return L
    if L == "F":
        return "H"
    return {"u8": "P", "code2": "P", "code1": "D", "ser": "S"}[kind]


def assignments(kinds, n):
    k = len(kinds)
    LS = ["D", "P", "Q", "O", "B", "X", "H", "F"] + (["R2", "R3"] if n == 1 else [])
    rows = [(L,) * k for L in LS]
    if k > 1:
        rows += [(L,) + ("D",) * (k - 1) for L in LS] + [("D",) * (k - 1) + (L,) for L in LS]
    rows.append(tuple(itertools.islice(itertools.cycle(("P", "Q", "O")), k)))
    if n == 1:
        rows.append(tuple(itertools.islice(itertools.cycle(("R2", "D", "R3")), k)))
    out = []
    for r in rows:
        f = tuple(fit(kd, L) for kd, L in zip(kinds, r))
        if f not in out:
            out.append(f)
    return out


def lay(arr, kind, L, poison):
    """one argument on layout L -> (the object handed to the api, its whole backing buffer on the device or None for a host array)"""
    if L == "H":
        return np.ascontiguousarray(arr).copy(), None
    if L == "F":
        return np.asfortranarray(arr), None
    if kind in ("f8", "ser"):
        def flat(size):
            return torch.full((size,), POISON[poison], dtype=torch.int64, device="cuda")
        view = lambda raw: raw.view(torch.float64)
    elif kind == "u8":
        def flat(size):
            return torch.full((size,), POISON_U8[poison], dtype=torch.uint8, device="cuda")
        view = lambda raw: raw
    else:
        def flat(size):
            return torch.full((size,), POISON_CODE[poison], dtype=torch.int64, device="cuda")
        view = lambda raw: raw
    src = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    if arr.ndim == 1:
        m = arr.shape[0]
        step = 2 if L == "S" else 1
        raw = flat(GUARD + step * m + GUARD)
        v = view(raw)[GUARD:GUARD + step * m][::step]
        v.copy_(src)
        return v, raw
    n, T = arr.shape
    if L == "X":
        raw = flat(GUARD + T * n + GUARD)
        v = view(raw)[GUARD:GUARD + T * n].view(T, n).t()
    elif L == "R2":
        raw = flat(GUARD + 3 * rs(T) + GUARD)
        v = view(raw)[GUARD:GUARD + 3 * rs(T)].view(3, rs(T))[1:2, :T]
    elif L == "R3":
        p = rs(T) + 16
        raw = flat(GUARD + 6 * p + GUARD)
        v = view(raw)[GUARD:GUARD + 6 * p].view(2, 3, p)[1, 1:2, :T]
    else:
        pitch = {"D": T, "P": even_pitch(T), "Q": rs(T) + 16, "O": T + 1 if T % 2 == 0 else T + 2, "B": even_pitch(T)}[L]
        off = GUARD + (1 if L == "B" else 0)
        raw = flat(off + n * pitch + GUARD)
        v = view(raw)[off:off + n * pitch].view(n, pitch)[:, :T]
    v.copy_(src)
    return v, raw


def to_np(x, tag):
    if isinstance(x, torch.Tensor):
        if x.dim() >= 1 and x.shape[-1] > 1 and x.numel():
            assert x.stride(-1) == 1, f"{tag}: inner stride {x.stride(-1)}"
        return x.detach().cpu().contiguous().numpy()
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x)
    if type(x).__module__.split(".")[0] == "pyarrow":
        a = np.array(x.to_numpy(zero_copy_only=False), dtype=np.float64 if str(x.type) == "double" else np.int32)
        if x.null_count:
            a[np.asarray(x.is_null())] = NULL
        return a
    return np.asarray(x)


def flatten(out, pre=""):
    """the outputs of a call -> {dotted name: host array}"""
    if out is None:
        return {}
    res = {}
    if isinstance(out, dict):
        for k, v in out.items():
            res.update(flatten(v, f"{pre}{k}."))
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            res.update(flatten(v, f"{pre}{i}."))
    else:
        res[pre.rstrip(".")] = to_np(out, pre)
    return res


class Refused:
    def __init__(self, e):
        self.kind, self.msg = type(e).__name__, str(e)


def invoke(api, e, a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", api.PqLayoutWarning)
        try:
            return flatten(e.run(api, a))
        except (api.PqError, ValueError, TypeError) as ex:
            if isinstance(ex, api.PqError) and str(ex).startswith(("pq status 2:", "pq status 4:")):
                raise        # a HIP error or out of memory is no refusal of the arguments
            return Refused(ex)


def same_bits(tag, got, base, bits=True):
    if isinstance(base, Refused) or isinstance(got, Refused):
        assert isinstance(base, Refused) and isinstance(got, Refused) and got.kind == base.kind, \
            f"{tag}: {'refused: ' + got.msg if isinstance(got, Refused) else 'ran'}, the dense call {'was refused: ' + base.msg if isinstance(base, Refused) else 'ran'}"
        return
    assert sorted(got) == sorted(base), f"{tag}: outputs {sorted(got)} vs {sorted(base)}"
    for k, b in base.items():
        g = got[k]
        assert g.shape == b.shape and g.dtype == b.dtype, f"{tag}: {k}: {g.shape} {g.dtype} vs {b.shape} {b.dtype}"
        if bits and g.tobytes() != b.tobytes():
            gi, bi = g.view(f"u{g.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
            bad = np.argwhere(gi != bi)
            raise AssertionError(f"{tag}: {k}: {len(bad)} of {b.size} cells differ from the dense call; first at {bad[:3].tolist()}: "
                                 f"{g[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def anchor(tag, base, ref):
    """the dense call against the reference of the entry point's own suite"""
    for k, r in ref.items():
        assert k in base, f"{tag}: the reference has {k}, the call returned {sorted(base)}"
        g, r = base[k], np.asarray(r)
        assert g.shape == r.shape, f"{tag}: {k}: {g.shape} vs the reference's {r.shape}"
        if g.dtype != np.float64:
            assert (g.astype(np.int64) == r.astype(np.int64)).all(), f"{tag}: {k}: {np.sum(g != r)} integer cells differ from the reference"
            continue
        g, r = g.reshape(-1), np.array(r, dtype=np.float64).reshape(-1)
        gn, rn = g.view(np.uint64) == np.uint64(NULL_BITS), r.view(np.uint64) == np.uint64(NULL_BITS)
        assert (gn == rn).all(), f"{tag}: {k}: NULL masks differ from the reference at {np.argwhere(gn != rn)[:3].tolist()}"
        ok = ~gn
        with np.errstate(invalid="ignore"):
            close = np.isclose(g[ok], r[ok], rtol=RTOL, atol=ATOL, equal_nan=True)
        assert close.all(), f"{tag}: {k}: {np.sum(~close)} cells differ from the reference; first got {g[ok][~close][:3]} expected {r[ok][~close][:3]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# data

def walk(rng, n, T, s=0.02):
    return 100.0 * np.exp(np.cumsum(s * rng.standard_normal((n, T)), axis=1))


def ohlcv(rng, n, T):
    c = walk(rng, n, T)
    o = c * (1.0 + 0.01 * rng.standard_normal((n, T)))
    h = np.maximum(o, c) * (1.0 + 0.01 * np.abs(rng.standard_normal((n, T))))
    l = np.minimum(o, c) * (1.0 - 0.01 * np.abs(rng.standard_normal((n, T))))
    v = 1e6 * (1.0 + rng.random((n, T)))
    return {"open": o, "high": h, "low": l, "close": c, "volume": v}


def fac(rng, n, T, nulls=0.05):
    f = rng.standard_normal((n, T))
    if nulls and n * T >= 20:
        f[rng.random((n, T)) < nulls] = NULL
    return f


def pos(rng, n, T):
    return 50.0 * np.exp(0.3 * rng.standard_normal((n, T)))


def sig(rng, n, T, p=0.3):
    return (rng.random((n, T)) < p).astype(np.uint8)


def f8(d, *names):
    return [(nm, "f8", d[nm]) for nm in names]


ENTRIES = {}


def entry(name, args, run, ref=None):
    ENTRIES[name] = types.SimpleNamespace(name=name, args=args, run=run, ref=ref)


def tup(res):
    return {str(i): r for i, r in enumerate(res)}


# -- indicators and recognisers
def _call_entry(fn, cols, **prm):
    entry(f"call_{fn}", lambda rng, n, T: f8(ohlcv(rng, n, T), *cols),
          lambda api, a: api.call(fn, *[a[c] for c in cols], **prm),
          lambda d: tup(O.call(fn, *[d[c] for c in cols], **prm)))


_call_entry("ema", ["close"], timeperiod=3)
_call_entry("midprice", ["high", "low"], timeperiod=4)
_call_entry("atr", ["high", "low", "close"], timeperiod=3)
_call_entry("ad", ["high", "low", "close", "volume"])
_call_entry("macd", ["close"], fastperiod=3, slowperiod=7, signalperiod=4)
HLC = ["high", "low", "close"]
entry("call_atr_series", lambda rng, n, T: [(c, "ser", ohlcv(rng, 1, T)[c][0]) for c in HLC],
      lambda api, a: api.call("atr", *[a[c] for c in HLC], timeperiod=3),
      lambda d: tup(O.call("atr", *[d[c] for c in HLC], timeperiod=3)))
OHLC = ["open", "high", "low", "close"]
CDL_ONE, CDL_SOME = O.PATTERN_NAMES[0], list(O.PATTERN_NAMES[:4])
entry("cdl", lambda rng, n, T: f8(ohlcv(rng, n, T), *OHLC), lambda api, a: api.cdl(CDL_ONE, *[a[c] for c in OHLC]),
      lambda d: {"": O.pattern(CDL_ONE, *[d[c] for c in OHLC])})
entry("cdl_all", lambda rng, n, T: f8(ohlcv(rng, n, T), *OHLC), lambda api, a: api.cdl_all(*[a[c] for c in OHLC], names=CDL_SOME),
      lambda d: {nm: O.pattern(nm, *[d[c] for c in OHLC]) for nm in CDL_SOME})


# -- backtests
def _bt_args(series_bench):
    def args(rng, n, T):
        p = walk(rng, n, T)
        bm = walk(rng, 1, T)[0] if series_bench else walk(rng, n, T)
        return [("price", "f8", p), ("buy", "u8", sig(rng, n, T)), ("sell", "u8", sig(rng, n, T)),
                ("benchmark", "ser" if series_bench else "f8", bm)]
    return args


entry("backtest_vectorized", _bt_args(False), lambda api, a: api.backtest_vectorized(a["price"], a["buy"], a["sell"], a["benchmark"]),
      lambda d: tup(O.backtest(d["price"], d["buy"], d["sell"], d["benchmark"])))
entry("backtest_leveraged", _bt_args(True),
      lambda api, a: api.backtest_leveraged(a["price"], a["buy"], a["sell"], a["benchmark"], max_trades=8),
      lambda d: O.backtest_leveraged(d["price"], d["buy"], d["sell"], d["benchmark"], max_trades=8))
entry("backtest_report", lambda rng, n, T: [("total_value", "f8", 1000.0 * walk(rng, n, T)), ("benchmark", "ser", walk(rng, 1, T)[0])],
      lambda api, a: api.backtest_report(a["total_value"], 100000.0, a["benchmark"]),
      lambda d: {"": RP.report(d["total_value"], 100000.0, d["benchmark"])})


def _sweep_args(rng, n, T):
    p = walk(rng, n, T)
    return [("price", "f8", p), ("line0", "f8", p * (1.0 + 0.02 * rng.standard_normal((n, T)))),
            ("line1", "f8", p * (1.0 + 0.02 * rng.standard_normal((n, T)))), ("benchmark", "f8", walk(rng, n, T))]


SWEEP = {"rule": [0, 1], "a": [0, 0], "b": [1, 0], "k0": [0.0, 97.0], "k1": [0.0, 103.0]}


def _sweep_ref(d):
    n = d["price"].shape[0]
    lines = [d["line0"], d["line1"]]
    cells = [[SW.sweep_cell(d["price"][s], lines[a][s], lines[b][s], rule, k0, k1, bench=d["benchmark"][s]) for s in range(n)]
             for rule, a, b, k0, k1 in zip(*[SWEEP[k] for k in ("rule", "a", "b", "k0", "k1")])]
    return {"": np.array(cells, dtype=np.float64).reshape(2, n, 8)}


entry("backtest_sweep", _sweep_args,
      lambda api, a: api.backtest_sweep(a["price"], [a["line0"], a["line1"]], api.sweep_params(SWEEP), benchmark=a["benchmark"]), _sweep_ref)

# -- rule helpers on _batch(dense=True)
entry("cross_signals", lambda rng, n, T: [("a", "f8", walk(rng, n, T)), ("b", "f8", walk(rng, n, T))],
      lambda api, a: api.cross_signals(a["a"], a["b"]), lambda d: tup(O.cross_signals(d["a"], d["b"])))
entry("channel_signals",
      lambda rng, n, T: [("price", "f8", walk(rng, n, T)), ("lo", "f8", walk(rng, n, T) * 0.99), ("hi", "f8", walk(rng, n, T) * 1.01)],
      lambda api, a: api.channel_signals(a["price"], a["lo"], a["hi"], 0),
      lambda d: tup(O.channel_signals(d["price"], d["lo"], d["hi"], 0)))
entry("gate_signals",
      lambda rng, n, T: [("buy", "u8", sig(rng, n, T, 0.6)), ("sell", "u8", sig(rng, n, T, 0.6)), ("a", "f8", walk(rng, n, T)),
                         ("c", "f8", walk(rng, n, T))],
      lambda api, a: api.gate_signals(a["buy"], a["sell"], a["a"], 2, 0.0, 0.0, a["c"]),
      lambda d: tup(SR.gate_signals(d["a"], d["c"], 2, 0.0, 0.0, d["buy"], d["sell"])))


# -- factor evaluation
def _fr(rng, n, T):
    return [("factor", "f8", fac(rng, n, T)), ("ret", "f8", 0.02 * fac(rng, n, T))]


def _groups_ref(mode, **kw):
    def ref(d):
        g = X.groups(d["factor"], d["ret"], mode, **kw)
        g["summary"] = X.summary(g)
        if mode == 1:
            g["ls_return"] = g.pop("spread")
        return g
    return ref


entry("factor_ic", _fr, lambda api, a: api.factor_ic(a["factor"], a["ret"], 0), lambda d: tup(O.factor_ic(d["factor"], d["ret"], 0)))
entry("factor_quantiles", _fr, lambda api, a: api.factor_quantiles(a["factor"], a["ret"], 2, labels=True), _groups_ref(0, q=2))
entry("factor_long_short", _fr, lambda api, a: api.factor_long_short(a["factor"], a["ret"], 0.4, 0.4, labels=True),
      _groups_ref(1, top=0.4, bottom=0.4))


def _double_ref(d):
    g = XD.groups(d["control"], d["factor"], d["ret"], 2, 2, True)
    g["summary"] = XD.summary(g)
    return g


entry("factor_double_sort", lambda rng, n, T: [("control", "f8", fac(rng, n, T))] + _fr(rng, n, T),
      lambda api, a: api.factor_double_sort(a["control"], a["factor"], a["ret"], 2, 2, True, labels=True), _double_ref)


def _days(T):
    return [min(1, T - 1)] if T > 0 else []


entry("factor_portfolio",
      lambda rng, n, T: [("labels", "u8", rng.choice(np.array([0, 1, 254, 255], dtype=np.uint8), size=(n, T), p=[0.4, 0.4, 0.1, 0.1])),
                         ("price", "f8", walk(rng, n, T)), ("weight", "f8", pos(rng, n, T))],
      lambda api, a: api.factor_portfolio(a["labels"], a["price"], 2, _days(a["price"].shape[1]), weight=a["weight"], cost_rate=0.001),
      lambda d: PF.portfolio(d["labels"], d["price"], 2, _days(d["price"].shape[1]), weight=d["weight"], cost_rate=0.001))


def _codes(rng, n, T=None):
    return rng.integers(-1, 2, size=(n,) if T is None else (n, T)).astype(np.int64)


entry("factor_clean_log_cap", lambda rng, n, T: [("factor", "f8", fac(rng, n, T)), ("cap", "f8", pos(rng, n, T))],
      lambda api, a: api.factor_clean(a["factor"], winsorize="mad", cap=a["cap"], log_cap=True, standardize=True),
      lambda d: {"": XC.clean(d["factor"], "mad", None, z=np.log(d["cap"]), standardize=True)})
entry("factor_clean_cap_industry",
      lambda rng, n, T: [("factor", "f8", fac(rng, n, T)), ("cap", "f8", pos(rng, n, T)), ("industry", "code2", _codes(rng, n, T))],
      lambda api, a: api.factor_clean(a["factor"], winsorize="sigma", cap=a["cap"], log_cap=False, industry=a["industry"]),
      lambda d: {"": XC.clean(d["factor"], "sigma", None, z=d["cap"], industry=d["industry"])})
entry("factor_clean_industry_per_symbol", lambda rng, n, T: [("factor", "f8", fac(rng, n, T)), ("industry", "code1", _codes(rng, n))],
      lambda api, a: api.factor_clean(a["factor"], industry=a["industry"], standardize=True),
      lambda d: {"": XC.clean(d["factor"], industry=d["industry"], standardize=True)})


def _regress_keys(r, n_key="n"):
    return {"coef": r["coef"], "t_stat": r["t"], "p_value": r["p"], "r_squared": r["r2"], n_key: r["n"]}


def _xsec_regress_ref(d):
    r = RG.xsec_regress([d["f0"]], d["ret"])
    return {**_regress_keys(r), "summary": RG.fm_summary(r["coef"])}


entry("xsec_regress", lambda rng, n, T: [("f0", "f8", fac(rng, n, T, 0.0)), ("ret", "f8", 0.02 * fac(rng, n, T, 0.02))],
      lambda api, a: api.xsec_regress([a["f0"]], a["ret"]), _xsec_regress_ref)


def _f_mkt_y(rng, n, T):
    return [("f0", "f8", fac(rng, n, T)), ("market", "ser", 0.01 * rng.standard_normal(T)), ("y", "f8", 0.02 * fac(rng, n, T))]


entry("ts_regress", _f_mkt_y, lambda api, a: api.ts_regress([a["f0"], a["market"]], a["y"]),
      lambda d: _regress_keys(RG.ts_regress([d["f0"], d["market"]], d["y"]), "n_obs"))
entry("factor_rolling_regress", _f_mkt_y, lambda api, a: api.factor_rolling_regress(a["y"], [a["f0"], a["market"]], 4),
      lambda d: RR.rolling_regress(d["y"], [d["f0"], d["market"]], 4))


def _linear_ref(d):
    r = LN.linear([d["x0"], d["x1"]], d["y"])
    return {**_regress_keys(r), "pred": r["pred"], "resid": r["resid"]}


entry("linear", lambda rng, n, T: [("x0", "f8", fac(rng, n, T)), ("x1", "f8", fac(rng, n, T)), ("y", "f8", fac(rng, n, T))],
      lambda api, a: api.linear([a["x0"], a["x1"]], a["y"]), _linear_ref)


def _two(rng, n, T):
    return [("f0", "f8", fac(rng, n, T)), ("f1", "f8", fac(rng, n, T))]


def _orth_out(api, a):
    cols = [a["f0"], a["f1"]]
    n, T = a["f0"].shape
    if n == 0 or T == 0:
        return api.factor_orthogonalize(cols, 0, out=[torch.empty((n, T), dtype=torch.float64, device="cuda")])
    mats = api._same_layout([api._to_device(c)[0] for c in cols])          # the pitch the call will run on
    s = api._batch(mats[0]).stride
    out = [torch.full((n, s), SENT, dtype=torch.float64, device="cuda")[:, :T]]
    res = api.factor_orthogonalize(cols, 0, out=out)
    assert res[0] is out[0]
    return res


entry("factor_orthogonalize", _two, lambda api, a: api.factor_orthogonalize([a["f0"], a["f1"]], 0),
      lambda d: {"": XO.orthogonalize(np.stack([d["f0"], d["f1"]]))})
entry("factor_orthogonalize_out", _two, _orth_out, lambda d: {"0": XO.orthogonalize(np.stack([d["f0"], d["f1"]]))[0]})
entry("factor_combine", _two, lambda api, a: api.factor_combine([a["f0"], a["f1"]], np.array([0.75, -0.5])),
      lambda d: {"": CB.composite([d["f0"], d["f1"]], np.array([0.75, -0.5]), True)})


def _ic_rows_ref(fn):
    def ref(d):
        ic, nv, summ = fn(d)
        return {"ic": ic, "n_valid": nv, "summary": summ}
    return ref


entry("ic_decay", _fr, lambda api, a: api.ic_decay(a["factor"], a["ret"], 2, 0), _ic_rows_ref(lambda d: RB.ic_decay(d["factor"], d["ret"], 2, 0)))
entry("ic_subgroup", lambda rng, n, T: _fr(rng, n, T) + [("group", "code2", np.abs(_codes(rng, n, T)))],
      lambda api, a: api.ic_subgroup(a["factor"], a["ret"], a["group"], 0),
      _ic_rows_ref(lambda d: RB.ic_subgroup(d["factor"], d["ret"], d["group"], 0)))
entry("ic_subgroup_per_symbol", lambda rng, n, T: _fr(rng, n, T) + [("group", "code1", np.abs(_codes(rng, n)))],
      lambda api, a: api.ic_subgroup(a["factor"], a["ret"], a["group"], 0),
      _ic_rows_ref(lambda d: RB.ic_subgroup(d["factor"], d["ret"], d["group"], 0)))

# -- factor building
_one = lambda rng, n, T: [("x", "f8", fac(rng, n, T))]
_price = lambda rng, n, T: [("x", "f8", walk(rng, n, T))]
entry("factor_rank", _one, lambda api, a: api.factor_rank(a["x"], 0), lambda d: {"": XB.rank(d["x"], "rank")})
entry("factor_normalize", _one, lambda api, a: api.factor_normalize(a["x"], "minmax"), lambda d: {"": XB.minmax(d["x"])})
entry("factor_weighted",
      lambda rng, n, T: [("factor", "f8", fac(rng, n, T)), ("weight", "f8", pos(rng, n, T)), ("group", "code2", _codes(rng, n, T))],
      lambda api, a: api.factor_weighted(a["factor"], a["weight"], a["group"]),
      lambda d: {"": XB.weighted(d["factor"], d["weight"], d["group"], max(int(d["group"].max()) + 1, 1))})
entry("factor_binary", _two, lambda api, a: api.factor_binary(a["f0"], a["f1"], 0), lambda d: {"": XB.binary(d["f0"], d["f1"], "ratio")})
entry("factor_rolling", _price, lambda api, a: api.factor_rolling(a["x"], 0, 3), lambda d: {"": RL.rolling(d["x"], "mean", 3)})
entry("factor_ts", _one, lambda api, a: api.factor_ts(a["x"], 0, 3), lambda d: {"": TS.ts(d["x"], "sum", 3)})
entry("factor_ts_pair", _two, lambda api, a: api.factor_ts_pair(a["f0"], a["f1"], 1, 3), lambda d: {"": TS.ts_pair(d["f0"], d["f1"], "corr", 3)})


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api(oracle):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from polars_quant_amd import api
    from polars_quant_amd._lib import lib
    lib()
    return api


def dense_dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def run_matrix(api, e, n, T, around=None):
    """the baseline, its anchor, and every assignment under both poisons; around(call) wraps each laid-out call (the wave-form counter)"""
    rng = np.random.default_rng([SEED, n, T] + [ord(c) for c in e.name])
    args = e.args(rng, n, T)
    tag0 = f"{e.name} {n}x{T}"
    base = invoke(api, e, {nm: dense_dev(arr) for nm, _k, arr in args})
    live = n * T > 0
    if isinstance(base, Refused):
        assert not live or T == 1, f"{tag0}: the dense call was refused: {base.kind}: {base.msg}"
    elif e.ref is not None and live and T > 1:
        anchor(tag0, base, flatten(e.ref({nm: arr for nm, _k, arr in args})))
    cache, calls = {}, 0
    for asg in assignments([k for _nm, k, _a in args], n):
        for poison in POISON:
            if poison == "inf" and all(L in ("H", "F") for L in asg):
                continue
            a, bufs = {}, []
            for (nm, kind, arr), L in zip(args, asg):
                key = (nm, L, poison)
                if key not in cache:
                    obj, raw = lay(arr, kind, L, poison)
                    cache[key] = (obj, raw, None if raw is None else raw.clone())
                obj, raw, pristine = cache[key]
                a[nm] = obj
                if raw is not None:
                    bufs.append((nm, raw, pristine))
            tag = f"{tag0} layouts {'/'.join(asg)} poison {poison}"
            got = invoke(api, e, a) if around is None else around(asg, lambda: invoke(api, e, a))
            calls += 1
            same_bits(tag, got, base, bits=live)
            for nm, raw, pristine in bufs:
                assert torch.equal(raw, pristine), f"{tag}: the buffer of argument {nm} was modified"
    return calls


CASES = [(name, shape) for name in ENTRIES for shape in SHAPES]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{nm}-{n}x{T}" for nm, (n, T) in CASES])
def test_layouts_do_not_change_the_result(api, name, shape):
    assert run_matrix(api, ENTRIES[name], *shape) > 8


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fn", ["atr", "ema", "macd"])
def test_wave_form_and_tiled_forms_agree(api, monkeypatch, fn, n):
    """T = 1100 under PQ_WT_ALL=1: an aligned even pitch runs the wave-per-symbol form, an odd pitch or a base 8 bytes off the 8-byte
    form -- and a mixed assignment whichever its re-housed columns land on"""
    monkeypatch.setenv("PQ_WT_ALL", "1")
    took = {}

    def around(asg, call):
        api.wt_stats(reset=True)
        got = call()
        took[asg] = took.get(asg, 0) + (api.wt_stats()[0] > 0)
        return got
    run_matrix(api, ENTRIES[f"call_{fn}"], n, 1100, around)
    wave = [a for a, k in took.items() if k]
    assert wave and len(wave) < len(took), f"{fn} {n}x1100: the wave form ran under {len(wave)} of {len(took)} assignments"


def test_arrow_inputs(api):
    """pyarrow arrays (one [T] series each; call and cdl take them) give the bits of the dense device call, as arrow arrays"""
    pa = pytest.importorskip("pyarrow")
    for name in ("call_atr_series", "cdl"):
        e = ENTRIES[name]
        for T in (37, 48):
            rng = np.random.default_rng([SEED, T])
            args = [(nm, arr if arr.ndim == 1 else arr[0]) for nm, _k, arr in e.args(rng, 1, T)]
            base = invoke(api, e, {nm: dense_dev(arr) for nm, arr in args})
            assert not isinstance(base, Refused)
            out = e.run(api, {nm: pa.array(arr) for nm, arr in args})
            for o in (out if isinstance(out, tuple) else (out,)):
                assert isinstance(o, pa.Array)
            same_bits(f"{name} T={T} arrow", flatten(out), base)
            mixed = {nm: (pa.array(arr) if i == 0 else lay(arr, "ser", "S", "null")[0]) for i, (nm, arr) in enumerate(args)}
            same_bits(f"{name} T={T} arrow first, x[::2] behind", flatten(e.run(api, mixed)), base)


def test_size_one_dimensions_at_the_other_stride_checks(api):
    """the stride(0) / is_contiguous() sites outside _same_layout under torch's rule for size-1 dimensions: backtest_report takes a
    one-row curve whose ignored stride is below T, and an expanded one-day column; sweep_select takes a one-symbol, one-set summary
    whose permuted view torch calls contiguous whatever its strides"""
    rng = np.random.default_rng(SEED)
    T = 37
    v = 1000.0 * walk(rng, 1, T)
    base = api.backtest_report(dense_dev(v), 100000.0)
    row = dense_dev(v)[0].as_strided((1, T), (1, 1))
    assert row.is_contiguous() and row.stride(0) < T
    assert torch.equal(api.backtest_report(row, 100000.0).view(torch.int64), base.view(torch.int64))
    day = dense_dev(v[:, :1])
    exp3 = api.backtest_report(day.repeat(3, 1), 100000.0)
    assert torch.equal(api.backtest_report(day.expand(3, 1), 100000.0).view(torch.int64), exp3.view(torch.int64))

    d = {nm: arr for nm, _k, arr in _sweep_args(rng, 1, T)}
    tab = api.sweep_params({"rule": [0], "a": [0], "b": [1]})
    summ = api.backtest_sweep(dense_dev(d["price"]), [dense_dev(d["line0"]), dense_dev(d["line1"])], tab, windows=[[0, 20], [20, T]])
    assert tuple(summ.shape) == (2, 1, 1, 8)
    exp = api.sweep_select(summ.contiguous(), [0], [1], 0)
    odd = torch.empty(16, dtype=torch.float64, device="cuda").as_strided((2, 1, 1, 8), (8, 3, 5, 1))   # size-1 strides of its own
    odd.copy_(summ)
    assert odd.permute(0, 2, 1, 3).is_contiguous() and odd.stride() != summ.contiguous().stride()
    got = api.sweep_select(odd, [0], [1], 0)
    for g, x in zip(got, exp):
        assert g.shape == x.shape and g.cpu().numpy().tobytes() == x.cpu().numpy().tobytes()

    # backtest_sequential: one tape (B = 1), out= tensors whose row stride is their own -- torch calls them contiguous, and the one
    # row the engine writes starts at their data pointer
    import seq_ref
    A, Ts = 5, 12
    tape = seq_ref.random_tape(44, Ts, A, 6)
    exp = api.backtest_sequential(*tape, A)
    spec = {"equity": (Ts, torch.float64), "cash": (Ts, torch.float64), "position": (A, torch.float64), "counts": (2, torch.int64),
            "summary": (8, torch.float64)}
    out = {k: torch.zeros(3 * w + 7, dtype=dt, device="cuda").as_strided((1, w), (w + 3, 1), 2) for k, (w, dt) in spec.items()}
    assert all(t.is_contiguous() and t.stride(0) != t.shape[1] for t in out.values())
    got = api.backtest_sequential(*tape, A, out=out)
    for k in spec:
        assert got[k] is out[k]
        assert got[k].cpu().numpy().tobytes() == exp[k].cpu().numpy().tobytes(), k
