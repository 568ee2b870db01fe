"""The CPU oracle is CAUSAL in time and independent across series -- the premise of the ragged re-housing (csrc/pq_dev.h above RgGather:
"row t of a series depends on rows <= t of that series only"), of the time-split job forms and of every backtest built on these columns.
The HIP kernels are held to the oracle bit for bit, so a look-ahead in the oracle would be copied faithfully into every kernel and every
parity test would agree with it; here the property itself is pinned, on the oracle (no GPU).

  prefix        f(X[:, :c]) is bit for bit the first c columns of f(X), for cuts c around every tile and block size of the kernels
  independence  row i of f(X) is bit for bit f(X[i]) passed alone

for every function of SPEC and EXTRA, every candlestick recogniser, macd_cross_signals and the row outputs of both backtests (their
summaries are statistics of the whole series and are not rows), on a clean and a dirty data set (NULLs, a NULL prefix, a series that goes
fully NULL, a NaN, +-inf), at the wrapper defaults and at the short parameters of tests/parity_util.py.  No tolerance: the oracle is the
same code on the same machine, so transcendental rows are bit-equal as well (equal NaNs count as equal; the NULL pattern is compared by
its bits)."""
import numpy as np
import pytest

from oracle import pq_oracle as _spec   # (names only: the library is built by the `oracle` fixture)
from parity_util import clean_data, dirty_data, param_sets, same_bits

SEED = 0x5EED0002
N, T = 6, 420
# 1, the values around the tile / block sizes 8, 16, 32, 64, 128, 256 of the kernels, and T - 1
CUTS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300, T - 1]
FUNCS = sorted(_spec.SPEC) + sorted(_spec.EXTRA)

# Functions whose prefix property does NOT hold, each with the reference lines the oracle restates that make it so.  The re-housing path
# must refuse such an op (Op::RG_GATHER, or IsPackable cleared): its premise is false for it.  Empty: none is known.
NON_CAUSAL = {}


@pytest.fixture(scope="module")
def sets(oracle):
    clean = clean_data(oracle, SEED, N, T, 0)
    rich = clean_data(oracle, SEED + 1, N, T, 1)     # candles on which the recognisers fire
    return {"clean": clean, "dirty": dirty_data(oracle, clean), "rich": rich, "rich-dirty": dirty_data(oracle, rich)}


def check_causal(tag, f, cols):
    """f(list of [n, t] or [t] arrays) -> tuple of row outputs; cols: the [N, T] inputs"""
    full = f(cols)
    for k, a in enumerate(full):
        assert a.shape == (N, T), (tag, k, a.shape)
    for c in CUTS:
        part = f([np.ascontiguousarray(x[:, :c]) for x in cols])
        for k, (p, a) in enumerate(zip(part, full)):
            ok = same_bits(p, a[:, :c])
            assert ok.all(), (f"{tag}[{k}]: the output on the first {c} rows is not the prefix of the full output: first at "
                              f"{np.argwhere(~ok)[:3].tolist()}, {p[~ok][:3]} against {a[:, :c][~ok][:3]}")
    for i in range(N):
        alone = f([np.ascontiguousarray(x[i]) for x in cols])
        for k, (p, a) in enumerate(zip(alone, full)):
            ok = same_bits(np.asarray(p).reshape(-1), a[i])
            assert ok.all(), f"{tag}[{k}]: series {i} alone differs from its row of the panel at rows {np.argwhere(~ok)[:3].ravel().tolist()}"


def test_no_exclusion_without_a_citation():
    for name, why in NON_CAUSAL.items():
        assert name in FUNCS or name in _spec.PATTERN_NAMES, name
        assert ".rs:" in why, f"{name}: an entry of NON_CAUSAL cites the reference lines that the oracle restates"


@pytest.mark.parametrize("which", ["clean", "dirty"])
@pytest.mark.parametrize("name", FUNCS)
def test_indicator_is_causal(oracle, sets, name, which):
    if name in NON_CAUSAL:
        pytest.fail(f"{name} is listed as non-causal ({NON_CAUSAL[name]}): the re-housing path must refuse it, and this test stays red "
                    "until the entry is reviewed")
    d = sets[which]
    for tag, prm in param_sets(oracle, name) + ([("log", dict(period=3, method=1))] if name == "returns" else []):
        check_causal(f"{name} ({tag}, {which})", lambda cols: oracle.call(name, *cols, **prm), [d[c] for c in oracle.input_cols(name)])


@pytest.mark.parametrize("which", ["rich", "rich-dirty", "clean"])
@pytest.mark.parametrize("name", _spec.PATTERN_NAMES)
def test_pattern_is_causal(oracle, sets, name, which):
    d = sets[which]
    pens = [None] + ([0.1] if name in ("cdldarkcloudcover", "cdleveningdojistar", "cdleveningstar", "cdlmathold", "cdlmorningdojistar",
                                       "cdlmorningstar", "cdlpiercing", "cdlabandonedbaby") else [])
    for pen in pens:
        check_causal(f"{name} (penetration {pen}, {which})", lambda cols: (oracle.pattern(name, *cols, penetration=pen),),
                     [d[c] for c in ("open", "high", "low", "close")])


@pytest.mark.parametrize("which", ["clean", "dirty"])
def test_macd_cross_signals_are_causal(oracle, sets, which):
    for prm in (dict(), dict(fast=3, slow=7, sig=4)):
        check_causal(f"macd_cross_signals{prm} ({which})", lambda cols: oracle.macd_cross_signals(cols[0], **prm), [sets[which]["close"]])


def _signals(shape, p):
    rng = np.random.default_rng(5)
    return (rng.random(shape) < p).astype(np.uint8), (rng.random(shape) < p).astype(np.uint8)


@pytest.mark.parametrize("which", ["clean", "dirty"])
def test_backtest_rows_are_causal(oracle, sets, which):
    """position, cash and equity of the vectorized backtest (the summary is over the whole series)"""
    buy, sell = _signals((N, T), 0.05)
    for kw in (dict(), dict(buy_slippage=0.01, sell_slippage=0.02, position_size=0.5, min_commission=1.0)):
        def f(cols):
            b, s = (np.ascontiguousarray(x.astype(np.uint8)) for x in cols[1:])
            return oracle.backtest(cols[0], b, s, **kw)[:3]
        check_causal(f"backtest{kw} ({which})", f, [sets[which]["close"], buy.astype(np.float64), sell.astype(np.float64)])


@pytest.mark.parametrize("which", ["clean", "dirty"])
def test_leveraged_backtest_rows_are_causal(oracle, sets, which):
    """cash, stock value and total value of the leveraged backtest (trade list and summary are over the whole series)"""
    buy, sell = _signals((N, T), 0.05)
    for kw in (dict(), dict(leverage=3.0, margin_call_threshold=0.5, slippage=0.01, position_size=0.7)):
        def f(cols):
            one = cols[0].ndim == 1
            b, s = (np.ascontiguousarray(x.astype(np.uint8)) for x in cols[1:])
            r = oracle.backtest_leveraged(cols[0], b, s, **kw)
            rows = (r["cash"], r["stock_value"], r["total_value"])
            return tuple(a[0] for a in rows) if one else rows
        check_causal(f"backtest_leveraged{kw} ({which})", f, [sets[which]["close"], buy.astype(np.float64), sell.astype(np.float64)])
