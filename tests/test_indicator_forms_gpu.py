"""-m gpu: DIRECT calls (not recorded into a suite) of the 62 indicators, the 3 extras, the 61 candlestick recognisers and the fused
multi-output entry points, through the C ABI on caller-owned buffers, at every tile remainder, row pitch and kernel form that
csrc/pq_dev.h chooses between -- against the oracle on the dense [n, T] block, bit for bit (tests/tolerance.py's rule for the outputs
that pass through a device transcendental; nothing else has a tolerance).

Every input and output column is a buffer of n + 2 rows at the case's pitch of which the middle n are the batch: a guard row in front
of the first series and one behind the last.  Outputs are prefilled with a sentinel no function produces; after the call every live
cell differs from it and equals the oracle, and every padding and guard cell still holds it.  The padding and the guard rows of the
INPUTS hold poison -- each case runs once with the NULL pattern (a null-transparent op would silently skip it) and once with +inf (which
propagates through every sum and extremum): a row read as data beyond `len` changes a live output in one of the two runs.  Inputs are
compared with a pristine copy after the call.

Layouts (T the length, rs(T) = recommended_stride(T), the next multiple of 16 elements):

| layout | row pitch                      | base            | form it reaches                                                          |
|--------|--------------------------------|-----------------|--------------------------------------------------------------------------|
| A      | T                              | 16-byte aligned | even T: the 16-byte tiled body; odd T: its 8-byte form                   |
| B      | rs(T)                          | 16-byte aligned | 16-byte tiled body, odd lengths under an even pitch (bench.py's layout)  |
| C      | T + 1 (T even), T + 2 (T odd)  | 16-byte aligned | 8-byte form, with padding behind every row                               |
| D      | rs(T)                          | + one element   | 8-byte form through the misaligned base alone (even pitch)               |
| E      | 2^22                           | 16-byte aligned | per-lane gather body on a REGULAR batch (n = 2; no guard rows: 64 MB a column) |

Where each branch of the dispatch is reached (the failure tag names entry point, parameters, n x T, layout and poison):

| branch                                                              | case                                                                  |
|---------------------------------------------------------------------|-----------------------------------------------------------------------|
| seq_cols_tiling -> 0 (seq_cols_aligned), launch_seq:                | test_tile_remainders, layouts A (even T) and B: T = 112 .. 128 is      |
|   seq_kernel<Op, true>, run_seq_lds<Op, false>; tiles of 16 rows    |   every remainder 0 .. 15 of the 16-row tile and 0 .. 7 of the 8-row   |
|   (TileK: PQ_K11, 1 in / 1 out), 8 rows (PQ_KXX), 4 (ULTOSC's       |   tile, 112 and 128 whole tiles; n = 66 = a full 64-series tile + 2    |
|   TILE_K) by 64 series                                              |   (the dead series of the last tile)                                   |
| seq_cols_tiling -> 1 by an odd pitch: seq_kernel<Op, true, true>    | test_tile_remainders, layouts A (odd T) and C                          |
| seq_cols_tiling -> 1 by a base 8 bytes off under an even pitch      | test_tile_remainders, layout D                                         |
| seq_cols_tiling -> -1 by stride >= 2^22: seq_kernel<Op, false>,     | test_huge_pitch_runs_the_gather_body (layout E, T = 121 live rows)     |
|   run_seq on a regular batch; an LDS-only fused op: its chain       |                                                                        |
| seq_lds_bytes > SEQ_LDS_LIMIT: the gather body behind a long window | test_long_window_runs_the_gather_body: period 200 (the smallest ring,  |
|   with live rows                                                    |   SMA's ring_slots() = p, is 200 x 512 B = 102 400 B > 65 536 B before |
|                                                                     |   any tile), T = 257, n = 66, layout B: rows 199 .. 256 are live       |
| a window of T - 1, T, T + 1 rows (one live row, none, none)         | test_period_at_the_series_length: every function with a `timeperiod`   |
| direct_lane (Op::DIRECT_LANE_MAX: SAR / SAREXT, OBV, the Hilbert    | test_tile_remainders (the default: the per-lane form) and              |
|   functions and MAMA, STOCH / STOCHF / STOCHRSI and the fused forms |   test_direct_lane_switched_off (PQ_NO_DIRECT_LANE=1: the tiled forms  |
|   over them) and seq_can_lds's refusal of an LDS-only op under it   |   of the same ops, and the fused forms as one job)                     |
| launch_row: row_kernel, ROW_BLOCK = 256 rows a block (the price     | test_row_block_edges: T = 255, 256, 257 (one block less a row, one,    |
|   functions, TRANGE, BOP, the lag family, HT_TRENDMODE, MIDPRICE)   |   two); also 16 and 32 tiles of 16 / 8 rows with a 1-row tail behind   |
| launch_row against launch_seq for MIDPRICE                          | test_midprice_both_forms (PQ_MIDPRICE_SEQ=1: the SEQ op)               |
| mama_zero_kernel against the walk at fastlimit = 0                  | test_mama_zero_both_forms (PQ_MAMA_WALK=1: HtOp<4>'s walk)             |
| series shorter than every warm-up and than a tile                   | test_short_series: T = 1, 2, 15, 16, 17, all functions, layouts A, C   |
| n = 1 (a lone series), 63, 64, 65 (around the 64-series tile), 129  | test_series_counts at T = 120 and 121, layouts A and B                 |
| cdl_one_kernel / cdl_all_kernel<*, vec>                             | every block with pq_cdl (61 recognisers, layouts A, B) and pq_cdl_all  |

PQ_TEST_FORM_LAYOUTS=B (any subset of ABCDE) restricts a run to those layouts.  It is there for runs against a deliberately broken
build: in layout B the end of the last tile lies inside the row pitch, so a tail that reads or stores up to it stays inside the test's
own buffers.  Three such builds of run_seq_lds's tail were tried when the module was written -- the tail walked on to the tile end;
only live rows computed but the whole tile stored; the last live row reading the cell behind it -- and each failed some 190 tests: the
first two on "cells outside the batch were written", the third on the comparison with the oracle under both poisons.
"""
import ctypes as C
import os

import numpy as np
import pytest

from parity_util import NULL_BITS, SHORT, TRANSCENDENTAL, assert_same, clean_data

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pq_oracle as O   # noqa: E402  (names, defaults and the expected values; the `oracle` fixture builds the library)

SEED = 0x5EED0F02
N_MAX, T_MAX = 129, 257
SENT = -7.25e300           # f64 sentinel of outputs (no indicator produces it)
SENT_I32 = -1234567        # int32 sentinel: odd, and no recogniser value (0, +-100, +-200) or trend mode (0, 1)
POISON = {"null": NULL_BITS, "inf": 0x7FF0000000000000}   # bit patterns of the inputs' padding and guard rows
HUGE = 1 << 22             # the row pitch from which seq_cols_tiling gives up the tiled body
POOL_COLS = 12             # layout E: at most 5 inputs + 7 outputs (pq_dm_system_all) are live at once
ONLY_LAYOUTS = os.environ.get("PQ_TEST_FORM_LAYOUTS", "ABCDE")   # a subset of the layouts: for a run against a deliberately broken build


def rs(T):
    return (T + 15) // 16 * 16


def geometry(layout, T):
    """-> (row pitch in elements, offset of the base in elements, guard rows on either side)"""
    return {"A": (T, 0, 1), "B": (rs(T), 0, 1), "C": (T + 1 if T % 2 == 0 else T + 2, 0, 1), "D": (rs(T), 1, 1), "E": (HUGE, 0, 0)}[layout]


class Entry:
    """one entry point of include/pq_hip.h: id, C name, input columns, {parameter-set tag: (scalar arguments, [(oracle function, its
    parameters)] whose outputs, in order, are the entry point's output columns)}, the data set it runs on and the layouts it is run on"""

    def __init__(self, id_, cname, cols, sets, rich=False, layouts="ABCD", invoke=None):
        self.id, self.cname, self.cols, self.sets, self.rich, self.layouts, self.invoke = id_, cname, cols, sets, rich, layouts, invoke

    def outputs(self, tag):
        """[(oracle function, parameters, index of the output, name, dtype)]"""
        res = []
        for fn, prm in self.sets[tag][1]:
            outs = [(fn, "i4")] if fn in O.PATTERN_NAMES else (O.SPEC[fn] if fn in O.SPEC else O.EXTRA[fn])[2]
            res += [(fn, prm, k, oname, dt) for k, (oname, dt) in enumerate(outs)]
        return res


def _spec_entry(name):
    cols, pspec, _outs = O.SPEC[name] if name in O.SPEC else O.EXTRA[name]
    sets = {}
    for tag, prm in [("defaults", {})] + ([("short", SHORT[name])] if name in SHORT else []):
        assert bool(pspec) or tag == "defaults"
        vals = [(int if kind == O.I else float)(prm.get(pn, default)) for pn, kind, default in pspec]
        sets[tag] = (vals, [(name, prm)])
    return Entry(name, "pq_" + name, cols, sets)


def _dflt(fn, **over):
    """the full parameter dict of oracle function fn: wrapper defaults, SHORT where `short` is passed, then `over`"""
    spec = O.SPEC[fn]
    short = over.pop("short", False)
    d = {pn: default for pn, _k, default in spec[1]}
    if short:
        d.update(SHORT.get(fn, {}))
    d.update(over)
    return d


def _fused_entries():
    E = []
    HLC, HLCV = ["high", "low", "close"], ["high", "low", "close", "volume"]

    def add(name, cols, build):
        E.append(Entry(name, "pq_" + name, cols, {"defaults": build(False), "short": build(True)}))

    def tp(fn, s):
        return _dflt(fn, short=s)["timeperiod"]

    add("ema_all", ["real"], lambda s: ([tp("ema", s)], [(f, dict(timeperiod=tp("ema", s))) for f in ("ema", "dema", "tema", "trix")]))
    add("atr_all", HLC, lambda s: ([tp("atr", s)], [(f, dict(timeperiod=tp("atr", s))) for f in ("atr", "natr")]))
    add("dm_pair", ["high", "low"], lambda s: ([tp("plus_dm", s)], [(f, dict(timeperiod=tp("plus_dm", s))) for f in ("plus_dm", "minus_dm")]))

    def ad_all(s):
        p = _dflt("adosc", short=s)
        return [p["fastperiod"], p["slowperiod"]], [("ad", {}), ("adosc", p)]
    add("ad_all", HLCV, ad_all)

    def macd_pair(s):
        m, f = _dflt("macd", short=s), _dflt("macdfix", short=s, **({"signalperiod": 5} if s else {}))
        return [m["fastperiod"], m["slowperiod"], m["signalperiod"], f["signalperiod"]], [("macd", m), ("macdfix", f)]
    add("macd_pair", ["real"], macd_pair)
    add("dm_system_all", HLC, lambda s: ([tp("adx", s)], [(f, dict(timeperiod=tp("adx", s)))
                                                          for f in ("dx", "plus_di", "minus_di", "adx", "adxr", "atr", "natr")]))
    add("sma_ma", ["real"], lambda s: ([tp("sma", s)], [("sma", dict(timeperiod=tp("sma", s))), ("ma", dict(timeperiod=tp("sma", s), matype=0))]))
    add("cmo_rsi", ["real"], lambda s: ([tp("cmo", s)], [(f, dict(timeperiod=tp("cmo", s))) for f in ("cmo", "rsi")]))

    def volume_all(s):
        m, a = _dflt("mfi", short=s), _dflt("adosc", short=s)
        return [m["timeperiod"], a["fastperiod"], a["slowperiod"]], [("mfi", m), ("ad", {}), ("adosc", a), ("obv", {})]
    E.append(Entry("volume_all", "pq_volume_all", HLCV, {"defaults": volume_all(False), "short": volume_all(True)}))
    E[-1].oracle_cols = {"obv": ["close", "volume"]}

    def sar_pair(s):
        a, x = _dflt("sar", short=s), _dflt("sarext", short=s)
        return [float(a[k]) for k in ("acceleration", "maximum")] + [float(v) for v in x.values()], [("sar", a), ("sarext", x)]
    add("sar_pair", ["high", "low"], sar_pair)

    def stoch_all(s):
        a, f = _dflt("stoch", short=s), _dflt("stochf", short=s)
        f["fastk_period"] = a["fastk_period"]
        return ([a[k] for k in ("fastk_period", "slowk_period", "slowk_matype", "slowd_period", "slowd_matype")]
                + [f["fastd_period"], f["fastd_matype"]], [("stoch", a), ("stochf", f)])
    add("stoch_all", HLC, stoch_all)

    def apo_ppo(s):
        a = _dflt("apo", short=s)
        return [a["fastperiod"], a["slowperiod"], a["matype"]], [("apo", a), ("ppo", a)]
    add("apo_ppo", ["real"], apo_ppo)
    add("aroon_all", ["high", "low"], lambda s: ([tp("aroon", s)], [(f, dict(timeperiod=tp("aroon", s))) for f in ("aroon", "aroonosc")]))
    add("dmi_all", HLC, lambda s: ([tp("dx", s)], [(f, dict(timeperiod=tp("dx", s))) for f in ("dx", "plus_di", "minus_di", "adx", "adxr")]))
    E.append(Entry("ht_all", "pq_ht_all", ["real"], {"defaults": ([], [(f, {}) for f in ("ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine")])}))
    return E


def _invoke_cdl(api, dev, b, ins, args, outs):
    api._call("pq_cdl", dev, b, args[0], *ins, args[1], *outs)


def _invoke_cdl_all(api, dev, b, ins, args, outs):
    pens = (C.c_double * 61)(*args)
    ptrs = (C.c_void_p * 61)(*[o.data_ptr() for o in outs])
    api._call("pq_cdl_all", dev, b, *ins, pens, ptrs)


OHLC = ["open", "high", "low", "close"]
FUNCS = [_spec_entry(n) for n in sorted(O.SPEC) + sorted(O.EXTRA)]
FUSED = _fused_entries()
CDL_ALL = Entry("cdl_all", "pq_cdl_all", OHLC, {"defaults": ([O.PATTERN_PEN_DEFAULT[p] for p in O.PATTERN_NAMES], [(p, {}) for p in O.PATTERN_NAMES])},
                rich=True, invoke=_invoke_cdl_all)
CDL = [Entry(p, "pq_cdl", OHLC, {"defaults": ([i, O.PATTERN_PEN_DEFAULT[p]], [(p, {})])}, rich=True, layouts="AB", invoke=_invoke_cdl)
       for i, p in enumerate(O.PATTERN_NAMES)]
ENTRIES = {e.id: e for e in FUNCS + FUSED + [CDL_ALL] + CDL}
assert len(ENTRIES) == 65 + 15 + 1 + 61
CASES = [(e.id, tag) for e in ENTRIES.values() for tag in e.sets]
F64_CASES = [(e.id, tag) for e in FUNCS + FUSED for tag in e.sets]
ids = lambda cases: [f"{i}-{t}" for i, t in cases]

# the shapes of each block: (n, T, layout)
TAIL = [(66, T, L) for T in range(112, 129) for L in "ABCD"]
ROWBLOCK = [(3, T, L) for T in (255, 256, 257) for L in "AB"]
SHORT_T = [(3, T, L) for T in (1, 2, 15, 16, 17) for L in "AC"]
SERIES = [(n, T, L) for n in (1, 63, 64, 65, 129) for T in (120, 121) for L in "AB"]

# entry points that reach an op with DIRECT_LANE_MAX (csrc/ops_overlap.h SarextOp, ops_misc.h ObvOp / HtOp, ops_fused.h StochOp / StochRsiOp;
# StochAllOp and HtAllOp are LDS-only ops that seq_can_lds refuses under it)
DIRECT_LANE = ["sar", "sarext", "obv", "ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine", "ht_trendline", "ht_trendmode", "mama", "stoch",
               "stochf", "stochrsi", "sar_pair", "volume_all", "stoch_all", "ht_all"]
# functions whose op carries a ring of `period` slots or more (ring_slots(), 512 B a slot): period 200 is 102 400 B of rings at the least
LONG_WINDOW = {"sma": dict(timeperiod=200), "wma": dict(timeperiod=200), "trima": dict(timeperiod=200), "bbands": dict(timeperiod=200),
               "midpoint": dict(timeperiod=200), "midprice": dict(timeperiod=200), "cci": dict(timeperiod=200), "willr": dict(timeperiod=200),
               "aroon": dict(timeperiod=200), "mfi": dict(timeperiod=200), "stoch": dict(fastk_period=200),
               "ultosc": dict(timeperiod1=7, timeperiod2=14, timeperiod3=200)}
TIMEPERIOD = [n for n in sorted(O.SPEC) if any(pn == "timeperiod" for pn, _k, _d in O.SPEC[n][1])]


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()
    return pq


class World:
    """the two data sets (generated once at the largest shape; a case takes the leading [n, T] block), and what is computed once and
    shared: the oracle's columns per (function, parameters, data set, shape), the dense device blocks, the poisoned input columns per
    (column, shape, layout, poison) with a pristine copy each, the masks of the cells outside the batch, layout E's pool"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.data = {False: clean_data(oracle, SEED, N_MAX, T_MAX, 0), True: clean_data(oracle, SEED + 1, N_MAX, T_MAX, 1)}
        self.ref, self.blocks, self.dense, self.inputs, self.masks = {}, {}, {}, {}, {}
        self.pool = None
        self.calls = 0

    def block(self, rich, col, n, T):
        key = (rich, col, n, T)
        if key not in self.blocks:
            a = np.ascontiguousarray(self.data[rich][col][:n, :T])
            a.setflags(write=False)
            self.blocks[key] = a
        return self.blocks[key]

    def expected(self, fn, prm, rich, n, T, cols=None):
        key = (fn, tuple(sorted(prm.items())), rich, n, T)
        if key not in self.ref:
            src = [self.block(rich, c, n, T) for c in (cols or self.oracle.input_cols(fn))]
            res = self.oracle.call(fn, *src, **prm)
            for r in res:
                r.setflags(write=False)
            self.ref[key] = res
        return self.ref[key]

    def dense_dev(self, rich, col, n, T):
        key = (rich, col, n, T)
        if key not in self.dense:
            self.dense[key] = torch.from_numpy(self.block(rich, col, n, T)).cuda()
        return self.dense[key]

    def pad_mask(self, n, T, pitch, off, guard):
        """flat boolean mask of a column buffer: True on every cell that is not a live cell of the batch"""
        key = (n, T, pitch, off, guard)
        if key not in self.masks:
            m = np.ones(off + (n + 2 * guard) * pitch, dtype=bool)
            m[off:].reshape(n + 2 * guard, pitch)[guard:guard + n, :T] = False
            self.masks[key] = m
        return self.masks[key]

    def pool_col(self, k, dtype):
        if self.pool is None:
            self.pool = torch.empty(POOL_COLS * 2 * HUGE, dtype=torch.float64, device="cuda")
        col = self.pool[k * 2 * HUGE:(k + 1) * 2 * HUGE]
        return col if dtype == torch.float64 else col.view(torch.int32)[:2 * HUGE]


@pytest.fixture(scope="module")
def world(oracle, pq):
    w = World(oracle)
    yield w
    print(f"\n[test_indicator_forms_gpu] {w.calls} direct calls checked")


def _rows(flat, n, T, pitch, off, guard):
    """the n batch rows (each `pitch` long) inside a flat column buffer"""
    return flat[off:off + (n + 2 * guard) * pitch].view(n + 2 * guard, pitch)[guard:guard + n]


def _input(W, rich, col, n, T, layout, poison, slot):
    pitch, off, guard = geometry(layout, T)
    if layout == "E":
        flat = W.pool_col(slot, torch.float64)
        flat.view(torch.int64).fill_(POISON[poison])
        _rows(flat, n, T, pitch, off, guard)[:, :T] = W.dense_dev(rich, col, n, T)
        return flat, None
    key = (rich, col, n, T, layout, poison)
    if key not in W.inputs:
        flat = torch.full((off + (n + 2 * guard) * pitch,), POISON[poison], dtype=torch.int64, device="cuda").view(torch.float64)
        _rows(flat, n, T, pitch, off, guard)[:, :T] = W.dense_dev(rich, col, n, T)
        W.inputs[key] = (flat, flat.clone())
    return W.inputs[key]


def run_case(W, entry, tag, n, T, layout, poison, args=None, comps=None):
    """one direct call of `entry` on an [n, T] batch in `layout` whose input padding holds `poison`, and every check of the module"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    pitch, off, guard = geometry(layout, T)
    if args is None:
        args, comps = entry.sets[tag]
        outs_spec = entry.outputs(tag)
    else:
        outs_spec = Entry(entry.id, entry.cname, entry.cols, {tag: (args, comps)}).outputs(tag)
    what = f"{entry.id}({tag}: {args if len(args) < 12 else '...'}) {n}x{T} layout {layout} pitch {pitch} padding {poison}"
    dev = torch.device("cuda", 0)
    ins = [_input(W, entry.rich, c, n, T, layout, poison, k) for k, c in enumerate(entry.cols)]
    outs = []
    for k, (_fn, _prm, _j, _oname, dt) in enumerate(outs_spec):
        tdt, sent = (torch.float64, SENT) if dt == "f8" else (torch.int32, SENT_I32)
        if layout == "E":
            flat = W.pool_col(len(ins) + k, tdt)
            flat.fill_(sent)
        else:
            flat = torch.full((off + (n + 2 * guard) * pitch,), sent, dtype=tdt, device="cuda")
        outs.append(flat)
    b = Batch(n, T, pitch)
    in_rows = [_rows(f, n, T, pitch, off, guard) for f, _p in ins]
    out_rows = [_rows(f, n, T, pitch, off, guard) for f in outs]
    if entry.invoke:
        entry.invoke(api, dev, b, in_rows, args, out_rows)
    else:
        api._call(entry.cname, dev, b, *in_rows, *args, *out_rows)
    W.calls += 1
    price = W.block(entry.rich, "close", n, T)
    oracle_cols = getattr(entry, "oracle_cols", {})
    for flat, rows, (fn, prm, j, oname, dt) in zip(outs, out_rows, outs_spec):
        tag_o = f"{fn}.{oname}"
        sent = SENT if dt == "f8" else SENT_I32
        if layout == "E":     # 64 MB a column: the live block comes to the host, the padding is counted on the device
            live = rows[:, :T].cpu().numpy()
            untouched = int((flat == sent).sum())
            assert untouched == flat.numel() - n * T, f"{what}: {tag_o}: {flat.numel() - n * T - untouched} padding cells were written (or live cells left)"
        else:
            host = flat.cpu().numpy()                 # (the one download of this column)
            live = host[off:].reshape(n + 2 * guard, pitch)[guard:guard + n, :T]
            outside = host[W.pad_mask(n, T, pitch, off, guard)]
            bad = outside != sent
            assert not bad.any(), (f"{what}: {tag_o}: {bad.sum()} cells outside the batch were written (flat indices "
                                   f"{np.flatnonzero(W.pad_mask(n, T, pitch, off, guard))[bad][:5].tolist()}; guard rows are the first and last "
                                   f"{pitch} cells, the rest is row padding)")
        unwritten = live == sent
        assert not unwritten.any(), f"{what}: {tag_o}: {unwritten.sum()} live cells were not written; first at {np.argwhere(unwritten)[:3].tolist()}"
        exp = W.expected(fn, prm, entry.rich, n, T, oracle_cols.get(fn))[j]
        assert_same(f"{tag_o}{{{what}}}", live, exp, exact=fn not in TRANSCENDENTAL, price=price)
    for c, (flat, pristine), rows in zip(entry.cols, ins, in_rows):
        if pristine is None:
            same = torch.equal(rows[:, :T].contiguous().view(torch.int64), W.dense_dev(entry.rich, c, n, T).view(torch.int64))
            same = same and int((flat.view(torch.int64) == POISON[poison]).sum()) == flat.numel() - n * T
        else:
            same = torch.equal(flat.view(torch.int64), pristine.view(torch.int64))
        assert same, f"{what}: input column {c} was modified"


def run_block(W, entry, tag, shapes, **kw):
    for n, T, layout in shapes:
        if layout in entry.layouts and layout in ONLY_LAYOUTS:
            for poison in POISON:
                run_case(W, entry, tag, n, T, layout, poison, **kw)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_tile_remainders(world, case):
    """T = 112 .. 128 at n = 66: every remainder of the 16-row and the 8-row tile, on layouts A - D"""
    run_block(world, ENTRIES[case[0]], case[1], TAIL)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_row_block_edges(world, case):
    """T = 255, 256, 257 at n = 3: around ROW_BLOCK and tile counts of 16 and 32"""
    run_block(world, ENTRIES[case[0]], case[1], ROWBLOCK)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_short_series(world, case):
    """T = 1, 2, 15, 16, 17: all-null or partly-null columns exactly as the oracle gives them"""
    run_block(world, ENTRIES[case[0]], case[1], SHORT_T)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_series_counts(world, case):
    """a lone series, and 63, 64, 65, 129 series: around one and two 64-series tiles"""
    run_block(world, ENTRIES[case[0]], case[1], SERIES)


@pytest.mark.parametrize("case", F64_CASES, ids=ids(F64_CASES))
def test_huge_pitch_runs_the_gather_body(world, case):
    """a regular batch at a row pitch of 2^22 elements: seq_cols_tiling returns -1"""
    e = ENTRIES[case[0]]
    for poison in POISON:
        if "E" in ONLY_LAYOUTS:
            run_case(world, e, case[1], 2, 121, "E", poison)


@pytest.mark.parametrize("name", sorted(LONG_WINDOW))
def test_long_window_runs_the_gather_body(world, name):
    """rings beyond the 64 KB LDS limit, with live rows behind the window"""
    e = ENTRIES[name]
    prm = LONG_WINDOW[name]
    args = [(int if kind == O.I else float)(prm.get(pn, d)) for pn, kind, d in O.SPEC[name][1]]
    for poison in POISON:
        run_case(world, e, "long", 66, 257, "B", poison, args=args, comps=[(name, prm)])
    exp = world.expected(name, prm, False, 66, 257)[0]
    assert (exp.view(np.uint64)[:, 210:] != np.uint64(NULL_BITS)).all(), "the rows behind the window (and STOCH's two smoothings) are live in the oracle"


@pytest.mark.parametrize("name", TIMEPERIOD)
def test_period_at_the_series_length(world, name):
    e = ENTRIES[name]
    T = 121
    for p in (T - 1, T, T + 1):
        prm = dict(timeperiod=p)
        args = [(int if kind == O.I else float)(prm.get(pn, d)) for pn, kind, d in O.SPEC[name][1]]
        for poison in POISON:
            run_case(world, e, f"timeperiod {p}", 66, T, "B", poison, args=args, comps=[(name, prm)])


DL_CASES = [(i, t) for i in DIRECT_LANE for t in ENTRIES[i].sets]


@pytest.mark.parametrize("case", DL_CASES, ids=ids(DL_CASES))
def test_direct_lane_switched_off(world, monkeypatch, case):
    """the ops with DIRECT_LANE_MAX in their tiled forms (test_tile_remainders runs them at the default: per lane)"""
    monkeypatch.setenv("PQ_NO_DIRECT_LANE", "1")
    run_block(world, ENTRIES[case[0]], case[1], TAIL)


@pytest.mark.parametrize("tag", ["defaults", "short"])
def test_midprice_both_forms(world, monkeypatch, tag):
    """the SEQ op of MIDPRICE (the other blocks run its default for a direct call, the ROW form)"""
    monkeypatch.setenv("PQ_MIDPRICE_SEQ", "1")
    for shapes in (TAIL, ROWBLOCK, SHORT_T, SERIES):
        run_block(world, ENTRIES["midprice"], tag, shapes)


@pytest.mark.parametrize("slowlimit", [0.0, 0.05])
def test_mama_zero_both_forms(world, monkeypatch, slowlimit):
    """fastlimit = 0: mama_zero_kernel by default, the walk under PQ_MAMA_WALK=1"""
    prm = dict(fastlimit=0.0, slowlimit=slowlimit)
    for walk in (False, True):
        if walk:
            monkeypatch.setenv("PQ_MAMA_WALK", "1")
        for shapes in (TAIL, ROWBLOCK, SHORT_T):
            run_block(world, ENTRIES["mama"], f"slowlimit {slowlimit}, walk {walk}", shapes, args=[0.0, slowlimit], comps=[("mama", prm)])
