"""Recorded suites the way real callers drive them, not only the record-and-replay-the-same-tensors pattern of the other suite tests:

- input binding: run(new tensors), run(the recorded tensors after an in-place change), unknown keys, re-recording after a re-housed
  record, record_staged() after one -- in place at the 128-byte pitch, re-housed from a dense odd pitch, and exact_layout=True;
- a small shard whose inputs are not all 16-byte aligned: the time-split Hilbert job inside the 8-byte job grid;
- shard parity: a rank's block of 2 500 / 1 250 / 625 symbols against the same rows of the 5 000-symbol recording;
- the gated fallback walks (NaN, inf, MAMA's finiteness bound, a failed Hilbert hand-over) recorded, replayed and called directly on a
  created, non-blocking stream."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_parity import TRANSCENDENTAL, _pitched, assert_same, bits, pq  # noqa: E402,F401  (pq: the module fixture)
from test_small_shard_gpu import STRIDE, TT, _compare_everything  # noqa: E402

HT = ("ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine")
OHLCV = ("open", "high", "low", "close", "volume")


def _same_bits(a, b):
    """bit-identical device tensors (NaN payloads included)"""
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    return torch.equal(a, b)


def _poison(st):
    """every row of every output must then be written by the next replay"""
    for t in [x for ts in st.out.values() for x in ts] + list(st.pat.values()) + st.bt + [st.summary]:
        t.fill_(-7)


# ---- A. input binding ------------------------------------------------------------------------------------------------------------

TASKS = ["sma", "ema_all", "dm_system_all", "ht_all", "cdl_all", "backtest_macd_cross"]
LAYOUTS = {   # name -> (symbols, days, Suite keyword arguments, row pitch of the caller's tensors)
    "in-place-2528": (70, TT, {"stride": STRIDE}, STRIDE),
    "rehoused-odd-pitch": (70, 301, {}, 301),
    "exact-layout": (70, 301, {"exact_layout": True}, 301),
}


def _subset_matches(pq, oracle, st, d):
    """the outputs of TASKS are the oracle's for the host data `d`"""
    from polars_quant_amd.suite import Suite
    src = dict(d, real=d["close"])
    names = ["sma"] + [m for t in TASKS if t in Suite.FUSED for m in Suite.FUSED[t]]
    for name in names:
        exp = oracle.call(name, *[src[c] for c in pq.SPEC[name][0]])
        for (oname, _), got, e in zip(pq.SPEC[name][2], st.out[name], exp):
            assert_same(f"{name}.{oname}{{binding}}", got.cpu().numpy(), e, exact=name not in TRANSCENDENTAL, price=d["close"])
    for nm in pq.PATTERN_NAMES:
        assert (st.pat[nm].cpu().numpy() == oracle.pattern(nm, d["open"], d["high"], d["low"], d["close"])).all(), nm
    ebuy, esell = oracle.macd_cross_signals(d["close"])
    epos, ecash, eeq, es = oracle.backtest(d["close"], ebuy, esell)
    for got, e in zip(st.bt, (epos, ecash, eeq)):
        g = got.cpu().numpy()
        assert ((bits(g) == bits(e)) | (np.isnan(g) & np.isnan(e))).all()
    np.testing.assert_allclose(st.summary.cpu().numpy(), es, rtol=1e-12, atol=1e-13)


def _step(pq, oracle, st, d, ohlcv=None):
    _poison(st)
    st.run(ohlcv)
    torch.cuda.synchronize()
    _subset_matches(pq, oracle, st, d)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_replay_reads_the_data_it_is_given(pq, oracle, layout):
    """run(B) with NEW tensors gives B's columns, or raises ValueError where the recording cannot honour them (a column read in
    place); an in-place change of the recorded tensors followed by run(A) gives the new columns; an unknown key raises"""
    from polars_quant_amd.suite import Suite
    n, T, kw, pitch = LAYOUTS[layout]
    da, db, dc = (oracle.gen_ohlcv(seed, n, T, 0) for seed in (0x5EED0B01, 0x5EED0B02, 0x5EED0B03))
    A = _pitched(da, pitch)
    st = Suite(n, T, "cuda", **kw)
    st.record(A, TASKS)
    rehoused = sorted(st._housed)
    assert rehoused == (sorted(OHLCV) if layout.startswith("rehoused") else []), rehoused
    _step(pq, oracle, st, da)

    B = _pitched(db, pitch)
    if rehoused:
        _step(pq, oracle, st, db, B)                       # new tensors at the caller's (odd) pitch: copied in
        # new tensors that are WELL pitched for the suite (304 elements, 16-byte aligned) must be copied as well: the recording
        # still reads its own buffers
        Bp = _pitched(dc, st.stride)
        assert all(t.stride(0) == st.stride and t.data_ptr() % 16 == 0 for t in Bp.values())
        _step(pq, oracle, st, dc, Bp)
        _step(pq, oracle, st, dc, {"close": Bp["close"]})  # a subset of the keys: the others keep what they hold
    else:
        for k in ("close", "high"):                        # a column read in place: only the recorded tensor is accepted
            with pytest.raises(ValueError, match="re-record"):
                st.run({k: B[k]})
        with pytest.raises(ValueError, match="re-record"):
            st.run({"close": A["close"][:, : T - 1]})     # the recorded buffer, another shape
        with pytest.raises(ValueError, match="re-record"):
            st.run(B)

    for k in OHLCV:                                        # the caller writes new data into the recorded tensors ...
        A[k].copy_(torch.from_numpy(db[k]))
    _step(pq, oracle, st, db, A)                           # ... and hands them back
    for k in OHLCV:
        A[k].copy_(torch.from_numpy(dc[k]))
    st.refresh_inputs(A)
    _step(pq, oracle, st, dc)                              # (refresh_inputs + run() without tensors: the same)

    with pytest.raises(ValueError, match="bogus"):
        st.run({"bogus": A["close"]})
    with pytest.raises(ValueError, match="bogus"):
        st.refresh_inputs({"close": A["close"], "bogus": A["close"]})
    st.close()


def test_rerecording_drops_the_copies_of_the_previous_recording(pq, oracle):
    """record() / record_staged() after a re-housed record(): no copies of the old recording stay behind (no stale-copy warning, no
    copies on the next run(ohlcv)), and the new recording reads the caller's tensors in place"""
    from polars_quant_amd.suite import Suite
    n, T = 70, 301
    da, db = oracle.gen_ohlcv(0x5EED0B11, n, T, 0), oracle.gen_ohlcv(0x5EED0B12, n, T, 0)
    st = Suite(n, T, "cuda")
    st.record({k: torch.from_numpy(v).cuda() for k, v in da.items()}, TASKS)   # dense odd pitch: re-housed
    assert sorted(st._housed) == sorted(OHLCV)
    G = _pitched(db, st.stride)                            # well pitched: used in place
    st.record(G, TASKS)
    assert st._housed == {}
    assert torch.cuda.current_stream().cuda_stream == 0    # (the created-stream warning is not what this is about)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _step(pq, oracle, st, db)
        _step(pq, oracle, st, db, G)
    for k in OHLCV:
        G[k].mul_(1.25)
    db = {k: v * 1.25 for k, v in db.items()}
    _step(pq, oracle, st, db)                              # in place: the replay reads the caller's memory

    st.record({k: torch.from_numpy(v).cuda() for k, v in da.items()}, TASKS)   # re-housed again ...
    assert sorted(st._housed) == sorted(OHLCV)
    stages = st.record_staged(G)                           # ... then the staged form, which reads every column in place
    assert st._housed == {} and sum(k for _, k in stages) == len(st.tasks(fused=True))
    _poison(st)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st.run_staged()
    torch.cuda.synchronize()
    _subset_matches(pq, oracle, st, db)
    st.close()


# ---- B. a small shard with inputs of mixed alignment -----------------------------------------------------------------------------

def _offset_view(v, pitch):
    """host [N, T] -> device view with row pitch `pitch` whose base is 8 bytes past a 16-byte boundary"""
    N, T = v.shape
    flat = torch.zeros(N * pitch + 2, dtype=torch.float64, device="cuda")
    t = flat[1: 1 + N * pitch].view(N, pitch)[:, :T]
    t.copy_(torch.from_numpy(v))
    assert t.data_ptr() % 16 == 8 and t.stride(0) == pitch
    return t


def _snapshot(st):
    cols = {name: [t.clone() for t in ts] for name, ts in st.out.items()}
    cols["__pat"] = [st.pat[nm].clone() for nm in sorted(st.pat)]
    cols["__bt"] = [t.clone() for t in st.bt] + [st.summary.clone()]
    return cols


_ALIGNED = {}   # N -> (host data, columns of the all-aligned recording): shared by the four misaligned inputs


def _aligned_reference(pq, oracle, N):
    from polars_quant_amd.suite import Suite
    if N not in _ALIGNED:
        d = oracle.gen_ohlcv(0x5EED0B20 + N, N, TT, 0)
        st = Suite(N, TT, "cuda:0", stride=STRIDE, exact_layout=True)
        st.record(_pitched(d, STRIDE))
        info = st.info()
        assert info["seq_jobs"] >= 40 and info["phases"] >= 3, info     # the small-shard plan, the Hilbert job split in time
        _poison(st)
        st.run(); st.run()
        torch.cuda.synchronize()
        _compare_everything(pq, oracle, d, st)
        _ALIGNED[N] = (d, _snapshot(st))
        st.close()
    return _ALIGNED[N]


@pytest.mark.parametrize("key", ["open", "high", "low", "volume"])
@pytest.mark.parametrize("N", [625, 1250], ids=["shard-625", "shard-1250"])
def test_small_shard_with_an_8_byte_aligned_input(pq, oracle, N, key):
    """exact_layout=True, `close` 16-byte aligned, one other input only 8-byte aligned: that input's jobs move their whole class to the
    8-byte job grid (seq_jobs_kernel<3>), which must run the time-split Hilbert chunks as chunks (`open` has no job: its users are ROW
    launches, which take 8-byte rows as they come).  Every column -- the Hilbert ones
    included -- must be bit-identical to the same data recorded with every input aligned (which is checked against the oracle)."""
    from polars_quant_amd.suite import Suite
    d, ref = _aligned_reference(pq, oracle, N)
    g = _pitched(d, STRIDE)
    g[key] = _offset_view(d[key], STRIDE)
    st = Suite(N, TT, "cuda:0", stride=STRIDE, exact_layout=True)
    st.record(g)
    info = st.info()
    assert info["seq_jobs"] >= 40 and info["phases"] >= 3, info
    kernels = {gs["kernel"] for gs in st.grid_stats()}
    if key == "open":   # read by ROW launches only (the patterns, BOP): every job of the grids stays 16-byte aligned
        assert "seq_jobs_kernel<3>" not in kernels, kernels
    else:               # the mixed grid is really reached
        assert "seq_jobs_kernel<3>" in kernels, kernels
    _poison(st)
    st.run(); st.run()
    torch.cuda.synchronize()
    got = _snapshot(st)
    bad = [(name, k) for name, ts in ref.items() for k, (a, b) in enumerate(zip(ts, got[name])) if not _same_bits(a, b)]
    assert not bad, f"columns that differ from the all-aligned recording: {bad}"
    st.close()


# ---- C. shard parity against the full-size recording -----------------------------------------------------------------------------

FULL_N = 5000


@pytest.fixture(scope="module")
def full_recording(oracle):
    from polars_quant_amd.suite import Suite
    d = oracle.gen_ohlcv(0x5EED0B30, FULL_N, TT, 0)
    st = Suite(FULL_N, TT, "cuda:0", stride=STRIDE)
    st.record(_pitched(d, STRIDE))
    st.run(); st.run()
    torch.cuda.synchronize()
    yield d, st
    st.close()


@pytest.mark.parametrize("n_shard", [2500, 1250, 625])
def test_shard_equals_the_same_rows_of_the_full_recording(pq, full_recording, n_shard):
    """the last block of n_shard symbols (what rank G - 1 of a 5 000-symbol run records) as a Suite of its own, on its own pitched
    copies: every column bit-identical to the same rows of the full-size recording, except the Hilbert columns, which a small shard
    computes in time-split chunks (within the transcendental tolerance).  The block starts mid-tile of the full recording."""
    from polars_quant_amd.suite import Suite
    d, full = full_recording
    lo, hi = FULL_N - n_shard, FULL_N
    assert lo % 64 != 0
    sub = {k: np.ascontiguousarray(v[lo:hi]) for k, v in d.items()}
    st = Suite(n_shard, TT, "cuda:0", stride=STRIDE)
    st.record(_pitched(sub, STRIDE))
    _poison(st)
    st.run(); st.run()
    torch.cuda.synchronize()
    bad = []
    for name, ts in st.out.items():
        for (oname, _), a, b in zip(pq.SPEC[name][2], ts, full.out[name]):
            if name in HT:
                assert_same(f"{name}.{oname}{{shard {lo}:{hi}}}", a.cpu().numpy(), b[lo:hi].cpu().numpy(), exact=False, price=sub["close"])
            elif not _same_bits(a, b[lo:hi]):
                bad.append(f"{name}.{oname}")
    bad += [nm for nm in pq.PATTERN_NAMES if not torch.equal(st.pat[nm], full.pat[nm][lo:hi])]
    bad += [f"bt[{k}]" for k, (a, b) in enumerate(zip(st.bt, full.bt)) if not _same_bits(a, b[lo:hi])]
    if not _same_bits(st.summary, full.summary[lo:hi]):
        bad.append("summary")
    assert not bad, f"shard {lo}:{hi} differs from the full recording in {bad}"
    st.close()


# ---- D. gates on a created stream ------------------------------------------------------------------------------------------------

def _fallback_data(oracle):
    """the series of test_small_shard_fallbacks_nulls_nans_infinities_and_flat_series: each one sends a fast form to its gated walk"""
    N = 330
    d = oracle.gen_ohlcv(0x5EED0601, N, TT, 0)
    for sym, row, val, cols in ((3, 100, np.nan, ("close",)), (70, 1000, np.nan, ("close",)), (71, 1500, np.inf, ("close",)),
                                (130, 900, np.nan, ("high",)), (131, 2519, np.nan, ("close",))):
        for c in cols:
            d[c][sym, row] = val
    for c in ("open", "high", "low", "close"):
        d[c][140] *= 1e200
        d[c][5] = 100.0
        d[c][329, :1300] = 50.0
    d["close"][328, 640:1280] = np.nan
    return d


def test_gated_fallbacks_on_a_created_stream(pq, oracle):
    """The gate flags of the fast forms are zeroed on the stream their kernels run on.  Recording, replaying and calling mama / ema /
    atr directly on a created (non-blocking) stream, with data that sets those gates, must give the oracle's columns.  The race a
    NULL-stream memset would open cannot be forced from here: this test exercises the path, it does not prove the ordering -- that is
    what review of the stream arguments is for."""
    from polars_quant_amd import api
    from polars_quant_amd.suite import Suite
    d = _fallback_data(oracle)
    N = d["close"].shape[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        g = _pitched(d, STRIDE)
        st = Suite(N, TT, "cuda:0", stride=STRIDE)
        st.record(g)
        assert st.info()["phases"] >= 3
        _poison(st)
        Suite._stream_warned = False
        with pytest.warns(api.PqLayoutWarning, match="created stream"):
            st.run()
        st.run()
        s.synchronize()
        _compare_everything(pq, oracle, d, st, ch=110)
        st.close()

        x = torch.from_numpy(d["close"]).cuda()
        hlc = [torch.from_numpy(d[k]).cuda() for k in ("high", "low", "close")]
        got = {"mama": api.call("mama", x), "ema": api.call("ema", x, timeperiod=30), "atr": api.call("atr", *hlc, timeperiod=14)}
        s.synchronize()
    exp = {"mama": oracle.call("mama", d["close"]), "ema": oracle.call("ema", d["close"], timeperiod=30),
           "atr": oracle.call("atr", d["high"], d["low"], d["close"], timeperiod=14)}
    for name, outs in got.items():
        for (oname, _), a, e in zip(pq.SPEC[name][2], outs, exp[name]):
            a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            assert_same(f"{name}.{oname}{{created stream}}", a, e, exact=name not in TRANSCENDENTAL, price=d["close"])
