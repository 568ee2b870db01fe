"""-m gpu: the jobs whose COMPUTE wave stores part of every out tile (the ops' ASSIST trait, csrc/pq_dev.h run_seq_lds).

Every assisted op -- BBANDS, SMA + MA, EMA / DEMA / TEMA / TRIX, MACD + MACDFIX -- and the seven-column DMI + ATR / NATR job (store-bound
as well, but without the registers for the split: its storer keeps all columns) are recorded into one job grid on the full-chip plan (where the multi-output forms are single jobs), replayed, and every output column compared bit for bit
with the direct, un-recorded call and with the oracle.  Shapes: the smallest that reach each branch of the split --

  symbols 1, 63, 64, 65, 130    one series, a ragged last tile (the dead series fold onto the last live one), a full tile, more than one
  days 64, 72, 77               an even tile count, an odd one (the storer's last pair holds one tile; the compute wave's last tile is
                                flushed behind the loop), a length that is no multiple of the 8-row tile (per-lane tail)
  row pitch                     a multiple of 16 elements (the aligned body); one case at an odd pitch: the 8-byte grid, assist off

The pitch padding of every output column and a guard row behind the last series hold a sentinel that must survive the run: the compute
wave obeys the same per-access liveness as the storer.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x5EED0A55
SENT = -7.25e300          # sentinel of padding and guard row (no indicator produces it)
NULLB = np.uint64(0x7FF80000504E554C)
N_MAX, T_MAX = 130, 77

# name -> (input columns, reference calls in output-column order: (oracle function, parameters, number of outputs), accepts NULLs)
OPS = {
    "bbands": (("close",), [("bbands", dict(timeperiod=5, nbdevup=2.0, nbdevdn=1.5), 3)], True),
    "sma_ma": (("close",), [("sma", dict(timeperiod=6), 1), ("ma", dict(timeperiod=6, matype=0), 1)], True),
    "ema_all": (("close",), [("ema", dict(timeperiod=4), 1), ("dema", dict(timeperiod=4), 1), ("tema", dict(timeperiod=4), 1),
                             ("trix", dict(timeperiod=4), 1)], False),
    "macd_pair": (("close",), [("macd", dict(fastperiod=3, slowperiod=7, signalperiod=4), 3), ("macdfix", dict(signalperiod=5), 3)], False),
    "dm_system_all": (("high", "low", "close"), [(f, dict(timeperiod=5), 1) for f in ("dx", "plus_di", "minus_di", "adx", "adxr", "atr", "natr")],
                      False),
}


def _launch(L, h, b, name, ins, outs):
    P = [C.c_void_p(t.data_ptr()) for t in ins]
    O = [C.c_void_p(t.data_ptr()) for t in outs]
    from polars_quant_amd._lib import check
    if name == "bbands":
        check(L.pq_bbands(h, C.byref(b), *P, 5, 2.0, 1.5, *O))
    elif name == "sma_ma":
        check(L.pq_sma_ma(h, C.byref(b), *P, 6, *O))
    elif name == "ema_all":
        check(L.pq_ema_all(h, C.byref(b), *P, 4, *O))
    elif name == "macd_pair":
        check(L.pq_macd_pair(h, C.byref(b), *P, 3, 7, 4, 5, *O))
    else:
        check(L.pq_dm_system_all(h, C.byref(b), *P, 5, *O))


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()
    return pq


@pytest.fixture(scope="module")
def world(oracle, pq):
    """the data sets (generated once at the largest shape; a case takes the leading [n, T] block) and a cache of oracle results"""
    clean = oracle.gen_ohlcv(SEED, N_MAX, T_MAX, 0)
    nan = {k: v.copy() for k, v in clean.items()}      # NaN values inside
    for k in ("high", "low", "close"):
        nan[k][0, 40] = np.nan                         # one alone, late: the tiles before it are straight-line ones
        nan[k][2, 9:12] = np.nan                       # a run
        nan[k][64 % N_MAX, 0] = np.nan                 # the very first value of the second tile's first series
        nan[k][5, T_MAX - 14] = np.nan
    holes = {k: v.copy() for k, v in nan.items()}      # ... and a NULL prefix
    for k in holes:
        holes[k][:, :3] = oracle.NULL
        holes[k][7, :20] = oracle.NULL                 # a longer prefix
        holes[k][3] = clean[k][3]                      # one series without either
    return {"clean": clean, "nan": nan, "holes": holes, "ref": {}}


def _expected(oracle, world, name, which, n, T):
    """oracle columns of op `name` on the leading [n, T] block of data set `which` (computed once per shape)"""
    key = (name, which, n, T)
    if key not in world["ref"]:
        cols, calls, _ = OPS[name]
        src = [np.ascontiguousarray(world[which][c][:n, :T]) for c in cols]
        exp = []
        for fn, prm, _k in calls:
            exp.extend(oracle.call(fn, *src, **prm))
        for e in exp:
            e.setflags(write=False)
        world["ref"][key] = exp
    return world["ref"][key]


def _same_bits(tag, got, exp):
    g, e = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(exp).view(np.uint64)
    assert ((g == NULLB) == (e == NULLB)).all(), f"{tag}: null masks differ at {np.argwhere((g == NULLB) != (e == NULLB))[:5].tolist()}"
    bad = (g != e) & ~(np.isnan(got) & np.isnan(exp))   # (a NaN's payload is not part of the contract)
    assert not bad.any(), f"{tag}: {bad.sum()} of {bad.size} values differ; first at {np.argwhere(bad)[:3].tolist()}"


def _run_case(pq, oracle, world, n, T, pitch, which_for):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check, lib
    L, h, b = lib(), api.ctx(0), Batch(n, T, pitch)

    def column(a=None):   # n series + a guard row at the case's pitch, sentinel everywhere outside [n, T]
        buf = torch.full((n + 1, pitch), SENT, dtype=torch.float64, device="cuda")
        if a is not None:
            buf[:n, :T] = torch.from_numpy(np.ascontiguousarray(a[:n, :T])).cuda()
        return buf

    ins = {w: {c: column(world[w][c]) for c in ("high", "low", "close")} for w in set(which_for.values())}
    nout = {name: sum(k for _f, _p, k in OPS[name][1]) for name in OPS}
    rec = {name: [column() for _ in range(nout[name])] for name in OPS}
    direct = {name: [column() for _ in range(nout[name])] for name in OPS}
    for name in OPS:
        _launch(L, h, b, name, [ins[which_for[name]][c] for c in OPS[name][0]], direct[name])
    old = os.environ.get("PQ_SMALL_SHARD_TILES")
    os.environ["PQ_SMALL_SHARD_TILES"] = "0"   # the full-chip plan: the multi-output forms are recorded as ONE job each
    try:
        check(L.pq_suite_begin(h, C.byref(b)))
        try:
            for name in OPS:
                _launch(L, h, b, name, [ins[which_for[name]][c] for c in OPS[name][0]], rec[name])
        except Exception:
            L.pq_suite_abort(h)
            raise
        suite = C.c_void_p()
        check(L.pq_suite_end(h, C.byref(suite)))
    finally:
        if old is None:
            del os.environ["PQ_SMALL_SHARD_TILES"]
        else:
            os.environ["PQ_SMALL_SHARD_TILES"] = old
    try:
        check(L.pq_suite_run(h, suite))
        check(L.pq_suite_run(h, suite))
        torch.cuda.synchronize()
        kernels, jobs, k = set(), 0, 0
        while True:
            var, ms, by, nj, lds, runs = C.c_int32(), C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
            if L.pq_suite_grid_variant(suite, k, C.byref(var)) != 0:
                break
            check(L.pq_suite_grid_stats(suite, k, C.byref(ms), C.byref(by), C.byref(nj), C.byref(lds), C.byref(runs)))
            kernels.add(var.value); jobs += nj.value; k += 1
    finally:
        check(L.pq_suite_destroy(h, suite))
    for name in OPS:
        exp = _expected(oracle, world, name, which_for[name], n, T)
        for j, (r, d, e) in enumerate(zip(rec[name], direct[name], exp)):
            tag = f"{name}[{j}] {n}x{T} pitch {pitch} ({which_for[name]})"
            rh, dh = r.cpu().numpy(), d.cpu().numpy()
            _same_bits(tag + " recorded vs direct", rh[:n, :T], dh[:n, :T])
            _same_bits(tag + " recorded vs oracle", rh[:n, :T], e)
            for what, a in (("recorded", rh), ("direct", dh)):
                assert (a[:n, T:] == SENT).all(), f"{tag}: the {what} run wrote into the pitch padding"
                assert (a[n] == SENT).all(), f"{tag}: the {what} run wrote behind the last series"
    return kernels, jobs


@pytest.mark.parametrize("T", [64, 72, 77])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_assisted_jobs_match_direct_calls_and_oracle(pq, oracle, world, n, T):
    pitch = (T + 15) // 16 * 16 + 16   # a multiple of 16 elements with padding behind every row
    kernels, jobs = _run_case(pq, oracle, world, n, T, pitch, {name: "clean" for name in OPS})
    assert kernels == {0}, f"expected the aligned light job kernel alone, got variants {kernels}"
    assert jobs == len(OPS), f"expected one job per call, got {jobs}"


@pytest.mark.parametrize("n,T", [(65, 72), (130, 77)])
def test_assisted_jobs_null_prefix_and_nans(pq, oracle, world, n, T):
    """NaN values inside the series for every op, a NULL prefix as well where the reference function accepts NULLs"""
    pitch = (T + 15) // 16 * 16 + 16
    kernels, jobs = _run_case(pq, oracle, world, n, T, pitch, {name: ("holes" if OPS[name][2] else "nan") for name in OPS})
    assert kernels == {0} and jobs == len(OPS), (kernels, jobs)


def test_odd_pitch_takes_the_unassisted_8_byte_grid(pq, oracle, world):
    """rows only 8-byte aligned: the UNAL job kernel, whose compute wave stores nothing, still gives the same columns"""
    n, T = 65, 72   # (T even, so that T + 1 is an odd pitch)
    kernels, _jobs = _run_case(pq, oracle, world, n, T, T + 1, {name: "clean" for name in OPS})
    assert kernels == {4}, f"expected the 8-byte job kernel (pq_suite_grid_variant 4 = seq_jobs_kernel<3>), got variants {kernels}"
