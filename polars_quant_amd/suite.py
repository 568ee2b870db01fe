"""The benchmark workload as a reusable object: the full indicator suite (every function of SURVEY 8(a)
with the reference's Python-wrapper default parameters) + the fused MACD-cross per-symbol backtest over
one symbol-major [N, T] OHLCV block resident in HBM.  Outputs are allocated once.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import Batch, BtParams
from ._spec import BT_DEFAULTS, I, PATTERN_NAMES, PATTERN_PEN_DEFAULT, SPEC
from .api import _call, ctx

COLMAP = {"real": "close"}


def algorithmic_bytes_per_row() -> dict:
    """8*(#f64 in + #f64 out) + 4*(#i32 out) per (symbol, day) row, per call."""
    per = {}
    for name, (cols, _p, outs, _f) in SPEC.items():
        per[name] = 8 * len(cols) + sum(8 if dt == "f8" else 4 for _, dt in outs)
    per["cdl_all"] = 8 * 4 + 4 * len(PATTERN_NAMES)          # fused: OHLC read once, 61 int32 written
    per["backtest_macd_cross"] = 8 + 24                       # close in; position, cash, equity out
    return per


class Suite:
    def __init__(self, n_series: int, T: int, device="cuda", stride: int | None = None, exact_layout: bool = False):
        """The suite OWNS its output columns and allocates them at a row pitch that is a multiple of 128 B (pq_recommended_stride:
        every 64 / 128-byte tile piece is then one aligned cache line): `stride` if it is such a multiple, else the smallest one
        >= T.  Inputs handed to record() at another pitch or at a base that is not 16-byte aligned -- a dense odd-T tensor would run
        the 8-byte forms of every kernel, 1.5 x slower -- are re-housed ONCE at that pitch (record() / refresh_inputs()).
        exact_layout=True keeps the caller's layout exactly (stride = `stride` or T, inputs used in place): what the tests of the
        8-byte forms and bench.py --exact-layout measure."""
        self.n, self.T = n_series, T
        self.exact_layout = bool(exact_layout)
        rec = (T + 15) // 16 * 16
        if self.exact_layout:
            self.stride = T if stride is None else int(stride)
        else:
            self.stride = int(stride) if (stride and int(stride) % 16 == 0 and int(stride) >= T) else rec
        assert self.stride >= T
        self._housed = {}
        self.dev = torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:     # ("cuda" != "cuda:0" for torch: every input would read as foreign and be re-housed)
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.batch = Batch(n_series, T, self.stride)
        f64 = lambda: torch.empty((n_series, self.stride), dtype=torch.float64, device=self.dev)[:, :T]
        i32 = lambda: torch.empty((n_series, self.stride), dtype=torch.int32, device=self.dev)[:, :T]
        self.out = {name: [f64() if dt == "f8" else i32() for _, dt in outs] for name, (_c, _p, outs, _f) in SPEC.items()}
        self.pat = {nm: i32() for nm in PATTERN_NAMES}
        self.bt = [f64(), f64(), f64()]
        self.summary = torch.empty((n_series, 8), dtype=torch.float64, device=self.dev)
        self.periods = f64()
        self.periods.copy_(torch.from_numpy(np.tile((2 + np.arange(T) % 29).astype(np.float64), (n_series, 1))))
        self._pens = (C.c_double * 61)(*[PATTERN_PEN_DEFAULT[nm] for nm in PATTERN_NAMES])
        self._pat_ptrs = (C.c_void_p * 61)(*[self.pat[nm].data_ptr() for nm in PATTERN_NAMES])
        self._prm = BtParams(**BT_DEFAULTS)
        self._defaults = {name: [int(d) if k == I else float(d) for _, k, d in p]
                          for name, (_c, p, _o, _f) in SPEC.items()}
        self.bytes_per_row = algorithmic_bytes_per_row()

    def out_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for ts in self.out.values() for t in ts) + \
            sum(t.numel() * 4 for t in self.pat.values()) + sum(t.numel() * 8 for t in self.bt)

    def _col(self, ohlcv, c):
        return self.periods if c == "periods" else ohlcv[COLMAP.get(c, c)]

    def _on_layout(self, ohlcv: dict) -> None:
        """run_one() reads the columns with the suite's batch descriptor: refuse a column at another pitch instead of reading it wrongly
        (record() / run_eager() re-house such columns themselves; direct callers of run_one() pass them through house() first)"""
        for k, t in ohlcv.items():
            if self.n > 1 and t.stride(0) != self.stride:
                raise ValueError(f"input column `{k}` has a row pitch of {t.stride(0)} elements, the suite's is {self.stride}: "
                                 f"pass the columns through Suite.house() (or build the suite with exact_layout=True)")

    def run_one(self, name: str, ohlcv: dict) -> None:
        self._on_layout(ohlcv)
        h, o = ctx(self.dev.index), self.out
        run = lambda fn, *args: _call("pq_" + fn, None, h, self.batch, *args)
        P = lambda *ks: [ohlcv[k] for k in ks]
        O = lambda *ns: [t for n in ns for t in o[n]]       # every output column of the named functions, in SPEC's order
        if name == "cdl_all":
            run(name, *P("open", "high", "low", "close"), self._pens, self._pat_ptrs)
        elif name == "backtest_macd_cross":
            run(name, ohlcv["close"], 12, 26, 9, self._prm, *self.bt, self.summary)
        # multi-output forms: the listed functions share their inputs and (default) parameters -> one job
        elif name == "dmi_all":   # calc_dm evaluated once for its five users (all timeperiod=14 by default)
            run(name, *P("high", "low", "close"), 14, *O("dx", "plus_di", "minus_di", "adx", "adxr"))
        elif name == "ema_all":
            run(name, ohlcv["close"], 30, *O("ema", "dema", "tema", "trix"))
        elif name == "atr_all":
            run(name, *P("high", "low", "close"), 14, *O("atr", "natr"))
        elif name == "dm_pair":
            run(name, *P("high", "low"), 14, *O("plus_dm", "minus_dm"))
        elif name == "ad_all":
            run(name, *P("high", "low", "close", "volume"), 3, 10, *O("ad", "adosc"))
        elif name == "dm_system_all":
            run(name, *P("high", "low", "close"), 14, *O("dx", "plus_di", "minus_di", "adx", "adxr", "atr", "natr"))
        elif name == "cmo_rsi":
            run(name, ohlcv["close"], 14, *O("cmo", "rsi"))
        elif name == "sma_ma":    # SMA(30) and MA(30, matype 0): the same walk (overlap.rs:857-869), one job, the value written twice
            run(name, ohlcv["close"], 30, *O("sma", "ma"))
        elif name == "volume_all":
            run(name, *P("high", "low", "close", "volume"), 14, 3, 10, *O("mfi", "ad", "adosc", "obv"))
        elif name == "sar_pair":   # Python-wrapper defaults: every parameter 0.0 (overlap.py:115-157)
            run(name, *P("high", "low"), *([0.0] * 10), *O("sar", "sarext"))
        elif name == "stoch_all":
            run(name, *P("high", "low", "close"), 5, 3, 0, 3, 0, 3, 0, *O("stoch", "stochf"))
        elif name == "macd_pair":
            run(name, ohlcv["close"], 12, 26, 9, 9, *O("macd", "macdfix"))
        elif name == "apo_ppo":
            run(name, ohlcv["close"], 12, 26, 0, *O("apo", "ppo"))
        elif name == "aroon_all":  # AROON + AROONOSC (both timeperiod=14 by default) from one window scan
            run(name, *P("high", "low"), 14, *O("aroon", "aroonosc"))
        elif name == "ht_all":    # the Hilbert pipeline evaluated once for dcperiod / dcphase / phasor / sine
            run(name, ohlcv["close"], *O("ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine"))
        else:
            run(name, *[self._col(ohlcv, c) for c in SPEC[name][0]], *self._defaults[name], *o[name])

    FUSED = {"dm_system_all": ("dx", "plus_di", "minus_di", "adx", "adxr", "atr", "natr"), "cmo_rsi": ("cmo", "rsi"),
             "ht_all": ("ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine"),
             "aroon_all": ("aroon", "aroonosc"), "ema_all": ("ema", "dema", "tema", "trix"), 
             "dm_pair": ("plus_dm", "minus_dm"), "apo_ppo": ("apo", "ppo"),
             "sar_pair": ("sar", "sarext"), "volume_all": ("mfi", "ad", "adosc", "obv"),
             "stoch_all": ("stoch", "stochf"), "macd_pair": ("macd", "macdfix"), "sma_ma": ("sma", "ma")}
    # pq_macd_pair (six output tiles, 27.6 KB) and pq_stoch_all (192 VGPRs since the moving-average cores were slimmed: it now runs in
    # the light job kernel) joined the list in round 3: time-neutral within the noise of a session (4.34 against 4.35 ms per step), two
    # jobs and four column reads fewer.  PQ_SUITE_UNFUSE=name,... keeps the listed ones as separate calls for A/B runs.

    def tasks(self, fused: bool = False):
        """every function of the suite; fused=True replaces the users of a shared core by the multi-output call"""
        names = list(SPEC)
        if fused:
            import os
            skip = set(filter(None, os.environ.get("PQ_SUITE_UNFUSE", "").split(",")))   # A/B runs: keep these as separate calls
            fused_map = {k: v for k, v in self.FUSED.items() if k not in skip}
            covered = {n for v in fused_map.values() for n in v}
            return [n for n in names if n not in covered] + list(fused_map) + ["cdl_all", "backtest_macd_cross"]
        return names + ["cdl_all", "backtest_macd_cross"]

    def run_eager(self, ohlcv: dict) -> None:
        """one step as ~90 separate launches (one per C-ABI call), enqueued on the current stream"""
        ohlcv = self._house(ohlcv)
        with torch.cuda.device(self.dev):
            for name in self.tasks():
                self.run_one(name, ohlcv)

    def _house(self, ohlcv: dict) -> dict:
        """the input columns on the suite's layout: a column already at the suite's pitch (and 16-byte aligned) is used in place,
        any other is copied into a suite-owned pitched buffer -- once; refresh_inputs() repeats the copy after the caller changed it"""
        if self.exact_layout:
            return ohlcv
        out = {}
        for k, t in ohlcv.items():
            ok = (t.dim() == 2 and tuple(t.shape) == (self.n, self.T) and t.dtype == torch.float64 and t.device == self.dev and
                  (self.T <= 1 or t.stride(1) == 1) and (self.n <= 1 or t.stride(0) == self.stride) and t.data_ptr() % 16 == 0)
            if ok:
                out[k] = t
                continue
            buf = self._housed.get(k)
            if buf is None:
                buf = self._housed[k] = torch.zeros((self.n, self.stride), dtype=torch.float64, device=self.dev)
            buf[:, :self.T].copy_(t)
            out[k] = buf[:, :self.T]
        self._stale_warned = False
        return out

    def _needs_housing(self, ohlcv: dict) -> list:
        """the columns of `ohlcv` that record() would copy instead of using in place"""
        if self.exact_layout:
            return []
        return [k for k, t in ohlcv.items()
                if not (t.dim() == 2 and tuple(t.shape) == (self.n, self.T) and t.dtype == torch.float64 and t.device == self.dev and
                        (self.T <= 1 or t.stride(1) == 1) and (self.n <= 1 or t.stride(0) == self.stride) and t.data_ptr() % 16 == 0)]

    house = _house

    def refresh_inputs(self, ohlcv: dict) -> None:
        """bind the caller's current data to the recording for the next replays (no re-recording): a column that record() re-housed
        is copied into the suite's buffer (current stream) whatever the layout of the tensor passed; a column that the recording reads
        in place accepts only the recorded tensor itself (same data_ptr, shape and strides) -- its data are read where they are.  Any
        other tensor for such a column, or a key the recording does not read, raises ValueError: re-record, or write into the recorded
        buffer.  run(ohlcv) does this itself."""
        rec = getattr(self, "_ohlcv", None) or {}
        unknown = sorted(set(ohlcv) - set(rec))
        if unknown:
            raise ValueError(f"input columns {unknown} are not read by the recorded step (it reads {sorted(rec)})")
        copies = []   # (every column is checked before any is copied: a refused call changes nothing)
        for k, t in ohlcv.items():
            r, buf = rec[k], self._housed.get(k)
            if buf is not None and buf.data_ptr() == r.data_ptr():      # the recording reads the suite's copy of this column
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (self.n, self.T):
                    raise ValueError(f"input column `{k}`: expected a [{self.n}, {self.T}] tensor, got {getattr(t, 'shape', type(t))}")
                copies.append((r, t))
            elif not (isinstance(t, torch.Tensor) and t.data_ptr() == r.data_ptr() and t.shape == r.shape and t.stride() == r.stride()
                      and t.dtype == r.dtype and t.device == r.device):
                raise ValueError(f"input column `{k}` is read in place by the recorded step, and this is not the recorded tensor: "
                                 f"re-record (Suite.record) with the new tensor, or write the new data into the recorded buffer")
        for r, t in copies:
            r.copy_(t)
        self._stale_warned = False

    def record(self, ohlcv: dict, tasks=None, summaries=None) -> None:
        """record the step once (pq_suite_begin/end): the sequential jobs of all functions become one grid per phase.
        summaries = [t0, t1] ([n, 8] f64 each): the step is recorded TWICE, the backtest of recording k writing its summary rows into
        summaries[k] (every other output column is shared) -- run(slot=k) then replays recording k, so that a multi-GPU caller can
        keep the exchange of one table in flight while the next step fills the other (distributed.OverlappedGather)."""
        self.close()
        self._housed, self._stale_warned = {}, False   # copies of an earlier recording are not this one's
        ohlcv = self._house(ohlcv)
        self._ohlcv = ohlcv  # keep the inputs alive: the suite holds raw device pointers
        handles, keep, ok = [], self.summary, False
        try:
            for summ in (summaries or [self.summary]):
                assert summ.shape == (self.n, 8) and summ.dtype == torch.float64 and summ.is_contiguous()
                self.summary = summ
                handles.append(self._record(tasks or self.tasks(fused=True), ohlcv))
            ok = True
        finally:
            if ok:
                self.summary = summaries[0] if summaries else keep
            else:   # a later recording failed: the earlier handles (job tables, events) must not leak, the object keeps its old table
                self.summary = keep
                for hnd in handles:
                    _call("pq_suite_destroy", None, ctx(self.dev.index), hnd, checked=False)
        self._summaries = list(summaries) if summaries else [self.summary]
        self._suites = handles
        self._suite = handles[0]

    def _record(self, names, ohlcv: dict):
        """pq_suite_begin, run_one for every name (pq_suite_abort if one raises), pq_suite_end -> the handle of the recording"""
        with torch.cuda.device(self.dev):
            h = ctx(self.dev.index)
            _call("pq_suite_begin", None, h, self.batch)
            try:
                for name in names:
                    self.run_one(name, ohlcv)
            except Exception:
                _call("pq_suite_abort", None, h, checked=False)
                raise
            out = C.c_void_p()
            _call("pq_suite_end", None, h, C.byref(out))
        return out

    # ---- staged form: the step split by the input columns a task needs, so that a stage starts as soon as ITS columns have
    # arrived from the host (loader.DeviceFrame.upload records one event per column on the copy stream)
    STAGE_ORDER = ("close", "high", "low", "open", "volume")   # copy order = the order in which the stages become runnable

    def task_inputs(self, name: str) -> set:
        if name == "cdl_all":
            return {"open", "high", "low", "close"}
        if name == "backtest_macd_cross":
            return {"close"}
        members = self.FUSED.get(name) or {"dmi_all": ("dx", "plus_di", "minus_di", "adx", "adxr"), "atr_all": ("atr", "natr"),
                                            "ad_all": ("ad", "adosc"), "macd_pair": ("macd", "macdfix"), "stoch_all": ("stoch", "stochf")}.get(name) or (name,)
        cols = set()
        for m in members:
            cols |= {COLMAP.get(c, c) for c in SPEC[m][0] if c != "periods"}
        return cols

    def record_staged(self, ohlcv: dict) -> list:
        """one recorded suite per prefix of STAGE_ORDER that completes some task's inputs -> [(columns needed, n tasks)]"""
        # The staged step waits for the upload events of the buffers it READS: a column that had to be re-housed would be read from
        # the suite's copy while the events speak of the caller's tensor.  Upload into the suite's own layout instead
        # (DeviceFrame(columns=suite.house(cols), stride=suite.stride), as bench.py --e2e does).
        slow = self._needs_housing(ohlcv)
        if slow:
            raise ValueError(f"record_staged: columns {slow} are not on the suite's row pitch ({self.stride} elements): pass suite.house(columns)")
        self.close()
        self._housed, self._stale_warned = {}, False   # every column is read in place: no copies of an earlier recording stay
        self._ohlcv = ohlcv
        stages, have, left = [], set(), list(self.tasks(fused=True))
        for col in self.STAGE_ORDER:
            have.add(col)
            ready = [t for t in left if self.task_inputs(t) <= have]
            left = [t for t in left if t not in ready]
            if ready:
                stages.append((col, ready))
        assert not left, left
        self._stages = []
        for col, names in stages:     # (one by one: close() finds the stages recorded before one that fails)
            self._stages.append((col, self._record(names, ohlcv), len(names)))
        return [(col, n) for col, _, n in self._stages]

    def run_staged(self, events: dict | None = None) -> None:
        """the staged step on the current stream; events[column] (from DeviceFrame.upload): wait for that column's copy first"""
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.device(self.dev):
            h = ctx(self.dev.index)
            for col, handle, _n in self._stages:
                if events is not None:
                    for c in self.STAGE_ORDER[: self.STAGE_ORDER.index(col) + 1]:
                        if c in events:
                            cur.wait_event(events[c])
                _call("pq_suite_run", None, h, handle)

    def info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _call("pq_suite_info", None, self._suite, C.byref(a), C.byref(b), C.byref(c))
        return {"phases": a.value, "seq_jobs": b.value, "row_launches": c.value}

    def set_timing(self, on: bool = True) -> None:
        """HIP events around every sequential-job grid (on its launch stream) for the following runs"""
        _call("pq_suite_set_timing", None, self._suite, 1 if on else 0)

    def grid_stats(self):
        """-> list of dicts per SEQ grid: avg_ms over the timed runs, algorithmic bytes per launch, jobs, LDS bytes"""
        out, k = [], 0
        while True:
            ms, by, nj, lds, runs = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
            if _call("pq_suite_grid_stats", None, self._suite, k, C.byref(ms), C.byref(by), C.byref(nj), C.byref(lds), C.byref(runs), checked=False) != 0:
                break
            var = C.c_int32()
            _call("pq_suite_grid_variant", None, self._suite, k, C.byref(var))
            out.append({"avg_ms": ms.value, "alg_bytes": by.value, "n_jobs": nj.value, "lds_bytes": lds.value, "runs": runs.value,
                        "kernel": f"seq_jobs_kernel<{var.value}>" if var.value < 3 else ("seq_jobs_kernel<3>" if var.value == 4 else "row_chain")})
            k += 1
        return out

    def span_stats(self, variant: int = 0):
        """-> (mean ms from the earliest start to the latest end of the grids launching seq_jobs_kernel<variant>, their
        algorithmic bytes per step)"""
        ms, by = C.c_double(), C.c_double()
        _call("pq_suite_span_stats", None, self._suite, variant, C.byref(ms), C.byref(by))
        return ms.value, by.value

    def run(self, ohlcv: dict | None = None, slot: int = 0) -> None:
        """one step: every indicator + all 61 patterns + the MACD-cross backtest, enqueued on the current stream
        (slot: which of the recordings of record(summaries=[...]) to replay).  ohlcv: the data of this step, bound as refresh_inputs()
        binds them -- copied into the suite's buffer for a re-housed column, the recorded tensor itself for a column read in place
        (any other tensor raises ValueError); without it the step replays on the recorded buffers as they are."""
        if getattr(self, "_suite", None) is None:
            self.record(ohlcv)
        elif ohlcv is not None:
            self.refresh_inputs(ohlcv)
        elif self._housed and not getattr(self, "_stale_warned", True):
            # the recording reads suite-owned copies of the columns that were handed over at a slow row pitch: a replay without tensors
            # reads those copies as they are -- said once per recording
            import warnings
            from .api import PqLayoutWarning
            self._stale_warned = True
            warnings.warn(f"Suite.run(): columns {sorted(self._housed)} were re-housed at record time; this replay reads those copies, not the "
                          f"caller's tensors -- pass the tensors to run() or call refresh_inputs() after changing them", PqLayoutWarning, stacklevel=2)
        if not Suite._stream_warned and torch.cuda.current_stream(self.dev).cuda_stream != 0:
            # (a replay needs four hardware queues on four compute pipes: the NULL stream + the three side streams of the context are a
            #  process's first four; a created stream shifts them and two chains share a pipe -- DESIGN.md section 6)
            import warnings
            from .api import PqLayoutWarning
            Suite._stream_warned = True
            warnings.warn("Suite.run() on a created stream: on this runtime a recorded suite replays 17-38 % slower there than on the NULL "
                          "(default) stream -- two of its four chains share a compute pipe of the command processor (INTEGRATION.md); "
                          "warned once per process", PqLayoutWarning, stacklevel=2)
        _call("pq_suite_run", self.dev, self._suites[slot])

    _stream_warned = False

    def close(self):
        for hnd in getattr(self, "_suites", []) or []:
            _call("pq_suite_destroy", None, ctx(self.dev.index), hnd)
        self._suites = []
        self._suite = None
        for _col, handle, _n in getattr(self, "_stages", []):
            _call("pq_suite_destroy", None, ctx(self.dev.index), handle)
        self._stages = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def suite_bytes_per_row(self) -> int:
        """per-call algorithmic bytes of the whole suite (SURVEY 8d accounting, independent of how calls are fused)"""
        return sum(self.bytes_per_row[t] for t in self.tasks())
