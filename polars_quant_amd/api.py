"""Host side of the drop-in: batches of series in, batches out, computed by the HIP library.

Inputs may be torch CUDA tensors (zero-copy), numpy arrays / pyarrow arrays / polars Series (copied to the
device through torch); shapes [T] (one series) or [N, T] (N symbols, symbol-major = long format sorted by
symbol, date).  Outputs come back in the container kind of the first input.  Nulls travel as the NaN bit
pattern NULL_BITS on the device and are converted from/to Arrow validity at the edge.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Batch, BtParams, LevParams, NullsNotAllowed, PqError, SeqParams, check, lib
from ._spec import BT_DEFAULTS, EXTRA, I, NB, PATTERN_NAMES, PATTERN_PEN_DEFAULT, SPEC, SUMMARY_KEYS

NULL = np.array([_lib.NULL_BITS], dtype=np.uint64).view(np.float64)[0]

_ctx_cache = {}


def _require_gpu():
    if not torch.cuda.is_available():
        raise PqError("polars_quant_amd needs an MI355X (HIP device); there is no CPU fallback")


def ctx(device: int | None = None):
    """pq_ctx bound to torch's current stream on `device` (cached per device+stream)."""
    _require_gpu()
    dev = torch.cuda.current_device() if device is None else device
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (dev, stream)
    h = _ctx_cache.get(key)
    if h is None:
        h = C.c_void_p()
        _call("pq_ctx_create", None, dev, stream or None, C.byref(h))
        _ctx_cache[key] = h
    return h


def _tensor_ptr(t):
    return t.data_ptr() if t.numel() else None


def _classify(t: type):
    """how _marshal converts an argument of type t: a function of the argument, or None where it is passed as it is"""
    if issubclass(t, torch.Tensor):
        return _tensor_ptr
    if issubclass(t, C.Structure):          # Batch and the parameter structs: the callee reads the caller's
        return C.byref
    if issubclass(t, np.ndarray):
        return lambda a: a.ctypes.data
    return None                             # numbers, None, context and suite handles, ctypes arrays and byref()s


# _classify by exact type, filled as types are first seen (a dict lookup, not an isinstance chain: torch.Tensor's costs 0.5 us a miss)
_convert = {t: _classify(t) for t in (int, float, type(None), C.c_void_p, Batch)}
_Tensor = torch.Tensor


def _marshal(args) -> list:
    """the one rule by which the package hands values to the C ABI: None -> NULL; a tensor -> its data_ptr(), NULL when it has no
    element; a numpy array -> its address; a Batch or parameter struct -> by reference; anything else (numbers, ctypes arrays and
    byref()s, handles) as it is, for the entry point's argtypes to convert or refuse"""
    out = []
    for a in args:
        t = type(a)
        if t is _Tensor:                    # most arguments: _tensor_ptr without the call
            out.append(a.data_ptr() if a.numel() else None)
            continue
        try:
            conv = _convert[t]
        except KeyError:
            conv = _convert[t] = _classify(t)
        out.append(a if conv is None else conv(a))
    return out


def _call(name: str, dev, *args, checked: bool = True):
    """every C-ABI call of the package: the entry point `name` on _marshal(args), its status checked (checked=False: for one that
    returns a value, which is returned as it is).  dev: the device of an entry point that takes a context -- it is made current and
    the context of its current stream goes in front of args; None for one that takes none, or is handed one in args.  `args` stay
    referenced until the call has returned.  A value that the declared signature refuses (a float for an int64_t) is a TypeError."""
    try:
        if dev is None:
            r = getattr(lib(), name)(*_marshal(args))
        else:
            with torch.cuda.device(dev):
                r = getattr(lib(), name)(ctx(dev.index), *_marshal(args))
    except C.ArgumentError as e:
        raise TypeError(f"{name}: {e}") from None
    if not checked:
        return r
    if r:
        check(r)


class _Kind:
    TORCH, NUMPY, ARROW, POLARS = range(4)


def _to_device(x, dtype=torch.float64):
    """-> (tensor [N,T] on cuda, kind, squeeze)"""
    kind = _Kind.TORCH
    if isinstance(x, torch.Tensor):
        t = x
    else:
        mod = type(x).__module__.split(".")[0]
        if mod == "polars":
            kind = _Kind.POLARS
            x = x.to_arrow()
            mod = "pyarrow"
        if mod == "pyarrow":
            if kind != _Kind.POLARS:
                kind = _Kind.ARROW
            import pyarrow as pa
            if isinstance(x, pa.ChunkedArray):
                x = x.combine_chunks()
            arr = x.cast(pa.float64()) if dtype == torch.float64 else x
            vals = arr.to_numpy(zero_copy_only=False).astype(np.float64 if dtype == torch.float64 else np.uint8, copy=True)
            if arr.null_count:
                mask = np.asarray(arr.is_null())
                if dtype == torch.float64:
                    vals[mask] = NULL
                else:
                    vals[mask] = 0
            t = torch.from_numpy(vals)
        else:
            kind = _Kind.NUMPY
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != dtype:
        t = t.to(torch.uint8 if dtype == torch.uint8 else dtype)
    squeeze = t.dim() == 1
    if squeeze:
        t = t.unsqueeze(0)
    if t.dim() != 2:
        raise PqError("inputs must be [T] or [N, T]")
    if not t.is_cuda:
        _require_gpu()
        n, T = t.shape
        pitch = recommended_stride(T)
        if n > 1 and pitch != T and dtype == torch.float64:
            # a host column is uploaded into a device copy this library owns: place it at the 128-byte row pitch straight away
            # (pq_recommended_stride; one strided H2D copy instead of a dense one -- a dense ODD-T copy would run the 8-byte forms)
            buf = torch.empty((n, pitch), dtype=dtype, device="cuda")
            buf[:, :T].copy_(t)
            t = buf[:, :T]
        else:
            t = t.cuda()
    elif t.dim() == 2 and t.shape[0] > 1 and t.dtype == torch.float64 and t.stride(1) == 1 and (t.stride(0) % 2 or t.data_ptr() % 16):
        _warn_slow_layout(t)
    if t.stride(1) != 1 and t.shape[1] > 1:
        t = t.contiguous()
    return t, kind, squeeze


def recommended_stride(T: int) -> int:
    """pq_recommended_stride: the row pitch (elements) to allocate [N, T] device columns with -- the smallest multiple of 128 B >= T"""
    return (int(T) + 15) // 16 * 16


class PqLayoutWarning(UserWarning):
    """A device tensor handed to the library sits on a layout whose rows are only 8-byte aligned (odd row pitch, or a base 8 bytes off a
    16-byte boundary): every kernel then runs its 8-byte form, about 1.5 x slower (pq_layout_check returns PQ_WARN_SLOW_LAYOUT).  Results
    are identical.  Allocate [N, recommended_stride(T)] and pass the [:, :T] view, or hand over host data (uploaded pitched), or use
    Suite / loader.DeviceFrame, which re-house such inputs once."""


_warned_layout = False


def _warn_slow_layout(t: torch.Tensor) -> None:
    global _warned_layout
    if _warned_layout:
        return
    _warned_layout = True
    import warnings
    warnings.warn(f"polars_quant_amd: device tensor of shape {tuple(t.shape)} has a row pitch of {t.stride(0)} elements / a base that is not "
                  f"16-byte aligned: the 8-byte kernel forms run (~1.5x slower, same results); use a row pitch of "
                  f"{recommended_stride(t.shape[1])} (api.recommended_stride) -- warned once per process", PqLayoutWarning, stacklevel=4)


def _from_device(t: torch.Tensor, kind: int, squeeze: bool, name: str = ""):
    if squeeze:
        t = t[0]
    if kind == _Kind.TORCH:
        return t
    a = np.ascontiguousarray(t.cpu().numpy())   # (a pitched device column comes back dense)
    if kind == _Kind.NUMPY:
        return a
    import pyarrow as pa
    if a.dtype == np.float64:
        mask = a.view(np.uint64) == np.uint64(_lib.NULL_BITS)
    else:
        mask = a == np.int32(_lib.NULL_I32)
    arr = pa.array(a.ravel(), mask=mask.ravel())
    if kind == _Kind.POLARS:
        import polars as pl
        return pl.Series(name, arr)
    return arr


def _batch(t: torch.Tensor, dense: bool = False, lone_dense: bool = False) -> Batch:
    """the Batch that describes an [N, T] tensor: its own row pitch; dense: T (the tensor was made contiguous).  A single series has no
    pitch to keep: it passes its own where that is at least T, and T otherwise or with lone_dense (the library picks its 16-byte or
    8-byte forms by this value, and each entry point keeps the one it always passed).
    The one-row rule: the stride that a one-row tensor reports is only passed on where every argument of the call reports the same one --
    _same_layout re-views the rows of a one-row call whose arguments disagree at stride T, so the Batch of any of its results (the first,
    or the last as linear and the regressions take it) never describes a pitch that another argument was not allocated with.  An empty
    tensor (N = 0 or T = 0) has no element to address, and its Batch is never launched on."""
    n, T = t.shape
    s = t.stride(0)
    return Batch(n, T, T if dense or (n <= 1 and (lone_dense or s < T)) else s)


def _same_layout(ts):
    """[N, T] tensors of one call -> the same tensors on one layout: inner stride 1 (wherever T > 1) and, for N > 1, one row pitch.
    Arguments that agree already are returned as they are (no copy, the same objects).  N > 1, T > 0: an argument that disagrees with
    the first one's pitch is made dense, and so are all of them unless the first one is dense already.
    One row (N = 1) and empty tensors (N = 0 or T = 0) have no pitch to agree on -- torch ignores the stride of a size-1 dimension and
    calls every zero-element tensor contiguous, so contiguous() would hand them back unchanged.  One-row arguments that report one
    stride(0) and inner stride 1 pass as they are; where they disagree, every one is re-viewed at stride(0) = T without a copy (a row with
    an inner stride other than 1 is copied), so that no batch stride taken from one argument makes a kernel address another beyond the T
    elements of its row.  Empty arguments pass as they are for N <= 1; for N > 1 those that disagree are replaced by fresh empty [N, 0]
    tensors of one stride."""
    n, T = ts[0].shape
    for t in ts:
        if t.shape != (n, T):
            raise PqError(f"input shapes differ: {tuple(t.shape)} vs {(n, T)}")
    s0 = ts[0].stride(0)
    if n <= 1 or T == 0:
        if n == 0 or all(t.stride(0) == s0 and (t.stride(1) == 1 or T <= 1) for t in ts):
            return list(ts)
        if T == 0:
            return [t.new_empty((n, 0)) for t in ts]
        return [t.as_strided((1, T), (T, 1)) if t.stride(1) == 1 or T == 1 else t.contiguous() for t in ts]
    dense = s0 != T and any(t.stride(0) != s0 or t.stride(1) != 1 for t in ts)
    return [t.contiguous() if dense or t.stride(0) != s0 or t.stride(1) != 1 else t for t in ts]


def count_nulls(t: torch.Tensor) -> int:
    t2, _, _ = _to_device(t)
    n = C.c_int64(0)
    _call("pq_count_nulls", None, ctx(t2.device.index), _batch(t2), t2, C.byref(n))
    return n.value


def ragged_batch(offsets, device):
    """offsets: n + 1 ascending row indices (series s = rows [offsets[s], offsets[s + 1]) of the long columns, sorted by symbol:
    the groups of `.over("symbol")`) -> (Batch, the device copy it points at)."""
    off = torch.as_tensor(np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets), dtype=torch.int64).reshape(-1)
    if off.numel() < 1 or (off.numel() > 1 and bool((off[1:] < off[:-1]).any())) or int(off[0]) != 0:
        raise PqError("offsets must be n + 1 ascending row indices starting at 0 (rows in front of the first group would belong to no "
                      "group and their outputs would stay unwritten)")
    n = off.numel() - 1
    longest = int((off[1:] - off[:-1]).max()) if n else 0
    total = int(off[-1])
    dev_off = off.to(device)
    return Batch(n, longest, total, dev_off.data_ptr()), dev_off


def call(name: str, *inputs, check_nulls: bool = False, offsets=None, **params):
    """Run indicator `name` (lower-case plugin name, e.g. "ema") -> tuple of outputs.
    offsets: run it over the groups of LONG columns ([rows], sorted by symbol) instead of [N, T] matrices -- every group as if it
    were passed alone, one launch for all of them (what the reference does with one plugin call per group under .over("symbol"))."""
    if name in PATTERN_NAMES:
        return (cdl(name, *inputs, offsets=offsets, **params),)
    cols, pspec, outs, fam = SPEC[name] if name in SPEC else EXTRA[name]
    if len(inputs) != len(cols):
        raise TypeError(f"{name}() takes inputs {cols}")
    conv = [_to_device(x) for x in inputs]
    kind, squeeze = conv[0][1], conv[0][2]
    ts = _same_layout([c[0] for c in conv])
    dev = ts[0].device
    if offsets is not None:
        if not squeeze:
            raise PqError("with offsets the inputs are long columns [rows]")
        ts = [t.contiguous() for t in ts]
        b, _off = ragged_batch(offsets, dev)       # (_off: the device offsets the batch points at)
        if b.stride != ts[0].shape[1]:
            raise PqError(f"offsets end at row {b.stride} but the columns have {ts[0].shape[1]} rows")
        shape, live = (1, b.stride), b.n_series and b.stride
    else:
        if fam == NB and (check_nulls or kind in (_Kind.ARROW, _Kind.POLARS)):
            for t in ts:
                if count_nulls(t):
                    raise NullsNotAllowed(f"{name}: input contains nulls (the reference's cont_slice() rejects them)")
        b = _batch(ts[0], lone_dense=True)
        shape, live = tuple(ts[0].shape), b.n_series * b.len > 0   # an empty batch has no device storage to point at
    pvals = []
    for pname, k, default in pspec:
        v = params.pop(pname, default)
        pvals.append(int(v) if k == I else float(v))
    if params:
        raise TypeError(f"{name}() got unexpected parameters {sorted(params)}")
    res = [torch.empty_strided(shape, (b.stride, 1), dtype=torch.float64 if dt == "f8" else torch.int32, device=dev) for _, dt in outs]
    if live:
        _call("pq_" + name, dev, b, *ts, *pvals, *res)
    return tuple(_from_device(r, kind, squeeze, oname) for r, (oname, _) in zip(res, outs))


def cdl(name: str, open, high, low, close, penetration: float | None = None, offsets=None):
    pid = PATTERN_NAMES.index(name)
    pen = PATTERN_PEN_DEFAULT[name] if penetration is None else float(penetration)
    conv = [_to_device(x) for x in (open, high, low, close)]
    kind, squeeze = conv[0][1], conv[0][2]
    ts = _same_layout([c[0] for c in conv])
    dev = ts[0].device
    if offsets is not None:
        ts = [t.contiguous() for t in ts]
        b, _off = ragged_batch(offsets, dev)
        out = torch.zeros((1, b.stride), dtype=torch.int32, device=dev)
        squeeze, live = True, b.n_series and b.stride
    else:
        if kind in (_Kind.ARROW, _Kind.POLARS):
            for t in ts:
                if count_nulls(t):
                    raise NullsNotAllowed(f"{name}: input contains nulls")
        b = _batch(ts[0], lone_dense=True)
        out = torch.empty_strided(tuple(ts[0].shape), (b.stride, 1), dtype=torch.int32, device=dev)
        live = True
    if live:
        _call("pq_cdl", dev, b, pid, *ts, pen, out)
    return _from_device(out, kind, squeeze, name)


def cdl_all(open, high, low, close, penetrations: dict | None = None, names=None):
    """All (or `names`) candlestick recognisers in one pass over OHLC -> dict name -> int32 [N,T]."""
    conv = [_to_device(x) for x in (open, high, low, close)]
    kind, squeeze = conv[0][1], conv[0][2]
    ts = _same_layout([c[0] for c in conv])
    dev = ts[0].device
    b = _batch(ts[0], lone_dense=True)
    want = PATTERN_NAMES if names is None else list(names)
    outs = {nm: torch.empty_strided(tuple(ts[0].shape), (b.stride, 1), dtype=torch.int32, device=dev) for nm in want}
    pens = (C.c_double * 61)(*[(penetrations or {}).get(nm, PATTERN_PEN_DEFAULT[nm]) for nm in PATTERN_NAMES])
    ptrs = (C.c_void_p * 61)(*[outs[nm].data_ptr() if nm in outs else None for nm in PATTERN_NAMES])
    _call("pq_cdl_all", dev, b, *ts, pens, ptrs)
    return {nm: _from_device(o, kind, squeeze, nm) for nm, o in outs.items()}


def backtest_vectorized(price, buy, sell, benchmark=None, want_curves: bool = True, offsets=None, **kw):
    """Batched VectorizedBacktester.run(): -> (position, cash, equity, summary[N,8]) (curves None if not wanted).
    offsets: the columns are long columns of ragged groups (see call()); summary [n_groups, 8]."""
    prm = BtParams(**{**BT_DEFAULTS, **kw})
    p, kind, squeeze = _to_device(price)
    bu, _, _ = _to_device(buy, torch.uint8)
    se, _, _ = _to_device(sell, torch.uint8)
    p = p.contiguous(); bu = bu.contiguous(); se = se.contiguous()
    dev = p.device
    n, T = p.shape
    bm = None
    if offsets is not None:
        b, _off = ragged_batch(offsets, dev)
        bm = _to_device(benchmark)[0].contiguous() if benchmark is not None else None
        for nm, t in (("buy", bu), ("sell", se), ("benchmark", bm)):
            if t is not None and t.shape != p.shape:
                raise PqError(f"backtest_vectorized: `{nm}` must be a long column like `price`")
        rows, sq, sq_summ, live = (1, b.stride), True, False, b.n_series
    else:
        # the kernel indexes every column as base + s * stride: all of them must be [N, T] like the prices
        for nm, t in (("buy", bu), ("sell", se)):
            if t.shape == (1, T) and n > 1:
                raise PqError(f"backtest_vectorized: `{nm}` is one series but `price` has {n}; signals are per series ([N, T])")
            if t.shape != (n, T):
                raise PqError(f"backtest_vectorized: `{nm}` has shape {tuple(t.shape)}, expected {(n, T)}")
        if benchmark is not None:
            bm = _to_device(benchmark)[0]
            if bm.shape == (1, T) and n > 1:
                bm = bm.expand(n, T)          # one benchmark series shared by all symbols (the reference is single-asset)
            if bm.shape != (n, T):
                raise PqError(f"backtest_vectorized: `benchmark` has shape {tuple(bm.shape)}, expected {(T,)} or {(n, T)}")
            bm = bm.contiguous()
        b = _batch(p, dense=True)
        rows, sq, sq_summ, live = (n, T), squeeze, squeeze, True
    mk = lambda: torch.empty(rows, dtype=torch.float64, device=dev)
    pos, cash, eq = (mk(), mk(), mk()) if want_curves else (None, None, None)
    summ = torch.empty((b.n_series, 8), dtype=torch.float64, device=dev)
    if live:
        _call("pq_backtest_vectorized", dev, b, p, bu, se, bm, prm, pos, cash, eq, summ)
    k = kind if kind in (_Kind.TORCH, _Kind.NUMPY) else _Kind.NUMPY
    f = lambda t, s: _from_device(t, k, s) if t is not None else None
    return f(pos, sq), f(cash, sq), f(eq, sq), f(summ, sq_summ)


def backtest_macd_cross(close, fastperiod=12, slowperiod=26, signalperiod=9, want_curves: bool = True, offsets=None, **kw):
    """Fused MACD-cross strategy + per-symbol backtest + summary (one kernel).  offsets: `close` is a long column of ragged
    groups (see call()); the curves come back as long columns, the summary as [n_groups, 8]."""
    prm = BtParams(**{**BT_DEFAULTS, **kw})
    p, kind, squeeze = _to_device(close)
    p = p.contiguous()
    dev = p.device
    b = _batch(p, dense=True)
    if offsets is not None:
        b, _off = ragged_batch(offsets, dev)
    mk = lambda: torch.empty(tuple(p.shape), dtype=torch.float64, device=dev)
    pos, cash, eq = (mk(), mk(), mk()) if want_curves else (None, None, None)
    summ = torch.empty((b.n_series, 8), dtype=torch.float64, device=dev)
    if b.n_series:
        _call("pq_backtest_macd_cross", dev, b, p, fastperiod, slowperiod, signalperiod, prm, pos, cash, eq, summ)
    f = lambda t, sq=squeeze: _from_device(t, kind if kind in (_Kind.TORCH, _Kind.NUMPY) else _Kind.NUMPY, sq) if t is not None else None
    return f(pos), f(cash), f(eq), f(summ, squeeze and offsets is None)


def _stats(name: str, k: int, reset: bool, device):
    """the k int64 counters of a pq_*_stats entry point since the last reset -> tuple; synchronises the stream"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = (C.c_int64 * k)()
    _call(name, dev, out, 1 if reset else 0)
    return tuple(int(v) for v in out)


def backtest_wave_stats(reset: bool = False, device=None):
    """(symbols run by the wave-per-symbol backtest, speculative chunks that failed the bit test, chunk re-runs) since the last
    reset -- pq_backtest_wave_stats (csrc/ops_backtest_wave.h).  Synchronises the stream."""
    return _stats("pq_backtest_wave_stats", 3, reset, device)


def ragged_rehouse_stats(reset: bool = False, device=None) -> int:
    """launches on a ragged batch that took the re-housed tiled path (pq_ragged_rehouse_stats) since the last reset"""
    return _stats("pq_ragged_rehouse_stats", 1, reset, device)[0]


def wt_stats(reset: bool = False, device=None):
    """(symbols computed by the wave-per-symbol indicator kernels, speculative chunks that failed the bit test, chunk re-runs,
    symbols handed to the gated lane-per-symbol path) since the last reset -- pq_wt_stats (csrc/wt_dev.h).  Synchronises."""
    return _stats("pq_wt_stats", 4, reset, device)


def factor_ic(factor, fwd_return, method: int = 0):
    """D-12: per-day cross-sectional IC of factor vs forward return, both [N, T] -> (ic [T], n_valid [T]) device tensors.
    method 0 = Pearson IC, 1 = Spearman Rank-IC"""
    f = _to_device(factor)[0].contiguous()
    r = _to_device(fwd_return)[0].contiguous()
    if f.shape != r.shape:
        raise ValueError("factor and fwd_return must have the same shape")
    dev = f.device
    n, T = f.shape
    ic = torch.empty(T, dtype=torch.float64, device=dev)
    nv = torch.zeros(T, dtype=torch.int32, device=dev)
    if T and n:
        _call("pq_factor_ic", dev, _batch(f, dense=True), f, r, int(method), ic, nv)
    elif T:
        ic.fill_(float("nan"))
    return ic, nv


def rolling_ic(ic, window: int):
    """D-12: rolling mean of the IC series and its information ratio -> (rolling_ic, rolling_ir) device tensors [T]"""
    t = _to_device(ic)[0].contiguous().reshape(-1)
    ric, rir = torch.empty_like(t), torch.empty_like(t)
    if t.numel():
        _call("pq_rolling_ic", t.device, t, t.numel(), int(window), ric, rir)
    return ric, rir


def _xsec_inputs(cols):
    """factor (+ fwd_return) -> device tensors on one row pitch and the Batch that describes them"""
    ts = [_to_device(c)[0] for c in cols]
    if any(t.shape != ts[0].shape for t in ts):
        raise ValueError("factor and fwd_return must have the same shape")
    ts = _same_layout(ts)
    return ts, _batch(ts[0])


def _factor_groups(fn_name, factor, fwd_return, n_groups, scalars, labels):
    (f, r), b = _xsec_inputs([factor, fwd_return])
    dev = f.device
    n, T = f.shape
    out = {
        "mean_return": torch.empty((n_groups, T), dtype=torch.float64, device=dev),
        "count": torch.empty((n_groups, T), dtype=torch.int32, device=dev),
        "turnover": torch.empty((n_groups, T), dtype=torch.float64, device=dev),
        "spread": torch.empty(T, dtype=torch.float64, device=dev),
        "summary": torch.empty((n_groups + 1, SUMMARY_COLS), dtype=torch.float64, device=dev),
    }
    lab = torch.empty((n, b.stride), dtype=torch.uint8, device=dev) if labels else None
    _call(fn_name, dev, b, f, r, *scalars, lab, *out.values())
    if lab is not None:
        out["labels"] = lab[:, :T]
    return out


SUMMARY_COLS = 5  # PQ_GROUP_SUMMARY_COLS: n_days, mean_return, std_return, sharpe, mean_turnover
LABEL_OUT, LABEL_MID = 255, 254  # PQ_LABEL_OUT (not in the day's cross-section), PQ_LABEL_MID (in neither leg)


def factor_quantiles(factor, fwd_return, n_quantiles: int = 5, labels: bool = False):
    """D-15: per-day quantile sort of the factor (bucket 0 = lowest values, ties share a bucket) -> dict of device tensors:
    mean_return / count / turnover [Q, T], spread [T] (top - bottom bucket), summary [Q + 1, 5] (last row: the spread), and with
    labels=True labels uint8 [N, T] (LABEL_OUT outside the day's cross-section)"""
    return _factor_groups("pq_factor_quantiles", factor, fwd_return, int(n_quantiles), [int(n_quantiles)], labels)


def factor_long_short(factor, fwd_return, top_pct: float = 0.2, bottom_pct: float = 0.2, labels: bool = False):
    """D-15: per-day long (top top_pct) and short (bottom bottom_pct) legs -> dict of device tensors: mean_return / count / turnover
    [2, T] (row 0 = short, row 1 = long), ls_return [T] = long - short, summary [3, 5], and with labels=True labels uint8 [N, T]
    (1 long, 0 short, LABEL_MID in neither leg, LABEL_OUT outside the day's cross-section)"""
    out = _factor_groups("pq_factor_long_short", factor, fwd_return, 2, [float(top_pct), float(bottom_pct)], labels)
    out["ls_return"] = out.pop("spread")
    return out


def factor_double_sort(control, factor, fwd_return, n_control: int = 2, n_quantiles: int = 3, dependent: bool = True,
                       labels: bool = False):
    """D-31: per-day two-way sort of the symbols into Qa = n_control buckets of `control` times Qb = n_quantiles buckets of `factor`,
    over the symbols where control, factor and return are all non-null and finite; dependent=True sorts the factor inside each
    control bucket, False sorts both over the whole sample.  -> dict of device tensors: mean_return / count / turnover [Qa * Qb, T]
    (cell a * Qb + b), spread_factor [Qa + 1, T] (top - bottom factor bucket inside control bucket a; last row: their average),
    spread_control [Qb + 1, T] (the same along the other axis), summary [Qa * Qb + Qa + Qb + 2, 5] (the cells, then the rows of
    spread_factor, then those of spread_control), and with labels=True labels uint8 [N, T] (a * Qb + b; LABEL_MID in a dependent
    bucket with fewer than Qb members, LABEL_OUT outside the day's sample)"""
    (a, f, r), b = _xsec_inputs([control, factor, fwd_return])
    dev = f.device
    n, T = f.shape
    qa, qb = int(n_control), int(n_quantiles)
    C = max(qa, 0) * max(qb, 0)
    out = {
        "mean_return": torch.empty((C, T), dtype=torch.float64, device=dev),
        "count": torch.empty((C, T), dtype=torch.int32, device=dev),
        "turnover": torch.empty((C, T), dtype=torch.float64, device=dev),
        "spread_factor": torch.empty((max(qa, 0) + 1, T), dtype=torch.float64, device=dev),
        "spread_control": torch.empty((max(qb, 0) + 1, T), dtype=torch.float64, device=dev),
        "summary": torch.empty((C + max(qa, 0) + max(qb, 0) + 2, SUMMARY_COLS), dtype=torch.float64, device=dev),
    }
    lab = torch.empty((n, b.stride), dtype=torch.uint8, device=dev) if labels else None
    _call("pq_factor_double_sort", dev, b, a, f, r, qa, qb, 1 if dependent else 0, lab, *out.values())
    if lab is not None:
        out["labels"] = lab[:, :T]
    return out


def factor_coverage(factor):
    """D-15: share of the symbols with a non-null finite factor value, per day -> device tensor [T]"""
    (f,), b = _xsec_inputs([factor])
    cov = torch.empty(f.shape[1], dtype=torch.float64, device=f.device)
    _call("pq_factor_coverage", f.device, b, f, cov)
    return cov


def ic_stats(ic):
    """D-15: statistics of an IC series over its non-null days -> device tensor [5]: n_days, mean, std, ir (mean / std), win_rate"""
    t = _to_device(ic)[0].contiguous().reshape(-1)
    out = torch.empty(5, dtype=torch.float64, device=t.device)
    _call("pq_ic_stats", t.device, t, t.numel(), out)
    return out


def _labels_on_pitch(labels, b, dev, shape):
    """uint8 group labels [N, T] -> a device tensor whose rows lie on the batch's pitch: the tensor that factor_quantiles / factor_long_short
    (labels=True) returned for columns of the same pitch is taken as it is, anything else is copied once"""
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if tuple(lab.shape) != tuple(shape):
        raise ValueError(f"labels must have the shape of price {tuple(shape)}, not {tuple(lab.shape)}")
    if lab.dtype != torch.uint8:
        raise ValueError(f"labels must be uint8 (group numbers, LABEL_MID, LABEL_OUT), not {lab.dtype}")
    n, T = shape
    if lab.device == dev and (T <= 1 or lab.stride(1) == 1) and (n <= 1 or lab.stride(0) == b.stride):
        return lab
    buf = torch.empty((n, b.stride), dtype=torch.uint8, device=dev)
    buf[:, :T].copy_(lab)
    return buf[:, :T]


def factor_portfolio(labels, price, n_groups: int, rebalance_days, weight=None, label_lag: int = 0, cost_rate: float = 0.0,
                     initial_capital: float = 1_000_000.0):
    """D-27: the portfolios of the groups 0 .. n_groups - 1 of `labels` (uint8 [N, T], as factor_quantiles / factor_long_short return
    them with labels=True), re-formed on the ascending day indices `rebalance_days` from the labels of day d - label_lag and held in
    between: members weighted by weight[s][d] (None: equally) drift with their prices (a symbol without a usable price keeps its last
    one), and every rebalance pays cost_rate on the traded value (buys and sells both counted).  -> dict of device tensors: value
    [G, T] (initial_capital before the first rebalance day), turnover [G, R] (traded value over portfolio value), count int32 [G, R]
    (members), rebalance_days int32 [R].  The definitions are in include/pq_hip.h."""
    days = np.asarray(rebalance_days)
    if days.size and days.dtype.kind not in "iu":
        raise ValueError("rebalance_days must hold integer day indices")
    days = days.reshape(-1).astype(np.int64)
    if days.size and (days.min() < -2**31 or days.max() >= 2**31):
        raise ValueError("rebalance_days must fit int32")
    days = np.ascontiguousarray(days.astype(np.int32))
    ts, b = _xsec_inputs([price] if weight is None else [price, weight])
    p, wt = ts[0], (ts[1] if weight is not None else None)
    dev = p.device
    n, T = p.shape
    lab = _labels_on_pitch(labels, b, dev, (n, T))
    G, R = max(int(n_groups), 0), days.size
    out = {"value": torch.empty((G, T), dtype=torch.float64, device=dev),
           "turnover": torch.empty((G, R), dtype=torch.float64, device=dev),
           "count": torch.empty((G, R), dtype=torch.int32, device=dev)}
    _call("pq_factor_portfolio", dev, b, lab, int(n_groups), int(label_lag), p, wt, days if R else None, R, float(cost_rate),
          float(initial_capital), *out.values())
    out["rebalance_days"] = torch.from_numpy(days).to(dev)
    return out


WEIGHTS_MAX_PORTFOLIOS = 8    # PQ_WEIGHTS_MAX_PORTFOLIOS


def _factor_weights_args(weights, price, rebalance_days, cost_rate, initial_capital, holdings_of):
    """argument checks of factor_weights that need no device -> (list of P [N, R] weight arrays, (N, T), int32 days [R], cost_rate,
    initial_capital, holdings_of as -1 or an index)"""
    shapes = "weights must be one [N, R] array, a list of [N, R] arrays or one [P, N, R] array"
    if isinstance(weights, (list, tuple)):
        cols = list(weights)
    else:
        ws = _shape(weights)
        if len(ws) not in (2, 3):
            raise ValueError(f"{shapes}, not {ws}")
        cols = [weights] if len(ws) == 2 else [weights[j] for j in range(ws[0])]
    if not 1 <= len(cols) <= WEIGHTS_MAX_PORTFOLIOS:
        raise ValueError(f"the number of portfolios must be in 1..{WEIGHTS_MAX_PORTFOLIOS}, not {len(cols)}")
    ps = _shape(price)
    if len(ps) != 2:
        raise ValueError(f"price must be [N, T], not {ps}")
    n, T = ps
    days = np.asarray(rebalance_days)
    if days.size and days.dtype.kind not in "iu":
        raise ValueError("rebalance_days must hold integer day indices")
    days = days.reshape(-1).astype(np.int64)
    if days.size and (days.min() < 0 or days.max() >= T):
        raise ValueError(f"rebalance_days must lie in [0, T) = [0, {T})")
    if (np.diff(days) <= 0).any():
        raise ValueError("rebalance_days must be strictly ascending")
    for j, c in enumerate(cols):
        if _shape(c) != (n, days.size):
            raise ValueError(f"weights {j} must be [N, R] = {(n, days.size)} (one column per rebalance day), not {_shape(c)}")
    cost, cap = float(cost_rate), float(initial_capital)
    if not 0.0 <= cost < 1.0:
        raise ValueError(f"cost_rate must be in [0, 1), not {cost_rate!r}")
    if not 0.0 < cap < float("inf"):
        raise ValueError(f"initial_capital must be positive and finite, not {initial_capital!r}")
    if holdings_of is None:
        ho = -1
    else:
        if not hasattr(holdings_of, "__index__") or isinstance(holdings_of, bool) or not 0 <= int(holdings_of) < len(cols):
            raise ValueError(f"holdings_of must be None or a portfolio index in 0..{len(cols) - 1}, not {holdings_of!r}")
        ho = int(holdings_of)
    return cols, (n, T), np.ascontiguousarray(days.astype(np.int32)), cost, cap, ho


def factor_weights(weights, price, rebalance_days, cost_rate: float = 0.001, initial_capital: float = 1_000_000.0, holdings_of=None):
    """D-35: the backtest of GIVEN target weights.  weights: one [N, R] array, a list of P such arrays or one [P, N, R] array
    (1 <= P <= 8), column k the weights bought on rebalance_days[k] (risk_solve's / Factor.optimal_portfolio's layout); they are signed,
    need not sum to one -- the remainder 1 - sum w is cash, negative under leverage -- and a NULL, NaN or infinite weight is not held.
    price [N, T]; rebalance_days strictly ascending in [0, T).  A target without a usable price on its rebalance day is dropped (counted,
    its weight stays in cash); holdings drift with their prices (a symbol without a usable price keeps its last one) and every rebalance
    pays cost_rate on the traded value.  The P portfolios share one pass over the prices.
    -> dict of device tensors: value [P, T], turnover, net, gross [P, R], n_long, n_short, n_dropped int32 [P, R], first_nonpositive
    int32 [P] (the first day whose value is not > 0, -1 if none: a signed, levered book can be ruined, and the curve after that day means
    nothing), rebalance_days int32 [R] and, with holdings_of = p, holdings [N, T]: portfolio p's drifted weights on every day (0.0 where
    nothing is held), the array that risk_portfolio reads.  The definitions are in include/pq_hip.h."""
    cols, (n, T), days, cost, cap, ho = _factor_weights_args(weights, price, rebalance_days, cost_rate, initial_capital, holdings_of)
    P, R = len(cols), days.size
    p = _to_device(price)[0]
    dev = p.device
    if T > 1 and p.stride(1) != 1:
        p = p.contiguous()
    b = _batch(p)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    hold = torch.empty((n, b.stride), **f64)[:, :T] if ho >= 0 else None
    if n == 0 or T == 0 or R == 0:                     # nothing is launched: every portfolio is its capital in cash
        out = {"value": torch.full((P, T), cap, **f64), "turnover": torch.zeros((P, R), **f64), "net": torch.zeros((P, R), **f64),
               "gross": torch.zeros((P, R), **f64), "n_long": torch.zeros((P, R), **i32), "n_short": torch.zeros((P, R), **i32),
               "n_dropped": torch.zeros((P, R), **i32), "first_nonpositive": torch.full((P,), -1, **i32)}
        if hold is not None:
            hold.zero_()
    else:
        wd = [_to_device(c)[0].to(dev) for c in cols]       # on one row pitch >= R (risk_solve's y passes as it is), else dense
        ws = wd[0].stride(0) if n > 1 and wd[0].stride(0) >= R else R
        if not all((R <= 1 or w.stride(1) == 1) and (n <= 1 or w.stride(0) == ws) for w in wd):
            wd, ws = [w.contiguous() for w in wd], R
        value, tov = torch.empty((P, T), **f64), torch.empty((P, R), **f64)
        expo, cnt, first = torch.empty((2, P, R), **f64), torch.empty((3, P, R), **i32), torch.empty((P,), **i32)
        wp = (C.c_void_p * P)(*[w.data_ptr() for w in wd])
        _call("pq_factor_weights", dev, b, wp, P, ws, p, days, R, cost, cap, value, tov, expo, cnt, first, ho, hold)
        out = {"value": value, "turnover": tov, "net": expo[0], "gross": expo[1], "n_long": cnt[0], "n_short": cnt[1],
               "n_dropped": cnt[2], "first_nonpositive": first}
    out["rebalance_days"] = torch.from_numpy(days).to(dev)
    if hold is not None:
        out["holdings"] = hold
    return out


CLEAN_WINSORIZE = {None: 0, "mad": 1, "sigma": 2, "percentile": 3}     # pq_factor_clean's winsorize codes
CLEAN_WINSORIZE_N = {"mad": 3.0, "sigma": 3.0, "percentile": 1.0}    # the README's defaults
IC_MAX_GROUPS = 256                  # PQ_IC_MAX_GROUPS: the one limit on group (industry) codes, XS_MAX_GROUPS in csrc/xsec
MAX_INDUSTRIES = IC_MAX_GROUPS       # its older name


def _int_codes(codes, what):
    """integer codes handed over as a tensor or an array -> tensor (where it is); floating point or boolean codes are refused"""
    g = codes if isinstance(codes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(codes)))
    if g.dtype.is_floating_point or g.dtype.is_complex or g.dtype == torch.bool:
        raise ValueError(f"{what} must hold integer codes")
    return g


def _n_codes(g, what, limit):
    """max code + 1 of the codes g (at least 1), at most `limit`"""
    G = int(g.max()) + 1 if g.numel() else 1
    if G > limit:
        raise ValueError(f"{what} codes must be < {limit} (negative = unclassified), got a code {G - 1}")
    return max(G, 1)


def _codes_on_pitch(codes, b, dev, spread: bool = False):
    """integer codes [N] or [N, T] -> (int32 device tensor, its row pitch): [N, T] codes go onto the batch's row pitch; [N] codes stay
    one per symbol (pitch 0), or with `spread` are written to every day of the symbol's row"""
    g = codes.to(device=dev, dtype=torch.int32)
    if g.dim() == 1 and not spread:
        return g.contiguous(), 0
    gp = torch.empty((b.n_series, b.stride), dtype=torch.int32, device=dev)
    gp[:, :b.len] = g if g.dim() == 2 else g[:, None]
    return gp, b.stride


def _clean_args(winsorize, winsorize_n, industry):
    """argument checks of factor_clean that need no device: -> (mode, winsorize_n, industry as an integer tensor or None, n_industries)"""
    if winsorize not in CLEAN_WINSORIZE:
        raise ValueError(f"winsorize must be one of None, 'mad', 'sigma', 'percentile', not {winsorize!r}")
    mode = CLEAN_WINSORIZE[winsorize]
    wn = 0.0 if winsorize is None else float(CLEAN_WINSORIZE_N[winsorize] if winsorize_n is None else winsorize_n)
    if winsorize in ("mad", "sigma") and not (0.0 <= wn < float("inf")):
        raise ValueError(f"winsorize_n must be finite and >= 0 for {winsorize!r}, not {wn}")
    if winsorize == "percentile" and not (0.0 <= wn / 100.0 < 0.5):
        raise ValueError(f"percentile winsorize needs 0 <= winsorize_n < 50 (percent), not {wn}")
    if industry is None:
        return mode, wn, None, 0
    ind = _int_codes(industry, "industry")
    return mode, wn, ind, _n_codes(ind, "industry", MAX_INDUSTRIES)


def factor_clean(factor, winsorize=None, winsorize_n=None, cap=None, log_cap: bool = True, industry=None, standardize: bool = False):
    """D-16: per-day cross-sectional cleaning of an [N, T] factor in the README's order -> device tensor [N, T] (f64, NULL outside the
    day's cross-section and on days with fewer than 2 members).
    winsorize: None, "mad" (clip to median +- winsorize_n * 1.4826 MAD, default 3), "sigma" (mean +- winsorize_n std, default 3) or
    "percentile" (the winsorize_n % and (100 - winsorize_n) % quantiles, default 1); cap [N, T]: OLS residual on log(cap) (log_cap) or
    on cap; industry int codes [N] or [N, T] (negative = unclassified, at most 256 industries): minus the day's industry mean;
    standardize: (x - mean) / sample std (NULL on days whose std is 0)."""
    mode, wn, ind, G = _clean_args(winsorize, winsorize_n, industry)
    f = _to_device(factor)[0]
    n, T = f.shape
    ts = [f]
    if cap is not None:
        z = _to_device(cap)[0]
        if z.shape != f.shape:
            raise ValueError(f"cap must have the factor's shape {tuple(f.shape)}, not {tuple(z.shape)}")
        if log_cap:      # into a column on the factor's row pitch, so that both keep it (whole rows: a lone row owns the pitch it reports)
            zl = torch.empty((n, max(f.stride(0), T)), dtype=torch.float64, device=f.device)[:, :T]
            torch.log(z, out=zl)
            z = zl
        ts.append(z)
    ts = _same_layout(ts)
    f, z = ts[0], ts[1] if cap is not None else None
    b = _batch(f)
    dev = f.device
    ib = None
    if ind is not None:
        ish = tuple(ind.shape) + ((1,) if ind.dim() == 1 else ())
        if len(ish) != 2 or ish[0] != n or ish[1] not in (1, T):
            raise ValueError(f"industry must be [N] or [N, T] with N = {n}, T = {T}, not {ish}")
        ib, _ = _codes_on_pitch(ind, b, dev, spread=True)
    out = torch.empty((n, b.stride), dtype=torch.float64, device=dev)
    _call("pq_factor_clean", dev, b, f, mode, wn, z, ib, G, 1 if standardize else 0, out)
    return out[:, :T]


REGRESS_MAX_K = 8             # PQ_REGRESS_MAX_K
REGRESS_SUMMARY_COLS = 5      # PQ_REGRESS_SUMMARY_COLS: n_days, mean_coef, std_coef, t_stat, p_value


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _columns(x, what, lo, hi, ndim=None, shapes="", exc=ValueError):
    """a list / tuple of columns, or one stacked [K, ...] array of `ndim` dimensions (`shapes` words the refusal of another), holding
    lo..hi columns (else exc: "`what` must be in lo..hi") -> the list of the columns"""
    if isinstance(x, (list, tuple)):
        cols = list(x)
    else:
        s = _shape(x)
        if ndim is not None and len(s) != ndim:
            raise ValueError(f"{shapes}, not {s}")
        cols = [x[j] for j in range(s[0])]
    if not lo <= len(cols) <= hi:
        raise exc(f"{what} must be in {lo}..{hi}, not {len(cols)}")
    return cols


def _regress_args(factors, ret, series_ok):
    """argument checks of xsec_regress / ts_regress that need no device: factors a list / tuple of [N, T] (or, series_ok, [T]) arrays
    or one [K, N, T] array -> (list of factor columns, [N, T] of the return)"""
    rs = _shape(ret)
    if len(rs) != 2:
        raise ValueError(f"the return must be [N, T], not {rs}")
    cols = _columns(factors, "the number of factors", 1, REGRESS_MAX_K, 3, "factors must be a list of [N, T] arrays or one [K, N, T] array")
    for j, c in enumerate(cols):
        cs = _shape(c)
        if cs != rs and not (series_ok and cs == rs[1:]):
            want = f"{rs} or {rs[1:]}" if series_ok else f"{rs}"
            raise ValueError(f"factor {j} must have shape {want}, not {cs}")
    return cols, rs


def _regress_upload(cols, ret, series_ok):
    """uploads the factor columns and the return onto one row pitch -> (the device columns, the mask of the [T] series among them, the
    device return, the host array of the columns' pointers or None for an empty batch)"""
    ser = [series_ok and len(_shape(c)) == 1 for c in cols]
    mats = _same_layout([_to_device(c)[0] for c, s in zip(cols, ser) if not s] + [_to_device(ret)[0]])
    r = mats[-1]
    it = iter(mats[:-1])
    fs = [_to_device(c)[0].reshape(-1).contiguous() if s else next(it) for c, s in zip(cols, ser)]
    mask = sum(1 << j for j, s in enumerate(ser) if s)
    ptrs = (C.c_void_p * len(fs))(*[f.data_ptr() for f in fs]) if r.numel() else None
    return fs, mask, r, ptrs


def _regress_call(fn_name, cols, ret, series_ok, make_outs, extra):
    """uploads the factor columns and the return onto one row pitch, allocates the outputs on their device (make_outs(device) -> list of
    output tensors, None: not written) and calls fn_name"""
    fs, mask, r, ptrs = _regress_upload(cols, ret, series_ok)
    outs = make_outs(r.device)
    _call(fn_name, r.device, _batch(r), ptrs, len(fs), *extra(mask), r, *outs)
    return outs


def xsec_regress(factors, fwd_return, summary: bool = True):
    """D-17: per-day cross-sectional OLS of the forward return on K factors (each [N, T]; a list or a [K, N, T] array) with an intercept
    -> dict of device tensors: coef / t_stat / p_value [K + 1, T] (row K = the intercept), r_squared [T], n [T] (int32), and with
    summary=True the Fama-MacBeth summary [K + 1, 5]: n_days, mean_coef, std_coef, t_stat, p_value over the days with a solution"""
    cols, (n, T) = _regress_args(factors, fwd_return, False)
    K = len(cols)

    def make(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        return [torch.empty((K + 1, T), **f64), torch.empty((K + 1, T), **f64), torch.empty((K + 1, T), **f64), torch.empty(T, **f64),
                torch.empty(T, dtype=torch.int32, device=dev), torch.empty((K + 1, REGRESS_SUMMARY_COLS), **f64) if summary else None]
    coef, t, p, r2, nobs, summ = _regress_call("pq_xsec_regress", cols, fwd_return, False, make, lambda mask: ())
    out = {"coef": coef, "t_stat": t, "p_value": p, "r_squared": r2, "n": nobs}
    if summ is not None:
        if T == 0:      # no day: nothing was launched
            summ.copy_(torch.tensor([[0.0] + [float("nan")] * 4] * (K + 1), dtype=torch.float64))
        out["summary"] = summ
    return out


def xsec_regress_wls(factors, fwd_return, weight=None, industry=None, summary: bool = True, resid: bool = False):
    """D-32: per-day weighted cross-sectional regression of the forward return on K factors (each [N, T]; a list or a [K, N, T] array)
    and G industry dummies, without a separate intercept.  weight [N, T] (None: 1.0; a symbol needs a finite weight > 0), industry int
    codes [N] or [N, T] (negative = unclassified, at most 256 industries, G = max code + 1; None: one group, whose row is the intercept)
    -> dict of device tensors: coef / t_stat / p_value [K + G, T] (the factors, then the industries), r_squared / r_squared_within
    [T], n / n_industries [T] (int32), with summary=True the Fama-MacBeth summary [K + G, 5], with resid=True resid [N, T]"""
    cols, (n, T) = _regress_args(factors, fwd_return, False)
    K = len(cols)
    ind, G = None, 1
    if industry is not None:
        ind = _int_codes(industry, "industry")
        if tuple(ind.shape) not in ((n,), (n, T)):
            raise ValueError(f"industry must be [N] or [N, T] with N = {n}, T = {T}, not {tuple(ind.shape)}")
        G = _n_codes(ind, "industry", MAX_INDUSTRIES)
    if weight is not None and _shape(weight) != (n, T):
        raise ValueError(f"weight must have the return's shape {(n, T)}, not {_shape(weight)}")
    # the weight rides in front of the return, so that _regress_upload puts it on the common pitch with the factors
    fs, _, r, _ = _regress_upload(cols + ([weight] if weight is not None else []), fwd_return, False)
    w = fs.pop() if weight is not None else None
    ptrs = (C.c_void_p * K)(*[f.data_ptr() for f in fs]) if r.numel() else None
    dev = r.device
    b = _batch(r)
    gp, gs = (None, 0) if ind is None else _codes_on_pitch(ind, b, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    coef, t, p = (torch.empty((K + G, T), **f64) for _ in range(3))
    r2 = torch.empty((2, T), **f64)
    nobs, gt = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(2))
    res = torch.empty_strided((n, T), (b.stride, 1), **f64) if resid else None
    summ = torch.empty((K + G, REGRESS_SUMMARY_COLS), **f64) if summary else None
    _call("pq_xsec_regress_wls", dev, b, ptrs, K, r, w, gp, gs, G, coef, t, p, r2, nobs, gt, res, summ)
    out = {"coef": coef, "t_stat": t, "p_value": p, "r_squared": r2[0], "r_squared_within": r2[1], "n": nobs, "n_industries": gt}
    if summ is not None:
        if T == 0:      # no day: nothing was launched
            summ.copy_(torch.tensor([[0.0] + [float("nan")] * 4] * (K + G), dtype=torch.float64))
        out["summary"] = summ
    if res is not None:
        out["resid"] = res
    return out


def ts_regress(factors, returns):
    """D-17: per-symbol time-series OLS of returns [N, T] on K factors, each [N, T] or a [T] series shared by every symbol (a list, or a
    [K, N, T] array), with an intercept -> dict of device tensors: coef / t_stat / p_value [N, K + 1] (column K = the intercept),
    r_squared [N], n_obs [N] (int32)"""
    cols, (n, T) = _regress_args(factors, returns, True)
    K = len(cols)

    def make(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        return [torch.empty((n, K + 1), **f64), torch.empty((n, K + 1), **f64), torch.empty((n, K + 1), **f64), torch.empty(n, **f64),
                torch.empty(n, dtype=torch.int32, device=dev)]
    coef, t, p, r2, nobs = _regress_call("pq_ts_regress", cols, returns, True, make, lambda mask: (mask,))
    return {"coef": coef, "t_stat": t, "p_value": p, "r_squared": r2, "n_obs": nobs}


def corr_t_test(corr, n_valid):
    """D-17: t-test of per-day correlations (IC or Rank-IC) -> (t_stat [T], p_value [T]) device tensors: t = corr sqrt((n - 2) /
    (1 - corr^2)), two-sided p on n - 2 degrees of freedom; NULL where corr is NaN, n < 3 or corr^2 == 1"""
    c = _to_device(corr)[0].contiguous().reshape(-1)
    nv = n_valid.to(device=c.device, dtype=torch.int32) if isinstance(n_valid, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(n_valid), dtype=np.int32)).to(c.device)
    nv = nv.contiguous().reshape(-1)
    if nv.numel() != c.numel():
        raise ValueError(f"n_valid must have one count per correlation: {nv.numel()} vs {c.numel()}")
    t, p = torch.empty_like(c), torch.empty_like(c)
    _call("pq_corr_t_test", c.device, c, nv, c.numel(), t, p)
    return t, p


LINEAR_TILE = 4096            # PQ_LINEAR_TILE: logical rows per workgroup tile of pq_linear's sums
LINEAR_STAGE2 = 256           # PQ_LINEAR_STAGE2: tile partials per step of its second stage


def linear(xs, y, outputs: bool = True):
    """D-24: one pooled OLS y = a + sum_j b_j x_j over all rows of the columns.  xs: K columns (a list, or one [K, ...] array), each [M]
    or [N, T] in the shape of y -> dict of device tensors: coef / t_stat / p_value [K + 1] (slopes first, the intercept last),
    r_squared and n (int64) 0-dim, and with outputs=True pred (wherever every x is valid) and resid (on the members) in the shape of y"""
    ys = _shape(y)
    if len(ys) not in (1, 2):
        raise ValueError(f"y must be [M] or [N, T], not {ys}")
    cols = _columns(xs, "the number of regressors", 1, REGRESS_MAX_K, len(ys) + 1,
                    "xs must be a list of columns shaped like y or one [K, ...] array")
    for j, c in enumerate(cols):
        if _shape(c) != ys:
            raise ValueError(f"x column {j} must have shape {ys}, not {_shape(c)}")
    K = len(cols)
    mats = [_to_device(c)[0] for c in cols] + [_to_device(y)[0]]
    if mats[-1].numel():          # (an empty column has no layout to agree on, and no pointer is passed)
        mats = _same_layout(mats)
    r = mats[-1]
    dev = r.device
    b = _batch(r)
    ptrs = (C.c_void_p * K)(*[m.data_ptr() for m in mats[:-1]]) if r.numel() else None
    f64 = dict(dtype=torch.float64, device=dev)
    coef, t, p = (torch.empty(K + 1, **f64) for _ in range(3))
    r2, nobs = torch.empty((), **f64), torch.empty((), dtype=torch.int64, device=dev)
    cols_out = [torch.empty_strided(tuple(r.shape), (b.stride, 1), **f64) for _ in range(2)] if outputs else [None, None]
    _call("pq_linear", dev, b, ptrs, K, r, coef, t, p, r2, nobs, *cols_out)
    out = {"coef": coef, "t_stat": t, "p_value": p, "r_squared": r2, "n": nobs}
    if outputs:
        out["pred"], out["resid"] = (o[0] if len(ys) == 1 else o for o in cols_out)
    return out


ORTH_MODES = {"orthogonalize": 0, "neutralize": 1}


def _orth_args(factors, mode):
    """argument checks of factor_orthogonalize that need no device: mode 0 / 1, factors a list / tuple of 2..8 [N, T] arrays of one
    shape or one [K, N, T] array -> (list of factor columns, (N, T))"""
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 (orthogonalize) or 1 (neutralize), not {mode!r}")
    cols = _columns(factors, "the number of factors", 2, REGRESS_MAX_K, 3, "factors must be a list of [N, T] arrays or one [K, N, T] array")
    s0 = _shape(cols[0])
    if len(s0) != 2:
        raise ValueError(f"factor 0 must be [N, T], not {s0}")
    _regress_args(cols, cols[0], False)
    return cols, s0


def factor_orthogonalize(factors, mode: int = 0, out=None, keep_first: bool = False):
    """D-19: per-day residuals of factors 1 .. K-1 (factors: a list of K [N, T] arrays or one [K, N, T] array, 2 <= K <= 8) over the
    day's joint sample: mode 0 (orthogonalize) the residual of factor k on factors 0 .. k-1, mode 1 (neutralize) on factor 0 alone,
    each with an intercept, NULL outside the sample and where the regression has no solution -> device tensor [K - 1, N, T].
    out: K - 1 device float64 [N, T] tensors on the inputs' row pitch to write instead (out[j] may be factor j + 1 itself), returned
    as given.  keep_first (mode 0, out None): -> [K, N, T] with row 0 a copy of factor 0 and rows 1 .. the residuals."""
    cols, (n, T) = _orth_args(factors, mode)
    K = len(cols)
    if keep_first and (mode != 0 or out is not None):
        raise ValueError("keep_first is for mode 0 without out")
    if n == 0 or T == 0:    # no cell: nothing is uploaded or launched
        if out is not None:
            return list(out)
        _require_gpu()
        c0 = cols[0]
        dev = c0.device if isinstance(c0, torch.Tensor) and c0.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return torch.empty((K - 1 + (1 if keep_first else 0), n, T), dtype=torch.float64, device=dev)
    mats = _same_layout([_to_device(c)[0] for c in cols])
    dev = mats[0].device
    b = _batch(mats[0])
    if out is None:
        lead = 1 if keep_first else 0
        buf = torch.empty((K - 1 + lead, n, b.stride), dtype=torch.float64, device=dev)[:, :, :T]
        if keep_first:
            buf[0].copy_(mats[0])
        res, outs = buf, [buf[lead + j] for j in range(K - 1)]
    else:
        res = outs = list(out)
        if len(outs) != K - 1:
            raise ValueError(f"out must hold {K - 1} tensors, not {len(outs)}")
        for j, o in enumerate(outs):
            if not (isinstance(o, torch.Tensor) and o.device == dev and o.dtype == torch.float64 and tuple(o.shape) == (n, T)
                    and (T <= 1 or o.stride(1) == 1) and (n <= 1 or o.stride(0) == b.stride)):
                raise ValueError(f"out[{j}] must be a float64 [N, T] tensor on {dev} with row pitch {b.stride}")
    fp = (C.c_void_p * K)(*[m.data_ptr() for m in mats])
    op = (C.c_void_p * (K - 1))(*[o.data_ptr() for o in outs])
    _call("pq_factor_orthogonalize", dev, b, fp, K, int(mode), op)
    return res


IC_DECAY_MAX_LAG = 256    # PQ_IC_DECAY_MAX_LAG
IC_SUMMARY_COLS = 5       # PQ_IC_SUMMARY_COLS: n_days, mean, std, t_stat, p_value


def _ic_pair_args(factor, fwd_return, method):
    """argument checks of the D-18 calls that need no device -> (n, T)"""
    if method not in (0, 1):
        raise ValueError(f"method must be 0 (Pearson IC) or 1 (Spearman Rank-IC), not {method!r}")
    fs, rs = _shape(factor), _shape(fwd_return)
    if len(rs) != 2 or fs != rs:
        raise ValueError(f"factor and fwd_return must both be [N, T] of one shape, not {fs} and {rs}")
    return rs


def _ic_rows(fn_name, factor, fwd_return, V, args):
    """uploads factor / fwd_return onto one row pitch and runs a D-18 call that writes ic / n_valid [V, T] and summary [V, 5]"""
    (f, r), b = _xsec_inputs([factor, fwd_return])
    dev = f.device
    T = f.shape[1]
    ic = torch.empty((V, T), dtype=torch.float64, device=dev)
    nv = torch.empty((V, T), dtype=torch.int32, device=dev)
    summ = torch.empty((V, IC_SUMMARY_COLS), dtype=torch.float64, device=dev)
    _call(fn_name, dev, b, f, r, *args(b, dev), ic, nv, summ)
    return {"ic": ic, "n_valid": nv, "summary": summ}


def ic_decay(factor, fwd_return, max_lag: int = 10, method: int = 0):
    """D-18: IC of the factor of day t against the return of day t + l - 1, l = 1 .. max_lag (1 <= max_lag <= 256) -> dict of device
    tensors: ic / n_valid [max_lag, T] (NULL / 0 for t > T - l) and summary [max_lag, 5] (n_days, mean, std, t_stat, p_value over the
    non-null days, D-17's Fama-MacBeth rules).  method 0 Pearson IC, 1 Spearman Rank-IC"""
    _ic_pair_args(factor, fwd_return, method)
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 1 <= max_lag <= IC_DECAY_MAX_LAG:
        raise ValueError(f"max_lag must be an integer in 1..{IC_DECAY_MAX_LAG}, not {max_lag!r}")
    L = int(max_lag)
    return _ic_rows("pq_ic_decay", factor, fwd_return, L, lambda b, dev: (int(method), L))


def _group_codes(group, n, T):
    """argument checks of ic_subgroup that need no device: integer codes [N] or [N, T] (negative = unclassified) -> (codes, G)"""
    g = _int_codes(group, "group")
    if tuple(g.shape) not in ((n,), (n, T)):
        raise ValueError(f"group must be [N] or [N, T] with N = {n}, T = {T}, not {tuple(g.shape)}")
    return g, _n_codes(g, "group", IC_MAX_GROUPS)


def ic_subgroup(factor, fwd_return, group, method: int = 0):
    """D-18: per-day IC within each group: group integer codes [N] or [N, T] (negative = unclassified, G = max code + 1 <= 256) -> dict
    of device tensors: ic / n_valid [G, T] (row g = the day's cross-section restricted to code g) and summary [G, 5] (n_days, mean,
    std, t_stat, p_value).  method 0 Pearson IC, 1 Spearman Rank-IC"""
    n, T = _ic_pair_args(factor, fwd_return, method)
    g, G = _group_codes(group, n, T)
    return _ic_rows("pq_ic_subgroup", factor, fwd_return, G, lambda b, dev: (*_codes_on_pitch(g, b, dev), G, int(method)))


RANK_MODES = {"rank": 0, "pct": 1, "quantile": 2}              # pq_factor_rank's mode codes
NORMALIZE_METHODS = ("zscore", "minmax", "quantile")
BINARY_OPS = {"ratio": 0, "diff": 1, "reldiff": 2}             # pq_factor_binary's op codes


def _build_shapes(names, cols):
    """argument check of the D-20 calls that needs no device: every column is [N, T] of one shape -> (N, T)"""
    s0 = _shape(cols[0])
    if len(s0) != 2:
        raise ValueError(f"{names[0]} must be [N, T], not {s0}")
    for nm, c in zip(names[1:], cols[1:]):
        if _shape(c) != s0:
            raise ValueError(f"{nm} must have the shape of {names[0]} {s0}, not {_shape(c)}")
    return s0


def _build_call(fn_name, cols, make_args):
    """uploads the columns onto one row pitch and runs a D-20 call fn(ctx, batch, *columns, *make_args(batch, device), out) ->
    the device f64 [N, T] output at the inputs' pitch"""
    ts, b = _xsec_inputs(cols)
    dev = ts[0].device
    n, T = ts[0].shape
    out = torch.empty((n, b.stride), dtype=torch.float64, device=dev)
    _call(fn_name, dev, b, *ts, *make_args(b, dev), out if T else None)
    return out[:, :T]


def factor_rank(factor, mode: int = 0, descending: bool = False):
    """D-20: per-day average rank of an [N, T] factor over its non-null finite symbols (-0 ties with +0; ties share the mean of their
    positions) -> device tensor [N, T], NULL outside the day's sample.  mode 0: rank in 1 .. n, 1: rank / n, 2: (rank - 0.5) / n (the
    mid-rank position, ascending only); descending: n + 1 - rank."""
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be 0 (rank), 1 (pct) or 2 (mid-rank position), not {mode!r}")
    if mode == 2 and descending:
        raise ValueError("mode 2 (mid-rank position) is ascending only")
    _build_shapes(("factor",), (factor,))
    return _build_call("pq_factor_rank", [factor], lambda b, dev: (int(mode), 1 if descending else 0))


def factor_normalize(factor, method: str = "zscore"):
    """D-20: per-day normalization of an [N, T] factor over its non-null finite symbols -> device tensor [N, T].  "zscore": D-16's
    standardize (factor_clean(standardize=True) itself); "minmax": (x - min) / (max - min), the day NULL where max == min; "quantile":
    (average rank - 0.5) / n."""
    if method not in NORMALIZE_METHODS:
        raise ValueError(f"method must be one of 'zscore', 'minmax', 'quantile', not {method!r}")
    _build_shapes(("factor",), (factor,))
    if method == "zscore":
        return factor_clean(factor, standardize=True)
    if method == "quantile":
        return factor_rank(factor, RANK_MODES["quantile"])
    return _build_call("pq_factor_minmax", [factor], lambda b, dev: ())


def factor_weighted(factor, weight, group=None):
    """D-20: (factor * weight) / W per day, W the sum of the weights over the day's sample (symbols whose factor and weight are both
    non-null and finite), or with group (integer codes [N] or [N, T], negative = unclassified, at most 256 groups) over the symbol's group
    on that day -> device tensor [N, T], NULL outside the sample and where W == 0."""
    n, T = _build_shapes(("factor", "weight"), (factor, weight))
    g, G = _group_codes(group, n, T) if group is not None else (None, 0)
    return _build_call("pq_factor_weighted", [factor, weight],
                       lambda b, dev: (None, 0, 0) if g is None else (*_codes_on_pitch(g, b, dev), G))


def factor_binary(a, b, op: int = 0):
    """D-20: elementwise op 0: a / b, 1: a - b, 2: (a - b) / |b| on [N, T] columns -> device tensor [N, T]; NULL where either input is
    NULL, otherwise plain IEEE-754 (a zero divisor gives inf or nan)."""
    if op not in (0, 1, 2):
        raise ValueError(f"op must be 0 (a / b), 1 (a - b) or 2 ((a - b) / |b|), not {op!r}")
    _build_shapes(("a", "b"), (a, b))
    return _build_call("pq_factor_binary", [a, b], lambda bb, dev: (int(op),))


ROLLING_OPS = {"mean": 0, "momentum": 1, "volatility": 2, "skewness": 3, "relative_strength": 4}   # pq_factor_rolling's op codes
ROLLING_MIN_WINDOW = {0: 1, 1: 1, 2: 2, 3: 3, 4: 1}            # per op code
ROLLING_MAX_WINDOW = 1024                                      # PQ_FACTOR_ROLLING_MAX_WINDOW


def factor_rolling(x, op: int, window: int, skip: int = 0):
    """D-21: one rolling technical factor along the days of every symbol of an [N, T] column -> device tensor [N, T], NULL where the
    row's sample is incomplete or the result is NaN.  op (ROLLING_OPS) 0: mean of x over the last `window` days, 1: momentum
    (x[t-skip] - x[t-skip-window]) / x[t-skip-window], 2: sample std and 3: population skewness of the last `window` period-1 simple
    returns, 4: relative strength 100 G / (G + L) over the last `window` differences.  1 <= window <= 1024 and at least
    ROLLING_MIN_WINDOW[op]; skip >= 0 is momentum's alone."""
    if isinstance(op, bool) or op not in ROLLING_MIN_WINDOW:
        raise ValueError(f"op must be one of {sorted(ROLLING_OPS.values())} (ROLLING_OPS), not {op!r}")
    for nm, v in (("window", window), ("skip", skip)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{nm} must be an integer, not {v!r}")
    if not ROLLING_MIN_WINDOW[op] <= window <= ROLLING_MAX_WINDOW:
        raise ValueError(f"window must be in {ROLLING_MIN_WINDOW[op]}..{ROLLING_MAX_WINDOW} for op {op}, not {window!r}")
    if skip < 0 or (skip != 0 and op != ROLLING_OPS["momentum"]):
        raise ValueError(f"skip must be >= 0, and 0 except for momentum, not {skip!r}")
    _build_shapes(("factor",), (x,))
    return _build_call("pq_factor_rolling", [x], lambda b, dev: (int(op), int(window), int(skip)))


TS_OPS = {"sum": 0, "std": 1, "zscore": 2, "min": 3, "max": 4, "argmin": 5, "argmax": 6, "rank": 7, "decay_linear": 8, "delay": 9,
          "delta": 10}                                         # pq_factor_ts's op codes
TS_PAIR_OPS = {"cov": 0, "corr": 1}                            # pq_factor_ts_pair's op codes
TS_MIN_WINDOW = {"sum": 1, "std": 2, "zscore": 2, "min": 1, "max": 1, "argmin": 1, "argmax": 1, "rank": 1, "decay_linear": 1, "delay": 1,
                 "delta": 1, "cov": 2, "corr": 2}              # per op name of either table


def _ts_args(table, op, window, mode=0):
    """argument checks of factor_ts / factor_ts_pair that need no device: op a code of `table`, window an integer in the op's range,
    mode 0, or 1 for rank"""
    names = {code: nm for nm, code in table.items()}
    if isinstance(op, bool) or not isinstance(op, (int, np.integer)) or op not in names:
        raise ValueError(f"op must be one of the integer codes {sorted(names)} ({table}), not {op!r}")
    for nm, v in (("window", window), ("mode", mode)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{nm} must be an integer, not {v!r}")
    lo = TS_MIN_WINDOW[names[op]]
    if not lo <= window <= ROLLING_MAX_WINDOW:
        raise ValueError(f"window must be in {lo}..{ROLLING_MAX_WINDOW} for op {op} ({names[op]}), not {window!r}")
    if mode != 0 and not (mode == 1 and op == TS_OPS["rank"] and table is TS_OPS):
        raise ValueError(f"mode must be 0, or 1 (rank / window) for rank alone, not {mode!r}")


def factor_ts(x, op: int, window: int, mode: int = 0):
    """D-29: one time-series operator along the days of every symbol of an [N, T] column -> device tensor [N, T], NULL unless every
    value of the row's window is non-null and finite, and where the result is NaN.  op (TS_OPS) over the last `window` days, oldest to
    newest: sum; std (sample, ddof 1); zscore (today - mean) / std; min; max; argmin / argmax (0-based offset from the window's oldest
    day, ties to the oldest); rank of today's value within the window (average rank in 1 .. window, mode 1: divided by the window);
    decay_linear (weights 1 .. window, the newest day the heaviest); delay x[t - window]; delta x[t] - x[t - window].
    1 <= window <= 1024 and at least TS_MIN_WINDOW[name]; mode is rank's alone."""
    _ts_args(TS_OPS, op, window, mode)
    _build_shapes(("x",), (x,))
    return _build_call("pq_factor_ts", [x], lambda b, dev: (int(op), int(window), int(mode)))


def factor_ts_pair(x, y, op: int, window: int):
    """D-29: the covariance (op 0, ddof 1) or the Pearson correlation (op 1; TS_PAIR_OPS) of two [N, T] columns over the last `window`
    days of every symbol -> device tensor [N, T], NULL unless both columns are non-null and finite on every day of the window, and for
    the correlation where either is constant over it.  2 <= window <= 1024."""
    _ts_args(TS_PAIR_OPS, op, window)
    _build_shapes(("x", "y"), (x, y))
    return _build_call("pq_factor_ts_pair", [x, y], lambda b, dev: (int(op), int(window)))


COMBINE_METHODS = {"ic": 0, "icir": 1, "max_icir": 2}          # pq_factor_combine_weights' method codes (PQ_COMBINE_*)
COMBINE_MAX_LAG = ROLLING_MAX_WINDOW                           # the window's bound holds for the lag


def combine_min_window(method: int, k: int) -> int:
    """the shortest window of a method code for k factors: 1 (ic), 2 (icir), k + 1 (max_icir)"""
    return (1, 2, k + 1)[method]


def _combine_weight_args(k, method, window, lag):
    """argument checks of factor_combine_weights that need no device: k factors, method a code of COMBINE_METHODS, window an integer in
    the method's range, lag an integer in 0..1024"""
    if isinstance(method, bool) or not isinstance(method, (int, np.integer)) or method not in COMBINE_METHODS.values():
        raise ValueError(f"method must be one of the integer codes {sorted(COMBINE_METHODS.values())} ({COMBINE_METHODS}), not {method!r}")
    if not 1 <= k <= REGRESS_MAX_K:
        raise ValueError(f"the number of factors must be in 1..{REGRESS_MAX_K}, not {k}")
    for nm, v in (("window", window), ("lag", lag)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{nm} must be an integer, not {v!r}")
    lo = combine_min_window(int(method), k)
    if not lo <= window <= ROLLING_MAX_WINDOW:
        raise ValueError(f"window must be in {lo}..{ROLLING_MAX_WINDOW} for method {method} and {k} factors, not {window!r}")
    if not 0 <= lag <= COMBINE_MAX_LAG:
        raise ValueError(f"lag must be in 0..{COMBINE_MAX_LAG}, not {lag!r}")


def factor_combine_weights(ic, method: int, window: int, lag: int = 1):
    """D-30: the combination weights of K factors from their IC series.  ic: [K, T] (row k the daily IC of factor k, factor_ic's; a
    [T] series is K = 1), 1 <= K <= 8 -> device tensor [K, T].  The weights of day t come from the `window` days that end at t - lag:
    method (COMBINE_METHODS) 0 ic: the mean IC; 1 icir: mean / sample std; 2 max_icir: C^-1 mean with C the sample covariance of the K
    series.  Day t is NULL in all K rows unless its whole window lies inside the series and holds no NULL IC, and where a std is not
    > 0, C is singular or a weight comes out NaN.  window: 1.. / 2.. / K + 1..1024, lag: 0..1024."""
    s = _shape(ic)
    if len(s) not in (1, 2):
        raise ValueError(f"ic must be [K, T] or [T], not {s}")
    K = 1 if len(s) == 1 else s[0]
    _combine_weight_args(K, method, window, lag)
    if isinstance(ic, torch.Tensor) and ic.is_cuda:         # K dense series, not a batch on a row pitch: no layout to warn about
        t = ic.to(torch.float64).reshape(K, -1).contiguous()
    else:
        t = _to_device(ic)[0].contiguous()
    out = torch.empty_like(t)
    if t.numel():
        _call("pq_factor_combine_weights", t.device, t, K, t.shape[1], int(method), int(window), int(lag), out)
    return out


def _combine_args(factors, weights):
    """argument checks of factor_combine that need no device: factors a list / tuple of 1..8 [N, T] arrays of one shape or one
    [K, N, T] array, weights [K] or [K, T] -> (list of factor columns, (N, T))"""
    cols = _columns(factors, "the number of factors", 1, REGRESS_MAX_K, 3, "factors must be a list of [N, T] arrays or one [K, N, T] array")
    s0 = _shape(cols[0])
    if len(s0) != 2:
        raise ValueError(f"factor 0 must be [N, T], not {s0}")
    _regress_args(cols, cols[0], False)
    if weights is not None and _shape(weights) not in ((len(cols),), (len(cols), s0[1])):
        raise ValueError(f"weights must be [K] or [K, T] with K = {len(cols)}, T = {s0[1]}, not {_shape(weights)}")
    return cols, s0


def combine_weight_rows(weights, K: int, T: int, dev):
    """weights [K] or [K, T] -> the contiguous device f64 [K, T] that pq_factor_combine reads; [K] is broadcast along the days on the
    device"""
    w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float64)))
    w = w.to(device=dev, dtype=torch.float64)
    if w.dim() == 1:
        w = w.reshape(K, 1).expand(K, T)
    return w.contiguous()


def factor_combine(factors, weights, normalize: bool = True):
    """D-30: the composite of K factors (a list of K [N, T] arrays or one [K, N, T] array, 1 <= K <= 8) under per-day weights [K, T]
    (factor_combine_weights'; or [K], the same on every day) -> device tensor [N, T]: sum_k weights[k, t] * factors[k][s, t], with
    normalize divided by sum_k |weights[k, t]|.  NULL unless all K cells are non-null and finite, and where a weight of the day is NULL
    or NaN, where normalize is set and the weights' absolute sum is 0, and where the result is NaN.  The factors are taken as given:
    standardise them first (factor_normalize, factor_clean)."""
    cols, (n, T) = _combine_args(factors, weights)
    K = len(cols)
    if n == 0 or T == 0:    # no cell: nothing is uploaded or launched
        _require_gpu()
        c0 = cols[0]
        dev = c0.device if isinstance(c0, torch.Tensor) and c0.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return torch.empty((n, T), dtype=torch.float64, device=dev)
    mats = _same_layout([_to_device(c)[0] for c in cols])
    dev = mats[0].device
    b = _batch(mats[0])
    w = combine_weight_rows(weights, K, T, dev)
    out = torch.empty((n, b.stride), dtype=torch.float64, device=dev)
    fp = (C.c_void_p * K)(*[m.data_ptr() for m in mats])
    _call("pq_factor_combine", dev, b, fp, K, w, 1 if normalize else 0, out)
    return out[:, :T]


RISK_MAX_SERIES = REGRESS_MAX_K + IC_MAX_GROUPS                # PQ_RISK_MAX_SERIES: the rows of xsec_regress_wls's coef block


def risk_weights(window: int, halflife=None) -> np.ndarray:
    """D-33: the weight vector of a risk window, numpy f64 [window], oldest day first: 0.5 ** ((window - 1 - k) / halflife), so the
    as-of day weighs 1.0 and the day `halflife` days before it 0.5; halflife=None: ones (equal weights)"""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= ROLLING_MAX_WINDOW:
        raise ValueError(f"window must be an integer in 1..{ROLLING_MAX_WINDOW}, not {window!r}")
    if halflife is None:
        return np.ones(int(window), dtype=np.float64)
    hl = float(halflife)
    if not (0.0 < hl < float("inf")):
        raise ValueError(f"halflife must be finite and > 0, not {halflife!r}")
    return 0.5 ** ((int(window) - 1 - np.arange(int(window), dtype=np.float64)) / hl)


def _risk_args(weights, min_periods, unbiased):
    """argument checks of risk_factor_cov / risk_specific_var that need no device -> the weights as a numpy f64 [window] array"""
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if w.ndim != 1:
        raise ValueError(f"weights must be one-dimensional [window], not {w.shape}")
    if not 1 <= w.shape[0] <= ROLLING_MAX_WINDOW:
        raise ValueError(f"the window (the number of weights) must be in 1..{ROLLING_MAX_WINDOW}, not {w.shape[0]}")
    if not np.isfinite(w).all() or (w < 0.0).any() or not (w > 0.0).any():
        raise ValueError("weights must be finite and >= 0, with at least one > 0")
    if isinstance(min_periods, bool) or not isinstance(min_periods, (int, np.integer)):
        raise ValueError(f"min_periods must be an integer, not {min_periods!r}")
    lo = 2 if unbiased else 1
    if not lo <= min_periods <= w.shape[0]:
        raise ValueError(f"min_periods must be in {lo}..{w.shape[0]} (the window){' for the unbiased estimate' if unbiased else ''}, "
                         f"not {min_periods!r}")
    return w


def _risk_days(T, day0, step, count):
    """the as-of days day0, day0 + step, ... of a series of T days -> (day0, step, count); count=None: every one that fits"""
    for nm, v in (("day0", day0), ("step", step)) + ((("count", count),) if count is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{nm} must be an integer, not {v!r}")
    day0, step = int(day0), int(step)
    if day0 < 0 or step < 1:
        raise ValueError(f"the as-of days need day0 >= 0 and step >= 1, not day0 = {day0}, step = {step}")
    fit = 0 if day0 >= T else (T - 1 - day0) // step + 1
    if count is None:
        return day0, step, fit
    if not 0 <= count <= fit:
        raise ValueError(f"count must be in 0..{fit}: the as-of days day0 + d * step must lie inside the {T} days, not {count!r}")
    return day0, step, int(count)


def _risk_windowed(fn_name, x, weights, min_periods, day0, step, count, unbiased, counts, max_series):
    """the common path of risk_factor_cov (max_series given: [D, M, M]) and risk_specific_var ([N, D])"""
    w = _risk_args(weights, min_periods, unbiased)
    s = _shape(x)
    if len(s) not in (1, 2):
        raise ValueError(f"the series must be [M, T] or [T], not {s}")
    M, T = (1, s[0]) if len(s) == 1 else s
    if max_series is not None and M > max_series:
        raise ValueError(f"at most {max_series} series, not {M}")
    day0, step, D = _risk_days(T, day0, step, count)
    t = _to_device(x)[0]
    dev = t.device
    if max_series is not None:
        out = torch.empty((D, M, M), dtype=torch.float64, device=dev)
        n = torch.empty((D, M), dtype=torch.int32, device=dev) if counts else None
        extra = ()
    else:
        out = torch.empty((M, D), dtype=torch.float64, device=dev)
        n = torch.empty((M, D), dtype=torch.int32, device=dev) if counts else None
        extra = (D,)
    if M and D:
        om = torch.from_numpy(w).to(dev)
        _call(fn_name, dev, _batch(t), t, om, len(w), int(min_periods), 1 if unbiased else 0, day0, step, D, out, *extra, n)
    return (out, n) if counts else out


def risk_factor_cov(series, weights, min_periods: int, day0: int = 0, step: int = 1, count=None, unbiased: bool = True,
                    counts: bool = False):
    """D-33: the weighted covariance matrix of M series [M, T] (the factor and industry returns of xsec_regress_wls: its coef block,
    M <= 264) on the as-of days day0, day0 + step, ... (count of them; None: every one inside the T days) -> device tensor [D, M, M],
    with counts=True (cov, n [D, M] int32: the sample size of the diagonal).  weights [window] (risk_weights), oldest day first, the last
    one weighs the as-of day.  Entry [d, j, l] runs over the days of the window on which BOTH series are non-null and finite and the
    weight is > 0 (pairwise-complete): C / (W - W2 / W) with unbiased (reliability weights), C / W otherwise, C the weighted sum of
    products of deviations from the pair's own weighted means; NULL below min_periods such days.  Exactly symmetric.
    The model of as-of day t reads the rows t - window + 1 .. t and nothing later.  xsec_regress_wls regresses the NEXT return, so its
    row t -- and a model "as of t" -- is known one day later: shifting is the caller's (Factor.delay)."""
    return _risk_windowed("pq_risk_factor_cov", series, weights, min_periods, day0, step, count, unbiased, counts, RISK_MAX_SERIES)


def risk_specific_var(x, weights, min_periods: int, day0: int = 0, step: int = 1, count=None, unbiased: bool = True, counts: bool = False):
    """D-33: the weighted variance of every symbol's series x [N, T] (the specific returns: xsec_regress_wls's resid) on the as-of days
    -> device tensor [N, D], with counts=True (var, n [N, D] int32).  risk_factor_cov's diagonal arithmetic, bit for bit: the days of
    the window on which the symbol is non-null and finite and the weight is > 0; NULL below min_periods of them.  The as-of days, the
    weights and the one-day shift of a next-return regression are risk_factor_cov's."""
    return _risk_windowed("pq_risk_specific_var", x, weights, min_periods, day0, step, count, unbiased, counts, None)


def risk_portfolio(holdings, exposures, cov, specific_var, industry=None, day0: int = 0, step: int = 1):
    """D-33: the predicted risk of the holdings [N, T] (weights or values; NULL or 0: not held) on the D as-of days day0 + d * step of
    cov [D, M, M] (risk_factor_cov's) and specific_var [N, D] (risk_specific_var's).  exposures: a list of K [N, T] arrays or one
    [K, N, T] array (0 <= K <= 8; None: K = 0), the factors of the regression; industry int codes [N] or [N, T] as in xsec_regress_wls,
    M = K + G (None: G = 1, row K is the net weight, matching the intercept row).
    -> dict of device tensors: exposure / contribution [M, D] (X = the holdings' exposure to every row, c_j = X_j (cov X)_j, which sum to
    factor_var), factor_var / specific_var / total_var / volatility [D], n_held / n_uncovered [D] (int32).  A day is NULL where nothing
    is held, where a held symbol is uncovered (an exposure that is NULL or not finite, a code outside [0, G), a specific variance that is
    NULL or negative) and where a covariance that the product needs (both exposures != 0) is NULL.  Pairwise-complete covariances need not
    be positive semi-definite: volatility is NULL where total_var < 0."""
    hs = _shape(holdings)
    if len(hs) != 2:
        raise ValueError(f"holdings must be [N, T], not {hs}")
    n, T = hs
    cols = [] if exposures is None else _columns(exposures, "the number of exposures", 0, REGRESS_MAX_K, 3,
                                                 "exposures must be a list of [N, T] arrays or one [K, N, T] array")
    K = len(cols)
    for j, c in enumerate(cols):
        if _shape(c) != hs:
            raise ValueError(f"exposure {j} must have the holdings' shape {hs}, not {_shape(c)}")
    D, M, G, ind, day0, step = _risk_model_args(hs, K, cov, specific_var, industry, day0, step, "holdings")
    mats = _same_layout([_to_device(c)[0] for c in [holdings] + cols])
    h = mats[0]
    dev = h.device
    b = _batch(h)
    f64 = dict(dtype=torch.float64, device=dev)
    expo, contrib = (torch.empty((M, D), **f64) for _ in range(2))
    risk = torch.empty((4, D), **f64)
    cnt = torch.empty((2, D), dtype=torch.int32, device=dev)
    if D:
        cv, sv, svs, gp, gs = _risk_model_dev(cov, specific_var, ind, n, D, b, dev)
        ptrs = (C.c_void_p * max(K, 1))(*[m.data_ptr() for m in mats[1:]]) if n else None
        _call("pq_risk_portfolio", dev, b, h, ptrs, K, gp, gs, G, cv, sv, svs, day0, step, D, expo, contrib, risk, cnt)
    return {"exposure": expo, "contribution": contrib, "factor_var": risk[0], "specific_var": risk[1], "total_var": risk[2],
            "volatility": risk[3], "n_held": cnt[0], "n_uncovered": cnt[1]}


def _risk_model_args(hs, K, cov, specific_var, industry, day0, step, of):
    """argument checks of risk_portfolio / risk_solve that need no device: the model's shapes against the [N, T] = hs of the `of` and
    the K exposures -> (D, M, G, industry as an integer tensor or None, day0, step)"""
    n, T = hs
    cs, vs = _shape(cov), _shape(specific_var)
    if len(cs) != 3 or cs[1] != cs[2]:
        raise ValueError(f"cov must be [D, M, M], not {cs}")
    D, M = cs[0], cs[1]
    G = M - K
    ind = None
    if industry is not None:
        ind = _int_codes(industry, "industry")
        if tuple(ind.shape) not in ((n,), (n, T)):
            raise ValueError(f"industry must be [N] or [N, T] with N = {n}, T = {T}, not {tuple(ind.shape)}")
        if not 1 <= G <= MAX_INDUSTRIES or _n_codes(ind, "industry", MAX_INDUSTRIES) > G:
            raise ValueError(f"cov must be [D, K + G, K + G] with K = {K} exposures and G industries (the codes are < G), not {cs}")
    elif G != 1:
        raise ValueError(f"cov must be [D, K + 1, K + 1] with K = {K} exposures and no industry codes, not {cs}")
    if vs != (n, D):
        raise ValueError(f"specific_var must be [N, D] = {(n, D)}, not {vs}")
    day0, step, fit = _risk_days(T, day0, step, None)
    if D > fit:
        raise ValueError(f"the {D} as-of days of cov do not fit the {T} days of the {of} from day0 = {day0} with step = {step}")
    return D, M, G, ind, day0, step


def _risk_model_dev(cov, specific_var, ind, n, D, b, dev):
    """the model on the device -> (cov contiguous, specific_var with unit inner stride, its row pitch, the codes on the batch's pitch,
    their pitch)"""
    f64 = dict(dtype=torch.float64, device=dev)
    cv = (cov if isinstance(cov, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(cov, dtype=np.float64))))
    cv = cv.to(**f64).contiguous()
    sv = (specific_var if isinstance(specific_var, torch.Tensor)
          else torch.from_numpy(np.ascontiguousarray(np.asarray(specific_var, dtype=np.float64)))).to(**f64)
    if sv.stride(1) != 1 or (n > 1 and sv.stride(0) < D):
        sv = sv.contiguous()
    gp, gs = (None, 0) if ind is None else _codes_on_pitch(ind, b, dev)
    return cv, sv, max(sv.stride(0), D) if n > 1 else D, gp, gs


RISK_SOLVE_MAX_RHS = 4        # PQ_RISK_SOLVE_MAX_RHS
RISK_SOLVE_MAX_M = 128        # PQ_RISK_SOLVE_MAX_M


def risk_solve(rhs, exposures, cov, specific_var, industry=None, day0: int = 0, step: int = 1):
    """D-34: y_r = Sigma^-1 v_r on the D as-of days day0 + d * step under the risk model Sigma = B F B^T + diag(s^2) of cov [D, M, M]
    (risk_factor_cov's) and specific_var [N, D] (risk_specific_var's), for the R right-hand sides of the list rhs at once (1 <= R <= 4;
    an entry is an [N, T] array or None for the vector of ones), and the matrix v_r' Sigma^-1 v_q.  exposures (a list of K [N, T] arrays
    or one [K, N, T] array, 0 <= K <= 8; None: K = 0) and industry are risk_portfolio's, M = K + G <= 128.  Sigma is never built: one
    pass over the symbols, an M x M solve per day and one more pass.
    -> (y [R, N, D], quad [R, R, D], n [2, D] int32: the universe and the uncovered symbols) as device tensors.  The universe of a day:
    every given rhs and every exposure non-null and finite, a code in [0, G) and a specific variance > 0; y is NULL outside it.  A symbol
    whose rhs are valid but that lacks an exposure, an industry or a variance is uncovered: it gets no y, the day goes on.  A day is
    NULL where the universe is empty, where a covariance between two rows that take part is NULL, and where the system is singular."""
    if not isinstance(rhs, (list, tuple)) or not 1 <= len(rhs) <= RISK_SOLVE_MAX_RHS:
        raise ValueError(f"rhs must be a list of 1..{RISK_SOLVE_MAX_RHS} [N, T] arrays (None: the vector of ones)")
    cols = [] if exposures is None else _columns(exposures, "the number of exposures", 0, REGRESS_MAX_K, 3,
                                                 "exposures must be a list of [N, T] arrays or one [K, N, T] array")
    R, K = len(rhs), len(cols)
    given = [v for v in rhs if v is not None]
    if not given and not cols:
        raise ValueError("with every rhs None and no exposure nothing tells the days: pass one rhs as an [N, T] array of ones")
    hs = _shape((given + cols)[0])
    if len(hs) != 2:
        raise ValueError(f"the columns must be [N, T], not {hs}")
    n, T = hs
    for j, v in enumerate(rhs):
        if v is not None and _shape(v) != hs:
            raise ValueError(f"rhs {j} must have the columns' shape {hs}, not {_shape(v)}")
    for j, c in enumerate(cols):
        if _shape(c) != hs:
            raise ValueError(f"exposure {j} must have the columns' shape {hs}, not {_shape(c)}")
    D, M, G, ind, day0, step = _risk_model_args(hs, K, cov, specific_var, industry, day0, step, "columns")
    if M > RISK_SOLVE_MAX_M:
        raise ValueError(f"K + G = {M} rows: risk_solve solves at most {RISK_SOLVE_MAX_M} (the system lives in LDS)")
    mats = _same_layout([_to_device(c)[0] for c in given + cols])
    dev = mats[0].device
    b = _batch(mats[0])
    y = torch.empty((R, n, D), dtype=torch.float64, device=dev)
    if not (D and n):                                           # nothing is launched: every day's universe is empty
        return y, torch.from_numpy(np.full((R, R, D), NULL)).to(dev), torch.zeros((2, D), dtype=torch.int32, device=dev)
    quad = torch.empty((R, R, D), dtype=torch.float64, device=dev)
    cnt = torch.empty((2, D), dtype=torch.int32, device=dev)
    cv, sv, svs, gp, gs = _risk_model_dev(cov, specific_var, ind, n, D, b, dev)
    vp = iter(mats[:len(given)])
    rp = (C.c_void_p * R)(*[None if v is None else next(vp).data_ptr() for v in rhs])
    xp = (C.c_void_p * max(K, 1))(*[m.data_ptr() for m in mats[len(given):]])
    yp = (C.c_void_p * R)(*[y[r].data_ptr() for r in range(R)])
    _call("pq_risk_solve", dev, b, rp, R, xp, K, gp, gs, G, cv, sv, svs, day0, step, D, yp, D, quad, cnt)
    return y, quad, cnt


ATTRIBUTION_TOTALS = ("style", "industry", "specific", "unexplained", "total", "realized")   # the rows of pq_return_attribution's totals_out


def _attribution_bounds(T, periods):
    """periods of return_attribution -> the S + 1 bounds as an int64 numpy array, or None: an int n is numpy.array_split(range(T), n)
    (split_periods), anything else the bounds themselves, strictly ascending in [0, T]"""
    if periods is None:
        return None
    if isinstance(periods, (int, np.integer)) and not isinstance(periods, bool):
        start, end = split_periods(T, periods)
        return np.ascontiguousarray(np.concatenate([start, end[-1:] + 1]).astype(np.int64))
    if isinstance(periods, torch.Tensor):
        periods = periods.detach().cpu().numpy()
    b = np.asarray(periods)
    if b.ndim != 1 or b.size < 2 or b.dtype.kind not in "iu":
        raise ValueError("periods must be an integer number of splits or S + 1 >= 2 integer day bounds")
    b = np.ascontiguousarray(b.astype(np.int64))
    if b[0] < 0 or b[-1] > T or (np.diff(b) <= 0).any():
        raise ValueError(f"the period bounds must be strictly ascending in [0, T] (T = {T})")
    return b


def _attribution_args(holdings, exposures, factor_return, specific_return, industry, next_return, benchmark, periods):
    """argument checks of return_attribution that need no device -> (exposure columns, (N, T), K, G, industry as an integer tensor or
    None, the period bounds or None)"""
    hs = _shape(holdings)
    if len(hs) != 2:
        raise ValueError(f"holdings must be [N, T], not {hs}")
    n, T = hs
    cols = [] if exposures is None else _columns(exposures, "the number of exposures", 0, REGRESS_MAX_K, 3,
                                                 "exposures must be a list of [N, T] arrays or one [K, N, T] array")
    K = len(cols)
    for j, c in enumerate(cols):
        if _shape(c) != hs:
            raise ValueError(f"exposure {j} must have the holdings' shape {hs}, not {_shape(c)}")
    for nm, v in (("specific_return", specific_return), ("next_return", next_return), ("benchmark", benchmark)):
        if v is None and nm == "specific_return":
            raise ValueError("specific_return is needed: pure_factor_return(..., specific_return=True)'s residuals")
        if v is not None and _shape(v) != hs:
            raise ValueError(f"{nm} must have the holdings' shape {hs}, not {_shape(v)}")
    fs = _shape(factor_return)
    if len(fs) != 2 or fs[1] != T:
        raise ValueError(f"factor_return must be [K + G, T] with T = {T}, not {fs}")
    G = fs[0] - K
    ind = None
    if industry is not None:
        ind = _int_codes(industry, "industry")
        if tuple(ind.shape) not in ((n,), (n, T)):
            raise ValueError(f"industry must be [N] or [N, T] with N = {n}, T = {T}, not {tuple(ind.shape)}")
        if not 1 <= G <= MAX_INDUSTRIES or _n_codes(ind, "industry", MAX_INDUSTRIES) > G:
            raise ValueError(f"factor_return must be [K + G, T] with K = {K} exposures and G industries (the codes are < G), not {fs}")
    elif G != 1:
        raise ValueError(f"factor_return must be [K + 1, T] with K = {K} exposures and no industry codes, not {fs}")
    return cols, hs, K, G, ind, _attribution_bounds(T, periods)


def return_attribution(holdings, exposures, factor_return, specific_return, industry=None, next_return=None, benchmark=None, periods=None):
    """D-36: the return attribution of the holdings [N, T] (weights or values; NULL or 0: not held) through the factor model, on every
    day.  exposures: a list of K [N, T] arrays or one [K, N, T] array (0 <= K <= 8; None: K = 0); factor_return [K + G, T], the K style
    rows and then the G industry rows (or the intercept) of xsec_regress_wls's coef; specific_return [N, T], its resid; industry int
    codes [N] or [N, T] (None: G = 1); next_return [N, T] (optional) the return that was regressed; benchmark [N, T] (optional) gives
    P = 3 books -- the portfolio, the benchmark and the active book h - b -- instead of P = 1; periods: an int (numpy.array_split of the
    days) or S + 1 day bounds strictly ascending in [0, T].
    -> dict of device tensors, the book axis first: exposure / contribution [P, M, T] (X_j = sum h x_j over the covered symbols, c_j =
    X_j f_j), style / industry / specific / unexplained / total / realized [P, T], n_held / n_uncovered / n_missing [P, T] (int32),
    summary [P, M + 6, 5] (n_days, mean, std, t_stat, p_value of the M contributions and the six totals over their non-NULL days) and,
    with periods, period_sum [P, M + 6, S], period_days [P, S] (int32) and period_bounds [S + 1] (int64).  A held symbol without an
    exposure, an industry or a specific return is uncovered: its h r goes to `unexplained` where next_return is valid, and it is counted
    missing where not.  A book's day is NULL where nothing is held and where a factor return that a non-zero exposure needs is NULL.  On
    a day without uncovered symbols total equals realized up to rounding.  The definitions are in include/pq_hip.h."""
    cols, (n, T), K, G, ind, bounds = _attribution_args(holdings, exposures, factor_return, specific_return, industry, next_return,
                                                         benchmark, periods)
    M, NS = K + G, K + G + len(ATTRIBUTION_TOTALS)
    P = 1 if benchmark is None else 3
    S = 0 if bounds is None else bounds.size - 1
    planes = [holdings] + ([benchmark] if benchmark is not None else []) + cols + [specific_return] + \
        ([next_return] if next_return is not None else [])
    mats = _same_layout([_to_device(c)[0] for c in planes])
    h = mats[0]
    dev = h.device
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    if n == 0 or T == 0:                                        # nothing is launched: nothing is held on any day
        null = lambda *s: torch.from_numpy(np.full(s, NULL)).to(dev)   # noqa: E731
        expo, contrib, tot = null(P, M, T), null(P, M, T), null(P, 6, T)
        cnt = torch.zeros((3, P, T), **i32)
        summ = null(P, NS, REGRESS_SUMMARY_COLS)
        summ[:, :, 0] = 0.0
        psum, pdays = torch.zeros((P, NS, S), **f64), torch.zeros((P, S), **i32)
    else:
        b = _batch(h)
        it = iter(mats[1:])
        bm = next(it) if benchmark is not None else None
        xs = [next(it) for _ in range(K)]
        u = next(it)
        r = next(it) if next_return is not None else None
        fr = _to_device(factor_return)[0].to(dev)
        if (T > 1 and fr.stride(1) != 1) or (M > 1 and fr.stride(0) < T):
            fr = fr.contiguous()
        frs = fr.stride(0) if M > 1 and fr.stride(0) >= T else T
        gp, gs = (None, 0) if ind is None else _codes_on_pitch(ind, b, dev)
        expo, contrib, tot = torch.empty((P, M, T), **f64), torch.empty((P, M, T), **f64), torch.empty((P, 6, T), **f64)
        cnt = torch.empty((3, P, T), **i32)
        summ = torch.empty((P, NS, REGRESS_SUMMARY_COLS), **f64)
        psum, pdays = (torch.empty((P, NS, S), **f64), torch.empty((P, S), **i32)) if S else (None, None)
        ptrs = (C.c_void_p * max(K, 1))(*[m.data_ptr() for m in xs])
        bp = bounds if S else None                             # a host array: the entry point copies it
        _call("pq_return_attribution", dev, b, h, bm, ptrs, K, gp, gs, G, fr, frs, u, r, bp, S, expo, contrib, tot, cnt, summ, psum, pdays)
    out = {"exposure": expo, "contribution": contrib}
    out.update({nm: tot[:, i] for i, nm in enumerate(ATTRIBUTION_TOTALS)})
    out.update({"n_held": cnt[0], "n_uncovered": cnt[1], "n_missing": cnt[2], "summary": summ})
    if bounds is not None:
        out.update({"period_sum": psum, "period_days": pdays, "period_bounds": torch.from_numpy(bounds).to(dev)})
    return out


ROLLING_REGRESS_MAX_K = 4                                      # PQ_ROLLING_REGRESS_MAX_K
ROLLING_REGRESS_OUTPUTS = ("beta", "alpha", "resid_std", "r_squared", "resid")   # pq_factor_rolling_regress's output pointers, in order


def _rolling_regress_args(y, xs, window, outputs):
    """argument checks of factor_rolling_regress that need no device -> (list of regressor columns, (N, T), tuple of output names)"""
    if isinstance(outputs, str):
        outputs = (outputs,)
    names = tuple(outputs)
    if not names:
        raise ValueError(f"outputs must name at least one of {ROLLING_REGRESS_OUTPUTS}")
    for nm in names:
        if nm not in ROLLING_REGRESS_OUTPUTS:
            raise ValueError(f"outputs must be among {ROLLING_REGRESS_OUTPUTS}, not {nm!r}")
    if len(_shape(y)) != 2:
        raise ValueError(f"y must be [N, T], not {_shape(y)}")
    cols = _columns(xs, "the number of regressors", 1, ROLLING_REGRESS_MAX_K, 3,
                    "xs must be a list of [N, T] or [T] arrays or one [K, N, T] array")
    cols, shape = _regress_args(cols, y, True)
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
        raise ValueError(f"window must be an integer, not {window!r}")
    if not len(cols) + 2 <= window <= ROLLING_MAX_WINDOW:
        raise ValueError(f"window must be in {len(cols) + 2}..{ROLLING_MAX_WINDOW} for {len(cols)} regressors, not {window!r}")
    return cols, shape, names


def factor_rolling_regress(y, xs, window: int, outputs=ROLLING_REGRESS_OUTPUTS):
    """D-28: the OLS y = a + sum_j b_j x_j over the last `window` days of every symbol, one fit per (symbol, day).  y [N, T]; xs: K
    regressors (1 <= K <= 4; a list, or one [K, N, T] array), each [N, T] or a [T] series shared by every symbol (e.g. a market return)
    -> dict of device tensors, only those named in `outputs`: beta [K, N, T], alpha, resid_std (sqrt(sse / (window - K - 1))),
    r_squared (NULL where y is constant over the window) and resid (the window's last day) [N, T].  A row is NULL unless all K + 1
    values are non-null and finite on every day of its window, and where the window is singular.  K + 2 <= window <= 1024."""
    cols, (n, T), names = _rolling_regress_args(y, xs, window, outputs)
    K = len(cols)
    fs, mask, r, ptrs = _regress_upload(cols, y, True)
    b = _batch(r)
    f64 = dict(dtype=torch.float64, device=r.device)      # the outputs sit on the inputs' row pitch
    outs = [(torch.empty((K, n, b.stride) if nm == "beta" else (n, b.stride), **f64) if nm in names else None)
            for nm in ROLLING_REGRESS_OUTPUTS]
    _call("pq_factor_rolling_regress", r.device, b, ptrs, K, mask, r, int(window), *outs)
    return {nm: o[..., :T] for nm, o in zip(ROLLING_REGRESS_OUTPUTS, outs) if o is not None}


def split_periods(T: int, n_splits: int):
    """numpy.array_split(range(T), n_splits) as inclusive (start, end) day indices -> two int64 numpy arrays; 1 <= n_splits <= T"""
    if isinstance(n_splits, bool) or not isinstance(n_splits, (int, np.integer)) or not 1 <= n_splits <= T:
        raise ValueError(f"n_splits must be an integer in 1..T (T = {T}), not {n_splits!r}")
    P = int(n_splits)
    q, r = divmod(int(T), P)
    p = np.arange(P, dtype=np.int64)
    start = p * q + np.minimum(p, r)
    return start, start + q + (p < r) - 1


def series_split_summary(x, n_splits: int):
    """D-18: summary rows of a series x [T] over numpy.array_split(range(T), n_splits) -> device tensor [n_splits, 5] (n_days, mean, std,
    t_stat, p_value over each period's non-null days)"""
    T = int(np.prod(_shape(x))) if len(_shape(x)) else 1
    split_periods(T, n_splits)
    t = _to_device(x)[0].contiguous().reshape(-1)
    out = torch.empty((int(n_splits), IC_SUMMARY_COLS), dtype=torch.float64, device=t.device)
    _call("pq_series_split_summary", t.device, t, T, int(n_splits), out)
    return out


def _signal_call(fn_name, cols, *scalars):
    ts = [_to_device(c)[0].contiguous() for c in cols]
    dev = ts[0].device
    n, T = ts[0].shape
    for t in ts:
        if t.shape != (n, T):
            raise ValueError("signal rule inputs must have the same shape")
    buy = torch.zeros((n, T), dtype=torch.uint8, device=dev)
    sell = torch.zeros((n, T), dtype=torch.uint8, device=dev)
    if n * T:
        _call(fn_name, dev, _batch(ts[0], dense=True), *ts, *scalars, buy, sell)
    return buy, sell


def cross_signals(a, b):
    """D-11: buy = a crosses above b, sell = a crosses below b -> (buy, sell) uint8 device tensors [N, T]"""
    return _signal_call("pq_cross_signals", [a, b])


def band_signals(x, lower: float, upper: float):
    """D-11: buy = x comes back up through `lower`, sell = x comes back down through `upper`"""
    return _signal_call("pq_band_signals", [x], float(lower), float(upper))


def channel_signals(price, lo, hi, mode: int):
    """D-11: mode 0 = reversion at the bands, mode 1 = breakout of the previous bar's channel"""
    return _signal_call("pq_channel_signals", [price, lo, hi], int(mode))


def _dev2(x, dtype=torch.float64):
    return _to_device(x, dtype)[0].contiguous()


def _rule(fn_name, shape_like, args, outs, same=()):
    """one of the strategy rule kernels (csrc/strategy.hip): args = the arguments between the batch and the outputs, outs = output
    tensors (returned); `same`: the other tensor arguments, which must have shape_like's shape (the kernel indexes all of them with
    one batch)"""
    for t in same:
        if t is not None and tuple(t.shape) != tuple(shape_like.shape):
            raise PqError(f"{fn_name}: input shapes differ: {tuple(t.shape)} vs {tuple(shape_like.shape)}")
    if shape_like.numel():
        _call(fn_name, shape_like.device, _batch(shape_like, dense=True), *args, *outs)
    return outs


def gate_signals(buy, sell, a, mode: int, k0: float = 0.0, k1: float = 0.0, c=None):
    """pq_gate_signals: filter existing signals by a comparison on column `a` (see include/pq_hip.h for the modes)"""
    a_, bu, se = _dev2(a), _dev2(buy, torch.uint8), _dev2(sell, torch.uint8)
    c_ = _dev2(c) if c is not None else None
    outs = [torch.empty_like(bu), torch.empty_like(se)]
    return tuple(_rule("pq_gate_signals", a_, [a_, c_, int(mode), float(k0), float(k1), bu, se], outs, same=(bu, se, c_)))


def zscore(price, upper, mid):
    p, u, m = _dev2(price), _dev2(upper), _dev2(mid)
    return _rule("pq_zscore", p, [p, u, m], [torch.empty_like(p)], same=(u, m))[0]


def scale_band(base, f_lo: float, f_hi: float):
    b_ = _dev2(base)
    return tuple(_rule("pq_scale_band", b_, [b_, float(f_lo), float(f_hi)], [torch.empty_like(b_), torch.empty_like(b_)]))


def _u8_pair(like):
    return [torch.zeros(like.shape, dtype=torch.uint8, device=like.device), torch.zeros(like.shape, dtype=torch.uint8, device=like.device)]


def volume_surge_signals(volume, avg_volume, close, multiplier: float):
    v, sv, c = _dev2(volume), _dev2(avg_volume), _dev2(close)
    return tuple(_rule("pq_volume_surge_signals", v, [v, sv, c, float(multiplier)], _u8_pair(v), same=(sv, c)))


def gap_signals(open, high, low, f_up: float, f_dn: float):
    o, h, l = _dev2(open), _dev2(high), _dev2(low)
    return tuple(_rule("pq_gap_signals", o, [o, h, l, float(f_up), float(f_dn)], _u8_pair(o), same=(h, l)))


def pattern_any_signals(bullish, bearish):
    """bullish / bearish: lists of int32 recogniser columns (device) -> (buy, sell)"""
    bu = [_dev2(t, torch.int32) for t in bullish]
    be = [_dev2(t, torch.int32) for t in bearish]
    like = (bu + be)[0]
    pb = (C.c_void_p * max(len(bu), 1))(*[t.data_ptr() for t in bu])
    ps = (C.c_void_p * max(len(be), 1))(*[t.data_ptr() for t in be])
    return tuple(_rule("pq_pattern_any_signals", like, [pb, len(bu), ps, len(be)], _u8_pair(like), same=bu + be))


def ma_stack_signals(mas):
    ms = [_dev2(t) for t in mas]
    ptrs = (C.c_void_p * len(ms))(*[t.data_ptr() for t in ms])
    return tuple(_rule("pq_ma_stack_signals", ms[0], [ptrs, len(ms)], _u8_pair(ms[0]), same=ms))


def backtest_leveraged(price, buy, sell, benchmark=None, max_trades: int = 64, **kw):
    """README `Backtest` engine (decision D-10): price/buy/sell [N, T], benchmark [T] or None.
    -> dict of device tensors: cash, stock_value, total_value [N,T]; trade_count [N]; trades {field: [N,max_trades]};
    summary [N,8]"""
    from ._spec import LEV_DEFAULTS, TRADE_FIELDS
    prm = LevParams(**{**LEV_DEFAULTS, **kw})
    p, _, _ = _to_device(price)
    bu, _, _ = _to_device(buy, torch.uint8)
    se, _, _ = _to_device(sell, torch.uint8)
    p = p.contiguous(); bu = bu.contiguous(); se = se.contiguous()
    dev = p.device
    n, T = p.shape
    bm = None
    if benchmark is not None:
        bm = _to_device(benchmark)[0].contiguous().reshape(-1)
        if bm.numel() != T:
            raise ValueError("benchmark must be one series with as many rows as the prices")
    mk = lambda: torch.empty((n, T), dtype=torch.float64, device=dev)
    cash, sv, tv = mk(), mk(), mk()
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    tr = {k: torch.zeros((n, max_trades), dtype=torch.int32 if k in ("entry_day", "exit_day", "reason") else torch.float64, device=dev)
          for k in TRADE_FIELDS}
    summ = torch.empty((n, 8), dtype=torch.float64, device=dev)
    if n * T:
        _call("pq_backtest_leveraged", dev, _batch(p, dense=True), p, bu, se, bm, prm, cash, sv, tv, max_trades, cnt,
              *[tr[k] for k in ("entry_day", "exit_day", "entry_price", "exit_price", "quantity", "pnl", "pnl_pct", "reason")], summ)
    return dict(cash=cash, stock_value=sv, total_value=tv, trade_count=cnt, trades=tr, summary=summ)


def portfolio_metrics(total_value, initial_total: float, benchmark=None):
    """get_performance_metrics: total_value [N, T] -> [T, 10] device tensor (columns: _spec.PORTFOLIO_COLS + reserved)"""
    tv, _, _ = _to_device(total_value)
    tv = tv.contiguous()
    bm = _to_device(benchmark)[0].contiguous().reshape(-1) if benchmark is not None else None
    out = torch.zeros((tv.shape[1], 10), dtype=torch.float64, device=tv.device)
    if tv.numel():
        _call("pq_portfolio_metrics", tv.device, _batch(tv, dense=True), tv, float(initial_total), bm, out)
    return out


def _rp_meta(x, what, ndim):
    """shape and dtype kind of an array-like, without moving it to the device"""
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
    if len(shape) != ndim:
        raise ValueError(f"{what} must have {ndim} dimension{'s' if ndim > 1 else ''}, got shape {shape}")
    dt = x.dtype if isinstance(x, torch.Tensor) else np.asarray(x).dtype
    if isinstance(dt, torch.dtype):
        numeric = dt.is_floating_point or dt in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8, torch.bool)
    else:
        numeric = dt.kind in "fiub"
    if not numeric:
        raise ValueError(f"{what} must be numeric, got {dt}")
    return shape


def _rp_numel(x, what):
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
    return int(np.prod(_rp_meta(x, what, len(shape))))


def _rp_dev(x, dtype, dev=None):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(device=dev if dev is not None else "cuda", dtype=dtype)


def backtest_report(total_value, initial_capital: float, benchmark=None, trades=None, trade_count=None, max_trades: int = 0, **lev_params):
    """The statistics report of `Backtest` (decision D-22): total_value [N, T], benchmark [T] or None, trades = {field: [N, max_trades]}
    with the fields _spec.REPORT_TRADE_FIELDS (further fields are ignored) and trade_count [N], as backtest_leveraged returns them;
    max_trades = 0 takes the records' width.  lev_params: the engine's commission_rate / min_commission (and the rest of its parameters).
    -> device [N, 48] f64, columns _spec.REPORT_COLS; a missing value is NULL.  Every check raises ValueError before any device work."""
    from ._spec import LEV_DEFAULTS, REPORT_COLS, REPORT_TRADE_FIELDS
    n, T = _rp_meta(total_value, "total_value", 2)
    if T < 1:
        raise ValueError("total_value needs at least one day")
    c0 = float(initial_capital)
    if not (c0 > 0.0 and np.isfinite(c0)):
        raise ValueError("initial_capital must be positive and finite")
    unknown = set(lev_params) - set(LEV_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown parameters {sorted(unknown)}")
    if benchmark is not None and _rp_numel(benchmark, "benchmark") != T:
        raise ValueError("benchmark must be one series with as many rows as total_value")
    width = 0
    if trades is not None:
        if trade_count is None:
            raise ValueError("trades need trade_count")
        missing = [k for k in REPORT_TRADE_FIELDS if k not in trades]
        if missing:
            raise ValueError(f"trades lack the fields {missing}")
        shapes = {k: _rp_meta(trades[k], f"trades[{k!r}]", 2) for k in REPORT_TRADE_FIELDS}
        if len(set(shapes.values())) != 1:
            raise ValueError(f"the trade arrays must have one shape, got {shapes}")
        rows, width = shapes["pnl"]
        if rows != n:
            raise ValueError(f"the trade arrays have {rows} rows for {n} symbols")
        if int(max_trades) not in (0, width):
            raise ValueError(f"max_trades = {max_trades} but the trade arrays are {width} wide")
    elif int(max_trades) < 0:
        raise ValueError("max_trades < 0")
    if trade_count is not None and _rp_meta(trade_count, "trade_count", 1) != (n,):
        raise ValueError(f"trade_count must have one entry per symbol ({n})")
    _require_gpu()
    prm = LevParams(**{**LEV_DEFAULTS, **lev_params})
    tv = _rp_dev(total_value, torch.float64)
    if tv.stride(1) != 1 or tv.stride(0) < T:
        tv = tv.contiguous()
    dev = tv.device
    out = torch.empty((n, len(REPORT_COLS)), dtype=torch.float64, device=dev)
    if n == 0:
        return out
    bm = _rp_dev(benchmark, torch.float64, dev).reshape(-1).contiguous() if benchmark is not None else None
    cnt = _rp_dev(trade_count, torch.int32, dev).contiguous() if trade_count is not None else None
    rec = [None] * len(REPORT_TRADE_FIELDS)
    if trades is not None and width > 0:
        rec = [_rp_dev(trades[k], torch.int32 if k in ("entry_day", "exit_day", "reason") else torch.float64, dev).contiguous()
               for k in REPORT_TRADE_FIELDS]
    _call("pq_backtest_report", dev, _batch(tv, lone_dense=True), tv, c0, bm, prm, int(width), cnt, *rec, out)
    return out


def report_portfolio(report, curve_row, initial_capital: float):
    """The portfolio row of the report (D-22): report = backtest_report's [N, 48] rows, curve_row = the [48] report row of the
    portfolio_value series on N times the capital, initial_capital = one symbol's -> device [48] f64"""
    from ._spec import REPORT_COLS
    ncol = len(REPORT_COLS)
    shape = _rp_meta(report, "report", 2)
    if shape[1] != ncol or shape[0] < 1:
        raise ValueError(f"report must be [N >= 1, {ncol}], got {shape}")
    if _rp_numel(curve_row, "curve_row") != ncol:
        raise ValueError(f"curve_row must hold {ncol} values")
    c0 = float(initial_capital)
    if not (c0 > 0.0 and np.isfinite(c0)):
        raise ValueError("initial_capital must be positive and finite")
    _require_gpu()
    rep = _rp_dev(report, torch.float64).contiguous()
    dev = rep.device
    cur = _rp_dev(curve_row, torch.float64, dev).reshape(-1).contiguous()
    out = torch.zeros(ncol, dtype=torch.float64, device=dev)
    _call("pq_report_portfolio", dev, shape[0], rep, cur, c0, out)
    return out


def backtest_sequential(period_offsets, asset, quantity, price, n_assets: int, benchmark=None, params=None, out=None):
    """SequentialBacktester's engine on order tapes (decision D-23): period_offsets [B, T + 1] (or [T + 1]) int64, absolute indices
    into the order arrays asset int32 / quantity / price [n_orders] (quantity signed); two tapes may point at the same orders.
    benchmark: [T] or None.  params: None (the defaults), one dict for every tape or a list of B dicts over _spec.SEQ_DEFAULTS.
    out: optional dict of preallocated device tensors under the result's names.
    -> dict of device tensors: equity, cash [B, T]; position [B, A]; counts [B, 2] int64 (trades, wins); summary [B, 8].
    T = 0 launches nothing.  Shape checks raise ValueError before any device work; n_assets above 6144 (PQ_SEQ_MAX_ASSETS) is the
    library's argument error (PqError)."""
    from ._spec import SEQ_DEFAULTS
    shape = tuple(period_offsets.shape) if isinstance(period_offsets, torch.Tensor) else np.shape(period_offsets)
    if len(shape) == 1:
        shape = (1,) + shape
    if len(shape) != 2 or shape[1] < 1:
        raise ValueError(f"period_offsets must be [B, T + 1], got shape {shape}")
    B, T = int(shape[0]), int(shape[1]) - 1
    n_orders = _rp_numel(asset, "asset")
    if _rp_numel(quantity, "quantity") != n_orders or _rp_numel(price, "price") != n_orders:
        raise ValueError("asset, quantity and price must have one entry per order")
    A = int(n_assets)
    if A < 0:
        raise ValueError("n_assets < 0")
    if benchmark is not None and _rp_numel(benchmark, "benchmark") != T:
        raise ValueError("benchmark must be one series with one row per period")
    plist = [{}] if params is None else ([params] if isinstance(params, dict) else list(params))
    if len(plist) not in (1, B):
        raise ValueError(f"params must hold 1 or {B} entries, got {len(plist)}")
    for d in plist:
        unknown = set(d) - set(SEQ_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown parameters {sorted(unknown)}")
    prm = (SeqParams * len(plist))(*[SeqParams(**{**SEQ_DEFAULTS, **{k: float(v) for k, v in d.items()}}) for d in plist])
    _require_gpu()
    off = _rp_dev(period_offsets, torch.int64).reshape(B, T + 1).contiguous()
    dev = off.device
    a = _rp_dev(asset, torch.int32, dev).reshape(-1).contiguous()
    q = _rp_dev(quantity, torch.float64, dev).reshape(-1).contiguous()
    px = _rp_dev(price, torch.float64, dev).reshape(-1).contiguous()
    bm = _rp_dev(benchmark, torch.float64, dev).reshape(-1).contiguous() if benchmark is not None else None
    spec = dict(equity=((B, T), torch.float64), cash=((B, T), torch.float64), position=((B, A), torch.float64),
                counts=((B, 2), torch.int64), summary=((B, 8), torch.float64))
    r = {}
    for k, (shp, dt) in spec.items():
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.zeros(shp, dtype=dt, device=dev)
        elif tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"out[{k!r}] must be a contiguous {dt} tensor of shape {shp} on {dev}")
        r[k] = t
    if B and T:
        _call("pq_backtest_sequential", dev, B, T, A, off, a, q, px, n_orders, bm, prm, len(plist), *r.values())
    return r


def macd_cross_signals(close, fastperiod=12, slowperiod=26, signalperiod=9):
    p, kind, squeeze = _to_device(close)
    p = p.contiguous()
    bu = torch.empty(tuple(p.shape), dtype=torch.uint8, device=p.device)
    se = torch.empty(tuple(p.shape), dtype=torch.uint8, device=p.device)
    _call("pq_macd_cross_signals", p.device, _batch(p, dense=True), p, fastperiod, slowperiod, signalperiod, bu, se)
    k = kind if kind in (_Kind.TORCH, _Kind.NUMPY) else _Kind.NUMPY
    return _from_device(bu, k, squeeze), _from_device(se, k, squeeze)


# pq_sweep_param (include/pq_hip.h): one parameter set of backtest_sweep -- rule 0: cross(lines[a], lines[b]); 1: band(lines[a], k0, k1)
SWEEP_PARAM_DTYPE = np.dtype([("rule", "<i4"), ("a", "<i4"), ("b", "<i4"), ("_pad", "<i4"), ("k0", "<f8"), ("k1", "<f8")])
SWEEP_MAX_LINES = 512


def SWEEP_ROW_TILE(n_lines: int) -> int:
    """pq_sweep_row_tile: the rows of one LDS tile of the sweep kernel for n_lines lines (0: n_lines is out of range)"""
    return int(_call("pq_sweep_row_tile", None, int(n_lines), checked=False))


def _rule_table(rules, dtype, dtype_name):
    """a `dtype` record array from one, or from a dict of equally long columns under its field names (missing ones are 0)"""
    if isinstance(rules, np.ndarray) and rules.dtype == dtype:
        return np.ascontiguousarray(rules.reshape(-1))
    if not isinstance(rules, dict) or "rule" not in rules or "a" not in rules:
        raise ValueError(f"rules must be a {dtype_name} array or a dict with at least the columns 'rule' and 'a'")
    unknown = set(rules) - (set(dtype.names) - {"_pad"})
    if unknown:
        raise ValueError(f"unknown rule columns {sorted(unknown)}")
    out = np.zeros(len(np.atleast_1d(rules["rule"])), dtype=dtype)
    for k, v in rules.items():
        v = np.atleast_1d(np.asarray(v))
        if v.shape != out.shape:
            raise ValueError(f"rule column {k!r} has shape {v.shape}, expected {out.shape}")
        out[k] = v
    return out


def sweep_params(rules) -> np.ndarray:
    """a SWEEP_PARAM_DTYPE array from one, or from a dict of equally long rule / a / b / k0 / k1 columns (missing ones are 0)"""
    return _rule_table(rules, SWEEP_PARAM_DTYPE, "SWEEP_PARAM_DTYPE")


def sweep_windows(windows) -> np.ndarray:
    """a contiguous int64 [W, 2] table of row ranges [t0, t1) (pq_sweep_window) from any integer array of that shape"""
    w = np.asarray(windows)
    if w.size == 0:
        w = np.zeros((0, 2), dtype=np.int64)
    if w.ndim != 2 or w.shape[1] != 2 or w.dtype.kind not in "iu":
        raise ValueError(f"windows must be an integer [W, 2] array of row ranges [t0, t1), not {w.dtype} {w.shape}")
    return np.ascontiguousarray(w, dtype=np.int64)


def _backtest_sweep(who, entry, tab, price, lines, benchmark, out, offsets, kw, windows=None):
    """pq_backtest_sweep and pq_backtest_sweep_rules take the same arguments: `entry` is the one to call, `tab` its 32-byte table.
    windows (D-26): a sweep_windows table, which goes to pq_backtest_sweep_windows instead (either table is the same 32 bytes)"""
    prm = BtParams(**{**BT_DEFAULTS, **kw})
    cols = _columns(lines, f"{who}: the number of lines", 1, SWEEP_MAX_LINES, exc=PqError)
    mats = _same_layout([_to_device(price)[0]] + [_to_device(c)[0] for c in cols])
    p = mats[0]
    dev = p.device
    n, T = p.shape
    b = _batch(p)
    if offsets is not None:
        b, _off = ragged_batch(offsets, dev)
    P = len(tab)
    bm, bstride = None, 0
    if benchmark is not None:
        bm = _to_device(benchmark)[0]
        if bm.shape == (1, T):
            bm = bm.contiguous()
        elif bm.shape == (n, T):
            bstride = bm.stride(0)
        else:
            raise PqError(f"{who}: `benchmark` has shape {tuple(bm.shape)}, expected {(T,)} or {(n, T)}")
    win = None if windows is None else sweep_windows(windows)
    shape = (n, P, 8) if win is None else (len(win), n, P, 8)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float64 tensor of shape {shape} on {dev}")
    if n and P and (win is None or len(win)):
        dtab = torch.from_numpy(tab.view(np.uint8).reshape(P, tab.dtype.itemsize)).to(dev)
        ptrs = (C.c_void_p * len(cols))(*[m.data_ptr() for m in mats[1:]])
        head, tail = (b, p, ptrs, len(cols), dtab, P), (bm, bstride, prm, out)
        if win is None:
            _call(entry, dev, *head, *tail)
        else:
            _call("pq_backtest_sweep_windows", dev, *head, win, len(win), *tail)
    return out.permute(1, 0, 2) if win is None else out.permute(0, 2, 1, 3)


def backtest_sweep(price, lines, params, benchmark=None, out=None, offsets=None, windows=None, **kw):
    """D-25: every parameter set of `params` (sweep_params) over every symbol in ONE launch -> device summary [P, N, 8], a permuted
    view of the kernel's [N, P, 8].  price [N, T]; lines: a list of [N, T] candidate indicator columns or one [L, N, T] array;
    benchmark: None, one [T] series shared by all symbols, or [N, T]; out: a contiguous device [N, P, 8] float64 tensor to write into;
    offsets: ragged groups of long columns (see call()) are not supported by the sweep and raise.
    windows (D-26): an integer [W, 2] array of row ranges [t0, t1) -> device [W, P, N, 8], a permuted view of the kernel's
    [W, N, P, 8] (the shape of `out`), still one launch; entry w is bit for bit the sweep of the rows [t0, t1) alone.  The windowed
    entry point knows all seven rules, so a rule beyond 1 is refused here, in Python, with a PqError whose text differs from the one
    pq_backtest_sweep itself gives for the same mistake without `windows`."""
    tab = sweep_params(params)
    if windows is not None and len(tab) and not (tab["rule"] <= 1).all():      # pq_backtest_sweep_windows knows all seven rules
        raise PqError("backtest_sweep: unknown rule (the rules are 0 and 1; backtest_sweep_rules has the others)")
    return _backtest_sweep("backtest_sweep", "pq_backtest_sweep", tab, price, lines, benchmark, out, offsets, kw, windows)


# pq_sweep_rule (include/pq_hip.h): pq_sweep_param with a third column index c (-1: the price) -- the rules of backtest_sweep_rules:
# 0 cross, 1 band, 2 channel (reversion), 3 breakout, 4 channel around lines[a] * k0 / k1, 5 cross in zones, 6 cross with strength
SWEEP_RULE_DTYPE = np.dtype([("rule", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("k0", "<f8"), ("k1", "<f8")])
(SWEEP_RULE_CROSS, SWEEP_RULE_BAND, SWEEP_RULE_CHANNEL, SWEEP_RULE_BREAKOUT, SWEEP_RULE_SCALED_CHANNEL, SWEEP_RULE_CROSS_ZONES,
 SWEEP_RULE_CROSS_STRENGTH) = range(7)


def sweep_rules(rules) -> np.ndarray:
    """a SWEEP_RULE_DTYPE array from one, or from a dict of equally long rule / a / b / c / k0 / k1 columns (missing ones are 0)"""
    return _rule_table(rules, SWEEP_RULE_DTYPE, "SWEEP_RULE_DTYPE")


def backtest_sweep_rules(price, lines, rules, benchmark=None, out=None, windows=None, **kw):
    """backtest_sweep with the seven rules of pq_backtest_sweep_rules: `rules` is a sweep_rules table whose column c names a third
    column (a line, or -1 for `price`) -> device summary [P, N, 8], or [W, P, N, 8] with `windows`.  The other arguments are
    backtest_sweep's."""
    return _backtest_sweep("backtest_sweep_rules", "pq_backtest_sweep_rules", sweep_rules(rules), price, lines, benchmark, out, None, kw, windows)


def sweep_select(summary, train, test, metric, maximize=True):
    """D-26, pq_sweep_select: summary: the device [W, P, N, 8] result of a windowed sweep (the permuted view of a contiguous
    [W, N, P, 8]); train / test: F window indices each; metric: a SUMMARY_KEYS name or column index.  Per fold and symbol the set with
    the largest (smallest) metric in the train window -- a NaN ranks last, the lowest index wins a tie, all NaN gives 0 -- ->
    (chosen [F, N] int32, in_sample [F, N, 8], out_sample [F, N, 8]): the chosen set's summary in the train and in the test window."""
    if not isinstance(summary, torch.Tensor) or summary.dim() != 4 or summary.shape[3] != 8 or summary.dtype != torch.float64 or not summary.is_cuda:
        raise ValueError("summary must be a device float64 [W, P, N, 8] tensor")
    base = summary.permute(0, 2, 1, 3)
    if not base.is_contiguous():
        base = base.contiguous()
    W, n, P, _ = base.shape
    col = SUMMARY_KEYS.index(metric) if isinstance(metric, str) and metric in SUMMARY_KEYS else metric
    if isinstance(col, str):
        raise KeyError(f"metric must be one of {SUMMARY_KEYS}")
    tr, te = (np.ascontiguousarray(np.atleast_1d(np.asarray(x)), dtype=np.int32) for x in (train, test))
    if tr.ndim != 1 or tr.shape != te.shape:
        raise ValueError(f"train and test must be equally long lists of window indices, not {tr.shape} and {te.shape}")
    F = len(tr)
    dev = base.device
    chosen = torch.empty((F, n), dtype=torch.int32, device=dev)
    ins, outs = (torch.empty((F, n, 8), dtype=torch.float64, device=dev) for _ in range(2))
    _call("pq_sweep_select", dev, base, W, n, P, tr, te, F, int(col), 1 if maximize else 0, chosen, ins, outs)
    return chosen, ins, outs
