"""The caller's side of the Polars expression plugin (include/pq_polars_plugin.h), shared by test_polars_plugin.py and
test_concurrency_gpu.py.  `polars` is not installed in this image, so what Polars does after dlsym is played by pyarrow: Series are
exported through the Arrow C Data Interface into hand-built SeriesExport structs.  The struct layout is the published polars-ffi one
and is NOT verified against the pinned polars 0.53."""
import ctypes as C
import pickle
from pathlib import Path

import numpy as np
import pyarrow as pa

ROOT = Path(__file__).resolve().parent.parent


class ArrowSchema(C.Structure):
    _fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64), ("n_children", C.c_int64),
                ("children", C.c_void_p), ("dictionary", C.c_void_p), ("release", C.c_void_p), ("private_data", C.c_void_p)]


class ArrowArray(C.Structure):
    _fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64), ("n_children", C.c_int64),
                ("buffers", C.c_void_p), ("children", C.c_void_p), ("dictionary", C.c_void_p), ("release", C.c_void_p), ("private_data", C.c_void_p)]


class SeriesExport(C.Structure):
    _fields_ = [("field", C.POINTER(ArrowSchema)), ("arrays", C.POINTER(C.POINTER(ArrowArray))), ("len", C.c_size_t), ("release", C.c_void_p),
                ("private_data", C.c_void_p)]


# every reference function of the shape (1..4 Float64 columns[, timeperiod]) -> Float64 has a plugin symbol pair
PLUGIN_FUNCS = ["sma", "ema", "wma", "dema", "tema", "trima", "kama", "midpoint", "rsi", "cmo", "mom", "roc", "rocp", "rocr", "rocr100",
                "trix", "ht_dcperiod", "ht_dcphase", "ht_trendline", "midprice", "plus_dm", "minus_dm", "aroonosc", "medprice", "obv",
                "adx", "adxr", "dx", "plus_di", "minus_di", "cci", "willr", "atr", "natr", "trange", "typprice", "wclprice", "mfi", "bop",
                "ad", "avgprice"]
# ... and the functions with other scalar parameters: name -> (input columns, [(parameter, reference default, a test value)])
MULTI_FUNCS = {"ma": (["real"], [("timeperiod", 30, 12), ("matype", 0, 1)]),
               "t3": (["real"], [("timeperiod", 5, 7), ("vfactor", 0.0, 0.7)]),
               "ultosc": (["high", "low", "close"], [("timeperiod1", 7, 5), ("timeperiod2", 14, 9), ("timeperiod3", 28, 20)]),
               "adosc": (["high", "low", "close", "volume"], [("fastperiod", 3, 4), ("slowperiod", 10, 13)]),
               "sar": (["high", "low"], [("acceleration", 0.0, 0.02), ("maximum", 0.0, 0.2)]),
               "sarext": (["high", "low"], [("startvalue", 0.0, 0.0), ("offsetonreverse", 0.0, 0.01), ("accelerationinitlong", 0.0, 0.02),
                                            ("accelerationlong", 0.0, 0.02), ("accelerationmaxlong", 0.0, 0.2),
                                            ("accelerationinitshort", 0.0, 0.03), ("accelerationshort", 0.0, 0.03),
                                            ("accelerationmaxshort", 0.0, 0.3)]),
               "ht_trendmode": (["real"], []),
               "apo": (["real"], [("fastperiod", 12, 5), ("slowperiod", 26, 13), ("matype", 0, 1)]),
               "ppo": (["real"], [("fastperiod", 12, 5), ("slowperiod", 26, 13), ("matype", 0, 1)]),
               "mavp": (["real", "periods"], [("minperiod", 2, 3), ("maxperiod", 30, 20), ("matype", 0, 1)])}
# ... and the Struct-valued ones: name -> (struct name, input columns, [(parameter, reference default, a test value)], field names)
STRUCT_FUNCS = {"bbands": ("bbands", ["real"], [("timeperiod", 20, 10), ("nbdevup", 2.0, 1.5), ("nbdevdn", 2.0, 2.5)], ["bb_upper", "bb_middle", "bb_lower"]),
                "mama": ("mama", ["real"], [("fastlimit", 0.0, 0.5), ("slowlimit", 0.0, 0.05)], ["mama", "fama"]),
                "aroon": ("aroon", ["high", "low"], [("timeperiod", 14, 9)], ["aroon_up", "aroon_down"]),
                "macd": ("macd_res", ["real"], [("fastperiod", 12, 5), ("slowperiod", 26, 13), ("signalperiod", 9, 4)], ["macd", "macd_signal", "macd_hist"]),
                "ht_phasor": ("ht_phasor", ["real"], [], ["inphase", "quadrature"]),
                "ht_sine": ("ht_sine", ["real"], [], ["sine", "leadsine"])}
TP_FUNCS = PLUGIN_FUNCS + list(MULTI_FUNCS) + list(STRUCT_FUNCS)   # (every symbol pair with the common signature: the argtypes loops below)


def _lib():
    so = ROOT / "polars_quant_amd" / "libpolars_quant_hip.so"
    if not so.exists():
        import __graft_entry__ as g
        g.build()
    try:
        import torch  # noqa: F401  (its bundled HIP runtime must be the first one in the process, as in polars_quant_amd._lib)
    except ImportError:
        pass
    L = C.CDLL(str(so))
    L._polars_plugin_get_version.restype = C.c_uint32
    L._polars_plugin_get_last_error_message.restype = C.c_char_p
    L.pq_plugin_kwargs_i64.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int64)]
    from polars_quant_amd._spec import PATTERN_NAMES
    both = [n + sfx for n in list(TP_FUNCS) + list(PATTERN_NAMES) for sfx in ("", "_over")]
    for f in ("_polars_plugin_" + n for n in both):
        getattr(L, f).argtypes = [C.POINTER(SeriesExport), C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(SeriesExport), C.c_void_p]
        getattr(L, f).restype = None
    for f in ("_polars_plugin_field_" + n for n in both):
        getattr(L, f).argtypes = [C.POINTER(ArrowSchema), C.c_size_t, C.POINTER(ArrowSchema), C.c_char_p, C.c_size_t]
        getattr(L, f).restype = None
    return L


def _export(chunks, name):
    """pyarrow chunks -> SeriesExport (keeps the ctypes objects alive through the returned tuple)"""
    field = ArrowSchema()
    arrs = [ArrowArray() for _ in chunks]
    ptrs = (C.POINTER(ArrowArray) * len(chunks))(*[C.pointer(a) for a in arrs])
    for i, (ch, a) in enumerate(zip(chunks, arrs)):
        sch = ArrowSchema()
        ch._export_to_c(C.addressof(a), C.addressof(sch) if i else C.addressof(field))
    field_named = pa.field(name, chunks[0].type)
    field2 = ArrowSchema()
    field_named._export_to_c(C.addressof(field2))
    se = SeriesExport(C.pointer(field2), ptrs, len(chunks), None, None)
    return se, (field, field2, arrs, ptrs)


def _import(ret):
    assert ret.release, "the plugin left return_value empty"
    assert ret.len == 1
    return pa.Array._import_from_c(C.addressof(ret.arrays[0].contents), C.addressof(ret.field.contents))


def _plugin_call(L, name, series, kwargs=None, literals=()):
    """series: [(pyarrow chunks, name)]; literals: trailing one-row literal arrays -> the imported result array"""
    ses, keep = [], []
    for chunks, nm in list(series) + [([lit], "literal") for lit in literals]:
        se, k = _export(chunks, nm)
        ses.append(se); keep.append(k)
    ins = (SeriesExport * len(ses))(*ses)
    kw = pickle.dumps(kwargs) if kwargs else None
    ret = SeriesExport()
    getattr(L, "_polars_plugin_" + name)(ins, len(ses), kw, len(kw) if kw else 0, C.byref(ret), None)
    assert ret.release, (name, L._polars_plugin_get_last_error_message())
    return _import(ret)


def _same_array(a, b):
    assert a.type == b.type and len(a) == len(b) and a.null_count == b.null_count
    na, nb = np.asarray(a.is_null()), np.asarray(b.is_null())
    assert (na == nb).all()
    va, vb = a.to_numpy(zero_copy_only=False)[~na], b.to_numpy(zero_copy_only=False)[~nb]
    if a.type == pa.float64():
        assert (va.view(np.uint64) == vb.view(np.uint64)).all()
    else:
        assert (va == vb).all()


def _groups(oracle, seed=0x5EED0010):
    lens = np.array([37, 1, 120, 64, 5, 300, 33, 2], dtype=np.int64)
    off = np.r_[0, np.cumsum(lens)]
    d = oracle.gen_ohlcv(seed, 1, int(off[-1]), 0)
    d = {k: np.ascontiguousarray(v[0]) for k, v in d.items()}
    d["real"] = d["close"]
    sym = np.repeat(np.arange(len(lens)), lens)
    return d, off, lens, sym


def _key_arrays(sym):
    """the same grouping as different Arrow layouts of the key column"""
    names = np.array([f"SYM{i:04d}{'x' * (i * 3)}" for i in range(int(sym.max()) + 1)])   # some longer than 12 bytes: out-of-line views
    out = {"int64": pa.array(sym.astype(np.int64)), "int32": pa.array(sym.astype(np.int32)), "uint8": pa.array(sym.astype(np.uint8)),
           "float64": pa.array(sym.astype(np.float64)), "utf8": pa.array(names[sym], type=pa.string()),
           "large_utf8": pa.array(names[sym], type=pa.large_string())}
    if hasattr(pa, "string_view"):
        out["string_view"] = pa.array(names[sym], type=pa.string_view())
    out["dictionary"] = pa.array(names[sym]).dictionary_encode()
    return out
