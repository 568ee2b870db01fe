"""ctypes binding of libpolars_quant_hip.so (the C ABI declared in include/pq_hip.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing the compute API raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` or `make -C polars_quant_amd/csrc`.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from ._spec import EXTRA, I, SPEC

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["PQ_LIB_PATH"]) if os.environ.get("PQ_LIB_PATH") else _HERE / "libpolars_quant_hip.so"  # override: A/B builds

PQ_OK = 0
NULL_BITS = 0x7FF80000504E554C
NULL_I32 = -2147483648


class PqError(RuntimeError):
    """Raised when a C-ABI call returns a non-zero status (message from pq_last_error)."""


class NullsNotAllowed(PqError):
    """The reference function rejects nulls (N-B family: rechunk().cont_slice()? fails, momentum.rs:12-13)."""


class Batch(C.Structure):
    # offsets: device pointer to n_series + 1 int64 row indices of a RAGGED batch (then len = the longest series, stride = the
    # total row count), or None for the regular [n_series][stride] layout (include/pq_hip.h)
    _fields_ = [("n_series", C.c_int64), ("len", C.c_int64), ("stride", C.c_int64), ("offsets", C.c_void_p)]


class BtParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("initial_capital", "buy_slippage", "sell_slippage", "buy_commission_rate",
                                          "sell_commission_rate", "min_commission", "position_size")]


class LevParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("initial_capital", "position_size", "leverage", "margin_call_threshold",
                                          "interest_rate", "commission_rate", "min_commission", "slippage")]


class SeqParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("initial_capital", "buy_slippage", "sell_slippage", "buy_commission_rate",
                                          "sell_commission_rate", "minimum_commission_fee")]


# One line per entry point of include/pq_hip.h that _spec does not describe: name (without pq_), the kind of the return value, the kinds
# of the parameters.  B / V / W / Q: const pq_batch / pq_bt_params / pq_lev_params / pq_seq_params *, s: const char *, p: any other
# pointer, i: int32_t / pq_status, l: int64_t, u: uint32_t, d: double, z: size_t.  tests/test_abi_signatures.py holds every line (and the
# derived ones) against the header.
_KINDS = {"p": C.c_void_p, "B": C.POINTER(Batch), "V": C.POINTER(BtParams), "W": C.POINTER(LevParams), "Q": C.POINTER(SeqParams),
          "s": C.c_char_p, "i": C.c_int32, "l": C.c_int64, "u": C.c_uint32, "d": C.c_double, "z": C.c_size_t}
_SIGNATURES = """
recommended_stride     l l
layout_check           i Bpi
abi_version            i
last_error             s
device_count           i p
ctx_create             i ipp
ctx_destroy            i p
ctx_set_stream         i pp
ctx_sync               i p
malloc                 i pzp
free                   i pp
host_register          i pz
host_unregister        i p
memcpy_h2d             i pppz
memcpy_d2h             i pppz
memcpy_h2d_pitched     i ppzpzzz
memcpy_d2h_pitched     i ppzpzzz
nulls_from_arrow       i pppll
validity_to_arrow      i pplpp
count_nulls            i pBpp
ema_all                i pBplpppp
atr_all                i pBppplpp
dm_pair                i pBpplpp
ad_all                 i pBppppllpp
macd_pair              i pBpllllpppppp
dm_system_all          i pBppplppppppp
sma_ma                 i pBplpp
cmo_rsi                i pBplpp
volume_all             i pBpppplllpppp
sar_pair               i pBppddddddddddpp
stoch_all              i pBppplllllllpppp
apo_ppo                i pBplllpp
aroon_all              i pBpplppp
dmi_all                i pBppplppppp
ht_all                 i pBppppppp
pattern_name           s i
pattern_id             i s
cdl                    i pBippppdp
cdl_all                i pBpppppp
backtest_vectorized    i pBppppVpppp
backtest_macd_cross    i pBplllVpppp
macd_cross_signals     i pBplllpp
backtest_wave_stats    i ppi
wt_stats               i ppi
ragged_rehouse_stats   i ppi
comm_unique_id         i p
comm_init              i piip
comm_destroy           i p
shard_range            i liipp
gather_summaries       i pplp
gather_summaries_begin i pplpi
gather_summaries_end   i pi
comm_sync              i p
cross_signals          i pBpppp
band_signals           i pBpddpp
channel_signals        i pBpppipp
gate_signals           i pBppiddpppp
zscore                 i pBpppp
scale_band             i pBpddpp
volume_surge_signals   i pBpppdpp
gap_signals            i pBpppddpp
pattern_any_signals    i pBpipipp
ma_stack_signals       i pBpipp
backtest_leveraged     i pBppppWpppipppppppppp
portfolio_metrics      i pBpdpp
backtest_report        i pBpdpWippppppppp
report_portfolio       i plppdp
backtest_sequential    i pllipppplpQlppppp
backtest_sweep         i pBppiplplVp
sweep_row_tile         i i
backtest_sweep_rules   i pBppiplplVp
backtest_sweep_windows i pBppiplplplVp
sweep_select           i pplllppliippp
factor_ic              i pBppipp
rolling_ic             i ppllpp
factor_quantiles       i pBppipppppp
factor_long_short      i pBppddpppppp
factor_double_sort     i pBpppiiippppppp
factor_coverage        i pBpp
ic_stats               i pplp
factor_portfolio       i pBpiippplddppp
factor_clean           i pBpidppiip
xsec_regress           i pBpippppppp
xsec_regress_wls       i pBpippplipppppppp
ts_regress             i pBpiupppppp
corr_t_test            i ppplpp
linear                 i pBpipppppppp
factor_orthogonalize   i pBpiip
ic_decay               i pBppiippp
ic_subgroup            i pBpppliippp
series_split_summary   i pplip
factor_rank            i pBpiip
factor_minmax          i pBpp
factor_weighted        i pBppplip
factor_binary          i pBppip
factor_rolling         i pBpillp
factor_rolling_regress i pBpiuplppppp
factor_ts              i pBpilip
factor_ts_pair         i pBppilp
factor_combine_weights i ppilillp
factor_combine         i pBpipip
risk_factor_cov        i pBppllilllpp
risk_specific_var      i pBppllilllplp
risk_portfolio         i pBppiplippllllpppp
risk_solve             i pBpipiplippllllplpp
factor_weights         i pBpilpplddpppppip
return_attribution     i pBpppipliplppplppppppp
suite_begin            i pB
suite_end              i pp
suite_abort            i p
suite_run              i pp
suite_destroy          i pp
suite_info             i pppp
suite_set_timing       i pi
suite_grid_stats       i pippppp
suite_grid_variant     i pip
suite_span_stats       i pipp
"""

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} not found: the MI355X HIP library is not built. "
                "Run `make -C polars_quant_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(str(LIB_PATH))
        sigs = [line.split() for line in _SIGNATURES.strip().splitlines()]
        # an indicator: (ctx, batch, input columns, parameters, output columns) -> pq_status, from its _spec entry
        sigs += [(name, "i", "pB" + "p" * len(cols) + "".join("l" if k == I else "d" for _, k, _ in params) + "p" * len(outs))
                 for name, (cols, params, outs, _fam) in {**SPEC, **EXTRA}.items()]
        for name, ret, *args in sigs:
            fn = getattr(L, "pq_" + name)
            fn.restype = _KINDS[ret]
            fn.argtypes = [_KINDS[k] for k in "".join(args)]
        _lib = L
    return _lib


def check(status: int) -> None:
    if status != PQ_OK:
        msg = lib().pq_last_error().decode("utf-8", "replace")
        raise (NullsNotAllowed if status == 3 else PqError)(f"pq status {status}: {msg}")
