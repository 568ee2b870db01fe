"""not-gpu: the static shape of every recordable sequential op -- rows per tile, bytes of its tiles in LDS, register class, row
masking -- is what it was before the tiled body (csrc/pq_dev.h run_seq_lds) changed how it addresses and stores its tiles.  These figures decide a job's LDS class, its grid and its kernel (csrc/suite.hip suite_finalize; seq_lds_bytes adds
the op's rings, whose size depends on its parameters alone), so that change must not move any of them.  The library lists them itself
(pq_seq_op_info, one row per op of the job kernels' op lists); the expected rows were printed from the op headers of the commit before
the change by a host-only program over the same lists.

The table is keyed by op type, not by function name: the functions of _spec.SPEC map onto these ops in the C entry points (several
functions share one op, the multi-output jobs cover several functions), and every op a recorded function can become is in the lists."""
import ctypes
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# (job kind, rows per tile, tile bytes in LDS, HEAVY, row-masked)
EXPECTED = [
    (1, 16, 8704, 0, 0),  # SmaOp
    (2, 16, 8704, 0, 0),  # EmaOp
    (3, 8, 13824, 0, 0),  # BbandsOp
    (4, 16, 8704, 0, 0),  # DemaOp
    (5, 16, 8704, 0, 0),  # TemaOp
    (6, 16, 8704, 0, 0),  # T3Op
    (7, 16, 8704, 0, 0),  # WmaOp
    (8, 16, 8704, 0, 0),  # KamaOp
    (9, 16, 8704, 0, 0),  # MidpointOp
    (10, 8, 9216, 0, 0),  # MidpriceOp
    (11, 8, 9216, 0, 0),  # SarextOp
    (12, 8, 9216, 0, 1),  # MavpPickOp
    (101, 8, 9216, 0, 1),  # MavpSelOp<SmaOp>
    (102, 8, 9216, 0, 1),  # MavpSelOp<EmaOp>
    (107, 8, 9216, 0, 1),  # MavpSelOp<WmaOp>
    (104, 8, 9216, 0, 1),  # MavpSelOp<DemaOp>
    (105, 8, 9216, 0, 1),  # MavpSelOp<TemaOp>
    (106, 8, 9216, 0, 1),  # MavpSelOp<T3Op>
    (108, 8, 9216, 0, 1),  # MavpSelOp<KamaOp>
    (20, 16, 8704, 0, 0),  # CmoOp
    (21, 16, 8704, 0, 0),  # RsiOp
    (22, 8, 13824, 0, 0),  # MacdOp
    (23, 16, 8704, 0, 0),  # TrixOp
    (24, 4, 7680, 0, 0),  # UltoscOp
    (25, 8, 18432, 0, 0),  # MfiOp
    (26, 8, 13824, 0, 0),  # DmOp<0>
    (27, 8, 13824, 0, 0),  # DmOp<1>
    (28, 8, 13824, 0, 0),  # DmOp<2>
    (29, 8, 9216, 0, 0),  # DmRawOp<true>
    (30, 8, 9216, 0, 0),  # DmRawOp<false>
    (31, 8, 13824, 0, 0),  # SmaTpOp
    (70, 16, 8704, 0, 0),  # TrimaOp
    (71, 16, 8704, 0, 0),  # MaDiffOp<0>
    (72, 16, 8704, 0, 0),  # MaDiffOp<1>
    (73, 8, 13824, 0, 0),  # MacdextOp
    (74, 8, 13824, 0, 0),  # StochOp<0>
    (75, 8, 13824, 0, 0),  # StochOp<1>
    (96, 8, 18432, 0, 0),  # StochAllOp
    (76, 8, 9216, 0, 0),  # StochRsiOp
    (77, 8, 13824, 0, 0),  # CciOp
    (78, 8, 23040, 0, 0),  # DmAllOp<true>
    (80, 8, 13824, 0, 0),  # DmAllOp<false>
    (82, 8, 9216, 0, 1),  # MavpBlockOp<1>
    (83, 8, 9216, 0, 1),  # MavpSma16Op
    (86, 8, 9216, 0, 1),  # MavpSma8Op
    (84, 8, 9216, 0, 0),  # MavpSma32Op
    (87, 8, 13824, 0, 0),  # UltoscOp8
    (40, 8, 13824, 0, 0),  # AtrOp<false>
    (41, 8, 13824, 0, 0),  # AtrOp<true>
    (44, 8, 9216, 0, 0),  # ObvOp
    (42, 8, 18432, 0, 0),  # AdOp<false>
    (43, 8, 18432, 0, 0),  # AdOp<true>
    (45, 16, 8704, 0, 0),  # HtOp<0>
    (46, 16, 8704, 0, 0),  # HtOp<1>
    (47, 8, 9216, 0, 0),  # HtOp<2>
    (48, 8, 9216, 0, 0),  # HtOp<3>
    (49, 8, 9216, 0, 0),  # HtOp<4>
    (79, 8, 13824, 0, 0),  # HtAllOp
    (85, 8, 13824, 0, 0),  # HtAll6Op
    (62, 8, 13824, 0, 0),  # BtMacdOp
    (63, 8, 13824, 0, 0),  # LevOp
    (90, 8, 18432, 0, 0),  # EmaAllOp
    (91, 8, 13824, 0, 0),  # AtrAllOp
    (92, 8, 9216, 0, 0),  # DmPairOp
    (93, 8, 18432, 0, 0),  # AdAllOp
    (94, 8, 27648, 0, 0),  # MacdPairOp
    (95, 8, 9216, 0, 0),  # ApoPpoOp
    (97, 8, 9216, 0, 0),  # SarPairOp
    (98, 8, 18432, 0, 0),  # VolumeAllOp
    (99, 8, 32256, 0, 0),  # DmiAtrOp
    (89, 8, 9216, 0, 0),  # CmoRsiOp
    (88, 8, 9216, 0, 0),  # SmaDupOp
]

def _table():
    so = ROOT / "polars_quant_amd" / "libpolars_quant_hip.so"
    if not so.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(so))
    lib.pq_seq_op_info.restype = ctypes.c_int32
    lib.pq_seq_op_info.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    rows, row = [], (ctypes.c_int32 * 5)()
    while lib.pq_seq_op_info(len(rows), row):
        rows.append(tuple(row))
    return rows


def test_tiles_lds_bytes_and_class_of_every_op_are_unchanged():
    got = _table()
    assert got == EXPECTED
