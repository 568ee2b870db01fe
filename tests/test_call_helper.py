"""not-gpu: the one rule by which the package hands arguments to the C ABI (api._marshal), and what the declared signatures do with
a value of the wrong kind (api._call)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_marshal_converts_by_one_rule():
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, BtParams, LevParams, SeqParams
    t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    view = t[:, 1:]                                   # an offset view: its own data_ptr, not the storage's
    a = np.arange(4, dtype=np.int32)
    structs = [Batch(2, 3, 3), BtParams(), LevParams(), SeqParams()]
    arr, ref = (C.c_double * 2)(1.0, 2.0), C.byref(C.c_int64())
    got = api._marshal((None, torch.empty((0, 5)), t[:, :0], t, view, a, *structs, 7, 2.5, arr, ref))
    assert got[0] is None
    assert got[1] is None and got[2] is None          # no element: NULL, whatever storage is behind it
    assert got[3] == t.data_ptr() and got[4] == view.data_ptr() == t.data_ptr() + 8
    assert got[5] == a.ctypes.data
    for g, s in zip(got[6:10], structs):              # by reference: the callee reads the caller's struct
        assert type(g) is type(C.byref(s))
        assert C.cast(g, C.c_void_p).value == C.addressof(s)
    assert got[10] == 7 and type(got[10]) is int and got[11] == 2.5 and type(got[11]) is float
    assert got[12] is arr and got[13] is ref          # ctypes values pass through for argtypes to convert
    assert api._marshal(()) == []


def test_subclasses_are_marshalled_like_their_base():
    from polars_quant_amd import api
    p = torch.nn.Parameter(torch.ones(3, dtype=torch.float64), requires_grad=False)
    m = np.arange(3.0).view(np.recarray)
    assert api._marshal((p, m)) == [p.data_ptr(), m.ctypes.data]


def test_a_float_for_an_integer_parameter_is_a_type_error():
    from polars_quant_amd import api
    from polars_quant_amd._lib import lib
    lo, hi = C.c_int64(), C.c_int64()
    api._call("pq_shard_range", None, 10, 1, 4, C.byref(lo), C.byref(hi))            # (int64_t, int32_t, int32_t, int64_t *, int64_t *)
    assert 0 <= lo.value < hi.value <= 10
    with pytest.raises(TypeError, match="pq_shard_range"):
        api._call("pq_shard_range", None, 10.5, 1, 4, C.byref(lo), C.byref(hi))      # int64_t
    with pytest.raises(TypeError, match="pq_shard_range"):
        api._call("pq_shard_range", None, 10, 1.0, 4, C.byref(lo), C.byref(hi))      # int32_t
    assert api._call("pq_recommended_stride", None, 17, checked=False) == 32
    with pytest.raises(TypeError):
        api._call("pq_recommended_stride", None, 17.0, checked=False)
    for name in ("pq_factor_rank", "pq_ic_stats", "pq_series_split_summary"):   # once undeclared: every integer slot refuses a float
        for t in getattr(lib(), name).argtypes:
            if t in (C.c_int32, C.c_int64, C.c_uint32):
                with pytest.raises(TypeError):
                    t.from_param(1.5)


def test_a_failed_status_raises_with_the_librarys_message():
    from polars_quant_amd import api
    from polars_quant_amd._lib import PqError
    lo = C.c_int64()
    with pytest.raises(PqError, match="pq status"):
        api._call("pq_shard_range", None, 10, 5, 4, C.byref(lo), C.byref(lo))       # rank 5 of 4
