"""The layout helpers of polars_quant_amd/api.py on CPU tensors, with no device call: _same_layout, _batch, _labels_on_pitch and
_codes_on_pitch must make the arguments of one call agree on ONE addressing (base + s * stride + t) before the C ABI sees them.

torch ignores the stride of a size-1 dimension and calls every zero-element tensor contiguous, so Tensor.contiguous() hands a one-row or
an empty tensor back unchanged whatever its strides: a helper that repairs a disagreement with contiguous() alone does nothing there
(_same_layout used to call itself for ever on the rows marked `recursed`).

The rules pinned here (the docstrings of _same_layout and _batch state them):
  * N > 1, T > 0: one stride(0) >= T for all, inner stride 1; arguments that agree come back as the same objects;
  * one row: arguments that report one stride pass as they are, arguments that disagree are re-viewed at stride T, without a copy
    where the inner stride is 1 -- so _batch of the first and of the last result are the same Batch;
  * empty: nothing to address; the call returns, and for N > 1 the results still report one stride.
"""
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from polars_quant_amd import api          # noqa: E402
from polars_quant_amd._lib import Batch   # noqa: E402

F64 = torch.float64


def rs(T):
    return (T + 15) // 16 * 16


def filled(*shape, start=1.0):
    """a float64 tensor of `shape` whose cells all differ (so a copy from the wrong cell shows)"""
    k = int(np.prod(shape))
    return (torch.arange(k, dtype=F64) + start).reshape(shape)


def pitched(n, T, pitch, base=0, start=1.0):
    """[n, T] view at row pitch `pitch`, `base` elements into its buffer"""
    flat = filled(base + max(n, 1) * pitch + 1, start=start)
    return flat[base:base + n * pitch].view(n, pitch)[:, :T]


def dense(n, T, start=1000.0):
    return filled(n, T, start=start)


def transposed(n, T, start=5000.0):
    return filled(T, n, start=start).t()


def even_pitch(T):
    return rs(T) if rs(T) != T else T + 16


def odd_pitch(T):
    return T + 1 if T % 2 == 0 else T + 2


# name -> builder of the argument list.  `recursed`: the rows on which _same_layout did not terminate before the one-row rule
TABLE = {}
RECURSED = {"row_of_pitched+fresh_row", "rows_of_two_pitches", "row_of_3d+unsqueezed", "empty_col_slices", "empty_col_slices_reversed"}


def row(name):
    def deco(fn):
        assert name not in TABLE
        TABLE[name] = fn
        return fn
    return deco


@row("row_of_pitched+fresh_row")
def _():
    return [filled(3, 2528)[1:2, :2520], dense(1, 2520)]


@row("rows_of_two_pitches")
def _():
    return [filled(3, 2528)[1:2, :2520], filled(3, 2544, start=7.0)[1:2, :2520]]


@row("row_of_3d+unsqueezed")
def _():
    return [filled(4, 3, 2528)[2, 1:2, :2520], filled(2520, start=9.0)[None]]


@row("empty_col_slices")
def _():
    return [filled(5, 16)[:, :0], torch.empty(5, 0, dtype=F64)]


@row("empty_col_slices_reversed")
def _():
    return [torch.empty(5, 0, dtype=F64), filled(5, 16)[:, :0]]


@row("fresh_row+row_of_pitched")
def _():
    return [filled(2520, start=9.0)[None], filled(3, 2528)[1:2, :2520]]


@row("one_row_three_ways")
def _():
    return [filled(3, 48)[2:3, :37], dense(1, 37), filled(2, 3, 64)[1, 1:2, :37]]


@row("one_row_inner_stride_2")
def _():
    return [dense(1, 37), filled(1, 74)[:, ::2]]


@row("one_row_transposed_first")
def _():
    return [filled(37, 1).t(), filled(3, 48)[0:1, :37]]


@row("one_row_same_pitch_agree")
def _():
    return [filled(3, 48)[1:2, :37], filled(3, 48, start=3.0)[2:3, :37]]


@row("one_row_T1_mixed")
def _():
    return [filled(3, 16)[1:2, :1], dense(1, 1), filled(1, 5).t()[3:4, :]]


@row("one_row_T0_mixed")
def _():
    return [filled(3, 16)[1:2, :0], torch.empty(1, 0, dtype=F64)]


@row("no_row_mixed")
def _():
    return [filled(3, 16)[:0, :5], torch.empty(0, 5, dtype=F64)]


for _T in (37, 48, 1, 0):
    def _add(T):
        n = 3
        P, Q, Od = even_pitch(T), even_pitch(T) + 16, odd_pitch(T) if odd_pitch(T) % 2 else odd_pitch(T) + 1
        TABLE[f"n3_T{T}_pitched+dense"] = lambda: [pitched(n, T, P), dense(n, T)]
        TABLE[f"n3_T{T}_dense+pitched"] = lambda: [dense(n, T), pitched(n, T, P)]
        TABLE[f"n3_T{T}_two_even_pitches"] = lambda: [pitched(n, T, P), pitched(n, T, Q, start=3.0), pitched(n, T, P, start=5.0)]
        TABLE[f"n3_T{T}_odd_pitch+pitched"] = lambda: [pitched(n, T, Od), pitched(n, T, P, start=3.0)]
        TABLE[f"n3_T{T}_odd_pitch_off_base_agree"] = lambda: [pitched(n, T, Od, base=1), pitched(n, T, Od, start=3.0)]
        TABLE[f"n3_T{T}_transposed+dense"] = lambda: [transposed(n, T), dense(n, T)]
        TABLE[f"n3_T{T}_pitched+transposed"] = lambda: [pitched(n, T, P), transposed(n, T)]
        TABLE[f"n3_T{T}_one_pitch_agree"] = lambda: [pitched(n, T, P), pitched(n, T, P, start=3.0), pitched(n, T, P, base=2, start=5.0)]
        TABLE[f"n3_T{T}_dense_agree"] = lambda: [dense(n, T), dense(n, T, start=3.0)]
    _add(_T)


def ibits(t):
    return t.contiguous().view(torch.int64) if t.numel() else t.reshape(-1)


def agree(ts):
    """the arguments describe one addressing already: one stride(0), inner stride 1"""
    return all(t.stride() == ts[0].stride() and t.stride(1) == 1 for t in ts)


@pytest.fixture
def low_recursion_limit():
    """a helper that recurses on its own arguments fails within a few frames instead of a thousand"""
    old = sys.getrecursionlimit()
    depth, f = 0, sys._getframe()
    while f is not None:
        depth, f = depth + 1, f.f_back
    sys.setrecursionlimit(depth + 60)
    try:
        yield
    finally:
        sys.setrecursionlimit(old)


def test_the_table_holds_the_rows_that_did_not_terminate():
    assert RECURSED <= set(TABLE)
    for T in (37, 48, 1, 0):
        for kind in ("pitched+dense", "two_even_pitches", "odd_pitch+pitched", "transposed+dense", "one_pitch_agree"):
            assert f"n3_T{T}_{kind}" in TABLE


@pytest.mark.parametrize("name", sorted(TABLE))
def test_same_layout(name, low_recursion_limit):
    ts = TABLE[name]()
    n, T = ts[0].shape
    before = [t.clone() for t in ts]
    strides = [t.stride() for t in ts]
    out = api._same_layout(list(ts))                                  # returns (a RecursionError fails the test here)
    assert len(out) == len(ts)
    for k, (t, o, b4) in enumerate(zip(ts, out, before)):
        assert tuple(o.shape) == (n, T) and o.dtype == F64, (name, k)
        assert torch.equal(ibits(o), ibits(b4)), f"{name}: argument {k} changed value"
        assert torch.equal(ibits(t), ibits(b4)) and t.stride() == strides[k], f"{name}: the caller's argument {k} was modified"
        if T > 1:
            assert o.stride(1) == 1, (name, k, o.stride())
    if n > 1 and T > 0:
        s = {o.stride(0) for o in out}
        assert len(s) == 1 and min(s) >= T, (name, [o.stride() for o in out])
    for pick in (0, -1):                                              # the first (most callers), the last (linear, the regressions)
        b = api._batch(out[pick])
        assert (b.n_series, b.len) == (n, T)
        assert b.stride >= T
        for k, o in enumerate(out):
            assert n <= 1 or o.stride(0) == b.stride, (name, pick, k, o.stride(), b.stride)
        if n == 1 and T > 0:
            # one row: the Batch must be the same whichever argument it is taken from, and a stride above T only where every
            # argument reports it (a pitch that another argument was not allocated with is never passed on)
            assert b.stride == api._batch(out[0]).stride
            assert b.stride == T or all(o.stride(0) == b.stride for o in out), (name, [o.stride() for o in out], b.stride)
    if agree(ts):
        assert all(o is t for o, t in zip(out, ts)), f"{name}: arguments that agree must pass as the same objects"
    if n == 1 and T > 0:                                              # the re-view is no copy where the inner stride is 1
        for t, o in zip(ts, out):
            if t.stride(1) == 1 or T == 1:
                assert o.data_ptr() == t.data_ptr(), f"{name}: a one-row argument was copied"


def test_same_layout_refuses_other_shapes():
    with pytest.raises(api.PqError):
        api._same_layout([dense(1, 5), dense(1, 6)])
    with pytest.raises(api.PqError):
        api._same_layout([dense(3, 0), dense(0, 3)])


@pytest.mark.parametrize("n,T,s,dense_,lone,exp", [
    (3, 37, 48, False, False, 48), (3, 37, 48, True, False, 37), (3, 37, 37, False, False, 37),
    (1, 37, 48, False, False, 48), (1, 37, 48, False, True, 37), (1, 37, 48, True, False, 37),
    (1, 37, 1, False, False, 37),      # a one-row view whose ignored stride is below T (x[None] of some builds, an expanded row)
    (1, 1, 16, False, False, 16), (1, 0, 16, False, False, 16), (0, 5, 16, False, False, 16), (3, 0, 16, False, False, 16),
])
def test_batch_stride(n, T, s, dense_, lone, exp):
    t = torch.empty(max(n, 1) * max(s, T) + 1, dtype=F64).as_strided((n, T), (s, 1))
    b = api._batch(t, dense=dense_, lone_dense=lone)
    assert (b.n_series, b.len, b.stride) == (n, T, exp)


# ---------------------------------------------------------------------------------------------------------------------------------
# _labels_on_pitch / _codes_on_pitch: the result is addressed by the BATCH's stride, whatever the argument's own layout was

CPU = torch.device("cpu")


def u8(n, T, pitch=None, base=0, transposed_=False):
    k = torch.arange(max(n, 1) * max(pitch or T, T, 1) + base + 1, dtype=torch.int64).remainder(251).to(torch.uint8)
    if transposed_:
        return k[:n * T].view(T, n).t()
    p = pitch or T
    return k[base:base + n * p].view(n, p)[:, :T]


LABEL_ROWS = {
    "n3_T37_dense_to_pitch48": lambda: (u8(3, 37), 48),
    "n3_T37_pitch48_agree": lambda: (u8(3, 37, 48), 48),
    "n3_T37_pitch64_to_pitch48": lambda: (u8(3, 37, 64), 48),
    "n3_T37_transposed_to_pitch48": lambda: (u8(3, 37, transposed_=True), 48),
    "n3_T37_pitch48_to_dense": lambda: (u8(3, 37, 48), 37),
    "n3_T48_dense_agree": lambda: (u8(3, 48), 48),
    "n3_T1_pitch16_to_dense": lambda: (u8(3, 1, 16), 1),
    "n3_T1_transposed_agree": lambda: (u8(3, 1, transposed_=True), 1),
    "n3_T0_pitch16_to_pitch32": lambda: (u8(3, 16, 16)[:, :0], 32),
    "n1_T37_row_of_pitch48_batch37": lambda: (u8(3, 37, 48)[1:2], 37),
    "n1_T37_dense_row_batch48": lambda: (u8(1, 37), 48),
    "n1_T37_inner_stride_2": lambda: (u8(1, 74)[:, ::2], 37),
    "n1_T1_batch16": lambda: (u8(3, 1, 16)[2:3], 16),
    "n1_T0": lambda: (u8(1, 16)[:, :0], 0),
    "n0_T5": lambda: (u8(3, 5)[:0], 16),
    "n3_T37_numpy": lambda: (u8(3, 37).numpy().copy(), 48),
    "n3_T37_numpy_fortran": lambda: (np.asfortranarray(u8(3, 37).numpy()), 48),
}


def addressed(t, n, T, stride):
    """the [n, T] cells that a kernel reads at base + s * stride + t (torch refuses a view beyond the storage)"""
    if n == 0 or T == 0:
        return t.new_empty((n, T))
    return t.as_strided((n, T), (stride if n > 1 else max(stride, T), 1))


@pytest.mark.parametrize("name", sorted(LABEL_ROWS))
def test_labels_on_pitch(name, low_recursion_limit):
    lab, stride = LABEL_ROWS[name]()
    n, T = lab.shape
    exp = torch.from_numpy(np.ascontiguousarray(np.asarray(lab))).clone() if not isinstance(lab, torch.Tensor) else lab.clone()
    b = Batch(n, T, stride)
    out = api._labels_on_pitch(lab, b, CPU, (n, T))
    assert tuple(out.shape) == (n, T) and out.dtype == torch.uint8
    assert torch.equal(out, exp), name
    assert T <= 1 or out.stride(1) == 1, (name, out.stride())
    assert n <= 1 or out.stride(0) == b.stride, (name, out.stride(), b.stride)
    assert torch.equal(addressed(out, n, T, out.stride(0) if n <= 1 else b.stride), exp), name
    if isinstance(lab, torch.Tensor) and (T <= 1 or lab.stride(1) == 1) and (n <= 1 or lab.stride(0) == stride):
        assert out is lab, f"{name}: labels on the batch's pitch must pass as they are"


def test_labels_on_pitch_refusals():
    b = Batch(3, 37, 48)
    with pytest.raises(ValueError):
        api._labels_on_pitch(u8(3, 36), b, CPU, (3, 37))
    with pytest.raises(ValueError):
        api._labels_on_pitch(u8(3, 37).to(torch.int32), b, CPU, (3, 37))


CODE_ROWS = {
    # name -> (codes, n, T, batch stride, spread)
    "n3_T37_matrix_dense_to_48": lambda: (torch.arange(111, dtype=torch.int64).view(3, 37) - 5, 3, 37, 48, False),
    "n3_T37_matrix_pitch64_to_48": lambda: (torch.arange(192, dtype=torch.int32).view(3, 64)[:, :37], 3, 37, 48, False),
    "n3_T37_matrix_transposed_to_37": lambda: (torch.arange(111, dtype=torch.int64).view(37, 3).t(), 3, 37, 37, True),
    "n3_T37_vector": lambda: (torch.tensor([4, -1, 2]), 3, 37, 48, False),
    "n3_T37_vector_strided": lambda: (torch.tensor([4, 9, -1, 9, 2, 9])[::2], 3, 37, 48, False),
    "n3_T37_vector_spread": lambda: (torch.tensor([4, -1, 2]), 3, 37, 48, True),
    "n3_T1_matrix": lambda: (torch.tensor([[4], [-1], [2]]), 3, 1, 16, False),
    "n3_T0_matrix": lambda: (torch.zeros((3, 0), dtype=torch.int64), 3, 0, 0, False),
    "n3_T0_vector_spread": lambda: (torch.tensor([4, -1, 2]), 3, 0, 0, True),
    "n1_T37_row_of_matrix_batch37": lambda: (torch.arange(192, dtype=torch.int32).view(3, 64)[1:2, :37], 1, 37, 37, False),
    "n1_T37_row_batch48": lambda: (torch.arange(37, dtype=torch.int64)[None], 1, 37, 48, False),
    "n1_T37_vector_spread": lambda: (torch.tensor([7]), 1, 37, 37, True),
    "n0_T5_matrix": lambda: (torch.zeros((0, 5), dtype=torch.int64), 0, 5, 16, False),
}


@pytest.mark.parametrize("name", sorted(CODE_ROWS))
def test_codes_on_pitch(name, low_recursion_limit):
    codes, n, T, stride, spread = CODE_ROWS[name]()
    exp = codes.clone().to(torch.int32)
    b = Batch(n, T, stride)
    out, pitch = api._codes_on_pitch(codes, b, CPU, spread=spread)
    assert out.dtype == torch.int32
    if codes.dim() == 1 and not spread:
        assert pitch == 0 and tuple(out.shape) == (n,) and out.is_contiguous() and (n <= 1 or out.stride(0) == 1)
        assert torch.equal(out, exp)
        return
    assert pitch == b.stride
    full = exp if exp.dim() == 2 else exp[:, None].expand(n, T)
    assert torch.equal(addressed(out, n, T, pitch), full), name
