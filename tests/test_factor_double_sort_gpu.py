"""-m gpu: the two-way (double) sort (D-31, csrc/xsec/double_sort.hip) against the numpy restatement in tests/xsec_double_ref.py and
against the single sort of D-15 on masked columns.  Every comparison is bitwise: labels, counts, means, turnover, both spread tables
and the summary rows."""
import ctypes as C

import numpy as np
import pytest

import test_factor_sorts_gpu as S
import xsec_double_ref as D
import xsec_ref as X
from test_factor_sorts_gpu import same, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq

GRIDS = [(2, 3), (3, 3), (5, 5), (10, 10), (2, 10), (10, 2)]
SHAPES = [(1, 5), (2, 3), (7, 9), (37, 50), (300, 131)]
KINDS = ["plain", "nulls", "discrete", "special", "same", "control_nulls"]
MODES = [False, True]


def make(kind, n, T, seed):
    """control, factor, return: the factor and the return as test_factor_sorts_gpu.make builds them, the control a second column of
    the same kind (A == B: the factor itself; control_nulls: a plain factor under a control with nulls, NaN and +-inf)"""
    base = {"same": "plain", "control_nulls": "plain"}.get(kind, kind)
    b, r = S.make(base, n, T, seed)
    if kind == "same":
        return b.copy(), b, r
    a, _ = S.make("nulls" if kind == "control_nulls" else base, n, T, seed + 1000)
    if kind == "control_nulls":
        rng = np.random.default_rng(seed + 2000)
        a[rng.random((n, T)) < 0.02] = np.nan
        a[rng.random((n, T)) < 0.02] = -np.inf
    return a, b, r


def check(a, b, r, qa, qb, dependent, pitch=None, exp=None):
    from polars_quant_amd import api
    got = api.factor_double_sort(to_dev(a, pitch), to_dev(b, pitch), to_dev(r, pitch), qa, qb, dependent, labels=True)
    torch.cuda.synchronize()
    exp = D.groups(a, b, r, qa, qb, dependent) if exp is None else exp
    tag = f"{qa}x{qb} dependent={dependent} {a.shape} pitch={pitch}"
    for k in ("labels", "count", "mean_return", "turnover", "spread_factor", "spread_control"):
        same(f"{k} {tag}", got[k].cpu().numpy(), exp[k])
    same("summary " + tag, got["summary"].cpu().numpy(), D.summary(exp))
    return got, exp


@pytest.mark.parametrize("dependent", MODES, ids=["independent", "dependent"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_double_sort_bitwise(pq, shape, kind, dependent):
    n, T = shape
    a, b, r = make(kind, n, T, 31 + n + T)
    for qa, qb in GRIDS:
        _, exp = check(a, b, r, qa, qb, dependent)
        if dependent and kind == "plain" and ((shape, (qa, qb)) in (((7, 9), (3, 3)), ((37, 50), (10, 10)))):
            assert (exp["labels"] == X.LABEL_MID).any()      # control buckets below Qb members: in the sample, in no cell


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.to(torch.int64)


def identical(name, got, exp):
    assert got.shape == exp.shape and bool((bits(got) == bits(exp)).all()), name


@pytest.mark.parametrize("shape", [(300, 131), (16385, 4)], ids=["300x131", "16385x4"])
def test_dependent_rows_are_the_single_sort_kernels_on_masked_factors(pq, shape):
    """dependent mode: row a's labels (OUT -> MID inside the bucket), mean, count, turnover, spread_factor[a] and summary rows are
    pq_factor_quantiles on the factor masked to control bucket a, bit for bit; the control marginal is pq_factor_quantiles on the
    control masked to the sample"""
    from polars_quant_amd import api
    n, T = shape
    a, b, r = make("nulls", n, T, 77)
    qa, qb = 3, 4
    ok = D.sample(a, b, r)
    ad, bd, rd = to_dev(a), to_dev(b), to_dev(r)
    got = api.factor_double_sort(ad, bd, rd, qa, qb, True, labels=True)
    null = torch.tensor(X.NULL, dtype=torch.float64, device="cuda")
    ctl = api.factor_quantiles(torch.where(torch.from_numpy(ok).cuda(), ad, null), rd, qa, labels=True)
    la = ctl["labels"]
    identical("control marginal", got["count"].view(qa, qb, T).sum(dim=1).to(torch.int32), ctl["count"])
    identical("out of sample", got["labels"] == X.LABEL_OUT, la == X.LABEL_OUT)
    for g in range(qa):
        one = api.factor_quantiles(torch.where(la == g, bd, null), rd, qb, labels=True)
        mem = la == g
        lab = torch.where(one["labels"] == X.LABEL_OUT, torch.tensor(X.LABEL_MID, dtype=torch.uint8, device="cuda"),
                          (one["labels"].to(torch.int32) + g * qb).to(torch.uint8))
        identical(f"labels {g}", got["labels"][mem], lab[mem])
        for k in ("mean_return", "count", "turnover"):
            identical(f"{k} {g}", got[k][g * qb:(g + 1) * qb], one[k])
        identical(f"spread {g}", got["spread_factor"][g], one["spread"])
        identical(f"summary cells {g}", got["summary"][g * qb:(g + 1) * qb], one["summary"][:qb])
        identical(f"summary spread {g}", got["summary"][qa * qb + g], one["summary"][qb])


def sized(n, T, seed, full=(0, 1, 3)):
    """plain columns with nulls on the days outside `full`: those days' sample is the whole cross-section (n = P, no +inf tail)"""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((n, T)), rng.standard_normal((n, T))
    r = np.round(0.1 * b + rng.standard_normal((n, T)) * 0.02, 4)
    for x in (a, b, r):
        hole = rng.random((n, T)) < 0.04
        hole[:, [t for t in full if t < T]] = False
        x[hole] = X.NULL
    return a, b, r


@pytest.mark.parametrize("n", [16, 17, 32, 255, 256, 257, 513, 1024, 1025, 16384])
def test_size_classes_of_the_lds_sort(pq, n):
    """the P boundaries of the LDS row, days with no +inf tail, the D-12 block boundaries; 16 384 is the widest LDS row"""
    a, b, r = sized(n, 5, n)
    for dependent in MODES:
        check(a, b, r, 3, 4, dependent)


@pytest.mark.parametrize("n", [16385, 20000])
def test_wide_cross_section_segmented_sort(pq, n):
    """n_series > 16384: two or three segmented sorts, with a discrete day and a day of signed zeros in both columns"""
    a, b, r = sized(n, 4, n)
    rng = np.random.default_rng(n + 1)
    a[:, 1] = np.round(a[:, 1] * 2.0) / 2.0
    b[:, 1] = np.round(b[:, 1] * 2.0) / 2.0
    a[:, 2] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    b[:, 2] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    for dependent in MODES:
        check(a, b, r, 3, 4, dependent)


@pytest.mark.parametrize("grid", [(2, 2), (2, 3), (2, 5), (3, 4), (4, 5), (3, 7), (4, 8), (5, 7), (8, 8), (7, 10), (9, 10), (10, 10)],
                         ids=lambda g: f"C{g[0] * g[1]}")
def test_cell_tiles(pq, grid):
    """the cells stage picks the accumulator form by the cell count.  Up to 20 cells they are registers: C = 4 in <5>, C = 6 and 10 in
    <10>, C = 12 and 20 in <20> (<2> has no Qa x Qb grid).  C = 21 is the first count in LDS tiles of XS_CT = 32 cells, walked with
    blockIdx.z: C = 32 | 35, 64 | 70, 90 | 100 lie on both sides of every tile count 1 | 2 | 3 | 4 that a Qa x Qb grid can reach (33,
    65 and 97 are no products of two numbers in [2, 10]); C = 4 and C = 100 are the ends; two blocks of symbols"""
    a, b, r = make("nulls", 300, 20, 9)
    for dependent in MODES:
        check(a, b, r, *grid, dependent)


@pytest.mark.parametrize("T", [63, 64, 65])
def test_day_tiles(pq, T):
    a, b, r = make("nulls", 40, T, T)
    for dependent in MODES:
        check(a, b, r, 2, 3, dependent)


def test_summary_past_one_chunk(pq):
    """T = 2 049 > XS_CHUNK days"""
    a, b, r = make("nulls", 20, 2049, 12)
    check(a, b, r, 2, 3, True)
    check(a, b, r, 2, 2, False)


def test_odd_row_pitch(pq):
    """batch stride > len (and odd): inputs read and labels written at the inputs' pitch"""
    a, b, r = make("nulls", 300, 131, 5)
    for dependent in MODES:
        got, _ = check(a, b, r, 2, 3, dependent, pitch=139)
        assert got["labels"].stride(0) == 139


def test_labels_omitted_against_labels_given(pq):
    """labels=False: the cells stage keeps the symbol-major labels in its workspace at row pitch len (the turnover reads day t - 1
    there); labels=True: in the caller's matrix at the inputs' pitch.  n = 257 (a second block of one symbol), T = 65 (a second day
    tile of one day), inputs at pitch 71: every other output of the single sorts and of the double sort is the same, bit for bit"""
    from polars_quant_amd import api
    a, b, r = make("nulls", 257, 65, 15)
    ad, bd, rd = (to_dev(x, 71) for x in (a, b, r))
    calls = {"quantiles": lambda lab: api.factor_quantiles(bd, rd, 7, labels=lab),
             "long_short": lambda lab: api.factor_long_short(bd, rd, 0.3, 0.2, labels=lab),
             "double independent": lambda lab: api.factor_double_sort(ad, bd, rd, 3, 4, False, labels=lab),
             "double dependent": lambda lab: api.factor_double_sort(ad, bd, rd, 3, 4, True, labels=lab)}
    for name, call in calls.items():
        without, given = call(False), call(True)
        assert "labels" not in without and given["labels"].stride(0) == 71
        assert set(without) == set(given) - {"labels"}
        for k, v in without.items():
            identical(f"{name} {k}", v, given[k])
        assert int(given["count"].sum()) > 0 and bool((given["turnover"][:, 1:] > 0.0).any())     # the calls compared something


def test_factor_method_shapes_and_defaults(pq):
    a, b, r = make("nulls", 60, 33, 21)
    exp = D.groups(a, b, r, 2, 3, True)
    s = D.summary(exp)
    got = pq.Factor().double_sort(a, b, r)
    T = 33
    assert {k: tuple(v.shape) for k, v in got.items() if k != "summary"} == {
        "mean_return": (2, 3, T), "count": (2, 3, T), "turnover": (2, 3, T), "spread": (2, T), "spread_avg": (T,),
        "control_spread": (3, T), "control_spread_avg": (T,)}
    assert {k: tuple(v.shape) for k, v in got["summary"].items()} == {"cells": (2, 3, 5), "spread": (3, 5), "control_spread": (4, 5)}
    for k in ("mean_return", "count", "turnover"):
        same(k, got[k].reshape(6, T).cpu().numpy(), exp[k])
    same("spread", got["spread"].cpu().numpy(), exp["spread_factor"][:2])
    same("spread_avg", got["spread_avg"].cpu().numpy(), exp["spread_factor"][2])
    same("control_spread", got["control_spread"].cpu().numpy(), exp["spread_control"][:3])
    same("control_spread_avg", got["control_spread_avg"].cpu().numpy(), exp["spread_control"][3])
    same("summary", torch.cat([got["summary"]["cells"].reshape(6, 5), got["summary"]["spread"], got["summary"]["control_spread"]])
         .cpu().numpy(), s)
    assert got["spread_avg"].data_ptr() == got["spread"].data_ptr() + 2 * T * 8          # views of one buffer, not copies
    ind = pq.Factor().double_sort(a, b, r, 5, 5, dependent=False)
    same("independent", ind["mean_return"].reshape(25, T).cpu().numpy(), D.groups(a, b, r, 5, 5, False)["mean_return"])


def test_refusals_launch_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as status, lib
    L = lib()
    n, T = 40, 30
    a, b, r = make("plain", n, T, 1)
    ad, bd, rd = to_dev(a), to_dev(b), to_dev(r)
    for qa, qb, what in ((1, 3, "n_control"), (11, 3, "n_control"), (2, 1, "n_quantiles"), (2, 11, "n_quantiles")):
        with pytest.raises(pq.PqError, match=what):
            api.factor_double_sort(ad, bd, rd, qa, qb)
    h = api.ctx()
    vp, i32 = C.c_void_p, C.c_int32
    bt = Batch(n, T, T)
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    mean, cnt, tov = f64(6, T), torch.full((6, T), 7, dtype=torch.int32, device="cuda"), f64(6, T)
    sf, sc, summ = f64(3, T), f64(4, T), f64(13, 5)
    lab = torch.full((n, T), 7, dtype=torch.uint8, device="cuda")
    ins = [vp(t.data_ptr()) for t in (ad, bd, rd)]
    outs = [vp(t.data_ptr()) for t in (lab, mean, cnt, tov, sf, sc, summ)]
    for mode in (-1, 2):
        with pytest.raises(pq.PqError, match="mode"):
            status(L.pq_factor_double_sort(h, C.byref(bt), *ins, i32(2), i32(3), i32(mode), *outs))
    for qa, qb, what in ((1, 3, "n_control"), (2, 11, "n_quantiles")):
        with pytest.raises(pq.PqError, match=what):
            status(L.pq_factor_double_sort(h, C.byref(bt), *ins, i32(qa), i32(qb), i32(1), *outs))
    status(L.pq_suite_begin(h, C.byref(bt)))
    try:
        with pytest.raises(pq.PqError, match="recorded"):
            status(L.pq_factor_double_sort(h, C.byref(bt), *ins, i32(2), i32(3), i32(1), *outs))
    finally:
        status(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    with pytest.raises(pq.PqError, match="ragged"):
        status(L.pq_factor_double_sort(h, C.byref(rb), *ins, i32(2), i32(3), i32(1), *outs))
    torch.cuda.synchronize()
    for name, t in (("labels", lab), ("mean", mean), ("count", cnt), ("turnover", tov), ("spread_factor", sf), ("spread_control", sc),
                    ("summary", summ)):
        assert bool((t == 7).all()), f"{name} was written by a refused call"
    check(a, b, r, 2, 3, True)        # the context computes again after the refusals


def test_empty_inputs(pq):
    """len == 0: PQ_OK and nothing written (the C ABI, on buffers that exist); n_series == 0: every day is empty"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as status, lib
    buf = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    bt = Batch(5, 0, 0)
    status(lib().pq_factor_double_sort(api.ctx(), C.byref(bt), p, p, p, C.c_int32(2), C.c_int32(3), C.c_int32(1), None, p, p, p, p, p, p))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    e, T = np.empty((0, 4)), 4
    for dependent in MODES:     # no symbols, NULL inputs: counts 0, every mean, spread and summary statistic NULL, n_days 0
        exp = D.groups(e, e, e, 2, 3, dependent)
        out = {"mean_return": (6, T), "count": (6, T), "turnover": (6, T), "spread_factor": (3, T), "spread_control": (4, T),
               "summary": (13, 5)}
        out = {k: torch.full(s, 7, dtype=torch.int32 if k == "count" else torch.float64, device="cuda") for k, s in out.items()}
        bt = Batch(0, T, T)
        status(lib().pq_factor_double_sort(api.ctx(), C.byref(bt), None, None, None, C.c_int32(2), C.c_int32(3),
                                           C.c_int32(int(dependent)), None, *[C.c_void_p(t.data_ptr()) for t in out.values()]))
        torch.cuda.synchronize()
        for k in exp:
            if k != "labels":
                same(k, out[k].cpu().numpy(), exp[k])
        same("summary", out["summary"].cpu().numpy(), D.summary(exp))
        assert bool((out["count"] == 0).all()) and bool((out["summary"][:, 0] == 0).all())
