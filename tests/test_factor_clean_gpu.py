"""-m gpu: per-day factor cleaning (D-16, csrc/xsec/clean.hip) against the numpy restatement in tests/xsec_clean_ref.py.  Every
comparison is bitwise.  The size regressor is log(cap) taken on the device by torch; the restatement is handed the same z."""
import ctypes as C
import itertools

import numpy as np
import pytest

import xsec_clean_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = [None, "mad", "sigma", "percentile"]
SHAPES = [(37, 50), (300, 131), (1, 5), (2, 3)]
COMBOS = list(itertools.product(MODES, (False, True), (False, True), (False, True)))   # winsorize, cap, industry, standardize


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def same(name, got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def make(kind, n, T, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, T)) * 3.0 + 0.25
    f[rng.random((n, T)) < 0.02] *= 40.0                       # outliers for the winsorizers
    cap = np.exp(rng.standard_normal((n, T)) * 1.5 + 10.0)
    ind = rng.integers(0, 6, n)                                  # a [N] vector, broadcast over days
    if kind == "special":        # NULL / NaN / +-inf factors, non-positive and NULL caps, negative codes, a constant day, a day of one
        f[rng.random((n, T)) < 0.05] = R.NULL
        f[rng.random((n, T)) < 0.03] = np.nan
        f[rng.random((n, T)) < 0.02] = np.inf
        f[rng.random((n, T)) < 0.02] = -np.inf
        cap[rng.random((n, T)) < 0.03] = 0.0
        cap[rng.random((n, T)) < 0.03] = -5.0
        cap[rng.random((n, T)) < 0.03] = R.NULL
        ind = rng.integers(-1, 6, (n, T))                        # [N, T] codes, some unclassified
        if T >= 3:
            f[:, 0] = 1.25
            f[1:, 1] = R.NULL
    elif kind == "discrete":     # tie runs of about n / 4, signed zeros
        f = rng.integers(-2, 2, (n, T)).astype(np.float64)
        f[(f == 0) & (rng.random((n, T)) < 0.5)] = -0.0
        cap = np.round(cap, -4) + 1.0
    return f, cap, ind


def to_dev(a, pitch=None, dtype=torch.float64):
    n, T = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if pitch is None:
        return t.cuda()
    buf = torch.full((n, pitch), 7, dtype=dtype, device="cuda")
    buf[:, :T] = t.cuda()
    return buf[:, :T]


def check(pq, f, cap, ind, mode, use_cap, use_ind, stdz, pitch=None, wn=None):
    from polars_quant_amd import api
    fd = to_dev(f, pitch)
    cd = to_dev(cap, pitch) if use_cap else None
    got = api.factor_clean(fd, mode, wn, cd, True, ind if use_ind else None, stdz)
    z = torch.log(cd).cpu().numpy() if use_cap else None
    exp = R.clean(f, mode, wn, z, ind if use_ind else None, None, stdz)
    same(f"clean {mode} cap={use_cap} ind={use_ind} std={stdz} {f.shape} wn={wn} pitch={pitch}", got.cpu().numpy(), exp)
    return got


@pytest.mark.parametrize("kind", ["plain", "special", "discrete"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_every_combination_bitwise(pq, shape, kind):
    n, T = shape
    f, cap, ind = make(kind, n, T, 31 + n + T)
    for mode, use_cap, use_ind, stdz in COMBOS:
        check(pq, f, cap, ind, mode, use_cap, use_ind, stdz)


def test_winsorize_n_values(pq):
    f, cap, ind = make("special", 300, 131, 8)
    for mode, wn in (("mad", 0.0), ("mad", 1.0), ("sigma", 0.5), ("sigma", 0.0), ("percentile", 0.0), ("percentile", 10.0),
                     ("percentile", 49.5)):
        check(pq, f, cap, ind, mode, False, False, False, wn=wn)
        check(pq, f, cap, ind, mode, True, True, True, wn=wn)


def test_odd_row_pitch(pq):
    """batch stride > len (and odd): inputs read and the output written at the inputs' pitch"""
    f, cap, ind = make("special", 300, 131, 5)
    for mode in MODES:
        got = check(pq, f, cap, ind, mode, True, True, True, pitch=139)
        check(pq, f, cap, ind, mode, False, True, False, pitch=139)
    assert got.stride(0) == 139


def test_heavily_discrete_factor_long_tie_runs(pq):
    """a four-valued factor over 3 000 symbols: tie runs of about 750 per day, MAD often 0 or 1"""
    rng = np.random.default_rng(3)
    f = rng.integers(-2, 2, (3000, 24)).astype(np.float64)
    f[f == 0] = np.where(rng.random(int((f == 0).sum())) < 0.5, -0.0, 0.0)
    f[:, 5] = np.where(rng.random(3000) < 0.9, 1.0, 2.0)        # MAD 0: not clipped
    cap = np.exp(rng.standard_normal((3000, 24)))
    ind = rng.integers(0, 31, 3000)
    for mode in MODES:
        check(pq, f, cap, ind, mode, False, False, False)
        check(pq, f, cap, ind, mode, True, True, True)


def test_many_industries(pq):
    """G = 256 (the LDS limit of the industry pass) and a single-member industry"""
    rng = np.random.default_rng(9)
    n, T = 700, 40
    f = rng.standard_normal((n, T))
    cap = np.exp(rng.standard_normal((n, T)))
    ind = rng.integers(0, 255, n)
    ind[17] = 255
    got = check(pq, f, cap, ind, "mad", True, True, False)
    assert (got[17].cpu().numpy() == 0.0).all()
    check(pq, f, cap, ind, "sigma", False, True, True)


@pytest.mark.parametrize("n", [16385, 20000])
def test_wide_cross_section_segmented_sort(pq, n):
    """n_series > 16384: mad / percentile bounds from rocPRIM's segmented sort, with ties, signed zeros and NULLs"""
    rng = np.random.default_rng(n)
    T = 7
    f = rng.standard_normal((n, T))
    f[:, 1] = np.round(f[:, 1] * 2.0) / 2.0
    f[:, 2] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    f[rng.random((n, T)) < 0.02] = R.NULL
    cap = np.exp(rng.standard_normal((n, T)))
    ind = rng.integers(0, 31, n)
    for mode in ("mad", "percentile"):
        check(pq, f, cap, ind, mode, False, False, False)
        check(pq, f, cap, ind, mode, True, True, True)
    check(pq, f, cap, ind, "percentile", False, False, False, wn=20.0)


def test_out_aliases_factor(pq):
    """pq_factor_clean(out = factor): cleaned in place, same bits as into a fresh column"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    f, cap, ind = make("special", 300, 131, 12)
    exp = R.clean(f, "mad", None, torch.log(to_dev(cap)).cpu().numpy(), ind, 6, True)
    fd, zd = to_dev(f), torch.log(to_dev(cap))
    idd = to_dev(ind, dtype=torch.int32)
    vp = C.c_void_p
    b = Batch(300, 131, 131)
    ok(lib().pq_factor_clean(api.ctx(), C.byref(b), vp(fd.data_ptr()), C.c_int32(1), C.c_double(3.0), vp(zd.data_ptr()),
                             vp(idd.data_ptr()), C.c_int32(6), C.c_int32(1), vp(fd.data_ptr())))
    same("in place", fd.cpu().numpy(), exp)


def test_top_level_clean(pq):
    f, cap, ind = make("plain", 300, 131, 21)
    z = torch.log(to_dev(cap)).cpu().numpy()
    got = pq.clean(f, winsorize="mad", neutralize_market_cap=True, cap=cap, neutralize_industry=True, industry=ind, standardize=True)
    same("pq.clean full", got.cpu().numpy(), R.clean(f, "mad", None, z, ind, None, True))
    got = pq.clean(f, winsorize="sigma", winsorize_n=2.0, cap=cap, industry=ind)     # arrays without the switches are not used
    same("pq.clean sigma", got.cpu().numpy(), R.clean(f, "sigma", 2.0))
    got = pq.clean(f, neutralize_market_cap=True, cap=cap, log_cap=False)
    same("pq.clean linear cap", got.cpu().numpy(), R.clean(f, None, None, cap))


def test_config4_full_size(pq):
    """10 000 x 5 040, mad + log cap + 31 industries + standardize: 10 days bitwise, and mean 0 / std 1 on every live day"""
    from polars_quant_amd import api
    N, T = 10000, 5040
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    f = torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g)
    f[torch.rand((N, T), device="cuda", generator=g) < 0.01] = float("nan")
    cap = torch.exp(torch.randn((N, T), dtype=torch.float64, device="cuda", generator=g) + 10.0)
    ind = torch.randint(0, 31, (N,), device="cuda", generator=g)
    out = api.factor_clean(f, "mad", None, cap, True, ind, True)
    days = [0, 1, 777, 1500, 2519, 2520, 3333, 4000, 5038, 5039]
    exp = R.clean(f[:, days].cpu().numpy(), "mad", None, torch.log(cap[:, days]).cpu().numpy(), ind.cpu().numpy(), None, True)
    same("config 4 sampled days", out[:, days].cpu().numpy(), exp)
    live = ~torch.isnan(out)
    n = live.sum(0).double()
    m = torch.where(live, out, 0.0).sum(0) / n
    assert float(m.abs().max()) < 1e-12
    v = torch.where(live, (out - m) ** 2, 0.0).sum(0) / (n - 1)
    assert float((v - 1.0).abs().max()) < 1e-10


def test_argument_errors_launch_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check as ok, lib
    L = lib()
    n, T = 40, 30
    f, cap, ind = make("plain", n, T, 1)
    fd, zd, idd = to_dev(f), to_dev(cap), to_dev(np.repeat(ind[:, None], T, 1), dtype=torch.int32)
    out = torch.full((n, T), 7.0, dtype=torch.float64, device="cuda")
    h = api.ctx()
    vp = C.c_void_p
    b = Batch(n, T, T)

    def call(bb, mode, wn, z, i, G, std):
        ok(L.pq_factor_clean(h, C.byref(bb), vp(fd.data_ptr()), C.c_int32(mode), C.c_double(wn), z, i, C.c_int32(G), C.c_int32(std),
                             vp(out.data_ptr())))

    zp, ip = vp(zd.data_ptr()), vp(idd.data_ptr())
    for args, msg in (((4, 3.0, None, None, 0, 0), "winsorize"), ((-1, 3.0, None, None, 0, 0), "winsorize"),
                      ((3, 50.0, None, None, 0, 0), "percentile"), ((3, -0.5, None, None, 0, 0), "percentile"),
                      ((1, -1.0, None, None, 0, 0), "winsorize_n"), ((2, float("inf"), None, None, 0, 0), "winsorize_n"),
                      ((0, 0.0, zp, ip, 0, 0), "n_industries"), ((0, 0.0, zp, ip, 257, 0), "n_industries"),
                      ((0, 0.0, None, None, 0, 2), "standardize")):
        with pytest.raises(pq.PqError, match=msg):
            call(b, *args)
    ok(L.pq_suite_begin(h, C.byref(b)))
    try:
        with pytest.raises(pq.PqError, match="recorded"):
            call(b, 1, 3.0, zp, ip, 6, 1)
    finally:
        ok(L.pq_suite_abort(h))
    off = torch.tensor([0, 10, 25, n * T], dtype=torch.int64, device="cuda")
    rb = Batch(3, n * T - 25, n * T, vp(off.data_ptr()))
    with pytest.raises(pq.PqError, match="ragged"):
        call(rb, 1, 3.0, None, None, 0, 0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "out was written by a refused call"
    check(pq, f, cap, ind, "mad", True, True, True)   # the context computes again after the refusals
