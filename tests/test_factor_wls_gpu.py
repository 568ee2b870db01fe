"""-m gpu: the weighted cross-sectional regression with industry dummies of D-32 (csrc/xsec/wls.hip) against the numpy restatement in
tests/xsec_wls_ref.py.  coef / t / both R^2 / n / G_t / resid and the Fama-MacBeth n_days / mean / std / t are compared bit for bit;
p-values against scipy.special.stdtr within |dp| <= 1e-11 p + 1e-300 (D-17's bound).  Also: pq_xsec_regress bit for bit under unit
weights and one group, the invariances on the device, the constructed NULL-rule days at the lanes 0, 63 and 64, the refusals of the C
entry point, empty batches, and the Factor methods' views."""
import ctypes as C
import functools

import numpy as np
import pytest

import xsec_wls_cases as cases
import xsec_wls_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 7.0
TAIL = 16


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


def same(name, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    g = got.astype(np.float64).view(np.uint64) if got.dtype != np.int32 else got
    e = exp.astype(np.float64).view(np.uint64) if exp.dtype != np.int32 else exp.astype(np.int32)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def close_p(name, got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, name
    gn, en = np.isnan(got), np.isnan(exp)
    assert (gn == en).all(), f"{name}: NaN / NULL pattern differs"
    assert (R.isnull(got) == R.isnull(exp)).all(), f"{name}: NULL pattern differs"
    g, e = got[~gn], exp[~en]
    err = np.abs(g - e) - (1e-11 * e + 1e-300)
    assert (err <= 0).all(), f"{name}: worst |dp| excess {err.max()!r}"


def to_dev(a, pitch=None):
    a = np.array(a, dtype=np.float64)                       # (a copy: the shared cases are read-only)
    if pitch is None:
        return torch.from_numpy(a).cuda()
    n, T = a.shape
    buf = torch.full((n, pitch), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(a).cuda()
    return buf[:, :T]


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(K, G, N, T, codes="2d", weights=True, holes=0.03, seed=0):
    """one random panel and its restatement (computed once, shared, never changed)"""
    F, r, w, ind = cases.panel(K, N, T, G, 1000 * K + 7 * G + N + T + seed, holes=holes, weights=weights, codes=codes)
    exp = R.wls(list(F), r, w, ind, G)
    for a in (F, r, w, ind, *exp.values()):
        if a is not None:
            a.setflags(write=False)
    return F, r, w, ind, exp


def wls_raw(F, r, w, ind, G, pitch=None, gpitch=None, resid=True, summary=True):
    """pq_xsec_regress_wls through the one call path of the package, on buffers prefilled with a sentinel and TAIL cells longer than
    what the call may write -> dict of host arrays; asserts that nothing beyond was written"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    K, N, T = F.shape
    stride = pitch or T
    cols = [to_dev(f, pitch) for f in F]
    rd, wd = to_dev(r, pitch), (None if w is None else to_dev(w, pitch))
    gd, gs = None, 0
    if ind is not None and ind.ndim == 1:
        gd = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    elif ind is not None:
        gs = gpitch or stride
        gd = torch.full((N, gs), 3, dtype=torch.int32, device="cuda")
        gd[:, :T] = torch.from_numpy(np.array(ind, dtype=np.int32)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    rows = K + G
    coef, t, p = (torch.full((rows * T + TAIL,), SENTINEL, **f64) for _ in range(3))
    r2 = torch.full((2 * T + TAIL,), SENTINEL, **f64)
    n, gt = (torch.full((T + TAIL,), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    res = torch.full((N * stride + TAIL,), SENTINEL, **f64) if resid else None
    summ = torch.full((rows * 5 + TAIL,), SENTINEL, **f64) if summary else None
    ptrs = (C.c_void_p * K)(*[c.data_ptr() for c in cols])
    api._call("pq_xsec_regress_wls", rd.device, Batch(N, T, stride), ptrs, K, rd, wd, gd, gs, G, coef, t, p, r2, n, gt, res, summ)
    torch.cuda.synchronize()
    out = {"coef": host(coef[:rows * T]).reshape(rows, T), "t": host(t[:rows * T]).reshape(rows, T),
           "p": host(p[:rows * T]).reshape(rows, T), "r2": host(r2[:2 * T]).reshape(2, T), "n": host(n[:T]), "gt": host(gt[:T])}
    for name, buf, used in (("coef", coef, rows * T), ("t", t, rows * T), ("p", p, rows * T), ("r2", r2, 2 * T)):
        assert bool((buf[used:] == SENTINEL).all()), f"{name}: written beyond its end"
    assert bool((n[T:] == 77).all()) and bool((gt[T:] == 77).all()), "n / G_t: written beyond len"
    if resid:
        grid = res[:N * stride].reshape(N, stride)
        out["resid"] = host(grid[:, :T])
        assert bool((grid[:, T:] == SENTINEL).all()) and bool((res[N * stride:] == SENTINEL).all()), "resid: written beyond len"
    if summary:
        out["summary"] = host(summ[:rows * 5]).reshape(rows, 5)
        assert bool((summ[rows * 5:] == SENTINEL).all()), "summary: written beyond its end"
    return out


def check(tag, got, exp, T):
    """got: host arrays under the restatement's keys (+ "summary")"""
    assert exp["ok"].sum() >= min(3, T), f"{tag}: only {exp['ok'].sum()} solved days in the restatement"
    for k in ("coef", "t", "r2", "n", "gt"):
        same(f"{k} {tag}", got[k], exp[k])
    close_p(f"p {tag}", got["p"], exp["p"])
    if "resid" in got:
        same(f"resid {tag}", got["resid"], exp["resid"])
    if "summary" in got:
        es = R.fm_summary(exp["coef"])
        same(f"summary {tag}", got["summary"][:, :4], es[:, :4])
        close_p(f"summary p {tag}", got["summary"][:, 4], es[:, 4])


def from_api(out):
    got = {"coef": host(out["coef"]), "t": host(out["t_stat"]), "p": host(out["p_value"]),
           "r2": np.stack([host(out["r_squared"]), host(out["r_squared_within"])]), "n": host(out["n"]), "gt": host(out["n_industries"])}
    if "resid" in out:
        got["resid"] = host(out["resid"])
    if "summary" in out:
        got["summary"] = host(out["summary"])
    return got


# ---------------------------------------------------------------- every N and T class, through the Python entry
SWEEP = [(N, T) for N in (7, 256, 257, 513) for T in (1, 64, 65, 130)]


@pytest.mark.parametrize("N,T", SWEEP, ids=[f"{N}x{T}" for N, T in SWEEP])
def test_every_size_class_through_api(pq, N, T):
    """N on both sides of the 256-symbol block and of two blocks, T on both sides of the 64-day workgroup; the flags alternate with the
    case.  The Python entry takes G from the codes, so the codes outside [0, G) are all -1 here (the raw cases below keep the others)."""
    from polars_quant_amd import api
    i = SWEEP.index((N, T))
    iN, iT = divmod(i, 4)
    K, G = (1, 2) if N == 7 else (3, 2)
    weights, codes, resid, summary = (iN + iT) % 2 == 0, ("2d", "1d")[iN % 2], i % 3 != 0, i % 4 != 1
    pitch = {1: 8, 64: 80, 65: 72, 130: 136}[T] if T % 2 or (iN + iT // 2) % 2 else None     # (an odd T never on its own odd pitch)
    F, r, w, ind, _ = case(K, G, N, T, codes, weights, 0.0 if N == 7 else 0.03)
    ind = np.where((ind >= 0) & (ind < G), ind, -1).astype(np.int32)
    exp = R.wls(list(F), r, w, ind)
    out = api.xsec_regress_wls([to_dev(f, pitch) for f in F], to_dev(r, pitch), None if w is None else to_dev(w, pitch),
                               torch.from_numpy(ind), summary=summary, resid=resid)
    assert ("resid" in out) == resid and ("summary" in out) == summary
    check(f"api K={K} G={G} {N}x{T} pitch={pitch} codes={codes} w={weights}", from_api(out), exp, T)


# ---------------------------------------------------------------- every K and G class, and each side of every column-chunk boundary
def n_for(K, G):
    return max(64, 2 * (K + G) + 3)


KG = [(K, G) for K in (1, 3, 8) for G in (1, 2, 31, 256)]
# wl_chunk(K + 3, G) = clamp(128 / G, 1, K + 3): at K = 8 (11 columns) the chunk changes between each of these pairs of G; 128 | 129 is
# where a one-column chunk first needs more than 64 KiB of LDS.  K = 3 (6 columns) and K = 1 (4) first split at 21 | 22 and 32 | 33.
CHUNK_EDGES = [(8, G) for G in (11, 12, 13, 14, 15, 16, 17, 18, 19, 21, 22, 25, 26, 32, 33, 42, 43, 64, 65, 128, 129)] + \
              [(3, 21), (3, 22), (1, 32), (1, 33)]


def test_the_listed_g_are_each_side_of_every_chunk_change():
    """the G listed above are each side of every change of clamp(128 / G, 1, 11), the rule in csrc/xsec/wls.hip"""
    chunk = lambda ncol, G: max(1, min(ncol, 128 // G))   # noqa: E731
    edges = sorted(G for G in range(1, 256) if chunk(11, G) != chunk(11, G + 1))
    assert edges == [11, 12, 14, 16, 18, 21, 25, 32, 42, 64]
    listed = {G for K, G in CHUNK_EDGES if K == 8}
    assert all(G in listed and G + 1 in listed for G in edges)
    assert chunk(6, 21) == 6 and chunk(6, 22) == 5 and chunk(4, 32) == 4 and chunk(4, 33) == 3


@pytest.mark.parametrize("K,G", KG, ids=[f"K{K}-G{G}" for K, G in KG])
def test_every_k_and_g_class(pq, K, G):
    """T = 65 on a pitch of 72 (two workgroups of days, the second with one live lane), [N, T] codes on a pitch of their own, weights,
    resid and summary; the codes keep values outside [0, G), INT32_MIN and INT32_MAX among them"""
    N, T = n_for(K, G), 65
    F, r, w, ind, exp = case(K, G, N, T)
    if G == 1 and K == 8:                                    # group NULL: every symbol in group 0
        ind, exp = None, R.wls(list(F), r, w, None)
    got = wls_raw(F, r, w, ind, G, pitch=72, gpitch=75)
    check(f"K={K} G={G} {N}x{T}", got, exp, T)


@pytest.mark.parametrize("K,G", CHUNK_EDGES, ids=[f"K{K}-G{G}" for K, G in CHUNK_EDGES])
def test_each_side_of_every_chunk_boundary(pq, K, G):
    """few days, [N] and [N, T] codes and weight NULL / given alternating with G; resid and summary alternate too"""
    N, T = n_for(K, G), 5
    codes, weights = ("1d", "2d")[G % 2], G % 3 != 0
    F, r, w, ind, exp = case(K, G, N, T, codes, weights, 0.01)
    got = wls_raw(F, r, w, ind, G, resid=G % 2 == 0, summary=G % 4 < 2)
    check(f"K={K} G={G} {N}x{T} codes={codes} w={weights}", got, exp, T)


# ---------------------------------------------------------------- the NULL rules at the lane edges
@pytest.mark.parametrize("rot", [0, 3, 5])
def test_null_rule_days_at_lanes_0_63_64(pq, rot):
    """the constructed days of xsec_wls_cases.put_special: three of them on the days 0, 63 and 64 (the first and last lane of a
    workgroup and the first of the next), the others on 1, 2, 3, 62; the three rotations put every kind on an edge once.  300 symbols:
    two blocks.  Exactly the short, const and collinear days lack a solution."""
    K, G, N, T = 3, 5, 300, 130
    F, r, w, ind, _ = case(K, G, N, T, seed=rot)
    F, r, w, ind = F.copy(), r.copy(), w.copy(), ind.copy()
    kinds = cases.kinds_for(K, G, True)
    kinds = kinds[rot:] + kinds[:rot]
    day_of = dict(zip(kinds, [0, 63, 64, 1, 2, 3, 62]))
    cases.put_special(F, r, w, ind, G, day_of, 90 + rot)
    exp = R.wls(list(F), r, w, ind, G)
    assert np.flatnonzero(~exp["ok"]).tolist() == sorted(day_of[k] for k in cases.UNSOLVED)
    t = day_of["perfect"]
    assert R.isnull(exp["t"][:, t]).all() and not R.isnull(exp["coef"][:K + 2, t]).any()
    t = day_of["empty"]
    assert exp["gt"][t] == 3 and R.isnull(exp["coef"][K + 1, t]) and not R.isnull(exp["coef"][K, t])
    got = wls_raw(F, r, w, ind, G, pitch=136)
    check(f"special days rot={rot}", got, exp, T)


# ---------------------------------------------------------------- D-17 on the device
@pytest.mark.parametrize("K", [1, 3, 8])
def test_unit_weights_and_zero_codes_equal_pq_xsec_regress(pq, K):
    """explicit all-ones weights and all-zero codes (so the new kernels run): pq_xsec_regress bit for bit, p and the summary included"""
    from polars_quant_amd import api
    N, T = 300, 131
    F, r, _, _, _ = case(K, 1, N, T, None, False)
    F, r = F.copy(), r.copy()
    F[K - 1, :, 0] = F[0, :, 0] if K > 1 else 2.5           # singular
    r[K + 1:, 1] = R.NULL                                    # n = K + 1
    cols, rd = [to_dev(f, 136) for f in F], to_dev(r, 136)
    a = api.xsec_regress(cols, rd)
    ones = torch.ones((N, 136), dtype=torch.float64, device="cuda")[:, :T]
    for codes in (torch.zeros(N, dtype=torch.int32), torch.zeros((N, T), dtype=torch.int32)):
        b = api.xsec_regress_wls(cols, rd, ones, codes)
        for k in ("coef", "t_stat", "p_value", "summary", "n"):
            same(f"{k} K={K}", host(b[k]), host(a[k]))
        same("r2", host(b["r_squared"]), host(a["r_squared"]))
        same("r2 within", host(b["r_squared_within"]), host(a["r_squared"]))
        assert R.isnull(host(b["coef"])[:, :2]).all() and (host(b["n_industries"])[2:] == 1).all()


def test_doubling_and_relabelling_on_the_device(pq):
    K, G, N, T = 3, 7, 300, 70
    F, r, w, ind, exp = case(K, G, N, T)
    a = wls_raw(F, r, w, ind, G)
    check("base", a, exp, T)
    b = wls_raw(F, r, 2.0 * w, ind, G)
    for k in ("coef", "t", "p", "r2", "n", "gt", "resid", "summary"):
        same(f"doubled {k}", b[k], a[k])
    perm = np.array([4, 2, 5, 0, 6, 3, 1])
    ind2 = np.where((ind >= 0) & (ind < G), perm[np.clip(ind, 0, G - 1)], ind).astype(np.int32)
    c = wls_raw(F, r, w, ind2, G)
    for k in ("coef", "t", "p", "summary"):
        same(f"relabelled {k}: factor rows", c[k][:K], a[k][:K])
        same(f"relabelled {k}: industry rows", c[k][K:][perm], a[k][K:])
    for k in ("r2", "n", "gt", "resid"):
        if k == "r2":
            same("relabelled r2 within", c[k][1], a[k][1])
        else:
            same(f"relabelled {k}", c[k], a[k])


# ---------------------------------------------------------------- the C entry point's refusals and empty batches
def test_refusals_write_nothing(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, lib
    L, h = lib(), api.ctx()
    K, G, N, T = 2, 3, 40, 30
    F, r, w, ind, exp = case(K, G, N, T)
    cols, rd, wd = [to_dev(f) for f in F], to_dev(r), to_dev(w)
    gd = torch.from_numpy(np.array(ind)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.full(((K + G) * T,), SENTINEL, **f64) for _ in range(3)] + [torch.full((2 * T,), SENTINEL, **f64)] + \
           [torch.full((T,), 77, dtype=torch.int32, device="cuda") for _ in range(2)] + \
           [torch.full((N * T,), SENTINEL, **f64), torch.full(((K + G) * 5,), SENTINEL, **f64)]
    b = Batch(N, T, T)

    def status(bb=b, cols_=cols, k=K, r_=rd, w_=wd, g_=gd, gs=T, G_=G, outs_=outs, ptrs=True):
        p = (C.c_void_p * max(len(cols_), 1))(*[None if c is None else c.data_ptr() for c in cols_]) if ptrs else None
        s = api._call("pq_xsec_regress_wls", rd.device, bb, p, k, r_, w_, g_, gs, G_, *outs_, checked=False)
        return s, L.pq_last_error().decode()

    bad = [(dict(k=0), "k must"), (dict(k=9), "k must"), (dict(G_=0), "n_groups"), (dict(G_=257), "n_groups"),
           (dict(g_=None, gs=0), "n_groups must be 1"), (dict(gs=T - 1), "group_stride"), (dict(gs=-1), "group_stride"),
           (dict(r_=None), "null pointer"), (dict(ptrs=False), "null pointer"), (dict(cols_=[cols[0], None]), "null factor")] + \
          [(dict(outs_=outs[:j] + [None] + outs[j + 1:]), "null output") for j in range(6)]
    for kw, msg in bad:
        s, err = status(**kw)
        assert s == 1 and msg in err, (kw.keys(), s, err)                                      # PQ_ERR_ARG
    off = torch.tensor([0, 10, 25, N * T], dtype=torch.int64, device="cuda")
    s, err = status(bb=Batch(3, N * T - 25, N * T, C.c_void_p(off.data_ptr())))
    assert s == 5 and "ragged" in err, (s, err)                                                # PQ_ERR_UNSUPPORTED
    assert L.pq_suite_begin(h, C.byref(b)) == 0
    try:
        s, err = status()
        assert s == 5 and "recorded" in err, (s, err)
    finally:
        assert L.pq_suite_abort(h) == 0
    torch.cuda.synchronize()
    assert all(bool((o == (77 if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs), "a refused call wrote"
    s, err = status()                                                                          # the context computes again
    assert s == 0, err
    torch.cuda.synchronize()
    same("coef after the refusals", host(outs[0]).reshape(K + G, T), exp["coef"])
    same("resid after the refusals", host(outs[6]).reshape(N, T), exp["resid"])


def test_empty_batches(pq):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    K = 2
    none = [None] * 8
    ptrs = (C.c_void_p * K)(None, None)
    for N in (0, 4):                                         # len == 0: PQ_OK, nothing launched, no pointer needed
        assert api._call("pq_xsec_regress_wls", torch.device("cuda", 0), Batch(N, 0, 0), ptrs, K, None, None, None, 0, 1, *none,
                         checked=False) == 0
        z = torch.empty((N, 0), dtype=torch.float64, device="cuda")
        out = api.xsec_regress_wls([z, z], z, z, np.zeros(N, dtype=np.int32), resid=True)
        assert tuple(out["coef"].shape) == (K + 1, 0) and tuple(out["resid"].shape) == (N, 0)
        s = host(out["summary"])
        assert (s[:, 0] == 0).all() and np.isnan(s[:, 1:]).all()
    # n_series == 0: every day has an empty sample
    T = 70
    z = torch.empty((0, T), dtype=torch.float64, device="cuda")
    out = api.xsec_regress_wls([z, z], z, z, torch.zeros((0, T), dtype=torch.int32), resid=True)
    assert tuple(out["resid"].shape) == (0, T)
    for k in ("coef", "t_stat", "p_value"):
        assert R.isnull(host(out[k])).all() and tuple(out[k].shape) == (K + 1, T)
    assert R.isnull(host(out["r_squared"])).all() and R.isnull(host(out["r_squared_within"])).all()
    assert (host(out["n"]) == 0).all() and (host(out["n_industries"]) == 0).all()
    s = host(out["summary"])
    assert (s[:, 0] == 0).all() and R.isnull(s[:, 1:]).all()
    got = wls_raw(np.zeros((K, 0, T)), np.zeros((0, T)), None, None, 1)
    assert R.isnull(got["coef"]).all() and (got["n"] == 0).all() and (got["gt"] == 0).all()


# ---------------------------------------------------------------- the Factor methods
def test_the_factor_methods_are_views_of_the_call(pq):
    from polars_quant_amd import api
    K, G, N, T = 3, 4, 120, 66
    F, r, w, ind, _ = case(K, G, N, T, "1d")
    ind = np.where((ind >= 0) & (ind < G), ind, -1).astype(np.int32)
    exp = R.wls(list(F), r, w, ind)
    cols, rd, wd, gd = [to_dev(f) for f in F], to_dev(r), to_dev(w), torch.from_numpy(ind)
    fac = pq.Factor()
    out = fac.pure_factor_return(cols, rd, wd, gd, specific_return=True)
    assert set(out) == {"factor_return", "t_stat", "p_value", "industry_return", "industry_t_stat", "industry_p_value", "r_squared",
                        "r_squared_within", "n", "n_industries", "summary", "specific_return"}
    same("factor_return", host(out["factor_return"]), exp["coef"][:K])
    same("industry_return", host(out["industry_return"]), exp["coef"][K:])
    same("t_stat", host(out["t_stat"]), exp["t"][:K])
    same("industry_t_stat", host(out["industry_t_stat"]), exp["t"][K:])
    close_p("p", host(out["p_value"]), exp["p"][:K])
    close_p("industry p", host(out["industry_p_value"]), exp["p"][K:])
    same("r2", np.stack([host(out["r_squared"]), host(out["r_squared_within"])]), exp["r2"])
    same("specific_return", host(out["specific_return"]), exp["resid"])
    es = R.fm_summary(exp["coef"])
    assert set(out["summary"]) == {"factor", "industry"}
    for part, rows in (("factor", es[:K]), ("industry", es[K:])):
        s = out["summary"][part]
        same(f"summary {part}", np.stack([host(s[k]) for k in ("n_days", "mean_coef", "std_coef", "t_stat")], axis=1), rows[:, :4])
        close_p(f"summary p {part}", host(s["p_value"]), rows[:, 4])
    # without industries: the group's row is the intercept
    exp1 = R.wls(list(F), r, w, None)
    out = fac.pure_factor_return(torch.stack(cols), rd, wd)
    assert "specific_return" not in out and "industry_return" not in out and set(out["summary"]) == {"factor", "intercept"}
    same("intercept", host(out["intercept"]), exp1["coef"][K])
    same("intercept t", host(out["intercept_t_stat"]), exp1["t"][K])
    same("factor_return", host(out["factor_return"]), exp1["coef"][:K])
    assert tuple(out["summary"]["intercept"]["mean_coef"].shape) == (1,)
    # and the summary of a weighted call is the Fama-MacBeth summary of its daily rows
    same("api summary", host(api.xsec_regress_wls(cols, rd, wd, gd)["summary"])[:, :4], es[:, :4])
