"""-m gpu: the group (industry) codes argument of the five entry points that take one -- pq_factor_weighted, pq_ic_subgroup,
pq_xsec_regress_wls, pq_risk_portfolio and pq_factor_clean -- through the raw C entries: [N] codes (pitch 0) against the same codes
spread to [N, T] on the batch's pitch bit for bit, a code of -1 against a code of G (both unclassified), and the refusals of a bad
n_groups or group_stride with their status and text.  N = 3, T = 5, and N = 300 so that two 256-symbol blocks are crossed."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G, K = 3, 1
SHAPES = [(3, 5), (300, 5)]
ENTRIES = ["factor_weighted", "ic_subgroup", "ic_subgroup_rank", "xsec_regress_wls", "risk_portfolio", "factor_clean", "factor_clean_mad"]
I_SENT, F_SENT = -5, 7.0      # what the output buffers hold before a call


@pytest.fixture(scope="module")
def pq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_quant_amd as pq
    from polars_quant_amd._lib import lib
    lib()  # fail loudly if the HIP library is missing
    return pq


@functools.lru_cache(maxsize=None)
def panel(N, T):
    """random columns (computed once, shared, never changed) and random [N] codes 0 .. G - 1 with every third symbol unclassified (-1)"""
    rng = np.random.default_rng(100 * N + T)
    cols = {k: rng.standard_normal((N, T)) for k in ("x", "y", "f")}
    cols["w"] = rng.uniform(0.5, 2.0, (N, T))
    cols["sv"] = rng.uniform(0.01, 0.04, (N, T))
    a = rng.standard_normal((T, K + G, K + G))
    cols["cov"] = a @ a.transpose(0, 2, 1)
    codes = rng.integers(0, G, N).astype(np.int32)
    codes[1::3] = -1
    for a in (*cols.values(), codes):
        a.setflags(write=False)
    return cols, codes


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=dtype)       # (a copy: the shared panel is read-only)


def run(entry, N, T, codes, gs=None, n_groups=G, checked=True):
    """one raw call of pq_<entry> on panel(N, T) with int32 `codes` ([N], [N, T] or None) -> (status, dict of host outputs); gs
    overrides the pitch that the codes' shape implies"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    c, _ = panel(N, T)
    x, y, f, w, sv, cov = (dev(c[k]) for k in ("x", "y", "f", "w", "sv", "cov"))
    g = None if codes is None else dev(codes, torch.int32)
    if gs is None:
        gs = T if g is not None and g.dim() == 2 else 0
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    b, d = Batch(N, T, T), x.device
    ptrs = (C.c_void_p * K)(f.data_ptr())
    if entry == "factor_weighted":
        out = {"out": torch.full((N, T), F_SENT, **f64)}
        s = api._call("pq_factor_weighted", d, b, x, w, g, gs, n_groups, out["out"], checked=False)
    elif entry in ("factor_clean", "factor_clean_mad"):     # no stride parameter: the codes lie on the batch's.  mad: the sorted path,
        out = {"out": torch.full((N, T), F_SENT, **f64)}    # whose key kernel reads the codes too
        mode, wn = (1, 3.0) if entry == "factor_clean_mad" else (0, 0.0)
        s = api._call("pq_factor_clean", d, b, x, mode, wn, None, g, n_groups, 0, out["out"], checked=False)
    elif entry in ("ic_subgroup", "ic_subgroup_rank"):      # Pearson IC and Rank-IC: two sets of kernels read the codes
        V = max(1, min(n_groups, 256))
        out = {"ic": torch.full((V, T), F_SENT, **f64), "n": torch.full((V, T), I_SENT, **i32), "summary": torch.full((V, 5), F_SENT, **f64)}
        method = 1 if entry == "ic_subgroup_rank" else 0
        s = api._call("pq_ic_subgroup", d, b, x, y, g, gs, n_groups, method, out["ic"], out["n"], out["summary"], checked=False)
    elif entry == "xsec_regress_wls":
        rows = K + max(1, min(n_groups, 256))
        out = {"coef": torch.full((rows, T), F_SENT, **f64), "t": torch.full((rows, T), F_SENT, **f64), "p": torch.full((rows, T), F_SENT, **f64),
               "r2": torch.full((2, T), F_SENT, **f64), "n": torch.full((T,), I_SENT, **i32), "gt": torch.full((T,), I_SENT, **i32),
               "resid": torch.full((N, T), F_SENT, **f64), "summary": torch.full((rows, 5), F_SENT, **f64)}
        s = api._call("pq_xsec_regress_wls", d, b, ptrs, K, y, w, g, gs, n_groups, *out.values(), checked=False)
    else:
        M = K + max(1, min(n_groups, 256))
        if M != K + G:
            cov = torch.zeros((T, M, M), **f64)
        out = {"exposure": torch.full((M, T), F_SENT, **f64), "contribution": torch.full((M, T), F_SENT, **f64),
               "risk": torch.full((4, T), F_SENT, **f64), "n": torch.full((2, T), I_SENT, **i32)}
        s = api._call("pq_risk_portfolio", d, b, x, ptrs, K, g, gs, n_groups, cov, sv, T, 0, 1, T, *out.values(), checked=False)
    torch.cuda.synchronize()
    if checked:
        assert s == 0, (entry, s, last_error())
    return s, {k: v.cpu().numpy() for k, v in out.items()}


def last_error():
    from polars_quant_amd._lib import lib
    return lib().pq_last_error().decode()


def same(tag, a, b):
    for k in a:
        ga = a[k] if a[k].dtype == np.int32 else a[k].view(np.uint64)
        gb = b[k] if b[k].dtype == np.int32 else b[k].view(np.uint64)
        assert (ga == gb).all(), f"{tag}: {k} differs in {int((ga != gb).sum())} cells"


@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_codes_per_symbol_and_per_cell_agree(pq, entry, N, T):
    _, codes = panel(N, T)
    spread = np.repeat(codes[:, None], T, axis=1)
    _, b = run(entry, N, T, spread)
    if not entry.startswith("factor_clean"):   # pq_factor_clean only takes [N, T] codes; the spread ones are compared with -1 -> G below
        _, a = run(entry, N, T, codes)
        same(f"{entry} [N] vs [N, T]", a, b)
    assert all(not (v == (I_SENT if v.dtype == np.int32 else F_SENT)).any() for v in b.values()), f"{entry}: an output cell was not written"


@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_codes_outside_the_range_are_unclassified(pq, entry, N, T):
    c, codes = panel(N, T)
    out_lo = codes < 0
    hi = np.where(out_lo, G, codes).astype(np.int32)                        # every -1 -> G
    mix = np.where(out_lo & (np.arange(N) % 2 == 0), G, codes).astype(np.int32)
    shape = (lambda g: np.repeat(g[:, None], T, axis=1)) if entry.startswith("factor_clean") else (lambda g: g)
    _, a = run(entry, N, T, shape(codes))
    for tag, other in (("G", hi), ("-1 and G", mix)):
        _, o = run(entry, N, T, shape(other))
        same(f"{entry} -1 vs {tag}", a, o)
    # and unclassified means outside the sample
    if entry in ("factor_weighted", "factor_clean", "factor_clean_mad"):
        assert np.isnan(a["out"][out_lo]).all() and not np.isnan(a["out"][~out_lo]).any()
    elif entry == "xsec_regress_wls":
        assert np.isnan(a["resid"][out_lo]).all() and (a["n"] == int((~out_lo).sum())).all()
    elif entry in ("ic_subgroup", "ic_subgroup_rank"):
        assert (a["n"].sum(axis=0) == int((~out_lo).sum())).all()
    else:
        assert (a["n"][0] == N).all() and (a["n"][1] == int(out_lo.sum())).all()       # held, uncovered


REFUSALS = {    # entry -> [(arguments of run, substring of the message)]; every status is PQ_ERR_ARG
    "factor_weighted": [(dict(n_groups=0), "n_groups must be in [1, 256]"), (dict(n_groups=257), "n_groups must be in [1, 256]"),
                        (dict(gs="len-1"), "group_stride"), (dict(gs=-1), "group_stride")],
    "factor_clean": [(dict(n_groups=0), "n_industries must be in [1, 256]"), (dict(n_groups=257), "n_industries must be in [1, 256]")],
    "ic_subgroup": [(dict(n_groups=0), "n_groups must be in [1, 256]"), (dict(n_groups=257), "n_groups must be in [1, 256]"),
                    (dict(gs="len-1"), "group_stride"), (dict(gs=-1), "group_stride")],
    "xsec_regress_wls": [(dict(n_groups=0), "n_groups must be in [1, 256]"), (dict(n_groups=257), "n_groups must be in [1, 256]"),
                         (dict(gs="len-1"), "group_stride"), (dict(gs=-1), "group_stride"),
                         (dict(codes=None, n_groups=2), "n_groups must be 1")],
    "risk_portfolio": [(dict(n_groups=0), "n_groups must be in [1, 256]"), (dict(n_groups=257), "n_groups must be in [1, 256]"),
                       (dict(gs="len-1"), "group_stride"), (dict(gs=-1), "group_stride"),
                       (dict(codes=None, n_groups=2), "n_groups must be 1")],
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals(pq, entry):
    N, T = SHAPES[0]
    _, codes = panel(N, T)
    spread = np.repeat(codes[:, None], T, axis=1)
    for kw, msg in REFUSALS[{"ic_subgroup_rank": "ic_subgroup", "factor_clean_mad": "factor_clean"}.get(entry, entry)]:
        kw = dict(kw)
        if kw.get("gs") == "len-1":
            kw["gs"] = T - 1
        kw.setdefault("codes", spread)
        s, out = run(entry, N, T, checked=False, **kw)
        err = last_error()
        assert s == 1 and msg in err, (entry, kw.keys(), s, err)                    # PQ_ERR_ARG
        assert all((v == (I_SENT if v.dtype == np.int32 else F_SENT)).all() for v in out.values()), f"{entry}: a refused call wrote"
    if entry in ("factor_weighted", "factor_clean", "factor_clean_mad"):            # without codes the count is ignored
        s, _ = run(entry, N, T, None, n_groups=300, checked=False)
        assert s == 0, (entry, s, last_error())
