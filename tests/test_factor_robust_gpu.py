"""-m gpu: the robustness tests of D-18 (csrc/xsec/robust.hip) against the restatement in tests/xsec_robust_ref.py (the CPU oracle's D-12
IC on shifted / masked arrays) and against the device's own pq_factor_ic on shifted / masked inputs.  Daily IC, n_valid and the summary's
n_days / mean / std / t are compared bit for bit; p-values against scipy.special.stdtr within |dp| <= 1e-11 p + 1e-300."""
import numpy as np
import pytest

import xsec_robust_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(37, 50), (300, 131), (2, 3), (1, 5)]
METHODS = [0, 1]


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


def same_summary(tag, got, exp):
    got = np.asarray(got)
    same(f"summary {tag}", got[:, :4], exp[:, :4])
    close_p(f"p {tag}", got[:, 4], exp[:, 4])


def to_dev(a, pitch=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1 or pitch is None:
        return torch.from_numpy(a).cuda()
    n, T = a.shape
    buf = torch.full((n, pitch), 7.0, dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(a).cuda()
    return buf[:, :T]


def make(n, T, seed, ties=False):
    """factor and return [n, T] with ~1 % NULL / NaN returns and a few invalid factor values; ties: a discretised factor"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, T))
    r = 0.05 * f + rng.standard_normal((n, T))
    if ties:
        f = np.round(f * 2.0) / 2.0
    r[rng.random((n, T)) < 0.01] = R.NULL
    r[rng.random((n, T)) < 0.005] = np.nan
    f[rng.random((n, T)) < 0.01] = R.NULL
    f[rng.random((n, T)) < 0.003] = np.inf
    return f, r


def np_(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pitch", [None, "odd"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decay_matches_shifted_ic(pq, shape, pitch, method):
    from polars_quant_amd import api
    n, T = shape
    for ties in (False, True):
        f, r = make(n, T, 100 + n + T + ties, ties)
        p = T + 3 if pitch else None
        for L in sorted({1, 2, 7, T + 2}):
            got = api.ic_decay(to_dev(f, p), to_dev(r, p), L, method)
            ic, nv, summ = R.ic_decay(f, r, L, method)
            tag = f"{shape} pitch={pitch} method={method} ties={ties} L={L}"
            same(f"ic {tag}", np_(got["ic"]), ic)
            same(f"n_valid {tag}", np_(got["n_valid"]), nv)
            same_summary(tag, np_(got["summary"]), summ)
        # row l against the device's own IC on shifted device views
        fd, rd = to_dev(f, p), to_dev(r, p)
        got = api.ic_decay(fd, rd, min(T, 7), method)
        for l in range(1, min(T, 7) + 1):
            e_ic, e_nv = api.factor_ic(fd[:, :T - l + 1], rd[:, l - 1:], method)
            same(f"shifted ic l={l}", np_(got["ic"][l - 1, :T - l + 1]), np_(e_ic))
            same(f"shifted n_valid l={l}", np_(got["n_valid"][l - 1, :T - l + 1]), np_(e_nv))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G", [1, 31, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_subgroup_matches_masked_ic(pq, shape, G, method):
    from polars_quant_amd import api
    n, T = shape
    f, r = make(n, T, 200 + n + G, ties=method == 1)
    rng = np.random.default_rng(G + n)
    for form in ("N", "NT"):
        codes = rng.integers(-2, G, (n,) if form == "N" else (n, T)).astype(np.int32)
        codes.flat[0] = G - 1                    # G is max code + 1
        for p in (None, T + 5):
            got = api.ic_subgroup(to_dev(f, p), to_dev(r, p), codes, method)
            ic, nv, summ = R.ic_subgroup(f, r, codes, method)
            tag = f"{shape} G={G} {form} pitch={p} method={method}"
            same(f"ic {tag}", np_(got["ic"]), ic)
            same(f"n_valid {tag}", np_(got["n_valid"]), nv)
            same_summary(tag, np_(got["summary"]), summ)
        full = R.group_codes(codes, f.shape)
        for g in sorted({0, G // 2, G - 1}):      # the device's own IC on the masked factor
            e_ic, e_nv = api.factor_ic(np.where(full == g, f, np.nan), r, method)
            same(f"masked ic g={g} {form}", np_(got["ic"][g]), np_(e_ic))
            same(f"masked n_valid g={g} {form}", np_(got["n_valid"][g]), np_(e_nv))


@pytest.mark.parametrize("method", ["pearson", "spearman"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_subsample_matches_slices(pq, shape, method):
    n, T = shape
    f, r = make(n, T, 300 + n + T)
    F = pq.Factor()
    ic = np_((F.ic if method == "pearson" else F.rank_ic)(f, r)[0])
    for k in sorted({1, 2, 3, T}):
        got = F.subsample_test(f, r, n_splits=k, method=method, dates=[f"d{i}" for i in range(T)])
        start, end = R.split_periods(T, k)
        exp = R.series_split_summary(ic, k)
        tag = f"{shape} {method} n_splits={k}"
        same(f"start {tag}", np_(got["start"]).astype(np.float64), start.astype(np.float64))
        same(f"end {tag}", np_(got["end"]).astype(np.float64), end.astype(np.float64))
        got_s = np.stack([np_(got[c]) for c in ("n_days", "mean_ic", "std_ic", "t_stat", "p_value")], axis=1)
        same_summary(tag, got_s, exp)
        assert got["start_date"] == [f"d{i}" for i in start] and got["end_date"] == [f"d{i}" for i in end]
        assert np_(got["period"]).tolist() == list(range(k))


@pytest.mark.parametrize("n", [16384, 16385])
def test_both_sides_of_the_lds_switch(pq, n):
    """n <= 16 384: the LDS sorts and histograms; above: pq_factor_ic per lag / per masked group"""
    from polars_quant_amd import api
    T = 4
    for method in METHODS:
        f, r = make(n, T, n + method, ties=True)
        got = api.ic_decay(to_dev(f), to_dev(r), 3, method)
        ic, nv, summ = R.ic_decay(f, r, 3, method)
        same(f"decay ic n={n} m={method}", np_(got["ic"]), ic)
        same(f"decay n_valid n={n} m={method}", np_(got["n_valid"]), nv)
        same_summary(f"decay n={n} m={method}", np_(got["summary"]), summ)
        codes = (np.arange(n) % 5 - 1).astype(np.int32)
        got = api.ic_subgroup(to_dev(f), to_dev(r), codes, method)
        ic, nv, summ = R.ic_subgroup(f, r, codes, method)
        same(f"subgroup ic n={n} m={method}", np_(got["ic"]), ic)
        same(f"subgroup n_valid n={n} m={method}", np_(got["n_valid"]), nv)
        same_summary(f"subgroup n={n} m={method}", np_(got["summary"]), summ)


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_factor_methods_known_answers(pq, method):
    """a factor equal to the return k days ahead has IC_k == 1 (to rounding) on every day that has it; a lag above T is an all-NULL
    row"""
    n, T, k = 40, 30, 4
    rng = np.random.default_rng(7)
    r = rng.standard_normal((n, T + k))
    f = r[:, k - 1:k - 1 + T].copy()
    r = r[:, :T]
    out = pq.Factor().ic_decay(f, r, max_lag=T + 2, method=method)
    ic = np_(out["daily"]["ic"])
    assert np.abs(ic[k - 1, :T - k + 1] - 1.0).max() < 1e-14
    assert R.isnull(ic[T:]).all() and (np_(out["n_days"])[T:] == 0).all()
    assert np_(out["lag"]).tolist() == list(range(1, T + 3))
    assert abs(float(np_(out["ic"])[k - 1]) - 1.0) < 1e-14
