"""-m gpu: multi-factor orthogonalization and neutralization of D-19 (csrc/xsec/orth.hip, Factor().clean(factors, method)) against the
numpy restatement in tests/xsec_orth_ref.py, bit for bit; the in-place form against the out-of-place one; cross-checks through the D-17
regression (the residuals carry no loading on their regressors; the last level is D-17 bit for bit) and the D-16 size neutralization
(bit identity)."""
import numpy as np
import pytest

import xsec_orth_ref as O
from xsec_clean_ref import bsum

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = [2, 3, 5, 8]
SHAPES = [(1, 5), (2, 3), (None, 7), (257, 40), (300, 131), (600, 20)]   # None: K + 2 symbols


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
    g, e = got.view(np.uint64), exp.view(np.uint64)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{name}: {len(bad)} cells differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}"


def to_dev(a, pitch=None):
    """[.., N, T] numpy -> device tensor, on a row pitch of `pitch` elements (padding filled with 7.0) when given"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if pitch is None:
        return torch.from_numpy(a).cuda()
    buf = torch.full(a.shape[:-1] + (pitch,), 7.0, dtype=torch.float64, device="cuda")
    buf[..., :a.shape[-1]] = torch.from_numpy(a).cuda()
    return buf[..., :a.shape[-1]]


def make(K, n, T, seed, special=True):
    """K correlated factors [K, n, T]; special: NULL / NaN / inf holes, and (where the shape allows) a singular day (collinear regressors;
    f_0 constant at K = 2), a day where f_0 is constant, a day where the last factor is constant, an all-NULL day, a day with only K + 1
    members and one with K"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, n, T))
    for k in range(1, K):
        F[k] += 0.5 * F[k - 1]
    if special:
        F[rng.random((K, n, T)) < 0.03] = O.NULL
        F[rng.random((K, n, T)) < 0.02] = np.nan
        F[rng.random((K, n, T)) < 0.01] = np.inf
        F[rng.random((K, n, T)) < 0.01] = -np.inf
        if T >= 7 and n >= K + 3:
            if K >= 3:
                F[1, :, 0] = 2.0 * F[0, :, 0] + 3.0                     # singular block from level 2 on
            else:
                F[0, :, 0] = 2.5
            F[0, :, 1] = 0.375                                          # constant f_0: every level singular
            F[K - 1, :, 2] = 0.375                                      # constant last factor: residual ~ 0
            F[:, :, 3] = O.NULL                                         # all-NULL day
            F[0, K + 1:, 4] = O.NULL                                    # n <= K + 1
            F[0, K:, 5] = O.NULL                                        # n <= K: the last level is NULL
    return F


def check(pq, F, method, pitch=None):
    fac = pq.Factor()
    got = fac.clean(to_dev(F, pitch) if pitch else [to_dev(f) for f in F], method=method)
    exp = O.clean_full(F, method)
    same(f"{method} K={F.shape[0]} {F.shape[1:]} pitch={pitch}", got.cpu().numpy(), exp)
    return got, exp


@pytest.mark.parametrize("method", O.MODES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0] or 'K+2'}x{s[1]}")
def test_clean_bitwise(pq, shape, K, method):
    n, T = shape
    n = K + 2 if n is None else n
    F = make(K, n, T, 1000 * K + 7 * n + T)
    got, exp = check(pq, F, method)
    if T >= 7 and n >= K + 3:    # the forced days really are what they claim
        e = exp[1:] if method == "orthogonalize" else exp
        assert O.isnull(e[:, :, 1]).all() and O.isnull(e[:, :, 3]).all()
        if method == "orthogonalize" and K >= 3:
            assert O.isnull(e[1:, :, 0]).all()
        if method == "orthogonalize":
            assert O.isnull(e[K - 2, :, 5]).all()


@pytest.mark.parametrize("method", O.MODES)
@pytest.mark.parametrize("K", [3, 8])
def test_odd_pitch_and_clean_data(pq, K, method):
    check(pq, make(K, 41, 77, 3 + K, special=False), method, pitch=83)
    check(pq, make(K, 300, 131, 5 + K), method, pitch=139)


@pytest.mark.parametrize("K", [2, 3, 8])
def test_inplace_matches_out_of_place(pq, K):
    F = make(K, 300, 131, 40 + K)
    fac = pq.Factor()
    for pitch in (None, 137):
        X = to_dev(F, pitch)
        ref = fac.clean(X.clone(), method="orthogonalize").cpu().numpy()
        got = fac.clean(X, method="orthogonalize", inplace=True)
        assert got is X
        same(f"in place K={K} pitch={pitch}", X.cpu().numpy(), ref)
        same(f"in place row 0 K={K}", X[0].cpu().numpy(), F[0])
        same(f"in place vs restatement K={K}", X.cpu().numpy(), O.clean_full(F))
    with pytest.raises(ValueError):
        fac.clean(to_dev(F).float(), inplace=True)
    with pytest.raises(ValueError):
        fac.clean(to_dev(F).transpose(1, 2), inplace=True)


def test_residuals_have_no_loading_on_their_regressors(pq):
    """Factor.fama_macbeth(f_0 .. f_{k-1}, e_k): every daily slope ~ 0, at a tolerance scaled by the data"""
    K = 5
    F = make(K, 600, 20, 99)
    fac = pq.Factor()
    X = to_dev(F)
    e = fac.clean(X, method="orthogonalize")
    nz = fac.clean(X, method="neutralize")
    for k in range(1, K):
        for res, regs in ((e[k], [X[j] for j in range(k)]), (nz[k - 1], [X[0]])):
            fm = fac.fama_macbeth(regs, res)
            coef = fm["daily"]["coef"][:len(regs)].cpu().numpy()
            r = res.cpu().numpy()
            scale = np.nanmax(np.abs(np.where(O.valid(r), r, np.nan)))
            ok = ~np.isnan(coef)
            assert ok.sum() >= 10 * len(regs)
            assert np.abs(coef[ok]).max() <= 1e-12 * scale, (k, len(regs), np.abs(coef[ok]).max())


def test_last_level_is_the_regression_of_the_last_factor(pq):
    """orthogonalize(K)'s last level is regress(K - 1) with r = f_{K-1}: the slopes pq_xsec_regress returns for f_3 on f_0 .. f_2, put
    through D-17's pass 3 in numpy (e = (f_3 - fbar_3) - fit, fit = 0.0; fit += b_j (f_j - fbar_j) for ascending j, the means from the
    restatement's blocked sums), are residual 3 of pq_factor_orthogonalize bit for bit on every member.  K = 4, two summation blocks."""
    from polars_quant_amd import api
    K, n, T = 4, 300, 5
    F = make(K, n, T, 321, special=False)
    holes = np.random.default_rng(322).random((K, n, T)) < 0.02
    F[holes] = np.nan
    mem = O.joint(F)
    assert holes.any(axis=0).any(axis=0).all() and (mem.sum(axis=0) > 256).all() and mem[256:].any(axis=0).all()
    coef = api.xsec_regress([to_dev(f) for f in F[:K - 1]], to_dev(F[K - 1]), summary=False)["coef"].cpu().numpy()
    assert coef.shape == (K, T) and np.isfinite(coef).all()
    dn = mem.sum(axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        fit = np.zeros((n, T))
        for j in range(K - 1):
            fit = fit + coef[j] * (F[j] - bsum(F[j], mem) / dn)
        e = (F[K - 1] - bsum(F[K - 1], mem) / dn) - fit
    got = pq.Factor().clean([to_dev(f) for f in F], method="orthogonalize").cpu().numpy()[K - 1]
    same("residual 3 on the members", got[mem], e[mem])


@pytest.mark.parametrize("K", [2, 3, 8])
def test_neutralize_is_size_neutralization(pq, K):
    """on days with n >= 3 and C[0][0] != 0, bit-identical to clean(where(joint, f_k, NaN), neutralize_market_cap=True, cap=f_0,
    log_cap=False)"""
    F = make(K, 300, 40, 7 * K)
    fac = pq.Factor()
    got = fac.clean([to_dev(f) for f in F], method="neutralize").cpu().numpy()
    mem = O.joint(F)
    exp = O.orthogonalize(F, "neutralize")
    days = ~O.isnull(exp[0]).all(axis=0)           # the days D-17 solves: n >= 3 and C[0][0] > 0
    assert days.sum() >= 30
    for k in range(1, K):
        c = pq.clean(to_dev(np.where(mem, F[k], np.nan)), neutralize_market_cap=True, cap=to_dev(F[0]), log_cap=False).cpu().numpy()
        same(f"neutralize vs clean k={k}", got[k - 1][:, days], c[:, days])


def test_empty_and_errors(pq):
    from polars_quant_amd import api
    fac = pq.Factor()
    for n, T in ((0, 5), (4, 0)):
        F = np.zeros((3, n, T))
        assert tuple(fac.clean(F).shape) == (3, n, T)
        assert tuple(fac.clean(F, method="neutralize").shape) == (2, n, T)
    X = to_dev(make(3, 20, 9, 1))
    with pytest.raises(ValueError):
        api.factor_orthogonalize(X, 0, out=[X[1]])
    with pytest.raises(ValueError):
        api.factor_orthogonalize(X, 0, out=[X[1], X[2].float()])


def test_full_size_config4_orthogonalize_k3(pq):
    """config 4 (10 000 x 5 040), K = 3, every day bit for bit (the restatement runs in slices of days)"""
    N, T, K = 10000, 5040, 3
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    Fd = torch.randn((K, N, T), dtype=torch.float64, device="cuda", generator=g)
    Fd[1] += 0.3 * Fd[0]
    Fd[2] += 0.2 * Fd[0] - 0.4 * Fd[1]
    Fd[torch.rand((K, N, T), device="cuda", generator=g) < 0.01] = float("nan")
    got = pq.Factor().clean(Fd, method="orthogonalize").cpu().numpy()
    F = Fd.cpu().numpy()
    same("row 0", got[0], F[0])
    for t0 in range(0, T, 630):
        sl = slice(t0, t0 + 630)
        same(f"residuals days {t0}", got[1:, :, sl], O.orthogonalize(F[:, :, sl]))
