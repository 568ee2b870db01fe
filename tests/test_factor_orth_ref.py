"""not-gpu: pins the numpy restatement of D-19 (tests/xsec_orth_ref.py) on hand-built days, against numpy.linalg.lstsq and against
D-16's size neutralization, and checks Factor().clean's argument errors (raised before any upload)."""
import numpy as np
import pytest

import xsec_clean_ref as CL
import xsec_orth_ref as O


def exact_days():
    """K = 3, N = 5: day 0 has exact dyadic residuals (e_1 = r, e_2 = s), day 1 has f_1 = 2 f_0 + 3 (e_1 = 0, e_2 NULL)"""
    f0 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    r = np.array([1.0, -2.0, 0.0, 2.0, -1.0])        # orthogonal to 1 and f0
    s = np.array([1.0, 0.0, -2.0, 0.0, 1.0])         # orthogonal to 1, f0 and r
    f1 = 3.0 + 0.5 * f0 + r
    f2 = 1.0 + f0 + f1 + s
    g0 = np.array([3.0, -1.0, 4.0, 1.0, -7.0])        # sum 0: exact means
    F = np.zeros((3, 5, 2))
    F[:, :, 0] = [f0, f1, f2]
    F[:, :, 1] = [g0, 2.0 * g0 + 3.0, np.array([1.0, 7.0, -2.0, 0.0, 5.0])]
    return F, r, s


def test_exact_residuals_and_singular_block():
    F, r, s = exact_days()
    e = O.orthogonalize(F)
    assert (e[0, :, 0] == r).all() and (e[1, :, 0] == s).all()
    assert (e[0, :, 1] == 0.0).all()                  # f_1 = 2 f_0 + 3: exact zero residual
    assert O.isnull(e[1, :, 1]).all()                 # singular block at k = 2: NULL
    full = O.clean_full(F)
    assert (full[0].view(np.uint64) == F[0].view(np.uint64)).all()
    n = O.orthogonalize(F, "neutralize")
    assert (n[0] == e[0]).all()                        # level 1 is the same regression in both modes
    assert not O.isnull(n[1, :, 1]).any()              # neutralize never regresses on f_1


@pytest.mark.parametrize("K", range(2, 9))
def test_sample_size_thresholds(K):
    """level k needs n >= k + 2: at n = K + 1 every level is solved, at n = K the last one is NULL, at n = K + 2 all again"""
    rng = np.random.default_rng(K)
    N = K + 4
    F = rng.integers(-6, 7, (K, N, 3)).astype(np.float64)
    F[0, K + 1:, 0] = O.NULL                           # n = K + 1
    F[K - 1, K:, 1] = np.nan                           # n = K
    F[1 % K, K + 2:, 2] = np.inf                       # n = K + 2
    e = O.orthogonalize(F)
    mem = O.joint(F)
    assert list(mem.sum(0)) == [K + 1, K, K + 2]
    for t in (0, 2):
        assert not O.isnull(e[:, mem[:, t], t]).any()
    assert O.isnull(e[K - 2, :, 1]).all()
    assert not O.isnull(e[:K - 2, mem[:, 1], 1]).any()
    assert O.isnull(e[:, ~mem]).all()


def random_factors(K, N, T, seed, holes=True):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, N, T))
    for k in range(1, K):
        F[k] += 0.4 * F[k - 1]                         # correlated, as real factors are
    if holes:
        F[rng.random((K, N, T)) < 0.05] = O.NULL
        F[rng.random((K, N, T)) < 0.02] = np.nan
        F[rng.random((K, N, T)) < 0.01] = -np.inf
    return F


@pytest.mark.parametrize("K", range(2, 9))
def test_against_lstsq_and_orthogonal(K):
    F = random_factors(K, 300, 6, 11 * K)
    e = O.orthogonalize(F)
    nz = O.orthogonalize(F, "neutralize")
    mem = O.joint(F)
    for t in range(F.shape[2]):
        m = mem[:, t]
        for k in range(1, K):
            for got, regs in ((e[k - 1, m, t], range(k)), (nz[k - 1, m, t], [0])):
                X = np.column_stack([np.ones(m.sum())] + [F[j, m, t] for j in regs])
                y = F[k, m, t]
                beta = np.linalg.lstsq(X, y, rcond=None)[0]
                exp = y - X @ beta
                assert np.abs(got - exp).max() <= 1e-12 * (np.abs(y).max() + 1.0)
        E = np.column_stack([F[0, m, t]] + [e[k, m, t] for k in range(K - 1)])
        E0 = E - E.mean(axis=0)
        G = E0.T @ E0
        nrm = np.sqrt(np.diag(G))
        off = np.abs(G - np.diag(np.diag(G))) / np.outer(nrm, nrm)
        assert off.max() <= 1e-12


def level_table(K, n, seed):
    """[K, n, 2K] factors on which the number of solved levels takes every value: day m - 1 (m = 1 .. K-1) has
    f_m = 2 f_{m-1} + 3, so the pivot of level m + 1 is rounding noise: levels 1 .. m are solved (level m with a residual of rounding
    noise) and the rest are NULL; day K + m - 2 (m = 1 .. K-1) has exactly m + 2 members, so level k <= m has its k + 2 members;
    on day 2K - 2 every value is scaled by 1e160, C[0][0] overflows and pivot 0 already fails (inf > 1e-12 inf is false); on day
    2K - 1 only f_1 is scaled by 1e160: D_0 is healthy and D_1 = inf - inf is NaN, which counts as singular, so level 1 alone is solved"""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((K, n, 2 * K))
    for k in range(1, K):
        F[k] += 0.5 * F[k - 1]
    for m in range(1, K):
        F[m, :, m - 1] = 2.0 * F[m - 1, :, m - 1] + 3.0
        F[0, m + 2:, K + m - 2] = O.NULL
    F[:, :, 2 * K - 2] *= 1e160
    F[1, :, 2 * K - 1] *= 1e160
    return F


def solved_levels(e):
    """residuals [K - 1, n, T] -> per day the number of levels with a residual, after asserting that they are levels 1 .. that number"""
    has = ~O.isnull(e).all(axis=1)                     # [K - 1, T]
    cnt = has.sum(axis=0)
    assert (has == (np.arange(1, e.shape[0] + 1)[:, None] <= cnt[None, :])).all(), "the solved levels are not a prefix"
    return cnt


def level_table_counts(K):
    return list(range(1, K)) + list(range(1, K)) + [0, 1]


@pytest.mark.parametrize("n", [40, 300])
@pytest.mark.parametrize("K", range(2, 9))
def test_every_solved_level_count(K, n):
    """level_table: the restatement solves exactly 1 .. K-1 levels on the collinear days, 1 .. K-1 on the size days, none on the
    overflow day and one on the NaN-pivot day, always a prefix; the solved residuals agree with lstsq on the size days, and the
    level-m residual of a collinear day is rounding noise"""
    F = level_table(K, n, 17 * K + n)
    e = O.orthogonalize(F)
    assert solved_levels(e).tolist() == level_table_counts(K)
    mem = O.joint(F)
    assert mem[:, :K - 1].all() and mem[:, 2 * K - 2:].all() and mem[:, K - 1:2 * K - 2].sum(axis=0).tolist() == list(range(3, K + 2))
    for m in range(1, K):
        assert np.abs(e[m - 1, :, m - 1]).max() <= 1e-12 * np.abs(F[m, :, m - 1]).max()
        t = K + m - 2
        sel = mem[:, t]
        for k in range(1, m + 1):
            X = np.column_stack([np.ones(m + 2)] + [F[j, sel, t] for j in range(k)])
            y = F[k, sel, t]
            exp = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
            assert np.abs(e[k - 1, sel, t] - exp).max() <= 1e-9 * (np.abs(y).max() + 1.0), (K, m, k)
    with np.errstate(all="ignore"):                       # the last day: pivot 0 is healthy, pivot 1 is inf - inf
        d0, d1 = (F[j, :, 2 * K - 1] - F[j, :, 2 * K - 1].mean() for j in (0, 1))
        c00, c10, c11 = (d0 * d0).sum(), (d1 * d0).sum(), (d1 * d1).sum()
        assert 0.0 < c00 < np.inf and np.isfinite(c10) and c11 == np.inf and np.isnan(c11 - c10 * (c10 / c00))
    nz = O.orthogonalize(F, "neutralize")                 # one regressor: solved on every day but the overflow day
    assert solved_levels(nz).tolist() == [K - 1] * (2 * K - 2) + [0, K - 1]


@pytest.mark.parametrize("K", [2, 4])
def test_neutralize_is_d16_size_neutralization(K):
    """on days with n >= 3 and C[0][0] != 0: bit-identical to clean(where(joint, f_k, NaN), z=f_0)"""
    F = random_factors(K, 260, 9, 5 + K)
    F[0, :, 3] = 1.5                                   # C[0][0] = 0: both NULL here, but not compared
    F[0, 2:, 4] = O.NULL                               # n = 2
    e = O.orthogonalize(F, "neutralize")
    mem = O.joint(F)
    days = [t for t in range(F.shape[2]) if t not in (3, 4)]
    for k in range(1, K):
        exp = CL.clean(np.where(mem, F[k], np.nan), z=F[0])
        assert (e[k - 1][:, days].view(np.uint64) == exp[:, days].view(np.uint64)).all()
    assert O.isnull(e[:, :, 3]).all() and O.isnull(e[:, :, 4]).all()


def test_clean_argument_errors():
    import polars_quant_amd as pq
    fac = pq.Factor()
    F = np.zeros((3, 4, 5))
    with pytest.raises(ValueError, match="method"):
        fac.clean(F, method="pca")
    with pytest.raises(ValueError, match="2..8"):
        fac.clean(F[:1])
    with pytest.raises(ValueError, match="2..8"):
        fac.clean(np.zeros((9, 4, 5)))
    with pytest.raises(ValueError, match="2..8"):
        fac.clean([F[0]])
    with pytest.raises(ValueError, match="shape"):
        fac.clean([F[0], F[1][:, :4]])
    with pytest.raises(ValueError):
        fac.clean([F[0][0], F[1][0]])                  # [T] series are refused
    with pytest.raises(ValueError):
        fac.clean([F[0], F[1][0]])
    with pytest.raises(ValueError):
        fac.clean(F[0])                                # one [N, T] array is not a list of factors
    with pytest.raises(ValueError, match="inplace"):
        fac.clean(F, inplace=True)                     # not a device tensor: no silent copy
    with pytest.raises(ValueError, match="inplace"):
        fac.clean(F, method="neutralize", inplace=True)
    from polars_quant_amd import api
    with pytest.raises(ValueError, match="mode"):
        api.factor_orthogonalize(F, 2)


def test_public_surface():
    """Factor().clean is D-19's multi-factor orthogonalization (README.md:1495), bound per instance; the class keeps no `clean`
    attribute, and the module-level clean stays D-16's single-factor cleaning"""
    import inspect
    import re
    from pathlib import Path

    import polars_quant_amd as pq
    root = Path(__file__).resolve().parent.parent
    assert not hasattr(pq.Factor, "clean")
    fac = pq.Factor()
    assert fac.clean is not pq.clean and fac.clean.__self__ is fac
    assert list(inspect.signature(fac.clean).parameters) == ["factors", "method", "inplace"]
    assert inspect.signature(fac.clean).parameters["method"].default == "orthogonalize"
    assert list(inspect.signature(pq.clean).parameters)[0] == "factor"
    txt = (root / "include" / "pq_hip.h").read_text()
    decl = re.search(r"pq_status\s+pq_factor_orthogonalize\s*\(([^)]*)\)", txt)
    assert decl, "pq_factor_orthogonalize is not declared"
    names = [re.findall(r"\w+", a)[-1] for a in decl.group(1).split(",")]
    assert names == ["pq_ctx", "pq_batch", "factors", "k", "mode", "out"]
    assert "xsec/orth.hip" in (root / "polars_quant_amd" / "csrc" / "Makefile").read_text()
