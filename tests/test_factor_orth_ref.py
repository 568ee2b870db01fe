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


@pytest.mark.parametrize("K", [2, 3, 5])
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


@pytest.mark.parametrize("K", [2, 3, 5, 8])
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
