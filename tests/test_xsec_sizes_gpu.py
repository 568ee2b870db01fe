"""-m gpu: the cross-sectional kernels of D-15 / D-16 / D-17 (csrc/xsec/) at every size class and template branch they dispatch on,
bit for bit against the numpy restatements (p-values within close_p's bound), with the helpers of the feature test modules.

Where each branch is reached (the failure tags name function, shape, Q / K and pitch):

| branch (never reached before)                   | case                                                                          |
|-------------------------------------------------|-------------------------------------------------------------------------------|
| LDS bitonic sort, P = next power of two >=      | test_sort_size_classes: P = 32 [n17, n31, n32], 128 [n65, n128],              |
|   max(16, n), xs_groups / cl_bounds_lds_kernel  |   256 [n255, n256], 1 024 [n1024], 2 048 [n1025, n2048], 8 192 [n4097, n8192] |
| n = P: a row without a +inf tail                |   [n16, n32, n128, n256, n1024, n2048, n8192, n16384] (days 0, 1, 3)          |
| n = 16 384, the largest LDS row (136 KiB)       |   [n16384], with [n16383] and [n8193] below it                                |
| xs_group_partial_kernel<G> with ng < G          | test_every_group_count: G = 5 [q3, q4], G = 10 [q6 .. q9], G = 20 [q11 .. q19] |
| rg_dispatch<K, false>, K = 4, 5, 6, 7           | test_xsec_regress_every_k[K4-*, K5-*, K6-*, K7-*]                             |
| rg_dispatch<K, true>, K = 4, 5, 6, 7            | test_ts_regress_every_k[K4-*, K5-*, K6-*, K7-*]                               |
| CPU pin of K = 4 .. 7 against lstsq             | test_factor_regress_ref.py: test_against_lstsq_and_inverse_normal_equations,  |
|                                                 |   test_time_series_form_against_lstsq                                         |
| xs_seq at T = 2 047, 2 048, 2 049, 4 097        | test_sequential_summaries_across_chunks[T2047, T2048, T2049, T4097]           |
| ic_stats past one chunk                         |   (also the group / long-short and Fama-MacBeth summaries)                    |
| D-12 blocks of 256: 255, 256, 257, 512, 513     | symbols per day: test_sort_size_classes[n255, n256, n257],                    |
|                                                 |   test_xsec_regress_every_k[*-n255 .. *-n513]; days per symbol:               |
|                                                 |   test_ts_regress_every_k[*-T255 .. *-T513]                                   |
| wide (rocPRIM) path at n = 100 000              | test_wide_path_at_the_limit                                                   |
| series_mask: a series at j = K - 1;             | test_ts_regress_every_k: the series-last call at every K;                     |
|   every factor a series                         |   every factor a series at K = 1, 4, 8                                        |

Every size family has one case at an odd row pitch: n = 257 (sorts), q = 7, n = 257 (xsec K), T = 257 (ts K), T = 2 049 (summaries)
and the wide percentile clean."""
import numpy as np
import pytest

import test_factor_clean_gpu as CL
import test_factor_regress_gpu as RG
import test_factor_sorts_gpu as S
import xsec_ref as X
from test_factor_sorts_gpu import pq  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SORT_NS = [16, 17, 31, 32, 33, 65, 128, 255, 256, 257, 1024, 1025, 2048, 2049, 4097, 8192, 8193, 16383, 16384]
SORT_QS = [3, 5, 7, 13, 20]
SORT_LS = [(0.2, 0.2), (0.1, 0.4)]
REG_NS = [255, 256, 257, 512, 513]
REG_TS = [255, 256, 257, 512, 513, 2049]
SEQ_TS = [2047, 2048, 2049, 4097]
SEQ_HOLES = [0, 1, 2046, 2047, 2048, 2049, 4094, 4095, 4096]   # dead days on both sides of each 2 048-day chunk boundary


def size_days(n, T, seed):
    """[n, T] factor and return in test_rank_ic_cross_section_sizes's day layout: day 0 every key equal, day 1 a two-valued factor
    (its zeros of both signs), day 2 ~10 % NULL / NaN factors and NaN returns, day 3 +0.0 and -0.0 among other values, day 4 only
    1 - 3 valid members.  Days 0, 1 and 3 have every symbol in the cross-section (n = P rows without a +inf tail)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, T))
    r = 0.1 * f + 0.02 * rng.standard_normal((n, T))
    f[:, 0] = 1.25
    f[:, 1] = (rng.random(n) < 0.5).astype(np.float64)
    f[(f[:, 1] == 0.0) & (rng.random(n) < 0.5), 1] = -0.0
    if T > 2:
        f[rng.random(n) < 0.05, 2] = X.NULL
        f[rng.random(n) < 0.05, 2] = np.nan
        r[rng.random(n) < 0.05, 2] = np.nan
    if T > 3:
        u = rng.random(n)
        f[:, 3] = np.where(u < 0.3, 0.0, np.where(u < 0.6, -0.0, f[:, 3]))
    if T > 4:
        keep = rng.choice(n, size=min(n, 1 + n % 3), replace=False)
        dead = np.ones(n, dtype=bool)
        dead[keep] = False
        f[dead, 4] = X.NULL
    return f, r


def clean_inputs(n, T, seed):
    f, _ = size_days(n, T, seed)
    rng = np.random.default_rng(seed + 1)
    cap = np.exp(rng.standard_normal((n, T)) * 1.5 + 10.0)
    ind = rng.integers(0, 6, n)
    return f, cap, ind


@pytest.mark.parametrize("n", SORT_NS, ids=[f"n{n}" for n in SORT_NS])
def test_sort_size_classes(pq, n):
    """both sides of every LDS bitonic sort size P = 16 .. 16 384 (64 .. 1 024 threads): quantiles, long-short legs, clean"""
    pitch = 11 if n == 257 else None
    f, r = size_days(n, 5, 500 + n)
    for q in SORT_QS:
        S.check_groups(pq, f, r, 0, q, pitch=pitch)
    for top, bottom in SORT_LS:
        S.check_groups(pq, f, r, 1, 0, top, bottom, pitch=pitch)
    f, cap, ind = clean_inputs(n, 5, 700 + n)
    for mode in ("mad", "percentile"):
        for on in (False, True):
            CL.check(pq, f, cap, ind, mode, on, on, on, pitch=pitch)


@pytest.fixture(scope="module")
def discrete3000():
    """test_heavily_discrete_factor_long_tie_runs's table: a three-valued factor over 3 000 symbols, tie runs of ~1 000 per day"""
    rng = np.random.default_rng(3)
    f = rng.integers(-1, 2, (3000, 24)).astype(np.float64)
    f[f == 0] = np.where(rng.random(int((f == 0).sum())) < 0.5, -0.0, 0.0)
    r = np.round(rng.standard_normal((3000, 24)), 2)
    return f, r


@pytest.mark.parametrize("q", range(2, 21), ids=[f"q{q}" for q in range(2, 21)])
def test_every_group_count(pq, q, discrete3000):
    """every Q: ng < G in each xs_group_partial_kernel<G> bucket (G = 5: Q 3, 4; G = 10: Q 6 .. 9; G = 20: Q 11 .. 19)"""
    f, r = S.make("nulls", 300, 131, 50 + q)
    S.check_groups(pq, f, r, 0, q, pitch=139 if q == 7 else None)
    S.check_groups(pq, *discrete3000, 0, q)


def test_wide_path_at_the_limit(pq):
    """n = 100 000, the largest cross-section the rocPRIM path accepts"""
    n = 100000
    f, r = size_days(n, 3, 11)
    S.check_groups(pq, f, r, 0, 7)
    S.check_groups(pq, f, r, 1, 0, 0.1, 0.4)
    f, cap, ind = clean_inputs(n, 3, 12)
    for mode in ("mad", "percentile"):
        CL.check(pq, f, cap, ind, mode, False, False, False)
        CL.check(pq, f, cap, ind, mode, True, True, True, pitch=5 if mode == "percentile" else None)


@pytest.mark.parametrize("n", REG_NS, ids=[f"n{n}" for n in REG_NS])
@pytest.mark.parametrize("K", range(1, 9), ids=[f"K{k}" for k in range(1, 9)])
def test_xsec_regress_every_k(pq, K, n):
    """rg_dispatch<K, false> for every K, symbols per day around the 256-symbol summation blocks, make's special days"""
    F, r = RG.make(K, n, 8, 1000 * K + n)
    _, exp = RG.check_xsec(pq, F, r, pitch=11 if n == 257 else None)
    assert RG.R.isnull(exp["coef"][:, 0]).all() and RG.R.isnull(exp["coef"][:, 1]).all()   # singular, n = K + 1
    assert not RG.R.isnull(exp["coef"][:, 2]).any() and exp["n"][2] == K + 2                  # solved on exactly K + 2
    assert exp["r2"][3] == 1.0 and RG.R.isnull(exp["r2"][4])                                   # perfect fit, constant return


@pytest.mark.parametrize("T", REG_TS, ids=[f"T{t}" for t in REG_TS])
@pytest.mark.parametrize("K", range(1, 9), ids=[f"K{k}" for k in range(1, 9)])
def test_ts_regress_every_k(pq, K, T):
    """rg_dispatch<K, true> for every K, days per symbol around the 256-day summation blocks.  make's special units become symbols
    0 .. 4 (singular, K + 1 days, exactly K + 2 days, a perfect fit on integers, a constant return).  Then a [T] series at j = K - 1
    (symbol 0's own factor 0, so symbol 0 stays singular), and at K = 1, 4, 8 every factor a series (symbol 3's integer rows, so symbol 3
    stays a perfect fit; series 0 with NULL days)."""
    F, r = RG.make(K, T, 70, 3000 * K + T)
    F, r = np.ascontiguousarray(F.transpose(0, 2, 1)), np.ascontiguousarray(r.T)
    cols = list(F)
    _, exp = RG.check_ts(pq, cols, r, pitch=T + 2 if T == 257 else None)
    assert RG.R.isnull(exp["coef"][0]).all() and RG.R.isnull(exp["coef"][1]).all()
    assert exp["n"][2] == K + 2 and not RG.R.isnull(exp["coef"][2]).any()
    assert exp["r2"][3] == 1.0 and RG.R.isnull(exp["r2"][4])
    RG.check_ts(pq, cols[:K - 1] + [F[0, 0] if K > 1 else F[0, 3]], r)
    if K in (1, 4, 8):
        ser = [F[j, 3].copy() for j in range(K)]
        ser[0][::97] = X.NULL
        _, exp = RG.check_ts(pq, ser, r)
        assert exp["r2"][3] == 1.0 and exp["n"][3] == T - len(range(0, T, 97))


@pytest.mark.parametrize("T", SEQ_TS, ids=[f"T{t}" for t in SEQ_TS])
def test_sequential_summaries_across_chunks(pq, T):
    """xs_seq stages 2 048 days per step: group / long-short summaries, ic_stats and the Fama-MacBeth summary (K = 5) on series with
    NULL days on both sides of each chunk boundary"""
    from polars_quant_amd import api
    holes = [t for t in SEQ_HOLES if t < T]
    pitch = T + 2 if T == 2049 else None
    f, r = S.make("nulls", 40, T, 60 + T)
    f[:, holes] = X.NULL                       # dead days: every group mean, the spread and the next day's turnover are NULL
    S.check_groups(pq, f, r, 0, 5, pitch=pitch)
    S.check_groups(pq, f, r, 1, 0, 0.2, 0.2, pitch=pitch)
    rng = np.random.default_rng(T)
    ic = rng.standard_normal(T) * 0.05 + 0.01
    ic[holes] = X.NULL
    ic[rng.random(T) < 0.03] = X.NULL
    ic[rng.random(T) < 0.03] = np.nan
    S.same(f"ic_stats T={T}", api.ic_stats(RG.to_dev(ic)).cpu().numpy(), X.ic_stats(ic))
    F, r = RG.make(5, 20, T, 80 + T)
    r[:, holes] = RG.R.NULL                    # days without a solution: NaN coefficient rows
    _, exp = RG.check_xsec(pq, F, r, pitch=pitch)
    assert RG.R.isnull(exp["coef"][:, holes]).all()
