"""-m gpu: the cross-sectional kernels of D-15 .. D-19 (csrc/xsec/: sorts, clean, regress, robust, orth) at every size class and
template branch they dispatch on, bit for bit against the numpy restatements (p-values within close_p's bound), with the helpers of the
feature test modules.

Where each branch is reached (the failure tags name function, shape, Q / K / L / G and pitch):

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
| D-18, robust.hip                                |                                                                               |
| rb_tie_start_kernel / rb_group_rank_kernel at   | test_rank_ic_sort_sizes: P = 16 [n16], 32 [n17 .. n32], 64 [n33], 128 [n65,   |
|   every P = 16 .. 16 384                        |   n128], 256 [n255, n256], 512 [n257 .. n512], 1 024 [n513 .. n1024], 2 048   |
|                                                 |   [n1025, n2048], 4 096 [n2049], 8 192 [n4097, n8192], 16 384 [n8193 ..]      |
| rb_search's last slot (lo == P - 1) on a row    |   [n16, n32, n128, n256, n512, n1024, n2048, n8192, n16384]: days 0, 1, 3 of  |
|   with n == P and no +inf tail; rb_search<true> |   lag 1 and of the G = 1 group have n_valid == n (asserted on the expected)   |
| rb_scan2 chunks, ch = ceil(n / 512): threads    |   [n511, n512, n513, n1023, n1025] (ic_decay, L = 3)                          |
|   with an empty chunk                           |                                                                               |
| rb_decay_partial_kernel: a full lag tile        | test_decay_lag_and_day_tiles: L = 8, 16, 256 full tiles, 9, 17, 255 with a    |
|   (RB_LT = 8), max_lag = 256, day tiles at      |   tail; T = 63 / 64 / 65 / 129 / 300; n = 255 / 256 / 257 / 512 / 513; rows   |
|   T = 63 / 64 / 65, blocks at n = 255 .. 513    |   l > T all NULL with n_days == 0 at [L256-T65-n255]; both methods            |
| rb_group_partial_kernel: group tiles around     | test_pearson_group_tiles: G = 32, 33, 63, 64, 65, 255, 256; the look-ahead of |
|   RB_GT = 32, the look-ahead of 8 at every      |   8 at n % 8 = 7 [n255], 0 [n256], 1 [n257, n513], 2 .. 6 [n258 .. n262]; an  |
|   n % 8                                         |   empty group and a one-member group (NULL rows, asserted on the expected)    |
| G = 256 at n = 16 384, the largest LDS          | test_rank_subgroup_largest_lds                                                |
|   footprint of robust.hip (147 KiB)             |                                                                               |
| wide rank fallbacks: max_lag > T (loop bound    | test_robust_wide_fallbacks[n16385, n100000]: rank decay at max_lag = 6, T =   |
|   l <= len, rb_decay_tail_kernel), rb_mask_     |   3; rank sub-group on a pitched input with [N, T] codes and an empty group;  |
|   kernel on d.stride, [N, T] codes, the limit   | test_robust_above_the_limit: Pearson at n = 100 001, Rank-IC raises, then an  |
|                                                 |   ordinary call on the same context                                           |
| rg_summary_kernel / rb_split_summary_kernel     | test_robust_summaries_across_chunks[T2047 .. T4097] (ic_decay, ic_subgroup,   |
|   past one XS_CHUNK; chunks relative to the     |   subsample_test at n_splits 1, 2, 3); test_split_summary_chunks_from_the_    |
|   period start                                  |   period_start: 6 151 days, periods from 0 / 2 051 / 4 101                    |
| D-19, orth.hip                                  |                                                                               |
| or_run<K, NEUT>, K = 4, 6, 7 (and 2, 3, 5, 8)   | test_orth_every_k[K2-* .. K8-*], both modes, in place at every K              |
| look-ahead B = 4 (K = 3, 4) at n % 4 != 0 in    |   [K3-*, K4-*] x [n257, n511, n513, n514] (n % 4 = 1, 3, 1, 2);               |
|   the last of several blocks; B = 2 (K >= 5)    |   [K5-* .. K8-*] x [n257, n513]                                               |
|   at odd n on a block boundary                  |                                                                               |
| day tiles at T = 63 / 64 / 65                   |   every case runs T = 63, 64 and 65                                           |
| nok = 1 .. K - 1 and 0 (the prefix rule); a NaN | test_orth_every_solved_level_count[K2 .. K8]: the table of                    |
|   pivot from an overflow counts as singular     |   test_factor_orth_ref.level_table, counts asserted on the expected; its last |
|                                                 |   day has D_1 = inf - inf behind a healthy D_0 (K >= 3)                       |
| more than three symbol blocks at K > 3          | test_orth_many_blocks[K4, K8]: n = 2 049, 9 blocks                            |
| CPU pin of K = 2 .. 8 against lstsq             | test_factor_orth_ref.py: test_against_lstsq_and_orthogonal,                   |
|                                                 |   test_sample_size_thresholds, test_every_solved_level_count                  |

Every size family has one case at an odd row pitch: n = 257 (sorts, rank sort sizes, lag tiles, group tiles, every orth K), q = 7,
n = 257 (xsec K), T = 257 (ts K), T = 2 049 (summaries, robust summaries), the wide percentile clean and the wide rank sub-group."""
import numpy as np
import pytest

import test_factor_clean_gpu as CL
import test_factor_orth_gpu as OG
import test_factor_orth_ref as OR
import test_factor_regress_gpu as RG
import test_factor_robust_gpu as RB
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


# ---------------------------------------------------------------- D-18: robust.hip
RANK_NS = sorted(SORT_NS + [511, 512, 513, 1023])
LAG_CASES = [(8, 63, 255), (9, 64, 256), (16, 65, 257), (17, 129, 512), (255, 300, 513), (256, 65, 255), (256, 300, 257)]   # L, T, n
GROUP_CASES = [(32, 255), (33, 256), (63, 257), (64, 513), (65, 258), (255, 259), (256, 260), (32, 261), (33, 262), (256, 513)]   # G, n


# the case tables reach every value the branch table names (checked at import, with or without a GPU)
assert {c[0] for c in LAG_CASES} == {8, 9, 16, 17, 255, 256} and {c[1] for c in LAG_CASES} == {63, 64, 65, 129, 300}
assert {c[2] for c in LAG_CASES} == {255, 256, 257, 512, 513} and {(256, 65), (256, 300)} <= {c[:2] for c in LAG_CASES}
assert {c[0] for c in GROUP_CASES} == {32, 33, 63, 64, 65, 255, 256} and {c[1] % 8 for c in GROUP_CASES} == set(range(8))
assert {255, 256, 257, 513} <= {c[1] for c in GROUP_CASES}


def check_decay(tag, f, r, L, method, pitch=None):
    """api.ic_decay against the restatement -> (ic, n_valid, summary) expected"""
    from polars_quant_amd import api
    got = api.ic_decay(RB.to_dev(f, pitch), RB.to_dev(r, pitch), L, method)
    exp = RB.R.ic_decay(f, r, L, method)
    tag = f"decay {tag} L={L} method={method} pitch={pitch}"
    RB.same(f"ic {tag}", RB.np_(got["ic"]), exp[0])
    RB.same(f"n_valid {tag}", RB.np_(got["n_valid"]), exp[1])
    RB.same_summary(tag, RB.np_(got["summary"]), exp[2])
    return exp


def check_subgroup(tag, f, r, codes, method, pitch=None):
    """api.ic_subgroup against the restatement -> (ic, n_valid, summary) expected"""
    from polars_quant_amd import api
    got = api.ic_subgroup(RB.to_dev(f, pitch), RB.to_dev(r, pitch), codes, method)
    exp = RB.R.ic_subgroup(f, r, codes, method)
    tag = f"subgroup {tag} G={exp[0].shape[0]} codes{list(codes.shape)} method={method} pitch={pitch}"
    RB.same(f"ic {tag}", RB.np_(got["ic"]), exp[0])
    RB.same(f"n_valid {tag}", RB.np_(got["n_valid"]), exp[1])
    RB.same_summary(tag, RB.np_(got["summary"]), exp[2])
    return exp


def null_rows(exp, rows):
    """the expected rows are all NULL: no IC on any day, n_days == 0, every summary column past it NULL"""
    ic, _, summ = exp
    return bool(RB.R.isnull(ic[rows]).all() and (summ[rows, 0] == 0).all() and RB.R.isnull(summ[rows, 1:]).all())


@pytest.mark.parametrize("n", RANK_NS, ids=[f"n{n}" for n in RANK_NS])
def test_rank_ic_sort_sizes(pq, n):
    """Rank-IC in LDS on both sides of every sort size P = 16 .. 16 384 and of rb_scan2's 512 chunks: decay (L = 3), one group over the
    whole row (G = 1) and G = 7 with unclassified symbols, [N] and [N, T] codes.  size_days' days 0, 1 and 3 are full rows: at n == P
    the sorted row has no +inf tail, under the composite key of G = 1 either."""
    T = 5
    pitch = 11 if n == 257 else None
    f, r = size_days(n, T, 900 + n)
    full = [0, 1, 3]
    _, nv, _ = check_decay(f"n={n}", f, r, 3, 1, pitch)
    assert (nv[0, full] == n).all() and nv[0, 4] <= 3 and nv[0, 2] == (X.valid(f[:, 2]) & X.valid(r[:, 2])).sum()
    rng = np.random.default_rng(n)
    for shape in ((n,), (n, T)):
        _, nv, _ = check_subgroup(f"n={n}", f, r, np.zeros(shape, np.int32), 1, pitch)
        assert nv.shape == (1, T) and (nv[0, full] == n).all()
        codes = rng.integers(-2, 7, shape).astype(np.int32)
        codes.flat[0] = 6
        _, nv, _ = check_subgroup(f"n={n}", f, r, codes, 1, pitch)
        assert nv.shape == (7, T) and (nv[:, full].sum(axis=0) == (RB.R.group_codes(codes, f.shape)[:, full] >= 0).sum(axis=0)).all()


@pytest.mark.parametrize("L,T,n", LAG_CASES, ids=[f"L{c[0]}-T{c[1]}-n{c[2]}" for c in LAG_CASES])
def test_decay_lag_and_day_tiles(pq, L, T, n):
    """lag tiles of 8 (full and with a tail, up to max_lag = 256), day tiles of 64 and symbol blocks of 256, Pearson and Spearman; the
    lags above T are all-NULL rows"""
    pitch = T + 3 if n == 257 and T == 65 else None
    for method in RB.METHODS:
        f, r = RB.make(n, T, 7 * L + T + n + method, ties=method == 1)
        exp = check_decay(f"{n}x{T}", f, r, L, method, pitch)
        assert not RB.R.isnull(exp[0][:min(L, T), 0]).any() and exp[2][min(L, T) - 1, 0] == T - min(L, T) + 1
        if L > T:
            assert null_rows(exp, slice(T, L)) and (exp[1][T:] == 0).all()


def group_tile_codes(G, shape, rng):
    """-> (codes in [-2, G), the large groups): group 1 has no member, group G - 1 exactly one (symbol 2, every day), and half of the
    symbols sit in a few large groups on both sides of the tile boundaries (so that these have real cross-sections at G = 256 too)"""
    big = np.array(sorted({c for c in (0, 30, 31, 32, 33, 63, 64, G // 2, G - 2) if c == 0 or 1 < c < G - 1}))
    codes = np.where(rng.random(shape) < 0.5, rng.choice(big, shape), rng.integers(-2, G, shape))
    codes[(codes == 1) | (codes == G - 1)] = 0
    codes[2] = G - 1
    return codes.astype(np.int32), big


@pytest.mark.parametrize("G,n", GROUP_CASES, ids=[f"G{c[0]}-n{c[1]}" for c in GROUP_CASES])
def test_pearson_group_tiles(pq, G, n):
    """Pearson sub-group IC with the groups on both sides of the 32-group LDS tiles and the symbols at every remainder of the
    look-ahead of 8; an empty group and a one-member group are NULL rows"""
    T = 66
    pitch = T + 5 if n == 257 else None
    f, r = RB.make(n, T, 31 * G + n)
    f[2], r[2] = 0.5, 0.25                       # the lone member of group G - 1 is valid on every day
    rng = np.random.default_rng(G * 1000 + n)
    for shape in ((n,), (n, T)):
        codes, big = group_tile_codes(G, shape, rng)
        exp = check_subgroup(f"{n}x{T}", f, r, codes, 0, pitch)
        assert exp[0].shape == (G, T)
        assert null_rows(exp, [1, G - 1]) and (exp[1][1] == 0).all() and (exp[1][G - 1] == 1).all()
        assert (exp[2][big, 0] == T).all()       # the large groups have an IC on every day


def test_rank_subgroup_largest_lds(pq):
    """n = 16 384 keys and G = 256 groups: the largest LDS footprint of robust.hip; days 0, 1 and 3 are full rows"""
    n, T, G = 16384, 4, 256
    f, r = size_days(n, T, 77)
    codes = np.random.default_rng(78).integers(-1, G, (n, T)).astype(np.int32)
    codes[0, 0] = G - 1
    _, nv, summ = check_subgroup(f"n={n}", f, r, codes, 1)
    assert nv.shape == (G, T) and (nv[:, [0, 1, 3]].sum(axis=0) == (codes[:, [0, 1, 3]] >= 0).sum(axis=0)).all()
    assert (summ[:, 0] >= 2).all()


@pytest.mark.parametrize("n", [16385, 100000], ids=["n16385", "n100000"])
def test_robust_wide_fallbacks(pq, n):
    """n > 16 384: pq_factor_ic per lag / per masked group.  max_lag = 6 above T = 3 (rows no pq_factor_ic call wrote), and the
    sub-group mask on a pitched input with [N, T] codes and an empty group; Pearson beside it"""
    T = 3
    f, r = size_days(n, T, 40 + n)
    for method in RB.METHODS:
        exp = check_decay(f"n={n}", f, r, 6, method)
        assert null_rows(exp, slice(T, 6)) and (exp[1][T:] == 0).all() and (exp[1][0, :2] == n).all()
    rng = np.random.default_rng(n)
    for shape, pitch in (((n, T), 5), ((n,), None)):
        codes = rng.integers(-1, 4, shape).astype(np.int32)
        codes[codes == 2] = 0                    # group 2 of 0 .. 3 has no member
        codes.flat[0] = 3
        for method in RB.METHODS:
            exp = check_subgroup(f"n={n}", f, r, codes, method, pitch)
            assert exp[0].shape == (4, T) and null_rows(exp, [2]) and (exp[1][2] == 0).all()
            assert not RB.R.isnull(exp[0][[0, 1, 3], 1:]).any()


def test_robust_above_the_limit(pq):
    """n = 100 001: Pearson is accepted, Rank-IC raises and leaves the context usable"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import PqError
    n, T = 100001, 3
    f, r = size_days(n, T, 5)
    codes = (np.arange(n) % 5 - 1).astype(np.int32)
    check_decay(f"n={n}", f, r, 2, 0)
    check_subgroup(f"n={n}", f, r, codes, 0)
    fd, rd = RB.to_dev(f), RB.to_dev(r)
    with pytest.raises(PqError, match="at most 100000"):
        api.ic_decay(fd, rd, 2, 1)
    with pytest.raises(PqError, match="at most 100000"):
        api.ic_subgroup(fd, rd, codes, 1)
    f, r = size_days(300, 5, 6)
    check_decay("after the error", f, r, 3, 1)
    check_subgroup("after the error", f, r, codes[:300], 1)


@pytest.mark.parametrize("T", SEQ_TS, ids=[f"T{t}" for t in SEQ_TS])
def test_robust_summaries_across_chunks(pq, T):
    """rg_summary_kernel on the rows of ic_decay (L = 3) and ic_subgroup (G = 3) and rb_split_summary_kernel under
    Factor.subsample_test, on IC series with NULL days on both sides of each 2 048-day chunk boundary"""
    n = 20
    holes = [t for t in SEQ_HOLES if t < T]
    pitch = T + 2 if T == 2049 else None
    fac = pq.Factor()
    for method, name in ((0, "pearson"), (1, "spearman")):
        f, r = RB.make(n, T, 90 + T + method, ties=method == 1)
        f[:, holes] = X.NULL                    # dead days: the IC of every lag and of every group is NULL
        ic, _, summ = check_decay(f"{n}x{T}", f, r, 3, method, pitch)
        assert RB.R.isnull(ic[:, holes]).all() and (summ[:, 0] > T - 3 - len(holes) - 0.02 * T).all()
        codes = (np.arange(n) % 4 - 1).astype(np.int32)
        ic3, _, summ = check_subgroup(f"{n}x{T}", f, r, codes, method, pitch)
        assert RB.R.isnull(ic3[:, holes]).all() and (summ[:, 0] > 0.9 * T).all()
        for k in (1, 2, 3):
            got = fac.subsample_test(RB.to_dev(f, pitch), RB.to_dev(r, pitch), n_splits=k, method=name)
            start, end = RB.R.split_periods(T, k)
            tag = f"subsample {n}x{T} {name} n_splits={k}"
            RB.same(f"start {tag}", RB.np_(got["start"]).astype(np.float64), start.astype(np.float64))
            RB.same(f"end {tag}", RB.np_(got["end"]).astype(np.float64), end.astype(np.float64))
            got_s = np.stack([RB.np_(got[c]) for c in ("n_days", "mean_ic", "std_ic", "t_stat", "p_value")], axis=1)
            RB.same_summary(tag, got_s, RB.R.series_split_summary(ic[0], k))


@pytest.mark.parametrize("dead", [(2047, 2048), (2047,), (2048,)], ids=["both", "last-of-chunk", "first-of-chunk"])
def test_split_summary_chunks_from_the_period_start(pq, dead):
    """6 151 days in 3 periods of 2 051 / 2 050 / 2 050 days from 0 / 2 051 / 4 101: each period is one full chunk and 2 or 3 days,
    staged from the period's start, with NULL entries at the chunk boundary of each period"""
    from polars_quant_amd import api
    T, k = 6151, 3
    start, end = RB.R.split_periods(T, k)
    assert start.tolist() == [0, 2051, 4101] and (end - start + 1).tolist() == [2051, 2050, 2050]
    rng = np.random.default_rng(61)
    x = rng.standard_normal(T) * 0.05 + 0.01
    for s in start:
        x[[s + o for o in dead]] = X.NULL
    exp = RB.R.series_split_summary(x, k)
    assert (exp[:, 0] == (end - start + 1) - len(dead)).all() and not RB.R.isnull(exp).any()
    RB.same_summary(f"series_split_summary dead={dead}", RB.np_(api.series_split_summary(RB.to_dev(x), k)), exp)


# ---------------------------------------------------------------- D-19: orth.hip
ORTH_NS = [255, 256, 257, 511, 513, 514]
ORTH_TS = [63, 64, 65]


@pytest.mark.parametrize("n", ORTH_NS, ids=[f"n{n}" for n in ORTH_NS])
@pytest.mark.parametrize("K", range(2, 9), ids=[f"K{k}" for k in range(2, 9)])
def test_orth_every_k(pq, K, n):
    """or_run<K, NEUT> for every K in both modes, symbols around the 256-symbol blocks (every remainder of the look-ahead of 4 and
    of 2 in the last block), days around the 64-day tiles, make's special days; in place against out of place"""
    fac = pq.Factor()
    for T in ORTH_TS:
        pitch = T + 6 if n == 257 else None
        F = OG.make(K, n, T, 500 * K + n + T)
        for method in OG.O.MODES:
            _, exp = OG.check(pq, F, method, pitch)
            e = exp[1:] if method == "orthogonalize" else exp
            assert OG.O.isnull(e[:, :, 1]).all() and OG.O.isnull(e[:, :, 3]).all()     # constant f_0, all-NULL day
            assert not OG.O.isnull(e[:, :, 6:]).all(axis=1).any()                        # every level solved on the ordinary days
            if method == "orthogonalize":
                assert OG.O.isnull(e[K - 2, :, 5]).all() and (K < 3 or OG.O.isnull(e[1:, :, 0]).all())
        Xd = OG.to_dev(F, pitch)
        ref = fac.clean(Xd.clone(), method="orthogonalize").cpu().numpy()
        assert fac.clean(Xd, method="orthogonalize", inplace=True) is Xd
        OG.same(f"in place K={K} {n}x{T} pitch={pitch}", Xd.cpu().numpy(), ref)
        OG.same(f"in place vs restatement K={K} {n}x{T} pitch={pitch}", Xd.cpu().numpy(), OG.O.clean_full(F))


@pytest.mark.parametrize("K", range(2, 9), ids=[f"K{k}" for k in range(2, 9)])
def test_orth_every_solved_level_count(pq, K):
    """test_factor_orth_ref.level_table: 1 .. K-1 solved levels on the collinear days, 1 .. K-1 on the size days, none on the overflow
    day (pivot 0 is inf), one on the day whose pivot 1 is NaN behind a healthy pivot 0, the solved levels a prefix; the level-m
    residual of a collinear day is rounding noise and still matches bit for bit"""
    for n in (300, 1030):
        F = OR.level_table(K, n, 23 * K + n)
        _, exp = OG.check(pq, F, "orthogonalize", pitch=2 * K + 3 if n == 300 else None)
        assert OR.solved_levels(exp[1:]).tolist() == OR.level_table_counts(K)
        _, exp = OG.check(pq, F, "neutralize")
        assert OR.solved_levels(exp).tolist() == [K - 1] * (2 * K - 2) + [0, K - 1]


@pytest.mark.parametrize("K", [4, 8], ids=["K4", "K8"])
def test_orth_many_blocks(pq, K):
    """n = 2 049: nine symbol blocks, the last of one symbol"""
    F = OG.make(K, 2049, 6, 70 + K)
    for method in OG.O.MODES:
        _, exp = OG.check(pq, F, method)
        assert not OG.O.isnull(exp).all(axis=1).any()
