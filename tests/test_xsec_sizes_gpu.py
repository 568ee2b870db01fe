"""-m gpu: the cross-sectional kernels of D-15 .. D-20 (csrc/xsec/: sorts, clean, regress, robust, orth, build) at every size class and
template branch they dispatch on, bit for bit against the numpy restatements (p-values within close_p's bound), with the helpers of the
feature test modules.

Where each branch is reached (the failure tags name function, shape, Q / K / L / G and pitch):

| branch (never reached before)                   | case                                                                          |
|-------------------------------------------------|-------------------------------------------------------------------------------|
| LDS bitonic sort, P = next power of two >=      | test_sort_size_classes: P = 32 [n17, n31, n32], 128 [n65, n128],              |
|   max(16, n), xs_groups / cl_bounds_lds_kernel  |   256 [n255, n256], 1 024 [n1024], 2 048 [n1025, n2048], 8 192 [n4097, n8192] |
| n = P: a row without a +inf tail                |   [n16, n32, n128, n256, n1024, n2048, n8192, n16384] (days 0, 1, 3)          |
| n = 16 384, the largest LDS row (136 KiB)       |   [n16384], with [n16383] and [n8193] below it                                |
| xs_cell_partial_reg_kernel<G> with C < G        | test_every_group_count: G = 5 [q3, q4], G = 10 [q6 .. q9], G = 20 [q11 .. q19] |
| rg_dispatch<K, false>, K = 4, 5, 6, 7           | test_xsec_regress_every_k[K4-*, K5-*, K6-*, K7-*]                             |
| rg_dispatch<K, true>, K = 4, 5, 6, 7            | test_ts_regress_every_k[K4-*, K5-*, K6-*, K7-*]                               |
| CPU pin of K = 4 .. 7 against lstsq             | test_factor_regress_ref.py: test_against_lstsq_and_inverse_normal_equations,  |
|                                                 |   test_time_series_form_against_lstsq                                         |
| xo_ldl's count of leading good pivots: the      | test_regress_failing_pivot_at_every_position[K3, K8]: test_factor_regress_    |
|   first singular pivot at j = 0 .. K - 1, an    |   ref.pivot_table, NULL days asserted on the expected; K8 also transposed     |
|   overflowing C[0][0] with NaN pivots behind it |   through pq_ts_regress (K + 2 symbols, 40 days)                              |
| xs_seq at T = 2 047, 2 048, 2 049, 4 097        | test_sequential_summaries_across_chunks[T2047, T2048, T2049, T4097]           |
| ic_stats past one chunk                         |   (also the group / long-short and Fama-MacBeth summaries)                    |
| D-12 blocks of 256: 255, 256, 257, 512, 513     | symbols per day: test_sort_size_classes[n255, n256, n257],                    |
|                                                 |   test_xsec_regress_every_k[*-n255 .. *-n513]; days per symbol:               |
|                                                 |   test_ts_regress_every_k[*-T255 .. *-T513]                                   |
| wide (rocPRIM) path at n = 100 000              | test_wide_path_at_the_limit                                                   |
| -0 and +0 on the wide path of the sorts: one    | test_wide_path_signed_zeros: n = 16 385, a factor from {-0, +0, 1}            |
|   tie run, though the radix sort orders them    |                                                                               |
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
| D-20, build.hip                                 |                                                                               |
| xs_sort_lds_kernel<BdRankOp> at every P = 16 .. | test_build_rank_sort_sizes: P = 16 [n16], 32 [n17 .. n32], 64 [n33], 128      |
|   16 384 (64 .. 1 024 threads); xs_tie_run's    |   [n65, n128], 256 [n255, n256], 512 [n257 .. n512], 1 024 [n513, n1024],     |
|   last slot on a row with n == P, no +inf tail  |   2 048 [n1025, n2048], 4 096 [n2049], 8 192 [n4097, n8192], 16 384 [n8193 .. |
|                                                 |   n16384]; days 0, 1, 3 have n_valid == n (asserted on the input's sample)    |
| nv == 0 (the return before the barrier), nv of  |   day 5 has no member, day 4 has 1 - 3, day 0 is one tie run of length n      |
|   1 - 3 under a +inf tail, one tie run of n     |   (up to n = 16 384)                                                          |
| pq_factor_rank(mode = 2, descending = 1), which |   every case, and test_build_wide_path, through the C ABI against             |
|   the Python layer refuses                      |   rank(f, "quantile", True)                                                   |
| wide (rocPRIM) rank: xs_sort_wide_kernel on     | test_build_wide_path[n16385, n100000]: days all equal / all NULL / one member |
|   an all-NULL day, a one-member day, one tie    |   / ties, signed zeros and ~5 % NULL, NaN, +-inf; n = 16 385 also at pitch 5  |
|   run of n; the limit and above it              | test_build_above_the_limit: n = 100 001, the rank family raises and writes    |
|                                                 |   nothing, minmax / zscore / weighted (G = 6, 256) / ratio / diff compute     |
| xs_prep / bd_transpose 32 x 32 tiles and the    | test_build_tiles: (n, T) over {31, 32, 33} x {1, 31, 32, 33}, (5, 300),       |
|   64-day passes: both tile edges at once, T = 1 |   (257, 129), every method, the corner cell in every sample; [n32-T33] at     |
|   many day tiles over few symbols               |   pitch 37                                                                    |
| look-ahead of 8 of bd_minmax / bd_weighted in   | test_build_look_ahead: n % 8 = 1 .. 7, 0 [n257 .. n264], [n511, n512, n513],  |
|   the last of several blocks                    |   nine blocks [n2049]; T = 63 and 65; the last symbol is in every sample      |
| bd_w_member's guard g < G; group_stride above   | test_build_group_codes_outside_the_range: n_groups = 4, codes from -3 .. 8,   |
|   the batch stride                              |   INT32_MIN, INT32_MAX as [N] and as [N, T] at group_stride T + 5 (pad        |
|                                                 |   columns hold the live code 0); n_groups = 1 with every code >= 1: all NULL  |
| bd_binary_kernel's second grid step             | test_build_binary_grid_stride: (2^20 + 3, 1), chunks = 1; (524 289, 257),     |
|   (total > 2^20 workgroups), s = w / chunks     |   chunks = 2, total = 2^20 + 2: row 524 288 is the second step                |
| minmax: a day of +-0, a day of one, a subnormal | test_build_minmax_and_weight_edges: one table of days at n = 300; the         |
|   range, a range that overflows; W = +inf       |   overflowing range and W = +inf compare non-NULL NaN with non-NULL NaN       |
| ctx->ws reuse: wide rank, LDS rank, grouped     | test_build_workspace_reuse: one context, five calls, the last bitwise equal   |
|   weighted, minmax, wide rank again             |   to the first                                                                |
| ctx->ws reuse across xs_cells_layout: 1 and 2   | test_sorts_workspace_reuse: quantiles, 5 x 5 dependent, long-short, 2 x 3     |
|   key rows, register and LDS cells, wide tail   |   independent at n = 16 385, rank, quantiles again bitwise equal to the first  |

Every size family has one case at an odd row pitch: n = 257 (sorts, rank sort sizes, lag tiles, group tiles, every orth K, the D-20 rank
sizes), q = 7, n = 257 (xsec K), T = 257 (ts K), T = 2 049 (summaries, robust summaries), the wide percentile clean, the wide rank
sub-group, the wide D-20 rank at n = 16 385 and the D-20 tiles at (32, 33)."""
import ctypes as C

import numpy as np
import pytest

import test_factor_build_gpu as BG
import test_factor_clean_gpu as CL
import test_factor_double_sort_gpu as DS
import test_factor_orth_gpu as OG
import test_factor_orth_ref as OR
import test_factor_regress_gpu as RG
import test_factor_regress_ref as RR
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
    """every Q: C < G in each xs_cell_partial_reg_kernel<G> bucket (G = 5: Q 3, 4; G = 10: Q 6 .. 9; G = 20: Q 11 .. 19)"""
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


def test_wide_path_signed_zeros(pq):
    """n = 16 385, the first wide row, on a factor drawn from {-0.0, +0.0, 1.0} with a few NULLs: the radix sort orders -0 before +0 by
    bit pattern where the LDS network leaves them as they fall; the labels must still treat the two zeros as one tie run.  (Whether the
    key itself keeps -0 does not show in a label and is not pinned here.)"""
    n, T = 16385, 2
    rng = np.random.default_rng(13)
    f = np.array([-0.0, 0.0, 1.0])[rng.integers(0, 3, (n, T))]
    f[rng.random((n, T)) < 0.01] = X.NULL
    r = np.round(rng.standard_normal((n, T)), 2)
    assert np.signbit(f[f == 0.0]).any() and not np.signbit(f[f == 0.0]).all()
    S.check_groups(pq, f, r, 0, 5)
    S.check_groups(pq, f, r, 1, 0, 0.3, 0.4)


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


@pytest.mark.parametrize("K", [3, 8], ids=["K3", "K8"])
def test_regress_failing_pivot_at_every_position(pq, K):
    """test_factor_regress_ref.pivot_table: the first singular pivot at every position 0 .. K - 1 and an overflow day; a day whose
    interior pivot fails is NULL although later pivots, computed from garbage, may pass.  K = 8 also in the time-series form."""
    F, r = RR.pivot_table(K, 60 + K)
    _, exp = RG.check_xsec(pq, F, r)
    assert RG.R.isnull(exp["coef"][:, :K + 1]).all() and np.isfinite(exp["coef"][:, K + 1]).all() and (exp["n"] == 40).all()
    if K == 8:
        _, exp = RG.check_ts(pq, [np.ascontiguousarray(f.T) for f in F], np.ascontiguousarray(r.T))
        assert RG.R.isnull(exp["coef"][:K + 1]).all() and np.isfinite(exp["coef"][K + 1]).all()


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


# ---------------------------------------------------------------- D-20: build.hip
R = BG.R
BUILD_NS = sorted(SORT_NS + [511, 512, 513])
TILE_CASES = [(n, T) for n in (31, 32, 33) for T in (1, 31, 32, 33)] + [(5, 300), (257, 129)]
AHEAD_NS = [257, 258, 259, 260, 261, 262, 263, 264, 511, 512, 513, 2049]
AHEAD_TS = [63, 65]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
CODE_KINDS = np.array(list(range(-3, 9)) + [I32_MIN, I32_MAX], dtype=np.int64)
SENTINEL = 7.0


def lds_p(n):
    """pq_factor_rank's padded LDS row: the next power of two >= max(16, n)"""
    P = 16
    while P < n:
        P <<= 1
    return P


# the case tables reach every value the branch table names (checked at import, with or without a GPU)
assert {lds_p(n) for n in BUILD_NS} == {16 << i for i in range(11)} and {n for n in BUILD_NS if n == lds_p(n)} >= {16, 32, 128, 256, 512}
assert {n % 8 for n in AHEAD_NS} == set(range(8)) and all(n > 256 for n in AHEAD_NS)


def build_c(name, cols, scalars, out=None):
    """one D-20 entry point through the C ABI on device columns of one row pitch -> out [N, T] at that pitch, prefilled with SENTINEL"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch, check, lib
    n, T = cols[0].shape
    pitch = max(int(cols[0].stride(0)), T)
    assert all(max(int(c.stride(0)), T) == pitch and tuple(c.shape) == (n, T) for c in cols)
    if out is None:
        out = torch.full((n, pitch), SENTINEL, dtype=torch.float64, device="cuda")[:, :T]
    b = Batch(n, T, pitch)
    check(getattr(lib(), name)(api.ctx(), C.byref(b), *[C.c_void_p(c.data_ptr()) for c in cols], *scalars, C.c_void_p(out.data_ptr())))
    return out


def check_mid_descending(f, fd, tag):
    """mode 2 with descending = 1: (n + 1 - rank - 0.5) / n, which only the C ABI accepts"""
    got = build_c("pq_factor_rank", [fd], (C.c_int32(2), C.c_int32(1)))
    BG.same(f"rank mode=2 descending=1 {f.shape} {tag}", got.cpu().numpy(), R.rank(f, "quantile", True))


def build_days(n, seed):
    """size_days' five days and a sixth on which every symbol is NULL; day 2 has at least one NULL"""
    f, _ = size_days(n, 6, seed)
    f[n // 2, 2] = X.NULL
    f[:, 5] = X.NULL
    return f


@pytest.mark.parametrize("n", BUILD_NS, ids=[f"n{n}" for n in BUILD_NS])
def test_build_rank_sort_sizes(pq, n):
    """the rank family on both sides of every LDS sort size P = 16 .. 16 384: four rank variants, normalize("quantile") and the
    descending mid-rank.  Days 0, 1 and 3 are full rows (at n == P no +inf tail: the last slot of both binary searches), day 0 is one
    tie run of n, day 4 has 1 - 3 members under a +inf tail, day 5 none (the return before the barrier)."""
    pitch = 11 if n == 257 else None
    f = build_days(n, 1100 + n)
    nv = R.valid(f).sum(axis=0)
    assert (nv[[0, 1, 3]] == n).all() and 1 <= nv[2] < n and 1 <= nv[4] <= 3 and nv[5] == 0
    assert (f[:, 0] == f[0, 0]).all() and np.signbit(f[f[:, 3] == 0.0, 3]).any() and not np.signbit(f[f[:, 3] == 0.0, 3]).all()
    fd = BG.to_dev(f, pitch)
    got = BG.check_rank(pq, f, fd, tag=f"pitch={pitch}")
    assert pitch is None or got.stride(0) == pitch
    check_mid_descending(f, fd, f"pitch={pitch}")


def wide_days(n, seed):
    """four days: every key equal; every symbol NULL; one member; ties, zeros of both signs and ~5 % NULL / NaN / +-inf"""
    rng = np.random.default_rng(seed)
    f = np.full((n, 4), X.NULL)
    f[:, 0] = -2.5
    f[n // 3, 2] = 0.75
    d = np.round(rng.standard_normal(n) * 4.0) / 4.0
    d[(d == 0.0) & (rng.random(n) < 0.5)] = -0.0
    for v in (X.NULL, np.nan, np.inf, -np.inf):
        d[rng.random(n) < 0.0125] = v
    f[:, 3] = d
    return f


@pytest.mark.parametrize("n", [16385, 100000], ids=["n16385", "n100000"])
def test_build_wide_path(pq, n):
    """n > 16 384: ranks from rocPRIM's segmented sort and xs_sort_wide_kernel, one symbol above the LDS limit and at the documented
    limit; n = 16 385 also at an odd row pitch"""
    f = wide_days(n, n)
    nv = R.valid(f).sum(axis=0)
    z = f[f[:, 3] == 0.0, 3]
    assert nv[:3].tolist() == [n, 0, 1] and 0.9 * n < nv[3] < 0.97 * n and np.signbit(z).any() and not np.signbit(z).all()
    assert len(np.unique(f[R.valid(f[:, 3]), 3])) < 60                      # long tie runs
    for pitch in (None, 5) if n == 16385 else (None,):
        fd = BG.to_dev(f, pitch)
        got = BG.check_rank(pq, f, fd, tag=f"pitch={pitch}")
        assert pitch is None or got.stride(0) == pitch
        check_mid_descending(f, fd, f"pitch={pitch}")


def test_build_above_the_limit(pq):
    """n = 100 001: the rank family raises, naming the limit, and writes nothing; the methods that sort nothing have no limit; an
    ordinary call on the same context computes afterwards"""
    from polars_quant_amd._lib import PqError
    n, T = 100001, 3
    f, w, grp = BG.make("special", n, T, 21)
    assert grp.shape == (n, T) and grp.max() == 5 and grp.min() == -1
    fd, wd = BG.to_dev(f), BG.to_dev(w)
    F = pq.Factor()
    for call in (lambda: F.rank(fd), lambda: F.rank(fd, ascending=False, pct=True), lambda: F.normalize(fd, "quantile")):
        with pytest.raises(PqError, match="at most 100000"):
            call()
    out = torch.full((n, T), SENTINEL, dtype=torch.float64, device="cuda")
    for mode, desc in ((0, 0), (1, 1), (2, 0), (2, 1)):
        with pytest.raises(PqError, match="at most 100000"):
            build_c("pq_factor_rank", [fd], (C.c_int32(mode), C.c_int32(desc)), out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "out was written by a refused call"
    BG.check_blocked(pq, f, w, grp, fd, wd)
    g256 = np.random.default_rng(22).integers(0, 256, n)
    assert g256.max() == 255
    BG.same("weighted G=256 n=100001", F.weighted(fd, wd, g256).cpu().numpy(), R.weighted(f, w, g256, 256))
    BG.check_binary(pq, f, w, fd, wd)
    BG.check_rank(pq, build_days(300, 23), tag="after the refusals")


@pytest.mark.parametrize("n,T", TILE_CASES, ids=[f"n{n}-T{t}" for n, t in TILE_CASES])
def test_build_tiles(pq, n, T):
    """the 32 x 32 tiles of xs_prep_kernel / bd_transpose_kernel with a symbol-tile edge and a day-tile edge at once, one day, many day
    tiles over few symbols, and the 64-day (day, block) passes: every method; the last cell of the table is in every sample"""
    pitch = 37 if (n, T) == (32, 33) else None
    f, w, grp = BG.make("special", n, T, 100 * n + T)
    f[-1, -1], w[-1, -1], grp[-1, -1] = 0.5, 2.0, 0
    f[0, -1], w[0, -1], grp[0, -1] = -0.5, 3.0, 0                  # a second member on the last day: minmax has a range
    assert grp.shape == (n, T)
    for exp in (R.rank(f), R.minmax(f), R.weighted(f, w), R.weighted(f, w, grp)):
        assert not R.isnull(exp[-1, -1]) and not R.isnull(exp[0, -1])
    fd, wd = BG.to_dev(f, pitch), BG.to_dev(w, pitch)
    tag = f"pitch={pitch}"
    BG.check_rank(pq, f, fd, tag=tag)
    check_mid_descending(f, fd, tag)
    got = BG.check_blocked(pq, f, w, grp, fd, wd, tag=tag)
    assert pitch is None or got.stride(0) == pitch
    BG.check_binary(pq, f, w, fd, wd, tag=tag)


@pytest.mark.parametrize("T", AHEAD_TS, ids=[f"T{t}" for t in AHEAD_TS])
@pytest.mark.parametrize("n", AHEAD_NS, ids=[f"n{n}" for n in AHEAD_NS])
def test_build_look_ahead(pq, n, T):
    """bd_minmax_kernel / bd_weighted_kernel read 8 symbols ahead, clamped to the block's last: every n % 8 in the last of several
    blocks, both sides of the 64-day pass.  The last symbol is in every day's sample, with the largest factor of the day (the first with
    the smallest)."""
    for kind in ("special", "discrete"):
        f, w, grp = BG.make(kind, n, T, 7 * n + T)
        f[-1], w[-1] = 40.0, 3.0
        f[0], w[0] = -40.0, 2.0                                     # a second member on every day: minmax has a range
        grp[-1] = grp[0] = 0
        for exp in (R.minmax(f), R.weighted(f, w), R.weighted(f, w, grp)):
            assert not R.isnull(exp[-1]).any()
        BG.check_blocked(pq, f, w, grp, tag=kind)


def test_build_group_codes_outside_the_range(pq):
    """pq_factor_weighted with n_groups below the largest code: codes >= G, negative codes and the extreme int32 values are outside
    every group (NULL, and in no sum).  [N, T] codes sit at a group_stride above the batch stride; the pad columns hold code 0, a live
    group, so a read off the pitch changes a sum."""
    n, T, G = 521, 70, 4
    f, w, _ = BG.make("special", n, T, 41)
    fd, wd = BG.to_dev(f), BG.to_dev(w)
    ok = R.valid(f) & R.valid(w)
    rng = np.random.default_rng(42)

    def run(codes, n_groups, gs):
        if codes.ndim == 1:
            gd = torch.from_numpy(codes.astype(np.int32)).cuda()
        else:
            gd = torch.zeros((n, gs), dtype=torch.int32, device="cuda")
            gd[:, :T] = torch.from_numpy(codes.astype(np.int32)).cuda()
        got = build_c("pq_factor_weighted", [fd, wd], (C.c_void_p(gd.data_ptr()), C.c_int64(gs), C.c_int32(n_groups)))
        exp = R.weighted(f, w, codes, n_groups)
        BG.same(f"weighted n_groups={n_groups} codes{list(codes.shape)} group_stride={gs}", got.cpu().numpy(), exp)
        return exp

    for shape, gs in (((n,), 0), ((n, T), T + 5)):
        codes = rng.choice(CODE_KINDS, shape)
        c2 = np.broadcast_to(codes[:, None] if codes.ndim == 1 else codes, (n, T))
        for kind in (c2 < 0, (c2 >= G) & (c2 < 9), c2 == I32_MIN, c2 == I32_MAX):
            assert (kind & ok).any()                                   # each kind falls on a cell whose factor and weight are valid
        exp = run(codes, G, gs)
        assert R.isnull(exp[(c2 < 0) | (c2 >= G)]).all()
        assert all(not R.isnull(exp[c2 == g]).all() for g in range(G))
        high = rng.choice(CODE_KINDS[CODE_KINDS >= 1], shape)
        assert R.isnull(run(high, 1, gs)).all()


def test_build_binary_grid_stride(pq):
    """bd_binary_kernel launches at most 2^20 workgroups and walks the rest with a grid stride.  (2^20 + 3, 1): chunks = 1, three
    series on the second step, compared in full.  (524 289, 257): chunks = 2, total = 2^20 + 2, so series 524 288 is the second step and
    s = w / chunks matters there; inputs drawn on the device in [1, 2), no result is the sentinel 7.0 the output starts from."""
    ops = ("ratio", "diff", "reldiff")
    n, T = (1 << 20) + 3, 1
    assert -(-T // 256) * n == (1 << 20) + 3
    rng = np.random.default_rng(51)
    a, b = 1.0 + rng.random((n, T)), 1.0 + rng.random((n, T))
    ad, bd = BG.to_dev(a), BG.to_dev(b)
    for op, name in enumerate(ops):
        got = build_c("pq_factor_binary", [ad, bd], (C.c_int32(op),))
        BG.same(f"{name} {n}x{T}", got.cpu().numpy(), R.binary(a, b, name), ieee_nan=True)
    n, T = 524289, 257
    assert -(-T // 256) == 2 and 2 * n == (1 << 20) + 2
    rows = [0, 1, 262144, 524287, 524288]
    g = torch.Generator(device="cuda")
    g.manual_seed(52)
    ad = torch.rand((n, T), dtype=torch.float64, device="cuda", generator=g).add_(1.0)
    bd = torch.rand((n, T), dtype=torch.float64, device="cuda", generator=g).add_(1.0)
    out = torch.empty((n, T), dtype=torch.float64, device="cuda")
    a, b = ad[rows].cpu().numpy(), bd[rows].cpu().numpy()
    for op, name in enumerate(ops):
        out.fill_(SENTINEL)
        build_c("pq_factor_binary", [ad, bd], (C.c_int32(op),), out=out)
        assert not bool((out == SENTINEL).any()), f"{name} {n}x{T}: cells were not written"
        BG.same(f"{name} {n}x{T} rows {rows}", out[rows].cpu().numpy(), R.binary(a, b, name), ieee_nan=True)
    del ad, bd, out
    torch.cuda.empty_cache()


SUB = 5e-324      # 2^-1074, the smallest subnormal


def edge_days(n=300, seed=61):
    """minmax days -> 0: every member +-0; 1: one member; 2: min = 0, max = 2^-1074; 3: members m * 2^-1074, m in 0 .. 1000; 4: members
    spanning +-1.5e308, the range overflows; 5: an ordinary day with NULLs"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 6))
    f[:, 0] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    f[:, 1] = X.NULL
    f[7, 1] = 3.0
    f[:, 2] = np.where(rng.random(n) < 0.5, 0.0, SUB)
    f[:3, 2] = -0.0, SUB, X.NULL
    f[:, 3] = rng.integers(0, 1001, n) * SUB
    f[:2, 3] = 0.0, 1000 * SUB
    f[:, 4] = rng.uniform(-1.5, 1.5, n) * 1e308
    f[:3, 4] = -1.5e308, 1.5e308, 0.0
    f[rng.random(n) < 0.05, 5] = X.NULL
    return f


def test_build_minmax_and_weight_edges(pq):
    """minmax on days that are dead (all +-0, one member), on subnormal ranges (f64 division of denormals: exact, m / 1000 correctly
    rounded) and on a range that overflows (the plain IEEE quotient: 0, or a NaN that is not NULL); weighted on a day whose W = +inf"""
    n = 300
    f = edge_days(n)
    exp = R.minmax(f)
    assert R.isnull(exp[:, :2]).all() and set(exp[R.valid(f[:, 2]), 2]) == {0.0, 1.0} and R.isnull(exp[2, 2])
    assert (exp[:, 3] == np.round(f[:, 3] / SUB) / 1000.0).all() and (exp[:, 3] > 0.0).any()
    over = exp[:, 4]
    assert (np.isnan(over) & ~R.isnull(over)).any() and (over == 0.0).any() and ((over == 0.0) | np.isnan(over)).all()
    got = pq.Factor().normalize(BG.to_dev(f), "minmax").cpu().numpy()
    keep = [0, 1, 2, 3, 5]
    BG.same("minmax edge days", got[:, keep], exp[:, keep])
    BG.same("minmax overflowing range", got[:, 4], over, ieee_nan=True)
    f, w, grp = BG.make("plain", n, 6, 62)
    w[:, 2] = 1e308
    for g in (None, grp):
        exp = R.weighted(f, w, g)
        assert ((exp[:, 2] == 0.0) | (np.isnan(exp[:, 2]) & ~R.isnull(exp[:, 2]))).all() and np.isnan(exp[:, 2]).any()
        assert (exp[:, 2] == 0.0).any() and not R.isnull(exp).any()
        got = pq.Factor().weighted(BG.to_dev(f), BG.to_dev(w), g).cpu().numpy()
        keep = [0, 1, 3, 4, 5]
        BG.same(f"weighted beside W = inf grouped={g is not None}", got[:, keep], exp[:, keep])
        BG.same(f"weighted W = inf grouped={g is not None}", got[:, 2], exp[:, 2], ieee_nan=True)


def test_build_workspace_reuse(pq):
    """one context: the wide rank (keys, counts, sorted keys, offsets and rocPRIM's temporary in ctx->ws), the LDS rank, the grouped
    weighted at G = 256, minmax, then the first call again; no result depends on what the call before left in the workspace"""
    F = pq.Factor()
    rng = np.random.default_rng(71)
    fw = BG.size_class(20000, 4, 72)
    fw[rng.random(fw.shape) < 0.05] = X.NULL
    fwd = BG.to_dev(fw)
    exp_w = R.rank(fw, "pct", True)
    first = F.rank(fwd, ascending=False, pct=True).cpu().numpy()
    BG.same("wide rank, first", first, exp_w)
    BG.check_rank(pq, build_days(300, 73), tag="after the wide rank")
    f, w, _ = BG.make("special", 700, 40, 74)
    grp = rng.integers(-1, 256, 700)
    grp[0] = 255
    BG.same("weighted G=256 after the ranks", F.weighted(f, w, grp).cpu().numpy(), R.weighted(f, w, grp, 256))
    f, _, _ = BG.make("special", 513, 20, 75)
    BG.same("minmax after weighted", F.normalize(f, "minmax").cpu().numpy(), R.minmax(f))
    again = F.rank(fwd, ascending=False, pct=True).cpu().numpy()
    BG.same("wide rank, again", again, exp_w)
    BG.same("wide rank, again against first", again, first)


def test_sorts_workspace_reuse(pq):
    """one context, six calls through the one workspace layout of the cells stage: one key row and five cells, two key rows and 25
    cells in LDS tiles, two cells, the wide tail behind two key rows and six register cells, the rank's own layout, then the first
    call again; every call against its reference, and no result depends on what the call before left in the workspace"""
    f, r = S.make("nulls", 300, 131, 81)
    first = S.check_groups(pq, f, r, 0, 5)
    a, b, r2 = DS.make("nulls", 300, 131, 82)
    DS.check(a, b, r2, 5, 5, True)
    S.check_groups(pq, f, r, 1, 0, 0.3, 0.3)
    DS.check(*DS.sized(16385, 4, 83), 2, 3, False)
    BG.check_rank(pq, build_days(300, 84), tag="after the wide double sort")
    again = S.check_groups(pq, f, r, 0, 5)
    for k, v in first.items():
        assert again[k].shape == v.shape and torch.equal(DS.bits(again[k]), DS.bits(v)), k
