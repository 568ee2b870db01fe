"""not-gpu: pins tests/xsec_double_ref.py, the numpy restatement of the two-way sort (decision D-31) that the GPU tests compare with:
a hand-derived example, an independent composite-key formulation of the labels, the control marginals and the no-cell rule."""
import numpy as np
import pytest

import xsec_double_ref as D
import xsec_ref as X

KEY_A = float(2 ** 18)


def tie_m(keys):
    """m = a + b of every key's tie run [a, b) in the ascending sort of `keys` (finite; -0 == +0)"""
    s = np.sort(keys)
    return np.searchsorted(s, keys, "left") + np.searchsorted(s, keys, "right")


def composite_label_day(a, b, r, qa, qb, dependent):
    """the labels of one day without xsec_ref: integer tie-run sums, and for the dependent mode ONE sort of the key la * 2^18 + m_B
    with the tie runs taken inside each bucket's key range"""
    ok = X.valid(a) & X.valid(b) & X.valid(r)
    n = int(ok.sum())
    out = np.full(a.shape[0], X.LABEL_OUT, dtype=np.uint8)
    if n < (qa if dependent else max(qa, qb)):
        return out
    la = tie_m(a[ok]) * qa // (2 * n)
    mb = tie_m(b[ok])
    if not dependent:
        out[ok] = la * qb + mb * qb // (2 * n)
        return out
    key = la.astype(np.float64) * KEY_A + mb.astype(np.float64)
    assert np.array_equal(key.astype(np.int64), la * 2 ** 18 + mb)          # exact in f64
    s = np.sort(key)
    lo = np.searchsorted(s, la * KEY_A, "left")
    hi = np.searchsorted(s, (la + 1) * KEY_A, "left")
    na = hi - lo
    m = np.searchsorted(s, key, "left") + np.searchsorted(s, key, "right") - 2 * lo
    out[ok] = np.where(na < qb, X.LABEL_MID, la * qb + m * qb // (2 * np.maximum(na, 1)))
    return out


def make(kind, n, T, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, T))
    b = 0.5 * a + rng.standard_normal((n, T))
    r = 0.1 * b + rng.standard_normal((n, T)) * 0.02
    if kind == "nulls":
        for x in (a, b, r):
            x[rng.random((n, T)) < 0.06] = X.NULL
        a[rng.random((n, T)) < 0.02] = np.nan
        b[rng.random((n, T)) < 0.02] = np.inf
        r[rng.random((n, T)) < 0.02] = -np.inf
    elif kind == "discrete":
        a = rng.integers(-1, 2, (n, T)).astype(np.float64)
        b = rng.integers(-1, 2, (n, T)).astype(np.float64)
        a[(a == 0) & (rng.random((n, T)) < 0.5)] = -0.0
        b[(b == 0) & (rng.random((n, T)) < 0.5)] = -0.0
    elif kind == "same":
        b = a.copy()
    return a, b, r


def test_hand_derived_2x2_on_8_symbols():
    """8 symbols, 2 days, Qa = Qb = 2, n = 8 on both days.

    control A = 1 .. 8 on both days: m_A = 1, 3, .., 15, la = floor(2 m / 16) = 0 for symbols 0-3 and 1 for symbols 4-7.
    day 0: B = 10 40 20 30 | 50 45 60 55, r = 0.5 1 1.5 2 | 2.5 3 3.5 4.5.
      independent: B ascending is s0 s2 s3 s1 s5 s4 s7 s6, lb = 0 for the first four: cells 0 0 0 0 | 3 3 3 3.  Cells 1 and 2 are
        empty, so their means and every spread and average are NULL; mean[0] = 5 / 4 = 1.25, mean[3] = 13.5 / 4 = 3.375.
      dependent: bucket 0 holds 10 40 20 30 -> lb 0 1 0 1; bucket 1 holds 50 45 60 55 -> lb 0 0 1 1: cells 0 1 0 1 | 2 2 3 3.
        means: cell 0 = (0.5 + 1.5) / 2 = 1.0, cell 1 = (1 + 2) / 2 = 1.5, cell 2 = (2.5 + 3) / 2 = 2.75, cell 3 = (3.5 + 4.5) / 2 = 4.0.
        spread_factor = 1.5 - 1.0 = 0.5 and 4.0 - 2.75 = 1.25, average (0.5 + 1.25) / 2 = 0.875.
        spread_control = 2.75 - 1.0 = 1.75 and 4.0 - 1.5 = 2.5, average (1.75 + 2.5) / 2 = 2.125.
    day 1: B of s0 and s1 swapped (40 10), and B of s6 = s7 = 55 (a tie), same r.
      dependent: bucket 0 -> lb 1 0 0 1 (cells 1 0 0 1); bucket 1 holds 50 45 55 55: m = 3, 1, 6, 6 -> lb = floor(2 m / 8) = 0 0 1 1.
        cell 0 = {s1, s2}: s1 is new -> turnover 1 / 2; cell 1 = {s0, s3}: s0 is new -> 1 / 2; cells 2 and 3 keep their members -> 0.
        means: cell 0 = (1 + 1.5) / 2 = 1.25, cell 1 = (0.5 + 2) / 2 = 1.25, cells 2 and 3 as on day 0.
        spread_factor = 0.0 and 1.25, average 0.625; spread_control = 1.5 and 2.75, average 2.125.
    """
    A = np.tile(np.arange(1.0, 9.0)[:, None], (1, 2))
    B = np.array([[10, 40, 20, 30, 50, 45, 60, 55], [40, 10, 20, 30, 50, 45, 55, 55]], dtype=np.float64).T.copy()
    r = np.tile(np.array([0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4.5])[:, None], (1, 2))
    dep = D.groups(A, B, r, 2, 2, True)
    assert dep["labels"][:, 0].tolist() == [0, 1, 0, 1, 2, 2, 3, 3]
    assert dep["labels"][:, 1].tolist() == [1, 0, 0, 1, 2, 2, 3, 3]
    assert dep["mean_return"].T.tolist() == [[1.0, 1.5, 2.75, 4.0], [1.25, 1.25, 2.75, 4.0]]
    assert dep["count"].tolist() == [[2, 2]] * 4
    assert X.isnull(dep["turnover"][:, 0]).all() and dep["turnover"][:, 1].tolist() == [0.5, 0.5, 0.0, 0.0]
    assert dep["spread_factor"].T.tolist() == [[0.5, 1.25, 0.875], [0.0, 1.25, 0.625]]
    assert dep["spread_control"].T.tolist() == [[1.75, 2.5, 2.125], [1.5, 2.75, 2.125]]
    ind = D.groups(A[:, :1], B[:, :1], r[:, :1], 2, 2, False)
    assert ind["labels"][:, 0].tolist() == [0, 0, 0, 0, 3, 3, 3, 3]
    assert ind["count"][:, 0].tolist() == [4, 0, 0, 4]
    assert ind["mean_return"][[0, 3], 0].tolist() == [1.25, 3.375] and X.isnull(ind["mean_return"][[1, 2], 0]).all()
    assert X.isnull(ind["spread_factor"]).all() and X.isnull(ind["spread_control"]).all()
    s = D.summary(dep)
    assert s.shape == (4 + 3 + 3, 5)
    assert s[0, :2].tolist() == [2.0, 1.125] and s[0, 4] == 0.5                 # cell 0: two days, mean of 1.0 and 1.25
    assert s[6, :2].tolist() == [2.0, 0.75] and X.isnull(s[6, 4])                # the averaged spread: (0.875 + 0.625) / 2
    assert s[9, :3].tolist() == [2.0, 2.125, 0.0] and X.isnull(s[9, 3])          # constant series: std 0, no sharpe


@pytest.mark.parametrize("kind", ["plain", "nulls", "discrete", "same"])
@pytest.mark.parametrize("dependent", [False, True], ids=["independent", "dependent"])
def test_labels_equal_the_composite_key_formulation(kind, dependent):
    mids = 0
    for n, T in ((1, 3), (2, 3), (7, 9), (23, 12), (60, 8)):
        a, b, r = make(kind, n, T, 100 + n)
        for qa, qb in ((2, 3), (3, 3), (5, 5), (10, 10), (2, 10), (10, 2)):
            got = D.labels(a, b, r, qa, qb, dependent)
            exp = np.stack([composite_label_day(a[:, t], b[:, t], r[:, t], qa, qb, dependent) for t in range(T)], axis=1)
            assert np.array_equal(got, exp), (kind, n, T, qa, qb)
            assert got[(got != X.LABEL_OUT) & (got != X.LABEL_MID)].max(initial=0) < qa * qb
            mids += int((got == X.LABEL_MID).sum())
    assert (mids > 0) == dependent          # the no-cell label belongs to the dependent mode alone


@pytest.mark.parametrize("dependent", [False, True], ids=["independent", "dependent"])
def test_count_marginals_are_the_single_sort_of_the_control(dependent):
    for kind in ("plain", "nulls", "discrete"):
        a, b, r = make(kind, 80, 6, 7)
        for qa, qb in ((2, 3), (5, 5), (3, 4)):
            res = D.groups(a, b, r, qa, qb, dependent)
            assert not (res["labels"] == X.LABEL_MID).any()
            ok = D.sample(a, b, r)
            one = X.groups(np.where(ok, a, X.NULL), r, 0, qa)
            assert np.array_equal(res["count"].reshape(qa, qb, -1).sum(axis=1), one["count"]), (kind, qa, qb)
            assert np.array_equal(res["labels"] == X.LABEL_OUT, one["labels"] == X.LABEL_OUT)


def test_no_cell_exactly_in_buckets_below_qb():
    seen = {False: 0, True: 0}
    for kind, n, T in (("plain", 7, 9), ("nulls", 37, 20), ("discrete", 12, 10)):
        a, b, r = make(kind, n, T, 3)
        for qa, qb in ((3, 3), (10, 10), (2, 10), (10, 2)):
            lab = D.labels(a, b, r, qa, qb, True)
            for t in range(T):
                ok = D.sample(a[:, t], b[:, t], r[:, t])
                if ok.sum() < qa:
                    assert (lab[:, t] == X.LABEL_OUT).all()
                    continue
                la = X.label_day(np.where(ok, a[:, t], X.NULL), r[:, t], 0, qa)
                for g in range(qa):
                    mem = la == g
                    small = mem.sum() < qb
                    if mem.any():
                        seen[bool(small)] += 1
                        assert ((lab[mem, t] == X.LABEL_MID) == small).all(), (kind, qa, qb, t, g)
                        if not small:
                            assert (lab[mem, t] // qb == g).all()
    assert seen[True] > 0 and seen[False] > 0


def test_dependent_rows_are_the_single_sort_of_the_masked_factor():
    """row a of the dependent result = D-15's quantiles of the factor masked to control bucket a (its OUT inside the bucket read as MID)"""
    a, b, r = make("nulls", 37, 12, 5)
    qa, qb = 3, 4
    res = D.groups(a, b, r, qa, qb, True)
    ctl = X.labels(np.where(D.sample(a, b, r), a, X.NULL), r, 0, qa)
    for g in range(qa):
        one = X.groups(np.where(ctl == g, b, X.NULL), r, 0, qb)
        for k in ("mean_return", "count", "turnover"):
            assert np.array_equal(res[k][g * qb:(g + 1) * qb].view(np.uint64 if k != "count" else np.int32),
                                  one[k].view(np.uint64 if k != "count" else np.int32)), (g, k)
        assert np.array_equal(res["spread_factor"][g].view(np.uint64), one["spread"].view(np.uint64))
