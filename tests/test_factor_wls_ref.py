"""not-gpu: the numpy restatement of decision D-32 (tests/xsec_wls_ref.py: the weighted cross-sectional regression with industry
dummies) against an example derived by hand, against numpy.linalg.lstsq on the sqrt(w)-scaled [F | dummies] design day by day, bit for
bit against the restatement of D-17 (tests/xsec_regress_ref.py) under unit weights and one group, its invariances (doubled weights,
relabelled industries), one constructed day per NULL rule; the public surface, the argument refusals that need no device, and the
register / scratch figures of csrc/xsec/wls.hip."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import xsec_regress_ref as R17
import xsec_wls_cases as cases
import xsec_wls_ref as R

ROOT = Path(__file__).resolve().parents[1]


def same(got, exp, what=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, what
    assert (got.view(np.uint64) == exp.view(np.uint64)).all(), (what, got, exp)


# ---------------------------------------------------------------- by hand
def test_hand_derived_example():
    """Two industries A (code 0) and B (code 1) of three symbols each, weights (1, 1, 2) in both, so W_A = W_B = 4; K = 1.
      f:  A (1.5, 1.5, -0.5)          S = 1.5 + 1.5 + 2(-0.5) = 2  -> m_A[f] = 0.5,   d_f = ( 1,  1, -1)
          B (0.75, 0.75, 2.75)        S = 0.75 + 0.75 + 5.5 = 7    -> m_B[f] = 1.75,  d_f = (-1, -1,  1)
      r = g + 0.25 f + e with g_A = 0.75, g_B = -2.25 and e = (0.75, -0.25, -0.25) in both (sum w e = 0 in each industry, and
          sum w d_f e = +1 in A, -1 in B: orthogonal to the factor):
          A (1.875, 0.875, 0.375)     S = 3.5   -> m_A[r] = 0.875,    d_r = ( 1,     0,    -0.5)
          B (-1.3125, -2.3125, -1.8125)  S = -7.25 -> m_B[r] = -1.8125,  d_r = ( 0.5,  -0.5,   0)
      C = sum w d_f^2 = 4 + 4 = 8;  c = sum w d_f d_r = (1 + 0 + 1) + (-0.5 + 0.5 + 0) = 2;  b = c / C = 0.25.
      Srr = sum w d_r^2 = (1 + 0 + 0.5) + (0.25 + 0.25 + 0) = 2;  SSE = sum w e^2 = 2 (0.5625 + 0.0625 + 0.125) = 1.5 (= Srr - b c).
      n = 6, G_t = 2: df = 6 - 1 - 2 = 3, s^2 = 0.5.  V_b = 1 / 8: se = sqrt(1 / 16) = 0.25, t = 1.
      g_A = 0.875 - 0.25 * 0.5 = 0.75,  V = 1 / 4 + 0.5^2 / 8 = 9 / 32:  se = sqrt(9 / 64) = 0.375,  t = 2.
      g_B = -1.8125 - 0.25 * 1.75 = -2.25,  V = 1 / 4 + 1.75^2 / 8 = 81 / 128:  se = sqrt(81 / 256) = 0.5625,  t = -4.
      R^2 within = 1 - 1.5 / 2 = 0.25.  rbar = (3.5 - 7.25) / 8 = -0.46875, and Stot = Srr + 4 (0.875 + 0.46875)^2 + 4 (-1.8125 +
      0.46875)^2 = 2 + 2 * 2.6875^2 = 16.4453125, every term a dyadic number: R^2 total = 1 - 1.5 / 16.4453125 (the one value here that
      is rounded).  resid = e.  The symbols are interleaved A, B, A, B, A, B."""
    f = np.array([1.5, 0.75, 1.5, 0.75, -0.5, 2.75])[:, None]
    r = np.array([1.875, -1.3125, 0.875, -2.3125, 0.375, -1.8125])[:, None]
    w = np.array([1.0, 1.0, 1.0, 1.0, 2.0, 2.0])[:, None]
    ind = np.array([0, 1, 0, 1, 0, 1])
    out = R.wls([f], r, w, ind)
    assert out["n"].tolist() == [6] and out["gt"].tolist() == [2] and out["ok"].tolist() == [True]
    same(out["coef"][:, 0], [0.25, 0.75, -2.25])
    same(out["t"][:, 0], [1.0, 2.0, -4.0])
    same(out["r2"][:, 0], [1.0 - 1.5 / 16.4453125, 0.25])
    same(out["resid"][:, 0], [0.75, 0.75, -0.25, -0.25, -0.25, -0.25])
    np.testing.assert_allclose(out["p"][:, 0], R.t_pvalue(np.array([1.0, 2.0, -4.0]), 3.0), rtol=0, atol=0)
    assert 0.39 < out["p"][0, 0] < 0.40                     # P(|t_3| > 1) = 0.391


# ---------------------------------------------------------------- numpy.linalg.lstsq, day by day
def lstsq_days(F, r, w, ind, G, days):
    K, N, T = F.shape
    mem = R.sample(F, r, w, ind, G)
    coef = np.full((K + G, T), np.nan)
    for t in days:
        m = mem[:, t]
        present = [g for g in range(G) if (m & (ind[:, t] == g)).any()]
        sw = np.sqrt(w[m, t])
        A = np.column_stack([F[j][m, t] for j in range(K)] + [(ind[m, t] == g).astype(np.float64) for g in present]) * sw[:, None]
        sol = np.linalg.lstsq(A, r[m, t] * sw, rcond=None)[0]
        coef[:K, t] = sol[:K]
        coef[[K + g for g in present], t] = sol[K:]
    return coef


LSTSQ_BOUND = 1e-12


def test_against_lstsq():
    """Well-conditioned inputs (xsec_wls_cases.panel: independent N(0, 1) factors, log-normal weights, holes in every column), K = 3
    with G = 7 at 200 x 12 and K = 8 with G = 31 at 400 x 8, [N, T] codes.  The deviation is max |restatement - lstsq| / max |lstsq| over
    the coefficient rows (factors and industries) of the solved days.  Measured on these inputs: 2.12e-15 at K = 3, G = 7 and 2.01e-15
    at K = 8, G = 31 (the two differ only in rounding order); the bound is 64 x the larger = 1.36e-13, rounded up to a power of ten:
    1e-12."""
    worst = 0.0
    for K, G, N, T, seed in ((3, 7, 200, 12, 32), (8, 31, 400, 8, 33)):
        F, r, w, ind = cases.panel(K, N, T, G, seed)
        out = R.wls(list(F), r, w, ind, G)
        assert out["ok"].all()
        exp = lstsq_days(F, r, w, ind, G, range(T))
        got = out["coef"]
        assert (R.isnull(got) == np.isnan(exp)).all()        # the rows of an industry without a member, and only those
        live = ~np.isnan(exp)
        dev = np.abs(got[live] - exp[live]).max() / np.abs(exp[live]).max()
        print(f"lstsq deviation K={K} G={G}: {dev:.3e}")
        worst = max(worst, dev)
    assert worst <= LSTSQ_BOUND, worst


# ---------------------------------------------------------------- bit for bit on the restatement
@pytest.mark.parametrize("K", [1, 3, 8])
def test_unit_weights_one_group_is_d17(K):
    """all-ones weights and all-zero codes: D-17's regression bit for bit (the group's row is the intercept, R^2 total = within)"""
    N, T = 300, 9
    F, r, _, _ = cases.panel(K, N, T, 1, 40 + K, codes=None)
    F[K - 1, :, 0] = F[0, :, 0] if K > 1 else 2.5           # a singular day
    r[K + 1:, 1] = R.NULL                                    # n = K + 1: one short of D-17's K + 2
    exp = R17.regress_units(F, r, R17.sample(F, r))
    for w, ind in ((np.ones((N, T)), np.zeros(N, dtype=np.int32)), (None, None), (np.ones((N, T)), np.zeros((N, T), dtype=np.int32))):
        got = R.wls(list(F), r, w, ind)
        for k in ("coef", "t", "p"):
            same(got[k], exp[k], k)
        same(got["r2"][0], exp["r2"])
        same(got["r2"][1], exp["r2"])
        assert (got["n"] == exp["n"]).all() and got["n"].dtype == np.int32
        assert R.isnull(got["coef"][:, :2]).all() and not R.isnull(got["coef"][:, 2:]).any()


def test_doubling_every_weight_changes_no_bit():
    F, r, w, ind = cases.panel(3, 150, 7, 5, 51)
    a, b = R.wls(list(F), r, w, ind, 5), R.wls(list(F), r, 2.0 * w, ind, 5)
    assert a["ok"].all()
    for k in ("coef", "t", "r2", "resid", "p"):
        same(a[k], b[k], k)
    assert (a["n"] == b["n"]).all() and (a["gt"] == b["gt"]).all()


def test_relabelling_the_industries_permutes_their_rows():
    K, G = 3, 6
    F, r, w, ind = cases.panel(K, 150, 7, G, 52)
    perm = np.array([4, 2, 5, 0, 3, 1])
    ind2 = np.where((ind >= 0) & (ind < G), perm[np.clip(ind, 0, G - 1)], ind).astype(np.int32)
    a, b = R.wls(list(F), r, w, ind, G), R.wls(list(F), r, w, ind2, G)
    assert a["ok"].all()
    for k in ("coef", "t", "p"):
        same(a[k][:K], b[k][:K], k)
        same(a[k][K:], b[k][K:][perm], k)
    same(a["resid"], b["resid"])
    same(a["r2"][1], b["r2"][1])                             # (rbar adds the industries in another order: R^2 total may differ in rounding)


# ---------------------------------------------------------------- NULL rules
@pytest.mark.parametrize("K,G", [(2, 3), (1, 2), (8, 5)])
def test_null_rules_one_constructed_day_each(K, G):
    N = 64
    kinds = cases.kinds_for(K, G, True)
    T = len(kinds) + 2
    F, r, w, ind = cases.panel(K, N, T, G, 60 + K, holes=0)
    day_of = {k: 1 + i for i, k in enumerate(kinds)}         # days 0 and T - 1 stay plain
    cases.put_special(F, r, w, ind, G, day_of, 61)
    out = R.wls(list(F), r, w, ind, G)
    unsolved = sorted(day_of[k] for k in kinds if k in cases.UNSOLVED)
    assert np.flatnonzero(~out["ok"]).tolist() == unsolved   # exactly these days lack a solution
    g2 = min(G, 4)
    for k in kinds:
        t = day_of[k]
        if k in cases.UNSOLVED:
            assert R.isnull(out["coef"][:, t]).all() and R.isnull(out["t"][:, t]).all() and R.isnull(out["p"][:, t]).all()
            assert R.isnull(out["r2"][:, t]).all() and R.isnull(out["resid"][:, t]).all()
            assert out["gt"][t] == g2
    t = day_of["short"]
    assert out["n"][t] == K + g2                             # one short of K + G_t + 1
    assert out["n"][day_of["const"]] == N
    if "collinear" in day_of:
        assert out["n"][day_of["collinear"]] == N
    t = day_of["empty"]
    present = np.array([g < g2 and g != 1 for g in range(G)])
    assert out["gt"][t] == g2 - 1 and out["n"][t] == N - (np.arange(N) % g2 == 1).sum()
    assert (R.isnull(out["coef"][K:, t]) == ~present).all() and (R.isnull(out["t"][K:, t]) == ~present).all()
    assert not R.isnull(out["coef"][:K, t]).any() and not R.isnull(out["r2"][:, t]).any()
    t = day_of["badw"]
    assert out["n"][t] == N - 5 and R.isnull(out["resid"][:5, t]).all() and not R.isnull(out["resid"][5:, t]).any()
    t = day_of["badcode"]
    assert out["n"][t] == N - 2 and R.isnull(out["resid"][:2, t]).all() and not R.isnull(out["resid"][2:, t]).any()
    t = day_of["perfect"]
    g_p = min(G, 2)
    assert out["n"][t] == 32 and out["gt"][t] == g_p
    same(out["coef"][:K, t], 0.25 * np.arange(1, K + 1) - 1.0)
    same(out["coef"][K:K + g_p, t], [0.5, -1.5][:g_p])
    assert R.isnull(out["t"][:, t]).all() and R.isnull(out["p"][:, t]).all()
    same(out["resid"][:32, t], np.zeros(32))
    same(out["r2"][1, t], 1.0)


def test_fm_summary_rows():
    K, G = 2, 3
    F, r, w, ind = cases.panel(K, 80, 20, G, 70)
    out = R.wls(list(F), r, w, ind, G)
    s = R.fm_summary(out["coef"])
    assert s.shape == (K + G, 5) and (s[:, 0] == 20).all()


# ---------------------------------------------------------------- the surface
def test_the_surface():
    import polars_quant_amd as pq
    from polars_quant_amd import _lib, api
    sig = inspect.signature(api.xsec_regress_wls)
    assert list(sig.parameters) == ["factors", "fwd_return", "weight", "industry", "summary", "resid"]
    sig = inspect.signature(pq.Factor.pure_factor_return)
    assert list(sig.parameters) == ["self", "factors", "next_return", "weight", "industry", "specific_return"]
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    decl = re.search(r"pq_status\s+pq_xsec_regress_wls\s*\(([^)]*)\)", txt)
    assert decl, "pq_xsec_regress_wls is not declared"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "pq_ctx *", "const pq_batch *", "const double *const *factors", "int32_t k", "const double *fwd_return", "const double *weight",
        "const int32_t *group", "int64_t group_stride", "int32_t n_groups", "double *coef", "double *t_stat", "double *p_value",
        "double *r2", "int32_t *n_obs", "int32_t *n_groups_present", "double *resid", "double *summary"]
    assert re.search(r"^xsec_regress_wls\s+i\s+pBpippplipppppppp$", _lib._SIGNATURES, flags=re.M)
    mk = (ROOT / "polars_quant_amd" / "csrc" / "Makefile").read_text()
    assert "xsec/wls.hip" in mk and mk.count("xsec/wls.resources.txt") == 1
    assert "polars_quant_amd/csrc/xsec/wls.resources.txt" in (ROOT / ".gitignore").read_text().split()


ONES = np.ones((6, 10))


@pytest.mark.parametrize("call, msg", [
    (lambda a: a.xsec_regress_wls([ONES], ONES, industry=np.zeros(6)), "integer codes"),
    (lambda a: a.xsec_regress_wls([ONES], ONES, industry=np.zeros(5, dtype=np.int32)), "industry must be"),
    (lambda a: a.xsec_regress_wls([ONES], ONES, industry=np.zeros((6, 1), dtype=np.int32)), "industry must be"),
    (lambda a: a.xsec_regress_wls([ONES], ONES, industry=np.full(6, 256)), "< 256"),
    (lambda a: a.xsec_regress_wls([ONES], ONES, weight=np.ones(10)), "weight must have"),
    (lambda a: a.xsec_regress_wls([ONES] * 9, ONES), "number of factors"),
    (lambda a: a.xsec_regress_wls([np.ones((6, 9))], ONES), "factor 0"),
])
def test_argument_refusals_without_a_device(call, msg):
    from polars_quant_amd import api
    with pytest.raises(ValueError, match=msg):
        call(api)


# ---------------------------------------------------------------- the kernels' resources
def test_no_kernel_uses_scratch():
    """The build writes the register / scratch figures of csrc/xsec/wls.hip (wls.resources.txt, from hipcc's kernel-resource-usage
    remarks): the pass-1, pass-2, pass-3, solve, final and industry kernels once per K = 1 .. 8, the three untemplated ones and the
    shared summary kernel, none with scratch or a spilled VGPR."""
    path = ROOT / "polars_quant_amd" / "csrc" / "xsec" / "wls.resources.txt"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    found = re.findall(r"Function Name: \S*?\d+((?:wl|rg)_\w+?_kernel)(?:ILi(\d+)E(?:Li(\d+)E)?)?\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: "
                       r"(\d+)\s+Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)", path.read_text())
    want = [(k, K, -1) for K in range(1, 9) for k in ("wl_pass1_kernel", "wl_solve_kernel", "wl_final_kernel", "wl_industry_kernel")] + \
           [("wl_pass_kernel", K, P) for K in range(1, 9) for P in (2, 3)] + \
           [(k, -1, -1) for k in ("wl_gsum_kernel", "wl_day_kernel", "wl_means_kernel", "rg_summary_kernel")]
    assert sorted((k, int(K) if K else -1, int(P) if P else -1) for k, K, P, *_ in found) == sorted(want)
    for k, K, P, vgprs, scratch, occ, spill in found:
        assert int(scratch) == 0 and int(spill) == 0, (k, K, P, vgprs, scratch, occ, spill)
