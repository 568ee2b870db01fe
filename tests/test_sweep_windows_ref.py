"""not-gpu: the host side of the walk-forward sweep (decision D-26): walk_forward_windows (polars_quant_amd/sweep.py), the numpy
restatement of pq_sweep_select's rule that test_sweep_windows_gpu.py compares the kernel with, api.sweep_windows, and the register /
scratch figures of the window and select kernels (csrc/sweep/sweep.resources.txt)."""
import os
import re

import numpy as np
import pytest


def select_ref(summary, train, test, col, maximize=True):
    """pq_sweep_select restated: summary [W, P, N, 8] (the layout api.backtest_sweep(..., windows=) returns); per fold f and symbol s
    the parameter sets of summary[train[f], :, s, col] are scanned in ascending order, a NaN counts as the worst value (-inf when
    maximizing, +inf when minimizing) and only a STRICTLY better value replaces the best so far: the lowest index wins a tie and an
    all-NaN column gives 0 -> (chosen [F, N] int32, in_sample [F, N, 8], out_sample [F, N, 8])"""
    summary = np.asarray(summary)
    _W, P, N, _ = summary.shape
    F = len(train)
    chosen = np.zeros((F, N), dtype=np.int32)
    ins, outs = np.zeros((F, N, 8)), np.zeros((F, N, 8))
    worst = -np.inf if maximize else np.inf
    for f in range(F):
        for s in range(N):
            best, bv = 0, None
            for p in range(P):
                v = summary[train[f], p, s, col]
                v = worst if np.isnan(v) else v
                if bv is None or (v > bv if maximize else v < bv):
                    best, bv = p, v
            chosen[f, s] = best
            ins[f, s] = summary[train[f], best, s]
            outs[f, s] = summary[test[f], best, s]
    return chosen, ins, outs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- walk_forward_windows -----------------------------------------------------------------------------------------------------------
def test_rolling_folds():
    from polars_quant_amd import walk_forward_windows
    w = walk_forward_windows(300, 100, 50)
    assert w.dtype == np.int64 and w.shape == (4, 2, 2)
    assert w[:, 0].tolist() == [[0, 100], [50, 150], [100, 200], [150, 250]]        # train [k step, k step + train)
    assert w[:, 1].tolist() == [[100, 150], [150, 200], [200, 250], [250, 300]]     # the test rows follow; step defaults to test
    # the issue's timing shape: 2 520 rows, 504 + 126 -> 16 folds
    w = walk_forward_windows(2520, 504, 126)
    assert w.shape == (16, 2, 2) and w[-1].tolist() == [[1890, 2394], [2394, 2520]]


def test_anchored_folds_and_an_explicit_step():
    from polars_quant_amd import walk_forward_windows
    w = walk_forward_windows(300, 100, 50, anchored=True)
    assert w[:, 0].tolist() == [[0, 100], [0, 150], [0, 200], [0, 250]]
    assert w[:, 1].tolist() == [[100, 150], [150, 200], [200, 250], [250, 300]]
    w = walk_forward_windows(300, 100, 50, step=70)
    assert w.tolist() == [[[0, 100], [100, 150]], [[70, 170], [170, 220]], [[140, 240], [240, 290]]]
    w = walk_forward_windows(300, 100, 50, step=70, anchored=True)
    assert w[:, 0].tolist() == [[0, 100], [0, 170], [0, 240]] and w[:, 1].tolist() == [[100, 150], [170, 220], [240, 290]]
    # overlapping test windows (step < test) are the caller's business
    assert walk_forward_windows(20, 10, 5, step=1).shape == (6, 2, 2)


def test_an_incomplete_last_fold_is_dropped():
    from polars_quant_amd import walk_forward_windows
    assert len(walk_forward_windows(299, 100, 50)) == 3            # the fourth test window would need row 299
    assert len(walk_forward_windows(300, 100, 50)) == 4
    assert walk_forward_windows(150, 100, 50).tolist() == [[[0, 100], [100, 150]]]
    for n in (150, 151, 199, 200, 201):
        w = walk_forward_windows(n, 100, 50)
        assert w[-1, 1, 1] <= n and (w[:, 1, 1] - w[:, 1, 0] == 50).all() and (w[:, 0, 1] == w[:, 1, 0]).all()


def test_walk_forward_windows_refusals():
    from polars_quant_amd import walk_forward_windows
    for kw in (dict(train=0, test=5), dict(train=5, test=0), dict(train=-1, test=5), dict(train=5, test=5, step=0),
               dict(train=5, test=5, step=-2)):
        with pytest.raises(ValueError, match="positive"):
            walk_forward_windows(100, **kw)
    for n in (0, 9, 149):
        with pytest.raises(ValueError, match="no fold"):
            walk_forward_windows(n, 100, 50)


def test_sweep_windows_table():
    from polars_quant_amd import api
    w = api.sweep_windows([[0, 5], [3, 9]])
    assert w.dtype == np.int64 and w.shape == (2, 2) and w.flags.c_contiguous
    assert api.sweep_windows(np.zeros((4, 2), dtype=np.int32)[::2]).shape == (2, 2)
    assert api.sweep_windows([]).shape == (0, 2)
    for bad in ([0, 5], [[0, 5, 7]], [[0.0, 5.0]], np.zeros((2, 2, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="windows"):
            api.sweep_windows(bad)


def test_the_surface():
    import inspect

    import polars_quant_amd as pq
    from polars_quant_amd import api
    for name in ("run", "run_rules", "ma", "macd", "rsi", "bband", "stoch", "cci", "adx", "breakout", "reversion", "grid"):
        assert inspect.signature(getattr(pq.ParameterSweep, name)).parameters["windows"].default is None, name
    for f in (api.backtest_sweep, api.backtest_sweep_rules):
        assert inspect.signature(f).parameters["windows"].default is None
    sig = inspect.signature(pq.ParameterSweep.walk_forward).parameters
    assert [sig[k].default for k in ("step", "anchored", "metric", "maximize")] == [None, False, "sharpe_ratio", True]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("train", "test", "step", "anchored", "metric", "maximize"))
    assert pq.SweepResult({}, None).windows is None
    r = pq.WalkForwardResult({"k": np.arange(3) * 10}, None, None, None, np.zeros((2, 4, 8)), np.ones((2, 4, 8)))
    assert (r.metric("sharpe_ratio") == 1).all() and (r.metric("sharpe_ratio", which="in") == 0).all() and r.metric("alpha").shape == (2, 4)
    with pytest.raises(KeyError):
        r.metric("nope")
    with pytest.raises(ValueError):
        r.metric("alpha", which="both")


# ---- the restatement of the select rule, on cases small enough to read ----------------------------------------------------------------
def test_select_ref_on_hand_made_columns():
    nan, inf = float("nan"), float("inf")
    W, P, N = 3, 5, 6
    s = np.zeros((W, P, N, 8))
    s[..., 0] = np.arange(W * P * N).reshape(W, P, N)               # tells the gathered rows apart
    cols = np.array([[1.0, 3.0, 3.0, 2.0, nan],                     # a tie of the maximum: the lower index; minimum 1.0 at 0
                     [nan, nan, nan, nan, nan],                     # all NaN: 0 both ways
                     [nan, -inf, -inf, nan, nan],                   # maximizing a NaN ties with -inf: index 0; minimizing -inf at 1
                     [nan, 2.0, inf, inf, -5.0],                    # +inf at 2; minimum -5.0 at 4
                     [-0.0, 0.0, -1.0, 0.0, nan],                   # -0.0 == 0.0: index 0
                     [nan, nan, 7.0, nan, 7.0]]).T                  # a NaN ranks last: 2 both ways
    s[1, :, :, 4] = cols
    chosen, ins, outs = select_ref(s, [1, 1], [2, 0], 4, True)
    assert chosen.tolist() == [[1, 0, 0, 2, 0, 2]] * 2
    assert (bits(ins[0]) == bits(s[1, chosen[0], np.arange(N)])).all() and (bits(outs[0]) == bits(s[2, chosen[0], np.arange(N)])).all()
    assert (bits(outs[1]) == bits(s[0, chosen[1], np.arange(N)])).all()
    chosen, _ins, _outs = select_ref(s, [1], [2], 4, False)
    assert chosen.tolist() == [[0, 0, 1, 4, 2, 2]]
    # what SweepResult.best() does on the same column (torch.argmax takes the first maximum)
    key = np.where(np.isnan(cols), -np.inf, cols)
    assert (np.argmax(key, axis=0) == select_ref(s, [1], [2], 4, True)[0][0]).all()


# ---- the figures of the build ---------------------------------------------------------------------------------------------------------
def test_window_and_select_kernels_use_no_scratch():
    """sixteen sweep_windows_kernel instantiations -- seven rules and the generic one, each with and without a benchmark -- and the select
    kernel: no scratch, no spilled VGPR, at least two waves per SIMD"""
    path = os.path.join(os.path.dirname(__file__), "..", "polars_quant_amd", "csrc", "sweep", "sweep.resources.txt")
    if not os.path.exists(path):
        pytest.skip("sweep.resources.txt not built (make -C polars_quant_amd/csrc)")
    txt = open(path).read()
    figures = r"\S*\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+Occupancy \[waves/SIMD\]: (\d+)\s+VGPRs Spill: (\d+)"
    found = re.findall(r"Function Name: \S*sweep_windows_kernelILi(n?\d)ELb([01])E" + figures, txt)
    assert sorted((r, b) for r, b, *_ in found) == sorted((r, b) for r in ("n1", "0", "1", "2", "3", "4", "5", "6") for b in "01")
    select = re.findall(r"Function Name: \S*(sweep_select_kernel)(E)" + figures, txt)
    assert len(select) == 1
    for r, b, vgprs, scratch, occ, spill in found + select:
        assert int(scratch) == 0 and int(spill) == 0 and int(occ) >= 2 and int(vgprs) <= 256, (r, b, vgprs, scratch, occ, spill)
