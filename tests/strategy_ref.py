"""Plain numpy reference of the seven rule entry points of csrc/strategy.hip, written from the comment block of include/pq_hip.h
("The remaining comparisons of the README's fourteen `Strategy` generators") and NOT from the kernels:

  gate_signals         mode 0 zones: buy &= a < k0, sell &= a > k1; 1 strength: both &= a > k0; 2: buy &= a > c;
                       3: buy &= a[i] > a[i-1]; 4: buy &= (a - c) > |c| * k0.  A non-zero input signal counts as set, outputs are 0 / 1.
  zscore               z = (price - mid) / (upper - mid), NULL where upper is
  scale_band           lo = base * f_lo, hi = base * f_hi, NULL where base is
  volume_surge_signals surge = volume > multiplier * avg_volume; buy = surge on an up close, sell = surge on a down close
  gap_signals          buy = open[i] > high[i-1] * f_up, sell = open[i] < low[i-1] * f_dn
  pattern_any_signals  buy = any column == +100, sell = any column == -100
  ma_stack_signals     buy = first bar where mas[0] > mas[1] > ... holds, sell = first bar of the reverse order

Layout.  Every column is an array of any shape; the series are the rows of its last axis ([N, T]: N series of T rows), or, with
`ranges` = a list of (lo, hi) pairs, the rows [lo, hi) of the FLATTENED column (a ragged batch of long columns, or a pitched batch
whose padding is simply not in any range).  Row 0 of a series has no predecessor: a rule that looks one row back is false there.
Rows that belong to no range are 0 in the signal outputs and +0.0 in the f64 outputs.

NULL is the NaN bit pattern 0x7FF80000504E554C; in a comparison it is a NaN and compares false.  Every f64 output is a chain of
single IEEE operations, so float64 numpy is exact: the only freedom is the sign / payload of a NaN that an operation produces or
forwards (same_f64 below).
"""
import numpy as np

NULL_BITS = np.uint64(0x7FF80000504E554C)
NULL = np.array([NULL_BITS], dtype=np.uint64).view(np.float64)[0]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def isnull(x):
    return bits(x) == NULL_BITS


def _layout(x, ranges):
    """-> (first, live): boolean arrays of x's shape; first marks row 0 of every series, live the rows that belong to a series."""
    x = np.asarray(x)
    first, live = np.zeros(x.size, dtype=bool), np.zeros(x.size, dtype=bool)
    if ranges is None:
        T = x.shape[-1] if x.ndim else 1
        if T > 0:
            first[::T] = True
        live[:] = True
    else:
        for lo, hi in ranges:
            if hi > lo:
                first[lo] = True
                live[lo:hi] = True
    return first.reshape(x.shape), live.reshape(x.shape)


def _prev(x):
    """x[i - 1] over the flattened column; the value at the first row of a series is never used (masked by `first`)."""
    x = np.asarray(x)
    return np.roll(x.reshape(-1), 1).reshape(x.shape)


def _u8(m, live):
    return (m & live).astype(np.uint8)


def gate_signals(a, c, mode, k0, k1, buy_in, sell_in, ranges=None):
    a = np.asarray(a, dtype=np.float64)
    first, live = _layout(a, ranges)
    b, s = np.asarray(buy_in) != 0, np.asarray(sell_in) != 0
    if mode in (2, 4) and c is None:
        raise ValueError("this mode compares with a second column")
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 0:
            b, s = b & (a < k0), s & (a > k1)
        elif mode == 1:
            g = a > k0
            b, s = b & g, s & g
        elif mode == 2:
            b = b & (a > np.asarray(c, dtype=np.float64))
        elif mode == 3:
            b = b & ~first & (a > _prev(a))
        elif mode == 4:
            c = np.asarray(c, dtype=np.float64)
            b = b & ((a - c) > np.abs(c) * k0)
        else:
            raise ValueError("mode must be 0 .. 4")
    return _u8(b, live), _u8(s, live)


def _f64_out(val, carrier, live):
    out = bits(np.where(live, val, 0.0)).copy()
    out[isnull(carrier) & live] = NULL_BITS       # the NULL is handed on bit for bit
    return out.view(np.float64)


def zscore(price, upper, mid, ranges=None):
    p, u, m = (np.asarray(x, dtype=np.float64) for x in (price, upper, mid))
    _, live = _layout(u, ranges)
    with np.errstate(all="ignore"):
        z = (p - m) / (u - m)
    return _f64_out(z, u, live)


def scale_band(base, f_lo, f_hi, ranges=None):
    b = np.asarray(base, dtype=np.float64)
    _, live = _layout(b, ranges)
    with np.errstate(all="ignore"):
        lo, hi = b * f_lo, b * f_hi
    return _f64_out(lo, b, live), _f64_out(hi, b, live)


def volume_surge_signals(volume, avg_volume, close, multiplier, ranges=None):
    v, sv, c = (np.asarray(x, dtype=np.float64) for x in (volume, avg_volume, close))
    first, live = _layout(v, ranges)
    with np.errstate(all="ignore"):
        surge = v > multiplier * sv
        up, dn = ~first & (c > _prev(c)), ~first & (c < _prev(c))
    return _u8(surge & up, live), _u8(surge & dn, live)


def gap_signals(open_, high, low, f_up, f_dn, ranges=None):
    o, h, l = (np.asarray(x, dtype=np.float64) for x in (open_, high, low))
    first, live = _layout(o, ranges)
    with np.errstate(all="ignore"):
        buy = ~first & (o > _prev(h) * f_up)
        sell = ~first & (o < _prev(l) * f_dn)
    return _u8(buy, live), _u8(sell, live)


def pattern_any_signals(bullish, bearish, shape=None, ranges=None):
    """bullish / bearish: lists of int32 columns (possibly empty: then `shape` gives the shape of the outputs)."""
    cols = list(bullish) + list(bearish)
    shape = np.asarray(cols[0]).shape if cols else shape
    _, live = _layout(np.zeros(shape), ranges)
    buy, sell = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    for col in bullish:
        buy |= np.asarray(col) == 100
    for col in bearish:
        sell |= np.asarray(col) == -100
    return _u8(buy, live), _u8(sell, live)


def ma_stack_signals(mas, ranges=None):
    mas = [np.asarray(x, dtype=np.float64) for x in mas]
    if not 2 <= len(mas) <= 16:
        raise ValueError("2 .. 16 moving averages")
    first, live = _layout(mas[0], ranges)
    bull, bear = np.ones(mas[0].shape, dtype=bool), np.ones(mas[0].shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for x, y in zip(mas[:-1], mas[1:]):
            bull &= x > y
            bear &= x < y
    buy = ~first & bull & ~_prev(bull)
    sell = ~first & bear & ~_prev(bear)
    return _u8(buy, live), _u8(sell, live)


def same_f64(got, exp, carrier):
    """Element-wise: got equals exp bit for bit, or both are NaN on a row whose carrier (upper / base) is not NULL.  IEEE 754 leaves
    the sign and payload of a NaN that an operation produces (0 / 0, inf - inf, inf * 0) or forwards from one of two NaN operands to the
    implementation -- x86 produces the negative default NaN, the GPU the positive one -- so such rows are asserted to be NaN on both
    sides and nothing more; a NULL carrier must come out as NULL_BITS exactly (the first alternative)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return (bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp) & ~isnull(carrier))


# ---- case generator shared by the CPU and the GPU tests ----------------------------------------------------------------------------
# A case is dict(rule, cols={name: flat column}, params={...}); a layout is dict(n, len, stride, offsets, size): `size` elements are
# allocated per column (the batch plus a guard tail), ranges_of(layout) are the rows that belong to a series.
RULES = ("gate0", "gate1", "gate2", "gate3", "gate4", "zscore", "scale_band", "volume_surge", "gap", "pattern_any", "ma_stack")
GUARD = 64                      # elements behind the last series that no call may touch
PAD_F64, PAD_U8, PAD_I32 = 1e300, 0xFF, -1   # what the padding of the INPUT columns holds (i32: 0xFF bytes)
PATTERN_VALUES = np.array([-200, -100, 0, 0, 0, 0, 0, 100, 200], dtype=np.int32)
NULL_I32 = np.int32(-2147483648)


def regular_layout(n, T, stride=None):
    stride = T if stride is None else stride
    return dict(n=n, len=T, stride=stride, offsets=None, size=n * stride + GUARD)


def ragged_layout(offsets):
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    return dict(n=len(lens), len=int(lens.max()) if len(lens) else 0, stride=int(offsets[-1]), offsets=offsets, size=int(offsets[-1]) + GUARD)


def ranges_of(lay):
    if lay["offsets"] is not None:
        return [(int(lo), int(hi)) for lo, hi in zip(lay["offsets"][:-1], lay["offsets"][1:])]
    return [(s * lay["stride"], s * lay["stride"] + lay["len"]) for s in range(lay["n"])]


def live_of(lay):
    live = np.zeros(lay["size"], dtype=bool)
    if lay["offsets"] is not None:
        live[: lay["stride"]] = True
    elif lay["len"] > 0:
        idx = np.arange(lay["n"] * lay["stride"])
        live[: len(idx)] = idx % lay["stride"] < lay["len"]
    return live


def random_layout(rng):
    n, T = int(rng.integers(1, 41)), int(rng.integers(1, 601))
    if rng.random() < 0.5:
        return regular_layout(n, T, T + int(rng.integers(0, 20)) * int(rng.integers(0, 2)))
    lens = rng.integers(0, T + 1, n)
    lens[int(rng.integers(0, n))] = T
    return ragged_layout(np.concatenate([[0], np.cumsum(lens)]))


def _q(rng, size, lo, hi, step=0.5, p_null=0.02, p_nan=0.02):
    """quantised values lo, lo + step, ... < hi (ties are frequent) with NULLs and plain NaNs"""
    x = rng.integers(0, int(round((hi - lo) / step)), size) * step + lo
    u = rng.random(size)
    x[u < p_null] = NULL
    x[(u >= p_null) & (u < p_null + p_nan)] = np.nan
    return x


def _sig(rng, size):
    return rng.choice(np.array([0, 0, 1, 1, 2, 255], dtype=np.uint8), size)


def gen_case(rule, rng, lay, n_cols=None, p_null=0.02, p_nan=0.02):
    size, kw = lay["size"], dict(p_null=p_null, p_nan=p_nan)
    cols, prm = {}, {}
    if rule.startswith("gate"):
        mode = int(rule[4])
        cols = dict(a=_q(rng, size, -3.0, 4.0, **kw), buy_in=_sig(rng, size), sell_in=_sig(rng, size))      # (a and c both negative: |c| matters)
        if mode in (2, 4) or rng.random() < 0.3:      # c is also passed (and ignored) in some calls of the other modes
            cols["c"] = _q(rng, size, -2.0, 3.0, **kw)
        prm = dict(mode=mode, k0=(1.5, 1.5, 0.0, 0.0, 0.25)[mode], k1=2.0)
    elif rule == "zscore":
        cols = dict(price=_q(rng, size, 0.0, 3.0, **kw), upper=_q(rng, size, 1.0, 4.0, **kw), mid=_q(rng, size, 0.0, 3.0, **kw))
    elif rule == "scale_band":
        cols = dict(base=_q(rng, size, -2.0, 6.0, **kw))
        prm = dict(f_lo=0.97, f_hi=1.03)
    elif rule == "volume_surge":
        cols = dict(volume=_q(rng, size, 0.0, 8.0, 1.0, **kw), avg_volume=_q(rng, size, 0.0, 4.0, 1.0, **kw), close=_q(rng, size, 0.0, 3.0, 1.0, **kw))
        prm = dict(multiplier=1.5)
    elif rule == "gap":
        cols = dict(open=_q(rng, size, 0.0, 5.0, **kw), high=_q(rng, size, 0.0, 5.0, **kw), low=_q(rng, size, 0.0, 5.0, **kw))
        prm = dict(f_up=float(rng.choice([1.0, 1.25])), f_dn=float(rng.choice([1.0, 0.75])))
    elif rule == "pattern_any":
        nb, ns = n_cols if n_cols is not None else (int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        for k in range(nb):
            cols[f"bull{k}"] = rng.choice(PATTERN_VALUES, size)
        for k in range(ns):
            cols[f"bear{k}"] = rng.choice(PATTERN_VALUES, size)
        for c in cols.values():
            c[rng.random(size) < p_null] = NULL_I32
        prm = dict(nb=nb, ns=ns)
    elif rule == "ma_stack":
        n = n_cols if n_cols is not None else int(rng.integers(2, 6))
        trend = rng.integers(-1, 2, size).astype(np.float64)        # the order of the stack on this row: rising, flat or falling in k
        for k in range(n):
            x = k * trend + (rng.random(size) < 0.05) * 1.0         # a jitter that breaks the order now and then
            u = rng.random(size)
            x[u < p_null / n] = NULL
            x[(u >= p_null / n) & (u < (p_null + p_nan) / n)] = np.nan
            cols[f"ma{k}"] = x
        prm = dict(n=n)
    else:
        raise KeyError(rule)
    pad = ~live_of(lay)
    for c in cols.values():
        c[pad] = PAD_F64 if c.dtype == np.float64 else PAD_U8 if c.dtype == np.uint8 else PAD_I32
    return dict(rule=rule, cols=cols, params=prm)


def ref_case(case, ranges, shape=None):
    """the reference outputs of a case: (buy, sell), (z,) or (lo, hi)"""
    r, c, p = case["rule"], case["cols"], case["params"]
    if r.startswith("gate"):
        return gate_signals(c["a"], c.get("c"), p["mode"], p["k0"], p["k1"], c["buy_in"], c["sell_in"], ranges)
    if r == "zscore":
        return (zscore(c["price"], c["upper"], c["mid"], ranges),)
    if r == "scale_band":
        return scale_band(c["base"], p["f_lo"], p["f_hi"], ranges)
    if r == "volume_surge":
        return volume_surge_signals(c["volume"], c["avg_volume"], c["close"], p["multiplier"], ranges)
    if r == "gap":
        return gap_signals(c["open"], c["high"], c["low"], p["f_up"], p["f_dn"], ranges)
    if r == "pattern_any":
        return pattern_any_signals([c[f"bull{k}"] for k in range(p["nb"])], [c[f"bear{k}"] for k in range(p["ns"])], shape, ranges)
    if r == "ma_stack":
        return ma_stack_signals([c[f"ma{k}"] for k in range(p["n"])], ranges)
    raise KeyError(r)


def carrier_of(case):
    """the column whose NULLs an f64 output hands on (None for the signal rules)"""
    return {"zscore": case["cols"].get("upper"), "scale_band": case["cols"].get("base")}.get(case["rule"])


RANDOM_SEED, RANDOM_CASES = 0x5EED0051, 150


def random_cases():
    """the cases of the randomised GPU test, in order: (case, layout)"""
    rng = np.random.default_rng(RANDOM_SEED)
    for i in range(RANDOM_CASES):
        lay = random_layout(rng)
        yield gen_case(RULES[int(rng.integers(0, len(RULES)))] if i >= len(RULES) else RULES[i], rng, lay), lay


def firing(case, outs):
    """what a case contributes to the firing count of its rule: set buys and sells, or finite non-zero and NULL f64 outputs"""
    if carrier_of(case) is None:
        return np.array([int(outs[0].sum()), int(outs[1].sum())])
    return np.array([int((np.isfinite(outs[0]) & (outs[0] != 0)).sum()), int(isnull(outs[0]).sum())])
