"""What the parity modules share: the comparison of one output column with the oracle's (bit for bit, or tests/tolerance.py's rule for the
outputs that pass through a device transcendental), the "short" parameter table and the data builders.

Parameter sets of a function: {} are the Python-wrapper defaults (oracle.SPEC / EXTRA); SHORT[name] makes every period-like parameter
small (2 .. 7), so that nearly every row of a short series is live and the walks run their steady state, not their warm-up -- and gives
MAMA and SAR the limits with which they really adapt / reverse (the wrapper defaults of both are 0.0: degenerate walks).  Modes that are
no periods keep their defaults: `returns` stays at method 0 -- its log form (method 1) passes through the device's log, which differs
from libm's in the last bits of about 1 % of the values and is in no tolerance table, so it cannot be held bit for bit."""
import numpy as np

from tolerance import RTOL, SCALE_OF  # which transcendental outputs are judged against a natural scale, and why

NULL_BITS = 0x7FF80000504E554C
NULLB = np.uint64(NULL_BITS)
TRANSCENDENTAL = {"ht_dcperiod", "ht_dcphase", "ht_phasor", "ht_sine", "mama"}   # functions whose outputs tests/tolerance.py judges


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same(name, got, exp, exact=True, price=None):
    got = np.asarray(got)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, got.shape, exp.shape, got.dtype, exp.dtype)
    if exp.dtype != np.float64:
        assert (got == exp).all(), f"{name}: {np.sum(got != exp)} int mismatches"
        return
    NULLB = np.uint64(0x7FF80000504E554C)
    gn, en = bits(got) == NULLB, bits(exp) == NULLB
    assert (gn == en).all(), f"{name}: null masks differ at {np.argwhere(gn != en)[:5].tolist()}"
    if exact:
        bad = (bits(got) != bits(exp)) & ~(np.isnan(got) & np.isnan(exp))
        assert not bad.any(), (f"{name}: {bad.sum()} of {bad.size} not bit-exact; first at {np.argwhere(bad)[:3].tolist()} "
                               f"got {got[bad][:3]} exp {exp[bad][:3]}")
    else:
        key = name.split("{")[0]
        scale = SCALE_OF.get(key, 0.0)
        if isinstance(scale, str):
            assert price is not None, f"{name}: judged against the price level, which the caller must pass"
            scale = np.abs(price)
        ok = ~en
        g, e = got[ok], exp[ok]
        sc = np.broadcast_to(scale, exp.shape)[ok]
        both_nan = np.isnan(g) & np.isnan(e)
        with np.errstate(invalid="ignore"):
            err = np.abs(g - e) / np.maximum(np.maximum(np.abs(e), sc), 1e-300)
        err[both_nan | (g == e)] = 0        # (equal infinities: inf - inf is NaN)
        assert (err <= RTOL).all(), f"{name}: max error {np.nanmax(err):.3e} (relative to max(|expected|, scale))"


def same_bits(a, b):
    """elementwise: the two arrays hold the same bit patterns (so a NULL equals only a NULL), or both hold a NaN that is not a NULL"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float64:
        return a == b
    ab, bb = bits(a), bits(b)
    return (ab == bb) | (np.isnan(a) & np.isnan(b) & (ab != NULLB) & (bb != NULLB))


SHORT = {
    "bbands": dict(timeperiod=5, nbdevup=2.0, nbdevdn=1.5), "dema": dict(timeperiod=4), "ema": dict(timeperiod=3), "kama": dict(timeperiod=5),
    "ma": dict(timeperiod=5, matype=1), "mama": dict(fastlimit=0.5, slowlimit=0.05), "mavp": dict(minperiod=2, maxperiod=7, matype=0),
    "midpoint": dict(timeperiod=3), "midprice": dict(timeperiod=4), "sar": dict(acceleration=0.02, maximum=0.2),
    "sarext": dict(startvalue=0.0, offsetonreverse=0.01, accelerationinitlong=0.02, accelerationlong=0.02, accelerationmaxlong=0.2,
                   accelerationinitshort=0.03, accelerationshort=0.03, accelerationmaxshort=0.3),
    "sma": dict(timeperiod=4), "t3": dict(timeperiod=3, vfactor=0.7), "tema": dict(timeperiod=3), "trima": dict(timeperiod=5),
    "wma": dict(timeperiod=4), "adx": dict(timeperiod=3), "adxr": dict(timeperiod=3), "apo": dict(fastperiod=2, slowperiod=5, matype=0),
    "aroon": dict(timeperiod=4), "aroonosc": dict(timeperiod=5), "cci": dict(timeperiod=5), "cmo": dict(timeperiod=4), "dx": dict(timeperiod=3),
    "macd": dict(fastperiod=3, slowperiod=7, signalperiod=4),
    "macdext": dict(fastperiod=4, fastmatype=1, slowperiod=7, slowmatype=0, signalperiod=3, signalmatype=0),
    "macdfix": dict(signalperiod=3), "mfi": dict(timeperiod=4), "minus_di": dict(timeperiod=3), "minus_dm": dict(timeperiod=4),
    "mom": dict(timeperiod=2), "plus_di": dict(timeperiod=4), "plus_dm": dict(timeperiod=3), "ppo": dict(fastperiod=3, slowperiod=6, matype=1),
    "roc": dict(timeperiod=2), "rocp": dict(timeperiod=3), "rocr": dict(timeperiod=4), "rocr100": dict(timeperiod=5), "rsi": dict(timeperiod=3),
    "stoch": dict(fastk_period=4, slowk_period=3, slowk_matype=1, slowd_period=2, slowd_matype=0),
    "stochf": dict(fastk_period=4, fastd_period=3, fastd_matype=1), "stochrsi": dict(timeperiod=5, fastk_period=4, fastd_period=3, fastd_matype=0),
    "trix": dict(timeperiod=3), "ultosc": dict(timeperiod1=2, timeperiod2=3, timeperiod3=5), "willr": dict(timeperiod=4),
    "atr": dict(timeperiod=3), "natr": dict(timeperiod=4), "adosc": dict(fastperiod=2, slowperiod=5),
    "returns": dict(period=2), "rolling_max": dict(window=3), "rolling_min": dict(window=5),
}


def param_sets(oracle, name):
    """[(tag, parameters)] of function `name`: the defaults, and the short set where the function has parameters at all"""
    spec = oracle.SPEC[name] if name in oracle.SPEC else oracle.EXTRA[name]
    assert bool(spec[1]) == (name in SHORT), f"{name}: SHORT must hold exactly the functions that take parameters"
    return [("defaults", {})] + ([("short", SHORT[name])] if name in SHORT else [])


def with_aliases(d, seed=7):
    """adds the two input columns that are no OHLCV column: `real` (the close) and MAVP's `periods` (integers 0 .. 39 as f64)"""
    d = dict(d)
    d["real"] = d["close"]
    d["periods"] = np.random.default_rng(seed).integers(0, 40, size=d["close"].shape).astype(np.float64)
    return d


def clean_data(oracle, seed, n, T, mode=0):
    """the oracle's seeded OHLCV generator (mode 1: candles built so that the recognisers fire) plus `real` and `periods`"""
    return with_aliases(oracle.gen_ohlcv(seed, n, T, mode))


def dirty_data(oracle, clean, seed=11):
    """a copy of `clean` with 2 % NULLs at random, a NULL prefix of 3 rows on every series but number 5 (which stays clean), a series
    (number 4, where there is one) that goes fully NULL from a third of its length on, one NaN that is no NULL, one +inf and one -inf"""
    n, T = clean["close"].shape
    mask = np.random.default_rng(seed).random((n, T)) < 0.02
    mask[:, :3] = True
    if n > 5:
        mask[5] = False
    if n > 4:
        mask[4, T // 3:] = True
    out = {}
    for k, v in clean.items():
        a = v.copy()
        a[mask] = oracle.NULL
        if T > 40:
            a[0, 40] = np.nan
            a[1 % n, T // 2] = np.inf
            a[2 % n, T // 2 + 3] = -np.inf
        out[k] = a
    return out
