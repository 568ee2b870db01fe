"""-m gpu: the expression plugin (csrc/plugin.hip) and the per-context state of the library under CONCURRENT callers.

Polars calls the plugin from its rayon workers: the sixty expressions of one `with_columns` arrive at the same time, from different
host threads, with the same `close` buffer and the same key column.  Three parts of the plugin are shared between those threads -- the
input-column cache (one mutex, `in_use` counts, LRU eviction, publication after the creator's sync), the host-block pool (blocks are
released by whichever thread drops the result) and the `thread_local` context -- and every other test drives them from one thread.
Here pyarrow plays Polars as in test_polars_plugin.py; `ctypes.CDLL` drops the GIL for the call, so the calls really overlap.

Rules of every test in this file: workers are daemon threads that start together behind a barrier (at most 16, at most 4 where a column
is 8 MB or more: such a call starts up to 16 hashing and 8 scanning helper threads of its own), catch everything into a dict and abort
the barrier; the main thread joins each with a 120 s hang guard (two orders of magnitude above the work) and ends the whole pytest run
if one is still alive, so that nothing else touches the GPU behind a stuck call.  The expected value of a concurrent call is the SAME
call made alone on the main thread before the workers start -- compared bit for bit on values, validity, type and length -- and that
serial result is checked once against the oracle by the rule test_polars_plugin.py uses for the function (bitwise; ht_dcphase at
rtol = atol = 1e-12).  Environment variables are set before the workers start and restored afterwards (getenv runs inside every
call).  Every plugin test begins with pq_plugin_cache_clear() and ends with a clear after which the counters must read (0, 0, 0, 0): an
entry that survives a clear is an `in_use` count that never came back to zero."""
import contextlib
import ctypes as C
import os
import queue
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

from plugin_ffi import STRUCT_FUNCS, SeriesExport, _export, _lib, _plugin_call, _same_array  # noqa: E402

HANG_GUARD_S = 120
OHLC = ("open", "high", "low", "close")
INT32_NULL = np.int32(-2147483648)


# ---- the harness -------------------------------------------------------------------------------------------------------------------

def run_threads(jobs):
    """jobs: callables without arguments, one per worker.  All start together; the first real exception of a worker is raised here."""
    assert 1 <= len(jobs) <= 16
    barrier, errs = threading.Barrier(len(jobs)), {}

    def wrap(i, job):
        try:
            barrier.wait()
            job()
        except BaseException as e:  # noqa: BLE001
            errs[i] = e
            try:
                barrier.abort()
            except Exception:  # noqa: BLE001
                pass

    ths = [threading.Thread(target=wrap, args=(i, j), daemon=True) for i, j in enumerate(jobs)]
    for t in ths:
        t.start()
    for i, t in enumerate(ths):
        t.join(timeout=HANG_GUARD_S)
        if t.is_alive():
            pytest.exit(f"worker {i} of {len(ths)} is still running after {HANG_GUARD_S} s: a call hangs; nothing else may touch the GPU in this run",
                        returncode=3)
    real = {i: e for i, e in errs.items() if not isinstance(e, threading.BrokenBarrierError)} or errs
    for i in sorted(real):
        raise AssertionError(f"worker {i}: {type(real[i]).__name__}: {real[i]}") from real[i]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib()
    lib.pq_plugin_cache_stats.argtypes = [C.POINTER(C.c_int64)] * 4
    lib.pq_plugin_cache_stats.restype = None
    lib.pq_plugin_cache_clear.restype = None
    return lib


def stats(L):
    v = [C.c_int64() for _ in range(4)]
    L.pq_plugin_cache_stats(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)     # hits, misses, bytes, entries


@pytest.fixture
def cache(L):
    """every plugin test begins with an empty cache and must leave one that a clear empties completely"""
    L.pq_plugin_cache_clear()
    assert stats(L) == (0, 0, 0, 0)
    yield
    L.pq_plugin_cache_clear()
    assert stats(L) == (0, 0, 0, 0), "an entry survived pq_plugin_cache_clear(): its in_use count never returned to zero"


def zero_copy(buf):
    """a one-chunk Float64 array over the numpy buffer itself (the address the cache keys on)"""
    arr = pa.Array.from_buffers(pa.float64(), len(buf), [None, pa.py_buffer(buf)])
    assert arr.buffers()[1].address == buf.ctypes.data
    return arr


def same_result(a, b):
    """_same_array, field by field for a Struct"""
    assert a.type == b.type and len(a) == len(b)
    if pa.types.is_struct(a.type):
        for k in range(a.type.num_fields):
            _same_array(a.field(k), b.field(k))
    else:
        _same_array(a, b)


def oracle_check(oracle, name, got, cols, params):
    """the serial plugin result against the oracle, by the rule test_polars_plugin.py uses for `name`.  cols: the host columns in the
    reference's order, [n] or (a balanced `_over` call) [groups, rows]"""
    if name.startswith("cdl"):
        exp = oracle.pattern(name, *cols).reshape(-1)
        assert got.type == pa.int32() and got.null_count == 0 and len(got) == len(exp) and (got.to_numpy() == exp).all(), name
        return
    exp = oracle.call(name, *cols, **params)
    if name in STRUCT_FUNCS:
        fields = STRUCT_FUNCS[name][3]
        assert pa.types.is_struct(got.type) and [got.type.field(i).name for i in range(got.type.num_fields)] == fields
        pairs = [(got.field(i), e) for i, e in enumerate(exp)]
    else:
        pairs = [(got, exp[0])]
    for g, e in pairs:
        e = np.asarray(e).reshape(-1)
        assert len(g) == len(e), name
        if e.dtype == np.int32:
            en = e == INT32_NULL
            assert g.type == pa.int32() and (np.asarray(g.is_null()) == en).all(), name
            assert (g.to_numpy(zero_copy_only=False)[~en].astype(np.int32) == e[~en]).all(), name
            continue
        en = e.view(np.uint64) == np.uint64(oracle.NULL_BITS)
        assert g.type == pa.float64() and (np.asarray(g.is_null()) == en).all(), name
        gv = g.to_numpy(zero_copy_only=False)[~en]
        if name in ("ht_dcperiod", "ht_dcphase"):           # transcendental class
            np.testing.assert_allclose(gv, e[~en], rtol=1e-12, atol=1e-12)
        else:
            assert (gv.view(np.uint64) == e[~en].view(np.uint64)).all(), name


def ema_call(L, arr, period):
    return _plugin_call(L, "ema", [([arr], "close")], kwargs={"timeperiod": period})


# ---- 1. sixty expressions on one column ------------------------------------------------------------------------------------------------

# (function, input columns, parameters): one input / three / four / several parameters / Struct / Int32 / the transcendental class
SIXTEEN = [("ema", ("close",), {"timeperiod": 20}), ("sma", ("close",), {"timeperiod": 10}), ("rsi", ("close",), {"timeperiod": 14}),
           ("trix", ("close",), {"timeperiod": 9}), ("atr", ("high", "low", "close"), {"timeperiod": 14}),
           ("willr", ("high", "low", "close"), {"timeperiod": 9}), ("mfi", ("high", "low", "close", "volume"), {"timeperiod": 10}),
           ("ad", ("high", "low", "close", "volume"), {}), ("ultosc", ("high", "low", "close"), {"timeperiod1": 5, "timeperiod2": 9, "timeperiod3": 20}),
           ("apo", ("close",), {"fastperiod": 5, "slowperiod": 13, "matype": 1}), ("macd", ("close",), {"fastperiod": 5, "slowperiod": 13, "signalperiod": 4}),
           ("bbands", ("close",), {"timeperiod": 10, "nbdevup": 1.5, "nbdevdn": 2.5}), ("aroon", ("high", "low"), {"timeperiod": 9}),
           ("ht_trendmode", ("close",), {}), ("cdlengulfing", OHLC, {}), ("ht_dcphase", ("close",), {})]


def test_sixty_expressions_on_one_column(L, oracle, cache):
    """16 threads x 6 calls from a fixed per-thread list over sixteen functions (every result shape) on ONE shared open / high / low /
    close / volume set.  Warm: every column has been used once, so the concurrent calls add exactly one hit per (call, input column)
    and nothing else.  Cold: 16 first callers of `close` at once.  The cache has no in-flight entry, so each thread that misses
    uploads and publishes its own copy: 1 <= entries <= misses, every copy counted in bytes, every result right.  (The observed number
    of cold misses is printed and recorded in EXPERIMENTS.md; it is an observation, not an assertion.)"""
    n = 40_000
    d = oracle.gen_ohlcv(0x5EED0E01, 1, n, 1)             # (the pattern-rich variant: cdlengulfing fires)
    host = {k: np.ascontiguousarray(v[0]) for k, v in d.items()}
    arrs = {k: zero_copy(v) for k, v in host.items()}

    def call(spec):
        name, cols, prm = spec
        return _plugin_call(L, name, [([arrs[c]], c) for c in cols], kwargs=prm or None)

    expected = []
    for spec in SIXTEEN:
        r = call(spec)
        oracle_check(oracle, spec[0], r, [host[c] for c in spec[1]], spec[2])
        expected.append(r)
    assert (expected[14].to_numpy() != 0).any()
    warm = stats(L)
    assert warm[1:] == (5, 5 * n * 8, 5), warm            # five columns, each uploaded once
    plan = [[(t + 3 * j) % 16 for j in range(6)] for t in range(16)]
    assert {k for p in plan for k in p} == set(range(16))
    pairs = sum(len(SIXTEEN[k][1]) for p in plan for k in p)

    def worker(t):
        def job():
            for k in plan[t]:
                same_result(call(SIXTEEN[k]), expected[k])
        return job

    run_threads([worker(t) for t in range(16)])
    after = stats(L)
    assert after[0] == warm[0] + pairs and after[1:] == warm[1:], (warm, after, pairs)

    # cold: 16 first callers of one column.  The serial expectations come from the same content at ANOTHER address and before the
    # clear, so that the column the threads call on has never been seen by the cache
    periods = list(range(5, 21))
    cold_expected = []
    for p in periods:
        r = ema_call(L, arrs["close"], p)
        oracle_check(oracle, "ema", r, [host["close"]], {"timeperiod": p})
        cold_expected.append(r)
    L.pq_plugin_cache_clear()
    assert stats(L) == (0, 0, 0, 0)
    fresh = host["close"].copy()
    arr = zero_copy(fresh)
    got = {}

    def cold(t):
        def job():
            got[t] = ema_call(L, arr, periods[t])
        return job

    run_threads([cold(t) for t in range(16)])
    h, m, by, ent = stats(L)
    print(f"\n[concurrency] cold start, 16 first callers of one column: {m} misses, {h} hits, {ent} entries")
    assert h + m == 16 and 1 <= ent <= m and by == ent * n * 8, (h, m, by, ent)
    for t in range(16):
        _same_array(got[t], cold_expected[t])


# ---- 2. eviction while other threads hold hits ---------------------------------------------------------------------------------------------

def test_eviction_while_other_threads_hold_hits(L, oracle, cache):
    """PQ_PLUGIN_CACHE_MB=1 and columns of 320 000 B: three fit.  8 threads cycle through four private columns each (32 columns compete
    for three places: every publication evicts) interleaved with calls on one shared column.  An eviction that freed a column another
    thread's kernel still reads would show as a wrong result; afterwards nobody holds an entry, so one more publication must bring the
    cache back under its limit."""
    n, T, K, ROUNDS = 40_000, 8, 4, 6
    rows = oracle.gen_ohlcv(0x5EED0E02, T * K + 2, n, 0)["close"]
    bufs = [np.ascontiguousarray(rows[i]) for i in range(T * K + 2)]
    arrs = [zero_copy(b) for b in bufs]
    shared, extra = T * K, T * K + 1
    period = [5 + i % 23 for i in range(T * K + 2)]
    with env(PQ_PLUGIN_CACHE_MB="1"):
        expected = []
        for i in range(T * K + 1):
            r = ema_call(L, arrs[i], period[i])
            oracle_check(oracle, "ema", r, [bufs[i]], {"timeperiod": period[i]})
            expected.append(r)

        def worker(t):
            def job():
                for _ in range(ROUNDS):
                    for k in range(K):
                        i = t * K + k
                        _same_array(ema_call(L, arrs[i], period[i]), expected[i])
                        _same_array(ema_call(L, arrs[shared], period[shared]), expected[shared])
            return job

        run_threads([worker(t) for t in range(T)])
        h, m, by, ent = stats(L)
        assert h + m == (T * K + 1) + T * ROUNDS * K * 2, (h, m)
        r = ema_call(L, arrs[extra], period[extra])       # a fresh column: its publication evicts down to the limit
        oracle_check(oracle, "ema", r, [bufs[extra]], {"timeperiod": period[extra]})
        h, m, by, ent = stats(L)
        assert by <= 1 << 20 and by == ent * n * 8 and ent >= 1, (by, ent)


# ---- 3. one address, changing content, beside readers of a stable column ---------------------------------------------------------------------

def test_changing_content_at_one_address_beside_readers(L, oracle, cache):
    """4 threads own one numpy buffer each, exported zero-copy: change one element in the middle, call, eight times (the hash of the
    whole buffer must make each a miss with the new content); 4 further threads hit a shared column that never changes.  A thread writes
    only its own buffer, so the test itself has no race."""
    n, STEPS = 40_000, 8
    rows = oracle.gen_ohlcv(0x5EED0E03, 5, n, 0)["close"]
    own = [np.ascontiguousarray(rows[i]) for i in range(4)]
    first = [b.copy() for b in own]
    own_arr = [zero_copy(b) for b in own]
    stable = np.ascontiguousarray(rows[4])
    stable_arr = zero_copy(stable)

    def change(buf, t, i):
        k = n // 2 + 17 + t
        buf[k] = first[t][k] * (1.25 + 0.5 * i)

    calls = 0
    expected = [[] for _ in range(4)]
    for t in range(4):                       # the thread's own sequence of contents beforehand -- from ANOTHER buffer, so that under the
        scratch = first[t].copy()            # thread's own address every content is new to the cache: a miss and a publication each
        scratch_arr = zero_copy(scratch)
        for i in range(STEPS):
            change(scratch, t, i)
            r = ema_call(L, scratch_arr, 12 + t)
            oracle_check(oracle, "ema", r, [scratch.copy()], {"timeperiod": 12 + t})
            expected[t].append(r)
            calls += 1
    for t in range(4):
        for i in range(1, STEPS):
            assert not expected[t][i].equals(expected[t][i - 1])        # (the change is visible in the result)
    stable_exp = [ema_call(L, stable_arr, 5 + i) for i in range(STEPS)]
    calls += STEPS
    oracle_check(oracle, "ema", stable_exp[0], [stable], {"timeperiod": 5})

    def mutator(t):
        def job():
            for i in range(STEPS):
                change(own[t], t, i)
                _same_array(ema_call(L, own_arr[t], 12 + t), expected[t][i])
        return job

    def reader(t):
        def job():
            for i in range(STEPS):
                _same_array(ema_call(L, stable_arr, 5 + (i + t) % STEPS), stable_exp[(i + t) % STEPS])
        return job

    before = stats(L)
    run_threads([mutator(t) for t in range(4)] + [reader(t) for t in range(4)])
    calls += 8 * STEPS
    h, m, by, ent = stats(L)
    assert h + m == calls and by == ent * n * 8, (h, m, by, ent, calls)
    # the readers' column was cached before they started and is never evicted at the default limit: they only hit; every content of a
    # mutator's buffer is new under its address: another hash, a miss
    assert (h - before[0], m - before[1]) == (4 * STEPS, 4 * STEPS), (before, (h, m))


# ---- 4. results that cross threads; the host pool ------------------------------------------------------------------------------------------------

def value_addresses(r):
    """the addresses of the values buffers of a result (three for a Struct), as plain integers: no reference to the result is kept"""
    kids = r.flatten() if pa.types.is_struct(r.type) else [r]
    return [k.buffers()[1].address for k in kids]


def value_bits(r):
    kids = r.flatten() if pa.types.is_struct(r.type) else [r]
    return [np.array(k.to_numpy(zero_copy_only=False)).view(np.uint64 if k.type == pa.float64() else np.uint32).copy() for k in kids]


@pytest.mark.parametrize("pool", ["default", "0"])
def test_results_cross_threads_host_pool(L, oracle, cache, pool):
    """n = 300 000 (2.4 MB result blocks: pooled).  4 producers make five results each (ema, macd: three blocks, cdlengulfing: an Int32
    block) and queue them; 4 consumers compare a result bit for bit with its expectation and only THEN drop it -- the block is released
    on another thread than the one that made it.  The serial results stay alive on the main thread throughout: two of them are compared
    with a snapshot of their bits at the end, and no values buffer of a new result may have the address of one that is still alive.
    pool = "0": the same with PQ_PLUGIN_HOSTPOOL_MB=0."""
    n = 300_000
    d = oracle.gen_ohlcv(0x5EED0E04, 1, n, 1)
    host = {k: np.ascontiguousarray(d[k][0]) for k in OHLC}
    arrs = {k: zero_copy(v) for k, v in host.items()}
    specs = {}
    for p in range(4):
        specs[p] = [("ema", ("close",), {"timeperiod": 9 + p}), ("macd", ("close",), {"fastperiod": 12, "slowperiod": 26, "signalperiod": 9}),
                    ("cdlengulfing", OHLC, {}), ("ema", ("close",), {"timeperiod": 21 + p}),
                    ("macd", ("close",), {"fastperiod": 5, "slowperiod": 13, "signalperiod": 4})]

    def call(spec):
        name, cols, prm = spec
        return _plugin_call(L, name, [([arrs[c]], c) for c in cols], kwargs=prm or None)

    def key(spec):
        return (spec[0], tuple(sorted(spec[2].items())))

    with env(PQ_PLUGIN_HOSTPOOL_MB=None if pool == "default" else "0"):
        lock, alive = threading.Lock(), set()

        def register(r):
            ad = value_addresses(r)
            with lock:
                assert len(set(ad)) == len(ad) and not (alive & set(ad)), "a values buffer was handed out while its previous owner is alive"
                alive.update(ad)
            return ad

        expected = {}
        for p in range(4):
            for spec in specs[p]:
                if key(spec) not in expected:
                    r = call(spec)
                    oracle_check(oracle, spec[0], r, [host[c] for c in spec[1]], spec[2])
                    register(r)
                    expected[key(spec)] = r
        assert len(expected) == 11
        early = [expected[key(specs[0][0])], expected[key(specs[0][1])]]
        snapshot = [value_bits(r) for r in early]
        q = queue.Queue()

        def producer(p):
            def job():
                try:
                    for spec in specs[p]:
                        r = call(spec)
                        q.put((key(spec), register(r), r))
                        del r
                finally:
                    q.put(None)              # one end mark per producer = one per consumer
            return job

        def consumer():
            while True:
                item = q.get()
                if item is None:
                    return
                k, ad, r = item
                del item
                same_result(r, expected[k])
                with lock:
                    alive.difference_update(ad)          # (before the drop: afterwards the block may be handed out again)
                del r

        run_threads([producer(p) for p in range(4)] + [consumer] * 4)
        assert q.empty()
        for r, snap in zip(early, snapshot):
            for now, was in zip(value_bits(r), snap):
                assert (now == was).all(), "a result held by the main thread changed while other threads' results came and went"
        assert len(alive) == sum(len(value_addresses(r)) for r in expected.values())
        del expected, early


# ---- 5. large _over calls: the helper-thread paths ----------------------------------------------------------------------------------------

def test_large_over_calls_helper_thread_paths(L, oracle, cache):
    """1 024 groups x 2 200 rows = 2 252 800 rows, 17.2 MB a column: above the 8 MB threshold of HashAhead and the chunked
    hash_buffer; above 2 x 2^20 rows, so plan_layout's in-place key scan and validity_from_host split over threads; 2 200 is no multiple
    of 16, so the panel is pitched to 2 208; 2 200 >= 1 024, so the wave-per-symbol forms run.  4 threads (columns of 8 MB and more)
    run ema_over / rsi_over / macd_over / cdlengulfing_over on the same columns and the same int64 key, three calls each.  Second round:
    a key whose group lengths alternate between 2 199 and 2 201 -- the ragged layout, d_off, no pitch."""
    G, glen = 1024, 2200
    n = G * glen
    d = oracle.gen_ohlcv(0x5EED0E05, G, glen, 1)
    panel = {k: d[k] for k in OHLC}                                        # [G, glen]
    host = {k: np.ascontiguousarray(panel[k]).reshape(-1) for k in OHLC}   # the long columns
    arrs = {k: zero_copy(v) for k, v in host.items()}
    key_even = np.repeat(np.arange(G, dtype=np.int64), glen)
    lens = np.where(np.arange(G) % 2 == 0, glen - 1, glen + 1).astype(np.int64)
    assert lens.sum() == n
    off = np.r_[0, np.cumsum(lens)]
    key_ragged = np.repeat(np.arange(G, dtype=np.int64), lens)
    keys = {"balanced": zero_copy_i64(key_even), "ragged": zero_copy_i64(key_ragged)}
    specs = [("ema", ("close",), {"timeperiod": 20}), ("rsi", ("close",), {"timeperiod": 14}),
             ("macd", ("close",), {"fastperiod": 12, "slowperiod": 26, "signalperiod": 9}), ("cdlengulfing", OHLC, {})]

    def call(spec, layout):
        name, cols, prm = spec
        return _plugin_call(L, name + "_over", [([arrs[c]], c) for c in cols] + [([keys[layout]], "symbol")], kwargs=prm or None)

    expected = {}
    for spec in specs:
        r = call(spec, "balanced")
        oracle_check(oracle, spec[0], r, [panel[c] for c in spec[1]], spec[2])        # one oracle call on the [1024, 2200] reshape
        expected[("balanced", spec[0])] = r
    for spec in specs:
        expected[("ragged", spec[0])] = call(spec, "ragged")
    r = expected[("ragged", "ema")]                                                   # the serial ema_over, group by group
    exp = np.concatenate([np.asarray(oracle.call("ema", host["close"][off[g]:off[g + 1]], timeperiod=20)[0]).reshape(-1) for g in range(G)])
    en = exp.view(np.uint64) == np.uint64(oracle.NULL_BITS)
    assert len(r) == n and (np.asarray(r.is_null()) == en).all()
    assert (r.to_numpy(zero_copy_only=False)[~en].view(np.uint64) == exp[~en].view(np.uint64)).all()
    warm = stats(L)
    assert warm[1] == 8 and warm[3] == 8 and warm[2] == 4 * (G * 2208 * 8) + 4 * (n * 8), warm   # four columns in two layouts
    pairs = 3 * sum(len(s[1]) for s in specs)
    for layout in ("balanced", "ragged"):
        def worker(spec, layout=layout):
            def job():
                for _ in range(3):
                    same_result(call(spec, layout), expected[(layout, spec[0])])
            return job

        before = stats(L)
        run_threads([worker(s) for s in specs])
        after = stats(L)
        assert after[0] == before[0] + pairs and after[1:] == before[1:], (layout, before, after)
    del expected


def zero_copy_i64(buf):
    arr = pa.Array.from_buffers(pa.int64(), len(buf), [None, pa.py_buffer(buf)])
    assert arr.buffers()[1].address == buf.ctypes.data
    return arr


# ---- 6. errors stay on their thread ------------------------------------------------------------------------------------------------------------

def test_errors_stay_on_their_thread(L, oracle, cache):
    """2 threads alternate refused calls (too few inputs; a null-bearing column into rsi; a string column; a key of the wrong length for
    ema_over -- argument refusals before any launch) with good ones, ten times; 6 others compute.  _polars_plugin_get_last_error_message()
    is b"" on the six after every call; on the two it carries the text of the refusal and is empty again after the next good call."""
    n = 40_000
    rows = oracle.gen_ohlcv(0x5EED0E06, 1, n, 0)["close"]
    x = np.ascontiguousarray(rows[0])
    arr = zero_copy(x)
    mask = np.zeros(n, bool); mask[[3, n // 2]] = True
    with_nulls = pa.array(x, mask=mask)
    strings = pa.array(["1", "2", "3"], type=pa.string())
    short_key = pa.array(np.zeros(n - 3, dtype=np.int64))
    refusals = [("ema_over", [([arr], "close")], b"too few"), ("rsi", [([with_nulls], "close")], b"nulls"),
                ("ema", [([strings], "strs")], b"not numeric"), ("ema_over", [([arr], "close"), ([short_key], "symbol")], b"key column")]
    msg = L._polars_plugin_get_last_error_message
    expected = [ema_call(L, arr, 5 + i) for i in range(10)]
    for i in (0, 9):
        oracle_check(oracle, "ema", expected[i], [x], {"timeperiod": 5 + i})

    def refused(name, series, text):
        ses, keep = [], []
        for chunks, nm in series:
            se, k = _export(chunks, nm)
            ses.append(se); keep.append(k)
        ins = (SeriesExport * len(ses))(*ses)
        ret = SeriesExport()
        getattr(L, "_polars_plugin_" + name)(ins, len(ses), None, 0, C.byref(ret), None)
        m = msg()
        assert not ret.release and text in m, (name, text, m)

    def faulty(t):
        def job():
            for i in range(10):
                refused(*refusals[(i + t) % 4])
                _same_array(ema_call(L, arr, 5 + i), expected[i])
                assert msg() == b"", msg()
        return job

    def good(t):
        def job():
            for i in range(10):
                _same_array(ema_call(L, arr, 5 + (i + t) % 10), expected[(i + t) % 10])
                assert msg() == b"", msg()
        return job

    run_threads([faulty(t) for t in range(2)] + [good(t) for t in range(6)])


# ---- 7. short-lived threads -----------------------------------------------------------------------------------------------------------------------

def test_short_lived_threads(L, oracle, cache):
    """Three successive waves of 8 FRESH threads, two calls each on a shared column: plugin_ctx() creates 24 contexts.  Results are right
    and every wave adds its 16 hits and nothing else.  Known leak, not fixed here: a per-thread plugin context (its 512-byte flag block,
    and whatever workspace its calls grew) is never destroyed when its thread ends -- DESIGN.md section 7, rank 4."""
    n = 40_000
    x = np.ascontiguousarray(oracle.gen_ohlcv(0x5EED0E07, 1, n, 0)["close"][0])
    arr = zero_copy(x)
    expected = [ema_call(L, arr, 7), _plugin_call(L, "rsi", [([arr], "close")], kwargs={"timeperiod": 14})]
    oracle_check(oracle, "ema", expected[0], [x], {"timeperiod": 7})
    oracle_check(oracle, "rsi", expected[1], [x], {"timeperiod": 14})
    assert stats(L) == (1, 1, n * 8, 1)

    def job():
        _same_array(ema_call(L, arr, 7), expected[0])
        _same_array(_plugin_call(L, "rsi", [([arr], "close")], kwargs={"timeperiod": 14}), expected[1])

    for wave in range(3):
        run_threads([job] * 8)
        assert stats(L) == (1 + 16 * (wave + 1), 1, n * 8, 1), (wave, stats(L))


# ---- 8. independent contexts, every kind of per-context state ------------------------------------------------------------------------------

def raw(t):
    """a device tensor -> its bytes on the host (synchronises the current stream)"""
    a = t.detach().cpu().contiguous().numpy()
    return a.dtype.str, a.shape, a.tobytes()


def _families(oracle):
    """name -> (shapes, make(shape) -> inputs on the device, run(inputs) -> list of device tensors, check(shape index, outputs) or None).
    Built and first run on the main thread; `run` reads api.ctx(), i.e. the context of the calling thread's current stream."""
    import sweep_rules_ref as S
    import polars_quant_amd as pq
    from polars_quant_amd import api
    from polars_quant_amd.suite import Suite
    from test_backtest_wave_gpu import check_summary, same_bits
    from test_factor_sorts_gpu import make as make_factor
    from test_gpu_parity import _pitched
    from test_linear_gpu import make as make_linear
    from test_suite_binding_gpu import TASKS, _subset_matches
    from test_wt_gpu import same as same_wt

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    fam = {}

    # (a) a wave-per-symbol indicator: the context's gate flags and its d_flag[24..27] counters
    def wt_make(shape):
        d = oracle.gen_ohlcv(0x5EED0E11, shape[0], shape[1], 0)
        return {"host": d["close"], "x": dev(d["close"])}

    def wt_check(k, inp, outs):
        (exp,) = oracle.call("tema", inp["host"], timeperiod=30)
        same_wt("tema", outs[0].cpu().numpy(), exp)
    fam["wave indicator"] = ([(130, 1100), (520, 1100)], wt_make, lambda inp: list(api.call("tema", inp["x"], timeperiod=30)), wt_check)

    # (b) the fused MACD-cross wave backtest: d_flag[4..6]
    def bt_check(k, inp, outs):
        ebuy, esell = oracle.macd_cross_signals(inp["host"])
        epos, ecash, eeq, es = oracle.backtest(inp["host"], ebuy, esell)
        for g, e in zip(outs[:3], (epos, ecash, eeq)):
            assert same_bits(g.cpu().numpy(), e).all()
        check_summary(outs[3].cpu().numpy(), es, "concurrency")
    fam["wave backtest"] = ([(130, 1100), (520, 1100)], wt_make, lambda inp: list(api.backtest_macd_cross(inp["x"])), bt_check)

    # (c) linear, K = 3: the tile partials in ws (one tile and a tail; four and a tail)
    def lin_make(shape):
        X, y = make_linear(3, shape, 0x5EED0E13, True)
        return {"xs": [dev(x) for x in X], "y": dev(y)}

    def lin_run(inp):
        r = api.linear(inp["xs"], inp["y"])
        return [r[k] for k in ("coef", "t_stat", "p_value", "r_squared", "n", "pred", "resid")]
    fam["linear"] = ([(api.LINEAR_TILE + 1,), (4 * api.LINEAR_TILE + 1,)], lin_make, lin_run, None)

    # (d) rank-IC, (e) one cross-sectional sort
    def xs_make(shape):
        f, r = make_factor("nulls", shape[0], shape[1], 0x5EED0E14)
        return {"f": dev(f), "r": dev(r)}
    fam["rank-IC"] = ([(255, 7), (1020, 7)], xs_make, lambda inp: list(api.factor_ic(inp["f"], inp["r"], 1)), None)

    def sort_run(inp):
        r = api.factor_quantiles(inp["f"], inp["r"], 5, labels=True)
        return [r[k] for k in ("labels", "count", "mean_return", "turnover", "spread", "summary")]
    fam["quantile sort"] = ([(37, 50), (148, 50)], xs_make, sort_run, None)

    # (f) an indicator on ragged groups of similar length: re-housed through rg_ws
    def rg_make(shape):
        lens = np.random.default_rng(0x5EED0E16).integers(170, 257, size=shape[0]).astype(np.int64)
        off = np.r_[0, np.cumsum(lens)]
        assert off[-1] >= 16384 and len(lens) * 256 <= 1.5 * off[-1]
        x = np.ascontiguousarray(oracle.gen_ohlcv(0x5EED0E16, 1, int(off[-1]), 0)["close"][0])
        return {"host": x, "x": dev(x), "off": off}

    def rg_check(k, inp, outs):
        got, off, x = outs[0].cpu().numpy().reshape(-1), inp["off"], inp["host"]
        for s in range(len(off) - 1):
            (e,) = oracle.call("sma", x[off[s]:off[s + 1]])
            e = np.asarray(e).reshape(-1)
            assert (got[off[s]:off[s + 1]].view(np.uint64) == e.view(np.uint64)).all(), s
    fam["ragged"] = ([(90,), (360,)], rg_make, lambda inp: list(api.call("sma", inp["x"], offsets=inp["off"])), rg_check)

    # (g) the mixed seven-rule sweep table, P = 65, L = 7, T = 3 R + 5
    R = api.SWEEP_ROW_TILE(7)

    def sw_make(shape):
        close = oracle.gen_ohlcv(0x5EED0003, shape[0], shape[1], 0)["close"]
        lines = S.make_lines(close, 7)
        return {"host": (close, lines), "p": dev(close), "l": [dev(l) for l in lines], "tab": S.make_table(api.SWEEP_RULE_DTYPE, 65, 7, None)}

    def sw_check(k, inp, outs):
        exp = S.oracle_cells(oracle, inp["host"][0], inp["host"][1], inp["tab"])
        P, N, _ = exp.shape
        check_summary(outs[0].cpu().numpy().reshape(P * N, 8), exp.reshape(P * N, 8), "concurrency sweep")
    fam["sweep"] = ([(3, 3 * R + 5), (12, 3 * R + 5)], sw_make, lambda inp: [api.backtest_sweep_rules(inp["p"], inp["l"], inp["tab"])], sw_check)

    # (h) a recorded Suite, replayed: the context's suite_aux streams.  The recording belongs to the context it was made on, so each
    # thread records its own (run() records on first use) and closes it itself
    def su_make(shape):
        d = oracle.gen_ohlcv(0x5EED0E18, shape[0], shape[1], 0)
        return {"host": d, "shape": shape, "suites": {}}

    def su_run(inp):
        st = inp["suites"].get(threading.get_ident())
        if st is None:
            st = Suite(inp["shape"][0], inp["shape"][1], "cuda")
            st.cols = _pitched(inp["host"], st.stride)          # well pitched: read in place
            st.record(st.cols, TASKS)
            inp["suites"][threading.get_ident()] = st
        outs = [t for name in ["sma"] + [m for t in TASKS if t in Suite.FUSED for m in Suite.FUSED[t]] for t in st.out[name]]
        outs += list(st.pat.values()) + st.bt + [st.summary]
        for t in outs:
            t.fill_(-7)                                          # every row must be written by the replay
        st.run()
        return outs

    def su_check(k, inp, outs):
        _subset_matches(pq, oracle, inp["suites"][threading.get_ident()], inp["host"])
    fam["suite"] = ([(70, 301), (280, 301)], su_make, su_run, su_check)
    return fam


def test_independent_contexts_every_kind_of_state(oracle):
    """api.ctx() is cached per (device, current stream) and torch's current stream is per thread: a worker under
    `with torch.cuda.stream(torch.cuda.Stream())` owns a context.  8 threads, one family of per-context state each -- gate flags, the
    d_flag statistics of the wave backtest, ws partials of linear / rank-IC / a quantile sort / the sweep, rg_ws, suite_aux streams --
    loop ten times, alternating between the family's small shape and one four times larger, so that a workspace is re-allocated while
    the other threads' kernels run.  Expected = the same calls made alone on the main thread first, every output bit for bit; the
    oracle-backed families are checked against the oracle once, by their own test's rule.  The d_flag counters a thread reads back from
    ITS context count its own symbols and nobody else's."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from polars_quant_amd import api
    with env(PQ_WT_ALL="1"):                        # (test_wt_gpu.py: every wave form, not only the ones that are the default)
        fam = _families(oracle)
        names = list(fam)
        assert len(names) == 8
        inputs, expected = {}, {}
        for nm in names:
            shapes, make, run, check = fam[nm]
            for k, shape in enumerate(shapes):
                inputs[nm, k] = make(shape)
                if nm == "wave indicator":
                    api.wt_stats(reset=True)
                if nm == "wave backtest":
                    api.backtest_wave_stats(reset=True)
                if nm == "ragged":
                    api.ragged_rehouse_stats(reset=True)
                outs = run(inputs[nm, k])
                expected[nm, k] = [raw(t) for t in outs]
                if nm == "wave indicator":
                    st = api.wt_stats()
                    assert st[0] == shape[0] and st[3] == 0, f"the wave form did not run: {st}"
                if nm == "wave backtest":
                    assert api.backtest_wave_stats()[0] == shape[0], "the wave form must have run"
                if nm == "ragged":
                    assert api.ragged_rehouse_stats() >= 1, "the re-housed path did not run"
                if check is not None and k == 0:
                    check(k, inputs[nm, k], outs)
                del outs
        for inp in inputs.values():                 # the main thread's recordings
            for st in inp.get("suites", {}).values():
                st.close()
            inp.get("suites", {}).clear()
        torch.cuda.synchronize()                    # the inputs were uploaded on the NULL stream; the workers' streams do not wait for it
        counters = {}

        def worker(nm):
            def job():
                run = fam[nm][2]
                with torch.cuda.stream(torch.cuda.Stream()):
                    # (api.ctx() is cached per stream handle and torch hands its pool streams out again: an earlier test of the
                    #  process may have counted on this context)
                    api.wt_stats(reset=True)
                    api.backtest_wave_stats(reset=True)
                    try:
                        for i in range(10):
                            k = i % 2
                            got = [raw(t) for t in run(inputs[nm, k])]
                            assert len(got) == len(expected[nm, k])
                            for j, (g, e) in enumerate(zip(got, expected[nm, k])):
                                assert g[:2] == e[:2] and g[2] == e[2], f"{nm}: output {j} of shape {fam[nm][0][k]} differs in round {i}"
                        if nm == "wave indicator":
                            counters[nm] = api.wt_stats()
                        if nm == "wave backtest":
                            counters[nm] = api.backtest_wave_stats()
                    finally:
                        for k in (0, 1):
                            st = inputs[nm, k].get("suites", {}).pop(threading.get_ident(), None)
                            if st is not None:
                                st.close()
                        torch.cuda.current_stream().synchronize()
            return job

        run_threads([worker(nm) for nm in names])
        per_thread = 5 * sum(s[0] for s in fam["wave indicator"][0])
        assert counters["wave indicator"][0] == per_thread and counters["wave indicator"][3] == 0, counters
        assert counters["wave backtest"][0] == per_thread, counters
