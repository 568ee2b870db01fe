"""The all-patterns kernel (pattern.hip cdl_all_kernel<ALL, VEC>) in every form it is launched in, against the single-recogniser kernel
(cdl_one_kernel, 61 calls of api.cdl) and the oracle.  Every comparison is exact int32 equality.

The kernel evaluates the recognisers in an order of its own (grouped by look-back) and reads column pointer and penetration of the k-th
one from slot k of its argument: a wrong slot shows as one recogniser's values in another one's column, or as a penetration applied to the
wrong recogniser -- hence inputs on which (nearly) every recogniser fires, and penetrations that all differ.

- lengths 1, 2, 4, 5 (rows below every look-back 0 .. 4), 255 / 256 / 257 (one block of ROW_BLOCK = 256 rows, its edge) and 513 (a ragged
  last block), 3 series each, at a dense row pitch and at one padded to 16 elements whose padding must stay untouched;
- subsets (the ALL = false instantiations): unrequested columns are not written;
- a ragged batch (the VEC = false instantiations); a recorded suite replayed twice."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pattern_kats import KATS, PEN_CASES, UNSAT, kat_series  # noqa: E402
from test_gpu_parity import pq  # noqa: E402,F401  (the module fixture)

LENS = (1, 2, 4, 5, 255, 256, 257, 513)
STARTS = (0, 30, 60)          # the three series start at different firing sequences of tests/pattern_kats.py
SENT = -7                     # no recogniser writes it
PEN_IDS = (14, 19, 20, 42, 43, 45)   # the recognisers that read their penetration
# all different, none a default (0.5 / 0.3): on the probe series below every one of them changes its recogniser's output
PENS = {14: 0.45, 19: 0.1, 20: 0.15, 42: 0.2, 43: 0.12, 45: 0.4}
FLAT = (10.0, 10.0, 10.0, 10.0)


@functools.lru_cache(maxsize=None)
def _host(T):
    """3 x T OHLC of tiled firing sequences (read-only)"""
    cols = [kat_series(T, s)[:4] for s in STARTS]
    out = tuple(np.stack([c[k] for c in cols]) for k in range(4))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(T):
    """oracle output of every recogniser at its default penetration for _host(T), computed once (read-only)"""
    from oracle import pq_oracle as oracle
    from polars_quant_amd import PATTERN_NAMES
    exp = {nm: oracle.pattern(nm, *_host(T)) for nm in PATTERN_NAMES}
    for a in exp.values():
        a.setflags(write=False)
    return exp


def _probe_host(T=257):
    """3 x T: two tiled series + one that is sensitive to the penetration: every hand-built case (firing or not) of the six recognisers,
    the PEN_CASES sequences, and the evening-star shape closing at 11.5 (fires iff 11.5 < 12 - 2 pen)"""
    from polars_quant_amd import PATTERN_NAMES
    seqs = [cs for i in PEN_IDS for cs, _, _ in KATS[PATTERN_NAMES[i]]] + [cs for _, cs, _, _ in PEN_CASES]
    seqs.append([(10, 12.1, 9.9, 12), (12.5, 12.9, 12.4, 12.8), (12.3, 12.4, 11.4, 11.5)])
    rows = []
    k = 0
    while len(rows) < T:
        rows.extend(seqs[k % len(seqs)])
        rows.append(FLAT)
        k += 1
    a = np.asarray(rows[:T], dtype=np.float64)
    base = [kat_series(T, s)[:4] for s in STARTS[:2]]
    return tuple(np.stack([base[0][j], base[1][j], a[:, j]]) for j in range(4))


def _device(host, stride):
    """[n, T] host columns -> device views with a row pitch of `stride` elements"""
    out = []
    for v in host:
        buf = torch.zeros((v.shape[0], stride), dtype=torch.float64, device="cuda")
        buf[:, : v.shape[1]] = torch.from_numpy(np.array(v)).cuda()
        out.append(buf[:, : v.shape[1]])
    return out


def _cdl_all_into(batch, cols, outs, pens=None):
    """pq_cdl_all into the caller's buffers: outs = {recogniser id: int32 tensor}, every other column pointer is null"""
    from polars_quant_amd._lib import check, lib
    from polars_quant_amd._spec import PATTERN_NAMES, PATTERN_PEN_DEFAULT
    from polars_quant_amd.api import ctx
    pv = (C.c_double * 61)(*[(pens or {}).get(i, PATTERN_PEN_DEFAULT[PATTERN_NAMES[i]]) for i in range(61)])
    ptrs = (C.c_void_p * 61)(*[outs[i].data_ptr() if i in outs else None for i in range(61)])
    check(lib().pq_cdl_all(ctx(0), C.byref(batch), *[C.c_void_p(t.data_ptr()) for t in cols], pv, ptrs))
    torch.cuda.synchronize()


def test_tiled_sequences_fire_every_satisfiable_recogniser():
    """zeros must not be compared with zeros: in the reference output at len 513 every recogniser but the unsatisfiable cdl2crows
     fires, in the first series alone"""
    exp = _expected(513)
    silent = [nm for nm, e in exp.items() if not (e[0] != 0).any()]
    assert silent == list(UNSAT), silent
    for T in (255, 256, 257):
        silent = [nm for nm, e in _expected(T).items() if not (e != 0).any()]
        assert silent == list(UNSAT), (T, silent)


@pytest.mark.parametrize("pitch", ["dense", "padded16"])
@pytest.mark.parametrize("T", LENS)
def test_fused_equals_single_and_oracle(pq, T, pitch):
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    n = len(STARTS)
    stride = T if pitch == "dense" else (T + 15) // 16 * 16
    cols = _device(_host(T), stride)
    exp = _expected(T)
    assert cols[0].stride(0) == stride
    # the fused kernel into sentinel-filled [n, stride] buffers
    bufs = {i: torch.full((n, stride), SENT, dtype=torch.int32, device="cuda") for i in range(61)}
    _cdl_all_into(Batch(n, T, stride, None), cols, bufs)
    fused = api.cdl_all(*cols)                                  # the same through the API (its own output tensors)
    for i, nm in enumerate(pq.PATTERN_NAMES):
        e = torch.from_numpy(exp[nm]).cuda()
        assert torch.equal(bufs[i][:, :T], e), f"{nm}: fused != oracle"
        assert bool((bufs[i][:, T:] == SENT).all()), f"{nm}: the padding of the rows was written"
        assert torch.equal(fused[nm], e), f"{nm}: api.cdl_all != oracle"
        single = api.cdl(nm, *cols)                             # cdl_one_kernel
        assert torch.equal(single, bufs[i][:, :T]), f"{nm}: fused != single"


@pytest.mark.parametrize("pitch", ["dense", "padded16"])
@pytest.mark.parametrize("subset", ["first", "last", "penetrations"])
def test_subsets_write_only_what_was_asked_for(pq, oracle, subset, pitch):
    """the ALL = false instantiations: only id 0, only id 60, and the six recognisers that read a penetration, each with another one"""
    from polars_quant_amd import api
    from polars_quant_amd._lib import Batch
    from polars_quant_amd._spec import PATTERN_PEN_DEFAULT
    T, n = 257, 3
    host = _probe_host(T)
    ids = {"first": (0,), "last": (60,), "penetrations": PEN_IDS}[subset]
    stride = T if pitch == "dense" else (T + 15) // 16 * 16
    cols = _device(host, stride)
    bufs = {i: torch.full((n, stride), SENT, dtype=torch.int32, device="cuda") for i in range(61)}
    _cdl_all_into(Batch(n, T, stride, None), cols, {i: bufs[i] for i in ids}, PENS)
    names = [pq.PATTERN_NAMES[i] for i in ids]
    via_api = api.cdl_all(*cols, names=names, penetrations={pq.PATTERN_NAMES[i]: p for i, p in PENS.items()})
    assert sorted(via_api) == sorted(names)
    for i in range(61):
        nm = pq.PATTERN_NAMES[i]
        if i not in ids:
            assert bool((bufs[i] == SENT).all()), f"{nm} was not requested but its column was written"
            continue
        pen = PENS.get(i)
        e = oracle.pattern(nm, *host, penetration=pen)
        if pen is not None:   # (a condition on the reference: the penetration matters on this input, and zeros are not compared with zeros)
            assert pen != PATTERN_PEN_DEFAULT[nm] and (e != 0).any() and (e != oracle.pattern(nm, *host)).any(), nm
        elif nm not in UNSAT:
            assert (e != 0).any(), nm
        e = torch.from_numpy(e).cuda()
        assert torch.equal(bufs[i][:, :T], e), f"{nm}: subset != oracle"
        assert bool((bufs[i][:, T:] == SENT).all()), f"{nm}: the padding of the rows was written"
        assert torch.equal(via_api[nm], e), f"{nm}: api.cdl_all(names=) != oracle"
        assert torch.equal(api.cdl(nm, *cols, penetration=pen), e), f"{nm}: single != oracle"


@pytest.mark.parametrize("which", ["all", "penetrations"])
def test_ragged_batch(pq, oracle, which):
    """groups of 1, 5 and 257 rows of one long column (the VEC = false instantiations, with and without every column)"""
    from polars_quant_amd import api
    lens = (1, 5, 257)
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    total = int(off[-1])
    groups = [kat_series(L, s)[:4] for L, s in zip(lens, (3, 9, 0))]
    longc = [np.concatenate([g[k] for g in groups]) for k in range(4)]
    cols = [torch.from_numpy(c).cuda() for c in longc]
    ids = tuple(range(61)) if which == "all" else PEN_IDS
    pens = PENS
    bufs = {i: torch.full((total + 16,), SENT, dtype=torch.int32, device="cuda") for i in range(61)}
    b, keep = api.ragged_batch(off, cols[0].device)
    _cdl_all_into(b, cols, {i: bufs[i] for i in ids}, pens)
    del keep
    fired = 0
    for i in range(61):
        nm = pq.PATTERN_NAMES[i]
        if i not in ids:
            assert bool((bufs[i] == SENT).all()), f"{nm} was not requested but its column was written"
            continue
        pen = pens.get(i)
        e = np.concatenate([oracle.pattern(nm, *g, penetration=pen) for g in groups])
        fired += int((e != 0).any())
        assert torch.equal(bufs[i][:total], torch.from_numpy(e).cuda()), f"{nm}: ragged fused != oracle"
        assert bool((bufs[i][total:] == SENT).all()), f"{nm}: rows behind the last group were written"
        single = api.cdl(nm, *cols, penetration=pen, offsets=off)
        assert torch.equal(single.reshape(-1), bufs[i][:total]), f"{nm}: ragged fused != single"
    assert fired >= (50 if which == "all" else len(PEN_IDS)), fired


def test_recorded_suite_replays_bit_identically(pq, oracle):
    """cdl_all recorded into a suite at 130 x 300 and replayed twice: both replays are the direct call's output"""
    from polars_quant_amd import api
    from polars_quant_amd.suite import Suite
    n, T = 130, 300
    d = oracle.gen_ohlcv(0x5EED0C01, n, T, 1)
    for sym, start in ((0, 0), (n - 1, 44)):
        d["open"][sym], d["high"][sym], d["low"][sym], d["close"][sym] = kat_series(T, start)[:4]
    st = Suite(n, T, "cuda")
    g = {k: torch.zeros((n, st.stride), dtype=torch.float64, device="cuda")[:, :T] for k in d}
    for k, v in d.items():
        g[k].copy_(torch.from_numpy(v))
    st.record(g, ["cdl_all"])
    direct = api.cdl_all(*[g[k] for k in ("open", "high", "low", "close")])
    assert sum(int(bool((v != 0).any())) for v in direct.values()) == 61 - len(UNSAT)
    for replay in range(2):
        for t in st.pat.values():
            t.fill_(SENT)
        st.run()
        torch.cuda.synchronize()
        for nm in pq.PATTERN_NAMES:
            assert torch.equal(st.pat[nm], direct[nm]), f"{nm}: replay {replay} != direct call"
    st.close()
