"""not-gpu: the ctypes side of the binding against include/pq_hip.h -- every prototype has argtypes and a restype of the header's
kinds, and the structures and record dtypes of the Python side have the header's fields in the header's order."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

SCALARS = {"int32_t": C.c_int32, "pq_status": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double,
           "size_t": C.c_size_t}
NUMPY = {"int32_t": "<i4", "int64_t": "<i8", "double": "<f8"}


def header():
    txt = (ROOT / "include" / "pq_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def prototypes():
    """[(return type, name, [parameter declarations])]"""
    out = []
    for ret, name, params in re.findall(r"([\w \*]+?)\b(pq_\w+)\s*\(([^;{]*?)\)\s*;", header()):
        params = " ".join(params.split())
        out.append((" ".join(ret.split()), name, [] if params in ("", "void") else [p.strip() for p in params.split(",")]))
    return out


def structs():
    """name -> [(field, C type)] of every `typedef struct { ... } pq_x;`"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(pq_\w+)\s*;", header()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(\*?\s*\w+(?:\s*,\s*\w+)*)", decl)
            assert m, decl
            ctype, names = m.groups()
            for nm in names.split(","):
                nm = nm.strip()
                fields.append((nm.lstrip("* "), ctype + (" *" if nm.startswith("*") else "")))
        out[name] = fields
    return out


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C.Array)))


STRUCTS = {"pq_batch": "Batch", "pq_bt_params": "BtParams", "pq_lev_params": "LevParams", "pq_seq_params": "SeqParams"}


def kind_matches(decl, t):
    """a C declaration (`const double *x`, `int64_t n`, a return type) against a ctypes type; a pointer to one of the structures that
    have a Python class takes a POINTER to that class and nothing else"""
    if "*" in decl or "[" in decl:
        for c, py in STRUCTS.items():
            if re.search(r"\b%s\b" % c, decl):
                from polars_quant_amd import _lib
                return t is C.POINTER(getattr(_lib, py))
        return is_pointer(t)
    base = decl.replace("const", " ").split()[0]
    return t is SCALARS[base]


def mismatches(L):
    bad = []
    for ret, name, params in prototypes():
        fn = getattr(L, name)
        if fn.argtypes is None:
            bad.append(f"{name}: no argtypes")
        elif len(fn.argtypes) != len(params):
            bad.append(f"{name}: {len(fn.argtypes)} argtypes for {len(params)} parameters")
        else:
            bad += [f"{name}: parameter {k} `{p}` declared as {t.__name__}" for k, (p, t) in enumerate(zip(params, fn.argtypes))
                    if not kind_matches(p, t)]
        if not kind_matches(ret + " r" if "*" not in ret else ret, fn.restype):
            bad.append(f"{name}: returns `{ret}`, restype {getattr(fn.restype, '__name__', fn.restype)}")
    return bad


@pytest.fixture(scope="module")
def L():
    from polars_quant_amd._lib import lib
    return lib()


def test_the_header_is_parsed_whole():
    protos = prototypes()
    assert len(protos) >= 168 and len({n for _, n, _ in protos}) == len(protos)
    assert {r for r, _, _ in protos} == {"pq_status", "int32_t", "int64_t", "const char *"}
    assert sorted(n for _, n, _ in protos) == sorted(set(re.findall(r"\b(pq_[a-z0-9_]+)\s*\(", header())))    # test_abi_exports' list


def test_every_prototype_has_the_headers_signature(L):
    bad = mismatches(L)
    assert not bad, "\n".join(bad)


def test_a_params_slot_refuses_another_struct(L):
    from polars_quant_amd._lib import BtParams, LevParams
    slot = L.pq_backtest_vectorized.argtypes[6]
    slot.from_param(C.byref(BtParams()))
    with pytest.raises(TypeError):
        slot.from_param(C.byref(LevParams()))


@pytest.mark.parametrize("py,c", [(py, c) for c, py in STRUCTS.items()])
def test_structures_have_the_headers_fields(py, c):
    from polars_quant_amd import _lib
    want = structs()[c]
    got = getattr(_lib, py)._fields_
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, ct) in zip(got, want):
        assert kind_matches(ct + " " + n if "*" not in ct else ct, t), (n, ct, t)


@pytest.mark.parametrize("py,c", [("SWEEP_PARAM_DTYPE", "pq_sweep_param"), ("SWEEP_RULE_DTYPE", "pq_sweep_rule")])
def test_record_dtypes_have_the_headers_fields(py, c):
    from polars_quant_amd import api
    want = structs()[c]
    dt = getattr(api, py)
    assert list(dt.names) == [n for n, _ in want]
    assert [dt[n].str for n in dt.names] == [NUMPY[ct] for _, ct in want]
    assert dt.itemsize == sum(np.dtype(NUMPY[ct]).itemsize for _, ct in want)      # no padding the C struct lacks
