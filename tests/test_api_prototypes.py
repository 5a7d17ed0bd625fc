"""zxc_amd.api's prototype table against include/zxc_mi355x.h, without a GPU: every zxc_mi355x_* entry names a function the header
declares, with the same arity, the same scalar parameter and return types, and a pointer where the header has a pointer; the built
library exports every one of them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from zxc_amd import api

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "void": None}


def _ctype(decl):
    """'const zxc_dev_item_t* d_items' -> 'pointer'; 'uint32_t n_items', 'uint64_t' -> the ctypes scalar"""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    return SCALARS[words[0]]


def _header():
    text = open(os.path.join(ROOT, "include", "zxc_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, args in re.findall(r"ZXC_EXPORT\s+([\w\s]+?\*?)\s*(zxc_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [] if args.strip() == "void" else [_ctype(a) for a in args.split(",")]
        protos[name] = (_ctype(ret), args)
    return protos


HEADER = _header()
TABLE = {name: p for name, p in api._PROTOTYPES.items() if name.startswith("zxc_mi355x_")}


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents")


def _same(want, got):
    return _is_pointer(got) if want == "pointer" else got is want


def test_the_header_parses():
    assert len(HEADER) == 59 and len(TABLE) >= 40
    assert HEADER["zxc_mi355x_device_count"] == (C.c_int, [])
    assert HEADER["zxc_mi355x_malloc"] == ("pointer", [C.c_size_t])
    assert HEADER["zxc_mi355x_release_cached"] == (None, [])
    assert HEADER["zxc_mi355x_compress_append_device"] == (C.c_int, ["pointer", "pointer", C.c_uint64, "pointer"])


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_entry_matches_the_header(name):
    assert name in HEADER, f"{name} is not declared in include/zxc_mi355x.h"
    (want_ret, want_args), (ret, args) = HEADER[name], TABLE[name]
    assert _same(want_ret, ret), (name, "return type", ret)
    assert len(args) == len(want_args), (name, "arity", len(args), len(want_args))
    for i, (want, got) in enumerate(zip(want_args, args)):
        assert _same(want, got), (name, "parameter", i, got)


def test_the_library_exports_every_entry():
    if os.path.exists(api.lib_path()):
        L = api.lib()
        for name in TABLE:
            assert hasattr(L, name), name
            f = getattr(L, name)
            assert (f.restype, list(f.argtypes)) == (TABLE[name][0], TABLE[name][1]), name  # bound once, at load
