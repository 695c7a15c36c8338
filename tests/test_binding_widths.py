"""Every argtypes entry of the ctypes binding (x3-rust_amd/x3hip/__init__.py) is as wide as the parameter include/x3hip.h
declares: a 64-bit offset, length, position or count declared as a 32-bit ctypes type would pass tests on small streams and
truncate the first value above 2^32.  The prototypes are parsed from the header; no GPU is needed."""
import ctypes as C
import os
import re

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"uint64_t": 8, "int64_t": 8, "size_t": 8, "long long": 8, "double": 8, "uint32_t": 4, "int32_t": 4, "int": 4,
         "unsigned": 4, "uint16_t": 2, "int16_t": 2, "uint8_t": 1, "char": 1}


def prototypes():
    """{function: [bytes of each parameter as the C ABI passes it]} of every x3_* function the header declares"""
    text = open(os.path.join(ROOT, "include", "x3hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(x3_\w+)\s*\(([^(){};]*)\)\s*;", text):
        name, params = m.group(1), m.group(2).strip()
        sizes = []
        for prm in ([] if params in ("", "void") else params.split(",")):
            prm = " ".join(prm.split())
            if "*" in prm or "[" in prm:
                sizes.append(8)
                continue
            words = [w for w in re.findall(r"[A-Za-z_]\w*", prm) if w != "const"]
            base = "long long" if words[:2] == ["long", "long"] else words[0]
            assert base in SIZES, (name, prm)
            sizes.append(SIZES[base])
        out[name] = sizes
    return out


def test_argtypes_are_as_wide_as_the_header_says():
    L = x3hip.lib()
    protos = prototypes()
    assert set(x3hip.SYMBOLS) <= set(protos), sorted(set(x3hip.SYMBOLS) - set(protos))
    checked, wide = 0, 0
    for name in x3hip.SYMBOLS:
        at = getattr(L, name).argtypes
        if at is None:
            continue          # (bound where it is called: the multi-channel calls and x3_place_buffers)
        want = protos[name]
        got = [C.sizeof(t) for t in at]
        assert got == want, "%s: argtypes are %s bytes wide, the header says %s" % (name, got, want)
        checked += 1
        wide += want.count(8)
    assert checked >= len(x3hip.SYMBOLS) - 4 and wide > 500, (checked, wide)
    # the device entry points, whose arguments the tests beyond 4 GiB pass values above 2^32 through, are all bound up front
    dev = [n for n in x3hip.SYMBOLS if n.endswith("_dev") or n.startswith("x3_corpus_") or n.startswith("x3_tuner_")]
    assert len(dev) > 40 and all(getattr(L, n).argtypes is not None for n in dev)


def test_a_truncating_entry_would_be_caught():
    """the check is able to fail: x3_decode_windows_dev's n_windows as a 32-bit type"""
    protos = prototypes()
    at = list(x3hip.lib().x3_decode_windows_dev.argtypes)
    assert [C.sizeof(t) for t in at] == protos["x3_decode_windows_dev"]
    at[10] = C.c_uint32
    assert [C.sizeof(t) for t in at] != protos["x3_decode_windows_dev"]
