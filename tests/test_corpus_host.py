"""Corpus windows on the host side (no GPU): the library exports the x3_corpus_* entry points, the Rust shim declares them,
and x3hip.Corpus refuses bad host arguments before it touches the device."""
import os
import re

import numpy as np
import pytest

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["x3_corpus_build", "x3_corpus_info", "x3_corpus_entries", "x3_corpus_seg_index", "x3_corpus_windows_dev",
         "x3_corpus_destroy"]


def test_library_exports_the_corpus_entry_points():
    L = x3hip.lib()
    for name in NAMES:
        assert name in x3hip.SYMBOLS
        assert hasattr(L, name), name


def test_rust_shim_declares_the_corpus_entry_points():
    rs = open(os.path.join(ROOT, "x3-rust_amd", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, rs), name
    assert re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_corpus_entry\s*\{", rs)
    assert "pub struct Corpus" in rs


def test_corpus_entry_dtype_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "x3hip.h")).read()
    body = re.search(r"typedef\s+struct\s+x3_corpus_entry\s*\{(.*?)\}\s*x3_corpus_entry\s*;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == list(x3hip.CORPUS_ENTRY_DTYPE.names)
    assert x3hip.CORPUS_ENTRY_DTYPE.itemsize == 32


class _NoDevice:
    """a context stand-in that fails the test if the Corpus touches it"""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


@pytest.mark.parametrize("offsets,lengths,kw", [
    ([], [], {}),                                      # no entry
    ([0, 1], [1], {}),                                 # offsets and lengths differ
    ([[0]], [[1]], {}),                                # not 1-D
    ([0], [101], {}),                                  # past the buffer
    ([101], [0], {}),                                  # starts past the buffer
    ([50], [51], {}),                                  # ends past the buffer
    ([0], [10], {"flags": 2}),                         # unknown flag
    ([0], [10], {"seg_blocks": 30}),                   # not a multiple of 4
    ([0], [10], {"seg_blocks": 3204}),                 # too many blocks
    ([0], [10], {"seg_blocks": -4}),
])
def test_corpus_refuses_bad_host_arguments_before_the_device(offsets, lengths, kw):
    with pytest.raises(ValueError):
        x3hip.Corpus(_NoDevice(), np.zeros(100, dtype=np.uint8), offsets, lengths, **kw)
