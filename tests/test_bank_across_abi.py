"""The bank's cross query (bf_bank_include_across*, include/bfhip.h) as far as it goes without a
GPU: exported symbols, the row-size helper and the refusals that come before any device call."""
import ctypes
import re
import subprocess

import pytest

NEW = ["bf_bank_across_row_bytes", "bf_bank_include_across", "bf_bank_include_across_dev"]


def test_across_symbols_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported and name in pkg._lib.SIGNATURES, name
    for name in ("across_row_bytes", "include_across", "include_across_dev"):
        assert callable(getattr(pkg.FilterBank, name)), name
    for name in ("include_across", "which"):
        assert callable(getattr(pkg.BloomfilterBank, name)), name


@pytest.mark.parametrize("count,want", [(0, 0), (1, 8), (63, 8), (64, 8), (65, 16), (128, 16), (129, 24),
                                        (1 << 32, 1 << 29), ((1 << 64) - 1, 1 << 61)])
def test_across_row_bytes(pkg, count, want):
    lib = pkg._lib.load()
    out = ctypes.c_uint64(7)
    assert lib.bf_bank_across_row_bytes(count, ctypes.byref(out)) == 0
    assert out.value == want
    assert pkg.FilterBank.across_row_bytes(count) == want


def test_across_row_bytes_null_out(pkg):
    assert pkg._lib.load().bf_bank_across_row_bytes(64, None) == pkg._lib.BF_EINVAL
    with pytest.raises(pkg.ArgumentError):
        pkg.FilterBank.across_row_bytes(-1)


def test_null_bank_is_einval_without_a_device(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.BF_EINVAL
    mask = (ctypes.c_uint8 * 16)(*([0xAB] * 16))
    offs = (ctypes.c_uint64 * 2)(0, 3)
    assert lib.bf_bank_include_across(None, b"abc", offs, 1, None, 1, mask) == E
    assert lib.bf_bank_include_across(None, None, None, 0, None, 0, None) == E
    assert lib.bf_bank_include_across_dev(None, None, None, 1, None, 1, None, None) == E
    assert lib.bf_bank_include_across_dev(None, None, None, 0, None, 0, None, None) == E
    assert bytes(mask) == b"\xab" * 16
