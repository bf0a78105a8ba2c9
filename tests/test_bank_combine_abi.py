"""The bank's combines (bf_bank_fold*, bf_bank_overlap*, include/bfhip.h) as far as they go without
a GPU: exported symbols, the bindings and the refusal that comes before any device call."""
import ctypes
import re
import subprocess

NEW = ["bf_bank_fold", "bf_bank_fold_dev", "bf_bank_overlap", "bf_bank_overlap_dev"]


def test_combine_symbols_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported and name in pkg._lib.SIGNATURES, name
    for name in ("fold", "fold_dev", "overlap", "overlap_dev"):
        assert callable(getattr(pkg.FilterBank, name)), name
    for name in ("merge", "rollup", "union_size", "intersection_size", "overlap"):
        assert callable(getattr(pkg.BloomfilterBank, name)), name


def test_null_bank_is_einval_without_a_device(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.BF_EINVAL
    OR = pkg._lib.BF_BITOP_OR
    seg = (ctypes.c_uint64 * 2)(0, 2)
    src = (ctypes.c_uint32 * 2)(0, 1)
    dst = (ctypes.c_uint32 * 1)(0)
    changed = (ctypes.c_uint8 * 4)(*([0xAB] * 4))
    counts = (ctypes.c_uint64 * 4)(*([0xABABABAB] * 4))
    assert lib.bf_bank_fold(None, OR, dst, seg, src, 1, changed, counts) == E
    assert lib.bf_bank_fold(None, OR, None, None, None, 0, None, None) == E
    assert lib.bf_bank_fold_dev(None, OR, dst, seg, src, 1, 2, changed, counts, None) == E
    assert lib.bf_bank_fold_dev(None, OR, None, None, None, 0, 0, None, None, None) == E
    assert lib.bf_bank_overlap(None, src, 2, src, 2, counts) == E
    assert lib.bf_bank_overlap(None, None, 0, None, 0, None) == E
    assert lib.bf_bank_overlap_dev(None, src, 2, src, 2, counts, None) == E
    assert lib.bf_bank_overlap_dev(None, None, 0, None, 0, None, None) == E
    assert bytes(changed) == b"\xab" * 4
    assert list(counts) == [0xABABABAB] * 4
