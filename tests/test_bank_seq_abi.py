"""The bank's sequential-flag insert (bf_bank_insert_many_seq*, bf_bank_seq_plan) as far as it
goes without a GPU: the exported symbols, the Python bindings and the refusals that come before
any device call."""
import ctypes
import re
import subprocess

import numpy as np

NEW = ["bf_bank_insert_many_seq", "bf_bank_insert_many_seq_dev", "bf_bank_seq_plan", "bf_bank_set_seq_form"]


def test_seq_symbols_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported, name
        assert name in pkg._lib.SIGNATURES, name
    lib = pkg._lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == pkg._lib.SIGNATURES[name][1]


def test_python_entry_points_are_callable(pkg):
    for name in ("insert_many_seq", "insert_many_seq_dev", "seq_plan", "set_seq_form"):
        assert callable(getattr(pkg.FilterBank, name)), name
    for name in ("first_seen_many", "first_seen"):
        assert callable(getattr(pkg.BloomfilterBank, name)), name
    assert callable(pkg.bank.BankFilter.first_seen)


def test_null_bank_is_einval_and_outputs_untouched(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.BF_EINVAL
    keys = np.frombuffer(b"abcdef" + b"\0" * 16, np.uint8).copy()
    offs = np.array([0, 3, 6], np.uint64)
    ids = np.zeros(2, np.uint32)
    flags = np.full(2, 7, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for n in (0, 2):
        assert lib.bf_bank_insert_many_seq(None, p(keys), p(offs), p(ids), n, p(flags)) == E
        assert lib.bf_bank_insert_many_seq_dev(None, p(keys), p(offs), p(ids), n, p(flags), None) == E
    assert lib.bf_bank_insert_many_seq(None, None, None, None, 0, None) == E
    assert lib.bf_bank_insert_many_seq_dev(None, None, None, None, 0, None, None) == E
    assert flags.tolist() == [7, 7]
    direct, chunk, scratch = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.bf_bank_seq_plan(None, 1000, ctypes.byref(direct), ctypes.byref(chunk), ctypes.byref(scratch)) == E
    assert lib.bf_bank_seq_plan(None, 0, None, None, None) == E
    assert (direct.value, chunk.value, scratch.value) == (7, 7, 7)
    for form in (0, 1, 2, 3):
        assert lib.bf_bank_set_seq_form(None, form) == E
