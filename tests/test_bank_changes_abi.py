"""bf_bank_insert_many_changes / _dev (include/bfhip.h) as far as they go without a GPU: the
symbols are exported, bound with the header's arguments and declared, the Python methods exist,
the facade knows the sync mode, and a NULL bank is refused before any output is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip.h")
NEW = ["bf_bank_insert_many_changes", "bf_bank_insert_many_changes_dev"]

# the header's C types as _lib.SIGNATURES spells them
C_TYPES = {"bf_bank*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p, "const uint64_t*": ctypes.c_void_p,
           "const uint32_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p, "uint32_t*": ctypes.c_void_p,
           "void*": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ret, args = re.search(r"\b(\w+)\s+%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S).groups()
    types = [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", "*") for a in args.split(",")]
    return ret, types


def test_symbols_exported_bound_and_declared(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported, name
        restype, argtypes = pkg._lib.SIGNATURES[name]
        ret, types = header_args(name)
        assert ret == "int" and restype is ctypes.c_int
        assert len(types) == len(argtypes), (name, types)
        for pos, (t, a) in enumerate(zip(types, argtypes)):
            if t == "uint64_t*":   # the host form's count may be the typed pointer: the binding passes byref(c_uint64)
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, pos, t, a)
            else:
                assert a is C_TYPES[t], (name, pos, t, a)
    host, dev = (header_args(n)[1] for n in NEW)
    assert dev[:-1] == host and dev[-1] == "void*"               # the _dev form: the same arguments and a stream
    assert host[5] == "uint32_t" and host[9] == "uint64_t"       # seq, cap


def test_python_surface(pkg):
    assert callable(pkg.FilterBank.insert_many_changes) and callable(pkg.FilterBank.insert_many_changes_dev)
    assert "write_through_bits" in pkg.BloomfilterBank.SYNC_MODES
    assert pkg.BloomfilterBank.SYNC_MODES[:2] == ("write_through", "manual")
    assert pkg.BloomfilterBank.SETBIT_BYTES is pkg.Hip.SETBIT_BYTES   # the one constant


@pytest.mark.parametrize("n", [0, 2])
def test_null_bank_is_einval_and_touches_nothing(pkg, n):
    lib = pkg._lib.load()
    keys = np.frombuffer(b"ab" + b"\0" * 16, np.uint8).copy()
    offs = np.array([0, 1, 2], np.uint64)
    fids = np.zeros(2, np.uint32)
    flags = np.full(2, 0xAB, np.uint8)
    ids = np.full(12, 0xCDCDCDCD, np.uint32)
    bits = np.full(12, 0xEFEFEFEFEFEFEFEF, np.uint64)
    count = ctypes.c_uint64(77)
    args = (None, keys.ctypes.data, offs.ctypes.data, fids.ctypes.data, n, 0, flags.ctypes.data, ids.ctypes.data,
            bits.ctypes.data, 12)
    assert lib.bf_bank_insert_many_changes(*args, ctypes.byref(count)) == pkg._lib.BF_EINVAL
    assert lib.bf_bank_insert_many_changes_dev(*args, ctypes.addressof(count), None) == pkg._lib.BF_EINVAL
    assert count.value == 77
    assert (flags == 0xAB).all() and (ids == 0xCDCDCDCD).all() and (bits == 0xEFEFEFEFEFEFEFEF).all()
