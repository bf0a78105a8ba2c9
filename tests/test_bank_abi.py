"""The filter-bank entry points of include/bfhip.h (bf_bank_*) as far as they go without a GPU:
exported symbols, the argument refusals that come before any device call, the stride helper,
and the ``BloomfilterBank`` facade's argument checks."""
import ctypes
import re
import subprocess

import pytest

NEW = ["bf_bank_create", "bf_bank_destroy", "bf_bank_last_error", "bf_bank_info", "bf_bank_stride",
       "bf_bank_stream", "bf_bank_sync", "bf_bank_insert_many", "bf_bank_insert_many_dev",
       "bf_bank_include_many", "bf_bank_include_many_dev", "bf_bank_clear", "bf_bank_clear_dev",
       "bf_bank_bitcount", "bf_bank_bitcount_dev", "bf_bank_export_filters", "bf_bank_import_filters"]


def test_bank_symbols_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported and name in pkg._lib.SIGNATURES, name
    assert pkg.FilterBank is pkg._lib.FilterBank


def _create(pkg, m, k, n, cfg=None):
    lib = pkg._lib.load()
    h = ctypes.c_void_p(0x1234)
    rc = lib.bf_bank_create(m, k, n, ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(h))
    return rc, h.value, lib.bf_bank_last_error(None).decode()


def _cfg(pkg, **kw):
    cfg = pkg._lib.bf_config(ctypes.sizeof(pkg._lib.bf_config), -1, 0, 0, 0, 0, 0, 0)
    for name, v in kw.items():
        setattr(cfg, name, v)
    return cfg


@pytest.mark.parametrize("m,k,n,what", [
    (0, 6, 4, "m_bits == 0"),
    (9585, 0, 4, "k must be"),
    (9585, 65, 4, "k must be"),
    (9585, 6, 0, "n_filters == 0"),
    (9585, 6, (1 << 32) + 1, "n_filters"),
    ((1 << 64) - 1, 6, 8, "overflow"),            # 2^61-byte filters x 8
    (1 << 40, 6, 1 << 30, "overflow"),            # 2^37-byte filters x 2^30
])
def test_create_argument_refusals_need_no_device(pkg, m, k, n, what):
    rc, h, msg = _create(pkg, m, k, n)
    assert rc == pkg._lib.BF_EINVAL and h is None
    assert what in msg, msg


def test_create_errors_are_per_family(pkg):
    """bf_last_error(NULL), bf_bank_last_error(NULL) and bf_lua_last_error(NULL) are three
    strings: a refused bank or Lua create leaves the single filter's create error alone."""
    lib = pkg._lib.load()
    E = pkg._lib.BF_EINVAL
    h = ctypes.c_void_p()
    assert lib.bf_create(0, 6, None, ctypes.byref(h)) == E
    single = lib.bf_last_error(None)
    assert b"m_bits == 0" in single
    assert lib.bf_bank_create(9585, 6, 0, None, ctypes.byref(h)) == E
    assert lib.bf_lua_create(-1.0, 0.01, None, ctypes.byref(h)) == E
    assert b"n_filters == 0" in lib.bf_bank_last_error(None)
    assert b"entries must be > 0" in lib.bf_lua_last_error(None)
    assert lib.bf_last_error(None) == single
    assert b"n_filters" not in single and b"entries" not in single


@pytest.mark.parametrize("field,value", [
    ("shard_count", 2), ("shard_index", 1), ("device_count", 1),
    ("flags", 2), ("flags", 4), ("flags", 8), ("flags", 1)])   # ENGINE_MD5, ENGINE_SHA1, ENCODER, ROUTE32
def test_create_refuses_every_config_field_but_device_and_batch(pkg, field, value):
    rc, h, msg = _create(pkg, 9585, 6, 4, _cfg(pkg, **{field: value}))
    assert rc == pkg._lib.BF_EINVAL and h is None and msg
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL"):
        pkg.FilterBank(0, 6, 4)


def test_create_null_out(pkg):
    lib = pkg._lib.load()
    assert lib.bf_bank_create(9585, 6, 4, None, None) == pkg._lib.BF_EINVAL
    assert b"out is NULL" in lib.bf_bank_last_error(None)


def test_bank_stride(pkg):
    stride = pkg._lib.bank_stride
    assert stride(1) == 128
    assert stride(9585) == 1280          # 1,199 bytes -> ten cache lines
    assert stride(95851) == 12032
    for j in (1, 2, 7, 94, 1 << 20):
        assert stride(8 * 128 * j) == 128 * j     # a whole number of lines: m / 8
        assert stride(8 * 128 * j + 1) == 128 * (j + 1)
    lib = pkg._lib.load()
    out = ctypes.c_uint64(7)
    E = pkg._lib.BF_EINVAL
    assert lib.bf_bank_stride(0, ctypes.byref(out)) == E
    assert lib.bf_bank_stride(9585, None) == E
    assert out.value == 7
    assert stride((1 << 64) - 1) == 1 << 61       # the largest m still has a 64-bit stride
    with pytest.raises(pkg.ArgumentError):
        stride(0)


def test_null_bank_is_einval_everywhere(pkg):
    lib = pkg._lib.load()
    E = pkg._lib.BF_EINVAL
    p = ctypes.c_void_p()
    n = ctypes.c_uint64(7)
    assert lib.bf_bank_destroy(None) == 0
    assert lib.bf_bank_info(None, ctypes.byref(n), None, None, None, None) == E
    assert lib.bf_bank_stream(None, ctypes.byref(p)) == E
    assert lib.bf_bank_sync(None) == E
    assert lib.bf_bank_insert_many(None, None, None, None, 0, None) == E
    assert lib.bf_bank_insert_many_dev(None, None, None, None, 0, None, None) == E
    assert lib.bf_bank_include_many(None, None, None, None, 0, None) == E
    assert lib.bf_bank_include_many_dev(None, None, None, None, 0, None, None) == E
    assert lib.bf_bank_clear(None, None, 0) == E
    assert lib.bf_bank_clear_dev(None, None, 0, None) == E
    assert lib.bf_bank_bitcount(None, None, 0, None) == E
    assert lib.bf_bank_bitcount_dev(None, None, 0, None, None) == E
    assert lib.bf_bank_export_filters(None, None, 0, None, None) == E
    assert lib.bf_bank_import_filters(None, None, 0, None, None, 0) == E
    assert n.value == 7


def test_facade_argument_errors_need_no_device(pkg):
    B = pkg.BloomfilterBank
    r = pkg.FakeRedis()
    with pytest.raises(pkg.ArgumentError, match="cannot be nil"):
        B(error_rate=0.01, key_names=["a"], redis=r)
    with pytest.raises(pkg.ArgumentError, match="cannot be nil"):
        B(size=1000, key_names=["a"], redis=r)
    with pytest.raises(pkg.ArgumentError, match="at least one"):
        B(size=1000, error_rate=0.01, key_names=[], redis=r)
    with pytest.raises(pkg.ArgumentError, match="at least one"):
        B(size=1000, error_rate=0.01, redis=r)
    with pytest.raises(pkg.ArgumentError, match="repeats 'b'"):
        B(size=1000, error_rate=0.01, key_names=["a", "b", "c", "b"], redis=r)
    with pytest.raises(pkg.ArgumentError, match="sync must be"):
        B(size=1000, error_rate=0.01, key_names=["a"], redis=r, sync="sometimes")
