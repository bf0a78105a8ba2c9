"""ctypes binding of libbfhip.so (the C ABI in include/bfhip.h).

This is the only way the package reaches the engine: there is no CPU
fallback.  If the shared library is missing or fails to load, importing the
driver raises ``BfHipUnavailable``.
"""
from __future__ import annotations

import ctypes
import functools
import os
import sys
import threading
from typing import List, Optional, Tuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(PKG_DIR, "lib", "libbfhip.so")

BF_OK, BF_EINVAL, BF_ENOMEM, BF_EDEVICE, BF_ERCCL, BF_ERANGE = 0, 1, 2, 3, 4, 5
BF_IMPORT_REPLACE, BF_IMPORT_OR = 0, 1
BF_BITOP_AND, BF_BITOP_OR, BF_BITOP_XOR = 0, 1, 2   # XOR: bitcount_op only
BF_FLAG_ROUTE32 = 1
BF_FLAG_ENGINE_MD5, BF_FLAG_ENGINE_SHA1 = 2, 4   # RubyTest hash engines (ruby_test.rb:43-61)
BF_FLAG_ENCODER = 8   # no bitset: region-set encodes only (a replicated filter's second, encoding handle)
BF_MAX_K = 64
PROFILE_NAME_LEN = 64   # BF_PROFILE_NAME_LEN
DIRTY_BLOCK_BYTES = 65536   # BF_DIRTY_BLOCK_BYTES

_STATUS = {BF_EINVAL: "BF_EINVAL", BF_ENOMEM: "BF_ENOMEM", BF_EDEVICE: "BF_EDEVICE",
           BF_ERCCL: "BF_ERCCL", BF_ERANGE: "BF_ERANGE"}


class BfHipUnavailable(ImportError):
    """libbfhip.so could not be loaded (not built, or no HIP runtime)."""


class BfHipError(RuntimeError):
    """A non-argument failure reported by the engine (device, memory, collective)."""

    def __init__(self, code: int, msg: str):
        super().__init__("%s: %s" % (_STATUS.get(code, "BF_E%d" % code), msg))
        self.code = code


class ArgumentError(ValueError):
    """Mirror of Ruby's ArgumentError (raised where the reference raises it)."""


BF_MAX_DEVICES = 16
BF_MODE_REPLICATED, BF_MODE_PARTITIONED = 0, 1


class bf_config(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("batch_keys", ctypes.c_uint64), ("batch_bytes", ctypes.c_uint64),
                ("shard_count", ctypes.c_uint32), ("shard_index", ctypes.c_uint32),
                ("shard_block_log2", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("device_count", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("devices", ctypes.c_int32 * BF_MAX_DEVICES)]


class bf_plan_detail(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_uint64), ("tiles", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64),
                ("planned", ctypes.c_uint32), ("binned", ctypes.c_uint32), ("region_log2", ctypes.c_uint32),
                ("regions", ctypes.c_uint32), ("superbins", ctypes.c_uint32), ("groups", ctypes.c_uint32),
                ("tiles_per_block", ctypes.c_uint32), ("front", ctypes.c_uint32), ("scan", ctypes.c_uint32),
                ("density", ctypes.c_uint32), ("apply", ctypes.c_uint32), ("apply_loads", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32

# name -> (restype, argtypes); must list every function declared in include/bfhip.h
SIGNATURES = {
    "bf_create": (ctypes.c_int, [_u64, _u32, ctypes.POINTER(bf_config), ctypes.POINTER(_vp)]),
    "bf_destroy": (ctypes.c_int, [_vp]),
    "bf_last_error": (ctypes.c_char_p, [_vp]),
    "bf_version": (ctypes.c_char_p, []),
    "bf_info": (ctypes.c_int, [_vp, _u64p, _u32p, _u64p, _u64p]),
    "bf_insert_many": (ctypes.c_int, [_vp, _vp, _vp, _u64, _u8p, _vp]),
    "bf_include_many": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "bf_indexes_many": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "bf_indexes": (ctypes.c_int, [_vp, _u64, _u64, _u32, _vp]),
    "bf_check_offsets": (ctypes.c_int, [_vp, _u64, _u64p]),
    "bf_clear": (ctypes.c_int, [_vp]),
    "bf_export_redis": (ctypes.c_int, [_vp, _vp, _u64, _u64p]),
    "bf_import_redis": (ctypes.c_int, [_vp, _vp, _u64, _u32]),
    "bf_insert_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "bf_include_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_indexes_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_device_bits": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), _u64p]),
    "bf_hash_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_insert_digests_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "bf_include_digests_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "bf_include_hash_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_region_sets_capacity": (ctypes.c_int, [_vp, _u64, _u64p]),
    "bf_encode_region_sets_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "bf_encode_region_sets_digests_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "bf_insert_region_sets_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp]),
    "bf_insert_encode_region_sets_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _vp, _u64,
                                                        _vp]),
    "bf_insert_plan": (ctypes.c_int, [_vp, _u64, _u32p, _u64p]),
    "bf_binned_plan_detail": (ctypes.c_int, [_u64, _u32, _u64, _u32, _u32, ctypes.POINTER(bf_plan_detail)]),
    "bf_insert_plan_detail": (ctypes.c_int, [_vp, _u64, ctypes.POINTER(bf_plan_detail)]),
    "bf_seq_plan": (ctypes.c_int, [_u64, _u32, _u64, _u32p, _u64p, _u64p]),
    "bf_seq_plan_chunk": (ctypes.c_int, [_u32, _u64p]),
    "bf_track_dirty": (ctypes.c_int, [_vp, _u32]),
    "bf_dirty_ranges": (ctypes.c_int, [_vp, _u64p, _u32, _u32p, _u64p, _u32]),
    "bf_export_range": (ctypes.c_int, [_vp, _u64, _u64, _vp]),
    "bf_insert_many_changes": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _u64p]),
    "bf_bitcount": (ctypes.c_int, [_vp, _u64, _u64, _u64p]),
    "bf_bitcount_dev": (ctypes.c_int, [_vp, _u64, _u64, _vp, _vp]),
    "bf_bitop": (ctypes.c_int, [_vp, _u32, _vp, _u8p, _u64p]),
    "bf_bitop_dev": (ctypes.c_int, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "bf_bitcount_op": (ctypes.c_int, [_vp, _u32, _vp, _u64p]),
    "bf_estimate_count": (ctypes.c_int, [_u64, _u32, _u32, _u64, ctypes.POINTER(ctypes.c_double)]),
    "bf_profile": (ctypes.c_int, [_vp, _u32]),
    "bf_profile_read": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u32, _u32p, _u32]),
    "bf_sync": (ctypes.c_int, [_vp]),
    "bf_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "bf_shard_info": (ctypes.c_int, [_vp, _u32p, _u32p, _u32p, _u64p]),
    "bf_route_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "bf_shard_insert_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "bf_shard_test_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "bf_combine_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_route_window_split": (ctypes.c_int, [_vp, _u32p]),
    "bf_route_windows_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "bf_shard_insert_hi_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "bf_shard_insert_windows_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u32, _u32, _vp, _vp]),
    "bf_shard_test_windows_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u32, _u32, _vp, _vp]),
    "bf_shard_test_hi_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "bf_combine_windows_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _vp]),
    "bf_pack_segments_dev": (ctypes.c_int, [_vp, _vp, _vp, _u32, _u64, _vp, _vp]),
    "bf_combine_windows_packed_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _vp]),
    "bf_route_chunk_info": (ctypes.c_int, [_vp, _u64, _u64p, _u64p, _u32p]),
    "bf_route_chunks_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp]),
    "bf_shard_insert_chunks_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _u32, _vp, _vp]),
    "bf_shard_test_chunks_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _u32, _vp, _vp]),
    "bf_shard_test_chunks_packed_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _u32, _vp, _vp]),
    "bf_shard_insert_test_chunks_packed_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _u64,
                                                              _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_route_chunks_digests_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp]),
    "bf_shard_test_chunks_hash_dev": (ctypes.c_int, [_vp, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _u32, _vp,
                                                     _vp, _vp, _u64, _vp, _vp]),
    "bf_combine_chunks_packed_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp]),
    "bf_shard_export": (ctypes.c_int, [_vp, _vp, _u64, _u64p]),
    "bf_shard_import": (ctypes.c_int, [_vp, _vp, _u64, _u32]),
    "bf_lua_create": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.POINTER(bf_config),
                                     ctypes.POINTER(_vp)]),
    "bf_lua_destroy": (ctypes.c_int, [_vp]),
    "bf_lua_last_error": (ctypes.c_char_p, [_vp]),
    "bf_lua_insert_many": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64p]),
    "bf_lua_insert_many_changes": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64p, _vp, _u64, _u64p]),
    "bf_lua_include_many": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "bf_lua_insert_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64p, _vp]),
    "bf_lua_include_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_lua_profile": (ctypes.c_int, [_vp, _u32]),
    "bf_lua_profile_read": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u32, _u32p, _u32]),
    "bf_lua_clear": (ctypes.c_int, [_vp]),
    "bf_lua_get_count": (ctypes.c_int, [_vp, _u64p]),
    "bf_lua_set_count": (ctypes.c_int, [_vp, _u64]),
    "bf_lua_layers": (ctypes.c_int, [_vp, _u32p]),
    "bf_lua_export_layer": (ctypes.c_int, [_vp, _u32, _vp, _u64, _u64p]),
    "bf_lua_import_layer": (ctypes.c_int, [_vp, _u32, _vp, _u64]),
    "bf_lua_layer_params": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, _u32, _u64p, _u32p]),
    "bf_lua_index": (ctypes.c_int, [ctypes.c_double, _u64, _u32p]),
    "bf_bank_create": (ctypes.c_int, [_u64, _u32, _u64, ctypes.POINTER(bf_config), ctypes.POINTER(_vp)]),
    "bf_bank_destroy": (ctypes.c_int, [_vp]),
    "bf_bank_last_error": (ctypes.c_char_p, [_vp]),
    "bf_bank_info": (ctypes.c_int, [_vp, _u64p, _u32p, _u64p, _u64p, _u64p]),
    "bf_bank_stride": (ctypes.c_int, [_u64, _u64p]),
    "bf_bank_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "bf_bank_sync": (ctypes.c_int, [_vp]),
    "bf_bank_insert_many": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bf_bank_insert_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_bank_insert_many_seq": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bf_bank_insert_many_seq_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_bank_insert_many_changes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _u64p]),
    "bf_bank_insert_many_changes_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_bank_set_seq_form": (ctypes.c_int, [_vp, _u32]),
    "bf_bank_seq_plan": (ctypes.c_int, [_vp, _u64, _u32p, _u64p, _u64p]),
    "bf_bank_include_many": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bf_bank_include_many_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_bank_across_row_bytes": (ctypes.c_int, [_u64, _u64p]),
    "bf_bank_include_across": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "bf_bank_include_across_dev": (ctypes.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "bf_bank_clear": (ctypes.c_int, [_vp, _vp, _u64]),
    "bf_bank_clear_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp]),
    "bf_bank_bitcount": (ctypes.c_int, [_vp, _vp, _u64, _vp]),
    "bf_bank_bitcount_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "bf_bank_export_filters": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "bf_bank_import_filters": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _u32]),
    "bf_bank_fold": (ctypes.c_int, [_vp, _u32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bf_bank_fold_dev": (ctypes.c_int, [_vp, _u32, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "bf_bank_overlap": (ctypes.c_int, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "bf_bank_overlap_dev": (ctypes.c_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "bf_optimal_m": (ctypes.c_int64, [ctypes.c_double, ctypes.c_double]),
    "bf_optimal_k": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
}

_lib = None
_lib_lock = threading.Lock()


def lib_path() -> str:
    return os.environ.get("BFHIP_LIB", DEFAULT_LIB)


def _share_torch_runtime() -> None:
    """Make libbfhip bind to the HIP runtime PyTorch-ROCm already uses.

    torch ships its own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``) and
    links it by the unversioned name.  If libbfhip is loaded first, the system
    runtime comes in under that SONAME and torch later maps a SECOND runtime,
    after which torch sees no GPU.  Loading torch first lets the dynamic
    loader satisfy libbfhip's ``libamdhip64.so.7`` with torch's copy: one
    runtime, shared streams and device pointers.  BFHIP_STANDALONE=1 skips this
    (e.g. a process that never imports torch).
    """
    if os.environ.get("BFHIP_STANDALONE") == "1" or "torch" in sys.modules:
        return
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load() -> ctypes.CDLL:
    """Load libbfhip.so once; raise BfHipUnavailable if it cannot be loaded."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        _share_torch_runtime()
        path = lib_path()
        if not os.path.exists(path):
            raise BfHipUnavailable(
                "libbfhip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C redis-bloomfilter_amd/csrc`)" % path)
        try:
            lib = ctypes.CDLL(path)
        except OSError as e:  # missing HIP runtime etc.
            raise BfHipUnavailable("cannot load %s: %s" % (path, e)) from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def version() -> str:
    return load().bf_version().decode()


BF_OPTIMAL_M_INVALID = -(1 << 63)


def optimal_m(n, error_rate) -> int:
    m = int(load().bf_optimal_m(float(n), float(error_rate)))
    if m == BF_OPTIMAL_M_INVALID:   # Infinity/NaN: Float#round raises FloatDomainError in Ruby
        raise FloatingPointError("FloatDomainError: optimal_m(%r, %r) is not finite" % (n, error_rate))
    return m


def optimal_k(n: int, m: int) -> int:
    return int(load().bf_optimal_k(int(n), int(m)))


def estimate_count(m: int, k: int, set_bits: int, flags: int = 0) -> float:
    """Distinct keys behind ``set_bits`` set bits of a filter of m bits and k hashes
    (bf_estimate_count): the expected-count model of the ruby derivation's probe law
    (ruby.rb:51), or the textbook -(m/k) ln(1 - X/m) with a BF_FLAG_ENGINE_* flag.  Host-only.
    ``inf`` for a full filter; ArgumentError when set_bits > m."""
    if not 0 <= int(set_bits) < 1 << 64 or not 0 < int(m) < 1 << 64:
        raise ArgumentError("estimate_count: m and set_bits must be unsigned 64-bit (m > 0)")
    out = ctypes.c_double()
    rc = load().bf_estimate_count(int(m), int(k), int(flags), int(set_bits), ctypes.byref(out))
    if rc:
        raise ArgumentError("bf_estimate_count(m=%r, k=%r, set_bits=%r): set_bits must be <= m and k in [1, %d]"
                            % (m, k, set_bits, BF_MAX_K))
    return float(out.value)


_OPS = {"and": BF_BITOP_AND, "or": BF_BITOP_OR, "xor": BF_BITOP_XOR}
_U64_MAX = (1 << 64) - 1


def _op(op) -> int:
    """BF_BITOP_* from the constant or its name ('and' / 'or' / 'xor', any case)."""
    if isinstance(op, str):
        if op.lower() not in _OPS:
            raise ArgumentError("op must be 'and', 'or' or 'xor', got %r" % (op,))
        return _OPS[op.lower()]
    return int(op)


def indexes(key: bytes, m: int, k: int) -> List[int]:
    """One key's k offsets (Ruby#indexes_for, ruby.rb:41-55) through bf_indexes: the device
    kernel on the current GPU, no filter needed."""
    buf = np.frombuffer(bytes(key), np.uint8) if len(key) else np.zeros(1, np.uint8)
    out = np.zeros(max(int(k), 1), np.uint64)
    _check(load().bf_indexes(_ptr(buf), len(key), int(m), int(k), _ptr(out)))
    return [int(x) for x in out[: int(k)]]


def device_bytes_for(m_bits: int, k: int) -> int:
    """Bytes of the device bitset of a whole (unsharded) filter of m bits and k hashes, as
    bf_info reports them: the reachable prefix min(m, k (2^32 - 1) + 1) in whole bytes, rounded
    up to 256."""
    bits = min(int(m_bits), int(k) * 0xFFFFFFFF + 1)
    return -(-max((bits + 7) // 8, 1) // 256) * 256


def binned_plan_detail(device_bytes: int, k: int, n: int, region_log2_pref: int = 19,
                       compute_units: int = 0) -> dict:
    """Which kernel variants a binned insert of n keys takes on a bitset of device_bytes bytes
    (bf_binned_plan_detail): host-only, no handle, no GPU needed.  compute_units 0: the current
    device's (256 without one).  The fields of bf_plan_detail as a dict of ints; "planned" is 0
    for a shape outside the binned path."""
    d = bf_plan_detail()
    _check(load().bf_binned_plan_detail(int(device_bytes), int(k), int(n), int(region_log2_pref),
                                        int(compute_units), ctypes.byref(d)))
    return d.as_dict()


SEQ_FORMS = ("hash", "direct", "binned")   # BF_SEQ_HASH, BF_SEQ_DIRECT, BF_SEQ_BINNED


def seq_plan(n: int, k: int, m: int) -> dict:
    """How the sequential insert runs one chunk of n keys on a filter or layer of m bits and k
    hashes (bf_seq_plan, bf_seq_plan_chunk): host-only, no handle, no GPU needed.  "form" is
    0 hash / 1 direct / 2 binned (SEQ_FORMS), "slots" the first-index table's entries,
    "scratch_bytes" the chunk's scratch, "chunk_keys" the most keys a chunk of this k holds."""
    form, slots, scratch, chunk = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    for rc in (load().bf_seq_plan(int(n), int(k), int(m), ctypes.byref(form), ctypes.byref(slots),
                                  ctypes.byref(scratch)),
               load().bf_seq_plan_chunk(int(k), ctypes.byref(chunk))):
        if rc:
            raise ArgumentError("bf_seq_plan(%r, %r, %r) failed" % (n, k, m))
    return {"form": int(form.value), "slots": int(slots.value), "scratch_bytes": int(scratch.value),
            "chunk_keys": int(chunk.value)}


def check_offsets(offsets: np.ndarray) -> None:
    """The key-offset rule every hashing kernel applies (bf_check_offsets): offsets[0..n]
    non-decreasing, every key below 2 GiB.  Raises ArgumentError naming the first bad key.
    Host-only: callers of the *_dev entry points can check their offsets before the upload."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offs.size == 0:
        raise ArgumentError("offsets needs n + 1 entries")
    bad = ctypes.c_uint64()
    _check(load().bf_check_offsets(_ptr(offs), offs.size - 1, ctypes.byref(bad)))


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data


def _check(code: int, h=None, last_error: str = "bf_last_error") -> None:
    """Raise for a non-OK status, with the message of the handle family's ``*_last_error``."""
    if code == BF_OK:
        return
    msg = getattr(load(), last_error)(h).decode(errors="replace")
    if code in (BF_EINVAL, BF_ERANGE):
        raise ArgumentError("%s: %s" % (_STATUS.get(code), msg))
    raise BfHipError(code, msg)


def _keys(keys: np.ndarray, offsets: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """A packed key batch as the C ABI takes it: (uint8 keys, uint64 offsets, n)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offsets.ndim != 1 or len(offsets) < 1:
        raise ArgumentError("offsets must be a 1-D array of n+1 entries")
    n = len(offsets) - 1
    if n and int(offsets[-1]) > len(keys):
        raise ArgumentError("offsets point past the key buffer")
    if len(keys) == 0:
        keys = np.zeros(1, np.uint8)
    return keys, offsets, n


class _Handle:
    """What FilterBank and LuaFilter share: the lifecycle of ``self._h`` and the stream argument
    of the ``*_dev`` methods.  A subclass names its C functions.  (Filter keeps its own copy.)"""

    _DESTROY = ""        # e.g. "bf_destroy"
    _LAST_ERROR = ""     # e.g. "bf_last_error"
    _STREAM = None       # e.g. "bf_stream"; None: the handle type has no own-stream getter
    _CLOSED = "filter is closed"

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(self._lib, self._DESTROY)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h:
            raise ArgumentError(self._CLOSED)
        return self._h

    def _s(self, stream):
        """A ``stream`` argument as the C ABI takes it: None is the handle's own stream (where
        the handle type has one), 0 HIP's null stream."""
        if stream is None and self._STREAM:
            if getattr(self, "_own_stream", None) is None:
                p = _vp()
                _check(getattr(self._lib, self._STREAM)(self.handle, ctypes.byref(p)), self._h, self._LAST_ERROR)
                self._own_stream = p.value or 0
            return self._own_stream or None
        return int(stream) or None


class Filter:
    """One device-resident filter (a `bf_handle*`).

    Arrays are numpy: ``keys`` uint8, ``offsets`` uint64 with n+1 entries.
    The ``*_dev`` methods take raw device addresses (ints), e.g. from
    ``torch.Tensor.data_ptr()``, and a hipStream_t as an int (``stream=None``:
    the filter's own stream; ``0`` is HIP's null stream, e.g. torch's default).
    """

    _keys = staticmethod(_keys)   # (kept: the module-level helper under its old name)

    def __init__(self, m_bits: int, k: int, device: int = -1, batch_keys: int = 0,
                 batch_bytes: int = 0, shard_count: int = 1, shard_index: int = 0,
                 shard_block_log2: int = 0, flags: int = 0, devices=None, mode: str = "replicated"):
        """devices: a list of HIP ordinals -> one multi-device handle over them (bf_config
        device_count / devices / mode; ``mode`` "replicated" or "partitioned")."""
        self._lib = load()
        cfg = bf_config(ctypes.sizeof(bf_config), int(device), int(batch_keys), int(batch_bytes),
                        int(shard_count), int(shard_index), int(shard_block_log2), int(flags))
        if devices is not None:
            devices = [int(d) for d in devices]
            if not 0 < len(devices) <= BF_MAX_DEVICES:
                raise ArgumentError("devices must list 1..%d ordinals" % BF_MAX_DEVICES)
            if mode not in ("replicated", "partitioned"):
                raise ArgumentError("mode must be 'replicated' or 'partitioned'")
            cfg.device_count = len(devices)
            cfg.mode = BF_MODE_PARTITIONED if mode == "partitioned" else BF_MODE_REPLICATED
            for i, d in enumerate(devices):
                cfg.devices[i] = d
        self.devices = devices
        self.mode = mode if devices is not None else None
        self.route32 = bool(flags & BF_FLAG_ROUTE32)
        h = _vp()
        rc = self._lib.bf_create(int(m_bits), int(k), ctypes.byref(cfg), ctypes.byref(h))
        _check(rc, None)
        self._h = h
        m = ctypes.c_uint64()
        kk = ctypes.c_uint32()
        reach = ctypes.c_uint64()
        devb = ctypes.c_uint64()
        _check(self._lib.bf_info(h, ctypes.byref(m), ctypes.byref(kk), ctypes.byref(reach),
                                 ctypes.byref(devb)), h)
        self.m, self.k, self.reach_bits, self.device_bytes = m.value, kk.value, reach.value, devb.value
        self.device = int(device)
        sc, si, bl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        lb = ctypes.c_uint64()
        _check(self._lib.bf_shard_info(h, ctypes.byref(sc), ctypes.byref(si), ctypes.byref(bl),
                                       ctypes.byref(lb)), h)
        self.shard_count, self.shard_index, self.block_log2, self.local_bits = sc.value, si.value, bl.value, lb.value

    # -- lifecycle
    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.bf_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h:
            raise ArgumentError("filter is closed")
        return self._h

    # -- host-pointer batch API
    def insert_many(self, keys: np.ndarray, offsets: np.ndarray, any_new: bool = False,
                    per_key_new: bool = False):
        keys, offsets, n = self._keys(keys, offsets)
        flag = ctypes.c_uint8(0)
        pk = np.zeros(max(n, 1), np.uint8) if per_key_new else None
        _check(self._lib.bf_insert_many(self.handle, _ptr(keys), _ptr(offsets), n,
                                        ctypes.byref(flag) if any_new else None, _ptr(pk)), self._h)
        return (bool(flag.value) if any_new else None), (pk[:n] if per_key_new else None)

    # bf_insert_many_changes limits (include/bfhip.h)
    CHANGES_MAX_PROBES = 4096
    CHANGES_MAX_BYTES = 64 << 10

    def insert_many_changes(self, keys: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """Insert a small batch; returns the bit offsets it flipped 0 -> 1 (each once, uint64):
        the SETBITs that bring a Redis copy up to date (ruby.rb:57-63)."""
        keys, offsets, n = self._keys(keys, offsets)
        out = np.zeros(max(n * self.k, 1), np.uint64)
        cnt = ctypes.c_uint64(0)
        _check(self._lib.bf_insert_many_changes(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(out), len(out),
                                                ctypes.byref(cnt)), self._h)
        return out[: cnt.value]

    def include_many(self, keys: np.ndarray, offsets: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """include? of every key -> uint8 answers (1/0).  out: an optional caller-owned uint8
        buffer of >= n entries (reused across calls, its pages are already mapped)."""
        keys, offsets, n = self._keys(keys, offsets)
        if out is None:
            out = np.empty(max(n, 1), np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.ndim != 1 or len(out) < max(n, 1):
            raise ArgumentError("out must be a contiguous 1-D uint8 array of at least n entries")
        _check(self._lib.bf_include_many(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(out)), self._h)
        return out[:n]

    def indexes_many(self, keys: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        keys, offsets, n = self._keys(keys, offsets)
        out = np.zeros(max(n * self.k, 1), np.uint64)
        _check(self._lib.bf_indexes_many(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(out)), self._h)
        return out[: n * self.k].reshape(n, self.k)

    def clear(self) -> None:
        _check(self._lib.bf_clear(self.handle), self._h)

    def sync(self) -> None:
        _check(self._lib.bf_sync(self.handle), self._h)

    # -- Redis string
    def export_redis(self) -> bytes:
        n = ctypes.c_uint64(0)
        _check(self._lib.bf_export_redis(self.handle, None, 0, ctypes.byref(n)), self._h)
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(self._lib.bf_export_redis(self.handle, _ptr(buf), len(buf), ctypes.byref(n)), self._h)
        return buf[: n.value].tobytes()

    def redis_len(self) -> int:
        n = ctypes.c_uint64(0)
        _check(self._lib.bf_export_redis(self.handle, None, 0, ctypes.byref(n)), self._h)
        return n.value

    def import_redis(self, data: bytes, mode: int = BF_IMPORT_REPLACE) -> None:
        buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
        _check(self._lib.bf_import_redis(self.handle, _ptr(buf), len(data), int(mode)), self._h)

    # -- incremental Redis sync
    def track_dirty(self, enable: bool = True) -> None:
        """Record which BF_DIRTY_BLOCK_BYTES blocks of the Redis string inserts change."""
        _check(self._lib.bf_track_dirty(self.handle, 1 if enable else 0), self._h)

    def dirty_ranges(self, clear: bool = True) -> Tuple[List[Tuple[int, int]], int]:
        """([(byte offset, length), ...], Redis string length) changed since the last clear."""
        n, rl = ctypes.c_uint32(), ctypes.c_uint64()
        _check(self._lib.bf_dirty_ranges(self.handle, None, 0, ctypes.byref(n), ctypes.byref(rl), 0), self._h)
        while True:
            cap = max(n.value, 1)
            buf = np.zeros(2 * cap, np.uint64)
            rc = self._lib.bf_dirty_ranges(self.handle, buf.ctypes.data_as(_u64p), cap, ctypes.byref(n),
                                           ctypes.byref(rl), 1 if clear else 0)
            if rc == BF_ERANGE and n.value > cap:   # an insert on another thread grew the set
                continue
            _check(rc, self._h)
            pairs = buf[: 2 * n.value].reshape(-1, 2)
            return [(int(o), int(l)) for o, l in pairs], int(rl.value)

    def export_range(self, offset: int, length: int) -> bytes:
        buf = np.zeros(max(int(length), 1), np.uint8)
        _check(self._lib.bf_export_range(self.handle, int(offset), int(length), _ptr(buf)), self._h)
        return buf[: int(length)].tobytes()

    # -- statistics and filter-to-filter combines (Redis BITCOUNT / BITOP on the device string)
    def bitcount_bytes(self, byte_start: int = 0, byte_len: int = _U64_MAX) -> int:
        """Set bits of bytes [byte_start, byte_start + byte_len) (bf_bitcount: clamped to the
        bitset; the default counts everything; a shard handle counts its local bytes)."""
        n = ctypes.c_uint64()
        _check(self._lib.bf_bitcount(self.handle, int(byte_start), min(int(byte_len), _U64_MAX), ctypes.byref(n)),
               self._h)
        return int(n.value)

    def bitcount(self, start: int = 0, end: int = -1) -> int:
        """Redis ``BITCOUNT key start end``: inclusive byte indices, negative ones counting from
        the end of the trimmed string (only those cost a ``redis_len()``; ``end=-1`` alone does
        not, the bytes past the string are zero)."""
        start, end = int(start), int(end)
        if start >= 0 and end == -1:
            return self.bitcount_bytes(start)
        if start < 0 or end < 0:
            n = self.redis_len()
            if start < 0 and end < 0 and start > end:
                return 0
            start = max(start + n, 0) if start < 0 else start
            end = max(end + n, 0) if end < 0 else end
            end = min(end, n - 1)
        if start > end:
            return 0
        return self.bitcount_bytes(start, end - start + 1)

    def bitcount_dev(self, d_set_bits: int, byte_start: int = 0, byte_len: int = _U64_MAX, stream=None) -> None:
        """bitcount_bytes on ``stream`` without a sync; the uint64 at d_set_bits is written."""
        _check(self._lib.bf_bitcount_dev(self.handle, int(byte_start), min(int(byte_len), _U64_MAX), d_set_bits,
                                         self._s(stream)), self._h)

    def bitop(self, op, other: "Filter") -> Tuple[bool, int]:
        """self = self OP other ('and' / 'or'), both on one device with the same geometry
        (bf_bitop) -> (changed, set bits of the result).  With dirty tracking on, exactly the
        blocks that changed are marked."""
        ch, n = ctypes.c_uint8(0), ctypes.c_uint64()
        _check(self._lib.bf_bitop(self.handle, _op(op), other.handle, ctypes.byref(ch), ctypes.byref(n)), self._h)
        return bool(ch.value), int(n.value)

    def bitop_dev(self, op, other: "Filter", d_changed: int = 0, d_set_bits: int = 0, stream=None) -> None:
        """bitop on ``stream`` without a sync: 1 is ORed into the uint32 at d_changed when a bit
        changed, the uint64 at d_set_bits is written (both optional)."""
        _check(self._lib.bf_bitop_dev(self.handle, _op(op), other.handle, d_changed or None, d_set_bits or None,
                                      self._s(stream)), self._h)

    def bitcount_op(self, op, other: "Filter") -> int:
        """Set bits of (self OP other), 'and' / 'or' / 'xor' (the Hamming distance), with
        neither filter modified (bf_bitcount_op)."""
        n = ctypes.c_uint64()
        _check(self._lib.bf_bitcount_op(self.handle, _op(op), other.handle, ctypes.byref(n)), self._h)
        return int(n.value)

    # -- device-resident API
    def insert_many_dev(self, d_keys: int, d_offsets: int, n: int, d_any_new: int = 0,
                        d_per_key_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_insert_many_dev(self.handle, d_keys, d_offsets, int(n), d_any_new or None,
                                            d_per_key_new or None, self._s(stream)), self._h)

    def include_many_dev(self, d_keys: int, d_offsets: int, n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_include_many_dev(self.handle, d_keys, d_offsets, int(n), d_out,
                                             self._s(stream)), self._h)

    def indexes_many_dev(self, d_keys: int, d_offsets: int, n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_indexes_many_dev(self.handle, d_keys, d_offsets, int(n), d_out,
                                             self._s(stream)), self._h)

    # -- SHA-1 words as an intermediate (digests: 4 uint32 per key, 16-byte aligned)
    def hash_many_dev(self, d_keys: int, d_offsets: int, n: int, d_digests: int, stream=None) -> None:
        _check(self._lib.bf_hash_many_dev(self.handle, d_keys, d_offsets, int(n), d_digests, self._s(stream)),
               self._h)

    def insert_digests_dev(self, d_digests: int, n: int, d_any_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_insert_digests_dev(self.handle, d_digests, int(n), d_any_new or None, None,
                                               self._s(stream)), self._h)

    def include_digests_dev(self, d_digests: int, n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_include_digests_dev(self.handle, d_digests, int(n), d_out, self._s(stream)), self._h)

    def include_hash_dev(self, d_keys: int, d_offsets: int, n: int, d_out: int, d_next_keys: int,
                         d_next_offsets: int, n_next: int, d_next_digests: int, stream=None) -> None:
        _check(self._lib.bf_include_hash_dev(self.handle, d_keys, d_offsets, int(n), d_out, d_next_keys or None,
                                             d_next_offsets or None, int(n_next), d_next_digests or None,
                                             self._s(stream)), self._h)

    # -- replicated inserts from region sets (include/bfhip.h): encode once per rank, OR in everywhere
    def region_sets_capacity(self, n: int) -> int:
        """Bytes a region-set buffer needs for any batch of <= n keys (the same on every
        handle of this m and k)."""
        b = ctypes.c_uint64()
        _check(self._lib.bf_region_sets_capacity(self.handle, int(n), ctypes.byref(b)), self._h)
        return int(b.value)

    def encode_region_sets_dev(self, d_keys: int, d_offsets: int, n: int, d_sets: int, sets_bytes: int,
                               stream=None) -> None:
        _check(self._lib.bf_encode_region_sets_dev(self.handle, d_keys or None, d_offsets or None, int(n), d_sets,
                                                   int(sets_bytes), self._s(stream)), self._h)

    def encode_region_sets_digests_dev(self, d_digests: int, n: int, d_sets: int, sets_bytes: int,
                                       stream=None) -> None:
        _check(self._lib.bf_encode_region_sets_digests_dev(self.handle, d_digests or None, int(n), d_sets,
                                                           int(sets_bytes), self._s(stream)), self._h)

    def insert_region_sets_dev(self, d_sets: int, stride_bytes: int, nsrc: int, probes_hint: int,
                               d_any_new: int = 0, d_status: int = 0, stream=None) -> None:
        _check(self._lib.bf_insert_region_sets_dev(self.handle, d_sets, int(stride_bytes), int(nsrc),
                                                   int(probes_hint), d_any_new or None, d_status or None,
                                                   self._s(stream)), self._h)

    def insert_encode_region_sets_dev(self, d_sets: int, stride_bytes: int, nsrc: int, probes_hint: int,
                                      d_next_digests: int, n_next: int, d_next_sets: int, next_sets_bytes: int,
                                      d_any_new: int = 0, d_status: int = 0, stream=None) -> None:
        """insert_region_sets_dev of nsrc buffers and encode_region_sets_digests_dev of the next
        batch's words into d_next_sets, in one pass over the regions
        (bf_insert_encode_region_sets_dev)."""
        _check(self._lib.bf_insert_encode_region_sets_dev(self.handle, d_sets or None, int(stride_bytes), int(nsrc),
                                                          int(probes_hint), d_any_new or None, d_status or None,
                                                          d_next_digests or None, int(n_next), d_next_sets,
                                                          int(next_sets_bytes), self._s(stream)), self._h)

    def _s(self, stream):
        if stream is None:
            if getattr(self, "_own_stream", None) is None:
                p = _vp()
                _check(self._lib.bf_stream(self.handle, ctypes.byref(p)), self._h)
                self._own_stream = p.value or 0
            return self._own_stream or None
        return int(stream) or None

    def insert_plan(self, n: int) -> dict:
        """How an insert of n keys runs: {"binned": bool, "scratch_bytes": int} (bf_insert_plan)."""
        b, sb = ctypes.c_uint32(), ctypes.c_uint64()
        _check(self._lib.bf_insert_plan(self.handle, int(n), ctypes.byref(b), ctypes.byref(sb)), self._h)
        return {"binned": bool(b.value), "scratch_bytes": int(sb.value)}

    def insert_plan_detail(self, n: int) -> dict:
        """Which kernel variants one insert_many_dev of n keys takes (bf_insert_plan_detail):
        the fields of bf_plan_detail as a dict of ints."""
        d = bf_plan_detail()
        _check(self._lib.bf_insert_plan_detail(self.handle, int(n), ctypes.byref(d)), self._h)
        return d.as_dict()

    def profile(self, enable: bool) -> None:
        """Per-kernel HIP-event timing of every keyed launch (bf_profile)."""
        _check(self._lib.bf_profile(self.handle, 1 if enable else 0), self._h)

    def profile_read(self, reset: bool = True) -> dict:
        """{kernel name: (total ms, launches)} since the last reset (bf_profile_read)."""
        cap = 32
        names = ctypes.create_string_buffer(cap * PROFILE_NAME_LEN)
        ms = np.zeros(cap, np.float64)
        cnt = np.zeros(cap, np.uint64)
        n = ctypes.c_uint32()
        _check(self._lib.bf_profile_read(self.handle, names, _ptr(ms), _ptr(cnt), cap, ctypes.byref(n),
                                         1 if reset else 0), self._h)
        out = {}
        for i in range(min(n.value, cap)):
            raw = names.raw[i * PROFILE_NAME_LEN:(i + 1) * PROFILE_NAME_LEN]
            out[raw.split(b"\0", 1)[0].decode()] = (float(ms[i]), int(cnt[i]))
        return out

    def device_bits(self) -> Tuple[int, int]:
        p = _vp()
        nb = ctypes.c_uint64()
        _check(self._lib.bf_device_bits(self.handle, ctypes.byref(p), ctypes.byref(nb)), self._h)
        return int(p.value or 0), int(nb.value)

    # -- partitioned filters (see include/bfhip.h)
    def route_dev(self, d_keys: int, d_offsets: int, n: int, d_send: int, d_slot: int, d_counts: int,
                  stream=None) -> None:
        _check(self._lib.bf_route_dev(self.handle, d_keys, d_offsets, int(n), d_send, d_slot or None, d_counts,
                                      self._s(stream)), self._h)

    def route_windows_dev(self, d_keys: int, d_offsets: int, n: int, d_send: int, d_slot: int, window_cap: int,
                          d_counts: int, stream=None) -> None:
        _check(self._lib.bf_route_windows_dev(self.handle, d_keys, d_offsets, int(n), d_send, d_slot or None,
                                              int(window_cap), d_counts, self._s(stream)), self._h)

    def route_window_split(self) -> int:
        nh = ctypes.c_uint32()
        _check(self._lib.bf_route_window_split(self.handle, ctypes.byref(nh)), self._h)
        return int(nh.value)

    # -- chunked windows (the owner skips its sort pass; include/bfhip.h)
    def route_chunk_info(self, n_bound: int):
        """(tiles, dir_bytes, superbins per window) for batches of <= n_bound keys, or None
        when this shard count cannot take chunked windows."""
        t, d, sb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        if self._lib.bf_route_chunk_info(self.handle, int(n_bound), ctypes.byref(t), ctypes.byref(d),
                                         ctypes.byref(sb)) != 0:
            return None
        return int(t.value), int(d.value), int(sb.value)

    def route_chunks_dev(self, d_keys: int, d_offsets: int, n: int, d_send: int, d_slot16: int, window_cap: int,
                         d_counts: int, d_dir: int, dir_bytes: int, tiles: int, stream=None) -> None:
        _check(self._lib.bf_route_chunks_dev(self.handle, d_keys, d_offsets, int(n), d_send, d_slot16 or None,
                                             int(window_cap), d_counts, d_dir, int(dir_bytes), int(tiles),
                                             self._s(stream)), self._h)

    def route_chunks_digests_dev(self, d_digests: int, n: int, d_send: int, d_slot16: int, window_cap: int,
                                 d_counts: int, d_dir: int, dir_bytes: int, tiles: int, stream=None) -> None:
        """route_chunks_dev from the keys' SHA-1 words (hash_many_dev's output)."""
        _check(self._lib.bf_route_chunks_digests_dev(self.handle, d_digests, int(n), d_send, d_slot16 or None,
                                                     int(window_cap), d_counts, d_dir, int(dir_bytes), int(tiles),
                                                     self._s(stream)), self._h)

    def shard_insert_chunks_dev(self, d_recv: int, window_cap: int, nsrc: int, d_dir: int, dir_bytes: int, tiles: int,
                                d_counts: int, count_stride: int, d_any_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_shard_insert_chunks_dev(self.handle, d_recv, int(window_cap), int(nsrc), d_dir,
                                                    int(dir_bytes), int(tiles), d_counts, int(count_stride),
                                                    d_any_new or None, self._s(stream)), self._h)

    def shard_test_chunks_dev(self, d_recv: int, window_cap: int, nsrc: int, d_dir: int, dir_bytes: int, tiles: int,
                              d_counts: int, count_stride: int, d_bits: int, stream=None) -> None:
        _check(self._lib.bf_shard_test_chunks_dev(self.handle, d_recv, int(window_cap), int(nsrc), d_dir,
                                                  int(dir_bytes), int(tiles), d_counts, int(count_stride), d_bits,
                                                  self._s(stream)), self._h)

    def shard_test_chunks_packed_dev(self, d_recv: int, window_cap: int, nsrc: int, d_dir: int, dir_bytes: int,
                                     tiles: int, d_counts: int, count_stride: int, d_packed: int, stream=None) -> None:
        """The owner test with its answers as packed bits in the return trip's layout (window
        (hi, src) at d_packed + (src * nh + hi) * ceil(window_cap / 8))."""
        _check(self._lib.bf_shard_test_chunks_packed_dev(self.handle, d_recv, int(window_cap), int(nsrc), d_dir,
                                                         int(dir_bytes), int(tiles), d_counts, int(count_stride),
                                                         d_packed, self._s(stream)), self._h)

    def shard_insert_test_chunks_packed_dev(self, d_ins_recv: int, d_ins_dir: int, d_ins_counts: int,
                                            d_tst_recv: int, d_tst_dir: int, d_tst_counts: int, window_cap: int,
                                            nsrc: int, dir_bytes: int, tiles: int, count_stride: int,
                                            d_packed: int, d_any_new: int = 0, d_next_keys: int = 0,
                                            d_next_offsets: int = 0, n_next: int = 0, d_next_digests: int = 0,
                                            stream=None) -> None:
        """One step's owner work: the insert windows ORed in, then the include? windows tested
        (packed answers as shard_test_chunks_packed_dev), in one pass over the shard; with
        n_next, that pass also hashes another key batch into d_next_digests."""
        _check(self._lib.bf_shard_insert_test_chunks_packed_dev(
            self.handle, d_ins_recv, d_ins_dir, d_ins_counts, d_tst_recv, d_tst_dir, d_tst_counts, int(window_cap),
            int(nsrc), int(dir_bytes), int(tiles), int(count_stride), d_any_new or None, d_packed,
            d_next_keys or None, d_next_offsets or None, int(n_next), d_next_digests or None,
            self._s(stream)), self._h)

    def shard_test_chunks_hash_dev(self, d_recv: int, window_cap: int, nsrc: int, d_dir: int, dir_bytes: int,
                                   tiles: int, d_counts: int, count_stride: int, d_bits: int, d_next_keys: int,
                                   d_next_offsets: int, n_next: int, d_next_digests: int, stream=None) -> None:
        """shard_test_chunks_dev that also hashes another key batch (SHA-1 words to d_next_digests)."""
        _check(self._lib.bf_shard_test_chunks_hash_dev(self.handle, d_recv, int(window_cap), int(nsrc), d_dir,
                                                       int(dir_bytes), int(tiles), d_counts, int(count_stride), d_bits,
                                                       d_next_keys or None, d_next_offsets or None, int(n_next),
                                                       d_next_digests or None, self._s(stream)), self._h)

    def combine_chunks_packed_dev(self, d_packed: int, d_slot16: int, window_cap: int, d_dir: int, dir_bytes: int,
                                  tiles: int, d_counts: int, n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_combine_chunks_packed_dev(self.handle, d_packed, d_slot16, int(window_cap), d_dir,
                                                      int(dir_bytes), int(tiles), d_counts, int(n), d_out,
                                                      self._s(stream)), self._h)

    def pack_segments_dev(self, d_bits: int, d_seg: int, nseg: int, max_count: int, d_packed: int,
                          stream=None) -> None:
        _check(self._lib.bf_pack_segments_dev(self.handle, d_bits, d_seg, int(nseg), int(max_count), d_packed,
                                              self._s(stream)), self._h)

    def combine_windows_packed_dev(self, d_packed: int, d_slot: int, window_cap: int, nwin: int, d_counts: int,
                                   n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_combine_windows_packed_dev(self.handle, d_packed, d_slot, int(window_cap), int(nwin),
                                                       d_counts, int(n), d_out, self._s(stream)), self._h)

    def shard_insert_windows_dev(self, d_local32: int, window_cap: int, nwin: int, d_counts: int, count_stride: int,
                                 hi: int, d_any_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_shard_insert_windows_dev(self.handle, d_local32, int(window_cap), int(nwin), d_counts,
                                                     int(count_stride), int(hi), d_any_new or None, self._s(stream)),
               self._h)

    def shard_test_windows_dev(self, d_local32: int, window_cap: int, nwin: int, d_counts: int, count_stride: int,
                               hi: int, d_bits: int, stream=None) -> None:
        _check(self._lib.bf_shard_test_windows_dev(self.handle, d_local32, int(window_cap), int(nwin), d_counts,
                                                   int(count_stride), int(hi), d_bits, self._s(stream)), self._h)

    def shard_insert_hi_dev(self, d_local32: int, count: int, hi: int, d_any_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_shard_insert_hi_dev(self.handle, d_local32, int(count), int(hi), d_any_new or None,
                                                self._s(stream)), self._h)

    def shard_test_hi_dev(self, d_local32: int, count: int, hi: int, d_bits: int, stream=None) -> None:
        _check(self._lib.bf_shard_test_hi_dev(self.handle, d_local32, int(count), int(hi), d_bits, self._s(stream)),
               self._h)

    def combine_windows_dev(self, d_bits: int, d_slot: int, window_cap: int, nwin: int, d_counts: int, n: int,
                            d_out: int, stream=None) -> None:
        _check(self._lib.bf_combine_windows_dev(self.handle, d_bits, d_slot, int(window_cap), int(nwin), d_counts,
                                                int(n), d_out, self._s(stream)), self._h)

    def shard_insert_dev(self, d_local: int, count: int, d_any_new: int = 0, stream=None) -> None:
        _check(self._lib.bf_shard_insert_dev(self.handle, d_local, int(count), d_any_new or None,
                                             self._s(stream)), self._h)

    def shard_test_dev(self, d_local: int, count: int, d_bits: int, stream=None) -> None:
        _check(self._lib.bf_shard_test_dev(self.handle, d_local, int(count), d_bits, self._s(stream)), self._h)

    def combine_dev(self, d_bits: int, d_slot: int, n: int, d_out: int, stream=None) -> None:
        _check(self._lib.bf_combine_dev(self.handle, d_bits, d_slot, int(n), d_out, self._s(stream)), self._h)

    def shard_export(self) -> np.ndarray:
        n = ctypes.c_uint64(0)
        _check(self._lib.bf_shard_export(self.handle, None, 0, ctypes.byref(n)), self._h)
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(self._lib.bf_shard_export(self.handle, _ptr(buf), len(buf), ctypes.byref(n)), self._h)
        return buf[: n.value]

    def shard_import(self, data, mode: int = BF_IMPORT_REPLACE) -> None:
        buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
        _check(self._lib.bf_shard_import(self.handle, _ptr(buf), len(buf) if len(data) else 0, int(mode)),
               self._h)


def bank_stride(m_bits: int) -> int:
    """Bytes between two filters of a bank: ceil(m_bits / 8) rounded up to 128 (bf_bank_stride)."""
    out = ctypes.c_uint64()
    if not 0 <= int(m_bits) < 1 << 64 or load().bf_bank_stride(int(m_bits), ctypes.byref(out)):
        raise ArgumentError("bf_bank_stride(%r): m_bits must be positive and its stride fit 64 bits" % (m_bits,))
    return int(out.value)


_bank_check = functools.partial(_check, last_error="bf_bank_last_error")


class FilterBank(_Handle):
    """``n_filters`` device-resident filters of one (m_bits, k) behind one handle (a ``bf_bank*``;
    see include/bfhip.h).  Filter ``f`` is a Redis string in SETBIT order at byte ``f * stride``
    of one allocation; a batch names each key's filter in ``filter_ids`` (uint32).

    Arrays are numpy as for ``Filter``; the ``*_dev`` methods take raw device addresses (ints)
    and a hipStream_t as an int (``stream=None``: the bank's own stream, ``0``: the null stream)
    and do not synchronise.  ``ids=None`` lists every filter in order."""

    _DESTROY, _LAST_ERROR, _STREAM = "bf_bank_destroy", "bf_bank_last_error", "bf_bank_stream"
    _CLOSED = "bank is closed"

    def __init__(self, m_bits: int, k: int, n_filters: int, device: int = -1, batch_keys: int = 0,
                 batch_bytes: int = 0):
        self._lib = load()
        for what, v in (("m_bits", m_bits), ("n_filters", n_filters)):
            if not 0 <= int(v) < 1 << 64:
                raise ArgumentError("%s must be an unsigned 64-bit integer, got %r" % (what, v))
        if not 0 <= int(k) < 1 << 32:
            raise ArgumentError("k must be in [1, %d], got %r" % (BF_MAX_K, k))
        cfg = bf_config(ctypes.sizeof(bf_config), int(device), int(batch_keys), int(batch_bytes), 1, 0, 0, 0)
        h = _vp()
        _bank_check(self._lib.bf_bank_create(int(m_bits), int(k), int(n_filters), ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        m, kk = ctypes.c_uint64(), ctypes.c_uint32()
        nf, st, db = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _bank_check(self._lib.bf_bank_info(h, ctypes.byref(m), ctypes.byref(kk), ctypes.byref(nf), ctypes.byref(st),
                                           ctypes.byref(db)), h)
        self.m, self.k, self.n_filters, self.stride, self.device_bytes = m.value, kk.value, nf.value, st.value, db.value
        self.device = int(device)
        # BFHIP_BANK_SEQ_FORM=hash|direct, read once here: the form of insert_many_seq's table
        # where it is legal.  It never changes a result (the tests run both forms with it).
        form = os.environ.get("BFHIP_BANK_SEQ_FORM")
        if form in self.SEQ_FORMS:
            self.set_seq_form(form)

    SEQ_FORMS = {"auto": 0, "hash": 1, "direct": 2}   # BF_BANK_SEQ_*

    def set_seq_form(self, form: str) -> None:
        """Force the first-index table of ``insert_many_seq*`` (``seq_plan``) to ``'hash'`` or
        ``'direct'`` where that form is legal, or back to the bank's own choice (``'auto'``)."""
        if form not in self.SEQ_FORMS:
            raise ArgumentError("form must be one of %s, got %r" % (sorted(self.SEQ_FORMS), form))
        _bank_check(self._lib.bf_bank_set_seq_form(self.handle, self.SEQ_FORMS[form]), self._h)

    def sync(self) -> None:
        """Wait for the bank's work; ArgumentError (once) when a ``*_dev`` call's kernel skipped
        a key or a listed filter (an id out of range, inconsistent key offsets)."""
        _bank_check(self._lib.bf_bank_sync(self.handle), self._h)

    # -- host-pointer batch API
    @staticmethod
    def _batch(keys, offsets, filter_ids):
        keys, offsets, n = _keys(keys, offsets)
        ids = np.ascontiguousarray(filter_ids)
        if ids.ndim != 1 or len(ids) != n:
            raise ArgumentError("filter_ids must be a 1-D array of n entries")
        if n and (ids.dtype.kind not in "iu" or int(ids.min()) < 0 or int(ids.max()) > 0xFFFFFFFF):
            raise ArgumentError("filter_ids must be unsigned 32-bit integers")
        ids = ids.astype(np.uint32, copy=False) if n else np.zeros(1, np.uint32)
        return keys, offsets, ids, n

    def insert_many(self, keys: np.ndarray, offsets: np.ndarray, filter_ids: np.ndarray,
                    key_flipped: bool = True) -> Optional[np.ndarray]:
        """Key j goes into filter filter_ids[j].  Returns the per-key flags (uint8: this key's own
        atomic flipped a bit; OR them per filter for "this filter's string changed"), or None
        with ``key_flipped=False``."""
        keys, offsets, ids, n = self._batch(keys, offsets, filter_ids)
        kf = np.zeros(max(n, 1), np.uint8) if key_flipped else None
        _bank_check(self._lib.bf_bank_insert_many(self.handle, _ptr(keys), _ptr(offsets), _ptr(ids), n, _ptr(kf)),
                    self._h)
        return kf[:n] if key_flipped else None

    def insert_many_seq(self, keys: np.ndarray, offsets: np.ndarray, filter_ids: np.ndarray) -> np.ndarray:
        """``insert_many`` with the exact sequential flag (first-seen dedup): [j] is 1 iff,
        inserting the pairs (filter_ids[j], key j) one at a time in batch order, key j flipped a
        bit of its filter (ruby.rb:57-63); its complement is include?-before-insert.  The bits
        left behind are ``insert_many``'s."""
        keys, offsets, ids, n = self._batch(keys, offsets, filter_ids)
        new = np.zeros(max(n, 1), np.uint8)
        _bank_check(self._lib.bf_bank_insert_many_seq(self.handle, _ptr(keys), _ptr(offsets), _ptr(ids), n, _ptr(new)),
                    self._h)
        return new[:n]

    def insert_many_changes(self, keys: np.ndarray, offsets: np.ndarray, filter_ids: np.ndarray, seq: bool = False,
                            cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``insert_many`` (``seq=True``: ``insert_many_seq``) that also lists the bits it flipped
        0 -> 1 (bf_bank_insert_many_changes).  Returns ``(flags, ids, bits)``: that insert's per-key
        flags, and the list as two arrays, bit ``bits[e]`` (uint64, the SETBIT offset of ruby.rb:59)
        of filter ``ids[e]`` (uint32); each flipped bit once, in no particular order.  ``cap``
        bounds the list and defaults to n * k, which always suffices; when the batch flips more
        bits than an explicit ``cap`` the insert is still applied and ArgumentError (BF_ERANGE)
        raised."""
        keys, offsets, fids, n = self._batch(keys, offsets, filter_ids)
        cap = n * self.k if cap is None else int(cap)
        if not 0 <= cap < 1 << 64:
            raise ArgumentError("cap must be an unsigned 64-bit integer, got %r" % (cap,))
        flags = np.zeros(max(n, 1), np.uint8)
        ids, bits = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64)
        count = ctypes.c_uint64()
        _bank_check(self._lib.bf_bank_insert_many_changes(self.handle, _ptr(keys), _ptr(offsets), _ptr(fids), n,
                                                          1 if seq else 0, _ptr(flags), _ptr(ids), _ptr(bits), cap,
                                                          ctypes.byref(count)), self._h)
        return flags[:n], ids[:count.value], bits[:count.value]

    def seq_plan(self, n: int) -> Tuple[bool, int, int]:
        """How ``insert_many_seq*`` runs a batch of ``n`` keys, without a launch: (direct: the
        first-index table is one word per bit of the bank, not a hash table; keys per chunk; bytes
        of scratch)."""
        direct, chunk, scratch = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        _bank_check(self._lib.bf_bank_seq_plan(self.handle, int(n), ctypes.byref(direct), ctypes.byref(chunk),
                                               ctypes.byref(scratch)), self._h)
        return bool(direct.value), chunk.value, scratch.value

    def include_many(self, keys: np.ndarray, offsets: np.ndarray, filter_ids: np.ndarray) -> np.ndarray:
        keys, offsets, ids, n = self._batch(keys, offsets, filter_ids)
        out = np.zeros(max(n, 1), np.uint8)
        _bank_check(self._lib.bf_bank_include_many(self.handle, _ptr(keys), _ptr(offsets), _ptr(ids), n, _ptr(out)),
                    self._h)
        return out[:n]

    @staticmethod
    def across_row_bytes(count: int) -> int:
        """Bytes of one mask row of a cross query over ``count`` list entries: 8 * ceil(count / 64)
        (bf_bank_across_row_bytes)."""
        out = ctypes.c_uint64()
        if not 0 <= int(count) < 1 << 64 or load().bf_bank_across_row_bytes(int(count), ctypes.byref(out)):
            raise ArgumentError("bf_bank_across_row_bytes(%r): count must be an unsigned 64-bit integer" % (count,))
        return int(out.value)

    def include_across(self, keys: np.ndarray, offsets: np.ndarray, ids=None) -> np.ndarray:
        """Which of the listed filters hold each key (bf_bank_include_across): a bool array of
        shape (n, count), [j, i] = include? of key j in filter ids[i].  The key is hashed once;
        ids may repeat and come in any order."""
        keys, offsets, n = _keys(keys, offsets)
        a, count = self._ids(ids)
        row = self.across_row_bytes(count)
        mask = np.zeros((max(n, 1), max(row, 1)), np.uint8)
        _bank_check(self._lib.bf_bank_include_across(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(a), count,
                                                     _ptr(mask)), self._h)
        if n == 0 or count == 0:
            return np.zeros((n, count), bool)
        return np.unpackbits(mask[:n, :row], axis=1, count=count, bitorder="little").astype(bool)

    def _ids(self, ids):
        """(uint32 array or None, count) of an id list; None lists every filter."""
        if ids is None:
            return None, self.n_filters
        a = np.ascontiguousarray(ids)
        if a.ndim != 1:
            raise ArgumentError("ids must be a 1-D array")
        if len(a) and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ArgumentError("ids must be unsigned 32-bit integers")
        return (a.astype(np.uint32, copy=False) if len(a) else np.zeros(1, np.uint32)), len(a)

    def clear(self, ids=None) -> None:
        a, count = self._ids(ids)
        _bank_check(self._lib.bf_bank_clear(self.handle, _ptr(a), count), self._h)

    def bitcount(self, ids=None) -> np.ndarray:
        """BITCOUNT of every listed filter (uint64), one launch."""
        a, count = self._ids(ids)
        out = np.zeros(max(count, 1), np.uint64)
        _bank_check(self._lib.bf_bank_bitcount(self.handle, _ptr(a), count, _ptr(out)), self._h)
        return out[:count]

    def export_filters(self, ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """(buf, lens): buf[i] holds the stride bytes of listed filter i (a (count, stride) uint8
        array), lens[i] its trimmed Redis length."""
        a, count = self._ids(ids)
        buf = np.zeros((max(count, 1), self.stride), np.uint8)
        lens = np.zeros(max(count, 1), np.uint64)
        _bank_check(self._lib.bf_bank_export_filters(self.handle, _ptr(a), count, _ptr(buf), _ptr(lens)), self._h)
        return buf[:count], lens[:count]

    def export_redis(self, ids=None) -> List[bytes]:
        """The trimmed Redis string of every listed filter (b"" for an empty one)."""
        buf, lens = self.export_filters(ids)
        return [buf[i, : int(lens[i])].tobytes() for i in range(len(lens))]

    def import_redis(self, ids, strings, mode: int = BF_IMPORT_REPLACE) -> None:
        """Load one Redis string per listed filter (bf_bank_import_filters); ArgumentError and
        nothing imported when one is longer than ceil(m / 8) or sets a bit at or past m."""
        a, count = self._ids(ids)
        strings = list(strings)
        if len(strings) != count:
            raise ArgumentError("%d strings for %d filters" % (len(strings), count))
        lens = np.array([len(s) for s in strings] or [0], np.uint64)
        buf = np.zeros((max(count, 1), self.stride), np.uint8)
        for i, s in enumerate(strings):
            ln = min(len(s), self.stride)   # a longer string is refused by its length
            buf[i, :ln] = np.frombuffer(bytes(s[:ln]), np.uint8)
        _bank_check(self._lib.bf_bank_import_filters(self.handle, _ptr(a), count, _ptr(buf), _ptr(lens), int(mode)),
                    self._h)

    # -- filters combined with each other
    def fold(self, op, sources, dst_ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """One fold per entry of ``sources`` (a sequence of id sequences), all in one launch
        (bf_bank_fold): result g = the AND / OR of the filters ``sources[g]``.  With ``dst_ids``
        filter ``dst_ids[g]`` is replaced by it (the destination may be among its own sources: an
        in-place merge; one source: a copy); without, nothing is written and 'xor' is allowed too.
        Returns ``(changed, set_bits)``: whether each destination's bytes differ afterwards (bool,
        all False without ``dst_ids``) and the BITCOUNT of each result (uint64)."""
        groups = [self._ids(s) for s in sources]
        seg = np.zeros(len(groups) + 1, np.uint64)
        if groups:
            np.cumsum([n for _, n in groups], out=seg[1:])
        live = [a[:n] for a, n in groups if n]
        src = np.concatenate(live) if live else np.zeros(1, np.uint32)
        dst = None
        if dst_ids is not None:
            dst, count = self._ids(dst_ids)
            if count != len(groups):
                raise ArgumentError("%d destinations for %d groups" % (count, len(groups)))
        n = len(groups)
        changed, set_bits = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64)
        _bank_check(self._lib.bf_bank_fold(self.handle, _op(op), _ptr(dst), _ptr(seg), _ptr(src), n, _ptr(changed),
                                           _ptr(set_bits)), self._h)
        return changed[:n].astype(bool), set_bits[:n]

    def overlap(self, row_ids=None, col_ids=None) -> np.ndarray:
        """BITCOUNT(filter row_ids[i] AND filter col_ids[j]) for every pair (bf_bank_overlap): a
        uint64 array of shape (rows, cols).  ``row_ids=None``: every filter; ``col_ids=None``: the
        row list, a symmetric matrix whose diagonal is ``bitcount``."""
        a, rows = self._ids(row_ids)
        c, cols = (None, rows) if col_ids is None else self._ids(col_ids)
        out = np.zeros((max(rows, 1), max(cols, 1)), np.uint64)
        _bank_check(self._lib.bf_bank_overlap(self.handle, _ptr(a), rows, _ptr(c), cols, _ptr(out)), self._h)
        return out if rows and cols else np.zeros((rows, cols), np.uint64)

    # -- device-resident API
    def fold_dev(self, op, d_seg: int, d_src_ids: int, groups: int, n_src: int, d_dst_ids: int = 0,
                 d_changed: int = 0, d_set_bits: int = 0, stream=None) -> None:
        """``groups`` folds on ``stream`` (bf_bank_fold_dev): d_seg holds groups + 1 uint64 ending in
        n_src, d_src_ids n_src uint32; d_dst_ids = 0 counts only; ``groups`` bytes are written at
        d_changed and ``groups`` uint64 at d_set_bits (each may be 0)."""
        _bank_check(self._lib.bf_bank_fold_dev(self.handle, _op(op), d_dst_ids or None, d_seg or None, d_src_ids or None,
                                               int(groups), int(n_src), d_changed or None, d_set_bits or None,
                                               self._s(stream)), self._h)

    def overlap_dev(self, d_out: int, d_row_ids: int = 0, rows: Optional[int] = None, d_col_ids: int = 0,
                    cols: Optional[int] = None, stream=None) -> None:
        """The overlap matrix on ``stream`` (bf_bank_overlap_dev): rows * cols uint64 are written at
        d_out (d_row_ids = 0: every filter, rows = n_filters; d_col_ids = 0: the row list)."""
        rows = self.n_filters if rows is None else int(rows)
        cols = rows if cols is None else int(cols)
        _bank_check(self._lib.bf_bank_overlap_dev(self.handle, d_row_ids or None, rows, d_col_ids or None, cols,
                                                  d_out or None, self._s(stream)), self._h)

    def insert_many_dev(self, d_keys: int, d_offsets: int, d_filter_ids: int, n: int, d_key_flipped: int = 0,
                        stream=None) -> None:
        _bank_check(self._lib.bf_bank_insert_many_dev(self.handle, d_keys, d_offsets, d_filter_ids, int(n),
                                                      d_key_flipped or None, self._s(stream)), self._h)

    def insert_many_seq_dev(self, d_keys: int, d_offsets: int, d_filter_ids: int, n: int, d_per_key_new: int = 0,
                            stream=None) -> None:
        """``insert_many_seq`` on device arrays.  Synchronises only when the bank's scratch has to
        grow (the first call of a shape; see ``seq_plan``)."""
        _bank_check(self._lib.bf_bank_insert_many_seq_dev(self.handle, d_keys, d_offsets, d_filter_ids, int(n),
                                                          d_per_key_new or None, self._s(stream)), self._h)

    def insert_many_changes_dev(self, d_keys: int, d_offsets: int, d_filter_ids: int, n: int, d_count: int,
                                d_out_ids: int = 0, d_out_bits: int = 0, cap: int = 0, seq: bool = False,
                                d_flags: int = 0, stream=None) -> None:
        """``insert_many_changes`` on device arrays (bf_bank_insert_many_changes_dev): the uint64 at
        d_count (8-byte aligned) is zeroed on ``stream`` and then counts every flipped bit; the first
        ``cap`` of them are listed at d_out_ids (uint32) and d_out_bits (uint64, 8-byte aligned),
        which may be 0 with ``cap=0``.  An overflow is not an error here: compare the count with
        ``cap``.  ``seq`` is passed as given (0 / 1)."""
        _bank_check(self._lib.bf_bank_insert_many_changes_dev(self.handle, d_keys or None, d_offsets or None,
                                                              d_filter_ids or None, int(n), int(seq), d_flags or None,
                                                              d_out_ids or None, d_out_bits or None, int(cap),
                                                              d_count or None, self._s(stream)), self._h)

    def include_many_dev(self, d_keys: int, d_offsets: int, d_filter_ids: int, n: int, d_out: int,
                         stream=None) -> None:
        _bank_check(self._lib.bf_bank_include_many_dev(self.handle, d_keys, d_offsets, d_filter_ids, int(n), d_out,
                                                       self._s(stream)), self._h)

    def include_across_dev(self, d_keys: int, d_offsets: int, n: int, d_mask: int, d_ids: int = 0,
                           count: Optional[int] = None, stream=None) -> None:
        """The cross query on ``stream``: n rows of ``across_row_bytes(count)`` bytes are written at
        d_mask (8-byte aligned; d_ids = 0: every filter, count = n_filters)."""
        count = self.n_filters if count is None else int(count)
        _bank_check(self._lib.bf_bank_include_across_dev(self.handle, d_keys, d_offsets, int(n), d_ids or None, count,
                                                         d_mask or None, self._s(stream)), self._h)

    def clear_dev(self, d_ids: int = 0, count: int = 0, stream=None) -> None:
        _bank_check(self._lib.bf_bank_clear_dev(self.handle, d_ids or None, int(count), self._s(stream)), self._h)

    def bitcount_dev(self, d_out: int, d_ids: int = 0, count: Optional[int] = None, stream=None) -> None:
        """Per-filter BITCOUNT on ``stream``; ``count`` uint64 are written at d_out (d_ids = 0:
        every filter, count = n_filters)."""
        count = self.n_filters if count is None else int(count)
        _bank_check(self._lib.bf_bank_bitcount_dev(self.handle, d_ids or None, count, d_out, self._s(stream)),
                    self._h)


def lua_layer_params(entries, precision, layer: int) -> Tuple[int, int]:
    """(bits, k) of layer `layer` of the Lua scalable filter (add.lua:16-25)."""
    b, k = ctypes.c_uint64(), ctypes.c_uint32()
    rc = load().bf_lua_layer_params(float(entries), float(precision), int(layer), ctypes.byref(b), ctypes.byref(k))
    if rc:
        raise ArgumentError("bf_lua_layer_params(%r, %r, %r) failed" % (entries, precision, layer))
    return int(b.value), int(k.value)


def lua_index(entries, count: int) -> int:
    """The layer a count maps to (add.lua:13-15 / check.lua:9-11)."""
    li = ctypes.c_uint32()
    if load().bf_lua_index(float(entries), int(count), ctypes.byref(li)):
        raise ArgumentError("bf_lua_index(%r, %r) failed" % (entries, count))
    return int(li.value)


_lua_check = functools.partial(_check, last_error="bf_lua_last_error")


class LuaFilter(_Handle):
    """The Lua driver's scalable filter on the device (a ``bf_lua*``; see include/bfhip.h)."""

    _DESTROY, _LAST_ERROR = "bf_lua_destroy", "bf_lua_last_error"   # (no own-stream getter: stream=0 by default)

    def __init__(self, entries, precision, device: int = -1):
        self._lib = load()
        cfg = bf_config(ctypes.sizeof(bf_config), int(device), 0, 0, 1, 0, 0, 0)
        h = _vp()
        _lua_check(self._lib.bf_lua_create(float(entries), float(precision), ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.entries, self.precision = entries, precision

    def insert_many(self, keys: np.ndarray, offsets: np.ndarray):
        """-> (per-key new flags, sorted list of layers that got a new item)."""
        keys, offsets, n = _keys(keys, offsets)
        pk = np.zeros(max(n, 1), np.uint8)
        mask = ctypes.c_uint64(0)
        _lua_check(self._lib.bf_lua_insert_many(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(pk),
                                                ctypes.byref(mask)), self._h)
        return pk[:n], [i + 1 for i in range(64) if mask.value >> i & 1]

    LAYER_SHIFT = 58   # BF_LUA_LAYER_SHIFT

    def insert_many_changes(self, keys: np.ndarray, offsets: np.ndarray):
        """-> (per-key new flags, layers that got a new item, [(layer, bit offset), ...] of every
        bit the batch flipped, each once: the SETBITs add.lua issued that changed something)."""
        keys, offsets, n = _keys(keys, offsets)
        pk = np.zeros(max(n, 1), np.uint8)
        mask = ctypes.c_uint64(0)
        cap = max(64 * n, 1)   # BF_MAX_K probes per key at most
        out = np.zeros(cap, np.uint64)
        cnt = ctypes.c_uint64(0)
        _lua_check(self._lib.bf_lua_insert_many_changes(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(pk),
                                                        ctypes.byref(mask), _ptr(out), cap, ctypes.byref(cnt)),
                   self._h)
        flips = out[: cnt.value]
        sh = np.uint64(self.LAYER_SHIFT)
        pairs = list(zip((flips >> sh).tolist(), (flips & ((np.uint64(1) << sh) - np.uint64(1))).tolist()))
        return pk[:n], [i + 1 for i in range(64) if mask.value >> i & 1], pairs

    def include_many(self, keys: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        keys, offsets, n = _keys(keys, offsets)
        out = np.zeros(max(n, 1), np.uint8)
        _lua_check(self._lib.bf_lua_include_many(self.handle, _ptr(keys), _ptr(offsets), n, _ptr(out)), self._h)
        return out[:n]

    # -- device-resident keys (bf_lua_insert_many_dev / bf_lua_include_many_dev): raw device
    #    addresses and a hipStream_t as ints, as Filter's *_dev methods
    def insert_many_dev(self, d_keys: int, d_offsets: int, n: int, d_per_key_new: int = 0, stream=0) -> list:
        """add.lua over n device keys; returns the layers that got a new item."""
        mask = ctypes.c_uint64()
        _lua_check(self._lib.bf_lua_insert_many_dev(self.handle, d_keys, d_offsets, int(n), d_per_key_new or None,
                                                    ctypes.byref(mask), self._s(stream)), self._h)
        return [i + 1 for i in range(64) if mask.value >> i & 1]

    def include_many_dev(self, d_keys: int, d_offsets: int, n: int, d_out: int, stream=0) -> None:
        _lua_check(self._lib.bf_lua_include_many_dev(self.handle, d_keys, d_offsets, int(n), d_out,
                                                     self._s(stream)), self._h)

    def profile(self, enable: bool) -> None:
        _lua_check(self._lib.bf_lua_profile(self.handle, 1 if enable else 0), self._h)

    def profile_read(self, reset: bool = True) -> dict:
        """{kernel name: (total ms, launches)} since the last reset (bf_lua_profile_read)."""
        cap = 64
        names = ctypes.create_string_buffer(cap * PROFILE_NAME_LEN)
        ms = np.zeros(cap, np.float64)
        cnt = np.zeros(cap, np.uint64)
        n = ctypes.c_uint32()
        _lua_check(self._lib.bf_lua_profile_read(self.handle, names, _ptr(ms), _ptr(cnt), cap, ctypes.byref(n),
                                                 1 if reset else 0), self._h)
        out = {}
        for i in range(min(n.value, cap)):
            raw = names.raw[i * PROFILE_NAME_LEN:(i + 1) * PROFILE_NAME_LEN]
            out[raw.split(b"\0", 1)[0].decode()] = (float(ms[i]), int(cnt[i]))
        return out

    def clear(self) -> None:
        _lua_check(self._lib.bf_lua_clear(self.handle), self._h)

    @property
    def count(self) -> int:
        c = ctypes.c_uint64()
        _lua_check(self._lib.bf_lua_get_count(self.handle, ctypes.byref(c)), self._h)
        return int(c.value)

    @count.setter
    def count(self, value: int) -> None:
        _lua_check(self._lib.bf_lua_set_count(self.handle, int(value)), self._h)

    @property
    def layers(self) -> int:
        n = ctypes.c_uint32()
        _lua_check(self._lib.bf_lua_layers(self.handle, ctypes.byref(n)), self._h)
        return int(n.value)

    def export_layer(self, layer: int) -> bytes:
        n = ctypes.c_uint64(0)
        _lua_check(self._lib.bf_lua_export_layer(self.handle, int(layer), None, 0, ctypes.byref(n)), self._h)
        buf = np.zeros(max(n.value, 1), np.uint8)
        _lua_check(self._lib.bf_lua_export_layer(self.handle, int(layer), _ptr(buf), len(buf), ctypes.byref(n)),
                   self._h)
        return buf[: n.value].tobytes()

    def import_layer(self, layer: int, data: bytes) -> None:
        buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
        _lua_check(self._lib.bf_lua_import_layer(self.handle, int(layer), _ptr(buf), len(data)), self._h)
