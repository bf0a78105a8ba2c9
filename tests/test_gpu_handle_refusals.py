"""What bf_handle's device entry points (bf_api.cpp) refuse, and how: the return code, the exact
bf_last_error text and, where a call has two faults at once, which message wins.

Every case returns before any launch, so the handles are shared by the whole module; the last
test inserts into them and checks the answers against the oracle.  The calls go through raw
ctypes, as the C ABI's callers see them.  A pending key-status error (a kernel met inconsistent
key offsets) is reported exactly once, by the next call on the handle, also when that call is
one of the composite chunk calls.  (A shard handle has no keyed insert: there the hash-only
pass raises the status.)

Pinned as found: bf_hash_many_dev and bf_include_hash_dev refuse a misaligned digest pointer
also for an empty batch, and bf_shard_test_chunks_packed_dev / the fused call refuse a NULL
d_packed also when nsrc == 0 would make the call a no-op.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, K = 95851, 6
P, BLOCK_LOG2 = 3, 10
CAP = 12288            # a window capacity (a multiple of BF_WINDOW_CAP_ALIGN)
N_BOUND = 6000         # the chunk directory's batch bound: 3 route tiles of 2048 keys
TILE_KEYS = 2048

OK, EINVAL = 0, 1
NULLP = "NULL device pointer"
MULTI = "multi-device handle: use the host-pointer API"
ENCODER = "an encoder handle (BF_FLAG_ENCODER) holds no bitset: region-set encodes only"
SHARD_ROUTE = "handle holds one shard of a partitioned filter: use bf_route_dev"
SHARD = "handle holds one shard of a partitioned filter"
KEY_STATUS = ("an earlier call's key offsets were inconsistent (offsets must be non-decreasing "
              "and every key below 2 GiB): those keys were hashed as empty strings")
DIG_ALIGN = "d_digests must be 16-byte aligned"
NEXT_ALIGN = "d_next_digests must be 16-byte aligned"
SETS_ALIGN = "d_sets must be 16-byte aligned"
SETS_STRIDE = "d_sets and stride_bytes must be 16-byte aligned"
SIDE = "NULL side-hash pointer"
HI_PAST = "hi=1 is past the shard"
RUBY_ONLY = "digests carry the ruby driver's derivation only"
SETS_RUBY_ONLY = "region sets carry the ruby driver's derivation only"
NK_OVERFLOW = "n*k overflows"
BIG = 1 << 62          # n * 6 wraps
N32 = 1 << 30          # n * 6 >= 2^32


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(pkg):
    c = Ctx()
    c.pkg = pkg
    c.lib = pkg._lib.load()
    c.plain = pkg.Filter(M, K, device=0)
    c.shard = pkg.Filter(M, K, device=0, shard_count=P, shard_index=0, shard_block_log2=BLOCK_LOG2)
    c.enc = pkg.Filter(M, K, device=0, flags=pkg._lib.BF_FLAG_ENCODER)
    c.md5 = pkg.Filter(M, K, device=0, flags=pkg._lib.BF_FLAG_ENGINE_MD5)
    c.multi = pkg.Filter(M, K, devices=[0])
    c.buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    c.D = c.buf.data_ptr()
    assert c.D % 16 == 0
    c.D4 = c.D + 4
    c.tiles, c.dbytes, _ = c.shard.route_chunk_info(N_BOUND)
    assert c.tiles == 3 and c.dbytes > 16 and c.dbytes % 16 == 0
    assert c.shard.route_window_split() == 1 and c.shard.local_bits == 32768
    yield c
    for f in (c.plain, c.shard, c.enc, c.md5, c.multi):
        f.close()


def last_error(c, f):
    return c.lib.bf_last_error(f.handle).decode()


def refused(c, f, name, args, msg, code=EINVAL):
    rc = getattr(c.lib, name)(f.handle, *args)
    assert rc == code, "%s%r returned %d: %s" % (name, args, rc, last_error(c, f))
    assert last_error(c, f) == msg, "%s%r" % (name, args)


def accepted(c, f, name, args):
    """A degenerate form: BF_OK, and nothing was written to the handle's error."""
    before = last_error(c, f)
    rc = getattr(c.lib, name)(f.handle, *args)
    assert rc == OK, "%s%r returned %d: %s" % (name, args, rc, last_error(c, f))
    assert last_error(c, f) == before


def dir_msg(dir_bytes, tiles):
    return "dir_bytes %d does not hold %d tiles (bf_route_chunk_info)" % (dir_bytes, tiles)


def dev_entry_points(c):
    """Every bf_handle *_dev function with all-zero arguments after the handle."""
    for name, (_, argtypes) in sorted(c.pkg._lib.SIGNATURES.items()):
        if not name.endswith("_dev") or name.startswith(("bf_lua_", "bf_bank_")):
            continue
        yield name, [None if t is ctypes.c_void_p else 0 for t in argtypes[1:]]


def test_null_and_multi_handles(ctx):
    c = ctx
    names = []
    for name, args in dev_entry_points(c):
        names.append(name)
        assert getattr(c.lib, name)(None, *args) == EINVAL, name
        if name == "bf_bitop_dev":
            args[1] = c.multi.handle      # src: a NULL one is BF_EINVAL without a message
        refused(c, c.multi, name, args, MULTI)
    assert len(names) == 33, names


def test_run_dev(ctx):
    c, D = ctx, ctx.D
    refused(c, c.plain, "bf_insert_many_dev", (None, D, 5, None, None, None), NULLP)
    refused(c, c.plain, "bf_insert_many_dev", (D, None, 5, None, None, None), NULLP)
    refused(c, c.plain, "bf_include_many_dev", (D, D, 5, None, None), "d_out is NULL")
    refused(c, c.plain, "bf_include_many_dev", (None, D, 5, None, None), NULLP)
    refused(c, c.plain, "bf_indexes_many_dev", (D, D, 5, None, None), "d_out is NULL")
    refused(c, c.plain, "bf_indexes_many_dev", (D, None, 5, None, None), NULLP)
    refused(c, c.shard, "bf_insert_many_dev", (D, D, 5, None, None, None), SHARD_ROUTE)
    refused(c, c.shard, "bf_include_many_dev", (D, D, 5, None, None), "d_out is NULL")
    refused(c, c.shard, "bf_include_many_dev", (D, D, 5, D, None), SHARD_ROUTE)
    refused(c, c.enc, "bf_include_many_dev", (D, D, 5, None, None), "d_out is NULL")
    refused(c, c.enc, "bf_insert_many_dev", (D, D, 5, None, None, None), ENCODER)
    refused(c, c.enc, "bf_include_many_dev", (D, D, 5, D, None), ENCODER)
    refused(c, c.enc, "bf_indexes_many_dev", (D, D, 5, D, None), ENCODER)
    for f in (c.plain, c.shard, c.enc):
        accepted(c, f, "bf_insert_many_dev", (None, None, 0, None, None, None))
        accepted(c, f, "bf_include_many_dev", (None, None, 0, None, None))
        accepted(c, f, "bf_indexes_many_dev", (None, None, 0, None, None))


def test_route(ctx):
    c, D = ctx, ctx.D
    slots = "n*k must be < 2^32 per call (slot indices are 32-bit)"
    for f in (c.shard, c.plain):
        refused(c, f, "bf_route_dev", (D, D, 5, D, None, None, None), "d_counts is NULL")
        refused(c, f, "bf_route_dev", (None, None, 0, None, None, None, None), "d_counts is NULL")
        refused(c, f, "bf_route_dev", (None, D, 5, D, None, None, None), "d_counts is NULL")
        refused(c, f, "bf_route_dev", (None, D, 5, D, None, D, None), NULLP)
        refused(c, f, "bf_route_dev", (D, None, 5, D, None, D, None), NULLP)
        refused(c, f, "bf_route_dev", (D, D, 5, None, None, D, None), NULLP)
        refused(c, f, "bf_route_dev", (D, D, BIG, D, None, D, None), NK_OVERFLOW)
        refused(c, f, "bf_route_dev", (D, D, N32, D, None, D, None), slots)
    refused(c, c.enc, "bf_route_dev", (D, D, 5, D, None, D, None), ENCODER)
    f = c.shard
    refused(c, f, "bf_route_windows_dev", (D, D, 5, D, None, CAP, None, None), "d_counts is NULL")
    refused(c, f, "bf_route_windows_dev", (None, D, 5, D, None, CAP, None, None), "d_counts is NULL")
    refused(c, f, "bf_route_windows_dev", (None, D, 5, D, None, CAP, D, None), NULLP)
    refused(c, f, "bf_route_windows_dev", (D, D, 5, None, None, CAP, D, None), NULLP)
    refused(c, f, "bf_route_windows_dev", (D, D, BIG, D, None, CAP, D, None), NK_OVERFLOW)
    refused(c, f, "bf_route_windows_dev", (D, D, N32, D, None, 1 << 63, D, None), slots)
    refused(c, f, "bf_route_windows_dev", (D, D, 5, D, None, 1 << 63, D, None), "window_cap overflows")
    refused(c, c.enc, "bf_route_windows_dev", (D, D, 5, D, None, CAP, D, None), ENCODER)


def test_route_chunks(ctx):
    c, D, T, B = ctx, ctx.D, ctx.tiles, ctx.dbytes
    f = c.shard

    def both(keys, offs, n, send, cap, counts, dirp, dbytes, tiles, msg, keyed_only=False):
        refused(c, f, "bf_route_chunks_dev", (keys, offs, n, send, None, cap, counts, dirp, dbytes, tiles, None), msg)
        if not keyed_only:
            refused(c, f, "bf_route_chunks_digests_dev", (keys, n, send, None, cap, counts, dirp, dbytes, tiles, None),
                    msg)

    both(D, D, 5, D, CAP, None, D, B, T, "d_counts / d_dir is NULL")
    both(D, D, 5, D, CAP, D, None, B, T, "d_counts / d_dir is NULL")
    both(None, D, 5, D, CAP, None, D, B, T, "d_counts / d_dir is NULL")
    both(None, D, 5, D, CAP, D, D, B, T, NULLP)
    both(D, None, 5, D, CAP, D, D, B, T, NULLP, keyed_only=True)
    both(D, D, 5, None, CAP, D, D, B, T, NULLP)
    refused(c, f, "bf_route_chunks_digests_dev", (c.D4, 5, D, None, CAP, D, D, B, T, None), DIG_ALIGN)
    refused(c, f, "bf_route_chunks_digests_dev", (c.D4, BIG, D, None, CAP, D, D, B, T, None), DIG_ALIGN)
    both(D, D, BIG, D, CAP, D, D, B, T, NK_OVERFLOW)
    both(D, D, N32, D, (1 << 32) - 1, D, D, B, T, "n*k must be < 2^32 per call")
    both(D, D, 5, D, (1 << 32) - 1, D, D, B, 0, "window_cap must be < 2^32 - 1")
    both(D, D, 5, D, CAP, D, D, B + 8, 0, "tiles is 0")
    both(D, D, 5, D, CAP, D, D, B + 8, T, dir_msg(B + 8, T))
    both(D, D, 5, D, CAP, D, D, B - 16, T, dir_msg(B - 16, T))
    both(D, D, T * TILE_KEYS + 1, D, CAP, D, D, B - 16, T, dir_msg(B - 16, T))
    both(D, D, T * TILE_KEYS + 1, D, CAP, D, D, B, T, "%d keys need more than %d route tiles" % (T * TILE_KEYS + 1, T))


def test_shard_chunks(ctx):
    c, D, T, B = ctx, ctx.D, ctx.tiles, ctx.dbytes
    f = c.shard
    big = "1 sub-ranges x 3 windows x %d entries must stay below 2^32"
    forms = ["bf_shard_insert_chunks_dev", "bf_shard_test_chunks_dev", "bf_shard_test_chunks_packed_dev"]

    def each(recv, cap, nsrc, dirp, dbytes, tiles, counts, stride, msg):
        for name in forms:
            refused(c, f, name, (recv, cap, nsrc, dirp, dbytes, tiles, counts, stride, D, None), msg)
        refused(c, f, "bf_shard_test_chunks_hash_dev",
                (recv, cap, nsrc, dirp, dbytes, tiles, counts, stride, D, None, None, 0, None, None), msg)
        refused(c, f, "bf_shard_test_chunks_hash_dev",
                (recv, cap, nsrc, dirp, dbytes, tiles, counts, stride, D, D, D, 5, D, None), msg)
        refused(c, f, "bf_shard_insert_test_chunks_packed_dev",
                (recv, dirp, counts, D, D, D, cap, nsrc, dbytes, tiles, stride, None, D, None, None, 0, None, None), msg)
        refused(c, f, "bf_shard_insert_test_chunks_packed_dev",
                (D, D, D, recv, dirp, counts, cap, nsrc, dbytes, tiles, stride, None, D, D, D, 5, D, None), msg)

    each(None, CAP, P, D, B, T, D, 1, NULLP)
    each(D, CAP, P, None, B, T, D, 1, NULLP)
    each(D, CAP, P, D, B, T, None, 1, NULLP)
    each(None, CAP, P, D, B, 0, D, 0, NULLP)
    each(D, CAP, P, D, B + 8, 0, D, 0, "tiles is 0")
    each(D, CAP, P, D, B + 8, T, D, 0, dir_msg(B + 8, T))
    each(D, CAP, P, D, B - 16, T, D, 1, dir_msg(B - 16, T))
    each(D, 1 << 31, P, D, B, T, D, 0, "count_stride 0 < 1 sub-ranges")
    each(D, 1 << 31, P, D, B, T, D, 1, big % (1 << 31))
    each(D, 1 << 63, P, D, B, T, D, 1, big % (1 << 63))
    # the answer pointer: a NULL d_bits is a NULL device pointer, a NULL d_packed has its own message,
    # which wins over every other fault and over the no-op forms
    refused(c, f, "bf_shard_test_chunks_dev", (D, CAP, P, D, B, T, D, 1, None, None), NULLP)
    refused(c, f, "bf_shard_test_chunks_hash_dev", (D, CAP, P, D, B, T, D, 1, None, None, None, 0, None, None), NULLP)
    refused(c, f, "bf_shard_test_chunks_packed_dev", (D, CAP, P, D, B, T, D, 1, None, None), "d_packed is NULL")
    refused(c, f, "bf_shard_test_chunks_packed_dev", (None, CAP, P, D, B, 0, D, 0, None, None), "d_packed is NULL")
    refused(c, f, "bf_shard_test_chunks_packed_dev", (None, 0, 0, None, 0, 0, None, 0, None, None), "d_packed is NULL")
    fused = "bf_shard_insert_test_chunks_packed_dev"
    refused(c, f, fused, (D, D, D, D, D, D, CAP, P, B, T, 1, None, None, None, None, 0, None, None), "d_packed is NULL")
    refused(c, f, fused, (None, None, None, None, None, None, 0, 0, 0, 0, 0, None, None, D, D, 5, None, None),
            "d_packed is NULL")
    # the side batch: its pointers before the no-op forms and the window pointers
    refused(c, f, "bf_shard_test_chunks_hash_dev", (None, 0, 0, None, 0, 0, None, 0, None, None, D, 5, D, None), SIDE)
    refused(c, f, "bf_shard_test_chunks_hash_dev", (None, CAP, P, D, B, T, D, 1, D, D, D, 5, None, None), SIDE)
    refused(c, f, "bf_shard_test_chunks_hash_dev", (None, 0, 0, None, 0, 0, None, 0, None, D, D, 5, c.D4, None),
            DIG_ALIGN)   # (from the hash-only pass the no-op form becomes)
    refused(c, f, fused, (None, None, None, None, None, None, 0, 0, 0, 0, 0, None, D, D, None, 5, D, None), SIDE)
    refused(c, f, fused, (None, D, D, D, D, D, CAP, P, B, T, 1, None, D, None, D, 5, D, None), SIDE)
    refused(c, f, fused, (None, None, None, None, None, None, 0, 0, 0, 0, 0, None, D, D, D, 5, c.D4, None), NEXT_ALIGN)
    refused(c, f, fused, (None, D, D, D, D, D, CAP, P, B, T, 1, None, D, D, D, 5, c.D4, None), NEXT_ALIGN)
    refused(c, f, fused, (D, D, D, D, D, None, CAP, P, B, T, 1, None, D, None, None, 0, None, None), NULLP)
    # no windows and no side batch: nothing to do
    for cap, nsrc in ((CAP, 0), (0, P), (0, 0)):
        for name in forms:
            accepted(c, f, name, (None, cap, nsrc, None, 0, 0, None, 0, D, None))
        accepted(c, f, "bf_shard_test_chunks_hash_dev", (None, cap, nsrc, None, 0, 0, None, 0, None, None, None, 0, None,
                                                         None))
        accepted(c, f, fused, (None, None, None, None, None, None, cap, nsrc, 0, 0, 0, None, D, None, None, 0, None, None))


def test_combine_chunks_packed(ctx):
    c, D, T, B = ctx, ctx.D, ctx.tiles, ctx.dbytes
    f, name = c.shard, "bf_combine_chunks_packed_dev"
    refused(c, f, name, (None, D, CAP, D, B, T, D, 5, D, None), NULLP)
    refused(c, f, name, (D, None, CAP, D, B, T, D, 5, D, None), NULLP)
    refused(c, f, name, (D, D, CAP, None, B, T, D, 5, D, None), NULLP)
    refused(c, f, name, (D, D, CAP, D, B, T, None, 5, D, None), NULLP)
    refused(c, f, name, (D, D, CAP, D, B, 0, D, 5, None, None), NULLP)
    refused(c, f, name, (None, None, CAP, None, 0, 0, None, 0, None, None), "tiles is 0")
    refused(c, f, name, (D, D, CAP, D, B + 8, T, D, T * TILE_KEYS + 1, D, None), dir_msg(B + 8, T))
    refused(c, f, name, (D, D, CAP, D, B, T, D, T * TILE_KEYS + 1, D, None), "n exceeds the directory's tiles")


def test_owner_windows_and_hi(ctx):
    c, D = ctx, ctx.D
    f = c.shard
    refused(c, f, "bf_shard_insert_dev", (None, 5, None, None), "d_local is NULL")
    refused(c, f, "bf_shard_test_dev", (None, 5, D, None), NULLP)
    refused(c, f, "bf_shard_test_dev", (D, 5, None, None), NULLP)
    refused(c, f, "bf_shard_insert_hi_dev", (D, 5, 1, None, None), HI_PAST)
    refused(c, f, "bf_shard_insert_hi_dev", (None, 5, 1, None, None), HI_PAST)
    refused(c, f, "bf_shard_insert_hi_dev", (None, 5, 0, None, None), "d_local is NULL")
    refused(c, f, "bf_shard_test_hi_dev", (D, 5, 1, D, None), HI_PAST)
    refused(c, f, "bf_shard_test_hi_dev", (None, 5, 1, None, None), HI_PAST)
    refused(c, f, "bf_shard_test_hi_dev", (None, 5, 0, D, None), NULLP)
    refused(c, f, "bf_shard_test_hi_dev", (D, 5, 0, None, None), NULLP)
    refused(c, c.plain, "bf_shard_insert_hi_dev", (D, 5, 1, None, None), HI_PAST)
    for name, out, null_local in (("bf_shard_insert_windows_dev", None, "d_local is NULL"),
                                  ("bf_shard_test_windows_dev", D, NULLP)):
        # (d_local32, window_cap, nwin, d_counts, count_stride, hi, d_any_new / d_bits, stream)
        refused(c, f, name, (D, CAP, P, D, 1, 1, out, None), HI_PAST)
        refused(c, f, name, (D, CAP, P, None, 1, 1, out, None), HI_PAST)
        refused(c, f, name, (D, CAP, P, None, 1, 0, out, None), "d_counts is NULL")
        refused(c, f, name, (D, 1 << 63, P, None, 1, 0, out, None), "d_counts is NULL")
        refused(c, f, name, (D, 1 << 63, P, D, 1, 0, out, None), "window sizes overflow")
        refused(c, f, name, (D, 1 << 60, 65536, D, 1, 0, out, None), "window sizes overflow")
        refused(c, f, name, (D, 1, 65536, D, 1, 0, out, None), "at most 65535 windows")
        refused(c, f, name, (None, 1, 65536, D, 1, 0, out, None), "at most 65535 windows")
        refused(c, f, name, (None, CAP, P, D, 1, 0, out, None), null_local)
    refused(c, f, "bf_shard_test_windows_dev", (D, CAP, P, D, 1, 0, None, None), NULLP)


def test_combines_and_pack(ctx):
    c, D = ctx, ctx.D
    for f in (c.shard, c.plain):
        refused(c, f, "bf_combine_dev", (None, D, 5, D, None), NULLP)
        refused(c, f, "bf_combine_dev", (D, None, 5, D, None), NULLP)
        refused(c, f, "bf_combine_dev", (D, D, 5, None, None), NULLP)
        for name in ("bf_combine_windows_dev", "bf_combine_windows_packed_dev"):
            refused(c, f, name, (None, D, CAP, P, D, 5, D, None), NULLP)
            refused(c, f, name, (D, None, CAP, P, D, 5, D, None), NULLP)
            refused(c, f, name, (D, D, CAP, P, None, 5, D, None), NULLP)
            refused(c, f, name, (D, D, CAP, P, D, 5, None, None), NULLP)
        refused(c, f, "bf_pack_segments_dev", (None, D, 3, CAP, D, None), NULLP)
        refused(c, f, "bf_pack_segments_dev", (D, None, 3, CAP, D, None), NULLP)
        refused(c, f, "bf_pack_segments_dev", (D, D, 3, CAP, None, None), NULLP)
        refused(c, f, "bf_pack_segments_dev", (None, D, 65536, CAP, D, None), NULLP)
        refused(c, f, "bf_pack_segments_dev", (D, D, 65536, CAP, D, None), "at most 65535 segments")
    refused(c, c.enc, "bf_combine_dev", (D, D, 5, D, None), ENCODER)
    refused(c, c.enc, "bf_pack_segments_dev", (D, D, 3, CAP, D, None), ENCODER)


def test_digests(ctx):
    c, D, D4 = ctx, ctx.D, ctx.D4
    f = c.plain
    per_key = "per_key_new needs the keys (bf_insert_many_dev)"
    refused(c, f, "bf_insert_digests_dev", (D, 5, None, D, None), per_key)
    refused(c, f, "bf_insert_digests_dev", (None, 0, None, D, None), per_key)
    refused(c, f, "bf_insert_digests_dev", (None, 5, None, None, None), "d_digests is NULL")
    refused(c, f, "bf_insert_digests_dev", (D4, 5, None, None, None), DIG_ALIGN)
    refused(c, f, "bf_include_digests_dev", (None, 5, None, None), "d_digests is NULL")
    refused(c, f, "bf_include_digests_dev", (D4, 5, None, None), DIG_ALIGN)
    refused(c, f, "bf_include_digests_dev", (D, 5, None, None), "d_out is NULL")
    refused(c, c.shard, "bf_include_digests_dev", (D, 5, None, None), "d_out is NULL")
    refused(c, c.shard, "bf_include_digests_dev", (D, 5, D, None), SHARD)
    refused(c, c.shard, "bf_insert_digests_dev", (D, 5, None, None, None), SHARD)
    refused(c, c.md5, "bf_insert_digests_dev", (D, 5, None, None, None), RUBY_ONLY)
    refused(c, c.enc, "bf_insert_digests_dev", (D, 5, None, None, None), ENCODER)
    for g in (f, c.shard, c.md5, c.enc):
        accepted(c, g, "bf_insert_digests_dev", (None, 0, None, None, None))
        accepted(c, g, "bf_include_digests_dev", (D4, 0, None, None))

    refused(c, f, "bf_hash_many_dev", (D, D, 5, None, None), "d_digests is NULL")
    refused(c, f, "bf_hash_many_dev", (None, D, 5, D4, None), DIG_ALIGN)
    refused(c, f, "bf_hash_many_dev", (None, None, 0, D4, None), DIG_ALIGN)
    refused(c, f, "bf_hash_many_dev", (None, D, 5, D, None), NULLP)
    refused(c, f, "bf_hash_many_dev", (D, None, 5, D, None), NULLP)
    refused(c, c.enc, "bf_hash_many_dev", (D, D, 5, D, None), ENCODER)
    for g in (f, c.shard, c.enc):
        accepted(c, g, "bf_hash_many_dev", (None, None, 0, None, None))

    # (d_keys, d_offsets, n, d_out, d_next_keys, d_next_offsets, n_next, d_next_digests, stream)
    refused(c, f, "bf_include_hash_dev", (D, D, 5, None, D, D, 5, None, None), NULLP)
    refused(c, f, "bf_include_hash_dev", (None, D, 5, D, None, None, 0, None, None), NULLP)
    refused(c, f, "bf_include_hash_dev", (D, D, 5, D, D, D, 5, None, None), "NULL device pointer (next batch)")
    refused(c, f, "bf_include_hash_dev", (D, D, 5, D, None, D, 5, D4, None), "NULL device pointer (next batch)")
    refused(c, f, "bf_include_hash_dev", (D, D, 5, D, D, D, 5, D4, None), NEXT_ALIGN)
    refused(c, f, "bf_include_hash_dev", (None, None, 0, None, None, None, 0, D4, None), NEXT_ALIGN)
    refused(c, c.shard, "bf_include_hash_dev", (D, D, 5, D, D, D, 5, D4, None), NEXT_ALIGN)
    refused(c, c.shard, "bf_include_hash_dev", (None, None, 0, None, None, None, 0, None, None), SHARD)
    refused(c, c.md5, "bf_include_hash_dev", (None, None, 0, None, None, None, 0, None, None), RUBY_ONLY)
    refused(c, c.enc, "bf_include_hash_dev", (D, D, 5, D, None, None, 0, None, None), ENCODER)
    accepted(c, f, "bf_include_hash_dev", (None, None, 0, None, None, None, 0, None, None))
    accepted(c, c.enc, "bf_include_hash_dev", (None, None, 0, None, None, None, 0, None, None))


def test_region_sets(ctx):
    c, D, D4 = ctx, ctx.D, ctx.D4
    for f in (c.plain, c.enc):
        refused(c, f, "bf_encode_region_sets_dev", (D, D, 5, None, 1024, None), SETS_ALIGN)
        refused(c, f, "bf_encode_region_sets_dev", (None, D, 5, D4, 1024, None), SETS_ALIGN)
        refused(c, f, "bf_encode_region_sets_dev", (None, D, 5, D, 1024, None), NULLP)
        refused(c, f, "bf_encode_region_sets_dev", (D, None, 5, D, 1024, None), NULLP)
        refused(c, f, "bf_encode_region_sets_digests_dev", (D, 5, None, 1024, None), SETS_ALIGN)
        refused(c, f, "bf_encode_region_sets_digests_dev", (None, 5, D, 1024, None), NULLP)
        refused(c, f, "bf_encode_region_sets_digests_dev", (D4, 5, D, 1024, None), DIG_ALIGN)
    refused(c, c.shard, "bf_encode_region_sets_dev", (D, D, 5, D, 1024, None), SHARD)
    refused(c, c.shard, "bf_encode_region_sets_digests_dev", (D4, 5, D, 1024, None), DIG_ALIGN)
    refused(c, c.md5, "bf_encode_region_sets_dev", (D, D, 5, D, 1024, None), SETS_RUBY_ONLY)

    # (d_sets, stride_bytes, nsrc, probes_hint, d_any_new, d_status, stream)
    f = c.plain
    refused(c, f, "bf_insert_region_sets_dev", (None, 1024, 1, 0, None, None, None), SETS_STRIDE)
    refused(c, f, "bf_insert_region_sets_dev", (D4, 1024, 1, 0, None, None, None), SETS_STRIDE)
    refused(c, f, "bf_insert_region_sets_dev", (D, 1032, 1, 0, None, None, None), SETS_STRIDE)
    refused(c, c.shard, "bf_insert_region_sets_dev", (D, 1032, 1, 0, None, None, None), SETS_STRIDE)
    refused(c, c.shard, "bf_insert_region_sets_dev", (D, 1024, 1, 0, None, None, None), SHARD)
    refused(c, c.md5, "bf_insert_region_sets_dev", (D, 1024, 1, 0, None, None, None), SETS_RUBY_ONLY)
    for g in (f, c.shard, c.md5, c.enc):
        accepted(c, g, "bf_insert_region_sets_dev", (None, 1032, 0, 0, None, None, None))

    # (d_sets, stride_bytes, nsrc, probes_hint, d_any_new, d_status, d_next_digests, n_next, d_next_sets,
    #  next_sets_bytes, stream); nsrc == 0 is the encode alone, with the encode's refusals
    name = "bf_insert_encode_region_sets_dev"
    refused(c, f, name, (None, 0, 0, 0, None, None, D, 5, None, 1024, None), SETS_ALIGN)
    refused(c, f, name, (None, 0, 0, 0, None, None, None, 5, D, 1024, None), NULLP)
    refused(c, f, name, (None, 0, 0, 0, None, None, D4, 5, D, 1024, None), DIG_ALIGN)
    refused(c, c.shard, name, (None, 0, 0, 0, None, None, D, 5, D, 1024, None), SHARD)
    refused(c, f, name, (None, 1024, 1, 0, None, None, D, 5, None, 1024, None), SETS_STRIDE)
    refused(c, f, name, (D, 1032, 1, 0, None, None, D, 5, None, 1024, None), SETS_STRIDE)
    refused(c, f, name, (D, 1024, 1, 0, None, None, D4, 5, None, 1024, None), "d_next_sets must be 16-byte aligned")
    refused(c, f, name, (D, 1024, 1, 0, None, None, D4, 5, D4 + 4096, 1024, None),
            "d_next_sets must be 16-byte aligned")
    refused(c, f, name, (D, 1024, 1, 0, None, None, D4, 5, D + 4096, 1024, None),
            "d_next_digests must be a 16-byte aligned device pointer")
    refused(c, f, name, (D, 1024, 1, 0, None, None, None, 5, D + 4096, 1024, None),
            "d_next_digests must be a 16-byte aligned device pointer")
    refused(c, c.shard, name, (D, 1024, 1, 0, None, None, D, 5, D + 4096, 1024, None), SHARD)
    refused(c, c.md5, name, (D, 1024, 1, 0, None, None, D, 5, D + 4096, 1024, None), SETS_RUBY_ONLY)


def test_bitcount_and_bitop(ctx):
    c, D = ctx, ctx.D
    lib = c.lib
    refused(c, c.plain, "bf_bitcount_dev", (0, 8, None, None), "d_set_bits is NULL")
    refused(c, c.shard, "bf_bitcount_dev", (0, 8, None, None), "d_set_bits is NULL")
    refused(c, c.enc, "bf_bitcount_dev", (0, 8, None, None), "d_set_bits is NULL")
    refused(c, c.enc, "bf_bitcount_dev", (0, 8, D, None), ENCODER)

    a = c.plain
    bad_op = "bf_bitop: op must be BF_BITOP_AND or BF_BITOP_OR, got %d (XOR only counts: bf_bitcount_op)"
    shards = "%s: the handles differ in shard_count (1 vs 3)"
    before = last_error(c, a)
    assert lib.bf_bitop_dev(a.handle, 1, None, None, None, None) == EINVAL
    assert lib.bf_bitop(a.handle, 1, None, None, None) == EINVAL
    assert last_error(c, a) == before
    for name, tail in (("bf_bitop_dev", (None, None, None)), ("bf_bitop", (None, None))):
        refused(c, a, name, (7, a.handle) + tail, bad_op % 7)
        refused(c, a, name, (2, a.handle) + tail, bad_op % 2)
        refused(c, a, name, (7, c.shard.handle) + tail, shards % "bf_bitop")
        refused(c, a, name, (1, c.shard.handle) + tail, shards % "bf_bitop")
        refused(c, a, name, (1, c.enc.handle) + tail, "bf_bitop: an encoder handle (BF_FLAG_ENCODER) holds no bitset")
        refused(c, c.enc, name, (1, a.handle) + tail, "bf_bitop: an encoder handle (BF_FLAG_ENCODER) holds no bitset")
        refused(c, a, name, (1, c.md5.handle) + tail, "bf_bitop: the filters differ in hash engine (ruby vs md5)")
        refused(c, a, name, (7, c.multi.handle) + tail, "bf_bitop: the other handle is a multi-device handle")
    n = ctypes.c_uint64()
    assert lib.bf_bitcount_op(a.handle, 0, a.handle, None) == EINVAL
    refused(c, a, "bf_bitcount_op", (9, a.handle, ctypes.byref(n)),
            "bf_bitcount_op: op must be BF_BITOP_AND, _OR or _XOR, got 9")
    refused(c, a, "bf_bitcount_op", (9, c.shard.handle, ctypes.byref(n)), shards % "bf_bitcount_op")
    refused(c, c.shard, "bf_bitcount_op", (0, a.handle, ctypes.byref(n)),
            "bf_bitcount_op: the handles differ in shard_count (3 vs 1)")


def bad_batch(n=300, seed=5):
    """A key batch whose offsets keep their length but run backwards at one key."""
    keys = [("refuse-%d-%d" % (seed, i)).encode() for i in range(n)]
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum([len(x) for x in keys], out=offs[1:])
    offs[n // 2 + 1] = offs[n // 2] - 3
    buf = np.frombuffer(b"".join(keys) + b"\0" * 16, np.uint8).copy()
    return torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64).copy()).cuda(), n


def test_pending_key_status_is_reported_once(ctx):
    c, D, T, B = ctx, ctx.D, ctx.tiles, ctx.dbytes
    lib = c.lib
    dk, do, n = bad_batch()
    f = c.plain
    assert lib.bf_sync(f.handle) == OK
    assert lib.bf_insert_many_dev(f.handle, dk.data_ptr(), do.data_ptr(), n, None, None, None) == OK
    torch.cuda.synchronize()
    refused(c, f, "bf_sync", (), KEY_STATUS)
    assert lib.bf_sync(f.handle) == OK
    # ... by whatever call comes next: an argument refusal does not take it, the next accepted call does
    assert lib.bf_insert_many_dev(f.handle, dk.data_ptr(), do.data_ptr(), n, None, None, None) == OK
    torch.cuda.synchronize()
    refused(c, f, "bf_include_many_dev", (D, D, 5, None, None), "d_out is NULL")
    refused(c, f, "bf_bitcount_dev", (0, 8, D, None), KEY_STATUS)
    assert lib.bf_sync(f.handle) == OK

    # the composite chunk calls.  The status is met before anything is launched; should that ever
    # fail, the arguments describe real, separate, zeroed buffers of the shape passed (empty
    # windows: zero counts; a side batch of five empty keys), so the launches would be harmless.
    f = c.shard
    dig = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    recv = torch.zeros(P * CAP, dtype=torch.int32, device="cuda")
    dirs = torch.zeros(P * B, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(P, dtype=torch.int64, device="cuda")
    out = torch.zeros(P * CAP, dtype=torch.uint8, device="cuda")          # answer bytes or packed bits
    side = torch.zeros(64, dtype=torch.int64, device="cuda")               # 5 + 1 zero offsets; 16 B of keys
    sdig = torch.zeros((5, 4), dtype=torch.int32, device="cuda")
    R, DR, C, O = recv.data_ptr(), dirs.data_ptr(), counts.data_ptr(), out.data_ptr()
    SK, SO, SD = side.data_ptr() + 256, side.data_ptr(), sdig.data_ptr()
    assert SD % 16 == 0
    composite = [
        ("bf_shard_insert_chunks_dev", (R, CAP, P, DR, B, T, C, 1, None, None)),
        ("bf_shard_test_chunks_dev", (R, CAP, P, DR, B, T, C, 1, O, None)),
        ("bf_shard_test_chunks_packed_dev", (R, CAP, P, DR, B, T, C, 1, O, None)),
        ("bf_shard_test_chunks_hash_dev", (R, CAP, P, DR, B, T, C, 1, O, SK, SO, 5, SD, None)),
        ("bf_shard_test_chunks_hash_dev", (None, 0, 0, None, 0, 0, None, 0, None, SK, SO, 5, SD, None)),
        ("bf_shard_insert_test_chunks_packed_dev", (R, DR, C, R, DR, C, CAP, P, B, T, 1, None, O, None, None, 0, None,
                                                    None)),
        ("bf_shard_insert_test_chunks_packed_dev", (None, None, None, None, None, None, 0, 0, 0, 0, 0, None, O, SK, SO,
                                                    5, SD, None)),
    ]
    assert lib.bf_sync(f.handle) == OK
    for name, args in composite:
        assert lib.bf_hash_many_dev(f.handle, dk.data_ptr(), do.data_ptr(), n, dig.data_ptr(), None) == OK
        torch.cuda.synchronize()
        refused(c, f, name, args, KEY_STATUS)
        assert lib.bf_sync(f.handle) == OK, name


def test_handles_still_work(ctx, oracle):
    """After every refusal above: the plain handle inserts and answers as the oracle does, and so
    does the shard handle over its own local offsets."""
    c = ctx
    pkg, lib = c.pkg, c.lib
    keys = ["after-%d" % i for i in range(3000)]
    ib, io = pkg.keys.pack(keys)
    pb, po = pkg.keys.pack(keys[:500] + ["fresh-%d" % i for i in range(2500)])
    bits = oracle.new_bitset(M, K)
    oracle.insert_many(bits, M, K, ib, io)

    f = c.plain
    f.clear()
    f.insert_many(ib, io)
    assert f.export_redis() == oracle.redis_string(bits)
    np.testing.assert_array_equal(f.include_many(pb, po), oracle.include_many(bits, M, K, pb, po))

    f = c.shard
    f.clear()
    idx = oracle.indexes_many(ib, io, M, K).reshape(-1)
    owner, local = pkg.distributed.block_owner_local(idx, P, BLOCK_LOG2)
    lo = local[owner == 0].astype(np.uint64)
    want = np.zeros(f.local_bits // 8, np.uint8)
    np.bitwise_or.at(want, (lo >> np.uint64(3)).astype(np.int64), (np.uint64(0x80) >> (lo & np.uint64(7))).astype(np.uint8))
    d_lo = torch.from_numpy(lo.view(np.int64).copy()).cuda()
    assert lib.bf_shard_insert_dev(f.handle, d_lo.data_ptr(), len(lo), None, None) == OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.asarray(f.shard_export()), want)
    every = torch.arange(f.local_bits, dtype=torch.int64, device="cuda")
    ans = torch.empty(f.local_bits, dtype=torch.uint8, device="cuda")
    assert lib.bf_shard_test_dev(f.handle, every.data_ptr(), f.local_bits, ans.data_ptr(), None) == OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ans.cpu().numpy(), np.unpackbits(want))
