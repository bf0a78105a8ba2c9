"""Every key-hashing kernel on key shapes (tests/key_shapes.py): SHA-1 block boundaries, the
key's start alignment against its length, and tiles on both sides of the LDS stage's edge.

One test per hashing site A-I (key_shapes.SITES), each over ``boundaries``,
``alignment`` (the base pointer moved by 0 / 1 / 3 / 15 bytes too) and the site's own
``stage_edge`` at a 16-aligned start and at 15 mod 16.  Every comparison is exact, against
hashlib, oracle.py or lua_oracle.py.  The batches reach the kernels through the ``*_dev`` entry
points on 256-byte aligned tensors, so a key's offset is its address mod 16 and the tiles are
the ones tests/test_key_shapes.py checked.  Each case shows that its own kernel ran: the knob
that forces the form, bf_insert_plan, and the kernel names of bf_profile_read.
"""
import functools

import numpy as np
import pytest

import key_shapes as KS
import lua_oracle as L
from test_gpu_bank import M as BANK_M, K as BANK_K, changed_of, check_bank
from test_gpu_bank_changes import diff, pairs_of, snapshot
from test_gpu_bank_seq import SeqModel
from test_gpu_distributed import check_chunk_route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = ["boundaries", "alignment", "stage_edge-0", "stage_edge-15"]
SIDE_SHAPES = ["boundaries", "stage_edge-0", "stage_edge-15"]   # F1 / F2: a side batch (no alignment sweep)


@functools.lru_cache(maxsize=None)
def batch(site, shape):
    tile, stage = KS.site(site)
    if shape == "boundaries":
        return KS.boundaries(tile)
    if shape == "alignment":
        return KS.alignment()
    return KS.stage_edge(tile, stage, int(shape.split("-")[1]))


@functools.lru_cache(maxsize=None)
def want_digests(site, shape):
    return KS.digests(*batch(site, shape))


def deltas(shape):
    return (0, 1, 3, 15) if shape == "alignment" else (0,)


@functools.lru_cache(maxsize=None)
def ordinary(n, tag):
    """A small batch of plain decimal keys (the windows of F1 / F2, pre-inserted members)."""
    rng = np.random.default_rng(KS.SEED + 77)
    keys = [("%s%d" % (tag, int(v))).encode() for v in rng.integers(0, 10**12, n)]
    return KS.pack_lengths([len(x) for x in keys], rng), keys


def plain_batch(n, tag):
    (buf, offs), keys = ordinary(n, tag)
    buf = buf.copy()
    buf[: int(offs[-1])] = np.frombuffer(b"".join(keys), np.uint8)
    return buf, offs


class Dev:
    """A batch on the device: the bytes ``delta`` into a 256-byte aligned tensor."""

    def __init__(self, buf, offs, delta=0):
        self.n = len(offs) - 1
        self.store = torch.zeros(len(buf) + delta + KS.SLACK, dtype=torch.uint8, device="cuda")
        assert self.store.data_ptr() % 256 == 0
        self.store[delta: delta + len(buf)] = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
        self.keys = self.store[delta:]                      # a view: data_ptr() is moved by delta
        self.kp = self.store.data_ptr() + delta
        self.offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
        self.op = self.offs.data_ptr()


def cuda_u8(n, fill=7):
    return torch.full((max(n, 1),), fill, dtype=torch.uint8, device="cuda")


def cuda_dig(n):
    return torch.full((max(n, 1), 4), -1, dtype=torch.int32, device="cuda")


def host_dig(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def ran(prof, *names):
    for name in names:
        assert any(p == name or p.startswith(name) for p in prof), (name, sorted(prof))


# ---- A: the direct key kernel ------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_site_a_direct_kernel(pkg, oracle, shape):
    m, k = 95851, 7
    buf, offs = batch("A", shape)
    want_idx = oracle.indexes_many(buf, offs, m, k)
    with pkg.Filter(m, k) as f:
        f.profile(True)
        for delta in deltas(shape):
            d = Dev(buf, offs, delta)
            dig = cuda_dig(d.n)
            idx = torch.full((d.n, k), -1, dtype=torch.int64, device="cuda")
            f.hash_many_dev(d.kp, d.op, d.n, dig.data_ptr(), stream=0)
            f.indexes_many_dev(d.kp, d.op, d.n, idx.data_ptr(), stream=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host_dig(dig, d.n), want_digests("A", shape))
            np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint64), want_idx)
        ran(f.profile_read(), "bf_keys_kernel<HASH>", "bf_keys_kernel<INDEXES>")


# ---- B: include? + hash, two independent stages ------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_site_b_include_hash(pkg, oracle, shape):
    """The shape batch as the query, as the side batch, and both at once from different batches
    (the side batch of the last run is the next shape's)."""
    m, k = 9585058, 6
    buf, offs = batch("B", shape)
    other = SHAPES[(SHAPES.index(shape) + 1) % len(SHAPES)]
    obuf, ooffs = batch("B", other)
    pbuf, poffs = plain_batch(700, "b")
    n = len(offs) - 1
    bits = oracle.new_bitset(m, k)
    oracle.insert_many(bits, m, k, buf[:], offs[: n // 2 + 1])          # half the shape batch are members
    oracle.insert_many(bits, m, k, pbuf, poffs[:351])
    want = oracle.include_many(bits, m, k, buf, offs)
    want_plain = oracle.include_many(bits, m, k, pbuf, poffs)
    assert 0 < want.sum() < n
    with pkg.Filter(m, k) as f:
        f.profile(True)
        ins, pl = Dev(buf, offs), Dev(pbuf, poffs)
        f.insert_many_dev(ins.kp, ins.op, n // 2, stream=0)
        f.insert_many_dev(pl.kp, pl.op, 350, stream=0)
        side = Dev(obuf, ooffs)
        for delta in deltas(shape):
            d = Dev(buf, offs, delta)
            out, dig = cuda_u8(n), cuda_dig(n)
            f.include_hash_dev(d.kp, d.op, n, out.data_ptr(), 0, 0, 0, 0, stream=0)                     # query only
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy()[:n], want)
            out2 = cuda_u8(pl.n)
            f.include_hash_dev(pl.kp, pl.op, pl.n, out2.data_ptr(), d.kp, d.op, n, dig.data_ptr(), stream=0)   # side
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out2.cpu().numpy()[: pl.n], want_plain)
            np.testing.assert_array_equal(host_dig(dig, n), want_digests("B", shape))
            out.fill_(7)
            sdig = cuda_dig(side.n)
            f.include_hash_dev(d.kp, d.op, n, out.data_ptr(), side.kp, side.op, side.n, sdig.data_ptr(), stream=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy()[:n], want)
            np.testing.assert_array_equal(host_dig(sdig, side.n), want_digests("B", other))
        ran(f.profile_read(), "include_hash_kernel")


# ---- C: the binned front pass (insert, include?, region-set encode) ----------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_site_c_binned_front(pkg, oracle, monkeypatch, shape):
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_INCLUDE_BINNED", "1")
    m, k = 9585058, 6                                   # k <= 6: two 1024-key sub-tiles per workgroup tile
    buf, offs = batch("C", shape)
    fbuf, foffs = batch("C", SHAPES[(SHAPES.index(shape) + 2) % len(SHAPES)])   # mostly non-members
    n = len(offs) - 1
    bits = oracle.new_bitset(m, k)
    oracle.insert_many(bits, m, k, buf, offs)
    want_str = oracle.redis_string(bits)
    want_fresh = oracle.include_many(bits, m, k, fbuf, foffs)
    for delta in deltas(shape):
        d, fr = Dev(buf, offs, delta), Dev(fbuf, foffs, delta)
        with pkg.Filter(m, k) as f, pkg.Filter(m, k) as g:
            assert f.insert_plan(n)["binned"]
            f.profile(True)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            f.insert_many_dev(d.kp, d.op, n, d_any_new=flag.data_ptr(), stream=0)
            out, out2 = cuda_u8(n), cuda_u8(fr.n)
            f.include_many_dev(d.kp, d.op, n, out.data_ptr(), stream=0)
            f.include_many_dev(fr.kp, fr.op, fr.n, out2.data_ptr(), stream=0)
            torch.cuda.synchronize()
            assert int(flag.item()) == 1
            assert f.export_redis() == want_str
            assert out.cpu().numpy()[:n].all()
            np.testing.assert_array_equal(out2.cpu().numpy()[: fr.n], want_fresh)
            prof = f.profile_read()
            ran(prof, "bin_front", "bin_front_keys", "bin_apply", "bin_test")
            assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)
            # the region sets of the batch, ORed into a second filter
            cap = f.region_sets_capacity(n)
            sets = torch.zeros(cap // 4, dtype=torch.int32, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            f.encode_region_sets_dev(d.kp, d.op, n, sets.data_ptr(), cap, stream=0)
            torch.cuda.synchronize()
            ran(f.profile_read(), "sets_encode")
            g.insert_region_sets_dev(sets.data_ptr(), cap, 1, n * k, d_status=status.data_ptr(), stream=0)
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            assert g.export_redis() == want_str


# ---- D, E: the route fronts --------------------------------------------------------------------

ROUTE_P, ROUTE_B = 3, 10
CAP_ALIGN = 12288


def _u64(send):
    s = send.cpu().numpy()
    return s.view(np.uint32).astype(np.uint64) if s.dtype == np.int32 else s.view(np.uint64)


def check_fused_route(oracle, D, m, k, P, b, send, slot, counts, buf, offs):
    """bf_route_dev: segment s holds exactly owner s's (key, local offset) pairs."""
    n = len(offs) - 1
    idx = oracle.indexes_many(buf, offs, m, k).reshape(-1)
    owner, local = D.block_owner_local(idx, P, b)
    c = counts.cpu().numpy()
    assert c.tolist() == np.bincount(owner, minlength=P).tolist()
    s_np, sl = _u64(send), slot.cpu().numpy().astype(np.int64)
    assert np.bincount(sl, minlength=n).tolist() == [k] * n
    displ = np.concatenate([[0], np.cumsum(c)[:-1]])
    key_of = np.arange(n * k) // k
    for s in range(P):
        seg = slice(int(displ[s]), int(displ[s] + c[s]))
        assert sorted(zip(sl[seg].tolist(), s_np[seg].tolist())) == \
            sorted(zip(key_of[owner == s].tolist(), local[owner == s].tolist()))


def check_window_route(oracle, D, m, k, P, b, nh, cap, send, slot, counts, buf, offs):
    """bf_route_windows_dev: window w = s * nh + hi holds exactly owner s's pairs of that sub-range."""
    n = len(offs) - 1
    idx = oracle.indexes_many(buf, offs, m, k).reshape(-1)
    owner, local = D.block_owner_local(idx, P, b)
    win = owner.astype(np.int64) * nh + (local >> np.uint64(32)).astype(np.int64)
    want_c = np.bincount(win, minlength=P * nh)
    assert counts.cpu().numpy().tolist() == want_c.tolist()
    s_np, sl = _u64(send), slot.cpu().numpy().astype(np.int64)
    key_of = np.arange(n * k) // k
    for w in range(P * nh):
        ws = slice(w * cap, w * cap + int(want_c[w]))
        got = sorted(zip(sl[ws].tolist(), (s_np[ws] | np.uint64((w % nh) << 32)).tolist()))
        assert got == sorted(zip(key_of[win == w].tolist(), local[win == w].tolist()))


@pytest.mark.parametrize("shape", SHAPES)
def test_site_d_route_front(pkg, oracle, monkeypatch, shape):
    """k = 6 (<= 12 probe slots): the fused route, the window route and the chunk route."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    D = pkg.distributed
    m, k, P, b = 95851, 6, ROUTE_P, ROUTE_B
    buf, offs = batch("D", shape)
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    e = D.HipEngine(m, k, P, 0, b, dev)
    try:
        e.filter.profile(True)
        nh = e.nh
        geo = e.chunk_info(n)
        assert geo is not None
        tiles, dbytes = geo
        S = e.filter.route_chunk_info(n)[2]
        cap = -(-n * k // CAP_ALIGN) * CAP_ALIGN
        for delta in deltas(shape):
            d = Dev(buf, offs, delta)
            send, slot, counts = e.route(d.keys, d.offs, n)
            torch.cuda.synchronize()
            check_fused_route(oracle, D, m, k, P, b, send, slot, counts, buf, offs)
            send, slot, counts = e.route_windows(d.keys, d.offs, n, cap)
            torch.cuda.synchronize()
            check_window_route(oracle, D, m, k, P, b, nh, cap, send, slot, counts, buf, offs)
            send, slot, counts, dirb = e.route_chunks(d.keys, d.offs, n, cap, tiles, dbytes)
            torch.cuda.synchronize()
            check_chunk_route(oracle, D, m, k, P, b, nh, cap, tiles, dbytes, S, send, slot, counts, dirb, buf, offs)
        prof = e.filter.profile_read()
        ran(prof, "route_front_slot", "route_win_slot", "route_chunks_slot")
        assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)
    finally:
        e.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_site_e_route_chunks_idx(pkg, oracle, monkeypatch, shape):
    """k = 13 (> 12 probe slots): the chunk route takes route_chunks_idx_kernel<HASH>, whose key
    stage is carved out of its index buffer.  The route does not care how large the shard is: the
    small filter has a chunk geometry like any other."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    D = pkg.distributed
    m, k, P, b = 95851, 13, ROUTE_P, ROUTE_B
    buf, offs = batch("E", shape)
    n = len(offs) - 1
    e = D.HipEngine(m, k, P, 0, b, torch.device("cuda", 0))
    try:
        e.filter.profile(True)
        geo = e.chunk_info(n)
        assert geo is not None
        tiles, dbytes = geo
        assert tiles == -(-n // 1024)                       # one key per lane at k > 6
        S = e.filter.route_chunk_info(n)[2]
        cap = -(-n * k // CAP_ALIGN) * CAP_ALIGN
        for delta in deltas(shape):
            d = Dev(buf, offs, delta)
            send, slot, counts, dirb = e.route_chunks(d.keys, d.offs, n, cap, tiles, dbytes)
            torch.cuda.synchronize()
            check_chunk_route(oracle, D, m, k, P, b, e.nh, cap, tiles, dbytes, S, send, slot, counts, dirb, buf, offs)
        prof = e.filter.profile_read()
        ran(prof, "route_chunks_slot")
        assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)
    finally:
        e.close()


# ---- F1, F2: the owner tests' side batch -------------------------------------------------------

def _owner_windows(pkg, e, n_keys, tag):
    """One rank's chunked windows of a small ordinary batch, delivered to the single owner."""
    buf, offs = plain_batch(n_keys, tag)
    d = Dev(buf, offs)
    k = e.k
    tiles, dbytes = e.chunk_info(n_keys)
    cap = -(-n_keys * k // CAP_ALIGN) * CAP_ALIGN
    send, slot, counts, dirb = e.route_chunks(d.keys, d.offs, d.n, cap, tiles, dbytes)
    rmsg = torch.zeros(1, e.nh + 1, dtype=torch.int64, device=e.device)
    rmsg[0, : e.nh] = counts[: e.nh]
    torch.cuda.synchronize()
    return send, dirb, rmsg, cap, tiles, dbytes


@pytest.mark.parametrize("shape", SIDE_SHAPES)
def test_site_f1_apply_test_side_batch(pkg, monkeypatch, shape):
    """The one-pass owner step with the shape batch as its side batch: bin_apply_test_kernel<SIDE>
    hashes it from a stage carved out of the region image.  The shard is one region, so the one
    workgroup's tiles are the batch's tiles of 1024 keys."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_SHARD_TEST_BINNED", "1")
    monkeypatch.setenv("BFHIP_CHUNK_TEST_L2", "0")
    buf, offs = batch("F1", shape)
    e = pkg.distributed.HipEngine(95851, 6, 1, 0, ROUTE_B, torch.device("cuda", 0))
    try:
        assert e.filter.device_bytes * 8 <= 1 << 19            # one 2^19-bit region: one workgroup
        isend, idir, imsg, cap, tiles, dbytes = _owner_windows(pkg, e, 500, "i")
        tsend, tdir, tmsg, cap2, tiles2, dbytes2 = _owner_windows(pkg, e, 500, "t")
        assert (cap, tiles, dbytes) == (cap2, tiles2, dbytes2)
        e.filter.profile(True)
        side = Dev(buf, offs)
        sdig = cuda_dig(side.n)
        e.shard_insert_test_chunks_packed(isend, idir, imsg, tsend, tdir, tmsg, cap, 1, dbytes, tiles, e.nh + 1,
                                          nxt=(side.keys, side.offs, side.n, sdig))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_dig(sdig, side.n), want_digests("F1", shape))
        prof = e.filter.profile_read()
        ran(prof, "apply_test_hash")
        assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)
    finally:
        e.close()


@pytest.mark.parametrize("shape", SIDE_SHAPES)
def test_site_f2_l2_test_side_batch(pkg, monkeypatch, shape):
    """The L2-local owner test with the shape batch as its side batch: chunk_test_l2_kernel<SIDE>'s
    private stager of 256 keys and 4 KiB."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_SHARD_TEST_BINNED", "1")
    monkeypatch.setenv("BFHIP_CHUNK_TEST_L2", "1")
    buf, offs = batch("F2", shape)
    e = pkg.distributed.HipEngine(95851, 6, 1, 0, ROUTE_B, torch.device("cuda", 0))
    try:
        tsend, tdir, tmsg, cap, tiles, dbytes = _owner_windows(pkg, e, 500, "t")
        e.filter.profile(True)
        side = Dev(buf, offs)
        sdig = cuda_dig(side.n)
        out = torch.zeros(e.nh * cap, dtype=torch.uint8, device=e.device)
        e.shard_test_chunks(tsend, cap, 1, tdir, dbytes, tiles, tmsg, e.nh + 1, out,
                            nxt=(side.keys, side.offs, side.n, sdig))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_dig(sdig, side.n), want_digests("F2", shape))
        prof = e.filter.profile_read()
        ran(prof, "test_l2_hash")
        assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)
    finally:
        e.close()


# ---- G: sequential per-key inserts -------------------------------------------------------------

# (form, m, k, least keys): bf_seq.hip takes the binned form from 4096 keys on filters of up to
# 2^27 bits; below that the one-word-per-bit table where 4 m <= 12 * slots(n, k) (9585 bits), and
# the hash table elsewhere (9,585,058 bits).  tests/test_seq_plan_abi.py asserts these forms with
# bf_seq_plan at the batch sizes used here (test_key_shape_site_g_forms).
SEQ_FORMS = [("direct", 9585, 6, 0), ("binned", 9585, 6, 4096), ("binned", 95851, 7, 4096), ("hash", 9585058, 7, 0)]


@pytest.mark.parametrize("form,m,k,least", SEQ_FORMS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES)
def test_site_g_sequential_insert(pkg, oracle, shape, form, m, k, least):
    """The batch followed by copies of itself (half the keys or more repeat, so the flags are not
    all 1); the first copy keeps the shape's offsets."""
    buf, offs = batch("G", shape)
    n1 = len(offs) - 1
    times = max(2, -(-least // n1))
    rbuf, roffs = KS.repeat(buf, offs, times)
    n = len(roffs) - 1
    assert (n >= 4096) == (form == "binned") and m <= 1 << 27
    bits = oracle.new_bitset(m, k)
    want_any, want_pk = oracle.insert_many(bits, m, k, rbuf, roffs, per_key=True)
    assert want_pk[:n1].any() and not want_pk[n1:].any()
    for delta in deltas(shape):
        d = Dev(rbuf, roffs, delta)
        with pkg.Filter(m, k) as f:
            f.profile(True)
            pk = cuda_u8(n)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            f.insert_many_dev(d.kp, d.op, n, d_any_new=flag.data_ptr(), d_per_key_new=pk.data_ptr(), stream=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(pk.cpu().numpy()[:n], want_pk)
            assert bool(flag.item()) == bool(want_any)
            assert f.export_redis() == oracle.redis_string(bits)
            prof = f.profile_read()
            ran(prof, "seq_candidates", "seq_mark")
            assert not any(p.startswith("bf_keys_kernel") for p in prof), sorted(prof)


# ---- H: the Lua layout -------------------------------------------------------------------------

LUA_ENTRIES, LUA_PRECISION = 100, 0.01


def _lua_layers_equal(f, r):
    assert f.count == int(r.get("lbf:count"))
    assert f.layers >= 2
    for layer in range(1, f.layers + 1):
        assert f.export_layer(layer) == (r.get("lbf:%d" % layer) or b""), layer


@pytest.mark.parametrize("shape", SHAPES)
def test_site_h_lua(pkg, shape):
    buf, offs = batch("H", shape)
    keys = KS.keys_of(buf, offs)
    n = len(keys)
    fbuf, foffs = batch("H", SHAPES[(SHAPES.index(shape) + 2) % len(SHAPES)])    # mostly fresh keys
    fresh = KS.keys_of(fbuf, foffs)
    # the scripts from an empty filter: the host entry points
    r = pkg.FakeRedis()
    want_flags = np.array([L.add(r, "lbf", LUA_ENTRIES, LUA_PRECISION, key) for key in keys], bool)
    want_in = np.array([L.check(r, "lbf", LUA_ENTRIES, LUA_PRECISION, key) for key in keys + fresh], bool)
    set_bits, layer = 0, 1
    while r.exists("lbf:%d" % layer):
        set_bits += int(np.unpackbits(np.frombuffer(r.get("lbf:%d" % layer), np.uint8)).sum())
        layer += 1
    for call in ("insert_many", "insert_many_changes"):
        with pkg.LuaFilter(LUA_ENTRIES, LUA_PRECISION) as f:
            f.profile(True)
            got = getattr(f, call)(buf, offs)
            np.testing.assert_array_equal(got[0].astype(bool), want_flags)
            if call == "insert_many_changes":               # every flipped bit once
                assert len(got[2]) == len(set(got[2])) == set_bits
            _lua_layers_equal(f, r)
            inc = np.concatenate([f.include_many(buf, offs), f.include_many(fbuf, foffs)]).astype(bool)
            np.testing.assert_array_equal(inc, want_in)
            ran(f.profile_read(), "lua_check", "lua_seq_candidates[L1]", "lua_seq_mark[L2]")
    # the device entry points, on a filter whose count says that layer 4 has room for the whole
    # batch: one launch hashes every tile of the batch where the shape put it
    r = pkg.FakeRedis()
    r.set("lbf:count", b"701")
    want_flags = np.array([L.add(r, "lbf", LUA_ENTRIES, LUA_PRECISION, key) for key in keys], bool)
    want_in = np.array([L.check(r, "lbf", LUA_ENTRIES, LUA_PRECISION, key) for key in keys], bool)
    want_fresh = np.array([L.check(r, "lbf", LUA_ENTRIES, LUA_PRECISION, key) for key in fresh], bool)
    assert want_in.all() and not want_fresh.all()
    for delta in deltas(shape):
        d, fr = Dev(buf, offs, delta), Dev(fbuf, foffs, delta)
        with pkg.LuaFilter(LUA_ENTRIES, LUA_PRECISION) as f:
            f.profile(True)
            f.count = 701
            flags = cuda_u8(n)
            f.insert_many_dev(d.kp, d.op, n, flags.data_ptr(), stream=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(flags.cpu().numpy()[:n].astype(bool), want_flags)
            _lua_layers_equal(f, r)
            out, out2 = cuda_u8(n), cuda_u8(fr.n)
            f.include_many_dev(d.kp, d.op, n, out.data_ptr(), stream=0)
            f.include_many_dev(fr.kp, fr.op, fr.n, out2.data_ptr(), stream=0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy()[:n].astype(bool), want_in)
            np.testing.assert_array_equal(out2.cpu().numpy()[: fr.n].astype(bool), want_fresh)
            ran(f.profile_read(), "lua_check", "lua_seq_candidates[L4]", "lua_seq_mark[L4]")


# ---- I: the filter bank ------------------------------------------------------------------------

BANK_FILTERS = 3


def _dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


@pytest.mark.parametrize("shape", SHAPES)
def test_site_i_bank(pkg, oracle, shape):
    """insert / include? / across / seq (both tables) / changes over the shape batch, ids cycling
    over 3 filters, against one oracle bitset per filter.  The bank's entry points reach the bank's
    own kernels only; the sequential table's form is set with bf_bank_set_seq_form."""
    m, k, nf = BANK_M, BANK_K, BANK_FILTERS
    buf, offs = batch("I", shape)
    keys = KS.keys_of(buf, offs)
    n = len(keys)
    ids = (np.arange(n) % nf).astype(np.uint32)
    rbuf, roffs = KS.repeat(buf, offs, 2)
    rkeys, rids = keys + keys, np.concatenate([ids, ids])
    for delta in deltas(shape):
        d, rd = Dev(buf, offs, delta), Dev(rbuf, roffs, delta)
        di, rdi = _dev_i32(ids), _dev_i32(rids)
        other = _dev_i32((ids + 1) % nf)
        # insert, include?, across
        model = SeqModel(oracle, m, k)
        with pkg.FilterBank(m, k, nf) as bank:
            flipped = cuda_u8(n)
            bank.insert_many_dev(d.kp, d.op, di.data_ptr(), n, flipped.data_ptr(), stream=0)
            bank.sync()
            torch.cuda.synchronize()
            assert changed_of(ids, flipped.cpu().numpy()[:n]) == model.insert(keys, ids)
            check_bank(bank, model, nf)
            out, out2 = cuda_u8(n), cuda_u8(n)
            bank.include_many_dev(d.kp, d.op, di.data_ptr(), n, out.data_ptr(), stream=0)
            bank.include_many_dev(d.kp, d.op, other.data_ptr(), n, out2.data_ptr(), stream=0)
            row = bank.across_row_bytes(nf)
            mask = torch.full((n * row,), 0xFF, dtype=torch.uint8, device="cuda")
            bank.include_across_dev(d.kp, d.op, n, mask.data_ptr(), stream=0)
            bank.sync()
            torch.cuda.synchronize()
            assert out.cpu().numpy()[:n].all()
            np.testing.assert_array_equal(out2.cpu().numpy()[:n], model.include(keys, (ids + 1) % nf))
            got = np.unpackbits(mask.cpu().numpy().reshape(n, row), axis=1, bitorder="little")[:, :nf]
            want = np.stack([oracle.include_many(model.bits[f], m, k, buf, offs) for f in range(nf)], axis=1)
            np.testing.assert_array_equal(got, want)
        # the sequential insert, both tables: the batch and a copy of it
        for form in ("hash", "direct"):
            model = SeqModel(oracle, m, k)
            with pkg.FilterBank(m, k, nf) as bank:
                bank.set_seq_form(form)
                assert bank.seq_plan(2 * n)[0] is (form == "direct")
                pk = cuda_u8(2 * n)
                bank.insert_many_seq_dev(rd.kp, rd.op, rdi.data_ptr(), 2 * n, pk.data_ptr(), stream=0)
                bank.sync()
                torch.cuda.synchronize()
                want_pk = model.insert_seq(rkeys, rids)
                assert want_pk[:n].any() and not want_pk[n:].any()
                np.testing.assert_array_equal(pk.cpu().numpy()[: 2 * n], want_pk)
                check_bank(bank, model, nf)
        # the insert that lists the bits it flipped
        model = SeqModel(oracle, m, k)
        with pkg.FilterBank(m, k, nf) as bank:
            cap = n * k
            out_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
            out_bits = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            flags = cuda_u8(n)
            before = snapshot(model)
            bank.insert_many_changes_dev(d.kp, d.op, di.data_ptr(), n, d_count=count.data_ptr(),
                                         d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr(), cap=cap,
                                         seq=False, d_flags=flags.data_ptr(), stream=0)
            bank.sync()
            torch.cuda.synchronize()
            want_flags = model.insert_seq(keys, ids)
            total = int(count.item())
            got = pairs_of(out_ids.cpu().numpy()[:total].view(np.uint32), out_bits.cpu().numpy()[:total].view(np.uint64))
            assert got == diff(before, model)
            assert changed_of(ids, flags.cpu().numpy()[:n]) == changed_of(ids, want_flags)
            check_bank(bank, model, nf)
