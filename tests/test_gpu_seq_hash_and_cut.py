"""The sequential insert's hash-table form (bf_seq.hip) and the Lua layout's layer cut (bf_lua.hip)
where no other test reaches them: the hash form called with i0 = 1, with a cut inside the chunk
(a host limit, a device limit) and with a flip list; the table's own edges (a probe run that wraps
from the last slot to slot 0, the exactly half-full table, k = 64); and lua_count_kernel /
lua_cut_kernel at fixed buffer alignments and cut positions.

Everything is exact.  Lua cases run the restated scripts (oracle/lua_oracle.py) over FakeRedis:
per-key INCR flags, count, every layer's string and check.lua's answers.  Filter cases run the C
oracle's one-by-one loop: per-key flags, any_new, the Redis string and the dirty blocks.  Each
case first derives the chunks its call issues from the scripts' own flags (``chunks_of``) and
asserts the form of each with bf_seq_plan; tests/test_seq_plan_abi.py pins those forms on a
machine without a GPU.
"""
import functools

import numpy as np
import pytest

import lua_oracle as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HASH, DIRECT, BINNED = 0, 1, 2
ENTRIES, PRECISION = 1000, 0.01          # layers 11027/7, 24940/8, 55652/9; full at 1000, 3000, 7000
POINTS = ["host", "changes", "dev"]      # bf_lua_insert_many, _changes, _dev
GUARD = 0xA5


# ---- the scripts, and what a call must do by them ----------------------------------------------

class Script:
    """add.lua / check.lua over one FakeRedis key."""

    def __init__(self, pkg, entries=ENTRIES, precision=PRECISION):
        self.r, self.entries, self.precision = pkg.FakeRedis(), entries, precision

    @property
    def count(self):
        return int(self.r.get("lbf:count") or 0)

    @count.setter
    def count(self, value):
        self.r.set("lbf:count", b"%d" % value)

    def add(self, keys):
        return np.array([L.add(self.r, "lbf", self.entries, self.precision, key) for key in keys], bool)

    def check(self, keys):
        return np.array([L.check(self.r, "lbf", self.entries, self.precision, key) for key in keys], bool)

    def string(self, layer):
        return self.r.get("lbf:%d" % layer) or b""

    def bits(self, layer):
        m, _ = L.layer_params(float(self.entries), float(self.precision), layer)
        a = np.zeros((m + 7) // 8, np.uint8)
        s = self.string(layer)
        a[: len(s)] = np.frombuffer(s, np.uint8)
        return np.unpackbits(a)

    def snapshot(self, upto=4):
        return {n: self.bits(n) for n in range(1, upto + 1)}


def capacity(entries, layer):
    """The largest count that still maps to ``layer`` (add.lua:13-15)."""
    cap = (2 ** layer - 1) * entries
    assert L.layer_index(float(entries), cap) == layer and L.layer_index(float(entries), cap + 1) == layer + 1
    return cap


def chunks_of(pkg, sc, count0, flags):
    """The chunks one insert call issues, from the scripts' own flags: the layer add.lua picks at
    the count, at most seq_plan's chunk_keys keys, cut after the key whose INCR fills the layer
    (the flags up to the cut are that layer's).  ``cut`` says the call has to look for one."""
    out, s, count, n = [], 0, count0, len(flags)
    while s < n:
        layer = L.layer_index(float(sc.entries), count + 1)
        m, k = L.layer_params(float(sc.entries), float(sc.precision), layer)
        room = capacity(sc.entries, layer) - count
        cn = min(n - s, pkg._lib.seq_plan(1, k, m)["chunk_keys"])
        take = cn
        fresh = np.cumsum(flags[s: s + cn])
        hit = np.flatnonzero(fresh == room)
        if len(hit):
            take = int(hit[0]) + 1
        out.append(dict(layer=layer, cn=cn, take=take, room=room, cut=room < cn,
                        form=pkg._lib.seq_plan(cn, k, m)["form"]))
        count += int(fresh[take - 1])
        s += take
    return out


def lua_form(layer, cn):
    """The form of a chunk on layers 1-3 of 1000 @ 0.01, as tests/test_seq_plan_abi.py pins it."""
    if cn >= 4096:
        return BINNED
    return HASH if cn <= {1: 146, 2: 512, 3: 910}[layer] else DIRECT


def shape(chunks):
    return [(c["layer"], c["cn"], c["take"]) for c in chunks]


class Dev:
    """A packed batch on the device, with the 16 readable bytes after the last key."""

    def __init__(self, buf, offs):
        self.n = len(offs) - 1
        self.keys = torch.from_numpy(np.concatenate([buf, np.zeros(16, np.uint8)])).cuda()
        self.offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
        self.kp, self.op = self.keys.data_ptr(), self.offs.data_ptr()


class Flags:
    """n flag bytes at byte ``align`` (mod 16) of a larger tensor, guard bytes on both sides."""

    def __init__(self, n, align=0):
        self.n, self.lead = n, 16 + align
        self.store = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.store.data_ptr() % 256 == 0
        self.ptr = self.store.data_ptr() + self.lead

    def read(self):
        a = self.store.cpu().numpy()
        assert (a[: self.lead] == GUARD).all() and (a[self.lead + self.n:] == GUARD).all(), "guard bytes written"
        return a[self.lead: self.lead + self.n]


def lua_insert(pkg, f, point, keys, align=0):
    """-> (flags, flips or None) of one call through the named entry point."""
    buf, offs = pkg.keys.pack(keys)
    if point == "host":
        return f.insert_many(buf, offs)[0].astype(bool), None
    if point == "changes":
        pk, _, flips = f.insert_many_changes(buf, offs)
        return pk.astype(bool), flips
    d, fl = Dev(buf, offs), Flags(len(keys), align)
    f.insert_many_dev(d.kp, d.op, d.n, fl.ptr, stream=0)
    torch.cuda.synchronize()
    got = fl.read()
    assert set(np.unique(got).tolist()) <= {0, 1}
    return got.astype(bool), None


def check_state(pkg, f, sc, probe):
    assert f.count == sc.count
    for layer in range(1, max(f.layers, 4) + 1):
        assert f.export_layer(layer) == sc.string(layer), layer
    got = f.include_many(*pkg.keys.pack(probe)).astype(bool)
    np.testing.assert_array_equal(got, sc.check(probe))


def check_flips(flips, before, after):
    """The flips are exactly the bits the scripts set, each once, tagged with its layer."""
    got = {}
    for layer, off in flips:
        got.setdefault(layer, []).append(off)
    assert set(got) <= set(after)
    for layer in after:
        want = np.flatnonzero(after[layer] & ~before[layer]).tolist()
        assert sorted(got.get(layer, [])) == want, layer


def ran(prof, *names):
    for name in names:
        assert name in prof, (name, sorted(prof))


def fresh_keys(tag, n=40):
    return [b"never-%s-%d" % (tag.encode(), i) for i in range(n)]


# ---- a. Lua, hash form, no cut -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batches_a(n):
    """Two batches of n keys: the first with repeats (keys 0 and 1 the same, the last two the
    same); the second alternates keys of the first with new ones, one new key back to back."""
    rng = np.random.default_rng(4100 + n)
    pool = [b"a%d-%d" % (n, i) for i in range(max(1, (2 * n + 2) // 3))]
    idx = rng.integers(0, len(pool), n)
    if n >= 2:
        idx[1] = idx[0]
    if n >= 4:
        idx[-1] = idx[-2]
    first = [pool[i] for i in idx]
    second = [first[j] if j % 2 == 0 else b"b%d-%d" % (n, j) for j in range(n)]
    if n >= 3:
        second[2] = second[1]
    return first, second


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("n", [1, 2, 73, 146])
def test_lua_hash_form_without_a_cut(pkg, point, n):
    """Layer 1 takes the hash form up to 146 keys: seq_candidates / seq_mark<hash> with i0 = 1,
    and with a flip list for the changes call."""
    sc = Script(pkg)
    with pkg.LuaFilter(ENTRIES, PRECISION) as f:
        f.profile(True)
        for keys in batches_a(n):
            before, count0 = sc.snapshot(), sc.count
            want = sc.add(keys)
            assert shape(chunks_of(pkg, sc, count0, want)) == [(1, n, n)]
            assert pkg._lib.seq_plan(n, 7, 11027)["form"] == HASH == lua_form(1, n)
            got, flips = lua_insert(pkg, f, point, keys)
            np.testing.assert_array_equal(got, want)
            check_state(pkg, f, sc, keys + fresh_keys("a"))
            if flips is not None:
                check_flips(flips, before, sc.snapshot())
        assert n < 2 or (want.any() and not want.all())
        ran(f.profile_read(), "lua_seq_candidates[L1]", "lua_seq_mark[L1]")


# ---- b. Lua, hash form, a cut inside the chunk -------------------------------------------------

CROSSINGS = {1: 120, 2: 400}     # lower layer -> batch size: hash form there and one layer up


@functools.lru_cache(maxsize=None)
def batch_b(lower, all_new):
    n = CROSSINGS[lower]
    if all_new:
        return tuple(b"n%d-%d" % (lower, i) for i in range(n))
    rng = np.random.default_rng(4200 + lower)
    pool = [b"c%d-%d" % (lower, i) for i in range(n * 3 // 5)]
    idx = rng.integers(0, len(pool), n)
    idx[1] = idx[0]
    idx[-6:] = idx[:6]               # the batch ends in repeats
    return tuple(pool[i] for i in idx)


@functools.lru_cache(maxsize=None)
def new_in_lower(lower, all_new):
    """How many keys of the batch are new when all of it lands on the lower layer."""
    import pkgload
    sc = Script(pkgload.load())
    sc.count = capacity(ENTRIES, lower - 1) if lower > 1 else 0
    flags = sc.add(batch_b(lower, all_new))
    assert sc.count <= capacity(ENTRIES, lower)
    return int(flags.sum()), int(np.flatnonzero(flags)[-1])


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("room", ["1", "2", "new", "new-1", "cn", "cn-1"])
@pytest.mark.parametrize("lower", [1, 2])
def test_lua_hash_form_cut_inside_the_chunk(pkg, point, room, lower):
    """The count is set so the lower layer has room for 1, 2, exactly the batch's new keys (the cut
    lands on the last new key; the trailing repeats go up a layer and come back new) or one fewer;
    "cn" / "cn-1" are an all-new batch with room for all of it (one pass, no cut) and for all but
    its last key (two passes).  Layers 1 -> 2 at count 1000 and 2 -> 3 at 3000, every chunk in the
    hash form."""
    all_new = room in ("cn", "cn-1")
    keys = list(batch_b(lower, all_new))
    n = len(keys)
    fresh, last_new = new_in_lower(lower, all_new)
    assert fresh == n if all_new else 2 < fresh < n and last_new < n - 6
    r = {"1": 1, "2": 2, "new": fresh, "new-1": fresh - 1, "cn": n, "cn-1": n - 1}[room]
    sc = Script(pkg)
    sc.count = count0 = capacity(ENTRIES, lower) - r
    before = sc.snapshot()
    want = sc.add(keys)
    chunks = chunks_of(pkg, sc, count0, want)
    if room == "cn":
        assert shape(chunks) == [(lower, n, n)] and not chunks[0]["cut"]
    else:
        take = chunks[0]["take"]
        assert shape(chunks) == [(lower, n, take), (lower + 1, n - take, n - take)] and chunks[0]["cut"]
        assert take == {"1": 1, "new": last_new + 1, "cn-1": n - 1}.get(room, take) and 0 < take < n
        assert int(want[:take].sum()) == r and want[take - 1] and want[take]
    assert all(c["form"] == HASH == lua_form(c["layer"], c["cn"]) for c in chunks)
    # a key past the cut would set a bit of the lower layer that stays 0
    if room not in ("new", "cn"):
        lo_m, lo_k = L.layer_params(float(ENTRIES), PRECISION, lower)
        lo_bits = sc.bits(lower)
        past = [key for key in keys[chunks[0]["take"]:] if key not in keys[: chunks[0]["take"]]]
        assert any(lo_bits[L._probe(L._h(key), i) % lo_m] == 0 for key in past for i in range(1, lo_k + 1))
    with pkg.LuaFilter(ENTRIES, PRECISION) as f:
        f.profile(True)
        f.count = count0
        got, flips = lua_insert(pkg, f, point, keys)
        np.testing.assert_array_equal(got, want)
        check_state(pkg, f, sc, keys + fresh_keys("b"))
        if flips is not None:
            after = sc.snapshot()
            check_flips(flips, before, after)
            assert room == "cn" or {lay for lay, _ in flips} == {lower, lower + 1}
        ran(f.profile_read(), *["lua_seq_mark[L%d]" % c["layer"] for c in chunks])


# ---- c. the hash table's edges, on both callers ------------------------------------------------

M64 = (1 << 64) - 1


def mix64(x):
    """bf_seq_table.h's slot hash: the SplitMix64 finalizer."""
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def lua_probes(keys, m, k):
    return [[L._probe(L._h(key), i) % m for i in range(1, k + 1)] for key in keys]


def wraps(offsets, slots):
    """Two distinct offsets whose home slot is the table's last: whichever is inserted second
    probes on from slot slots - 1 to slot 0."""
    return sum(1 for o in set(offsets) if mix64(o) & (slots - 1) == slots - 1) >= 2


def wrap_batch(seed):
    """73 keys (2 n k = 1022: 1024 slots), 60 distinct and 13 repeated in the middle."""
    keys = [b"w%d-%d" % (seed, i) for i in range(60)]
    return keys[:30] + keys[:13] + keys[30:]


# Found by a search over seeds on the CPU (about one seed in eleven wraps); each test asserts its
# seed's property before it runs, so a changed key format or hash cannot lapse unnoticed.
WRAP_SEED_FILTER, WRAP_SEED_LUA = 6, 19
HALF_SEED_FILTER, HALF_SEED_LUA = 1, 3
HALF_LUA = (80000, 0.005)                        # layer 1: 997635 bits, k = 8
K64_LUA = (2000, 1e-19)                          # layer 1: 185001 bits, k = 64


def half_batch(seed):
    return [b"h%d-%d" % (seed, i) for i in range(64)]


def k64_batch(n):
    rng = np.random.default_rng(4300 + n)
    keys = [b"k64-%d" % i for i in range(n // 2)] * 2
    return [keys[i] for i in rng.permutation(n)]


def filter_case(pkg, oracle, point, m, k, batches, slots):
    """Filter.insert_many(per_key_new=True) / insert_many_dev(d_per_key_new) (i0 = 0) against the
    C oracle's one-by-one loop: flags, any_new, the Redis string, and dirty blocks that bound the
    change.  Returns the oracle's flags of every batch."""
    bits = oracle.new_bitset(m, k)
    flags = []
    with pkg.Filter(m, k) as f:
        f.profile(True)
        f.track_dirty(True)
        for keys in batches:
            buf, offs = pkg.keys.pack(keys)
            n = len(keys)
            p = pkg._lib.seq_plan(n, k, m)
            assert p["form"] == HASH and n <= p["chunk_keys"]
            assert flags or p["slots"] == slots             # the first batch's table
            s0 = oracle.redis_string(bits)
            want_any, want_pk = oracle.insert_many(bits, m, k, buf, offs, per_key=True)
            s1 = oracle.redis_string(bits)
            if point == "host":
                got_any, got_pk = f.insert_many(buf, offs, any_new=True, per_key_new=True)
            else:
                d, fl = Dev(buf, offs), Flags(n)
                flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                f.insert_many_dev(d.kp, d.op, n, d_any_new=flag.data_ptr(), d_per_key_new=fl.ptr, stream=0)
                torch.cuda.synchronize()
                got_any, got_pk = bool(flag.item()), fl.read()
            np.testing.assert_array_equal(got_pk, want_pk)
            assert got_any == want_any
            assert f.export_redis() == s1
            ranges, rlen = f.dirty_ranges(clear=True)
            assert rlen == len(s1)
            size = max(len(s0), len(s1))
            a0, a1 = np.zeros(size, np.uint8), np.zeros(size, np.uint8)
            a0[: len(s0)], a1[: len(s1)] = np.frombuffer(s0, np.uint8), np.frombuffer(s1, np.uint8)
            changed = set((np.flatnonzero(a0 != a1) >> 16).tolist())
            touched = set((oracle.indexes_many(buf, offs, m, k).reshape(-1) >> np.uint64(19)).tolist())
            got = set()
            for off, ln in ranges:
                got.update(range(off >> 16, (off + ln - 1 >> 16) + 1))
            assert changed <= got <= touched
            flags.append(want_pk.astype(bool))
        ran(f.profile_read(), "seq_candidates", "seq_mark")
    return flags


def lua_case(pkg, point, params, batches, slots):
    """The same batches on layer 1 of a LuaFilter (i0 = 1), against the scripts."""
    sc = Script(pkg, *params)
    m, k = L.layer_params(float(params[0]), float(params[1]), 1)
    flags = []
    with pkg.LuaFilter(*params) as f:
        f.profile(True)
        for keys in batches:
            before, count0 = sc.snapshot(1), sc.count
            want = sc.add(keys)
            chunks = chunks_of(pkg, sc, count0, want)
            assert shape(chunks) == [(1, len(keys), len(keys))] and chunks[0]["form"] == HASH
            assert flags or pkg._lib.seq_plan(len(keys), k, m)["slots"] == slots   # the first batch's table
            got, flips = lua_insert(pkg, f, point, keys)
            np.testing.assert_array_equal(got, want)
            assert f.count == sc.count and f.export_layer(1) == sc.string(1)
            probe = keys + fresh_keys("c")
            np.testing.assert_array_equal(f.include_many(*pkg.keys.pack(probe)).astype(bool), sc.check(probe))
            if flips is not None:
                check_flips(flips, before, sc.snapshot(1))
            flags.append(want)
        ran(f.profile_read(), "lua_seq_candidates[L1]", "lua_seq_mark[L1]")
    return flags


@pytest.mark.parametrize("point", ["host", "dev"])
def test_hash_table_wrap_filter(pkg, oracle, point):
    """An empty 95851-bit filter, 1024 slots: two distinct offsets of the batch hash to slot 1023,
    so one of them is stored at (1023 + 1) & 1023 = 0, and seq_mark's lookup follows it there."""
    m, k = 95851, 7
    keys = wrap_batch(WRAP_SEED_FILTER)
    assert wraps(oracle.indexes_many(*pkg.keys.pack(keys), m, k).reshape(-1).tolist(), 1024)
    again = keys[::2] + [b"x" + key for key in keys[1::2]]
    flags = filter_case(pkg, oracle, point, m, k, [keys, again], 1024)
    assert flags[0].sum() == 60 and 0 < flags[1].sum() < len(again)


@pytest.mark.parametrize("point", POINTS)
def test_hash_table_wrap_lua(pkg, point):
    m, k = 11027, 7
    keys = wrap_batch(WRAP_SEED_LUA)
    assert wraps([o for row in lua_probes(keys, m, k) for o in row], 1024)
    again = keys[::2] + [b"x" + key for key in keys[1::2]]
    flags = lua_case(pkg, point, (ENTRIES, PRECISION), [keys, again], 1024)
    assert flags[0].sum() == 60 and 0 < flags[1].sum() < len(again)


@pytest.mark.parametrize("point", ["host", "dev"])
def test_hash_table_half_full_filter(pkg, oracle, point):
    """64 keys of 8 probes, all 512 distinct and all 0-probes: 2 n k = 1024 slots, exactly half
    of them taken.  The batch again (no 0-probe at all), then half of it with new keys."""
    m, k = 1 << 20, 8
    keys = half_batch(HALF_SEED_FILTER)
    assert len(set(oracle.indexes_many(*pkg.keys.pack(keys), m, k).reshape(-1).tolist())) == 512
    flags = filter_case(pkg, oracle, point, m, k, [keys, keys, keys[:32] + half_batch(HALF_SEED_FILTER + 1)[:32]], 1024)
    assert flags[0].all() and not flags[1].any() and not flags[2][:32].any() and flags[2][32:].all()


@pytest.mark.parametrize("point", POINTS)
def test_hash_table_half_full_lua(pkg, point):
    m, k = L.layer_params(float(HALF_LUA[0]), HALF_LUA[1], 1)
    assert (m, k) == (997635, 8)
    keys = half_batch(HALF_SEED_LUA)
    assert len({o for row in lua_probes(keys, m, k) for o in row}) == 512
    flags = lua_case(pkg, point, HALF_LUA, [keys, keys, keys[:32] + half_batch(HALF_SEED_LUA + 1)[:32]], 1024)
    assert flags[0].all() and not flags[1].any() and not flags[2][:32].any() and flags[2][32:].all()


@pytest.mark.parametrize("point", ["host", "dev"])
def test_hash_table_lookup_walks_filter(pkg, oracle, point):
    """k = 1: a key's flag rests on its one probe, so a lookup that stops short of a displaced bit
    shows in the flag (with more probes another new bit of the key hides it).  512 keys, 448
    distinct and 64 of them again: 2 n k = 1024 slots; at least ten bits share their home slot
    with another and are stored further on."""
    m, k = 95851, 1
    keys = [b"d%d" % i for i in range(448)]
    keys = keys[:200] + keys[:64] + keys[200:]
    offsets = set(oracle.indexes_many(*pkg.keys.pack(keys), m, k).reshape(-1).tolist())
    homes = [mix64(o) & 1023 for o in offsets]
    assert len(homes) - len(set(homes)) >= 10
    flags = filter_case(pkg, oracle, point, m, k, [keys], 1024)
    assert not flags[0][200:264].any() and flags[0].sum() == len(offsets)


@pytest.mark.parametrize("point", ["host", "dev"])
def test_hash_form_k64_filter(pkg, oracle, point):
    """k = 64: the 0-probe mask's bit 63 (1ull << i).  300 keys, every key twice."""
    keys = k64_batch(300)
    flags = filter_case(pkg, oracle, point, (1 << 20) + 3, 64, [keys, keys[:100] + [b"y" + x for x in keys[:100]]],
                        65536)
    assert flags[0].sum() == 150 and flags[1].sum() >= 50


@pytest.mark.parametrize("point", POINTS)
def test_hash_form_k64_lua(pkg, point):
    """A Lua layer of 64 hashes: probe indices 1 .. 64."""
    assert L.layer_params(float(K64_LUA[0]), K64_LUA[1], 1) == (185001, 64)
    keys = k64_batch(200)
    flags = lua_case(pkg, point, K64_LUA, [keys, keys[:60] + [b"y" + x for x in keys[:60]]], 32768)
    assert flags[0].sum() == 100 and flags[1].sum() >= 30


# ---- d. the device cut kernels -----------------------------------------------------------------

SEEN = b"seen"
ALIGNS = (0, 1, 7, 15)

# n -> the indices of the new keys.  lua_cut_kernel gives each of its 1024 lanes ceil(n / 1024)
# bytes: one up to 1024 keys, 2 at 1025 (a last segment of 1 byte: index 1024), 4 at 3 * 1024 + 5
# (a last segment of 1 byte: index 3076), 5 at 5000 (the binned form; no short segment).
#   n <= 17           index 0, one inside, n - 1 (15 / 16 / 17: the count kernel's tail only, one whole
#                     vector, a vector and a tail byte when the buffer is aligned)
#   1024              index 0, 1, the middle, n - 1 (every segment is one byte)
#   1025              a segment's first byte (0), a segment's last byte (5, 1023), the short segment
#   3 * 1024 + 5      0, a first byte (4), a last byte (7), inside a segment (2049), the last whole
#                     segment's last byte (3075), the short segment (3076)
#   5000              0, a first byte (5), a last byte (9), inside (2502), n - 1
CUT_NEW = {15: (0, 5, 14), 16: (0, 12, 15), 17: (0, 8, 16), 1024: (0, 1, 511, 1023), 1025: (0, 5, 1023, 1024),
           3 * 1024 + 5: (0, 4, 7, 2049, 3075, 3076), 5000: (0, 5, 9, 2502, 4999)}
# exactly `room` new keys with repeats after the last (the cut is not at n), and one fewer than
# `room` (lua_cut_kernel's "the whole chunk stays" branch)
CUT_EXTRA = [(17, (3, 9), 2), (17, (3, 9), 3), (1025, (2, 1000), 2), (1025, (2, 1000), 3), (5000, (7, 2503), 2)]


def _cut_cases():
    out = []
    for n, new_at in CUT_NEW.items():
        for room in range(1, len(new_at) + 1):
            for a in (ALIGNS if n <= 17 else (ALIGNS[(room - 1) % 4],)):
                out.append((n, new_at, room, a))
    for i, (n, new_at, room) in enumerate(CUT_EXTRA):
        out.append((n, new_at, room, ALIGNS[(i + 1) % 4]))
    # the handle's own flag buffer (d_per_key_new = 0)
    out += [(15, CUT_NEW[15], 2, None), (1025, CUT_NEW[1025], 3, None), (5000, CUT_NEW[5000], 2, None)]
    return out


CUT_CASES = _cut_cases()


def cut_at(n, new_at, room):
    """Where the chunk is cut: after the room-th new key, or not at all."""
    return new_at[room - 1] + 1 if room <= len(new_at) else n


def test_cut_cases_cover_every_head():
    """The call goes on past the cut at d_per_key_new + take, so the second chunk's
    lua_count_kernel starts (align + take) mod 16 into a vector: its head is -(align + take) mod
    16 bytes.  As (n, align, take) the cases above give head 0: (15, 15, 1); 1: (3077, 7, 8);
    2: (16, 1, 13); 3: (15, 7, 6); 4: (16, 15, 13); 5: (17, 1, 10); 6: (17, 1, 9); 7: (17, 0, 9);
    8: (15, 7, 1); 9: (15, 1, 6); 10: (15, 0, 6); 11: (15, 15, 6); 12: (16, 7, 13); 13: (1024, 1, 2);
    14: (15, 1, 1); 15: (15, 0, 1).  The first chunk's heads are 0, 15, 9 and 1 (alignments 0, 1, 7,
    15), and many second chunks are shorter than one vector."""
    heads, first, short = set(), set(), 0
    for n, new_at, room, a in CUT_CASES:
        take = cut_at(n, new_at, room)
        if a is None:
            continue
        first.add(-a % 16)
        if take < n:
            heads.add(-(a + take) % 16)
            short += n - take < 16
    assert heads == set(range(16)) and first == {0, 15, 9, 1} and short >= 8


@functools.lru_cache(maxsize=None)
def cut_script(n, new_at, room):
    """(Script, count before, flags, chunks) of the batch: SEEN (already in layer 1) n times, with
    new distinct keys at ``new_at``, on a filter whose layer 1 has room for ``room`` more keys."""
    import pkgload
    pkg = pkgload.load()
    sc = Script(pkg)
    assert sc.add([SEEN]).all()
    sc.count = count0 = capacity(ENTRIES, 1) - room
    keys = [SEEN] * n
    for i in new_at:
        keys[i] = b"new-%d-%d" % (n, i)
    want = sc.add(keys)
    return sc, count0, keys, want, chunks_of(pkg, sc, count0, want)


@pytest.mark.parametrize("n,new_at,room,align", CUT_CASES,
                         ids=["%d-%s-room%d-%s" % (n, "_".join(map(str, p)), r, "own" if a is None else "a%d" % a)
                              for n, p, r, a in CUT_CASES])
def test_device_cut_kernels(pkg, n, new_at, room, align):
    """bf_lua_insert_many_dev with the cut right after the room-th new key: lua_count_kernel's sum
    (head, vectors, tail) and lua_cut_kernel's index, then the rest of the batch one layer up."""
    sc, count0, keys, want, chunks = cut_script(n, new_at, room)
    take = cut_at(n, new_at, room)
    # before the GPU is touched: the flags up to the cut are 1 exactly at the new keys
    mark = np.zeros(n, bool)
    mark[list(new_at)] = True
    np.testing.assert_array_equal(want[:take], mark[:take])
    rest = [(2, n - take, n - take)] if take < n else []
    assert shape(chunks) == [(1, n, take)] + rest and chunks[0]["cut"] and chunks[0]["room"] == room
    assert [c["form"] for c in chunks] == [lua_form(c["layer"], c["cn"]) for c in chunks]
    assert chunks[0]["form"] == (HASH if n <= 17 else BINNED if n == 5000 else DIRECT)
    with pkg.LuaFilter(ENTRIES, PRECISION) as f:
        f.profile(True)
        assert f.insert_many(*pkg.keys.pack([SEEN]))[0].all()
        f.count = count0
        if align is None:
            d = Dev(*pkg.keys.pack(keys))
            f.insert_many_dev(d.kp, d.op, n, 0, stream=0)
            torch.cuda.synchronize()
        else:
            got, _ = lua_insert(pkg, f, "dev", keys, align)
            np.testing.assert_array_equal(got, want)
        assert f.count == sc.count == count0 + int(want.sum())
        for layer in (1, 2, 3):
            assert f.export_layer(layer) == sc.string(layer), layer
        probe = [SEEN] + [keys[i] for i in new_at] + fresh_keys("d", 8)
        np.testing.assert_array_equal(f.include_many(*pkg.keys.pack(probe)).astype(bool), sc.check(probe))
        ran(f.profile_read(), "lua_count[L1]", *["lua_seq_mark[L%d]" % c["layer"] for c in chunks])


@pytest.mark.parametrize("align", ALIGNS)
def test_device_count_of_one_key(pkg, align):
    """n = 1 (room >= n: no cut to look for): lua_count_kernel on a single byte, which is its head
    or its tail; the key fills layer 1, so the next call starts on layer 2."""
    sc = Script(pkg)
    sc.count = count0 = capacity(ENTRIES, 1) - 1
    keys, more = [b"one"], [b"one", b"two"]
    want = sc.add(keys)
    assert shape(chunks_of(pkg, sc, count0, want)) == [(1, 1, 1)] and want.all()
    want_more = sc.add(more)
    assert shape(chunks_of(pkg, sc, count0 + 1, want_more)) == [(2, 2, 2)] and want_more.all()
    with pkg.LuaFilter(ENTRIES, PRECISION) as f:
        f.count = count0
        np.testing.assert_array_equal(lua_insert(pkg, f, "dev", keys, align)[0], want)
        np.testing.assert_array_equal(lua_insert(pkg, f, "dev", more, align)[0], want_more)
        check_state(pkg, f, sc, more + fresh_keys("e", 4))
