"""BITCOUNT, filter-to-filter BITOP and the size estimate on the device (bf_stats.hip,
include/bfhip.h: bf_bitcount, bf_bitop, bf_bitcount_op, bf_estimate_count).

The checker for every count is NumPy on the exported bytes: a 256-entry popcount table
indexed by the bytes, summed.  Strings after a BITOP are checked against the oracle's bitsets
combined with NumPy."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 65536
POP = np.array([bin(i).count("1") for i in range(256)], np.uint64)
M_BIG, K = 9_585_058, 6            # 1M keys @ 1 %: 18 full dirty blocks and a partial one
NORTH_STAR = (9_585_058_377, 6)    # 1B keys @ 1 %


def popcount(data) -> int:
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)
    return int(POP[a].sum())


def rand_keys(rng, n, lo=1, hi=24):
    lens = rng.integers(lo, hi + 1, size=n)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    return rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs


def padded(s: bytes, size: int) -> np.ndarray:
    a = np.zeros(size, np.uint8)
    a[: len(s)] = np.frombuffer(s, np.uint8)
    return a


def trimmed(a: np.ndarray) -> bytes:
    nz = np.flatnonzero(a)
    return a[: int(nz[-1]) + 1].tobytes() if len(nz) else b""


def blocks_of(ranges):
    out = set()
    for off, n in ranges:
        assert off % BLOCK == 0 and n > 0
        out.update(range(off // BLOCK, (off + n - 1) // BLOCK + 1))
    return out


def prefixed_decimal_keys(pkg, seed: int, n: int):
    """The keys "%d-%d" % (seed, j), j < n, packed without a Python loop over the keys."""
    prefix = np.frombuffer(("%d-" % seed).encode(), np.uint8)
    dbuf, doffs = pkg.keys.pack_decimal(np.arange(n, dtype=np.int64))
    dlen = np.diff(doffs.astype(np.int64))
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(dlen + len(prefix), out=offs[1:])
    out = np.empty(int(offs[-1]), np.uint8)
    starts = offs[:-1].astype(np.int64)
    for i, ch in enumerate(prefix):
        out[starts + i] = ch
    key_of = np.repeat(np.arange(n, dtype=np.int64), dlen)
    out[np.arange(len(dbuf), dtype=np.int64) + len(prefix) * (key_of + 1)] = dbuf
    return out, offs


def test_prefixed_decimal_keys_are_the_formatted_strings(pkg):
    buf, offs = prefixed_decimal_keys(pkg, 17, 1234)
    want = pkg.keys.pack(["%d-%d" % (17, j) for j in range(1234)])
    assert np.array_equal(buf, want[0]) and np.array_equal(offs, want[1])


class Loaded:
    """A filter with keys in it, its oracle bitset and its exported string, computed once."""

    def __init__(self, pkg, oracle, m, k, n, seed, **kw):
        self.m, self.k = m, k
        self.keys = rand_keys(np.random.default_rng(seed), n)
        self.f = pkg.Filter(m, k, **kw)
        self.f.insert_many(*self.keys)
        self.s = self.f.export_redis()
        self.bits = None
        if oracle is not None:
            self.bits = oracle.new_bitset(m, k)
            oracle.insert_many(self.bits, m, k, *self.keys)


@pytest.fixture(scope="module")
def big(pkg, oracle):
    """m = 9,585,058 with 400,000 keys: read-only for every test that uses it."""
    ld = Loaded(pkg, oracle, M_BIG, K, 400_000, 11)
    yield ld
    ld.f.close()


# ---- bitcount -------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(9585, 700), (95851, 8000)])
def test_bitcount_whole_string_small(pkg, m, n):
    """9,585 bits: device_bytes = 1,280, less than one vector pass of one workgroup."""
    with pkg.Filter(m, K) as f:
        assert f.bitcount() == 0 and f.bitcount_bytes() == 0            # an empty filter
        f.insert_many(*rand_keys(np.random.default_rng(m), n))
        s = f.export_redis()
        assert f.bitcount() == f.bitcount_bytes() == popcount(s) > 0
        assert f.export_redis() == s


def test_bitcount_whole_string_many_blocks(pkg, big):
    assert big.f.device_bytes > 18 * BLOCK and big.f.device_bytes % BLOCK != 0
    assert big.s == trimmed(big.bits)
    assert big.f.bitcount() == popcount(big.s)


def test_bitcount_md5_engine(pkg):
    with pkg.Filter(95851, K, flags=pkg.BF_FLAG_ENGINE_MD5) as f:
        f.insert_many(*rand_keys(np.random.default_rng(5), 5000))
        assert f.bitcount() == popcount(f.export_redis()) > 0


def test_bitcount_ranges(pkg, big):
    f, s = big.f, big.s
    full = padded(s, f.device_bytes)
    n = len(s)
    for start, ln in [(0, 0), (1, 1), (3, 5), (15, 17), (16, 16), (65_535, 2), (n - 1, 1), (n, 5),
                      (0, 2**64 - 1), (7, f.device_bytes), (f.device_bytes, 1), (2**64 - 1, 2**64 - 1)]:
        want = popcount(full[start:start + ln]) if start < len(full) else 0
        assert f.bitcount_bytes(start, ln) == want, (start, ln)
    # Redis's inclusive indices, negative ones from the end of the trimmed string
    assert f.bitcount(2, -3) == popcount(s[2:n - 2])
    assert f.bitcount(-1, -1) == popcount(s[-1:]) > 0
    assert f.bitcount(0, 0) == popcount(s[:1])
    assert f.bitcount(5, 4) == 0 and f.bitcount(-2, -5) == 0
    assert f.bitcount(-10**9, 10**9) == popcount(s)
    assert f.bitcount(n, n + 10) == 0


def test_bitcount_past_2_to_32(pkg):
    """2^29 + 3 bytes of 0xFF: 4,294,967,320 set bits, more than a 32-bit count holds."""
    nbytes = (1 << 29) + 3
    with pkg.Filter(*NORTH_STAR) as f:
        f.import_redis(bytes(np.full(nbytes, 0xFF, np.uint8)))
        assert f.bitcount() == 8 * nbytes == 4_294_967_320
        assert f.bitcount_bytes(1, nbytes) == 8 * (nbytes - 1)


def test_bitcount_dev_on_a_side_stream(pkg, big):
    torch = pytest.importorskip("torch")
    out = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    big.f.bitcount_dev(out.data_ptr(), stream=st.cuda_stream)
    big.f.bitcount_dev(out.data_ptr() + 8, 3, 70_000, stream=st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert int(got[0]) == big.f.bitcount() == popcount(big.s)
    assert int(got[1]) == big.f.bitcount_bytes(3, 70_000)


# ---- bitop ----------------------------------------------------------------------------------

def _check_or(pkg, oracle, m, n_a, n_b):
    a, b = Loaded(pkg, oracle, m, K, n_a, 21), Loaded(pkg, oracle, m, K, n_b, 22)
    try:
        a.f.track_dirty(True)
        b.f.track_dirty(True)
        want = oracle.redis_string(np.bitwise_or(a.bits, b.bits))
        assert want != a.s
        changed, set_bits = a.f.bitop("or", b.f)
        s1 = a.f.export_redis()
        assert s1 == want
        assert changed is True
        assert set_bits == popcount(want) == a.f.bitcount()
        # the dirty map is exact: the reported blocks ARE the blocks whose bytes differ
        ranges, rlen = a.f.dirty_ranges(clear=True)
        size = max(len(a.s), len(s1))
        diff = np.flatnonzero(padded(a.s, size) != padded(s1, size))
        assert rlen == len(s1)
        assert blocks_of(ranges) == set((diff // BLOCK).tolist())
        r = pkg.FakeRedis()
        if a.s:
            r.set("bf", a.s)
        for off, ln in ranges:
            r.setrange("bf", off, a.f.export_range(off, ln))
        assert (r.get("bf") or b"") == s1
        # the source is read only
        assert b.f.export_redis() == b.s and b.f.dirty_ranges()[0] == []
        # a second identical OR changes nothing
        assert a.f.bitop(pkg._lib.BF_BITOP_OR, b.f) == (False, set_bits)
        assert a.f.dirty_ranges()[0] == [] and a.f.export_redis() == s1
        return len(blocks_of(ranges)), -(-a.f.device_bytes // BLOCK)
    finally:
        a.f.close()
        b.f.close()


def test_bitop_or_one_partial_block(pkg, oracle):
    _check_or(pkg, oracle, 9585, 300, 200)


def test_bitop_or_many_blocks(pkg, oracle):
    marked, total = _check_or(pkg, oracle, M_BIG, 100_000, 50_000)
    assert marked == total == 19


def test_bitop_or_marks_only_changed_blocks(pkg, oracle):
    """Three keys into a filter of 19 blocks: the blocks they miss stay clean."""
    marked, total = _check_or(pkg, oracle, M_BIG, 100_000, 3)
    assert 0 < marked < total


def test_bitop_and(pkg, oracle):
    rng = np.random.default_rng(31)
    common, only_a, only_b = rand_keys(rng, 5), rand_keys(rng, 2000), rand_keys(rng, 700)
    with pkg.Filter(M_BIG, K) as a, pkg.Filter(M_BIG, K) as b, pkg.Filter(M_BIG, K) as c:
        for f, sets in ((a, (common, only_a)), (b, (common,)), (c, (common, only_b))):
            for ks in sets:
                f.insert_many(*ks)
        sa, sb, sc = a.export_redis(), b.export_redis(), c.export_redis()
        # keys in a only: its high bytes vanish from the result and the string shrinks
        a.track_dirty(True)
        changed, set_bits = a.bitop("and", b)
        size = max(len(sa), len(sb))
        want = trimmed(padded(sa, size) & padded(sb, size))
        assert want == sb and len(sb) < len(sa)
        assert a.export_redis() == want and a.redis_len() == len(want)
        assert changed is True and set_bits == popcount(want)
        assert all(off + ln <= len(want) for off, ln in a.dirty_ranges()[0])
        # nothing to remove: unchanged, and said so
        assert a.bitop("and", b) == (False, set_bits)
        assert a.export_redis() == want and b.export_redis() == sb
        # two overlapping filters, neither inside the other
        a.import_redis(sa)
        changed, set_bits = a.bitop("and", c)
        size = max(len(sa), len(sc))
        want = trimmed(padded(sa, size) & padded(sc, size))
        assert a.export_redis() == want
        assert changed == (want != sa) and changed is True
        assert set_bits == popcount(want) and c.export_redis() == sc


def test_bitcount_op(pkg, oracle, big):
    other = Loaded(pkg, None, M_BIG, K, 150_000, 41)
    try:
        big.f.track_dirty(True)
        other.f.track_dirty(True)
        size = max(len(big.s), len(other.s))
        x, y = padded(big.s, size), padded(other.s, size)
        assert big.f.bitcount_op("and", other.f) == popcount(x & y)
        assert big.f.bitcount_op("or", other.f) == popcount(x | y)
        assert big.f.bitcount_op("xor", other.f) == popcount(x ^ y) == other.f.bitcount_op("xor", big.f)
        assert big.f.bitcount_op("xor", big.f) == 0
        assert big.f.bitcount_op("and", big.f) == big.f.bitcount_op("or", big.f) == popcount(big.s)
        for ld in (big, other):
            assert ld.f.export_redis() == ld.s and ld.f.dirty_ranges()[0] == []
        with pkg.Filter(M_BIG, K) as twin:       # a replica that has not diverged
            twin.import_redis(big.s)
            assert big.f.bitcount_op("xor", twin) == 0
            twin.insert_many(*pkg.keys.pack(["one more key"]))
            assert 0 < big.f.bitcount_op("xor", twin) <= K
        with pytest.raises(pkg.ArgumentError, match="op must be"):
            big.f.bitcount_op(3, other.f)
    finally:
        big.f.track_dirty(False)
        other.f.close()


def test_shard_handles(pkg):
    kw = dict(shard_count=3, shard_index=1, shard_block_log2=12)
    rng = np.random.default_rng(51)
    with pkg.Filter(M_BIG, K, **kw) as a, pkg.Filter(M_BIG, K, **kw) as b:
        nbytes = a.local_bits // 8
        assert a.local_bits % 8 == 0 and 0 < nbytes <= a.device_bytes
        da = rng.integers(0, 256, nbytes, dtype=np.uint8) & rng.integers(0, 256, nbytes, dtype=np.uint8)
        db = rng.integers(0, 256, nbytes, dtype=np.uint8) & rng.integers(0, 256, nbytes, dtype=np.uint8)
        a.shard_import(da)
        b.shard_import(db)
        assert a.bitcount_bytes() == popcount(da)
        for start, ln in [(5, 1000), (4095, 4100), (nbytes - 3, 100), (0, nbytes)]:
            assert a.bitcount_bytes(start, ln) == popcount(da[start:start + ln]), (start, ln)
        assert a.bitcount_op("xor", b) == popcount(da ^ db)
        changed, set_bits = a.bitop("or", b)
        assert changed is True and set_bits == popcount(da | db)
        assert np.array_equal(a.shard_export(), da | db) and np.array_equal(b.shard_export(), db)
        changed, set_bits = a.bitop("and", b)
        assert changed is True and set_bits == popcount(db)
        assert np.array_equal(a.shard_export(), db)


def test_bitop_refusals(pkg):
    m = 95851
    shard = dict(shard_count=3, shard_block_log2=12)
    keys = pkg.keys.pack(["a", "b", "c"])
    with pkg.Filter(m, K) as dst, pkg.Filter(m, K) as good:
        dst.insert_many(*keys)
        before = dst.export_redis()
        cases = [
            (lambda: pkg.Filter(9585, K), "differ in m"),
            (lambda: pkg.Filter(m, 5), "differ in k"),
            (lambda: pkg.Filter(m, K, flags=pkg.BF_FLAG_ENGINE_MD5), "hash engine"),
            (lambda: pkg.Filter(m, K, shard_index=1, **shard), "shard_count"),
            (lambda: pkg.Filter(m, K, flags=pkg._lib.BF_FLAG_ENCODER), "encoder"),
            (lambda: pkg.Filter(m, K, devices=[0, 0]), "multi-device"),
        ]
        for make, field in cases:
            with make() as other:
                for call in (lambda: dst.bitop("or", other), lambda: dst.bitop("and", other),
                             lambda: dst.bitcount_op("xor", other), lambda: other.bitop("or", dst)):
                    with pytest.raises(pkg.ArgumentError, match=field):
                        call()
        with pytest.raises(pkg.ArgumentError, match="op must be"):
            dst.bitop("xor", good)                       # XOR only counts
        with pytest.raises(pkg.ArgumentError, match="op must be"):
            dst.bitop(7, good)
        assert dst.export_redis() == before and dst.bitcount() == popcount(before)
        assert dst.bitop("or", dst) == (False, popcount(before))       # dst == src: a no-op
        assert dst.bitop("or", good) == (False, popcount(before))      # an empty filter ORed in
        assert dst.export_redis() == before
    with pkg.Filter(m, K, shard_index=1, **shard) as s1, pkg.Filter(m, K, shard_index=2, **shard) as s2:
        s1.shard_import(np.full(16, 0x5A, np.uint8))
        with pytest.raises(pkg.ArgumentError, match="shard_index"):
            s1.bitop("or", s2)
        assert np.array_equal(s1.shard_export()[:17], np.array([0x5A] * 16 + [0], np.uint8))


@pytest.mark.parametrize("mode", ["replicated", "partitioned"])
def test_bitcount_multi_device(pkg, big, mode):
    with pkg.Filter(M_BIG, K, devices=[0, 0, 0], mode=mode) as f:
        assert f.bitcount() == 0
        f.insert_many(*big.keys)
        assert f.bitcount() == popcount(big.s)
        assert f.bitcount_bytes(0, (M_BIG + 7) // 8) == popcount(big.s)
        if mode == "partitioned":
            for start, ln in [(1, 2**64 - 1), (0, 100), (0, len(big.s) // 2)]:
                with pytest.raises(pkg.ArgumentError, match="whole string"):
                    f.bitcount_bytes(start, ln)
        else:
            assert f.bitcount_bytes(3, 70_000) == popcount(big.s[3:70_003])
        with pytest.raises(pkg.ArgumentError):
            f.bitcount_dev(8, stream=0)
        with pytest.raises(pkg.ArgumentError):
            f.bitop("or", big.f)


def test_bitop_waits_for_the_sources_stream(pkg, oracle):
    """src's insert runs on a torch side stream and is not waited for; dst's bitop goes to
    dst's own stream and must still see every bit (the launch waits on both handles)."""
    torch = pytest.importorskip("torch")
    n = 1 << 20
    buf, offs = pkg.keys.pack_decimal(np.random.default_rng(61).integers(0, 10**12, size=n))
    kb = torch.from_numpy(np.concatenate([buf, np.zeros(16, np.uint8)])).cuda()
    ko = torch.from_numpy(offs.view(np.int64)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pkg.Filter(M_BIG, K) as src, pkg.Filter(M_BIG, K) as dst:
        src.insert_many_dev(kb.data_ptr(), ko.data_ptr(), n, stream=side.cuda_stream)
        changed, set_bits = dst.bitop("or", src)
        got = dst.export_redis()
        torch.cuda.synchronize()
    bits = oracle.new_bitset(M_BIG, K)
    oracle.insert_many(bits, M_BIG, K, buf, offs)
    want = oracle.redis_string(bits)
    assert got == want and changed is True and set_bits == popcount(want)


# ---- the estimate, end to end ---------------------------------------------------------------

@pytest.mark.parametrize("m,k,log2n,seed", [NORTH_STAR + (22, 1), (19_170_116_755, 13, 21, 2)])
def test_estimate_from_the_device_count(pkg, oracle, m, k, log2n, seed):
    """n distinct keys, X from bitcount(): the density-aware estimate is within four standard
    errors of the collision count, 4 sqrt(n k - X) / k, and the textbook formula is not (CPU
    prototype: bounds 125 and 45 keys, errors 26 and 14 against 356 and 147)."""
    n = 1 << log2n
    buf, offs = prefixed_decimal_keys(pkg, seed, n)
    with pkg.Filter(m, k) as f:
        first = 1 << 18                      # the count itself, against the oracle's offsets
        f.insert_many(buf[: int(offs[first])], offs[: first + 1])
        idx = oracle.indexes_many(buf, offs[: first + 1], m, k)
        assert f.bitcount() == len(np.unique(idx))
        f.insert_many(buf, offs)
        x = f.bitcount()
    bound = 4.0 * math.sqrt(n * k - x) / k
    est = pkg._lib.estimate_count(m, k, x)
    text = -(m / k) * math.log(1.0 - x / m)
    print("m=%d k=%d n=%d X=%d bound=%.1f estimate error=%.1f textbook error=%.1f"
          % (m, k, n, x, bound, est - n, text - n))
    assert abs(est - n) <= bound, (est - n, bound)
    assert abs(text - n) > bound, (text - n, bound)


# ---- driver and facade ----------------------------------------------------------------------

def _bound(n, k, x):
    return 4.0 * math.sqrt(max(n * k - x, 0)) / k


def test_driver_merge_and_sizes(pkg, oracle):
    r = pkg.FakeRedis()
    mk = lambda name, **kw: pkg.Bloomfilter(size=1000, error_rate=0.01, driver="hip", redis=r, key_name=name, **kw)
    a, b = mk("stats:a"), mk("stats:b")
    m, k = a.options["bits"], a.options["hashes"]
    assert (m, k) == (9585, 6)
    ka = ["key-%d" % i for i in range(600)]
    kb = ["key-%d" % i for i in range(300, 900)]
    a.insert_many(ka)
    b.insert_many(kb)
    b_before = r.get("stats:b")
    xa, xb = a.count_bits(), b.count_bits()
    assert xa == popcount(r.get("stats:a")) and xb == popcount(b_before)
    assert a.fill_ratio() == xa / m
    # sizes before the merge: neither filter is modified by asking
    xu = a.driver.filter.bitcount_op("or", b.driver.filter)
    inter, union = a.intersection_size(b), a.union_size(b)
    budget = _bound(600, k, xa) + _bound(600, k, xb) + _bound(900, k, xu)
    assert abs(union - 900) <= _bound(900, k, xu), (union, _bound(900, k, xu))
    assert abs(inter - 300) <= budget, "intersection %.1f, bound %.1f" % (inter, budget)
    assert r.get("stats:a") == a.driver.to_redis_string() and r.get("stats:b") == b_before
    # merge: BITOP OR on the device, the changed blocks written through
    assert a.merge(b) is True
    bits = oracle.new_bitset(m, k)
    oracle.insert_many(bits, m, k, *pkg.keys.pack(ka + kb))
    assert r.get("stats:a") == oracle.redis_string(bits) == a.driver.to_redis_string()
    assert r.get("stats:b") == b_before
    assert a.include_many(ka + kb).all()
    assert a.count_bits() == xu
    sent = r.bytes_in
    assert a.merge(b) is False and r.bytes_in == sent
    # EXPIRE only when something changed (ruby.rb:62)
    assert r.ttl("stats:a") == -1
    assert a.merge(b, 60) is False and r.ttl("stats:a") == -1
    b.insert("a key nobody has seen")
    assert a.merge(b, 60) is True and 0 < r.ttl("stats:a") <= 60
    assert r.get("stats:a") == a.driver.to_redis_string()
    # refusals
    other = pkg.Bloomfilter(size=2000, error_rate=0.01, driver="hip", redis=r, key_name="stats:c")
    for call in (lambda: a.merge(other), lambda: a.union_size(other), lambda: a.intersection_size(other)):
        with pytest.raises(pkg.ArgumentError, match="bits"):
            call()
    md5 = pkg.Bloomfilter(size=1000, error_rate=0.01, driver="hip-test", redis=r, key_name="stats:d")
    with pytest.raises(pkg.ArgumentError, match="hash engine"):
        a.merge(md5)
    lua = pkg.Bloomfilter(size=1000, error_rate=0.01, driver="hip-lua", redis=r, key_name="stats:e")
    for call in (lua.count_bits, lua.estimated_size, lambda: lua.merge(a)):
        with pytest.raises(NotImplementedError, match="hip-lua"):
            call()


@pytest.mark.parametrize("driver", ["hip", "hip-test"])
def test_driver_estimated_size(pkg, driver):
    """1000 distinct keys in 9,585 bits: within 2 % (the collision bound from the run's own X
    is printed and stated on failure)."""
    bf = pkg.Bloomfilter(size=1000, error_rate=0.01, driver=driver, redis=pkg.FakeRedis(), key_name="stats:n")
    bf.insert_many(["member-%d" % i for i in range(1000)])
    x, k = bf.count_bits(), bf.options["hashes"]
    est = bf.estimated_size()
    print("%s: X=%d estimate=%.1f collision bound=%.1f" % (driver, x, est, _bound(1000, k, x)))
    assert abs(est - 1000) <= 20, "estimate %.1f; four-sigma collision bound %.1f keys" % (est, _bound(1000, k, x))
    assert est == pkg._lib.estimate_count(bf.options["bits"], k, x, bf.driver._flags)
