"""Filter banks (bf_bank_*, include/bfhip.h): many filters of one (m, k) behind one handle.

Every comparison is bit-exact against the oracle.  A bank is modelled as one
``COracle.new_bitset(m, k)`` per touched filter; the keys routed to a filter are inserted in
batch order.  Per key the bank's ``key_flipped`` is not the sequential flag (which of several
racing keys wins a bit is unspecified), but its OR over a filter's keys is "this filter's
string changed", which the oracle's ``any_new`` gives per filter.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, K = 9585, 6          # 1000 keys @ 1 %: 1,199 bytes, stride 1,280
STR_BYTES = 1199


def pack(keys):
    offs = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        np.cumsum([len(x) for x in keys], out=offs[1:])
    buf = np.frombuffer(b"".join(keys) + b"\0" * 16, np.uint8).copy()
    return buf, offs


def make_keys(n, seed, lo=0, hi=70):
    """n distinct keys of lo..hi bytes (some beyond 55: the two-block SHA-1 path)."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.randint(lo, hi)
        tag = ("%d:%d:" % (seed, i)).encode()
        out.append((tag + bytes(rng.getrandbits(8) for _ in range(max(ln - len(tag), 0))))[:max(ln, 0)] if ln else b"")
    return out


class Model:
    """The oracle's view of a bank: one bitset per touched filter."""

    def __init__(self, oracle, m, k):
        self.o, self.m, self.k, self.bits = oracle, m, k, {}

    def _bits(self, f):
        if f not in self.bits:
            self.bits[f] = self.o.new_bitset(self.m, self.k)
        return self.bits[f]

    def insert(self, keys, ids):
        """Insert in batch order; returns the set of filters whose string changed."""
        by = {}
        for key, f in zip(keys, ids):
            by.setdefault(int(f), []).append(key)
        changed = set()
        for f, ks in by.items():
            buf, offs = pack(ks)
            any_new, _ = self.o.insert_many(self._bits(f), self.m, self.k, buf, offs)
            if any_new:
                changed.add(f)
        return changed

    def include(self, keys, ids):
        out = np.zeros(len(keys), np.uint8)
        for j, (key, f) in enumerate(zip(keys, ids)):
            if int(f) in self.bits:
                buf, offs = pack([key])
                out[j] = self.o.include_many(self.bits[int(f)], self.m, self.k, buf, offs)[0]
        return out

    def string(self, f):
        return self.o.redis_string(self.bits[f]) if f in self.bits else b""

    def popcount(self, f):
        return int(np.unpackbits(self.bits[f]).sum()) if f in self.bits else 0


def changed_of(ids, flipped):
    return set(np.asarray(ids)[np.asarray(flipped) != 0].tolist())


def check_bank(bank, model, n_filters):
    strings = bank.export_redis()
    assert len(strings) == n_filters
    for f in range(n_filters):
        assert strings[f] == model.string(f), "filter %d" % f
    _, lens = bank.export_filters()
    assert lens.tolist() == [len(model.string(f)) for f in range(n_filters)]


def run_parity(pkg, oracle, m, k, n_filters, n, n_probe, seed):
    rng = np.random.default_rng(seed)
    keys = make_keys(n, seed)
    ids = rng.integers(0, n_filters, n).astype(np.uint32)
    model = Model(oracle, m, k)
    with pkg.FilterBank(m, k, n_filters) as bank:
        assert (bank.m, bank.k, bank.n_filters) == (m, k, n_filters)
        assert bank.stride == pkg._lib.bank_stride(m) and bank.device_bytes == bank.stride * n_filters
        buf, offs = pack(keys)
        flipped = bank.insert_many(buf, offs, ids)
        assert changed_of(ids, flipped) == model.insert(keys, ids)
        check_bank(bank, model, n_filters)
        probe = keys[: n_probe // 2] + make_keys(n_probe - n_probe // 2, seed + 1)
        pids = rng.integers(0, n_filters, len(probe)).astype(np.uint32)
        pids[: n_probe // 4] = ids[: n_probe // 4]          # a quarter are members of their filter
        pb, po = pack(probe)
        got = bank.include_many(pb, po, pids)
        assert np.array_equal(got, model.include(probe, pids))
        assert got[: n_probe // 4].all()
        # the same insert again: no string changes, nothing is reported
        again = bank.insert_many(buf, offs, ids)
        assert not again.any()
        check_bank(bank, model, n_filters)


def test_parity_small_m(pkg, oracle):
    run_parity(pkg, oracle, M, K, 37, 1000, 2000, seed=11)


@pytest.mark.parametrize("m,k", [(7, 1), (33, 3), (958_506, 7)])
def test_other_modulo_paths_and_word_edges(pkg, oracle, m, k):
    """m = 7 and 33: the conditional-subtraction-free float64 path and a filter inside one or two
    words; m >= 2^17: the float32 quotient path."""
    run_parity(pkg, oracle, m, k, 5, 600, 600, seed=m)


def test_isolation(pkg, oracle):
    keys = make_keys(500, 3)
    ids = np.full(len(keys), 3, np.uint32)
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    with pkg.FilterBank(M, K, 7) as bank:
        bank.insert_many(*pack(keys), ids)
        buf, lens = bank.export_filters()
        assert buf.shape == (7, 1280)
        assert lens[2] == 0 and lens[4] == 0 and not buf[2].any() and not buf[4].any()
        assert buf[3, : int(lens[3])].tobytes() == model.string(3)
        assert not buf[3, STR_BYTES:].any()                    # the pad to the stride stays zero
        assert bank.bitcount().tolist() == [model.popcount(f) for f in range(7)]
        assert bank.bitcount(np.array([3, 0, 3], np.uint32)).tolist() == [model.popcount(3), 0, model.popcount(3)]


def test_one_filter_behaves_as_a_filter(pkg):
    keys = make_keys(1500, 4)
    buf, offs = pack(keys)
    with pkg.FilterBank(M, K, 1) as bank, pkg.Filter(M, K) as f:
        bank.insert_many(buf, offs, np.zeros(len(keys), np.uint32))
        f.insert_many(buf, offs)
        assert bank.export_redis()[0] == f.export_redis()
        assert int(bank.bitcount()[0]) == f.bitcount()


def test_contention_and_tiles(pkg, oracle):
    keys = make_keys(4096, 5, lo=4, hi=30)
    buf, offs = pack(keys)
    # every key races into one filter of 64
    model = Model(oracle, M, K)
    ids = np.full(4096, 41, np.uint32)
    with pkg.FilterBank(M, K, 64) as bank:
        flipped = bank.insert_many(buf, offs, ids)
        assert changed_of(ids, flipped) == model.insert(keys, ids) == {41}
        check_bank(bank, model, 64)
        # every bit was reported by exactly one key: at most one report per set bit
        assert 0 < int(flipped.sum()) <= model.popcount(41)
        assert bank.include_many(buf, offs, ids).all()
    # every key alone in its own filter
    perm = np.random.default_rng(5).permutation(4096).astype(np.uint32)
    model = Model(oracle, M, K)
    with pkg.FilterBank(M, K, 4096) as bank:
        flipped = bank.insert_many(buf, offs, perm)
        assert flipped.all()                                    # nobody to race with
        model.insert(keys, perm)
        check_bank(bank, model, 4096)
        assert bank.include_many(buf, offs, perm).all()
        # n = 0 and n = 1
        e = np.zeros(0, np.uint32)
        assert len(bank.insert_many(np.zeros(0, np.uint8), np.zeros(1, np.uint64), e)) == 0
        assert len(bank.include_many(np.zeros(0, np.uint8), np.zeros(1, np.uint64), e)) == 0
        one = bank.insert_many(*pack([b"just one"]), np.array([7], np.uint32))
        assert one.tolist() == [1]
        model.insert([b"just one"], [7])
        assert bank.export_redis(np.array([7], np.uint32))[0] == model.string(7)
    # a tile whose key bytes exceed the 16 KiB LDS stage: keys are read from global memory
    long_keys = make_keys(256, 6, lo=200, hi=200)
    lids = (np.arange(256) % 3).astype(np.uint32)
    model = Model(oracle, M, K)
    with pkg.FilterBank(M, K, 3) as bank:
        flipped = bank.insert_many(*pack(long_keys), lids)
        assert changed_of(lids, flipped) == model.insert(long_keys, lids)
        check_bank(bank, model, 3)
        assert bank.include_many(*pack(long_keys), lids).all()


def test_past_4_gib(pkg, oracle):
    """3,400,000 filters of stride 1,280 are 4.35 GB: ids 3,355,442..3,355,444 straddle byte 2^32."""
    n_filters = 3_400_000
    targets = [0, 3_355_442, 3_355_443, 3_355_444, 3_399_999]
    assert targets[1] * 1280 < 1 << 32 <= targets[3] * 1280
    keys = make_keys(400, 7)
    ids = np.array([targets[j % 5] for j in range(len(keys))], np.uint32)
    model = Model(oracle, M, K)
    with pkg.FilterBank(M, K, n_filters) as bank:
        assert bank.device_bytes == 4_352_000_000
        flipped = bank.insert_many(*pack(keys), ids)
        assert changed_of(ids, flipped) == model.insert(keys, ids) == set(targets)
        look = targets + [3_355_441, 3_355_445]
        strings = bank.export_redis(np.array(look, np.uint32))
        assert strings == [model.string(f) for f in targets] + [b"", b""]
        assert bank.include_many(*pack(keys), ids).all()
        counts = bank.bitcount()
        assert len(counts) == n_filters
        assert int(counts.sum()) == sum(model.popcount(f) for f in targets)
        assert [int(counts[f]) for f in targets] == [model.popcount(f) for f in targets]


def dev_batch(keys, ids):
    buf, offs = pack(keys)
    return (torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64).copy()).cuda(),
            torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).cuda())


def test_bad_ids_on_the_device_path(pkg, oracle):
    n_filters = 9
    keys = make_keys(700, 8)
    ids = np.random.default_rng(8).integers(0, n_filters, len(keys)).astype(np.uint32)
    bad = [5, 300, 699]
    ids[5], ids[300], ids[699] = n_filters, 0xFFFFFFFF, n_filters + 1
    good = [j for j in range(len(keys)) if j not in bad]
    model = Model(oracle, M, K)
    want_changed = model.insert([keys[j] for j in good], ids[good])
    dk, do, di = dev_batch(keys, ids)
    with pkg.FilterBank(M, K, n_filters) as bank:
        # the host form refuses the batch, names the first bad key and changes nothing
        with pytest.raises(pkg.ArgumentError, match=r"key 5: filter id 9 "):
            bank.insert_many(*pack(keys), ids)
        with pytest.raises(pkg.ArgumentError, match=r"key 5: filter id 9 "):
            bank.include_many(*pack(keys), ids)
        assert bank.export_redis() == [b""] * n_filters
        bank.sync()
        # the device form skips exactly the bad keys
        flipped = torch.full((len(keys),), 7, dtype=torch.uint8, device="cuda")
        out = torch.full((len(keys),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bank.insert_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(keys), flipped.data_ptr())
        bank.include_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(keys), out.data_ptr())
        with pytest.raises(pkg.ArgumentError, match="filter id at or past n_filters"):
            bank.sync()
        bank.sync()                                            # reported once
        fl, got = flipped.cpu().numpy(), out.cpu().numpy()
        assert fl[bad].tolist() == [0, 0, 0] and got[bad].tolist() == [0, 0, 0]
        assert got[good].all()
        assert changed_of(ids[good], fl[good]) == want_changed
        check_bank(bank, model, n_filters)
        # a later call still runs
        assert bank.include_many(*pack([keys[0]]), ids[:1]).tolist() == [1]
        # a listed filter out of range: refused by the host form, skipped by the device form
        with pytest.raises(pkg.ArgumentError, match=r"ids\[1\] = 9 "):
            bank.bitcount(np.array([0, 9], np.uint32))
        with pytest.raises(pkg.ArgumentError, match=r"ids\[1\] = 9 "):
            bank.clear(np.array([0, 9], np.uint32))
        check_bank(bank, model, n_filters)


def test_clear_import_export(pkg, oracle):
    n_filters = 11
    keys = make_keys(900, 9)
    ids = np.random.default_rng(9).integers(0, n_filters, len(keys)).astype(np.uint32)
    a = Model(oracle, M, K)
    a.insert(keys, ids)
    more = make_keys(500, 10)
    mids = np.random.default_rng(10).integers(0, n_filters, len(more)).astype(np.uint32)
    b = Model(oracle, M, K)
    b.insert(more, mids)
    every = np.arange(n_filters, dtype=np.uint32)
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(keys), ids)
        bank.clear(np.array([2, 9, 10], np.uint32))
        want = [b"" if f in (2, 9, 10) else a.string(f) for f in range(n_filters)]
        assert bank.export_redis() == want
        # import(REPLACE) of oracle strings, then export, is the identity (shorter strings
        # replace longer ones: the tail is zero-filled)
        sa = [a.string(f) for f in range(n_filters)]
        bank.import_redis(every, sa)
        assert bank.export_redis() == sa
        short = [s[: len(s) // 3].rstrip(b"\0") for s in sa]
        bank.import_redis(every[::-1].copy(), short[::-1])
        assert bank.export_redis() == short
        bank.import_redis(None, sa)
        # import(OR) is the oracle's union
        bank.import_redis(every, [b.string(f) for f in range(n_filters)], pkg.BF_IMPORT_OR)
        union = Model(oracle, M, K)
        union.insert(keys, ids)
        union.insert(more, mids)
        check_bank(bank, union, n_filters)
        assert bank.include_many(*pack(more), mids).all()
        # refusals change nothing: a bit at m (byte 1198, mask 0x80 >> (9585 & 7)), a string too long
        before = bank.export_redis()
        at_m = bytes(STR_BYTES - 1) + bytes([0x80 >> (M & 7)])
        for mode in (pkg.BF_IMPORT_REPLACE, pkg.BF_IMPORT_OR):
            with pytest.raises(pkg.ArgumentError, match="BF_ERANGE.*string 1 sets bits at offsets >= 9585"):
                bank.import_redis(np.array([4, 6], np.uint32), [b"\xff" * 20, at_m], mode)
            with pytest.raises(pkg.ArgumentError, match="BF_ERANGE.*string 1 of 1200 bytes"):
                bank.import_redis(np.array([4, 6], np.uint32), [b"\xff" * 20, bytes(STR_BYTES) + b"\x01"], mode)
        assert bank.export_redis() == before
        last_bit = bytes(STR_BYTES - 1) + bytes([0x80 >> ((M - 1) & 7)])     # bit m - 1 is fine
        bank.import_redis(np.array([6], np.uint32), [last_bit])
        assert bank.export_redis(np.array([6], np.uint32)) == [last_bit]
        bank.clear()
        assert bank.export_redis() == [b""] * n_filters and not bank.bitcount().any()


def test_dev_calls_on_a_side_stream(pkg, oracle):
    """An insert then an include? on the caller's stream, ordered after the bank's own earlier
    host call (which ran on the bank's stream), and the per-filter counts after both."""
    n_filters = 6
    first, second = make_keys(300, 12), make_keys(513, 13)
    ids1 = (np.arange(len(first)) % n_filters).astype(np.uint32)
    ids2 = np.random.default_rng(13).integers(0, n_filters, len(second)).astype(np.uint32)
    model = Model(oracle, M, K)
    model.insert(first, ids1)
    model.insert(second, ids2)
    dk, do, di = dev_batch(second, ids2)
    pk, po, pi = dev_batch(first + second, np.concatenate([ids1, ids2]))
    n_all = len(first) + len(second)
    out = torch.zeros(n_all, dtype=torch.uint8, device="cuda")
    counts = torch.full((n_filters,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(first), ids1)
        bank.insert_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(second), stream=st.cuda_stream)
        bank.include_many_dev(pk.data_ptr(), po.data_ptr(), pi.data_ptr(), n_all, out.data_ptr(),
                              stream=st.cuda_stream)
        bank.bitcount_dev(counts.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        bank.sync()
        assert out.cpu().numpy().all()
        assert counts.cpu().numpy().tolist() == [model.popcount(f) for f in range(n_filters)]
        check_bank(bank, model, n_filters)
        # clear_dev of a device list on the side stream, then the host call sees it
        gone = torch.from_numpy(np.array([1, 4], np.int32)).cuda()
        bank.clear_dev(gone.data_ptr(), 2, stream=st.cuda_stream)
        assert bank.bitcount().tolist() == [0 if f in (1, 4) else model.popcount(f) for f in range(n_filters)]


# ---- the BloomfilterBank facade with FakeRedis ---------------------------------------------

NAMES = ["tenant:%d" % i for i in range(5)]


def test_driver_with_fakeredis(pkg, O):
    now = [1000.0]
    clock = lambda: now[0]   # noqa: E731
    r, r_ruby = pkg.FakeRedis(clock=clock), pkg.FakeRedis()
    m, k = pkg.Bloomfilter.optimal_m(1000, 0.01), 6
    # a key name the ruby driver wrote before the bank attaches
    pre = O.RubyDriverRestatement({"bits": m, "hashes": k, "key_name": NAMES[4], "redis": r})
    early = ["early%d" % i for i in range(40)]
    for key in early:
        pre.insert(key)
    r.expire(NAMES[4], 500)
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, clock=clock)
    assert (bank.options["bits"], bank.options["hashes"]) == (m, k) == (9585, 6)
    assert bank.include_many([NAMES[4]] * 40, early).all()      # readable after attach
    assert not bank.include_many([NAMES[0]] * 40, early).any()

    rubies = {n: O.RubyDriverRestatement({"bits": m, "hashes": k, "key_name": n, "redis": r_ruby}) for n in NAMES}
    for key in early:
        rubies[NAMES[4]].insert(key)
    rng = random.Random(14)
    keys = ["k%d" % i for i in range(600)] + list(range(100))
    names = [NAMES[rng.randrange(5)] for _ in keys]
    r.calls.clear()
    changed = bank.insert_many(names, keys, expire=90)
    assert changed == set(NAMES)
    for n, key in zip(names, keys):
        rubies[n].insert(key)
    for n in NAMES:
        assert r.get(n) == r_ruby.get(n), n                     # byte for byte the ruby driver's string
        assert r.ttl(n) == 90
    assert sorted(c for c in r.calls if c[0] in ("SETRANGE", "EXPIRE")) == \
        sorted([("SETRANGE", n) for n in NAMES] + [("EXPIRE", n) for n in NAMES])

    # only the names whose string changed are written and EXPIREd
    r.calls.clear()
    again = [NAMES[0]] * 3 + [NAMES[1]] * 2 + [NAMES[2]]
    again_keys = [k_ for n, k_ in zip(names, keys) if n == NAMES[0]][:3] + ["new-a", "new-b"] + \
                 [k_ for n, k_ in zip(names, keys) if n == NAMES[2]][:1]
    assert bank.insert_many(again, again_keys, expire=30) == {NAMES[1]}
    assert [c for c in r.calls if c[0] != "GET"] == [("SETRANGE", NAMES[1]), ("EXPIRE", NAMES[1])]
    assert r.ttl(NAMES[1]) == 30 and r.ttl(NAMES[0]) == 90
    for key in ("new-a", "new-b"):
        rubies[NAMES[1]].insert(key)
    assert r.get(NAMES[1]) == r_ruby.get(NAMES[1])

    # the per-name view and the statistics
    view = bank[NAMES[1]]
    for x in ("new-a", "nope", keys[0]):
        assert view.include(x) == bank.include(NAMES[1], x) == rubies[NAMES[1]].include(x)
    assert view.insert("via-view") is True and bank.include(NAMES[1], "via-view")
    bits = bank.count_bits()
    assert bits.tolist() == [int(np.unpackbits(np.frombuffer(r.get(n), np.uint8)).sum()) for n in NAMES]
    est = bank.estimated_sizes()
    assert [est[i] == pkg._lib.estimate_count(m, k, int(bits[i])) for i in range(5)] == [True] * 5
    with pytest.raises(pkg.ArgumentError, match="unknown key name"):
        bank.include("nobody", "x")

    # clear(name) DELs one key and leaves the rest
    r.calls.clear()
    bank.clear(NAMES[2])
    assert r.calls == [("DEL", NAMES[2])]
    assert r.get(NAMES[2]) is None and r.get(NAMES[3]) == r_ruby.get(NAMES[3])
    assert bank.count_bits()[2] == 0 and bank.count_bits()[3] == bits[3]

    # a per-name deadline clears only that filter: tenant:1 has 30 s, the others 90 s
    now[0] += 31
    assert bank.include(NAMES[1], "new-a") is False
    assert r.get(NAMES[1]) is None
    assert bank.include(NAMES[0], again_keys[0]) is True
    assert bank.count_bits().tolist() == [int(bits[0]), 0, 0, int(bits[3]), int(bits[4])]
    bank.close()


def test_driver_manual_sync(pkg):
    r = pkg.FakeRedis()
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, sync="manual")
    r.calls.clear()
    assert bank.insert_many([NAMES[0], NAMES[3]], ["a", "b"], expire=60) == {NAMES[0], NAMES[3]}
    assert r.calls == []                                        # manual: Redis untouched
    sent = bank.flush()
    assert sent == len(r.get(NAMES[0])) + len(r.get(NAMES[3])) and r.get(NAMES[1]) is None
    assert bank.flush() == 0
    # reload takes Redis's word: a key that vanished empties its filter
    r.delete(NAMES[0])
    bank.reload([NAMES[0]])
    assert bank.include(NAMES[0], "a") is False and bank.include(NAMES[3], "b") is True
    bank.close()
