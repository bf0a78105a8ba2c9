"""The bank's cross query (bf_bank_include_across*, include/bfhip.h): one key tested against
many filters of a bank, the key hashed once.

Every mask is checked bit for bit twice: against the oracle (one ``COracle.new_bitset`` per touched
filter, an untouched filter answers 0) and against ``FilterBank.include_many`` on the crossed
product of the same keys and ids, the only way to ask before.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, K = 9585, 6          # 1000 keys @ 1 %: stride 1,280


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
        tag = ("x%d:%d:" % (seed, i)).encode()
        out.append((tag + bytes(rng.getrandbits(8) for _ in range(max(ln - len(tag), 0))))[:ln])
    return out


class Model:
    """The oracle's view of a bank: one bitset per touched filter."""

    def __init__(self, oracle, m, k):
        self.o, self.m, self.k, self.bits = oracle, m, k, {}

    def insert(self, keys, ids):
        by = {}
        for key, f in zip(keys, ids):
            by.setdefault(int(f), []).append(key)
        for f, ks in by.items():
            if f not in self.bits:
                self.bits[f] = self.o.new_bitset(self.m, self.k)
            self.o.insert_many(self.bits[f], self.m, self.k, *pack(ks))

    def across(self, keys, ids):
        """(n, count) bool: include? of every key in every listed filter."""
        buf, offs = pack(keys)
        cols, out = {}, np.zeros((len(keys), len(ids)), bool)
        for i, f in enumerate(int(x) for x in ids):
            if f not in cols:
                cols[f] = (self.o.include_many(self.bits[f], self.m, self.k, buf, offs).astype(bool)
                           if f in self.bits else np.zeros(len(keys), bool))
            out[:, i] = cols[f]
        return out


def crossed(bank, keys, ids):
    """The same answers through include_many: every key repeated once per listed filter."""
    rep = [key for key in keys for _ in range(len(ids))]
    got = bank.include_many(*pack(rep), np.tile(np.asarray(ids, np.uint32), len(keys)))
    return got.reshape(len(keys), len(ids)).astype(bool)


def check(bank, model, keys, ids):
    """include_across(keys, ids) against both references; ids=None lists every filter."""
    listed = np.arange(bank.n_filters, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
    got = bank.include_across(*pack(keys), ids)
    assert got.shape == (len(keys), len(listed)) and got.dtype == bool
    want = model.across(keys, listed)
    assert np.array_equal(got, want), "differs from the oracle at %s" % (np.argwhere(got != want)[:5].tolist(),)
    assert np.array_equal(got, crossed(bank, keys, listed)), "differs from the crossed include_many"
    return got


def raw_mask(bank, keys, ids, count, fill=0xAB):
    """The C call itself on a pre-filled mask: (status, mask rows as the call left them)."""
    buf, offs = pack(keys)
    row = bank.across_row_bytes(count)
    mask = np.full((len(keys), row), fill, np.uint8)
    a = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    rc = bank._lib.bf_bank_include_across(bank.handle, buf.ctypes.data, offs.ctypes.data, len(keys),
                                          None if a is None else a.ctypes.data, count, mask.ctypes.data)
    return rc, mask


# ---- word and tile edges: one bank and one oracle matrix shared by the cases ------------------

N_FILTERS, N_QUERY = 130, 257


@pytest.fixture(scope="module")
def edges(pkg, oracle):
    rng = np.random.default_rng(21)
    keys = make_keys(600, 21)
    ids = rng.integers(0, N_FILTERS, len(keys)).astype(np.uint32)
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    # every other query key is a member of some filter
    fresh = make_keys(N_QUERY, 22)
    query = [keys[j] if j % 2 == 0 else fresh[j] for j in range(N_QUERY)]
    want = model.across(query, np.arange(N_FILTERS))
    assert all(want[j, ids[j]] for j in range(0, N_QUERY, 2))
    with pkg.FilterBank(M, K, N_FILTERS) as bank:
        bank.insert_many(*pack(keys), ids)
        yield bank, model, query, want


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129, 130])
def test_word_edges(edges, count):
    bank, model, query, want = edges
    keys = query[:120]
    ids = None if count == N_FILTERS else np.arange(count, dtype=np.uint32)     # a prefix list
    got = check(bank, model, keys, ids)
    assert np.array_equal(got, want[:120, :count])
    assert not got.all() and (count < 63 or got.any())
    # the mask itself: every word written, the spare bits of the last word 0
    rc, mask = raw_mask(bank, keys, ids, count, fill=0xFF)
    assert rc == 0 and mask.shape == (120, 8 * ((count + 63) // 64))
    bits = np.unpackbits(mask, axis=1, bitorder="little").astype(bool)
    assert np.array_equal(bits[:, :count], want[:120, :count])
    assert not bits[:, count:].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_tile_edges(edges, n):
    bank, model, query, want = edges
    got = check(bank, model, query[:n], np.arange(65, dtype=np.uint32))
    assert np.array_equal(got, want[:n, :65])


def test_list_semantics(edges):
    """A shuffled subset with repeats: every entry is answered on its own."""
    bank, model, query, want = edges
    rng = np.random.default_rng(23)
    ids = rng.permutation(N_FILTERS)[:70].astype(np.uint32)
    ids = np.concatenate([ids, ids[:25], ids[3:4].repeat(5)])
    rng.shuffle(ids)
    assert len(ids) == 100 and len(set(ids.tolist())) == 70
    got = check(bank, model, query, ids)
    assert np.array_equal(got, want[:, ids])                       # column i is filter ids[i]'s straight column
    first = {}
    for i, f in enumerate(ids.tolist()):
        assert np.array_equal(got[:, i], got[:, first.setdefault(f, i)])


# ---- the other modulo paths, and k past one round of probes ------------------------------------

@pytest.mark.parametrize("m,k", [(7, 1), (33, 3), (958_506, 7), (958_506, 13)])
def test_modulo_paths_and_later_rounds(pkg, oracle, m, k):
    n_filters = 9
    keys = make_keys(64, m + k)
    model = Model(oracle, m, k)
    with pkg.FilterBank(m, k, n_filters) as bank:
        for j, key in enumerate(keys[:48]):                        # 16 keys are in no filter
            fs = np.array([j % n_filters, (7 * j + 3) % n_filters], np.uint32)
            bank.insert_many(*pack([key, key]), fs)
            model.insert([key, key], fs)
        got = check(bank, model, keys, None)
        for j in range(48):
            assert got[j, j % n_filters] and got[j, (7 * j + 3) % n_filters]   # passed every probe
        if m > 1000:
            assert not got[48:].any() and int(got.sum()) < 3 * 48


# ---- many list chunks, few keys ---------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_many_chunks_few_keys(pkg, oracle, n):
    """5,000 filters are 79 list chunks of 64 entries for one tile of 1 or 3 keys."""
    n_filters = 5000
    homes = [[0, 63, 64, 127, 128, 129, 255, 256, 257, 1000, 2500, 4095, 4096, 4999],
             [1, 62, 65, 126, 130, 383, 384, 2047, 2048, 4998],
             []]
    keys = make_keys(3, 24, lo=5, hi=40)
    model = Model(oracle, M, K)
    with pkg.FilterBank(M, K, n_filters) as bank:
        for key, fs in zip(keys, homes):
            if fs:
                bank.insert_many(*pack([key] * len(fs)), np.array(fs, np.uint32))
                model.insert([key] * len(fs), fs)
        got = check(bank, model, keys[:n], None)
        for j in range(n):
            assert set(homes[j]) <= set(np.flatnonzero(got[j]).tolist())
            assert not got[j, [f for f in range(n_filters) if f not in model.bits]].any()
        rc, mask = raw_mask(bank, keys[:n], None, n_filters, fill=0xFF)
        assert rc == 0 and mask.shape == (n, 632)
        assert not np.unpackbits(mask, axis=1, bitorder="little")[:, n_filters:].any()


def test_tile_past_the_lds_stage(pkg, oracle):
    """256 keys of 100 bytes are 25,600 bytes: past the 16 KiB stage, read from global memory."""
    keys = make_keys(256, 25, lo=100, hi=100)
    ids = (np.arange(256) % 5).astype(np.uint32)
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    with pkg.FilterBank(M, K, 7) as bank:
        bank.insert_many(*pack(keys), ids)
        got = check(bank, model, keys, None)
        assert all(got[j, j % 5] for j in range(256)) and not got[:, 5:].any()


def test_past_4_gib(pkg, oracle):
    """3,400,000 filters of stride 1,280 are 4.35 GB: ids 3,355,442..3,355,444 straddle byte 2^32."""
    n_filters = 3_400_000
    targets = [0, 3_355_442, 3_355_443, 3_355_444, 3_399_999]
    assert targets[1] * 1280 < 1 << 32 <= targets[3] * 1280
    keys = make_keys(100, 26)
    ids = np.array([targets[j % 5] for j in range(len(keys))], np.uint32)
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    look = np.array(targets + [3_355_441, 3_355_445, 1, 3_399_998], np.uint32)
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(keys), ids)
        got = check(bank, model, keys, look)
        for j in range(len(keys)):
            assert got[j, j % 5]
        assert not got[:, 5:].any()                                # the neighbours are empty filters


# ---- the device path --------------------------------------------------------------------------

def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()).cuda()


def unpack_dev(d_mask, n, count):
    row = 8 * ((count + 63) // 64)
    bits = np.unpackbits(d_mask.cpu().numpy().reshape(n, row), axis=1, bitorder="little").astype(bool)
    assert not bits[:, count:].any()
    return bits[:, :count]


def test_device_path_guards(pkg, oracle):
    n_filters = 9
    keys = make_keys(300, 27)
    ids = np.random.default_rng(27).integers(0, n_filters, len(keys)).astype(np.uint32)
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    query = keys[:150] + make_keys(150, 28)
    buf, offs = pack(query)
    dk, do = dev(buf), dev(offs)
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(keys), ids)
        # one list entry at n_filters: its column is 0, every other column is right
        listed = np.array([3, 0, 8, n_filters, 5, 3], np.uint32)
        di = dev(listed)
        d_mask = torch.full((len(query) * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bank.include_across_dev(dk.data_ptr(), do.data_ptr(), len(query), d_mask.data_ptr(), di.data_ptr(), len(listed))
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*filter id at or past n_filters"):
            bank.sync()
        bank.sync()                                                # reported once
        got = unpack_dev(d_mask, len(query), len(listed))
        good = [0, 1, 2, 4, 5]
        assert not got[:, 3].any()
        assert np.array_equal(got[:, good], model.across(query, listed[good]))
        assert np.array_equal(got[:, good], crossed(bank, query, listed[good]))
        # key 40's offsets run backwards: its row is zeros, every other row is what its offsets name
        bad = offs.copy()
        bad[41] = bad[40] - 2
        named = [b"" if j == 40 else buf[int(bad[j]):int(bad[j + 1])].tobytes() for j in range(len(query))]
        db = dev(bad)
        d_mask.fill_(0xFF)
        torch.cuda.synchronize()
        bank.include_across_dev(dk.data_ptr(), db.data_ptr(), len(query), d_mask.data_ptr())   # d_ids = 0: every filter
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*inconsistent key offsets"):
            bank.sync()
        bank.sync()
        got = unpack_dev(d_mask.view(-1)[: len(query) * 8], len(query), n_filters)
        want = model.across(named, np.arange(n_filters))
        want[40] = False
        assert np.array_equal(got, want)
        assert want[:40].any() and want[41:150].any()
        # NULL and misaligned device pointers are refused before any launch
        for args in ((0, do.data_ptr(), d_mask.data_ptr()), (dk.data_ptr(), 0, d_mask.data_ptr()),
                     (dk.data_ptr(), do.data_ptr(), 0), (dk.data_ptr(), do.data_ptr() + 4, d_mask.data_ptr()),
                     (dk.data_ptr(), do.data_ptr(), d_mask.data_ptr() + 4)):
            with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*device pointer"):
                bank.include_across_dev(args[0], args[1], len(query), args[2])
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*count must be n_filters"):
            bank.include_across_dev(dk.data_ptr(), do.data_ptr(), len(query), d_mask.data_ptr(), count=n_filters - 1)
        bank.sync()


def test_side_stream_then_host_form(pkg, oracle):
    """An insert and a cross query on the caller's stream, then the host form on the bank's own
    stream with no synchronisation between: it sees the insert."""
    n_filters = 70
    first, second = make_keys(200, 29), make_keys(300, 30)
    ids1 = (np.arange(len(first)) % n_filters).astype(np.uint32)
    ids2 = np.random.default_rng(30).integers(0, n_filters, len(second)).astype(np.uint32)
    model = Model(oracle, M, K)
    model.insert(first, ids1)
    model.insert(second, ids2)
    query = first[:60] + second[:60] + make_keys(20, 31)
    b2, o2 = pack(second)
    dk, do, di = dev(b2), dev(o2), dev(ids2)
    qb, qo = pack(query)
    dq, dqo = dev(qb), dev(qo)
    d_mask = torch.full((len(query) * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(first), ids1)
        bank.insert_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(second), stream=st.cuda_stream)
        bank.include_across_dev(dq.data_ptr(), dqo.data_ptr(), len(query), d_mask.data_ptr(), stream=st.cuda_stream)
        host = bank.include_across(qb, qo)
        st.synchronize()
        bank.sync()
        want = model.across(query, np.arange(n_filters))
        assert np.array_equal(host, want)
        assert np.array_equal(unpack_dev(d_mask, len(query), n_filters), want)
        assert all(want[60 + j, ids2[j]] for j in range(60))


# ---- the host form's refusals -----------------------------------------------------------------

def test_host_refusals(pkg):
    n_filters = 9
    keys = make_keys(20, 32, lo=3, hi=20)
    buf, offs = pack(keys)
    E = pkg._lib.BF_EINVAL
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(buf, offs, np.zeros(len(keys), np.uint32))
        lib, h = bank._lib, bank.handle
        before = bank.export_redis()

        def refused(offsets, ids, count, what):
            mask = np.full((len(keys), 8), 0xAB, np.uint8)
            a = None if ids is None else np.ascontiguousarray(ids, np.uint32)
            rc = lib.bf_bank_include_across(h, buf.ctypes.data, offsets.ctypes.data, len(keys),
                                            None if a is None else a.ctypes.data, count, mask.ctypes.data)
            assert rc == E and (mask == 0xAB).all()
            assert what in lib.bf_bank_last_error(h).decode(), lib.bf_bank_last_error(h)

        refused(offs, None, n_filters - 1, "count must be n_filters = 9, got 8")
        refused(offs, None, n_filters + 1, "count must be n_filters = 9, got 10")
        refused(offs, [0, 8, 9, 77], 4, "ids[2] = 9 is not below n_filters = 9")
        backwards = offs.copy()
        backwards[6] = backwards[5] - 1
        refused(backwards, None, n_filters, "key 5: offsets must be non-decreasing")
        past = offs.copy()
        past[3] = past[-1] + 1
        refused(past, [1, 2], 2, "key 2: offsets must be non-decreasing")
        assert lib.bf_bank_include_across(h, buf.ctypes.data, offs.ctypes.data, len(keys), None, n_filters, None) == E
        assert b"mask is NULL" in lib.bf_bank_last_error(h)
        assert lib.bf_bank_include_across(h, buf.ctypes.data, None, len(keys), None, n_filters, None) == E
        # the wrapper raises the same refusals
        with pytest.raises(pkg.ArgumentError, match=r"BF_EINVAL.*ids\[1\] = 4000000000 "):
            bank.include_across(buf, offs, np.array([0, 4_000_000_000], np.uint64))
        with pytest.raises(pkg.ArgumentError, match=r"BF_EINVAL.*key 5: offsets"):
            bank.include_across(buf, backwards)
        # n == 0 and count == 0 write nothing and are no error
        mask = np.full(64, 0xAB, np.uint8)
        assert lib.bf_bank_include_across(h, buf.ctypes.data, offs.ctypes.data, 0, None, n_filters, mask.ctypes.data) == 0
        ids = np.zeros(1, np.uint32)
        assert lib.bf_bank_include_across(h, buf.ctypes.data, offs.ctypes.data, len(keys), ids.ctypes.data, 0,
                                          mask.ctypes.data) == 0
        assert (mask == 0xAB).all()
        assert bank.include_across(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).shape == (0, n_filters)
        assert bank.include_across(buf, offs, np.zeros(0, np.uint32)).shape == (len(keys), 0)
        bank.sync()                                                # nothing was launched, nothing to report
        assert bank.export_redis() == before
        assert bank.include_across(buf, offs)[:, 0].all()          # a later call runs


# ---- the BloomfilterBank facade with FakeRedis -------------------------------------------------

NAMES = ["day:%d" % i for i in range(6)]


def test_facade_which_and_include_across(pkg):
    now = [1000.0]
    r = pkg.FakeRedis(clock=lambda: now[0])
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, clock=lambda: now[0])
    bank.insert_many([NAMES[4], NAMES[1], NAMES[5]], ["url-a"] * 3)
    bank.insert_many([NAMES[2]], ["url-b"])
    bank.insert_many([NAMES[3], NAMES[0]], ["url-a", 77], expire=30)      # day:3 and day:0 vanish after 30 s
    r.calls.clear()
    assert bank.which("url-a") == [NAMES[1], NAMES[3], NAMES[4], NAMES[5]]          # key_names order
    assert bank.which("url-a", [NAMES[5], NAMES[2], NAMES[1], NAMES[5]]) == [NAMES[5], NAMES[1], NAMES[5]]
    assert bank.which(77) == [NAMES[0]] and bank.which("url-c") == []
    keys = ["url-a", "url-b", "url-c", 77]
    got = bank.include_across(keys)
    assert got.shape == (4, 6) and got.dtype == bool
    for i, name in enumerate(NAMES):
        assert got[:, i].tolist() == [bank.include(name, key) for key in keys], name
    sub = [NAMES[2], NAMES[0], NAMES[2]]
    assert np.array_equal(bank.include_across(keys, sub), got[:, [2, 0, 2]])
    assert r.calls == []                                           # reads: Redis is not touched
    with pytest.raises(pkg.ArgumentError, match="unknown key name"):
        bank.which("url-a", ["nobody"])
    # a name past its deadline reads as empty
    now[0] += 31
    assert bank.which("url-a") == [NAMES[1], NAMES[4], NAMES[5]]
    assert not bank.include_across([77, "url-a"], [NAMES[0], NAMES[3]]).any()
    assert bank.which("url-b") == [NAMES[2]]
    bank.close()
