"""The bank's insert with exact sequential per-key flags (bf_bank_insert_many_seq*,
include/bfhip.h): first-seen dedup over a mixed batch of (filter id, key) pairs.

The model is ``test_gpu_bank.Model`` extended: one ``COracle.new_bitset(m, k)`` per touched
filter, each filter's keys inserted in batch order with ``insert_many(..., per_key=True)`` and
the flags scattered back to their batch positions.  Every comparison is exact: the flags array
equals the oracle's and ``export_redis()`` equals the oracle's strings.  "Both forms" runs the
hash table and the one-word-per-bit table through ``BFHIP_BANK_SEQ_FORM``, which ``FilterBank``
reads when it creates a bank (and applies with bf_bank_set_seq_form).
"""
import random

import numpy as np
import pytest

from test_gpu_bank import M, K, Model, check_bank, dev_batch, make_keys, pack
from test_gpu_seq_hash_and_cut import half_batch, wraps

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = ["hash", "direct"]


class SeqModel(Model):
    def insert_seq(self, keys, ids):
        """Insert in batch order; returns the sequential flag of every key (uint8)."""
        by = {}
        for j, f in enumerate(ids):
            by.setdefault(int(f), []).append(j)
        flags = np.zeros(len(keys), np.uint8)
        for f, js in by.items():
            buf, offs = pack([keys[j] for j in js])
            _, pk = self.o.insert_many(self._bits(f), self.m, self.k, buf, offs, per_key=True)
            flags[js] = pk
        return flags


def make_bank(pkg, monkeypatch, form, m, k, n_filters, **kw):
    """A bank whose sequential insert is forced to ``form`` (None: the bank's own choice)."""
    if form is None:
        monkeypatch.delenv("BFHIP_BANK_SEQ_FORM", raising=False)
    else:
        monkeypatch.setenv("BFHIP_BANK_SEQ_FORM", form)
    bank = pkg.FilterBank(m, k, n_filters, **kw)
    if form is not None:
        assert bank.seq_plan(1000)[0] is (form == "direct")     # every bank of these tests is below 2^28 bits
    return bank


def seq_and_check(bank, model, keys, ids, n_filters):
    got = bank.insert_many_seq(*pack(keys), np.asarray(ids, np.uint32))
    want = model.insert_seq(keys, ids)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    check_bank(bank, model, n_filters)
    return got


# ---- parity -------------------------------------------------------------------------------------

def dedup_batch(seed, n_filters):
    """1,000 pairs: 850 keys of 0-70 bytes with random ids, 100 copies of earlier (id, key) pairs
    and 50 earlier keys sent to another filter, each placed after its source.  The sources are
    keys long enough to carry their whole tag, so no other key of the batch equals them."""
    rng = random.Random(seed)
    base = make_keys(850, seed)
    ids = np.random.default_rng(seed).integers(0, n_filters, len(base)).tolist()
    items = [(float(i), base[i], ids[i], "base") for i in range(len(base))]
    long_enough = [i for i in range(700) if len(base[i]) >= 12]
    src = rng.sample(long_enough, 150)
    for s in src[:100]:
        items.append((rng.uniform(s + 0.5, len(base)), base[s], ids[s], "copy"))
    for s in src[100:]:
        other = (ids[s] + 1 + rng.randrange(n_filters - 1)) % n_filters
        items.append((rng.uniform(s + 0.5, len(base)), base[s], other, "cross"))
    items.sort(key=lambda t: t[0])
    keys = [t[1] for t in items]
    out_ids = np.array([t[2] for t in items], np.uint32)
    kind = np.array([t[3] for t in items])
    return keys, out_ids, kind


@pytest.mark.parametrize("pre", [False, True], ids=["empty", "half-inserted"])
@pytest.mark.parametrize("form", FORMS)
def test_parity_with_duplicates(pkg, oracle, monkeypatch, form, pre):
    n_filters = 37
    keys, ids, kind = dedup_batch(41, n_filters)
    assert len(keys) == 1000 and (kind == "copy").sum() == 100 and (kind == "cross").sum() == 50
    assert min(map(len, keys)) == 0 and max(map(len, keys)) > 55      # both SHA-1 block paths
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, form, M, K, n_filters) as bank:
        if pre:                                                       # a plain insert of half the keys first
            bank.insert_many(*pack(keys[:500]), ids[:500])
            model.insert(keys[:500], ids[:500])
        flags = seq_and_check(bank, model, keys, ids, n_filters)
        assert not flags[kind == "copy"].any()                        # the same pair again: not new
        cross = kind == "cross"
        if pre:
            assert not flags[:500].any()                              # !flag is include?-before-insert
            cross &= np.arange(len(keys)) >= 500
        assert cross.sum() >= 25 and flags[cross].all()               # the same key in another filter: new there
        assert flags.any()
        # the OR of the flags over a filter's keys is "this filter's string changed"
        again = bank.insert_many_seq(*pack(keys), ids)
        assert not again.any()
        check_bank(bank, model, n_filters)


# ---- dense collisions ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(7, 1), (33, 3), (958_506, 7)])
@pytest.mark.parametrize("form", FORMS)
def test_modulo_paths_and_word_edges(pkg, oracle, monkeypatch, form, m, k):
    """The three modulo paths and filters inside one or two words.  At m = 7 and 33 almost every
    flag is 0: which few are 1 is the point."""
    n_filters = 5
    keys = make_keys(600, m)
    ids = np.random.default_rng(m).integers(0, n_filters, len(keys)).astype(np.uint32)
    model = SeqModel(oracle, m, k)
    with make_bank(pkg, monkeypatch, form, m, k, n_filters) as bank:
        flags = seq_and_check(bank, model, keys, ids, n_filters)
        if m <= 33:
            assert 0 < int(flags.sum()) <= n_filters * m
        assert not bank.insert_many_seq(*pack(keys), ids).any()
        check_bank(bank, model, n_filters)


@pytest.mark.parametrize("form", FORMS)
def test_one_full_filter_and_one_key_per_filter(pkg, oracle, monkeypatch, form):
    keys = make_keys(4096, 5, lo=4, hi=30)
    # every key into ONE filter of 64: it fills up, so many late keys are not new
    ids = np.full(len(keys), 41, np.uint32)
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, form, M, K, 64) as bank:
        flags = seq_and_check(bank, model, keys, ids, 64)
        late = flags[-1024:]
        assert 0 < int(late.sum()) < len(late)
    # one key into each of 4,096 filters: every one is new
    perm = np.random.default_rng(5).permutation(4096).astype(np.uint32)
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, form, M, K, 4096) as bank:
        flags = seq_and_check(bank, model, keys, perm, 4096)
        assert flags.all()


# ---- agreement with a single filter ----------------------------------------------------------------

def test_one_filter_bank_is_a_filter(pkg, monkeypatch):
    keys = make_keys(1900, 6) + make_keys(100, 6)                    # the last 100 repeat the first
    buf, offs = pack(keys)
    with make_bank(pkg, monkeypatch, None, M, K, 1) as bank, pkg.Filter(M, K) as f:
        got = bank.insert_many_seq(buf, offs, np.zeros(len(keys), np.uint32))
        _, want = f.insert_many(buf, offs, per_key_new=True)
        assert np.array_equal(got, want)
        assert got[:100].any() and not got[1900:].any()
        assert bank.export_redis()[0] == f.export_redis()


# ---- chunk edges --------------------------------------------------------------------------------

def test_chunk_edges(pkg, oracle, monkeypatch):
    n_filters = 8
    keys = make_keys(1000, 7, lo=12)
    ids = np.random.default_rng(7).integers(0, n_filters, len(keys)).astype(np.uint32)
    keys[256], ids[256] = keys[255], ids[255]                         # one pair on both sides of a chunk edge
    keys[700], ids[700] = keys[100], ids[100]                         # ... and three chunks apart
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, n_filters, batch_keys=256) as cut, \
            make_bank(pkg, monkeypatch, None, M, K, n_filters) as whole:
        flags = seq_and_check(cut, model, keys, ids, n_filters)
        assert np.array_equal(flags, whole.insert_many_seq(*pack(keys), ids))
        assert flags[[255, 256]].tolist() == [1, 0] and flags[[100, 700]].tolist() == [1, 0]
        assert cut.export_redis() == whole.export_redis()


@pytest.mark.parametrize("form", FORMS)
def test_tiny_batches_and_a_tile_past_the_stage(pkg, oracle, monkeypatch, form):
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, form, M, K, 9) as bank:
        none = bank.insert_many_seq(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
        assert none.dtype == np.uint8 and len(none) == 0
        assert bank.export_redis() == [b""] * 9
        assert seq_and_check(bank, model, [b"just one"], [7], 9).tolist() == [1]
        assert seq_and_check(bank, model, [b"just one"], [7], 9).tolist() == [0]
        assert seq_and_check(bank, model, [b"just one"], [6], 9).tolist() == [1]
        # a tile whose key bytes exceed the 16 KiB LDS stage: keys are read from global memory
        long_keys = make_keys(256, 8, lo=200, hi=200)
        long_keys[200] = long_keys[3]
        lids = (np.arange(256) % 3).astype(np.uint32)
        lids[200] = lids[3]
        flags = seq_and_check(bank, model, long_keys, lids, 9)
        assert flags[3] == 1 and flags[200] == 0


# ---- 64-bit addressing ----------------------------------------------------------------------------

def test_past_4_gib(pkg, oracle, monkeypatch):
    """3,400,000 filters of stride 1,280 are 4.35 GB: filter 3,355,443 straddles byte 2^32, and a
    bit's bank-wide number (the hash table's key) passes 2^35 there."""
    n_filters = 3_400_000
    straddle = 3_355_443
    assert straddle * 1280 < 1 << 32 < (straddle + 1) * 1280
    targets = list(range(straddle - 3, straddle + 4)) + [0, n_filters - 1]
    keys = make_keys(2000, 9, lo=12)
    ids = np.array([targets[j % len(targets)] for j in range(len(keys))], np.uint32)
    below, above = 9 * 20 + 1, 9 * 20 + 5                             # ids straddle - 2 and straddle + 2
    assert ids[below] == straddle - 2 and ids[above] == straddle + 2
    for first, dup in ((below, 1500), (above, 1501)):
        keys[dup], ids[dup] = keys[first], ids[first]
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, n_filters) as bank:
        assert bank.device_bytes == 4_352_000_000
        direct, chunk, scratch = bank.seq_plan(len(keys))
        assert direct is False and chunk == len(keys)                 # a word per bit would be 139 GB
        assert scratch == 32768 * 12 + 32000 + 16128                  # 2nk = 24,000 -> 2^15 slots; digests; masks
        got = bank.insert_many_seq(*pack(keys), ids)
        assert np.array_equal(got, model.insert_seq(keys, ids))
        assert got[[below, above]].tolist() == [1, 1] and got[[1500, 1501]].tolist() == [0, 0]
        look = targets + [straddle - 4, straddle + 4]
        assert bank.export_redis(np.array(look, np.uint32)) == [model.string(f) for f in targets] + [b"", b""]
        assert int(bank.bitcount().sum()) == sum(model.popcount(f) for f in targets)


# ---- the device path ------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_dev_form_on_a_side_stream(pkg, oracle, monkeypatch, form):
    n_filters = 6
    first, second = make_keys(300, 12), make_keys(513, 13) + make_keys(40, 12)
    ids1 = (np.arange(len(first)) % n_filters).astype(np.uint32)
    ids2 = np.random.default_rng(13).integers(0, n_filters, len(second)).astype(np.uint32)
    ids2[513:] = ids1[:40]                                            # pairs the host call before it inserted
    model = SeqModel(oracle, M, K)
    model.insert(first, ids1)
    want = model.insert_seq(second, ids2)
    dk, do, di = dev_batch(second, ids2)
    flags = torch.full((len(second),), 7, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with make_bank(pkg, monkeypatch, form, M, K, n_filters) as bank, \
            make_bank(pkg, monkeypatch, form, M, K, n_filters) as host, \
            make_bank(pkg, monkeypatch, form, M, K, n_filters) as quiet:
        bank.insert_many(*pack(first), ids1)                          # on the bank's own stream
        bank.insert_many_seq_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(second), flags.data_ptr(),
                                 stream=st.cuda_stream)
        st.synchronize()
        bank.sync()
        got = flags.cpu().numpy()
        assert np.array_equal(got, want) and not got[513:].any()
        check_bank(bank, model, n_filters)
        # the host form gives the same
        host.insert_many(*pack(first), ids1)
        assert np.array_equal(host.insert_many_seq(*pack(second), ids2), got)
        assert host.export_redis() == bank.export_redis()
        # d_per_key_new = 0 (NULL) leaves the same bits
        quiet.insert_many(*pack(first), ids1)
        quiet.insert_many_seq_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(second), stream=st.cuda_stream)
        st.synchronize()
        quiet.sync()
        assert quiet.export_redis() == bank.export_redis()


@pytest.mark.parametrize("form", FORMS)
def test_dev_form_skips_bad_keys(pkg, oracle, monkeypatch, form):
    n_filters = 9
    keys = make_keys(700, 8, lo=8)
    ids = np.random.default_rng(8).integers(0, n_filters, len(keys)).astype(np.uint32)
    keys[600], ids[600] = keys[20], ids[20]                           # a duplicate pair among the valid keys
    ids[5], ids[300] = n_filters, 0xFFFFFFFF
    buf, offs = pack(keys)
    offs[41] = offs[40] - 2                                           # key 40's offsets run backwards
    bad = [5, 40, 300]
    good = [j for j in range(len(keys)) if j not in bad]
    named = [buf[int(offs[j]):int(offs[j + 1])].tobytes() for j in good]   # the keys the offsets name
    model = SeqModel(oracle, M, K)
    want = model.insert_seq(named, ids[good])
    dk = torch.from_numpy(buf).cuda()
    do = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    di = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    flags = torch.full((len(keys),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with make_bank(pkg, monkeypatch, form, M, K, n_filters) as bank:
        bank.insert_many_seq_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(keys), flags.data_ptr())
        with pytest.raises(pkg.ArgumentError, match="filter id at or past n_filters and inconsistent key offsets"):
            bank.sync()
        bank.sync()                                                   # reported once
        got = flags.cpu().numpy()
        assert got[bad].tolist() == [0, 0, 0]
        assert np.array_equal(got[good], want)
        assert got[20] == 1 and got[600] == 0
        check_bank(bank, model, n_filters)
        # NULL key, offset and id pointers are refused before any launch
        for args in ((0, do.data_ptr(), di.data_ptr()), (dk.data_ptr(), 0, di.data_ptr()),
                     (dk.data_ptr(), do.data_ptr(), 0)):
            with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*NULL device pointer"):
                bank.insert_many_seq_dev(*args, len(keys), flags.data_ptr())
        check_bank(bank, model, n_filters)


def test_dev_form_cuts_a_long_batch_itself(pkg, oracle, monkeypatch):
    """k = 64 bounds a chunk at 2^25 / 64 = 2^19 keys (32-bit indices into a table of at most 2^26
    slots): 2^19 + 300 keys in one ``_dev`` call are two chunks, the second handed ``d_offsets +
    2^19``.  A pair on both sides of the cut is new at its first place only."""
    m, k, n_filters = 958_506, 64, 16
    cut = 1 << 19
    n = cut + 300
    i = np.arange(n, dtype=np.int64)
    i[cut] = i[cut - 1]                                               # one pair across the cut
    i[cut + 200] = i[5]
    digits = (np.stack([(i // 10 ** p) % 10 for p in range(11, -1, -1)], axis=1) + 48).astype(np.uint8)
    ids = np.random.default_rng(16).integers(0, n_filters, n).astype(np.uint32)
    ids[cut], ids[cut + 200] = ids[cut - 1], ids[5]
    want = np.zeros(n, np.uint8)
    strings = []
    for f in range(n_filters):                                        # SeqModel.insert_seq on arrays
        js = np.flatnonzero(ids == f)
        bits = oracle.new_bitset(m, k)
        buf = np.concatenate([digits[js].reshape(-1), np.zeros(16, np.uint8)])
        _, want[js] = oracle.insert_many(bits, m, k, buf, np.arange(len(js) + 1, dtype=np.uint64) * 12, per_key=True)
        strings.append(oracle.redis_string(bits))
    dk = torch.from_numpy(np.concatenate([digits.reshape(-1), np.zeros(16, np.uint8)])).cuda()
    do = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 12
    di = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    flags = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with make_bank(pkg, monkeypatch, None, m, k, n_filters) as bank:
        assert bank.seq_plan(n)[1] == cut
        bank.insert_many_seq_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), n, flags.data_ptr())
        bank.sync()
        got = flags.cpu().numpy()
        assert np.array_equal(got, want)
        assert got[[cut - 1, cut, 5, cut + 200]].tolist() == [1, 0, 1, 0]
        assert bank.export_redis() == strings


# ---- the first-index table: one rule with the single filter's, and the hash table's edges --------

@pytest.mark.parametrize("n_filters,line", [(2, 342), (5, 1366)])
def test_bank_plan_follows_the_filter_rule(pkg, monkeypatch, n_filters, line):
    """A bank of B bits takes the direct form exactly when a single filter of m = B bits does (one
    word per bit is no bigger than the hash table: 4 B <= 12 slots), with the same scratch.
    ``line`` is the first n on the direct side; all n are below 4096, where the single filter's
    plan turns to the binned form."""
    def slots(n):                                                     # the hash table: >= 2 n k, at least 1024
        return max(1024, 1 << (2 * n * K - 1).bit_length())

    with make_bank(pkg, monkeypatch, None, M, K, n_filters) as bank:
        B = bank.device_bytes * 8                                     # bf_bank_info
        assert B == n_filters * 10240
        assert 4 * B > 12 * slots(line - 1) and 4 * B <= 12 * slots(line)
        for n in (1, 85, 86, line - 1, line, line + 1, 2730, 2731, 4095):
            single = pkg._lib.seq_plan(n, K, B)
            assert single["form"] == (1 if n >= line else 0)          # BF_SEQ_DIRECT / BF_SEQ_HASH
            assert single["slots"] == (B if n >= line else slots(n))
            direct, chunk, scratch = bank.seq_plan(n)
            assert direct is (n >= line) and chunk == n
            assert scratch == single["scratch_bytes"]


TABLE_POINTS = ["seq", "dev", "changes"]     # bf_bank_insert_many_seq, _seq_dev, _changes with seq = 1


def align256(x):
    return (x + 255) & ~255


def bank_bits(pkg, oracle, bank, keys, ids):
    """Every probe of the batch by its bank-wide bit number, the first-index table's key."""
    idx = oracle.indexes_many(*pkg.keys.pack(keys), bank.m, bank.k)
    return [int(f) * bank.stride * 8 + int(o) for f, row in zip(ids, idx) for o in row]


def table_case(pkg, oracle, monkeypatch, point, m, k, n_filters, batches, precondition):
    """Batches of a 1024-slot hash table through one entry point of a fresh bank, each exact against
    the oracle's one-by-one loop (flags, strings; the changes call also its list).  Returns the
    flags of every batch."""
    from test_gpu_bank_changes import changes_and_check              # it imports this module
    model = SeqModel(oracle, m, k)
    out = []
    with make_bank(pkg, monkeypatch, "hash", m, k, n_filters) as bank:
        assert not bank.bitcount().any()
        precondition(bank_bits(pkg, oracle, bank, *batches[0]))
        for keys, ids in batches:
            n = len(keys)
            assert 2 * n * k <= 1024
            assert bank.seq_plan(n) == (False, n, 1024 * 12 + align256(n * 16) + align256(n * 8))
            if point == "seq":
                flags = seq_and_check(bank, model, keys, ids, n_filters)
            elif point == "changes":
                flags, _ = changes_and_check(bank, model, keys, ids, n_filters, True)
            else:
                dk, do, di = dev_batch(keys, ids)
                d_flags = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                bank.insert_many_seq_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), n, d_flags.data_ptr())
                bank.sync()
                flags = d_flags.cpu().numpy()
                assert np.array_equal(flags, model.insert_seq(keys, ids))
                check_bank(bank, model, n_filters)
            out.append(flags.astype(bool))
    return out


# Found by a search over seeds on the CPU (about one seed in fifteen wraps); the test asserts its
# seed's property before it runs, so a changed key format or hash cannot lapse unnoticed.
BANK_WRAP_SEED, BANK_HALF_SEED = 1, 2


@pytest.mark.parametrize("point", TABLE_POINTS)
def test_bank_hash_table_wraps(pkg, oracle, monkeypatch, point):
    """73 pairs over 5 filters (2 n k = 876: 1024 slots): two distinct bank-wide bits of the batch
    hash to slot 1023, so one of them is stored at slot 0 and the mark's lookup follows it there.
    60 keys are distinct, 13 come again: 7 to the same filter (not new), 6 wherever the ids fall."""
    keys = [b"bw%d-%d" % (BANK_WRAP_SEED, i) for i in range(60)]
    keys = keys[:30] + keys[:13] + keys[30:]
    ids = np.random.default_rng(BANK_WRAP_SEED).integers(0, 5, len(keys)).astype(np.uint32)
    ids[30:37] = ids[:7]
    again = keys[::2] + [b"x" + key for key in keys[1::2]]           # half of the keys replaced
    again_ids = np.concatenate([ids[::2], ids[1::2]])

    def two_bits_at_the_last_slot(bits):
        assert wraps(bits, 1024)

    flags = table_case(pkg, oracle, monkeypatch, point, M, K, 5, [(keys, ids), (again, again_ids)],
                       two_bits_at_the_last_slot)
    assert not flags[0][30:37].any() and flags[0][:30].all() and flags[0][43:].all()
    assert not flags[1][:37].any() and 0 < flags[1][37:].sum() < 36  # a replaced key that comes twice is new once


@pytest.mark.parametrize("point", TABLE_POINTS)
def test_bank_hash_table_half_full(pkg, oracle, monkeypatch, point):
    """64 keys of 8 probes over 2 filters of 2^20 bits, all 512 bank-wide bits distinct and 0:
    2 n k = 1024 slots, exactly half of them taken.  The batch again (no 0-probe at all), then
    half of it with new keys."""
    m, k = 1 << 20, 8
    keys = half_batch(BANK_HALF_SEED)
    ids = (np.arange(64) % 2).astype(np.uint32)

    def all_distinct(bits):                                           # and 0: the bank is empty
        assert len(bits) == 512 == len(set(bits))

    mixed = keys[:32] + half_batch(BANK_HALF_SEED + 1)[:32]
    flags = table_case(pkg, oracle, monkeypatch, point, m, k, 2, [(keys, ids), (keys, ids), (mixed, ids)], all_distinct)
    assert flags[0].all() and not flags[1].any() and not flags[2][:32].any() and flags[2][32:].all()


# ---- the host form's refusals ---------------------------------------------------------------------

def test_host_refusals(pkg, monkeypatch):
    n_filters = 9
    keys = make_keys(50, 14, lo=3, hi=20)
    buf, offs = pack(keys)
    ids = np.zeros(len(keys), np.uint32)
    with make_bank(pkg, monkeypatch, None, M, K, n_filters) as bank:
        bad_ids = ids.copy()
        bad_ids[5] = n_filters
        with pytest.raises(pkg.ArgumentError, match=r"BF_EINVAL.*key 5: filter id 9 "):
            bank.insert_many_seq(buf, offs, bad_ids)
        backwards = offs.copy()
        backwards[7] = backwards[6] - 1
        lib, h = bank._lib, bank.handle
        flags = np.full(len(keys), 0xAB, np.uint8)
        rc = lib.bf_bank_insert_many_seq(h, buf.ctypes.data, backwards.ctypes.data, ids.ctypes.data, len(keys),
                                         flags.ctypes.data)
        assert rc == pkg._lib.BF_EINVAL and (flags == 0xAB).all()
        assert b"key 6: offsets must be non-decreasing" in lib.bf_bank_last_error(h)
        assert lib.bf_bank_insert_many_seq(h, buf.ctypes.data, None, ids.ctypes.data, len(keys), None) == pkg._lib.BF_EINVAL
        assert not bank.bitcount().any()                              # the bank is unchanged
        # forcing a form: by name, back to the bank's own rule, and an unknown one refused
        assert bank.seq_plan(1000)[0] is False
        bank.set_seq_form("direct")
        assert bank.seq_plan(1000)[0] is True
        assert lib.bf_bank_set_seq_form(h, 3) == pkg._lib.BF_EINVAL and b"unknown form 3" in lib.bf_bank_last_error(h)
        with pytest.raises(pkg.ArgumentError, match="form must be one of"):
            bank.set_seq_form("sometimes")
        assert bank.seq_plan(1000)[0] is True
        bank.set_seq_form("auto")
        assert bank.seq_plan(1000)[0] is False
        assert bank.insert_many_seq(buf, offs, ids).any()             # and still works


# ---- the BloomfilterBank facade with FakeRedis -------------------------------------------------------

NAMES = ["tenant:%d" % i for i in range(5)]


def facade_batch():
    rng = random.Random(15)
    keys = ["k%d" % i for i in range(300)] + list(range(60))
    names = [NAMES[rng.randrange(4)] for _ in keys]                   # tenant:4 gets nothing
    for dst, src in ((120, 7), (200, 7), (359, 310)):                 # pairs repeated inside the batch
        keys[dst], names[dst] = keys[src], names[src]
    return names, keys


def test_first_seen_write_through(pkg, O, oracle):
    now = [1000.0]
    clock = lambda: now[0]   # noqa: E731
    r, r_ruby = pkg.FakeRedis(clock=clock), pkg.FakeRedis()
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, clock=clock)
    m, k = bank.options["bits"], bank.options["hashes"]
    assert (m, k) == (M, K)
    rubies = {n: O.RubyDriverRestatement({"bits": m, "hashes": k, "key_name": n, "redis": r_ruby}) for n in NAMES}
    names, keys = facade_batch()
    model = SeqModel(oracle, m, k)
    want = model.insert_seq([pkg.keys.to_s(x) for x in keys], [bank.ids[n] for n in names])
    r.calls.clear()
    got = bank.first_seen_many(names, keys, expire=90)
    assert got.dtype == np.bool_ and np.array_equal(got, want.astype(bool))
    assert not got[[120, 200, 359]].any() and got[[7, 310]].all()
    for n, key in zip(names, keys):
        rubies[n].insert(key)
    wrote = {n for n, new in zip(names, got) if new}
    assert wrote == set(NAMES[:4])
    assert sorted(c for c in r.calls if c[0] in ("SETRANGE", "EXPIRE")) == \
        sorted([("SETRANGE", n) for n in wrote] + [("EXPIRE", n) for n in wrote])
    for n in NAMES:
        assert r.get(n) == r_ruby.get(n), n                           # byte for byte the ruby driver's string
    assert r.get(NAMES[4]) is None

    # only the key names with a True flag are written and EXPIREd
    r.calls.clear()
    got = bank.first_seen_many([NAMES[0], NAMES[1], NAMES[1], NAMES[4]], [keys[7], "fresh", "fresh", keys[7]],
                               expire=30)
    seen_in_0 = names[7] == NAMES[0]
    assert got.tolist() == [not seen_in_0, True, False, True]
    expect = sorted({NAMES[1], NAMES[4]} | (set() if seen_in_0 else {NAMES[0]}))
    assert [c for c in r.calls if c[0] != "GET"] == [("SETRANGE", n) for n in expect] + [("EXPIRE", n) for n in expect]
    assert r.ttl(NAMES[1]) == 30 and r.ttl(NAMES[4]) == 30 and r.ttl(NAMES[2]) == 90

    # the per-name view, and insert_many as before
    view = bank[NAMES[2]]
    assert view.first_seen("via-view") is True and view.first_seen("via-view") is False
    assert bank.first_seen(NAMES[3], "via-view") is True
    assert bank.insert_many([NAMES[2], NAMES[3], NAMES[0]], ["via-view", "plain", "via-view"]) == {NAMES[3], NAMES[0]}
    assert bank.insert_many([NAMES[3]], ["plain"]) == set()
    with pytest.raises(pkg.ArgumentError, match="unknown key name"):
        bank.first_seen("nobody", "x")
    bank.close()


def test_first_seen_manual_sync(pkg):
    r = pkg.FakeRedis()
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, sync="manual")
    r.calls.clear()
    assert bank.first_seen_many([NAMES[0], NAMES[3], NAMES[0]], ["a", "b", "a"], expire=60).tolist() == [True, True, False]
    assert r.calls == []                                              # manual: Redis untouched
    sent = bank.flush()
    assert sent == len(r.get(NAMES[0])) + len(r.get(NAMES[3])) and r.get(NAMES[1]) is None
    assert bank.first_seen(NAMES[0], "a") is False and bank.flush() == 0
    bank.close()
