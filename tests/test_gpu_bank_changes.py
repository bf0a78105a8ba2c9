"""Bank inserts that list the bits they flipped (bf_bank_insert_many_changes*, include/bfhip.h) and
the facade's SETBIT write-through built on them (``sync='write_through_bits'``).

The model is ``test_gpu_bank.Model`` / ``test_gpu_bank_seq.SeqModel``.  The expected list is the
oracle's diff: every (filter, bit position in SETBIT order) where a filter's Redis string after the
batch has a 1 and the string before it had a 0.  Every comparison is exact: the sorted pairs equal
the diff, no pair repeats, the flags are the plain or the sequential insert's, and the bank's
strings equal the oracle's.  The modes are the plain insert (seq = 0) and the sequential one in
both table forms (``BFHIP_BANK_SEQ_FORM``).
"""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_bank import M, K, changed_of, check_bank, dev_batch, make_keys, pack
from test_gpu_bank_seq import SeqModel, dedup_batch, make_bank

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["plain", "hash", "direct"]            # seq = 0; seq = 1 with either first-index table


def open_bank(pkg, monkeypatch, mode, m, k, n_filters, **kw):
    return make_bank(pkg, monkeypatch, None if mode == "plain" else mode, m, k, n_filters, **kw)


def snapshot(model):
    return {f: model.string(f) for f in model.bits}


def string_bits(s, nbits):
    out = np.zeros(nbits, np.uint8)
    out[: len(s) * 8] = np.unpackbits(np.frombuffer(s, np.uint8))   # bit o: byte o >> 3, mask 0x80 >> (o & 7)
    return out


def diff(before, model):
    """The sorted (filter, SETBIT offset) pairs that are 1 in the model now and were 0 in `before`."""
    out = []
    for f in model.bits:
        after = model.string(f)
        new = string_bits(after, len(after) * 8) & (1 - string_bits(before.get(f, b""), len(after) * 8))
        out += [(f, int(o)) for o in np.flatnonzero(new)]
    return sorted(out)


def pairs_of(ids, bits):
    assert ids.dtype == np.uint32 and bits.dtype == np.uint64 and len(ids) == len(bits)
    got = sorted(zip(ids.tolist(), bits.tolist()))
    assert len(set(got)) == len(got), "a bit is listed twice"
    return got


def changes_and_check(bank, model, keys, ids, n_filters, seq, check=True):
    """One insert_many_changes against the model: the list is the oracle's diff, the flags are the
    mode's, the bank's strings the oracle's.  Returns (flags, pairs)."""
    ids = np.asarray(ids, np.uint32)
    before = snapshot(model)
    flags, lids, lbits = bank.insert_many_changes(*pack(keys), ids, seq=seq)
    want_flags = model.insert_seq(keys, ids)
    got = pairs_of(lids, lbits)
    assert got == diff(before, model)
    assert flags.dtype == np.uint8 and len(flags) == len(keys)
    if seq:
        assert np.array_equal(flags, want_flags)
    else:   # the OR of key_flipped over a filter's keys is "this filter's string changed"
        assert changed_of(ids, flags) == set(lids.tolist()) == changed_of(ids, want_flags)
    if check:
        check_bank(bank, model, n_filters)
    return flags, got


# ---- parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("pre", [False, True], ids=["empty", "half-inserted"])
@pytest.mark.parametrize("mode", MODES)
def test_parity(pkg, oracle, monkeypatch, mode, pre):
    n_filters = 37
    keys, ids, _ = dedup_batch(41, n_filters)
    assert len(keys) == 1000
    model = SeqModel(oracle, M, K)
    with open_bank(pkg, monkeypatch, mode, M, K, n_filters) as bank:
        if pre:
            bank.insert_many(*pack(keys[:500]), ids[:500])
            model.insert(keys[:500], ids[:500])
        flags, got = changes_and_check(bank, model, keys, ids, n_filters, mode != "plain")
        assert flags.any() and len(got) > (1500 if pre else 3000)
        # the same call again flips nothing and lists nothing
        again, lids, lbits = bank.insert_many_changes(*pack(keys), ids, seq=mode != "plain")
        assert not again.any() and len(lids) == 0 and len(lbits) == 0
        check_bank(bank, model, n_filters)


# ---- races for one bit ----------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(7, 1), (33, 3), (M, K)])
@pytest.mark.parametrize("seq", [False, True], ids=["plain", "seq"])
def test_races_for_one_bit(pkg, oracle, monkeypatch, seq, m, k):
    """4,096 distinct keys into ONE filter: at m = 7 every bit is wanted by hundreds of lanes of
    every workgroup, and each is listed once."""
    keys = make_keys(4096, 5, lo=4, hi=30)
    ids = np.full(len(keys), 3, np.uint32)
    model = SeqModel(oracle, m, k)
    with make_bank(pkg, monkeypatch, None, m, k, 5) as bank:
        _, got = changes_and_check(bank, model, keys, ids, 5, seq)
        assert len(got) == int(bank.bitcount().sum()) == model.popcount(3)
        assert {f for f, _ in got} == {3}
        if m <= 33:
            assert len(got) == m                                       # the filter is full


@pytest.mark.parametrize("seq", [False, True], ids=["plain", "seq"])
def test_one_key_per_filter(pkg, oracle, monkeypatch, seq):
    keys = make_keys(4096, 5, lo=4, hi=30)
    perm = np.random.default_rng(5).permutation(4096).astype(np.uint32)
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, 4096) as bank:
        flags, got = changes_and_check(bank, model, keys, perm, 4096, seq)
        assert flags.all() and len(got) == int(bank.bitcount().sum())
        assert {f for f, _ in got} == set(range(4096))


# ---- tile and chunk edges -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_tile_edges(pkg, oracle, monkeypatch, mode):
    seq = mode != "plain"
    n_filters = 9
    for n in (1, 255, 256, 257, 1000):
        keys = make_keys(n, 100 + n)
        ids = np.random.default_rng(n).integers(0, n_filters, n).astype(np.uint32)
        model = SeqModel(oracle, M, K)
        with open_bank(pkg, monkeypatch, mode, M, K, n_filters) as bank:
            _, got = changes_and_check(bank, model, keys, ids, n_filters, seq)
            assert 0 < len(got) <= n * K
    model = SeqModel(oracle, M, K)
    with open_bank(pkg, monkeypatch, mode, M, K, n_filters) as bank:
        # n == 0: nothing listed, and the C call writes count = 0
        flags, lids, lbits = bank.insert_many_changes(np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                                                      np.zeros(0, np.uint32), seq=seq)
        assert len(flags) == 0 and len(lids) == 0 and len(lbits) == 0
        count = ctypes.c_uint64(77)
        offs = np.zeros(1, np.uint64)
        rc = bank._lib.bf_bank_insert_many_changes(bank.handle, None, offs.ctypes.data, None, 0, int(seq), None, None,
                                                   None, 0, ctypes.byref(count))
        assert rc == 0 and count.value == 0
        assert bank.export_redis() == [b""] * n_filters
        # a tile whose key bytes exceed the 16 KiB LDS stage: keys are read from global memory
        long_keys = make_keys(256, 8, lo=200, hi=200)
        long_keys[200] = long_keys[3]
        lids = (np.arange(256) % 3).astype(np.uint32)
        lids[200] = lids[3]
        changes_and_check(bank, model, long_keys, lids, n_filters, seq)


@pytest.mark.parametrize("seq", [False, True], ids=["plain", "seq"])
def test_host_chunks_are_concatenated(pkg, oracle, monkeypatch, seq):
    n_filters = 8
    keys = make_keys(1000, 7, lo=12)
    ids = np.random.default_rng(7).integers(0, n_filters, len(keys)).astype(np.uint32)
    keys[100], ids[100] = keys[99], ids[99]                           # one pair on both sides of a chunk edge
    keys[700], ids[700] = keys[150], ids[150]                         # ... and chunks apart
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, n_filters, batch_keys=100) as cut, \
            make_bank(pkg, monkeypatch, None, M, K, n_filters) as whole:
        flags, got = changes_and_check(cut, model, keys, ids, n_filters, seq)       # ten chunks' lists
        _, wi, wb = whole.insert_many_changes(*pack(keys), ids, seq=seq)
        assert pairs_of(wi, wb) == got
        assert cut.export_redis() == whole.export_redis()
        if seq:
            assert flags[[99, 100, 150, 700]].tolist() == [1, 0, 1, 0]


# ---- cap ------------------------------------------------------------------------------------------

def raw_changes(bank, keys, ids, seq, cap, with_lists=True, with_flags=True):
    buf, offs = pack(keys)
    ids = np.ascontiguousarray(ids, np.uint32)
    flags = np.full(len(keys), 0xAB, np.uint8)
    oi, ob = np.full(max(cap, 1), 0xCDCDCDCD, np.uint32), np.full(max(cap, 1), 0xEFEFEFEFEFEFEFEF, np.uint64)
    count = ctypes.c_uint64(77)
    rc = bank._lib.bf_bank_insert_many_changes(
        bank.handle, buf.ctypes.data, offs.ctypes.data, ids.ctypes.data, len(keys), int(seq),
        flags.ctypes.data if with_flags else None, oi.ctypes.data if with_lists else None,
        ob.ctypes.data if with_lists else None, cap, ctypes.byref(count))
    return rc, count.value, flags, oi, ob


@pytest.mark.parametrize("mode", MODES)
def test_cap(pkg, oracle, monkeypatch, mode):
    seq = mode != "plain"
    n_filters = 11
    keys = make_keys(600, 21)
    ids = np.random.default_rng(21).integers(0, n_filters, len(keys)).astype(np.uint32)
    E = pkg._lib
    model = SeqModel(oracle, M, K)
    with open_bank(pkg, monkeypatch, mode, M, K, n_filters) as bank:
        # cap > 0 with a NULL list: refused, nothing touched
        rc, count, flags, _, _ = raw_changes(bank, keys, ids, seq, 10, with_lists=False)
        assert rc == E.BF_EINVAL and count == 77 and (flags == 0xAB).all()
        assert b"NULL out_ids" in bank._lib.bf_bank_last_error(bank.handle)
        assert bank._lib.bf_bank_insert_many_changes(bank.handle, None, None, None, 1, 2, None, None, None, 0,
                                                     ctypes.byref(ctypes.c_uint64())) == E.BF_EINVAL       # seq = 2
        assert bank._lib.bf_bank_insert_many_changes(bank.handle, None, None, None, 1, 0, None, None, None, 0,
                                                     None) == E.BF_EINVAL                                   # NULL count
        assert not bank.bitcount().any()
        # cap = 10 below the true count: BF_ERANGE after the insert is fully applied
        before = snapshot(model)
        want_flags = model.insert_seq(keys, ids)
        truth = diff(before, model)
        assert len(truth) > 3000
        rc, count, flags, oi, ob = raw_changes(bank, keys, ids, seq, 10)
        assert rc == E.BF_ERANGE and count == len(truth)
        assert b"flipped %d bits" % len(truth) in bank._lib.bf_bank_last_error(bank.handle)
        first = pairs_of(oi, ob)
        assert len(first) == 10 and set(first) <= set(truth)
        if seq:
            assert np.array_equal(flags, want_flags)
        else:
            assert changed_of(ids, flags) == changed_of(ids, want_flags)
        check_bank(bank, model, n_filters)
        # the Python method raises the library's error for an explicit cap that overflows
        more = make_keys(50, 22)
        mids = np.arange(50, dtype=np.uint32) % n_filters
        with pytest.raises(pkg.ArgumentError, match="BF_ERANGE.*the lists hold 3"):
            bank.insert_many_changes(*pack(more), mids, seq=seq, cap=3)
        model.insert(more, mids)
        check_bank(bank, model, n_filters)
        # cap = 0 with NULL lists: the count only
        last = make_keys(40, 23)
        lids = np.arange(40, dtype=np.uint32) % n_filters
        before = snapshot(model)
        model.insert(last, lids)
        truth = diff(before, model)
        rc, count, _, _, _ = raw_changes(bank, last, lids, seq, 0, with_lists=False, with_flags=False)
        assert 0 < len(truth) == count and rc == E.BF_ERANGE
        rc, count, flags, _, _ = raw_changes(bank, last, lids, seq, 0, with_lists=False)
        assert rc == 0 and count == 0 and not flags.any()             # nothing left to flip: 0 <= cap
        check_bank(bank, model, n_filters)


# ---- 64-bit addressing ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_long_filters_and_word_edges(pkg, oracle, monkeypatch, mode):
    m, k, n_filters = 958_506, 7, 5
    keys = make_keys(600, m)
    ids = np.random.default_rng(m).integers(0, n_filters, len(keys)).astype(np.uint32)
    model = SeqModel(oracle, m, k)
    with open_bank(pkg, monkeypatch, mode, m, k, n_filters) as bank:
        _, got = changes_and_check(bank, model, keys, ids, n_filters, mode != "plain")
        offsets = np.array([o for _, o in got])
        assert offsets.max() > 900_000 and len(set((offsets % 32).tolist())) == 32    # every position of a word


def test_past_4_gib(pkg, oracle, monkeypatch):
    """The 3,400,000-filter bank of test_gpu_bank.test_past_4_gib: filter 3,355,443 straddles byte
    2^32.  The listed ids and offsets on both sides of it are the oracle's."""
    n_filters = 3_400_000
    straddle = 3_355_443
    targets = list(range(straddle - 3, straddle + 4)) + [0, n_filters - 1]
    keys = make_keys(72, 9, lo=12)
    ids = np.array([targets[j % len(targets)] for j in range(len(keys))], np.uint32)
    keys[60], ids[60] = keys[2], ids[2]                               # a pair of the first batch again in the second
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, n_filters) as bank:
        assert bank.device_bytes == 4_352_000_000
        for seq, lo, hi in ((False, 0, 36), (True, 36, 72)):
            before = snapshot(model)
            flags, lids, lbits = bank.insert_many_changes(*pack(keys[lo:hi]), ids[lo:hi], seq=seq)
            want = model.insert_seq(keys[lo:hi], ids[lo:hi])
            assert pairs_of(lids, lbits) == diff(before, model)
            assert set(lids.tolist()) == set(targets)
            if seq:
                assert np.array_equal(flags, want)
        look = targets + [straddle - 4, straddle + 4]
        assert bank.export_redis(np.array(look, np.uint32)) == [model.string(f) for f in targets] + [b"", b""]
        assert int(bank.bitcount().sum()) == sum(model.popcount(f) for f in targets)


# ---- the device path ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_dev_form_on_a_side_stream(pkg, oracle, monkeypatch, mode):
    seq = mode != "plain"
    n_filters = 9
    first = make_keys(300, 12)
    ids1 = (np.arange(len(first)) % n_filters).astype(np.uint32)
    keys = make_keys(700, 8, lo=8)
    ids = np.random.default_rng(8).integers(0, n_filters, len(keys)).astype(np.uint32)
    keys[600], ids[600] = keys[20], ids[20]                           # a duplicate pair among the valid keys
    keys[650], ids[650] = first[7], ids1[7]                           # a pair the host call before it inserted
    ids[5], ids[300] = n_filters, 0xFFFFFFFF
    buf, offs = pack(keys)
    offs[41] = offs[40] - 2                                           # key 40's offsets run backwards
    bad = [5, 40, 300]
    good = [j for j in range(len(keys)) if j not in bad]
    named = [buf[int(offs[j]):int(offs[j + 1])].tobytes() for j in good]   # the keys the offsets name
    model = SeqModel(oracle, M, K)
    model.insert(first, ids1)
    before = snapshot(model)
    want_flags = model.insert_seq(named, ids[good])
    truth = diff(before, model)
    cap = len(keys) * K
    dk = torch.from_numpy(buf).cuda()
    do = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    di = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    flags = torch.full((len(keys),), 7, dtype=torch.uint8, device="cuda")
    out_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    out_bits = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((2,), -12345, dtype=torch.int64, device="cuda")   # garbage: the call zeroes it
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with open_bank(pkg, monkeypatch, mode, M, K, n_filters) as bank:
        bank.insert_many(*pack(first), ids1)                          # on the bank's own stream
        args = (dk.data_ptr(), do.data_ptr(), di.data_ptr(), len(keys))
        # refused before any launch: misaligned lists and counter, seq = 2, NULL lists with cap > 0
        for kw, what in ((dict(d_count=count.data_ptr() + 4, d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr()),
                          "misaligned"),
                         (dict(d_count=count.data_ptr(), d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr() + 4),
                          "misaligned"),
                         (dict(d_count=count.data_ptr(), d_out_ids=out_ids.data_ptr() + 2, d_out_bits=out_bits.data_ptr()),
                          "misaligned"),
                         (dict(d_count=count.data_ptr(), d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr(), seq=2),
                          "seq must be 0 or 1"),
                         (dict(d_count=count.data_ptr(), d_out_ids=0, d_out_bits=out_bits.data_ptr()), "NULL device pointer"),
                         (dict(d_count=0, d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr()), "NULL device pointer")):
            with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*" + what):
                bank.insert_many_changes_dev(*args, cap=cap, stream=st.cuda_stream, **kw)
        assert int(count[0].item()) == -12345
        bank.insert_many_changes_dev(*args, d_count=count.data_ptr(), d_out_ids=out_ids.data_ptr(),
                                     d_out_bits=out_bits.data_ptr(), cap=cap, seq=seq, d_flags=flags.data_ptr(),
                                     stream=st.cuda_stream)
        st.synchronize()
        with pytest.raises(pkg.ArgumentError, match="filter id at or past n_filters and inconsistent key offsets"):
            bank.sync()
        bank.sync()                                                   # reported once
        total = int(count[0].item())
        assert total == len(truth) and int(count[1].item()) == -12345
        got = pairs_of(out_ids.cpu().numpy()[:total].view(np.uint32), out_bits.cpu().numpy()[:total].view(np.uint64))
        assert got == truth                                           # the skipped keys list nothing
        assert (out_ids.cpu().numpy()[total:] == -1).all() and (out_bits.cpu().numpy()[total:] == -1).all()
        fl = flags.cpu().numpy()
        assert fl[bad].tolist() == [0, 0, 0] and fl[650] == 0
        if seq:
            assert np.array_equal(fl[good], want_flags)
        else:
            assert changed_of(ids[good], fl[good]) == {f for f, _ in truth}
        check_bank(bank, model, n_filters)
        # the count-only form on device arrays, NULL lists and flags: nothing left to flip
        bank.insert_many_changes_dev(*args, d_count=count.data_ptr() + 8, seq=seq, stream=st.cuda_stream)
        st.synchronize()
        with pytest.raises(pkg.ArgumentError, match="filter id at or past n_filters"):
            bank.sync()
        assert count.cpu().numpy().tolist() == [total, 0]
        check_bank(bank, model, n_filters)


# ---- the BloomfilterBank facade with FakeRedis ------------------------------------------------------

NAMES = ["tenant:%d" % i for i in range(5)]


def writes(r):
    return [c for c in r.calls if c[0] != "GET"]


def test_setbit_write_through(pkg, O):
    now = [1000.0]
    clock = lambda: now[0]   # noqa: E731
    r, r_def, r_ruby = pkg.FakeRedis(clock=clock), pkg.FakeRedis(clock=clock), pkg.FakeRedis()
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, clock=clock,
                               sync="write_through_bits")
    default = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r_def, clock=clock)
    m, k = bank.options["bits"], bank.options["hashes"]
    assert (m, k) == (M, K) and bank.sync_mode == "write_through_bits"
    rubies = {n: O.RubyDriverRestatement({"bits": m, "hashes": k, "key_name": n, "redis": r_ruby}) for n in NAMES}

    def same_everywhere():
        for n in NAMES:
            assert r.get(n) == r_ruby.get(n) == r_def.get(n), n       # byte for byte the ruby driver's string

    # one insert of a new key: its SETBITs and, with expire, one EXPIRE; no string is sent
    r.calls.clear()
    assert bank[NAMES[2]].insert("fresh", expire=90) is True and default[NAMES[2]].insert("fresh", expire=90) is True
    rubies[NAMES[2]].insert("fresh")
    calls = writes(r)
    assert 1 <= len(calls) - 1 <= k and calls[:-1] == [("SETBIT", NAMES[2])] * (len(calls) - 1)
    assert calls[-1] == ("EXPIRE", NAMES[2]) and r.bytes_in == 0
    assert r.ttl(NAMES[2]) == 90
    same_everywhere()

    # a second new key without expire: SETBITs only, and the key's TTL is kept
    now[0] += 10
    r.calls.clear()
    assert bank.insert(NAMES[2], "fresh too") is True and default.insert(NAMES[2], "fresh too") is True
    rubies[NAMES[2]].insert("fresh too")
    calls = writes(r)
    assert 1 <= len(calls) <= k and set(calls) == {("SETBIT", NAMES[2])} and r.bytes_in == 0
    assert r.ttl(NAMES[2]) == 80 == r_def.ttl(NAMES[2])
    same_everywhere()

    # a key already present: no write, no EXPIRE
    r.calls.clear()
    assert bank.insert(NAMES[2], "fresh", expire=30) is False and bank.first_seen(NAMES[2], "fresh", expire=30) is False
    assert r.calls == [] and r.ttl(NAMES[2]) == 80

    # a 700-key batch: four names get ~175 new keys each (over the budget: their string), tenant:4
    # gets one new key and one it has seen (its SETBITs)
    default.insert(NAMES[4], "seen")
    bank.insert(NAMES[4], "seen")
    rubies[NAMES[4]].insert("seen")
    keys = ["k%d" % i for i in range(698)] + ["seen", "only new key of tenant:4"]
    names = [NAMES[i % 4] for i in range(698)] + [NAMES[4], NAMES[4]]
    r.calls.clear()
    changed = bank.insert_many(names, keys, expire=60)
    assert changed == default.insert_many(names, keys, expire=60) == set(NAMES)
    for n, key in zip(names, keys):
        rubies[n].insert(key)
    calls = writes(r)
    assert sorted(c for c in calls if c[0] == "SETRANGE") == [("SETRANGE", n) for n in NAMES[:4]]
    setbits = [c for c in calls if c[0] == "SETBIT"]
    assert 1 <= len(setbits) <= k and set(setbits) == {("SETBIT", NAMES[4])}
    assert sorted(c for c in calls if c[0] == "EXPIRE") == [("EXPIRE", n) for n in NAMES]
    assert len(calls) == 4 + len(setbits) + 5
    assert r.bytes_in == sum(len(r.get(n)) for n in NAMES[:4])
    assert [r.ttl(n) for n in NAMES] == [60] * 5
    same_everywhere()

    # first_seen_many: the flags and the written names of the default mode
    rng = random.Random(15)
    fkeys = ["f%d" % i for i in range(40)] + keys[:10]
    fnames = [NAMES[rng.randrange(5)] for _ in range(40)] + names[:10]
    fkeys[30], fnames[30] = fkeys[4], fnames[4]                       # a pair repeated inside the batch
    r.calls.clear()
    r_def.calls.clear()
    got, want = bank.first_seen_many(fnames, fkeys), default.first_seen_many(fnames, fkeys)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert got[4] and not got[30] and not got[40:].any()
    for n, key in zip(fnames, fkeys):
        rubies[n].insert(key)
    assert {n for c, n in writes(r) if c in ("SETBIT", "SETRANGE")} == {n for c, n in writes(r_def) if c == "SETRANGE"}
    assert not [c for c in writes(r) if c[0] == "EXPIRE"]
    same_everywhere()

    # merge / clear behave as in 'write_through'
    r.calls.clear()
    assert bank.merge(NAMES[0], [NAMES[1]]) is True and default.merge(NAMES[0], [NAMES[1]]) is True
    assert writes(r) == [("SETRANGE", NAMES[0])]
    bank.clear(NAMES[3])
    default.clear(NAMES[3])
    assert r.get(NAMES[3]) is None and r.get(NAMES[0]) == r_def.get(NAMES[0])
    now[0] += 61                                                      # the deadlines pass: DEL as in write_through
    assert bank.include(NAMES[1], "k1") is False and r.get(NAMES[1]) is None
    bank.close()
    default.close()
