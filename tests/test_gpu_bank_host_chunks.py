"""The chunks of the bank's host-pointer keyed calls (bf_bank_insert_many, _include_many,
_insert_many_seq, _insert_many_changes and _include_across, include/bfhip.h): a batch is cut at
``batch_keys`` keys and again at ``batch_bytes`` key bytes (a longer key goes alone), every chunk's
offsets rebased to 0.

Every expectation is the oracle model's (``test_gpu_bank.Model`` / ``test_gpu_bank_seq.SeqModel``):
where a batch is cut never shows in a result.  ``cuts`` restates the cut rule only to place keys
at chunk edges and to tell the chunks of a capped list apart.
"""
import bisect
import ctypes

import numpy as np
import pytest

from test_gpu_bank import M, K, Model, changed_of, check_bank, make_keys, pack
from test_gpu_bank_changes import diff, pairs_of, snapshot
from test_gpu_bank_seq import SeqModel, make_bank

pytestmark = pytest.mark.gpu

N_FILTERS = 8


def cuts(keys, batch_keys, batch_bytes=64 << 20):
    """The chunks [a, e) of a batch: at most batch_keys keys, and the longest run within batch_bytes
    (at least one key)."""
    offs = [0]
    for x in keys:
        offs.append(offs[-1] + len(x))
    out, a, n = [], 0, len(keys)
    while a < n:
        e = min(n, a + batch_keys)
        if offs[e] - offs[a] > batch_bytes:
            e = max(bisect.bisect_right(offs, offs[a] + batch_bytes, a, e + 1) - 1, a + 1)
        out.append((a, e))
        a = e
    return out


def across_of(model, keys, ids):
    """(n, count) bool: the model's include? of every key in every listed filter."""
    buf, offs = pack(keys)
    cols, out = {}, np.zeros((len(keys), len(ids)), bool)
    for i, f in enumerate(int(x) for x in ids):
        if f not in cols:
            cols[f] = (model.o.include_many(model.bits[f], model.m, model.k, buf, offs).astype(bool)
                       if f in model.bits else np.zeros(len(keys), bool))
        out[:, i] = cols[f]
    return out


def some_ids(n, seed, n_filters=N_FILTERS):
    return np.random.default_rng(seed).integers(0, n_filters, n).astype(np.uint32)


# ---- 1. the key cut, plain forms --------------------------------------------------------------

def test_key_cut_plain(pkg, oracle, monkeypatch):
    keys = make_keys(1000, 31, lo=12)
    ids = some_ids(len(keys), 31)
    assert len(set(zip(ids.tolist(), keys))) == 1000 and len(cuts(keys, 100)) == 10
    model = Model(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_keys=100) as bank:
        flags = bank.insert_many(*pack(keys), ids)
        assert changed_of(ids, flags) == model.insert(keys, ids)
        check_bank(bank, model, N_FILTERS)
        probe = keys + make_keys(200, 32, lo=12)
        pids = np.concatenate([ids, some_ids(200, 32)])
        got = bank.include_many(*pack(probe), pids)
        assert np.array_equal(got, model.include(probe, pids))
        assert got[:1000].all() and not got[1000:].all()


# ---- 2. the byte cut, all four families -------------------------------------------------------

BATCH_BYTES = 64


def byte_cut_batch():
    """300 keys of 0..40 bytes with, placed by hand: a zero-length key first, last and right after
    a chunk edge (behind the key that goes alone: only there can a chunk begin with one), a key of
    200 bytes and one of exactly batch_bytes."""
    keys = make_keys(300, 33, lo=0, hi=40)
    keys[0] = keys[299] = keys[151] = b""
    keys[150] = b"alone:" + bytes(range(194))
    keys[152] = b"exactly:" + bytes(range(56))
    assert len(keys[150]) == 200 and len(keys[152]) == BATCH_BYTES
    chunks = cuts(keys, 1 << 22, BATCH_BYTES)
    assert len(chunks) > 60 and (150, 151) in chunks                  # the long key goes alone
    after = [c for c in chunks if c[0] == 151]                        # ... and the next chunk begins with b""
    assert after and after[0][1] >= 153                               # ... and holds the 64-byte key, full to the byte
    assert sum(map(len, keys[151:after[0][1]])) == BATCH_BYTES
    assert chunks[-1][1] == 300 and chunks[-1][1] - chunks[-1][0] > 1  # the last b"" closes a chunk of several keys
    return keys, some_ids(len(keys), 33)


def test_byte_cut_plain(pkg, oracle, monkeypatch):
    keys, ids = byte_cut_batch()
    model = Model(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_bytes=BATCH_BYTES) as bank:
        flags = bank.insert_many(*pack(keys), ids)
        assert changed_of(ids, flags) == model.insert(keys, ids)
        check_bank(bank, model, N_FILTERS)
        probe = keys + make_keys(100, 34, lo=0, hi=40)
        pids = np.concatenate([ids, some_ids(100, 34)])
        got = bank.include_many(*pack(probe), pids)
        assert np.array_equal(got, model.include(probe, pids))
        assert got[:300].all() and not got[300:].all()


@pytest.mark.parametrize("form", ["hash", "direct"])
def test_byte_cut_seq(pkg, oracle, monkeypatch, form):
    keys, ids = byte_cut_batch()
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, form, M, K, N_FILTERS, batch_bytes=BATCH_BYTES) as bank:
        got = bank.insert_many_seq(*pack(keys), ids)
        want = model.insert_seq(keys, ids)
        assert np.array_equal(got, want) and 0 < int(got.sum()) < len(keys)   # the repeated b"" are not new
        check_bank(bank, model, N_FILTERS)


@pytest.mark.parametrize("seq", [0, 1])
def test_byte_cut_changes(pkg, oracle, monkeypatch, seq):
    keys, ids = byte_cut_batch()
    model = SeqModel(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_bytes=BATCH_BYTES) as bank:
        before = snapshot(model)
        flags, lids, lbits = bank.insert_many_changes(*pack(keys), ids, seq=seq)
        want = model.insert_seq(keys, ids)
        truth = diff(before, model)
        assert len(truth) > 1000 and pairs_of(lids, lbits) == truth
        if seq:
            assert np.array_equal(flags, want)
        else:
            assert changed_of(ids, flags) == changed_of(ids, want)
        check_bank(bank, model, N_FILTERS)


def test_byte_cut_across(pkg, oracle, monkeypatch):
    keys, ids = byte_cut_batch()
    model = Model(oracle, M, K)
    model.insert(keys[::2], ids[::2])
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_bytes=BATCH_BYTES) as bank:
        bank.insert_many(*pack(keys[::2]), ids[::2])
        got = bank.include_across(*pack(keys))
        want = across_of(model, keys, np.arange(N_FILTERS))
        assert got.shape == want.shape and np.array_equal(got, want)
        assert got.any() and not got.all()


# ---- 3. offsets[0] != 0 -----------------------------------------------------------------------

def test_offsets_need_not_begin_at_zero(pkg, oracle, monkeypatch):
    """37 bytes of junk in front of the keys and offsets[0] = 37: every chunk is rebased from its
    own first offset."""
    keys = make_keys(250, 35, lo=12)
    ids = some_ids(len(keys), 35)
    buf, offs = pack(keys)
    buf = np.concatenate([np.full(37, 0xA5, np.uint8), buf])
    offs = offs + np.uint64(37)
    assert offs.dtype == np.uint64 and offs[0] == 37
    model = Model(oracle, M, K)
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_keys=100) as bank:
        flags = np.full(len(keys), 0xAB, np.uint8)
        rc = bank._lib.bf_bank_insert_many(bank.handle, buf.ctypes.data, offs.ctypes.data, ids.ctypes.data, len(keys),
                                           flags.ctypes.data)
        assert rc == 0 and changed_of(ids, flags) == model.insert(keys, ids) and set(flags.tolist()) <= {0, 1}
        check_bank(bank, model, N_FILTERS)
        row = bank.across_row_bytes(N_FILTERS)
        mask = np.full((len(keys), row), 0xFF, np.uint8)
        rc = bank._lib.bf_bank_include_across(bank.handle, buf.ctypes.data, offs.ctypes.data, len(keys), None, N_FILTERS,
                                              mask.ctypes.data)
        assert rc == 0
        bits = np.unpackbits(mask, axis=1, bitorder="little").astype(bool)
        want = across_of(model, keys, np.arange(N_FILTERS))
        assert np.array_equal(bits[:, :N_FILTERS], want) and not bits[:, N_FILTERS:].any()
        assert all(want[j, ids[j]] for j in range(len(keys)))


# ---- 4. the cross query, cut ------------------------------------------------------------------

def test_across_cut(pkg, oracle, monkeypatch):
    n_filters = 70
    keys = make_keys(600, 36, lo=12)
    ids = some_ids(len(keys), 36, n_filters)
    fresh = make_keys(250, 37, lo=12)
    query = [keys[j] if j % 2 == 0 else fresh[j] for j in range(250)]
    model = Model(oracle, M, K)
    model.insert(keys, ids)
    scrambled = np.random.default_rng(36).permutation(n_filters).astype(np.uint32)
    assert len(cuts(query, 100)) == 3
    with make_bank(pkg, monkeypatch, None, M, K, n_filters, batch_keys=100) as bank:
        bank.insert_many(*pack(keys), ids)
        for lst in (scrambled, None):
            listed = np.arange(n_filters, dtype=np.uint32) if lst is None else lst
            want = across_of(model, query, listed)
            assert all(want[j, listed.tolist().index(ids[j])] for j in range(0, 250, 2)) and not want.all()
            assert np.array_equal(bank.include_across(*pack(query), lst), want)
            # the mask itself: two words a row, the spare bits of the second 0
            buf, offs = pack(query)
            mask = np.full((len(query), 16), 0xFF, np.uint8)
            assert bank.across_row_bytes(n_filters) == 16
            rc = bank._lib.bf_bank_include_across(bank.handle, buf.ctypes.data, offs.ctypes.data, len(query),
                                                  None if lst is None else lst.ctypes.data, n_filters, mask.ctypes.data)
            assert rc == 0
            bits = np.unpackbits(mask, axis=1, bitorder="little").astype(bool)
            assert np.array_equal(bits[:, :n_filters], want) and not bits[:, n_filters:].any()


# ---- 5. changes: the cap reached inside a middle chunk ----------------------------------------

def raw_changes(bank, keys, ids, seq, cap, with_lists=True):
    buf, offs = pack(keys)
    flags = np.full(len(keys), 0xAB, np.uint8)
    oi, ob = np.full(max(cap, 1), 0xCDCDCDCD, np.uint32), np.full(max(cap, 1), 0xEFEFEFEFEFEFEFEF, np.uint64)
    count = ctypes.c_uint64(77)
    rc = bank._lib.bf_bank_insert_many_changes(
        bank.handle, buf.ctypes.data, offs.ctypes.data, ids.ctypes.data, len(keys), int(seq), flags.ctypes.data,
        oi.ctypes.data if with_lists else None, ob.ctypes.data if with_lists else None, cap, ctypes.byref(count))
    return rc, count.value, flags, oi, ob


@pytest.mark.parametrize("seq", [0, 1])
def test_changes_cap_inside_a_middle_chunk(pkg, oracle, monkeypatch, seq):
    keys = make_keys(600, 38, lo=12)
    ids = some_ids(len(keys), 38)
    chunks = cuts(keys, 100)
    assert len(chunks) == 6
    # the model replays the chunks: the diff of each tells which chunk a listed bit belongs to
    model = SeqModel(oracle, M, K)
    chunk_of, sizes, want_flags = {}, [], []
    for c, (a, e) in enumerate(chunks):
        before = snapshot(model)
        want_flags.append(model.insert_seq(keys[a:e], ids[a:e]))
        d = diff(before, model)
        assert len(d) > 100 and not set(d) & set(chunk_of)
        chunk_of.update((p, c) for p in d)
        sizes.append(len(d))
    want_flags = np.concatenate(want_flags)
    total = sum(sizes)
    cap = sum(sizes[:3]) + sizes[3] // 2                               # strictly inside chunk 3 of 0..5
    assert sum(sizes[:3]) < cap < sum(sizes[:4]) and cap == total - (sizes[3] - sizes[3] // 2) - sizes[4] - sizes[5]
    E = pkg._lib
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_keys=100) as bank:
        rc, count, flags, oi, ob = raw_changes(bank, keys, ids, seq, cap)
        assert rc == E.BF_ERANGE and count == total
        assert b"flipped %d bits, the lists hold %d" % (total, cap) in bank._lib.bf_bank_last_error(bank.handle)
        listed = list(zip(oi.tolist(), ob.tolist()))
        assert len(listed) == cap and len(set(listed)) == cap and set(listed) <= set(chunk_of)
        order = [chunk_of[p] for p in listed]
        assert order == sorted(order) and max(order) == 3              # a later chunk's entries never come first
        assert [order.count(c) for c in range(4)] == sizes[:3] + [cap - sum(sizes[:3])]
        if seq:
            assert np.array_equal(flags, want_flags)
        else:
            assert changed_of(ids, flags) == changed_of(ids, want_flags)
        check_bank(bank, model, N_FILTERS)                            # the insert is fully applied
    # cap = 0 with NULL lists: the count only
    with make_bank(pkg, monkeypatch, None, M, K, N_FILTERS, batch_keys=100) as bank:
        rc, count, flags, oi, ob = raw_changes(bank, keys, ids, seq, 0, with_lists=False)
        assert rc == E.BF_ERANGE and count == total
        assert oi.tolist() == [0xCDCDCDCD] and ob.tolist() == [0xEFEFEFEFEFEFEFEF]
        check_bank(bank, model, N_FILTERS)
        rc, count, flags, _, _ = raw_changes(bank, keys, ids, seq, 0, with_lists=False)
        assert rc == 0 and count == 0 and not flags.any()             # nothing left to flip: 0 <= cap
        check_bank(bank, model, N_FILTERS)
