"""The bank's combines (bf_bank_fold*, bf_bank_overlap*, include/bfhip.h): filters of one bank
ANDed / ORed into each other, counted without writing, and the matrix of pairwise AND counts.

Every expectation is numpy over ``export_filters`` taken BEFORE the call; after every write the
whole bank is exported again and compared, so the untouched filters and every pad byte are
checked too.  Each bank holds an empty filter (id 0) and the all-ones string below m (id 1).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, K = 9585, 6          # 1000 keys @ 1 %: stride 1,280, a wave owns a filter
N_MAIN = 131
POP = np.array([bin(i).count("1") for i in range(256)], np.uint64)
OPS = {"or": np.bitwise_or, "and": np.bitwise_and, "xor": np.bitwise_xor}


def pack(keys):
    offs = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        np.cumsum([len(x) for x in keys], out=offs[1:])
    return np.frombuffer(b"".join(keys) + b"\0" * 16, np.uint8).copy(), offs


def all_ones(m):
    """The Redis string with every bit below m set (SETBIT order: offset o is bit 7 - o % 8 of byte o / 8)."""
    s = bytearray(b"\xff" * ((m + 7) // 8))
    if m % 8:
        s[-1] = (0xFF << (8 - m % 8)) & 0xFF
    return bytes(s)


def fill(bank, seed, max_keys=4000):
    """Filter 0 stays empty, filter 1 is all ones, filter f >= 2 gets keys up to about (f % 5 + 1) / 6
    of a half-full load, every third key shared with the next filter."""
    per = max(1, min(max_keys, int(bank.m * 0.69 / bank.k)))
    keys, ids = [], []
    for f in range(2, bank.n_filters):
        n = max(1, per * (f % 5 + 1) // 6)
        for j in range(n):
            keys.append(b"s%d:f%d:%d" % (seed, f, j))
            ids.append(f)
            if j % 3 == 0 and f + 1 < bank.n_filters:
                keys.append(keys[-1])
                ids.append(f + 1)
    bank.insert_many(*pack(keys), np.array(ids, np.uint32))
    bank.import_redis(np.array([1], np.uint32), [all_ones(bank.m)])


def popcount(rows):
    return POP[rows].sum(axis=-1, dtype=np.uint64)


def want_fold(before, op, sources):
    return [OPS[op].reduce(before[np.asarray(s, np.int64)], axis=0) for s in sources]


def check_fold(bank, op, sources, dst=None):
    """fold() against numpy; returns (changed, set_bits)."""
    before = bank.export_filters()[0].copy()
    want = want_fold(before, op, sources)
    changed, set_bits = bank.fold(op, sources, dst)
    assert changed.dtype == bool and set_bits.dtype == np.uint64 and len(changed) == len(set_bits) == len(sources)
    after = before.copy()
    if dst is not None:
        for g, d in enumerate(dst):
            after[d] = want[g]
    got = bank.export_filters()[0]
    assert np.array_equal(got, after), "filters %s differ" % np.flatnonzero((got != after).any(axis=1))[:8].tolist()
    assert not got[:, (bank.m + 7) // 8:].any(), "a pad byte is set"
    assert np.array_equal(set_bits, [int(popcount(w)) for w in want])
    if dst is None:
        assert not changed.any()
    else:
        assert changed.tolist() == [bool((before[d] != want[g]).any()) for g, d in enumerate(dst)]
        assert np.array_equal(bank.bitcount(np.array(dst, np.uint32)), set_bits)
    return changed, set_bits


def want_overlap(before, rows, cols, m):
    """AND counts by an exact float matmul of the unpacked bits (every count is below 2^24)."""
    assert m < 1 << 24
    a = np.unpackbits(before[np.asarray(rows, np.int64)], axis=1).astype(np.float32)
    b = np.unpackbits(before[np.asarray(cols, np.int64)], axis=1).astype(np.float32)
    return (a @ b.T).astype(np.uint64)


@pytest.fixture(scope="module")
def main(pkg):
    with pkg.FilterBank(M, K, N_MAIN) as bank:
        fill(bank, 1, max_keys=600)
        yield bank


# ---- both regimes and the boundary ------------------------------------------------------------

@pytest.mark.parametrize("m,k,n_filters", [(7, 1, 9), (33, 3, 9), (9585, 6, 9), (32_768, 6, 9), (32_769, 6, 9),
                                           (958_506, 7, 9), (8_388_608, 7, 5)])
def test_regimes(pkg, m, k, n_filters):
    """Wave owner, workgroup owner and the slice grid; the overlap's one slice and its stride split."""
    last = n_filters - 1
    with pkg.FilterBank(m, k, n_filters) as bank:
        assert bank.stride == {32_768: 4096, 32_769: 4224, 958_506: 119_936}.get(m, bank.stride)
        fill(bank, m)
        before = bank.export_filters()[0].copy()
        # the matrix of every pair, and a rectangle with a repeat
        bits8 = np.unpackbits(before, axis=1)
        if m <= 1 << 20:
            full = want_overlap(before, range(n_filters), range(n_filters), m)
        else:   # too long for a float matmul: pair by pair
            full = np.array([[int(popcount(before[i] & before[j])) for j in range(n_filters)] for i in range(n_filters)],
                            np.uint64)
        assert int(full[1, 1]) == m and not full[0].any() and int(bits8[1].sum()) == m
        got = bank.overlap()
        assert got.dtype == np.uint64 and np.array_equal(got, full)
        rows, cols = [last, 1, 2], [2, 0, last, 2, 3]
        assert np.array_equal(bank.overlap(rows, cols), full[np.ix_(rows, cols)])
        # at most 4 x 4: long strides stream these pair by pair
        for r, c in (([2], [2]), ([last, 1], [2, 0, 3]), ([1, 2, 3, last], None), ([2, 2, 3], [3, 3, 2, 0])):
            assert np.array_equal(bank.overlap(r, c), full[np.ix_(r, r if c is None else c)]), (r, c)
        # count-only: all three ops, nothing written
        srcs = [[2, 3], [1, last], [last, 2, 3, 4], [0, 2], [3]]
        for op in ("or", "and", "xor"):
            check_fold(bank, op, srcs)
        # writes: in place, to an outside destination, a copy
        check_fold(bank, "or", [[2, 3, last]], [2])
        check_fold(bank, "and", [[3, 4]], [0])
        check_fold(bank, "or", [[4], [2, 3]], [last, 0])
        ch, _ = check_fold(bank, "and", [[2, 1]], [2])          # AND with a superset changes nothing
        assert not ch[0]
        ch, _ = check_fold(bank, "or", [[1, 3]], [1])           # OR with a subset changes nothing
        assert not ch[0]
        # the device form overwrites pre-filled outputs
        seg, src = dev(np.array([0, 2, 3], np.uint64)), dev(np.array([2, 3, 1], np.uint32))
        d_ch = torch.full((2,), 0xFF, dtype=torch.uint8, device="cuda")
        d_sb = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        d_out = torch.full((n_filters * n_filters,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        bank.fold_dev("and", seg.data_ptr(), src.data_ptr(), 2, 3, d_changed=d_ch.data_ptr(), d_set_bits=d_sb.data_ptr())
        bank.overlap_dev(d_out.data_ptr())
        bank.sync()
        now = bank.export_filters()[0]
        assert d_ch.cpu().tolist() == [0, 0]
        assert d_sb.cpu().tolist() == [int(popcount(now[2] & now[3])), m]
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n_filters, n_filters), bank.overlap())
        # ... also where the pairs are few, a bad row reading zeros
        d_few = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        d_r, d_c = dev(np.array([2, n_filters], np.uint32)), dev(np.array([3], np.uint32))
        torch.cuda.synchronize()
        bank.overlap_dev(d_few.data_ptr(), d_r.data_ptr(), 2, d_c.data_ptr(), 1)
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*filter id at or past n_filters"):
            bank.sync()
        assert d_few.cpu().tolist() == [int(popcount(now[2] & now[3])), 0]


# ---- folds on the main bank -------------------------------------------------------------------

def test_group_sizes(main):
    rng = np.random.default_rng(3)
    sources = [rng.integers(0, 100, n).tolist() for n in (1, 2, 7, 64)]
    for op in ("or", "and"):
        check_fold(main, op, sources, [100, 101, 102, 103])
    check_fold(main, "xor", sources)


@pytest.mark.parametrize("groups", [1, 3, 4, 5, 300])
def test_group_counts(main, groups):
    """4 wave owners a workgroup: 1, 3 and 5 groups leave waves idle."""
    rng = np.random.default_rng(groups)
    sources = [rng.integers(0, 100, int(rng.integers(1, 6))).tolist() for _ in range(groups)]
    for op in ("or", "and", "xor"):
        check_fold(main, op, sources)
    if groups <= 31:
        check_fold(main, "or", sources, list(range(100, 100 + groups)))
        check_fold(main, "and", [s + [1] for s in sources], list(range(100 + groups - 1, 99, -1)))


def test_destinations_copies_and_repeats(main):
    # inside its own sources (first, middle, last), and outside them
    ch, _ = check_fold(main, "or", [[110, 7, 8], [9, 111, 10], [11, 12, 112], [13, 14]], [110, 111, 112, 113])
    assert ch.all()
    check_fold(main, "and", [[110, 7], [8, 111]], [110, 111])
    # a copy, also of the empty and of the all-ones filter; a copy onto itself changes nothing
    ch, bits = check_fold(main, "or", [[22], [0], [1], [23]], [114, 115, 116, 23])
    assert ch.tolist() == [True, True, True, False] and bits.tolist()[1:3] == [0, M]
    ch, _ = check_fold(main, "or", [[0]], [115])                 # the empty filter onto an empty one
    assert not ch[0]
    ch, _ = check_fold(main, "and", [[0]], [116])                # all ones -> empty
    assert ch[0]
    # repeated sources
    check_fold(main, "or", [[30, 30, 31, 30], [32, 32]], [117, 118])
    check_fold(main, "xor", [[30, 30], [30, 31, 30]])
    # changed is 0 exactly when nothing differs
    ch, _ = check_fold(main, "or", [[117, 30, 31]], [117])       # OR with its own subsets
    assert not ch[0]
    ch, _ = check_fold(main, "and", [[118, 1]], [118])           # AND with a superset
    assert not ch[0]
    ch, _ = check_fold(main, "and", [[117, 30]], [117])          # ... with a proper subset it shrinks
    assert ch[0]


# ---- the overlap matrix -----------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 65), (63, 64), (65, 33)])
def test_overlap_shapes(main, rows, cols):
    """Shuffled lists with repeats, the empty and the all-ones filter among them."""
    rng = np.random.default_rng(rows * 100 + cols)
    r = rng.integers(0, N_MAIN, rows)
    c = rng.integers(0, N_MAIN, cols)
    c[: min(cols, 3)] = [1, 0, int(r[0])][: min(cols, 3)]
    before = main.export_filters()[0]
    got = main.overlap(r, c)
    assert got.shape == (rows, cols) and np.array_equal(got, want_overlap(before, r, c, M))
    assert np.array_equal(got[:, 0], main.bitcount(r.astype(np.uint32)))     # against the all-ones filter
    if cols > 1:
        assert not got[:, 1].any()                                           # against the empty one
    if rows * cols > 60 * 60:
        assert len(set(r.tolist())) < rows or len(set(c.tolist())) < cols    # the lists do repeat


def test_overlap_square_symmetric(main):
    rng = np.random.default_rng(130)
    r = rng.permutation(N_MAIN)[:100]
    r = np.concatenate([r, r[:28], [0, 1]]).astype(np.uint32)
    rng.shuffle(r)
    assert len(r) == 130
    before = main.export_filters()[0]
    got = main.overlap(r)
    assert got.shape == (130, 130) and np.array_equal(got, want_overlap(before, r, r, M))
    assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), main.bitcount(r))
    assert np.array_equal(got, main.overlap(r, r))               # the same lists given twice: no mirroring
    # the same pairs asked of fold as count-only ANDs
    pairs = [[int(a), int(b)] for a in r for b in r]
    _, bits = main.fold("and", pairs)
    assert np.array_equal(bits.reshape(130, 130), got)
    assert np.array_equal(main.overlap(), want_overlap(before, range(N_MAIN), range(N_MAIN), M))
    assert np.array_equal(main.export_filters()[0], before)


# ---- past 4 GiB -------------------------------------------------------------------------------

def test_past_4_gib(pkg):
    """3,400,000 filters of stride 1,280 are 4.35 GB: ids 3,355,442..3,355,444 straddle byte 2^32."""
    n_filters = 3_400_000
    lo, mid, hi, end = 3_355_442, 3_355_443, 3_355_444, 3_399_999
    assert lo * 1280 < 1 << 32 <= hi * 1280
    look = np.array([0, 1, 2, lo - 1, lo, mid, hi, hi + 1, end - 1, end], np.uint32)
    at = {int(f): i for i, f in enumerate(look)}
    keys, ids = [], []
    for f, n in ((0, 300), (lo, 500), (mid, 200), (hi, 400), (end, 100)):
        keys += [b"g%d:%d" % (f % 7, j) for j in range(n)]
        ids += [f] * n
    with pkg.FilterBank(M, K, n_filters) as bank:
        bank.insert_many(*pack(keys), np.array(ids, np.uint32))
        before = bank.export_filters(look)[0].copy()
        sources = [[0, lo, end], [mid, lo], [hi, lo]]
        dst = [hi + 1, 1, hi]                                    # past, before, and in place past 2^32
        want = [np.bitwise_or.reduce(before[[at[s] for s in grp]], axis=0) for grp in sources]
        changed, bits = bank.fold("or", sources, dst)
        after = before.copy()
        for g, d in enumerate(dst):
            after[at[d]] = want[g]
        got = bank.export_filters(look)[0]
        assert np.array_equal(got, after) and changed.all()
        assert np.array_equal(bits, [int(popcount(w)) for w in want])
        _, cnt = bank.fold("and", [[lo, hi], [0, end], [mid, hi + 1]])
        assert np.array_equal(cnt, [int(popcount(got[at[a]] & got[at[b]])) for a, b in ((lo, hi), (0, end), (mid, hi + 1))])
        rows, cols = [0, lo, hi, lo - 1], [mid, end, 1, hi + 1, 2]
        assert np.array_equal(bank.overlap(rows, cols),
                              want_overlap(got, [at[f] for f in rows], [at[f] for f in cols], M))
        assert not got[[at[2], at[lo - 1], at[end - 1]]].any()   # the neighbours stayed empty


# ---- the device forms -------------------------------------------------------------------------

def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()).cuda()


def test_device_guards(pkg, main):
    before = main.export_filters()[0].copy()
    # group 1 names a bad id, group 2 is empty, group 4's destination is bad: skipped, zeros
    seg = np.array([0, 2, 4, 4, 6, 7], np.uint64)
    src = np.array([5, 6, 7, N_MAIN, 8, 9, 10], np.uint32)
    dst = np.array([120, 121, 122, 123, N_MAIN + 5], np.uint32)
    d_seg, d_src, d_dst = dev(seg), dev(src), dev(dst)
    d_ch = torch.full((5,), 0xFF, dtype=torch.uint8, device="cuda")
    d_sb = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    main.fold_dev("or", d_seg.data_ptr(), d_src.data_ptr(), 5, 7, d_dst.data_ptr(), d_ch.data_ptr(), d_sb.data_ptr())
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*filter id at or past n_filters"):
        main.sync()
    main.sync()                                                  # reported once
    after = before.copy()
    after[120], after[123] = before[5] | before[6], before[8] | before[9]
    assert np.array_equal(main.export_filters()[0], after)
    assert d_ch.cpu().tolist() == [1, 0, 0, 1, 0]
    assert d_sb.cpu().tolist() == [int(popcount(after[120])), 0, 0, int(popcount(after[123])), 0]
    # an empty group alone also reports
    d_sb.fill_(-1)
    main.fold_dev("and", dev(np.array([0, 0], np.uint64)).data_ptr(), d_src.data_ptr(), 1, 0, d_set_bits=d_sb.data_ptr())
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL"):
        main.sync()
    assert d_sb.cpu().tolist()[0] == 0
    # a bad row and a bad column: zeros there, every other entry right
    rows, cols = np.array([3, N_MAIN, 4], np.uint32), np.array([4, 5, 1 << 31, 3], np.uint32)
    d_out = torch.full((12,), -1, dtype=torch.int64, device="cuda")
    d_r, d_c = dev(rows), dev(cols)
    torch.cuda.synchronize()
    main.overlap_dev(d_out.data_ptr(), d_r.data_ptr(), 3, d_c.data_ptr(), 4)
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*filter id at or past n_filters"):
        main.sync()
    main.sync()
    got = d_out.cpu().numpy().view(np.uint64).reshape(3, 4)
    want = np.zeros((3, 4), np.uint64)
    want[np.ix_([0, 2], [0, 1, 3])] = want_overlap(after, [3, 4], [4, 5, 3], M)
    assert np.array_equal(got, want) and want.any()
    # NULL and misaligned pointers, XOR with a destination, an unknown op, the count rules
    s, i, d, c, b, o = (t.data_ptr() for t in (d_seg, d_src, d_dst, d_ch, d_sb, d_out))
    for args in ((0, i, d, c, b), (s, 0, d, c, b), (s + 4, i, d, c, b), (s, i + 2, d, c, b), (s, i, d + 1, c, b),
                 (s, i, d, c, b + 4)):
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*device pointer"):
            main.fold_dev("or", args[0], args[1], 5, 7, args[2], args[3], args[4])
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*XOR"):
        main.fold_dev("xor", s, i, 5, 7, d)
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*unknown op 7"):
        main.fold_dev(7, s, i, 5, 7)
    for kw in (dict(d_out=0), dict(d_out=o + 4), dict(d_out=o, d_row_ids=d_r.data_ptr() + 2, rows=2),
               dict(d_out=o, d_row_ids=d_r.data_ptr(), rows=2, d_col_ids=d_c.data_ptr() + 1, cols=2)):
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*device pointer"):
            main.overlap_dev(**kw)
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*rows must be n_filters"):
        main.overlap_dev(o, rows=3)
    with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*cols must be rows"):
        main.overlap_dev(o, d_r.data_ptr(), 3, 0, 4)
    assert main._lib.bf_bank_fold_dev(main.handle, 1, None, None, None, 0, 0, None, None, None) == 0
    assert main._lib.bf_bank_overlap_dev(main.handle, None, 0, None, 0, None, None) == 0
    main.sync()
    assert np.array_equal(main.export_filters()[0], after)


def test_side_stream_then_host_form(pkg):
    """A fold and an overlap on the caller's stream, then the host forms on the bank's own stream
    with no synchronisation between: they see the fold."""
    with pkg.FilterBank(M, K, 12) as bank:
        fill(bank, 9, max_keys=500)
        before = bank.export_filters()[0].copy()
        d_seg, d_src, d_dst = dev(np.array([0, 3, 5], np.uint64)), dev(np.array([2, 3, 4, 5, 6], np.uint32)), \
            dev(np.array([10, 11], np.uint32))
        d_sb = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        d_out = torch.full((144,), -1, dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        bank.fold_dev("or", d_seg.data_ptr(), d_src.data_ptr(), 2, 5, d_dst.data_ptr(), d_set_bits=d_sb.data_ptr(),
                      stream=st.cuda_stream)
        bank.overlap_dev(d_out.data_ptr(), stream=st.cuda_stream)
        host = bank.overlap()
        _, cnt = bank.fold("and", [[10, 2], [11, 6]])
        st.synchronize()
        bank.sync()
        after = before.copy()
        after[10], after[11] = before[2] | before[3] | before[4], before[5] | before[6]
        assert np.array_equal(bank.export_filters()[0], after)
        want = want_overlap(after, range(12), range(12), M)
        assert np.array_equal(host, want)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(12, 12), want)
        assert cnt.tolist() == [int(popcount(before[2])), int(popcount(before[6]))]
        assert d_sb.cpu().tolist() == [int(popcount(after[10])), int(popcount(after[11]))]


# ---- the host forms' refusals -----------------------------------------------------------------

def test_host_refusals(pkg):
    n_filters = 9
    with pkg.FilterBank(M, K, n_filters) as bank:
        fill(bank, 11, max_keys=300)
        lib, h, E = bank._lib, bank.handle, pkg._lib.BF_EINVAL
        before = bank.export_filters()[0].copy()
        AND, OR, XOR = pkg._lib.BF_BITOP_AND, pkg._lib.BF_BITOP_OR, pkg._lib.BF_BITOP_XOR

        def p(a, t):
            return None if a is None else np.ascontiguousarray(a, t)

        def fold_refused(op, dst, seg, src, what, groups=None):
            dst, seg, src = p(dst, np.uint32), p(seg, np.uint64), p(src, np.uint32)
            groups = (len(seg) - 1) if groups is None else groups
            ch, sb = np.full(8, 0xAB, np.uint8), np.full(8, 0xABAB, np.uint64)
            rc = lib.bf_bank_fold(h, op, *(None if a is None else a.ctypes.data for a in (dst, seg, src)), groups,
                                  ch.ctypes.data, sb.ctypes.data)
            assert rc == E and (ch == 0xAB).all() and (sb == 0xABAB).all()
            assert what in lib.bf_bank_last_error(h).decode(), lib.bf_bank_last_error(h)

        fold_refused(OR, None, None, [2, 3], "seg / src_ids is NULL", groups=1)
        fold_refused(OR, None, [0, 2], None, "seg / src_ids is NULL")
        fold_refused(OR, None, [0, 2, 2, 3], [2, 3, 4], "group 1 is empty")
        fold_refused(OR, None, [0, 0], [2], "group 0 is empty")
        fold_refused(OR, None, [1, 2], [2, 3], "seg[0] must be 0, got 1")
        fold_refused(OR, None, [0, 2, 1, 3], [2, 3, 4], "group 1: seg must be non-decreasing")
        fold_refused(AND, None, [0, 2, 3], [2, 3, n_filters], "src_ids[2] = 9 is not below n_filters = 9")
        fold_refused(AND, [4, n_filters], [0, 2, 3], [2, 3, 5], "dst_ids[1] = 9 is not below n_filters = 9")
        fold_refused(3, None, [0, 2], [2, 3], "unknown op 3")
        fold_refused(XOR, [4], [0, 2], [2, 3], "BF_BITOP_XOR only counts")
        fold_refused(OR, [4, 5, 4], [0, 1, 2, 3], [2, 3, 6], "dst_ids[2] = 4 is also the destination of group 0")
        fold_refused(OR, [4, 5], [0, 2, 4], [4, 2, 3, 4], "group 1 reads filter 4 (src_ids[3]), the destination of group 0")
        fold_refused(AND, [4, 5], [0, 2, 4], [5, 2, 5, 3], "group 0 reads filter 5 (src_ids[0]), the destination of group 1")

        def overlap_refused(rows, nr, cols, nc, what, out=True):
            rows, cols = p(rows, np.uint32), p(cols, np.uint32)
            o = np.full(128, 0xABAB, np.uint64)
            rc = lib.bf_bank_overlap(h, None if rows is None else rows.ctypes.data, nr,
                                     None if cols is None else cols.ctypes.data, nc, o.ctypes.data if out else None)
            assert rc == E and (o == 0xABAB).all()
            assert what in lib.bf_bank_last_error(h).decode(), lib.bf_bank_last_error(h)

        overlap_refused([2, 3], 2, None, 2, "out is NULL", out=False)
        overlap_refused(None, n_filters - 1, None, n_filters - 1, "rows must be n_filters = 9, got 8")
        overlap_refused([2, 3], 2, None, 3, "cols must be rows = 2, got 3")
        overlap_refused([2, n_filters], 2, None, 2, "row_ids[1] = 9 is not below n_filters = 9")
        overlap_refused([2, 3], 2, [4, 5, 77], 3, "col_ids[2] = 77 is not below n_filters = 9")
        overlap_refused([2, 3], 1 << 32, [4, 5], 1 << 32, "overflow a 64-bit byte size")
        # the wrapper raises the same refusals
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*group 1 is empty"):
            bank.fold("or", [[2], []])
        with pytest.raises(pkg.ArgumentError, match="BF_EINVAL.*only counts"):
            bank.fold("xor", [[2, 3]], [4])
        with pytest.raises(pkg.ArgumentError, match=r"BF_EINVAL.*row_ids\[0\] = 4000000000 "):
            bank.overlap(np.array([4_000_000_000], np.uint64))
        with pytest.raises(pkg.ArgumentError, match="destinations for"):
            bank.fold("or", [[2], [3]], [4])
        # groups == 0, rows == 0 and cols == 0 write nothing and are no error
        ch, sb = bank.fold("or", [])
        assert len(ch) == 0 and len(sb) == 0
        o = np.full(4, 0xABAB, np.uint64)
        ids = np.array([2, 3], np.uint32)
        seg0 = np.zeros(1, np.uint64)
        assert lib.bf_bank_fold(h, OR, None, seg0.ctypes.data, ids.ctypes.data, 0, None, o.ctypes.data) == 0
        assert lib.bf_bank_overlap(h, ids.ctypes.data, 0, ids.ctypes.data, 2, o.ctypes.data) == 0
        assert lib.bf_bank_overlap(h, ids.ctypes.data, 2, ids.ctypes.data, 0, o.ctypes.data) == 0
        assert (o == 0xABAB).all()
        assert bank.overlap(ids, np.zeros(0, np.uint32)).shape == (2, 0)
        assert bank.overlap(np.zeros(0, np.uint32)).shape == (0, 0)
        bank.sync()                                              # nothing was launched, nothing to report
        assert np.array_equal(bank.export_filters()[0], before)
        check_fold(bank, "or", [[2, 3]], [4])                    # a later call runs


# ---- the BloomfilterBank facade with FakeRedis ------------------------------------------------

NAMES = ["day:%d" % i for i in range(6)] + ["week", "month"]


def oracle_string(pkg, oracle, m, k, keys):
    bits = oracle.new_bitset(m, k)
    oracle.insert_many(bits, m, k, *pkg.keys.pack(sorted(keys)))
    return oracle.redis_string(bits)


@pytest.mark.parametrize("sync", ["write_through", "manual"])
def test_facade_merge_and_rollup(pkg, oracle, sync):
    now = [1000.0]
    r = pkg.FakeRedis(clock=lambda: now[0])
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, sync=sync, clock=lambda: now[0])
    m, k = bank.options["bits"], bank.options["hashes"]
    members = {n: {"%s/%d" % (n, j) for j in range(40)} | {"shared-%d" % j for j in range(i, i + 10)}
               for i, n in enumerate(NAMES[:6])}
    for n, ks in members.items():
        bank.insert_many([n] * len(ks), sorted(ks))
    bank.insert_many(["week"] * 5, ["w%d" % j for j in range(5)])
    bank.flush()

    def stored(name):
        bank.flush()
        return r.get(name)

    # merge: week |= day:0 | day:1, the TTL armed because the string changed
    assert bank.merge("week", ["day:0", "day:1"], expire=50) is True
    want = members["day:0"] | members["day:1"] | {"w%d" % j for j in range(5)}
    assert stored("week") == oracle_string(pkg, oracle, m, k, want) == bank.to_redis_string("week")
    if sync == "write_through":
        assert r.ttl("week") == 50
    # the same merge again changes nothing: no write, no EXPIRE
    r.calls.clear()
    now[0] += 10
    assert bank.merge("week", ["day:1", "day:0"], expire=500) is False
    assert [c for c in r.calls if c[0] in ("SETRANGE", "EXPIRE", "DEL")] == []
    if sync == "write_through":
        assert r.ttl("week") == 40
    # rollup to a shorter string: month is first the long all-days union, then one small day
    assert bank.rollup("month", NAMES[:6], expire=70) is True
    long = stored("month")
    assert long == oracle_string(pkg, oracle, m, k, set().union(*members.values()))
    tiny = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=["t"], redis=pkg.FakeRedis(), clock=lambda: now[0])
    tiny.insert("t", "only")
    short = tiny.to_redis_string("t")
    tiny.close()
    bank.clear("day:0")
    bank.insert("day:0", "only")
    assert bank.rollup("month", ["day:0"]) is True
    assert len(short) < len(long)
    assert stored("month") == short and r.strlen("month") == len(short)
    assert r.ttl("month") == -1                                  # the TTL went with the DEL, none was given since
    # a rollup of empty sources leaves no key at all
    bank.clear("day:1")
    assert bank.rollup("month", ["day:1"]) is True
    assert stored("month") is None and bank.to_redis_string("month") == b""
    assert bank.rollup("month", ["day:1"]) is False
    with pytest.raises(pkg.ArgumentError, match="unknown key name"):
        bank.merge("week", ["nobody"])
    bank.close()


def test_facade_sizes_and_overlap(pkg):
    now = [1000.0]
    r = pkg.FakeRedis(clock=lambda: now[0])
    bank = pkg.BloomfilterBank(size=1000, error_rate=0.01, key_names=NAMES, redis=r, clock=lambda: now[0])
    # four days of 400 keys, each sharing 200 with the next: 1,000 distinct in all
    for i in range(4):
        bank.insert_many([NAMES[i]] * 400, ["member-%d" % j for j in range(200 * i, 200 * i + 400)],
                         expire=30 if i == 3 else None)
    r.calls.clear()
    before = bank.bank.export_filters()[0].copy()
    est = bank.union_size(NAMES[:4])
    print("union estimate %.1f for 1000 distinct keys" % est)
    assert abs(est - 1000) <= 20                                 # tests/test_gpu_stats.py's 2 %
    # the smaller sets against the four-sigma collision bound of tests/test_gpu_stats.py (_bound):
    # n keys set n k bits less the collisions, whose count has about their own number as variance
    k = bank.options["hashes"]
    x = bank.count_bits()
    _, xu = bank.bank.fold("or", [[0, 1], [0, 2]])

    def bound(n, set_bits):
        return 4.0 * math.sqrt(max(n * k - int(set_bits), 0)) / k

    one = bank.union_size([NAMES[0]])
    print("one name: estimate %.1f for 400 keys, bound %.1f" % (one, bound(400, x[0])))
    assert abs(one - 400) <= bound(400, x[0])
    shared = bank.intersection_size(NAMES[0], NAMES[1])
    budget = bound(400, x[0]) + bound(400, x[1]) + bound(600, xu[0])
    print("intersection estimate %.1f for 200 shared keys, bound %.1f" % (shared, budget))
    assert abs(shared - 200) <= budget
    assert abs(bank.intersection_size(NAMES[0], NAMES[2])) <= bound(400, x[0]) + bound(400, x[2]) + bound(800, xu[1])
    got = bank.overlap()
    assert got.shape == (8, 8) and got.dtype == np.uint64
    assert np.array_equal(got, want_overlap(before, range(8), range(8), bank.options["bits"]))
    assert np.array_equal(np.diag(got), bank.count_bits())
    assert np.array_equal(bank.overlap(["day:1", "day:3"], ["day:2", "week", "day:1"]), got[np.ix_([1, 3], [2, 6, 1])])
    assert np.array_equal(bank.overlap(["day:3", "day:0"]), got[np.ix_([3, 0], [3, 0])])
    assert r.calls == [] and np.array_equal(bank.bank.export_filters()[0], before)   # reads: nothing touched
    # a name past its deadline reads as empty
    now[0] += 31
    late = bank.overlap()
    assert not late[3].any() and not late[:, 3].any() and np.array_equal(late[:3, :3], got[:3, :3])
    _, xl = bank.bank.fold("or", [[0, 1, 2]])
    assert abs(bank.union_size(NAMES[:4]) - 800) <= bound(800, xl[0])
    bank.close()
