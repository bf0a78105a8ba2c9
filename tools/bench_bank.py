#!/usr/bin/env python3
"""Time a filter bank (bf_bank.hip) against what the library offered before it.

Workload: 2^22 twelve-byte keys with uniformly random filter ids into banks of 10^3 and 10^5
filters of 10k @ 1 % (m = 95,851; k = 6 as the facade derives it, bloomfilter.rb:54-58 divides
Integers; --hashes 7 measures the real-valued quotient's k).  Per bank size, insert (into the cleared bank) and
include? (of the same keys, all members) through the *_dev calls, HIP events around each call,
the median of --runs runs after --warmup.  Two baselines, timed the same way:

    handles   (10^3 filters only) the one way a caller had before: the same keys grouped by id
              and sent through 10^3 ``Filter`` handles one after another, one *_dev call each,
              events around the whole loop (so the host's launch gaps count, as they did)
    flat      ONE ``Filter`` of the same total bits: the random-fill ceiling (every probe of a
              key lands anywhere in the allocation, no filter id to read)

One JSON line on stdout (and in --out).

    python tools/bench_bank.py [--filters 1000,100000] [--hashes 7] [--runs 25] [--out profiles/bank_ops.json]

--across times the cross query instead (bf_bank_include_across_dev: one key against many
filters, hashed once) against the only way there was before: the crossed batch through
bf_bank_include_many_dev, every key repeated once per listed filter and the ids tiled, built on
the device before timing.  Four shapes (ACROSS_SHAPES), filters half full (5,000 random keys
each; the first query keys on top, each in one listed filter).  The two calls run alternately, HIP
events around each, median / min / max of --runs runs after --warmup; the answers are compared
once outside the timed region.

    python tools/bench_bank.py --across [--hashes 7] [--runs 25] [--out profiles/bank_across.json]

--combine times the bank's folds and overlap matrix (bf_bank_fold_dev, bf_bank_overlap_dev) against
what there was before them: ``export_filters`` of the sources, a numpy OR and ``import_redis`` of
the destination for a roll-up; ``export_filters`` of the list and host counts of the ANDs for the
matrix.  Both baselines include their copies.  The same method: the two alternate, HIP events
around each, median / min / max, the results compared once outside the timed region.  Before
each timed roll-up its destinations are cleared (untimed), so every vector is stored.  The 10k @
1 % filters hold 5,000 random keys each; the 120-MB ones (m = 958,505,838) are random strings,
every bit set with probability 1/2.

    python tools/bench_bank.py --combine [--only small|many|big] [--runs 25] [--out profiles/bank_combine.json]

--seq times the insert with exact sequential per-key flags (bf_bank_insert_many_seq_dev) on the
first workload (2^22 keys, random ids, 10^3 and 10^5 filters, a cleared bank before every run)
against (b) bf_bank_insert_many_dev on the same keys, include?-then-insert through the two *_dev
calls (approximate answers) and, for 10^3 filters, (c) the one way there was to get the same
flags: the keys grouped by id through 10^3 ``Filter`` handles' ``insert_many_dev`` with
``d_per_key_new``.  Where the bank picks the direct table the forced hash form is timed too.  The
flags of (a) and (c) and the bits of all of them are compared once outside the timed region.

    python tools/bench_bank.py --seq [--filters 1000,100000] [--runs 25] [--out profiles/bank_seq.json]

--changes times what listing the flipped bits costs (bf_bank_insert_many_changes_dev, cap = n k)
on the first workload: against bf_bank_insert_many_dev for seq = 0 and bf_bank_insert_many_seq_dev
for seq = 1, the two alternating, a cleared bank before every run, median / min / max.  The list's
length and distinctness are checked once outside the timed region.  Then the facade: one
``bank[name].insert(key)`` of a new key into a half-full 10k @ 1 % key name with FakeRedis under
``sync='write_through'`` and ``'write_through_bits'``: microseconds per call (host clock; the call
ends in a device synchronise), and the bytes and SETBITs FakeRedis received per call.

    python tools/bench_bank.py --changes [--filters 1000,100000] [--runs 25] [--out profiles/bank_changes.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pkgload  # noqa: E402

SIZE, ERROR_RATE = 10_000, 0.01
KEY_BYTES = 12
HANDLES_MAX = 1000      # the loop over handles is only practical (and only measured) up to here


def decimal_keys(n: int):
    """n distinct keys "000000000000".."..." of KEY_BYTES decimal digits, packed."""
    i = np.arange(n, dtype=np.int64)
    digits = np.stack([(i // 10 ** p) % 10 for p in range(KEY_BYTES - 1, -1, -1)], axis=1).astype(np.uint8) + 48
    buf = np.concatenate([digits.reshape(-1), np.zeros(16, np.uint8)])
    offs = (np.arange(n + 1, dtype=np.uint64) * np.uint64(KEY_BYTES))
    return buf, offs


def to_dev(buf, offs, ids=None):
    out = [torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64).copy()).cuda()]
    if ids is not None:
        out.append(torch.from_numpy(ids.view(np.int32).copy()).cuda())
    return out


def timed_events(fn, runs: int, warmup: int, before=None):
    """Median / min ms of fn() between two events on the null stream (the stream fn launches on),
    and the median host time of the same span."""
    ms, host = [], []
    for i in range(warmup + runs):
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
            host.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), statistics.median(host)


def entry(t, n: int) -> dict:
    med, lo, host = t
    return {"ms": round(med, 4), "min_ms": round(lo, 4), "host_ms": round(host, 4),
            "Mkeys_per_s": round(n / (med * 1e-3) / 1e6, 1)}


def run_bank(pkg, m, k, nf, n, buf, offs, runs, warmup) -> dict:
    ids = np.random.default_rng([0xBA2C, nf]).integers(0, nf, n).astype(np.uint32)
    dk, do, di = to_dev(buf, offs, ids)
    out8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = {"n_filters": nf}
    with pkg.FilterBank(m, k, nf, device=0) as bank:
        res["stride"], res["device_bytes"] = bank.stride, bank.device_bytes
        res["insert"] = entry(timed_events(
            lambda: bank.insert_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), n, stream=0), runs, warmup,
            before=lambda: bank.clear_dev(stream=0)), n)
        res["include"] = entry(timed_events(
            lambda: bank.include_many_dev(dk.data_ptr(), do.data_ptr(), di.data_ptr(), n, out8.data_ptr(), stream=0),
            runs, warmup), n)
        torch.cuda.synchronize()
        bank.sync()
        assert bool(out8.all()), "a member answered 0"
        counts = bank.bitcount()
        res["set_bits"] = int(counts.sum())

    # ONE filter of the same total bits
    with pkg.Filter(m * nf, k, device=0) as flat:
        res["flat_m"] = flat.m
        res["flat_insert"] = entry(timed_events(
            lambda: flat.insert_many_dev(dk.data_ptr(), do.data_ptr(), n, stream=0), runs, warmup,
            before=flat.clear), n)
        res["flat_include"] = entry(timed_events(
            lambda: flat.include_many_dev(dk.data_ptr(), do.data_ptr(), n, out8.data_ptr(), stream=0), runs, warmup), n)
        torch.cuda.synchronize()
        assert bool(out8.all())

    # the same keys grouped by id through nf handles, one after another
    if nf <= HANDLES_MAX:
        order = np.argsort(ids, kind="stable")
        sorted_buf = np.concatenate([buf[:-16].reshape(n, KEY_BYTES)[order].reshape(-1), np.zeros(16, np.uint8)])
        starts = np.searchsorted(ids[order], np.arange(nf + 1), side="left")
        sk, so = to_dev(sorted_buf, offs)
        filters = [pkg.Filter(m, k, device=0) for _ in range(nf)]
        spans = [(f, so.data_ptr() + 8 * int(starts[i]), int(starts[i + 1] - starts[i]), int(starts[i]))
                 for i, f in enumerate(filters) if starts[i + 1] > starts[i]]

        def insert_loop():
            for f, d_off, cnt, _ in spans:
                f.insert_many_dev(sk.data_ptr(), d_off, cnt, stream=0)

        def include_loop():
            for f, d_off, cnt, first in spans:
                f.include_many_dev(sk.data_ptr(), d_off, cnt, out8.data_ptr() + first, stream=0)

        def clear_all():
            for f in filters:
                f.clear()

        res["handles_insert"] = entry(timed_events(insert_loop, runs, warmup, before=clear_all), n)
        res["handles_include"] = entry(timed_events(include_loop, runs, warmup), n)
        torch.cuda.synchronize()
        assert bool(out8.all())
        assert sum(f.bitcount() for f in filters) == res["set_bits"], "the handles hold other filters than the bank"
        for f in filters:
            f.close()
        res["speedup_insert_vs_handles"] = round(res["handles_insert"]["ms"] / res["insert"]["ms"], 1)
        res["speedup_include_vs_handles"] = round(res["handles_include"]["ms"] / res["include"]["ms"], 1)
    res["insert_vs_flat"] = round(res["flat_insert"]["ms"] / res["insert"]["ms"], 2)
    res["include_vs_flat"] = round(res["flat_include"]["ms"] / res["include"]["ms"], 2)
    return res


# ---- --seq: the insert with exact sequential flags against the plain insert and the handles ------

def run_seq(pkg, m, k, nf, n, buf, offs, runs, warmup) -> dict:
    """run_bank's workload through bf_bank_insert_many_seq_dev (a), against bf_bank_insert_many_dev
    on the same keys (b), include?-then-insert (approximate answers: two copies of a pair inside
    the batch both read "not seen") and, up to HANDLES_MAX filters, the one way there was to get
    the same flags (c): the keys grouped by id through one ``Filter`` handle each,
    ``insert_many_dev`` with ``d_per_key_new``.  Every insert starts from cleared filters."""
    ids = np.random.default_rng([0xBA2C, nf]).integers(0, nf, n).astype(np.uint32)
    dk, do, di = to_dev(buf, offs, ids)
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = {"n_filters": nf}

    def time_bank(bank):
        args = (dk.data_ptr(), do.data_ptr(), di.data_ptr(), n)
        clear = lambda: bank.clear_dev(stream=0)   # noqa: E731
        t = {"seq": entry(timed_events(lambda: bank.insert_many_seq_dev(*args, flags.data_ptr(), stream=0), runs, warmup,
                                       before=clear), n)}
        torch.cuda.synchronize()
        bank.sync()
        t["set_bits"], t["new_keys"] = int(bank.bitcount().sum()), int(flags.sum())
        return t

    with pkg.FilterBank(m, k, nf, device=0) as bank:
        res["stride"], res["device_bytes"] = bank.stride, bank.device_bytes
        direct, chunk, scratch = bank.seq_plan(n)
        res["plan"] = {"form": "direct" if direct else "hash", "chunk_keys": chunk, "scratch_bytes": scratch}
        t = time_bank(bank)
        res["seq"], res["set_bits"], res["new_keys"] = t["seq"], t["set_bits"], t["new_keys"]
        bank_flags = flags.cpu().numpy()
        args = (dk.data_ptr(), do.data_ptr(), di.data_ptr(), n)
        clear = lambda: bank.clear_dev(stream=0)   # noqa: E731
        res["insert"] = entry(timed_events(lambda: bank.insert_many_dev(*args, stream=0), runs, warmup, before=clear), n)
        torch.cuda.synchronize()
        assert int(bank.bitcount().sum()) == res["set_bits"], "the two inserts leave different bits"

        def include_then_insert():
            bank.include_many_dev(*args, out8.data_ptr(), stream=0)
            bank.insert_many_dev(*args, stream=0)

        res["include_then_insert"] = entry(timed_events(include_then_insert, runs, warmup, before=clear), n)
        torch.cuda.synchronize()
        bank.sync()
        # on distinct keys into cleared filters include?-before-insert of the whole batch is all 0
        assert not bool(out8.any())

    if direct:   # the other form on the same bank, forced
        with pkg.FilterBank(m, k, nf, device=0) as bank:
            bank.set_seq_form("hash")
            assert bank.seq_plan(n)[0] is False
            t = time_bank(bank)
        assert (t["set_bits"], t["new_keys"]) == (res["set_bits"], res["new_keys"])
        assert np.array_equal(flags.cpu().numpy(), bank_flags), "the two forms differ"
        res["seq_hash_forced"] = t["seq"]

    if nf <= HANDLES_MAX:
        order = np.argsort(ids, kind="stable")
        sorted_buf = np.concatenate([buf[:-16].reshape(n, KEY_BYTES)[order].reshape(-1), np.zeros(16, np.uint8)])
        starts = np.searchsorted(ids[order], np.arange(nf + 1), side="left")
        sk, so = to_dev(sorted_buf, offs)
        filters = [pkg.Filter(m, k, device=0) for _ in range(nf)]
        spans = [(f, so.data_ptr() + 8 * int(starts[i]), int(starts[i + 1] - starts[i]), int(starts[i]))
                 for i, f in enumerate(filters) if starts[i + 1] > starts[i]]

        def handles_loop():
            for f, d_off, cnt, first in spans:
                f.insert_many_dev(sk.data_ptr(), d_off, cnt, d_per_key_new=flags.data_ptr() + first, stream=0)

        def clear_all():
            for f in filters:
                f.clear()

        res["handles_seq"] = entry(timed_events(handles_loop, runs, warmup, before=clear_all), n)
        torch.cuda.synchronize()
        # the same answers: a stable sort keeps each filter's keys in batch order
        assert np.array_equal(flags.cpu().numpy(), bank_flags[order]), "the handles' flags differ from the bank's"
        assert sum(f.bitcount() for f in filters) == res["set_bits"]
        for f in filters:
            f.close()
        res["handles_over_seq"] = round(res["handles_seq"]["ms"] / res["seq"]["ms"], 2)
    res["seq_over_insert"] = round(res["seq"]["ms"] / res["insert"]["ms"], 2)
    res["seq_over_include_then_insert"] = round(res["seq"]["ms"] / res["include_then_insert"]["ms"], 2)
    print("%d filters: seq %.3f ms, insert %.3f ms, include+insert %.3f ms%s" % (
        nf, res["seq"]["ms"], res["insert"]["ms"], res["include_then_insert"]["ms"],
        ", handles %.3f ms" % res["handles_seq"]["ms"] if "handles_seq" in res else ""), file=sys.stderr, flush=True)
    return res


# ---- --across: the cross query (bf_bank_include_across_dev) against the crossed batch ----------

# (label, keys, listed filters or None for all, filters of the bank)
ACROSS_SHAPES = [("2^20 keys x 32 of 10^3 filters", 1 << 20, 32, 1000),
                 ("2^12 keys x all 10^3 filters", 1 << 12, None, 1000),
                 ("64 keys x all 10^5 filters", 64, None, 100_000),
                 # many tiles AND many list chunks: where hashing a tile again per chunk costs most
                 ("2^16 keys x all 10^3 filters", 1 << 16, None, 1000)]
FILL_PER_FILTER = SIZE // 2     # half full: 5,000 of the 10,000 keys a filter is sized for
FILL_BATCH = 1 << 24


def timed_pair(fns, runs: int, warmup: int):
    """The functions run alternately, HIP events around each call on the null stream; per
    function the sorted ms of the runs after the warm-up."""
    ms = [[] for _ in fns]
    for i in range(warmup + runs):
        for which, fn in enumerate(fns):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms[which].append(e0.elapsed_time(e1))
    return [sorted(x) for x in ms]


def spread(ms, pairs: int) -> dict:
    med = statistics.median(ms)
    return {"ms": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "Gpairs_per_s": round(pairs / (med * 1e-3) / 1e9, 2)}


def fill_half(bank, nf: int) -> None:
    """FILL_PER_FILTER random 12-byte keys into every filter, generated on the device."""
    total, gen = nf * FILL_PER_FILTER, torch.Generator(device="cuda").manual_seed(0xAC2055)
    offs = torch.arange(FILL_BATCH + 1, dtype=torch.int64, device="cuda") * KEY_BYTES
    for a in range(0, total, FILL_BATCH):
        cn = min(FILL_BATCH, total - a)
        keys = torch.randint(0, 256, (cn * KEY_BYTES + 16,), dtype=torch.uint8, device="cuda", generator=gen)
        ids = (torch.arange(a, a + cn, dtype=torch.int64, device="cuda") % nf).to(torch.int32)
        bank.insert_many_dev(keys.data_ptr(), offs.data_ptr(), ids.data_ptr(), cn, stream=0)
        torch.cuda.synchronize()


def run_across(pkg, m, k, label, n, listed, nf, runs, warmup) -> dict:
    rng = np.random.default_rng([0xAC2055, n, nf])
    ids = None if listed is None else rng.choice(nf, listed, replace=False).astype(np.uint32)
    count = nf if ids is None else len(ids)
    pairs = n * count
    buf, offs = decimal_keys(n)
    dk, do = to_dev(buf, offs)
    # the crossed batch: key j once per list entry, the ids tiled, all on the device
    d_listed = torch.arange(nf, dtype=torch.int32, device="cuda") if ids is None else \
        torch.from_numpy(ids.view(np.int32).copy()).cuda()
    xk = torch.cat([dk[:-16].view(n, KEY_BYTES).repeat_interleave(count, dim=0).reshape(-1), dk[-16:]])
    xo = torch.arange(pairs + 1, dtype=torch.int64, device="cuda") * KEY_BYTES
    xi = d_listed.repeat(n)
    out8 = torch.zeros(pairs, dtype=torch.uint8, device="cuda")
    res = {"shape": label, "keys": n, "listed": count, "n_filters": nf, "pairs": pairs}
    with pkg.FilterBank(m, k, nf, device=0) as bank:
        row = bank.across_row_bytes(count)
        res["device_bytes"], res["mask_bytes"], res["crossed_key_bytes"] = bank.device_bytes, n * row, pairs * KEY_BYTES
        mask = torch.full((n * row,), 0xFF, dtype=torch.uint8, device="cuda")
        fill_half(bank, nf)
        # the first query keys are members of one listed filter each (at most 16 more keys per
        # filter), so both answers occur
        members = min(n, 16 * count)
        home = d_listed[torch.from_numpy(rng.integers(0, count, members)).cuda()]
        bank.insert_many_dev(dk.data_ptr(), do.data_ptr(), home.data_ptr(), members, stream=0)
        torch.cuda.synchronize()
        d_ids = 0 if ids is None else d_listed.data_ptr()
        t_across, t_crossed = timed_pair(
            [lambda: bank.include_across_dev(dk.data_ptr(), do.data_ptr(), n, mask.data_ptr(), d_ids, count, stream=0),
             lambda: bank.include_many_dev(xk.data_ptr(), xo.data_ptr(), xi.data_ptr(), pairs, out8.data_ptr(), stream=0)],
            runs, warmup)
        torch.cuda.synchronize()
        bank.sync()
        # the same answers, once, outside the timed region
        shifts = torch.arange(8, dtype=torch.uint8, device="cuda")
        bits = ((mask.view(n, row, 1) >> shifts) & 1).view(n, row * 8)
        assert bool((bits[:, :count] == out8.view(n, count)).all()), "the cross query and the crossed batch differ"
        assert not bool(bits[:, count:].any())
        res["hits"] = int(out8.sum())
        assert res["hits"] >= members
    res["across"], res["crossed"] = spread(t_across, pairs), spread(t_crossed, pairs)
    res["ratio"] = round(res["crossed"]["ms"] / res["across"]["ms"], 2)
    res["ratio_min"] = round(t_crossed[0] / t_across[-1], 2)      # the baseline's fastest run over the query's slowest
    res["ratio_max"] = round(t_crossed[-1] / t_across[0], 2)
    return res


# ---- --combine: folds and the overlap matrix against export + numpy + import ----------------------

BIG_M = 958_505_838     # 100M @ 1 %: 120 MB a filter


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def timed_alternating(fns, befores, runs: int, warmup: int):
    """timed_pair with an untimed step before each call (None: nothing)."""
    ms = [[] for _ in fns]
    for i in range(warmup + runs):
        for which, fn in enumerate(fns):
            if befores[which]:
                befores[which]()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms[which].append(e0.elapsed_time(e1))
    return [sorted(x) for x in ms]


def span(ms) -> dict:
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def ratios(res: dict, new, base) -> dict:
    res["new"], res["baseline"] = span(new), span(base)
    res["ratio"] = round(res["baseline"]["ms"] / res["new"]["ms"], 1)
    res["ratio_min"] = round(base[0] / new[-1], 1)      # the baseline's fastest run over the new call's slowest
    res["ratio_max"] = round(base[-1] / new[0], 1)
    res["ranges_overlap"] = bool(base[0] <= new[-1])
    print("%s: %.4f ms against %.4f ms" % (res["shape"], res["new"]["ms"], res["baseline"]["ms"]), file=sys.stderr,
          flush=True)
    return res


def fill_random_bits(bank) -> None:
    """Every filter a random string (each bit set with probability 1/2), imported."""
    rng = np.random.default_rng(0xB16)
    nbytes = (bank.m + 7) // 8
    for f in range(bank.n_filters):
        s = rng.integers(0, 256, nbytes, dtype=np.uint8)
        if bank.m % 8:
            s[-1] &= (0xFF << (8 - bank.m % 8)) & 0xFF
        bank.import_redis(np.array([f], np.uint32), [s.tobytes()])


def host_overlap(buf) -> np.ndarray:
    """AND counts of every pair of exported filters on the host: an exact float matmul of the
    unpacked bits while a count fits a float32's 24 bits, else popcounts of the ANDed words."""
    if buf.shape[1] * 8 < 1 << 24:
        a = np.unpackbits(buf, axis=1).astype(np.float32)
        return (a @ a.T).astype(np.uint64)
    w = buf.view(np.uint64)
    return np.array([[int(np.bitwise_count(x & y).sum(dtype=np.uint64)) for y in w] for x in w], np.uint64)


def run_fold(bank, label, sources, dst, runs, warmup) -> dict:
    """Roll-ups dst[g] = OR(sources[g]): bf_bank_fold_dev against export, numpy OR, import."""
    groups = len(sources)
    seg = np.zeros(groups + 1, np.uint64)
    np.cumsum([len(s) for s in sources], out=seg[1:])
    src = np.concatenate(sources).astype(np.uint32)
    dst = np.asarray(dst, np.uint32)
    d_seg, d_src, d_dst = i64(seg), i32(src), i32(dst)
    d_ch = torch.zeros(groups, dtype=torch.uint8, device="cuda")
    d_sb = torch.zeros(groups, dtype=torch.int64, device="cuda")
    state = {}

    def new():
        bank.fold_dev("or", d_seg.data_ptr(), d_src.data_ptr(), groups, len(src), d_dst.data_ptr(), d_ch.data_ptr(),
                      d_sb.data_ptr(), stream=0)

    def baseline():
        buf, _ = bank.export_filters(src)
        out = np.bitwise_or.reduceat(buf, seg[:-1].astype(np.int64), axis=0)
        nbytes = (bank.m + 7) // 8
        bank.import_redis(dst, [row[:nbytes].tobytes() for row in out])
        state["want"] = out

    t_new, t_base = timed_alternating([new, baseline], [lambda: bank.clear_dev(d_dst.data_ptr(), groups, stream=0), None],
                                      runs, warmup)
    bank.clear_dev(d_dst.data_ptr(), groups, stream=0)
    new()
    torch.cuda.synchronize()
    bank.sync()
    got, _ = bank.export_filters(dst)
    assert np.array_equal(got, state["want"]), "the fold and the host OR differ"
    assert bool(d_ch.all()) and int(d_sb.sum()) == int(bank.bitcount(dst).sum())
    res = ratios({"shape": label, "groups": groups, "sources": len(src), "stride": bank.stride}, t_new, t_base)
    moved = (len(src) + 2 * groups) * bank.stride        # every source and the old destination read, the new one written
    res["new_GB_per_s"] = round(moved / (res["new"]["ms"] * 1e-3) / 1e9, 1)
    return res


def run_overlap(bank, label, ids, runs, warmup, with_fold=False) -> dict:
    """The matrix of a list against itself: bf_bank_overlap_dev against export + host counts."""
    n = bank.n_filters if ids is None else len(ids)
    listed = np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
    d_ids = None if ids is None else i32(listed)
    d_out = torch.full((n * n,), -1, dtype=torch.int64, device="cuda")
    state = {}

    def new():
        bank.overlap_dev(d_out.data_ptr(), 0 if d_ids is None else d_ids.data_ptr(), n, stream=0)

    def baseline():
        state["want"] = host_overlap(bank.export_filters(ids)[0])

    t_new, t_base = timed_alternating([new, baseline], [None, None], runs, warmup)
    torch.cuda.synchronize()
    bank.sync()
    got = d_out.cpu().numpy().view(np.uint64).reshape(n, n)
    assert np.array_equal(got, state["want"]), "the overlap kernel and the host counts differ"
    res = ratios({"shape": label, "rows": n, "cols": n, "stride": bank.stride}, t_new, t_base)
    res["new_filter_GB_per_s"] = round(len(set(listed.tolist())) * bank.stride / (res["new"]["ms"] * 1e-3) / 1e9, 1)
    if with_fold:   # informational: the same matrix as n * n count-only AND pairs of the streaming fold
        pairs = np.stack([np.repeat(listed, n), np.tile(listed, n)], axis=1).reshape(-1)
        d_seg, d_src = i64(np.arange(n * n + 1, dtype=np.uint64) * 2), i32(pairs)
        d_sb = torch.zeros(n * n, dtype=torch.int64, device="cuda")
        (t_fold,) = timed_alternating(
            [lambda: bank.fold_dev("and", d_seg.data_ptr(), d_src.data_ptr(), n * n, 2 * n * n, d_set_bits=d_sb.data_ptr(),
                                   stream=0)], [None], runs, warmup)
        torch.cuda.synchronize()
        bank.sync()
        assert np.array_equal(d_sb.cpu().numpy().view(np.uint64).reshape(n, n), got)
        res["fold_pairs"] = span(t_fold)
        res["fold_pairs_over_overlap"] = round(res["fold_pairs"]["ms"] / res["new"]["ms"], 1)
    return res


def run_combine(pkg, m, k, runs, warmup, only=None) -> list:
    rng = np.random.default_rng(0xC0B1)
    shapes = []
    if only in (None, "small"):
        with pkg.FilterBank(m, k, 1000, device=0) as bank:
            fill_half(bank, 1000)
            bank.clear(np.array([999], np.uint32))
            shapes.append(run_fold(bank, "1 roll-up of 30 of 10^3 filters", [rng.choice(999, 30, replace=False)], [999],
                                   runs, warmup))
            fill_half(bank, 1000)
            shapes.append(run_overlap(bank, "overlap of all 10^3 filters", None, runs, warmup, with_fold=True))
            shapes.append(run_overlap(bank, "overlap of 32 x 32 of 10^3 filters", rng.choice(1000, 32, replace=False), runs,
                                      warmup))
    if only in (None, "many"):
        with pkg.FilterBank(m, k, 10_000, device=0) as bank:
            fill_half(bank, 10_000)
            sources = [rng.choice(9000, 7, replace=False) for _ in range(1000)]
            shapes.append(run_fold(bank, "10^3 roll-ups of 7 of 10^4 filters", sources, np.arange(9000, 10_000), runs, warmup))
    if only in (None, "big"):
        with pkg.FilterBank(BIG_M, 7, 5, device=0) as bank:
            fill_random_bits(bank)
            shapes.append(run_fold(bank, "1 fold of 4 filters of 120 MB", [np.arange(4)], [4], runs, warmup))
            shapes.append(run_overlap(bank, "overlap of 2 x 2 filters of 120 MB", [1, 2], runs, warmup))
    return shapes


# ---- --changes: what listing the flipped bits costs, on the device and at the facade -------------

def run_changes(pkg, m, k, nf, n, buf, offs, runs, warmup) -> dict:
    """run_bank's insert through bf_bank_insert_many_changes_dev (cap = n k) against the call
    without a list, for both flag kinds; every insert starts from the cleared bank."""
    ids = np.random.default_rng([0xBA2C, nf]).integers(0, nf, n).astype(np.uint32)
    dk, do, di = to_dev(buf, offs, ids)
    cap = n * k
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out_ids = torch.zeros(cap, dtype=torch.int32, device="cuda")
    out_bits = torch.zeros(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = {"n_filters": nf, "cap": cap, "list_bytes": cap * 12}
    args = (dk.data_ptr(), do.data_ptr(), di.data_ptr(), n)
    with pkg.FilterBank(m, k, nf, device=0) as bank:
        res["stride"], res["device_bytes"] = bank.stride, bank.device_bytes
        clear = lambda: bank.clear_dev(stream=0)   # noqa: E731
        for seq, name in ((0, "plain"), (1, "seq")):
            without = (lambda: bank.insert_many_seq_dev(*args, flags.data_ptr(), stream=0)) if seq else \
                (lambda: bank.insert_many_dev(*args, flags.data_ptr(), stream=0))
            listing = lambda: bank.insert_many_changes_dev(   # noqa: E731
                *args, d_count=count.data_ptr(), d_out_ids=out_ids.data_ptr(), d_out_bits=out_bits.data_ptr(), cap=cap,
                seq=seq, d_flags=flags.data_ptr(), stream=0)
            t_without, t_listing = timed_alternating([without, listing], [clear, clear], runs, warmup)
            torch.cuda.synchronize()
            bank.sync()
            # the last timed call was the listing one, into the cleared bank: its list is every set bit, once
            total = int(count.item())
            assert total == int(bank.bitcount().sum()), "the list's length is not the bank's bit count"
            named = out_ids[:total].to(torch.int64) * m + out_bits[:total]
            assert int(torch.unique(named).numel()) == total, "a bit is listed twice"
            assert 0 <= int(out_bits[:total].min()) and int(out_bits[:total].max()) < m
            r = {"without_list": span(t_without), "with_list": span(t_listing), "flipped_bits": total}
            r["ratio"] = round(r["with_list"]["ms"] / r["without_list"]["ms"], 3)
            r["ranges_overlap"] = bool(t_listing[0] <= t_without[-1])
            res[name] = r
            print("%d filters, %s: %.3f ms [%.3f, %.3f] without a list, %.3f ms [%.3f, %.3f] with it (%d bits)" % (
                nf, name, r["without_list"]["ms"], t_without[0], t_without[-1], r["with_list"]["ms"], t_listing[0],
                t_listing[-1], total), file=sys.stderr, flush=True)
    return res


def run_changes_facade(pkg, calls: int) -> dict:
    """One ``bank[name].insert(key)`` of a new key into a half-full 10k @ 1 % key name, FakeRedis
    behind it, under the two write-through modes."""
    names = ["tenant:%d" % i for i in range(5)]
    fill = ["fill-%d" % i for i in range(FILL_PER_FILTER)]
    res = {"calls": calls, "key_names": len(names), "fill_per_filter": FILL_PER_FILTER}
    for mode in ("write_through", "write_through_bits"):
        r = pkg.FakeRedis()
        bank = pkg.BloomfilterBank(size=SIZE, error_rate=ERROR_RATE, key_names=names, redis=r, sync=mode)
        for name in names:
            bank.insert_many([name] * len(fill), fill)
        view = bank[names[2]]
        for i in range(20):
            view.insert("warm-%d" % i)
        r.calls.clear()
        bytes0, us = r.bytes_in, []
        for i in range(calls):
            t0 = time.perf_counter()
            view.insert("new-%d" % i)
            us.append((time.perf_counter() - t0) * 1e6)
        us.sort()
        res[mode] = {"us_per_call": round(statistics.median(us), 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1),
                     "bytes_in_per_call": round((r.bytes_in - bytes0) / calls, 1),
                     "setbits_per_call": round(sum(1 for c in r.calls if c[0] == "SETBIT") / calls, 2),
                     "setranges_per_call": round(sum(1 for c in r.calls if c[0] == "SETRANGE") / calls, 2),
                     "string_bytes": len(r.get(names[2]))}
        print("%s: %.1f us per insert, %.1f bytes and %.2f SETBITs per call" % (
            mode, res[mode]["us_per_call"], res[mode]["bytes_in_per_call"], res[mode]["setbits_per_call"]),
            file=sys.stderr, flush=True)
        bank.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", default="1000,100000")
    ap.add_argument("--log2-keys", type=int, default=22)
    ap.add_argument("--hashes", type=int, default=0, help="k (default: Bloomfilter.optimal_k of 10k @ 1 %%)")
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--across", action="store_true",
                    help="time the cross query against the crossed batch instead (profiles/bank_across.json)")
    ap.add_argument("--combine", action="store_true",
                    help="time folds and the overlap matrix against export + numpy + import (profiles/bank_combine.json)")
    ap.add_argument("--seq", action="store_true",
                    help="time the insert with sequential flags against the plain insert and the handles "
                         "(profiles/bank_seq.json)")
    ap.add_argument("--changes", action="store_true",
                    help="time the insert that lists its flipped bits against the one that does not, and a per-key "
                         "facade insert under the two write-through modes (profiles/bank_changes.json)")
    ap.add_argument("--facade-calls", type=int, default=500, help="--changes: timed per-key inserts per sync mode")
    ap.add_argument("--only", choices=["small", "many", "big"], default=None,
                    help="--combine: the shapes of one bank only (10^3 filters, 10^4 filters, 5 x 120 MB)")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20 (the medians quoted in DESIGN.md)")
    if not torch.cuda.is_available():
        sys.exit("bench_bank.py needs a GPU: nothing is timed without one")
    pkg = pkgload.load()
    torch.cuda.set_device(0)
    m = pkg.Bloomfilter.optimal_m(SIZE, ERROR_RATE)
    k = args.hashes or pkg.Bloomfilter.optimal_k(SIZE, m)
    if args.across:
        doc = {"tool": "tools/bench_bank.py --across", "device": torch.cuda.get_device_name(0), "m": m, "k": k,
               "key_bytes": KEY_BYTES, "fill_per_filter": FILL_PER_FILTER, "runs": args.runs, "warmup": args.warmup,
               "shapes": [run_across(pkg, m, k, *shape, args.runs, args.warmup) for shape in ACROSS_SHAPES]}
        line = json.dumps(doc)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    if args.combine:
        doc = {"tool": "tools/bench_bank.py --combine", "device": torch.cuda.get_device_name(0), "m": m, "k": k,
               "big_m": BIG_M, "fill_per_filter": FILL_PER_FILTER, "runs": args.runs, "warmup": args.warmup,
               "shapes": run_combine(pkg, m, k, args.runs, args.warmup, args.only)}
        line = json.dumps(doc)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    n = 1 << args.log2_keys
    buf, offs = decimal_keys(n)
    if args.seq:
        doc = {"tool": "tools/bench_bank.py --seq", "device": torch.cuda.get_device_name(0), "m": m, "k": k, "keys": n,
               "key_bytes": KEY_BYTES, "runs": args.runs, "warmup": args.warmup,
               "banks": {str(nf): run_seq(pkg, m, k, int(nf), n, buf, offs, args.runs, args.warmup)
                         for nf in args.filters.split(",")}}
        line = json.dumps(doc)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    if args.changes:
        doc = {"tool": "tools/bench_bank.py --changes", "device": torch.cuda.get_device_name(0), "m": m, "k": k, "keys": n,
               "key_bytes": KEY_BYTES, "runs": args.runs, "warmup": args.warmup,
               "banks": {str(nf): run_changes(pkg, m, k, int(nf), n, buf, offs, args.runs, args.warmup)
                         for nf in args.filters.split(",")},
               "facade": run_changes_facade(pkg, args.facade_calls)}
        line = json.dumps(doc)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    doc = {"tool": "tools/bench_bank.py", "device": torch.cuda.get_device_name(0), "m": m, "k": k, "keys": n,
           "key_bytes": KEY_BYTES, "runs": args.runs, "warmup": args.warmup,
           "banks": {str(nf): run_bank(pkg, m, k, int(nf), n, buf, offs, args.runs, args.warmup)
                     for nf in args.filters.split(",")}}
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
