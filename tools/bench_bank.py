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
    n = 1 << args.log2_keys
    buf, offs = decimal_keys(n)
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
