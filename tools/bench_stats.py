#!/usr/bin/env python3
"""Time the statistics kernels (bf_stats.hip) against what the library offered before them.

For each filter (north-star 1B @ 1 % and 10B @ 0.01 %, both half full of random bits):

    bitcount            bf_bitcount_dev over the whole string
    bitop_or_changing   bf_bitop_dev(OR) into an empty filter: every vector is stored
    bitop_or_unchanged  the same OR again: nothing changes, no vector is stored
    bitcount_op_or/xor  bf_bitcount_op (synchronous: a host clock around a call that ends in a
                        stream synchronise)

each the median of --runs runs after --warmup, HIP events around the *_dev calls, with the
bytes the kernel must move per second.  Then the same two jobs the way a caller had to do them
without these entry points, timed with a host clock in the same process:

    host_bitcount       export_redis + a NumPy table popcount on the host
    host_merge          export_redis + import_redis(BF_IMPORT_OR)

One JSON line on stdout (and in --out).

    python tools/bench_stats.py [--configs nstar,10b] [--runs 25] [--out profiles/stats_ops.json]
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

import bench  # noqa: E402
import pkgload  # noqa: E402

POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def host_popcount(data: bytes, chunk: int = 64 << 20) -> int:
    a = np.frombuffer(data, np.uint8)
    return sum(int(POP8[a[i:i + chunk]].sum(dtype=np.uint64)) for i in range(0, len(a), chunk))


def zero_bits(f) -> None:
    ptr, nbytes = f.device_bits()
    torch.as_tensor(bench._DevBytes(ptr, nbytes), device="cuda").zero_()


def timed_events(fn, runs: int, warmup: int, before=None):
    """Median / min ms of fn() between two events on the null stream (the stream fn launches on)."""
    ms = []
    for i in range(warmup + runs):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def timed_host(fn, runs: int, warmup: int):
    ms = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def entry(med_min, nbytes: int) -> dict:
    med, lo = med_min
    return {"ms": round(med, 4), "min_ms": round(lo, 4), "bytes": nbytes, "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}


def run_config(pkg, name: str, runs: int, warmup: int, base_runs: int) -> dict:
    n, p = bench.CONFIGS[name][:2]
    m = pkg.Bloomfilter.optimal_m(n, p)
    k = pkg.Bloomfilter.optimal_k(n, m)
    a, b, c = (pkg.Filter(m, k, device=0) for _ in range(3))
    bench.prefill_random(a, m, k, 0, host_copy=False)
    bench.prefill_random(b, m, k, 1, host_copy=False)
    nb = a.device_bytes
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    chg = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {"m": m, "k": k, "device_bytes": nb, "runs": runs, "warmup": warmup}

    out["bitcount"] = entry(timed_events(lambda: a.bitcount_dev(cnt.data_ptr(), stream=0), runs, warmup), nb)
    bits_a = int(cnt.item())
    out["bitop_or_changing"] = entry(
        timed_events(lambda: c.bitop_dev("or", a, chg.data_ptr(), cnt.data_ptr(), stream=0), runs, warmup,
                     before=lambda: zero_bits(c)), 3 * nb)
    assert int(cnt.item()) == bits_a and int(chg.item()) == 1
    chg.zero_()
    out["bitop_or_unchanged"] = entry(
        timed_events(lambda: c.bitop_dev("or", a, chg.data_ptr(), cnt.data_ptr(), stream=0), runs, warmup), 2 * nb)
    assert int(cnt.item()) == bits_a and int(chg.item()) == 0
    out["bitcount_op_or"] = entry(timed_host(lambda: a.bitcount_op("or", b), runs, warmup), 2 * nb)
    out["bitcount_op_xor"] = entry(timed_host(lambda: a.bitcount_op("xor", b), runs, warmup), 2 * nb)

    # the same jobs through the host, as before these entry points
    got = []
    hb = timed_host(lambda: got.append(host_popcount(a.export_redis())), base_runs, 0)
    assert got[-1] == bits_a, (got[-1], bits_a)
    zero_bits(c)
    hm = timed_host(lambda: c.import_redis(a.export_redis(), pkg.BF_IMPORT_OR), base_runs, 0)
    assert c.bitcount_op("xor", a) == 0
    out["host_bitcount"] = {"ms": round(hb[0], 1), "min_ms": round(hb[1], 1), "runs": base_runs}
    out["host_merge"] = {"ms": round(hm[0], 1), "min_ms": round(hm[1], 1), "runs": base_runs}
    out["speedup_bitcount"] = round(hb[0] / out["bitcount"]["ms"], 1)
    out["speedup_merge"] = round(hm[0] / out["bitop_or_changing"]["ms"], 1)
    for f in (a, b, c):
        f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="nstar,10b")
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20 (the medians quoted in DESIGN.md)")
    if not torch.cuda.is_available():
        sys.exit("bench_stats.py needs a GPU: nothing is timed without one")
    pkg = pkgload.load()
    torch.cuda.set_device(0)
    doc = {"tool": "tools/bench_stats.py", "device": torch.cuda.get_device_name(0),
           "configs": {name: run_config(pkg, name, args.runs, args.warmup, args.baseline_runs)
                       for name in args.configs.split(",")}}
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
