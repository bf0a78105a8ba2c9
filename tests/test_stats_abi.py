"""The statistics entry points of include/bfhip.h (bf_bitcount, bf_bitop, bf_bitcount_op,
bf_estimate_count) as far as they go without a GPU: exported symbols, argument checks, and
the host-only size estimate against closed forms and a measured case."""
import ctypes
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUBY = os.path.join(ROOT, "redis-bloomfilter_amd", "ruby", "lib")

NEW = ["bf_bitcount", "bf_bitcount_dev", "bf_bitop", "bf_bitop_dev", "bf_bitcount_op", "bf_estimate_count"]

NORTH_STAR = (9_585_058_377, 6)   # 1B keys @ 1 %


def textbook(m, k, x):
    return -(m / k) * math.log(1.0 - x / m)


def test_new_symbols_exported_and_null_arguments_refused(pkg):
    lib = pkg._lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    for name in NEW:
        assert name in exported and name in pkg._lib.SIGNATURES, name
    n, ch, d = ctypes.c_uint64(7), ctypes.c_uint8(7), ctypes.c_double(7.0)
    E = pkg._lib.BF_EINVAL
    assert lib.bf_bitcount(None, 0, 1, ctypes.byref(n)) == E
    assert lib.bf_bitcount_dev(None, 0, 1, None, None) == E
    assert lib.bf_bitop(None, pkg._lib.BF_BITOP_OR, None, ctypes.byref(ch), ctypes.byref(n)) == E
    assert lib.bf_bitop_dev(None, pkg._lib.BF_BITOP_OR, None, None, None, None) == E
    assert lib.bf_bitcount_op(None, pkg._lib.BF_BITOP_XOR, None, ctypes.byref(n)) == E
    assert lib.bf_bitcount_op(None, pkg._lib.BF_BITOP_XOR, None, None) == E
    assert lib.bf_estimate_count(9585, 6, 0, 10, None) == E
    assert lib.bf_estimate_count(0, 6, 0, 0, ctypes.byref(d)) == E
    assert lib.bf_estimate_count(9585, 0, 0, 10, ctypes.byref(d)) == E
    assert lib.bf_estimate_count(9585, 65, 0, 10, ctypes.byref(d)) == E
    assert (n.value, ch.value, d.value) == (7, 7, 7.0)       # nothing written on refusal
    assert (pkg._lib.BF_BITOP_AND, pkg._lib.BF_BITOP_OR, pkg._lib.BF_BITOP_XOR) == (0, 1, 2)


def test_estimate_count_edge_cases(pkg):
    est = pkg._lib.estimate_count
    for m, k in [(9585, 6), (9_585_058, 6), (1 << 32, 3)] + [NORTH_STAR]:
        assert est(m, k, 0) == 0.0
        with pytest.raises(pkg.ArgumentError):
            est(m, k, m + 1)
    for m, k in [(9585, 6), (9_585_058, 6), (1 << 32, 3)]:
        assert est(m, k, m) == math.inf
        assert est(m, k, m, pkg.BF_FLAG_ENGINE_MD5) == math.inf
    # the ruby derivation of one hash only ever reaches the first 2^32 bits (ruby.rb:51)
    assert est(1 << 34, 1, 1 << 32) == math.inf
    assert math.isfinite(est(1 << 34, 1, (1 << 32) - 1000))


@pytest.mark.parametrize("m,k", [(9585, 6), (9_585_058, 6), NORTH_STAR, (19_170_116_755, 13)])
def test_estimate_count_is_strictly_increasing(pkg, m, k):
    xs = [max(1, int(m * 0.9 * (i + 1) / 50)) for i in range(50)]
    vals = [pkg._lib.estimate_count(m, k, x) for x in xs]
    assert all(math.isfinite(v) and v > 0 for v in vals)
    assert all(b > a for a, b in zip(vals, vals[1:])), vals


def test_estimate_count_flat_density_agreement(pkg):
    """m << 2^32 folds every probe's density about 448 times over [0, m): flat to second
    order, so the model must reproduce the textbook formula (1e-6 relative); with a hash
    engine flag the probes ARE uniform and it is the formula (1e-12), at any m."""
    m, k = 9_585_058, 6
    for frac in (0.01, 0.17, 0.47, 0.9):
        x = int(m * frac)
        got, want = pkg._lib.estimate_count(m, k, x), textbook(m, k, x)
        print("m=%d X/m=%.2f model=%.6f textbook=%.6f rel=%.3e" % (m, frac, got, want, (got - want) / want))
        assert abs(got - want) <= 1e-6 * want
    for mm, kk in [(m, k), NORTH_STAR, (19_170_116_755, 13), (9585, 6)]:
        for flag in (pkg.BF_FLAG_ENGINE_MD5, pkg.BF_FLAG_ENGINE_SHA1):
            for frac in (0.01, 0.17, 0.47, 0.9):
                x = int(mm * frac)
                got, want = pkg._lib.estimate_count(mm, kk, x, flag), textbook(mm, kk, x)
                assert abs(got - want) <= 1e-12 * want, (mm, kk, flag, frac)


def test_estimate_count_known_answer(pkg):
    """SHA-1 of 2^22 distinct keys set X = 25,130,685 bits of the north-star filter.  The
    bound is four standard errors of the collision count, 4 sqrt(n k - X) / k = 125 keys;
    the textbook formula (4,193,948) misses it."""
    m, k = NORTH_STAR
    n, x = 1 << 22, 25_130_685
    bound = 4.0 * math.sqrt(n * k - x) / k
    assert 124.0 < bound < 126.0
    got = pkg._lib.estimate_count(m, k, x)
    print("estimate %.2f, error %.2f, bound %.2f; textbook %.2f" % (got, got - n, bound, textbook(m, k, x)))
    assert abs(got - n) <= 125
    assert abs(textbook(m, k, x) - n) > 125


def _ruby(path):
    return open(os.path.join(RUBY, path)).read()


def test_ruby_binding_attaches_the_new_functions_and_delegates():
    """Static, as tests/test_abi.py does for the rest of hip.rb (no Ruby interpreter here)."""
    rb = _ruby("bloomfilter_driver/hip.rb")
    attached = set(re.findall(r"attach_function :(bf_\w+),", rb))
    assert set(NEW) <= attached
    methods = set(re.findall(r"^\s*def (\w+[?!]?)", rb, re.M))
    assert {"count_bits", "fill_ratio", "estimated_size", "merge", "union_size", "intersection_size"} <= methods
    batch = _ruby("redis/bloomfilter/batch.rb")
    for name in ("count_bits", "fill_ratio", "estimated_size", "merge", "union_size", "intersection_size"):
        assert re.search(r"^\s*def %s\b" % name, batch, re.M), name
        assert re.search(r"\.%s\b" % name, batch), "%s does not reach the driver" % name
    assert "NotImplementedError" in batch


def test_facade_refuses_drivers_without_statistics(pkg):
    """A driver without the method raises NotImplementedError naming the driver (no device
    needed: the check comes before any driver call)."""

    class Plain:
        def __init__(self, options):
            self.redis = None

    pkg.register_driver(Plain, "PlainStats")
    try:
        bf = pkg.Bloomfilter(size=100, error_rate=0.01, driver="plain-stats", redis=pkg.FakeRedis())
        for call in (bf.count_bits, bf.fill_ratio, bf.estimated_size, lambda: bf.merge(bf),
                     lambda: bf.union_size(bf), lambda: bf.intersection_size(bf)):
            with pytest.raises(NotImplementedError, match="plain-stats"):
                call()
    finally:
        pkg.DRIVERS.pop("PlainStats", None)
