"""bf_binned_plan_detail: which kernel variants the binned insert takes for a shape (CPU only).

The binned pipeline picks its front, scan and apply kernels from the shape of the call.  The
GPU tests that are about one of those variants assert it through this description before they
run; this module pins shape -> variant for every shape they rely on and for the project's own
workloads, so a moved threshold fails here, without a GPU.  The expectations are arithmetic
on the constants of the pipeline (written out below), not read back from the library.
"""
import ctypes

import pytest

CU = 256   # compute units of the part the thresholds were tuned on, always passed explicitly

TWO_KEY, SLOTS12, WIDE = 0, 1, 2
ONE_WG, HIER = 0, 1
PER_REGION, PIPE = 0, 1


def dev_bytes(m, k):
    """Device bitset of a whole filter: the reachable prefix in bytes, rounded up to 256."""
    bits = min(m, k * 0xFFFFFFFF + 1)
    return -(-((bits + 7) // 8) // 256) * 256


M_PIPE = 2**31 + 2**18 + 5       # 4097 regions of 2^19 bits: one more than 16 x 256
M_NSTAR = 9585058377             # 1B@1 % (north star), k = 6
M_10B = 13 * (2**32 - 1) + 1     # the 10B@0.01 % filter's reachable prefix, k = 13
M_1M = 9585058                   # 1M@1 %
M_10K = 95851                    # 10k@1 %: one region at every size
M_100M = 1437758757              # 100M@0.1 %, k = 10


def detail(pkg, m, k, n, pref=19, cu=CU):
    return pkg._lib.binned_plan_detail(dev_bytes(m, k), k, n, pref, cu)


def test_device_bytes_helper_agrees(pkg):
    for m, k in [(M_PIPE, 16), (M_NSTAR, 6), (M_10B, 13), (191701167547, 13), (M_1M, 6), (M_10K, 6), (1, 1)]:
        assert pkg._lib.device_bytes_for(m, k) == dev_bytes(m, k)
    assert dev_bytes(M_10B, 13) * 8 == 106496 << 19   # exactly 13 x 8192 regions


# (m, k, n, preferred region log2) -> the fields that must hold
TABLE = [
    # the pipelined tests' filter: 4097 regions, 4097 x 4096 = 16,781,312 vectors of 16 B
    ((M_PIPE, 16, 1_050_000, 19), dict(region_log2=19, regions=4097, superbins=129, density=2, apply=PIPE,
                                       scan=ONE_WG, front=WIDE, apply_loads=0, tiles=1026, tiles_per_block=3,
                                       groups=6, passes=1)),
    ((M_PIPE, 6, 2_800_000, 19), dict(regions=4097, density=2, apply=PIPE, front=TWO_KEY, scan=ONE_WG,
                                      tiles=1368, passes=1)),
    # 2^20 keys x 16 = 16,777,216 probes < 16,781,312: why a host-pointer call (cut into 2^20-key
    # chunks) never pipelines on this filter
    ((M_PIPE, 16, 1 << 20, 19), dict(regions=4097, density=1, apply=PER_REGION, apply_loads=2, front=WIDE)),
    # north star: 18,283 regions, 100.7 M probes over 74.9 M vectors
    ((M_NSTAR, 6, 1 << 24, 19), dict(region_log2=19, regions=18283, superbins=143, density=2, apply=PIPE,
                                     scan=ONE_WG, front=TWO_KEY, tiles=8192, tiles_per_block=16, groups=8,
                                     passes=1)),
    # 10B step: 218 M probes over 436 M vectors, 2048 per region
    ((M_10B, 13, 1 << 24, 19), dict(region_log2=19, regions=106496, superbins=208, density=1, apply=PER_REGION,
                                    apply_loads=2, scan=ONE_WG, front=WIDE, groups=16, passes=1)),
    # test_gpu_merged: 436,368,101 probes >= 436,207,616 vectors; 208 x 33 = 6864 windows > 4096
    ((M_10B, 13, (1 << 25) + 12345, 19), dict(regions=106496, superbins=208, groups=33, density=2, apply=PIPE,
                                              scan=HIER, front=WIDE, tiles=32781, tiles_per_block=16, passes=1)),
    ((191701167547, 13, (1 << 25) + 12345, 19), dict(regions=106496, density=2, apply=PIPE, scan=HIER)),
    # the per-region matrix: 1M@1 % at every region size, line-dense and vector-dense
    ((M_1M, 6, 5_000, 18), dict(region_log2=18, regions=37, superbins=37, density=1, apply=PER_REGION, apply_loads=0)),
    ((M_1M, 6, 20_000, 18), dict(region_log2=18, regions=37, density=2, apply=PER_REGION, apply_loads=0)),
    ((M_1M, 6, 5_000, 19), dict(region_log2=19, regions=19, density=1, apply=PER_REGION, apply_loads=2)),
    ((M_1M, 6, 20_000, 19), dict(region_log2=19, regions=19, density=2, apply=PER_REGION, apply_loads=8)),
    ((M_1M, 6, 5_000, 20), dict(region_log2=20, regions=10, superbins=10, density=1, apply=PER_REGION, apply_loads=0)),
    ((M_1M, 6, 20_000, 20), dict(region_log2=20, regions=10, density=2, apply=PER_REGION, apply_loads=0)),
    ((M_10K, 6, 2_000, 18), dict(region_log2=18, regions=1, superbins=1, density=2, apply=PER_REGION)),
    ((M_10K, 6, 2_000, 19), dict(region_log2=19, regions=1, density=2, apply=PER_REGION, apply_loads=8)),
    ((M_10K, 6, 2_000, 20), dict(region_log2=20, regions=1, density=2, apply=PER_REGION)),
    # sparse rows of the matrix
    ((M_100M, 10, 3_000, 18), dict(region_log2=18, regions=5485, density=0, apply=PER_REGION, front=SLOTS12)),
    ((M_100M, 10, 3_000, 19), dict(region_log2=19, regions=2743, density=0, apply=PER_REGION, apply_loads=2)),
    ((M_100M, 10, 3_000, 20), dict(region_log2=20, regions=1372, density=0, apply=PER_REGION)),
    # run-table passes: one superbin, 9 M probes = 1099 chunk blocks of 8192
    ((M_10K, 6, 1_500_000, 19), dict(regions=1, superbins=1, groups=6, density=2, apply=PER_REGION, apply_loads=8,
                                     tiles=733, tiles_per_block=2)),
    # second run-table pass of the pipelined kernel: 9.05 M keys, k = 6
    ((M_PIPE, 6, 9_050_000, 19), dict(regions=4097, superbins=129, groups=8, density=2, apply=PIPE, scan=ONE_WG,
                                      front=TWO_KEY, tiles=4419, tiles_per_block=9)),
]


@pytest.mark.parametrize("shape,want", TABLE, ids=["%d-k%d-n%d-r%d" % s for s, _ in TABLE])
def test_shape_to_variant(pkg, shape, want):
    m, k, n, pref = shape
    d = detail(pkg, m, k, n, pref)
    assert d["planned"] == 1 and d["binned"] == 1
    got = {f: d[f] for f in want}
    assert got == want, d
    assert d["scratch_bytes"] >= 2 * 4 * n * k   # the two 4-byte probe arrays


def test_density_lines(pkg):
    """One key either side of both density lines, on the 4097-region filter at k = 16: the
    16,781,312 vectors are 16 x 1,048,832 and an eighth of them 16 x 131,104."""
    vecs = 4097 * 4096
    assert vecs == 16 * 1_048_832 and vecs // 8 == 16 * 131_104
    assert detail(pkg, M_PIPE, 16, 1_048_832)["density"] == 2
    assert detail(pkg, M_PIPE, 16, 1_048_831)["density"] == 1
    assert detail(pkg, M_PIPE, 16, 131_104)["density"] == 1
    assert detail(pkg, M_PIPE, 16, 131_103)["density"] == 0
    # the pipelined form follows density 2 exactly
    assert detail(pkg, M_PIPE, 16, 1_048_832)["apply"] == PIPE
    assert detail(pkg, M_PIPE, 16, 1_048_831)["apply"] == PER_REGION
    # the per-region kernel's loads: 8 above 4096 probes per region on average (k = 1: n = probes)
    few = pkg._lib.binned_plan_detail(19 << 16, 1, 19 * 4096, 19, CU)
    many = pkg._lib.binned_plan_detail(19 << 16, 1, 19 * 4096 + 1, 19, CU)
    assert (few["apply_loads"], many["apply_loads"]) == (2, 8)


def test_pipeline_needs_16_regions_per_compute_unit(pkg):
    lib = pkg._lib
    for regions, want in ((16 * CU - 1, PER_REGION), (16 * CU, PIPE)):
        d = lib.binned_plan_detail(regions << 16, 16, 1_100_000, 19, CU)   # 17.6 M probes: density 2 on both
        assert (d["regions"], d["density"], d["apply"]) == (regions, 2, want)
        assert d["apply_loads"] == (8 if want == PER_REGION else 0)
    # the same 4097 regions on parts of other sizes
    assert detail(pkg, M_PIPE, 16, 1_050_000, cu=257)["apply"] == PER_REGION   # 16 x 257 = 4112
    assert detail(pkg, M_PIPE, 16, 1_050_000, cu=128)["apply"] == PIPE
    # compute_units = 0 asks the current device; without one the library assumes 256
    import torch
    if not torch.cuda.is_available():
        assert detail(pkg, M_PIPE, 16, 1_050_000, cu=0) == detail(pkg, M_PIPE, 16, 1_050_000, cu=256)
    # only 2^19-bit regions are pipelined
    for pref in (18, 20):
        d = detail(pkg, M_PIPE, 16, 4_200_000, pref)
        assert (d["region_log2"], d["density"], d["apply"]) == (pref, 2, PER_REGION)


def test_scan_switches_above_4096_windows(pkg):
    """256 superbins (131,072 regions): 16 groups = 4096 windows stay on the one-workgroup scan,
    17 take the hierarchical one.  A group is 64 front workgroups of 16 tiles of 1024 keys."""
    nbytes = 131072 << 16
    per_group = 64 * 16 * 1024
    a = pkg._lib.binned_plan_detail(nbytes, 13, 16 * per_group, 19, CU)
    b = pkg._lib.binned_plan_detail(nbytes, 13, 16 * per_group + 1, 19, CU)
    assert (a["superbins"], a["groups"], a["scan"]) == (256, 16, ONE_WG)
    assert (b["superbins"], b["groups"], b["scan"]) == (256, 17, HIER)


def test_fronts_by_k(pkg):
    assert [detail(pkg, M_NSTAR, k, 100_000)["front"] for k in (1, 6, 7, 12, 13, 16)] == \
        [TWO_KEY, TWO_KEY, SLOTS12, SLOTS12, WIDE, WIDE]
    # two keys per lane: tiles of 2048 keys
    assert detail(pkg, M_NSTAR, 6, 2049)["tiles"] == 2 and detail(pkg, M_NSTAR, 7, 2049)["tiles"] == 3


def test_shapes_outside_the_binned_path(pkg):
    zero = {f: 0 for f, _ in pkg._lib.bf_plan_detail._fields_}
    for k, n in ((0, 1000), (17, 1000), (6, 0)):
        assert detail(pkg, M_NSTAR, k, n) == zero
    # more than 256 superbins of 2^9 regions of 2^20 bits: no geometry
    d = pkg._lib.binned_plan_detail(131072 << 17, 6, 1000, 19, CU)
    assert (d["planned"], d["region_log2"], d["regions"], d["superbins"]) == (1, 20, 131072, 256)
    assert pkg._lib.binned_plan_detail(131073 << 17, 6, 1000, 19, CU)["planned"] == 0
    assert pkg._lib.load().bf_binned_plan_detail(1 << 20, 6, 1000, 19, CU, None) == pkg._lib.BF_EINVAL
    assert pkg._lib.load().bf_insert_plan_detail(None, 1000, ctypes.byref(pkg._lib.bf_plan_detail())) == \
        pkg._lib.BF_EINVAL


def test_larger_batches_go_in_passes(pkg):
    """A batch beyond one launch's 16384 front workgroups x 16 tiles is cut into sub-batches;
    the description is of the first."""
    one = 16384 * 16 * 2048   # k <= 6: 2048 keys per tile; 2 superbins x 256 groups fit the scan
    d = pkg._lib.binned_plan_detail(1 << 17, 1, one, 19, CU)
    assert (d["planned"], d["passes"], d["tiles"]) == (1, 1, 16384 * 16)
    d = pkg._lib.binned_plan_detail(1 << 17, 1, 2 * one + 1, 19, CU)
    assert (d["planned"], d["passes"], d["tiles"]) == (1, 3, 16384 * 16)
