"""The binned insert's size-gated kernel variants against the CPU oracle.

The binned pipeline (bf_binned.hip) picks its kernels from the shape of the call: the
persistent pipelined apply for vector-dense batches over many 2^19-bit regions, the
per-region apply's read-first (density 1) and store-everything (density 2) branches at every
region size, extra run-table passes for a superbin of more than 1024 chunk blocks.  Every
test here first asserts, through ``insert_plan_detail``, that its call takes the variant it
is about, then compares with the oracle: the Redis string byte for byte, the include? answers,
``any_new``, and with dirty tracking the reported 64 KiB blocks against the blocks whose bytes
changed.  The binned apply marks a block only for a 16-byte vector that gained a bit, so the
two sets are equal, not merely nested.

Calls go through the device-pointer API in one launch each: a host-pointer call is cut into
chunks of 2^20 keys, which changes the plan.  Where a batch repeats one key many times the
oracle inserts it once: OR is idempotent.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 65536
PIPE, PER_REGION = 1, 0

M_PIPE = 2**31 + 2**18 + 5   # 4097 regions of 2^19 bits = 16 x 256 + 1: workgroup 0 of 256 walks 17
#                              regions and the others 16 (both exits of the pipeline's unrolled loop);
#                              the last region is half empty
ENV = ("BFHIP_INSERT_BINNED", "BFHIP_INCLUDE_BINNED", "BFHIP_BIN_REGION_LOG2")


def cat(*batches):
    """Packed key batches (bytes, offsets) joined into one."""
    bufs, offs, base = [], [np.zeros(1, np.uint64)], np.uint64(0)
    for b, o in batches:
        o = np.asarray(o, np.uint64)
        bufs.append(b[int(o[0]):int(o[-1])])
        offs.append(o[1:] - o[0] + base)
        base = base + o[-1] - o[0]
    return np.concatenate(bufs), np.concatenate(offs)


def rand_keys(rng, n, lo=0, hi=24):
    lens = rng.integers(lo, hi + 1, size=n)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    return rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs


class Dev:
    """A packed batch on the device (16 readable bytes past the last key)."""

    def __init__(self, batch):
        import torch
        buf, offs = batch
        self.n = len(offs) - 1
        self.kb = torch.from_numpy(np.concatenate([buf, np.zeros(16, np.uint8)])).cuda()
        self.ko = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()


def insert_dev(f, d):
    """One insert_many_dev launch of the whole batch -> any_new."""
    import torch
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # the handle launches on its own non-blocking stream
    f.insert_many_dev(d.kb.data_ptr(), d.ko.data_ptr(), d.n, d_any_new=flag.data_ptr())
    torch.cuda.synchronize()
    return bool(flag.item())


def include_dev(f, d):
    import torch
    out = torch.full((d.n,), 7, dtype=torch.uint8, device="cuda")   # 7: an answer never written shows
    torch.cuda.synchronize()
    f.include_many_dev(d.kb.data_ptr(), d.ko.data_ptr(), d.n, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def as_array(s, size):
    a = np.zeros(size, np.uint8)
    a[: len(s)] = np.frombuffer(s, np.uint8)
    return a


def same_string(got: bytes, want: bytes):
    assert len(got) == len(want)
    assert got == want


def changed_blocks(s0: bytes, s1: bytes):
    size = -(-max(len(s0), len(s1), 1) // BLOCK) * BLOCK
    diff = (as_array(s0, size) != as_array(s1, size)).reshape(-1, BLOCK).any(axis=1)
    return set(np.flatnonzero(diff).tolist())


def blocks_of(ranges):
    out = set()
    for off, ln in ranges:
        assert off % BLOCK == 0 and ln > 0
        out.update(range(off // BLOCK, (off + ln - 1) // BLOCK + 1))
    return out


def check_dirty(f, s0, s1):
    """The reported blocks are exactly the changed ones, and replaying them rebuilds s1."""
    ranges, rlen = f.dirty_ranges(clear=True)
    assert rlen == len(s1)
    assert blocks_of(ranges) == changed_blocks(s0, s1)
    rebuilt = as_array(s0, max(len(s0), len(s1)))
    for off, ln in ranges:
        rebuilt[off:off + ln] = np.frombuffer(f.export_range(off, ln), np.uint8)
    assert rebuilt[: len(s1)].tobytes() == s1 and not rebuilt[len(s1):].any()
    return ranges


def assert_pipelined(f, n, **more):
    d = f.insert_plan_detail(n)
    want = dict(planned=1, binned=1, passes=1, region_log2=19, regions=4097, density=2, apply=PIPE, **more)
    assert {key: d[key] for key in want} == want, d
    assert f.insert_plan(n) == {"binned": True, "scratch_bytes": d["scratch_bytes"]}
    return d


@pytest.fixture
def default_env(monkeypatch):
    for name in ENV:   # the automatic policy itself must pick the binned path
        monkeypatch.delenv(name, raising=False)


class Ref:
    """A batch, the oracle's bitset after inserting it into an empty filter, and the string."""

    def __init__(self, oracle, m, k, batch, base=None):
        self.m, self.k, self.batch = m, k, batch
        self.bits = oracle.new_bitset(m, k) if base is None else base.copy()
        self.any_new, _ = oracle.insert_many(self.bits, m, k, batch[0], batch[1])
        self.bits.setflags(write=False)
        self.string = oracle.redis_string(self.bits)


@pytest.fixture(scope="module")
def uniform16(pkg, oracle):
    """1,050,000 random decimal keys at k = 16 on the 4097-region filter: 16.8 M probes over
    16,781,312 vectors (shared, read-only)."""
    rng = np.random.default_rng(0xD15E)
    vals = rng.integers(0, 10**12, size=1_050_000)
    ref = Ref(oracle, M_PIPE, 16, pkg.keys.pack_decimal(vals))
    ref.vals = vals
    return ref


def _uniform(pkg, oracle, ref, front):
    m, k = ref.m, ref.k
    rng = np.random.default_rng(0xD15E + k)
    d = Dev(ref.batch)
    members = rng.choice(ref.vals, size=20_000, replace=False)
    probe = pkg.keys.pack_decimal(np.concatenate([members, rng.integers(10**12, 2 * 10**12, size=5_000)]))
    with pkg.Filter(m, k, device=0) as f:
        assert_pipelined(f, d.n, superbins=129, scan=0, front=front)
        assert insert_dev(f, d) is True
        same_string(f.export_redis(), ref.string)
        # the repeat finds every bit set: the kernel's fresh == 0 exit
        assert insert_dev(f, d) is False
        same_string(f.export_redis(), ref.string)
        got = include_dev(f, Dev(probe))
    want = oracle.include_many(ref.bits, m, k, probe[0], probe[1])
    np.testing.assert_array_equal(got, want)
    assert got[:20_000].all()


def test_pipelined_apply_uniform_k16(pkg, oracle, default_env, uniform16):
    """bin_apply_pipe_kernel behind the wide (16-slot) front: string, any_new True then False
    with the string unchanged, include? of 20 k members and 5 k fresh keys."""
    _uniform(pkg, oracle, uniform16, front=2)


def test_pipelined_apply_uniform_k6(pkg, oracle, default_env):
    """The same at the north star's k = 6 (two keys per lane in the front): 2,800,000 keys."""
    rng = np.random.default_rng(0xD15E + 1)
    vals = rng.integers(0, 10**12, size=2_800_000)
    ref = Ref(oracle, M_PIPE, 6, pkg.keys.pack_decimal(vals))
    ref.vals = vals
    _uniform(pkg, oracle, ref, front=0)


def test_pipelined_apply_multi_step_regions(pkg, oracle, default_env, uniform16):
    """The uniform batch plus one key 20,000 times: each of that key's 16 probes puts 20,000
    probes into one region (or more, where two share one), against the 8 x 1024 = 8192 a
    workgroup takes per step, so those regions run the kernel's extra-step loop three times
    or more while their neighbours take one step."""
    m, k = M_PIPE, 16
    hot = pkg.keys.pack(["hot-key"])
    batch = cat(uniform16.batch, (np.tile(hot[0], 20_000), np.arange(20_001, dtype=np.uint64) * len(hot[0])))
    want = Ref(oracle, m, k, hot, base=uniform16.bits)
    assert want.any_new   # the hot key is not covered by the uniform batch
    d = Dev(batch)
    with pkg.Filter(m, k, device=0) as f:
        assert_pipelined(f, d.n, front=2)
        assert insert_dev(f, d) is True
        same_string(f.export_redis(), want.string)
        assert insert_dev(f, d) is False
        got = include_dev(f, Dev(cat(hot, pkg.keys.pack(["cold-key"]))))
    np.testing.assert_array_equal(got, oracle.include_many(want.bits, m, k, *cat(hot, pkg.keys.pack(["cold-key"]))))


def test_pipelined_apply_second_run_table_pass(pkg, oracle, default_env):
    """k = 6, one 8-byte key 9,000,000 times plus 50,000 random keys.  A superbin's probes lie
    in chunk blocks of 8192, and the kernel takes a superbin's run table 1024 blocks per pass.
    Each superbin one of the key's 6 probes falls into holds >= 9,000,000 probes >
    1024 x 8192 = 8,388,608, i.e. >= 1099 blocks: its 32 regions all walk a second pass (31 of
    them finding nothing there, one finding ~600 k probes in many steps)."""
    m, k = M_PIPE, 6
    rng = np.random.default_rng(0xD15E + 2)
    hot = pkg.keys.pack(["hot8byte"])
    assert len(hot[0]) == 8
    rest = pkg.keys.pack_decimal(rng.integers(0, 10**12, size=50_000))
    reps = 9_000_000
    batch = cat((np.tile(hot[0], reps), np.arange(reps + 1, dtype=np.uint64) * 8), rest)
    want = Ref(oracle, m, k, cat(hot, rest))
    d = Dev(batch)
    assert reps > 1024 * 8192
    with pkg.Filter(m, k, device=0) as f:
        assert_pipelined(f, d.n, superbins=129, groups=8, front=0, scan=0)
        assert insert_dev(f, d) is True
        same_string(f.export_redis(), want.string)
        assert insert_dev(f, d) is False
        same_string(f.export_redis(), want.string)
        probe = cat(hot, rest, pkg.keys.pack_decimal(rng.integers(10**12, 2 * 10**12, size=5_000)))
        got = include_dev(f, Dev(probe))
    np.testing.assert_array_equal(got, oracle.include_many(want.bits, m, k, probe[0], probe[1]))


def test_pipelined_apply_prefilled_dirty_blocks(pkg, oracle, default_env, uniform16):
    """On a filter that already holds batch A, with dirty tracking on: A again plus 300 new
    keys in one pipelined launch changes only the new keys' bits; the reported 64 KiB blocks
    are exactly the blocks whose bytes changed and replaying them rebuilds the string; A once
    more reports nothing and any_new False."""
    m, k = M_PIPE, 16
    rng = np.random.default_rng(0xD15E + 3)
    fresh = pkg.keys.pack_decimal(rng.integers(10**12, 2 * 10**12, size=300))
    a, a_plus = Dev(uniform16.batch), Dev(cat(uniform16.batch, fresh))
    want = Ref(oracle, m, k, fresh, base=uniform16.bits)
    with pkg.Filter(m, k, device=0) as f:
        assert_pipelined(f, a.n)
        assert_pipelined(f, a_plus.n)
        assert insert_dev(f, a) is True
        f.track_dirty(True)
        assert f.dirty_ranges(clear=True)[0] == []
        s0 = f.export_redis()
        same_string(s0, uniform16.string)
        assert insert_dev(f, a_plus) is True
        s1 = f.export_redis()
        same_string(s1, want.string)
        ranges = check_dirty(f, s0, s1)
        assert 0 < len(blocks_of(ranges)) <= 300 * k
        assert insert_dev(f, a) is False
        assert f.dirty_ranges()[0] == []
        same_string(f.export_redis(), want.string)


# ---- the per-region kernel at every region size and density -------------------------------

# density -> (m, k, n): 100M@0.1 % sparse; 1M@1 % with a probe per line / per vector on average;
# 10k@1 %, a single partial region
MATRIX = {0: (1437758757, 10, 3_000), 1: (9585058, 6, 5_000), 2: (9585058, 6, 20_000), "one": (95851, 6, 2_000)}
REGIONS = {("18", 0): 5485, ("19", 0): 2743, ("20", 0): 1372, ("18", 1): 37, ("19", 1): 19, ("20", 1): 10,
           ("18", 2): 37, ("19", 2): 19, ("20", 2): 10, ("18", "one"): 1, ("19", "one"): 1, ("20", "one"): 1}


@pytest.fixture(scope="module")
def matrix_refs(pkg, oracle):
    """Per shape: the batch, 20 k other keys, and the oracle's results on a fresh and on a
    prefilled filter (shared by the three region sizes, read-only)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            m, k, n = MATRIX[shape]
            rng = np.random.default_rng(0xD15E + 10 + n)
            batch = rand_keys(rng, n)
            other = rand_keys(rng, 20_000)
            fresh = Ref(oracle, m, k, batch)
            pre = Ref(oracle, m, k, other)
            both = Ref(oracle, m, k, batch, base=pre.bits)
            probe = cat(batch, rand_keys(rng, 5_000), (other[0], other[1][:2001]))
            cache[shape] = (batch, other, fresh, pre, both, probe)
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", [0, 1, 2, "one"])
@pytest.mark.parametrize("rl", ["18", "19", "20"])
def test_per_region_apply_matrix(pkg, oracle, monkeypatch, matrix_refs, rl, shape):
    """bin_apply_kernel<18 / 19 / 20> on its sparse (0), read-first (1) and store-everything (2)
    branches, and bin_test_kernel at each size, forced binned: string on a fresh and on a
    prefilled filter, any_new True then False, include? answers, and the dirty blocks (a
    2^18-bit region is half a dirty block, a 2^20-bit one two)."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_INCLUDE_BINNED", "1")
    monkeypatch.setenv("BFHIP_BIN_REGION_LOG2", rl)
    m, k, n = MATRIX[shape]
    batch, other, fresh, pre, both, probe = matrix_refs(shape)
    d, dp = Dev(batch), Dev(probe)
    want_plan = dict(planned=1, binned=1, passes=1, region_log2=int(rl), regions=REGIONS[rl, shape],
                     density=2 if shape == "one" else shape, apply=PER_REGION, scan=0)
    with pkg.Filter(m, k, device=0) as f:
        det = f.insert_plan_detail(n)
        assert {key: det[key] for key in want_plan} == want_plan, det
        assert f.insert_plan(n) == {"binned": True, "scratch_bytes": det["scratch_bytes"]}
        assert insert_dev(f, d) is True
        same_string(f.export_redis(), fresh.string)
        assert insert_dev(f, d) is False
        np.testing.assert_array_equal(include_dev(f, dp), oracle.include_many(fresh.bits, m, k, probe[0], probe[1]))
    with pkg.Filter(m, k, device=0) as f:
        assert insert_dev(f, Dev(other)) is True
        f.track_dirty(True)
        assert f.dirty_ranges(clear=True)[0] == []
        s0 = f.export_redis()
        same_string(s0, pre.string)
        assert insert_dev(f, d) is both.any_new
        s1 = f.export_redis()
        same_string(s1, both.string)
        check_dirty(f, s0, s1)
        assert insert_dev(f, d) is False
        assert f.dirty_ranges()[0] == []
        np.testing.assert_array_equal(include_dev(f, dp), oracle.include_many(both.bits, m, k, probe[0], probe[1]))


@pytest.mark.parametrize("keys", ["random", "tail"])
def test_per_region_kernels_run_table_passes(pkg, oracle, monkeypatch, keys):
    """1,500,000 keys into the one region of the 95,851-bit filter in ONE launch: 9,000,000
    probes in one superbin are >= 1099 chunk blocks of 8192, more than the 1024 a run-table
    pass takes, so bin_apply_kernel walks a second pass; one include? of those keys plus
    20,000 fresh ones (9,120,000 probes) does the same in bin_test_kernel.

    "random": 1.5 M random keys.  They set every bit of the filter, so this case shows that the
    passes run and agree with the oracle, not that the second pass contributes.  "tail": one
    key 1,495,000 times (8,970,000 probes = 1094 full blocks) and then 5,000 random keys, whose
    probes therefore lie in the blocks past the first pass: about a quarter of the bits end up
    set, every one but the repeated key's six through the second pass, and the include?
    answers of the tail keys come from bin_test_kernel's second pass."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_INCLUDE_BINNED", "1")
    monkeypatch.delenv("BFHIP_BIN_REGION_LOG2", raising=False)
    m, k, n = 95851, 6, 1_500_000
    rng = np.random.default_rng(0xD15E + 20)
    if keys == "random":
        batch = distinct = rand_keys(rng, n)
    else:
        hot, reps = pkg.keys.pack(["hot8byte"]), n - 5_000
        assert reps * k > 1024 * 8192
        tail = rand_keys(rng, 5_000)
        batch = cat((np.tile(hot[0], reps), np.arange(reps + 1, dtype=np.uint64) * 8), tail)
        distinct = cat(hot, tail)
    probe = cat(batch, rand_keys(rng, 20_000))
    want = Ref(oracle, m, k, distinct)
    assert n * k > 1024 * 8192
    with pkg.Filter(m, k, device=0) as f:
        det = f.insert_plan_detail(n)
        want_plan = dict(planned=1, binned=1, passes=1, regions=1, superbins=1, density=2, apply=PER_REGION,
                         apply_loads=8, scan=0)
        assert {key: det[key] for key in want_plan} == want_plan, det
        one = f.insert_plan_detail(n + 20_000)
        assert (one["passes"], one["superbins"]) == (1, 1)   # the include?'s shape: one launch, one superbin
        assert insert_dev(f, Dev(batch)) is True
        same_string(f.export_redis(), want.string)
        got = include_dev(f, Dev(probe))
    np.testing.assert_array_equal(got, oracle.include_many(want.bits, m, k, probe[0], probe[1]))
    assert got[:n].all()


def test_mid_window_of_three_blocks(pkg, oracle, monkeypatch):
    """One (superbin, group) window of three chunk blocks with a short last one, through the
    block loop the two bin_mid kernels share: 4000 keys at k = 6 on a 2^19-bit filter (one region,
    so one superbin) are 24,000 probes in one group (two front tiles of 2048 keys), so the window
    is cut into blocks of 8192, 8192 and 7616.  Part 0 of the window's two workgroups sorts
    one block (no prefetch), part 1 sorts two (the prefetch-and-copy iteration, then the short
    block).  Insert runs bin_mid_kernel<false>, the forced binned include? bin_mid_kernel<true>
    with the key indices riding along."""
    monkeypatch.setenv("BFHIP_INSERT_BINNED", "1")
    monkeypatch.setenv("BFHIP_INCLUDE_BINNED", "1")
    monkeypatch.delenv("BFHIP_BIN_REGION_LOG2", raising=False)
    m, k, n = 2**19, 6, 4000
    assert (n * k - 1) // 8192 + 1 == 3 and n * k - 2 * 8192 == 7616
    rng = np.random.default_rng(0xD15E + 30)
    batch = rand_keys(rng, n)
    # include?: 2000 members and 2000 other keys, again 24,000 probes in a three-block window
    probe = cat((batch[0], batch[1][:2001]), rand_keys(rng, 2000))
    want = Ref(oracle, m, k, batch)
    with pkg.Filter(m, k, device=0) as f:
        det = f.insert_plan_detail(n)
        want_plan = dict(planned=1, binned=1, passes=1, region_log2=19, regions=1, superbins=1, groups=1, tiles=2)
        assert {key: det[key] for key in want_plan} == want_plan, det
        assert insert_dev(f, Dev(batch)) is True
        same_string(f.export_redis(), want.string)
        assert insert_dev(f, Dev(batch)) is False
        got = include_dev(f, Dev(probe))
    np.testing.assert_array_equal(got, oracle.include_many(want.bits, m, k, probe[0], probe[1]))
    assert got[:2000].all() and not got[2000:].all()
