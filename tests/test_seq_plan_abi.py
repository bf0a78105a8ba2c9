"""bf_seq_plan: which form the sequential insert takes for a chunk, on both sides of every line
(CPU only; the call launches nothing and needs no GPU).

The expected form is the rule of bf_seq.hip's comments, restated here (``rule``):

* binned  from 4096 keys on, on filters of up to 2^27 bits;
* direct  (one uint32 per filter bit) when that table is no bigger than the hash table,
          4 m <= 12 * slots(n, k), and the filter has at most 2^28 bits;
* hash    everything else: a table of slots(n, k) = the power of two >= max(1024, 2 n k).

A chunk holds at most min(2^22, 2^25 / k) keys.  The shapes tests/test_gpu_seq_hash_and_cut.py and
test_gpu_key_shapes.py's SEQ_FORMS rely on are pinned at the end, so a moved threshold fails here,
without a GPU, and says which GPU test has lost its form.
"""
import numpy as np
import pytest

import key_shapes as KS
import lua_oracle as L

HASH, DIRECT, BINNED = 0, 1, 2


def slots_of(n, k):
    s = 1024
    while s < 2 * n * k:
        s *= 2
    return s


def a256(x):
    return -(-x // 256) * 256


def rule(n, k, m):
    """(form, table entries, scratch bytes) as bf_seq.hip states them."""
    if n >= 4096 and m <= 1 << 27:
        nreg = -(-m // (1 << 14))
        # per-region counts, bases and cursors; a digest and a 0-probe mask per key; one entry per probe
        return BINNED, nreg, 3 * a256(4 * nreg) + a256(16 * n) + a256(8 * n) + a256(8 * n * k)
    s = slots_of(n, k)
    if m <= 1 << 28 and 4 * m <= 12 * s:
        return DIRECT, m, a256(4 * m) + a256(16 * n) + a256(8 * n)
    return HASH, s, a256(8 * s) + a256(4 * s) + a256(16 * n) + a256(8 * n)


def chunk_rule(k):
    return max(1, min(1 << 22, (1 << 25) // k))


def plan(pkg, n, k, m):
    return pkg._lib.seq_plan(n, k, m)


def check(pkg, n, k, m, form):
    """The shape takes ``form`` by the rule AND by the library."""
    want = rule(n, k, m)
    assert want[0] == form, ("the restated rule", n, k, m, want)
    p = plan(pkg, n, k, m)
    assert (p["form"], p["slots"], p["scratch_bytes"]) == want, (n, k, m, p)
    assert p["chunk_keys"] == chunk_rule(k)
    return p


def test_layer_sizes_are_the_pinned_ones(pkg):
    """1000 @ 0.01 -> 11027/7, 24940/8, 55652/9; layers fill at 1000, 3000, 7000."""
    assert [pkg._lib.lua_layer_params(1000, 0.01, n) for n in (1, 2, 3)] == [(11027, 7), (24940, 8), (55652, 9)]
    assert [L.layer_params(1000.0, 0.01, n) for n in (1, 2, 3)] == [(11027, 7), (24940, 8), (55652, 9)]
    # the two other layouts of the GPU file: a layer of 8 hashes that 512 probes rarely collide in,
    # and one of 64 hashes
    for (entries, precision), want in (((80000, 0.005), (997635, 8)), ((2000, 1e-19), (185001, 64))):
        assert pkg._lib.lua_layer_params(entries, precision, 1) == L.layer_params(float(entries), precision, 1) == want
    for cap, layer in ((1000, 1), (3000, 2), (7000, 3)):
        assert pkg._lib.lua_index(1000, cap) == L.layer_index(1000.0, cap) == layer
        assert pkg._lib.lua_index(1000, cap + 1) == L.layer_index(1000.0, cap + 1) == layer + 1


@pytest.mark.parametrize("n,k,m,form", [
    # the binned form's least batch
    (4095, 7, 95851, DIRECT), (4096, 7, 95851, BINNED),
    # ... and its largest filter: 8192 regions of 2^14 bits
    (4096, 7, 1 << 27, BINNED), (4096, 7, (1 << 27) + 1, HASH),
    (4095, 7, 1 << 27, HASH),
    # the direct table's 1 GiB bound, at a batch whose hash table (2^27 slots) would allow 2^28 + 1
    # bits.  (No chunk is that large: at the chunk bound 2 n k <= 2^26, so 4 m <= 12 * 2^26 ends the
    # direct form at 3 * 2^26 bits; the bound is checked where the function can be asked.)
    (1 << 20, 64, 1 << 28, DIRECT), (1 << 20, 64, (1 << 28) + 1, HASH),
    (1 << 19, 64, 3 << 26, DIRECT), (1 << 19, 64, (3 << 26) + 1, HASH),
    # 4 m <= 12 * slots on the Lua layout's layers 1 and 2 (1000 @ 0.01)
    (146, 7, 11027, HASH), (147, 7, 11027, DIRECT),
    (512, 8, 24940, HASH), (513, 8, 24940, DIRECT),
    # the same line met from the filter's side: 12 * 1024 slots = 4 * 3072 bits
    (1, 7, 3072, DIRECT), (1, 7, 3073, HASH),
    (73, 7, 3072, DIRECT), (74, 7, 3072, DIRECT), (73, 7, 3073, HASH), (74, 7, 3073, DIRECT),
])
def test_form_on_both_sides_of_every_line(pkg, n, k, m, form):
    check(pkg, n, k, m, form)


@pytest.mark.parametrize("n,k,slots", [
    (1, 1, 1024), (1, 7, 1024), (1, 64, 1024),      # the floor of 1024 slots
    (8, 64, 1024), (9, 64, 2048),                   # 2 n k = 1024: exactly half full
    (64, 8, 1024), (65, 8, 2048),
    (128, 8, 2048), (129, 8, 4096),
    (73, 7, 1024), (74, 7, 2048),                   # 1022 and 1036 probes
    (300, 64, 65536), (4095, 13, 131072),
    (1 << 19, 64, 1 << 26),                         # the largest table a chunk takes (768 MiB)
])
def test_hash_table_slots(pkg, n, k, slots):
    m = (1 << 29) + 3                               # too large for the other two forms at any n
    p = check(pkg, n, k, m, HASH)
    assert p["slots"] == slots == slots_of(n, k)
    assert slots >= 2 * n * k and (slots == 1024 or slots < 4 * n * k)


@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 13, 63, 64])
def test_chunk_bound(pkg, k):
    c = plan(pkg, 1, k, 1000)["chunk_keys"]
    assert c == chunk_rule(k)
    assert c <= 1 << 22 and 2 * c * k <= 1 << 26 and (c == 1 << 22 or 2 * (c + 1) * k > 1 << 26)


def test_every_form_over_a_grid(pkg):
    """The rule and the library agree on a grid that straddles every threshold at once."""
    seen = set()
    for k in (1, 6, 7, 13, 64):
        for n in (1, 2, 73, 74, 146, 147, 1023, 4095, 4096, 4097, 100_000, chunk_rule(k)):
            for m in (1, 64, 3072, 3073, 9585, 11027, 95851, 1 << 14, (1 << 14) + 1, 9585058, 1 << 27,
                      (1 << 27) + 1, 1 << 28, (1 << 28) + 1, 1 << 33):
                want = rule(n, k, m)
                p = plan(pkg, n, k, m)
                assert (p["form"], p["slots"], p["scratch_bytes"]) == want, (n, k, m)
                seen.add(want[0])
    assert seen == {HASH, DIRECT, BINNED}


def test_refusals(pkg):
    for n, k, m in ((10, 0, 1000), (10, 65, 1000), (10, 7, 0)):
        with pytest.raises(pkg.ArgumentError):
            plan(pkg, n, k, m)
    lib = pkg._lib.load()
    assert lib.bf_seq_plan(10, 7, 1000, None, None, None) == 0      # every output is nullable
    assert lib.bf_seq_plan_chunk(7, None) == pkg._lib.BF_EINVAL
    assert plan(pkg, 0, 7, 1000)["form"] == DIRECT                  # an empty chunk launches nothing


# ---- the shapes the GPU tests rely on ----------------------------------------------------------

LUA = (1000, 0.01)
LAYER = {1: (11027, 7), 2: (24940, 8), 3: (55652, 9)}


@pytest.mark.parametrize("layer,n,form", [
    # (a) batches of 1, 2, 73 and 146 keys on layer 1
    (1, 1, HASH), (1, 2, HASH), (1, 73, HASH), (1, 146, HASH), (1, 147, DIRECT),
    # (b) what is left of a batch after a cut: any count up to 512 on layer 2, 910 on layer 3
    (2, 1, HASH), (2, 300, HASH), (2, 512, HASH), (2, 513, DIRECT),
    (3, 1, HASH), (3, 910, HASH), (3, 911, DIRECT),
    # (d) the device cut cases: the hash form up to 146 keys on layer 1, the direct form above,
    # one binned chunk of 5000 keys
    (1, 15, HASH), (1, 16, HASH), (1, 17, HASH), (1, 1024, DIRECT), (1, 1025, DIRECT),
    (1, 3 * 1024 + 5, DIRECT), (1, 5000, BINNED), (2, 5000, BINNED),
    # the pre-inserts that fill a layer in one large batch
    (1, 1000, DIRECT), (2, 2000, DIRECT), (2, 3000, DIRECT),
])
def test_lua_layer_shapes_of_the_gpu_file(pkg, layer, n, form):
    m, k = LAYER[layer]
    assert pkg._lib.lua_layer_params(*LUA, layer) == (m, k)
    check(pkg, n, k, m, form)
    # the form holds for every smaller chunk too where the GPU file says "up to"
    if form == HASH:
        assert all(rule(c, k, m)[0] == HASH for c in range(1, n + 1))


@pytest.mark.parametrize("n,k,m,form,slots", [
    (73, 7, 95851, HASH, 1024),                     # (c) wrap: 73 keys of 7 probes in 1024 slots
    (64, 8, 1 << 20, HASH, 1024),                   # (c) half full
    (300, 64, (1 << 20) + 3, HASH, 65536),          # (c) k = 64, and its second batch of 200 keys
    (200, 64, (1 << 20) + 3, HASH, 32768),
    (64, 8, 997635, HASH, 1024),                    # (c) the same on layer 1 of 80000 @ 0.005 ...
    (200, 64, 185001, HASH, 32768),                 # ... and of 2000 @ 1e-19
    (120, 64, 185001, HASH, 16384),
])
def test_filter_shapes_of_the_gpu_file(pkg, n, k, m, form, slots):
    assert check(pkg, n, k, m, form)["slots"] == slots


def test_key_shape_site_g_forms(pkg):
    """SEQ_FORMS of test_gpu_key_shapes.py, at the batch sizes that test builds (the shape batch
    and copies of it, at least ``least`` keys)."""
    forms = [("direct", 9585, 6, 0), ("binned", 9585, 6, 4096), ("binned", 95851, 7, 4096), ("hash", 9585058, 7, 0)]
    tile, stage = KS.site("G")
    batches = [KS.boundaries(tile), KS.alignment(), KS.stage_edge(tile, stage, 0), KS.stage_edge(tile, stage, 15)]
    for name, m, k, least in forms:
        for buf, offs in batches:
            n1 = len(offs) - 1
            n = n1 * max(2, -(-least // n1))
            assert n <= chunk_rule(k)                # one chunk
            check(pkg, n, k, m, {"hash": HASH, "direct": DIRECT, "binned": BINNED}[name])


def test_numpy_and_python_ints_alike(pkg):
    assert plan(pkg, np.uint64(146), np.uint32(7), np.int64(11027)) == plan(pkg, 146, 7, 11027)
