"""The guarantees of tests/key_shapes.py, checked on the CPU, so that no case of
tests/test_gpu_key_shapes.py can pass because its batch missed the condition it is named for;
and the helper's (tile, stage) table against the constants in csrc/, so that a retuned stage
cannot silently move the tests off the boundary."""
import os
import re

import numpy as np
import pytest

import key_shapes as KS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "redis-bloomfilter_amd", "csrc")


def _runs_of_64(n):
    return [(a, min(a + 64, n)) for a in range(0, n, 64)]


def _has_special_bytes(buf, offs):
    body = buf[int(offs[0]):int(offs[-1])]
    return all((body == v).any() for v in (0x00, 0x80, 0xFF))


# ---- the helper's own guarantees ---------------------------------------------------------------

@pytest.mark.parametrize("tile", sorted({t for t, _ in KS.tile_stage_pairs()}))
def test_boundaries_conditions(tile):
    buf, offs = KS.boundaries(tile)
    lens, marks = KS.boundaries_layout(tile)
    L = KS.lengths(offs)
    assert L.tolist() == lens and int(offs[0]) == 0 and len(buf) == int(offs[-1]) + KS.SLACK
    assert _has_special_bytes(buf, offs)
    mixed = L[: marks["fill"]]
    assert sorted(mixed.tolist()) == list(range(KS.MAX_LEN + 1))           # every length once
    for a, b in _runs_of_64(len(mixed)):                                    # each wave mixes both kinds
        if b - a >= 8:
            assert (mixed[a:b] <= KS.SHORT_MAX).any() and (mixed[a:b] > KS.SHORT_MAX).any(), (a, b)
    for e in KS.FIPS_EDGES:                                                 # each edge between short keys
        j = mixed.tolist().index(e)
        assert 0 < j < len(mixed) - 1 and mixed[j - 1] <= KS.SHORT_MAX and mixed[j + 1] <= KS.SHORT_MAX, e
    # the parts start on whole tiles / whole waves of a tile
    assert marks["staged_long"] % tile == 0 and marks["wave_short"] % tile == 0
    assert marks["wave_one_56"] == marks["wave_short"] + 64 and marks["end"] == marks["wave_one_56"] + 64
    ws = L[marks["wave_short"]: marks["wave_one_56"]]
    assert len(ws) == 64 and ws.max() == KS.SHORT_MAX and (ws.max() >> 2) == 13
    assert {52, 53, 54, 55} <= set(ws.tolist())
    w56 = L[marks["wave_one_56"]: marks["end"]]
    assert len(w56) == 64 and sorted(w56.tolist())[-2:][0] <= KS.SHORT_MAX and w56.max() == 56
    assert (w56 > KS.SHORT_MAX).sum() == 1
    sl = L[marks["staged_long"]: marks["wave_short"]]
    assert {56, 64, 119, 120, 183, 184} <= set(sl.tolist())
    # for every site of this tile size: the first tile overflows the stage (global reads), the
    # multi-block tile and the two closing waves are staged
    for name in KS.SITES:
        t, stage = KS.site(name)
        if t != tile:
            continue
        tl = KS.tiles(offs, tile)
        assert KS.nvec(offs, *tl[0]) > stage // 16, name
        assert KS.nvec(offs, marks["staged_long"], tile) <= stage // 16, name
        assert tl[-1] == (marks["wave_short"], 128) and KS.nvec(offs, *tl[-1]) <= stage // 16, name


def test_alignment_conditions():
    buf, offs = KS.alignment()
    lens, target = KS.alignment_layout()
    L = KS.lengths(offs)
    assert L.tolist() == lens and int(offs[0]) == KS.ALIGN_LEAD != 0
    assert _has_special_bytes(buf, offs)
    start = offs[:-1].astype(np.int64)
    for group, long in ((KS.ALIGN_SHORT, False), (KS.ALIGN_LONG, True)):
        assert all((x > KS.SHORT_MAX) == long and x <= 70 for x in group)
        pairs = {(int(s) % 16, int(x) % 4) for s, x, tg in zip(start, L, target) if tg and (x > KS.SHORT_MAX) == long}
        assert pairs == {(a, r) for a in range(16) for r in range(4)}
        for x in group:                                       # each listed length at every start
            assert {int(s) % 16 for s, y, tg in zip(start, L, target) if tg and y == x} == set(range(16)), x
    assert {0, 1, 3, 4, 5, 19, 20, 52, 53, 54, 55} <= set(KS.ALIGN_SHORT)
    assert (L[~target] < 16).all()                            # the fillers are short keys themselves
    # a moved base pointer rotates the starts and keeps the set complete
    for delta in (1, 3, 15):
        assert {((int(s) + delta) % 16, int(x) % 4) for s, x, tg in zip(start, L, target) if tg} == \
            {(a, r) for a in range(16) for r in range(4)}
    # whole waves of short keys come first: the branch-free path sees every pair
    n_short = 2 * 16 * len(KS.ALIGN_SHORT)
    assert n_short % 64 == 0 and (L[:n_short] <= KS.SHORT_MAX).all() and (L[n_short:] > KS.SHORT_MAX).any()
    # the batch fits one stage of the 1024-key sites, delta included: staged there
    assert (int(offs[-1]) + 15 + 15) >> 4 <= 16384 // 16


@pytest.mark.parametrize("addr", [0, 15])
@pytest.mark.parametrize("tile,stage", KS.tile_stage_pairs())
def test_stage_edge_conditions(tile, stage, addr):
    buf, offs = KS.stage_edge(tile, stage, addr)
    assert _has_special_bytes(buf, offs) and len(buf) == int(offs[-1]) + KS.SLACK
    assert int(offs[0]) % 16 == addr and int(offs[0]) != 0
    L = KS.lengths(offs)
    tl = KS.tiles(offs, tile)
    assert len(tl) == 4 and [c for _, c in tl[:3]] == [tile] * 3 and 0 < tl[3][1] < tile
    sv = stage // 16
    nv = [KS.nvec(offs, *t) for t in tl]
    assert nv[0] == sv                  # the last tile that fits
    assert nv[1] == sv + 1              # the first that does not
    assert nv[2] <= sv and nv[3] <= sv  # staged again after it, and a partial tile
    assert (L[2 * tile: 3 * tile] <= KS.SHORT_MAX).all()
    # tile 0 ends on the stage's last byte with a one-block key: the branch-free path reads the slack
    assert int(offs[tile]) - (int(offs[0]) & ~15) == stage and L[tile - 1] == KS.SHORT_MAX
    assert (L[tile - 64: tile] <= KS.SHORT_MAX).any()
    # both full tiles hold multi-block keys on each side of every edge
    for t in (0, 1):
        assert set(KS.FIPS_EDGES[1:]) | {64} <= set(L[t * tile:(t + 1) * tile].tolist())
    assert len(L) <= 4 * tile


def test_repeat_and_digests():
    buf, offs = KS.stage_edge(256, 4096, 15)
    rb, ro = KS.repeat(buf, offs, 3)
    n = len(offs) - 1
    assert len(ro) == 3 * n + 1 and (ro[: n + 1] == offs).all() and len(rb) == int(ro[-1]) + KS.SLACK
    keys = KS.keys_of(buf, offs)
    assert KS.keys_of(rb, ro) == keys * 3
    d = KS.digests(buf, offs)
    assert d.shape == (n, 4) and d.dtype == np.uint32
    # FIPS 180-4 known answers through the same packing
    kb, ko = KS.pack_lengths([0, 3], np.random.default_rng(0))
    kb[0:3] = np.frombuffer(b"abc", np.uint8)
    assert KS.digests(kb, ko).tolist() == [[0xDA39A3EE, 0x5E6B4B0D, 0x3255BFEF, 0x95601890],
                                           [0xA9993E36, 0x4706816A, 0xBA3E2571, 0x7850C26C]]


# ---- the table against the source --------------------------------------------------------------

_DECL = re.compile(r"constexpr\s+(?:unsigned\s+)?\w+\s+(k[A-Z]\w*)\s*=\s*([^;]+);")


def _constants(fname):
    with open(os.path.join(CSRC, fname)) as fh:
        return {m.group(1): m.group(2).strip() for m in _DECL.finditer(fh.read())}


def _value(fname, name, seen=()):
    """The integer value of constant ``name`` as ``fname`` sees it (its own definition, else
    bf_device.h's), for expressions of integers, other constants and + - * / ( )."""
    consts = _constants(fname)
    if name not in consts:
        assert fname != "bf_device.h", "constant %s not found" % name
        return _value("bf_device.h", name, seen)
    assert (fname, name) not in seen
    expr = consts[name]
    assert re.fullmatch(r"[\w\s+\-*/()]+", expr), "%s = %s is not a plain integer expression" % (name, expr)

    def sub(m):
        tok = m.group(0)
        if re.fullmatch(r"\d+[uUlL]*", tok):
            return str(int(re.match(r"\d+", tok).group(0)))
        return str(_value(fname, tok, seen + ((fname, name),)))
    return int(eval(re.sub(r"\w+", sub, expr).replace("/", "//"), {"__builtins__": {}}))


@pytest.mark.parametrize("name", sorted(KS.SITES))
def test_table_matches_source(name):
    row = KS.SITES[name]
    for key, src in (("tile", row["tile_src"]), ("stage", row["stage_src"])):
        fname, const, factor = src
        assert row[key] == _value(fname, const) * factor, "%s: %s %s in %s" % (name, key, const, fname)


def test_named_constants_are_the_ones_the_table_reads():
    """The constants the stagers are built from, by name: one that disappears or is renamed
    fails here rather than leaving a row of the table pointing at nothing."""
    want = {"bf_device.h": ["kBlock", "kStageBytes"], "bf_kernels.hip": ["kHalfStageVec"],
            "bf_binned.hip": ["kTile", "kStageVec", "kSideVec", "kApplyLanes", "kL2Lanes"],
            "bf_seq.hip": ["kSeqTile", "kSeqStageVec"], "bf_lua.hip": ["kLuaTile", "kLuaStageVec"],
            "bf_bank.hip": ["kBankTile", "kBankStageVec"]}
    used = {(r[k][0], r[k][1]) for r in KS.SITES.values() for k in ("tile_src", "stage_src")}
    assert used == {(f, c) for f, cs in want.items() for c in cs}
    for f, cs in want.items():
        for c in cs:
            assert _value(f, c) > 0
    assert _value("bf_device.h", "kStageBytes") == 16 * _value("bf_device.h", "kStageVec")
    assert _value("bf_kernels.hip", "kStageVec") == _value("bf_binned.hip", "kStageVec")   # A's stage = C's
