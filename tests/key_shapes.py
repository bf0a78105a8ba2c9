"""Key batches that pin the key-hashing code on key *shapes* (a helper, not a test).

Every hashing kernel stages a tile of keys into LDS and hashes each key from there, or, when
the tile's bytes do not fit its stage, reads each key from global memory (csrc/bf_device.h:
sha1_key, sha1_key_staged, for_key_tile, and the private stagers of bf_kernels.hip and
bf_binned.hip).  What can go wrong there depends on the keys' lengths, on where they start
and on how many bytes a tile holds, not on what the keys say.  The batches below are built
for exactly those conditions; tests/test_key_shapes.py asserts that they hold, and
tests/test_gpu_key_shapes.py runs every hashing site over them.

All batches are packed ``(buf, offs)`` pairs as the C ABI takes them: ``buf`` uint8,
``offs`` uint64 with n + 1 entries, key j = buf[offs[j]:offs[j + 1]], and ``SLACK`` readable
bytes after ``offs[n]``.  They are deterministic (fixed seeds, numpy only) and hold arbitrary
bytes, 0x00 / 0x80 / 0xFF among them, so that a padding mistake cannot hide behind ASCII.
"""
import hashlib

import numpy as np

SEED = 0x5EED + 900
SLACK = 16          # readable bytes after offsets[n] (include/bfhip.h)
SHORT_MAX = 55      # the longest key of one SHA-1 block
MAX_LEN = 192       # boundaries() holds every length 0..MAX_LEN
FIPS_EDGES = (55, 56, 119, 120, 183, 184)   # L and L + 1 around every block edge below MAX_LEN

# The hashing sites: keys per tile, bytes of the LDS stage, and where the source says so
# (file, constant, factor).  A kernel that gains a stager gains a row here.
SITES = {
    "A": dict(tile=256, stage=16384, what="bf_kernels.hip direct key kernel",
              tile_src=("bf_device.h", "kBlock", 1), stage_src=("bf_device.h", "kStageBytes", 1)),
    "B": dict(tile=256, stage=7680, what="bf_kernels.hip include?+hash, two stages",
              tile_src=("bf_device.h", "kBlock", 1), stage_src=("bf_kernels.hip", "kHalfStageVec", 16)),
    "C": dict(tile=1024, stage=16384, what="bf_binned.hip bin_front*",
              tile_src=("bf_binned.hip", "kTile", 1), stage_src=("bf_binned.hip", "kStageVec", 16)),
    "D": dict(tile=1024, stage=16384, what="bf_binned.hip route front (k <= 12)",
              tile_src=("bf_binned.hip", "kTile", 1), stage_src=("bf_binned.hip", "kStageVec", 16)),
    "E": dict(tile=1024, stage=16384, what="bf_binned.hip route_chunks_idx_kernel (k > 12)",
              tile_src=("bf_binned.hip", "kTile", 1), stage_src=("bf_binned.hip", "kStageVec", 16)),
    "F1": dict(tile=1024, stage=16384, what="bf_binned.hip bin_apply_test_kernel side batch",
               tile_src=("bf_binned.hip", "kApplyLanes", 1), stage_src=("bf_binned.hip", "kStageVec", 16)),
    "F2": dict(tile=256, stage=4096, what="bf_binned.hip chunk_test_l2_kernel side batch",
               tile_src=("bf_binned.hip", "kL2Lanes", 1), stage_src=("bf_binned.hip", "kSideVec", 16)),
    "G": dict(tile=256, stage=16384, what="bf_seq.hip sequential per-key inserts",
              tile_src=("bf_seq.hip", "kSeqTile", 1), stage_src=("bf_seq.hip", "kSeqStageVec", 16)),
    "H": dict(tile=256, stage=16384, what="bf_lua.hip lua_check (inserts: G's kernels, i0 = 1)",
              tile_src=("bf_lua.hip", "kLuaTile", 1), stage_src=("bf_lua.hip", "kLuaStageVec", 16)),
    "I": dict(tile=256, stage=16384, what="bf_bank.hip keyed kernels",
              tile_src=("bf_bank.hip", "kBankTile", 1), stage_src=("bf_bank.hip", "kBankStageVec", 16)),
}


def site(name):
    """(keys per tile, stage bytes) of a hashing site."""
    return SITES[name]["tile"], SITES[name]["stage"]


def tile_stage_pairs():
    """The distinct (tile, stage) pairs of the table."""
    return sorted({site(s) for s in SITES})


# ---- bytes and packing -------------------------------------------------------------------------

def _bytes(rng, n):
    """n arbitrary bytes, about a quarter of them 0x00 / 0x80 / 0xFF (the SHA-1 pad byte and
    the values a wrong mask or a sign extension turns into something else)."""
    b = rng.integers(0, 256, size=n, dtype=np.uint8)
    special = np.array([0x00, 0x80, 0xFF], np.uint8)
    pick = rng.random(n) < 0.25
    b[pick] = special[rng.integers(0, 3, size=int(pick.sum()))]
    return b


def pack_lengths(lens, rng, lead=0):
    """Keys of the given lengths, packed back to back after ``lead`` bytes that belong to no
    key (so offs[0] == lead), with SLACK bytes of 0xFF after the last key."""
    lens = np.asarray(lens, np.uint64)
    offs = np.empty(len(lens) + 1, np.uint64)
    offs[0] = lead
    np.cumsum(lens, out=offs[1:])
    offs[1:] += np.uint64(lead)
    buf = _bytes(rng, int(offs[-1]) + SLACK)
    buf[int(offs[-1]):] = 0xFF
    # whole keys of the special values: an all-zero key, and keys ending in the pad byte
    for j in range(0, len(lens), 17):
        a, b = int(offs[j]), int(offs[j + 1])
        if b > a:
            buf[a:b] = (0x00, 0x80, 0xFF)[(j // 17) % 3]
    return buf, offs


def lengths(offs):
    return np.diff(offs.astype(np.int64))


def repeat(buf, offs, times):
    """The batch followed by times - 1 further copies of its keys (the first copy keeps its
    offsets, so its tiles stay where they were; every later key repeats an earlier one)."""
    a, b = int(offs[0]), int(offs[-1])
    out_buf = np.concatenate([buf[:b]] + [buf[a:b]] * (times - 1) + [np.full(SLACK, 0xFF, np.uint8)])
    out_offs = np.concatenate([offs] + [offs[1:] + np.uint64(i * (b - a)) for i in range(1, times)])
    return out_buf, out_offs


def digests(buf, offs):
    """The first four big-endian words of SHA-1(key) (ruby.rb:42-47's h[0..3]) via hashlib:
    bf_hash_many_dev's layout, (n, 4) uint32."""
    n = len(offs) - 1
    out = np.zeros((n, 4), np.uint32)
    raw = bytes(buf)
    for j in range(n):
        d = hashlib.sha1(raw[int(offs[j]):int(offs[j + 1])]).digest()
        out[j] = np.frombuffer(d[:16], ">u4")
    return out


def keys_of(buf, offs):
    """The keys as a list of bytes objects."""
    raw = bytes(buf)
    return [raw[int(offs[j]):int(offs[j + 1])] for j in range(len(offs) - 1)]


def nvec(offs, first, cnt):
    """16-byte vectors a stager loads for the tile of cnt keys from key ``first`` on: the rule of
    for_key_tile and of every private stager, on effective byte addresses (pointer + offset; the
    tests pass 16-byte aligned pointers, so offsets stand for addresses)."""
    start, end = int(offs[first]), int(offs[first + cnt])
    return (end - (start & ~15) + 15) >> 4


def tiles(offs, tile):
    """[(first key, count)] of the tiles a kernel cuts the batch into."""
    n = len(offs) - 1
    return [(t0, min(tile, n - t0)) for t0 in range(0, n, tile)]


# ---- boundaries --------------------------------------------------------------------------------

def _mixed_order():
    """Every length 0..MAX_LEN once: first the FIPS edges, each between two short keys, then
    the rest with every fourth key short, so each run of 64 keys mixes both kinds."""
    rng = np.random.default_rng(SEED)
    shorts = [int(x) for x in rng.permutation(SHORT_MAX)]          # 0..54 (55 is an edge)
    longs = [int(x) for x in rng.permutation(np.arange(SHORT_MAX + 1, MAX_LEN + 1)) if int(x) not in FIPS_EDGES]
    order = []
    for e in FIPS_EDGES:
        order += [shorts.pop(), e]
    order.append(shorts.pop())
    while longs or shorts:
        if shorts and (len(order) % 4 == 0 or not longs):
            order.append(shorts.pop())
        else:
            order.append(longs.pop())
    return order


def boundaries_layout(tile=256):
    """(lengths, marks) of boundaries(tile); marks name the first key of each part."""
    rng = np.random.default_rng(SEED + 1)
    lens = _mixed_order()
    marks = {"mixed": 0}
    # fill the mixed part up to whole tiles with short keys (a few long ones keep the waves mixed)
    marks["fill"] = len(lens)
    while len(lens) % tile:
        lens.append(int(rng.integers(56, 130)) if len(lens) % 64 == 7 else int(rng.integers(0, 9)))
    # a tile that fits every stage and still holds multi-block keys on both sides of each edge
    marks["staged_long"] = len(lens)
    part = [0] * tile
    for i, e in enumerate((56, 64, 119, 120, 183, 184)):
        part[5 + 37 * i] = e
    for j in range(tile):
        if part[j] == 0 and j % 64 != 0:
            part[j] = int(rng.integers(0, 5))
    lens += part
    # one wave of keys that all fit one block, the longest of them 52..55 bytes (lim = 13) ...
    marks["wave_short"] = len(lens)
    wave = [int(x) for x in rng.integers(0, 24, 64)]
    for i, L in enumerate((52, 53, 54, 55, 0, 1, 3, 4)):
        wave[3 + 7 * i] = L
    lens += wave
    # ... and one wave with exactly one key of 56 bytes: 63 short keys take the generic path
    marks["wave_one_56"] = len(lens)
    wave = [int(x) for x in rng.integers(0, 24, 64)]
    wave[29] = 56
    lens += wave
    marks["end"] = len(lens)
    return lens, marks


def boundaries(tile=256):
    """SHA-1 block boundaries for a site of ``tile`` keys per tile:

    * "mixed": every length 0..192 once, the FIPS edges 55/56, 119/120, 183/184 each between two
      short keys, short and long keys mixed in every run of 64 keys (one wave), filled up to
      whole tiles.  Its first tile holds more bytes than any stage: the global-read path.
    * "staged_long": one tile of few bytes (it fits the smallest stage) with keys of 56, 64, 119,
      120, 183 and 184 bytes among short ones: multi-block SHA-1 from LDS.
    * "wave_short": 64 keys of <= 55 bytes with 52..55 among them: the branch-free path with the
      wave maximum of L / 4 at 13.
    * "wave_one_56": 64 keys, exactly one of 56 bytes.
    """
    lens, _ = boundaries_layout(tile)
    return pack_lengths(lens, np.random.default_rng(SEED + 2))


# ---- alignment ---------------------------------------------------------------------------------

ALIGN_SHORT = (0, 1, 2, 3, 4, 5, 19, 20, 52, 53, 54, 55)
ALIGN_LONG = (56, 57, 58, 59, 63, 64, 65, 70)
ALIGN_LEAD = 5      # offs[0] of alignment()


def alignment_layout():
    """(lengths, target) of alignment(): target[j] is True for the keys whose (start, length)
    pair is swept, False for the filler keys that move the next start."""
    lens, target = [], []
    at = ALIGN_LEAD
    for group in (ALIGN_SHORT, ALIGN_LONG):
        for L in group:
            for a in range(16):
                fill = (a - at) % 16
                lens.append(fill)
                target.append(False)
                at += fill
                lens.append(L)
                target.append(True)
                at += L
    return lens, np.array(target)


def alignment():
    """Keys of <= 55 bytes (first: whole waves on the branch-free path) and of 56..70 bytes, each
    length at every start address mod 16, so every pair (start mod 16, L mod 4) of the
    alignbyte / keep / pad arithmetic occurs in both kinds.  The starts are moved by filler keys
    and by offs[0] = ALIGN_LEAD; a device test also moves the base pointer."""
    lens, _ = alignment_layout()
    return pack_lengths(lens, np.random.default_rng(SEED + 3), lead=ALIGN_LEAD)


# ---- stage edge --------------------------------------------------------------------------------

def _compose(rng, n, total, last=None):
    """n key lengths summing to ``total``: long keys (56..192, the FIPS edges first) where the
    mean needs them and always a few, short ones otherwise; ``last`` fixes the final length."""
    m = n - (last is not None)
    budget = total - (last or 0)
    if m <= 0 or budget < 0 or budget > m * MAX_LEN:
        raise ValueError("cannot cut %d bytes into %d keys" % (total, n))
    n_long = int(np.clip(-(-(budget - 14 * m) // 110), 6, m))
    lens = np.concatenate([np.array((56, 64, 119, 120, 183, 184)[:n_long]),
                           rng.integers(SHORT_MAX + 1, MAX_LEN + 1, max(n_long - 6, 0)),
                           rng.integers(0, 29, m - n_long)]).astype(np.int64)
    lo = np.where(lens > SHORT_MAX, SHORT_MAX + 1, 0)
    hi = np.where(lens > SHORT_MAX, MAX_LEN, SHORT_MAX)
    lo[:6], hi[:6] = lens[:6], lens[:6]           # the edge lengths stay
    diff = budget - int(lens.sum())
    order = rng.permutation(m)
    while diff:                                   # spread the difference, a few bytes per key
        moved = False
        for j in order:
            room = int(hi[j] - lens[j]) if diff > 0 else int(lens[j] - lo[j])
            step = min(room, abs(diff), 7)
            if step:
                lens[j] += step if diff > 0 else -step
                diff += -step if diff > 0 else step
                moved = True
            if not diff:
                break
        if not moved:
            raise ValueError("cannot cut %d bytes into %d keys" % (total, n))
    lens = lens[rng.permutation(m)]
    return [int(x) for x in lens] + ([int(last)] if last is not None else [])


def stage_edge(tile, stage_bytes, addr_mod16):
    """Four tiles of a site with ``tile`` keys per tile and ``stage_bytes`` of LDS stage, the
    first key at address ``addr_mod16`` mod 16 (offs[0] = 16 + addr_mod16, on an aligned base):

    0. nvec == stage_bytes / 16: the last tile that fits.  It ends on the stage's last byte with
       a key of 55 bytes, so the branch-free SHA-1 reads the slack past the stage.
    1. nvec == stage_bytes / 16 + 1: the first tile that does not fit (one byte too many).
    2. short keys only: staged again, right after an unstaged tile.
    3. a final partial tile.
    """
    if not 0 <= addr_mod16 < 16:
        raise ValueError("addr_mod16 must be 0..15")
    rng = np.random.default_rng(SEED + 4 + 16 * tile + addr_mod16 + stage_bytes)
    lead = 16 + addr_mod16
    lens = _compose(rng, tile, stage_bytes - addr_mod16, last=SHORT_MAX)
    lens += _compose(rng, tile, stage_bytes + 1)
    lens += [int(x) for x in rng.integers(0, 12, tile)]
    part = [int(x) for x in rng.integers(0, 24, tile // 2 + 3)]
    part[1], part[-2] = 120, 56
    lens += part
    return pack_lengths(lens, rng, lead=lead)
