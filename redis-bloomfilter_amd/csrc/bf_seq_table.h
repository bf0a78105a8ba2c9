// bf_seq_table.h — the first-index table of the exact sequential insert, for bf_seq.hip (one
// filter, a Lua layer) and bf_bank.hip (a bank, its bits numbered bank-wide).
//
// The insert runs as two kernels per chunk: `candidates` notes, for every probe that finds its
// bit 0, the key's index under the bit's number; `mark` reads back the smallest index noted for a
// bit, which is the key that sets it first.  `bit` is whatever the caller numbers: the offset o
// for a filter, id * stride_words * 32 + o for a bank.  Two forms:
//   DIRECT  one uint32 per bit of the caller's bit space (table_bits of them): tvals[bit];
//   hash    an open-addressing table of `slots` (a power of two) entries, linear probing from
//           mix64(bit) & tmask: tkeys[slot] names the bit, tvals[slot] holds its index.
//
// Invariants, which every user of the table relies on:
//   * a slot's key is bit + 1, and 0 means empty: the keys are cleared to 0 before a chunk;
//   * the values are cleared to 0xFF bytes: 0xFFFFFFFF is above every index and equals none;
//   * a chunk notes at most n * k bits and slots >= 2 * n * k (seq_slots), so the table is at
//     most half full: a claim always reaches a free or matching slot, and a lookup always ends
//     at its key or at an empty slot;
//   * the index j is relative to the chunk (chunks hold at most 2^22 keys: bf_seq_chunk_keys).
#pragma once
#include "bf_internal.h"

namespace bfseq {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {   // SplitMix64 finalizer
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Key j probes `bit` and found it 0: the table keeps the smallest such j.
template <bool DIRECT>
__device__ __forceinline__ void seq_note(unsigned long long* tkeys, uint32_t* tvals, uint64_t tmask, uint64_t bit,
                                         uint32_t j) {
    if constexpr (DIRECT) {   // one word per bit: no claim, no probing
        atomicMin(tvals + bit, j);
    } else {
        const unsigned long long key = bit + 1;
        uint64_t slot = mix64(bit) & tmask;
        for (;;) {
            const unsigned long long cur = atomicCAS(tkeys + slot, 0ull, key);
            if (cur == 0ull || cur == key) {
                atomicMin(tvals + slot, j);
                break;
            }
            slot = (slot + 1) & tmask;
        }
    }
}

// The smallest index noted for `bit`; 0xFFFFFFFF for a bit nobody noted.
template <bool DIRECT>
__device__ __forceinline__ uint32_t seq_first(const unsigned long long* tkeys, const uint32_t* tvals, uint64_t tmask,
                                              uint64_t bit) {
    uint64_t slot = bit;
    if constexpr (!DIRECT) {
        const unsigned long long key = bit + 1;
        slot = mix64(bit) & tmask;
        for (unsigned long long cur = tkeys[slot]; cur != key && cur != 0ull; cur = tkeys[slot])
            slot = (slot + 1) & tmask;
    }
    return tvals[slot];
}

// ---- host side: the form, the bytes, the carve and the clear ------------------------------------

// The hash table's slots for n keys of k probes.
inline uint64_t seq_slots(uint64_t n, uint32_t k) {
    uint64_t s = 1024;
    while (s < 2 * n * (uint64_t)k) s <<= 1;
    return s;
}

// The direct form when its table is no bigger than the hash table (12 B per slot) it replaces,
// so neither the clear nor the scratch grows, and at most 1 GiB: the Lua layout's 1M-scale
// layers (11M bits = 44 MB against a 16M-slot, 192 MB table for a 2^20-key chunk), small
// filters or banks under big batches.  (an older bound let the direct table reach
// twice the hash table's bytes.)
inline bool seq_direct_fits(uint64_t table_bits, uint64_t n, uint32_t k) {
    return table_bits <= (1ull << 28) && 4 * table_bits <= 12 * seq_slots(n, k);
}

// The table's entries: one per bit (direct) or the hash table's slots.
inline uint64_t seq_table_slots(bool direct, uint64_t table_bits, uint64_t n, uint32_t k) {
    return direct ? table_bits : seq_slots(n, k);
}

inline uint64_t seq_table_bytes(bool direct, uint64_t table_bits, uint64_t n, uint32_t k) {
    const uint64_t slots = seq_table_slots(direct, table_bits, n, k);
    return direct ? align256(slots * 4) : align256(slots * 8) + align256(slots * 4);
}

// A chunk's scratch: the table, then a digest and a mask of 0-probes per key, in this order.
inline uint64_t seq_scratch_bytes(bool direct, uint64_t table_bits, uint64_t n, uint32_t k) {
    return seq_table_bytes(direct, table_bits, n, k) + align256(n * 16) + align256(n * 8);
}

struct SeqCarve {
    unsigned long long* tkeys;   // NULL: the direct form
    uint32_t* tvals;
    uint64_t tmask;   // slots - 1 (hash form)
    uint64_t slots;   // seq_table_slots
    uint4* digests;
    unsigned long long* cand;
};

inline SeqCarve seq_carve(void* base, bool direct, uint64_t table_bits, uint64_t n, uint32_t k) {
    SeqCarve c{};
    uint8_t* at = static_cast<uint8_t*>(base);
    c.slots = seq_table_slots(direct, table_bits, n, k);
    if (direct) {
        c.tvals = reinterpret_cast<uint32_t*>(at);
    } else {
        c.tkeys = reinterpret_cast<unsigned long long*>(at);
        c.tvals = reinterpret_cast<uint32_t*>(at + align256(c.slots * 8));
        c.tmask = c.slots - 1;
    }
    at += seq_table_bytes(direct, table_bits, n, k);
    c.digests = reinterpret_cast<uint4*>(at);
    at += align256(n * 16);
    c.cand = reinterpret_cast<unsigned long long*>(at);
    return c;
}

inline hipError_t seq_table_clear(const SeqCarve& c, hipStream_t s) {
    if (c.tkeys)
        if (hipError_t e = hipMemsetAsync(c.tkeys, 0, c.slots * 8, s); e != hipSuccess) return e;
    return hipMemsetAsync(c.tvals, 0xFF, c.slots * 4, s);
}

}  // namespace bfseq
