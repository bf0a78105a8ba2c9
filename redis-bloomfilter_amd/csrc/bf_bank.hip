// bf_bank.hip — a filter bank: n_filters Bloom filters of identical (m, k) behind one handle
// (include/bfhip.h, bf_bank_*).  In the reference `key_name` names a filter
// (lib/redis/bloomfilter.rb:30) and an application keeps one per tenant, per day or per feed;
// here they share one device allocation and a mixed batch of (filter id, key) pairs is one
// launch.
//
// Layout: filter f is the Redis string SETBIT builds (ruby.rb:59), exactly as a bf_handle holds
// one, at byte f * stride of the allocation; stride = ceil(m / 8) rounded up to 128 bytes, so
// every filter starts on a cache line and no 32-bit word straddles two filters.  The bytes
// from ceil(m / 8) to stride stay zero.  Every address is formed in 64 bits: n_filters * stride
// may exceed 4 GiB.
//
// Kernels:
//   bank_keys_kernel    insert / include?: one lane per key, 256 keys per workgroup staged
//                       through LDS (bfdev::for_key_tile), SHA-1 and the offsets of ruby.rb:41-55
//                       from bf_device.h, the k probes inside the lane's own filter.
//   bank_seq_*_kernel   insert with the exact sequential per-key flag (first-seen dedup): bf_seq.hip's
//                       candidates / mark pair, the first-index table (bf_seq_table.h) keyed by the
//                       bank-wide bit.
//   bank_list_tile      bf_bank_insert_many_changes*: the LIST instantiations of the two insert
//                       kernels also list every bit their own atomics flipped, as (filter id,
//                       SETBIT offset) pairs; slots reserved once per workgroup.
//   bank_across_kernel  include? of one key in many filters: the same tile, hashed once per
//                       workgroup, its k bit positions tested in every filter of a chunk of the
//                       list; one 64-entry mask word per lane and group.
//   bank_*_kernel       per-filter BITCOUNT, clear, gather-and-trim (export) and scatter
//                       (import): a workgroup, or a wave when stride <= kWaveStrideBytes, owns
//                       one listed filter, streams it in 16-byte vectors and reduces with
//                       shuffles; one writer per output, no global atomics.
//   bank_fold_kernel    BITOP AND / OR / XOR over groups of filters, every group of a call in one
//                       launch: the same owners up to kFoldSliceStride, above it a 2-D grid of
//                       stride slices x groups with one atomic add per workgroup.
//   bank_overlap_kernel BITCOUNT(A AND B) for every pair of two lists: a tiled binary GEMM, 64 x
//                       64 pairs per workgroup staged through LDS, the stride split over grid z
//                       where the tiles are few.  bank_overlap_few_kernel streams at most 4 x 4
//                       pairs of long filters without a tile.
//
// Host side: every host-pointer keyed call (insert, include?, the sequential and the listing
// insert, the cross query) walks its batch with the same two steps: chunk_end cuts at the call's
// key bound and at batch_bytes (a longer key goes alone), stage_chunk copies the chunk's keys,
// offsets (from 0) and ids to the device.  The caller's loop launches, queues its copy-back and
// synchronises.  seq_plan is the one place that decides a sequential call's table form, chunk
// bound and scratch bytes, for bf_bank_seq_plan, the host forms and the _dev forms alike.
#include "bfhip.h"
#include "bf_device.h"
#include "bf_host.h"
#include "bf_seq_table.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace bfdev;
using namespace bfseq;

namespace {

constexpr int kBankTile = 256;                 // lanes = keys per workgroup of the keyed kernel
constexpr int kBankStageVec = kStageBytes / 16;
constexpr uint32_t kBankLanes = 256;           // lanes per workgroup of the per-filter kernels
constexpr uint32_t kWaveStrideBytes = 4096;    // a filter this small is owned by one wave (<= 4 vectors per lane)
constexpr uint32_t kBankMaxBlocks = 1u << 16;  // per-filter kernels: the grid strides beyond this

thread_local std::string g_bank_create_error;

enum : int { BANK_INSERT = 0, BANK_INCLUDE = 1 };

// ---- the list of flipped bits (bf_bank_insert_many_changes*) -----------------------------------

// Where an insert kernel lists the bits it flipped 0 -> 1: entry e is the pair (ids[e], bits[e]) =
// (filter, SETBIT offset within it, ruby.rb:59).  *count counts every flipped bit of the call;
// an entry at or past cap is counted and not written.  BankList<false> is empty: the kernels of
// the entry points without a list are instantiated without any of it.
template <bool LIST>
struct BankList {};
template <>
struct BankList<true> {
    uint32_t* ids;
    uint64_t* bits;
    uint64_t cap;
    unsigned long long* count;
};

// A workgroup of kBankTile lanes lists its flipped probes.  fm is the lane's mask of them (probe
// i: bit i; k <= BF_MAX_K = 64, as cand below), 0 for a lane without a key.  Slots are reserved
// per workgroup, not per bit: the popcounts' prefix sum over the wave by shuffles and over the
// waves through LDS, then ONE returning add on the counter (none for a tile that flipped
// nothing), and every lane writes its entries from its own base, the offsets derived again from
// the digest.  One contended word takes about 88 returning atomics per microsecond: an add per
// flipped bit would serialise a batch of 2^22 keys for tens of milliseconds, an add per tile
// for about 0.2.  Every lane of the workgroup calls this once (two barriers).
__device__ __forceinline__ void bank_list_tile(const BfGeom& g, const BankList<true>& list, unsigned long long fm,
                                               uint32_t id, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3) {
    __shared__ unsigned long long s_base[kBankTile / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t mine = (uint32_t)__popcll(fm);
    uint32_t incl = mine;   // inclusive prefix sum over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63u) s_base[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long part[kBankTile / 64], total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBankTile / 64; ++w) {
            part[w] = total;
            total += s_base[w];
        }
        const unsigned long long base =
            total ? __hip_atomic_fetch_add(list.count, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#pragma unroll
        for (uint32_t w = 0; w < kBankTile / 64; ++w) s_base[w] = base + part[w];
    }
    __syncthreads();
    unsigned long long e = s_base[wave] + (incl - mine);
    while (fm) {
        const uint32_t i = (uint32_t)__builtin_ctzll(fm);
        fm &= fm - 1;
        if (e < list.cap) {
            list.ids[e] = id;
            list.bits[e] = probe_offset(g, h0, h1, h2, h3, i);
        }
        ++e;
    }
}

// status[0]: a key's offsets failed bfdev::key_ok; status[1]: a filter id >= n_filters.
// Both live in the bank's pinned status block, which bf_bank_sync reports.

// Whether lane's pair (id, key) of a tile of cnt keys is taken.  for_key_tile hands a refused key
// over as the empty key: its offsets tell the two apart again.  Every lane hashes (the staged
// SHA-1 reduces over the wave); a refused lane drops out after it.
__device__ __forceinline__ bool bank_pair_ok(const uint64_t* s_off, uint32_t lane, uint32_t cnt, uint32_t id,
                                             uint64_t n_filters, uint32_t* status) {
    bool ok = key_ok(s_off[0], s_off[lane], s_off[lane + 1], s_off[cnt], nullptr);
    if ((uint64_t)id >= n_filters) {
        status[1] = 1u;
        ok = false;
    }
    return ok;
}

// LIST (insert only): every bit a lane's own atomic flipped goes to `list` (bank_list_tile).
template <int OP, bool LIST = false>
__global__ __launch_bounds__(kBankTile) void bank_keys_kernel(BfGeom g, uint64_t n_filters, uint64_t stride_words,
                                                              const uint8_t* __restrict__ keys16,
                                                              const uint64_t* __restrict__ offsets, uint64_t bias,
                                                              const uint32_t* __restrict__ ids, uint64_t n,
                                                              uint8_t* __restrict__ out8,
                                                              uint32_t* __restrict__ status, BankList<LIST> list) {
    static_assert(!LIST || OP == BANK_INSERT, "only an insert flips bits");
    __shared__ uint64_t s_off[kBankTile + 1];
    __shared__ uint4 s_stage[kBankStageVec + kStageSlackVec];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kBankTile;
    const uint32_t cnt = (uint32_t)((n - tile0) < (uint64_t)kBankTile ? (n - tile0) : kBankTile);
    // LIST: what the lane lists after the tile; a lane without a key, or with a refused one, keeps 0
    [[maybe_unused]] unsigned long long fm = 0;
    [[maybe_unused]] uint32_t fid = 0, fh[4] = {0u, 0u, 0u, 0u};
    for_key_tile<kBankTile, kBankStageVec>(keys16, offsets, bias, tile0, cnt, s_off, s_stage, status,
        [&](auto staged, uint32_t lane, const uint32_t* src, uint32_t s, uint32_t L) {
            const uint64_t j = tile0 + lane;
            const uint32_t id = ids[j];
            // a refused pair: no bit set, answer 0, key_flipped 0
            const bool ok = bank_pair_ok(s_off, lane, cnt, id, n_filters, status);
            uint32_t H[5];
            sha1_any<decltype(staged)::value>(src, s, L, H);
            if (!ok) {
                if (out8) out8[j] = 0;
                return;
            }
            uint32_t* __restrict__ fb = g.bits + (uint64_t)id * stride_words;   // 64-bit word index
            const uint32_t k = g.k;
            if constexpr (OP == BANK_INCLUDE) {
                // every load of a round is issued before any is used; a lane whose AND already
                // failed stops after its round (ruby.rb:23's early exit)
                uint32_t hit = 1u;
                for (uint32_t i0 = 0; i0 < k && (hit & 1u); i0 += kChunk) {
                    uint32_t v[kChunk], sh[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        v[c] = 0xFFFFFFFFu; sh[c] = 0;
                        if (i0 + c < k) {
                            const uint64_t o = probe_offset(g, H[0], H[1], H[2], H[3], i0 + c);
                            sh[c] = (uint32_t)(o ^ 7u) & 31u;
                            v[c] = fb[o >> 5];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) hit &= v[c] >> sh[c];
                }
                out8[j] = (uint8_t)(hit & 1u);
            } else {
                // test-then-set (the insert_test policy of bf_kernels.hip): a 1 seen by the load
                // is final, a stale 0 costs an atomic whose return value tells the truth.  The
                // atomic's old value decides "flipped": of several lanes racing for one bit
                // exactly one sees it unset.
                uint32_t flipped = 0;
                for (uint32_t i0 = 0; i0 < k; i0 += kChunk) {
                    uint32_t w[kChunk], mask[kChunk], v[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        w[c] = 0; mask[c] = 0; v[c] = 0;
                        if (i0 + c < k) {
                            const uint64_t o = probe_offset(g, H[0], H[1], H[2], H[3], i0 + c);
                            w[c] = (uint32_t)(o >> 5);   // < stride_words <= 2^32 (checked at create)
                            mask[c] = 1u << ((uint32_t)(o ^ 7u) & 31u);
                            v[c] = fb[w[c]];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        if (mask[c] && !(v[c] & mask[c])) {
                            const uint32_t old = __hip_atomic_fetch_or(fb + w[c], mask[c], __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT);
                            flipped |= (old & mask[c]) ? 0u : 1u;
                            if constexpr (LIST) fm |= (unsigned long long)((old & mask[c]) ? 0u : 1u) << (i0 + c);
                        }
                    }
                }
                if (out8) out8[j] = (uint8_t)flipped;
                if constexpr (LIST) {
                    fid = id;
                    fh[0] = H[0]; fh[1] = H[1]; fh[2] = H[2]; fh[3] = H[3];
                }
            }
        });
    // after the tile, so that every lane of the workgroup, refused ones included, reaches the barriers
    if constexpr (LIST) bank_list_tile(g, list, fm, fid, fh[0], fh[1], fh[2], fh[3]);
}

// ---- sequential per-key flags: the mixed batch inserted one pair at a time ---------------------

// bf_seq.hip's two-kernel scheme with the bit space widened to the whole bank.  Inserting the
// pairs (ids[j], key j) one by one in batch order (ruby.rb:57-63 per key_name), key j is new iff
// one of its bits was 0 before the batch and no earlier key of the batch going to the SAME filter
// probes it.  With first(f, b) = the smallest batch index whose key goes to filter f and probes
// bit b:
//
//     new(j)  <=>  exists probe b of j:  prebit(ids[j], b) == 0  and  first(ids[j], b) == j
//
// A bit is named bank-wide: id * stride * 8 + o, which is also its position in the allocation.
//   1. bank_seq_candidates: hash, test every probe against the pre-batch bits (plain loads, the
//      bank is not written) and note the index j under the bit's number for each 0 bit, in the
//      first-index table of bf_seq_table.h (DIRECT: one uint32 per bit of the bank; else the hash
//      table).  The digest and the key's mask of 0-probes go to scratch.
//   2. bank_seq_mark: new(j) from the table, then the 0-probes ORed in.
// Indices are 32-bit and relative to the chunk (bf_seq_chunk_keys); chunks run in stream order.

// cand[j] = the mask of key j's probes whose bit is 0 (probe i: bit i; k <= BF_MAX_K = 64),
// digests[j] = H0..H3.  A refused pair (bank_pair_ok) has mask 0.  status as in bank_keys_kernel.
template <bool DIRECT>
__global__ __launch_bounds__(kBankTile) void bank_seq_candidates_kernel(
    BfGeom g, uint64_t n_filters, uint64_t stride_words, const uint8_t* __restrict__ keys16,
    const uint64_t* __restrict__ offsets, uint64_t bias, const uint32_t* __restrict__ ids, uint64_t n,
    unsigned long long* __restrict__ tkeys, uint32_t* __restrict__ tvals, uint64_t tmask, uint4* __restrict__ digests,
    unsigned long long* __restrict__ cand, uint32_t* __restrict__ status) {
    __shared__ uint64_t s_off[kBankTile + 1];
    __shared__ uint4 s_stage[kBankStageVec + kStageSlackVec];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kBankTile;
    const uint32_t cnt = (uint32_t)((n - tile0) < (uint64_t)kBankTile ? (n - tile0) : kBankTile);
    for_key_tile<kBankTile, kBankStageVec>(keys16, offsets, bias, tile0, cnt, s_off, s_stage, status,
        [&](auto staged, uint32_t lane, const uint32_t* src, uint32_t s, uint32_t L) {
            const uint32_t j = (uint32_t)(tile0 + lane);   // chunk-relative: n <= 2^22
            const uint32_t id = ids[j];
            const bool ok = bank_pair_ok(s_off, lane, cnt, id, n_filters, status);   // refused: mask 0
            uint32_t H[5];
            sha1_any<decltype(staged)::value>(src, s, L, H);
            digests[j] = make_uint4(H[0], H[1], H[2], H[3]);
            unsigned long long cm = 0;
            if (ok) {
                const uint32_t* __restrict__ fb = g.bits + (uint64_t)id * stride_words;   // 64-bit word index
                const uint64_t bit0 = (uint64_t)id * stride_words * 32u;                  // the filter's first bit number
                const uint32_t k = g.k;
                for (uint32_t i0 = 0; i0 < k; i0 += kChunk) {
                    // every load of a round is issued before any is used
                    uint64_t o[kChunk];
                    uint32_t v[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        o[c] = 0; v[c] = 0xFFFFFFFFu;
                        if (i0 + c < k) {
                            o[c] = probe_offset(g, H[0], H[1], H[2], H[3], i0 + c);
                            v[c] = fb[o[c] >> 5];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        if ((v[c] >> ((uint32_t)(o[c] ^ 7u) & 31u)) & 1u) continue;   // set already, or past k
                        cm |= 1ull << (i0 + c);
                        seq_note<DIRECT>(tkeys, tvals, tmask, bit0 + o[c], j);
                    }
                }
            }
            cand[j] = cm;
        });
}

// out8[j] (nullable) = new(j); every 0-probe of key j is ORed into its filter.
// LIST: the probes whose atomicOr found the bit still 0 go to `list` (bank_list_tile): of the keys
// of a chunk that probe one bit, and of one key's probes that name one bit, exactly one lists it.
template <bool DIRECT, bool LIST = false>
__global__ __launch_bounds__(kBankTile) void bank_seq_mark_kernel(
    BfGeom g, uint64_t stride_words, const uint32_t* __restrict__ ids, uint64_t n,
    const unsigned long long* __restrict__ tkeys, const uint32_t* __restrict__ tvals, uint64_t tmask,
    const uint4* __restrict__ digests, const unsigned long long* __restrict__ cand, uint8_t* __restrict__ out8,
    BankList<LIST> list) {
    const uint64_t j = (uint64_t)blockIdx.x * kBankTile + threadIdx.x;
    [[maybe_unused]] unsigned long long fm = 0;   // LIST: a lane past n keeps 0 and still reaches the barriers
    [[maybe_unused]] uint32_t fid = 0;
    uint4 H = make_uint4(0u, 0u, 0u, 0u);
    if (j < n) {
        uint32_t isnew = 0;
        unsigned long long cm = cand[j];
        if (cm) {   // a key with a 0-probe passed the candidates' checks: its id is in range
            H = digests[j];
            const uint64_t id = ids[j];
            if constexpr (LIST) fid = (uint32_t)id;
            uint32_t* __restrict__ fb = g.bits + id * stride_words;
            const uint64_t bit0 = id * stride_words * 32u;
            while (cm) {
                const uint32_t i = (uint32_t)__builtin_ctzll(cm);
                cm &= cm - 1;
                const uint64_t o = probe_offset(g, H.x, H.y, H.z, H.w, i);
                isnew |= seq_first<DIRECT>(tkeys, tvals, tmask, bit0 + o) == (uint32_t)j ? 1u : 0u;
                const uint32_t bit = 1u << ((uint32_t)(o ^ 7u) & 31u);
                [[maybe_unused]] const uint32_t old =
                    __hip_atomic_fetch_or(fb + (o >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (LIST) fm |= (unsigned long long)((old & bit) ? 0u : 1u) << i;
            }
        }
        if (out8) out8[j] = (uint8_t)isnew;
    }
    if constexpr (LIST) bank_list_tile(g, list, fm, fid, H.x, H.y, H.z, H.w);
}

// ---- cross query: one key against many filters ----------------------------------------------

// List entries a workgroup walks with one hashed key tile: one 64-entry mask word.  Every
// (tile, chunk) workgroup hashes its tile again, so the length trades that SHA-1 against spread.
// Measured at 64 / 128 / 256 (DESIGN.md 6h "Cross queries"; build with -DBFHIP_ACROSS_CHUNK=...
// to repeat it): the SHA-1 is lost in the loads where there are many tiles and many chunks
// (under 1 %), while a workgroup's time grows with its chunk where there are few tiles.  At 64
// one key against 10^5 filters is 1,563 workgroups and 2^20 keys against 32 filters hash once.
#ifndef BFHIP_ACROSS_CHUNK
#define BFHIP_ACROSS_CHUNK 64
#endif
constexpr uint32_t kAcrossChunk = BFHIP_ACROSS_CHUNK;
constexpr uint32_t kAcrossMaxY = 65535;   // the grid's y limit: beyond it a workgroup strides over chunks
static_assert(kAcrossChunk % 64 == 0 && kAcrossChunk <= kBankTile, "whole mask words, staged by one pass of the workgroup");

// mask word (j, e / 64) bit e % 64 = Ruby#include? (ruby.rb:20-30) of key j in the filter of
// list entry e (ids == NULL: filter e).  A key's k offsets (ruby.rb:41-55) do not depend on the
// filter, so the lane hashes once, keeps the first round's (word, shift) pairs in registers and
// tests them at id * stride for every entry of its chunk; rounds past the first are recomputed
// from the digest and reached only by a lane whose AND still holds.  One writer per mask word,
// zeros included.  status as in bank_keys_kernel: a refused key's row and a refused entry's
// column read 0.
__global__ __launch_bounds__(kBankTile) void bank_across_kernel(BfGeom g, uint64_t n_filters, uint64_t stride_words,
                                                                const uint8_t* __restrict__ keys16,
                                                                const uint64_t* __restrict__ offsets, uint64_t bias,
                                                                const uint32_t* __restrict__ ids, uint64_t count,
                                                                uint64_t n, uint64_t row_words,
                                                                unsigned long long* __restrict__ mask,
                                                                uint32_t* __restrict__ status) {
    __shared__ uint64_t s_off[kBankTile + 1];
    __shared__ uint4 s_stage[kBankStageVec + kStageSlackVec];
    __shared__ uint32_t s_ids[kAcrossChunk];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kBankTile;
    const uint32_t cnt = (uint32_t)((n - tile0) < (uint64_t)kBankTile ? (n - tile0) : kBankTile);
    const uint64_t nchunks = (count + kAcrossChunk - 1) / kAcrossChunk;
    for (uint64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        const uint64_t e0 = chunk * kAcrossChunk;
        const uint32_t len = (uint32_t)((count - e0) < (uint64_t)kAcrossChunk ? (count - e0) : kAcrossChunk);
        // the chunk's ids, read once per workgroup; for_key_tile's first barrier publishes them
        // and its last one frees s_ids for the next chunk
        if (threadIdx.x < len) {
            const uint64_t f = ids ? (uint64_t)ids[e0 + threadIdx.x] : e0 + threadIdx.x;
            if (f >= n_filters) status[1] = 1u;
            s_ids[threadIdx.x] = (uint32_t)f;
        }
        for_key_tile<kBankTile, kBankStageVec>(keys16, offsets, bias, tile0, cnt, s_off, s_stage, status,
            [&](auto staged, uint32_t lane, const uint32_t* src, uint32_t s, uint32_t L) {
                // a refused key arrives as the empty key (bank_keys_kernel): its row is zeros
                const bool ok = key_ok(s_off[0], s_off[lane], s_off[lane + 1], s_off[cnt], nullptr);
                uint32_t H[5];
                sha1_any<decltype(staged)::value>(src, s, L, H);
                const uint32_t k = g.k;
                // the first round's (word, shift) pairs; a probe past k reads word 0 and is ORed
                // away by pad, so a round's loads are issued without a branch between them
                uint32_t w[kChunk], sh[kChunk], pad[kChunk];
#pragma unroll
                for (int c = 0; c < kChunk; ++c) {
                    w[c] = 0; sh[c] = 0; pad[c] = 1u;
                    if ((uint32_t)c < k) {
                        const uint64_t o = probe_offset(g, H[0], H[1], H[2], H[3], (uint32_t)c);
                        w[c] = (uint32_t)(o >> 5);   // < stride_words <= 2^32 (checked at create)
                        sh[c] = (uint32_t)(o ^ 7u) & 31u;
                        pad[c] = 0u;
                    }
                }
                // One list entry in two steps, so that two entries' loads are in flight together.
                // issue: the entry's filter (the id is the same in every lane: a scalar; a refused
                // id reads filter 0 and answers 0) and the first round's loads.
                auto issue = [&](uint32_t e, uint32_t (&v)[kChunk], uint32_t& live) -> const uint32_t* {
                    const uint32_t id = __builtin_amdgcn_readfirstlane(s_ids[e]);
                    live = (uint64_t)id < n_filters ? 1u : 0u;
                    const uint32_t* fb = g.bits + (uint64_t)(live ? id : 0u) * stride_words;   // 64-bit word index
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) v[c] = fb[w[c]];
                    return fb;
                };
                // settle: the AND; with k > kChunk the later rounds, recomputed from the digest, for
                // a lane whose AND still holds (ruby.rb:23's early exit)
                auto settle = [&](const uint32_t* fb, const uint32_t (&v)[kChunk], uint32_t live) -> unsigned long long {
                    uint32_t hit = live;
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) hit &= (v[c] >> sh[c]) | pad[c];
                    for (uint32_t i0 = kChunk; i0 < k && (hit & 1u); i0 += kChunk) {
                        uint32_t v2[kChunk], s2[kChunk];
#pragma unroll
                        for (int c = 0; c < kChunk; ++c) {
                            v2[c] = 0xFFFFFFFFu; s2[c] = 0;
                            if (i0 + c < k) {
                                const uint64_t o = probe_offset(g, H[0], H[1], H[2], H[3], i0 + c);
                                s2[c] = (uint32_t)(o ^ 7u) & 31u;
                                v2[c] = fb[o >> 5];
                            }
                        }
#pragma unroll
                        for (int c = 0; c < kChunk; ++c) hit &= v2[c] >> s2[c];
                    }
                    return hit & 1u;
                };
                unsigned long long* __restrict__ row = mask + (tile0 + lane) * row_words + (e0 >> 6);
                for (uint32_t g0 = 0; g0 < len; g0 += 64) {
                    const uint32_t ge = len - g0 < 64u ? len - g0 : 64u;
                    unsigned long long acc = 0;
                    if (ok) {
                        uint32_t va[kChunk], vb[kChunk], la, lb;
                        uint32_t i = 0;
                        for (; i + 2 <= ge; i += 2) {
                            const uint32_t* fa = issue(g0 + i, va, la);
                            const uint32_t* fb = issue(g0 + i + 1, vb, lb);
                            acc |= settle(fa, va, la) << i;
                            acc |= settle(fb, vb, lb) << (i + 1);
                        }
                        if (i < ge) acc |= settle(issue(g0 + i, va, la), va, la) << i;
                    }
                    row[g0 >> 6] = acc;
                }
            });
    }
}

// ---- per-filter kernels -------------------------------------------------------------------

// 1 + the index of the last non-zero byte of a vector (device byte b is bits 8 (b & 3).. of
// word b >> 2), 0 for a zero vector.
__device__ __forceinline__ uint32_t last_byte(const uint4& v) {
    if (v.w) return 16u - ((uint32_t)__builtin_clz(v.w) >> 3);
    if (v.z) return 12u - ((uint32_t)__builtin_clz(v.z) >> 3);
    if (v.y) return 8u - ((uint32_t)__builtin_clz(v.y) >> 3);
    if (v.x) return 4u - ((uint32_t)__builtin_clz(v.x) >> 3);
    return 0u;
}

// Who owns which listed filter: by stride (a kernel argument, so the choice is
// workgroup-uniform) either each wave of the workgroup one item or the whole workgroup one.
struct Owner {
    bool wave;        // a wave owns an item
    uint32_t lane;    // this lane's index among the owner's lanes
    uint32_t lanes;   // lanes of the owner
};

__device__ __forceinline__ Owner bank_owner(uint64_t stride_vec) {
    Owner o;
    o.wave = stride_vec * 16 <= kWaveStrideBytes;
    o.lane = o.wave ? (threadIdx.x & 63u) : threadIdx.x;
    o.lanes = o.wave ? 64u : kBankLanes;
    return o;
}

// Sum / max over the owner's lanes, returned to every one of them.  Workgroup owners go
// through LDS with two barriers (every lane of the workgroup calls this together).
template <bool MAX>
__device__ __forceinline__ unsigned long long owner_reduce(unsigned long long v, const Owner& o,
                                                           unsigned long long* s_part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(v, off);
        v = MAX ? (v > y ? v : y) : v + y;
    }
    if (o.wave) return v;
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = s_part[0];
#pragma unroll
    for (uint32_t w = 1; w < kBankLanes / 64; ++w) r = MAX ? (r > s_part[w] ? r : s_part[w]) : r + s_part[w];
    __syncthreads();
    return r;
}

// Calls body(item, live, f, valid) for every listed item this owner takes: live = the item
// exists (a wave past the end of the list idles), f = its filter (ids == NULL: item itself),
// valid = live and f < n_filters (a bad id sets status[1] and is skipped).  The loop bound is
// the same for every lane of a workgroup, so body may use barriers when the owner is one.
template <typename Body>
__device__ __forceinline__ void for_owned(const Owner& o, const uint32_t* __restrict__ ids, uint64_t count,
                                          uint64_t n_filters, uint32_t* __restrict__ status, Body&& body) {
    const uint32_t per = o.wave ? kBankLanes / 64 : 1u;
    for (uint64_t base = (uint64_t)blockIdx.x * per; base < count; base += (uint64_t)gridDim.x * per) {
        const uint64_t item = base + (o.wave ? (threadIdx.x >> 6) : 0u);
        const bool live = item < count;
        const uint64_t f = live ? (ids ? (uint64_t)ids[item] : item) : 0;
        const bool valid = live && f < n_filters;
        if (live && !valid && o.lane == 0) status[1] = 1u;
        body(item, live, f, valid);
    }
}

// out[item] = BITCOUNT of the item's filter (0 for a refused id).
__global__ __launch_bounds__(kBankLanes) void bank_bitcount_kernel(const uint4* __restrict__ bits, uint64_t stride_vec,
                                                                   uint64_t n_filters, const uint32_t* __restrict__ ids,
                                                                   uint64_t count, unsigned long long* __restrict__ out,
                                                                   uint32_t* __restrict__ status) {
    __shared__ unsigned long long s_part[kBankLanes / 64];
    const Owner o = bank_owner(stride_vec);
    for_owned(o, ids, count, n_filters, status, [&](uint64_t item, bool live, uint64_t f, bool valid) {
        unsigned long long acc = 0;
        if (valid) {
            const uint4* __restrict__ p = bits + f * stride_vec;
#pragma unroll 4
            for (uint64_t v = o.lane; v < stride_vec; v += o.lanes) acc += popc4(p[v]);
        }
        acc = owner_reduce<false>(acc, o, s_part);
        if (live && o.lane == 0) out[item] = acc;
    });
}

__global__ __launch_bounds__(kBankLanes) void bank_clear_kernel(uint4* __restrict__ bits, uint64_t stride_vec,
                                                                uint64_t n_filters, const uint32_t* __restrict__ ids,
                                                                uint64_t count, uint32_t* __restrict__ status) {
    const Owner o = bank_owner(stride_vec);
    for_owned(o, ids, count, n_filters, status, [&](uint64_t, bool, uint64_t f, bool valid) {
        if (!valid) return;
        uint4* __restrict__ p = bits + f * stride_vec;
        for (uint64_t v = o.lane; v < stride_vec; v += o.lanes) p[v] = make_uint4(0u, 0u, 0u, 0u);
    });
}

// Export: the item's filter copied to dst + item * stride and its trimmed Redis length (last
// non-zero byte + 1, 0 for an empty filter) to lens[item].  A refused id exports zeros.
__global__ __launch_bounds__(kBankLanes) void bank_gather_kernel(const uint4* __restrict__ bits, uint64_t stride_vec,
                                                                 uint64_t n_filters, const uint32_t* __restrict__ ids,
                                                                 uint64_t count, uint4* __restrict__ dst,
                                                                 unsigned long long* __restrict__ lens,
                                                                 uint32_t* __restrict__ status) {
    __shared__ unsigned long long s_part[kBankLanes / 64];
    const Owner o = bank_owner(stride_vec);
    for_owned(o, ids, count, n_filters, status, [&](uint64_t item, bool live, uint64_t f, bool valid) {
        unsigned long long last = 0;
        if (live) {
            const uint4* __restrict__ p = bits + f * stride_vec;   // read only when valid
            uint4* __restrict__ d = dst + item * stride_vec;
            for (uint64_t v = o.lane; v < stride_vec; v += o.lanes) {
                const uint4 x = valid ? p[v] : make_uint4(0u, 0u, 0u, 0u);
                d[v] = x;
                const uint32_t lb = last_byte(x);
                if (lb) last = v * 16 + lb;   // v grows: the lane's last non-zero vector wins
            }
        }
        last = owner_reduce<true>(last, o, s_part);
        if (live && o.lane == 0) lens[item] = last;
    });
}

// Import: the first lens[item] bytes of src + item * stride replace (zero-filled to stride) or
// are ORed into the item's filter.  One writer per filter when the listed ids are distinct.
template <bool OR>
__global__ __launch_bounds__(kBankLanes) void bank_scatter_kernel(uint4* __restrict__ bits, uint64_t stride_vec,
                                                                  uint64_t n_filters, const uint32_t* __restrict__ ids,
                                                                  uint64_t count, const uint4* __restrict__ src,
                                                                  const unsigned long long* __restrict__ lens,
                                                                  uint32_t* __restrict__ status) {
    const Owner o = bank_owner(stride_vec);
    for_owned(o, ids, count, n_filters, status, [&](uint64_t item, bool, uint64_t f, bool valid) {
        if (!valid) return;
        const unsigned long long cap = stride_vec * 16;
        const unsigned long long len = lens[item] < cap ? lens[item] : cap;
        uint4* __restrict__ p = bits + f * stride_vec;
        const uint4* __restrict__ s = src + item * stride_vec;
        for (uint64_t v = o.lane; v < stride_vec; v += o.lanes) {
            const unsigned long long at = v * 16;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (at < len) x = mask_bytes(s[v], 0u, len - at < 16 ? (uint32_t)(len - at) : 16u);
            if (OR) {
                if (x.x | x.y | x.z | x.w) {
                    const uint4 c = p[v];
                    p[v] = make_uint4(c.x | x.x, c.y | x.y, c.z | x.z, c.w | x.w);
                }
            } else {
                p[v] = x;
            }
        }
    });
}

uint32_t owned_grid(uint64_t stride, uint64_t count) {
    const uint64_t per = stride <= kWaveStrideBytes ? kBankLanes / 64 : 1;
    const uint64_t g = (count + per - 1) / per;
    return g > kBankMaxBlocks ? kBankMaxBlocks : (g ? (uint32_t)g : 1u);
}

// ---- folds: filters of the bank combined with each other ------------------------------------

// A stride above this is cut into slices over a 2-D grid (slices x groups); up to it one owner
// (bank_owner) takes a whole group.  Measured (DESIGN.md 6h "Folds"; build with
// -DBFHIP_FOLD_SLICE_STRIDE=... to repeat it).
#ifndef BFHIP_FOLD_SLICE_STRIDE
#define BFHIP_FOLD_SLICE_STRIDE (64u << 10)
#endif
constexpr uint64_t kFoldSliceStride = BFHIP_FOLD_SLICE_STRIDE;
constexpr uint32_t kFoldUnroll = 4;                          // vectors a lane folds side by side
constexpr uint32_t kFoldSliceVec = kBankLanes * kFoldUnroll; // vectors of one workgroup's slice: 16 KiB
constexpr uint64_t kFoldMaxBlocks = 1ull << 22;              // the slice grid: groups stride beyond this
constexpr uint64_t kFoldMaxSlices = 1024;                    // workgroups of one group: 4 a CU
static_assert(kFoldSliceStride >= kWaveStrideBytes, "the slice grid is a workgroup's");

// Group g = src[seg[g]] OP src[seg[g] + 1] OP ... (ruby.rb:59's strings, combined bit for bit as
// BITOP does).  WRITE: the result replaces filter dst_ids[g], a vector stored only where it
// differs (changed[g], ruby.rb:61-62's "the string changed"); set_bits[g] = BITCOUNT of the result.
// A lane reads its vector of every source and of the destination before it stores that vector
// and no other lane touches it, so the destination may be one of its own group's sources.
// `bits` is read and written through one pointer: no __restrict__.
//
// Up to kFoldSliceStride an owner takes a group (grid x: groups); one writer per output.  Above
// it grid x cuts the stride into slices of kFoldSliceVec vectors (at most kFoldMaxSlices workgroups
// a group, each striding over the slices: atomics on one address serialise) and grid y walks the
// groups; each workgroup adds its slices' count into set_bits[g] and raises changed[g], both zeroed
// on the stream by the caller (every raiser stores the same 1, so the byte needs no atomic).
// A group that is empty, whose seg runs backwards or past n_src, or that names an id >=
// n_filters is skipped (destination untouched, outputs 0) and sets status[1].
template <uint32_t OP, bool WRITE>
__global__ __launch_bounds__(kBankLanes) void bank_fold_kernel(uint4* bits, uint64_t stride_vec, uint64_t n_filters,
                                                               const uint32_t* __restrict__ dst_ids,
                                                               const unsigned long long* __restrict__ seg,
                                                               const uint32_t* __restrict__ src_ids, uint64_t groups,
                                                               uint64_t n_src, uint8_t* __restrict__ changed,
                                                               unsigned long long* __restrict__ set_bits,
                                                               uint32_t* __restrict__ status) {
    __shared__ unsigned long long s_part[kBankLanes / 64];
    const bool sliced = stride_vec * 16 > kFoldSliceStride;
    const Owner o = bank_owner(stride_vec);
    const uint32_t per = o.wave ? kBankLanes / 64 : 1u;
    // a slice is one pass of the workgroup's lanes; workgroup x takes slices x, x + gridDim.x, ...
    const uint64_t v0 = sliced ? (uint64_t)blockIdx.x * kFoldSliceVec : 0, v1 = stride_vec;
    const uint64_t vstep = sliced ? (uint64_t)gridDim.x * kFoldSliceVec : (uint64_t)o.lanes * kFoldUnroll;
    const uint64_t first = sliced ? blockIdx.y : (uint64_t)blockIdx.x * per;
    const uint64_t step = sliced ? gridDim.y : (uint64_t)gridDim.x * per;
    for (uint64_t base = first; base < groups; base += step) {
        const uint64_t g = base + (o.wave ? (threadIdx.x >> 6) : 0u);
        const bool live = g < groups;
        uint64_t lo = 0, hi = 0;
        unsigned long long bad = 0;
        if (live) {
            lo = seg[g];
            hi = seg[g + 1];
            if (!(lo < hi && hi <= n_src)) {
                bad = 1;
                hi = lo;   // nothing of src_ids is read
            }
            for (uint64_t s = lo + o.lane; s < hi; s += o.lanes)
                if ((uint64_t)src_ids[s] >= n_filters) bad = 1;
            if (WRITE && (uint64_t)dst_ids[g] >= n_filters) bad = 1;
        }
        bad = owner_reduce<true>(bad, o, s_part);
        unsigned long long pop = 0, chg = 0;
        if (live && !bad) {
            uint4* d = WRITE ? bits + (uint64_t)dst_ids[g] * stride_vec : nullptr;
            for (uint64_t vb = v0 + o.lane; vb < v1; vb += vstep) {
                uint4 acc[kFoldUnroll];
                const uint4* p = bits + (uint64_t)src_ids[lo] * stride_vec;
#pragma unroll
                for (uint32_t u = 0; u < kFoldUnroll; ++u) {
                    const uint64_t v = vb + (uint64_t)u * o.lanes;
                    acc[u] = v < v1 ? p[v] : make_uint4(0u, 0u, 0u, 0u);
                }
                for (uint64_t s = lo + 1; s < hi; ++s) {
                    p = bits + (uint64_t)src_ids[s] * stride_vec;
#pragma unroll
                    for (uint32_t u = 0; u < kFoldUnroll; ++u) {
                        const uint64_t v = vb + (uint64_t)u * o.lanes;
                        if (v < v1) acc[u] = bitop4<OP>(acc[u], p[v]);
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kFoldUnroll; ++u) {
                    const uint64_t v = vb + (uint64_t)u * o.lanes;
                    if (v >= v1) continue;
                    pop += popc4(acc[u]);
                    if constexpr (WRITE) {
                        const uint4 old = d[v];
                        if ((old.x ^ acc[u].x) | (old.y ^ acc[u].y) | (old.z ^ acc[u].z) | (old.w ^ acc[u].w)) {
                            d[v] = acc[u];
                            chg = 1;
                        }
                    }
                }
            }
        }
        pop = owner_reduce<false>(pop, o, s_part);
        if (WRITE) chg = owner_reduce<true>(chg, o, s_part);
        if (live && o.lane == 0) {
            if (bad) status[1] = 1u;
            if (sliced) {
                if (set_bits && pop) atomicAdd(set_bits + g, pop);
                if (changed && chg) changed[g] = 1;
            } else {
                if (set_bits) set_bits[g] = pop;
                if (changed) changed[g] = (uint8_t)chg;
            }
        }
    }
}

// ---- overlap matrix: BITCOUNT(row filter AND column filter) for every pair --------------------

// The binary analogue of a tiled GEMM, C[i][j] = sum over words of popc(A[i][w] & B[j][w]).  A
// workgroup owns kOvTile x kOvTile pairs and walks its slice of the stride in chunks of
// kOvChunkVec vectors per filter, staged through LDS (16-byte loads, ds_write_b128); every staged
// word is then used by the tile's 64 filters of the other side.  Lane (ty, tx) = (lane / 16,
// lane % 16) keeps the 4 x 4 pairs of rows ty + 16 i and columns tx + 16 j.
//
// LDS: a filter's chunk is a row of kOvPitchVec = 17 vectors (68 words).  The 16 lanes one
// ds_read_b128 group serves hold every tx and at most two ty: the column rows tx * 68 words
// start at bank 4 tx mod 64, sixteen disjoint runs of 4 banks, and the row-side address is a
// broadcast per ty, two runs 4 banks apart.  The stage's ds_write_b128 groups of 8 lanes write 32
// consecutive words.
constexpr uint32_t kOvTile = 64;
constexpr uint32_t kOvBlock = 4;
constexpr uint32_t kOvChunkVec = 16;
constexpr uint32_t kOvPitchVec = kOvChunkVec + 1;
constexpr uint64_t kOvMaxSliceVec = 1ull << 24;   // 2^31 bits a slice: a pair's 32-bit count cannot overflow
constexpr uint64_t kOvFill = 1024;                // workgroups wanted before the stride stops being split
constexpr uint64_t kOvMinChunks = 8;              // chunks a slice keeps at least (2 KiB per filter)
constexpr uint32_t kOvMaxGrid = 2048;             // tiles per grid dimension; a workgroup strides beyond
static_assert(kOvTile == 16 * kOvBlock && kBankLanes == 256 && 2 * kOvTile * kOvChunkVec == 8 * kBankLanes,
              "16 x 16 lanes, 4 x 4 pairs each, 8 staged vectors per lane and chunk");

// One staged chunk's share of a lane's counters: rows ty + 16 i, columns tx + 16 j.  NI x NJ live
// register blocks compiled in (the full tile and the two small squares), or 0: ni x nj at run
// time, a uniform branch per block.
template <uint32_t NI, uint32_t NJ>
__device__ __forceinline__ void ov_chunk(const uint4* s_ab, uint32_t ty, uint32_t tx, uint32_t ni, uint32_t nj,
                                         uint32_t (&acc)[kOvBlock][kOvBlock]) {
    constexpr uint32_t CI = NI ? NI : kOvBlock, CJ = NJ ? NJ : kOvBlock;
#pragma unroll 2
    for (uint32_t vv = 0; vv < kOvChunkVec; ++vv) {
        uint4 a[CI], b[CJ];
#pragma unroll
        for (uint32_t i = 0; i < CI; ++i)
            if (NI || i < ni) a[i] = s_ab[(ty + 16 * i) * kOvPitchVec + vv];
#pragma unroll
        for (uint32_t j = 0; j < CJ; ++j)
            if (NJ || j < nj) b[j] = s_ab[(kOvTile + tx + 16 * j) * kOvPitchVec + vv];
#pragma unroll
        for (uint32_t i = 0; i < CI; ++i)
#pragma unroll
            for (uint32_t j = 0; j < CJ; ++j)
                if ((NI || i < ni) && (NJ || j < nj))
                    acc[i][j] += __builtin_popcount(a[i].x & b[j].x) + __builtin_popcount(a[i].y & b[j].y) +
                                 __builtin_popcount(a[i].z & b[j].z) + __builtin_popcount(a[i].w & b[j].w);
    }
}

// out[(r * cols + c)] = BITCOUNT(filter of row r AND filter of column c); row r is filter
// row_ids[r] (NULL: row0 + r), column c is col_ids[c] (NULL: c).  sym: the column list IS the row
// list (cols == rows), the tiles strictly below the diagonal are skipped and mirrored from above.
// add: gridDim.z > 1, the caller zeroed out and every slice adds its part (64-bit atomics; integer
// sums are exact in any order); otherwise one writer per entry, zeros included.  A row or column
// whose id is >= n_filters reads as the empty filter and sets status[1].
__global__ __launch_bounds__(kBankLanes) void bank_overlap_kernel(const uint4* __restrict__ bits, uint64_t stride_vec,
                                                                  uint64_t n_filters,
                                                                  const uint32_t* __restrict__ row_ids, uint64_t row0,
                                                                  uint64_t rows, const uint32_t* __restrict__ col_ids,
                                                                  uint64_t cols, uint32_t sym, uint64_t slice_vec,
                                                                  uint32_t add, unsigned long long* __restrict__ out,
                                                                  uint32_t* __restrict__ status) {
    __shared__ uint4 s_ab[2 * kOvTile * kOvPitchVec];   // [row side | column side]
    __shared__ uint64_t s_f[2 * kOvTile];               // the tile's filters, ~0: none
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15u;
    const uint64_t row_tiles = (rows + kOvTile - 1) / kOvTile, col_tiles = (cols + kOvTile - 1) / kOvTile;
    const uint64_t z0 = (uint64_t)blockIdx.z * slice_vec;
    const uint64_t z1 = z0 + slice_vec < stride_vec ? z0 + slice_vec : stride_vec;
    for (uint64_t ti = blockIdx.y; ti < row_tiles; ti += gridDim.y) {
        for (uint64_t tj = blockIdx.x; tj < col_tiles; tj += gridDim.x) {
            if (sym && tj < ti) continue;
            const uint64_t r0 = ti * kOvTile, c0 = tj * kOvTile;
            const uint32_t nr = (uint32_t)(rows - r0 < kOvTile ? rows - r0 : kOvTile);
            const uint32_t nc = (uint32_t)(cols - c0 < kOvTile ? cols - c0 : kOvTile);
            const uint32_t ni = (nr + 15u) / 16u, nj = (nc + 15u) / 16u;   // live register-block rows / columns
            __syncthreads();   // the previous tile's s_f is read no more
            if (tid < 2 * kOvTile) {
                const bool col = tid >= kOvTile;
                const uint32_t t = col ? tid - kOvTile : tid;
                uint64_t f = ~0ull;
                if (t < (col ? nc : nr)) {
                    f = col ? (col_ids ? (uint64_t)col_ids[c0 + t] : c0 + t)
                            : (row_ids ? (uint64_t)row_ids[r0 + t] : row0 + r0 + t);
                    if (f >= n_filters) {
                        status[1] = 1u;
                        f = ~0ull;
                    }
                }
                s_f[tid] = f;
            }
            __syncthreads();
            uint32_t acc[kOvBlock][kOvBlock];
#pragma unroll
            for (uint32_t i = 0; i < kOvBlock; ++i)
#pragma unroll
                for (uint32_t j = 0; j < kOvBlock; ++j) acc[i][j] = 0;
            for (uint64_t v0 = z0; v0 < z1; v0 += kOvChunkVec) {
                // stage: pass `it` brings 16 filters (it < 4: rows 16 it.., else columns), 16 lanes a filter
                uint4 x[8];
#pragma unroll
                for (uint32_t it = 0; it < 8; ++it) {
                    x[it] = make_uint4(0u, 0u, 0u, 0u);
                    if (it < kOvBlock ? it >= ni : it - kOvBlock >= nj) continue;
                    const uint64_t f = s_f[it * 16 + ty];
                    if (f != ~0ull && v0 + tx < z1) x[it] = bits[f * stride_vec + v0 + tx];
                }
#pragma unroll
                for (uint32_t it = 0; it < 8; ++it) {
                    if (it < kOvBlock ? it >= ni : it - kOvBlock >= nj) continue;
                    s_ab[(it * 16 + ty) * kOvPitchVec + tx] = x[it];
                }
                __syncthreads();
                if (ni == kOvBlock && nj == kOvBlock) ov_chunk<kOvBlock, kOvBlock>(s_ab, ty, tx, ni, nj, acc);
                else if (ni == 2 && nj == 2) ov_chunk<2, 2>(s_ab, ty, tx, ni, nj, acc);
                else if (ni == 1 && nj == 1) ov_chunk<1, 1>(s_ab, ty, tx, ni, nj, acc);
                else ov_chunk<0, 0>(s_ab, ty, tx, ni, nj, acc);
                __syncthreads();
            }
            const bool mirror = sym && tj != ti;
#pragma unroll
            for (uint32_t i = 0; i < kOvBlock; ++i)
#pragma unroll
                for (uint32_t j = 0; j < kOvBlock; ++j) {
                    const uint32_t lr = ty + 16 * i, lc = tx + 16 * j;
                    if (i >= ni || j >= nj || lr >= nr || lc >= nc) continue;
                    const uint64_t r = r0 + lr, c = c0 + lc;
                    const unsigned long long val = acc[i][j];
                    if (add) {
                        if (val) {
                            atomicAdd(out + r * cols + c, val);
                            if (mirror) atomicAdd(out + c * cols + r, val);
                        }
                    } else {
                        out[r * cols + c] = val;
                        if (mirror) out[c * cols + r] = val;
                    }
                }
        }
    }
}

// At most kOvFew x kOvFew pairs of long filters: a tile's slices would keep only a few hundred
// bytes per filter in flight between two barriers, so the pairs are streamed instead, as the
// fold's slice grid streams its sources.  At most kOvFewBlocks workgroups stride over the vectors
// (every one ends in an atomic per pair on the same few addresses, which serialise); a lane loads
// its vector of every listed filter, counts the up to 16 ANDs and the workgroup adds each pair's
// sum into the zeroed out[] with one 64-bit atomic.  Ids as in bank_overlap_kernel
// (NULL: row r is filter r, column c filter c).
constexpr uint32_t kOvFew = 4;
constexpr uint64_t kOvFewBlocks = 512;

__global__ __launch_bounds__(kBankLanes) void bank_overlap_few_kernel(const uint4* __restrict__ bits, uint64_t stride_vec,
                                                                      uint64_t n_filters,
                                                                      const uint32_t* __restrict__ row_ids, uint32_t rows,
                                                                      const uint32_t* __restrict__ col_ids, uint32_t cols,
                                                                      unsigned long long* __restrict__ out,
                                                                      uint32_t* __restrict__ status) {
    __shared__ unsigned long long s_part[kBankLanes / 64];
    uint64_t fr[kOvFew], fc[kOvFew];   // ~0: no such row / column, or a refused id
#pragma unroll
    for (uint32_t i = 0; i < kOvFew; ++i) {
        fr[i] = i < rows ? (row_ids ? (uint64_t)row_ids[i] : i) : ~0ull;
        fc[i] = i < cols ? (col_ids ? (uint64_t)col_ids[i] : i) : ~0ull;
        if ((i < rows && fr[i] >= n_filters) || (i < cols && fc[i] >= n_filters)) status[1] = 1u;
        if (fr[i] >= n_filters) fr[i] = ~0ull;
        if (fc[i] >= n_filters) fc[i] = ~0ull;
    }
    uint32_t acc[kOvFew][kOvFew];   // a lane sees at most 2^30 / 256 vectors of 128 bits: no overflow
#pragma unroll
    for (uint32_t i = 0; i < kOvFew; ++i)
#pragma unroll
        for (uint32_t j = 0; j < kOvFew; ++j) acc[i][j] = 0;
#pragma unroll 2
    for (uint64_t v = (uint64_t)blockIdx.x * kBankLanes + threadIdx.x; v < stride_vec; v += (uint64_t)gridDim.x * kBankLanes) {
        uint4 a[kOvFew], b[kOvFew];
#pragma unroll
        for (uint32_t i = 0; i < kOvFew; ++i) {
            a[i] = fr[i] != ~0ull ? bits[fr[i] * stride_vec + v] : make_uint4(0u, 0u, 0u, 0u);
            b[i] = fc[i] != ~0ull ? bits[fc[i] * stride_vec + v] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t i = 0; i < kOvFew; ++i)
#pragma unroll
            for (uint32_t j = 0; j < kOvFew; ++j)
                if (i < rows && j < cols)   // uniform
                    acc[i][j] += __builtin_popcount(a[i].x & b[j].x) + __builtin_popcount(a[i].y & b[j].y) +
                                 __builtin_popcount(a[i].z & b[j].z) + __builtin_popcount(a[i].w & b[j].w);
    }
    Owner o;
    o.wave = false;
    o.lane = threadIdx.x;
    o.lanes = kBankLanes;
#pragma unroll
    for (uint32_t i = 0; i < kOvFew; ++i)
#pragma unroll
        for (uint32_t j = 0; j < kOvFew; ++j) {
            if (i >= rows || j >= cols) continue;   // uniform
            const unsigned long long sum = owner_reduce<false>(acc[i][j], o, s_part);
            if (threadIdx.x == 0 && sum) atomicAdd(out + (uint64_t)i * cols + j, sum);
        }
}

}  // namespace

struct bf_bank : BfHostCore {   // mutex, device, stream, error, stream order: bf_host.h (the profile state idle)
    uint64_t m = 0, reach = 0, n_filters = 0, stride = 0, bytes = 0;
    uint32_t k = 0;
    uint64_t batch_keys = 0, batch_bytes = 0;
    BfGeom g{};                        // g.bits: the whole allocation, filter f at word f * stride / 4
    uint32_t* h_status = nullptr;      // pinned [key offsets | filter id], written by the kernels
    uint32_t* d_status = nullptr;      // ... its device address
    // staging of the host-pointer calls
    uint8_t *d_keys = nullptr, *d_out = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t* d_ids = nullptr;
    uint64_t keys_cap = 0, n_cap = 0;
    uint8_t* d_io = nullptr;           // export / import: [count * stride bytes | count lengths]
    uint64_t io_cap = 0;
    uint32_t* d_list = nullptr;        // a host call's id list
    uint64_t list_cap = 0;
    // bf_bank_insert_many_seq*: [first-index table | 16 B digest per key | 8 B 0-probe mask per key]
    uint8_t* d_seq = nullptr;
    uint64_t seq_cap = 0;
    uint32_t seq_form = 0;             // bf_bank_set_seq_form: BF_BANK_SEQ_*
    // bf_bank_insert_many_changes (host form): [count, 8 B | bits, 8 B an entry | ids, 4 B an entry]
    uint8_t* d_chg = nullptr;
    uint64_t chg_cap = 0;
};

namespace {

// b == NULL: a create-time error, read back with bf_bank_last_error(NULL).
template <typename... A>
int bank_err(bf_bank* b, int code, const char* fmt, A... a) {
    return bf_set_err(b, &g_bank_create_error, code, fmt, a...);
}

// stride of a filter of m bits; false when it does not fit 64 bits.
bool bank_stride(uint64_t m_bits, uint64_t* stride) {
    const uint64_t bytes = m_bits / 8 + (m_bits % 8 ? 1 : 0);
    if (bytes > UINT64_MAX - 127) return false;
    *stride = (bytes + 127) / 128 * 128;
    return true;
}

int grow(bf_bank* b, void** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return BF_OK;
    // an earlier call's launches may still read the old buffer
    HIPCHK(b, hipStreamSynchronize(b->stream));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t want = std::max<uint64_t>(need, 1 << 16);
    HIPCHK(b, hipMalloc(p, want));
    *cap = want;
    return BF_OK;
}

int ensure_keys_io(bf_bank* b, uint64_t key_bytes, uint64_t n) {
    int rc = grow(b, (void**)&b->d_keys, &b->keys_cap, key_bytes + 16);
    if (rc) return rc;
    if (n + 1 > b->n_cap) {
        HIPCHK(b, hipStreamSynchronize(b->stream));
        for (void* p : {(void*)b->d_off, (void*)b->d_ids, (void*)b->d_out})
            if (p) (void)hipFree(p);
        b->d_off = nullptr;
        b->d_ids = nullptr;
        b->d_out = nullptr;
        b->n_cap = 0;
        const uint64_t cap = std::max<uint64_t>(n + 1, 1 << 12);
        HIPCHK(b, hipMalloc((void**)&b->d_off, cap * 8));
        HIPCHK(b, hipMalloc((void**)&b->d_ids, cap * 4));
        HIPCHK(b, hipMalloc((void**)&b->d_out, cap));
        b->n_cap = cap;
    }
    return BF_OK;
}

// list (insert only): the kernel also lists the bits it flipped.
int launch_keys(bf_bank* b, int op, const uint8_t* d_keys, const uint64_t* d_off, const uint32_t* d_ids, uint64_t n,
                uint8_t* d_out8, hipStream_t s, const BankList<true>* list = nullptr) {
    if (n >= (1ull << 31) * (uint64_t)kBankTile) return bank_err(b, BF_EINVAL, "n too large for one launch");
    uint64_t bias = 0;
    const uint8_t* k16 = align_keys(d_keys, &bias);
    const dim3 grid((uint32_t)((n + kBankTile - 1) / kBankTile)), block(kBankTile);
#define BF_KEYS_LAUNCH(OP, LIST, list_arg)                                                                              \
    hipLaunchKernelGGL((bank_keys_kernel<OP, LIST>), grid, block, 0, s, b->g, b->n_filters, b->stride / 4, k16, d_off, \
                       bias, d_ids, n, d_out8, b->d_status, list_arg)
    if (op == BANK_INSERT && list) BF_KEYS_LAUNCH(BANK_INSERT, true, *list);
    else if (op == BANK_INSERT) BF_KEYS_LAUNCH(BANK_INSERT, false, BankList<false>{});
    else BF_KEYS_LAUNCH(BANK_INCLUDE, false, BankList<false>{});
#undef BF_KEYS_LAUNCH
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// Every id of a host list below n_filters; `what` names the list in the refusal.
int check_ids(bf_bank* b, const char* what, const uint32_t* ids, uint64_t count) {
    for (uint64_t i = 0; i < count; ++i)
        if ((uint64_t)ids[i] >= b->n_filters)
            return bank_err(b, BF_EINVAL, "%s[%llu] = %u is not below n_filters = %llu", what, (unsigned long long)i, ids[i],
                            (unsigned long long)b->n_filters);
    return BF_OK;
}

// A _dev call's alignment refusal: the addresses (addr) that must be multiples of 8 ORed together,
// and those of 4; `rule` spells the pointers out.
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
int check_aligned(bf_bank* b, uintptr_t by8, uintptr_t by4, const char* rule) {
    if ((by8 & 7u) || (by4 & 3u)) return bank_err(b, BF_EINVAL, "misaligned device pointer (%s)", rule);
    return BF_OK;
}

// Key by key, lowest first: bf_check_offsets' rule, then (ids != NULL) the key's filter id in range.
int check_keys(bf_bank* b, const uint64_t* offsets, const uint32_t* ids, uint64_t n) {
    const uint64_t lo = offsets[0], hi = offsets[n];
    for (uint64_t j = 0; j < n; ++j) {
        if (!key_ok(lo, offsets[j], offsets[j + 1], hi, nullptr))
            return bank_err(b, BF_EINVAL, "key %llu: offsets must be non-decreasing and every key below 2 GiB",
                            (unsigned long long)j);
        if (ids && (uint64_t)ids[j] >= b->n_filters)
            return bank_err(b, BF_EINVAL, "key %llu: filter id %u is not below n_filters = %llu", (unsigned long long)j,
                            ids[j], (unsigned long long)b->n_filters);
    }
    return BF_OK;
}

// The host forms' refusals (nothing is launched).
int check_batch(bf_bank* b, const uint8_t* keys, const uint64_t* offsets, const uint32_t* ids, uint64_t n) {
    if (!offsets || !ids || (!keys && offsets[n] != offsets[0])) return bank_err(b, BF_EINVAL, "NULL keys / offsets / filter_ids");
    return check_keys(b, offsets, ids, n);
}

// ---- the chunks of the host-pointer keyed calls -----------------------------------------------

// Where the chunk that begins at key a ends: at most max_keys keys (the caller's bound) and, where
// their bytes exceed batch_bytes, the longest run within it, at least one key (a longer key goes alone).
uint64_t chunk_end(const bf_bank* b, const uint64_t* offsets, uint64_t n, uint64_t a, uint64_t max_keys) {
    uint64_t e = std::min<uint64_t>(n, a + max_keys);
    if (offsets[e] - offsets[a] > b->batch_bytes) {
        e = (uint64_t)(std::upper_bound(offsets + a, offsets + e + 1, offsets[a] + b->batch_bytes) - offsets) - 1;
        if (e <= a) e = a + 1;
    }
    return e;
}

// The keys [a, e) staged on the bank's stream: their bytes at d_keys with 16 zero bytes behind,
// their offsets rebased to 0 at d_off (offsets[0] need not be 0), their ids at d_ids (ids == NULL:
// a call without per-key ids).  The staging buffers and the caller's `rebased` are in use until
// the caller has synchronised the stream.
int stage_chunk(bf_bank* b, const uint8_t* keys, const uint64_t* offsets, const uint32_t* ids, uint64_t a, uint64_t e,
                std::vector<uint64_t>& rebased) {
    const uint64_t cn = e - a, nbytes = offsets[e] - offsets[a];
    int rc = ensure_keys_io(b, nbytes, cn);
    if (rc) return rc;
    rebased.resize(cn + 1);
    for (uint64_t j = 0; j <= cn; ++j) rebased[j] = offsets[a + j] - offsets[a];
    if (nbytes) HIPCHK(b, hipMemcpyAsync(b->d_keys, keys + offsets[a], nbytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(b, hipMemsetAsync(b->d_keys + nbytes, 0, 16, b->stream));
    HIPCHK(b, hipMemcpyAsync(b->d_off, rebased.data(), (cn + 1) * 8, hipMemcpyHostToDevice, b->stream));
    if (ids) HIPCHK(b, hipMemcpyAsync(b->d_ids, ids + a, cn * 4, hipMemcpyHostToDevice, b->stream));
    return BF_OK;
}

// Host-pointer insert / include?: chunks of at most batch_keys keys.
int run_host(bf_bank* b, int op, const uint8_t* keys, const uint64_t* offsets, const uint32_t* ids, uint64_t n,
             uint8_t* out) {
    if (!b) return BF_EINVAL;
    if (n == 0) return BF_OK;
    CallScope cs(b);
    if (op == BANK_INCLUDE && !out) return bank_err(b, BF_EINVAL, "out is NULL");
    int rc = check_batch(b, keys, offsets, ids, n);
    if (rc) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    std::vector<uint64_t> h_off;   // stage_chunk's, read by its copy until the synchronise
    for (uint64_t a = 0, e; a < n; a = e) {
        e = chunk_end(b, offsets, n, a, b->batch_keys);
        if ((rc = stage_chunk(b, keys, offsets, ids, a, e, h_off))) return rc;
        if ((rc = launch_keys(b, op, b->d_keys, b->d_off, b->d_ids, e - a, out ? b->d_out : nullptr, b->stream))) return rc;
        if (out) HIPCHK(b, hipMemcpyAsync(out + a, b->d_out, e - a, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(b, hipStreamSynchronize(b->stream));   // the staging buffers are free again
    }
    return BF_OK;
}

int run_dev(bf_bank* b, int op, const uint8_t* d_keys, const uint64_t* d_off, const uint32_t* d_ids, uint64_t n,
            uint8_t* d_out, void* stream) {
    if (!b) return BF_EINVAL;
    if (n == 0) return BF_OK;
    CallScope cs(b);
    if (!d_keys || !d_off || !d_ids || (op == BANK_INCLUDE && !d_out)) return bank_err(b, BF_EINVAL, "NULL device pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_keys(b, op, d_keys, d_off, d_ids, n, d_out, s);
}

// ---- sequential flags: the plan, the scratch and the chunk loop ------------------------------

constexpr uint64_t kSeqDirectMaxBytes = 1ull << 25;   // a bank of 2^28 bits: a direct table of 1 GiB

// The table's form for a call whose largest chunk has cn keys.  bf_bank_set_seq_form forces a
// form where it is legal: the hash form always is, the direct form up to 1 GiB.  Otherwise the
// table's own rule, over the bank's bits.
bool seq_direct(const bf_bank* b, uint64_t cn) {
    if (b->seq_form == BF_BANK_SEQ_HASH) return false;
    if (b->seq_form == BF_BANK_SEQ_DIRECT) return b->bytes <= kSeqDirectMaxBytes;
    return seq_direct_fits(b->bytes * 8, cn, b->k);
}

// How a sequential call of n keys runs (bf_bank_seq_plan reports it): the table's form, the keys
// of its largest chunk and the scratch that chunk needs.  batch_keys is the caller's own bound on
// a chunk (UINT64_MAX: none, the _dev forms).  The form is the call's, from min(n,
// bf_seq_chunk_keys(k)) whatever batch_keys is; the scratch is sized for the chunks launched.
struct BankSeqPlan {
    bool direct;
    uint64_t chunk, scratch;
};

BankSeqPlan seq_plan(const bf_bank* b, uint64_t n, uint64_t batch_keys) {
    const uint64_t by_width = bf_seq_chunk_keys(b->k), chunk = std::min<uint64_t>(n, std::min<uint64_t>(batch_keys, by_width));
    const bool direct = seq_direct(b, std::min<uint64_t>(n, by_width));
    return {direct, chunk, chunk ? seq_scratch_bytes(direct, b->bytes * 8, chunk, b->k) : 0};
}

// The scratch is the bank's and grows on demand.  An earlier call may still use the old buffer
// on ITS stream (a _dev call on a caller's stream), so growth waits as bf_bank_sync does, not on
// the bank's own stream only.
int ensure_seq_scratch(bf_bank* b, uint64_t need) {
    if (need <= b->seq_cap) return BF_OK;
    HIPCHK(b, hipStreamSynchronize(b->stream));
    if (b->order_valid) HIPCHK(b, hipEventSynchronize(b->order_ev));
    if (b->d_seq) (void)hipFree(b->d_seq);
    b->d_seq = nullptr;
    b->seq_cap = 0;
    HIPCHK(b, hipMalloc((void**)&b->d_seq, need));
    b->seq_cap = need;
    return BF_OK;
}

// One chunk of at most bf_seq_chunk_keys(k) keys: clear, candidates, mark, in stream order.
// list: the mark kernel also lists the bits it flipped.
int launch_seq_chunk(bf_bank* b, bool direct, const uint8_t* d_keys, const uint64_t* d_off, const uint32_t* d_ids,
                     uint64_t cn, uint8_t* d_out8, hipStream_t s, const BankList<true>* list = nullptr) {
    const SeqCarve c = seq_carve(b->d_seq, direct, b->bytes * 8, cn, b->k);
    HIPCHK(b, seq_table_clear(c, s));
    uint64_t bias = 0;
    const uint8_t* k16 = align_keys(d_keys, &bias);
    const dim3 grid((uint32_t)((cn + kBankTile - 1) / kBankTile)), block(kBankTile);
    const uint64_t sw = b->stride / 4;
#define BF_SEQ_MARK(DIRECT, LIST, list_arg)                                                                           \
    hipLaunchKernelGGL((bank_seq_mark_kernel<DIRECT, LIST>), grid, block, 0, s, b->g, sw, d_ids, cn, c.tkeys, c.tvals, \
                       c.tmask, c.digests, c.cand, d_out8, list_arg)
#define BF_SEQ_LAUNCH(DIRECT)                                                                                          \
    do {                                                                                                               \
        hipLaunchKernelGGL(bank_seq_candidates_kernel<DIRECT>, grid, block, 0, s, b->g, b->n_filters, sw, k16, d_off,  \
                           bias, d_ids, cn, c.tkeys, c.tvals, c.tmask, c.digests, c.cand, b->d_status);                \
        if (list) BF_SEQ_MARK(DIRECT, true, *list);                                                                    \
        else BF_SEQ_MARK(DIRECT, false, BankList<false>{});                                                            \
    } while (0)
    if (direct) BF_SEQ_LAUNCH(true);
    else BF_SEQ_LAUNCH(false);
#undef BF_SEQ_LAUNCH
#undef BF_SEQ_MARK
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// The sequential insert on device arrays, on an opened stream: the batch cut into chunks, every
// chunk's list entries (list != NULL) added behind the ones before through the one counter.
int seq_dev_chunks(bf_bank* b, const uint8_t* d_keys, const uint64_t* d_off, const uint32_t* d_ids, uint64_t n,
                   uint8_t* d_out8, hipStream_t s, const BankList<true>* list) {
    const BankSeqPlan plan = seq_plan(b, n, UINT64_MAX);
    int rc = ensure_seq_scratch(b, plan.scratch);   // synchronises only when the scratch has to grow
    if (rc) return rc;
    // offsets[0] need not be 0, so d_off + a is the offsets array of the keys from a on
    for (uint64_t a = 0; a < n; a += plan.chunk) {
        const uint64_t cn = std::min<uint64_t>(n - a, plan.chunk);
        if ((rc = launch_seq_chunk(b, plan.direct, d_keys, d_off + a, d_ids + a, cn, d_out8 ? d_out8 + a : nullptr, s, list)))
            return rc;
    }
    return BF_OK;
}

// ---- the list of flipped bits: the host form's scratch ----------------------------------------

// Up to this many bytes of [count | bits | ids] come back in one copy with the count; a longer list
// is fetched after its count is known.  A per-key call (k entries) pays one round trip.
constexpr uint64_t kChgOneCopy = 16u << 10;

uint64_t chg_bytes(uint64_t entries) { return 8 + entries * 12; }

// ids == NULL lists every filter in order; then count must be n_filters.
int check_list(bf_bank* b, const uint32_t* ids, uint64_t count, bool host_ids) {
    if (!ids) {
        if (count != b->n_filters)
            return bank_err(b, BF_EINVAL, "ids == NULL lists every filter: count must be n_filters = %llu, got %llu",
                            (unsigned long long)b->n_filters, (unsigned long long)count);
        return BF_OK;
    }
    return host_ids ? check_ids(b, "ids", ids, count) : BF_OK;
}

// A host id list on the device (NULL stays NULL).
int stage_list(bf_bank* b, const uint32_t* ids, uint64_t count, const uint32_t** d_ids) {
    *d_ids = nullptr;
    if (!ids || !count) return BF_OK;
    int rc = grow(b, (void**)&b->d_list, &b->list_cap, count * 4);
    if (rc) return rc;
    HIPCHK(b, hipMemcpyAsync(b->d_list, ids, count * 4, hipMemcpyHostToDevice, b->stream));
    *d_ids = b->d_list;
    return BF_OK;
}

// The staged mask of one chunk of a host cross query stays under this (a row longer than it goes alone).
constexpr uint64_t kAcrossMaskCap = 64ull << 20;

// Bytes of a mask row of count entries, 8 * ceil(count / 64).
uint64_t across_row_bytes(uint64_t count) { return (count / 64 + (count % 64 ? 1 : 0)) * 8; }

int launch_across(bf_bank* b, const uint8_t* d_keys, const uint64_t* d_off, uint64_t n, const uint32_t* d_ids,
                  uint64_t count, uint8_t* d_mask, hipStream_t s) {
    if (n >= (1ull << 31) * (uint64_t)kBankTile) return bank_err(b, BF_EINVAL, "n too large for one launch");
    uint64_t bias = 0;
    const uint8_t* k16 = align_keys(d_keys, &bias);
    const uint64_t chunks = (count + kAcrossChunk - 1) / kAcrossChunk;
    const dim3 grid((uint32_t)((n + kBankTile - 1) / kBankTile), (uint32_t)std::min<uint64_t>(chunks, kAcrossMaxY));
    hipLaunchKernelGGL(bank_across_kernel, grid, dim3(kBankTile), 0, s, b->g, b->n_filters, b->stride / 4, k16, d_off,
                       bias, d_ids, count, n, across_row_bytes(count) / 8, reinterpret_cast<unsigned long long*>(d_mask),
                       b->d_status);
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

int launch_bitcount(bf_bank* b, const uint32_t* d_ids, uint64_t count, uint64_t* d_out, hipStream_t s) {
    hipLaunchKernelGGL(bank_bitcount_kernel, dim3(owned_grid(b->stride, count)), dim3(kBankLanes), 0, s,
                       reinterpret_cast<const uint4*>(b->g.bits), b->stride / 16, b->n_filters, d_ids, count,
                       reinterpret_cast<unsigned long long*>(d_out), b->d_status);
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// Export and import stage count filters as [count * stride bytes | count lengths]: *data is the
// bytes of the first part, *total of both.
int io_bytes(bf_bank* b, uint64_t count, uint64_t* data, uint64_t* total) {
    if (__builtin_mul_overflow(count, b->stride, data) || __builtin_add_overflow(*data, count * 8, total))
        return bank_err(b, BF_EINVAL, "%llu filters of %llu bytes overflow a 64-bit byte size", (unsigned long long)count,
                        (unsigned long long)b->stride);
    return BF_OK;
}

// ids == NULL clears every filter (one fill of the allocation; count is not read).
int launch_clear(bf_bank* b, const uint32_t* d_ids, uint64_t count, hipStream_t s) {
    if (!d_ids) {
        HIPCHK(b, hipMemsetAsync(b->g.bits, 0, b->bytes, s));
        return BF_OK;
    }
    if (count == 0) return BF_OK;
    hipLaunchKernelGGL(bank_clear_kernel, dim3(owned_grid(b->stride, count)), dim3(kBankLanes), 0, s,
                       reinterpret_cast<uint4*>(b->g.bits), b->stride / 16, b->n_filters, d_ids, count, b->d_status);
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// What both fold forms refuse without reading a list.
int check_fold_op(bf_bank* b, uint32_t op, bool has_dst) {
    if (op != BF_BITOP_AND && op != BF_BITOP_OR && op != BF_BITOP_XOR) return bank_err(b, BF_EINVAL, "unknown op %u", op);
    if (op == BF_BITOP_XOR && has_dst)
        return bank_err(b, BF_EINVAL, "BF_BITOP_XOR only counts: dst_ids must be NULL (a parity is not a filter)");
    return BF_OK;
}

// One launch for every group.  The slice regime adds into the outputs, which are zeroed here.
int launch_fold(bf_bank* b, uint32_t op, const uint32_t* d_dst, const uint64_t* d_seg, const uint32_t* d_src,
                uint64_t groups, uint64_t n_src, uint8_t* d_changed, uint64_t* d_set_bits, hipStream_t s) {
    const uint64_t stride_vec = b->stride / 16;
    dim3 grid(owned_grid(b->stride, groups));
    if (b->stride > kFoldSliceStride) {
        const uint64_t slices = std::min<uint64_t>((stride_vec + kFoldSliceVec - 1) / kFoldSliceVec, kFoldMaxSlices);
        const uint64_t gy = std::min<uint64_t>(std::min<uint64_t>(groups, 65535), std::max<uint64_t>(1, kFoldMaxBlocks / slices));
        grid = dim3((uint32_t)slices, (uint32_t)gy);
        if (d_set_bits) HIPCHK(b, hipMemsetAsync(d_set_bits, 0, groups * 8, s));
        if (d_changed) HIPCHK(b, hipMemsetAsync(d_changed, 0, groups, s));
    } else if (d_changed && !d_dst) {
        HIPCHK(b, hipMemsetAsync(d_changed, 0, groups, s));   // a count-only fold changes nothing
    }
    uint4* bits = reinterpret_cast<uint4*>(b->g.bits);
    const unsigned long long* seg = reinterpret_cast<const unsigned long long*>(d_seg);
    unsigned long long* sb = reinterpret_cast<unsigned long long*>(d_set_bits);
#define BF_FOLD_LAUNCH(OP, WRITE)                                                                                      \
    hipLaunchKernelGGL((bank_fold_kernel<OP, WRITE>), grid, dim3(kBankLanes), 0, s, bits, stride_vec, b->n_filters,    \
                       d_dst, seg, d_src, groups, n_src, (WRITE) ? d_changed : nullptr, sb, b->d_status)
    if (op == BF_BITOP_XOR) BF_FOLD_LAUNCH(BF_BITOP_XOR, false);
    else if (op == BF_BITOP_AND && d_dst) BF_FOLD_LAUNCH(BF_BITOP_AND, true);
    else if (op == BF_BITOP_AND) BF_FOLD_LAUNCH(BF_BITOP_AND, false);
    else if (d_dst) BF_FOLD_LAUNCH(BF_BITOP_OR, true);
    else BF_FOLD_LAUNCH(BF_BITOP_OR, false);
#undef BF_FOLD_LAUNCH
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// The list rules both overlap forms share; *out_bytes = rows * cols * 8.
int check_overlap(bf_bank* b, const uint32_t* row_ids, uint64_t rows, const uint32_t* col_ids, uint64_t cols,
                  uint64_t* out_bytes) {
    if (!row_ids && rows != b->n_filters)
        return bank_err(b, BF_EINVAL, "row_ids == NULL lists every filter: rows must be n_filters = %llu, got %llu",
                        (unsigned long long)b->n_filters, (unsigned long long)rows);
    if (!col_ids && cols != rows)
        return bank_err(b, BF_EINVAL, "col_ids == NULL is the row list: cols must be rows = %llu, got %llu",
                        (unsigned long long)rows, (unsigned long long)cols);
    uint64_t pairs = 0;
    if (__builtin_mul_overflow(rows, cols, &pairs) || __builtin_mul_overflow(pairs, (uint64_t)8, out_bytes))
        return bank_err(b, BF_EINVAL, "%llu x %llu counts overflow a 64-bit byte size", (unsigned long long)rows,
                        (unsigned long long)cols);
    return BF_OK;
}

// rows x cols counts at d_out.  d_rows == NULL: row r is filter row0 + r; d_cols == NULL: column
// c is filter c.  sym: the column list is the row list, the lower tiles are mirrored.
int launch_overlap(bf_bank* b, const uint32_t* d_rows, uint64_t row0, uint64_t rows, const uint32_t* d_cols,
                   uint64_t cols, bool sym, uint64_t* d_out, hipStream_t s) {
    const uint64_t stride_vec = b->stride / 16;
    if (rows <= kOvFew && cols <= kOvFew && row0 == 0 && b->stride > kFoldSliceStride) {
        // a handful of long filters: streamed pair by pair, every slice adding into the zeroed counts
        HIPCHK(b, hipMemsetAsync(d_out, 0, rows * cols * 8, s));
        hipLaunchKernelGGL(bank_overlap_few_kernel, dim3((uint32_t)std::min<uint64_t>((stride_vec + kBankLanes - 1) / kBankLanes, kOvFewBlocks)),
                           dim3(kBankLanes), 0, s, reinterpret_cast<const uint4*>(b->g.bits), stride_vec, b->n_filters,
                           d_rows, (uint32_t)rows, d_cols, (uint32_t)cols, reinterpret_cast<unsigned long long*>(d_out),
                           b->d_status);
        HIPCHK(b, hipGetLastError());
        return BF_OK;
    }
    const uint64_t rt = (rows + kOvTile - 1) / kOvTile, ct = (cols + kOvTile - 1) / kOvTile;
    const uint64_t chunks = (stride_vec + kOvChunkVec - 1) / kOvChunkVec;
    // few tiles and a long stride: split it until about kOvFill workgroups run, a slice keeping
    // kOvMinChunks chunks at least and kOvMaxSliceVec vectors at most
    const uint64_t gx = std::min<uint64_t>(ct, kOvMaxGrid), gy = std::min<uint64_t>(rt, kOvMaxGrid);
    const uint64_t tiles = sym ? gx * (gy + 1) / 2 : gx * gy;
    uint64_t nz = std::min<uint64_t>((kOvFill + tiles - 1) / tiles, std::max<uint64_t>(1, chunks / kOvMinChunks));
    nz = std::max<uint64_t>(nz, (stride_vec + kOvMaxSliceVec - 1) / kOvMaxSliceVec);
    const uint64_t per = (chunks + nz - 1) / nz;
    nz = (chunks + per - 1) / per;
    if (nz > 1) HIPCHK(b, hipMemsetAsync(d_out, 0, rows * cols * 8, s));
    hipLaunchKernelGGL(bank_overlap_kernel, dim3((uint32_t)gx, (uint32_t)gy, (uint32_t)nz), dim3(kBankLanes), 0, s,
                       reinterpret_cast<const uint4*>(b->g.bits), stride_vec, b->n_filters, d_rows, row0, rows, d_cols,
                       cols, sym ? 1u : 0u, per * kOvChunkVec, nz > 1 ? 1u : 0u,
                       reinterpret_cast<unsigned long long*>(d_out), b->d_status);
    HIPCHK(b, hipGetLastError());
    return BF_OK;
}

// The staged counts of one chunk of a host overlap stay under this (a row longer than it goes alone).
constexpr uint64_t kOverlapOutCap = 64ull << 20;

}  // namespace

extern "C" {

int bf_bank_stride(uint64_t m_bits, uint64_t* stride) {
    if (!stride || m_bits == 0 || !bank_stride(m_bits, stride)) return BF_EINVAL;
    return BF_OK;
}

int bf_bank_create(uint64_t m_bits, uint32_t k, uint64_t n_filters, const bf_config* cfg, bf_bank** out) {
    if (!out) return bank_err(nullptr, BF_EINVAL, "out is NULL");
    *out = nullptr;
    if (m_bits == 0) return bank_err(nullptr, BF_EINVAL, "m_bits == 0 (ruby.rb:51 divides by m)");
    if (k == 0 || k > BF_MAX_K) return bank_err(nullptr, BF_EINVAL, "k must be in [1, %u], got %u", BF_MAX_K, k);
    if (n_filters == 0) return bank_err(nullptr, BF_EINVAL, "n_filters == 0");
    if (n_filters > (1ull << 32)) return bank_err(nullptr, BF_EINVAL, "n_filters must be at most 2^32 (filter ids are uint32)");
    uint64_t stride = 0, bytes = 0;
    if (!bank_stride(m_bits, &stride) || __builtin_mul_overflow(stride, n_filters, &bytes))
        return bank_err(nullptr, BF_EINVAL, "%llu filters of %llu bits overflow a 64-bit byte size",
                        (unsigned long long)n_filters, (unsigned long long)m_bits);
    if (stride / 4 > (1ull << 32)) return bank_err(nullptr, BF_EINVAL, "m_bits too large for a bank (a filter's words are indexed in 32 bits)");
    bf_config c{};
    if (cfg && cfg->struct_size) memcpy(&c, cfg, std::min<size_t>(cfg->struct_size, sizeof c));
    else c.device = -1;
    if (c.struct_size < 8) c.device = -1;
    if (c.shard_count > 1 || c.shard_index != 0)
        return bank_err(nullptr, BF_EINVAL, "a bank is not sharded (shard_count / shard_index)");
    if (c.device_count != 0) return bank_err(nullptr, BF_EINVAL, "a bank lives on one device (device_count)");
    if (c.flags != 0) return bank_err(nullptr, BF_EINVAL, "a bank takes no flags (hash engines and encoder handles are single filters), got %u", c.flags);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bank_err(nullptr, BF_EDEVICE, "no HIP device available");
    int dev = c.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return bank_err(nullptr, BF_EINVAL, "device %d out of range (%d devices)", dev, ndev);
    bf_bank* b = new (std::nothrow) bf_bank();
    if (!b) return bank_err(nullptr, BF_ENOMEM, "host allocation failed");
    b->device = dev;
    b->m = m_bits;
    b->k = k;
    b->n_filters = n_filters;
    b->stride = stride;
    b->bytes = bytes;
    const uint64_t maxval = (uint64_t)k * 0xFFFFFFFFull;   // ruby.rb:51 reaches k (2^32 - 1) at most
    b->reach = std::min<uint64_t>(m_bits, maxval + 1);
    b->batch_keys = c.batch_keys ? c.batch_keys : (1ull << 22);
    b->batch_bytes = c.batch_bytes ? c.batch_bytes : (64ull << 20);
    DeviceGuard dg(dev);
    auto fail = [&](int code, const char* what, hipError_t e) {
        bank_err(nullptr, code, "%s failed: %s", what, hipGetErrorString(e));
        if (b->stream) (void)hipStreamDestroy(b->stream);
        if (b->order_ev) (void)hipEventDestroy(b->order_ev);
        if (b->h_status) (void)hipHostFree(b->h_status);
        if (b->g.bits) (void)hipFree(b->g.bits);
        delete b;
        return code;
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess) return fail(BF_EDEVICE, "hipStreamCreate", e);
    if ((e = hipEventCreateWithFlags(&b->order_ev, hipEventDisableTiming)) != hipSuccess) return fail(BF_EDEVICE, "hipEventCreate", e);
    if ((e = hipHostMalloc((void**)&b->h_status, 64, hipHostMallocDefault)) != hipSuccess) return fail(BF_ENOMEM, "hipHostMalloc", e);
    b->h_status[0] = b->h_status[1] = 0u;
    if ((e = hipHostGetDevicePointer((void**)&b->d_status, b->h_status, 0)) != hipSuccess) return fail(BF_EDEVICE, "hipHostGetDevicePointer", e);
    if ((e = hipMalloc((void**)&b->g.bits, bytes)) != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? BF_ENOMEM : BF_EDEVICE, "hipMalloc(bank)", e);
    if ((e = hipMemsetAsync(b->g.bits, 0, bytes, b->stream)) != hipSuccess) return fail(BF_EDEVICE, "hipMemset", e);
    if ((e = hipStreamSynchronize(b->stream)) != hipSuccess) return fail(BF_EDEVICE, "hipStreamSynchronize", e);
    b->g.m = m_bits;
    b->g.inv_m = 1.0 / (double)m_bits;
    b->g.k = k;
    b->g.nomod = m_bits > maxval ? 1u : 0u;
    b->g.mod_f32 = m_bits >= (1ull << 17) ? 1u : 0u;
    b->g.inv_m_f = (float)(1.0 / (double)m_bits);
    b->g.mod_sub = bf_mod_sub(m_bits, maxval);
    b->g.shards = 1;
    b->g.inv_shards = 1.0;
    b->g.shards_pow2 = 1;
    b->g.block_log2 = 20;
    b->g.limit = m_bits;
    b->g.key_status = b->d_status;
    *out = b;
    return BF_OK;
}

int bf_bank_destroy(bf_bank* b) {
    if (!b) return BF_OK;
    {
        std::lock_guard<std::mutex> lk(b->mu);
        DeviceGuard dg(b->device);
        (void)hipStreamSynchronize(b->stream);
        if (b->order_valid) (void)hipEventSynchronize(b->order_ev);
        for (void* p : {(void*)b->g.bits, (void*)b->d_keys, (void*)b->d_out, (void*)b->d_off, (void*)b->d_ids,
                        (void*)b->d_io, (void*)b->d_list, (void*)b->d_seq, (void*)b->d_chg})
            if (p) (void)hipFree(p);
        if (b->order_ev) (void)hipEventDestroy(b->order_ev);
        if (b->h_status) (void)hipHostFree(b->h_status);
        (void)hipStreamDestroy(b->stream);
    }
    delete b;
    return BF_OK;
}

const char* bf_bank_last_error(const bf_bank* b) { return b ? b->err.c_str() : g_bank_create_error.c_str(); }

int bf_bank_info(const bf_bank* b, uint64_t* m_bits, uint32_t* k, uint64_t* n_filters, uint64_t* stride,
                 uint64_t* device_bytes) {
    if (!b) return BF_EINVAL;
    if (m_bits) *m_bits = b->m;
    if (k) *k = b->k;
    if (n_filters) *n_filters = b->n_filters;
    if (stride) *stride = b->stride;
    if (device_bytes) *device_bytes = b->bytes;
    return BF_OK;
}

int bf_bank_stream(bf_bank* b, void** stream) {
    if (!b || !stream) return BF_EINVAL;
    *stream = reinterpret_cast<void*>(b->stream);
    return BF_OK;
}

int bf_bank_sync(bf_bank* b) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (int drc = cs.device()) return drc;
    HIPCHK(b, hipStreamSynchronize(b->stream));
    if (b->order_valid) HIPCHK(b, hipEventSynchronize(b->order_ev));   // a _dev call's stream
    const uint32_t bad_key = __atomic_exchange_n(&b->h_status[0], 0u, __ATOMIC_ACQ_REL);
    const uint32_t bad_id = __atomic_exchange_n(&b->h_status[1], 0u, __ATOMIC_ACQ_REL);
    if (bad_key || bad_id)
        return bank_err(b, BF_EINVAL, "an earlier device call met %s%s%s: those keys were skipped (no bit set, answer 0), "
                                      "those filters left alone",
                        bad_id ? "a filter id at or past n_filters" : "", bad_id && bad_key ? " and " : "",
                        bad_key ? "inconsistent key offsets (offsets must be non-decreasing and every key below 2 GiB)" : "");
    return BF_OK;
}

int bf_bank_insert_many(bf_bank* b, const uint8_t* key_bytes, const uint64_t* offsets, const uint32_t* filter_ids,
                        uint64_t n, uint8_t* key_flipped) {
    return run_host(b, BANK_INSERT, key_bytes, offsets, filter_ids, n, key_flipped);
}

int bf_bank_include_many(bf_bank* b, const uint8_t* key_bytes, const uint64_t* offsets, const uint32_t* filter_ids,
                         uint64_t n, uint8_t* out) {
    return run_host(b, BANK_INCLUDE, key_bytes, offsets, filter_ids, n, out);
}

int bf_bank_insert_many_dev(bf_bank* b, const uint8_t* d_key_bytes, const uint64_t* d_offsets,
                            const uint32_t* d_filter_ids, uint64_t n, uint8_t* d_key_flipped, void* stream) {
    return run_dev(b, BANK_INSERT, d_key_bytes, d_offsets, d_filter_ids, n, d_key_flipped, stream);
}

int bf_bank_include_many_dev(bf_bank* b, const uint8_t* d_key_bytes, const uint64_t* d_offsets,
                             const uint32_t* d_filter_ids, uint64_t n, uint8_t* d_out, void* stream) {
    return run_dev(b, BANK_INCLUDE, d_key_bytes, d_offsets, d_filter_ids, n, d_out, stream);
}

int bf_bank_set_seq_form(bf_bank* b, uint32_t form) {
    if (!b) return BF_EINVAL;
    std::lock_guard<std::mutex> lk(b->mu);
    if (form != BF_BANK_SEQ_AUTO && form != BF_BANK_SEQ_HASH && form != BF_BANK_SEQ_DIRECT)
        return bank_err(b, BF_EINVAL, "unknown form %u", form);
    b->seq_form = form;
    return BF_OK;
}

int bf_bank_seq_plan(const bf_bank* b, uint64_t n, uint32_t* direct, uint64_t* chunk_keys, uint64_t* scratch_bytes) {
    if (!b) return BF_EINVAL;
    const BankSeqPlan plan = seq_plan(b, n, UINT64_MAX);
    if (direct) *direct = plan.direct ? 1u : 0u;
    if (chunk_keys) *chunk_keys = plan.chunk;
    if (scratch_bytes) *scratch_bytes = plan.scratch;
    return BF_OK;
}

int bf_bank_insert_many_seq(bf_bank* b, const uint8_t* key_bytes, const uint64_t* offsets, const uint32_t* filter_ids,
                            uint64_t n, uint8_t* per_key_new) {
    if (!b) return BF_EINVAL;
    if (n == 0) return BF_OK;
    CallScope cs(b);
    int rc = check_batch(b, key_bytes, offsets, filter_ids, n);
    if (rc) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    const BankSeqPlan plan = seq_plan(b, n, b->batch_keys);
    if ((rc = ensure_seq_scratch(b, plan.scratch))) return rc;
    std::vector<uint64_t> h_off;   // stage_chunk's, read by its copy until the synchronise
    for (uint64_t a = 0, e; a < n; a = e) {
        e = chunk_end(b, offsets, n, a, plan.chunk);
        if ((rc = stage_chunk(b, key_bytes, offsets, filter_ids, a, e, h_off))) return rc;
        if ((rc = launch_seq_chunk(b, plan.direct, b->d_keys, b->d_off, b->d_ids, e - a, per_key_new ? b->d_out : nullptr,
                                   b->stream)))
            return rc;
        if (per_key_new) HIPCHK(b, hipMemcpyAsync(per_key_new + a, b->d_out, e - a, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(b, hipStreamSynchronize(b->stream));   // the staging buffers are free again
    }
    return BF_OK;
}

int bf_bank_insert_many_seq_dev(bf_bank* b, const uint8_t* d_key_bytes, const uint64_t* d_offsets,
                                const uint32_t* d_filter_ids, uint64_t n, uint8_t* d_per_key_new, void* stream) {
    if (!b) return BF_EINVAL;
    if (n == 0) return BF_OK;
    CallScope cs(b);
    if (!d_key_bytes || !d_offsets || !d_filter_ids) return bank_err(b, BF_EINVAL, "NULL device pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return seq_dev_chunks(b, d_key_bytes, d_offsets, d_filter_ids, n, d_per_key_new, s, nullptr);
}

int bf_bank_insert_many_changes(bf_bank* b, const uint8_t* key_bytes, const uint64_t* offsets,
                                const uint32_t* filter_ids, uint64_t n, uint32_t seq, uint8_t* flags,
                                uint32_t* out_ids, uint64_t* out_bits, uint64_t cap, uint64_t* count) {
    if (!b || !count) return BF_EINVAL;
    CallScope cs(b);
    if (seq > 1) return bank_err(b, BF_EINVAL, "seq must be 0 or 1, got %u", seq);
    if (cap && (!out_ids || !out_bits)) return bank_err(b, BF_EINVAL, "cap > 0 with a NULL out_ids / out_bits");
    if (n == 0) {
        *count = 0;
        return BF_OK;
    }
    int rc = check_batch(b, key_bytes, offsets, filter_ids, n);
    if (rc) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    // seq: bf_bank_insert_many_seq's form, chunk bound and scratch; else chunks of batch_keys keys
    BankSeqPlan plan{false, b->batch_keys, 0};
    if (seq) {
        plan = seq_plan(b, n, b->batch_keys);
        if ((rc = ensure_seq_scratch(b, plan.scratch))) return rc;
    }
    std::vector<uint8_t> back;
    uint64_t total = 0, written = 0;
    std::vector<uint64_t> h_off;   // stage_chunk's, read by its copy until the synchronise
    for (uint64_t a = 0, e; a < n; a = e) {
        e = chunk_end(b, offsets, n, a, plan.chunk);
        const uint64_t cn = e - a;
        // the chunk lists into the bank's scratch: what the caller's arrays still hold, at most a
        // probe per entry
        uint64_t entries = cap - written;
        if (entries / b->k >= cn) entries = cn * b->k;
        if (entries > (UINT64_MAX - 8) / 12) return bank_err(b, BF_ENOMEM, "a list of %llu entries", (unsigned long long)entries);
        if ((rc = stage_chunk(b, key_bytes, offsets, filter_ids, a, e, h_off))) return rc;
        if ((rc = grow(b, (void**)&b->d_chg, &b->chg_cap, chg_bytes(entries)))) return rc;
        unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(b->d_chg);
        uint64_t* d_bits = reinterpret_cast<uint64_t*>(b->d_chg + 8);
        uint32_t* d_lids = reinterpret_cast<uint32_t*>(b->d_chg + 8 + entries * 8);
        const BankList<true> list{d_lids, d_bits, entries, d_cnt};
        HIPCHK(b, hipMemsetAsync(d_cnt, 0, 8, b->stream));
        uint8_t* d_flags = flags ? b->d_out : nullptr;
        if (seq) rc = launch_seq_chunk(b, plan.direct, b->d_keys, b->d_off, b->d_ids, cn, d_flags, b->stream, &list);
        else rc = launch_keys(b, BANK_INSERT, b->d_keys, b->d_off, b->d_ids, cn, d_flags, b->stream, &list);
        if (rc) return rc;
        if (flags) HIPCHK(b, hipMemcpyAsync(flags + a, b->d_out, cn, hipMemcpyDeviceToHost, b->stream));
        unsigned long long flipped = 0;
        const bool one_copy = chg_bytes(entries) <= kChgOneCopy;
        if (one_copy) {
            back.resize(chg_bytes(entries));
            HIPCHK(b, hipMemcpyAsync(back.data(), b->d_chg, back.size(), hipMemcpyDeviceToHost, b->stream));
        } else {
            HIPCHK(b, hipMemcpyAsync(&flipped, d_cnt, 8, hipMemcpyDeviceToHost, b->stream));
        }
        HIPCHK(b, hipStreamSynchronize(b->stream));   // the staging buffers are free again
        if (one_copy) memcpy(&flipped, back.data(), 8);
        const uint64_t got = std::min<uint64_t>(flipped, entries);   // this chunk's entries behind the earlier ones
        if (got && one_copy) {
            memcpy(out_bits + written, back.data() + 8, got * 8);
            memcpy(out_ids + written, back.data() + 8 + entries * 8, got * 4);
        } else if (got) {
            HIPCHK(b, hipMemcpyAsync(out_bits + written, d_bits, got * 8, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(b, hipMemcpyAsync(out_ids + written, d_lids, got * 4, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(b, hipStreamSynchronize(b->stream));
        }
        written += got;
        total += flipped;
    }
    *count = total;
    if (total > cap)
        return bank_err(b, BF_ERANGE, "the batch flipped %llu bits, the lists hold %llu (the insert is applied, the first "
                                      "%llu entries are valid)",
                        (unsigned long long)total, (unsigned long long)cap, (unsigned long long)cap);
    return BF_OK;
}

int bf_bank_insert_many_changes_dev(bf_bank* b, const uint8_t* d_key_bytes, const uint64_t* d_offsets,
                                    const uint32_t* d_filter_ids, uint64_t n, uint32_t seq, uint8_t* d_flags,
                                    uint32_t* d_out_ids, uint64_t* d_out_bits, uint64_t cap, uint64_t* d_count,
                                    void* stream) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (seq > 1) return bank_err(b, BF_EINVAL, "seq must be 0 or 1, got %u", seq);
    if (!d_count || (cap && (!d_out_ids || !d_out_bits)) || (n && (!d_key_bytes || !d_offsets || !d_filter_ids)))
        return bank_err(b, BF_EINVAL, "NULL device pointer");
    if (int arc = check_aligned(b, addr(d_out_bits) | addr(d_count), addr(d_out_ids),
                                "d_out_bits and d_count: 8 bytes, d_out_ids: 4"))
        return arc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    HIPCHK(b, hipMemsetAsync(d_count, 0, 8, s));   // the kernels of every chunk add to it
    if (n == 0) return BF_OK;
    const BankList<true> list{d_out_ids, d_out_bits, cap, reinterpret_cast<unsigned long long*>(d_count)};
    if (seq) return seq_dev_chunks(b, d_key_bytes, d_offsets, d_filter_ids, n, d_flags, s, &list);
    return launch_keys(b, BANK_INSERT, d_key_bytes, d_offsets, d_filter_ids, n, d_flags, s, &list);
}

int bf_bank_across_row_bytes(uint64_t count, uint64_t* bytes) {
    if (!bytes) return BF_EINVAL;
    *bytes = across_row_bytes(count);
    return BF_OK;
}

int bf_bank_include_across(bf_bank* b, const uint8_t* key_bytes, const uint64_t* offsets, uint64_t n,
                           const uint32_t* ids, uint64_t count, uint8_t* mask) {
    if (!b) return BF_EINVAL;
    if (n == 0 || count == 0) return BF_OK;
    CallScope cs(b);
    if (!mask) return bank_err(b, BF_EINVAL, "mask is NULL");
    if (!offsets || (!key_bytes && offsets[n] != offsets[0])) return bank_err(b, BF_EINVAL, "NULL keys / offsets");
    int rc = check_keys(b, offsets, nullptr, n);
    if (rc) return rc;
    if ((rc = check_list(b, ids, count, true))) return rc;
    const uint64_t row = across_row_bytes(count);
    uint64_t total = 0;
    if (__builtin_mul_overflow(n, row, &total))
        return bank_err(b, BF_EINVAL, "%llu mask rows of %llu bytes overflow a 64-bit byte size", (unsigned long long)n,
                        (unsigned long long)row);
    if (int orc = cs.open(b->stream)) return orc;
    const uint32_t* d_ids = nullptr;
    if ((rc = stage_list(b, ids, count, &d_ids))) return rc;
    // chunks of batch_keys keys, bounded again so that the staged mask stays under kAcrossMaskCap
    const uint64_t max_keys = std::min<uint64_t>(b->batch_keys, std::max<uint64_t>(1, kAcrossMaskCap / row));
    std::vector<uint64_t> h_off;   // stage_chunk's, read by its copy until the synchronise
    for (uint64_t a = 0, e; a < n; a = e) {
        e = chunk_end(b, offsets, n, a, max_keys);
        if ((rc = stage_chunk(b, key_bytes, offsets, nullptr, a, e, h_off))) return rc;
        if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, (e - a) * row))) return rc;
        if ((rc = launch_across(b, b->d_keys, b->d_off, e - a, d_ids, count, b->d_io, b->stream))) return rc;
        HIPCHK(b, hipMemcpyAsync(mask + a * row, b->d_io, (e - a) * row, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(b, hipStreamSynchronize(b->stream));   // the staging buffers and `ids` are free again
    }
    return BF_OK;
}

int bf_bank_include_across_dev(bf_bank* b, const uint8_t* d_key_bytes, const uint64_t* d_offsets, uint64_t n,
                               const uint32_t* d_ids, uint64_t count, uint8_t* d_mask, void* stream) {
    if (!b) return BF_EINVAL;
    if (n == 0 || count == 0) return BF_OK;
    CallScope cs(b);
    if (!d_key_bytes || !d_offsets || !d_mask) return bank_err(b, BF_EINVAL, "NULL device pointer");
    int rc = check_aligned(b, addr(d_offsets) | addr(d_mask), addr(d_ids), "d_offsets and d_mask: 8 bytes, d_ids: 4");
    if (rc) return rc;
    if ((rc = check_list(b, d_ids, count, false))) return rc;
    uint64_t total = 0;
    if (__builtin_mul_overflow(n, across_row_bytes(count), &total))
        return bank_err(b, BF_EINVAL, "%llu mask rows of %llu bytes overflow a 64-bit byte size", (unsigned long long)n,
                        (unsigned long long)across_row_bytes(count));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_across(b, d_key_bytes, d_offsets, n, d_ids, count, d_mask, s);
}

int bf_bank_clear_dev(bf_bank* b, const uint32_t* d_ids, uint64_t count, void* stream) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_clear(b, d_ids, count, s);
}

int bf_bank_clear(bf_bank* b, const uint32_t* ids, uint64_t count) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    int rc = ids ? check_list(b, ids, count, true) : BF_OK;
    if (rc) return rc;
    if (ids && count == 0) return BF_OK;
    if (int orc = cs.open(b->stream)) return orc;
    const uint32_t* d_ids = nullptr;
    if ((rc = stage_list(b, ids, count, &d_ids))) return rc;
    if ((rc = launch_clear(b, d_ids, count, b->stream))) return rc;
    HIPCHK(b, hipStreamSynchronize(b->stream));   // `ids` is the caller's again
    return BF_OK;
}

int bf_bank_bitcount_dev(bf_bank* b, const uint32_t* d_ids, uint64_t count, uint64_t* d_out, void* stream) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    int rc = check_list(b, d_ids, count, false);
    if (rc) return rc;
    if (count == 0) return BF_OK;
    if (!d_out) return bank_err(b, BF_EINVAL, "d_out is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_bitcount(b, d_ids, count, d_out, s);
}

int bf_bank_bitcount(bf_bank* b, const uint32_t* ids, uint64_t count, uint64_t* out) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    int rc = check_list(b, ids, count, true);
    if (rc) return rc;
    if (count == 0) return BF_OK;
    if (!out) return bank_err(b, BF_EINVAL, "out is NULL");
    if (int orc = cs.open(b->stream)) return orc;
    const uint32_t* d_ids = nullptr;
    if ((rc = stage_list(b, ids, count, &d_ids))) return rc;
    if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, count * 8))) return rc;
    if ((rc = launch_bitcount(b, d_ids, count, reinterpret_cast<uint64_t*>(b->d_io), b->stream))) return rc;
    HIPCHK(b, hipMemcpyAsync(out, b->d_io, count * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(b, hipStreamSynchronize(b->stream));
    return BF_OK;
}

int bf_bank_export_filters(bf_bank* b, const uint32_t* ids, uint64_t count, uint8_t* buf, uint64_t* lens) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    int rc = check_list(b, ids, count, true);
    if (rc) return rc;
    if (count == 0) return BF_OK;
    if (!buf || !lens) return bank_err(b, BF_EINVAL, "buf / lens is NULL");
    uint64_t data = 0, total = 0;
    if ((rc = io_bytes(b, count, &data, &total))) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    const uint32_t* d_ids = nullptr;
    if ((rc = stage_list(b, ids, count, &d_ids))) return rc;
    if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, total))) return rc;
    hipLaunchKernelGGL(bank_gather_kernel, dim3(owned_grid(b->stride, count)), dim3(kBankLanes), 0, b->stream,
                       reinterpret_cast<const uint4*>(b->g.bits), b->stride / 16, b->n_filters, d_ids, count,
                       reinterpret_cast<uint4*>(b->d_io), reinterpret_cast<unsigned long long*>(b->d_io + data),
                       b->d_status);
    HIPCHK(b, hipGetLastError());
    HIPCHK(b, hipMemcpyAsync(buf, b->d_io, data, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(b, hipMemcpyAsync(lens, b->d_io + data, count * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(b, hipStreamSynchronize(b->stream));
    return BF_OK;
}

int bf_bank_import_filters(bf_bank* b, const uint32_t* ids, uint64_t count, const uint8_t* buf, const uint64_t* lens,
                           uint32_t mode) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (mode != BF_IMPORT_REPLACE && mode != BF_IMPORT_OR) return bank_err(b, BF_EINVAL, "bad import mode %u", mode);
    int rc = check_list(b, ids, count, true);
    if (rc) return rc;
    if (count == 0) return BF_OK;
    if (!buf || !lens) return bank_err(b, BF_EINVAL, "buf / lens is NULL");
    // bf_import_redis' refusals, for every string before anything is written
    const uint64_t max_bytes = (b->reach + 7) / 8;
    for (uint64_t i = 0; i < count; ++i) {
        if (lens[i] > max_bytes)
            return bank_err(b, BF_ERANGE, "string %llu of %llu bytes exceeds the filter's %llu reachable bytes",
                            (unsigned long long)i, (unsigned long long)lens[i], (unsigned long long)max_bytes);
        if (lens[i] == max_bytes && (b->reach & 7) && (buf[i * b->stride + lens[i] - 1] & (uint8_t)(0xFFu >> (b->reach & 7))))
            return bank_err(b, BF_ERANGE, "string %llu sets bits at offsets >= %llu", (unsigned long long)i,
                            (unsigned long long)b->reach);
    }
    uint64_t data = 0, total = 0;
    if ((rc = io_bytes(b, count, &data, &total))) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    const uint32_t* d_ids = nullptr;
    if ((rc = stage_list(b, ids, count, &d_ids))) return rc;
    if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, total))) return rc;
    HIPCHK(b, hipMemcpyAsync(b->d_io, buf, data, hipMemcpyHostToDevice, b->stream));
    HIPCHK(b, hipMemcpyAsync(b->d_io + data, lens, count * 8, hipMemcpyHostToDevice, b->stream));
    const dim3 grid(owned_grid(b->stride, count)), block(kBankLanes);
    uint4* bits = reinterpret_cast<uint4*>(b->g.bits);
    const uint4* src = reinterpret_cast<const uint4*>(b->d_io);
    const unsigned long long* d_lens = reinterpret_cast<const unsigned long long*>(b->d_io + data);
    if (mode == BF_IMPORT_OR)
        hipLaunchKernelGGL(bank_scatter_kernel<true>, grid, block, 0, b->stream, bits, b->stride / 16, b->n_filters, d_ids,
                           count, src, d_lens, b->d_status);
    else
        hipLaunchKernelGGL(bank_scatter_kernel<false>, grid, block, 0, b->stream, bits, b->stride / 16, b->n_filters, d_ids,
                           count, src, d_lens, b->d_status);
    HIPCHK(b, hipGetLastError());
    HIPCHK(b, hipStreamSynchronize(b->stream));
    return BF_OK;
}

int bf_bank_fold(bf_bank* b, uint32_t op, const uint32_t* dst_ids, const uint64_t* seg, const uint32_t* src_ids,
                 uint64_t groups, uint8_t* changed, uint64_t* set_bits) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (!seg || !src_ids) return bank_err(b, BF_EINVAL, "seg / src_ids is NULL");
    int rc = check_fold_op(b, op, dst_ids != nullptr);
    if (rc) return rc;
    if (seg[0] != 0) return bank_err(b, BF_EINVAL, "seg[0] must be 0, got %llu", (unsigned long long)seg[0]);
    for (uint64_t g = 0; g < groups; ++g) {
        if (seg[g + 1] < seg[g])
            return bank_err(b, BF_EINVAL, "group %llu: seg must be non-decreasing (seg[%llu] = %llu after %llu)",
                            (unsigned long long)g, (unsigned long long)(g + 1), (unsigned long long)seg[g + 1],
                            (unsigned long long)seg[g]);
        if (seg[g + 1] == seg[g])
            return bank_err(b, BF_EINVAL, "group %llu is empty (the AND of nothing is not a filter)", (unsigned long long)g);
    }
    if (groups == 0) return BF_OK;
    const uint64_t n_src = seg[groups];
    if ((rc = check_ids(b, "src_ids", src_ids, n_src))) return rc;
    if (dst_ids) {
        if ((rc = check_ids(b, "dst_ids", dst_ids, groups))) return rc;
        // a destination is written by one group and read by no other: sorted (id, group) pairs
        std::vector<std::pair<uint32_t, uint64_t>> owner(groups);
        for (uint64_t g = 0; g < groups; ++g) owner[g] = {dst_ids[g], g};
        std::sort(owner.begin(), owner.end());
        uint64_t twice = UINT64_MAX;   // the first group (in list order) whose destination an earlier group has
        for (uint64_t i = 1; i < groups; ++i)
            if (owner[i].first == owner[i - 1].first) twice = std::min(twice, owner[i].second);
        if (twice != UINT64_MAX) {
            uint64_t other = 0;
            while (dst_ids[other] != dst_ids[twice]) ++other;
            return bank_err(b, BF_EINVAL, "dst_ids[%llu] = %u is also the destination of group %llu", (unsigned long long)twice,
                            dst_ids[twice], (unsigned long long)other);
        }
        for (uint64_t g = 0; g < groups; ++g)
            for (uint64_t i = seg[g]; i < seg[g + 1]; ++i) {
                auto it = std::lower_bound(owner.begin(), owner.end(), std::make_pair(src_ids[i], (uint64_t)0));
                if (it != owner.end() && it->first == src_ids[i] && it->second != g)
                    return bank_err(b, BF_EINVAL, "group %llu reads filter %u (src_ids[%llu]), the destination of group %llu: "
                                                  "the result would depend on the order of the groups",
                                    (unsigned long long)g, src_ids[i], (unsigned long long)i, (unsigned long long)it->second);
            }
    }
    // staged as [seg | set_bits | src_ids | dst_ids | changed]: the 8-byte fields first
    uint64_t total = 0;
    if (groups > (1ull << 56) || n_src > (1ull << 56)) return bank_err(b, BF_EINVAL, "too many groups or sources");
    const uint64_t off_sb = (groups + 1) * 8, off_src = off_sb + groups * 8, off_dst = off_src + n_src * 4;
    const uint64_t off_chg = off_dst + groups * 4;
    total = off_chg + groups;
    if (int orc = cs.open(b->stream)) return orc;
    if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, total))) return rc;
    uint8_t* io = b->d_io;
    HIPCHK(b, hipMemcpyAsync(io, seg, (groups + 1) * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(b, hipMemcpyAsync(io + off_src, src_ids, n_src * 4, hipMemcpyHostToDevice, b->stream));
    if (dst_ids) HIPCHK(b, hipMemcpyAsync(io + off_dst, dst_ids, groups * 4, hipMemcpyHostToDevice, b->stream));
    if ((rc = launch_fold(b, op, dst_ids ? reinterpret_cast<const uint32_t*>(io + off_dst) : nullptr,
                          reinterpret_cast<const uint64_t*>(io), reinterpret_cast<const uint32_t*>(io + off_src), groups,
                          n_src, changed ? io + off_chg : nullptr,
                          set_bits ? reinterpret_cast<uint64_t*>(io + off_sb) : nullptr, b->stream)))
        return rc;
    if (set_bits) HIPCHK(b, hipMemcpyAsync(set_bits, io + off_sb, groups * 8, hipMemcpyDeviceToHost, b->stream));
    if (changed) HIPCHK(b, hipMemcpyAsync(changed, io + off_chg, groups, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(b, hipStreamSynchronize(b->stream));   // the lists are the caller's again
    return BF_OK;
}

int bf_bank_fold_dev(bf_bank* b, uint32_t op, const uint32_t* d_dst_ids, const uint64_t* d_seg, const uint32_t* d_src_ids,
                     uint64_t groups, uint64_t n_src, uint8_t* d_changed, uint64_t* d_set_bits, void* stream) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    int rc = check_fold_op(b, op, d_dst_ids != nullptr);
    if (rc) return rc;
    if (groups == 0) return BF_OK;
    if (!d_seg || !d_src_ids) return bank_err(b, BF_EINVAL, "NULL device pointer (d_seg / d_src_ids)");
    if ((rc = check_aligned(b, addr(d_seg) | addr(d_set_bits), addr(d_src_ids) | addr(d_dst_ids),
                            "d_seg and d_set_bits: 8 bytes, d_src_ids and d_dst_ids: 4")))
        return rc;
    if (groups > (1ull << 56)) return bank_err(b, BF_EINVAL, "too many groups");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_fold(b, op, d_dst_ids, d_seg, d_src_ids, groups, n_src, d_changed, d_set_bits, s);
}

int bf_bank_overlap(bf_bank* b, const uint32_t* row_ids, uint64_t rows, const uint32_t* col_ids, uint64_t cols,
                    uint64_t* out) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (rows == 0 || cols == 0) return BF_OK;
    uint64_t out_bytes = 0;
    int rc = check_overlap(b, row_ids, rows, col_ids, cols, &out_bytes);
    if (rc) return rc;
    if (!out) return bank_err(b, BF_EINVAL, "out is NULL");
    if (row_ids && (rc = check_ids(b, "row_ids", row_ids, rows))) return rc;
    if (col_ids && (rc = check_ids(b, "col_ids", col_ids, cols))) return rc;
    if (int orc = cs.open(b->stream)) return orc;
    // both lists side by side in d_list; without col_ids the columns are the row list
    const uint64_t n_row = row_ids ? rows : 0, n_col = col_ids ? cols : 0;
    const uint32_t *d_rows = nullptr, *d_cols = nullptr;
    if (n_row + n_col) {
        if ((rc = grow(b, (void**)&b->d_list, &b->list_cap, (n_row + n_col) * 4))) return rc;
        if (n_row) HIPCHK(b, hipMemcpyAsync(b->d_list, row_ids, n_row * 4, hipMemcpyHostToDevice, b->stream));
        if (n_col) HIPCHK(b, hipMemcpyAsync(b->d_list + n_row, col_ids, n_col * 4, hipMemcpyHostToDevice, b->stream));
        d_rows = n_row ? b->d_list : nullptr;
        d_cols = n_col ? b->d_list + n_row : d_rows;
    }
    // runs of rows whose counts stay under kOverlapOutCap; one run is the whole (then maybe symmetric) matrix
    const uint64_t max_rows = std::max<uint64_t>(1, kOverlapOutCap / (cols * 8));
    for (uint64_t a = 0; a < rows; a += max_rows) {
        const uint64_t cn = std::min<uint64_t>(max_rows, rows - a);
        if ((rc = grow(b, (void**)&b->d_io, &b->io_cap, cn * cols * 8))) return rc;
        if ((rc = launch_overlap(b, d_rows ? d_rows + a : nullptr, a, cn, d_cols, cols, !col_ids && cn == rows,
                                 reinterpret_cast<uint64_t*>(b->d_io), b->stream)))
            return rc;
        HIPCHK(b, hipMemcpyAsync(out + a * cols, b->d_io, cn * cols * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(b, hipStreamSynchronize(b->stream));   // d_io is free again
    }
    return BF_OK;
}

int bf_bank_overlap_dev(bf_bank* b, const uint32_t* d_row_ids, uint64_t rows, const uint32_t* d_col_ids, uint64_t cols,
                        uint64_t* d_out, void* stream) {
    if (!b) return BF_EINVAL;
    CallScope cs(b);
    if (rows == 0 || cols == 0) return BF_OK;
    uint64_t out_bytes = 0;
    int rc = check_overlap(b, d_row_ids, rows, d_col_ids, cols, &out_bytes);
    if (rc) return rc;
    if (!d_out) return bank_err(b, BF_EINVAL, "NULL device pointer (d_out)");
    if ((rc = check_aligned(b, addr(d_out), addr(d_row_ids) | addr(d_col_ids), "d_out: 8 bytes, d_row_ids and d_col_ids: 4")))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int orc = cs.open(s)) return orc;
    return launch_overlap(b, d_row_ids, 0, rows, d_col_ids ? d_col_ids : d_row_ids, cols, !d_col_ids, d_out, s);
}

}  // extern "C"
