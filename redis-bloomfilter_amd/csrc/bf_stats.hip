// bf_stats.hip — whole-bitset statistics and filter-to-filter combines (include/bfhip.h:
// bf_bitcount, bf_bitop, bf_bitcount_op).  The device bitset is the Redis string SETBIT builds
// (ruby.rb:59), so these are Redis's BITCOUNT and BITOP AND / OR on it, without the string
// leaving the device.
//
// All three kernels are pure streams: uint4 loads, 256-lane workgroups, at most kMaxBlocks
// workgroups that stride over the rest, per-lane 64-bit counts reduced per wave (shuffles) and
// per workgroup (LDS), then ONE 64-bit atomicAdd per workgroup.
#include "bf_device.h"

using namespace bfdev;

namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kMaxBlocks = 2048;                       // 8 workgroups per CU; stride beyond
constexpr uint32_t kBlockVecs = (1u << kDirtyShiftBits) / 128;   // uint4 per dirty-tracking block: 4096
constexpr uint32_t kVecsPerLane = kBlockVecs / kLanes;      // 16
static_assert(kVecsPerLane * kLanes == kBlockVecs, "a dirty block is a whole number of workgroup passes");

// Sum of `acc` over the workgroup, added to *d_count by one lane.
__device__ __forceinline__ void block_add(unsigned long long acc, unsigned long long* d_count) {
    __shared__ unsigned long long s_part[kLanes / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kLanes / 64; ++w) t += s_part[w];
        if (t) atomicAdd(d_count, t);
    }
}

// Set bits of bytes [byte_start, byte_start + byte_len), byte_len > 0, inside the bitset.
// The first and last vectors are masked by one lane; the whole vectors between them stream.
__global__ __launch_bounds__(kLanes) void bitcount_kernel(const uint4* __restrict__ bits, uint64_t byte_start,
                                                          uint64_t byte_len, unsigned long long* __restrict__ d_count) {
    const uint64_t end = byte_start + byte_len;
    const uint64_t v0 = byte_start >> 4, v1 = (end - 1) >> 4;   // first and last vector touched
    unsigned long long acc = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t lo = (uint32_t)(byte_start - (v0 << 4));
        if (v0 == v1) {
            acc += popc4(mask_bytes(bits[v0], lo, (uint32_t)(end - (v0 << 4))));
        } else {
            acc += popc4(mask_bytes(bits[v0], lo, 16u));
            acc += popc4(mask_bytes(bits[v1], 0u, (uint32_t)(end - (v1 << 4))));
        }
    }
    const uint64_t first = v0 + 1, n = v1 > v0 ? v1 - v0 - 1 : 0;   // whole vectors
    const uint4* __restrict__ p = bits + first;
    const uint64_t stride = (uint64_t)gridDim.x * kLanes;
    uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {   // four loads in flight per lane
        const uint4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
        acc += popc4(a) + popc4(b) + popc4(c) + popc4(d);
    }
    for (; i < n; i += stride) acc += popc4(p[i]);
    block_add(acc, d_count);
}

// popcount(a OP b) over nvec vectors; nothing else is written.
template <uint32_t OP>
__global__ __launch_bounds__(kLanes) void bitcount_op_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                             uint64_t nvec, unsigned long long* __restrict__ d_count) {
    unsigned long long acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kLanes;
    uint64_t i = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const uint4 a0 = a[i], a1 = a[i + stride], a2 = a[i + 2 * stride], a3 = a[i + 3 * stride];
        const uint4 b0 = b[i], b1 = b[i + stride], b2 = b[i + 2 * stride], b3 = b[i + 3 * stride];
        acc += popc4(bitop4<OP>(a0, b0)) + popc4(bitop4<OP>(a1, b1)) + popc4(bitop4<OP>(a2, b2)) +
               popc4(bitop4<OP>(a3, b3));
    }
    for (; i < nvec; i += stride) acc += popc4(bitop4<OP>(a[i], b[i]));
    block_add(acc, d_count);
}

// dst = dst OP src over nvec vectors.  One workgroup iteration covers exactly one
// dirty-tracking block (kBlockVecs vectors, the last block may be partial): a vector is stored
// only when it changed, the result is popcounted, and the block's mark is set (never cleared)
// iff one of its vectors changed, so the map after the launch is exact.
template <uint32_t OP>
__global__ __launch_bounds__(kLanes) void bitop_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src,
                                                       uint64_t nvec, uint8_t* __restrict__ dirty,
                                                       uint32_t* __restrict__ d_changed,
                                                       unsigned long long* __restrict__ d_count) {
    const uint64_t nblk = (nvec + kBlockVecs - 1) / kBlockVecs;
    unsigned long long acc = 0;
    int any_block = 0;
    for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint64_t base = blk * kBlockVecs + threadIdx.x;
        int changed = 0;
#pragma unroll
        for (uint32_t h = 0; h < kVecsPerLane; h += 8) {   // eight vectors of each input in flight
            uint4 a[8], b[8];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) {
                const uint64_t i = base + (uint64_t)(h + u) * kLanes;
                if (i < nvec) {
                    a[u] = dst[i];
                    b[u] = src[i];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) {
                const uint64_t i = base + (uint64_t)(h + u) * kLanes;
                if (i < nvec) {
                    const uint4 r = bitop4<OP>(a[u], b[u]);
                    acc += popc4(r);
                    if ((r.x ^ a[u].x) | (r.y ^ a[u].y) | (r.z ^ a[u].z) | (r.w ^ a[u].w)) {
                        dst[i] = r;
                        changed = 1;
                    }
                }
            }
        }
        const int any = __syncthreads_or(changed);   // blk is uniform over the workgroup
        if (any && threadIdx.x == 0 && dirty) dirty[blk] = 1;
        any_block |= any;
    }
    if (any_block && threadIdx.x == 0 && d_changed) atomicOr(d_changed, 1u);
    if (d_count) block_add(acc, d_count);   // d_count is uniform
}

uint32_t stream_blocks(uint64_t nvec) {
    const uint64_t g = (nvec + kLanes - 1) / kLanes;
    return g > kMaxBlocks ? kMaxBlocks : (g ? (uint32_t)g : 1u);
}

}  // namespace

hipError_t bf_launch_bitcount(const uint32_t* bits, uint64_t byte_start, uint64_t byte_len,
                              unsigned long long* d_count, hipStream_t s) {
    if (byte_len == 0) return hipSuccess;
    hipLaunchKernelGGL(bitcount_kernel, dim3(stream_blocks((byte_len + 15) / 16)), dim3(kLanes), 0, s,
                       reinterpret_cast<const uint4*>(bits), byte_start, byte_len, d_count);
    return hipGetLastError();
}

hipError_t bf_launch_bitcount_op(uint32_t op, const uint32_t* a, const uint32_t* b, uint64_t nwords,
                                 unsigned long long* d_count, hipStream_t s) {
    const uint64_t nvec = nwords / 4;
    if (nvec == 0) return hipSuccess;
    const uint4* va = reinterpret_cast<const uint4*>(a);
    const uint4* vb = reinterpret_cast<const uint4*>(b);
    const dim3 grid(stream_blocks(nvec)), block(kLanes);
    if (op == BF_BITOP_AND) hipLaunchKernelGGL(bitcount_op_kernel<BF_BITOP_AND>, grid, block, 0, s, va, vb, nvec, d_count);
    else if (op == BF_BITOP_OR) hipLaunchKernelGGL(bitcount_op_kernel<BF_BITOP_OR>, grid, block, 0, s, va, vb, nvec, d_count);
    else if (op == BF_BITOP_XOR) hipLaunchKernelGGL(bitcount_op_kernel<BF_BITOP_XOR>, grid, block, 0, s, va, vb, nvec, d_count);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t bf_launch_bitop(uint32_t op, uint32_t* dst, const uint32_t* src, uint64_t nwords, uint8_t* dirty,
                           uint32_t* d_changed, unsigned long long* d_count, hipStream_t s) {
    const uint64_t nvec = nwords / 4;
    if (nvec == 0) return hipSuccess;
    const uint64_t nblk = (nvec + kBlockVecs - 1) / kBlockVecs;
    const dim3 grid(nblk > kMaxBlocks ? kMaxBlocks : (uint32_t)nblk), block(kLanes);
    uint4* vd = reinterpret_cast<uint4*>(dst);
    const uint4* vs = reinterpret_cast<const uint4*>(src);
    if (op == BF_BITOP_AND) hipLaunchKernelGGL(bitop_kernel<BF_BITOP_AND>, grid, block, 0, s, vd, vs, nvec, dirty, d_changed, d_count);
    else if (op == BF_BITOP_OR) hipLaunchKernelGGL(bitop_kernel<BF_BITOP_OR>, grid, block, 0, s, vd, vs, nvec, dirty, d_changed, d_count);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
