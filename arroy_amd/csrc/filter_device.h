// filter_device.h — the device side of a candidate filter that search.hip (the descents) and filter.hip (the creators) share: what a
// filter is on the device, the test of one leaf's ids against a bitmap, the per-node counts of one bitmap, and the block sum.
#pragma once

#include "index_device.h"

namespace ah {

struct FilterSlot {  // what an ah_filter holds on the device
    const uint32_t *bits;
    uint64_t len_bits;
    const uint32_t *leaf_kept;
};
// What a pass over the Descendants ids of an index under ONE bitmap reads (filled by launch_leaf_walk, filter.h).
struct LeafWalk {
    const DNode *nodes;
    const uint32_t *desc;
    const uint32_t *bits;  // over [0, len_bits)
    uint64_t len_bits;
};

// `descendants & candidates` of one leaf by one octet: the kept ids, in the leaf's order, to dst (nullptr: count only);
// returns how many.  32 ids per step (4 per lane, their bitmap words requested together); a ballot gives every lane the
// number of kept ids before its own.  Octets of a wave may be here with different leaves or not at all: a lane reads only
// its octet's byte of the ballot.
__device__ __forceinline__ uint32_t copy_filtered(const uint32_t *__restrict__ filter_bits, uint64_t filter_len_bits,
                                                  const uint32_t *__restrict__ ids, uint32_t n, uint32_t *__restrict__ dst, uint32_t j) {
    const uint32_t shift = threadIdx.x & 56u;  // first lane of the octet
    uint32_t written = 0;
    for (uint32_t base = 0; base < n; base += 32) {
        uint32_t id[4], keep[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t i = base + 8 * u + j;
            id[u] = i < n ? ids[i] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool in = base + 8 * u + j < n && id[u] < filter_len_bits;
            keep[u] = in ? (filter_bits[id[u] >> 5] >> (id[u] & 31)) & 1u : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t mask = (uint32_t)(__ballot(keep[u] != 0) >> shift) & 0xFFu;
            if (keep[u] && dst) dst[written + __popc(mask & ((1u << j) - 1u))] = id[u];
            written += __popc(mask);
        }
    }
    return written;
}

// |descendants & candidates| of every leaf, once per filtered submission (the descent then pays one load per popped leaf
// instead of a walk over its ids): one octet per node.
static __global__ __launch_bounds__(256) void k_leaf_kept(LeafWalk lw, uint32_t n_nodes, uint32_t *__restrict__ kept) {
    const uint32_t j = threadIdx.x & 7u;
    const uint32_t octets = (gridDim.x * blockDim.x) >> 3;
    for (uint32_t node = (blockIdx.x * blockDim.x + threadIdx.x) >> 3; node < n_nodes; node += octets) {
        const DNode nd = lw.nodes[node];
        uint32_t c = 0;
        if ((nd.kind & 0xFFu) == AH_NODE_DESCENDANTS) c = copy_filtered(lw.bits, lw.len_bits, lw.desc + nd.a, nd.b, nullptr, j);
        if (j == 0) kept[node] = c;
    }
}

// The sum of v over the block into *out: reduced per wave, then one 64-bit atomic per block.  Every thread of the block calls;
// s_part: a word per wave of the caller's LDS, which a kernel may pass to several calls.
__device__ __forceinline__ void block_add_u64(unsigned long long v, unsigned long long *out, unsigned long long *s_part) {
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    const uint32_t wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63u) >> 6;
    __syncthreads();  // (s_part may still be read from the call before)
    if ((threadIdx.x & 63u) == 0) s_part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < n_waves; w++) t += s_part[w];
        if (t) atomicAdd(out, t);
    }
}

}  // namespace ah
