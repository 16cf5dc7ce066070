// scan_device.h — an exclusive scan of 32-bit counts in global memory, in three launches: the keep flags of a dataset update
// (update.hip), the segment sizes and change flags of an index delete, the in-use and row flags of an index compaction
// (index_update.hip).
#pragma once

#include "common.h"

namespace ah {

constexpr unsigned kScanBlock = 256;                         // 4 waves
constexpr uint32_t kScanPer = 16;                            // elements per thread of the scan
constexpr uint32_t kScanTile = kScanBlock * kScanPer;        // elements per block of the scan

// inclusive sum over the 64 lanes of a wave
static __device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(x, off, 64);
        if (lane >= off) x += t;
    }
    return x;
}

// exclusive scan of n 32-bit counts in place, tile by tile (kScanTile elements a block) ...
static __global__ __launch_bounds__(kScanBlock) void k_scan_tiles(uint32_t *__restrict__ v, uint64_t n, uint32_t *__restrict__ tile_sums) {
    __shared__ uint32_t wave_sums[kScanBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint32_t x[kScanPer];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; k++) {
        x[k] = base + k < n ? v[base + k] : 0u;
        sum += x[k];
    }
    const uint32_t incl = wave_inclusive_sum(sum);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t w = 0; w < wave; w++) run += wave_sums[w];
    if (threadIdx.x == kScanBlock - 1) tile_sums[blockIdx.x] = run + sum;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; k++) {
        if (base + k < n) v[base + k] = run;
        run += x[k];
    }
}
// ... the tiles' sums scanned by one block (their exclusive prefix in place, the grand total into *total) ...
static __global__ __launch_bounds__(1024) void k_scan_sums(uint32_t *__restrict__ sums, uint64_t nb, uint32_t *__restrict__ total) {
    __shared__ uint32_t wave_sums[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < nb; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        const uint32_t x = i < nb ? sums[i] : 0u;
        const uint32_t incl = wave_inclusive_sum(x);
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 63u) wave_sums[wave] = incl;
        __syncthreads();
        uint32_t off = carry;
        for (uint32_t w = 0; w < wave; w++) off += wave_sums[w];
        if (i < nb) sums[i] = off + incl - x;
        __syncthreads();  // (every thread has read `carry` and `wave_sums`)
        if (threadIdx.x == 1023) carry = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
// ... and added back to every element of its tile
static __global__ __launch_bounds__(kScanBlock) void k_scan_add(uint32_t *__restrict__ v, uint64_t n, const uint32_t *__restrict__ tile_sums) {
    const uint32_t add = tile_sums[blockIdx.x];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
    for (uint32_t k = threadIdx.x; k < kScanTile; k += kScanBlock)
        if (base + k < n) v[base + k] += add;
}

// v[0, n) -> its exclusive prefix sums in place, the grand total into *total (written for n = 0 too); tile_sums: scratch of
// ceil(n / kScanTile) words.  Queued on `s`.
static inline void launch_exclusive_scan(uint32_t *v, uint64_t n, uint32_t *tile_sums, uint32_t *total, hipStream_t s) {
    const uint64_t nb = (n + kScanTile - 1) / kScanTile;
    if (n) hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)nb), dim3(kScanBlock), 0, s, v, n, tile_sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, tile_sums, nb, total);
    if (n) hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(kScanBlock), 0, s, v, n, (const uint32_t *)tile_sums);
}

}  // namespace ah
