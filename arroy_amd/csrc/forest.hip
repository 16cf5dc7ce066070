// forest.hip — whole-forest build on one GPU: `make_tree_in_file` (src/writer.rs:1167-1261) for every tree
// of the batch, level-synchronously.
//
// The reference recurses depth-first per tree under rayon (src/writer.rs:568-591,798-828); every node of
// every tree at the same depth is independent, so here ONE set of launches handles one level of ALL trees:
//
//   per level   create_split (one wave per node)  ->  margins + sides over node-major tiles (the HBM-bound
//               pass: 4*dims bytes per (item, node visit))  ->  accept / retry (<= 4 attempts,
//               src/writer.rs:1193-1216)  ->  random fallback (:1220-1227)  ->  stable partition of every
//               node's id list into its two children (ascending ids preserved, :1230-1231).
//
// Item lists live in HBM as one permutation of row indices per tree: a node owns perm[start, start+count),
// its children subdivide that range, so positions never move between nodes.  Randomness is the
// counter-based policy of include/arroy_hip_policy.h: a pure function of (tree_seed, node path, attempt,
// draw), so this breadth-first build and the depth-first CPU oracle produce the same forest bit for bit.
// No atomics on floats, no dependence on workgroup scheduling: results are deterministic.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <array>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <cstdlib>
#include <immintrin.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <new>

#include "common.h"
#include "split_device.h"
#include "screen_device.h"
#include "level_plan.h"
#include "forest_records.h"  // FNode, LevelInfo, FTile, HostRec ...: the PODs host and kernels share
#include "forest_resident.h"  // a resident forest: which record becomes which row of its device copy
#include "index_device.h"     // ForestDevice, for_spans, IndexCall::span
#include "encode.h"
#include "node_codec.h"

namespace ah {

static constexpr int kBlock = 256;
static constexpr int kMaxBlocks = 4096;

// The build's abort word (device memory, written by a DMA on the side stream when the caller's cancel flag turns
// non-zero).  Every block of the margin kernels reads it first and drains if it is set: launches that start after the
// write has landed cost nothing.  The read is an ordinary cached load on purpose — an uncached (system-scope) read of
// one word by ~100 000 blocks per launch serialises on that address and was measured to cost 70 % of the build
// (0.088 s -> 0.150 s at 1M x 768), so a kernel that is already running may keep seeing a stale line and finish.
// `gate` (the retry attempts of a level, nullptr otherwise): the number of nodes the attempt before left pending.  On most
// data a level's first attempt settles every node, and the three attempts that follow — five launches each, over every node
// and tile of the level — found nothing to do at 0.9-2.3 ms per level of the 10M x 100-tree build: with the count at zero
// their blocks leave at once.
struct AbortFlags {
    const uint32_t *dev;
    const uint32_t *gate;
};
// (read once, when a block starts: a second dependent load in front of every tile of the node-major kernels' loops cost the
// retries of a build that HAS retries 75 ms — 10M clustered rows, 741 k re-drawn splits)
__device__ __forceinline__ bool abort_requested(const AbortFlags f) { return __builtin_nontemporal_load(f.dev) != 0u; }
__device__ __forceinline__ bool gate_closed(const uint32_t *gate) { return gate != nullptr && __builtin_nontemporal_load(gate) == 0u; }

struct ScreenCounters {
    unsigned long long fallbacks, violations, stage8_pairs, stage8_decided, stage8b_decided, pad;
};

__global__ void k_init_perm(uint32_t *perm, uint64_t n, uint32_t n_trees) {
    const uint64_t total = n * n_trees;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride)
        perm[g] = (uint32_t)(g % n);
}
// item ids -> rows, in place (sub-tree builds start from caller-given id lists)
__global__ void k_ids_to_rows(DataView dv, uint32_t *perm, uint64_t total, uint32_t *err) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint64_t row = row_of_id(dv, perm[g]);
        if (row == ~0ull) atomicOr(err, 1u);
        perm[g] = (uint32_t)row;
    }
}

// A resident forest's rows: entries [lo, hi), a block each.  The record of the entry (where its level left it: vector first,
// header at hdr_off) -> row `row` of the forest's device rows and its header words, as k_unpack_normals (search.hip) writes
// them from a view: the words of the stored vector are copied, the rest of the row pitch is zero.  W: uint4 where the record
// stride, the row pitch and the vector are whole 16-byte pieces, else 32-bit words (a BQ row is made of uint64_t words).
struct ResidentEntry {
    const uint8_t *rec;
    uint32_t row, pad;
};
template <typename W>
__global__ __launch_bounds__(256) void k_resident_rows(const ResidentEntry *__restrict__ entries, uint32_t lo, uint32_t hi,
                                                       uint64_t hdr_off, uint32_t valid_w, uint32_t row_w, uint32_t hf,
                                                       uint32_t n_rows, W *__restrict__ rows, float *__restrict__ hdrs) {
    const uint64_t e = (uint64_t)lo + blockIdx.x;
    if (e >= hi) return;
    const ResidentEntry en = entries[e];
    if (en.row >= n_rows) return;  // (never: the host numbers the rows it allocated)
    const W *src = reinterpret_cast<const W *>(en.rec);
    W *dst = rows + (uint64_t)en.row * row_w;
    for (uint32_t i = threadIdx.x; i < row_w; i += blockDim.x) dst[i] = i < valid_w ? src[i] : W{};
    if (threadIdx.x < hf) hdrs[(uint64_t)en.row * hf + threadIdx.x] = reinterpret_cast<const float *>(en.rec + hdr_off)[threadIdx.x];
}

// One wave per pending node: sample 2+10 items with the policy RNG, run create_split.
//
// Normal records (device layout == the layout handed to the caller): [vector, row_bytes][header, 16-byte slot].
// M = f32_space_metric(dv.metric): one instantiation per arithmetic (the switch inside one kernel made every build carry the
// registers of the heaviest branch: 115 VGPRs and 80 spilled SGPRs for a kernel that lives on the number of waves in flight)
template <int M>
__global__ __launch_bounds__(64) void k_forest_create_split(DataView dv, FNode *nodes, uint32_t n_nodes,
                                                            const uint32_t *__restrict__ perm, uint64_t n_items,
                                                            uint8_t *normals, uint64_t nstride, uint64_t hdr_off,
                                                            const uint32_t *gate) {
    extern __shared__ float4 s_buf4[];
    float *s_buf = reinterpret_cast<float *>(s_buf4);
    __shared__ uint32_t s_rows[AH_SPLIT_SAMPLES];
    if (gate_closed(gate)) return;
    const uint32_t fpitch = f32_space_pitch(dv.metric, dv.dims);
    for (uint32_t node = blockIdx.x; node < n_nodes; node += gridDim.x) {  // grid-stride: see node_grid in build_batch
        FNode &nd = nodes[node];
        if (nd.state != ST_PENDING) continue;
        __syncthreads();  // the previous node's samples / two-means buffers are dead
        const uint32_t *pp = perm + nd.start;  // starts are absolute positions in the batch permutation
        if (threadIdx.x == 0) {
            uint64_t a, b;
            ah_choose_two(nd.key, nd.attempt, nd.count, &a, &b);  // src/parallel.rs:342-355
            s_rows[0] = pp[a];
            s_rows[1] = pp[b];
            nd.n_left = 0;
        } else if (threadIdx.x >= 2 && threadIdx.x < AH_SPLIT_SAMPLES) {
            s_rows[threadIdx.x] = pp[ah_choose(nd.key, nd.attempt, threadIdx.x - 2, nd.count)];  // :358-367
        }
        __syncthreads();
        uint8_t *rec = normals + node * nstride;
        float *hdr = reinterpret_cast<float *>(rec + hdr_off);
        wave_create_split<M>(dv, s_rows, s_buf, s_buf + fpitch, s_buf + 2 * fpitch, rec, hdr, threadIdx.x);
        if (threadIdx.x == 0) hdr[2] = hdr[3] = 0.0f;  // deterministic padding
        for (uint32_t i = 4 + threadIdx.x; i < (uint32_t)((nstride - hdr_off) >> 2); i += 64) hdr[i] = 0.0f;
    }
}

// The margin loop (src/writer.rs:1201-1207) for all pending nodes of the level, tile by tile.
// Output per tile: 32 side masks (bit i of mask o = side of item o + 32 i of the tile; 1 = Right) and the
// number of Left items; per node: n_left.
// Algorithmic traffic: 4*dims bytes per item (+4 B of permutation, +1 bit out).
template <int METRIC>
__global__ __launch_bounds__(kBlock) void k_forest_margin_f32(DataView dv, FNode *nodes, const FTile *__restrict__ tiles,
                                                              uint32_t n_tiles, const uint32_t *__restrict__ perm,
                                                              uint64_t n_items, const uint8_t *__restrict__ normals,
                                                              uint64_t nstride, uint64_t hdr_off,
                                                              uint64_t *__restrict__ masks,
                                                              uint32_t *__restrict__ tile_left,
                                                              const AbortFlags abort_flag) {
    extern __shared__ float4 s_n4[];
    __shared__ uint32_t s_left;
    const float *s_n = reinterpret_cast<const float *>(s_n4);
    const uint32_t o = threadIdx.x >> 3, j = threadIdx.x & 7u;
    if (gate_closed(abort_flag.gate)) return;  // a retry attempt with no node left pending
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (abort_requested(abort_flag)) return;  // build cancelled: drain (block-uniform)
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (nd->state != ST_PENDING) continue;  // block-uniform
        __syncthreads();
        const float4 *g_n4 = reinterpret_cast<const float4 *>(normals + tl.node * nstride);
        for (uint32_t i = threadIdx.x; i < (dv.pitch >> 2); i += blockDim.x) s_n4[i] = g_n4[i];
        if (threadIdx.x == 0) s_left = 0;
        __syncthreads();
        const float *g_h = reinterpret_cast<const float *>(normals + tl.node * nstride + hdr_off);
        const LeafHdr nh = {g_h[0], g_h[1]};
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        const uint32_t *pp = perm + nd->start + tl.first;
        uint64_t mask = 0;
        uint32_t lefts = 0;
        for (uint32_t i = 0; i < 64; i++) {
            const uint32_t p = o + 32 * i;
            if (p >= in_tile) break;
            const uint64_t row = pp[p];
            const float m = margin_f32<METRIC>(dv, s_n, nh, row, j);
            const uint32_t side = side_of_margin(m);
            mask |= (uint64_t)side << i;
            lefts += side ^ 1u;
        }
        if (j == 0) {
            masks[(uint64_t)tile * 32 + o] = mask;
            if (lefts) atomicAdd(&s_left, lefts);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            tile_left[tile] = s_left;
            if (s_left) atomicAdd(&nodes[tl.node].n_left, s_left);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_forest_margin_bq(DataView dv, FNode *nodes, const FTile *__restrict__ tiles,
                                                             uint32_t n_tiles, const uint32_t *__restrict__ perm,
                                                             uint64_t n_items, const uint8_t *__restrict__ normals,
                                                             uint64_t nstride, uint64_t hdr_off,
                                                             uint64_t *__restrict__ masks,
                                                             uint32_t *__restrict__ tile_left,
                                                             const AbortFlags abort_flag) {
    extern __shared__ uint64_t s_nw[];
    __shared__ uint32_t s_left;
    __shared__ uint8_t s_side[kTile];
    if (gate_closed(abort_flag.gate)) return;  // a retry attempt with no node left pending
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (abort_requested(abort_flag)) return;
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (nd->state != ST_PENDING) continue;
        __syncthreads();
        const uint64_t *g_n = reinterpret_cast<const uint64_t *>(normals + tl.node * nstride);
        for (uint32_t i = threadIdx.x; i < dv.pitch; i += blockDim.x) s_nw[i] = g_n[i];
        if (threadIdx.x == 0) s_left = 0;
        __syncthreads();
        const float *g_h = reinterpret_cast<const float *>(normals + tl.node * nstride + hdr_off);
        const LeafHdr nh = {g_h[0], g_h[1]};
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        const uint32_t *pp = perm + nd->start + tl.first;
        for (uint32_t p = threadIdx.x; p < in_tile; p += blockDim.x)
            s_side[p] = (uint8_t)side_of_margin(margin_bq(dv, s_nw, nh, pp[p]));
        __syncthreads();
        if (threadIdx.x < 32) {  // pack into the same mask layout as the f32 kernel
            uint64_t mask = 0;
            uint32_t lefts = 0;
            for (uint32_t i = 0; i < 64; i++) {
                const uint32_t p = threadIdx.x + 32 * i;
                if (p >= in_tile) break;
                mask |= (uint64_t)s_side[p] << i;
                lefts += s_side[p] ^ 1u;
            }
            masks[(uint64_t)tile * 32 + threadIdx.x] = mask;
            if (lefts) atomicAdd(&s_left, lefts);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            tile_left[tile] = s_left;
            if (s_left) atomicAdd(&nodes[tl.node].n_left, s_left);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Row-major margin pass (first attempt of a level, full-dataset trees, f32 metrics).
//
// Node-major tiles read every item row once PER TREE: T x N x 4*dims bytes of HBM per level.  But at a given
// level every tree partitions the same N rows, so one pass over the rows can serve several trees at once: an
// octet streams row r ONCE and, for each of up to TC trees, looks up the node that owns r in that tree
// (`node_of[t][r]`) and accumulates the dot with that node's normal.  The normals of one level
// (trees x nodes x 4*dims bytes) are small and re-used by thousands of rows, i.e. they come from L2 / the
// Infinity Cache, while HBM traffic drops to ceil(T / TC) x N x 4*dims bytes.  The arithmetic per (row, normal)
// pair is unchanged — the same 32-chain FMA order, the same reduction tree — so the sides are bit-identical to
// the node-major kernel; the host picks whichever mode moves fewer bytes for the level (deep levels, where few
// rows are still active and the normals no longer fit in cache, stay node-major).
// Output: one side byte per (tree, row); k_forest_masks_from_bytes turns them into the tile masks / counts the
// rest of the pipeline consumes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_forest_assign_node_of(const FNode *__restrict__ nodes,
                                                                  const FTile *__restrict__ tiles, uint32_t n_tiles,
                                                                  const uint32_t *__restrict__ perm, uint64_t n_items,
                                                                  uint32_t *__restrict__ node_of, uint32_t only_fix) {
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (only_fix && !nd->fix) continue;
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        const uint32_t *pp = perm + nd->start + tl.first;
        uint32_t *dst = node_of + (uint64_t)nd->tree * n_items;
        for (uint32_t p = threadIdx.x; p < in_tile; p += blockDim.x) dst[pp[p]] = tl.node;
    }
}

// node_of for the next level, in row order: when the level before was row-major too, every (tree, row) pair already
// knows its node and its side, so its child is one table lookup away — a coalesced sweep instead of the scattered
// 4-byte writes of k_forest_assign_node_of (36 ms -> 2 ms per level at 10M x 100 trees).  `child[2 * node + side]` is
// the index of the child in the next level, or 0xFFFFFFFF when it is a leaf (or when the parent's sides were
// re-drawn after the row-major pass: those few nodes are then assigned the scattered way).
__global__ __launch_bounds__(kBlock) void k_forest_advance_node_of(uint32_t *__restrict__ node_of,
                                                                   const uint8_t *__restrict__ side_bytes,
                                                                   const uint32_t *__restrict__ child, uint64_t total) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 4;
    for (uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; g < total; g += stride) {
        if (g + 4 <= total) {
            uint4 n = *reinterpret_cast<const uint4 *>(node_of + g);
            const uchar4 sd = *reinterpret_cast<const uchar4 *>(side_bytes + g);
            if (n.x != 0xFFFFFFFFu) n.x = child[2 * n.x + sd.x];
            if (n.y != 0xFFFFFFFFu) n.y = child[2 * n.y + sd.y];
            if (n.z != 0xFFFFFFFFu) n.z = child[2 * n.z + sd.z];
            if (n.w != 0xFFFFFFFFu) n.w = child[2 * n.w + sd.w];
            *reinterpret_cast<uint4 *>(node_of + g) = n;
        } else {
            for (uint64_t e = g; e < total; e++) {
                const uint32_t n = node_of[e];
                if (n != 0xFFFFFFFFu) node_of[e] = child[2 * n + side_bytes[e]];
            }
        }
    }
}

template <int METRIC, int TC>
__global__ __launch_bounds__(kBlock) void k_forest_margin_rows(DataView dv, const uint32_t *__restrict__ node_of,
                                                               uint32_t tree0, uint32_t n_pass,
                                                               const uint8_t *__restrict__ normals, uint64_t nstride,
                                                               uint64_t hdr_off, uint8_t *__restrict__ side_bytes,
                                                               const AbortFlags abort_flag) {
    const uint32_t j = threadIdx.x & 7u;
    const uint64_t n_octets = ((uint64_t)gridDim.x * blockDim.x) >> 3;
    const uint32_t blocks = dv.dims >> 5;
    if (abort_requested(abort_flag)) return;
    for (uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; row < dv.n; row += n_octets) {
        const float *rp = dv.rows_f32 + row * dv.pitch;
        const float4 *r4 = reinterpret_cast<const float4 *>(rp) + j;
        const float4 *n4[TC];
        bool on[TC];
        float4 acc[TC];
#pragma unroll
        for (int t = 0; t < TC; t++) {
            uint32_t node = 0xFFFFFFFFu;
            if ((uint32_t)t < n_pass) node = node_of[(uint64_t)(tree0 + t) * dv.n + row];
            on[t] = node != 0xFFFFFFFFu;
            n4[t] = reinterpret_cast<const float4 *>(normals + (on[t] ? (uint64_t)node : 0ull) * nstride) + j;
            acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        uint32_t k = 0;
        for (; k + 8 <= blocks; k += 8) {
            float4 x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = ld_stream(r4 + (k + u) * 8);
#pragma unroll
            for (int t = 0; t < TC; t++) {
                if (on[t]) {
#pragma unroll
                    for (int u = 0; u < 8; u++) fma_step<OP_DOT>(acc[t], n4[t][(k + u) * 8], x[u]);
                }
            }
        }
        for (; k < blocks; k++) {
            const float4 x = r4[k * 8];
#pragma unroll
            for (int t = 0; t < TC; t++)
                if (on[t]) fma_step<OP_DOT>(acc[t], n4[t][k * 8], x);
        }
#pragma unroll
        for (int t = 0; t < TC; t++) {
            if (on[t]) {
                const float *np = reinterpret_cast<const float *>(n4[t] - j);
                float d = octet_finish(acc[t]);
                d = scalar_tail<OP_DOT>(d, np, rp, blocks << 5, dv.dims);
                const float *nh = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(np) + hdr_off);
                float m = d;
                if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN) m = f_add(nh[0], d);
                if (METRIC == AH_DOT_PRODUCT) m = f_add(d, f_mul(nh[0], dv.headers[2 * row]));
                if (j == 0) side_bytes[(uint64_t)(tree0 + t) * dv.n + row] = (uint8_t)side_of_margin(m);
            }
        }
    }
}

// Top levels of the forest: a group of trees has so few nodes that ALL its normals of the level fit in LDS (a level's
// nodes are ordered by tree, so a group owns the contiguous range [first_node, first_node + n_group_nodes)).  The
// row-major pass above is bound by the L1/L2 request rate of the normals (0.097 ns per margin at 16 trees); serving them
// from LDS leaves L1 to the row stream and the pass approaches the HBM time of the rows.  One big block per CU shares one
// copy of the normals: 1024 threads for 8 trees (114 VGPRs), 512 for 16 trees (the 64 accumulators need > 128 VGPRs);
// same arithmetic, bit-identical sides.
template <int METRIC, int TC>
__global__ __launch_bounds__(TC >= 16 ? 512 : 1024) void k_forest_margin_rows_lds(DataView dv, const uint32_t *__restrict__ node_of,
                                                                 uint32_t tree0, uint32_t n_pass,
                                                                 const uint8_t *__restrict__ normals, uint64_t nstride,
                                                                 uint64_t hdr_off, uint8_t *__restrict__ side_bytes,
                                                                 uint32_t first_node, uint32_t n_group_nodes,
                                                                 const AbortFlags abort_flag) {
    extern __shared__ float4 s_norm4[];
    if (abort_requested(abort_flag)) return;
    const uint32_t stride4 = (uint32_t)(nstride >> 4);  // record size in float4 (row bytes are a multiple of 128, + 16)
    {
        const float4 *g = reinterpret_cast<const float4 *>(normals + (uint64_t)first_node * nstride);
        const uint32_t total = n_group_nodes * stride4;
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) s_norm4[i] = g[i];
    }
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    const uint64_t n_octets = ((uint64_t)gridDim.x * blockDim.x) >> 3;
    const uint32_t blocks = dv.dims >> 5;
    const uint32_t hdr4 = (uint32_t)(hdr_off >> 4);
    for (uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; row < dv.n; row += n_octets) {
        const float *rp = dv.rows_f32 + row * dv.pitch;
        const float4 *r4 = reinterpret_cast<const float4 *>(rp) + j;
        uint32_t off[TC];  // float4 index of the normal record in LDS
        bool on[TC];
        float4 acc[TC];
#pragma unroll
        for (int t = 0; t < TC; t++) {
            uint32_t node = 0xFFFFFFFFu;
            if ((uint32_t)t < n_pass) node = node_of[(uint64_t)(tree0 + t) * dv.n + row];
            on[t] = node != 0xFFFFFFFFu;
            off[t] = (on[t] ? node - first_node : 0u) * stride4;
            acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        uint32_t k = 0;
        for (; k + 8 <= blocks; k += 8) {
            float4 x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = ld_stream(r4 + (k + u) * 8);
#pragma unroll
            for (int t = 0; t < TC; t++) {
                if (on[t]) {
#pragma unroll
                    for (int u = 0; u < 8; u++) fma_step<OP_DOT>(acc[t], s_norm4[off[t] + (k + u) * 8 + j], x[u]);
                }
            }
        }
        for (; k < blocks; k++) {
            const float4 x = r4[k * 8];
#pragma unroll
            for (int t = 0; t < TC; t++)
                if (on[t]) fma_step<OP_DOT>(acc[t], s_norm4[off[t] + k * 8 + j], x);
        }
#pragma unroll
        for (int t = 0; t < TC; t++) {
            if (on[t]) {
                const float *np = reinterpret_cast<const float *>(s_norm4 + off[t]);
                float d = octet_finish(acc[t]);
                d = scalar_tail<OP_DOT>(d, np, rp, blocks << 5, dv.dims);
                const float *nh = reinterpret_cast<const float *>(s_norm4 + off[t] + hdr4);
                float m = d;
                if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN) m = f_add(nh[0], d);
                if (METRIC == AH_DOT_PRODUCT) m = f_add(d, f_mul(nh[0], dv.headers[2 * row]));
                if (j == 0) side_bytes[(uint64_t)(tree0 + t) * dv.n + row] = (uint8_t)side_of_margin(m);
            }
        }
    }
}

// The side bytes of a level (0 / 1 per (tree, row)) as one bit each, bit g of the flat array = pair g = tree * N + row.
// k_forest_masks_from_bytes reads the sides in the order of the trees' permutations, i.e. at random: a tree's bits are
// N / 8 bytes (1.25 MB at 10M rows: they stay in an L2) where its bytes are N (10 MB: most gathers go out to the fabric).
__global__ __launch_bounds__(256) void k_forest_pack_sides(const uint8_t *__restrict__ side_bytes, uint64_t n_words,
                                                           uint32_t *__restrict__ bits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        const uint4 a = *reinterpret_cast<const uint4 *>(side_bytes + w * 32);
        const uint4 b = *reinterpret_cast<const uint4 *>(side_bytes + w * 32 + 16);
        // bits 0 / 8 / 16 / 24 of a word -> bits 24..27 of the product (no two partial products meet, nothing carries)
        const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t out = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) out |= ((((v[e] & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * e);
        bits[w] = out;
    }
}

// side bytes (by row) -> the per-tile masks / left counts of the node-major pipeline.  `side_bits` != nullptr: the same
// sides, packed by k_forest_pack_sides.
__global__ __launch_bounds__(kBlock) void k_forest_masks_from_bytes(FNode *nodes, const FTile *__restrict__ tiles,
                                                                    uint32_t n_tiles, const uint32_t *__restrict__ perm,
                                                                    uint64_t n_items,
                                                                    const uint8_t *__restrict__ side_bytes,
                                                                    const uint32_t *__restrict__ side_bits,
                                                                    uint64_t *__restrict__ masks,
                                                                    uint32_t *__restrict__ tile_left) {
    // Item p of a tile is bit (p >> 5) of mask (p & 31).  Thread (wave w, lane l) takes the items 256 k + 64 w + l, k = 0..7:
    // the ballot of its k-th side over the wave holds, for every mask o, the two bits 8 k + 2 w (lane o) and 8 k + 2 w + 1
    // (lane o + 32).  The 32 ballots of a tile go through LDS; thread o < 32 assembles mask o from them.
    __shared__ uint64_t s_ballot[8][kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (nd->state != ST_PENDING) continue;
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        const uint32_t *pp = perm + nd->start + tl.first;
        const uint8_t *sb = side_bytes + (uint64_t)nd->tree * n_items;
        uint32_t rows[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t p = 256u * k + threadIdx.x;
            rows[k] = p < in_tile ? pp[p] : 0xFFFFFFFFu;
        }
        uint32_t side[8];
        if (side_bits) {
            const uint64_t g0 = (uint64_t)nd->tree * n_items;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const uint64_t g = g0 + rows[k];
                side[k] = rows[k] != 0xFFFFFFFFu ? side_bits[g >> 5] >> (uint32_t)(g & 31u) : 0u;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) side[k] = rows[k] != 0xFFFFFFFFu ? (uint32_t)sb[rows[k]] : 0u;
        }
        __syncthreads();  // the previous tile's ballots have been consumed
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const unsigned long long bal = __ballot(side[k] & 1u);
            if (lane == 0) s_ballot[k][wave] = bal;
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const uint32_t o = threadIdx.x;
            uint64_t mask = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
#pragma unroll
                for (uint32_t w = 0; w < kBlock / 64; w++) {
                    const uint64_t bal = s_ballot[k][w];
                    mask |= ((bal >> o) & 1ull) << (8 * k + 2 * w);
                    mask |= ((bal >> (o + 32)) & 1ull) << (8 * k + 2 * w + 1);
                }
            const uint32_t n_mine = in_tile > o ? (in_tile - o + 31u) / 32u : 0u;  // items o, o + 32, ... of the tile
            uint32_t lefts = n_mine - (uint32_t)__popcll((unsigned long long)mask);
            masks[(uint64_t)tile * 32 + o] = mask;
            for (int off = 16; off > 0; off >>= 1) lefts += __shfl_down(lefts, off, 32);
            if (o == 0) {
                tile_left[tile] = lefts;
                if (lefts) atomicAdd(&nodes[tl.node].n_left, lefts);
            }
        }
    }
}

// split_imbalance (src/writer.rs:1348-1353, f64) and the accept / retry / random decision (:1209-1227).
__global__ void k_forest_decide(FNode *nodes, uint32_t n_nodes, uint32_t *pend_out, const uint32_t *gate) {
    if (gate_closed(gate)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool again = false;
    if (i < n_nodes && nodes[i].state == ST_PENDING) {
        FNode &nd = nodes[i];
        const double ls = (double)nd.n_left, rs = (double)(nd.count - nd.n_left);
        const double f = ls / (ls + rs + 2.220446049250313e-16);
        const double g = 1.0 - f;
        const double imb = f > g ? f : g;
        if (imb < 0.95 || nd.attempt == 3) {
            if (imb > 0.99) {
                nd.state = ST_RANDOM;
                nd.n_left = 0;
            } else {
                nd.state = ST_ACCEPTED;
            }
        } else {
            nd.attempt += 1;  // remaining_attempts -= 1; n_left is reset by the next create_split
            again = true;
        }
    }
    // nodes left pending, counted once per wave (the gate of the next attempt's launches)
    const unsigned long long m = __ballot(again);
    if (pend_out && m && (threadIdx.x & 63u) == 0) atomicAdd(pend_out, (uint32_t)__popcll(m));
}

// randomly_split_children (src/writer.rs:1310-1326) with the policy coin, same mask layout.
__global__ __launch_bounds__(64) void k_forest_random_sides(FNode *nodes, const FTile *__restrict__ tiles,
                                                            uint32_t n_tiles, uint64_t *__restrict__ masks,
                                                            uint32_t *__restrict__ tile_left) {
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (nd->state != ST_RANDOM) continue;
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        uint32_t lefts = 0;
        if (threadIdx.x < 32) {
            uint64_t mask = 0;
            for (uint32_t i = 0; i < 64; i++) {
                const uint32_t p = threadIdx.x + 32 * i;
                if (p >= in_tile) break;
                const uint32_t left = ah_random_side_is_left(nd->key, (uint64_t)tl.first + p);
                mask |= (uint64_t)(left ^ 1u) << i;
                lefts += left;
            }
            masks[(uint64_t)tile * 32 + threadIdx.x] = mask;
        }
        for (int off = 32; off > 0; off >>= 1) lefts += __shfl_down(lefts, off);
        if (threadIdx.x == 0) {
            tile_left[tile] = lefts;
            if (lefts) atomicAdd(&nodes[tl.node].n_left, lefts);
        }
    }
}

// Exclusive scan of the per-tile left counts inside every node: one wave per node.
__global__ __launch_bounds__(64) void k_forest_tile_offsets(const FNode *__restrict__ nodes, uint32_t n_nodes,
                                                            const uint32_t *__restrict__ tile_left,
                                                            uint32_t *__restrict__ tile_left_off) {
    for (uint32_t node = blockIdx.x; node < n_nodes; node += gridDim.x) {
        const FNode nd = nodes[node];
        uint32_t carry = 0;
        for (uint32_t base = 0; base < nd.n_tiles; base += 64) {
            const uint32_t t = base + threadIdx.x;
            const uint32_t v = t < nd.n_tiles ? tile_left[nd.tile_begin + t] : 0u;
            uint32_t incl = v;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(incl, off);
                if ((int)threadIdx.x >= off) incl += up;
            }
            if (t < nd.n_tiles) tile_left_off[nd.tile_begin + t] = carry + incl - v;
            carry += __shfl(incl, 63);
        }
    }
}

// Stable partition of every split node into its children (ascending order kept inside each child =
// RoaringBitmap::from_sorted_iter, src/writer.rs:1230-1231).  A child that fits in a Descendants node
// (count <= split_after, :474-477) is written to `final_perm`, the others to the next level's permutation.
__global__ __launch_bounds__(kBlock) void k_forest_scatter(const FNode *__restrict__ nodes,
                                                           const FTile *__restrict__ tiles, uint32_t n_tiles,
                                                           const uint32_t *__restrict__ perm_cur,
                                                           uint32_t *__restrict__ perm_next,
                                                           uint32_t *__restrict__ final_perm, uint64_t n_items,
                                                           const uint64_t *__restrict__ masks,
                                                           const uint32_t *__restrict__ tile_left_off,
                                                           uint32_t split_after) {
    __shared__ uint64_t s_masks[32];
    __shared__ uint32_t s_wave[kBlock / 64];
    __shared__ uint32_t s_in[kTile], s_out[kTile];  // the tile's items as read / partitioned (lefts first)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const FTile tl = tiles[tile];
        const FNode nd = nodes[tl.node];
        const uint32_t in_tile = min(kTile, nd.count - tl.first);
        const uint64_t base = nd.start;
        __syncthreads();
        if (threadIdx.x < 32) s_masks[threadIdx.x] = masks[(uint64_t)tile * 32 + threadIdx.x];
        {  // coalesced read of the tile
            const uint32_t *src = perm_cur + base + tl.first;
            for (uint32_t p = threadIdx.x; p < in_tile; p += kBlock) s_in[p] = src[p];
        }
        __syncthreads();
        const uint32_t p0 = threadIdx.x * 8;
        const uint32_t i = p0 >> 5;
        const uint32_t nvalid = p0 < in_tile ? min(8u, in_tile - p0) : 0u;
        uint32_t sidebits = 0;
        for (uint32_t e = 0; e < nvalid; e++) sidebits |= (uint32_t)((s_masks[(p0 + e) & 31u] >> i) & 1ull) << e;
        const uint32_t my_left = nvalid - (uint32_t)__popc(sidebits);
        // block-wide exclusive scan of my_left
        uint32_t incl = my_left;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if ((int)lane >= off) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t wave_base = 0, tile_lefts = 0;
        for (uint32_t w = 0; w < kBlock / 64; w++) {
            if (w < wave) wave_base += s_wave[w];
            tile_lefts += s_wave[w];
        }
        // stable partition inside LDS: lefts to [0, tile_lefts), rights to [tile_lefts, in_tile), order kept
        uint32_t lp = wave_base + incl - my_left;  // lefts of the tile before p0
        uint32_t rp = tile_lefts + (p0 - lp);      // rights of the tile before p0, behind all lefts
        for (uint32_t e = 0; e < nvalid; e++) {
            const uint32_t row = s_in[p0 + e];
            if ((sidebits >> e) & 1u) s_out[rp++] = row;
            else s_out[lp++] = row;
        }
        __syncthreads();
        // two contiguous runs out, coalesced: the node's lefts before this tile = tile_left_off, its rights before it =
        // items before the tile - lefts before the tile
        const uint32_t lefts_before = tile_left_off[tile];
        const uint32_t n_right = nd.count - nd.n_left;
        uint32_t *dst_l = (nd.n_left <= split_after ? final_perm : perm_next) + base + lefts_before;
        uint32_t *dst_r = (n_right <= split_after ? final_perm : perm_next) + base + nd.n_left + (tl.first - lefts_before);
        for (uint32_t p = threadIdx.x; p < in_tile; p += kBlock) {
            const uint32_t row = s_out[p];
            if (p < tile_lefts) dst_l[p] = row;
            else dst_r[p - tile_lefts] = row;
        }
    }
}

__global__ void k_rows_to_ids(uint32_t *perm, uint64_t total, const uint32_t *__restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) perm[g] = ids[perm[g]];
}

// ------------------------------------------------------------------------------------------------
// Certified binary16 screen (screen_device.h): shadow copies and the screened variants of the three margin kernels.
// ------------------------------------------------------------------------------------------------

// (to_shadow_half and kTinyBits: screen_device.h — the search's certified top-k screen makes the same copies of its queries)

// rows -> binary16 shadow + per-row stats.  One octet per row, lane j converts elements 32k + 4j .. +3 (8 bytes out).
__global__ __launch_bounds__(kBlock) void k_shadow_rows(DataView dv, uint16_t *__restrict__ h_rows, uint32_t hpitch,
                                                        float4 *__restrict__ stats) {
    const uint32_t j = threadIdx.x & 7u;
    const uint64_t n_octets = ((uint64_t)gridDim.x * blockDim.x) >> 3;
    const uint32_t blocks = dv.pitch >> 5;  // the padding of the f32 row is zero
    for (uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; row < dv.n; row += n_octets) {
        const float4 *r4 = reinterpret_cast<const float4 *>(dv.rows_f32 + row * dv.pitch) + j;
        uint2 *o2 = reinterpret_cast<uint2 *>(h_rows + row * hpitch) + j;
        float sa = 0.f, sb = 0.f, sc = 0.f;
        uint32_t xbits = 0u;
        for (uint32_t k = 0; k < blocks; k++) {
            float4 x = ld_stream(r4 + k * 8);
            const uint32_t e0 = 32 * k + 4 * j;  // elements beyond dims (row padding) count as zeros
            if (e0 + 0 >= dv.dims) x.x = 0.0f;
            if (e0 + 1 >= dv.dims) x.y = 0.0f;
            if (e0 + 2 >= dv.dims) x.z = 0.0f;
            if (e0 + 3 >= dv.dims) x.w = 0.0f;
            xbits = max(max(xbits, __float_as_uint(x.x) & 0x7FFFFFFFu), max(__float_as_uint(x.y) & 0x7FFFFFFFu,
                        max(__float_as_uint(x.z) & 0x7FFFFFFFu, __float_as_uint(x.w) & 0x7FFFFFFFu)));
            const _Float16 h0 = to_shadow_half(x.x), h1 = to_shadow_half(x.y), h2 = to_shadow_half(x.z), h3 = to_shadow_half(x.w);
            const float y0 = (float)h0, y1 = (float)h1, y2 = (float)h2, y3 = (float)h3;
            sa += y0 * y0 + y1 * y1 + y2 * y2 + y3 * y3;
            const float d0 = x.x - y0, d1 = x.y - y1, d2 = x.z - y2, d3 = x.w - y3;
            sb += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
            sc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
            f16x2_t lo = {h0, h1}, hi = {h2, h3};
            o2[k * 8] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
        }
        if (hpitch > dv.pitch) o2[blocks * 8] = make_uint2(0u, 0u);  // pitch is 32 mod 64: zero the last half line
        sa = octet_sum(sa);
        sb = octet_sum(sb);
        sc = octet_sum(sc);
        // 2-norms rounded UP: the f32 sums of squares carry a relative error below (dims + 8) * 2^-24
        const float up = 1.0f + (float)(dv.pitch + 64u) * 1.2e-7f;
        xbits = max(xbits, (uint32_t)__shfl_xor((int)xbits, 1, 8));
        xbits = max(xbits, (uint32_t)__shfl_xor((int)xbits, 2, 8));
        xbits = max(xbits, (uint32_t)__shfl_xor((int)xbits, 4, 8));
        const bool tiny = xbits != 0u && xbits < kTinyBits;
        const float inf = __uint_as_float(0x7F800000u);
        if (j == 0) stats[row] = tiny ? make_float4(inf, inf, inf, 0.0f) : make_float4(sqrtf(sa) * up, sqrtf(sb) * up, sqrtf(sc) * up, 0.0f);
    }
}

// Component-wise maximum of the per-row stats (all >= 0, so the bit patterns order like the values; inf / NaN end up on
// top and simply disable the cheap test below).  The node-major screen tries the bound built from these maxima first — it
// needs no per-row load — and fetches the row's own stats (a 16-byte random read = one more 128-byte line per pair) only
// when that bound cannot decide: for rows of similar norms that is ~1.5 % of the pairs.
__global__ __launch_bounds__(256) void k_stats_max(const float4 *__restrict__ stats, uint64_t n, uint32_t *__restrict__ out) {
    __shared__ uint32_t s_m[3];
    __shared__ float s_sum;
    if (threadIdx.x < 3) s_m[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_sum = 0.0f;
    __syncthreads();
    uint32_t a = 0, b = 0, c = 0;
    float sum = 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const float4 v = stats[i];
        a = max(a, __float_as_uint(v.x));
        b = max(b, __float_as_uint(v.y));
        c = max(c, __float_as_uint(v.z));
        sum += v.z;
    }
    atomicMax(&s_m[0], a);
    atomicMax(&s_m[1], b);
    atomicMax(&s_m[2], c);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x < 3) atomicMax(&out[threadIdx.x], s_m[threadIdx.x]);
    // out[3]: sum of the row norms (a float; its summation order is not fixed — it only feeds the heuristic that decides
    // whether the int8 copy is worth keeping, never a result)
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<float *>(out) + 3, s_sum);
}

// ------------------------------------------------------------------------------------------------
// First stage of the node-major screen: an int8 copy.  The deep levels move one row per (item, node) pair and run at the
// device's gather rate (1.6 KB per pair with the binary16 copy); the same certified-sign argument holds for ANY copy whose
// distance to the original is measured, so a coarser copy goes first.
//
//   rows      y = x / d (d = one power of two per DIMENSION: the largest |x_i| of the column rounded up, so a few
//             "outlier dimensions" do not eat the 8 bits of all the others; exact, <n, x> = <n o d, x / d>), then
//             y~ = s_r q with ONE SCALE PER ROW (s_r = max|y| / 127, q = int8): rows of very different norms and data with
//             long tails (N(0,1): the 5-sigma entries of the dataset) quantise as well as uniform data;
//   normals   n' = n o d, n~' = s_n (q_hi + q_lo / 256): TWO int8 digits.  The normal sits in LDS, so its second digit
//             costs no HBM byte, and it removes the normal's half of the error bound (76 % -> ~90 % of the pairs decided
//             on the uniform benchmark rows, ~69 % -> ~84 % on N(0,1) rows);
//   screen    S = s_n (<q_hi, q> + <q_lo, q> / 256), integer dot products (v_dot4_i32_i8), exact;
//   bound     |s_r S - r| <= s_r (|n' - n~'| |q| + |n'| |y/s_r - q| + g8 |n~'||q|) + gamma_r |n||x|.
//
// The sign of a cosine margin does not depend on s_r > 0, so for Cosine the test runs in units of s_r with the
// DATASET-WIDE maxima of |q|, |y/s_r - q|, |x|/s_r (all dimensionless, the same for every row up to a few percent): a decided
// pair costs its 768-byte int8 row and nothing else — no per-row load at all.  Euclidean / Manhattan add the bias in real
// units and fetch s_r (4 bytes per pair from a 40 MB array).  DotProduct has no int8 stage (its margin needs the row's header
// anyway).  Rows that are all zero, not finite, or so small that f32 squares underflow (max|x| < 2^-40) get q = 0 and
// s_r = inf: they are never decided here.  Sides stay identical by construction; AH_SCREEN_VERIFY checks every pair at
// every stage.  (NormalStats8, the tail of a normal's int8 record, is in forest_records.h: its size is part of a batch's sizes.)
// ------------------------------------------------------------------------------------------------

// column-wise max |x| (as bits) over all rows: thread t of a block owns columns t, t + 256, ...
__global__ __launch_bounds__(256) void k_col_maxabs(DataView dv, uint32_t *__restrict__ out_bits) {
    const uint64_t rows_per_block = (dv.n + gridDim.x - 1) / gridDim.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block, r1 = min(dv.n, r0 + rows_per_block);
    for (uint32_t c = threadIdx.x; c < dv.dims; c += blockDim.x) {
        uint32_t m = 0;
        for (uint64_t r = r0; r < r1; r++) m = max(m, __float_as_uint(dv.rows_f32[r * dv.pitch + c]) & 0x7FFFFFFFu);
        atomicMax(&out_bits[c], m);
    }
}
// column maxima -> one power of two per dimension (d >= max|x_i|; 1 for empty / non-finite columns), and its inverse
__global__ void k_dim_scales(const uint32_t *__restrict__ max_bits, uint32_t dims, uint32_t pitch8, float *__restrict__ d,
                             float *__restrict__ inv_d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pitch8) return;
    float v = 1.0f;
    if (i < dims) {
        const uint32_t b = max_bits[i];
        uint32_t e = b >> 23;                      // biased exponent of the column maximum
        if ((b & 0x7FFFFFu) != 0u) e += 1;         // not a power of two itself: round up
        if (b != 0u && b < 0x7F800000u && e >= 64u && e <= 190u) v = __uint_as_float(e << 23);  // 2^-63 .. 2^63, else 1
    }
    d[i] = v;
    inv_d[i] = 1.0f / v;  // exact: a power of two
}
__device__ __forceinline__ uint32_t octet_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__shfl_xor((int)v, 1, 8));
    v = max(v, (uint32_t)__shfl_xor((int)v, 2, 8));
    return max(v, (uint32_t)__shfl_xor((int)v, 4, 8));
}
// rows -> int8 copy with one scale per row; max_bits[0..2] = max over the rows of |q|, |y / s_r - q|, |x| / s_r (rounded up).
// One octet per row: a pass for the row's max |y|, a pass that quantises (the row comes back from L2).
// rows8_lo: the rows' SECOND int8 digit, q2 = round((y / s_r - q) 256) (stage 1 of the node-major screen: a pair the first
// digit cannot decide reads 768 more bytes instead of the 1536-byte binary16 row); max_bits[3..4] = max |q + q2/256| and
// max |y / s_r - q - q2/256|.
__global__ __launch_bounds__(kBlock) void k_shadow_rows8(DataView dv, const float *__restrict__ inv_d, int8_t *__restrict__ rows8,
                                                         int8_t *__restrict__ rows8_lo, uint32_t pitch8,
                                                         float *__restrict__ row_scale, uint32_t *__restrict__ max_bits) {
    __shared__ uint32_t s_m[5];
    if (threadIdx.x < 5) s_m[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    const uint64_t n_octets = ((uint64_t)gridDim.x * blockDim.x) >> 3;
    const uint32_t blocks = dv.pitch >> 5;
    const float4 *id4 = reinterpret_cast<const float4 *>(inv_d) + j;
    float ma = 0.f, mb = 0.f, mc = 0.f, ma2 = 0.f, mb2 = 0.f;
    for (uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; row < dv.n; row += n_octets) {
        const float4 *r4 = reinterpret_cast<const float4 *>(dv.rows_f32 + row * dv.pitch) + j;
        uint32_t *o = reinterpret_cast<uint32_t *>(rows8 + row * pitch8);
        uint32_t *o2 = reinterpret_cast<uint32_t *>(rows8_lo + row * pitch8);
        uint32_t mbits = 0u, xbits = 0u;  // max |y|, max |x| (non-finite values end up on top)
        for (uint32_t k = 0; k < blocks; k++) {
            const float4 x = r4[k * 8];  // (the padding of a row is zero)
            const float4 g = id4[k * 8];
            mbits = max(max(mbits, __float_as_uint(x.x * g.x) & 0x7FFFFFFFu), max(__float_as_uint(x.y * g.y) & 0x7FFFFFFFu,
                        max(__float_as_uint(x.z * g.z) & 0x7FFFFFFFu, __float_as_uint(x.w * g.w) & 0x7FFFFFFFu)));
            xbits = max(max(xbits, __float_as_uint(x.x) & 0x7FFFFFFFu), max(__float_as_uint(x.y) & 0x7FFFFFFFu,
                        max(__float_as_uint(x.z) & 0x7FFFFFFFu, __float_as_uint(x.w) & 0x7FFFFFFFu)));
        }
        mbits = octet_max_u32(mbits);
        xbits = octet_max_u32(xbits);
        // usable: finite, and neither the row nor its column-scaled image is so small that squares underflow
        const bool ok = mbits >= kTinyBits && xbits >= kTinyBits && mbits < 0x7F800000u && xbits < 0x7F800000u;
        const float m = __uint_as_float(mbits);
        const float scale = ok ? m / 127.0f : 0.0f, inv_scale = ok ? 127.0f / m : 0.0f;
        float sa = 0.f, sb = 0.f, sc = 0.f, sa2 = 0.f, sb2 = 0.f;
        for (uint32_t k = 0; k < blocks; k++) {
            float4 x = ld_stream(r4 + k * 8);
            const float4 g = id4[k * 8];
            const uint32_t e0 = 32 * k + 4 * j;
            if (e0 + 0 >= dv.dims) x.x = 0.0f;
            if (e0 + 1 >= dv.dims) x.y = 0.0f;
            if (e0 + 2 >= dv.dims) x.z = 0.0f;
            if (e0 + 3 >= dv.dims) x.w = 0.0f;
            const float y[4] = {x.x * g.x, x.y * g.y, x.z * g.z, x.w * g.w};  // exact: g is a power of two
            uint32_t w1 = 0u, w2 = 0u;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                // (!ok rows — all zero, tiny, or not finite — store q = r = 0: inf * 0 = NaN would otherwise clamp to -127 and,
                // with Cosine's scale-free test, let a non-finite row be "decided" by the sign of garbage)
                const float t = y[c] * inv_scale;
                const int q = ok ? quantize8(y[c], inv_scale) : 0;
                const int r = ok ? (int)fminf(fmaxf(rintf((t - (float)q) * 256.0f), -127.0f), 127.0f) : 0;
                const float z = (float)q * scale, z2 = ((float)q + (float)r * 0.00390625f) * scale;  // the digits sum exactly
                sa += (float)(q * q);  // exact integers (< 2^24 per lane up to 8000 dims)
                const float d = y[c] - z, d2 = y[c] - z2, v2 = (float)q + (float)r * 0.00390625f;
                sb += d * d;
                sa2 += v2 * v2;
                sb2 += d2 * d2;
                w1 |= ((uint32_t)q & 0xFFu) << (8 * c);
                w2 |= ((uint32_t)r & 0xFFu) << (8 * c);
            }
            sc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
            o[k * 8 + j] = w1;
            if (rows8_lo) o2[k * 8 + j] = w2;
        }
        for (uint32_t w = (dv.pitch >> 2) + j; w < (pitch8 >> 2); w += 8) {  // zero tail of the int8 rows
            o[w] = 0u;
            if (rows8_lo) o2[w] = 0u;
        }
        sa = octet_sum(sa);
        sb = octet_sum(sb);
        sc = octet_sum(sc);
        sa2 = octet_sum(sa2);
        sb2 = octet_sum(sb2);
        // inf: the row never decides here.  An all-zero row is exact at scale 0 (q = 0, every product with it is 0): the top-k
        // screen of the search (search.hip) then needs no fall-back for the zero vectors real corpora hold
        if (j == 0) row_scale[row] = ok ? scale : (xbits == 0u ? 0.0f : __uint_as_float(0x7F800000u));
        if (ok) {
            // in units of the row's scale, rounded UP: f32 sums of squares (relative error < (pitch + 8) 2^-24), the
            // rounding of scale * q inside the difference (2^-24 |z| per element, |z| <= 127 scale), the division
            const float up = (1.0f + (float)(dv.pitch + 64u) * 1.2e-7f) * 1.000001f;
            ma = fmaxf(ma, sqrtf(sa) * up);
            mb = fmaxf(mb, (sqrtf(sb) * up + 127.0f * scale * 6.0e-8f * sqrtf((float)dv.pitch)) / scale * 1.000001f);
            mc = fmaxf(mc, sqrtf(sc) * up / scale * 1.000001f);
            ma2 = fmaxf(ma2, sqrtf(sa2) * up);
            mb2 = fmaxf(mb2, (sqrtf(sb2) * up + 128.0f * scale * 6.0e-8f * sqrtf((float)dv.pitch)) / scale * 1.000001f);
        }
    }
    atomicMax(&s_m[0], __float_as_uint(ma));
    atomicMax(&s_m[1], __float_as_uint(mb));
    atomicMax(&s_m[2], __float_as_uint(mc));
    atomicMax(&s_m[3], __float_as_uint(ma2));
    atomicMax(&s_m[4], __float_as_uint(mb2));
    __syncthreads();
    if (threadIdx.x < 5) atomicMax(&max_bits[threadIdx.x], s_m[threadIdx.x]);
}
// The level's normals -> int8 records [pitch8 bytes q_hi][pitch8 bytes q_lo][NormalStats8], one wave per pending node.
__global__ __launch_bounds__(64) void k_forest_shadow_normals8(DataView dv, const FNode *__restrict__ nodes, uint32_t n_nodes,
                                                               const uint8_t *__restrict__ normals, uint64_t nstride,
                                                               uint64_t hdr_off, const float *__restrict__ dim_scale,
                                                               uint8_t *__restrict__ shadow8, uint64_t stride8,
                                                               uint32_t pitch8, const uint32_t *gate) {
    if (gate_closed(gate)) return;
    for (uint32_t node = blockIdx.x; node < n_nodes; node += gridDim.x) {
        if (nodes[node].state != ST_PENDING) continue;
        const float *nv = reinterpret_cast<const float *>(normals + node * nstride);
        int8_t *out_hi = reinterpret_cast<int8_t *>(shadow8 + node * stride8);
        int8_t *out_lo = out_hi + pitch8;
        uint32_t mbits = 0;
        for (uint32_t i = threadIdx.x; i < dv.dims; i += 64) mbits = max(mbits, __float_as_uint(nv[i] * dim_scale[i]) & 0x7FFFFFFFu);
        for (int off = 32; off > 0; off >>= 1) mbits = max(mbits, (uint32_t)__shfl_xor((int)mbits, off));
        const float m = __uint_as_float(mbits);
        const bool ok = mbits >= kTinyBits && mbits < 0x7F800000u;  // finite, not (nearly) zero
        const float scale = ok ? m / 127.0f : 0.0f, inv_scale = ok ? 127.0f / m : 0.0f;
        float sa = 0.f, sb = 0.f, sc = 0.f, s0 = 0.f;
        for (uint32_t i = threadIdx.x; i < pitch8; i += 64) {
            const float x0 = i < dv.dims ? nv[i] : 0.0f;
            const float x = i < dv.dims ? x0 * dim_scale[i] : 0.0f;  // exact: a power of two
            const float t = x * inv_scale;
            const int qh = ok ? quantize8(x, inv_scale) : 0;
            const int ql = ok ? (int)fminf(fmaxf(rintf((t - (float)qh) * 256.0f), -127.0f), 127.0f) : 0;
            const float y = ((float)qh + (float)ql * 0.00390625f) * scale, d = x - y;  // the digits sum exactly (16 bits)
            sa += y * y;
            sb += d * d;
            sc += x * x;
            s0 += x0 * x0;
            out_hi[i] = (int8_t)qh;
            out_lo[i] = (int8_t)ql;
        }
        for (int off = 32; off > 0; off >>= 1) {
            sa += __shfl_xor(sa, off);
            sb += __shfl_xor(sb, off);
            sc += __shfl_xor(sc, off);
            s0 += __shfl_xor(s0, off);
        }
        if (threadIdx.x == 0) {
            const float up = 1.0f + (float)(pitch8 + 64u) * 1.2e-7f;
            const float *nh = reinterpret_cast<const float *>(normals + node * nstride + hdr_off);
            NormalStats8 st;
            st.an = sqrtf(sa) * up;
            st.bn = ok ? sqrtf(sb) * up + 128.0f * scale * 6.0e-8f * sqrtf((float)pitch8) : __uint_as_float(0x7F800000u);
            st.cn = sqrtf(sc) * up;
            st.cn0 = sqrtf(s0) * up;
            st.extra = dv.metric == AH_COSINE ? 0.0f : nh[0];
            st.scale = scale;
            st.pad0 = st.pad1 = 0.0f;
            *reinterpret_cast<NormalStats8 *>(shadow8 + node * stride8 + 2 * (uint64_t)pitch8) = st;
        }
    }
}
// integer dot of one int8 row against the two int8 digits of the normal in LDS, octet-cooperative: lane j covers bytes
// 128 k + 16 j .. +15.  hi4 / lo4 = normal digits (LDS) + j, r4 = row (global, streamed) + j.
// Result: <q_hi, q> + <q_lo, q> / 256 as float (the integers are exact; one rounding per lane total and per octet add).
__device__ __forceinline__ float screen8_octet_dot(const uint4 *hi4, const uint4 *lo4, const uint4 *r4, uint32_t steps) {
    int h0 = 0, h1 = 0, l0 = 0, l1 = 0;
    uint32_t k = 0;
    for (; k + 6 <= steps; k += 6) {
        uint4 x[6];
#pragma unroll
        for (int u = 0; u < 6; u++) x[u] = ld_stream_u4(r4 + (k + u) * 8);
#pragma unroll
        for (int u = 0; u < 6; u += 2) {
            h0 = dot16_i8(hi4[(k + u) * 8], x[u], h0);
            l0 = dot16_i8(lo4[(k + u) * 8], x[u], l0);
            h1 = dot16_i8(hi4[(k + u + 1) * 8], x[u + 1], h1);
            l1 = dot16_i8(lo4[(k + u + 1) * 8], x[u + 1], l1);
        }
    }
    for (; k < steps; k++) {
        const uint4 x = ld_stream_u4(r4 + k * 8);
        h0 = dot16_i8(hi4[k * 8], x, h0);
        l0 = dot16_i8(lo4[k * 8], x, l0);
    }
    return octet_sum((float)(h0 + h1) + (float)(l0 + l1) * 0.00390625f);
}
// the same with the row's chunks already in registers (PRE of them; chunk u exists when u < steps)
template <int PRE>
__device__ __forceinline__ float screen8_octet_dot_regs(const uint4 *hi4, const uint4 *lo4, const uint4 (&x)[PRE], uint32_t steps) {
    int h0 = 0, h1 = 0, l0 = 0, l1 = 0;
#pragma unroll
    for (int u = 0; u < PRE; u += 2) {
        if ((uint32_t)u < steps) {
            h0 = dot16_i8(hi4[u * 8], x[u], h0);
            l0 = dot16_i8(lo4[u * 8], x[u], l0);
        }
        if ((uint32_t)(u + 1) < steps) {
            h1 = dot16_i8(hi4[(u + 1) * 8], x[u + 1], h1);
            l1 = dot16_i8(lo4[(u + 1) * 8], x[u + 1], l1);
        }
    }
    return octet_sum((float)(h0 + h1) + (float)(l0 + l1) * 0.00390625f);
}
// the decision of the int8 stage.  S = s_n x (the digits' dot products), i.e. the screen value in units of the row's scale;
// max8 = dataset-wide {|q|, |y / s_r - q|, |x| / s_r}; s_row = the row's scale (Euclidean / Manhattan; unused for Cosine).
template <int METRIC>
__device__ __forceinline__ bool screen8_decides(float S, float s_row, const float4 max8, const NormalStats8 ns, float gamma_r,
                                                uint32_t &side) {
    // g8 = 2e-6: the conversions and sums of the lane totals (each exact below 2^24) and the scale product
    float e = ns.bn * max8.x + ns.cn * max8.y + 2.0e-6f * (ns.an * max8.x) + gamma_r * (ns.cn0 * max8.z);
    float m = S;
    if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN) {
        // back to real units (s_row = inf for rows that must not be decided here: m and e turn NaN / inf -> undecided),
        // then r = fl(bias + fl_ref(dot)) as in screen_decides
        const float sd = S * s_row;
        e = e * s_row * 1.000001f + 1.2e-7f * fabsf(sd);
        m = ns.extra + sd;
        e += 2.4e-7f * (fabsf(ns.extra) + fabsf(sd) + e);
    }
    e = e * 1.002f + 1e-30f;
    side = (__float_as_uint(m) >> 31) ^ 1u;
    return fabsf(m) > e;  // false for NaN / inf
}

// The level's normals (records [vector][header slot]) -> shadow records [hpitch halves][NormalStats], one wave per node.
__global__ __launch_bounds__(64) void k_forest_shadow_normals(DataView dv, const FNode *__restrict__ nodes,
                                                              const uint8_t *__restrict__ normals, uint64_t nstride,
                                                              uint64_t hdr_off, uint8_t *__restrict__ shadow,
                                                              uint64_t hstride, uint32_t hpitch, uint32_t n_nodes,
                                                              const uint32_t *gate) {
    if (gate_closed(gate)) return;
    for (uint32_t node = blockIdx.x; node < n_nodes; node += gridDim.x) {
    if (nodes[node].state != ST_PENDING) continue;
    const float *nv = reinterpret_cast<const float *>(normals + node * nstride);
    uint16_t *out = reinterpret_cast<uint16_t *>(shadow + node * hstride);
    float sa = 0.f, sb = 0.f, sc = 0.f;
    for (uint32_t i = threadIdx.x; i < hpitch; i += 64) {
        const float x = i < dv.dims ? nv[i] : 0.0f;
        const _Float16 h = to_shadow_half(x);
        const float y = (float)h, d = x - y;
        sa += y * y;
        sb += d * d;
        sc += x * x;
        out[i] = __builtin_bit_cast(uint16_t, h);
    }
    for (int off = 32; off > 0; off >>= 1) {
        sa += __shfl_xor(sa, off);
        sb += __shfl_xor(sb, off);
        sc += __shfl_xor(sc, off);
    }
    if (threadIdx.x == 0) {
        const float up = 1.0f + (float)(hpitch + 64u) * 1.2e-7f;
        const float *nh = reinterpret_cast<const float *>(normals + node * nstride + hdr_off);
        NormalStats st;
        st.an = sqrtf(sa) * up;
        st.bn = sqrtf(sb) * up;
        st.cn = sqrtf(sc) * up;
        st.extra = dv.metric == AH_COSINE ? 0.0f : nh[0];  // bias (Euclidean / Manhattan) or the normal's extra dimension
        *reinterpret_cast<NormalStats *>(shadow + node * hstride + (uint64_t)hpitch * 2) = st;
    }
    }
}

// screen dot product of one row against one normal, octet-cooperative: lane j covers halves 64k + 8j .. +7
// a4 = normal (LDS or global), r4 = row (global, streamed); steps = hpitch / 64.  Result on every lane of the octet.
__device__ __forceinline__ float screen_octet_dot(const uint4 *a4, const uint4 *r4, uint32_t steps) {
    float acc0 = 0.f, acc1 = 0.f;
    uint32_t k = 0;
    for (; k + 8 <= steps; k += 8) {
        uint4 x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = ld_stream_u4(r4 + (k + u) * 8);
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            acc0 = screen_dot8(a4[(k + u) * 8], x[u], acc0);
            acc1 = screen_dot8(a4[(k + u + 1) * 8], x[u + 1], acc1);
        }
    }
    if (k + 4 <= steps) {
        uint4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = ld_stream_u4(r4 + (k + u) * 8);
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            acc0 = screen_dot8(a4[(k + u) * 8], x[u], acc0);
            acc1 = screen_dot8(a4[(k + u + 1) * 8], x[u + 1], acc1);
        }
        k += 4;
    }
    for (; k < steps; k++) acc0 = screen_dot8(a4[k * 8], ld_stream_u4(r4 + k * 8), acc0);
    return octet_sum(acc0 + acc1);
}

// Node-major margin pass with the screen: as k_forest_margin_f32, but an item costs 2*dims bytes of HBM unless the
// screen cannot decide its side (then the reference arithmetic runs for that item, from the f32 normal kept in LDS).
// PRE > 0 (int8 rows of at most PRE 128-byte steps): the int8 chunks of the NEXT item of an octet are requested before the
// current item is evaluated, and its row index one item earlier still — an item otherwise costs two dependent memory round
// trips (perm -> row) with nothing else in flight on the octet.
template <int METRIC, int PRE>
__global__ __launch_bounds__(kBlock) void k_forest_screen_node(DataView dv, ScreenView sv, FNode *nodes,
                                                               const FTile *__restrict__ tiles, uint32_t n_tiles,
                                                               const uint32_t *__restrict__ perm,
                                                               const uint8_t *__restrict__ normals, uint64_t nstride,
                                                               uint64_t hdr_off, const uint8_t *__restrict__ shadow,
                                                               uint64_t hstride, const uint8_t *__restrict__ shadow8,
                                                               uint64_t stride8, uint64_t *__restrict__ masks,
                                                               uint32_t *__restrict__ tile_left,
                                                               const AbortFlags abort_flag,
                                                               ScreenCounters *__restrict__ counters, uint32_t verify) {
    extern __shared__ float4 s_n4[];  // [pitch floats f32 normal][hpitch halves shadow normal][2 x pitch8 bytes: the int8 digits]
    __shared__ uint32_t s_left, s_fb, s_bad, s_n8, s_d8, s_d8b;
    const float *s_n = reinterpret_cast<const float *>(s_n4);
    const uint4 *s_h4 = reinterpret_cast<const uint4 *>(s_n4 + (dv.pitch >> 2));
    const uint4 *s_q4 = s_h4 + (sv.hpitch >> 3);        // q_hi
    const uint4 *s_ql4 = s_q4 + (sv.pitch8 >> 4);        // q_lo
    const bool stage8 = METRIC != AH_DOT_PRODUCT && sv.rows8 != nullptr && shadow8 != nullptr;  // (DotProduct needs the row's header anyway)
    const uint32_t steps8 = sv.pitch8 >> 7;
    const uint32_t o = threadIdx.x >> 3, j = threadIdx.x & 7u;
    const uint32_t steps = sv.hpitch >> 6;
    uint32_t fallbacks = 0, bad = 0, met8 = 0, decided8 = 0, decided8b = 0;
    if (gate_closed(abort_flag.gate)) return;  // a retry attempt with no node left pending
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (abort_requested(abort_flag)) return;
        const FTile tl = tiles[tile];
        const FNode *nd = nodes + tl.node;
        if (nd->state != ST_PENDING) continue;  // block-uniform
        __syncthreads();
        {
            const float4 *g_n4 = reinterpret_cast<const float4 *>(normals + tl.node * nstride);
            for (uint32_t i = threadIdx.x; i < (dv.pitch >> 2); i += blockDim.x) s_n4[i] = g_n4[i];
            const uint4 *g_h4 = reinterpret_cast<const uint4 *>(shadow + tl.node * hstride);
            uint4 *d_h4 = reinterpret_cast<uint4 *>(s_n4 + (dv.pitch >> 2));
            for (uint32_t i = threadIdx.x; i < (sv.hpitch >> 3); i += blockDim.x) d_h4[i] = g_h4[i];
            if (stage8) {
                const uint4 *g_q4 = reinterpret_cast<const uint4 *>(shadow8 + tl.node * stride8);
                uint4 *d_q4 = d_h4 + (sv.hpitch >> 3);
                for (uint32_t i = threadIdx.x; i < (sv.pitch8 >> 3); i += blockDim.x) d_q4[i] = g_q4[i];  // both digits
            }
        }
        if (threadIdx.x == 0) s_left = 0;
        __syncthreads();
        const float *g_h = reinterpret_cast<const float *>(normals + tl.node * nstride + hdr_off);
        const LeafHdr nh = {g_h[0], g_h[1]};
        const NormalStats ns = *reinterpret_cast<const NormalStats *>(shadow + tl.node * hstride + (uint64_t)sv.hpitch * 2);
        NormalStats8 ns8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (stage8) ns8 = *reinterpret_cast<const NormalStats8 *>(shadow8 + tl.node * stride8 + 2 * (uint64_t)sv.pitch8);
        const uint32_t in_tile = min(kTile, nd->count - tl.first);
        const uint32_t *pp = perm + nd->start + tl.first;
        uint64_t mask = 0;
        uint32_t lefts = 0;
        // software pipeline of the int8 stage (PRE > 0): row index two items ahead, row chunks one item ahead
        constexpr int NPRE = PRE > 0 ? PRE : 1;
        uint4 xn[NPRE];
        uint32_t row_n = 0, row_nn = 0;
        if (PRE > 0 && stage8) {
            if (o < in_tile) row_n = pp[o];
            if (o + 32 < in_tile) row_nn = pp[o + 32];
            if (o < in_tile) {
                const uint4 *r8 = reinterpret_cast<const uint4 *>(sv.rows8 + (uint64_t)row_n * sv.pitch8) + j;
#pragma unroll
                for (int u = 0; u < NPRE; u++)
                    if ((uint32_t)u < steps8) xn[u] = ld_stream_u4(r8 + u * 8);
            }
        }
        for (uint32_t i = 0; i < 64; i++) {
            const uint32_t p = o + 32 * i;
            if (p >= in_tile) break;
            uint64_t row;
            uint4 x[NPRE];
            if (PRE > 0 && stage8) {
                row = row_n;
#pragma unroll
                for (int u = 0; u < NPRE; u++) x[u] = xn[u];
                row_n = row_nn;
                if (p + 64 < in_tile) row_nn = pp[p + 64];
                if (p + 32 < in_tile) {
                    const uint4 *r8n = reinterpret_cast<const uint4 *>(sv.rows8 + (uint64_t)row_n * sv.pitch8) + j;
#pragma unroll
                    for (int u = 0; u < NPRE; u++)
                        if ((uint32_t)u < steps8) xn[u] = ld_stream_u4(r8n + u * 8);
                }
            } else {
                row = pp[p];
            }
            uint32_t side = 0;
            bool decided = false;
            if (stage8) {  // first stage: the int8 copy, 768 bytes of a 768-d row; bound from the dataset-wide maxima
                const uint4 *r8 = reinterpret_cast<const uint4 *>(sv.rows8 + row * sv.pitch8) + j;
                const float s_row = METRIC == AH_COSINE ? 1.0f : sv.scale8_rows[row];  // a cosine margin's sign needs no scale
                const float u8 = PRE > 0 ? screen8_octet_dot_regs<NPRE>(s_q4 + j, s_ql4 + j, x, steps8)
                                         : screen8_octet_dot(s_q4 + j, s_ql4 + j, r8, steps8);
                decided = screen8_decides<METRIC>(u8 * ns8.scale, s_row, sv.max8, ns8, sv.gamma_r, side);
                met8++;
                decided8 += decided ? 1u : 0u;
                if (!decided && sv.rows8_lo != nullptr) {  // octet-uniform: the row's second int8 digit (768 more bytes)
                    const uint4 *r8l = reinterpret_cast<const uint4 *>(sv.rows8_lo + row * sv.pitch8) + j;
                    const float u8b = u8 + screen8_octet_dot(s_q4 + j, s_ql4 + j, r8l, steps8) * 0.00390625f;
                    decided = screen8_decides<METRIC>(u8b * ns8.scale, s_row, sv.max8b, ns8, sv.gamma_r, side);
                    decided8b += decided ? 1u : 0u;
                }
            }
            if (!decided) {  // octet-uniform: second stage, the binary16 copy
                const uint4 *r4 = reinterpret_cast<const uint4 *>(sv.rows + row * sv.hpitch) + j;
                const float s = screen_octet_dot(s_h4 + j, r4, steps);
                const float row_extra = METRIC == AH_DOT_PRODUCT ? dv.headers[2 * row] : 0.0f;
                // the bound from the dataset-wide maxima first (monotone in every stat, so it is >= the row's own bound);
                // the row's stats only when that one cannot decide
                decided = screen_decides<METRIC>(s, sv.max_stats, ns, row_extra, sv.gamma_s, sv.gamma_r, side);
                if (!decided) decided = screen_decides<METRIC>(s, sv.stats[row], ns, row_extra, sv.gamma_s, sv.gamma_r, side);
            }
            if (!decided || verify) {  // octet-uniform
                const uint32_t exact = side_of_margin(margin_f32<METRIC>(dv, s_n, nh, row, j));
                if (decided && exact != side) bad++;
                if (!decided) fallbacks++;
                side = exact;
            }
            mask |= (uint64_t)side << i;
            lefts += side ^ 1u;
        }
        if (j == 0) {
            masks[(uint64_t)tile * 32 + o] = mask;
            if (lefts) atomicAdd(&s_left, lefts);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            tile_left[tile] = s_left;
            if (s_left) atomicAdd(&nodes[tl.node].n_left, s_left);
        }
    }
    // statistics: one atomic per block
    __syncthreads();
    if (threadIdx.x == 0) s_fb = s_bad = s_n8 = s_d8 = s_d8b = 0;
    __syncthreads();
    if (j == 0 && fallbacks) atomicAdd(&s_fb, fallbacks);
    if (j == 0 && bad) atomicAdd(&s_bad, bad);
    if (j == 0 && met8) atomicAdd(&s_n8, met8);
    if (j == 0 && decided8) atomicAdd(&s_d8, decided8);
    if (j == 0 && decided8b) atomicAdd(&s_d8b, decided8b);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_fb) atomicAdd(&counters->fallbacks, (unsigned long long)s_fb);
        if (s_bad) atomicAdd(&counters->violations, (unsigned long long)s_bad);
        if (s_n8) atomicAdd(&counters->stage8_pairs, (unsigned long long)s_n8);
        if (s_d8) atomicAdd(&counters->stage8_decided, (unsigned long long)s_d8);
        if (s_d8b) atomicAdd(&counters->stage8b_decided, (unsigned long long)s_d8b);
    }
}

// exact margin of (row, normal record in global memory) by one octet: the arithmetic of k_forest_margin_rows
template <int METRIC>
__device__ __forceinline__ float rows_exact_margin(const DataView &dv, uint64_t row, const uint8_t *nrec, uint64_t hdr_off,
                                                   uint32_t j) {
    const float *rp = dv.rows_f32 + row * dv.pitch;
    const float *np = reinterpret_cast<const float *>(nrec);
    const float d = octet_reduce_stream<OP_DOT>(reinterpret_cast<const float4 *>(np), rp, dv.dims, j);
    const float *nh = reinterpret_cast<const float *>(nrec + hdr_off);
    if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN) return f_add(nh[0], d);
    if (METRIC == AH_DOT_PRODUCT) return f_add(d, f_mul(nh[0], dv.headers[2 * row]));
    return d;
}

// The same bits with every line of the row AND of the normal requested before the first multiply-add (octet_reduce_wide: two
// trips to memory per pair — node index, then both operands — instead of one per eight lines): k_forest_exact_pairs, whose waves
// spend their time between dependent loads (192 registers: for kernels that live on loads in flight, not on occupancy).
template <int METRIC>
__device__ __forceinline__ float rows_exact_margin_wide(const DataView &dv, uint64_t row, const uint8_t *nrec, uint64_t hdr_off,
                                                        uint32_t j) {
    const float *rp = dv.rows_f32 + row * dv.pitch;
    const float *np = reinterpret_cast<const float *>(nrec);
    const float *nh = reinterpret_cast<const float *>(nrec + hdr_off);
    float h0 = 0.0f, rh = 0.0f;
    if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN || METRIC == AH_DOT_PRODUCT) h0 = nh[0];
    if (METRIC == AH_DOT_PRODUCT) rh = dv.headers[2 * row];
    const float d = octet_reduce_wide<OP_DOT, false>(np, rp, dv.dims, j);  // (normal x row: the operand order of octet_reduce_stream above)
    if (METRIC == AH_EUCLIDEAN || METRIC == AH_MANHATTAN) return f_add(h0, d);
    if (METRIC == AH_DOT_PRODUCT) return f_add(d, f_mul(h0, rh));
    return d;
}

#ifndef AH_SCREEN_CHUNK
#define AH_SCREEN_CHUNK 8
#endif
// NS steps (64 dims each) of one row against the normals of TC trees.  Branch-free over the trees (a row that is already
// a leaf in tree t reads record 0 for nothing): the loads of a tree's NS chunks are issued together and the compiler is
// free to run ahead into the next trees, so a wave keeps dozens of 16-byte loads in flight.
template <int TC, int NS>
__device__ __forceinline__ void screen_rows_chunk(float (&acc)[TC], const uint4 *base4, const uint32_t (&noff)[TC],
                                                  const uint4 *r4, uint32_t k, bool nt_rows = false) {
    uint4 x[NS];
    if (nt_rows) {
#pragma unroll
        for (int u = 0; u < NS; u++) x[u] = ld_stream_u4(r4 + (k + u) * 8);
    } else {
#pragma unroll
        for (int u = 0; u < NS; u++) x[u] = r4[(k + u) * 8];  // cached on purpose: the other tree groups re-read the chunk
    }
#pragma unroll
    for (int t = 0; t < TC; t++) {
        const uint4 *np = base4 + noff[t] + k * 8;
        uint4 nv[NS];
#pragma unroll
        for (int u = 0; u < NS; u++) nv[u] = np[u * 8];
        float a0 = acc[t], a1 = 0.f;
#pragma unroll
        for (int u = 0; u < NS; u += 2) {
            a0 = screen_dot8(nv[u], x[u], a0);
            a1 = screen_dot8(nv[u + 1], x[u + 1], a1);
        }
        acc[t] = a0 + a1;
    }
}

// Row-major pass with the screen.  LDS_NORMALS: the shadow records of the group's nodes [first_node, +n_group_nodes) are
// resident in LDS (top levels); otherwise they come from L2.  The f32 normals (fallback) always come from global memory.
// The loads of a tree's 8 normal chunks are issued together, ahead of the 32 dot2c that consume them (two independent
// accumulation chains): the pass is bound by the vector-memory pipeline, so what matters is how many loads a wave keeps
// in flight, not the arithmetic.
#ifndef AH_SCREEN_WAVES
#define AH_SCREEN_WAVES 1  // minimum waves per SIMD the compiler must leave room for (caps the VGPRs of the global variant)
#endif
// Schedule of a launch: ONE launch serves `n_groups` groups of TC trees (tree0 + g * TC ...) and blocks are numbered
// chunk-major — block b works on rows [chunk * chunk_rows + tile * rows_per_block, ...) of group g with
// chunk = b / (n_groups * tiles), g = (b / tiles) % n_groups, tile = b % tiles — so the passes of all groups over one chunk
// of rows (48 MB of binary16 rows) run back to back and every pass but the first finds the chunk in the 256 MB Infinity
// Cache (which is also why the blocks must be launched one per work item: a grid-stride loop lets the blocks drift apart,
// the window of rows in flight spreads over many chunks and the pass takes 1.5-2x as long; bigger blocks — 128 / 512 rows —
// lose 20-60 %).  Measured on the pass in isolation (scripts/micro/rows_pass_model.hip): a pass costs the L2 gather of its normals
// PLUS ~4.6 ms of HBM-latency-bound row stream (11.9 ms for 16 trees, 10M rows); with the rows coming from the Infinity
// Cache 9.1-9.6 ms; 7.8 ms if they came from L2.  The row loads must be ordinary cached loads for that (non-temporal
// ones do not stay: 11.1 ms).  group_nodes (LDS variant): first node of every tree in the level, nodes ordered by tree.
struct RowsSchedule {
    uint32_t n_groups, tiles, chunk_rows, rows_per_block;
    uint32_t xcd_slots;  // 0: every (chunk, group) is spread over all XCDs; k > 0: one XCD per (chunk, group), k groups per XCD
                         // (bit 31: stream the rows with non-temporal loads)
    uint32_t chunk0;     // first chunk of this launch (a launch is limited to 2^32 work-items, so big levels take several)
    const uint32_t *tree_first;  // LDS variant: device copy of tree_first[n_trees + 1]
};
// block -> (group, rows) of a row-major launch; false when the block has nothing to do.  Shared by the margin kernel and
// by k_rows_schedule_coverage (the test that every (group, row) pair is served exactly once runs THIS function on the
// device, with the grids plan_rows_launches hands the build).
__device__ __forceinline__ bool rows_block_map(const RowsSchedule &sch, uint32_t b, uint64_t n_rows, uint32_t &group,
                                               uint64_t &row_begin, uint64_t &row_end) {
    uint32_t chunk, tile;
    if (sch.xcd_slots & 0x7FFFFFFFu) {
        // One XCD per (chunk, group): workgroups go to the XCDs round-robin (block b -> XCD b & 7), so XCD x takes, for
        // chunk c, the groups g = ((x - c) mod 8) + 8 k — the rotation by c evens out n_groups mod 8 over the chunks.  An
        // XCD's L2 (4 MiB) then holds the normals of ONE group next to the row stream instead of those of the two
        // groups that are in flight at any time when every group is spread over all eight.
        const uint32_t x = b & 7u, slot = b >> 3;
        const uint32_t per_chunk = (sch.xcd_slots & 0x7FFFFFFFu) * sch.tiles;
        chunk = sch.chunk0 + slot / per_chunk;
        const uint32_t rem = slot % per_chunk;
        tile = rem % sch.tiles;
        group = ((x + 8u - (chunk & 7u)) & 7u) + 8u * (rem / sch.tiles);
        if (group >= sch.n_groups) return false;
    } else {
        const uint32_t per_chunk = sch.n_groups * sch.tiles;
        chunk = sch.chunk0 + b / per_chunk;
        const uint32_t in_chunk = b % per_chunk;
        group = in_chunk / sch.tiles;
        tile = in_chunk % sch.tiles;
    }
    row_begin = (uint64_t)chunk * sch.chunk_rows + (uint64_t)tile * sch.rows_per_block;
    row_end = min(min(row_begin + sch.rows_per_block, (uint64_t)(chunk + 1) * sch.chunk_rows), n_rows);
    return row_begin < row_end;
}
// test aid (ah_debug_launch_coverage): counts[group * n_rows + row] += 1 for every row the block would serve
__global__ void k_rows_schedule_coverage(RowsSchedule sch, uint64_t n_rows, uint32_t *__restrict__ counts) {
    uint32_t group;
    uint64_t row_begin, row_end;
    if (!rows_block_map(sch, blockIdx.x, n_rows, group, row_begin, row_end)) return;
    for (uint64_t row = row_begin + (threadIdx.x >> 3); row < row_end; row += blockDim.x >> 3)
        if ((threadIdx.x & 7u) == 0) atomicAdd(&counts[(uint64_t)group * n_rows + row], 1u);
}

template <int METRIC, int TC, bool LDS_NORMALS>
__global__ __launch_bounds__(LDS_NORMALS ? (TC >= 16 ? 512 : 1024) : kBlock,
                             LDS_NORMALS ? 1 : (AH_SCREEN_WAVES > 1 ? AH_SCREEN_WAVES : (TC == 8 ? 4 : 1))) void k_forest_screen_rows(
    DataView dv, ScreenView sv, const uint32_t *__restrict__ node_of, uint32_t tree_base, uint32_t n_pass,
    const uint8_t *__restrict__ normals, uint64_t nstride, uint64_t hdr_off, const uint8_t *__restrict__ shadow,
    uint64_t hstride, uint8_t *__restrict__ side_bytes, RowsSchedule sch, const AbortFlags abort_flag,
    ScreenCounters *__restrict__ counters, uint32_t verify) {
    extern __shared__ uint4 s_shadow4[];
    __shared__ uint32_t s_fb, s_bad;
    if (abort_requested(abort_flag)) return;
    uint32_t group;
    uint64_t row_begin, row_end;
    if (!rows_block_map(sch, blockIdx.x, dv.n, group, row_begin, row_end)) return;  // block-uniform
    const uint32_t tree0 = tree_base + group * TC;
    const uint32_t hstride4 = (uint32_t)(hstride >> 4);
    uint32_t first_node = 0;
    if (LDS_NORMALS) {
        first_node = sch.tree_first[tree0];
        const uint32_t n_group_nodes = sch.tree_first[tree0 + n_pass] - first_node;
        const uint4 *g = reinterpret_cast<const uint4 *>(shadow + (uint64_t)first_node * hstride);
        const uint32_t total = n_group_nodes * hstride4;
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) s_shadow4[i] = g[i];
    }
    if (threadIdx.x == 0) s_fb = s_bad = 0;
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    const uint32_t octets = blockDim.x >> 3;
    const uint32_t steps = sv.hpitch >> 6;
    const uint32_t stats4 = sv.hpitch >> 3;  // uint4 index of the NormalStats inside a shadow record
    // all shadow records of the level, as uint4: LDS copy of the group or the global chunk (32-bit indices either way)
    const uint4 *base4 = LDS_NORMALS ? s_shadow4 : reinterpret_cast<const uint4 *>(shadow);
    const uint32_t node0 = first_node;
    const uint32_t last_tree = n_pass - 1;
    constexpr int N = TC >= 8 ? 8 : TC;        // trees per transposing reduction
    constexpr int SETS = TC >= 8 ? TC / 8 : 1;  // sets of N trees
    const uint32_t my_t = octet_owned_tree<N>(j);
    const bool owner = octet_is_owner<N>(j);
    uint32_t fallbacks = 0, bad = 0;
    for (uint64_t row = row_begin + (threadIdx.x >> 3); row < row_end; row += octets) {
        const uint4 *r4 = reinterpret_cast<const uint4 *>(sv.rows + row * sv.hpitch) + j;
        // Lane j owns tree octet_owned_tree(j) of each set of 8 trees: it loads that tree's node index (one load instruction
        // for 8 trees), broadcasts it to the octet, and later runs the tree's epilogue.  n_pass == TC except for the last
        // trees of a forest: spare slots repeat the last tree and are not stored.
        uint32_t my_node[SETS];
        uint32_t noff[TC];  // uint4 index of (record of the node that owns the row in tree t) + j
        float acc[TC];
#pragma unroll
        for (int st = 0; st < SETS; st++)
            my_node[st] = node_of[(uint64_t)(tree0 + min(my_t + 8u * st, last_tree)) * dv.n + row];
#pragma unroll
        for (int t = 0; t < TC; t++) {
            const uint32_t node = (uint32_t)__shfl((int)my_node[t / 8], (int)octet_owner_lane<N>(t % 8), 8);
            noff[t] = (node != 0xFFFFFFFFu ? node - node0 : 0u) * hstride4 + j;
            acc[t] = 0.f;
        }
        // chunks of AH_SCREEN_CHUNK steps (64 dims each), then of 4, then single steps.  Measured on 10M x 768 (12 steps):
        // 8 + 4 beats a single chunk of 12 (the extra 16 row registers cost a wave of occupancy per SIMD: 7.7 -> 10.8 ms
        // per 8-tree pass).
        uint32_t k = 0;
        const bool nt_rows = (sch.xcd_slots & 0x80000000u) != 0;
        for (; k + AH_SCREEN_CHUNK <= steps; k += AH_SCREEN_CHUNK) screen_rows_chunk<TC, AH_SCREEN_CHUNK>(acc, base4, noff, r4, k, nt_rows);
#if AH_SCREEN_CHUNK > 4
        if (k + 4 <= steps) {
            screen_rows_chunk<TC, 4>(acc, base4, noff, r4, k, nt_rows);
            k += 4;
        }
#endif
        for (; k < steps; k++) {
            const uint4 x = r4[k * 8];
#pragma unroll
            for (int t = 0; t < TC; t++) acc[t] = screen_dot8(base4[noff[t] + k * 8], x, acc[t]);
        }
        // Epilogue, once per tree on its owner lane: total of the octet (transposing reduction), error bound, decision.
        // Pairs the screen cannot decide are recomputed in the reference arithmetic by the whole octet.
        const float4 rs = sv.stats[row];
        const float row_extra = METRIC == AH_DOT_PRODUCT ? dv.headers[2 * row] : 0.0f;
#pragma unroll
        for (int st = 0; st < SETS; st++) {
            const float total = octet_transpose_sum<N>(acc + 8 * st, j);
            const uint32_t t = my_t + 8u * st;
            const bool valid = owner && t <= last_tree && my_node[st] != 0xFFFFFFFFu;
            uint32_t side = 0;
            bool decided = false;
            if (valid) {
                const uint4 raw = base4[(my_node[st] - node0) * hstride4 + stats4];
                NormalStats ns;
                ns.an = __uint_as_float(raw.x);
                ns.bn = __uint_as_float(raw.y);
                ns.cn = __uint_as_float(raw.z);
                ns.extra = __uint_as_float(raw.w);
                decided = screen_decides<METRIC>(total, rs, ns, row_extra, sv.gamma_s, sv.gamma_r, side);
            }
            const unsigned long long und = __ballot(valid && (!decided || verify));
            const uint32_t mask8 = (uint32_t)(und >> (8u * ((threadIdx.x & 63u) >> 3))) & 0xFFu;
            if (mask8) {  // octet-uniform, ~8 % of the (octet, set) pairs
#pragma unroll
                for (int tt = 0; tt < N; tt++) {
                    constexpr uint32_t kOwner[8] = {octet_owner_lane<N>(0), octet_owner_lane<N>(1), octet_owner_lane<N>(2),
                                                    octet_owner_lane<N>(3), octet_owner_lane<N>(4), octet_owner_lane<N>(5),
                                                    octet_owner_lane<N>(6), octet_owner_lane<N>(7)};
                    const uint32_t ol = kOwner[tt];
                    if ((mask8 >> ol) & 1u) {
                        const uint32_t node = (noff[8 * st + tt] - j) / hstride4 + node0;
                        const uint32_t exact =
                            side_of_margin(rows_exact_margin<METRIC>(dv, row, normals + (uint64_t)node * nstride, hdr_off, j));
                        if (j == ol) {
                            if (decided && exact != side) bad++;
                            if (!decided) fallbacks++;
                            side = exact;
                        }
                    }
                }
            }
            if (valid) side_bytes[(uint64_t)(tree0 + t) * dv.n + row] = (uint8_t)side;
        }
    }
    if (fallbacks) atomicAdd(&s_fb, fallbacks);
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_fb) atomicAdd(&counters->fallbacks, (unsigned long long)s_fb);
        if (s_bad) atomicAdd(&counters->violations, (unsigned long long)s_bad);
    }
}

// ------------------------------------------------------------------------------------------------
// The next level, built on the device: children of every split node that are still too large for a Descendants node
// (src/writer.rs:474-477) become the next level's nodes, in node order, left child first — the order the host used to
// produce.  Three small kernels (count per block, scan of the block sums, emit) plus the tile list; the host reads back
// only the LevelInfo block before it launches the level, the node tables follow asynchronously for the final node list.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void child_counts(const FNode &nd, uint32_t split_after, uint32_t cnt[2], uint32_t split[2]) {
    cnt[0] = nd.n_left;
    cnt[1] = nd.count - nd.n_left;
    split[0] = cnt[0] > split_after ? 1u : 0u;
    split[1] = cnt[1] > split_after ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_next_count(const FNode *__restrict__ nodes, uint32_t n_nodes, uint32_t split_after,
                                                    NextCounts *__restrict__ block_sums) {
    __shared__ uint32_t s_k[4], s_t[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t kids = 0, tiles = 0;
    if (i < n_nodes) {
        uint32_t cnt[2], sp[2];
        child_counts(nodes[i], split_after, cnt, sp);
        kids = sp[0] + sp[1];
        tiles = sp[0] * ((cnt[0] + kTile - 1) / kTile) + sp[1] * ((cnt[1] + kTile - 1) / kTile);
    }
    for (int off = 32; off > 0; off >>= 1) {
        kids += __shfl_xor(kids, off);
        tiles += __shfl_xor(tiles, off);
    }
    if ((threadIdx.x & 63u) == 0) {
        s_k[threadIdx.x >> 6] = kids;
        s_t[threadIdx.x >> 6] = tiles;
    }
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = NextCounts{s_k[0] + s_k[1] + s_k[2] + s_k[3], s_t[0] + s_t[1] + s_t[2] + s_t[3]};
}
// exclusive scan of the block sums in place (one block; n_blocks <= a few thousand) + the level totals
__global__ __launch_bounds__(1024) void k_next_scan(NextCounts *__restrict__ block_sums, uint32_t n_blocks,
                                                    LevelInfo *__restrict__ info, uint32_t *__restrict__ tree_first,
                                                    uint32_t n_trees, uint32_t *__restrict__ pend) {
    __shared__ uint32_t s_k[16], s_t[16];
    __shared__ uint32_t s_carry_k, s_carry_t;
    if (threadIdx.x == 0) s_carry_k = s_carry_t = 0;
    if (threadIdx.x < 3) pend[threadIdx.x] = 0;  // the level's attempts are over: the next level counts its own pending nodes
    for (uint32_t t = threadIdx.x; t <= n_trees; t += blockDim.x) tree_first[t] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n_blocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const NextCounts v = i < n_blocks ? block_sums[i] : NextCounts{0u, 0u};
        uint32_t ik = v.kids, it = v.tiles;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t uk = __shfl_up(ik, off), ut = __shfl_up(it, off);
            if ((int)lane >= off) {
                ik += uk;
                it += ut;
            }
        }
        if (lane == 63) {
            s_k[wave] = ik;
            s_t[wave] = it;
        }
        __syncthreads();
        uint32_t wk = 0, wt = 0;
        for (uint32_t w = 0; w < wave; w++) {
            wk += s_k[w];
            wt += s_t[w];
        }
        const uint32_t ck = s_carry_k, ct = s_carry_t;
        if (i < n_blocks) block_sums[i] = NextCounts{ck + wk + ik - v.kids, ct + wt + it - v.tiles};
        __syncthreads();
        if (threadIdx.x == 1023) {
            s_carry_k = ck + wk + ik;
            s_carry_t = ct + wt + it;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        info->n_nodes = s_carry_k;
        info->n_tiles = s_carry_t;
        info->n_fix = 0;
        info->pairs = 0;
    }
}
__global__ __launch_bounds__(256) void k_next_emit(const FNode *__restrict__ nodes, uint32_t n_nodes, uint32_t split_after,
                                                   const NextCounts *__restrict__ block_sums, FNode *__restrict__ next,
                                                   uint32_t *__restrict__ child, LevelInfo *__restrict__ info,
                                                   uint32_t *__restrict__ tree_first) {
    __shared__ uint32_t s_k[4], s_t[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    FNode nd{};
    uint32_t cnt[2] = {0, 0}, sp[2] = {0, 0};
    if (i < n_nodes) {
        nd = nodes[i];
        child_counts(nd, split_after, cnt, sp);
    }
    const uint32_t kids = sp[0] + sp[1];
    const uint32_t nt[2] = {sp[0] * ((cnt[0] + kTile - 1) / kTile), sp[1] * ((cnt[1] + kTile - 1) / kTile)};
    uint32_t ik = kids, it = nt[0] + nt[1];
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t uk = __shfl_up(ik, off), ut = __shfl_up(it, off);
        if ((int)lane >= off) {
            ik += uk;
            it += ut;
        }
    }
    if (lane == 63) {
        s_k[wave] = ik;
        s_t[wave] = it;
    }
    __syncthreads();
    uint32_t idx = block_sums[blockIdx.x].kids + ik - kids, tidx = block_sums[blockIdx.x].tiles + it - (nt[0] + nt[1]);
    for (uint32_t w = 0; w < wave; w++) {
        idx += s_k[w];
        tidx += s_t[w];
    }
    if (i >= n_nodes) return;
    // sides of a first-attempt accept are the ones a row-major pass left in side_bytes; anything else was re-drawn
    const uint32_t fix = (nd.state == ST_ACCEPTED && nd.attempt == 0) ? 0u : 1u;
    unsigned long long pairs = 0;
    uint32_t n_fix = 0;
    for (uint32_t side = 0; side < 2; side++) {
        uint32_t link = 0xFFFFFFFFu;
        if (sp[side]) {
            FNode cn{};
            cn.key = ah_node_key_child(nd.key, side);
            cn.start = side ? nd.start + nd.n_left : nd.start;
            cn.tree = nd.tree;
            cn.count = cnt[side];
            cn.tile_begin = tidx;
            cn.n_tiles = nt[side];
            cn.fix = fix;
            next[idx] = cn;
            if (!fix) link = idx;
            atomicMin(&tree_first[nd.tree], idx);
            pairs += cnt[side];
            n_fix += fix;
            idx++;
            tidx += nt[side];
        }
        child[2 * (uint64_t)i + side] = link;
    }
    if (pairs) atomicAdd(&info->pairs, pairs);
    if (n_fix) atomicAdd(&info->n_fix, n_fix);
}
// A level cut into groups of trees (BatchBuild::run_tail_groups): per group the tiles and the items under its nodes, and its
// nodes' tile indices rebased to the group's first tile — from there on the group is a level of its own over the shared
// tile tables.  One block per group; nodes [first[g], first[g + 1]) of the level's table.
struct GroupCuts {
    uint32_t first[33];
};
struct GroupInfo {
    uint32_t n_tiles, n_fix;
    unsigned long long pairs;
};
__global__ __launch_bounds__(256) void k_fork_groups(FNode *__restrict__ nodes, GroupCuts cuts, GroupInfo *__restrict__ out) {
    __shared__ unsigned long long s_pairs[4];
    __shared__ uint32_t s_fix[4];
    const uint32_t lo = cuts.first[blockIdx.x], hi = cuts.first[blockIdx.x + 1];
    uint32_t t0 = 0, t1 = 0;
    if (hi > lo) {
        t0 = nodes[lo].tile_begin;
        t1 = nodes[hi - 1].tile_begin + nodes[hi - 1].n_tiles;
    }
    __syncthreads();  // every thread holds the first tile before the first node is rebased
    unsigned long long pairs = 0;
    uint32_t fix = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
        pairs += nodes[i].count;
        fix += nodes[i].fix;
        nodes[i].tile_begin -= t0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        pairs += __shfl_xor(pairs, off);
        fix += __shfl_xor(fix, off);
    }
    if ((threadIdx.x & 63u) == 0) {
        s_pairs[threadIdx.x >> 6] = pairs;
        s_fix[threadIdx.x >> 6] = fix;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        out[blockIdx.x] = GroupInfo{t1 - t0, s_fix[0] + s_fix[1] + s_fix[2] + s_fix[3], s_pairs[0] + s_pairs[1] + s_pairs[2] + s_pairs[3]};
}
// tile list of a level: one wave per node
__global__ __launch_bounds__(256) void k_build_tiles(const FNode *__restrict__ nodes, uint32_t n_nodes,
                                                     FTile *__restrict__ tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4;
    for (uint32_t node = blockIdx.x * 4 + (threadIdx.x >> 6); node < n_nodes; node += n_waves) {
        const uint32_t begin = nodes[node].tile_begin, nt = nodes[node].n_tiles;
        for (uint32_t t = lane; t < nt; t += 64) tiles[begin + t] = FTile{node, t * kTile};
    }
}

}  // namespace ah

#include "dense_device.h"

using namespace ah;

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// ---- host memory of the forests' blobs, recycled --------------------------------------------------------------------
// A 10M x 768 x 100-tree forest is 5.4 GB of normals + 4 GB of item ids.  Handing every build FRESH pageable memory means
// 2.3 M first-touch page faults per build, taken by a dozen threads of one process that contend for the address-space lock
// with each other and with the HIP runtime's own mappings — measured: 8 threads commit 4 KiB pages at 1.3 GB/s in total,
// 2 threads at 4.9, and the round-3 driver run saw the same build take 1.47 .. 1.82 s.  So: (1) blobs are mapped with
// MADV_HUGEPAGE on 2 MiB boundaries (512x fewer faults where transparent huge pages are available: 7.3 GB/s on 8 threads),
// and (2) the blobs of a destroyed forest are KEPT, committed, in a process-wide pool and handed to the next build, which
// then faults nothing at all.  AH_HOST_CACHE_MB bounds what the pool holds (0 = recycle nothing); ah_host_cache_trim
// returns it to the system.
struct HostBlob {
    uint8_t *p = nullptr;
    size_t cap = 0;        // usable bytes at p
    size_t committed = 0;  // bytes from p whose pages have been written before (a recycled blob): nothing to fault there
    bool recycled = false; // came out of the pool (HostBlobPool::take), not from a fresh mapping
    void *map = nullptr;   // the mapping p lives in (nullptr: malloc'd — small blobs)
    size_t map_len = 0;
    int node = -1;         // host NUMA node its pages prefer (-1: none asked for)
};
// the host node of the device whose build is running on this thread (BatchBuild::setup_host sets it): what fresh blobs prefer, and what
// the pool matches recycled blobs against
static thread_local int tl_blob_node = -1;
class HostBlobPool {
    std::mutex mu;
    std::vector<HostBlob> idle;
    size_t held = 0;  // committed bytes of the idle blobs
    static constexpr size_t kSmall = 16u << 20, kHuge = 2u << 20;
    static void release(HostBlob &b) {
        if (b.map) munmap(b.map, b.map_len);
        else free(b.p);
        b = HostBlob{};
    }

  public:
    // a blob of at least `bytes` bytes; false = out of memory
    bool take(size_t bytes, HostBlob *out) {
        bytes += 16;
        if (bytes >= kSmall) {
            std::lock_guard<std::mutex> lk(mu);
            size_t best = idle.size();
            // the smallest blob that fits, and never one more than twice the size asked for: a 20 MB request must not walk off
            // with the 5 GB blob the next big build is counting on
            // ... of those on the asking device's host node first (a blob committed on the far socket halves the rate its copy
            // threads reach), then of the others
            for (int pass = 0; pass < 2 && best == idle.size(); pass++)
                for (size_t i = 0; i < idle.size(); i++) {
                    if (pass == 0 && tl_blob_node >= 0 && idle[i].node != tl_blob_node) continue;
                    if (idle[i].cap >= bytes && idle[i].cap <= 2 * bytes + kHuge && (best == idle.size() || idle[i].cap < idle[best].cap))
                        best = i;
                }
            if (best != idle.size()) {
                *out = idle[best];
                out->recycled = true;
                held -= std::min(held, idle[best].committed);
                idle.erase(idle.begin() + (ptrdiff_t)best);
                return true;
            }
        }
        if (fail_alloc_tick()) return false;
        HostBlob b;
        if (bytes < kSmall) {
            b.p = reinterpret_cast<uint8_t *>(malloc(bytes));
            if (!b.p) return false;
            b.cap = bytes;
        } else {
            const size_t cap = (bytes + kHuge - 1) & ~(kHuge - 1);
            void *m = mmap(nullptr, cap + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
            if (m == MAP_FAILED) return false;
            b.map = m;
            b.map_len = cap + kHuge;
            b.p = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(m) + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
            b.cap = cap;
            (void)madvise(b.p, cap, MADV_HUGEPAGE);  // a hint: 4 KiB pages where it is refused
            // the pages prefer the host node of the device whose build asks (api.hip "NUMA placement"; tl_blob_node < 0: wherever
            // they are first touched)
            numa_prefer_node(b.p, cap, tl_blob_node);
            b.node = tl_blob_node;
        }
        *out = b;
        return true;
    }
    void give(HostBlob &b, size_t used) {
        if (!b.p) return;
        NoFailScope no_fail;
        b.committed = std::min(b.cap, std::max(b.committed, used));
        const size_t limit = (size_t)std::max<long long>(0, tun(TUN_HOST_CACHE_MB)) << 20;
        if (!b.map || limit == 0) {
            release(b);
            return;
        }
        std::lock_guard<std::mutex> lk(mu);
        idle.push_back(b);
        held += b.committed;
        b = HostBlob{};
        while (held > limit && !idle.empty()) {  // over the budget: the oldest go first
            held -= std::min(held, idle.front().committed);
            release(idle.front());
            idle.erase(idle.begin());
        }
    }
    size_t trim() {
        NoFailScope no_fail;
        std::lock_guard<std::mutex> lk(mu);
        const size_t was = held;
        for (HostBlob &b : idle) release(b);
        idle.clear();
        held = 0;
        return was;
    }
};
static HostBlobPool &host_pool() {
    static HostBlobPool *pool = new HostBlobPool();  // never destroyed: forests may outlive static destruction order
    return *pool;
}
static size_t records_pool_trim();  // (the node records of the last build, below)
namespace ah {
size_t host_cache_trim() { return host_pool().trim() + records_pool_trim() + pinned_spare_trim(); }
}  // namespace ah
// grow `blob` to at least `need` bytes keeping its first `keep` bytes; the old mapping goes back to the pool
static bool host_blob_reserve(HostBlob &blob, size_t need, size_t keep) {
    if (need + 16 <= blob.cap) return true;
    HostBlob grown;
    if (!host_pool().take(need, &grown)) return false;
    if (keep) memcpy(grown.p, blob.p, keep);
    grown.committed = std::max(grown.committed, keep);
    host_pool().give(blob, keep);
    blob = grown;
    return true;
}

struct ah_forest {
    std::vector<uint32_t> roots;
    std::vector<ah_node> nodes;
    HostBlob normals_blob, desc_blob;  // raw buffers: filled by D2H copies only, never repacked; recycled (HostBlobPool)
    uint8_t *normals = nullptr;        // = normals_blob.p
    uint64_t normals_len = 0;
    uint32_t *descendants = nullptr;   // = desc_blob.p
    uint64_t descendants_len = 0;
    uint64_t normal_stride = 0, normal_vector_offset = 0, normal_header_offset = 0;
    ah_build_stats stats{};
    // A resident forest (ah_build_forest_resident / ah_build_subtrees_resident): next to the host content, the arrays an index
    // of this forest holds, on the device it was built on.  want_device: the build is to leave them (cleared when it cannot);
    // has_device: the build is over and they are complete — until ah_forest_release_device or an index call that consumes them.
    ForestDevice dev;
    uint32_t dev_rows_cap = 0;
    bool want_device = false, has_device = false;
    void release_device(bool keep_ids = false, bool keep_rows = false) {
        NoFailScope no_fail;
        if ((dev.ids && !keep_ids) || ((dev.rows || dev.hdrs) && !keep_rows)) {
            DeviceRestore restore_device;
            if (dev.device >= 0) (void)hipSetDevice(dev.device);
            if (dev.ids && !keep_ids) (void)dev_free(dev.ids);
            if (dev.rows && !keep_rows) (void)dev_free(dev.rows);
            if (dev.hdrs && !keep_rows) (void)dev_free(dev.hdrs);
        }
        dev = ForestDevice{};
        dev_rows_cap = 0;
        want_device = has_device = false;
    }
    ~ah_forest() {
        release_device();
        host_pool().give(normals_blob, normals_len);
        host_pool().give(desc_blob, descendants_len * 4);
    }
};

namespace {

// The records of a build and their index vector, kept for the next build of the process like the forests' blobs (and under
// the same switch, AH_HOST_CACHE_MB; ah_host_cache_trim frees them): 136 MB + 14 MB at 10M x 100 trees, whose fresh pages
// used to be faulted in under the levels by the launching thread and unmapped — 11 ms — between the last copy and the return.
struct RecordsPool {
    std::mutex mu;
    std::vector<HostRec> recs;
    std::vector<uint32_t> index;
};
static RecordsPool &records_pool() {
    static RecordsPool *pool = new RecordsPool();  // never destroyed (see host_pool)
    return *pool;
}
struct RecordsLease {  // takes the pooled vectors for one batch and gives the larger ones back
    std::vector<HostRec> &recs;
    std::vector<uint32_t> &index;
    RecordsLease(std::vector<HostRec> &r, std::vector<uint32_t> &i) : recs(r), index(i) {
        if (tun(TUN_HOST_CACHE_MB) <= 0) return;
        RecordsPool &pool = records_pool();
        std::lock_guard<std::mutex> lk(pool.mu);
        recs.swap(pool.recs);
        index.swap(pool.index);
        recs.clear();
        index.clear();
    }
    ~RecordsLease() {
        if (tun(TUN_HOST_CACHE_MB) <= 0) return;
        RecordsPool &pool = records_pool();
        std::lock_guard<std::mutex> lk(pool.mu);
        if (recs.capacity() > pool.recs.capacity()) recs.swap(pool.recs);
        if (index.capacity() > pool.index.capacity()) index.swap(pool.index);
    }
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return AH_OK;
        if (p) AH_HIP(dev_free(p));
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)1024);
        AH_HIP(dev_malloc((void **)&p, want * sizeof(T)));
        cap = want;
        return AH_OK;
    }
    void release() {
        if (p) (void)dev_free(p);
        p = nullptr;
        cap = 0;
    }
    ~DevBuf() { release(); }
};

// Device memory for the normal records of all levels of a batch: a few big blocks handed out level by level (a level's
// records are contiguous), so that a level costs no hipMalloc.  Everything is freed when the batch ends.
struct Arena {
    std::vector<void *> blocks;
    uint8_t *cur = nullptr;
    size_t left = 0, block_bytes = 0;
    int take(size_t bytes, uint8_t **out) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes > left) {
            size_t got = std::max(bytes, block_bytes);
            void *p = nullptr;
            blocks.reserve(blocks.size() + 1);  // (may throw: BEFORE the block exists, so that it cannot be lost)
            hipError_t e = dev_malloc(&p, got);
            if (e != hipSuccess && got > bytes) {  // tight on memory: exactly this level
                (void)hipGetLastError();
                got = bytes;
                e = dev_malloc(&p, got);
            }
            if (e != hipSuccess) {
                set_error("hipMalloc of %zu bytes of normals failed: %s", bytes, hipGetErrorString(e));
                return e == hipErrorOutOfMemory ? AH_ERR_OUT_OF_MEMORY : AH_ERR_DEVICE;
            }
            blocks.push_back(p);
            cur = reinterpret_cast<uint8_t *>(p);
            left = got;
        }
        *out = cur;
        cur += bytes;
        left -= bytes;
        return AH_OK;
    }
    ~Arena() {
        for (void *p : blocks) (void)dev_free(p);
    }
};

// Measurement and test aids: the tunables of common.h (environment variable at load time, ah_tuning_set at run time).
// The per-call knob is ah_build_options.margin_mode; the tunables only steer AH_MARGIN_AUTO and the schedule of a level.
// None of them changes a result.
#define AH_DBG(s, what)                                                       \
    do {                                                                      \
        if (tun(TUN_DEBUG)) {                                                 \
            hipError_t _e = hipStreamSynchronize(s);                          \
            fprintf(stderr, "[ah] %s: %s\n", what, hipGetErrorString(_e));    \
            fflush(stderr);                                                   \
        }                                                                     \
    } while (0)

struct BatchCleanup {  // events / side stream of one batch
    hipEvent_t ev_attempt[8] = {};  // begin / end of the margin pass of attempts 0..3, re-used by every level
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_level = nullptr, ev_copy[2] = {nullptr, nullptr};
    hipStream_t side = nullptr;
    int create() {
        for (hipEvent_t &e : ev_attempt) AH_HIP(hipEventCreate(&e));
        AH_HIP(hipEventCreate(&ev_begin));
        AH_HIP(hipEventCreate(&ev_end));
        AH_HIP(hipEventCreateWithFlags(&ev_level, hipEventDisableTiming));
        AH_HIP(hipEventCreateWithFlags(&ev_copy[0], hipEventDisableTiming));
        AH_HIP(hipEventCreateWithFlags(&ev_copy[1], hipEventDisableTiming));
        AH_HIP(create_copy_stream(&side));  // (node tables, the abort word, a group's rows -> ids: under the level's kernels)
        return AH_OK;
    }
    ~BatchCleanup() {
        if (side) (void)hipStreamSynchronize(side);
        for (hipEvent_t e : ev_attempt)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_begin, ev_end, ev_level, ev_copy[0], ev_copy[1]})
            if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
};

// index into ah_build_stats.margin_mode_launches
enum { MM_NODE = 0, MM_ROWS2 = 1, MM_ROWS4 = 2, MM_ROWS8 = 3, MM_ROWS16 = 4, MM_LDS8 = 5, MM_LDS16 = 6, MM_BQ = 7 };
inline int mm_rows(uint32_t tc) { return tc >= 16 ? MM_ROWS16 : tc == 8 ? MM_ROWS8 : tc == 4 ? MM_ROWS4 : MM_ROWS2; }

}  // namespace

// Size of a normal record [vector, row_bytes][header, 16-byte slot][padding].  For the f32 metrics it is rounded up to
// whole 128-byte lines (768-d: 3088 -> 3200 bytes; the binary16 shadow records likewise, 1552 -> 1664): the row-major
// passes gather normals as 128-byte pieces, one per octet and load instruction, and a piece that straddles two lines
// costs the L1 three 64-byte accesses instead of two — measured with TCP_TOTAL_CACHE_ACCESSES, that was 6.1e9 accesses
// per 16-tree pass against 4.1e9 useful, in a pass that runs at ~80 % of the L1's access rate.  Callers see the stride
// in ah_forest_view.normal_stride.
static size_t records_pool_trim() {
    RecordsPool &pool = records_pool();
    std::vector<HostRec> r;
    std::vector<uint32_t> i;
    {
        std::lock_guard<std::mutex> lk(pool.mu);
        r.swap(pool.recs);
        i.swap(pool.index);
    }
    return r.capacity() * sizeof(HostRec) + i.capacity() * sizeof(uint32_t);
}
static uint64_t normal_record_stride(const ah_dataset *ds) {
    const uint64_t raw = ds->row_bytes() + 16;
    return metric_is_bq(ds->metric) ? raw : (raw + 127) & ~(uint64_t)127;
}

// Binary16 shadow of an f32 dataset (screen_device.h) and the int8 copy of the first node-major stage, built by the first
// forest build that wants them.  Returns false when the screen cannot be used: never for 1-bit metrics / short vectors,
// and — NOT remembered, the next build tries again — when the memory for the copies is not available right now (another
// build's arenas may be live); ah_build_stats.screen_unavailable then says why the build ran in f32 arithmetic only.
static bool ensure_screen8(ah_dataset *ds, hipStream_t s, bool force, bool want_lo = true);
// (ensure_screen is shared with search.hip: the certified top-k screen of the re-rank uses the same copy)
namespace ah {
bool ensure_screen(ah_dataset *ds, hipStream_t s, bool want8, bool retry_failed) {
    std::lock_guard<std::mutex> lk(ds->mu);
    if (metric_is_bq(ds->metric) || ds->dims < 32 || ds->n == 0) {
        ds->screen_never = true;
        return false;
    }
    if (!ds->d_rows_h16) {
        // a reader that found no memory for the copies does not ask again on every call (each attempt would cost an
        // allocation of n x hpitch x 2 bytes): the next build does
        if (ds->screen_alloc_failed && !retry_failed) return false;
        ds->screen_alloc_failed = true;  // until the copies exist
        const uint32_t hpitch = (ds->dims + 63u) & ~63u;
        uint16_t *rows = nullptr;
        float4 *stats = nullptr;
        // (optional allocations: a full device does not make them empty the cache)
        if (dev_malloc((void **)&rows, ds->n * (size_t)hpitch * 2, true) != hipSuccess ||
            dev_malloc((void **)&stats, ds->n * sizeof(float4), true) != hipSuccess) {
            (void)hipGetLastError();
            if (rows) (void)dev_free_unused(rows);
            return false;
        }
        const DataView dv = ds->view();
        const unsigned grid = (unsigned)std::min<uint64_t>((ds->n + 31) / 32, 1u << 20);
        hipLaunchKernelGGL(k_shadow_rows, dim3(grid), dim3(kBlock), 0, s, dv, rows, hpitch, stats);
        uint32_t *d_max = nullptr;
        uint32_t h_max[4] = {0u, 0u, 0u, 0u};
        bool ok = dev_malloc((void **)&d_max, 16) == hipSuccess && hipMemsetAsync(d_max, 0, 16, s) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(k_stats_max, dim3(1024), dim3(256), 0, s, stats, (uint64_t)ds->n, d_max);
            ok = hipMemcpyAsync(h_max, d_max, 16, hipMemcpyDeviceToHost, s) == hipSuccess;
        }
        if (hipStreamSynchronize(s) != hipSuccess || !ok) {
            (void)hipGetLastError();
            (void)dev_free(rows);
            (void)dev_free(stats);
            if (d_max) (void)dev_free(d_max);
            return false;
        }
        (void)dev_free(d_max);
        memcpy(ds->screen_max, h_max, 12);
        ds->hpitch = hpitch;
        ds->d_screen_stats = stats;
        ds->d_rows_h16 = rows;
        ds->screen_alloc_failed = false;
        ds->screen_ready.store(true, std::memory_order_release);  // readers without `mu` look at this flag only
    }
    const long long tun8 = tun(TUN_SCREEN8);
    if (want8 && tun8 != 0 && ds->metric != AH_DOT_PRODUCT && !ds->d_rows_i8 && (!ds->screen8_decided || tun8 == 1))
        (void)ensure_screen8(ds, s, tun8 == 1);
    return true;
}
// The int8 copy for the SEARCH side (round 6: the first stage of the certified top-k screen of ah_search_batch /
// ah_rerank_batch): the copy the node-major levels of the build use — made here for DotProduct as well, whose build has no use
// for it (and therefore without the second digit of the rows, which only the build's stage 1 reads).
bool ensure_screen8_search(ah_dataset *ds, hipStream_t s) {
    if (ds->screen8_ready.load(std::memory_order_acquire)) return true;
    std::lock_guard<std::mutex> lk(ds->mu);
    if ((ds->metric != AH_COSINE && ds->metric != AH_DOT_PRODUCT) || ds->dims < 32 || ds->n == 0) return false;
    if (ds->d_rows_i8) return ds->screen8_ready.load(std::memory_order_acquire);
    const long long tun8 = tun(TUN_SCREEN8);
    if (tun8 == 0 || (ds->screen8_decided && tun8 != 1)) return false;  // found useless (or unavailable) before
    return ensure_screen8(ds, s, tun8 == 1, ds->metric != AH_DOT_PRODUCT);
}
}  // namespace ah
// The int8 copy (rows, one scale per row, one power of two per dimension).  Kept only when it will decide most pairs: the
// margin of a row against a normal of an unrelated direction is ~ |n||x| / sqrt(dims), the bound ~ |n| |x - x~8| (the
// normal's two int8 digits make its own error negligible), so the copy is useful while quality = max|y/s - q| sqrt(dims)
// / (typical |x|/s) is small: 0.06 for uniform 768-d rows (~90 % of the pairs decided), 0.2 for N(0,1) rows (~84 %); a
// few huge entries in otherwise small rows blow it up.  `force` (AH_SCREEN8=1, a test aid) keeps it whatever the data.
static bool ensure_screen8(ah_dataset *ds, hipStream_t s, bool force, bool want_lo) {
    const DataView dv = ds->view();
    const uint32_t pitch8 = (ds->dims + 127u) & ~127u;
    const unsigned grid = (unsigned)std::min<uint64_t>((ds->n + 31) / 32, 1u << 20);
    int8_t *rows8 = nullptr, *rows8_lo = nullptr;
    float *scales = nullptr, *dimsc = nullptr;
    uint32_t *d_m = nullptr;  // [pitch8 column maxima][5 row maxima + pad]
    uint32_t h_m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    // the rows' second digit is optional: without the memory for it stage 1 is simply the binary16 row
    if (want_lo && tun(TUN_SCREEN8_LO) != 0 && dev_malloc((void **)&rows8_lo, ds->n * (size_t)pitch8) != hipSuccess) {
        (void)hipGetLastError();
        rows8_lo = nullptr;
    }
    bool ok = dev_malloc((void **)&rows8, ds->n * (size_t)pitch8) == hipSuccess &&
              dev_malloc((void **)&scales, ds->n * sizeof(float)) == hipSuccess &&
              dev_malloc((void **)&dimsc, 2 * (size_t)pitch8 * sizeof(float)) == hipSuccess &&
              dev_malloc((void **)&d_m, ((size_t)pitch8 + 8) * 4) == hipSuccess;
    const bool alloc_ok = ok;
    ok = ok && hipMemsetAsync(d_m, 0, ((size_t)pitch8 + 8) * 4, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_col_maxabs, dim3((unsigned)std::min<uint64_t>(4096, (ds->n + 255) / 256)), dim3(256), 0, s, dv, d_m);
        hipLaunchKernelGGL(k_dim_scales, dim3((pitch8 + 255) / 256), dim3(256), 0, s, d_m, ds->dims, pitch8, dimsc, dimsc + pitch8);
        hipLaunchKernelGGL(k_shadow_rows8, dim3(grid), dim3(kBlock), 0, s, dv, dimsc + pitch8, rows8, rows8_lo, pitch8, scales,
                           d_m + pitch8);
        ok = hipMemcpyAsync(h_m, d_m + pitch8, 20, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    bool keep = false;
    if (ok) {
        float a8, b8, c8;
        memcpy(&a8, &h_m[0], 4);
        memcpy(&b8, &h_m[1], 4);
        memcpy(&c8, &h_m[2], 4);
        // against a TYPICAL |q| rather than the largest: rows are ~ isotropic after the column scaling, |q| ~ |x| / s
        const double quality = (double)b8 * std::sqrt((double)ds->dims) / std::max((double)a8, 1e-300);
        ds->screen8_quality = quality;
        if (tun(TUN_TIMING) != 0)
            fprintf(stderr, "[ah] int8 copy of %llu x %u rows: max |q| %.1f, max |y/s - q| %.2f, max |x|/s %.1f, quality %.3f (kept below 0.6)\n",
                    (unsigned long long)ds->n, ds->dims, (double)a8, (double)b8, (double)c8, quality);
        keep = std::isfinite(a8) && std::isfinite(b8) && std::isfinite(c8) && a8 > 0.0f && (force || quality < 0.6);
        if (keep) {
            ds->d_rows_i8 = rows8;
            ds->d_rows_i8_lo = rows8_lo;
            memcpy(&ds->screen8_max[3], &h_m[3], 8);
            ds->d_scale8_rows = scales;
            ds->d_dim_scale = dimsc;
            ds->pitch8 = pitch8;
            ds->screen8_max[0] = a8;
            ds->screen8_max[1] = b8;
            ds->screen8_max[2] = c8;
            ds->screen8_ready.store(true, std::memory_order_release);  // (readers without `mu`: the search paths)
        }
        ds->screen8_decided = true;
    } else {
        (void)hipGetLastError();
        if (alloc_ok) ds->screen8_decided = true;  // a device fault, not a lack of memory: do not loop on it
    }
    if (!keep) {
        if (rows8_lo) (void)dev_free(rows8_lo);
        if (rows8) (void)dev_free(rows8);
        if (scales) (void)dev_free(scales);
        if (dimsc) (void)dev_free(dimsc);
    }
    if (d_m) (void)dev_free(d_m);
    return keep;
}

// Device -> pageable host copies off the build's critical path.  hipMemcpy into pageable memory is staged by the
// runtime on one thread and pays the first-touch page faults of the fresh destination there (measured: 4 GB of item
// ids in 0.60 s = 6.7 GB/s, whatever the number of concurrent calls).  Instead a worker thread owns a pinned double
// buffer: the DMA engine fills one half while a few threads copy the other half to its final place, and the level
// loop never waits for it — each level's normals travel while the next levels are computed.
// One delivery of a streaming build (ah_build_forest_stream): the payloads of `nodes` lie back to back at a device address, in
// the order of the list (split planes of a level: one record per node; item ids: the leaves in (tree, position) order).  The
// read-back worker moves them through its pinned double buffer in pieces of whole nodes and calls the sink on every piece.
// (a list of 819 000 nodes is 39 MB: value-initialising it on the launching thread — page faults of fresh memory included — was
// most of the 37 ms a streaming build's deepest digest took; the threads that fill it touch its pages instead)
struct StreamNodeRaw {
    ah_stream_node v;
    StreamNodeRaw() {}  // NOLINT: no initialisation on purpose
};
static_assert(sizeof(StreamNodeRaw) == sizeof(ah_stream_node), "a plain wrapper");
struct StreamNodeList {
    std::vector<StreamNodeRaw> raw;
    void resize(size_t n) { raw.resize(n); }
    size_t size() const { return raw.size(); }
    bool empty() const { return raw.empty(); }
    ah_stream_node *data() { return reinterpret_cast<ah_stream_node *>(raw.data()); }
    ah_stream_node &operator[](size_t i) { return raw[i].v; }
    const ah_stream_node &operator[](size_t i) const { return raw[i].v; }
};
struct StreamJob {
    ah_node_batch head{};                // kind, level, record geometry
    StreamNodeList nodes;                // payload_offset: byte offset from the job's device address, ascending, contiguous
    uint64_t fixed_len = 0;              // bytes of one payload (split planes), or 0: count * 4 (item ids)
    // ah_build_forest_stream_encoded: the payloads above are the SOURCE of an encode on the worker's stream; the sink gets
    // NodeCodec values of explicit lengths (Readback::deliver_encoded)
    bool encoded = false;
    uint32_t header_size = 0, vector_size = 0;
};
// Device side of an encoded streaming build, obtained once per batch of trees (the worker never allocates or frees device
// memory: a free waits for the whole device).  Values are encoded piece by piece into `out`, the twin of the pinned double
// buffer; node descriptions and value offsets go through `nodes` / `off` in chunks of `chunk` nodes.  64 MiB + 40 bytes per
// node of a chunk, whatever the size of the forest: no second copy of the item ids.
struct EncodeScratch {
    DevBuf<uint8_t> out;
    DevBuf<EncNode> nodes;
    DevBuf<uint64_t> off, sums;
    DevBuf<uint32_t> info, err;
    size_t chunk = 0;
    int ensure(size_t half) {
        chunk = std::min<size_t>(std::max<size_t>(half / 256, 1024), (size_t)1 << 18);
        AH_TRY(out.ensure(2 * half));
        AH_TRY(nodes.ensure(chunk));
        AH_TRY(off.ensure(chunk + 1));
        AH_TRY(sums.ensure(enc_scan_sums(chunk)));
        AH_TRY(info.ensure(chunk));
        AH_TRY(err.ensure(1));
        return AH_OK;
    }
};
struct StreamTarget {
    ah_node_batch_fn sink = nullptr;
    void *user = nullptr;
    std::atomic<int> sink_rc{0};         // first non-zero return of the sink: the build stops with AH_ERR_CANCELLED
    std::atomic<int> too_big{0};         // a single payload larger than half of the pinned buffer
    uint64_t batches = 0, bytes = 0;
};

struct Readback {
    struct Job {
        void *dst;
        const void *src;
        size_t bytes;
        StreamJob *stream = nullptr;     // non-null: deliver to the sink (dst unused); owned by the job
    };
    StreamTarget *target = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> q;
    size_t pending = 0;
    bool stop = false, started = false, inline_mode = false;
    hipError_t err = hipSuccess;
    int device = 0;
    int numa_node = -1;      // host node of the device: the worker and its copy threads run there (api.hip "NUMA placement")
    uint8_t *pin = nullptr;  // 2 x half bytes of pinned memory (owned by the build's Context)
    size_t half = 0;

    void start(int dev, void *pinned, size_t pinned_bytes) {
        device = dev;
        pin = reinterpret_cast<uint8_t *>(pinned);
        half = pinned_bytes / 2;
        started = true;
        try {
            th = std::thread([this] { run(); });
        } catch (...) {  // no worker: push() copies synchronously
            started = false;
            inline_mode = true;
        }
    }
    // pinned bounce buffer -> final place, with non-temporal stores: the destination is written once and read much
    // later by the caller, so its lines need neither be read for ownership nor stay in the host caches
    __attribute__((target("avx2"))) static void copy_stream(uint8_t *dst, const uint8_t *src, size_t bytes) {
        size_t i = 0;
        const size_t head = std::min<size_t>(bytes, (32 - (reinterpret_cast<uintptr_t>(dst) & 31u)) & 31u);
        if (head) memcpy(dst, src, head);
        for (i = head; i + 128 <= bytes; i += 128) {
            const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
            const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
            const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
            const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
            _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
            _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
            _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c);
            _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
        }
        if (i < bytes) memcpy(dst + i, src + i, bytes - i);
        _mm_sfence();
    }
    static void copy_part(uint8_t *dst, const uint8_t *src, size_t bytes) {
        static const bool avx2 = __builtin_cpu_supports("avx2");
        if (avx2 && bytes >= 4096) copy_stream(dst, src, bytes);
        else memcpy(dst, src, bytes);
    }
    unsigned copy_threads = 8;
    void spread(uint8_t *dst, const uint8_t *src, size_t bytes) const {  // copy on up to copy_threads cores
        const unsigned n_threads = (unsigned)std::min<size_t>(copy_threads, bytes >> 20);
        if (n_threads <= 1) {
            copy_part(dst, src, bytes);
            return;
        }
        const size_t per = ((bytes + n_threads - 1) / n_threads + 4095) & ~(size_t)4095;
        parallel_run(n_threads, [=](unsigned t) {
            const size_t lo = (size_t)t * per;
            if (lo < bytes) copy_part(dst + lo, src + lo, std::min(per, bytes - lo));
        });
    }
    hipError_t copy(const Job &job, hipStream_t cs, hipEvent_t *ev) {
        const bool direct = tun(TUN_READBACK_DIRECT) != 0;  // A/B: let the runtime stage the copy
        if (direct) {
            hipError_t e = hipMemcpyAsync(job.dst, job.src, job.bytes, hipMemcpyDeviceToHost, cs);
            return e == hipSuccess ? hipStreamSynchronize(cs) : e;
        }
        const uint8_t *src = reinterpret_cast<const uint8_t *>(job.src);
        uint8_t *dst = reinterpret_cast<uint8_t *>(job.dst);
        size_t issued = 0, landed = 0, prev_len = 0;
        int b = 0;
        hipError_t e = hipSuccess;
        while (landed < job.bytes && e == hipSuccess) {
            size_t len = 0;
            if (issued < job.bytes) {
                len = std::min(half, job.bytes - issued);
                e = hipMemcpyAsync(pin + (size_t)b * half, src + issued, len, hipMemcpyDeviceToHost, cs);
                if (e == hipSuccess) e = hipEventRecord(ev[b], cs);
                issued += len;
            }
            if (prev_len && e == hipSuccess) {  // the other half is in flight while this one is spread out
                e = hipEventSynchronize(ev[b ^ 1]);
                if (e == hipSuccess) spread(dst + landed, pin + (size_t)(b ^ 1) * half, prev_len);
                landed += prev_len;
            }
            prev_len = len;
            b ^= 1;
        }
        return e;
    }
    // device -> pinned half -> sink, piece by piece: the DMA of piece p + 1 is in flight while the sink looks at piece p
    hipError_t deliver(StreamJob &job, const uint8_t *src, hipStream_t cs, hipEvent_t *ev) {
        if (job.encoded) return deliver_encoded(job, src, cs, ev);
        struct Piece {
            size_t a = 0, b = 0;      // nodes [a, b)
            uint64_t off = 0, len = 0;
            int buf = 0;
            bool live = false;
        } cur, prev;
        auto len_of = [&](const ah_stream_node &nd) -> uint64_t { return job.fixed_len ? job.fixed_len : (uint64_t)nd.count * 4; };
        const size_t n = job.nodes.size();
        size_t next = 0;
        int b = 0;
        hipError_t e = hipSuccess;
        while ((next < n || prev.live) && e == hipSuccess) {
            cur = Piece{};
            if (next < n && !target->sink_rc.load() && !target->too_big.load()) {
                cur.a = next;
                cur.off = job.nodes[next].payload_offset;
                size_t k = next;
                while (k < n && job.nodes[k].payload_offset + len_of(job.nodes[k]) - cur.off <= half) k++;
                if (k == next) {  // one payload alone does not fit: nothing sensible to hand over
                    target->too_big.store(1);
                    next = n;
                } else {
                    cur.b = k;
                    cur.len = job.nodes[k - 1].payload_offset + len_of(job.nodes[k - 1]) - cur.off;
                    cur.buf = b;
                    cur.live = true;
                    if (cur.len) e = hipMemcpyAsync(pin + (size_t)b * half, src + cur.off, cur.len, hipMemcpyDeviceToHost, cs);
                    if (e == hipSuccess) e = hipEventRecord(ev[b], cs);
                    next = k;
                    b ^= 1;
                }
            } else {
                next = n;
            }
            if (prev.live && e == hipSuccess) {
                e = hipEventSynchronize(ev[prev.buf]);
                if (e == hipSuccess && !target->sink_rc.load()) {
                    for (size_t i = prev.a; i < prev.b; i++) job.nodes[i].payload_offset -= prev.off;
                    ah_node_batch batch = job.head;
                    batch.n_nodes = prev.b - prev.a;
                    batch.nodes = job.nodes.data() + prev.a;
                    batch.payload = pin + (size_t)prev.buf * half;
                    batch.payload_len = prev.len;
                    const int rc = target->sink(target->user, &batch);
                    target->batches++;
                    target->bytes += prev.len;
                    if (rc != 0) target->sink_rc.store(rc);
                }
            }
            prev = cur;
        }
        return e;
    }
    // The encoded stream: the job's payloads are encoded on this stream, piece by piece, into the device twin of the pinned
    // half that then carries them to the sink.  A chunk of nodes first gets its value offsets — split values from
    // has_normal on the host, Descendants from the measure + scan kernels — so that pieces are cut at explicit lengths:
    // whole values that fit one half.  The encode and the DMA of piece p + 1 are in flight while the sink looks at piece p.
    EncodeScratch *enc = nullptr;
    hipError_t deliver_encoded(StreamJob &job, const uint8_t *src, hipStream_t cs, hipEvent_t *ev) {
        struct Piece {
            size_t a = 0, b = 0;  // nodes [a, b) of the job
            uint64_t len = 0;
            int buf = 0;
            bool live = false;
        } prev;
        const bool leaves = job.head.kind == AH_NODE_DESCENDANTS;
        const size_t n = job.nodes.size();
        ah_node_batch head = job.head;
        head.normal_stride = head.normal_vector_offset = head.normal_header_offset = 0;  // the mark of an encoded batch
        const uint32_t hdr_off = (uint32_t)job.head.normal_header_offset;
        std::vector<EncNode> meta;
        std::vector<uint64_t> off;
        hipError_t e = hipSuccess;
        int b = 0;
        auto stopped = [&] { return target->sink_rc.load() != 0 || target->too_big.load() != 0; };
        auto hand_over = [&](const Piece &p) -> hipError_t {
            const hipError_t w = hipEventSynchronize(ev[p.buf]);
            if (w != hipSuccess || target->sink_rc.load()) return w;
            ah_node_batch batch = head;
            batch.n_nodes = p.b - p.a;
            batch.nodes = job.nodes.data() + p.a;
            batch.payload = pin + (size_t)p.buf * half;
            batch.payload_len = p.len;
            const int rc = target->sink(target->user, &batch);
            target->batches++;
            target->bytes += p.len;
            if (rc != 0) target->sink_rc.store(rc);
            return hipSuccess;
        };
        auto status = [](int st) { return st == AH_OK ? hipSuccess : hipErrorLaunchFailure; };  // (the launchers report through set_error)
        for (size_t c0 = 0; c0 < n && e == hipSuccess && !stopped(); c0 += enc->chunk) {
            const size_t cn = std::min(enc->chunk, n - c0);
            try {
                meta.resize(cn);
                off.resize(cn + 1);
            } catch (const std::bad_alloc &) {  // (nobody catches for this thread)
                return hipErrorOutOfMemory;
            }
            off[0] = 0;
            for (size_t i = 0; i < cn; i++) {
                const ah_stream_node &nd = job.nodes[c0 + i];
                meta[i] = leaves ? EncNode{nd.payload_offset, nd.count, 0u} : EncNode{nd.payload_offset, nd.left, nd.right};
                if (!leaves) off[i + 1] = off[i] + codec::split_value_len(nd.has_normal != 0, job.header_size, job.vector_size);
            }
            uint32_t flags = 0;
            e = hipMemcpyAsync(enc->nodes.p, meta.data(), cn * sizeof(EncNode), hipMemcpyHostToDevice, cs);
            if (leaves) {
                if (e == hipSuccess) e = hipMemsetAsync(enc->err.p, 0, 4, cs);
                if (e == hipSuccess) e = status(launch_measure_descendants(src, enc->nodes.p, cn, enc->off.p, enc->info.p, enc->sums.p, enc->err.p, cs));
                if (e == hipSuccess) e = hipMemcpyAsync(off.data(), enc->off.p, (cn + 1) * 8, hipMemcpyDeviceToHost, cs);
                if (e == hipSuccess) e = hipMemcpyAsync(&flags, enc->err.p, 4, hipMemcpyDeviceToHost, cs);
            } else if (e == hipSuccess) {
                e = hipMemcpyAsync(enc->off.p, off.data(), (cn + 1) * 8, hipMemcpyHostToDevice, cs);
            }
            // (the host vectors are pageable: they change hands only once the stream has drained)
            if (e == hipSuccess) e = hipStreamSynchronize(cs);
            if (e == hipSuccess && (flags & kEncErrOrder)) e = hipErrorInvalidValue;  // the build's own lists ascend: internal error
            size_t next = 0;
            while (next < cn && e == hipSuccess && !stopped()) {
                size_t k = next;
                while (k < cn && off[k + 1] - off[next] <= half) k++;
                if (k == next) {  // one value alone does not fit: nothing sensible to hand over
                    target->too_big.store(1);
                    break;
                }
                Piece cur;
                cur.a = c0 + next;
                cur.b = c0 + k;
                cur.len = off[k] - off[next];
                cur.buf = b;
                cur.live = true;
                uint8_t *d_out = enc->out.p + (size_t)b * half;
                e = status(leaves ? launch_write_descendants(src, enc->nodes.p + next, k - next, enc->off.p + next, enc->info.p + next, off[next],
                                                             d_out, (flags & kEncHasBitmap) != 0, cs)
                                  : launch_write_splits(src, enc->nodes.p + next, k - next, enc->off.p + next, off[next], d_out, hdr_off,
                                                        job.header_size, cs));
                if (e == hipSuccess && cur.len) e = hipMemcpyAsync(pin + (size_t)b * half, d_out, cur.len, hipMemcpyDeviceToHost, cs);
                if (e == hipSuccess) e = hipEventRecord(ev[b], cs);
                for (size_t i = next; i < k; i++) job.nodes[c0 + i].payload_offset = off[i] - off[next];
                if (prev.live && e == hipSuccess) e = hand_over(prev);
                prev = cur;
                next = k;
                b ^= 1;
            }
            // (the next chunk reuses `nodes` / `off` in stream order, behind this chunk's last write kernel)
        }
        if (prev.live && e == hipSuccess) e = hand_over(prev);
        return e;
    }
    void run() {
        hipStream_t cs = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        (void)numa_bind_thread_to_node(numa_node);  // (threads this one starts — the copies' spread — inherit its CPUs)
        hipError_t e = hipSetDevice(device);
        // A stream of its own PRIORITY: the runtime multiplexes a process's streams onto a few hardware queues per priority
        // (four by default), and once more than four streams are alive — a second dataset with its context is enough — this
        // stream could land on the queue of the build's compute stream: every chunk of the read-back then waited for the
        // level's kernel in front of it, and the ids of a group of trees arrived 0.1 s late (10M x 100 trees: 1.43 instead of
        // 1.31 s for every build of the second dataset; scripts/exp_second_dataset.py).  High-priority streams have queues
        // of their own.
        if (e == hipSuccess) e = create_copy_stream(&cs);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[0], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[1], hipEventDisableTiming);
        for (;;) {
            Job job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this] { return stop || !q.empty(); });
                if (q.empty()) break;
                job = q.front();
                q.pop_front();
            }
            if (e == hipSuccess) e = job.stream ? deliver(*job.stream, reinterpret_cast<const uint8_t *>(job.src), cs, ev) : copy(job, cs, ev);
            delete job.stream;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e != hipSuccess && err == hipSuccess) err = e;
                pending--;
            }
            cv.notify_all();
        }
        if (ev[0]) (void)hipEventDestroy(ev[0]);
        if (ev[1]) (void)hipEventDestroy(ev[1]);
        if (cs) (void)hipStreamDestroy(cs);
    }
    void push(void *dst, const void *src, size_t bytes) {
        if (!bytes) return;
        if (inline_mode) {  // the worker thread could not be created: a plain synchronous copy
            const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess && err == hipSuccess) err = e;
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back(Job{dst, src, bytes, nullptr});
            pending++;
        }
        cv.notify_all();
    }
    // hand a stream job (ownership included) to the worker; without a worker thread it is delivered right here
    void push_stream(StreamJob *job, const void *src) {
        if (job->nodes.empty()) {
            delete job;
            return;
        }
        if (inline_mode) {
            hipStream_t cs = nullptr;
            hipEvent_t ev[2] = {nullptr, nullptr};
            hipError_t e = create_copy_stream(&cs);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[0], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[1], hipEventDisableTiming);
            if (e == hipSuccess) e = deliver(*job, reinterpret_cast<const uint8_t *>(src), cs, ev);
            if (e != hipSuccess && err == hipSuccess) err = e;
            if (ev[0]) (void)hipEventDestroy(ev[0]);
            if (ev[1]) (void)hipEventDestroy(ev[1]);
            if (cs) (void)hipStreamDestroy(cs);
            delete job;
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back(Job{nullptr, src, 1, job});
            pending++;
        }
        cv.notify_all();
    }
    hipError_t drain() {  // every pushed copy has landed
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return pending == 0; });
        return err;
    }
    ~Readback() {
        if (!started) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        th.join();
    }
};

// What the launchers of one level share: the level's tables and the buffers its margin kernels read and write.
namespace {
struct LevelBufs {
    DataView dv;
    ScreenView sv;
    int metric, device;
    hipStream_t s;
    uint64_t N;
    uint32_t n_trees, n_nodes, n_tiles;
    FNode *nodes;  // the level's node table, its tiles, the permutation it reads
    FTile *tiles;
    uint32_t *perm;
    uint8_t *normals;  // the level's chunk of normal records, then its binary16 and int8 shadows
    uint64_t nstride, hdr_off;
    uint8_t *shadow;
    uint64_t hstride;
    uint8_t *shadow8;
    uint64_t stride8;
    uint64_t *masks;
    uint32_t *tile_left, *node_of;  // (row-major levels: node index and side per (tree, row))
    uint8_t *side_bytes;
    uint32_t *side_bits;
    ScreenCounters *counters;
    AbortFlags abort_all, abort_gated;  // the cancel word alone; with the gate of the attempt (attempts 1-3: nodes left pending)
    uint32_t verify;
};

// The dispatch over the metric of every margin-kernel family.
template <class F>
int with_metric(int metric, F &&f) {
    return with_metric_of<AH_EUCLIDEAN, AH_MANHATTAN, AH_COSINE, AH_DOT_PRODUCT>(metric, f);
}

// k_forest_create_split of an attempt (`metric`: the f32 space the two-means run in).
int launch_create_split(const LevelBufs &b, int metric, unsigned grid, size_t cs_shared) {
    return with_metric(metric, [&](auto m) -> int {
        constexpr int M = decltype(m)::value;
        AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_create_split<M>), b.device, cs_shared));
        hipLaunchKernelGGL(k_forest_create_split<M>, dim3(grid), dim3(64), cs_shared, b.s, b.dv, b.nodes, b.n_nodes, b.perm, b.N,
                           b.normals, b.nstride, b.hdr_off, b.abort_gated.gate);
        return AH_OK;
    });
}

// One launch of k_forest_screen_rows (metric x trees per group x LDS-resident normals).
template <int M, int TC, bool LDS>
int launch_screen_rows_inst(const LevelBufs &b, const RowsLaunch &l, const RowsSchedule &sch, unsigned grid, size_t sh, size_t lds_grant) {
    const unsigned threads = LDS ? (TC >= 16 ? 512u : 1024u) : (unsigned)kBlock;
    if (LDS) AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_screen_rows<M, TC, LDS>), b.device, lds_grant));
    hipLaunchKernelGGL((k_forest_screen_rows<M, TC, LDS>), dim3(grid), dim3(threads), LDS ? sh : 0, b.s, b.dv, b.sv, b.node_of,
                       l.t0, l.np, b.normals, b.nstride, b.hdr_off, b.shadow, b.hstride, b.side_bytes, sch, b.abort_all,
                       b.counters, b.verify);
    return AH_OK;
}
int launch_screen_rows(const LevelBufs &b, const RowsLaunch &l, bool lds, const RowsSchedule &sch, unsigned grid, size_t sh,
                       size_t lds_grant) {
    return with_metric(b.metric, [&](auto m) -> int {
        constexpr int M = decltype(m)::value;
        if (lds) return l.tcv >= 16 ? launch_screen_rows_inst<M, 16, true>(b, l, sch, grid, sh, lds_grant)
                                    : launch_screen_rows_inst<M, 8, true>(b, l, sch, grid, sh, lds_grant);
        switch (l.tcv) {
        case 16: return launch_screen_rows_inst<M, 16, false>(b, l, sch, grid, sh, lds_grant);
        case 8: return launch_screen_rows_inst<M, 8, false>(b, l, sch, grid, sh, lds_grant);
        case 4: return launch_screen_rows_inst<M, 4, false>(b, l, sch, grid, sh, lds_grant);
        default: return launch_screen_rows_inst<M, 2, false>(b, l, sch, grid, sh, lds_grant);
        }
    });
}
}  // namespace

// Grids of the dense MFMA screen and of the exact-pairs pass behind it (also used by ah_debug_launch_coverage).
namespace {
struct DensePlan {
    uint32_t n_row_tiles, n_col_tiles, group;
    bool wide;    // k_forest_dense_screen: 256-column tiles (512 threads) unless one 128-column tile covers the level
    int narrow;   // 0: k_forest_dense_screen (256-row tiles); 2 / 4: k_forest_dense_narrow<NT> (160-row tiles, 32 NT columns)
    bool stream;  // narrow: rows read once per level (one column tile): non-temporal loads
    uint32_t tile_rows, tile_cols, threads, lds;
    uint64_t grid;
};
DensePlan dense_plan(uint64_t N, uint32_t n_cols) {
    DensePlan p{};
    // the narrow kernel while the level is bound by the rows' HBM time rather than by the matrix units
    const long long narrow_max = tun(TUN_DENSE_NARROW_MAX_COLS), narrow_force = tun(TUN_DENSE_NARROW);
    p.narrow = narrow_force == 0 || (long long)n_cols > narrow_max ? 0 : (n_cols <= 64 ? 2 : 4);
    if (p.narrow) {
        p.tile_rows = kNarrowRows;
        p.tile_cols = 32u * (uint32_t)p.narrow;
        p.threads = kNarrowThreads;
        p.lds = p.narrow == 2 ? NarrowShape<2>::kLds : NarrowShape<4>::kLds;
        p.wide = false;
    } else {
        p.wide = n_cols > 128;
        p.tile_rows = kDM;
        p.tile_cols = p.wide ? 256u : 128u;
        p.threads = p.wide ? DenseShape<4>::kThreads : DenseShape<2>::kThreads;
        p.lds = kDenseLds;
    }
    p.n_row_tiles = (uint32_t)((N + p.tile_rows - 1) / p.tile_rows);
    p.n_col_tiles = (n_cols + p.tile_cols - 1) / p.tile_cols;
    p.group = p.n_col_tiles > 1 ? (p.narrow ? 12u : kDenseGroup) : 1u;  // ~3 MB of X~ tiles per group and XCD
    const long long st = tun(TUN_DENSE_NARROW_STREAM);
    p.stream = p.narrow && (st < 0 ? p.n_col_tiles == 1 : st != 0);
    const uint64_t r8 = (p.n_row_tiles + 7) / 8;
    p.grid = 8 * ((r8 + p.group - 1) / p.group) * p.group * p.n_col_tiles;
    return p;
}
unsigned exact_pairs_grid(uint64_t N, uint32_t n_trees) {  // a multiple of 8: block b and b + grid land on the same XCD
    return (unsigned)std::min<uint64_t>((((N + 1023) / 1024 + 7) / 8) * 8 * ((n_trees + 3) / 4), 1u << 16);
}
}  // namespace

// Launch plan of one screened row-major pass over `groups` groups of `tcv` trees (RowsSchedule): chunk size, one XCD per
// (chunk, group) or not, non-temporal rows or not, and the launches the pass is cut into (a launch carries at most
// LAUNCH_MAX_ITEMS work-items).  The build and ah_debug_launch_coverage both launch exactly what this returns.
namespace {
struct RowsPlan {
    RowsSchedule sch{};
    unsigned threads = kBlock;
    bool xcd = false, nt = false;
    std::vector<std::pair<uint32_t, unsigned>> launches;  // (first chunk, grid)
};
int plan_rows_launches(uint64_t N, uint32_t hpitch, uint32_t tcv, uint32_t groups, bool lds, uint64_t group_normal_bytes,
                       RowsPlan *plan) {
    const uint32_t env_rpb = (uint32_t)std::max<long long>(0, tun(TUN_ROWS_PER_BLOCK)) / 32u * 32u;
    const uint32_t rpb = lds ? 1024u : env_rpb ? env_rpb : 32u;  // rows per block
    const uint64_t hrow = (uint64_t)hpitch * 2;
    const uint64_t want_rows = tun(TUN_ROWS_CHUNK_ROWS) > 0 ? (uint64_t)tun(TUN_ROWS_CHUNK_ROWS)
                                                             : ((uint64_t)std::max<long long>(1, tun(TUN_ROWS_CHUNK_MB)) << 20) / hrow;
    uint32_t chunk_rows = (uint32_t)std::max<uint64_t>(rpb, want_rows / rpb * rpb);
    if (chunk_rows > N) chunk_rows = (uint32_t)((N + rpb - 1) / rpb * rpb);
    const uint32_t n_chunks = (uint32_t)((N + chunk_rows - 1) / chunk_rows);
    RowsSchedule &sch = plan->sch;
    sch.n_groups = groups;
    sch.tiles = chunk_rows / rpb;
    sch.chunk_rows = chunk_rows;
    sch.rows_per_block = rpb;
    // one XCD per (chunk, group) pays for small groups of many trees (measured at 10M x 100 trees: TC=4 level 9 139 -> 124 ms,
    // level 10 199 -> 188; TC=2 level 10 211 -> 193; TC=8 with its 12 groups on 8 XCDs: level 8 111 -> 120, so not there)
    plan->xcd = !lds && tun(TUN_ROWS_XCD) != 0 && tcv <= 4 && groups >= (uint32_t)std::max<long long>(1, tun(TUN_ROWS_XCD_MIN_GROUPS));
    sch.xcd_slots = plan->xcd ? (groups + 7) / 8 : 0u;
    const uint64_t per_chunk = plan->xcd ? 8ull * sch.xcd_slots * sch.tiles : (uint64_t)groups * sch.tiles;
    // One XCD per group: the rows of a (chunk, group) are read once by that XCD, so in its L2 they only compete with the
    // group's normals.  When those no longer fit (> ~5 MB) the rows are streamed with non-temporal loads (level 10 at 10M x
    // 100 trees: 188 -> 171 ms); while they fit, cached row loads are better (the chunk then stays in the Infinity Cache
    // for the other groups: level 9 125 vs 142 ms).
    const long long nt_force = tun(TUN_ROWS_NT);
    plan->nt = plan->xcd && (nt_force >= 0 ? nt_force != 0 : group_normal_bytes > (uint64_t)std::max<long long>(0, tun(TUN_ROWS_NT_BYTES)));
    if (plan->nt) sch.xcd_slots |= 0x80000000u;
    plan->threads = lds ? (tcv >= 16 ? 512u : 1024u) : (unsigned)kBlock;
    // a launch carries at most 2^32 - 1 work-items: big levels go out in several launches over chunk ranges
    const uint64_t max_items = (uint64_t)std::min<long long>(0xFFFFFFFFll, std::max<long long>(1, tun(TUN_LAUNCH_MAX_ITEMS)));
    AH_REQUIRE(per_chunk * plan->threads <= max_items, AH_ERR_INVALID_ARGUMENT, "forest build: too many trees for one row-major launch");
    const uint32_t chunks_per_launch = (uint32_t)std::min<uint64_t>(n_chunks, (max_items / plan->threads) / per_chunk);
    plan->launches.clear();
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += chunks_per_launch)
        plan->launches.emplace_back(c0, (unsigned)((uint64_t)std::min<uint32_t>(chunks_per_launch, n_chunks - c0) * per_chunk));
    return AH_OK;
}
}  // namespace

// The margin pass of a level's first attempt, one launcher per kernel family.  Each launches what the level's plan
// (plan_level, level_plan.h) says and counts it in the build's statistics.
namespace {
// The dense product on the matrix units (wide, narrow or streaming narrow: dense_plan), then k_forest_exact_pairs for the
// pairs it left open.
template <int M, int WN>
int launch_dense_wide(const LevelBufs &b, const DensePlan &dp, const DenseArgs &da) {
    AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_dense_screen<M, WN>), b.device, kDenseLds));
    hipLaunchKernelGGL((k_forest_dense_screen<M, WN>), dim3((unsigned)dp.grid), dim3(DenseShape<WN>::kThreads), kDenseLds, b.s, da,
                       b.abort_all);
    return AH_OK;
}
template <int M, int NT>
int launch_dense_narrow(const LevelBufs &b, const DensePlan &dp, const DenseArgs &da) {
    if (dp.stream)
        hipLaunchKernelGGL((k_forest_dense_narrow<M, NT, true>), dim3((unsigned)dp.grid), dim3(kNarrowThreads), NarrowShape<NT>::kLds,
                           b.s, da, b.abort_all);
    else
        hipLaunchKernelGGL((k_forest_dense_narrow<M, NT, false>), dim3((unsigned)dp.grid), dim3(kNarrowThreads), NarrowShape<NT>::kLds,
                           b.s, da, b.abort_all);
    return AH_OK;
}
int launch_dense(const LevelBufs &b, const DensePlan &dp, bool exact_wide, ah_build_stats &st) {
    DenseArgs da{};
    da.rows = b.sv.rows;
    da.stats = b.sv.stats;
    da.headers = b.dv.headers;
    da.n = b.N;
    da.hpitch = b.sv.hpitch;
    da.shadow = b.shadow;
    da.hstride = b.hstride;
    da.n_cols = b.n_nodes;
    da.nodes = b.nodes;
    da.node_of = b.node_of;
    da.side_bytes = b.side_bytes;
    // accumulation error of the product: every one of the hpitch exact binary16 products enters one f32
    // chain; whatever the order and the rounding mode of the matrix unit's adders (nearest or truncating,
    // aligned to the largest addend of a 16-wide step or not), the sum is off by less than
    // (hpitch + hpitch / 16) * 2^-23 * sum |x~_i n~_i|; taken twice over
    da.gamma_s = (float)(2.0 * ((double)b.sv.hpitch + (double)b.sv.hpitch / 16 + 16.0) * 1.1920929e-7);
    da.gamma_r = b.sv.gamma_r;
    da.n_row_tiles = dp.n_row_tiles;
    da.n_col_tiles = dp.n_col_tiles;
    da.group = dp.group;
    da.verify = b.verify;
    AH_REQUIRE(dp.grid < 0x7FFFFFFFull, AH_ERR_INVALID_ARGUMENT, "forest build: too many tiles for one launch");
    const unsigned egrid = exact_pairs_grid(b.N, b.n_trees);
    AH_TRY(with_metric(b.metric, [&](auto m) -> int {
        constexpr int M = decltype(m)::value;
        if (dp.narrow == 2) AH_TRY((launch_dense_narrow<M, 2>(b, dp, da)));
        else if (dp.narrow == 4) AH_TRY((launch_dense_narrow<M, 4>(b, dp, da)));
        else if (dp.wide) AH_TRY((launch_dense_wide<M, 4>(b, dp, da)));
        else AH_TRY((launch_dense_wide<M, 2>(b, dp, da)));
        if (exact_wide)
            hipLaunchKernelGGL((k_forest_exact_pairs<M, true>), dim3(egrid), dim3(256), 0, b.s, b.dv, b.node_of, b.side_bytes,
                               b.n_trees, b.normals, b.nstride, b.hdr_off, b.counters, b.abort_all);
        else
            hipLaunchKernelGGL((k_forest_exact_pairs<M>), dim3(egrid), dim3(256), 0, b.s, b.dv, b.node_of, b.side_bytes, b.n_trees,
                               b.normals, b.nstride, b.hdr_off, b.counters, b.abort_all);
        return AH_OK;
    }));
    st.dense_launches++;
    st.dense_columns += b.n_nodes;
    return AH_OK;
}

// The screened row-major pass.  Chunk-major launches (RowsSchedule): all full groups of the level in ONE launch, so that the
// passes over a chunk of rows run back to back and find it in the Infinity Cache; the last trees (fewer than a group) in
// launches of their own.  The LDS variant reads the first node of every tree from a device copy (`d_tree_first`).
int launch_rows_screened(const LevelBufs &b, const LevelPlan &plan, uint64_t nodes_per_tree, uint64_t rec_bytes,
                         const uint32_t *d_tree_first, size_t lds_grant, ah_build_stats &st) {
    const bool lds = plan.lds_tc != 0;
    const size_t lds_sh = (size_t)plan.lds_worst * rec_bytes;
    for (const RowsLaunch &l : plan.launches) {
        RowsPlan rp;
        AH_TRY(plan_rows_launches(b.N, b.sv.hpitch, l.tcv, l.groups, lds, (uint64_t)l.tcv * nodes_per_tree * rec_bytes, &rp));
        rp.sch.tree_first = d_tree_first;
        for (const auto &c : rp.launches) {
            rp.sch.chunk0 = c.first;
            AH_TRY(launch_screen_rows(b, l, lds, rp.sch, c.second, lds_sh, lds_grant));
        }
        st.margin_mode_launches[lds ? (l.tcv >= 16 ? MM_LDS16 : MM_LDS8) : mm_rows(l.tcv)]++;
        st.rows_xcd_launches += rp.xcd ? rp.launches.size() : 0;
        st.rows_nt_launches += rp.nt ? rp.launches.size() : 0;
        st.rows_split_launches += rp.launches.size() - 1;
    }
    return AH_OK;
}

// The f32 row-major pass: one launch per group of the plan's list, LDS-resident (a group without a node in the level is
// skipped) or plain.
template <int M, int TC>
int launch_rows_lds_inst(const LevelBufs &b, uint32_t t0, uint32_t np, uint32_t first, uint32_t cnt, size_t sh, size_t lds_grant) {
    const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(2, (150u << 10) / std::max<size_t>(sh, 1)));
    const unsigned threads = TC >= 16 ? 512u : 1024u;
    const unsigned grid = (unsigned)std::min<uint64_t>((b.N * 8 + threads - 1) / threads, 256u * per_cu);
    AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_margin_rows_lds<M, TC>), b.device, lds_grant));
    hipLaunchKernelGGL((k_forest_margin_rows_lds<M, TC>), dim3(grid), dim3(threads), sh, b.s, b.dv, b.node_of, t0, np, b.normals,
                       b.nstride, b.hdr_off, b.side_bytes, first, cnt, b.abort_all);
    return AH_OK;
}
template <int M, int TC>
int launch_rows_inst(const LevelBufs &b, uint32_t t0, uint32_t np, unsigned row_grid) {
    hipLaunchKernelGGL((k_forest_margin_rows<M, TC>), dim3(row_grid), dim3(kBlock), 0, b.s, b.dv, b.node_of, t0, np, b.normals,
                       b.nstride, b.hdr_off, b.side_bytes, b.abort_all);
    return AH_OK;
}
int launch_rows_f32(const LevelBufs &b, const LevelPlan &plan, uint64_t rec_bytes, unsigned row_grid, size_t lds_grant,
                    ah_build_stats &st) {
    for (const RowsLaunch &l : plan.launches)
        for (uint32_t g = 0; g < l.groups; g++) {
            const uint32_t t0 = l.t0 + g * l.tcv;
            if (plan.lds_tc) {
                const uint32_t first = plan.tree_first[t0], cnt = plan.tree_first[t0 + l.np] - first;
                if (cnt == 0) continue;
                const size_t sh = (size_t)cnt * rec_bytes;
                AH_TRY(with_metric(b.metric, [&](auto m) -> int {
                    constexpr int M = decltype(m)::value;
                    return l.tcv >= 16 ? launch_rows_lds_inst<M, 16>(b, t0, l.np, first, cnt, sh, lds_grant)
                                       : launch_rows_lds_inst<M, 8>(b, t0, l.np, first, cnt, sh, lds_grant);
                }));
                st.margin_mode_launches[l.tcv >= 16 ? MM_LDS16 : MM_LDS8]++;
            } else {
                AH_TRY(with_metric(b.metric, [&](auto m) -> int {
                    constexpr int M = decltype(m)::value;
                    switch (l.tcv) {
                    case 16: return launch_rows_inst<M, 16>(b, t0, l.np, row_grid);
                    case 8: return launch_rows_inst<M, 8>(b, t0, l.np, row_grid);
                    case 4: return launch_rows_inst<M, 4>(b, t0, l.np, row_grid);
                    default: return launch_rows_inst<M, 2>(b, t0, l.np, row_grid);
                    }
                }));
                st.margin_mode_launches[mm_rows(l.tcv)]++;
            }
        }
    return AH_OK;
}

// The node-major pass of an attempt on a persistent grid: binary-quantised, screened (`node_pre`: the pipelined variant of
// the int8 stage) or f32.  Very long vectors need more dynamic LDS than the default limit.
int launch_node_major(const LevelBufs &b, bool bq, bool screen, bool screen8, bool node_pre, unsigned node_grid, ah_build_stats &st) {
    if (bq) {
        hipLaunchKernelGGL(k_forest_margin_bq, dim3(node_grid), dim3(kBlock), b.dv.pitch * 8, b.s, b.dv, b.nodes, b.tiles, b.n_tiles,
                           b.perm, b.N, b.normals, b.nstride, b.hdr_off, b.masks, b.tile_left, b.abort_gated);
        st.margin_mode_launches[MM_BQ]++;
        return AH_OK;
    }
    if (screen) {
        const size_t sh = (size_t)b.dv.pitch * 4 + (size_t)b.sv.hpitch * 2 + (screen8 ? 2 * (size_t)b.sv.pitch8 : 0);
        auto launch = [&](auto m, auto pre) -> int {
            constexpr int M = decltype(m)::value, PRE = decltype(pre)::value;
            AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_screen_node<M, PRE>), b.device, sh));
            hipLaunchKernelGGL((k_forest_screen_node<M, PRE>), dim3(node_grid), dim3(kBlock), sh, b.s, b.dv, b.sv, b.nodes, b.tiles,
                               b.n_tiles, b.perm, b.normals, b.nstride, b.hdr_off, b.shadow, b.hstride, b.shadow8, b.stride8, b.masks,
                               b.tile_left, b.abort_gated, b.counters, b.verify);
            return AH_OK;
        };
        AH_TRY(with_metric(b.metric, [&](auto m) -> int {
            return node_pre ? launch(m, std::integral_constant<int, 6>{}) : launch(m, std::integral_constant<int, 0>{});
        }));
        st.margin_mode_launches[MM_NODE]++;
        st.screened_launches++;
        return AH_OK;
    }
    const size_t sh = (size_t)b.dv.pitch * 4;
    AH_TRY(with_metric(b.metric, [&](auto m) -> int {
        constexpr int M = decltype(m)::value;
        AH_TRY(lds_opt_in(reinterpret_cast<const void *>(k_forest_margin_f32<M>), b.device, sh));
        hipLaunchKernelGGL((k_forest_margin_f32<M>), dim3(node_grid), dim3(kBlock), sh, b.s, b.dv, b.nodes, b.tiles, b.n_tiles, b.perm,
                           b.N, b.normals, b.nstride, b.hdr_off, b.masks, b.tile_left, b.abort_gated);
        return AH_OK;
    }));
    st.margin_mode_launches[MM_NODE]++;
    return AH_OK;
}

// The tunables (common.h) a level reads, once per batch.
LevelKnobs read_level_knobs() {
    LevelKnobs k{};
    k.screen = tun(TUN_SCREEN) != 0;
    k.screen_verify = tun(TUN_SCREEN_VERIFY) != 0;
    k.rows_force = (int)tun(TUN_ROWMAJOR);
    k.dense = (int)tun(TUN_DENSE);
    k.tile_blocks = (uint32_t)std::max<long long>(1, tun(TUN_FOREST_TILE_BLOCKS));
    k.node_blocks = (uint32_t)std::max<long long>(0, tun(TUN_FOREST_NODE_BLOCKS));
    k.split_blocks = (uint32_t)std::max<long long>(1, tun(TUN_FOREST_SPLIT_BLOCKS));
    k.row_blocks = (uint32_t)std::max<long long>(1, tun(TUN_FOREST_ROW_BLOCKS));
    k.rows_advance = tun(TUN_ROWMAJOR_ADVANCE) != 0;
    k.rows_lds = tun(TUN_ROWMAJOR_LDS) != 0;
    k.rows_max_tc = (uint32_t)std::max<long long>(2, tun(TUN_ROWMAJOR_MAX_TC));
    k.rows_cache_mb = (double)tun(TUN_ROWMAJOR_CACHE_MB);
    k.dense_max_cols = (uint32_t)std::max<long long>(0, tun(TUN_DENSE_MAX_COLS));
    k.dense_gmacs = (double)std::max<long long>(1, tun(TUN_DENSE_GMACS));
    k.retry_gate = tun(TUN_RETRY_GATE) != 0;
    k.mask_bits = tun(TUN_MASK_BITS);
    k.exact_wide = tun(TUN_EXACT_WIDE) != 0;
    k.node_prefetch = tun(TUN_NODE_PREFETCH) != 0;
    k.tail_groups = (uint32_t)std::min<long long>(32, std::max<long long>(0, tun(TUN_TAIL_GROUPS)));
    k.tail_node_items = (double)std::max<long long>(1, tun(TUN_TAIL_NODE_ITEMS));
    k.tail_min_items = (uint64_t)std::max<long long>(0, tun(TUN_TAIL_MIN_MB)) * (1u << 20) / 4;
    return k;
}
}  // namespace

// `subset_ids` == nullptr: every tree covers all items (Writer::build with missing trees).  Otherwise tree t covers
// the ascending id list subset_ids[subset_offsets[first_tree + t] .. subset_offsets[first_tree + t + 1]) — the
// "descendants that became too large" of an incremental build (src/writer.rs:660-739).
//
// One level = one set of launches, and ONE host wait: the host needs the next level's sizes (LevelInfo, read back
// through pinned memory) before it can launch it; everything else about a level — its node table, from which the final
// node list is assembled — follows on a side stream and is digested by the host while the GPU runs the next level.
// host threads one build may keep busy at a time for its output path (page commits, bounce copies, digests, node list):
// ah_build_options.max_host_threads, else AH_HOST_THREADS (8).  Eight concurrent builds of an 8-GPU node in a 16-CPU
// container want 2 each.
static unsigned host_thread_budget(const ah_build_options *opt) {
    const long long v = opt->max_host_threads ? (long long)opt->max_host_threads : tun(TUN_HOST_THREADS);
    return (unsigned)std::min<long long>(64, std::max<long long>(1, v));
}

// State of one ah_build_forest_stream call across its batches.
struct StreamBuild {
    StreamTarget target;
    uint32_t id_base = 0;       // node ids handed out by earlier batches
    uint32_t *roots = nullptr;  // the caller's out_roots
    bool encoded = false;       // ah_build_forest_stream_encoded: id_base starts at the caller's node_id_base
};

struct BlobNodeScope {  // the blobs this thread asks the pool for prefer the device's host node
    int prev = -1;
    bool entered = false;
    void enter(int n) {
        prev = tl_blob_node;
        tl_blob_node = n;
        entered = true;
    }
    ~BlobNodeScope() {
        if (entered) tl_blob_node = prev;
    }
};
struct Toucher {  // commits the pages of a fresh (still unwritten) host range in the background
    std::thread th;
    unsigned max_threads = 8;
    int numa_node = -1;  // the pages are committed from the CPUs of the device's host node: first touch decides where they live
    // [off, off + bytes) of `blob`; what a recycled blob already has committed needs no touch
    void start(const HostBlob &blob, size_t off, size_t bytes) {
        join();
        const size_t lo_off = std::max(off, blob.committed), hi_off = std::min(off + bytes, blob.cap);
        if (hi_off <= lo_off || hi_off - lo_off < (8u << 20)) return;
        uint8_t *lo = blob.p + lo_off;
        const size_t len = hi_off - lo_off;
        const unsigned budget = max_threads;
        const int node = numa_node;
        try {
            th = std::thread([lo, len, budget, node] {
                (void)numa_bind_thread_to_node(node);
                // (several threads: the 2.6 GB of the deepest level's normals must be committed within that level's
                // ~140 ms, or the level loop waits for page faults before it can hand the chunk to the read-back worker)
                const unsigned parts = (unsigned)std::min<size_t>(budget, std::max<size_t>(1, len >> 26));
                parallel_run(parts, [=](unsigned p) {
                    const size_t a = len * p / parts, b = len * (p + 1) / parts;
                    for (size_t o = a; o < b; o += 4096) reinterpret_cast<volatile uint8_t *>(lo)[o] = 0;
                });
            });
        } catch (...) {  // no thread to be had: the read-back worker faults the pages in itself
        }
    }
    void join() {
        if (th.joinable()) th.join();
    }
    ~Toucher() { join(); }
};

using BuildClock = std::chrono::steady_clock::time_point;
static double ms_of(BuildClock a, BuildClock b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static double sec(BuildClock a, BuildClock b) { return std::chrono::duration<double>(b - a).count(); }

// One level from its plan to the hand-over of its node table.
struct Level {
    std::chrono::steady_clock::time_point t_top, t_launched, t_digested;
    double ms_tail_prev = 0.0;
    uint32_t n_nodes = 0, n_tiles = 0;
    LevelPlan plan;
    uint8_t *chunk_d = nullptr;  // its normal records on the device, and where they land in the forest's blob
    uint64_t chunk_bytes = 0, chunk_host_off = 0;
};
// Where a tree group of the tail starts: a slice of the table of the level the groups were cut from.
struct TailGroup {
    LevelInfo info;
    FNode *table, *other;  // the group's nodes; the table its next level is emitted into
    uint32_t *cur, *nxt;
    uint32_t depth, n0;    // n0: its first node in the whole level (its records: level_rec_full[n0 ...])
};

// One batch of trees, built level by level: the stages below, run in sequence by build_batch.  Its host bookkeeping (records,
// ring, group cuts, buffer sizes) is forest_records.h; this struct owns the device side and the order of the HIP calls.
struct BatchBuild {
    // ---- the call and what is fixed for the batch
    ah_dataset *ds;
    const ah_build_options *opt;
    uint32_t first_tree, n_trees, split_after;
    ah_forest *forest;
    Context *ctx;
    const uint32_t *subset_ids;
    const uint64_t *subset_offsets;
    StreamBuild *sb;
    std::chrono::steady_clock::time_point t_batch, t_setup_alloc, t_setup_pin, t_setup_rows, t_setup_screen, t_loop_end;
    uint64_t N, M;  // rows; entries of the batch permutation
    std::vector<uint64_t> tree_base;
    DataView dv;
    hipStream_t s;
    bool bq;
    uint64_t hdr_off, nstride;
    LevelKnobs knobs;  // the tunables (common.h), read once per batch
    int timing;
    uint32_t mode_req;
    bool exact_only, rows_allowed;
    unsigned host_threads;
    int numa_node = -1;
    BatchSizes z;

    // ---- what owns memory or threads.  MEMBER ORDER MATTERS: an early return (AH_TRY) destroys these in reverse order.
    // The device buffers come first (freed last); the Touchers join before the blobs can move; Arenas and EncodeScratch are
    // declared before the read-back worker, which is joined before the memory it reads is freed; BatchCleanup syncs the side
    // stream before its events die; RecordsLease follows the records it hands back to the pool.
    DevBuf<uint32_t> perm_a, perm_b, final_perm, tile_left, tile_left_off, d_child, d_small;
    DevBuf<FNode> d_nodes_a, d_nodes_b, d_nodes_c;  // (c: the tail in groups of trees)
    DevBuf<GroupInfo> d_groups;
    DevBuf<FTile> d_tiles;
    DevBuf<uint64_t> masks;
    DevBuf<NextCounts> d_block_sums;
    DevBuf<uint32_t> d_tree_first_buf;  // first node of every tree of the level, gaps closed (LDS variant of the row pass)
    DevBuf<uint32_t> node_of;           // row-major margin mode: node index and side byte per (tree, row)
    DevBuf<uint8_t> side_bytes;
    DevBuf<uint32_t> side_bits;
    BlobNodeScope blob_node_scope;
    Toucher prefault, touch_normals[2];  // [level & 1]: commits the level's normals, started one level ahead
    Arena arena, shadow_arena, shadow8_arena;
    BatchCleanup bc;
    EncodeScratch enc_scratch;
    Readback rb;
    BatchRecords records;
    RecordsLease records_lease;
    TableRing ring;  // node tables on their way to the digest

    // ---- views into d_small and the pinned block
    AbortFlags d_abort{};
    ScreenCounters *d_counters = nullptr;
    LevelInfo *d_info = nullptr, *h_info[2] = {nullptr, nullptr};
    uint32_t *d_tree_first = nullptr, *d_tree_first_fixed = nullptr, *h_one = nullptr, *h_tree_first = nullptr;
    uint8_t *pin = nullptr, *ring_base = nullptr;

    // ---- the screen
    bool screen = false, screen8 = false;
    ScreenView sv{};
    uint64_t hstride = 0, stride8 = 0;
    uint32_t verify = 0;

    // ---- the level loop (run_levels); a tree group of the tail re-enters it through enter_group
    LevelInfo info{};
    std::vector<uint32_t> tree_first;
    LevelShape shape{};  // the batch's part of every level's shape
    uint32_t *cur = nullptr, *nxt = nullptr;
    FNode *d_cur = nullptr, *d_next = nullptr;
    uint32_t depth = 0;
    uint32_t step = 0;  // levels launched so far: the parity of the double buffers (== depth until the tail runs in groups)
    bool prev_rows = false;  // the previous level ran row-major: node_of / side_bytes describe it, d_child links it
    bool abort_sent = false;
    std::chrono::steady_clock::time_point t_prev_waited;
    size_t cs_shared = 0;
    int split_metric = 0;
    uint64_t desc_base = 0, normals_base = 0, normals_bytes = 0, normals_cap = 0;
    size_t roots_base = 0;

    // ---- the tail in groups of trees (run_tail_groups)
    bool grouped = false, fork_now = false, group_first_level = false;
    uint32_t group_n0 = 0;
    std::vector<uint32_t> group_tree;  // tree range of group g: [group_tree[g], group_tree[g + 1])
    int pending_hand = -1;             // group whose item ids are final and still to be handed to the read-back worker
    FNode *group_spare = nullptr;      // third node table of the grouped tail
    std::deque<int> done_groups;       // groups whose tables are all digested and whose node list is still to be emitted

    // ---- a resident forest (resident_stage): where every level left its records, in launch order
    std::vector<ResidentChunk> res_chunks;
    std::vector<const uint8_t *> res_chunk_dev;

    BatchBuild(ah_dataset *ds_, const ah_build_options *opt_, uint32_t first_tree_, uint32_t n_trees_, uint32_t split_after_,
               ah_forest *forest_, Context *ctx_, const uint32_t *subset_ids_, const uint64_t *subset_offsets_, StreamBuild *sb_)
        : ds(ds_), opt(opt_), first_tree(first_tree_), n_trees(n_trees_), split_after(split_after_), forest(forest_), ctx(ctx_),
          subset_ids(subset_ids_), subset_offsets(subset_offsets_), sb(sb_), t_batch(std::chrono::steady_clock::now()), N(ds_->n),
          tree_base(n_trees_ + 1, 0), records_lease(records.recs, records.new_index) {
        for (uint32_t t = 0; t < n_trees; t++)
            tree_base[t + 1] = tree_base[t] + (subset_ids ? subset_offsets[first_tree + t + 1] - subset_offsets[first_tree + t] : N);
        M = tree_base[n_trees];
        dv = ds->view();
        s = ctx->stream;
        bq = metric_is_bq(ds->metric);
        hdr_off = ds->row_bytes();
        nstride = normal_record_stride(ds);
        knobs = read_level_knobs();
        timing = (int)tun(TUN_TIMING);
        // AH_MARGIN_MODE (measurement aid): the kernel family for callers that leave the choice to the library
        const uint32_t env_mode = (uint32_t)tun(TUN_MARGIN_MODE) & 0xFFFu;
        mode_req = (opt->margin_mode & 0xFFFu) ? (opt->margin_mode & 0xFFFu) : env_mode;
        exact_only = (opt->margin_mode & AH_MARGIN_EXACT_ONLY) != 0 || !knobs.screen;
        // row-major margin mode (full-dataset trees, f32 metrics)
        rows_allowed = !subset_ids && !bq && ds->dims >= 32 && n_trees >= 2 &&
                       (mode_req != AH_MARGIN_AUTO ? mode_req != AH_MARGIN_NODE_MAJOR : knobs.rows_force != 0);
        host_threads = host_thread_budget(opt);
        // (the shadow arenas' blocks are sized for the strides their records have WHEN a screen is up — ensure_screen decides
        // that after the buffers exist; an arena nobody takes from never allocates)
        const bool f32 = !bq && ds->dims >= 32;
        z = batch_sizes(N, n_trees, M, split_after, nstride, f32 ? shadow_stride16(screen_hpitch(ds->dims)) : 0,
                        f32 ? shadow_stride8(screen_pitch8(ds->dims)) : 0, rows_allowed,
                        knobs.mask_bits > 0 || (knobs.mask_bits < 0 && N >= (1u << 20)), tun(TUN_READBACK_MB));
    }

    // Device buffers (zeroed), the pinned block, the row-major buffers, the screen's copies, the first permutation.
    int setup_device() {
        AH_TRY(perm_a.ensure(z.perm));
        AH_TRY(perm_b.ensure(z.perm));
        AH_TRY(final_perm.ensure(z.perm));
        AH_TRY(d_nodes_a.ensure(z.nodes));
        AH_TRY(d_nodes_b.ensure(z.nodes));
        AH_TRY(d_tiles.ensure(z.tiles));
        AH_TRY(masks.ensure(z.masks));
        AH_TRY(tile_left.ensure(z.tile_left));
        AH_TRY(tile_left_off.ensure(z.tile_left));
        AH_TRY(d_child.ensure(z.child));
        AH_TRY(d_block_sums.ensure(z.block_sums));
        // small device block: [abort flag, 3 pad][ScreenCounters][LevelInfo + tree_first[n_trees + 1]]
        AH_TRY(d_small.ensure(4 + 12 + z.info_words));
        d_abort = AbortFlags{d_small.p, nullptr};
        d_counters = reinterpret_cast<ScreenCounters *>(d_small.p + 4);
        d_info = reinterpret_cast<LevelInfo *>(d_small.p + 16);
        d_tree_first = reinterpret_cast<uint32_t *>(d_info + 1);
        AH_TRY(d_tree_first_buf.ensure((size_t)n_trees + 2));
        // The control structures start from zeros.  Blocks come from the caching allocator with whatever their last user left in
        // them, and a CANCELLED level lets its bookkeeping kernels run over tables its drained margin kernels never wrote: with
        // zeros (what fresh device memory used to hold) those kernels find empty nodes and tiles; with the item indices of
        // another build in a tile table they would scatter out of bounds.  ~0.7 GB of memsets: 0.2 ms.
        AH_HIP(hipMemsetAsync(d_nodes_a.p, 0, z.nodes * sizeof(FNode), s));
        AH_HIP(hipMemsetAsync(d_nodes_b.p, 0, z.nodes * sizeof(FNode), s));
        AH_HIP(hipMemsetAsync(d_tiles.p, 0, z.tiles * sizeof(FTile), s));
        AH_HIP(hipMemsetAsync(masks.p, 0, z.masks * sizeof(uint64_t), s));
        AH_HIP(hipMemsetAsync(tile_left.p, 0, z.tile_left * 4, s));
        AH_HIP(hipMemsetAsync(tile_left_off.p, 0, z.tile_left * 4, s));
        AH_HIP(hipMemsetAsync(d_child.p, 0, z.child * 4, s));
        AH_HIP(hipMemsetAsync(d_block_sums.p, 0, z.block_sums * sizeof(NextCounts), s));
        AH_HIP(hipMemsetAsync(d_tree_first_buf.p, 0, ((size_t)n_trees + 2) * 4, s));
        t_setup_alloc = std::chrono::steady_clock::now();
        d_tree_first_fixed = d_tree_first_buf.p;
        AH_HIP(hipMemsetAsync(d_small.p, 0, (16 + z.info_words) * 4, s));

        // pinned host memory: [2 x LevelInfo block][one word for the abort flag][2 x node table][read-back bounce]
        AH_TRY(ctx->ensure_pinned(z.pinned_bytes()));
        t_setup_pin = std::chrono::steady_clock::now();
        pin = reinterpret_cast<uint8_t *>(ctx->h_pinned);
        h_info[0] = reinterpret_cast<LevelInfo *>(pin);
        h_info[1] = reinterpret_cast<LevelInfo *>(pin + z.pin_info);
        h_one = reinterpret_cast<uint32_t *>(pin + 2 * z.pin_info);
        *h_one = 1u;
        h_tree_first = reinterpret_cast<uint32_t *>(pin + 2 * z.pin_info + 256);  // staging of d_tree_first_fixed
        ring_base = pin + z.pin_head;  // the two node tables, as one ring
        ring.cap = 2 * z.pin_nodes;

        if (rows_allowed) {
            AH_TRY(node_of.ensure(z.node_of));
            // zeroed once: k_forest_exact_pairs scans it 16 bytes per lane for marks
            AH_TRY(side_bytes.ensure(z.side_bytes));
            AH_HIP(hipMemsetAsync(side_bytes.p, 0, z.side_bytes, s));
            // the same sides one bit each for the permutation-order gather of k_forest_masks_from_bytes (worth its pass from
            // the size on at which a tree's bytes no longer sit in an L2)
            if (z.side_bits && side_bits.ensure(z.side_bits) != AH_OK) (void)hipGetLastError();  // no room: the tiles gather the bytes
        }
        // certified binary16 screen: f32 metrics with AVX-tier rows, unless the caller (or AH_SCREEN=0) asks for f32 only
        t_setup_rows = std::chrono::steady_clock::now();
        screen = !exact_only && !bq && ds->dims >= 32 && ensure_screen(ds, s, true, true);
        t_setup_screen = std::chrono::steady_clock::now();
        if (!exact_only && !screen && ds->screen_alloc_failed) forest->stats.screen_unavailable = 1;
        if (screen) {
            sv.rows = ds->d_rows_h16;
            sv.stats = ds->d_screen_stats;
            sv.max_stats = make_float4(ds->screen_max[0], ds->screen_max[1], ds->screen_max[2], 0.0f);
            sv.rows8 = tun(TUN_SCREEN8) != 0 ? ds->d_rows_i8 : nullptr;  // nullptr: no int8 first stage
            sv.pitch8 = ds->pitch8;
            sv.scale8_rows = ds->d_scale8_rows;
            sv.max8 = make_float4(ds->screen8_max[0], ds->screen8_max[1], ds->screen8_max[2], 0.0f);
            sv.rows8_lo = tun(TUN_SCREEN8_LO) != 0 ? ds->d_rows_i8_lo : nullptr;  // nullptr: stage 1 is the binary16 row
            sv.max8b = make_float4(ds->screen8_max[3], ds->screen8_max[4], ds->screen8_max[2], 0.0f);
            sv.hpitch = ds->hpitch;
            // accumulation-error factors (screen_device.h), each with a 4x safety factor over the standard model:
            //   screen: hpitch/16 dot2c per lane (2 roundings each) + 4 adds;  reference: dims/32 FMAs per chain, 6 adds of
            //   the hsum tree, and a scalar tail of up to 31 multiply-adds (2 roundings each)
            sv.gamma_s = (float)(4.0 * (2.0 * (ds->hpitch / 16) + 8.0) * 5.9604645e-8);
            sv.gamma_r = (float)(4.0 * ((double)(ds->dims / 32) + 6.0 + 62.0) * 5.9604645e-8);
            hstride = shadow_stride16(ds->hpitch);  // whole lines, see normal_record_stride
        }
        verify = screen && knobs.screen_verify ? 1u : 0u;
        screen8 = screen && sv.rows8 != nullptr;
        stride8 = screen8 ? shadow_stride8(sv.pitch8) : 0;
        if (!subset_ids) {
            hipLaunchKernelGGL(k_init_perm, dim3(2048), dim3(256), 0, s, perm_a.p, N, n_trees);
        } else if (M) {
            const uint32_t *src = subset_ids + subset_offsets[first_tree];
            AH_HIP(hipMemcpyAsync(perm_a.p, src, M * 4, hipMemcpyHostToDevice, s));
            DevBuf<uint32_t> d_err;
            AH_TRY(d_err.ensure(1));
            AH_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
            hipLaunchKernelGGL(k_ids_to_rows, dim3(2048), dim3(256), 0, s, dv, perm_a.p, M, d_err.p);
            uint32_t e = 0;
            AH_HIP(hipMemcpyAsync(&e, d_err.p, 4, hipMemcpyDeviceToHost, s));
            AH_HIP(hipStreamSynchronize(s));
            AH_REQUIRE(e == 0, AH_ERR_MISSING_ITEM, "a sub-tree item id does not exist in the dataset");
        }
        AH_HIP(hipGetLastError());
        return AH_OK;
    }

    // The forest's blobs, the page touchers, the arenas' block sizes, events and side stream, the read-back worker, the records.
    int setup_host() {
        // The item-id lists come back in one piece at the very end; their size is known now, so the host memory is
        // allocated up front and its pages are touched in the background while the GPU works (first-touch faults of
        // fresh memory, not the copy, bound a read-back of several GB).
        desc_base = forest->descendants_len;
        numa_node = numa_node_of_device(ds->device);
        blob_node_scope.enter(numa_node);
        if (!sb) {  // (a streaming build hands the ids to the sink from the pinned ring: no blob)
            AH_REQUIRE(host_blob_reserve(forest->desc_blob, (desc_base + M) * 4, desc_base * 4), AH_ERR_OUT_OF_MEMORY,
                       "host allocation of the descendants failed");
            forest->descendants = reinterpret_cast<uint32_t *>(forest->desc_blob.p);
        }
        prefault.max_threads = touch_normals[0].max_threads = touch_normals[1].max_threads = host_threads;
        prefault.numa_node = touch_normals[0].numa_node = touch_normals[1].numa_node = numa_node;
        if (!sb) prefault.start(forest->desc_blob, desc_base * 4, M * 4);
        arena.block_bytes = z.arena_block;
        shadow_arena.block_bytes = z.shadow_block;
        shadow8_arena.block_bytes = z.shadow8_block;
        AH_TRY(bc.create());
        if (sb && sb->encoded) AH_TRY(enc_scratch.ensure(z.bounce / 2));
        rb.enc = &enc_scratch;
        rb.target = sb ? &sb->target : nullptr;
        rb.copy_threads = host_threads;
        rb.numa_node = numa_node;
        rb.start(ds->device, pin + z.pin_head + 2 * z.pin_nodes, z.bounce);
        records.init(n_trees, first_tree, split_after, sb != nullptr, sb ? sb->id_base : 0u, nstride, forest->nodes.size());
        records.reserve(z.max_nodes);
        roots_base = forest->roots.size();
        tree_first.assign(n_trees + 1, 0xFFFFFFFFu);
        return AH_OK;
    }

    // Level 0 on the host (the roots), and what the level loop starts from.
    int seed_roots() {
        FNode *lv = reinterpret_cast<FNode *>(ring_base);
        records.seed_roots(tree_base.data(), opt->tree_seeds + first_tree, lv, &info, tree_first.data());
        if (info.n_nodes) AH_HIP(hipMemcpyAsync(d_nodes_a.p, lv, info.n_nodes * sizeof(FNode), hipMemcpyHostToDevice, s));
        cur = perm_a.p, nxt = perm_b.p;
        d_cur = d_nodes_a.p, d_next = d_nodes_b.p;
        AH_HIP(hipEventRecord(bc.ev_begin, s));
        forest->stats.seconds_setup += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_batch).count();
        if (timing) {
            fprintf(stderr, "[ah] batch setup: device buffers %.1f ms, pinned %.1f ms, row-major buffers %.1f ms, screen copies %.1f ms, "
                            "host blobs + workers + roots %.1f ms\n",
                    ms_of(t_batch, t_setup_alloc), ms_of(t_setup_alloc, t_setup_pin), ms_of(t_setup_pin, t_setup_rows),
                    ms_of(t_setup_rows, t_setup_screen), ms_of(t_setup_screen, std::chrono::steady_clock::now()));
        }
        cs_shared = (size_t)f32_space_pitch(ds->metric, ds->dims) * 4 * 3;
        AH_REQUIRE(cs_shared <= 150 * 1024, AH_ERR_INVALID_DIMENSION, "dimensions %u too large for the LDS-resident two-means",
                   ds->dims);
        split_metric = f32_space_metric(ds->metric);
        normals_base = forest->normals_len;  // this batch appends its levels after earlier batches
        // The host blob gets lazily committed head-room (splits in total ~1.3-1.6 x items / split_after) so that finished
        // levels can land in their final place while the build continues; it only moves when no copy is in flight.
        normals_cap = forest->normals_blob.cap >= 16 ? forest->normals_blob.cap - 16 : 0;
        t_prev_waited = std::chrono::steady_clock::now();
        shape.N = N;
        shape.n_trees = n_trees;
        shape.split_after = split_after;
        shape.rec_bytes = screen ? hstride : nstride;  // bytes of one normal as the margin pass streams it
        shape.row_bytes = ds->row_bytes();
        shape.hpitch = ds->hpitch;
        shape.metric = ds->metric;
        shape.screen = screen;
        shape.screen8 = screen8;
        shape.rows8_lo = sv.rows8_lo != nullptr;
        shape.screen8_quality = ds->screen8_quality;
        shape.rows_allowed = rows_allowed;
        shape.subset = subset_ids != nullptr;
        shape.mode_req = mode_req;
        return AH_OK;
    }

    int reserve_normals(uint64_t need, uint64_t landed) {  // landed: bytes of earlier levels / batches to keep
        if (need <= normals_cap) return AH_OK;
        touch_normals[0].join();  // the blob may move: nothing may be touching it
        touch_normals[1].join();
        AH_REQUIRE(rb.drain() == hipSuccess, AH_ERR_DEVICE, "device -> host copy of the normals failed");
        uint64_t want = std::max<uint64_t>(need + need / 2, normals_base + 2 * z.max_nodes * nstride);
        if (!host_blob_reserve(forest->normals_blob, want, landed)) {
            want = need;
            AH_REQUIRE(host_blob_reserve(forest->normals_blob, want, landed), AH_ERR_OUT_OF_MEMORY,
                       "host allocation of %llu bytes of normals failed", (unsigned long long)want);
        }
        forest->normals = forest->normals_blob.p;
        normals_cap = forest->normals_blob.cap - 16;
        return AH_OK;
    }

    // ---- the node tables' way to the records ---------------------------------------------------------------------------
    // Digest the oldest pending table (BatchRecords::digest_level), report it, and — a streaming build — send the level's
    // split planes to the read-back worker as one job (record i <-> node i).
    int digest_front() {
        const PendingTable e = ring.tables.front();
        // (copies on the side stream complete in order: the event of this parity was recorded by this table's copy or a later one)
        AH_HIP(hipEventSynchronize(bc.ev_copy[e.step & 1]));
        const uint32_t *rec_of = e.rec_off >= 0 ? records.level_rec_full.data() + e.rec_off : records.level_rec.data();
        StreamJob *job = nullptr;
        if (sb) {
            job = new (std::nothrow) StreamJob();
            AH_REQUIRE(job, AH_ERR_OUT_OF_MEMORY, "host allocation failed");
            job->head.kind = AH_NODE_SPLIT;
            job->head.level = e.depth;
            job->head.normal_stride = nstride;
            job->head.normal_vector_offset = 0;
            job->head.normal_header_offset = hdr_off;
            job->fixed_len = nstride;
            job->encoded = sb->encoded;
            job->header_size = (uint32_t)ah_header_size(ds->metric);
            job->vector_size = (uint32_t)ah_vector_size(ds->metric, ds->dims);
            if (sb->encoded && records.stream_ids_wrap(e.n_nodes)) {
                delete job;  // (the children's ids are written into the values: they must not wrap)
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node_id_base + the nodes of this build pass 2^32 - 1");
            }
            job->nodes.resize(e.n_nodes);
        }
        const DigestResult r = records.digest_level(e.depth, e.n_nodes, reinterpret_cast<const FNode *>(ring_base + e.ring_off), e.host_off,
                                                    rec_of, records.digest_threads(e.n_nodes, host_threads), job ? job->nodes.data() : nullptr);
        if (r.bad != 0xFFFFFFFFu) delete job;
        else if (job) rb.push_stream(job, e.chunk_dev);  // the level's planes travel while the next levels are computed
        AH_REQUIRE(r.bad == 0xFFFFFFFFu, AH_ERR_DEVICE, "forest build: node %u of level %u left pending (internal error)", r.bad,
                   e.depth);
        forest->stats.margin_evaluations += r.evals;
        forest->stats.retries += r.retries;
        forest->stats.dummy_normals += r.dummies;
        forest->stats.levels = std::max(forest->stats.levels, e.depth + 1);
        if (opt->progress) opt->progress(opt->progress_user, e.depth + 1, records.n_recs, records.items_routed);
        if (e.fork_parent) records.level_rec_full.swap(records.level_rec);
        ring.tables.pop_front();
        // a streaming build's leaves' job starts the transfer of the group's ids: at once; a node list only costs host time
        if (e.group_done >= 0) {
            if (sb) AH_TRY(group_complete(group_tree[e.group_done], group_tree[e.group_done + 1]));
            else done_groups.push_back(e.group_done);
        }
        return AH_OK;
    }
    // the tables a level of `pairs` margin evaluations covers (all of them: pairs = ~0)
    int digest_under(uint64_t pairs) {
        // host nanoseconds the level covers: 0.14 ns per pair on the device, three quarters of it at most; a table costs ~45 ns
        // per node (four threads), a node list ~10 ns per node (eight) — both next to the read-back worker's copy threads
        double budget = (double)pairs * 0.105;
        // (a table of a few thousand nodes is a fraction of a millisecond: always — progress reports stay level by level)
        while (!ring.tables.empty() && (45.0 * ring.tables.front().n_nodes <= budget || ring.tables.front().n_nodes < 16384u)) {
            budget -= 45.0 * ring.tables.front().n_nodes;
            AH_TRY(digest_front());
        }
        while (!done_groups.empty()) {
            const uint32_t tA = group_tree[done_groups.front()], tB = group_tree[done_groups.front() + 1];
            double nodes = 0.0;
            for (uint32_t t = tA; t < tB; t++) nodes += (double)records.tree_count[t];
            if (10.0 * nodes > budget) break;
            budget -= 10.0 * nodes;
            done_groups.pop_front();
            AH_TRY(group_complete(tA, tB));
        }
        return AH_OK;
    }
    // Streaming build: the Descendants nodes of trees [tA, tB) as one job, in the order their ids lie in the final permutation.
    int push_leaves_job(uint32_t tA, uint32_t tB) {
        StreamJob *job = new (std::nothrow) StreamJob();
        AH_REQUIRE(job, AH_ERR_OUT_OF_MEMORY, "host allocation failed");
        job->head.kind = AH_NODE_DESCENDANTS;
        job->head.normal_stride = nstride;
        job->head.normal_header_offset = hdr_off;
        job->encoded = sb->encoded;
        records.leaves_of(tA, tB, host_threads, job->nodes);
        rb.push_stream(job, final_perm.p);
        return AH_OK;
    }
    // The item ids of trees [tA, tB) are final (every kernel that writes them has been waited for): rows -> item ids where the
    // two differ (on the side stream: the main one is busy with the next group), then — the blob's slice of a materialised
    // forest — to the worker.  (A streaming build hands them over as the leaves' job, once the group's tables are digested.)
    int hand_over_ids(uint32_t tA, uint32_t tB) {
        const uint64_t a = tree_base[tA], b = tree_base[tB];
        if (b > a && !ds->identity_ids) {
            hipLaunchKernelGGL(k_rows_to_ids, dim3(2048), dim3(256), 0, bc.side, final_perm.p + a, b - a, ds->d_ids);
            AH_HIP(hipStreamSynchronize(bc.side));
        }
        if (sb) return AH_OK;
        prefault.join();
        rb.push(forest->descendants + desc_base + a, final_perm.p + a, (b - a) * 4);
        return AH_OK;
    }
    int hand_over_pending() {
        if (pending_hand < 0) return AH_OK;
        const int g = pending_hand;
        pending_hand = -1;
        return hand_over_ids(group_tree[g], group_tree[g + 1]);
    }
    // the post-order node list of trees [tA, tB) (BatchRecords::emit_range); a streaming build has none
    int emit_range(uint32_t tA, uint32_t tB) {
        if (sb) return AH_OK;
        AH_REQUIRE(records.emit_range(tA, tB, host_threads, forest->nodes, forest->roots, roots_base, desc_base), AH_ERR_DEVICE,
                   "forest build: trees emitted out of order (internal error)");
        return AH_OK;
    }
    // node list / leaves' job of a finished group
    int group_complete(uint32_t tA, uint32_t tB) { return sb ? push_leaves_job(tA, tB) : emit_range(tA, tB); }

    // ---- one level -------------------------------------------------------------------------------------------------------
    // Wait for the level on the stream.  With a cancel flag the wait polls it: a cancelled build raises the device-side
    // abort word (on the side stream), the margin kernels still queued or running drain without work, and the call
    // returns AH_ERR_CANCELLED as soon as the stream is idle (src/writer.rs:1178,1196 poll per node / per item).
    int wait_level() {
        if (!opt->cancel) {
            AH_HIP(hipEventSynchronize(bc.ev_level));
            return AH_OK;
        }
        for (uint32_t spins = 0;; spins++) {
            const hipError_t e = hipEventQuery(bc.ev_level);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) {
                set_error("forest build: %s", hipGetErrorString(e));
                return AH_ERR_DEVICE;
            }
            if (*opt->cancel && !abort_sent) {
                AH_HIP(hipMemcpyAsync(d_small.p, h_one, 4, hipMemcpyHostToDevice, bc.side));
                abort_sent = true;
            }
            if (spins < 4096) std::this_thread::yield();
            else std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        if (abort_sent || *opt->cancel) {
            set_error("build cancelled");
            return AH_ERR_CANCELLED;
        }
        return AH_OK;
    }

    // plan the level (level_plan.h): the margin mode of its first attempt, its row-major launches, the tail in groups?
    void plan_current(Level &lv) {
        shape.n_nodes = lv.n_nodes;
        shape.pairs = info.pairs;
        shape.prev_rows = prev_rows;
        shape.grouped = grouped;
        shape.fork_now = fork_now;
        // (a launch carries at most 2^32 - 1 work-items: threads x row tiles x column tiles of the shape the level would take)
        const DensePlan dp_legal = dense_plan(N, std::max(lv.n_nodes, 1u));
        shape.dense_grid_legal = (dp_legal.grid + 64) * (uint64_t)dp_legal.threads < 0xFFFFFFFFull && dp_legal.grid < 0x7FFFFFFFull;
        shape.tree_first = tree_first.data();
        lv.plan = plan_level(shape, knobs);
        tree_first = lv.plan.tree_first;  // (with its gaps closed where the LDS variant was wanted)
    }

    // Everything the level puts on the stream: its tiles, up to four attempts, the scatter, the next level's table and sizes.
    int launch_level(Level &lv) {
        const uint32_t n_nodes = lv.n_nodes, n_tiles = lv.n_tiles;
        const LevelPlan &plan = lv.plan;
        const unsigned tile_grid = std::min<uint32_t>(n_tiles, knobs.tile_blocks);
        // The node-major margin kernels walk their tiles with a persistent grid: at the deep levels a tile is ~1200 items
        // (~2 MB of rows) and launching one workgroup per tile — 819 000 of them at level 13 of the 10M x 100 build — cost
        // 20 % of the level (measured: 306 -> 236 ms, the same 1.70 TB of fabric reads, TCC_EA0_RDREQ).  The small
        // bookkeeping kernels keep one tile per block (their random 1-byte / 4-byte gathers want every block in flight),
        // except the byte -> mask conversion of the top levels, whose reads are still nearly sequential.
        const unsigned node_grid = knobs.node_blocks ? std::min<uint32_t>(n_tiles, knobs.node_blocks)
                                                     : std::min<uint32_t>(n_tiles, std::max<uint32_t>(2048u, std::min<uint32_t>(65536u, n_tiles / 16u)));
        const unsigned masks_grid = n_nodes <= 4 * n_trees ? std::min<uint32_t>(tile_grid, 32768u) : tile_grid;
        const uint64_t rec_bytes = shape.rec_bytes;
        const uint64_t nodes_per_tree = (n_nodes + n_trees - 1) / n_trees;
        const uint32_t row_tc = plan.row_tc, lds_tc = plan.lds_tc;
        const bool dense = plan.dense;
        hipLaunchKernelGGL(k_build_tiles, dim3(std::min<uint32_t>((n_nodes + 3) / 4, kMaxBlocks)), dim3(256), 0, s, d_cur,
                           n_nodes, d_tiles.p);
        uint8_t *chunk_d = nullptr, *shadow_d = nullptr, *shadow8_d = nullptr;
        const uint64_t chunk_bytes = (uint64_t)n_nodes * nstride;
        const uint64_t chunk_host_off = normals_base + normals_bytes;
        AH_TRY(arena.take(chunk_bytes, &chunk_d));
        if (screen) AH_TRY(shadow_arena.take((uint64_t)n_nodes * hstride, &shadow_d));
        if (screen8) AH_TRY(shadow8_arena.take((uint64_t)n_nodes * stride8, &shadow8_d));
        normals_bytes += chunk_bytes;
        lv.chunk_d = chunk_d, lv.chunk_bytes = chunk_bytes, lv.chunk_host_off = chunk_host_off;
        if (forest->want_device) {  // (a resident forest: the records stay where they are until resident_stage has read them)
            res_chunks.push_back(ResidentChunk{chunk_host_off, n_nodes});
            res_chunk_dev.push_back(chunk_d);
        }
        // Host side of the normals: reserved now; the pages of THIS level's records were started one level ago (a level has
        // about twice the nodes of the one before), those of the NEXT level start now — committing the 2.6 GB of the deepest
        // level takes longer than the ~160 ms that level runs, and the loop must not wait for page faults before it can
        // hand a chunk to the read-back worker.  Whatever the prediction missed is faulted in by the worker itself.
        if (!sb) AH_TRY(reserve_normals(chunk_host_off + chunk_bytes, chunk_host_off));
        if (!sb && depth == 0) touch_normals[0].start(forest->normals_blob, chunk_host_off, chunk_bytes);
        if (!sb) {
            // next level: twice the nodes while the nodes are large; once they hold fewer than 2 x split_after items on
            // average most children are Descendants and the next level is a remnant (an eighth); nothing below that
            const uint64_t next_begin = chunk_host_off + chunk_bytes;
            const double avg_items = n_nodes ? (double)info.pairs / (double)n_nodes : 0.0;
            const uint64_t predicted = avg_items > 2.0 * split_after ? 2 * chunk_bytes : avg_items > (double)split_after ? chunk_bytes / 8 : 0;
            const uint64_t next_len = normals_cap > next_begin ? std::min<uint64_t>(normals_cap - next_begin, predicted) : 0;
            touch_normals[(step + 1) & 1].start(forest->normals_blob, next_begin, (size_t)next_len);
        }
        LevelBufs lb{dv, sv, ds->metric, ds->device, s, N, n_trees, n_nodes, n_tiles, d_cur, d_tiles.p, cur, chunk_d, nstride, hdr_off,
                     shadow_d, hstride, shadow8_d, stride8, masks.p, tile_left.p, node_of.p, side_bytes.p, side_bits.p, d_counters,
                     d_abort, d_abort, verify};
        for (int attempt = 0; attempt < 4; attempt++) {
            // (attempts 1-3: gated by the number of nodes the attempt before left pending, d_small[attempt])
            const uint32_t *gate = attempt && knobs.retry_gate ? d_small.p + attempt : nullptr;
            lb.abort_gated = AbortFlags{d_small.p, gate};
            AH_TRY(launch_create_split(lb, split_metric, std::min<uint32_t>(n_nodes, knobs.split_blocks), cs_shared));
            AH_DBG(s, "create_split");
            if (screen)
                hipLaunchKernelGGL(k_forest_shadow_normals, dim3(std::min<uint32_t>(n_nodes, attempt ? 65536u : 1u << 20)), dim3(64), 0, s,
                                   dv, d_cur, chunk_d, nstride, hdr_off, shadow_d, hstride, sv.hpitch, n_nodes, gate);
            // the int8 records are only read by the node-major screen: the first attempt of a row-order level skips them
            if (screen8 && !(attempt == 0 && row_tc >= 2))
                hipLaunchKernelGGL(k_forest_shadow_normals8, dim3(std::min<uint32_t>(n_nodes, 65536u)), dim3(64), 0, s, dv, d_cur,
                                   n_nodes, chunk_d, nstride, hdr_off, ds->d_dim_scale, shadow8_d, stride8, sv.pitch8, gate);
            AH_HIP(hipEventRecord(bc.ev_attempt[2 * attempt], s));
            if (attempt == 0 && row_tc >= 2) {
                // one pass over the rows serves up to row_tc trees (see k_forest_margin_rows)
                if (prev_rows && knobs.rows_advance) {
                    hipLaunchKernelGGL(k_forest_advance_node_of, dim3(kMaxBlocks), dim3(kBlock), 0, s, node_of.p, side_bytes.p,
                                       d_child.p, (uint64_t)n_trees * N);
                    if (info.n_fix)
                        hipLaunchKernelGGL(k_forest_assign_node_of, dim3(std::min<uint32_t>(n_tiles, kMaxBlocks)), dim3(kBlock), 0,
                                           s, d_cur, d_tiles.p, n_tiles, cur, N, node_of.p, 1u);
                } else {
                    AH_HIP(hipMemsetAsync(node_of.p, 0xFF, (size_t)n_trees * N * 4, s));
                    hipLaunchKernelGGL(k_forest_assign_node_of, dim3(tile_grid), dim3(kBlock), 0, s, d_cur, d_tiles.p, n_tiles,
                                       cur, N, node_of.p, 0u);
                }
                uint32_t passes = dense ? 1u : 0u;  // (row-major: one per group of trees)
                for (const RowsLaunch &l : plan.launches) passes += l.groups;
                if (dense) {
                    AH_TRY(launch_dense(lb, dense_plan(N, n_nodes), knobs.exact_wide, forest->stats));
                } else if (screen) {
                    if (lds_tc) {
                        memcpy(h_tree_first, tree_first.data(), ((size_t)n_trees + 1) * 4);
                        AH_HIP(hipMemcpyAsync(d_tree_first_fixed, h_tree_first, ((size_t)n_trees + 1) * 4, hipMemcpyHostToDevice, s));
                    }
                    AH_TRY(launch_rows_screened(lb, plan, nodes_per_tree, rec_bytes, d_tree_first_fixed, knobs.lds_normals_bytes, forest->stats));
                } else {
                    AH_TRY(launch_rows_f32(lb, plan, rec_bytes, (unsigned)std::min<uint64_t>((N + 31) / 32, knobs.row_blocks),
                                           knobs.lds_normals_bytes, forest->stats));
                }
                if (side_bits.p) {
                    const uint64_t n_words = ((uint64_t)n_trees * N + 31) / 32;
                    hipLaunchKernelGGL(k_forest_pack_sides, dim3((uint32_t)std::min<uint64_t>((n_words + 255) / 256, 1u << 16)),
                                       dim3(256), 0, s, side_bytes.p, n_words, side_bits.p);
                }
                hipLaunchKernelGGL(k_forest_masks_from_bytes, dim3(masks_grid), dim3(kBlock), 0, s, d_cur, d_tiles.p, n_tiles,
                                   cur, N, side_bytes.p, side_bits.p, masks.p, tile_left.p);
                forest->stats.margin_row_passes += passes;
                if (screen) forest->stats.screened_launches += passes;
            } else {
                // rows of at most six 128-byte int8 steps (768 dimensions): the pipelined variant of the int8 stage
                const bool node_pre = screen8 && ds->metric != AH_DOT_PRODUCT && sv.pitch8 <= 6 * 128 && knobs.node_prefetch;
                AH_TRY(launch_node_major(lb, bq, screen, screen8, node_pre, node_grid, forest->stats));
            }
            AH_HIP(hipEventRecord(bc.ev_attempt[2 * attempt + 1], s));
            AH_DBG(s, "margin");
            hipLaunchKernelGGL(k_forest_decide, dim3((n_nodes + 255) / 256), dim3(256), 0, s, d_cur, n_nodes,
                               attempt < 3 ? d_small.p + attempt + 1 : nullptr, gate);
            AH_DBG(s, "decide");
        }
        hipLaunchKernelGGL(k_forest_random_sides, dim3(std::min<uint32_t>(n_tiles, kMaxBlocks)), dim3(64), 0, s, d_cur,
                           d_tiles.p, n_tiles, masks.p, tile_left.p);
        AH_DBG(s, "random_sides");
        hipLaunchKernelGGL(k_forest_tile_offsets, dim3(std::min<uint32_t>(n_nodes, kMaxBlocks)), dim3(64), 0, s, d_cur,
                           n_nodes, tile_left.p, tile_left_off.p);
        AH_DBG(s, "tile_offsets");
        hipLaunchKernelGGL(k_forest_scatter, dim3(tile_grid), dim3(kBlock), 0, s, d_cur, d_tiles.p, n_tiles, cur, nxt,
                           final_perm.p, N, masks.p, tile_left_off.p, split_after);
        AH_DBG(s, "scatter");
        // the next level, on the device (its node table lands in the buffer the level before this one used: the side-stream
        // copy of that table must be over)
        if (step >= 1) AH_HIP(hipStreamWaitEvent(s, bc.ev_copy[(step + 1) & 1], 0));
        // (a group's first level emits into the table the group before it may have finished in: that copy is one step old)
        if (grouped && step >= 1) AH_HIP(hipStreamWaitEvent(s, bc.ev_copy[step & 1], 0));
        const uint32_t n_blocks = (n_nodes + 255) / 256;
        hipLaunchKernelGGL(k_next_count, dim3(n_blocks), dim3(256), 0, s, d_cur, n_nodes, split_after, d_block_sums.p);
        hipLaunchKernelGGL(k_next_scan, dim3(1), dim3(1024), 0, s, d_block_sums.p, n_blocks, d_info, d_tree_first, n_trees,
                           d_small.p + 1);
        hipLaunchKernelGGL(k_next_emit, dim3(n_blocks), dim3(256), 0, s, d_cur, n_nodes, split_after, d_block_sums.p, d_next,
                           d_child.p, d_info, d_tree_first);
        AH_DBG(s, "next_level");
        AH_HIP(hipGetLastError());
        AH_HIP(hipMemcpyAsync(h_info[step & 1], d_info, z.info_words * 4, hipMemcpyDeviceToHost, s));
        AH_HIP(hipEventRecord(bc.ev_level, s));
        return AH_OK;
    }

    // While the level runs: room for the records of the two digests to come (the level before this one, now; this one, under
    // the next level), the ids of the group before this one, then the node tables (and node lists) the level covers.
    int under_level(Level &lv) {
        records.grow_ahead(lv.n_nodes, ring.tables);
        lv.t_launched = std::chrono::steady_clock::now();
        // the group before this one is complete (its last level was waited for): its ids travel under this group's kernels
        AH_TRY(hand_over_pending());
        AH_TRY(digest_under(info.pairs));
        lv.t_digested = std::chrono::steady_clock::now();
        return AH_OK;
    }

    // The wait, the level's timings, its node table onto the side stream and its normals to the worker, the next level's sizes.
    int after_level(const Level &lv) {
        const uint32_t n_nodes = lv.n_nodes, row_tc = lv.plan.row_tc, lds_tc = lv.plan.lds_tc;
        const bool dense = lv.plan.dense;
        AH_TRY(wait_level());
        const auto t_waited = std::chrono::steady_clock::now();
        t_prev_waited = t_waited;
        float attempt_ms[4] = {0.f, 0.f, 0.f, 0.f};
        for (int attempt = 0; attempt < 4; attempt++) {
            float m = 0.0f;
            if (hipEventElapsedTime(&m, bc.ev_attempt[2 * attempt], bc.ev_attempt[2 * attempt + 1]) == hipSuccess) {
                forest->stats.seconds_margin += m * 1e-3;
                attempt_ms[attempt] = m;
            }
        }
        if (timing >= 2)
            fprintf(stderr, "[ah] level %2u: %8u nodes %12llu pairs  mode %s  margin pass %.2f ms (+ retries %.2f) = %.3f ns per pair\n",
                    depth, n_nodes, (unsigned long long)info.pairs,
                    dense ? "dense-mfma" : lds_tc ? "rows-lds" : row_tc >= 2 ? "rows" : "node-major", attempt_ms[0],
                    attempt_ms[1] + attempt_ms[2] + attempt_ms[3], info.pairs ? attempt_ms[0] * 1e6 / (double)info.pairs : 0.0);
        if (timing >= 3) {
            fprintf(stderr, "[ah]          host: after the previous wait %.2f ms, launch %.2f ms, under the level (ids handed over, tables digested, node lists) %.2f ms, wait %.2f ms\n",
                    lv.ms_tail_prev, ms_of(lv.t_top, lv.t_launched), ms_of(lv.t_launched, lv.t_digested), ms_of(lv.t_digested, t_waited));
        }
        forest->stats.margin_launches += 4;
        // this level's node table follows on the side stream (the level is complete: no stream dependency needed)
        size_t table_off = 0;
        const size_t table_bytes = ((size_t)n_nodes * sizeof(FNode) + 4095) & ~(size_t)4095;
        while (!ring.alloc(table_bytes, &table_off)) AH_TRY(digest_front());  // (no room: the oldest tables first)
        AH_HIP(hipMemcpyAsync(ring_base + table_off, d_cur, n_nodes * sizeof(FNode), hipMemcpyDeviceToHost, bc.side));
        AH_HIP(hipEventRecord(bc.ev_copy[step & 1], bc.side));
        // (a millisecond at most — and it must not queue behind the gigabytes of normals the worker is about to request: the
        // digest of this table runs under the NEXT level, which at the bottom of the forest is a short one)
        if (n_nodes >= 65536) AH_HIP(hipEventSynchronize(bc.ev_copy[step & 1]));
        ring.tables.push_back(PendingTable{depth, step, n_nodes, table_off, lv.chunk_host_off, lv.chunk_d,
                                           group_first_level ? (int64_t)group_n0 : -1, false, -1});
        // this level's normals are final: the worker copies them while the next level runs
        touch_normals[step & 1].join();  // never touch a page the worker may already have filled
        if (!sb) rb.push(forest->normals + lv.chunk_host_off, lv.chunk_d, lv.chunk_bytes);  // (streaming: pushed by the level's digest)

        const LevelInfo *hi = h_info[step & 1];
        info = *hi;
        const uint32_t *tf = reinterpret_cast<const uint32_t *>(hi + 1);
        for (uint32_t t = 0; t <= n_trees; t++) tree_first[t] = tf[t];
        prev_rows = row_tc >= 2;
        std::swap(cur, nxt);
        std::swap(d_cur, d_next);
        if (group_first_level) {  // the group's first table was a slice of the level's: from here on it has two of its own
            d_next = group_spare;
            group_first_level = false;
        }
        depth++;
        step++;
        return AH_OK;
    }

    // One level = one set of launches, and ONE host wait.  Ends with the forest (or the group) complete, or — fork_now — with
    // a level handed back unlaunched for run_tail_groups to cut into groups of trees.
    int run_levels() {
        while (info.n_nodes) {
            if (opt->cancel && *opt->cancel) {
                set_error("build cancelled");
                return AH_ERR_CANCELLED;  // Error::BuildCancelled
            }
            AH_REQUIRE(depth < 100000, AH_ERR_DEVICE, "forest build: depth %u exceeded (internal error)", depth);
            if (sb && (sb->target.sink_rc.load() || sb->target.too_big.load())) break;  // reported after the loop
            Level lv;
            lv.t_top = std::chrono::steady_clock::now();
            lv.ms_tail_prev = std::chrono::duration<double, std::milli>(lv.t_top - t_prev_waited).count();
            lv.n_nodes = info.n_nodes, lv.n_tiles = info.n_tiles;
            AH_REQUIRE(lv.n_nodes <= z.max_nodes && lv.n_tiles <= z.max_tiles, AH_ERR_DEVICE, "forest build: node / tile bound exceeded");
            plan_current(lv);
            if (lv.plan.fork) {
                fork_now = true;
                return AH_OK;
            }
            AH_TRY(launch_level(lv));
            AH_TRY(under_level(lv));
            AH_TRY(after_level(lv));
        }
        return AH_OK;
    }

    // ---- the tail in groups of trees (AH_BUILD_TAIL_GROUPS) ----------------------------------------------------------
    // The item ids of a tree are final with its last scatter, and 95 % of them (10M x 768 x 100 trees) are still under
    // splitting nodes when the last big level starts: level by level, the 4 GB of ids and the 2.6 GB of that level's
    // normals leave the device after the last launch — 0.10 s of 1.43.  So the last big level and whatever follows it
    // run GROUP BY GROUP (contiguous ranges of trees, each to its end): the ids and normals of group g travel while
    // group g + 1 computes, and only the last group's are left for the tail.  A group is a level-by-level build of fewer
    // trees over the same tables: its nodes are a slice of the level's table (tile indices rebased by k_fork_groups), its
    // levels always node-major (they are by then), its records digested like any level's.  The forest is the same node
    // for node — trees never interact — only the order of the normals in the blob (and the ids of a streaming build)
    // follows the order of the launches.
    void enter_group(const TailGroup &g) {  // everything the level loop reads that a group starts anew
        info = g.info;
        d_cur = g.table;
        d_next = g.other;
        cur = g.cur;
        nxt = g.nxt;
        depth = g.depth;
        prev_rows = false;
        grouped = true;
        group_first_level = true;
        group_n0 = g.n0;
        group_spare = d_nodes_c.p;
    }
    int run_tail_groups() {
        if (!fork_now) return AH_OK;
        group_tree = tail_group_trees(n_trees, knobs.tail_groups, tun(TUN_TAIL_RATIO));
        const uint32_t K = (uint32_t)group_tree.size() - 1;
        GroupCuts cuts{};
        for (uint32_t g = 0; g <= K; g++) cuts.first[g] = g < K ? tree_first[group_tree[g]] : info.n_nodes;
        AH_TRY(d_nodes_c.ensure(z.nodes));
        AH_TRY(d_groups.ensure(32));
        AH_HIP(hipMemsetAsync(d_nodes_c.p, 0, z.nodes * sizeof(FNode), s));  // (zeros: see the tables above)
        hipLaunchKernelGGL(k_fork_groups, dim3(K), dim3(256), 0, s, d_cur, cuts, d_groups.p);
        GroupInfo gi[32];
        AH_HIP(hipMemcpyAsync(gi, d_groups.p, K * sizeof(GroupInfo), hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        // the records of the level's nodes: the children's list of the level before it, digested under the first group
        if (!ring.tables.empty()) ring.tables.back().fork_parent = true;
        else records.level_rec_full.swap(records.level_rec);
        TailGroup start{LevelInfo{}, d_cur, d_next, cur, nxt, depth, 0u};
        forest->stats.tail_groups += K;
        if (timing)
            fprintf(stderr, "[ah] tail: level %u on (%u nodes, %llu pairs) in %u groups of trees\n", depth, info.n_nodes,
                    (unsigned long long)info.pairs, K);
        for (uint32_t g = 0; g < K; g++) {
            TailGroup grp = start;
            grp.n0 = cuts.first[g];
            grp.table = start.table + grp.n0;
            grp.info.n_nodes = cuts.first[g + 1] - cuts.first[g];
            grp.info.n_tiles = gi[g].n_tiles;
            grp.info.n_fix = gi[g].n_fix;
            grp.info.pairs = gi[g].pairs;
            enter_group(grp);
            AH_TRY(run_levels());
            if (sb && (sb->target.sink_rc.load() || sb->target.too_big.load())) break;  // reported after the loop
            // its ids: handed over under the next group's first level (the last group's: after the loop); its node list (the
            // leaves' job of a streaming build): when its last table has been digested
            pending_hand = (int)g;
            if (!ring.tables.empty()) ring.tables.back().group_done = (int)g;
        }
        return AH_OK;
    }

    // ---- after the last launch ---------------------------------------------------------------------------------------------
    // Results come back with plain D2H copies straight into their final place — no host-side repacking:
    //   normals      one copy per level chunk (device record layout == caller-visible layout), already under way
    //   descendants  the final permutations themselves (rows -> item ids on device first)
    std::chrono::steady_clock::time_point t_tail_prefault, t_tail_sync, t_levels;
    float device_ms = 0.0f;
    int finish_device() {
        AH_HIP(hipEventRecord(bc.ev_end, s));
        t_loop_end = std::chrono::steady_clock::now();
        prefault.join();
        t_tail_prefault = std::chrono::steady_clock::now();
        if (!sb) forest->descendants_len = desc_base + M;
        // trees that are a single Descendants node never went through a scatter: their list is the input itself
        // (a tail in groups has no such tree, and its ids were converted group by group)
        for (uint32_t t = 0; t < n_trees && !fork_now; t++)
            if (records.recs[records.tree_root[t]].kind == AH_NODE_DESCENDANTS && tree_base[t + 1] > tree_base[t])
                AH_HIP(hipMemcpyAsync(final_perm.p + tree_base[t], perm_a.p + tree_base[t],
                                      (tree_base[t + 1] - tree_base[t]) * 4, hipMemcpyDeviceToDevice, s));
        if (!ds->identity_ids && M && !fork_now)
            hipLaunchKernelGGL(k_rows_to_ids, dim3(2048), dim3(256), 0, s, final_perm.p, M, ds->d_ids);
        ScreenCounters sc{};
        AH_HIP(hipMemcpyAsync(&sc, d_counters, sizeof sc, hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        t_tail_sync = std::chrono::steady_clock::now();
        forest->stats.screen_fallbacks += sc.fallbacks;
        forest->stats.screen_violations += sc.violations;
        forest->stats.screen8_pairs += sc.stage8_pairs;
        forest->stats.screen8_decided += sc.stage8_decided;
        forest->stats.screen8b_decided += sc.stage8b_decided;
        if (!sb && !fork_now) rb.push(forest->descendants + desc_base, final_perm.p, M * 4);  // lands while the host emits the node list
        if (fork_now) AH_TRY(hand_over_pending());  // (the last group's)
        // the last level's node table is digested only now: the 4 GB of item ids are already on their way
        AH_TRY(digest_under(~0ull));
        if (sb && !fork_now) AH_TRY(push_leaves_job(0, n_trees));  // (in groups: every group's job followed its last table)
        t_levels = std::chrono::steady_clock::now();
        AH_HIP(hipEventElapsedTime(&device_ms, bc.ev_begin, bc.ev_end));
        forest->stats.seconds_device += device_ms * 1e-3;
        return AH_OK;
    }
    // no node list, no blobs: the roots, the counts, and the worker's verdict
    int finish_streamed() {
        const uint32_t id_base = records.id_base;
        records.count_records();
        forest->stats.split_nodes += records.n_split;
        forest->stats.descendant_nodes += records.n_desc;
        for (uint32_t t = 0; t < n_trees; t++) sb->roots[first_tree + t] = id_base + records.tree_root[t];
        AH_REQUIRE((uint64_t)id_base + records.n_recs < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "more than 2^32 tree nodes in one build");
        sb->id_base = id_base + (uint32_t)records.n_recs;
        const hipError_t rb_err = rb.drain();
        AH_REQUIRE(rb_err != hipErrorOutOfMemory, AH_ERR_OUT_OF_MEMORY, "host allocation failed in the encoded stream");
        AH_REQUIRE(rb_err == hipSuccess, AH_ERR_DEVICE, "device -> host copy of the forest failed");
        AH_REQUIRE(!sb->target.too_big.load(), AH_ERR_INVALID_ARGUMENT,
                   "a Descendants node holds more item ids than the streaming buffer (split_after too large for ah_build_forest_stream)");
        AH_REQUIRE(!sb->target.sink_rc.load(), AH_ERR_CANCELLED, "node sink asked to stop (code %d)", sb->target.sink_rc.load());
        forest->stats.seconds_after_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop_end).count();
        if (timing)
            fprintf(stderr, "[ah] streamed batch of %u trees: %.3f s (device %.3f), %llu sink calls, %.2f GB handed over\n", n_trees,
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t_batch).count(), device_ms * 1e-3,
                    (unsigned long long)sb->target.batches, sb->target.bytes / 1e9);
        return AH_OK;
    }
    // A resident forest: this batch's share of the device copy (ForestDevice), once its node list is complete and while the
    // read-back of its last chunks is still under way.  The planes of every level, read where the level left them, become rows
    // in view order — the host uploads one 16-byte entry per plane (forest_resident.h) — and the batch's permutation becomes
    // the ids at desc_base.  No memory for it = no device copy: the forest is an ordinary one and the build goes on.
    int resident_stage() {
        if (!forest->want_device) return AH_OK;
        ForestDevice &fd = forest->dev;
        const uint32_t hf = header_floats(ds->metric);
        const size_t row_bytes = ds->row_bytes();
        ResidentPlan plan;
        std::vector<ResidentEntry> entries;
        DevMem table, grown_rows, grown_hdrs;
        bool ok = desc_base + M <= fd.ids_len;
        try {
            ok = ok && resident_plan(forest->nodes.data() + records.node_base, forest->nodes.size() - records.node_base, res_chunks, nstride,
                                     fd.n_rows, desc_base, M, &plan);
            if (ok) {
                entries.resize(plan.rows.size());
                for (size_t i = 0; i < entries.size(); i++)
                    entries[i] = ResidentEntry{res_chunk_dev[plan.rows[i].chunk] + (uint64_t)plan.rows[i].index * nstride, plan.rows[i].row, 0u};
            }
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        const uint32_t total = ok ? fd.n_rows + (uint32_t)entries.size() : 0u;
        if (ok && total > forest->dev_rows_cap)  // exactly the rows so far: an index may adopt the blocks as its own
            ok = dev_malloc(&grown_rows.p, (size_t)total * row_bytes, true) == hipSuccess &&
                 dev_malloc(&grown_hdrs.p, (size_t)total * hf * 4, true) == hipSuccess;
        if (ok && !entries.empty()) ok = dev_malloc(&table.p, entries.size() * sizeof(ResidentEntry), true) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            forest->release_device();
            return AH_OK;
        }
        // Everything below is queued on `s`; a failure waits for the stream before the blocks above are freed, and the forest's
        // pointers change only after the last wait.
        struct StreamWait {
            hipStream_t s;
            bool armed = true;
            ~StreamWait() {
                if (armed) (void)hipStreamSynchronize(s);
            }
        } wait_on_failure{s};
        AH_HIP(hipEventRecord(bc.ev_attempt[0], s));
        void *rows_to = grown_rows.p ? grown_rows.p : fd.rows;
        float *hdrs_to = grown_rows.p ? grown_hdrs.as<float>() : fd.hdrs;
        if (grown_rows.p && fd.n_rows) {  // (a later batch: the rows of the batches before it move)
            AH_HIP(hipMemcpyAsync(rows_to, fd.rows, (size_t)fd.n_rows * row_bytes, hipMemcpyDeviceToDevice, s));
            AH_HIP(hipMemcpyAsync(hdrs_to, fd.hdrs, (size_t)fd.n_rows * hf * 4, hipMemcpyDeviceToDevice, s));
        }
        if (M) AH_HIP(hipMemcpyAsync(fd.ids + desc_base, final_perm.p, M * 4, hipMemcpyDeviceToDevice, s));
        if (!entries.empty()) {
            AH_HIP(hipMemcpyAsync(table.p, entries.data(), entries.size() * sizeof(ResidentEntry), hipMemcpyHostToDevice, s));
            const size_t valid_bytes = ah_vector_size(ds->metric, ds->dims);
            const bool wide = (nstride % 16) == 0 && (row_bytes % 16) == 0 && (valid_bytes % 16) == 0;
            const uint32_t unit = wide ? 16u : 4u;
            for_spans(entries.size(), std::min<uint64_t>(IndexCall::span(), 1ull << 30), [&](uint64_t lo, uint64_t hi) {
                if (wide)
                    hipLaunchKernelGGL(k_resident_rows<uint4>, dim3((unsigned)(hi - lo)), dim3(256), 0, s, table.as<const ResidentEntry>(), (uint32_t)lo,
                                       (uint32_t)hi, hdr_off, (uint32_t)(valid_bytes / unit), (uint32_t)(row_bytes / unit), hf, total,
                                       reinterpret_cast<uint4 *>(rows_to), hdrs_to);
                else
                    hipLaunchKernelGGL(k_resident_rows<uint32_t>, dim3((unsigned)(hi - lo)), dim3(256), 0, s, table.as<const ResidentEntry>(),
                                       (uint32_t)lo, (uint32_t)hi, hdr_off, (uint32_t)(valid_bytes / unit), (uint32_t)(row_bytes / unit), hf, total,
                                       reinterpret_cast<uint32_t *>(rows_to), hdrs_to);
            });
            AH_HIP(hipGetLastError());
        }
        AH_HIP(hipEventRecord(bc.ev_attempt[1], s));
        AH_HIP(hipStreamSynchronize(s));  // (the table and the levels' records are read no more)
        wait_on_failure.armed = false;
        if (grown_rows.p) {  // the grown blocks become the forest's; the old ones go when the stage returns
            std::swap(grown_rows.p, fd.rows);
            void *old_hdrs = fd.hdrs;
            fd.hdrs = grown_hdrs.as<float>();
            grown_hdrs.p = old_hdrs;
            forest->dev_rows_cap = total;
            fd.bytes = std::max<uint64_t>(1, fd.ids_len) * 4 + (uint64_t)total * (row_bytes + (uint64_t)hf * 4);
        }
        fd.n_rows = total;
        float stage_ms = 0.0f;
        if (hipEventElapsedTime(&stage_ms, bc.ev_attempt[0], bc.ev_attempt[1]) == hipSuccess) forest->stats.seconds_device += stage_ms * 1e-3;
        if (timing)
            fprintf(stderr, "[ah] resident stage: %zu planes -> rows, %llu ids: %.3f ms on the device\n", entries.size(), (unsigned long long)M, stage_ms);
        return AH_OK;
    }
    // the node list of the trees not emitted yet (all of them, unless the tail ran in groups), then the copies still in flight
    int finish_materialised() {
        AH_TRY(emit_range(records.emit_tree, n_trees));
        AH_REQUIRE(records.emit_cursor - records.node_base == records.n_recs, AH_ERR_DEVICE,
                   "forest build: %zu nodes emitted of %zu (internal error)", records.emit_cursor - records.node_base, records.n_recs);
        AH_TRY(resident_stage());
        forest->stats.split_nodes += records.n_split;
        forest->stats.descendant_nodes += records.n_desc;
        const auto t_emitted = std::chrono::steady_clock::now();
        AH_REQUIRE(rb.drain() == hipSuccess, AH_ERR_DEVICE, "device -> host copy of the forest failed");
        forest->normals_len = normals_base + normals_bytes;
        touch_normals[0].join();  // (the last level started the commit of a level that never came)
        touch_normals[1].join();
        // (the head-room of the blob stays mapped: untouched pages cost nothing, and the pool hands the whole blob to the next build)
        forest->stats.host_blob_recycled += (forest->normals_blob.recycled ? 1u : 0u) + (forest->desc_blob.recycled ? 1u : 0u);
        forest->stats.seconds_after_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop_end).count();
        if (timing) {
            const auto t_end = std::chrono::steady_clock::now();
            fprintf(stderr, "[ah] batch of %u trees: levels %.3f s (device %.3f; after the last launch: ids' pages %.3f, stream %.3f, last "
                            "digest %.3f), emit %.3f s, read-back still in flight after it %.3f s (%.2f GB normals%s, %.2f GB ids%s)\n",
                    n_trees, sec(t_batch, t_levels), device_ms * 1e-3, sec(t_loop_end, t_tail_prefault), sec(t_tail_prefault, t_tail_sync),
                    sec(t_tail_sync, t_levels), sec(t_levels, t_emitted), sec(t_emitted, t_end), normals_bytes / 1e9,
                    forest->normals_blob.committed ? ", recycled pages" : "", M * 4 / 1e9,
                    forest->desc_blob.committed ? ", recycled pages" : "");
        }
        return AH_OK;
    }
};

static int build_batch(ah_dataset *ds, const ah_build_options *opt, uint32_t first_tree, uint32_t n_trees,
                       uint32_t split_after, ah_forest *forest, Context *ctx, const uint32_t *subset_ids,
                       const uint64_t *subset_offsets, StreamBuild *sb = nullptr) {
    BatchBuild b(ds, opt, first_tree, n_trees, split_after, forest, ctx, subset_ids, subset_offsets, sb);
    AH_TRY(b.setup_device());
    AH_TRY(b.setup_host());
    AH_TRY(b.seed_roots());
    AH_TRY(b.run_levels());
    AH_TRY(b.run_tail_groups());
    AH_TRY(b.finish_device());
    return sb ? b.finish_streamed() : b.finish_materialised();
}

extern "C" {

// The blocks of a resident forest's device copy: the ids whole (their number is known before the build), one row for the
// batches to grow from.  false: no memory — the forest will be an ordinary one.
static bool forest_device_begin(ah_forest *forest, const ah_dataset *ds, uint64_t total_ids) {
    if (total_ids >= 0xFFFFFFFFull) return false;  // (no index takes such a forest)
    ForestDevice &fd = forest->dev;
    const uint32_t hf = header_floats(ds->metric);
    fd.device = ds->device;
    fd.metric = ds->metric;
    fd.dims = ds->dims;
    const bool ok = dev_malloc((void **)&fd.ids, std::max<uint64_t>(1, total_ids) * 4, true) == hipSuccess &&
                    dev_malloc(&fd.rows, ds->row_bytes(), true) == hipSuccess && dev_malloc((void **)&fd.hdrs, (size_t)hf * 4, true) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        forest->release_device();
        return false;
    }
    fd.ids_len = total_ids;
    forest->dev_rows_cap = 1;
    fd.bytes = std::max<uint64_t>(1, total_ids) * 4 + ds->row_bytes() + (uint64_t)hf * 4;
    forest->want_device = true;
    return true;
}

static int build_forest_impl(ah_dataset *ds, const ah_build_options *options, const uint32_t *subset_ids,
                             const uint64_t *subset_offsets, ah_forest **out, StreamBuild *sb = nullptr, bool resident = false) {
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(ds && options, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    AH_REQUIRE(ds->finalized, AH_ERR_NOT_FINALIZED, "dataset not finalized (call ah_dataset_finalize)");
    AH_REQUIRE(options->n_trees == 0 || options->tree_seeds, AH_ERR_INVALID_ARGUMENT, "tree_seeds is NULL");
    {
        const uint32_t m = options->margin_mode & 0xFFFu;
        AH_REQUIRE((options->margin_mode & ~(0xFFFu | AH_MARGIN_EXACT_ONLY)) == 0 &&
                       (m == AH_MARGIN_AUTO || m == AH_MARGIN_NODE_MAJOR || m == AH_MARGIN_ROWS_2 || m == AH_MARGIN_ROWS_4 ||
                        m == AH_MARGIN_ROWS_8 || m == AH_MARGIN_ROWS_16 || m == AH_MARGIN_ROWS_LDS_8 || m == AH_MARGIN_ROWS_LDS_16 ||
                        m == AH_MARGIN_DENSE_MFMA),
                   AH_ERR_INVALID_ARGUMENT, "unknown margin_mode 0x%x", options->margin_mode);
    }
    AH_REQUIRE(ds->metric != AH_DOT_PRODUCT || ds->dot_preprocessed, AH_ERR_NEED_PREPROCESS,
               "DotProduct needs ah_preprocess_dot before the build (src/writer.rs:964-976)");
    AH_HIP(hipSetDevice(ds->device));
    {
        const auto tw = std::chrono::steady_clock::now();
        ds->join_reserve();  // (ah_dataset_reserve_build still filling the cache)
        ds->reserve_wait_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    }
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t split_after = options->split_after ? options->split_after : ds->dims;  // src/writer.rs:474-477
    ah_forest *forest = new (std::nothrow) ah_forest();
    AH_REQUIRE(forest, AH_ERR_OUT_OF_MEMORY, "host allocation failed");
    forest->normal_vector_offset = 0;
    forest->normal_header_offset = ds->row_bytes();
    forest->normal_stride = normal_record_stride(ds);
    int st = AH_OK;
    if (resident && !sb)
        (void)forest_device_begin(forest, ds, subset_ids ? (options->n_trees ? subset_offsets[options->n_trees] - subset_offsets[0] : 0)
                                                         : ds->n * options->n_trees);
    if (!subset_ids && ds->n <= split_after) {
        // fit_in_descendant at the root (src/writer.rs:1183-1188): every tree is one Descendants node
        const uint64_t total = sb ? ds->n : ds->n * options->n_trees;  // (streaming: one copy of the id list serves every tree)
        if (!host_blob_reserve(forest->desc_blob, total * 4, 0)) {
            delete forest;
            set_error("host allocation failed");
            return AH_ERR_OUT_OF_MEMORY;
        }
        forest->descendants = reinterpret_cast<uint32_t *>(forest->desc_blob.p);
        forest->descendants_len = total;
        if (sb) {
            for (uint64_t i = 0; i < ds->n; i++) forest->descendants[i] = ds->identity_ids ? (uint32_t)i : ds->h_ids[i];
            // encoded stream: the one list every tree shares becomes one value (the same kernels as ah_encode_descendants)
            std::vector<uint8_t> value;
            if (sb->encoded && options->n_trees) {
                const uint64_t lists[2] = {0, ds->n};
                uint64_t ends[2] = {0, 0};
                st = encode_id_lists(ds, forest->descendants, lists, 1, nullptr, 0, ends);
                if (st == AH_OK) {
                    value.resize(ends[1]);
                    st = encode_id_lists(ds, forest->descendants, lists, 1, value.data(), value.size(), ends);
                }
            }
            for (uint32_t t = 0; t < options->n_trees && st == AH_OK; t++) {
                ah_stream_node sn{};
                sn.id = sb->id_base + t;
                sn.tree = t;
                sn.kind = AH_NODE_DESCENDANTS;
                sn.count = (uint32_t)ds->n;
                ah_node_batch batch{};
                batch.kind = AH_NODE_DESCENDANTS;
                batch.n_nodes = 1;
                batch.nodes = &sn;
                batch.payload = reinterpret_cast<const uint8_t *>(forest->descendants);
                batch.payload_len = ds->n * 4;
                batch.normal_stride = forest->normal_stride;
                batch.normal_header_offset = forest->normal_header_offset;
                if (sb->encoded) {
                    batch.payload = value.data();
                    batch.payload_len = value.size();
                    batch.normal_stride = batch.normal_header_offset = 0;
                }
                const int rc = sb->target.sink(sb->target.user, &batch);
                if (rc != 0) {
                    set_error("node sink asked to stop (code %d)", rc);
                    st = AH_ERR_CANCELLED;
                }
                sb->roots[t] = sb->id_base + t;
                forest->stats.descendant_nodes++;
            }
        }
        for (uint32_t t = 0; t < options->n_trees && !sb; t++) {
            for (uint64_t i = 0; i < ds->n; i++)
                forest->descendants[t * ds->n + i] = ds->identity_ids ? (uint32_t)i : ds->h_ids[i];
            ah_node nd{};
            nd.kind = AH_NODE_DESCENDANTS;
            nd.tree = t;
            nd.count = (uint32_t)ds->n;
            nd.offset = t * ds->n;
            forest->roots.push_back((uint32_t)forest->nodes.size());
            forest->nodes.push_back(nd);
            forest->stats.descendant_nodes++;
        }
        if (forest->want_device && total) {  // the same lists on the device: every tree's is the dataset's ids in row order
            ContextLease lease(ds);
            hipError_t e = lease.c ? hipSuccess : hipErrorUnknown;
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_init_perm, dim3(64), dim3(256), 0, lease.c->stream, forest->dev.ids, ds->n, options->n_trees);
                if (!ds->identity_ids) hipLaunchKernelGGL(k_rows_to_ids, dim3(64), dim3(256), 0, lease.c->stream, forest->dev.ids, total, ds->d_ids);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(lease.c->stream);
            }
            if (e != hipSuccess) forest->release_device();
        }
    } else if (options->n_trees) {
        ContextLease lease(ds);
        if (!lease.c) {
            set_error("cannot create a HIP stream");
            st = AH_ERR_DEVICE;
        } else {
            // the binary16 shadow of the rows is made (once per dataset) before the batch is sized against free memory
            if (!(options->margin_mode & AH_MARGIN_EXACT_ONLY) && tun(TUN_SCREEN)) (void)ensure_screen(ds, lease.c->stream, true, true);
            // Trees in flight: bounded by HBM (per item and tree: 3 permutations + node index + side byte + masks = 18
            // bytes, plus the normals of all levels and their shadow) or by the caller.
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            free_b += dev_cache_idle_bytes(ds->device);  // idle blocks of the caching allocator are ours to use
            uint32_t batch = options->n_trees;
            if (!subset_ids) {
                uint64_t per_tree =
                    ds->n * 18 + ((ds->n / ((uint64_t)split_after + 1)) + 2) * 3 * (ds->row_bytes() + 192) + (1u << 20);
                // a resident forest: its rows while they grow (the old and the new block of a later batch) next to the arena
                if (forest->want_device) per_tree += ((ds->n / ((uint64_t)split_after + 1)) + 2) * 2 * 2 * (ds->row_bytes() + 8);
                uint64_t fit = (uint64_t)(free_b * 0.8) / per_tree;
                if (fit < 1) fit = 1;
                batch = (uint32_t)std::min<uint64_t>(fit, options->n_trees);
            }
            if (options->max_trees_in_flight) batch = std::min(batch, options->max_trees_in_flight);
            try {
                for (uint32_t first = 0; first < options->n_trees && st == AH_OK; first += batch) {
                    const auto tb = std::chrono::steady_clock::now();
                    st = build_batch(ds, options, first, std::min(batch, options->n_trees - first), split_after, forest,
                                     lease.c, subset_ids, subset_offsets, sb);
                    if (tun(TUN_TIMING))
                        fprintf(stderr, "[ah] build: %.1f ms before the batch, the batch and the teardown of its buffers %.1f ms\n",
                                std::chrono::duration<double, std::milli>(tb - t0).count(),
                                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count());
                }
            } catch (const std::bad_alloc &) {
                set_error("host allocation failed during the forest build");
                st = AH_ERR_OUT_OF_MEMORY;
            }
        }
    }
    if (st != AH_OK) {
        delete forest;
        return st;
    }
    forest->has_device = forest->want_device;  // (every batch has added its share)
    forest->stats.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    {  // the reserve helper's figures go to the first build that joined it
        std::lock_guard<std::mutex> lk(ds->mu);
        forest->stats.seconds_reserve = ds->reserve_seconds;
        forest->stats.seconds_reserve_wait = ds->reserve_wait_seconds;
        ds->reserve_seconds = ds->reserve_wait_seconds = 0.0;
    }
    *out = forest;
    return AH_OK;
}

// ah_dataset_reserve_build: the device memory the first build of this dataset will ask for — the binary16 / int8 copies of the
// rows and the scratch of an `n_trees`-tree batch — obtained NOW, on a helper thread, and parked in the caching allocator.
// Meant to be called right after ah_dataset_create, while the records are still being staged over PCIe: fresh HBM costs the
// driver 20+ ms per GB on a box whose memory was recently released (r04: 59 GB of fresh blocks put 1.3 s in front of a cold
// 10M x 100-tree build's first launch and stretched its kernels from 1.33 to 1.8 s); under the 0.6 s of staging it is free.
// The batch's sizes are the build's own (batch_sizes, forest_records.h: one struct read by both); only the screen's copies
// restate ensure_screen / ensure_screen8, where a mismatch would cost the cache hit and nothing else.
int ah_dataset_reserve_build(ah_dataset *ds, uint32_t n_trees, uint32_t split_after_opt) {
    AH_GUARDED("ah_dataset_reserve_build")
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    ds->join_reserve();
    const uint64_t N = std::max<uint64_t>(ds->n, ds->capacity);
    if (N == 0 || n_trees == 0 || tun(TUN_DEVICE_CACHE_MB) <= 0) return AH_OK;
    const uint32_t split_after = split_after_opt ? split_after_opt : ds->dims;
    std::vector<size_t> sizes;
    const bool f32 = !metric_is_bq(ds->metric) && ds->dims >= 32;
    const bool want_screen = f32 && tun(TUN_SCREEN) != 0 && !ds->d_rows_h16;
    const uint32_t hpitch = (ds->dims + 63u) & ~63u, pitch8 = (ds->dims + 127u) & ~127u;
    if (want_screen) {  // ensure_screen / ensure_screen8
        sizes.push_back(N * (size_t)hpitch * 2);
        sizes.push_back(N * sizeof(float4));
        if (ds->metric != AH_DOT_PRODUCT && tun(TUN_SCREEN8) != 0) {
            if (tun(TUN_SCREEN8_LO) != 0) sizes.push_back(N * (size_t)pitch8);
            sizes.push_back(N * (size_t)pitch8);
            sizes.push_back(N * sizeof(float));
        }
    }
    // one batch of n_trees full-dataset trees, in the order BatchBuild::setup_device and the level loop ask (the pinned host
    // memory of that batch — node tables, level info, the read-back worker's double buffer — is z.pinned_bytes())
    const bool f32_rows = f32 && n_trees >= 2;
    const BatchSizes z = batch_sizes(N, n_trees, (uint64_t)n_trees * N, split_after, normal_record_stride(ds), shadow_stride16(hpitch),
                                     shadow_stride8(pitch8), f32_rows, tun(TUN_MASK_BITS) > 0 || (tun(TUN_MASK_BITS) < 0 && N >= (1u << 20)),
                                     tun(TUN_READBACK_MB));
    {
        auto buf = [&](uint64_t n, size_t elem) { sizes.push_back((size_t)std::max<uint64_t>(n, 1024) * elem); };  // (DevBuf's floor)
        buf(z.perm, 4); buf(z.perm, 4); buf(z.perm, 4);
        buf(z.nodes, sizeof(FNode)); buf(z.nodes, sizeof(FNode));
        buf(z.tiles, sizeof(FTile));
        buf(z.masks, 8);
        buf(z.tile_left, 4); buf(z.tile_left, 4);
        buf(z.child, 4);
        buf(z.block_sums, sizeof(NextCounts));
        if (f32_rows) {
            buf(z.node_of, 4);
            buf(z.side_bytes, 1);
            if (z.side_bits) buf(z.side_bits, 4);
        }
        sizes.push_back((size_t)z.arena_block);
        if (f32 && tun(TUN_SCREEN) != 0) {
            sizes.push_back((size_t)z.shadow_block);
            sizes.push_back((size_t)z.shadow_block);  // (a 100-tree 10M build takes a second block for its deepest levels)
            if (ds->metric != AH_DOT_PRODUCT && tun(TUN_SCREEN8) != 0) sizes.push_back((size_t)z.shadow8_block);
        }
    }
    const size_t pinned_bytes = z.pinned_bytes();
    const int device = ds->device;
    double *const took = &ds->reserve_seconds;  // (the handle outlives the helper: every build and the destroy join it)
    try {
        std::thread helper([device, sizes, took, pinned_bytes] {
            const auto th = std::chrono::steady_clock::now();
            if (hipSetDevice(device) != hipSuccess) return;
            pinned_spare_fill(device, pinned_bytes);
            std::vector<void *> got;
            for (size_t b : sizes) {
                void *p = nullptr;
                if (dev_malloc(&p, b) != hipSuccess) {  // no room: the build will see for itself
                    (void)hipGetLastError();
                    break;
                }
                got.push_back(p);
            }
            for (void *p : got) (void)dev_free_unused(p);
            *took += std::chrono::duration<double>(std::chrono::steady_clock::now() - th).count();
        });
        std::thread stale;  // (a helper another thread started since the join above: wait for that one too)
        {
            std::lock_guard<std::mutex> lk(ds->mu);
            stale = std::move(ds->reserve_thread);
            ds->reserve_thread = std::move(helper);
        }
        if (stale.joinable()) stale.join();
    } catch (...) {  // no thread: the first build allocates as before
    }
    return AH_OK;
    AH_GUARDED_END
}

int ah_build_forest(ah_dataset *ds, const ah_build_options *options, ah_forest **out) {
    AH_GUARDED("ah_build_forest")
    return build_forest_impl(ds, options, nullptr, nullptr, out);
    AH_GUARDED_END
}

// The same build with the node sink inside it (include/arroy_hip.h, "Streaming build"): nothing is materialised.
// ... and with the device copy an index is made from kept (include/arroy_hip.h, "Resident forests")
int ah_build_forest_resident(ah_dataset *ds, const ah_build_options *options, ah_forest **out) {
    AH_GUARDED("ah_build_forest_resident")
    return build_forest_impl(ds, options, nullptr, nullptr, out, nullptr, true);
    AH_GUARDED_END
}

int ah_build_forest_stream(ah_dataset *ds, const ah_build_options *options, ah_node_batch_fn sink, void *user,
                           uint32_t *out_roots, ah_build_stats *out_stats) {
    AH_GUARDED("ah_build_forest_stream")
    AH_REQUIRE(sink, AH_ERR_INVALID_ARGUMENT, "sink is NULL");
    AH_REQUIRE(options && (out_roots || options->n_trees == 0), AH_ERR_INVALID_ARGUMENT, "NULL argument");
    StreamBuild sb;
    sb.target.sink = sink;
    sb.target.user = user;
    sb.roots = out_roots;
    ah_forest *forest = nullptr;
    const int st = build_forest_impl(ds, options, nullptr, nullptr, &forest, &sb);
    if (st == AH_OK && out_stats) *out_stats = forest->stats;
    delete forest;
    return st;
    AH_GUARDED_END
}

// The streaming build with the NodeCodec values encoded on the device (include/arroy_hip.h, "Encoded node stream").
int ah_build_forest_stream_encoded(ah_dataset *ds, const ah_build_options *options, const ah_encode_options *enc,
                                   ah_node_batch_fn sink, void *user, uint32_t *out_roots, ah_build_stats *out_stats) {
    AH_GUARDED("ah_build_forest_stream_encoded")
    AH_REQUIRE(sink, AH_ERR_INVALID_ARGUMENT, "sink is NULL");
    AH_REQUIRE(enc && options && (out_roots || options->n_trees == 0), AH_ERR_INVALID_ARGUMENT, "NULL argument");
    AH_REQUIRE(enc->flags == 0, AH_ERR_INVALID_ARGUMENT, "ah_encode_options.flags must be 0");
    AH_REQUIRE((uint64_t)enc->node_id_base + options->n_trees <= 0x100000000ull, AH_ERR_INVALID_ARGUMENT,
               "node_id_base + the nodes of this build pass 2^32 - 1");
    StreamBuild sb;
    sb.target.sink = sink;
    sb.target.user = user;
    sb.roots = out_roots;
    sb.encoded = true;
    sb.id_base = enc->node_id_base;
    ah_forest *forest = nullptr;
    const int st = build_forest_impl(ds, options, nullptr, nullptr, &forest, &sb);
    if (st == AH_OK && out_stats) *out_stats = forest->stats;
    delete forest;
    return st;
    AH_GUARDED_END
}

// `incremental_index_large_descendant` (src/writer.rs:660-739) for many descendants at once: tree t of the result is
// `make_tree_in_file` over the ascending id list item_ids[offsets[t] .. offsets[t+1]).
static int build_subtrees_impl(ah_dataset *ds, const ah_build_options *options, const uint32_t *item_ids, const uint64_t *offsets,
                               ah_forest **out, bool resident) {
    AH_REQUIRE(options, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    AH_REQUIRE((item_ids && offsets) || options->n_trees == 0, AH_ERR_INVALID_ARGUMENT, "NULL id lists");
    for (uint32_t t = 0; t < options->n_trees; t++) {
        AH_REQUIRE(offsets[t + 1] >= offsets[t], AH_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing");
        for (uint64_t i = offsets[t] + 1; i < offsets[t + 1]; i++)
            AH_REQUIRE(item_ids[i] > item_ids[i - 1], AH_ERR_INVALID_ARGUMENT,
                       "sub-tree id lists must be strictly ascending (RoaringBitmap order)");
    }
    static const uint32_t dummy = 0;
    return build_forest_impl(ds, options, item_ids ? item_ids : &dummy, offsets, out, nullptr, resident);
}
int ah_build_subtrees(ah_dataset *ds, const ah_build_options *options, const uint32_t *item_ids, const uint64_t *offsets,
                      ah_forest **out) {
    AH_GUARDED("ah_build_subtrees")
    return build_subtrees_impl(ds, options, item_ids, offsets, out, false);
    AH_GUARDED_END
}
int ah_build_subtrees_resident(ah_dataset *ds, const ah_build_options *options, const uint32_t *item_ids, const uint64_t *offsets,
                               ah_forest **out) {
    AH_GUARDED("ah_build_subtrees_resident")
    return build_subtrees_impl(ds, options, item_ids, offsets, out, true);
    AH_GUARDED_END
}

int ah_forest_view_get(const ah_forest *forest, ah_forest_view *out) {
    AH_GUARDED("ah_forest_view_get")
    AH_REQUIRE(forest && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    out->n_trees = (uint32_t)forest->roots.size();
    out->n_nodes = forest->nodes.size();
    out->roots = forest->roots.data();
    out->nodes = forest->nodes.data();
    out->normals = forest->normals;
    out->normals_len = forest->normals_len;
    out->normal_stride = forest->normal_stride;
    out->normal_vector_offset = forest->normal_vector_offset;
    out->normal_header_offset = forest->normal_header_offset;
    out->descendants = forest->descendants;
    out->descendants_len = forest->descendants_len;
    return AH_OK;
    AH_GUARDED_END
}

// ---- content digest ---------------------------------------------------------------------------------------------------
namespace {
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// 64-bit hash of a byte range: four multiply-rotate lanes over 32-byte blocks (a plain word-at-a-time chain would bound the
// digest of a 10 GB forest by the multiplier's latency), folded with the splitmix finaliser of arroy_hip_policy.h
uint64_t hash_bytes(const void *data, size_t len, uint64_t seed) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(data);
    uint64_t h0 = seed ^ 0x9E3779B97F4A7C15ull, h1 = seed + 0xC2B2AE3D27D4EB4Full, h2 = ~seed, h3 = seed * 0x165667B19E3779F9ull + len;
    size_t i = 0;
    for (; i + 32 <= len; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        h0 = rotl64((h0 ^ w[0]) * 0x9FB21C651E98DF25ull, 29);
        h1 = rotl64((h1 ^ w[1]) * 0xD6E8FEB86659FD93ull, 31);
        h2 = rotl64((h2 ^ w[2]) * 0xBF58476D1CE4E5B9ull, 27);
        h3 = rotl64((h3 ^ w[3]) * 0x94D049BB133111EBull, 33);
    }
    uint64_t tail[4] = {0, 0, 0, 0};
    if (i < len) memcpy(tail, p + i, len - i);
    h0 = (h0 ^ tail[0]) * 0x9FB21C651E98DF25ull;
    h1 = (h1 ^ tail[1]) * 0xD6E8FEB86659FD93ull;
    h2 = (h2 ^ tail[2]) * 0xBF58476D1CE4E5B9ull;
    h3 = (h3 ^ tail[3]) * 0x94D049BB133111EBull;
    return ah_mix64(ah_mix64(h0 ^ rotl64(h1, 17)) + ah_mix64(h2 ^ rotl64(h3, 41)) + len);
}
}  // namespace

static int forest_digest_impl(const ah_forest *forest, const uint64_t *tree_keys, uint64_t *out_per_tree, uint64_t *out_total);
int ah_forest_digest(const ah_forest *forest, uint64_t *out_per_tree, uint64_t *out_total) {
    AH_GUARDED("ah_forest_digest")
    return forest_digest_impl(forest, nullptr, out_per_tree, out_total);
    AH_GUARDED_END
}
int ah_forest_digest_keyed(const ah_forest *forest, const uint64_t *tree_keys, uint64_t *out_per_tree) {
    AH_GUARDED("ah_forest_digest_keyed")
    AH_REQUIRE(tree_keys, AH_ERR_INVALID_ARGUMENT, "tree_keys is NULL");
    return forest_digest_impl(forest, tree_keys, out_per_tree, nullptr);
    AH_GUARDED_END
}
static int forest_digest_impl(const ah_forest *forest, const uint64_t *tree_keys, uint64_t *out_per_tree, uint64_t *out_total) {
    AH_REQUIRE(forest && (out_per_tree || out_total), AH_ERR_INVALID_ARGUMENT, "NULL argument");
    const uint32_t n_trees = (uint32_t)forest->roots.size();
    const size_t n_nodes = forest->nodes.size();
    // the nodes of a tree are contiguous and the trees ascend (BatchRecords::emit_range emits tree by tree)
    std::vector<size_t> first(n_trees + 1, n_nodes);
    for (size_t i = n_nodes; i-- > 0;) {
        const uint32_t t = forest->nodes[i].tree;
        AH_REQUIRE(t < n_trees, AH_ERR_INVALID_ARGUMENT, "forest digest: node %zu names tree %u of %u", i, t, n_trees);
        first[t] = i;
    }
    for (uint32_t t = n_trees; t-- > 0;) first[t] = std::min(first[t], first[t + 1]);
    // header bytes of a record: up to the 16-byte slot, but only the metric's own floats are content (the rest is zero
    // padding either way); vector bytes: everything before the header
    const size_t vec_off = forest->normal_vector_offset, hdr_off = forest->normal_header_offset;
    const size_t vec_len = hdr_off > vec_off ? hdr_off - vec_off : 0;
    const size_t hdr_len = std::min<size_t>(8, forest->normal_stride - hdr_off);
    std::vector<uint64_t> per(n_trees, 0);
    std::atomic<uint32_t> next{0};
    auto work = [&](unsigned) {
        for (;;) {
            const uint32_t t = next.fetch_add(1, std::memory_order_relaxed);
            if (t >= n_trees) break;
            // the tree's identity is part of the content (seeds are per tree): its index in this forest, or the caller's key
            uint64_t h = ah_mix64(0x61727279ull + (tree_keys ? tree_keys[t] : (uint64_t)t));
            const size_t base = first[t];
            for (size_t i = first[t]; i < first[t + 1]; i++) {
                const ah_node &nd = forest->nodes[i];
                if (nd.tree != t) continue;
                uint64_t f[4] = {(uint64_t)nd.kind | (uint64_t)nd.has_normal << 8 | (uint64_t)nd.depth << 32, nd.count, 0, 0};
                if (nd.kind == AH_NODE_SPLIT) {
                    f[2] = nd.left - base;  // children by their position inside the tree
                    f[3] = nd.right - base;
                }
                h = ah_mix64(h ^ hash_bytes(f, sizeof f, i - base));
                if (nd.kind == AH_NODE_SPLIT) {
                    if (nd.has_normal) {
                        const uint8_t *rec = forest->normals + nd.offset;
                        h = ah_mix64(h ^ hash_bytes(rec + vec_off, vec_len, 1));
                        h = ah_mix64(h ^ hash_bytes(rec + hdr_off, hdr_len, 2));
                    }
                } else {
                    h = ah_mix64(h ^ hash_bytes(forest->descendants + nd.offset, (size_t)nd.count * 4, 3));
                }
            }
            per[t] = h;
        }
    };
    parallel_run(n_nodes < 100000 ? 1u : std::min({n_trees, (uint32_t)std::max<long long>(1, tun(TUN_HOST_THREADS)),
                                                    std::max(1u, std::thread::hardware_concurrency())}),
                 work);
    uint64_t total = ah_mix64(n_trees);
    for (uint32_t t = 0; t < n_trees; t++) {
        total = ah_mix64(total ^ per[t]);
        if (out_per_tree) out_per_tree[t] = per[t];
    }
    if (out_total) *out_total = total;
    return AH_OK;
}

// Test aid: the block -> work-item maps of the build's launches, run on the device (see include/arroy_hip.h).
int ah_debug_launch_coverage(int device, int kind, uint64_t n_rows, uint32_t dims, uint32_t a, uint32_t b, uint32_t *out_counts,
                             uint64_t out_len) {
    AH_GUARDED("ah_debug_launch_coverage")
    AH_REQUIRE(out_counts && n_rows && dims, AH_ERR_INVALID_ARGUMENT, "NULL / empty argument");
    AH_HIP(hipSetDevice(device));
    const uint32_t hpitch = (dims + 63u) & ~63u;
    uint64_t need = 0;
    DensePlan dp{};
    if (kind == 0) {
        AH_REQUIRE((a == 2 || a == 4 || a == 8 || a == 16) && b >= 1, AH_ERR_INVALID_ARGUMENT, "kind 0: a = trees per group, b = groups");
        need = (uint64_t)b * n_rows;
    } else if (kind == 1) {
        AH_REQUIRE(a >= 1, AH_ERR_INVALID_ARGUMENT, "kind 1: a = columns");
        dp = dense_plan(n_rows, a);
        AH_REQUIRE(dp.grid < 0x7FFFFFFFull, AH_ERR_INVALID_ARGUMENT, "too many tiles for one launch");
        need = (uint64_t)dp.n_row_tiles * dp.n_col_tiles;
    } else if (kind == 2) {
        AH_REQUIRE(a >= 1, AH_ERR_INVALID_ARGUMENT, "kind 2: a = trees");
        need = (uint64_t)a * ((n_rows + 1023) >> 10);
    } else {
        AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "unknown coverage kind %d", kind);
    }
    AH_REQUIRE(out_len >= need, AH_ERR_INVALID_ARGUMENT, "out_counts holds %llu counters, %llu needed", (unsigned long long)out_len,
               (unsigned long long)need);
    DevMem d;
    AH_HIP(dev_malloc(&d.p, need * 4));
    AH_HIP(hipMemset(d.p, 0, need * 4));
    if (kind == 0) {
        RowsPlan plan;
        // normals of a group as the build would size them for a level with 64 nodes per tree (only the nt policy reads it)
        const uint64_t hstride = ((uint64_t)hpitch * 2 + 16 + 127) & ~(uint64_t)127;
        AH_TRY(plan_rows_launches(n_rows, hpitch, a, b, false, (uint64_t)a * 64 * hstride, &plan));
        for (const auto &l : plan.launches) {
            plan.sch.chunk0 = l.first;
            hipLaunchKernelGGL(k_rows_schedule_coverage, dim3(l.second), dim3(plan.threads), 0, 0, plan.sch, n_rows, d.as<uint32_t>());
        }
    } else if (kind == 1) {
        hipLaunchKernelGGL(k_dense_coverage, dim3((unsigned)dp.grid), dim3(64), 0, 0, dp.group, dp.n_col_tiles, dp.n_row_tiles, d.as<uint32_t>());
    } else {
        hipLaunchKernelGGL(k_exact_coverage, dim3(exact_pairs_grid(n_rows, a)), dim3(256), 0, 0, n_rows, a, d.as<uint32_t>());
    }
    AH_HIP(hipGetLastError());
    AH_HIP(hipDeviceSynchronize());
    AH_HIP(hipMemcpy(out_counts, d.p, need * 4, hipMemcpyDeviceToHost));
    return AH_OK;
    AH_GUARDED_END
}

int ah_debug_dense_tiles(uint64_t n_rows, uint32_t n_cols, uint32_t *out_tile_rows, uint32_t *out_tile_cols) {
    AH_GUARDED("ah_debug_dense_tiles")
    AH_REQUIRE(n_rows && n_cols && out_tile_rows && out_tile_cols, AH_ERR_INVALID_ARGUMENT, "NULL / empty argument");
    const DensePlan dp = dense_plan(n_rows, n_cols);
    *out_tile_rows = dp.tile_rows;
    *out_tile_cols = dp.tile_cols;
    return AH_OK;
    AH_GUARDED_END
}

int ah_forest_stats(const ah_forest *forest, ah_build_stats *out) {
    AH_GUARDED("ah_forest_stats")
    AH_REQUIRE(forest && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = forest->stats;
    return AH_OK;
    AH_GUARDED_END
}

// payload: SPLIT -> the normal record (vector at normal_vector_offset, header at normal_header_offset) or
// NULL for `normal: None`; DESCENDANTS -> u32 item ids.
int ah_forest_visit(const ah_forest *forest, ah_node_sink_fn sink, void *user) {
    AH_GUARDED("ah_forest_visit")
    AH_REQUIRE(forest && sink, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (size_t i = 0; i < forest->nodes.size(); i++) {
        const ah_node &nd = forest->nodes[i];
        const void *payload = nullptr;
        size_t len = 0;
        if (nd.kind == AH_NODE_SPLIT) {
            if (nd.has_normal) {
                payload = forest->normals + nd.offset;
                len = forest->normal_stride;
            }
        } else {
            payload = forest->descendants + nd.offset;
            len = (size_t)nd.count * 4;
        }
        const int rc = sink(user, nd.tree, (uint32_t)i, nd.kind, nd.left, nd.right, payload, len);
        AH_REQUIRE(rc == 0, AH_ERR_CANCELLED, "node sink asked to stop (code %d)", rc);
    }
    return AH_OK;
    AH_GUARDED_END
}

int ah_forest_resident_info(const ah_forest *forest, int *out_resident, uint64_t *out_device_bytes) {
    AH_GUARDED("ah_forest_resident_info")
    AH_REQUIRE(forest, AH_ERR_INVALID_ARGUMENT, "forest is NULL");
    if (out_resident) *out_resident = forest->has_device ? 1 : 0;
    if (out_device_bytes) *out_device_bytes = forest->has_device ? forest->dev.bytes : 0;
    return AH_OK;
    AH_GUARDED_END
}

int ah_forest_release_device(ah_forest *forest) {
    AH_GUARDED("ah_forest_release_device")
    AH_REQUIRE(forest, AH_ERR_INVALID_ARGUMENT, "forest is NULL");
    forest->release_device();
    return AH_OK;
    AH_GUARDED_END
}

int ah_forest_destroy(ah_forest *forest) {
    AH_GUARDED("ah_forest_destroy")
    NoFailScope no_fail;
    delete forest;
    return AH_OK;
    AH_GUARDED_END
}

int ah_device_cache_trim(int device, uint64_t *out_bytes) {
    AH_GUARDED("ah_device_cache_trim")
    const size_t was = dev_cache_trim(device);
    if (out_bytes) *out_bytes = was;
    return AH_OK;
    AH_GUARDED_END
}

int ah_device_cache_stats(int device, uint64_t *out_live_bytes, uint64_t *out_idle_bytes) {
    AH_GUARDED("ah_device_cache_stats")
    if (out_live_bytes) *out_live_bytes = dev_cache_live_bytes(device);
    if (out_idle_bytes) {
        uint64_t idle = 0;
        if (device >= 0) {
            idle = dev_cache_idle_bytes(device);
        } else {
            int n_dev = 0;
            if (hipGetDeviceCount(&n_dev) != hipSuccess) n_dev = 0;
            for (int d = 0; d < n_dev; d++) idle += dev_cache_idle_bytes(d);
        }
        *out_idle_bytes = idle;
    }
    return AH_OK;
    AH_GUARDED_END
}

int ah_host_cache_trim(uint64_t *out_bytes) {
    AH_GUARDED("ah_host_cache_trim")
    const size_t was = host_pool().trim();
    if (out_bytes) *out_bytes = was;
    return AH_OK;
    AH_GUARDED_END
}

// Benchmark harness only: the policy header's generator on the host cores (the rows ah_dataset_fill_synthetic makes in HBM).
int ah_synth_rows_host(uint64_t seed, int distribution, uint64_t first_item, uint64_t n, uint32_t dims, float *out) {
    AH_GUARDED("ah_synth_rows_host")
    AH_REQUIRE(out || n == 0, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    AH_REQUIRE(distribution >= AH_SYNTH_UNIFORM_01 && distribution <= AH_SYNTH_LAST, AH_ERR_INVALID_ARGUMENT,
               "unknown distribution %d", distribution);
    // the per-dataset part of the structured distributions (cluster centres / factor loadings), computed once
    std::vector<int32_t> table(ah_synth_table_len(dims, distribution));
    if (!table.empty()) ah_synth_table_fill(seed, dims, distribution, table.data());
    const int32_t *tab = table.empty() ? nullptr : table.data();
    const unsigned n_threads = (unsigned)std::min<uint64_t>(std::max(1u, std::thread::hardware_concurrency()), std::max<uint64_t>(1, n / 1024));
    parallel_run(std::min(n_threads, 64u), [=](unsigned t) {
        const unsigned parts = std::min(n_threads, 64u);
        const uint64_t lo = n * t / parts, hi = n * (t + 1) / parts;
        for (uint64_t i = lo; i < hi; i++) ah_synth_row(seed, first_item + i, dims, distribution, tab, out + i * dims);
    });
    return AH_OK;
    AH_GUARDED_END
}

}  // extern "C"

namespace ah {
// the index calls' side of a resident forest (index_device.h)
const ForestDevice *forest_device(const ah_forest *forest) { return forest && forest->has_device ? &forest->dev : nullptr; }
void forest_device_consume(ah_forest *forest, bool adopted_ids, bool adopted_rows) { forest->release_device(adopted_ids, adopted_rows); }
}  // namespace ah
