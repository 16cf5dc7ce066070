// index_update.hip — ah_index_delete_items / ah_index_suspend / ah_index_resume (include/arroy_hip.h): the part of an
// incremental `Writer::build` that takes the updated ids out of every tree (`delete_items_from_trees`, src/writer.rs:978-1114)
// done where the forest lives, so that the index of the last build serves the routing of the next one instead of being
// uploaded again.
//
// Shape of a delete ("Deletes on a resident index"); every pass reads the index and writes new memory only:
//   1. bitmap    one bit per listed id over [0, largest listed id];
//   2. levels    the nodes in breadth-first order from the roots (the view carries no depths), one launch per level: what is
//                reachable, and the ranges the two passes below walk level by level;
//   3. count     a wave per Descendants node: ids that stay (ballot + popcount, 64 ids a step);
//   4. resolve   bottom-up, per node (replacement node, Some(count) | None) by the four cases of `delete_items_in_file`
//                (src/writer.rs:1066-1112), with flags `removed` / `put` / `merged`;
//   5. owners    top-down: the node that ends up holding a leaf's ids is its topmost merged ancestor, else the leaf itself;
//                three exclusive scans (scan_device.h) turn the owners' counts into the offsets of the new blob, the
//                changed nodes into the positions of the delta and the put Descendants nodes into the delta's id array;
//   6. write     a wave per leaf copies its survivors, in order, into its owner's segment; a segment filled by several
//                leaves (at most split_after ids) is sorted by one block, in LDS when it fits;
//   7. apply     the new node array, every node's rank among the nodes in use (a fourth scan: the index it would have in a
//                fresh view, which the coin of ah_route_items is keyed by), the sorted roots and the delta; read back; the
//                index's pointers are swapped last.
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "common.h"
#include "index_device.h"
#include "scan_device.h"

using namespace ah;

// what ah_index_delta_get shows: the host's copy of the delta
struct ah_index_delta {
    std::vector<uint32_t> removed, put_index, desc, roots;
    std::vector<ah_node> put;
};

namespace {

constexpr unsigned kIxBlock = 256;       // 4 waves
constexpr uint32_t kNone = 0xFFFFFFFFu;  // the count of a branch that is no single Descendants node (`None`)
constexpr uint32_t kSortLds = 4096;      // ids of a merged segment (or roots) sorted in LDS; longer ones in place in HBM
enum Flag : uint32_t { kReached = 1, kRemoved = 2, kPut = 4, kMerged = 8 };
enum Ctl { CTL_TAIL = 0, CTL_ERR, CTL_LEAVES, CTL_MAX_DESC, CTL_MERGED, CTL_DESC_LEN, CTL_CHANGED, CTL_DELTA_DESC, CTL_WORDS };

struct DeltaEntry {  // one changed node, in node order: kind 0 = removed, else the node as it is now
    uint32_t node, kind, a, b;  // kind: AH_NODE_* | has_normal << 8; a / b: left / right, or offset into the delta's ids / count
};

struct DeleteArgs {
    const DNode *nodes;
    uint32_t n_nodes;
    const uint32_t *desc;
    const uint32_t *bits;  // the listed ids (nullptr: none)
    uint64_t len_bits;
    uint32_t split_after;
    // per node, zeroed before the first kernel
    uint32_t *order;   // the reachable nodes, level by level
    uint32_t *rep;     // the node that stands where this one stood
    uint32_t *cnt;     // ids of the branch if it is one Descendants node, else kNone
    uint32_t *flags;
    uint32_t *own;     // 1 + the merged ancestor that takes this node's ids (0: none)
    uint32_t *seg;     // ids this node holds in the new blob -> (scan) where they start
    uint32_t *chg;     // 1 for a removed or put node -> (scan) its position in the delta
    uint32_t *dseg;    // ids of a put Descendants node -> (scan) where they start in the delta's ids
    uint32_t *cursor;  // ids already placed in a merged node's segment
    uint32_t *merged;  // the merged nodes that stay
    uint32_t *ctl;
    // what the scans gave (set before the write pass): every store into the new blob and the delta is checked against them
    uint32_t new_desc_len, n_changed, delta_desc_len;
};

unsigned grid_of(uint64_t work, uint64_t per_block, unsigned cap) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((work + per_block - 1) / per_block, cap));
}

__global__ __launch_bounds__(kIxBlock) void k_delete_seed(DeleteArgs a, const uint32_t *__restrict__ roots, uint32_t n_trees) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_trees; t += stride) {
        a.order[t] = roots[t];
        a.flags[roots[t]] = kReached;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[CTL_TAIL] = n_trees;
}

// levels: the children of order[begin, end) are appended behind the tail
__global__ __launch_bounds__(kIxBlock) void k_delete_level(DeleteArgs a, uint32_t begin, uint32_t end) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        const DNode nd = a.nodes[a.order[i]];
        if ((nd.kind & 0xFFu) != AH_NODE_SPLIT) continue;
        const uint64_t pos = atomicAdd(&a.ctl[CTL_TAIL], 2u);
        if (pos + 2 > a.n_nodes || nd.a >= a.n_nodes || nd.b >= a.n_nodes) {  // (not a forest: create_from_view has refused it)
            atomicOr(&a.ctl[CTL_ERR], 1u);
            continue;
        }
        a.order[pos] = nd.a;
        a.order[pos + 1] = nd.b;
        a.flags[nd.a] = kReached;
        a.flags[nd.b] = kReached;
    }
}

// count: `descendants -= to_delete` of the leaves among order[lo, hi), a wave each
__global__ __launch_bounds__(kIxBlock) void k_delete_count(DeleteArgs a, uint32_t lo, uint32_t hi) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < hi; i += n_waves) {
        const uint32_t node = a.order[i];
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;  // (wave-uniform)
        uint32_t kept = 0;
        for (uint32_t j0 = 0; j0 < nd.b; j0 += 64) {
            bool keep = false;
            if (j0 + lane < nd.b) {
                const uint32_t id = a.desc[nd.a + j0 + lane];
                keep = !(id < a.len_bits && ((a.bits[id >> 5] >> (id & 31)) & 1u));
            }
            kept += (uint32_t)__popcll(__ballot(keep));
        }
        if (lane == 0) {
            a.rep[node] = node;
            a.cnt[node] = kept;
            if (kept != nd.b) a.flags[node] = kReached | kPut;
        }
    }
}

// resolve: the split nodes among order[begin, end), one level; their children are done
__global__ __launch_bounds__(kIxBlock) void k_delete_resolve(DeleteArgs a, uint32_t begin, uint32_t end) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        const uint32_t node = a.order[i];
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_SPLIT) continue;
        const uint32_t rl = a.rep[nd.a], cl = a.cnt[nd.a], rr = a.rep[nd.b], cr = a.cnt[nd.b];
        if (cl == 0) {  // the left branch is empty: the right one takes this node's place
            a.flags[rl] |= kRemoved;
            a.flags[node] |= kRemoved;
            a.rep[node] = rr;
            a.cnt[node] = cr;
        } else if (cr == 0) {
            a.flags[rr] |= kRemoved;
            a.flags[node] |= kRemoved;
            a.rep[node] = rl;
            a.cnt[node] = cl;
        } else if (cl != kNone && cr != kNone && (uint64_t)cl + cr <= a.split_after) {  // fit_in_descendant: one node
            a.flags[rl] |= kRemoved;
            a.flags[rr] |= kRemoved;
            a.flags[node] |= kPut | kMerged;
            a.rep[node] = node;
            a.cnt[node] = cl + cr;
        } else {
            a.rep[node] = node;
            a.cnt[node] = kNone;
            if (rl != nd.a || rr != nd.b) a.flags[node] |= kPut;
        }
    }
}

// owners: order[begin, end), one level, parents done
__global__ __launch_bounds__(kIxBlock) void k_delete_owners(DeleteArgs a, uint32_t begin, uint32_t end) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        const uint32_t node = a.order[i];
        const DNode nd = a.nodes[node];
        const uint32_t f = a.flags[node];
        const bool split = (nd.kind & 0xFFu) == AH_NODE_SPLIT;
        uint32_t o = a.own[node];
        if ((f & kMerged) && o == 0) o = node + 1;
        if (split) {
            a.own[nd.a] = o;
            a.own[nd.b] = o;
        }
        const bool owner = split ? o == node + 1 : o == 0;
        const uint32_t held = owner ? a.cnt[node] : 0u;
        a.seg[node] = held;
        a.chg[node] = (f & (kRemoved | kPut)) ? 1u : 0u;
        a.dseg[node] = (f & kPut) && !(f & kRemoved) ? held : 0u;
        if (split && owner) {
            const uint32_t m = atomicAdd(&a.ctl[CTL_MERGED], 1u);
            if (m < a.n_nodes) a.merged[m] = node;
        }
    }
}

// write: the survivors of the leaves among order[lo, hi), in order, into their owner's segment (seg: scanned)
__global__ __launch_bounds__(kIxBlock) void k_delete_write(DeleteArgs a, uint32_t lo, uint32_t hi, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < hi; i += n_waves) {
        const uint32_t node = a.order[i];
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;  // (wave-uniform, as is every branch below)
        const uint32_t kept = a.cnt[node];
        if (kept == 0) continue;
        const uint32_t o = a.own[node];
        uint32_t base = a.seg[o ? o - 1 : node];
        if (o) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&a.cursor[o - 1], kept);
            base += __shfl(at, 0, 64);
        }
        for (uint32_t j0 = 0; j0 < nd.b; j0 += 64) {
            bool keep = false;
            uint32_t id = 0;
            if (j0 + lane < nd.b) {
                id = a.desc[nd.a + j0 + lane];
                keep = !(id < a.len_bits && ((a.bits[id >> 5] >> (id & 31)) & 1u));
            }
            const unsigned long long mask = __ballot(keep);
            const uint64_t at = (uint64_t)base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (keep) {
                if (at < a.new_desc_len) out[at] = id;
                else atomicOr(&a.ctl[CTL_ERR], 2u);
            }
            base += (uint32_t)__popcll(mask);
        }
    }
}

// v[0, m) ascending, by the whole block: the bitonic network whose comparators all point one way, so the tail beyond m
// counts as +infinity without being stored
__device__ void block_sort_u32(uint32_t *v, uint32_t m) {
    uint64_t np2 = 2;
    while (np2 < m) np2 <<= 1;
    for (uint64_t k = 2; k <= np2; k <<= 1) {
        for (uint64_t j = k >> 1; j > 0; j >>= 1) {
            for (uint64_t t = threadIdx.x; t < np2 / 2; t += blockDim.x) {
                const uint64_t w = t & (j - 1);
                const uint64_t first = (t - w) * 2 + w;  // the t-th element whose bit j is clear
                const uint64_t second = j == k >> 1 ? first + 2 * (j - w) - 1 : first + j;
                if (second < m) {
                    const uint32_t x = v[first], y = v[second];
                    if (x > y) {
                        v[first] = y;
                        v[second] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}
__device__ void block_sort_segment(uint32_t *v, uint32_t m, uint32_t *lds) {
    if (m < 2) return;  // (block-uniform)
    if (m > kSortLds) {
        block_sort_u32(v, m);
        return;
    }
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) lds[i] = v[i];
    __syncthreads();
    block_sort_u32(lds, m);
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) v[i] = lds[i];
    __syncthreads();
}

// the segments several leaves were written into: l U r ascending, a block each
__global__ __launch_bounds__(kIxBlock) void k_delete_sort(DeleteArgs a, uint32_t n_merged, uint32_t *__restrict__ out) {
    __shared__ uint32_t lds[kSortLds];
    for (uint32_t i = blockIdx.x; i < n_merged; i += gridDim.x) {
        const uint32_t node = a.merged[i];
        if ((uint64_t)a.seg[node] + a.cnt[node] > a.new_desc_len) continue;  // (block-uniform; the write pass has flagged it)
        block_sort_segment(out + a.seg[node], a.cnt[node], lds);
    }
}

// roots.sort_unstable() (src/writer.rs:1001) of the replaced roots; one block
__global__ __launch_bounds__(kIxBlock) void k_delete_roots(DeleteArgs a, const uint32_t *__restrict__ roots, uint32_t n_trees,
                                                           uint32_t *__restrict__ out) {
    __shared__ uint32_t lds[kSortLds];
    for (uint32_t t = threadIdx.x; t < n_trees; t += blockDim.x) out[t] = a.rep[roots[t]];
    __syncthreads();
    block_sort_segment(out, n_trees, lds);
}

// apply: every node as it is afterwards, the changed ones into the delta as well (chg / dseg: scanned)
__global__ __launch_bounds__(kIxBlock) void k_delete_apply(DeleteArgs a, DNode *__restrict__ out, uint32_t *__restrict__ in_use,
                                                           DeltaEntry *__restrict__ entries) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t rounds = (a.n_nodes + stride - 1) / stride;
    uint32_t leaves = 0, largest = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t node = r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        if (node >= a.n_nodes) break;
        const uint32_t f = a.flags[node];
        DNode nd = a.nodes[node];
        const bool alive = (f & kReached) && !(f & kRemoved);
        if (!alive) {
            nd = DNode{0, 0, 0, 0};
        } else if ((nd.kind & 0xFFu) == AH_NODE_SPLIT && !(f & kMerged)) {
            nd.a = a.rep[nd.a];
            nd.b = a.rep[nd.b];
        } else {  // a Descendants node that stays owns its ids (every node below a merged one is removed)
            nd = DNode{AH_NODE_DESCENDANTS, a.seg[node], a.cnt[node], 0};
            leaves++;
            largest = max(largest, nd.b);
        }
        out[node] = nd;
        in_use[node] = alive ? 1u : 0u;
        if (f & (kRemoved | kPut)) {
            DeltaEntry e{node, alive ? nd.kind : 0u, nd.a, nd.b};
            if (alive && (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS) e.a = a.dseg[node];
            if (a.chg[node] < a.n_changed) entries[a.chg[node]] = e;
            else atomicOr(&a.ctl[CTL_ERR], 4u);
        }
    }
    for (uint32_t d = 32; d > 0; d >>= 1) {
        leaves += __shfl_xor(leaves, d, 64);
        largest = max(largest, (uint32_t)__shfl_xor(largest, d, 64));
    }
    if (lane == 0 && leaves) {
        atomicAdd(&a.ctl[CTL_LEAVES], leaves);
        atomicMax(&a.ctl[CTL_MAX_DESC], largest);
    }
}

// the ids of the put Descendants nodes, node after node, for the host; a wave per changed node
__global__ __launch_bounds__(kIxBlock) void k_delete_gather(DeleteArgs a, const DeltaEntry *__restrict__ entries, uint32_t n_changed,
                                                            const uint32_t *__restrict__ blob, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_changed; i += n_waves) {
        const DeltaEntry e = entries[i];
        if ((e.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;
        if (e.node >= a.n_nodes || (uint64_t)e.a + e.b > a.delta_desc_len || (uint64_t)a.seg[e.node] + e.b > a.new_desc_len) {
            if (lane == 0) atomicOr(&a.ctl[CTL_ERR], 8u);
            continue;
        }
        const uint32_t *src = blob + a.seg[e.node];
        for (uint32_t j = lane; j < e.b; j += 64) out[e.a + j] = src[j];
    }
}

int alloc(DevMem *m, size_t bytes) {
    const hipError_t e = dev_malloc(&m->p, std::max<size_t>(bytes, 1));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation of %zu bytes for the index delete failed: %s", bytes, hipGetErrorString(e));
        set_error_status(e == hipErrorOutOfMemory ? AH_ERR_OUT_OF_MEMORY : AH_ERR_DEVICE);
        return e == hipErrorOutOfMemory ? AH_ERR_OUT_OF_MEMORY : AH_ERR_DEVICE;
    }
    return AH_OK;
}

int delete_impl(ah_index *ix, const uint32_t *ids, size_t n, uint32_t split_after, ah_index_delta *delta) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    const bool timing = tun(TUN_TIMING) != 0;
    ah_dataset *ds = ix->ds;
    AH_HIP(hipSetDevice(ds->device));
    ContextLease lease(ds);
    AH_REQUIRE(lease.c, AH_ERR_DEVICE, "cannot create a HIP stream");
    const hipStream_t s = lease.c->stream;
    auto phase_end = [&]() -> std::chrono::steady_clock::time_point {
        if (timing) (void)hipStreamSynchronize(s);
        return now();
    };
    const auto t0 = now();
    const uint32_t nn = ix->n_nodes, n_trees = ix->n_trees;
    const uint64_t old_desc_len = ix->desc_len;
    // every buffer whose size is known now; kernels write only into these
    const uint64_t len_bits = n ? (uint64_t)ids[n - 1] + 1 : 0;
    const size_t bit_words = (size_t)((len_bits + 31) / 32);
    const size_t per_node = (size_t)nn + 1;
    const size_t scan_tiles = (nn + kScanTile - 1) / kScanTile + 1;
    const size_t work_words = 10 * per_node + scan_tiles + CTL_WORDS;
    DevMem bitmap, work, new_nodes, new_roots, new_rank, new_desc, out;
    AH_TRY(alloc(&bitmap, (bit_words + n) * 4));
    AH_TRY(alloc(&work, work_words * 4));
    AH_TRY(alloc(&new_nodes, (size_t)nn * sizeof(DNode)));
    AH_TRY(alloc(&new_roots, (size_t)n_trees * 4));
    AH_TRY(alloc(&new_rank, per_node * 4));
    delta->roots.resize(n_trees);
    uint32_t *w = work.as<uint32_t>();
    DeleteArgs a{};
    a.nodes = ix->d_nodes;
    a.n_nodes = nn;
    a.desc = ix->d_desc;
    a.bits = n ? bitmap.as<const uint32_t>() : nullptr;
    a.len_bits = len_bits;
    a.split_after = split_after;
    uint32_t **fields[10] = {&a.order, &a.rep, &a.cnt, &a.flags, &a.own, &a.seg, &a.chg, &a.dseg, &a.cursor, &a.merged};
    for (int i = 0; i < 10; i++) *fields[i] = w + (size_t)i * per_node;
    uint32_t *tile_sums = w + 10 * per_node;
    a.ctl = tile_sums + scan_tiles;
    AH_HIP(hipMemsetAsync(work.p, 0, work_words * 4, s));
    // 1. bitmap
    if (n) {
        uint32_t *d_ids = bitmap.as<uint32_t>() + bit_words;
        AH_HIP(hipMemsetAsync(bitmap.p, 0, bit_words * 4, s));
        AH_HIP(hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_filter_bitmap, dim3(grid_of(n, kIxBlock, 1024)), dim3(kIxBlock), 0, s, (const uint32_t *)d_ids, (uint64_t)n,
                           bitmap.as<uint32_t>());
    }
    AH_HIP(hipGetLastError());
    const auto t_bitmap = phase_end();
    // 2. levels
    uint32_t ctl[CTL_WORDS];
    std::vector<uint32_t> level_begin;
    uint32_t begin = 0, end = n_trees;
    if (n_trees) hipLaunchKernelGGL(k_delete_seed, dim3(grid_of(n_trees, kIxBlock, 1024)), dim3(kIxBlock), 0, s, a, (const uint32_t *)ix->d_roots, n_trees);
    while (begin < end) {
        level_begin.push_back(begin);
        hipLaunchKernelGGL(k_delete_level, dim3(grid_of(end - begin, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, begin, end);
        AH_HIP(hipGetLastError());
        AH_HIP(hipMemcpyAsync(ctl, a.ctl, 2 * 4, hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        AH_REQUIRE(ctl[CTL_ERR] == 0 && ctl[CTL_TAIL] >= end && ctl[CTL_TAIL] <= nn, AH_ERR_DEVICE,
                   "the nodes of the index are not a forest (a node is reachable twice)");
        begin = end;
        end = ctl[CTL_TAIL];
    }
    level_begin.push_back(end);
    const uint32_t reached = end;
    const size_t levels = level_begin.size() - 1;
    const auto t_levels = now();
    // the passes over every reachable node, a wave each, in launches of at most AH_LAUNCH_MAX_ITEMS nodes
    const uint32_t span = (uint32_t)std::min<long long>(std::max<uint32_t>(reached, 1), std::max<long long>(1, tun(TUN_LAUNCH_MAX_ITEMS)));
    // 3. count
    for (uint32_t lo = 0; lo < reached; lo += span) {
        const uint32_t hi = std::min(reached - lo, span) + lo;
        hipLaunchKernelGGL(k_delete_count, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, lo, hi);
    }
    AH_HIP(hipGetLastError());
    const auto t_count = phase_end();
    // 4. resolve, 5. owners and the scans
    for (size_t l = levels; l-- > 0;)
        hipLaunchKernelGGL(k_delete_resolve, dim3(grid_of(level_begin[l + 1] - level_begin[l], kIxBlock, 4096)), dim3(kIxBlock), 0, s, a,
                           level_begin[l], level_begin[l + 1]);
    for (size_t l = 0; l < levels; l++)
        hipLaunchKernelGGL(k_delete_owners, dim3(grid_of(level_begin[l + 1] - level_begin[l], kIxBlock, 4096)), dim3(kIxBlock), 0, s, a,
                           level_begin[l], level_begin[l + 1]);
    launch_exclusive_scan(a.seg, nn, tile_sums, a.ctl + CTL_DESC_LEN, s);
    launch_exclusive_scan(a.chg, nn, tile_sums, a.ctl + CTL_CHANGED, s);
    launch_exclusive_scan(a.dseg, nn, tile_sums, a.ctl + CTL_DELTA_DESC, s);
    AH_HIP(hipGetLastError());
    AH_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    const auto t_resolve = now();
    const uint32_t desc_len = ctl[CTL_DESC_LEN], n_changed = ctl[CTL_CHANGED], delta_desc = ctl[CTL_DELTA_DESC], n_merged = ctl[CTL_MERGED];
    AH_REQUIRE(desc_len <= old_desc_len && n_changed <= nn && delta_desc <= desc_len && n_merged <= nn, AH_ERR_DEVICE,
               "the index delete counted more ids or nodes than the index holds");
    a.new_desc_len = desc_len;
    a.n_changed = n_changed;
    a.delta_desc_len = delta_desc;
    // the buffers whose size the scans have just given, and the host's
    AH_TRY(alloc(&new_desc, (size_t)desc_len * 4));
    AH_TRY(alloc(&out, (size_t)n_changed * sizeof(DeltaEntry) + (size_t)delta_desc * 4));
    std::vector<DeltaEntry> entries(n_changed);
    delta->desc.resize(delta_desc);
    DeltaEntry *d_entries = out.as<DeltaEntry>();
    uint32_t *d_delta_desc = reinterpret_cast<uint32_t *>(d_entries + n_changed);
    // 6. write
    for (uint32_t lo = 0; lo < reached; lo += span) {
        const uint32_t hi = std::min(reached - lo, span) + lo;
        hipLaunchKernelGGL(k_delete_write, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, lo, hi, new_desc.as<uint32_t>());
    }
    if (n_merged) hipLaunchKernelGGL(k_delete_sort, dim3(grid_of(n_merged, 1, 1u << 16)), dim3(kIxBlock), 0, s, a, n_merged, new_desc.as<uint32_t>());
    // 7. apply
    if (n_trees) hipLaunchKernelGGL(k_delete_roots, dim3(1), dim3(kIxBlock), 0, s, a, (const uint32_t *)ix->d_roots, n_trees, new_roots.as<uint32_t>());
    if (nn)
        hipLaunchKernelGGL(k_delete_apply, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, new_nodes.as<DNode>(),
                           new_rank.as<uint32_t>(), d_entries);
    launch_exclusive_scan(new_rank.as<uint32_t>(), nn, tile_sums, new_rank.as<uint32_t>() + nn, s);
    if (n_changed)
        hipLaunchKernelGGL(k_delete_gather, dim3(grid_of(n_changed, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (const DeltaEntry *)d_entries,
                           n_changed, new_desc.as<const uint32_t>(), d_delta_desc);
    AH_HIP(hipGetLastError());
    const auto t_write = phase_end();
    // read back
    if (n_changed) AH_HIP(hipMemcpyAsync(entries.data(), d_entries, (size_t)n_changed * sizeof(DeltaEntry), hipMemcpyDeviceToHost, s));
    if (delta_desc) AH_HIP(hipMemcpyAsync(delta->desc.data(), d_delta_desc, (size_t)delta_desc * 4, hipMemcpyDeviceToHost, s));
    if (n_trees) AH_HIP(hipMemcpyAsync(delta->roots.data(), new_roots.p, (size_t)n_trees * 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    AH_REQUIRE(ctl[CTL_ERR] == 0, AH_ERR_DEVICE, "the index delete found its own counts inconsistent (%u): the index is unchanged", ctl[CTL_ERR]);
    size_t n_removed = 0;
    for (const DeltaEntry &e : entries) n_removed += e.kind == 0;
    delta->removed.reserve(n_removed);
    delta->put_index.reserve(n_changed - n_removed);
    delta->put.reserve(n_changed - n_removed);
    for (const DeltaEntry &e : entries) {
        if (e.kind == 0) {
            delta->removed.push_back(e.node);
            continue;
        }
        ah_node nd{};
        nd.kind = (uint8_t)(e.kind & 0xFFu);
        if (nd.kind == AH_NODE_SPLIT) {
            nd.has_normal = (e.kind & 0x100u) ? 1 : 0;
            nd.left = e.a;
            nd.right = e.b;
        } else {
            nd.offset = e.a;
            nd.count = e.b;
        }
        delta->put_index.push_back(e.node);
        delta->put.push_back(nd);
    }
    const auto t_read = now();
    {
        // commit: nothing here can fail.  The old arrays go into the DevMems, which free them (dev_free waits for the device).
        NoFailScope no_fail;
        void *old_nodes = ix->d_nodes, *old_roots = ix->d_roots, *old_desc = ix->d_desc, *old_rank = ix->d_rank;
        ix->d_rank = new_rank.as<uint32_t>();
        new_rank.p = old_rank;
        ix->d_nodes = new_nodes.as<DNode>();
        ix->d_roots = new_roots.as<uint32_t>();
        ix->d_desc = new_desc.as<uint32_t>();
        new_nodes.p = old_nodes;
        new_roots.p = old_roots;
        new_desc.p = old_desc;
        ix->desc_len = desc_len;
        ix->n_leaves = ctl[CTL_LEAVES];
        ix->max_desc = ctl[CTL_MAX_DESC];
    }
    if (timing) {
        auto secs = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
            return std::chrono::duration<double>(y - x).count();
        };
        fprintf(stderr, "[ah] index delete: %zu ids, %u of %u nodes reachable in %zu levels, %llu -> %u stored ids, %zu removed + %zu put nodes: "
                        "bitmap %.6f s, levels %.6f s, count %.6f s, resolve %.6f s, write %.6f s, read-back %.6f s\n",
                n, reached, nn, levels, (unsigned long long)old_desc_len, desc_len,
                delta->removed.size(), delta->put.size(), secs(t0, t_bitmap), secs(t_bitmap, t_levels), secs(t_levels, t_count),
                secs(t_count, t_resolve), secs(t_resolve, t_write), secs(t_write, t_read));
    }
    return AH_OK;
}

}  // namespace

extern "C" {

int ah_index_delete_items(ah_index *ix, const uint32_t *sorted_ids, size_t n, uint32_t split_after, ah_index_delta **out_delta) {
    AH_GUARDED("ah_index_delete_items")
    AH_REQUIRE(out_delta, AH_ERR_INVALID_ARGUMENT, "out_delta is NULL");
    *out_delta = nullptr;
    // (what can be judged without the index first)
    AH_REQUIRE(n == 0 || sorted_ids, AH_ERR_INVALID_ARGUMENT, "sorted_ids is NULL");
    AH_REQUIRE(n < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "more ids than the u32 item-id space holds");
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(sorted_ids[i - 1] < sorted_ids[i], AH_ERR_INVALID_ARGUMENT, "sorted_ids is not strictly ascending at position %zu (%u after %u)",
                   i, sorted_ids[i], sorted_ids[i - 1]);
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        AH_REQUIRE(ix->fstats.filters_alive == 0, AH_ERR_INVALID_ARGUMENT, "the index has %llu live filters: ah_filter_destroy them first",
                   (unsigned long long)ix->fstats.filters_alive);
    }
    DeviceRestore restore_device;
    std::unique_ptr<ah_index_delta> delta(new ah_index_delta);
    AH_TRY(delete_impl(ix, sorted_ids, n, split_after, delta.get()));
    *out_delta = delta.release();
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_delta_get(const ah_index_delta *d, ah_index_delta_view *out) {
    AH_GUARDED("ah_index_delta_get")
    AH_REQUIRE(d && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    out->n_removed = d->removed.size();
    out->removed = d->removed.data();
    out->n_put = d->put.size();
    out->put_index = d->put_index.data();
    out->put = d->put.data();
    out->desc = d->desc.data();
    out->desc_len = d->desc.size();
    out->n_trees = (uint32_t)d->roots.size();
    out->roots = d->roots.data();
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_delta_destroy(ah_index_delta *d) {
    AH_GUARDED("ah_index_delta_destroy")
    NoFailScope no_fail;
    delete d;
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_suspend(ah_index *ix) {
    AH_GUARDED("ah_index_suspend")
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        AH_REQUIRE(ix->fstats.filters_alive == 0, AH_ERR_INVALID_ARGUMENT, "the index has %llu live filters: ah_filter_destroy them first",
                   (unsigned long long)ix->fstats.filters_alive);
    }
    {
        // no queued search of this index reads the rows any more
        DeviceRestore restore_device;
        AH_HIP(hipSetDevice(ix->ds->device));
        AH_HIP(hipDeviceSynchronize());
    }
    ix->suspended = true;
    if (ix->counted) ix->ds->live_indexes.fetch_sub(1, std::memory_order_acq_rel);
    ix->counted = false;
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_resume(ah_index *ix, ah_dataset *ds) {
    AH_GUARDED("ah_index_resume")
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    AH_REQUIRE(ix->suspended, AH_ERR_INVALID_ARGUMENT, "the index is not suspended");
    AH_REQUIRE(ds->metric == ix->nv.metric, AH_ERR_INVALID_ARGUMENT, "the dataset has another metric (%d) than the index (%d)", ds->metric,
               ix->nv.metric);
    AH_REQUIRE(ds->dims == ix->nv.dims, AH_ERR_INVALID_ARGUMENT, "the dataset has %u dimensions, the index %u", ds->dims, ix->nv.dims);
    AH_REQUIRE(ds->device == ix->ds->device, AH_ERR_INVALID_ARGUMENT, "the dataset lives on device %d, the index on device %d", ds->device,
               ix->ds->device);
    AH_REQUIRE(ds->finalized, AH_ERR_NOT_FINALIZED, "dataset not finalized");
    AH_REQUIRE(ds == ix->ds, AH_ERR_INVALID_ARGUMENT, "the dataset is not the one the index was created on");
    ds->live_indexes.fetch_add(1, std::memory_order_acq_rel);
    ix->counted = true;
    ix->suspended = false;
    DeviceRestore restore_device;
    AH_HIP(hipSetDevice(ds->device));
    index_prepare_screens(ds);  // (the update dropped the copies of the rows the screens read: as ah_index_create* does)
    return AH_OK;
    AH_GUARDED_END
}

}  // extern "C"
