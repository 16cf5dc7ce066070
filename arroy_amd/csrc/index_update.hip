// index_update.hip — ah_index_delete_items / ah_index_drop_trees / ah_index_insert_items / ah_index_graft / ah_index_compact /
// ah_index_footprint_get / ah_index_export / ah_index_suspend / ah_index_resume (include/arroy_hip.h): the kernels of the five
// updates, each call's host function (delete_impl, drop_impl, insert_impl, graft_impl, compact_count / footprint_impl /
// compact_impl) and the entry points.  What the
// host functions share is not here: the call scope, the span loop, the read-back, the commit and the node conversions are in
// index_device.h, the workspace layouts in index_workspace.h, grid_of and the allocation helper in common.h.  The dropped trees,
// the inserts, the grafts and the compaction are described above their kernels; the delete is the part of an
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
#include <memory>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "index_device.h"
#include "index_workspace.h"
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

// ---- dropped trees ------------------------------------------------------------------------------------------------------------
// ah_index_drop_trees: `delete_extra_trees` (src/writer.rs:631-655), the tree step of an incremental `Writer::build` that runs
// before the delete: n_drop times `root = roots.swap_remove(0); delete_tree(root)` ("Dropped trees on a resident
// index").  Which roots go and the order of those that stay is a host computation on the n_trees words read back from d_roots;
// every pass reads the index and writes new memory only:
//   1. levels    the nodes of the dropped trees in breadth-first order from the dropped roots only, one launch per level, as the
//                delete walks the whole forest: `dropped[node]`;
//   2. lengths   per node: the ids it holds if it is an in-use Descendants node that stays, whether it is dropped, whether it is
//                in use afterwards; three exclusive scans (scan_device.h) turn them into the offsets of the new blob, the
//                positions of the dropped nodes in the delta's `removed` and every node's rank among the nodes in use;
//   3. copy      a wave per Descendants node that stays copies its ids to the new offset, 64 ids a step: the lists end up in
//                ascending node order with their exact lengths, the invariant ah_index_compact relies on;
//   4. apply     the new node array (a dropped node becomes a free slot, a list that stays gets its new offset, everything else
//                is copied bit for bit) and the `removed` list; read back; the index's pointers are swapped last.
// The normal rows are not touched: those of the dropped split nodes are orphaned until ah_index_compact.
enum DCtl { DCTL_TAIL = 0, DCTL_ERR, DCTL_LEAVES, DCTL_MAX_DESC, DCTL_DESC_LEN, DCTL_REMOVED, DCTL_WORDS };

struct DropArgs {
    const DNode *nodes;
    uint32_t n_nodes;
    const uint32_t *desc;
    uint64_t old_desc_len;
    // per node, zeroed before the first kernel
    uint32_t *order;    // the nodes of the dropped trees, level by level
    uint32_t *dropped;  // 1 for a node of a dropped tree
    uint32_t *len;      // ids a Descendants node that stays holds -> (scan) where they start in the new blob
    uint32_t *rpos;     // `dropped` again -> (scan) the node's position in `removed`
    uint32_t *ctl;
    // what the scans gave (set before the passes that store through them)
    uint32_t new_desc_len, n_removed;
};

// the roots of the dropped trees (the host has checked that each is a node of the index)
__global__ __launch_bounds__(kIxBlock) void k_drop_seed(DropArgs a, const uint32_t *__restrict__ roots, uint32_t n_drop) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_drop; t += stride) {
        a.order[t] = roots[t];
        if (atomicExch(&a.dropped[roots[t]], 1u)) atomicOr(&a.ctl[DCTL_ERR], 1u);  // (a root listed twice)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[DCTL_TAIL] = n_drop;
}

// levels: the children of order[begin, end) are appended behind the tail
__global__ __launch_bounds__(kIxBlock) void k_drop_level(DropArgs a, uint32_t begin, uint32_t end) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        const DNode nd = a.nodes[a.order[i]];
        if ((nd.kind & 0xFFu) != AH_NODE_SPLIT) continue;
        const uint64_t pos = atomicAdd(&a.ctl[DCTL_TAIL], 2u);
        if (pos + 2 > a.n_nodes || nd.a >= a.n_nodes || nd.b >= a.n_nodes) {  // (not a forest: create_from_view has refused it)
            atomicOr(&a.ctl[DCTL_ERR], 1u);
            continue;
        }
        a.order[pos] = nd.a;
        a.order[pos + 1] = nd.b;
        if (atomicExch(&a.dropped[nd.a], 1u) | atomicExch(&a.dropped[nd.b], 1u)) atomicOr(&a.ctl[DCTL_ERR], 1u);  // (reachable twice)
    }
}

// lengths: what the three scans start from
__global__ __launch_bounds__(kIxBlock) void k_drop_lengths(DropArgs a, uint32_t *__restrict__ in_use) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = blockIdx.x * blockDim.x + threadIdx.x; node < a.n_nodes; node += stride) {
        const DNode nd = a.nodes[node];
        const uint32_t d = a.dropped[node];
        const bool stays = nd.kind != 0 && !d;
        if (d && nd.kind == 0) atomicOr(&a.ctl[DCTL_ERR], 2u);  // (a dropped tree led into a free slot)
        a.len[node] = stays && (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS ? nd.b : 0u;
        a.rpos[node] = d;
        in_use[node] = stays ? 1u : 0u;
    }
}

// copy: the Descendants nodes that stay among [lo, hi), a wave each (len: scanned): 64 ids a step, four steps in flight
__global__ __launch_bounds__(kIxBlock) void k_drop_copy(DropArgs a, uint32_t lo, uint32_t hi, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t node = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); node < hi; node += n_waves) {
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS || a.dropped[node]) continue;  // (wave-uniform, as is every branch below)
        if ((uint64_t)nd.a + nd.b > a.old_desc_len) {
            if (lane == 0) atomicOr(&a.ctl[DCTL_ERR], 4u);
            continue;
        }
        const uint32_t *src = a.desc + nd.a;
        const uint64_t base = a.len[node];
        for (uint64_t j0 = lane; j0 < nd.b; j0 += 4 * 64) {
            uint32_t id[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (j0 + k * 64 < nd.b) id[k] = src[j0 + k * 64];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                if (j0 + k * 64 >= nd.b) continue;
                const uint64_t at = base + j0 + k * 64;
                if (at < a.new_desc_len) out[at] = id[k];
                else atomicOr(&a.ctl[DCTL_ERR], 8u);
            }
        }
    }
}

// apply: every node as it is afterwards, the dropped ones into `removed` (len / rpos: scanned)
__global__ __launch_bounds__(kIxBlock) void k_drop_apply(DropArgs a, DNode *__restrict__ out, uint32_t *__restrict__ removed) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t rounds = (a.n_nodes + stride - 1) / stride;
    uint32_t leaves = 0, largest = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t node = (uint64_t)r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        if (node >= a.n_nodes) break;
        DNode nd = a.nodes[node];
        if (a.dropped[node]) {
            nd = DNode{0, 0, 0, 0};
            if (a.rpos[node] < a.n_removed) removed[a.rpos[node]] = (uint32_t)node;
            else atomicOr(&a.ctl[DCTL_ERR], 16u);
        } else if ((nd.kind & 0xFFu) == AH_NODE_DESCENDANTS) {
            nd.a = a.len[node];
            leaves++;
            largest = max(largest, nd.b);
        }
        out[node] = nd;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) {
        leaves += __shfl_xor(leaves, d, 64);
        largest = max(largest, (uint32_t)__shfl_xor(largest, d, 64));
    }
    if (lane == 0 && leaves) {
        atomicAdd(&a.ctl[DCTL_LEAVES], leaves);
        atomicMax(&a.ctl[DCTL_MAX_DESC], largest);
    }
}

// ---- inserts ------------------------------------------------------------------------------------------------------------------
// ah_index_insert_items: `insert_items_in_descendants_from_frozen_reader` (src/writer.rs:1398-1459) for every tree at once, the
// lists included ("Inserts and grafts on a resident index"); every pass reads the index and writes new memory only:
//   1. check     every id is a row of the dataset (the first that is not is named);
//   2. route     k_route_items (search.hip), AH_LAUNCH_MAX_ITEMS pairs a launch: the landing node of every (tree, id) pair;
//   3. count     pairs per landing node (atomics), scanned into the segments of `landed`; the touched nodes, ascending;
//   4. scatter   every id into its node's segment; a block sorts each segment (LDS up to 4096 ids);
//   5. fresh     a wave per touched node drops from its segment the ids its list already holds (binary search, ballot +
//                popcount, 64 ids a step); the new lengths, scanned into the offsets of the new blob and of the delta;
//   6. write     a wave per Descendants node: an untouched list is copied, a touched one merged with its segment, every id
//                going to (its position in its own list) + (ids below it in the other);
//   7. apply     the new node array and the delta; read back; the index's pointers are swapped last.
enum ICtl { ICTL_ERR = 0, ICTL_FIRST_BAD, ICTL_TOUCHED, ICTL_DESC_LEN, ICTL_DELTA_DESC, ICTL_LEAVES, ICTL_MAX_DESC, ICTL_WORDS };

struct InsertArgs {
    const DNode *nodes;
    uint32_t n_nodes;
    const uint32_t *desc;
    uint64_t old_desc_len;
    // per node, zeroed before the first kernel
    uint32_t *cnt;      // pairs that landed in the node
    uint32_t *seg;      // (cnt, scanned) where the node's pairs start in `landed`
    uint32_t *cursor;   // pairs already placed there
    uint32_t *chg;      // 1 for a touched node -> (scan) its position in the delta
    uint32_t *fresh;    // ids of the node's segment that its list does not hold yet
    uint32_t *nlen;     // ids the node holds afterwards -> (scan) where they start in the new blob
    uint32_t *dlen;     // the same of the touched nodes only -> (scan) where they start in the delta's ids
    uint32_t *touched;  // the touched nodes, ascending
    uint32_t *landed;   // n_pairs ids, by landing node
    uint32_t *ctl;
    uint64_t n_pairs;
    // what the scans gave (set before the passes that store through them)
    uint32_t n_touched, new_desc_len, delta_desc_len;
};

// positions of v[0, m) (ascending) that hold a value below x
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *v, uint32_t m, uint32_t x) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kIxBlock) void k_insert_check(DataView dv, const uint32_t *__restrict__ ids, uint64_t n, uint32_t *ctl) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (row_of_id(dv, ids[i]) == ~0ull) atomicMin(&ctl[ICTL_FIRST_BAD], (uint32_t)i);
}

// count: the m pairs of one routing launch
__global__ __launch_bounds__(kIxBlock) void k_insert_count(InsertArgs a, const uint32_t *__restrict__ leaf, uint64_t m) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += stride) {
        const uint32_t node = leaf[p];
        if (node >= a.n_nodes || (a.nodes[node].kind & 0xFFu) != AH_NODE_DESCENDANTS) atomicOr(&a.ctl[ICTL_ERR], 1u);
        else atomicAdd(&a.cnt[node], 1u);
    }
}

// per node: touched or not, and the length an untouched list keeps
__global__ __launch_bounds__(kIxBlock) void k_insert_flags(InsertArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = blockIdx.x * blockDim.x + threadIdx.x; node < a.n_nodes; node += stride) {
        const DNode nd = a.nodes[node];
        a.chg[node] = a.cnt[node] ? 1u : 0u;
        a.nlen[node] = (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS ? nd.b : 0u;
    }
}

// the touched nodes in node order (chg: scanned)
__global__ __launch_bounds__(kIxBlock) void k_insert_touched(InsertArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = blockIdx.x * blockDim.x + threadIdx.x; node < a.n_nodes; node += stride)
        if (a.cnt[node]) a.touched[a.chg[node]] = (uint32_t)node;  // (chg[node] < touched nodes <= n_nodes)
}

// scatter: the m pairs of one routing launch (ids: the cn ids of that launch) into the segments (seg: scanned)
__global__ __launch_bounds__(kIxBlock) void k_insert_scatter(InsertArgs a, const uint32_t *__restrict__ ids, uint64_t cn,
                                                             const uint32_t *__restrict__ leaf, uint64_t m) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += stride) {
        const uint32_t node = leaf[p];
        if (node >= a.n_nodes) continue;  // (the count pass has flagged it)
        const uint64_t at = (uint64_t)a.seg[node] + atomicAdd(&a.cursor[node], 1u);
        if (at < a.n_pairs) a.landed[at] = ids[p % cn];
        else atomicOr(&a.ctl[ICTL_ERR], 2u);
    }
}

// the segments ascending, a block each
__global__ __launch_bounds__(kIxBlock) void k_insert_sort(InsertArgs a) {
    __shared__ uint32_t lds[kSortLds];
    for (uint32_t i = blockIdx.x; i < a.n_touched; i += gridDim.x) {
        const uint32_t node = a.touched[i];
        if (node >= a.n_nodes || (uint64_t)a.seg[node] + a.cnt[node] > a.n_pairs) continue;  // (block-uniform; flagged by the next pass)
        block_sort_segment(a.landed + a.seg[node], a.cnt[node], lds);
    }
}

// fresh: touched[lo, hi), a wave each: `descendants | to_insert` adds only what the list does not hold; the segment is
// compacted in place (a step stores at or below the positions it has read)
__global__ __launch_bounds__(kIxBlock) void k_insert_fresh(InsertArgs a, uint32_t lo, uint32_t hi) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < hi; i += n_waves) {
        const uint32_t node = a.touched[i];
        if (node >= a.n_nodes) {  // (wave-uniform, as is every branch below)
            if (lane == 0) atomicOr(&a.ctl[ICTL_ERR], 4u);
            continue;
        }
        const DNode nd = a.nodes[node];
        const uint32_t m = a.cnt[node];
        if ((uint64_t)a.seg[node] + m > a.n_pairs || (uint64_t)nd.a + nd.b > a.old_desc_len) {
            if (lane == 0) atomicOr(&a.ctl[ICTL_ERR], 4u);
            continue;
        }
        uint32_t *seg = a.landed + a.seg[node];
        const uint32_t *list = a.desc + nd.a;
        uint32_t kept = 0;
        for (uint32_t j0 = 0; j0 < m; j0 += 64) {
            bool keep = false;
            uint32_t id = 0;
            if (j0 + lane < m) {
                id = seg[j0 + lane];
                const uint32_t at = lower_bound_u32(list, nd.b, id);
                keep = !(at < nd.b && list[at] == id);
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) seg[kept + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = id;
            kept += (uint32_t)__popcll(mask);
        }
        if (lane == 0) {
            a.fresh[node] = kept;
            a.nlen[node] = nd.b + kept;
            a.dlen[node] = nd.b + kept;
        }
    }
}

// write: the Descendants nodes among [lo, hi), a wave each (nlen: scanned)
__global__ __launch_bounds__(kIxBlock) void k_insert_write(InsertArgs a, uint32_t lo, uint32_t hi, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t node = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); node < hi; node += n_waves) {
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;  // (wave-uniform, as is every branch below)
        const uint32_t f = a.cnt[node] ? a.fresh[node] : 0u;
        const uint64_t base = a.nlen[node];
        if (base + nd.b + f > a.new_desc_len || (uint64_t)nd.a + nd.b > a.old_desc_len || (uint64_t)a.seg[node] + f > a.n_pairs) {
            if (lane == 0) atomicOr(&a.ctl[ICTL_ERR], 8u);
            continue;
        }
        const uint32_t *list = a.desc + nd.a;
        const uint32_t *seg = a.landed + a.seg[node];
        for (uint32_t j = lane; j < nd.b; j += 64) {
            const uint32_t id = list[j];
            out[base + j + (f ? lower_bound_u32(seg, f, id) : 0u)] = id;
        }
        for (uint32_t j = lane; j < f; j += 64) {
            const uint32_t id = seg[j];
            out[base + j + lower_bound_u32(list, nd.b, id)] = id;
        }
    }
}

// apply: every node as it is afterwards, the touched ones into the delta as well (chg / dlen / nlen: scanned)
__global__ __launch_bounds__(kIxBlock) void k_insert_apply(InsertArgs a, DNode *__restrict__ out, DeltaEntry *__restrict__ entries) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t rounds = (a.n_nodes + stride - 1) / stride;
    uint32_t leaves = 0, largest = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t node = (uint64_t)r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        if (node >= a.n_nodes) break;
        DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) == AH_NODE_DESCENDANTS) {
            nd.a = a.nlen[node];
            if (a.cnt[node]) {
                nd.b += a.fresh[node];
                if (a.chg[node] < a.n_touched) entries[a.chg[node]] = DeltaEntry{(uint32_t)node, AH_NODE_DESCENDANTS, a.dlen[node], nd.b};
                else atomicOr(&a.ctl[ICTL_ERR], 16u);
            }
            leaves++;
            largest = max(largest, nd.b);
        }
        out[node] = nd;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) {
        leaves += __shfl_xor(leaves, d, 64);
        largest = max(largest, (uint32_t)__shfl_xor(largest, d, 64));
    }
    if (lane == 0 && leaves) {
        atomicAdd(&a.ctl[ICTL_LEAVES], leaves);
        atomicMax(&a.ctl[ICTL_MAX_DESC], largest);
    }
}

// the new lists of the touched nodes, node after node, for the host; a wave per touched node
__global__ __launch_bounds__(kIxBlock) void k_insert_gather(InsertArgs a, const DeltaEntry *__restrict__ entries,
                                                            const uint32_t *__restrict__ blob, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < a.n_touched; i += n_waves) {
        const DeltaEntry e = entries[i];
        if (e.node >= a.n_nodes || (uint64_t)e.a + e.b > a.delta_desc_len || (uint64_t)a.nlen[e.node] + e.b > a.new_desc_len) {
            if (lane == 0) atomicOr(&a.ctl[ICTL_ERR], 32u);
            continue;
        }
        const uint32_t *src = blob + a.nlen[e.node];
        for (uint32_t j = lane; j < e.b; j += 64) out[e.a + j] = src[j];
    }
}

// ---- grafts -------------------------------------------------------------------------------------------------------------------
// ah_index_graft: the trees of a view become part of the index, each root in place of a Descendants node or as a new root, and
// every node gets the index it has in a fresh view of the host's store:
//   1. named     one flag per final position a new node names; its scan gives every unnamed position p the old node of rank
//                p - named_before(p), hence every old node its new index;
//   2. lengths   per final position the ids it holds, scanned into the offsets of the new blob;
//   3. nodes     the new node array, children remapped; the new roots;
//   4. lists     a wave per Descendants node copies its ids, from the old blob or from the view's;
//   5. normals   the view's records are unpacked (k_unpack_normals, search.hip) into the rows behind the index's own.
enum GCtl { GCTL_ERR = 0, GCTL_NAMED, GCTL_DESC_LEN, GCTL_LEAVES, GCTL_MAX_DESC, GCTL_WORDS };

struct GraftArgs {
    const DNode *nodes;    // the index as it is
    uint32_t n_old, n_used;
    const uint32_t *rank;  // nullptr: no holes
    const uint32_t *desc;
    uint64_t old_desc_len;
    const DNode *vnodes;   // the view's nodes: children and offsets in the view's own numbering, c = the normal's ordinal
    uint32_t n_view;
    const uint32_t *vfin;  // the final index a new node names, kNone for a replacing root
    const uint32_t *vtgt;  // the node a replacing root replaces, else kNone
    const uint32_t *vdesc;
    uint64_t vdesc_len;
    uint32_t n_new;        // nodes afterwards
    uint32_t first_row;    // the normal row of the view's first normal
    uint32_t *named;       // n_new + 1: flags -> (scan) named positions below
    uint32_t *pos_of_rank; // n_used
    uint32_t *new_of_old;  // n_old; kNone for a free slot
    uint32_t *replaced;    // n_old: 1 for a target
    uint32_t *fin;         // n_view: the final index of every view node
    uint32_t *len;         // n_new + 1: ids per final position -> (scan) offsets
    uint32_t *ctl;
    uint32_t new_desc_len;
};

__global__ __launch_bounds__(kIxBlock) void k_graft_named(GraftArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t k = blockIdx.x * blockDim.x + threadIdx.x; k < a.n_view; k += stride) {
        const uint32_t p = a.vfin[k], t = a.vtgt[k];
        if (t != kNone) {
            if (t < a.n_old) a.replaced[t] = 1u;
            else atomicOr(&a.ctl[GCTL_ERR], 1u);
        } else if (p < a.n_new) {
            a.named[p] = 1u;
        } else {
            atomicOr(&a.ctl[GCTL_ERR], 1u);
        }
    }
}

// (named: scanned, the total behind it) the p-th unnamed position belongs to the old node of rank p - named_before(p)
__global__ __launch_bounds__(kIxBlock) void k_graft_positions(GraftArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t p = blockIdx.x * blockDim.x + threadIdx.x; p < a.n_new; p += stride) {
        if (a.named[p + 1] != a.named[p]) continue;
        const uint64_t r = p - a.named[p];
        if (r < a.n_used) a.pos_of_rank[r] = (uint32_t)p;
        else atomicOr(&a.ctl[GCTL_ERR], 2u);
    }
}

__global__ __launch_bounds__(kIxBlock) void k_graft_old_map(GraftArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t o = blockIdx.x * blockDim.x + threadIdx.x; o < a.n_old; o += stride) {
        uint32_t p = kNone;
        if (a.nodes[o].kind != 0) {
            const uint32_t r = a.rank ? a.rank[o] : (uint32_t)o;
            if (r < a.n_used) p = a.pos_of_rank[r];
            else atomicOr(&a.ctl[GCTL_ERR], 4u);
        }
        a.new_of_old[o] = p;
    }
}

__global__ __launch_bounds__(kIxBlock) void k_graft_fin(GraftArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t k = blockIdx.x * blockDim.x + threadIdx.x; k < a.n_view; k += stride) {
        const uint32_t t = a.vtgt[k];
        a.fin[k] = t == kNone ? a.vfin[k] : (t < a.n_old ? a.new_of_old[t] : kNone);
    }
}

// The final position and the node of work item w: the old nodes first, then the view's.  false: nothing moves (a free slot, a
// replaced node)
__device__ __forceinline__ bool graft_item(const GraftArgs &a, uint64_t w, uint32_t *p, DNode *nd, bool *from_view) {
    *from_view = w >= a.n_old;
    if (!*from_view) {
        *nd = a.nodes[w];
        if (nd->kind == 0 || a.replaced[w]) return false;
        *p = a.new_of_old[w];
    } else {
        *nd = a.vnodes[w - a.n_old];
        *p = a.fin[w - a.n_old];
    }
    if (*p >= a.n_new) {
        atomicOr(&a.ctl[GCTL_ERR], 8u);
        return false;
    }
    return true;
}

__global__ __launch_bounds__(kIxBlock) void k_graft_len(GraftArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint64_t work = (uint64_t)a.n_old + a.n_view;
    for (uint64_t w = blockIdx.x * blockDim.x + threadIdx.x; w < work; w += stride) {
        uint32_t p;
        DNode nd;
        bool from_view;
        if (!graft_item(a, w, &p, &nd, &from_view)) continue;
        a.len[p] = (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS ? nd.b : 0u;
    }
}

// nodes (len: scanned); every position of the new array is written by exactly one work item
__global__ __launch_bounds__(kIxBlock) void k_graft_nodes(GraftArgs a, DNode *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint64_t work = (uint64_t)a.n_old + a.n_view;
    const uint32_t rounds = (uint32_t)((work + stride - 1) / stride);
    uint32_t leaves = 0, largest = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t w = (uint64_t)r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        if (w >= work) break;
        uint32_t p;
        DNode nd;
        bool from_view;
        if (!graft_item(a, w, &p, &nd, &from_view)) continue;
        if ((nd.kind & 0xFFu) == AH_NODE_DESCENDANTS) {
            nd = DNode{AH_NODE_DESCENDANTS, a.len[p], nd.b, 0};
            leaves++;
            largest = max(largest, nd.b);
        } else {
            const uint32_t limit = from_view ? a.n_view : a.n_old;
            if (nd.a >= limit || nd.b >= limit) {
                atomicOr(&a.ctl[GCTL_ERR], 16u);
                continue;
            }
            nd.a = from_view ? a.fin[nd.a] : a.new_of_old[nd.a];
            nd.b = from_view ? a.fin[nd.b] : a.new_of_old[nd.b];
            if (from_view) nd.c = (nd.kind & 0x100u) ? a.first_row + nd.c : 0u;
            if (nd.a >= a.n_new || nd.b >= a.n_new) atomicOr(&a.ctl[GCTL_ERR], 16u);
        }
        out[p] = nd;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) {
        leaves += __shfl_xor(leaves, d, 64);
        largest = max(largest, (uint32_t)__shfl_xor(largest, d, 64));
    }
    if (lane == 0 && leaves) {
        atomicAdd(&a.ctl[GCTL_LEAVES], leaves);
        atomicMax(&a.ctl[GCTL_MAX_DESC], largest);
    }
}

// lists: work items [lo, hi), a wave each
__global__ __launch_bounds__(kIxBlock) void k_graft_lists(GraftArgs a, uint64_t lo, uint64_t hi, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint64_t w = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); w < hi; w += n_waves) {
        uint32_t p;
        DNode nd;
        bool from_view;
        if (!graft_item(a, w, &p, &nd, &from_view)) continue;  // (wave-uniform, as is every branch below)
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;
        const uint64_t base = a.len[p];
        if (base + nd.b > a.new_desc_len || (uint64_t)nd.a + nd.b > (from_view ? a.vdesc_len : a.old_desc_len)) {
            if (lane == 0) atomicOr(&a.ctl[GCTL_ERR], 32u);
            continue;
        }
        const uint32_t *src = (from_view ? a.vdesc : a.desc) + nd.a;
        for (uint32_t j = lane; j < nd.b; j += 64) out[base + j] = src[j];
    }
}

// the roots: the index's own in their order, then the view's new roots in view order
__global__ __launch_bounds__(kIxBlock) void k_graft_roots(GraftArgs a, const uint32_t *__restrict__ roots, uint32_t n_trees,
                                                          const uint32_t *__restrict__ new_roots, uint32_t n_added,
                                                          uint32_t *__restrict__ out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t t = blockIdx.x * blockDim.x + threadIdx.x; t < (uint64_t)n_trees + n_added; t += stride) {
        uint32_t p = kNone;
        if (t < n_trees) {
            if (roots[t] < a.n_old) p = a.new_of_old[roots[t]];
        } else if (new_roots[t - n_trees] < a.n_view) {
            p = a.fin[new_roots[t - n_trees]];
        }
        if (p >= a.n_new) atomicOr(&a.ctl[GCTL_ERR], 64u);
        out[t] = p;
    }
}

// what the host must know of the targets before anything is touched
__global__ __launch_bounds__(kIxBlock) void k_graft_peek(const DNode *__restrict__ nodes, const uint32_t *__restrict__ which, uint32_t n,
                                                         uint32_t *__restrict__ kinds) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) kinds[i] = nodes[which[i]].kind;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------
// ah_index_compact: the free node slots, the normal rows no node names any more and the spare rows go, and the index becomes what
// ah_index_create_from_view makes of the forest as it is ("Compaction of a resident index"); every pass reads the
// index and writes new memory only:
//   1. flags     per node slot: in use, and in-use split node with a normal; two exclusive scans give every node its new index
//                (the rank d_rank holds) and every such node its new row; how many rows are not where a fresh index has them.
//                ah_index_footprint_get stops here;
//   2. nodes     a thread per in-use node writes it at its new index, children and row remapped; the roots; the old row of
//                every new row;
//   3. rows      a wave per new row copies row and header from the old arrays.
enum CCtl { CCTL_ERR = 0, CCTL_USED, CCTL_LIVE, CCTL_MISPLACED, CCTL_WORDS };

struct CompactArgs {
    const DNode *nodes;
    uint32_t n_nodes;
    uint32_t old_rows;     // n_normals before the call
    uint32_t *new_index;   // n_nodes + 1: in-use flags -> (scan) in-use nodes below
    uint32_t *new_row;     // n_nodes + 1: flags of the in-use split nodes with a normal -> (scan) such nodes below
    uint32_t *ctl;
    uint32_t n_used, n_live;  // what the scans gave (set before the passes that store through them)
};

typedef uint32_t u32x4_c __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool owns_row(uint32_t kind) { return (kind & 0xFFu) == AH_NODE_SPLIT && (kind & 0x100u); }

__global__ __launch_bounds__(kIxBlock) void k_compact_flags(CompactArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = blockIdx.x * blockDim.x + threadIdx.x; node < a.n_nodes; node += stride) {
        const uint32_t kind = a.nodes[node].kind;
        a.new_index[node] = kind != 0 ? 1u : 0u;
        a.new_row[node] = owns_row(kind) ? 1u : 0u;
    }
}

// (new_row: scanned) the nodes whose row is not the row a fresh index gives them
__global__ __launch_bounds__(kIxBlock) void k_compact_placed(CompactArgs a) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = blockIdx.x * blockDim.x + threadIdx.x; node < a.n_nodes; node += stride) {
        const DNode nd = a.nodes[node];
        if (owns_row(nd.kind) && nd.c != a.new_row[node]) atomicOr(&a.ctl[CCTL_MISPLACED], 1u);
    }
}

// nodes: the slots [lo, hi); every position of the new array is written by exactly one in-use node
__global__ __launch_bounds__(kIxBlock) void k_compact_nodes(CompactArgs a, uint32_t lo, uint32_t hi, DNode *__restrict__ out,
                                                            uint32_t *__restrict__ src_of_row, uint32_t *__restrict__ map) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t node = (uint64_t)lo + blockIdx.x * blockDim.x + threadIdx.x; node < hi; node += stride) {
        DNode nd = a.nodes[node];
        if (nd.kind == 0) {
            if (map) map[node] = kNone;
            continue;
        }
        const uint32_t p = a.new_index[node];
        if (map) map[node] = p;
        if (p >= a.n_used) {
            atomicOr(&a.ctl[CCTL_ERR], 1u);
            continue;
        }
        if ((nd.kind & 0xFFu) == AH_NODE_SPLIT) {
            if (nd.a >= a.n_nodes || nd.b >= a.n_nodes || a.nodes[nd.a].kind == 0 || a.nodes[nd.b].kind == 0) {  // (a child in a free slot)
                atomicOr(&a.ctl[CCTL_ERR], 2u);
                continue;
            }
            nd.a = a.new_index[nd.a];
            nd.b = a.new_index[nd.b];
            if (nd.kind & 0x100u) {
                const uint32_t r = a.new_row[node];
                if (r >= a.n_live || nd.c >= a.old_rows) {
                    atomicOr(&a.ctl[CCTL_ERR], 4u);
                    continue;
                }
                src_of_row[r] = nd.c;
                nd.c = r;
            } else {
                nd.c = 0;
            }
        } else {
            nd.c = 0;
        }
        out[p] = nd;
    }
}

__global__ __launch_bounds__(kIxBlock) void k_compact_roots(CompactArgs a, const uint32_t *__restrict__ roots, uint32_t n_trees,
                                                            uint32_t *__restrict__ out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_trees; t += stride) {
        const uint32_t r = roots[t];
        uint32_t p = kNone;
        if (r < a.n_nodes && a.nodes[r].kind != 0) p = a.new_index[r];
        if (p >= a.n_used) atomicOr(&a.ctl[CCTL_ERR], 8u);
        out[t] = p;
    }
}

// rows: the new rows [lo, hi), a wave each: 16 bytes a lane a step, four steps in flight, the last one partial (rb is a multiple
// of 16: f32 rows are whole 128-byte lines, 1-bit rows an even number of 64-bit words); the header floats ride along
__global__ __launch_bounds__(kIxBlock) void k_compact_rows(const uint8_t *__restrict__ old_rows, const float *__restrict__ old_hdr,
                                                           const uint32_t *__restrict__ src_of_row, uint32_t n_old_rows, uint64_t lo,
                                                           uint64_t hi, uint64_t rb, uint32_t hf, uint8_t *__restrict__ rows,
                                                           float *__restrict__ hdr, uint32_t *ctl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kIxBlock / 64);
    for (uint64_t q = lo + (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6); q < hi; q += n_waves) {
        const uint32_t from = src_of_row[q];
        if (from >= n_old_rows) {  // (wave-uniform; the node pass has flagged it)
            if (lane == 0) atomicOr(&ctl[CCTL_ERR], 16u);
            continue;
        }
        const uint8_t *src = old_rows + (uint64_t)from * rb;
        uint8_t *dst = rows + q * rb;
        for (uint64_t c0 = (uint64_t)lane * 16; c0 < rb; c0 += 4 * 64 * 16) {
            u32x4_c v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint64_t c = c0 + (uint64_t)k * 64 * 16;
                if (c < rb) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_c *>(src + c));
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint64_t c = c0 + (uint64_t)k * 64 * 16;
                if (c < rb) __builtin_nontemporal_store(v[k], reinterpret_cast<u32x4_c *>(dst + c));
            }
        }
        if (lane < hf) hdr[q * hf + lane] = old_hdr[(uint64_t)from * hf + lane];
    }
}

int alloc(DevMem *m, size_t bytes) { return ah::alloc(m, bytes, "the index update"); }

int delete_impl(ah_index *ix, const uint32_t *ids, size_t n, uint32_t split_after, ah_index_delta *delta) {
    IndexCall call;
    AH_TRY(call.begin(ix->ds));
    const hipStream_t s = call.stream();
    const uint32_t nn = ix->n_nodes, n_trees = ix->n_trees;
    const uint64_t old_desc_len = ix->desc_len;
    // every buffer whose size is known now; kernels write only into these
    const uint64_t len_bits = n ? (uint64_t)ids[n - 1] + 1 : 0;
    const size_t bit_words = (size_t)((len_bits + 31) / 32);
    DeleteArgs a{};
    a.nodes = ix->d_nodes;
    a.n_nodes = nn;
    a.desc = ix->d_desc;
    a.len_bits = len_bits;
    a.split_after = split_after;
    uint32_t *tile_sums = nullptr;
    const Workspace ws = delete_workspace(a, &tile_sums, nn, kScanTile, CTL_WORDS);
    DevMem bitmap, work, new_nodes, new_roots, new_rank, new_desc, out;
    AH_TRY(alloc(&bitmap, (bit_words + n) * 4));
    AH_TRY(alloc(&work, ws.bytes()));
    ws.carve(work.p, ws.bytes());
    AH_TRY(alloc(&new_nodes, (size_t)nn * sizeof(DNode)));
    AH_TRY(alloc(&new_roots, (size_t)n_trees * 4));
    AH_TRY(alloc(&new_rank, ((size_t)nn + 1) * 4));
    delta->roots.resize(n_trees);
    a.bits = n ? bitmap.as<const uint32_t>() : nullptr;
    AH_HIP(hipMemsetAsync(work.p, 0, ws.zeroed_bytes(), s));
    // 1. bitmap
    if (n) {
        uint32_t *d_ids = bitmap.as<uint32_t>() + bit_words;
        AH_HIP(hipMemsetAsync(bitmap.p, 0, bit_words * 4, s));
        AH_HIP(hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_filter_bitmap, dim3(grid_of(n, kIxBlock, 1024)), dim3(kIxBlock), 0, s, (const uint32_t *)d_ids, (uint64_t)n,
                           bitmap.as<uint32_t>());
    }
    AH_HIP(hipGetLastError());
    const auto t_bitmap = call.phase_end();
    // 2. levels
    uint32_t ctl[CTL_WORDS];
    std::vector<uint32_t> level_begin;
    uint32_t begin = 0, end = n_trees;
    if (n_trees) hipLaunchKernelGGL(k_delete_seed, dim3(grid_of(n_trees, kIxBlock, 1024)), dim3(kIxBlock), 0, s, a, (const uint32_t *)ix->d_roots, n_trees);
    while (begin < end) {
        level_begin.push_back(begin);
        hipLaunchKernelGGL(k_delete_level, dim3(grid_of(end - begin, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, begin, end);
        AH_TRY(read_back(ctl, a.ctl, 2, s));
        AH_REQUIRE(ctl[CTL_ERR] == 0 && ctl[CTL_TAIL] >= end && ctl[CTL_TAIL] <= nn, AH_ERR_DEVICE,
                   "the nodes of the index are not a forest (a node is reachable twice)");
        begin = end;
        end = ctl[CTL_TAIL];
    }
    level_begin.push_back(end);
    const uint32_t reached = end;
    const size_t levels = level_begin.size() - 1;
    const auto t_levels = call.now();
    // the passes over every reachable node, a wave each, in launches of at most AH_LAUNCH_MAX_ITEMS nodes
    // 3. count
    for_spans(reached, call.span(), [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_delete_count, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi);
    });
    AH_HIP(hipGetLastError());
    const auto t_count = call.phase_end();
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
    AH_TRY(read_back(ctl, a.ctl, CTL_WORDS, s));
    const auto t_resolve = call.now();
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
    for_spans(reached, call.span(), [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_delete_write, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi,
                           new_desc.as<uint32_t>());
    });
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
    const auto t_write = call.phase_end();
    // read back
    if (n_changed) AH_HIP(hipMemcpyAsync(entries.data(), d_entries, (size_t)n_changed * sizeof(DeltaEntry), hipMemcpyDeviceToHost, s));
    if (delta_desc) AH_HIP(hipMemcpyAsync(delta->desc.data(), d_delta_desc, (size_t)delta_desc * 4, hipMemcpyDeviceToHost, s));
    if (n_trees) AH_HIP(hipMemcpyAsync(delta->roots.data(), new_roots.p, (size_t)n_trees * 4, hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(ctl, a.ctl, CTL_WORDS, s));
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
        delta->put_index.push_back(e.node);
        delta->put.push_back(to_host_node(DNode{e.kind, e.a, e.b, 0}));
    }
    const auto t_read = call.now();
    IndexCommit c(ix, &new_nodes, &new_roots, &new_desc, &new_rank);
    c.desc_len = desc_len;
    c.n_leaves = ctl[CTL_LEAVES];
    c.max_desc = ctl[CTL_MAX_DESC];
    c.compacted = false;
    index_commit(ix, c);
    if (call.timing)
        fprintf(stderr, "[ah] index delete: %zu ids, %u of %u nodes reachable in %zu levels, %llu -> %u stored ids, %zu removed + %zu put nodes: "
                        "bitmap %.6f s, levels %.6f s, count %.6f s, resolve %.6f s, write %.6f s, read-back %.6f s\n",
                n, reached, nn, levels, (unsigned long long)old_desc_len, desc_len, delta->removed.size(), delta->put.size(),
                call.secs(call.t0, t_bitmap), call.secs(t_bitmap, t_levels), call.secs(t_levels, t_count), call.secs(t_count, t_resolve),
                call.secs(t_resolve, t_write), call.secs(t_write, t_read));
    return AH_OK;
}

// what the updates and ah_index_suspend ask of an index before they look at it
int index_updatable(ah_index *ix) {
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    AH_REQUIRE(ix->fstats.filters_alive == 0, AH_ERR_INVALID_ARGUMENT, "the index has %llu live filters: ah_filter_destroy them first",
               (unsigned long long)ix->fstats.filters_alive);
    return AH_OK;
}

int drop_impl(ah_index *ix, uint32_t n_drop, bool sort_roots, ah_index_delta *delta) {
    IndexCall call;
    AH_TRY(call.begin(ix->ds));
    const hipStream_t s = call.stream();
    const uint32_t nn = ix->n_nodes, n_trees = ix->n_trees;
    const uint64_t old_desc_len = ix->desc_len;
    n_drop = std::min(n_drop, n_trees);
    // the roots: `roots.swap_remove(0)` n_drop times on the host's copy
    std::vector<uint32_t> roots(n_trees), gone;
    if (n_trees) AH_TRY(read_back(roots.data(), ix->d_roots, n_trees, s));
    if (n_drop == 0) {  // nothing to do: the current roots, and the index keeps its arrays
        delta->roots = std::move(roots);
        return AH_OK;
    }
    AH_REQUIRE(n_trees <= nn, AH_ERR_DEVICE, "the index has more trees (%u) than nodes (%u)", n_trees, nn);
    gone.reserve(n_drop);
    for (uint32_t k = 0; k < n_drop; k++) {
        AH_REQUIRE(roots[0] < nn, AH_ERR_DEVICE, "root %u of the index is no node of it (%u nodes)", roots[0], nn);
        gone.push_back(roots[0]);
        roots[0] = roots.back();
        roots.pop_back();
    }
    if (sort_roots) std::sort(roots.begin(), roots.end());  // roots.sort_unstable() (src/writer.rs:1001)
    const uint32_t kept = n_trees - n_drop;
    // every buffer whose size is known now; kernels write only into these
    DropArgs a{};
    a.nodes = ix->d_nodes;
    a.n_nodes = nn;
    a.desc = ix->d_desc;
    a.old_desc_len = old_desc_len;
    uint32_t *tile_sums = nullptr, *d_gone = nullptr;
    const Workspace ws = drop_workspace(a, &tile_sums, &d_gone, nn, n_drop, kScanTile, DCTL_WORDS);
    DevMem work, new_nodes, new_roots, new_rank, new_desc, out;
    AH_TRY(alloc(&work, ws.bytes()));
    ws.carve(work.p, ws.bytes());
    AH_TRY(alloc(&new_nodes, (size_t)nn * sizeof(DNode)));
    AH_TRY(alloc(&new_roots, (size_t)kept * 4));
    AH_TRY(alloc(&new_rank, ((size_t)nn + 1) * 4));
    AH_HIP(hipMemsetAsync(work.p, 0, ws.zeroed_bytes(), s));
    AH_HIP(hipMemcpyAsync(d_gone, gone.data(), (size_t)n_drop * 4, hipMemcpyHostToDevice, s));
    if (kept) AH_HIP(hipMemcpyAsync(new_roots.p, roots.data(), (size_t)kept * 4, hipMemcpyHostToDevice, s));
    // 1. levels
    uint32_t ctl[DCTL_WORDS];
    uint32_t begin = 0, end = n_drop;
    size_t levels = 0;
    hipLaunchKernelGGL(k_drop_seed, dim3(grid_of(n_drop, kIxBlock, 1024)), dim3(kIxBlock), 0, s, a, (const uint32_t *)d_gone, n_drop);
    while (begin < end) {
        levels++;
        hipLaunchKernelGGL(k_drop_level, dim3(grid_of(end - begin, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, begin, end);
        AH_TRY(read_back(ctl, a.ctl, 2, s));
        AH_REQUIRE(ctl[DCTL_ERR] == 0 && ctl[DCTL_TAIL] >= end && ctl[DCTL_TAIL] <= nn, AH_ERR_DEVICE,
                   "the nodes of the index are not a forest (a node is reachable twice)");
        begin = end;
        end = ctl[DCTL_TAIL];
    }
    const uint32_t reached = end;
    const auto t_levels = call.now();
    // 2. lengths and the scans
    hipLaunchKernelGGL(k_drop_lengths, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, new_rank.as<uint32_t>());
    launch_exclusive_scan(a.len, nn, tile_sums, a.ctl + DCTL_DESC_LEN, s);
    launch_exclusive_scan(a.rpos, nn, tile_sums, a.ctl + DCTL_REMOVED, s);
    launch_exclusive_scan(new_rank.as<uint32_t>(), nn, tile_sums, new_rank.as<uint32_t>() + nn, s);
    AH_TRY(read_back(ctl, a.ctl, DCTL_WORDS, s));
    const auto t_lengths = call.now();
    const uint32_t desc_len = ctl[DCTL_DESC_LEN], n_removed = ctl[DCTL_REMOVED];
    AH_REQUIRE(ctl[DCTL_ERR] == 0 && desc_len <= old_desc_len && n_removed == reached, AH_ERR_DEVICE,
               "the index drop found the index inconsistent (%u): the index is unchanged", ctl[DCTL_ERR]);
    a.new_desc_len = desc_len;
    a.n_removed = n_removed;
    // the buffers whose size the scans have just given, and the host's
    AH_TRY(alloc(&new_desc, (size_t)desc_len * 4));
    AH_TRY(alloc(&out, (size_t)n_removed * 4));
    delta->removed.resize(n_removed);
    // 3. copy, in launches of at most AH_LAUNCH_MAX_ITEMS nodes
    for_spans(nn, call.span(), [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_drop_copy, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi,
                           new_desc.as<uint32_t>());
    });
    AH_HIP(hipGetLastError());
    const auto t_copy = call.phase_end();
    // 4. apply
    hipLaunchKernelGGL(k_drop_apply, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, new_nodes.as<DNode>(), out.as<uint32_t>());
    // read back
    AH_HIP(hipMemcpyAsync(delta->removed.data(), out.p, (size_t)n_removed * 4, hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(ctl, a.ctl, DCTL_WORDS, s));
    AH_REQUIRE(ctl[DCTL_ERR] == 0, AH_ERR_DEVICE, "the index drop found its own counts inconsistent (%u): the index is unchanged", ctl[DCTL_ERR]);
    delta->roots = std::move(roots);
    const auto t_apply = call.now();
    IndexCommit c(ix, &new_nodes, &new_roots, &new_desc, &new_rank);
    c.n_trees = kept;
    c.desc_len = desc_len;
    c.n_leaves = ctl[DCTL_LEAVES];
    c.max_desc = ctl[DCTL_MAX_DESC];
    c.compacted = false;
    index_commit(ix, c);
    if (call.timing)
        fprintf(stderr, "[ah] index drop: %u of %u trees, %u of %u nodes freed in %zu levels, %llu -> %u stored ids: "
                        "levels %.6f s, lengths %.6f s, copy %.6f s, apply and read-back %.6f s\n",
                n_drop, n_trees, n_removed, nn, levels, (unsigned long long)old_desc_len, desc_len, call.secs(call.t0, t_levels),
                call.secs(t_levels, t_lengths), call.secs(t_lengths, t_copy), call.secs(t_copy, t_apply));
    return AH_OK;
}

int insert_impl(ah_index *ix, const uint32_t *ids, size_t n, const uint64_t *seeds, ah_index_delta *delta) {
    ah_dataset *ds = ix->ds;
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    const uint32_t nn = ix->n_nodes, n_trees = ix->n_trees;
    const uint64_t old_desc_len = ix->desc_len;
    const uint64_t pairs = (uint64_t)n * n_trees;
    AH_REQUIRE(old_desc_len + pairs < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
               "%llu stored ids + %llu inserted ones are too many for 32-bit descendant offsets", (unsigned long long)old_desc_len,
               (unsigned long long)pairs);
    // every buffer whose size is known now; kernels write only into these
    InsertArgs a{};
    a.nodes = ix->d_nodes;
    a.n_nodes = nn;
    a.desc = ix->d_desc;
    a.old_desc_len = old_desc_len;
    a.n_pairs = pairs;
    uint64_t *d_seeds = nullptr;
    uint32_t *tile_sums = nullptr, *d_ids = nullptr, *d_leaf = nullptr;
    const Workspace ws = insert_workspace(a, &d_seeds, &tile_sums, &d_ids, &d_leaf, nn, n_trees, n, kScanTile, ICTL_WORDS);
    DevMem work, new_nodes, new_desc, out;
    AH_TRY(alloc(&work, ws.bytes()));
    ws.carve(work.p, ws.bytes());
    AH_TRY(alloc(&new_nodes, (size_t)nn * sizeof(DNode)));
    delta->roots.resize(n_trees);
    AH_HIP(hipMemsetAsync(a.cnt, 0, ws.zeroed_bytes(), s));  // (a.cnt: the first array behind the seeds)
    AH_HIP(hipMemsetAsync(a.ctl + ICTL_FIRST_BAD, 0xFF, 4, s));
    uint32_t ctl[ICTL_WORDS] = {};
    // 1. check
    if (n) {
        AH_HIP(hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, s));
        if (n_trees) AH_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t)n_trees * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_insert_check, dim3(grid_of(n, kIxBlock, 4096)), dim3(kIxBlock), 0, s, ds->view(), (const uint32_t *)d_ids, (uint64_t)n,
                           a.ctl);
        AH_TRY(read_back(ctl, a.ctl, ICTL_WORDS, s));
        AH_REQUIRE(ctl[ICTL_FIRST_BAD] >= n, AH_ERR_INVALID_ARGUMENT, "item %u (position %u of sorted_ids) is not a row of the dataset",
                   ids[std::min<size_t>(ctl[ICTL_FIRST_BAD], n - 1)], ctl[ICTL_FIRST_BAD]);
    }
    const uint64_t span = call.span();
    // the ids in runs of at most AH_LAUNCH_MAX_ITEMS pairs; the pairs of ids [i0, i1) are d_leaf[i0 * n_trees, i1 * n_trees), tree-major
    const uint64_t run = pairs ? std::max<uint64_t>(1, std::min<uint64_t>(n, span / n_trees)) : 1;
    if (pairs) {
        // 2. route, 3. count
        uint32_t *d_route_err = a.ctl + ICTL_ERR;  // (bit 0, as the count pass: an id without a row, refused above)
        for (uint64_t i0 = 0; i0 < n; i0 += run) {  // (no for_spans: the routing may refuse)
            const uint64_t cn = std::min<uint64_t>(run, n - i0), m = cn * n_trees;
            AH_TRY(launch_route_items(ix, d_ids + i0, cn, d_seeds, d_leaf + i0 * n_trees, d_route_err, s));
            hipLaunchKernelGGL(k_insert_count, dim3(grid_of(m, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, (const uint32_t *)(d_leaf + i0 * n_trees), m);
        }
        AH_HIP(hipGetLastError());
        AH_HIP(hipMemcpyAsync(a.seg, a.cnt, (size_t)nn * 4, hipMemcpyDeviceToDevice, s));
        launch_exclusive_scan(a.seg, nn, tile_sums, a.ctl + ICTL_DESC_LEN, s);  // (the total, n_pairs, is overwritten below)
    }
    if (nn) hipLaunchKernelGGL(k_insert_flags, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    launch_exclusive_scan(a.chg, nn, tile_sums, a.ctl + ICTL_TOUCHED, s);
    if (pairs) {
        hipLaunchKernelGGL(k_insert_touched, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
        // 4. scatter
        for_spans(n, run, [&](uint64_t i0, uint64_t i1) {
            const uint64_t cn = i1 - i0, m = cn * n_trees;
            hipLaunchKernelGGL(k_insert_scatter, dim3(grid_of(m, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, (const uint32_t *)(d_ids + i0), cn,
                               (const uint32_t *)(d_leaf + i0 * n_trees), m);
        });
    }
    AH_TRY(read_back(ctl, a.ctl, ICTL_WORDS, s));
    AH_REQUIRE(ctl[ICTL_ERR] == 0 && ctl[ICTL_TOUCHED] <= nn && ctl[ICTL_TOUCHED] <= pairs, AH_ERR_DEVICE,
               "the index insert routed an id to a node that is no Descendants node (%u): the index is unchanged", ctl[ICTL_ERR]);
    const uint32_t n_touched = ctl[ICTL_TOUCHED];
    a.n_touched = n_touched;
    // 5. fresh and the scans
    if (n_touched) {
        hipLaunchKernelGGL(k_insert_sort, dim3(grid_of(n_touched, 1, 1u << 16)), dim3(kIxBlock), 0, s, a);
        for_spans(n_touched, span, [&](uint64_t lo, uint64_t hi) {
            hipLaunchKernelGGL(k_insert_fresh, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi);
        });
    }
    launch_exclusive_scan(a.nlen, nn, tile_sums, a.ctl + ICTL_DESC_LEN, s);
    launch_exclusive_scan(a.dlen, nn, tile_sums, a.ctl + ICTL_DELTA_DESC, s);
    AH_TRY(read_back(ctl, a.ctl, ICTL_WORDS, s));
    const uint32_t desc_len = ctl[ICTL_DESC_LEN], delta_desc = ctl[ICTL_DELTA_DESC];
    AH_REQUIRE(ctl[ICTL_ERR] == 0 && desc_len <= old_desc_len + pairs && delta_desc <= desc_len, AH_ERR_DEVICE, "the index insert found its own counts inconsistent (%u): the index is unchanged", ctl[ICTL_ERR]);
    a.new_desc_len = desc_len;
    a.delta_desc_len = delta_desc;
    // the buffers whose size the scans have just given, and the host's
    AH_TRY(alloc(&new_desc, (size_t)desc_len * 4));
    AH_TRY(alloc(&out, (size_t)n_touched * sizeof(DeltaEntry) + (size_t)delta_desc * 4));
    std::vector<DeltaEntry> entries(n_touched);
    delta->desc.resize(delta_desc);
    delta->put_index.reserve(n_touched);
    delta->put.reserve(n_touched);
    DeltaEntry *d_entries = out.as<DeltaEntry>();
    uint32_t *d_delta_desc = reinterpret_cast<uint32_t *>(d_entries + n_touched);
    // 6. write, 7. apply
    for_spans(nn, span, [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_insert_write, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi,
                           new_desc.as<uint32_t>());
    });
    if (nn) hipLaunchKernelGGL(k_insert_apply, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, new_nodes.as<DNode>(), d_entries);
    if (n_touched)
        hipLaunchKernelGGL(k_insert_gather, dim3(grid_of(n_touched, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, (const DeltaEntry *)d_entries,
                           new_desc.as<const uint32_t>(), d_delta_desc);
    // read back
    if (n_touched) AH_HIP(hipMemcpyAsync(entries.data(), d_entries, (size_t)n_touched * sizeof(DeltaEntry), hipMemcpyDeviceToHost, s));
    if (delta_desc) AH_HIP(hipMemcpyAsync(delta->desc.data(), d_delta_desc, (size_t)delta_desc * 4, hipMemcpyDeviceToHost, s));
    if (n_trees) AH_HIP(hipMemcpyAsync(delta->roots.data(), ix->d_roots, (size_t)n_trees * 4, hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(ctl, a.ctl, ICTL_WORDS, s));
    AH_REQUIRE(ctl[ICTL_ERR] == 0, AH_ERR_DEVICE, "the index insert found its own counts inconsistent (%u): the index is unchanged", ctl[ICTL_ERR]);
    for (const DeltaEntry &e : entries) {
        delta->put_index.push_back(e.node);
        delta->put.push_back(to_host_node(DNode{e.kind, e.a, e.b, 0}));
    }
    IndexCommit c(ix, &new_nodes, nullptr, &new_desc, nullptr);
    c.desc_len = desc_len;
    c.n_leaves = ctl[ICTL_LEAVES];
    c.max_desc = ctl[ICTL_MAX_DESC];
    index_commit(ix, c);
    if (tun(TUN_TIMING) != 0)
        fprintf(stderr, "[ah] index insert: %zu ids x %u trees into %u of %u nodes, %llu -> %u stored ids\n", n, n_trees, n_touched, nn,
                (unsigned long long)old_desc_len, desc_len);
    return AH_OK;
}

// `src` (ah_index_graft_forest, ah_index_create_from_forest): the view is the one of the resident forest whose device copy `src`
// is.  The lists are gathered from its ids and its rows are copied behind the index's own, device to device: neither blob of the
// view is read.  An index without a normal row ADOPTS the rows and headers instead (*adopted_rows: the blocks changed hands).
int graft_impl(ah_index *ix, const ah_forest_view &v, const uint32_t *targets, const uint32_t *new_index, uint32_t *out_new_of_old,
               const ForestDevice *src = nullptr, bool *adopted_rows = nullptr) {
    ah_dataset *ds = ix->ds;
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    const uint32_t n_old = ix->n_nodes, n_trees = ix->n_trees, n_view = (uint32_t)v.n_nodes;
    // ---- validation: nothing is touched before it is through
    uint32_t n_used = n_old;
    if (ix->d_rank) {
        AH_HIP(hipMemcpyAsync(&n_used, ix->d_rank + n_old, 4, hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        AH_REQUIRE(n_used <= n_old, AH_ERR_DEVICE, "the index counts more nodes in use than it has");
    }
    std::vector<uint32_t> vtgt(n_view, kNone), vfin(n_view, kNone), added_roots, repl;
    for (uint32_t t = 0; t < v.n_trees; t++) {
        if (targets[t] == AH_NEW_ROOT) {
            added_roots.push_back(v.roots[t]);
            continue;
        }
        AH_REQUIRE(targets[t] < n_old, AH_ERR_INVALID_ARGUMENT, "targets[%u] = %u is no node of the index (%u nodes)", t, targets[t], n_old);
        vtgt[v.roots[t]] = targets[t];
        repl.push_back(targets[t]);
    }
    const uint32_t n_repl = (uint32_t)repl.size();
    {
        std::vector<uint32_t> sorted(repl);
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 1; i < sorted.size(); i++)
            AH_REQUIRE(sorted[i - 1] != sorted[i], AH_ERR_INVALID_ARGUMENT, "node %u is the target of two trees", sorted[i]);
    }
    const uint64_t n_new64 = (uint64_t)n_used + n_view - n_repl;
    AH_REQUIRE(n_new64 < 0xFFFFFFFFull && ix->desc_len + v.descendants_len < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
               "the index would outgrow 32-bit node / descendant offsets");
    const uint32_t n_new = (uint32_t)n_new64;
    {
        uint32_t next = n_used;
        std::vector<uint32_t> named;
        named.reserve(n_view - n_repl);
        for (uint32_t k = 0; k < n_view; k++) {
            if (vtgt[k] != kNone) {
                AH_REQUIRE(!new_index || new_index[k] == kNone, AH_ERR_INVALID_ARGUMENT,
                           "new_index[%u] = %u: a root that replaces a node takes that node's place and must be given as 0xFFFFFFFF", k,
                           new_index[k]);
                continue;
            }
            vfin[k] = new_index ? new_index[k] : next++;
            AH_REQUIRE(vfin[k] < n_new, AH_ERR_INVALID_ARGUMENT, "new_index[%u] = %u is not below the %u nodes the index will have", k, vfin[k],
                       n_new);
            named.push_back(vfin[k]);
        }
        std::sort(named.begin(), named.end());
        for (size_t i = 1; i < named.size(); i++)
            AH_REQUIRE(named[i - 1] != named[i], AH_ERR_INVALID_ARGUMENT, "new_index names position %u twice", named[i]);
    }
    // the view's nodes in the device's shape: c of a split node with a plane = the ordinal of its record
    std::vector<DNode> vnodes(n_view);
    std::vector<uint64_t> offsets;
    for (uint32_t k = 0; k < n_view; k++) {
        vnodes[k] = to_device_node(v.nodes[k], (uint32_t)offsets.size());
        if (vnodes[k].kind & 0x100u) offsets.push_back(v.nodes[k].offset);
    }
    const uint32_t n_vnormals = (uint32_t)offsets.size(), n_added = (uint32_t)added_roots.size();
    AH_REQUIRE((uint64_t)ix->n_normals + n_vnormals < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "too many normals for 32-bit rows");
    AH_REQUIRE(!src || (src->n_rows == n_vnormals && src->ids_len == v.descendants_len), AH_ERR_DEVICE,
               "the forest's device copy does not match its view (internal error)");
    // ---- buffers
    const uint32_t hf = header_floats(ds->metric);
    const size_t row_bytes = ds->row_bytes();
    GraftArgs a{};
    a.nodes = ix->d_nodes;
    a.n_old = n_old;
    a.n_used = n_used;
    a.rank = ix->d_rank;
    a.desc = ix->d_desc;
    a.old_desc_len = ix->desc_len;
    a.n_view = n_view;
    a.vdesc_len = v.descendants_len;
    a.n_new = n_new;
    a.first_row = ix->n_normals;
    uint32_t *tile_sums = nullptr;
    GraftUploads<DNode> u{};
    const Workspace ws = graft_workspace(a, &tile_sums, u, GraftSizes{n_old, n_used, n_view, n_new, n_repl, n_added, src ? 0 : v.descendants_len},
                                         kScanTile, GCTL_WORDS);
    DevMem work, new_nodes, new_roots, new_desc, recs, offs, grown_rows, grown_hdrs;
    AH_TRY(alloc(&work, ws.bytes()));
    ws.carve(work.p, ws.bytes());
    a.vfin = u.vfin;  // (the kernels read what the host uploads through these)
    a.vtgt = u.vtgt;
    a.vdesc = src ? src->ids : u.vdesc;
    a.vnodes = u.vnodes;
    AH_TRY(alloc(&new_nodes, (size_t)n_new * sizeof(DNode)));
    AH_TRY(alloc(&new_roots, ((size_t)n_trees + n_added) * 4));
    AH_HIP(hipMemsetAsync(work.p, 0, ws.zeroed_bytes(), s));
    if (n_view) {
        AH_HIP(hipMemcpyAsync(u.vfin, vfin.data(), (size_t)n_view * 4, hipMemcpyHostToDevice, s));
        AH_HIP(hipMemcpyAsync(u.vtgt, vtgt.data(), (size_t)n_view * 4, hipMemcpyHostToDevice, s));
        AH_HIP(hipMemcpyAsync(u.vnodes, vnodes.data(), (size_t)n_view * sizeof(DNode), hipMemcpyHostToDevice, s));
    }
    if (n_repl) AH_HIP(hipMemcpyAsync(u.repl, repl.data(), (size_t)n_repl * 4, hipMemcpyHostToDevice, s));
    if (n_added) AH_HIP(hipMemcpyAsync(u.added, added_roots.data(), (size_t)n_added * 4, hipMemcpyHostToDevice, s));
    if (v.descendants_len && !src) AH_HIP(hipMemcpyAsync(u.vdesc, v.descendants, v.descendants_len * 4, hipMemcpyHostToDevice, s));
    if (n_repl) {  // the targets: in use and Descendants nodes
        std::vector<uint32_t> kinds(n_repl);
        hipLaunchKernelGGL(k_graft_peek, dim3(grid_of(n_repl, kIxBlock, 1024)), dim3(kIxBlock), 0, s, (const DNode *)ix->d_nodes,
                           (const uint32_t *)u.repl, n_repl, u.kinds);
        AH_TRY(read_back(kinds.data(), u.kinds, n_repl, s));
        for (uint32_t i = 0; i < n_repl; i++)
            AH_REQUIRE((kinds[i] & 0xFFu) == AH_NODE_DESCENDANTS, AH_ERR_INVALID_ARGUMENT, "target %u is %s", repl[i],
                       kinds[i] == 0 ? "a free slot of the index" : "a split node, not a Descendants node");
    }
    // ---- 1. named, 2. lengths
    if (n_view) hipLaunchKernelGGL(k_graft_named, dim3(grid_of(n_view, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    launch_exclusive_scan(a.named, n_new, tile_sums, a.named + n_new, s);
    if (n_new) hipLaunchKernelGGL(k_graft_positions, dim3(grid_of(n_new, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    if (n_old) hipLaunchKernelGGL(k_graft_old_map, dim3(grid_of(n_old, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    if (n_view) hipLaunchKernelGGL(k_graft_fin, dim3(grid_of(n_view, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    const uint64_t items = (uint64_t)n_old + n_view;
    if (items) hipLaunchKernelGGL(k_graft_len, dim3(grid_of(items, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a);
    launch_exclusive_scan(a.len, n_new, tile_sums, a.ctl + GCTL_DESC_LEN, s);
    uint32_t ctl[GCTL_WORDS] = {};
    AH_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(&ctl[GCTL_NAMED], a.named + n_new, 1, s));
    AH_REQUIRE(ctl[GCTL_ERR] == 0 && ctl[GCTL_NAMED] == n_view - n_repl && ctl[GCTL_DESC_LEN] <= ix->desc_len + v.descendants_len,
               AH_ERR_DEVICE, "the index graft found its own counts inconsistent (%u): the index is unchanged", ctl[GCTL_ERR]);
    const uint32_t desc_len = ctl[GCTL_DESC_LEN];
    a.new_desc_len = desc_len;
    AH_TRY(alloc(&new_desc, (size_t)desc_len * 4));
    // ---- 5. normals: into the spare rows, or into arrays grown geometrically
    const uint32_t need = ix->n_normals + n_vnormals;
    uint32_t cap = ix->normals_cap;
    void *rows = ix->d_nrows;
    float *hdrs = ix->d_nhdrs;
    const bool adopt = src && ix->n_normals == 0 && n_vnormals != 0;  // (the forest's blocks hold exactly its rows)
    if (adopt) {
        cap = n_vnormals;
    } else if (need > cap) {
        cap = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, std::max<uint64_t>(need, 2 * (uint64_t)cap));
        AH_TRY(alloc(&grown_rows, (size_t)cap * row_bytes));
        AH_TRY(alloc(&grown_hdrs, (size_t)cap * hf * 4));
        rows = grown_rows.p;
        hdrs = grown_hdrs.as<float>();
        if (ix->n_normals) {
            AH_HIP(hipMemcpyAsync(rows, ix->d_nrows, (size_t)ix->n_normals * row_bytes, hipMemcpyDeviceToDevice, s));
            AH_HIP(hipMemcpyAsync(hdrs, ix->d_nhdrs, (size_t)ix->n_normals * hf * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    if (n_vnormals && src && !adopt) {
        AH_HIP(hipMemcpyAsync(static_cast<uint8_t *>(rows) + (size_t)ix->n_normals * row_bytes, src->rows, (size_t)n_vnormals * row_bytes,
                              hipMemcpyDeviceToDevice, s));
        AH_HIP(hipMemcpyAsync(hdrs + (size_t)ix->n_normals * hf, src->hdrs, (size_t)n_vnormals * hf * 4, hipMemcpyDeviceToDevice, s));
    } else if (n_vnormals && !src) {
        AH_TRY(alloc(&recs, v.normals_len));
        AH_TRY(alloc(&offs, offsets.size() * 8));
        AH_HIP(hipMemcpyAsync(recs.p, v.normals, v.normals_len, hipMemcpyHostToDevice, s));
        AH_HIP(hipMemcpyAsync(offs.p, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice, s));
        AH_TRY(launch_unpack_normals(ds, recs.as<uint8_t>(), offs.as<uint64_t>(), n_vnormals, v.normal_vector_offset, v.normal_header_offset,
                                     static_cast<uint8_t *>(rows) + (size_t)ix->n_normals * row_bytes, hdrs + (size_t)ix->n_normals * hf, s));
    }
    // ---- 3. nodes, 4. lists
    if (items) hipLaunchKernelGGL(k_graft_nodes, dim3(grid_of(items, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, new_nodes.as<DNode>());
    for_spans(items, call.span(), [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_graft_lists, dim3(grid_of(hi - lo, kIxBlock / 64, 1u << 16)), dim3(kIxBlock), 0, s, a, lo, hi, new_desc.as<uint32_t>());
    });
    if (n_trees + n_added)
        hipLaunchKernelGGL(k_graft_roots, dim3(grid_of((uint64_t)n_trees + n_added, kIxBlock, 1024)), dim3(kIxBlock), 0, s, a,
                           (const uint32_t *)ix->d_roots, n_trees, (const uint32_t *)u.added, n_added, new_roots.as<uint32_t>());
    std::vector<uint32_t> map_out(out_new_of_old ? n_old : 0);
    if (out_new_of_old && n_old) AH_HIP(hipMemcpyAsync(map_out.data(), a.new_of_old, (size_t)n_old * 4, hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(ctl, a.ctl, GCTL_WORDS, s));
    AH_REQUIRE(ctl[GCTL_ERR] == 0, AH_ERR_DEVICE, "the index graft found its own counts inconsistent (%u): the index is unchanged", ctl[GCTL_ERR]);
    if (out_new_of_old && n_old) memcpy(out_new_of_old, map_out.data(), (size_t)n_old * 4);
    if (adopt) {  // (nothing fails from here on: the blocks change hands, the index's own go when the call returns)
        grown_rows.p = src->rows;
        grown_hdrs.p = src->hdrs;
        if (adopted_rows) *adopted_rows = true;
    }
    const bool grown = grown_rows.p != nullptr;  // (the rows moved into larger arrays: cap is their room)
    IndexCommit c(ix, &new_nodes, &new_roots, &new_desc, nullptr, grown ? &grown_rows : nullptr, grown ? &grown_hdrs : nullptr);
    c.drop_rank = true;
    c.normals_cap = cap;
    c.n_normals = need;
    c.n_nodes = n_new;
    c.n_trees = n_trees + n_added;
    c.desc_len = desc_len;
    c.n_leaves = ctl[GCTL_LEAVES];
    c.max_desc = ctl[GCTL_MAX_DESC];
    c.compacted = false;
    index_commit(ix, c);
    if (tun(TUN_TIMING) != 0)
        fprintf(stderr, "[ah] index graft: %u view nodes (%u replacing roots, %u new roots, %u normals) into %u nodes -> %u nodes, %u stored ids\n",
                n_view, n_repl, n_added, n_vnormals, n_used, n_new, desc_len);
    return AH_OK;
}

// HBM an index of these sizes holds: what ah_index_create_from_view obtains, plus the ranks when a delete has left some
uint64_t index_device_bytes(const ah_index *ix, uint64_t n_nodes, bool rank, uint64_t normals_cap) {
    const uint64_t per_row = ix->ds->row_bytes() + (uint64_t)header_floats(ix->ds->metric) * 4;
    return std::max<uint64_t>(1, n_nodes) * sizeof(DNode) + std::max<uint64_t>(1, ix->n_trees) * 4 + (rank ? (n_nodes + 1) * 4 : 0) +
           std::max<uint64_t>(1, ix->desc_len) * 4 + normals_cap * per_row;
}

// pass 1 of the compaction, which is all of ah_index_footprint_get: `work` gets the workspace (compact_workspace, `extra` words
// behind it); ctl[CCTL_*] is read back
int compact_count(ah_index *ix, hipStream_t s, DevMem *work, size_t extra_words, CompactArgs *a, uint32_t **extra, uint32_t *ctl) {
    const uint32_t nn = ix->n_nodes;
    a->nodes = ix->d_nodes;
    a->n_nodes = nn;
    a->old_rows = ix->n_normals;
    uint32_t *tile_sums = nullptr;
    const Workspace ws = compact_workspace(*a, &tile_sums, extra, nn, extra_words, kScanTile, CCTL_WORDS);
    AH_TRY(alloc(work, ws.bytes()));
    ws.carve(work->p, ws.bytes());
    AH_HIP(hipMemsetAsync(a->ctl, 0, CCTL_WORDS * 4, s));
    if (nn) hipLaunchKernelGGL(k_compact_flags, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, *a);
    launch_exclusive_scan(a->new_index, nn, tile_sums, a->ctl + CCTL_USED, s);
    launch_exclusive_scan(a->new_row, nn, tile_sums, a->ctl + CCTL_LIVE, s);
    if (nn) hipLaunchKernelGGL(k_compact_placed, dim3(grid_of(nn, kIxBlock, 4096)), dim3(kIxBlock), 0, s, *a);
    AH_TRY(read_back(ctl, a->ctl, CCTL_WORDS, s));
    AH_REQUIRE(ctl[CCTL_USED] <= nn && ctl[CCTL_LIVE] <= ctl[CCTL_USED], AH_ERR_DEVICE, "the index counts more nodes in use than it has");
    a->n_used = ctl[CCTL_USED];
    a->n_live = ctl[CCTL_LIVE];
    return AH_OK;
}

int footprint_impl(ah_index *ix, ah_index_footprint *out) {
    IndexCall call;
    AH_TRY(call.begin(ix->ds));
    DevMem work;
    CompactArgs a{};
    uint32_t *extra = nullptr;
    uint32_t ctl[CCTL_WORDS] = {};
    AH_TRY(compact_count(ix, call.stream(), &work, 0, &a, &extra, ctl));
    out->n_nodes = ix->n_nodes;
    out->free_slots = ix->n_nodes - a.n_used;
    out->n_normals = ix->n_normals;
    out->live_normals = a.n_live;
    out->normals_cap = ix->normals_cap;
    out->desc_len = ix->desc_len;
    out->device_bytes = index_device_bytes(ix, ix->n_nodes, ix->d_rank != nullptr, ix->normals_cap);
    return AH_OK;
}

int compact_impl(ah_index *ix, uint32_t *out_new_of_old, ah_index_compact_stats *stats) {
    ah_dataset *ds = ix->ds;
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    const uint32_t nn = ix->n_nodes, n_trees = ix->n_trees, old_rows = ix->n_normals, old_cap = ix->normals_cap;
    ah_index_compact_stats st{};
    st.nodes_before = st.nodes_after = nn;
    st.normals_before = st.normals_after = old_rows;
    st.normals_cap_before = st.normals_cap_after = old_cap;
    st.device_bytes_before = st.device_bytes_after = index_device_bytes(ix, nn, ix->d_rank != nullptr, old_cap);
    auto nothing_to_do = [&]() {
        if (out_new_of_old)
            for (uint32_t i = 0; i < nn; i++) out_new_of_old[i] = i;
        if (stats) *stats = st;
        return AH_OK;
    };
    // a fresh index, or one compacted and not deleted from or grafted on since: the host knows, and nothing is allocated
    if (ix->compacted) return nothing_to_do();
    // 1. flags and scans
    DevMem work, new_nodes, new_roots, new_rows, new_hdrs, row_src;
    CompactArgs a{};
    uint32_t *d_map = nullptr;
    uint32_t ctl[CCTL_WORDS] = {};
    AH_TRY(compact_count(ix, s, &work, out_new_of_old ? nn : 0, &a, &d_map, ctl));
    if (!out_new_of_old) d_map = nullptr;
    const uint32_t n_used = a.n_used, n_live = a.n_live;
    const uint32_t new_cap = std::max<uint32_t>(1, n_live);
    const auto t_count = call.now();
    if (n_used == nn && n_live == old_rows && ctl[CCTL_MISPLACED] == 0 && old_cap == new_cap && !ix->d_rank) {
        // no free slot, no dead row, every row where a fresh index has it, no spare row, no ranks: nothing but the scratch of
        // the count was obtained, and it goes back here
        ix->compacted = true;
        return nothing_to_do();
    }
    // every other buffer; kernels write only into these
    const uint32_t hf = header_floats(ds->metric);
    const size_t row_bytes = ds->row_bytes();
    AH_TRY(alloc(&new_nodes, std::max<size_t>(1, n_used) * sizeof(DNode)));
    AH_TRY(alloc(&new_roots, std::max<size_t>(1, n_trees) * 4));
    AH_TRY(alloc(&new_rows, (size_t)new_cap * row_bytes));
    AH_TRY(alloc(&new_hdrs, (size_t)new_cap * hf * 4));
    AH_TRY(alloc(&row_src, (size_t)new_cap * 4));
    std::vector<uint32_t> map_out(out_new_of_old ? nn : 0);
    AH_HIP(hipMemsetAsync(row_src.p, 0, (size_t)new_cap * 4, s));
    // 2. nodes, in launches of at most AH_LAUNCH_MAX_ITEMS slots
    const uint64_t span = call.span();
    for_spans(nn, span, [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_compact_nodes, dim3(grid_of(hi - lo, kIxBlock, 4096)), dim3(kIxBlock), 0, s, a, (uint32_t)lo, (uint32_t)hi,
                           new_nodes.as<DNode>(), row_src.as<uint32_t>(), d_map);
    });
    if (n_trees)
        hipLaunchKernelGGL(k_compact_roots, dim3(grid_of(n_trees, kIxBlock, 1024)), dim3(kIxBlock), 0, s, a, (const uint32_t *)ix->d_roots, n_trees,
                           new_roots.as<uint32_t>());
    AH_HIP(hipGetLastError());
    const auto t_nodes = call.phase_end();
    // 3. rows, in launches of at most AH_LAUNCH_MAX_ITEMS rows
    for_spans(n_live, span, [&](uint64_t lo, uint64_t hi) {
        hipLaunchKernelGGL(k_compact_rows, dim3(grid_of(hi - lo, kIxBlock / 64, 8192)), dim3(kIxBlock), 0, s, (const uint8_t *)ix->d_nrows,
                           (const float *)ix->d_nhdrs, row_src.as<const uint32_t>(), old_rows, lo, hi, (uint64_t)row_bytes, hf, new_rows.as<uint8_t>(),
                           new_hdrs.as<float>(), a.ctl);
    });
    if (out_new_of_old && nn) AH_HIP(hipMemcpyAsync(map_out.data(), d_map, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
    AH_TRY(read_back(ctl, a.ctl, CCTL_WORDS, s));
    AH_REQUIRE(ctl[CCTL_ERR] == 0, AH_ERR_DEVICE, "the index compaction found the index inconsistent (%u): the index is unchanged", ctl[CCTL_ERR]);
    const auto t_rows = call.now();
    if (out_new_of_old && nn) memcpy(out_new_of_old, map_out.data(), (size_t)nn * 4);
    IndexCommit c(ix, &new_nodes, &new_roots, nullptr, nullptr, &new_rows, &new_hdrs);
    c.drop_rank = true;
    c.n_nodes = n_used;
    c.n_normals = n_live;
    c.normals_cap = new_cap;
    c.compacted = true;
    index_commit(ix, c);
    st.nodes_after = n_used;
    st.normals_after = n_live;
    st.normals_cap_after = new_cap;
    st.device_bytes_after = index_device_bytes(ix, n_used, false, new_cap);
    st.moved = 1;
    if (stats) *stats = st;
    if (call.timing)
        fprintf(stderr, "[ah] index compact: %u -> %u nodes, %u -> %u normal rows (room for %u -> %u), %llu -> %llu bytes: "
                        "flags and scans %.6f s, nodes %.6f s, rows %.6f s, swap %.6f s\n",
                nn, n_used, old_rows, n_live, old_cap, new_cap, (unsigned long long)st.device_bytes_before,
                (unsigned long long)st.device_bytes_after, call.secs(call.t0, t_count), call.secs(t_count, t_nodes), call.secs(t_nodes, t_rows),
                call.secs(t_rows, call.now()));
    return AH_OK;
}

// what the delete and the insert ask of their id list (judged before the index is looked at)
int check_sorted_ids(const uint32_t *sorted_ids, size_t n) {
    AH_REQUIRE(n == 0 || sorted_ids, AH_ERR_INVALID_ARGUMENT, "sorted_ids is NULL");
    AH_REQUIRE(n < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "more ids than the u32 item-id space holds");
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(sorted_ids[i - 1] < sorted_ids[i], AH_ERR_INVALID_ARGUMENT, "sorted_ids is not strictly ascending at position %zu (%u after %u)",
                   i, sorted_ids[i], sorted_ids[i - 1]);
    return AH_OK;
}

}  // namespace

extern "C" {

int ah_index_delete_items(ah_index *ix, const uint32_t *sorted_ids, size_t n, uint32_t split_after, ah_index_delta **out_delta) {
    AH_GUARDED("ah_index_delete_items")
    AH_REQUIRE(out_delta, AH_ERR_INVALID_ARGUMENT, "out_delta is NULL");
    *out_delta = nullptr;
    // (what can be judged without the index first)
    AH_TRY(check_sorted_ids(sorted_ids, n));
    AH_TRY(index_updatable(ix));
    DeviceRestore restore_device;
    std::unique_ptr<ah_index_delta> delta(new ah_index_delta);
    AH_TRY(delete_impl(ix, sorted_ids, n, split_after, delta.get()));
    *out_delta = delta.release();
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_drop_trees(ah_index *ix, uint32_t n_drop, uint32_t flags, ah_index_delta **out_delta) {
    AH_GUARDED("ah_index_drop_trees")
    AH_REQUIRE(out_delta, AH_ERR_INVALID_ARGUMENT, "out_delta is NULL");
    *out_delta = nullptr;
    // (what can be judged without the index first)
    AH_REQUIRE((flags & ~AH_DROP_SORT_ROOTS) == 0, AH_ERR_INVALID_ARGUMENT, "flags = 0x%x: only AH_DROP_SORT_ROOTS is known", flags);
    AH_TRY(index_updatable(ix));
    DeviceRestore restore_device;
    std::unique_ptr<ah_index_delta> delta(new ah_index_delta);
    AH_TRY(drop_impl(ix, n_drop, (flags & AH_DROP_SORT_ROOTS) != 0, delta.get()));
    *out_delta = delta.release();
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_insert_items(ah_index *ix, const uint32_t *sorted_ids, size_t n, const uint64_t *tree_seeds, ah_index_delta **out_delta) {
    AH_GUARDED("ah_index_insert_items")
    AH_REQUIRE(out_delta, AH_ERR_INVALID_ARGUMENT, "out_delta is NULL");
    *out_delta = nullptr;
    // (what can be judged without the index first)
    AH_TRY(check_sorted_ids(sorted_ids, n));
    AH_TRY(index_updatable(ix));
    AH_REQUIRE(n == 0 || ix->n_trees == 0 || tree_seeds, AH_ERR_INVALID_ARGUMENT, "tree_seeds is NULL");
    DeviceRestore restore_device;
    std::unique_ptr<ah_index_delta> delta(new ah_index_delta);
    AH_TRY(insert_impl(ix, sorted_ids, n, tree_seeds, delta.get()));
    *out_delta = delta.release();
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_graft(ah_index *ix, const ah_forest_view *view, const uint32_t *targets, const uint32_t *new_index, uint32_t *out_new_of_old) {
    AH_GUARDED("ah_index_graft")
    AH_TRY(index_updatable(ix));
    AH_REQUIRE(view, AH_ERR_INVALID_ARGUMENT, "view is NULL");
    const ah_forest_view v = *view;
    AH_TRY(validate_forest_view(ix->ds, v));
    AH_REQUIRE(v.n_trees == 0 || targets, AH_ERR_INVALID_ARGUMENT, "targets is NULL");
    DeviceRestore restore_device;
    return graft_impl(ix, v, targets, new_index, out_new_of_old);
    AH_GUARDED_END
}

// The forest's device copy when it can serve a call on `ds`, else nullptr (the call then takes the host view): resident, on the
// dataset's device, of its metric and dimensions.
static const ForestDevice *usable_forest_device(const ah_dataset *ds, const ah_forest *forest) {
    const ForestDevice *fd = forest_device(forest);
    return fd && fd->device == ds->device && fd->metric == ds->metric && fd->dims == ds->dims ? fd : nullptr;
}

int ah_index_graft_forest(ah_index *ix, ah_forest *forest, const uint32_t *targets, const uint32_t *new_index, uint32_t *out_new_of_old,
                          int *out_from_device) {
    AH_GUARDED("ah_index_graft_forest")
    if (out_from_device) *out_from_device = 0;
    AH_TRY(index_updatable(ix));
    AH_REQUIRE(forest, AH_ERR_INVALID_ARGUMENT, "forest is NULL");
    ah_forest_view v;
    AH_TRY(ah_forest_view_get(forest, &v));
    const ForestDevice *src = usable_forest_device(ix->ds, forest);
    if (!src) AH_TRY(validate_forest_view(ix->ds, v));  // (a library-built forest: only the caller's arrays are judged on the device path)
    AH_REQUIRE(v.n_trees == 0 || targets, AH_ERR_INVALID_ARGUMENT, "targets is NULL");
    DeviceRestore restore_device;
    bool adopted_rows = false;
    AH_TRY(graft_impl(ix, v, targets, new_index, out_new_of_old, src, &adopted_rows));
    if (src) {
        forest_device_consume(forest, false, adopted_rows);
        if (out_from_device) *out_from_device = 1;
    }
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_create_from_forest(ah_dataset *ds, ah_forest *forest, const uint32_t *new_index, int *out_from_device, ah_index **out) {
    AH_GUARDED("ah_index_create_from_forest")
    if (out_from_device) *out_from_device = 0;
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(ds && forest, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    ah_forest_view v;
    AH_TRY(ah_forest_view_get(forest, &v));
    const ForestDevice *src = usable_forest_device(ds, forest);
    DeviceRestore restore_device;
    if (!new_index) {  // the forest's own numbering: the index of ah_index_create, on the forest's blocks
        AH_TRY(index_create_impl(ds, v, src, out));
        if (src) forest_device_consume(forest, true, true);
    } else {
        // the store's numbering: every tree grafted as a new root onto an index of nothing, under the graft's renumbering and checks
        if (!src) AH_TRY(validate_forest_view(ds, v));
        ah_forest_view none{};
        none.normal_stride = v.normal_stride;
        none.normal_vector_offset = v.normal_vector_offset;
        none.normal_header_offset = v.normal_header_offset;
        ah_index *ix = nullptr;
        AH_TRY(index_create_impl(ds, none, nullptr, &ix));
        std::vector<uint32_t> targets(v.n_trees, AH_NEW_ROOT);
        bool adopted_rows = false;
        const int st = graft_impl(ix, v, targets.data(), new_index, nullptr, src, &adopted_rows);
        if (st != AH_OK) {
            (void)ah_index_destroy(ix);
            return st;
        }
        if (src) forest_device_consume(forest, false, adopted_rows);
        *out = ix;
    }
    if (src && out_from_device) *out_from_device = 1;
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_footprint_get(ah_index *ix, ah_index_footprint *out) {
    AH_GUARDED("ah_index_footprint_get")
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    AH_INDEX_LIVE(ix);
    DeviceRestore restore_device;
    return footprint_impl(ix, out);
    AH_GUARDED_END
}

int ah_index_compact(ah_index *ix, uint32_t *out_new_of_old, ah_index_compact_stats *out_stats) {
    AH_GUARDED("ah_index_compact")
    AH_TRY(index_updatable(ix));
    DeviceRestore restore_device;
    return compact_impl(ix, out_new_of_old, out_stats);
    AH_GUARDED_END
}

int ah_index_export_info(const ah_index *ix, ah_index_info *out) {
    AH_GUARDED("ah_index_export_info")
    AH_REQUIRE(ix && ix->ds && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    out->n_nodes = ix->n_nodes;
    out->desc_len = ix->desc_len;
    out->n_trees = ix->n_trees;
    out->n_normals = ix->n_normals;
    out->normal_row_bytes = ix->ds->row_bytes();
    out->normal_header_floats = header_floats(ix->ds->metric);
    out->reserved = 0;
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_export(ah_index *ix, ah_node *nodes, uint32_t *roots, uint32_t *descendants, void *normal_rows, float *normal_headers) {
    AH_GUARDED("ah_index_export")
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    DeviceRestore restore_device;
    ah_dataset *ds = ix->ds;
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    std::vector<DNode> raw(nodes ? ix->n_nodes : 0);
    if (!raw.empty()) AH_HIP(hipMemcpyAsync(raw.data(), ix->d_nodes, raw.size() * sizeof(DNode), hipMemcpyDeviceToHost, s));
    if (roots && ix->n_trees) AH_HIP(hipMemcpyAsync(roots, ix->d_roots, (size_t)ix->n_trees * 4, hipMemcpyDeviceToHost, s));
    if (descendants && ix->desc_len) AH_HIP(hipMemcpyAsync(descendants, ix->d_desc, ix->desc_len * 4, hipMemcpyDeviceToHost, s));
    if (normal_rows && ix->n_normals)
        AH_HIP(hipMemcpyAsync(normal_rows, ix->d_nrows, (size_t)ix->n_normals * ds->row_bytes(), hipMemcpyDeviceToHost, s));
    if (normal_headers && ix->n_normals)
        AH_HIP(hipMemcpyAsync(normal_headers, ix->d_nhdrs, (size_t)ix->n_normals * header_floats(ds->metric) * 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < raw.size(); i++) nodes[i] = to_host_node(raw[i]);
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
    AH_TRY(index_updatable(ix));
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
