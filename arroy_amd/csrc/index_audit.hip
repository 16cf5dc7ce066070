// index_audit.hip — ah_index_audit / ah_forest_view_audit (include/arroy_hip.h): `Reader::assert_validity`
// (src/reader.rs:509-589) and `Reader::stats` (src/reader.rs:210-252) where the forest lives.  The kernels work on raw
// arrays (DNode *, roots, ids, DataView), so the audit of a resident index and the audit of a view the host holds (uploaded
// into scratch, never made an ah_index) are the same code.  The classes are defined in the header and in DESIGN.md 4,
// "Audit of a resident index"; every count is a property of the arrays, not of the order the launches ran in.
//
// Shape of an audit; every pass reads the index and writes scratch only:
//   1. walk      level-synchronous from the roots, one launch per level.  A node is CLAIMED by a compare-and-swap on its owner
//                word (tree position + 1); only the claimer appends it to the frontier, so a node is expanded once whatever
//                links to it.  Every valid link also counts in links[node]: LINKED_TWICE = links followed - nodes reached.
//   2. nodes     one pass over the node slots: in use, floating, linked twice (first), bad normal rows and list ranges, and the
//                per-tree stats, one atomic per wave and tree.
//   3. lists     a wave per reached Descendants node, 64 ids a step: ascending, row_of_id, one atomicOr on the ROW's bit of the
//                owning tree's coverage words (a set old bit is a duplicate).  The trees are audited in groups whose coverage
//                words fit AH_AUDIT_COVER_MB; a group's pass skips the leaves other groups own.
//   4. compare   per group, over its coverage words: popc(~word) = missing, the smallest missing (tree, id) by a 64-bit min.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "index_device.h"
#include "index_workspace.h"

using namespace ah;

namespace {

constexpr unsigned kAuBlock = 256;  // 4 waves
constexpr uint32_t kNone = 0xFFFFFFFFu;

// the report as the kernels fill it.  [first_node .. first_dup] starts as all ones, the rest as zeros.
struct AuditCtl {
    unsigned long long count[AH_AUDIT_CLASSES];
    unsigned long long links, in_use;
    uint32_t tail, pad;
    uint32_t first_node[AH_AUDIT_CLASSES];
    unsigned long long first_missing, first_dup;  // tree position << 32 | id
};

struct TreeWords {  // per tree, zeroed
    uint32_t depth, split_nodes, dummy_normals, descendants;
};

struct AuditArgs {
    const DNode *nodes;
    uint32_t n_nodes;
    const uint32_t *roots;
    uint32_t n_trees;
    const uint32_t *desc;
    uint64_t desc_len;
    uint32_t n_normals;
    // scratch, zeroed before the first kernel
    uint32_t *owner;  // per node: 1 + the position in roots[] of the tree that claimed it (0: not reached)
    uint32_t *links;  // per node: valid root entries and valid child links of reached split nodes that name it
    uint32_t *order;  // the claimed nodes, level by level
    TreeWords *tree;
    unsigned long long *tree_items;
    AuditCtl *ctl;
};

__device__ __forceinline__ bool kind_valid(uint32_t kind) {
    const uint32_t k = kind & 0xFFu;
    return k == AH_NODE_DESCENDANTS || k == AH_NODE_SPLIT;
}

// lanes of `mask` below this one
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// one atomic per wave: the lanes of `mask` are offenders of class `cls`, my_node the node (BAD_ROOT: the position) of this lane
__device__ __forceinline__ void note_class(AuditCtl *ctl, int cls, uint64_t mask, uint32_t lane, uint32_t my_node) {
    if (mask == 0) return;
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
    if (lane == first) {
        atomicAdd(&ctl->count[cls], (unsigned long long)__popcll(mask));
        atomicMin(&ctl->first_node[cls], my_node);  // (lanes hold ascending nodes / positions: the first lane has the smallest)
    }
}

// Claims `node` for tree word `own` and appends the claimed ones of this wave behind the tail with one atomic.  Every lane of
// the wave calls it (want = false: nothing to claim).  A node is appended only by the lane whose compare-and-swap found its
// owner word 0, so at most once in the whole audit: the frontier never holds more than n_nodes entries.
__device__ __forceinline__ void claim_and_append(const AuditArgs &a, bool want, uint32_t node, uint32_t own, uint32_t lane) {
    bool won = false;
    if (want) {
        atomicAdd(&a.links[node], 1u);
        won = atomicCAS(&a.owner[node], 0u, own) == 0u;
    }
    const uint64_t m = __ballot(won);
    if (m == 0) return;
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(&a.ctl->tail, (uint32_t)__popcll(m));
    base = __shfl(base, (int)first);
    const uint32_t pos = base + lanes_below(m, lane);
    if (won && pos < a.n_nodes) a.order[pos] = node;  // (pos < n_nodes by the argument above; checked all the same)
}

// walk, level 1: the valid entries of roots[]
__global__ __launch_bounds__(kAuBlock) void k_audit_seed(AuditArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); t0 < a.n_trees; t0 += stride) {  // (wave-uniform)
        const uint32_t t = t0 + lane;
        const bool active = t < a.n_trees;
        const uint32_t r = active ? a.roots[t] : 0u;
        const bool ok = active && r < a.n_nodes && kind_valid(a.nodes[r].kind);
        note_class(a.ctl, AH_AUDIT_BAD_ROOT, __ballot(active && !ok), lane, t);
        const uint64_t mok = __ballot(ok);
        if (mok && lane == (uint32_t)__ffsll((unsigned long long)mok) - 1u) atomicAdd(&a.ctl->links, (unsigned long long)__popcll(mok));
        claim_and_append(a, ok, r, t + 1u, lane);
    }
}

// walk, level `depth` (the roots are level 1): order[begin, end) are the nodes claimed at this level; the children its split
// nodes claim are appended behind the tail.
//
// Termination.  A node enters the frontier only through claim_and_append, at most once; so the frontier holds at most n_nodes
// entries over the whole walk.  Every launch covers a non-empty level [begin, end), and the host follows it with another only
// when the tail moved, i.e. when the level appended at least one entry: the loop ends at the first empty level and is bounded
// by n_nodes levels.  A cycle, a shared sub-tree or a root that is also a child costs a link count and a failed
// compare-and-swap, never a second expansion; a child that is out of range, free or of an unknown kind costs a counter and is
// never used as an index.
__global__ __launch_bounds__(kAuBlock) void k_audit_level(AuditArgs a, uint32_t begin, uint32_t end, uint32_t depth) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = begin + blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < end; i0 += stride) {  // (wave-uniform)
        const uint32_t i = i0 + lane;
        const bool active = i < end;
        uint32_t node = 0, own = 0;
        DNode nd{};
        if (active) {
            node = a.order[i];  // (< n_nodes: only range-checked nodes are claimed)
            nd = a.nodes[node];
            own = a.owner[node];
        }
        // the depth of every tree with a node on this level: one atomicMax per wave and tree
        uint64_t todo = __ballot(active);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t lo = __shfl(own, leader);
            if ((int)lane == leader && lo >= 1u && lo <= a.n_trees) atomicMax(&a.tree[lo - 1u].depth, depth);
            todo &= ~__ballot(active && own == lo);
        }
        const bool split = active && (nd.kind & 0xFFu) == AH_NODE_SPLIT;
        const bool ok_l = split && nd.a < a.n_nodes && kind_valid(a.nodes[nd.a].kind);
        const bool ok_r = split && nd.b < a.n_nodes && kind_valid(a.nodes[nd.b].kind);
        const uint64_t bad_l = __ballot(split && !ok_l), bad_r = __ballot(split && !ok_r);
        if (bad_l | bad_r) {
            const uint32_t first = (uint32_t)__ffsll((unsigned long long)(bad_l | bad_r)) - 1u;
            if (lane == first) atomicAdd(&a.ctl->count[AH_AUDIT_BAD_LINK], (unsigned long long)(__popcll(bad_l) + __popcll(bad_r)));
            if (split && (!ok_l || !ok_r)) atomicMin(&a.ctl->first_node[AH_AUDIT_BAD_LINK], node);  // (frontier order: not ascending)
        }
        const uint64_t m_l = __ballot(ok_l), m_r = __ballot(ok_r);
        if ((m_l | m_r) && lane == (uint32_t)__ffsll((unsigned long long)(m_l | m_r)) - 1u)
            atomicAdd(&a.ctl->links, (unsigned long long)(__popcll(m_l) + __popcll(m_r)));
        claim_and_append(a, ok_l, nd.a, own, lane);
        claim_and_append(a, ok_r, nd.b, own, lane);
    }
}

// nodes: every slot once.  What the walk left in owner / links decides the structure classes that are properties of a node,
// and the per-tree stats are summed per wave and tree (node order keeps a tree's nodes together: mostly one tree a wave).
__global__ __launch_bounds__(kAuBlock) void k_audit_nodes(AuditArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < a.n_nodes; i0 += stride) {  // (wave-uniform)
        const uint32_t i = i0 + lane;
        const bool active = i < a.n_nodes;
        DNode nd{};
        uint32_t own = 0, links = 0;
        if (active) {
            nd = a.nodes[i];
            own = a.owner[i];
            links = a.links[i];
        }
        const bool in_use = active && kind_valid(nd.kind);
        const bool reached = in_use && own >= 1u && own <= a.n_trees;
        const bool split = reached && (nd.kind & 0xFFu) == AH_NODE_SPLIT;
        const bool leaf = reached && (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS;
        const bool has_normal = (nd.kind & 0x100u) != 0;
        const bool bad_list = leaf && (uint64_t)nd.a + nd.b > a.desc_len;
        const uint64_t m_use = __ballot(in_use);
        if (m_use && lane == (uint32_t)__ffsll((unsigned long long)m_use) - 1u) atomicAdd(&a.ctl->in_use, (unsigned long long)__popcll(m_use));
        note_class(a.ctl, AH_AUDIT_FLOATING, __ballot(in_use && !reached), lane, i);
        note_class(a.ctl, AH_AUDIT_BAD_NORMAL, __ballot(split && has_normal && nd.c >= a.n_normals), lane, i);
        note_class(a.ctl, AH_AUDIT_BAD_LIST, __ballot(bad_list), lane, i);
        {
            const uint64_t m_twice = __ballot(active && links > 1u);  // (counted as links followed - nodes reached: the first only)
            if (m_twice && lane == (uint32_t)__ffsll((unsigned long long)m_twice) - 1u) atomicMin(&a.ctl->first_node[AH_AUDIT_LINKED_TWICE], i);
        }
        uint64_t todo = __ballot(reached);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t lo = __shfl(own, leader);
            const bool mine = reached && own == lo;
            const uint32_t n_split = (uint32_t)__popcll(__ballot(mine && split));
            const uint32_t n_dummy = (uint32_t)__popcll(__ballot(mine && split && !has_normal));
            const uint32_t n_leaf = (uint32_t)__popcll(__ballot(mine && leaf));
            unsigned long long items = (mine && leaf && !bad_list) ? nd.b : 0ull;
            for (int off = 32; off > 0; off >>= 1) items += __shfl_down(items, off);
            if (lane == 0) {
                TreeWords *tw = &a.tree[lo - 1u];
                if (n_split) atomicAdd(&tw->split_nodes, n_split);
                if (n_dummy) atomicAdd(&tw->dummy_normals, n_dummy);
                if (n_leaf) atomicAdd(&tw->descendants, n_leaf);
                if (items) atomicAdd(&a.tree_items[lo - 1u], items);
            }
            todo &= ~__ballot(mine);
        }
    }
}

// lists: the reached Descendants nodes of the trees [tree_lo, tree_hi) among the node slots [lo, hi), a wave each.  cover holds
// `words` words per tree of the group, zeroed: bit r of tree t's words = "row r occurs in tree t".
__global__ __launch_bounds__(kAuBlock) void k_audit_lists(AuditArgs a, DataView dv, uint32_t lo, uint32_t hi, uint32_t tree_lo, uint32_t tree_hi,
                                                          uint32_t *__restrict__ cover, uint64_t words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t n_unsorted = 0, first_unsorted = kNone, first_foreign = kNone;
    unsigned long long n_foreign = 0, n_dup = 0, first_dup = ~0ull;
    for (uint32_t node = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); node < hi; node += n_waves) {  // (wave-uniform)
        const uint32_t own = a.owner[node];
        if (own <= tree_lo || own > tree_hi) continue;  // not reached, or a tree of another group
        const DNode nd = a.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS || (uint64_t)nd.a + nd.b > a.desc_len) continue;  // (BAD_LIST: its ids are not read)
        const uint32_t t = own - 1u;
        uint32_t *tree_cover = cover + (uint64_t)(t - tree_lo) * words;
        bool unsorted = false, foreign_here = false;
        uint32_t carry = 0;  // the last id of the step before
        for (uint32_t j0 = 0; j0 < nd.b; j0 += 64) {
            const bool live = j0 + lane < nd.b;
            const uint32_t id = live ? a.desc[(uint64_t)nd.a + j0 + lane] : 0u;
            uint32_t prev = __shfl_up(id, 1);
            if (lane == 0) prev = carry;
            carry = __shfl(id, 63);
            const bool inverted = live && (j0 + lane) > 0u && prev >= id;
            uint64_t row = ~0ull;
            if (live) row = row_of_id(dv, id);
            const bool stored = live && row < dv.n;
            bool dup = false;
            if (stored) {
                const uint32_t bit = 1u << (row & 31u);
                dup = (atomicOr(&tree_cover[row >> 5], bit) & bit) != 0u;
            }
            const uint64_t m_foreign = __ballot(live && !stored), m_dup = __ballot(dup);
            unsorted |= __ballot(inverted) != 0ull;
            foreign_here |= m_foreign != 0ull;
            n_foreign += (unsigned long long)__popcll(m_foreign);
            n_dup += (unsigned long long)__popcll(m_dup);
            if (dup) first_dup = min(first_dup, ((unsigned long long)t << 32) | id);
        }
        if (unsorted) {
            n_unsorted++;
            first_unsorted = min(first_unsorted, node);
        }
        if (foreign_here) first_foreign = min(first_foreign, node);
    }
    // one atomic per wave and counter (the counters above are wave-uniform, first_dup is per lane)
    for (int off = 32; off > 0; off >>= 1) first_dup = min(first_dup, (unsigned long long)__shfl_down(first_dup, off));
    if (lane == 0) {
        if (first_dup != ~0ull) atomicMin(&a.ctl->first_dup, first_dup);
        if (n_unsorted) {
            atomicAdd(&a.ctl->count[AH_AUDIT_UNSORTED], (unsigned long long)n_unsorted);
            atomicMin(&a.ctl->first_node[AH_AUDIT_UNSORTED], first_unsorted);
        }
        if (n_foreign) {
            atomicAdd(&a.ctl->count[AH_AUDIT_FOREIGN], n_foreign);
            atomicMin(&a.ctl->first_node[AH_AUDIT_FOREIGN], first_foreign);
        }
        if (n_dup) atomicAdd(&a.ctl->count[AH_AUDIT_DUPLICATE], n_dup);
    }
}

// compare: the coverage words of the trees [tree_lo, tree_lo + n_group): a clear bit below n_items is a (tree, item) pair the
// tree does not hold.  ids ascend with rows (DataView::ids), so the smallest missing row of a tree is its smallest missing id.
__global__ __launch_bounds__(kAuBlock) void k_audit_compare(AuditCtl *ctl, DataView dv, const uint32_t *__restrict__ cover, uint64_t words,
                                                            uint32_t tree_lo, uint32_t n_group) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t total = words * n_group, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t tail_bits = (uint32_t)(dv.n & 31u);
    unsigned long long missing = 0, first = ~0ull;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const uint64_t t = w / words, wi = w - t * words;
        const uint32_t valid = (wi == words - 1 && tail_bits) ? (1u << tail_bits) - 1u : 0xFFFFFFFFu;
        const uint32_t miss = ~cover[w] & valid;
        if (miss == 0u) continue;
        missing += (unsigned long long)__popc(miss);
        const uint64_t row = wi * 32u + (uint32_t)(__ffs((int)miss) - 1);  // (< n_items by the mask)
        const uint32_t id = dv.identity_ids ? (uint32_t)row : dv.ids[row];
        first = min(first, ((unsigned long long)(tree_lo + t) << 32) | id);
    }
    for (int off = 32; off > 0; off >>= 1) {
        missing += __shfl_down(missing, off);
        first = min(first, (unsigned long long)__shfl_down(first, off));
    }
    if (lane == 0 && missing) {
        atomicAdd(&ctl->count[AH_AUDIT_MISSING], missing);
        atomicMin(&ctl->first_missing, first);
    }
}

int alloc(DevMem *m, size_t bytes) { return ah::alloc(m, bytes, "the index audit"); }

// the forest to audit; on the device unless the up_* pointers say where the host holds it (a view: uploaded into scratch)
struct AuditIn {
    const DNode *nodes = nullptr;
    const uint32_t *roots = nullptr, *desc = nullptr;
    const DNode *up_nodes = nullptr;
    const uint32_t *up_roots = nullptr, *up_desc = nullptr;
    uint32_t n_nodes = 0, n_trees = 0, n_normals = 0;
    uint64_t desc_len = 0;
};

int audit_run(ah_dataset *ds, const AuditIn &in, ah_index_audit_report *out, ah_tree_stats *out_trees) {
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    const DataView dv = ds->view();
    const uint32_t nn = in.n_nodes, n_trees = in.n_trees;
    // the tree groups: as many trees' coverage words as fit the budget
    const uint64_t words = (dv.n + 31) / 32;
    const uint64_t budget = (uint64_t)std::max<long long>(0, tun(TUN_AUDIT_COVER_MB)) << 20;
    uint32_t group = n_trees;
    if (words) group = (uint32_t)std::min<uint64_t>(n_trees, std::max<uint64_t>(1, budget / (words * 4)));
    // every block the audit needs, before the first launch or copy
    AuditArgs a{};
    const Workspace ws = audit_workspace(a, nn, n_trees, sizeof(AuditCtl) / 4, sizeof(TreeWords) / 4);
    DevMem work, cover, up_nodes, up_roots, up_desc;
    AH_TRY(alloc(&work, ws.bytes()));
    ws.carve(work.p, ws.bytes());
    AH_TRY(alloc(&cover, (size_t)(words * group) * 4));
    if (in.up_nodes) AH_TRY(alloc(&up_nodes, (size_t)nn * sizeof(DNode)));
    if (in.up_roots) AH_TRY(alloc(&up_roots, (size_t)n_trees * 4));
    if (in.up_desc) AH_TRY(alloc(&up_desc, (size_t)in.desc_len * 4));
    std::vector<TreeWords> tree_words(n_trees);
    std::vector<unsigned long long> tree_items(n_trees);
    std::vector<uint32_t> roots(n_trees);
    a.nodes = in.up_nodes ? up_nodes.as<const DNode>() : in.nodes;
    a.roots = in.up_roots ? up_roots.as<const uint32_t>() : in.roots;
    a.desc = in.up_desc ? up_desc.as<const uint32_t>() : in.desc;
    a.n_nodes = nn;
    a.n_trees = n_trees;
    a.desc_len = in.desc_len;
    a.n_normals = in.n_normals;
    if (in.up_nodes && nn) AH_HIP(hipMemcpyAsync(up_nodes.p, in.up_nodes, (size_t)nn * sizeof(DNode), hipMemcpyHostToDevice, s));
    if (in.up_roots && n_trees) AH_HIP(hipMemcpyAsync(up_roots.p, in.up_roots, (size_t)n_trees * 4, hipMemcpyHostToDevice, s));
    if (in.up_desc && in.desc_len) AH_HIP(hipMemcpyAsync(up_desc.p, in.up_desc, (size_t)in.desc_len * 4, hipMemcpyHostToDevice, s));
    AH_HIP(hipMemsetAsync(work.p, 0, ws.zeroed_bytes(), s));
    AH_HIP(hipMemsetAsync(&a.ctl->first_node[0], 0xFF, sizeof(AuditCtl) - offsetof(AuditCtl, first_node), s));
    // 1. walk
    AuditCtl ctl{};
    uint32_t begin = 0, end = 0;
    if (n_trees) {
        hipLaunchKernelGGL(k_audit_seed, dim3(grid_of(n_trees, kAuBlock, 1024)), dim3(kAuBlock), 0, s, a);
        AH_TRY(read_back(&end, &a.ctl->tail, 1, s));
        AH_REQUIRE(end <= nn, AH_ERR_DEVICE, "the audit's walk claimed more nodes than the forest has");
    }
    for (uint32_t depth = 1; begin < end; depth++) {
        hipLaunchKernelGGL(k_audit_level, dim3(grid_of(end - begin, kAuBlock, 4096)), dim3(kAuBlock), 0, s, a, begin, end, depth);
        uint32_t tail = 0;
        AH_TRY(read_back(&tail, &a.ctl->tail, 1, s));
        AH_REQUIRE(tail >= end && tail <= nn, AH_ERR_DEVICE, "the audit's walk claimed more nodes than the forest has");
        begin = end;
        end = tail;
    }
    // 2. nodes
    if (nn) hipLaunchKernelGGL(k_audit_nodes, dim3(grid_of(nn, kAuBlock, 4096)), dim3(kAuBlock), 0, s, a);
    AH_HIP(hipGetLastError());
    // 3. lists and 4. compare, tree group by tree group
    for (uint32_t t0 = 0; t0 < n_trees; t0 += group) {
        const uint32_t n_group = std::min(group, n_trees - t0);
        if (words) AH_HIP(hipMemsetAsync(cover.p, 0, (size_t)(words * n_group) * 4, s));
        for_spans(nn, call.span(), [&](uint64_t lo, uint64_t hi) {
            hipLaunchKernelGGL(k_audit_lists, dim3(grid_of(hi - lo, kAuBlock / 64, 1u << 16)), dim3(kAuBlock), 0, s, a, dv, (uint32_t)lo, (uint32_t)hi,
                               t0, t0 + n_group, cover.as<uint32_t>(), words);
        });
        if (words)
            hipLaunchKernelGGL(k_audit_compare, dim3(grid_of(words * n_group, kAuBlock, 4096)), dim3(kAuBlock), 0, s, a.ctl, dv,
                               cover.as<const uint32_t>(), words, t0, n_group);
        AH_HIP(hipGetLastError());
    }
    AH_HIP(hipMemcpyAsync(&ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    if (n_trees) {
        AH_HIP(hipMemcpyAsync(tree_items.data(), a.tree_items, (size_t)n_trees * 8, hipMemcpyDeviceToHost, s));
        AH_HIP(hipMemcpyAsync(tree_words.data(), a.tree, (size_t)n_trees * sizeof(TreeWords), hipMemcpyDeviceToHost, s));
        if (in.up_roots) std::copy(in.up_roots, in.up_roots + n_trees, roots.begin());
        else AH_HIP(hipMemcpyAsync(roots.data(), in.roots, (size_t)n_trees * 4, hipMemcpyDeviceToHost, s));
    }
    AH_HIP(hipStreamSynchronize(s));
    AH_REQUIRE(ctl.tail == end && ctl.links >= ctl.tail, AH_ERR_DEVICE, "the audit's walk lost count of the nodes it reached");
    // the report: nothing fails from here on
    ah_index_audit_report r{};
    r.n_items = dv.n;
    r.n_trees = n_trees;
    r.nodes_in_use = ctl.in_use;
    r.nodes_reached = ctl.tail;
    ctl.count[AH_AUDIT_LINKED_TWICE] = ctl.links - ctl.tail;
    bool valid = true;
    for (int c = 0; c < AH_AUDIT_CLASSES; c++) {
        r.count[c] = ctl.count[c];
        r.first_node[c] = ctl.first_node[c];
        valid = valid && ctl.count[c] == 0;
    }
    r.first_missing_tree = r.first_missing_id = r.first_duplicate_tree = r.first_duplicate_id = kNone;
    if (ctl.count[AH_AUDIT_MISSING]) {  // first_node of the coverage classes: the root of the first pair's tree
        r.first_missing_tree = (uint32_t)(ctl.first_missing >> 32);
        r.first_missing_id = (uint32_t)ctl.first_missing;
        if (r.first_missing_tree < n_trees) r.first_node[AH_AUDIT_MISSING] = roots[r.first_missing_tree];
    }
    if (ctl.count[AH_AUDIT_DUPLICATE]) {
        r.first_duplicate_tree = (uint32_t)(ctl.first_dup >> 32);
        r.first_duplicate_id = (uint32_t)ctl.first_dup;
        if (r.first_duplicate_tree < n_trees) r.first_node[AH_AUDIT_DUPLICATE] = roots[r.first_duplicate_tree];
    }
    r.valid = valid ? 1 : 0;
    *out = r;
    if (out_trees)
        for (uint32_t t = 0; t < n_trees; t++) {
            ah_tree_stats ts{};
            ts.root = roots[t];
            ts.depth = tree_words[t].depth;
            ts.split_nodes = tree_words[t].split_nodes;
            ts.dummy_normals = tree_words[t].dummy_normals;
            ts.descendants = tree_words[t].descendants;
            ts.items = tree_items[t];
            out_trees[t] = ts;
        }
    return AH_OK;
}

}  // namespace

extern "C" {

int ah_index_audit(ah_index *ix, ah_index_audit_report *out, ah_tree_stats *out_trees) {
    AH_GUARDED("ah_index_audit")
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    DeviceRestore restore_device;
    AuditIn in;
    in.nodes = ix->d_nodes;
    in.roots = ix->d_roots;
    in.desc = ix->d_desc;
    in.n_nodes = ix->n_nodes;
    in.n_trees = ix->n_trees;
    in.n_normals = ix->n_normals;
    in.desc_len = ix->desc_len;
    return audit_run(ix->ds, in, out, out_trees);
    AH_GUARDED_END
}

int ah_forest_view_audit(ah_dataset *ds, const ah_forest_view *view, ah_index_audit_report *out, ah_tree_stats *out_trees) {
    AH_GUARDED("ah_forest_view_audit")
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    AH_REQUIRE(view, AH_ERR_INVALID_ARGUMENT, "view is NULL");
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    AH_REQUIRE(ds->finalized, AH_ERR_NOT_FINALIZED, "dataset not finalized");
    const ah_forest_view v = *view;
    AH_REQUIRE(v.n_nodes == 0 || v.nodes, AH_ERR_INVALID_ARGUMENT, "nodes is NULL");
    AH_REQUIRE(v.n_trees == 0 || v.roots, AH_ERR_INVALID_ARGUMENT, "roots is NULL");
    AH_REQUIRE(v.descendants_len == 0 || v.descendants, AH_ERR_INVALID_ARGUMENT, "descendants is NULL");
    AH_REQUIRE(v.descendants_len < 0xFFFFFFFFull && v.n_nodes < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
               "forest too large for 32-bit node / descendant offsets");
    bool any_normal = false;
    for (uint64_t i = 0; i < v.n_nodes && !any_normal; i++) any_normal = v.nodes[i].kind == AH_NODE_SPLIT && v.nodes[i].has_normal;
    if (any_normal) {
        const uint64_t hs = ah_header_size(ds->metric), vs = ah_vector_size(ds->metric, ds->dims);
        AH_REQUIRE(v.normals, AH_ERR_INVALID_ARGUMENT, "normals is NULL");
        AH_REQUIRE(v.normal_vector_offset + vs <= v.normal_stride && v.normal_header_offset + hs <= v.normal_stride, AH_ERR_INVALID_ARGUMENT,
                   "normal vector / header do not fit the record stride %llu", (unsigned long long)v.normal_stride);
        AH_REQUIRE((v.normal_vector_offset & 3) == 0 && (v.normal_header_offset & 3) == 0, AH_ERR_INVALID_ARGUMENT,
                   "normal vector / header offsets must be multiples of 4");
    }
    // the nodes as ah_index_create_from_view would store them; what it refuses is marked so that the kernels count it: a
    // normal record out of the blob or misaligned gets row 0xFFFFFFFF (>= n_normals), a list range beyond the blob starts at
    // 0xFFFFFFFF (beyond every blob of < 2^32 - 1 ids).  The normals themselves are not read.
    std::vector<DNode> nodes(v.n_nodes);
    uint32_t n_normals = 0;
    for (uint64_t i = 0; i < v.n_nodes; i++) {
        const ah_node &nd = v.nodes[i];
        DNode d = to_device_node(nd, n_normals);
        if (d.kind & 0x100u) {
            if ((nd.offset & 3) == 0 && nd.offset <= v.normals_len && v.normal_stride <= v.normals_len - nd.offset) n_normals++;
            else d.c = kNone;
        } else if (nd.kind == AH_NODE_DESCENDANTS && !(nd.offset <= v.descendants_len && nd.count <= v.descendants_len - nd.offset)) {
            d.a = kNone;
        }
        nodes[i] = d;
    }
    DeviceRestore restore_device;
    AuditIn in;
    in.up_nodes = nodes.data();
    in.up_roots = v.roots;
    in.up_desc = v.descendants;
    in.n_nodes = (uint32_t)v.n_nodes;
    in.n_trees = v.n_trees;
    in.n_normals = n_normals;
    in.desc_len = v.descendants_len;
    // (the copies are queued from pageable memory: hipMemcpyAsync returns once they are staged, and audit_run waits for the
    // stream before it returns)
    return audit_run(ds, in, out, out_trees);
    AH_GUARDED_END
}

}  // extern "C"
