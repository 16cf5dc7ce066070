// index_device.h — what search.hip (the searches and the routing of an ah_index), filter.hip (its resident filters),
// index_update.hip (its deletes, inserts, grafts, compaction, export, suspend / resume) and index_audit.hip (its audit) share.  Device side: the node record and the
// id-list -> bitmap kernel.  Host side: the index handle, the two conversions between the ABI's ah_node and the node record,
// and the scaffolding of a maintenance call — IndexCall (device, stream lease, launch span, phase clock), for_spans,
// read_back, and IndexCommit / index_commit, the one place where new arrays are swapped into an index and its normals view
// is derived from them.  The layouts of the calls' workspaces are in index_workspace.h.
#pragma once

#include <chrono>
#include <optional>

#include "common.h"

namespace ah {

struct DNode {
    uint32_t kind;  // AH_NODE_*; bit 8 = has_normal; 0 = a free slot (a node a delete removed: nothing reaches it)
    uint32_t a;     // SPLIT: left            DESCENDANTS: first id (index into the blob)
    uint32_t b;     // SPLIT: right           DESCENDANTS: count
    uint32_t c;     // SPLIT: normal row      DESCENDANTS: unused
};

// The ABI's node -> the device's.  `row`: the normal row a split node with a plane gets (c; the caller counts the rows).  A
// record that is neither kind keeps its kind and nothing else: the views the index calls take hold none (validate_forest_view),
// the audit counts them.
inline DNode to_device_node(const ah_node &nd, uint32_t row) {
    if (nd.kind == AH_NODE_SPLIT) return nd.has_normal ? DNode{nd.kind | 0x100u, nd.left, nd.right, row} : DNode{nd.kind, nd.left, nd.right, 0};
    if (nd.kind == AH_NODE_DESCENDANTS) return DNode{nd.kind, (uint32_t)nd.offset, nd.count, 0};
    return DNode{nd.kind, 0, 0, 0};
}
// ... and back: `offset` of a split node is its normal row, a free slot (kind 0) is all zeros
inline ah_node to_host_node(const DNode &d) {
    ah_node nd{};
    nd.kind = (uint8_t)(d.kind & 0xFFu);
    if (nd.kind == AH_NODE_SPLIT) {
        nd.has_normal = (d.kind & 0x100u) ? 1 : 0;
        nd.left = d.a;
        nd.right = d.b;
        nd.offset = d.c;
    } else if (nd.kind == AH_NODE_DESCENDANTS) {
        nd.offset = d.a;
        nd.count = d.b;
    }
    return nd;
}

// one bit per listed id (ah_filter_create, the candidate list of ah_search_batch, the ids of ah_index_delete_items)
static __global__ void k_filter_bitmap(const uint32_t *__restrict__ ids, uint64_t n, uint32_t *bits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride)
        atomicOr(&bits[ids[g] >> 5], 1u << (ids[g] & 31));
}

}  // namespace ah

// The forest next to its dataset.  It holds ITEM IDS, never row positions: d_desc is a copy of the view's ids, every kernel
// goes from an id to its row through the dataset's current view (row_of_id) at the time of the call, and the normals are
// rows of their own.  That is why an index may outlive an update of its dataset (ah_index_suspend / ah_index_resume).
struct ah_index {
    ah_dataset *ds = nullptr;
    ah::DataView nv{};  // the normals as a row matrix
    ah::DNode *d_nodes = nullptr;
    uint32_t *d_roots = nullptr, *d_desc = nullptr;
    // after a delete: per node, how many nodes below its index are in use, i.e. the index the node has in a view of the
    // forest as it is now — what the coin of ah_route_items at a `normal: None` node is keyed by.  nullptr: no holes yet
    uint32_t *d_rank = nullptr;
    void *d_nrows = nullptr;
    float *d_nhdrs = nullptr;
    // rows d_nrows / d_nhdrs have room for (>= n_normals): ah_index_graft appends into the spare ones and grows geometrically
    uint32_t normals_cap = 0;
    // the index is what ah_index_create_from_view makes of its forest (no free slot, no orphaned or spare normal row, every row
    // in node order): true from its creation and after ah_index_compact, until a delete or a graft
    bool compacted = true;
    uint32_t n_trees = 0, n_nodes = 0, n_normals = 0, max_desc = 0;
    uint32_t n_leaves = 0;  // Descendants nodes (desc_len / n_leaves: the mean leaf, what the small-submission gate estimates with)
    uint64_t desc_len = 0;
    std::mutex stats_mu;       // ah_search_batch may run on any number of threads
    ah_search_stats stats{};
    std::atomic<uint32_t> search8_fails{0};  // sub-batches whose int8 stage left too many survivors ...
    std::atomic<uint32_t> search8_seen{0};   // ... among this many it served (screen8_window_note: windows of 64) ...
    std::atomic<bool> search8_off{false};    // ... eight in one window: the index's tile re-rank starts on the binary16 rows from now on
    bool counted = false;                    // counted in ds->live_indexes (an update of the dataset refuses meanwhile)
    bool suspended = false;                  // ah_index_suspend: not counted, and every call that reads the dataset refuses
    ah_params_stats pstats{};                // under stats_mu: how ah_search_batch_params cut its calls
    ah_filter_stats fstats{};                // under stats_mu; filters_alive is a level (ah_index_destroy refuses above 0)
    // under stats_mu: filters ah_filter_suspend took out of filters_alive (the maintenance calls and ah_index_suspend do not
    // see them; ah_index_destroy refuses above 0, their `ix` would dangle)
    uint64_t filters_suspended = 0;
    ah_exhausted_stats xstats{};             // under stats_mu: queries answered from their filter's kept list (AH_SEARCH_EXHAUSTED)
};

// every entry point that reads the dataset through the index
#define AH_INDEX_LIVE(ix) \
    AH_REQUIRE(!(ix)->suspended, AH_ERR_INVALID_ARGUMENT, "the index is suspended (ah_index_suspend): ah_index_resume it first")

namespace ah {
// ---- the scaffolding of a maintenance call.  IndexCall: the device of the dataset made current, a stream context leased from
// it for the call, and what every call reads off them
struct IndexCall {
    using Clock = std::chrono::steady_clock;
    std::optional<ContextLease> lease;
    bool timing = false;  // AH_TIMING: the phases are timed, and phase_end() waits for the stream
    Clock::time_point t0;

    int begin(ah_dataset *ds) {
        AH_HIP(hipSetDevice(ds->device));
        lease.emplace(ds);
        AH_REQUIRE(lease->c, AH_ERR_DEVICE, "cannot create a HIP stream");
        timing = tun(TUN_TIMING) != 0;
        t0 = Clock::now();
        return AH_OK;
    }
    hipStream_t stream() const { return lease->c->stream; }
    // items a launch of a pass takes at most (AH_LAUNCH_MAX_ITEMS)
    static uint64_t span() { return (uint64_t)std::max<long long>(1, tun(TUN_LAUNCH_MAX_ITEMS)); }
    static Clock::time_point now() { return Clock::now(); }
    Clock::time_point phase_end() const {
        if (timing) (void)hipStreamSynchronize(stream());
        return now();
    }
    static double secs(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double>(y - x).count(); }
};

// fn(lo, hi) for [0, total) in runs of at most `span`
template <class F>
inline void for_spans(uint64_t total, uint64_t span, F &&fn) {
    for (uint64_t lo = 0; lo < total; lo += span) fn(lo, std::min<uint64_t>(total, lo + span));
}

// what the launches queued so far left in `words` 32-bit words on the device, once they are through
inline int read_back(void *host, const void *dev, size_t words, hipStream_t s) {
    AH_HIP(hipGetLastError());
    AH_HIP(hipMemcpyAsync(host, dev, words * 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    return AH_OK;
}

// the normals view of an index from its arrays and counts: after EVERY change of d_nrows / d_nhdrs / n_normals
inline void index_derive_normals_view(ah_index *ix) {
    const bool bq = metric_is_bq(ix->ds->metric);
    ix->nv.rows_f32 = bq ? nullptr : reinterpret_cast<const float *>(ix->d_nrows);
    ix->nv.rows_bq = bq ? reinterpret_cast<const uint64_t *>(ix->d_nrows) : nullptr;
    ix->nv.headers = ix->d_nhdrs;
    ix->nv.n = ix->n_normals;
}

// What a call made of an index: the new arrays (nullptr: that array stays; the normal rows and headers come together, with the
// rows they have room for) and the counts afterwards, which start as the index's own.
struct IndexCommit {
    DevMem *nodes, *roots, *desc, *rank, *nrows, *nhdrs;
    bool drop_rank = false;  // the call has renumbered the nodes: no holes, no ranks
    uint32_t normals_cap, n_trees, n_nodes, n_normals, max_desc, n_leaves;
    uint64_t desc_len;
    bool compacted;
    IndexCommit(const ah_index *ix, DevMem *nodes, DevMem *roots, DevMem *desc, DevMem *rank, DevMem *nrows = nullptr, DevMem *nhdrs = nullptr)
        : nodes(nodes), roots(roots), desc(desc), rank(rank), nrows(nrows), nhdrs(nhdrs), normals_cap(ix->normals_cap), n_trees(ix->n_trees),
          n_nodes(ix->n_nodes), n_normals(ix->n_normals), max_desc(ix->max_desc), n_leaves(ix->n_leaves), desc_len(ix->desc_len),
          compacted(ix->compacted) {}
};
// The commit: nothing here can fail.  The old arrays go into the DevMems the new ones came in, which free them when the call
// returns (dev_free waits for the device).
inline void index_commit(ah_index *ix, const IndexCommit &c) {
    NoFailScope no_fail;
    auto swap_in = [](auto *&mine, DevMem *theirs) {
        if (!theirs) return;
        void *old = mine;
        mine = static_cast<decltype(+mine)>(theirs->p);
        theirs->p = old;
    };
    swap_in(ix->d_nodes, c.nodes);
    swap_in(ix->d_roots, c.roots);
    swap_in(ix->d_desc, c.desc);
    swap_in(ix->d_rank, c.rank);
    swap_in(ix->d_nrows, c.nrows);
    swap_in(ix->d_nhdrs, c.nhdrs);
    DevMem no_rank;
    if (c.drop_rank) swap_in(ix->d_rank, &no_rank);
    ix->normals_cap = c.normals_cap;
    ix->n_trees = c.n_trees;
    ix->n_nodes = c.n_nodes;
    ix->n_normals = c.n_normals;
    ix->max_desc = c.max_desc;
    ix->n_leaves = c.n_leaves;
    ix->desc_len = c.desc_len;
    ix->compacted = c.compacted;
    index_derive_normals_view(ix);
}

// search.hip: the copies of the rows the certified top-k screen of the searches reads, made when an index starts to serve a
// dataset (ah_index_create*, ah_index_resume).  No memory for them = no screen, not an error.
void index_prepare_screens(ah_dataset *ds);
// search.hip: what ah_index_create_from_view and ah_index_graft ask of a view before they touch anything (pointers, record
// geometry, node ranges, every node reachable at most once)
int validate_forest_view(const ah_dataset *ds, const ah_forest_view &v);
// search.hip: k_route_items for n ids (on the device) down every tree of the index, queued on `s`; d_leaf[t * n + i], bit 0 of
// *d_err (zeroed by the caller) when an id is no row of the dataset
int launch_route_items(ah_index *ix, const uint32_t *d_ids, uint64_t n, const uint64_t *d_seeds, uint32_t *d_leaf, uint32_t *d_err,
                       hipStream_t s);
// The device copy of a resident forest (forest.hip, ah_build_forest_resident / ah_build_subtrees_resident): the arrays
// ah_index_create_from_view would make of the forest's own view, on the device the forest was built on.  rows: n_rows rows at
// the dataset's row pitch, row r the r-th split node with a plane in view order; hdrs: header_floats words per row; ids: the
// view's descendants blob.  Every array is a block of dev_malloc of exactly max(1, count) elements.
struct ForestDevice {
    int device = -1, metric = 0;
    uint32_t dims = 0;
    uint32_t *ids = nullptr;
    uint64_t ids_len = 0;
    void *rows = nullptr;
    float *hdrs = nullptr;
    uint32_t n_rows = 0;
    uint64_t bytes = 0;  // what the three blocks were asked for
};
// forest.hip: the device copy of `forest`, nullptr when it has none (an ordinary forest, a released or a consumed one)
const ForestDevice *forest_device(const ah_forest *forest);
// forest.hip: an index call has been served by the device copy: the forest is an ordinary forest from here on.  The blocks
// named adopted now belong to the caller, the others are freed.  Nothing here can fail.
void forest_device_consume(ah_forest *forest, bool adopted_ids, bool adopted_rows);
// search.hip: the index of a view (ah_index_create_from_view); with `src`, the view of the resident forest whose device copy
// it is: nothing is validated, uploaded or unpacked, and on success the index has adopted the blocks of `src`
int index_create_impl(ah_dataset *ds, const ah_forest_view &v, const ForestDevice *src, ah_index **out);
// search.hip: k_unpack_normals, queued on `s`: n records (recs + offsets[r]) -> rows / headers of the normals
int launch_unpack_normals(const ah_dataset *ds, const uint8_t *d_recs, const uint64_t *d_offsets, uint32_t n, uint64_t vec_off,
                          uint64_t hdr_off, void *d_rows, float *d_headers, hipStream_t s);
}  // namespace ah
