// index_device.h — what search.hip (the searches and the routing of an ah_index) and index_update.hip (its deletes, inserts,
// grafts, export, suspend / resume) share: the device node record, the index handle and the id-list -> bitmap kernel.
#pragma once

#include "common.h"

namespace ah {

struct DNode {
    uint32_t kind;  // AH_NODE_*; bit 8 = has_normal; 0 = a free slot (a node a delete removed: nothing reaches it)
    uint32_t a;     // SPLIT: left            DESCENDANTS: first id (index into the blob)
    uint32_t b;     // SPLIT: right           DESCENDANTS: count
    uint32_t c;     // SPLIT: normal row      DESCENDANTS: unused
};

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
    ah_filter_stats fstats{};                // under stats_mu; filters_alive is a level (ah_index_destroy refuses above 0)
};

// every entry point that reads the dataset through the index
#define AH_INDEX_LIVE(ix) \
    AH_REQUIRE(!(ix)->suspended, AH_ERR_INVALID_ARGUMENT, "the index is suspended (ah_index_suspend): ah_index_resume it first")

namespace ah {
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
// search.hip: k_unpack_normals, queued on `s`: n records (recs + offsets[r]) -> rows / headers of the normals
int launch_unpack_normals(const ah_dataset *ds, const uint8_t *d_recs, const uint64_t *d_offsets, uint32_t n, uint64_t vec_off,
                          uint64_t hdr_off, void *d_rows, float *d_headers, hipStream_t s);
}  // namespace ah
