// filter.h — the host side of a candidate filter that search.hip reads: the handle, the length of every filter of a dataset, the
// cut of an id list at it, the launcher of a pass over the Descendants ids under one bitmap, the kept total and list (filter.hip).
#pragma once

#include <algorithm>

#include "filter_device.h"
// `QueryBuilder::candidates` resident on the device of its index: one block (FilterBlock, filter.hip), immutable after its
// creation.  The bitmap has no bit set at or above len_bits, its padding words included: ah_filter_combine reads them whole.
struct ah_filter {
    ah_index *ix = nullptr;
    uint32_t *d_bits = nullptr, *d_leaf_kept = nullptr;
    uint64_t len_bits = 0, listed = 0, stored = 0;
    std::atomic<uint64_t> device_bytes{0};  // the block, and the kept list's block from the moment it exists
    // ah_filter_suspend: counted in ix->filters_suspended instead of filters_alive.  It keeps its block; only d_bits / len_bits
    // still mean something (d_leaf_kept is of the node array as it was), and only ah_filter_resume_batch reads them
    bool suspended = false;
    // Exhausted filters: kept_total (the sum of d_leaf_kept) and the kept list K(f) (d_list: n_list ascending ids, a block of
    // its own, none while n_list is 0), each made on first request under list_mu and published by its flag (release / acquire):
    // any number of searching threads, one list.  ah_filter_suspend drops both; ah_filter_destroy frees the list.
    std::mutex list_mu;
    std::atomic<bool> total_ready{false}, list_ready{false};
    uint64_t kept_total = 0, n_list = 0, list_bytes = 0;
    uint32_t *d_list = nullptr;
};

namespace ah {

// Largest stored id + 1: the length of every filter of an index over this dataset (0: no rows).
inline uint64_t filter_len_bits(const ah_dataset *ds) {
    if (!ds->n) return 0;
    return (uint64_t)(ds->identity_ids ? (uint32_t)(ds->n - 1) : ds->last_id) + 1;
}
// How many ids of a strictly ascending list lie below len_bits: the others match no stored id and stay behind.
inline size_t filter_list_cut(const uint32_t *sorted_ids, size_t n, uint64_t len_bits) {
    if (!n || !len_bits) return 0;
    return (size_t)(std::upper_bound(sorted_ids, sorted_ids + n, (uint32_t)(len_bits - 1)) - sorted_ids);
}

// One pass over the Descendants ids of `ix` under the bitmap `bits` over [0, len_bits), queued on `s`: `kernel` gets the
// LeafWalk, the number of node slots and `args`.  launch_leaf_kept: the per-node counts of the bitmap into out[0 .. n_nodes).
template <class Kernel, class... Args>
inline void launch_leaf_walk(Kernel kernel, dim3 grid, const ah_index *ix, const uint32_t *bits, uint64_t len_bits, hipStream_t s,
                             Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, LeafWalk{ix->d_nodes, ix->d_desc, bits, len_bits}, ix->n_nodes, args...);
}
inline void launch_leaf_kept(const ah_index *ix, const uint32_t *bits, uint64_t len_bits, uint32_t *out, hipStream_t s) {
    launch_leaf_walk(k_leaf_kept, dim3(1024), ix, bits, len_bits, s, out);
}

// filter.hip: kept_total(f), the sum of the per-node counts, and the kept list K(f) (f->d_list, f->n_list): made on `ctx` the first time
int filter_kept_total(ah_filter *f, Context *ctx, uint64_t &out);
int filter_kept_list(ah_filter *f, Context *ctx);

}  // namespace ah
