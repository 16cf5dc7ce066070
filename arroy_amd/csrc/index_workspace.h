// index_workspace.h — the device workspaces of the maintenance calls of a resident index (index_update.hip, index_audit.hip): one
// block each, carved into arrays of 32-bit words.  A layout is written down ONCE, as the list of (pointer to carve, words) in
// the order the arrays lie in the block; the bytes to allocate, the part the call zeroes and the pointers all come from that
// list.  Plain C++ with no device call, so that tests/index_workspace_check.cpp and tests/index_drop_workspace_check.cpp can put the
// layouts through a sanitizer.
#pragma once

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace ah {

class Workspace {
    struct Seg {
        void *field;  // the address of the T* that gets the segment
        size_t words;
    };
    Seg segs_[16];  // (the longest layout, the graft's, has 15; no heap: the allocation-failure sweeps count host allocations too)
    size_t n_ = 0, words_ = 0, zero_lo_ = 0, zero_hi_ = ~(size_t)0;

  public:
    // the next `words` 32-bit words go to *field (an array of 8-byte elements must start on an even word: the blocks
    // themselves are aligned far beyond that)
    template <class T>
    Workspace &add(T **field, size_t words) {
        assert(n_ < sizeof segs_ / sizeof segs_[0]);
        segs_[n_++] = Seg{static_cast<void *>(field), words};
        words_ += words;
        return *this;
    }
    // the call zeroes from here / up to here only (without either: the whole block)
    void zeroed_from_here() { zero_lo_ = words_; }
    void zeroed_to_here() { zero_hi_ = words_; }
    size_t bytes() const { return words_ * 4; }
    size_t zeroed_bytes() const { return ((zero_hi_ < words_ ? zero_hi_ : words_) - zero_lo_) * 4; }
    // hand every segment its pointer into the block at `base`, which was allocated with `allocated` bytes
    void carve(void *base, size_t allocated) const {
        uint32_t *at = static_cast<uint32_t *>(base);
        for (size_t i = 0; i < n_; i++) {
            std::memcpy(segs_[i].field, &at, sizeof at);  // (every object pointer has the representation of uint32_t *)
            at += segs_[i].words;
        }
        assert((size_t)(at - static_cast<uint32_t *>(base)) * 4 == allocated && "a workspace was carved past its block");
        (void)allocated;
    }
};

// the words an exclusive scan of n counts needs for its tile sums (scan_device.h), one spare
inline size_t scan_tile_words(uint64_t n, uint32_t tile) { return (size_t)((n + tile - 1) / tile + 1); }

// ---- the layouts.  Args: the argument struct of the call's kernels (DeleteArgs, ...), or anything with members of those names.

// ah_index_delete_items: ten arrays per node, all zeroed
template <class Args>
Workspace delete_workspace(Args &a, uint32_t **tile_sums, uint32_t n_nodes, uint32_t scan_tile, size_t ctl_words) {
    const size_t per_node = (size_t)n_nodes + 1;
    Workspace ws;
    for (uint32_t **f : {&a.order, &a.rep, &a.cnt, &a.flags, &a.own, &a.seg, &a.chg, &a.dseg, &a.cursor, &a.merged}) ws.add(f, per_node);
    return ws.add(tile_sums, scan_tile_words(n_nodes, scan_tile)).add(&a.ctl, ctl_words);
}

// ah_index_drop_trees: four arrays per node, zeroed; the dropped roots the host uploads are written whole
template <class Args>
Workspace drop_workspace(Args &a, uint32_t **tile_sums, uint32_t **seed_roots, uint32_t n_nodes, uint32_t n_drop, uint32_t scan_tile,
                         size_t ctl_words) {
    const size_t per_node = (size_t)n_nodes + 1;
    Workspace ws;
    for (uint32_t **f : {&a.order, &a.dropped, &a.len, &a.rpos}) ws.add(f, per_node);
    ws.add(tile_sums, scan_tile_words(n_nodes, scan_tile)).add(&a.ctl, ctl_words).zeroed_to_here();
    return ws.add(seed_roots, n_drop);
}

// ah_index_insert_items: the tree seeds (8 bytes each) first; the ids, the leaf of every pair and `landed` are written whole
template <class Args>
Workspace insert_workspace(Args &a, uint64_t **seeds, uint32_t **tile_sums, uint32_t **ids, uint32_t **leaf, uint32_t n_nodes, uint32_t n_trees,
                           size_t n, uint32_t scan_tile, size_t ctl_words) {
    const size_t per_node = (size_t)n_nodes + 1, pairs = n * n_trees;
    Workspace ws;
    ws.add(seeds, 2 * (size_t)n_trees).zeroed_from_here();
    for (uint32_t **f : {&a.cnt, &a.seg, &a.cursor, &a.chg, &a.fresh, &a.nlen, &a.dlen, &a.touched}) ws.add(f, per_node);
    ws.add(tile_sums, scan_tile_words(n_nodes, scan_tile)).add(&a.ctl, ctl_words).zeroed_to_here();
    return ws.add(ids, n).add(leaf, pairs).add(&a.landed, pairs);
}

// ah_index_graft: what the kernels fill (zeroed), then what the host uploads; the view's nodes are 4 words each
struct GraftSizes {
    uint32_t n_old, n_used, n_view, n_new, n_repl, n_added;
    uint64_t view_desc_len;
};
template <class Node>
struct GraftUploads {
    uint32_t *vfin, *vtgt, *repl, *kinds, *added, *vdesc;
    Node *vnodes;
};
template <class Args, class Node>
Workspace graft_workspace(Args &a, uint32_t **tile_sums, GraftUploads<Node> &u, const GraftSizes &z, uint32_t scan_tile, size_t ctl_words) {
    Workspace ws;
    ws.add(&a.named, (size_t)z.n_new + 1).add(&a.len, (size_t)z.n_new + 1).add(&a.pos_of_rank, z.n_used).add(&a.new_of_old, z.n_old);
    ws.add(&a.replaced, z.n_old).add(&a.fin, z.n_view).add(tile_sums, scan_tile_words(z.n_new, scan_tile)).add(&a.ctl, ctl_words);
    ws.zeroed_to_here();
    ws.add(&u.vfin, z.n_view).add(&u.vtgt, z.n_view).add(&u.repl, z.n_repl).add(&u.kinds, z.n_repl).add(&u.added, z.n_added);
    return ws.add(&u.vdesc, (size_t)z.view_desc_len).add(&u.vnodes, 4 * (size_t)z.n_view);
}

// pass 1 of ah_index_compact, all of ah_index_footprint_get: only ctl is zeroed, by the call itself; `extra`: the node map
template <class Args>
Workspace compact_workspace(Args &a, uint32_t **tile_sums, uint32_t **extra, uint32_t n_nodes, size_t extra_words, uint32_t scan_tile,
                            size_t ctl_words) {
    const size_t per_node = (size_t)n_nodes + 1;
    Workspace ws;
    ws.add(&a.new_index, per_node).add(&a.new_row, per_node).add(tile_sums, scan_tile_words(n_nodes, scan_tile));
    return ws.add(&a.ctl, ctl_words).add(extra, extra_words);
}

// ah_index_audit / ah_forest_view_audit: the report and the per-tree counters (8-byte members: in front), three arrays per node
template <class Args>
Workspace audit_workspace(Args &a, uint32_t n_nodes, uint32_t n_trees, size_t ctl_words, size_t tree_words) {
    Workspace ws;
    ws.add(&a.ctl, ctl_words).add(&a.tree_items, 2 * (size_t)n_trees).add(&a.tree, tree_words * n_trees);
    return ws.add(&a.owner, n_nodes).add(&a.links, n_nodes).add(&a.order, n_nodes);
}

}  // namespace ah
