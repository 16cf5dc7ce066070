// forest_records.h — the host side of one batch of the forest build (BatchBuild in forest.hip): the PODs host and kernels
// share, the sizes of a batch's buffers (batch_sizes: the build and ah_dataset_reserve_build read the same struct), the
// records of the batch's tree nodes with the digest of a level's node table, the leaves' merge and the post-order node list,
// the FIFO ring of node tables still to be digested, and the tree cuts of the grouped tail.  Plain C++ with no device call
// and no tunable read, so that tests/forest_records_check.cpp can drive every branch on the host — the ones a build only
// reaches at 10M rows included.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/arroy_hip.h"
#include "../../include/arroy_hip_policy.h"  // ah_node_key_root
#include "host_parallel.h"

namespace ah {

static constexpr uint32_t kTile = 2048;  // items per tile = 32 octets x 64 items

enum { ST_PENDING = 0, ST_ACCEPTED = 1, ST_RANDOM = 2 };

struct FNode {
    uint64_t key;      // ah_node_key_* of this node
    uint64_t start;    // first position inside the batch permutation (absolute: tree base + offset)
    uint32_t tree;     // tree index inside the batch
    uint32_t count;    // items under the node
    uint32_t n_left;   // accumulated by the margin kernel (integer atomics)
    uint32_t attempt;  // current / final split attempt (0..3)
    uint32_t state;    // ST_*
    uint32_t tile_begin, n_tiles;
    uint32_t fix;      // the parent's sides were re-drawn after its row-major pass (retry / random fallback): the rows of
                       // this node cannot take their node index from k_forest_advance_node_of
};
// What the host needs to know about a level before it can launch it (written by the k_next_* kernels, read back
// through pinned memory): sizes, the cost model's inputs, and the first node of every tree (nodes are ordered by tree).
struct LevelInfo {
    uint32_t n_nodes, n_tiles, n_fix, pad;
    unsigned long long pairs;  // items under the level's nodes = margin evaluations of a first attempt
    unsigned long long pad2;
    // followed by uint32_t tree_first[n_trees + 1]
};
struct FTile {
    uint32_t node;
    uint32_t first;  // offset of the tile inside its node
};
struct NormalStats8 {
    float an, bn, cn, extra;    // |n~'|, |n' - n~'|, |n'| (in the column-scaled space), bias
    float scale, cn0, pad0, pad1;  // s_n; |n| in the original space (for the reference's own rounding error)
};
struct NextCounts {
    uint32_t kids, tiles;
};

struct HostRec {  // one tree node, in creation (breadth-first) order
    uint8_t kind, has_normal;
    uint32_t tree;
    uint32_t left = 0, right = 0;  // HostRec indices
    uint64_t start;
    uint32_t count;
    uint32_t depth;
    uint64_t normal_off = 0;  // byte offset of the normal record inside the forest's normals buffer
};
struct LeafRec {  // a Descendants node of a streaming build: its ids are final_perm[start, start + count)
    uint64_t start;
    uint32_t count, id, tree, depth;
};

// Row pitches of the screen's copies (binary16: whole 128-byte lines of halves; int8: whole 128-byte steps) and the strides
// of a normal's shadow records next to them: [vector][header / NormalStats8], whole lines (see normal_record_stride).
inline uint32_t screen_hpitch(uint32_t dims) { return (dims + 63u) & ~63u; }
inline uint32_t screen_pitch8(uint32_t dims) { return (dims + 127u) & ~127u; }
inline uint64_t shadow_stride16(uint32_t hpitch) { return ((uint64_t)hpitch * 2 + 16 + 127) & ~(uint64_t)127; }
inline uint64_t shadow_stride8(uint32_t pitch8) { return (2 * (uint64_t)pitch8 + sizeof(NormalStats8) + 127) & ~(uint64_t)127; }

// ---- the sizes of one batch ------------------------------------------------------------------------------------------
// Upper bounds known up front (every split node owns > split_after items), so nothing is reallocated between levels:
// nodes per level <= M / (split_after + 1) + n_trees, tiles <= items / kTile + nodes.  Element counts unless named bytes.
struct BatchSizes {
    uint64_t max_nodes, max_tiles;
    uint64_t perm;                                // each of the three permutations
    uint64_t nodes, tiles, masks, tile_left;      // node tables, tile table, side masks, tile_left / tile_left_off
    uint64_t child, block_sums;                   // d_child, d_block_sums (NextCounts)
    uint64_t node_of, side_bytes, side_bits;      // row-major buffers (0: not wanted)
    uint64_t arena_block, shadow_block, shadow8_block;  // bytes of one block of the normals / binary16 / int8 arenas
    // small device block: [abort flag, 3 pad][ScreenCounters][LevelInfo + tree_first[n_trees + 1]]
    size_t info_words;
    // pinned host memory: [2 x LevelInfo block][one word for the abort flag][tree_first staging][2 x node table][bounce]
    size_t pin_info, pin_nodes, pin_head, bounce;
    size_t pinned_bytes() const { return pin_head + 2 * pin_nodes + bounce; }
};
// N rows, M entries of the batch permutation (n_trees * N unless the trees are sub-trees); nstride / hstride / stride8: bytes
// of a normal record, of its binary16 and of its int8 shadow (0: no such screen)
inline BatchSizes batch_sizes(uint64_t N, uint32_t n_trees, uint64_t M, uint32_t split_after, uint64_t nstride, uint64_t hstride,
                              uint64_t stride8, bool want_rows, bool want_side_bits, long long readback_mb) {
    BatchSizes z{};
    z.max_nodes = M / ((uint64_t)split_after + 1) + n_trees;
    z.max_tiles = M / kTile + n_trees + z.max_nodes;
    z.perm = M;
    z.nodes = z.max_nodes;
    z.tiles = z.max_tiles;
    z.masks = z.max_tiles * 32;
    z.tile_left = z.max_tiles;
    z.child = 2 * z.max_nodes;
    z.block_sums = z.max_nodes / 256 + 2;
    if (want_rows) {
        z.node_of = (uint64_t)n_trees * N + 4;
        // padded to whole 1 KiB windows: k_forest_exact_pairs scans it 16 bytes per lane for marks
        z.side_bytes = (uint64_t)n_trees * N + 1024 + 16;
        if (want_side_bits) z.side_bits = ((uint64_t)n_trees * N + 31) / 32 + 4;
    }
    z.arena_block = std::max<uint64_t>(32ull << 20, std::min<uint64_t>(2 * z.max_nodes * nstride, 16ull << 30));
    z.shadow_block = std::max<uint64_t>(16ull << 20, std::min<uint64_t>(z.max_nodes * std::max<uint64_t>(hstride, 16), 8ull << 30));
    z.shadow8_block = std::max<uint64_t>(16ull << 20, std::min<uint64_t>(z.max_nodes * std::max<uint64_t>(stride8, 16), 4ull << 30));
    z.info_words = (sizeof(LevelInfo) + ((size_t)n_trees + 1) * 4 + 3) / 4;
    z.pin_info = (z.info_words * 4 + 255) & ~(size_t)255;
    z.pin_nodes = (z.max_nodes * sizeof(FNode) + 4095) & ~(size_t)4095;
    z.pin_head = (3 * z.pin_info + 256 + 4095) & ~(size_t)4095;
    // pinned double buffer of the read-back worker (a streaming build hands a sink at most one half at a time)
    z.bounce = (size_t)std::min<long long>(4096, std::max<long long>(2, readback_mb)) << 20;
    return z;
}

// ---- the grouped tail's cuts -----------------------------------------------------------------------------------------
// Tree range of group g: [cut[g], cut[g + 1]), K = min(groups, n_trees) groups of at least one tree.  Shrinking groups:
// group g + 1 computes while group g's ids and normals travel (~0.76 of the time its kernels took at PCIe rate), and only
// the last group's are left after the last launch — so the last one is the smallest.  ratio_percent is clamped to 10..100.
inline std::vector<uint32_t> tail_group_trees(uint32_t n_trees, uint32_t groups, long long ratio_percent) {
    const uint32_t K = std::min(groups, n_trees);
    std::vector<uint32_t> cut(K + 1, 0);
    const double ratio = (double)std::min<long long>(100, std::max<long long>(10, ratio_percent)) / 100.0;
    double total_w = 0.0, w = 1.0, cum = 0.0;
    for (uint32_t g = 0; g < K; g++, w *= ratio) total_w += w;
    w = 1.0;
    for (uint32_t g = 1; g < K; g++, w *= ratio) {
        cum += w;
        const uint32_t at = (uint32_t)std::llround((double)n_trees * cum / total_w);
        cut[g] = std::min(std::max(at, cut[g - 1] + 1), n_trees - (K - g));  // at least one tree each
    }
    cut[K] = n_trees;
    return cut;
}

// ---- node tables still to be digested --------------------------------------------------------------------------------
// Node tables that arrived on the side stream and are still to be digested, oldest first.  A table is digested under a
// level that runs long enough to cover it (~45 ns per node on four threads against ~0.15 ns per pair on the device): the
// table of the last big level — 819 000 nodes, 35 ms — used to be digested under the 9 ms remnant level after it, and
// the loop, the hand-over of the ids and the next group of trees waited for it.  The tables live in a ring over the two
// pinned table buffers; a table that finds no room there forces the oldest digests first.
struct PendingTable {
    uint32_t depth, step, n_nodes;
    size_t ring_off;
    uint64_t host_off;
    const uint8_t *chunk_dev;
    int64_t rec_off;      // >= 0: its record indices are level_rec_full[off ...] (first level of a tree group)
    bool fork_parent;     // it is the level the groups were cut from: its children's list is kept whole
    int group_done;       // >= 0: the last level of that tree group — its node list (its leaves' job) can follow
};
struct TableRing {  // FIFO ring; head == tail only when nothing is live
    std::deque<PendingTable> tables;
    size_t cap = 0, head = 0;
    bool alloc(size_t bytes, size_t *off) {  // false: no room (nothing changed)
        const size_t tail = tables.empty() ? 0 : tables.front().ring_off;
        if (tables.empty() || head > tail) {
            const size_t from = tables.empty() ? 0 : head;
            if (from + bytes <= cap) {
                *off = from;
                head = from + bytes;
                return true;
            }
            if (!tables.empty() && bytes < tail) {
                *off = 0;
                head = bytes;
                return true;
            }
            return false;
        }
        if (head + bytes < tail) {
            *off = head;
            head += bytes;
            return true;
        }
        return false;
    }
};

// ---- the records of a batch ------------------------------------------------------------------------------------------
struct DigestResult {  // what one table added to the build's statistics; bad: the smallest node left pending or over-counted
    uint64_t evals = 0, retries = 0, dummies = 0, routed = 0;
    uint32_t bad = 0xFFFFFFFFu;
};

struct BatchRecords {
    uint32_t n_trees = 0, first_tree = 0, split_after = 0;
    bool streaming = false;  // the Descendants nodes are collected per level, ids are id_base + record index
    uint32_t id_base = 0;
    uint64_t nstride = 0;    // bytes of a normal record
    std::vector<HostRec> recs;
    std::vector<uint32_t> new_index;  // (emit_range's: record -> forest-local node index)
    // records in use; the vector itself is grown AHEAD of the digest (value-initialising 80 MB of fresh pages on the thread
    // that digests the deepest level was most of that digest's 35 ms)
    size_t n_recs = 0;
    std::vector<uint32_t> tree_root;
    std::vector<uint64_t> tree_count;  // nodes of every tree so far: its root, then two per digested split
    std::vector<uint32_t> level_rec, next_rec;  // HostRec index of every node of the level being digested / of the next
    std::vector<uint32_t> level_rec_full;       // the grouped tail: the whole list of the level the groups were cut from
    // streaming build: the Descendants nodes, one list per level of creation (each ascending in (tree, position))
    std::vector<std::vector<LeafRec>> stream_leaves;
    uint64_t items_routed = 0;
    size_t node_base = 0, emit_cursor = 0;  // forest node index of the batch's first node / of the next tree to be emitted
    uint32_t emit_tree = 0;                 // trees [0, emit_tree) are emitted
    uint64_t n_split = 0, n_desc = 0;

    void init(uint32_t trees, uint32_t first, uint32_t split, bool stream, uint32_t ids_from, uint64_t stride, size_t nodes_so_far) {
        n_trees = trees, first_tree = first, split_after = split, streaming = stream, id_base = ids_from, nstride = stride;
        tree_root.assign(n_trees, 0);
        tree_count.assign(n_trees, 1);
        node_base = emit_cursor = nodes_so_far;
    }
    // (room for every node of a balanced forest — leaves of split_after / 2 .. split_after items, as many split nodes — so that
    // the vector never moves: at 10M x 100 trees the 1.7 M + 1.7 M records outgrew the former 4 / 3 x max_nodes at the last big
    // level, and copying 136 MB of records held the launching thread for 38 ms with the device idle; untouched pages cost nothing)
    void reserve(uint64_t max_nodes) {
        try {
            recs.reserve(4 * max_nodes + n_trees + 16);
        } catch (const std::bad_alloc &) {  // (a tiny split_after on a huge dataset: grow as needed, as before)
            recs.reserve(4 * max_nodes / 3 + 16);
        }
    }
    // room for the records of the digests to come: `level_nodes` of the level just launched, and every pending table's
    void grow_ahead(uint32_t level_nodes, const std::deque<PendingTable> &pending) {
        size_t want = n_recs + 2 * (size_t)level_nodes;
        for (const PendingTable &e : pending) want += 2 * (size_t)e.n_nodes;
        if (recs.size() < want) recs.resize(want);
    }

    // Level 0 on the host: a record per tree; the trees that do not fit a Descendants node get a node of the first table
    // `lv` (tiles, key), `info` its sizes, tree_first[t] its index.  tree_base: n_trees + 1 offsets into the permutation.
    void seed_roots(const uint64_t *tree_base, const uint64_t *tree_seeds, FNode *lv, LevelInfo *info, uint32_t *tree_first) {
        if (streaming) stream_leaves.emplace_back();
        for (uint32_t t = 0; t < n_trees; t++) {
            const uint32_t cnt = (uint32_t)(tree_base[t + 1] - tree_base[t]);
            HostRec r{};
            r.tree = t;
            r.start = tree_base[t];
            r.count = cnt;
            r.depth = 0;
            tree_root[t] = (uint32_t)n_recs;
            if (cnt <= split_after) {  // fit_in_descendant at the root: the tree is one Descendants node
                r.kind = AH_NODE_DESCENDANTS;
                if (streaming) stream_leaves[0].push_back(LeafRec{r.start, cnt, id_base + (uint32_t)n_recs, first_tree + t, 0u});
                recs.push_back(r);
                n_recs++;
                continue;
            }
            r.kind = AH_NODE_SPLIT;
            FNode nd{};
            nd.key = ah_node_key_root(tree_seeds[t]);
            nd.start = tree_base[t];
            nd.tree = t;
            nd.count = cnt;
            nd.tile_begin = info->n_tiles;
            nd.n_tiles = (cnt + kTile - 1) / kTile;
            tree_first[t] = info->n_nodes;
            level_rec.push_back((uint32_t)n_recs);
            recs.push_back(r);
            n_recs++;
            lv[info->n_nodes++] = nd;
            info->n_tiles += nd.n_tiles;
            info->pairs += cnt;
        }
    }

    // (a streaming build also writes the level's 48-byte stream nodes and collects its leaves: twice the threads)
    unsigned digest_threads(uint32_t n_nodes, unsigned host_threads) const {
        return n_nodes >= 65536 ? std::min(streaming ? 8u : 4u, host_threads) : 1u;
    }
    // encoded stream: the children's ids are written into the values, so they must not wrap
    bool stream_ids_wrap(uint32_t n_nodes) const { return (uint64_t)id_base + n_recs + 2 * (uint64_t)n_nodes > 0xFFFFFFFFull; }

    // Digest the node table of a finished level: split records, children, statistics, and which HostRec every node of the
    // next level belongs to — the same walk the device did in k_next_emit.  `rec_of`: HostRec index of every node of the
    // table (level_rec of the level-by-level loop; a slice of level_rec_full for the first level of a tree group).
    // stream_nodes (streaming build): n_nodes entries, record i <-> node i.  With a bad node nothing but recs is changed.
    DigestResult digest_level(uint32_t depth, uint32_t n_nodes, const FNode *tbl, uint64_t chunk_host_off, const uint32_t *rec_of,
                              unsigned n_threads, ah_stream_node *stream_nodes) {
        // Children get the records base + 2 i (left) and base + 2 i + 1 (right) of node i, so the walk splits over a few
        // threads (the deepest level of the 10M x 100-tree build has 819 000 nodes: 37 ms on one thread, more than the GPU
        // needs for the level after it); the list of children that split again is concatenated in node order afterwards.
        const size_t base = n_recs;
        if (recs.size() < base + 2 * (size_t)n_nodes) recs.resize(base + 2 * (size_t)n_nodes);
        n_recs = base + 2 * (size_t)n_nodes;
        struct Part {
            DigestResult r;
            std::vector<uint32_t> splits;
            std::vector<LeafRec> leaves;  // streaming build: the children that are Descendants nodes, in node order
            std::vector<std::pair<uint32_t, uint32_t>> runs;  // (tree, nodes of it in this part): the table is ordered by tree
        };
        std::vector<Part> parts(n_threads);
        parallel_run(n_threads, [&](unsigned t) {
            Part &pt = parts[t];
            const uint32_t lo = (uint32_t)((uint64_t)n_nodes * t / n_threads), hi = (uint32_t)((uint64_t)n_nodes * (t + 1) / n_threads);
            pt.splits.reserve(2 * (size_t)(hi - lo));
            if (streaming) pt.leaves.reserve(2 * (size_t)(hi - lo));
            for (uint32_t i = lo; i < hi; i++) {
                const FNode nd = tbl[i];
                if (nd.state == ST_PENDING || nd.n_left > nd.count) {
                    pt.r.bad = std::min(pt.r.bad, i);
                    continue;
                }
                if (pt.runs.empty() || pt.runs.back().first != nd.tree) pt.runs.push_back({nd.tree, 0u});
                pt.runs.back().second++;
                pt.r.evals += (uint64_t)(nd.attempt + 1) * nd.count;
                pt.r.retries += nd.attempt;
                pt.r.routed += nd.count;
                const uint32_t rec_idx = rec_of[i];
                recs[rec_idx].has_normal = nd.state == ST_ACCEPTED;
                recs[rec_idx].normal_off = chunk_host_off + (uint64_t)i * nstride;
                if (nd.state != ST_ACCEPTED) pt.r.dummies++;
                const uint32_t child_cnt[2] = {nd.n_left, nd.count - nd.n_left};
                const uint64_t child_start[2] = {nd.start, nd.start + nd.n_left};
                for (uint32_t side = 0; side < 2; side++) {
                    HostRec c{};
                    c.tree = nd.tree;
                    c.start = child_start[side];
                    c.count = child_cnt[side];
                    c.depth = depth + 1;
                    const uint32_t cidx = (uint32_t)(base + 2 * (size_t)i + side);
                    if (c.count <= split_after) {
                        c.kind = AH_NODE_DESCENDANTS;
                        if (streaming) pt.leaves.push_back(LeafRec{c.start, c.count, id_base + cidx, first_tree + nd.tree, depth + 1});
                    } else {
                        c.kind = AH_NODE_SPLIT;
                        pt.splits.push_back(cidx);
                    }
                    recs[cidx] = c;
                    if (side == 0) recs[rec_idx].left = cidx;
                    else recs[rec_idx].right = cidx;
                }
                if (stream_nodes) {
                    ah_stream_node sn{};
                    sn.id = id_base + rec_idx;
                    sn.tree = first_tree + nd.tree;
                    sn.kind = AH_NODE_SPLIT;
                    sn.has_normal = nd.state == ST_ACCEPTED;
                    sn.left = id_base + (uint32_t)(base + 2 * (size_t)i);
                    sn.right = sn.left + 1;
                    sn.count = nd.count;
                    sn.depth = depth;
                    sn.payload_offset = (uint64_t)i * nstride;
                    stream_nodes[i] = sn;
                }
            }
        });
        DigestResult sum;
        for (const Part &pt : parts) sum.bad = std::min(sum.bad, pt.r.bad);
        if (sum.bad != 0xFFFFFFFFu) return sum;
        if (streaming) {
            stream_leaves.emplace_back();
            for (Part &pt : parts) stream_leaves.back().insert(stream_leaves.back().end(), pt.leaves.begin(), pt.leaves.end());
        }
        next_rec.clear();
        for (const Part &pt : parts) {
            sum.evals += pt.r.evals;
            sum.retries += pt.r.retries;
            sum.dummies += pt.r.dummies;
            sum.routed += pt.r.routed;
            next_rec.insert(next_rec.end(), pt.splits.begin(), pt.splits.end());
            for (const auto &run : pt.runs) tree_count[run.first] += 2ull * run.second;
        }
        items_routed += sum.routed;
        level_rec.swap(next_rec);
        return sum;
    }

    // Streaming build: the Descendants nodes of trees [tA, tB), ascending in (tree, position) — i.e. in the order their ids lie
    // in the final permutation.  Every level's list is already in that order; the levels of one tree are merged per tree
    // (a few threads: 1.7 M leaves at 10M x 100 trees).  `out`: resize(n) and data() of ah_stream_node.
    template <class List>
    void leaves_of(uint32_t tA, uint32_t tB, unsigned host_threads, List &out) const {
        // per tree: where its leaves start in every level's list, and in the output
        const size_t n_lv = stream_leaves.size();
        const uint32_t nt = tB - tA;
        std::vector<size_t> cut((size_t)(nt + 1) * n_lv, 0), out_at(nt + 1, 0);
        for (size_t l = 0; l < n_lv; l++) {
            const auto &lv = stream_leaves[l];
            // (by tree, not by position: an EMPTY child at the very end of a tree starts where the next tree does)
            for (uint32_t t = 0; t <= nt; t++)
                cut[(size_t)t * n_lv + l] = (size_t)(std::lower_bound(lv.begin(), lv.end(), first_tree + tA + t, [](const LeafRec &r, uint32_t v) { return r.tree < v; }) - lv.begin());
        }
        for (uint32_t t = 0; t < nt; t++) {
            size_t c = 0;
            for (size_t l = 0; l < n_lv; l++) c += cut[(size_t)(t + 1) * n_lv + l] - cut[(size_t)t * n_lv + l];
            out_at[t + 1] = out_at[t] + c;
        }
        const size_t total = out_at[nt];
        out.resize(total);
        ah_stream_node *const out_nodes = out.data();
        std::atomic<uint32_t> next_tree{0};
        parallel_run(total < 100000 ? 1u : std::min(nt, host_threads), [&](unsigned) {
            std::vector<LeafRec> mine;
            for (;;) {
                const uint32_t t = next_tree.fetch_add(1, std::memory_order_relaxed);
                if (t >= nt) break;
                mine.clear();
                for (size_t l = 0; l < n_lv; l++)
                    mine.insert(mine.end(), stream_leaves[l].begin() + (ptrdiff_t)cut[(size_t)t * n_lv + l],
                                stream_leaves[l].begin() + (ptrdiff_t)cut[(size_t)(t + 1) * n_lv + l]);
                // (an empty leaf shares its position with its sibling: it goes first, so that offsets never step back)
                std::sort(mine.begin(), mine.end(), [](const LeafRec &a, const LeafRec &b) {
                    return a.start != b.start ? a.start < b.start : a.count < b.count;
                });
                ah_stream_node *dst = out_nodes + out_at[t];
                for (const LeafRec &r : mine) {
                    ah_stream_node sn{};
                    sn.id = r.id;
                    sn.tree = r.tree;
                    sn.kind = AH_NODE_DESCENDANTS;
                    sn.count = r.count;
                    sn.depth = r.depth;
                    sn.payload_offset = r.start * 4;
                    *dst++ = sn;
                }
            }
        });
    }

    // Emit trees [tA, tB) in post-order (children before parents: the order TmpNodes::put receives them,
    // src/writer.rs:1235-1258), with forest-local indices.  Trees are independent: the number of nodes of every tree
    // is known (counted while the levels were digested), so each tree is written into its own slice by a few threads —
    // all trees after the last level, or, when the tail runs in groups, a group's trees under the next group's kernels.
    // roots: the batch's start at roots_base.  false: tA is not the next tree to be emitted (nothing changed).
    bool emit_range(uint32_t tA, uint32_t tB, unsigned host_threads, std::vector<ah_node> &nodes, std::vector<uint32_t> &roots,
                    size_t roots_base, uint64_t desc_base) {
        if (tB <= tA) return true;
        if (tA != emit_tree) return false;
        std::vector<uint64_t> off(tB - tA + 1, 0);
        for (uint32_t t = tA; t < tB; t++) off[t - tA + 1] = off[t - tA] + tree_count[t];
        const uint64_t total = off[tB - tA];
        nodes.resize(emit_cursor + total);
        if (roots.size() < roots_base + n_trees) roots.resize(roots_base + n_trees);
        new_index.resize(n_recs, 0xFFFFFFFFu);
        uint32_t *roots_out = roots.data() + roots_base;
        std::atomic<uint32_t> next_tree{tA};
        std::atomic<uint64_t> all_splits{0}, all_descs{0};
        parallel_run(total < 200000 ? 1u : std::min({tB - tA, host_threads, std::max(1u, std::thread::hardware_concurrency())}),
                     [&](unsigned) {
            std::vector<std::pair<uint32_t, int>> stack;
            uint64_t splits = 0, descs = 0;
            for (;;) {
                const uint32_t t = next_tree.fetch_add(1, std::memory_order_relaxed);
                if (t >= tB) break;
                uint64_t out = emit_cursor + off[t - tA];
                stack.clear();
                stack.push_back({tree_root[t], 0});
                while (!stack.empty()) {
                    const uint32_t ri = stack.back().first;
                    const HostRec &r = recs[ri];
                    if (r.kind == AH_NODE_SPLIT && stack.back().second == 0) {
                        stack.back().second = 1;
                        const uint32_t l = r.left, rr = r.right;
                        stack.push_back({rr, 0});
                        stack.push_back({l, 0});
                        continue;
                    }
                    ah_node nd{};
                    nd.kind = r.kind;
                    nd.has_normal = r.has_normal;
                    nd.tree = first_tree + t;
                    nd.count = r.count;
                    nd.depth = r.depth;
                    if (r.kind == AH_NODE_SPLIT) {
                        nd.left = new_index[r.left];
                        nd.right = new_index[r.right];
                        nd.offset = r.normal_off;
                        splits++;
                    } else {
                        nd.offset = desc_base + r.start;
                        descs++;
                    }
                    new_index[ri] = (uint32_t)out;
                    nodes[out++] = nd;
                    stack.pop_back();
                }
                roots_out[t] = new_index[tree_root[t]];
            }
            all_splits.fetch_add(splits, std::memory_order_relaxed);
            all_descs.fetch_add(descs, std::memory_order_relaxed);
        });
        n_split += all_splits.load();
        n_desc += all_descs.load();
        emit_cursor += total;
        emit_tree = tB;
        return true;
    }
    // a streaming build has no node list: the counts of its records
    void count_records() {
        recs.resize(n_recs);
        for (const HostRec &r : recs) (r.kind == AH_NODE_SPLIT ? n_split : n_desc)++;
    }
};

}  // namespace ah
