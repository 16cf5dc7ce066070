// search_plan.h — what one sub-batch of ah_search_batch / _filters / _params (search.hip: search_chunk) chooses before the
// first device result comes back, and where its scratch lies.  plan_chunk is one pure function of the sub-batch's shape and
// of the tunables: search_chunk launches exactly what it returns.  The two layouts are walked twice by a Carver
// (rerank_workspace.h): without a block for the bytes, then over the block for the pointers.  Plain C++ with no device call
// and no tunable read, so that tests/search_plan_check.cpp can replay recorded sub-batches on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/arroy_hip.h"  // ah_metric
#include "rerank_workspace.h"         // Carver, pad256

namespace ah {

// Capacities of the search kernels (search.hip) the plan compares against.
constexpr uint32_t kSortLds = 16384;             // candidate ids sorted in LDS per query (64 KiB)
constexpr uint32_t kTileSlab = 128;              // rows per block and unit of more than 8 visits (twice that up to 8): k_leaf_tiles*
constexpr uint32_t kTileSmallSlab = 64;          // rows per block of k_leaf_tiles16 in a small submission (32 octets x 2 rows)
constexpr uint32_t kMultiMaxBlocks = 16, kMultiMaxQueries = 32, kMultiCap = 1024;  // k_descend_multi
constexpr uint32_t kBitmapMaxWords = 39 * 1024;  // 156 KiB of the 160 KiB of LDS: 1 277 952 ids
constexpr uint32_t kLeafScanItems = 2048;        // 256 threads x 8
constexpr uint32_t kSmallVisits = 2048;          // visits one call of k_units_small holds
constexpr uint32_t kHashMaxCandidates = 24576;   // candidates of a query k_flag_duplicates_hash holds
constexpr uint32_t kSelectCap = 1024;            // keys the selections behind the tiles hold
constexpr uint32_t kStatusWords = 16;            // the per-chunk status block (SS_WORDS)

// The tunables (common.h) the sub-batch path reads, filled once per API call (search.hip: search_knobs).
struct SearchKnobs {
    bool bitmap, tiles, screen, screen8, item_list, small_gate, status_wipe, fused_prepare, multi, multi_own_units, flat_tiles,
        single_fused, multi_ids_by_tiles, multi_trace, fused_flag, spin_wait, wave, debug;
    long long small_tiles_max_queries, screen8_min_queries, small_units_max_queries, block_max_queries, multi_trees_per_block,
        multi_max_queries, screen8_max_visits;
};

// One sub-batch as the plan sees it.
struct ChunkShape {
    // the sub-batch
    uint64_t nq, count;
    uint32_t search_k, nns_stride;
    bool by_vector;       // queries given as vectors (by item: rows of the dataset)
    bool filtered;        // under one filter, or mixed
    bool mixed, varied;   // queries under different filters; with counts / search_k of their own
    bool uniform_filter;  // one bitmap for all its queries
    double filter_share;  // the share of the items the filter keeps (mixed: the smallest)
    bool wave_descent, allow8;
    // the index
    uint32_t n_nodes, n_trees, n_leaves;
    uint64_t desc_len;
    uint32_t max_desc;
    // the dataset
    int metric;
    uint32_t dims, pitch, hpitch, pitch8;
    uint64_t row_bytes, n;
    uint32_t max_id;
    // atomics as sampled
    bool screen_ready, screen8_ready, search8_off;
    // the batched re-rank (batch.hip) as asked: candidates per tile, the counters of the row-major re-rank (0: not wanted),
    // whether `count` is within the tournament top-k, and the keys per query of the tournament / of the single-query top-k
    // (the latter filled only when it is not: 0 otherwise)
    uint32_t tile_candidates;
    uint64_t inv_bytes;
    bool batch_count;
    uint64_t kstride_batch, kstride_single;
};

enum class Descent : uint8_t { Octet, WaveBig, WaveSmallBig, Block, Multi };  // of the tile pass; k_descend<false> follows the waves
enum class UnitBuilder : uint8_t { None, Descent, UnitsSmall, LeafScan };     // None: no tile pass
enum class TileLaunch : uint8_t { None, Tiles8And16, Flat, ItemList, Small2D, Big2D, F32 };
enum class Flagger : uint8_t { None, Fused, Bitmap, Hash };                   // nns.dedup() of the tile pass
enum class SortedDedup : uint8_t { Bitmap, SortLds, SortGlobal };             // ... of the sorted path

struct ChunkPlan {
    bool big_k;  // count beyond the batched tournament top-k: the single-query kernels, one query after the other
    uint64_t kstride;
    uint32_t max_tiles_bound, heap_cap;
    uint32_t bitmap_words;
    bool bitmap_fits, hash_fits;
    bool tiles;  // the leaf-tile path
    uint32_t visit_cap, n_leaf_sums;
    bool screened, screened8;
    uint64_t items_cap;  // != 0: the list of (unit, slab) pairs k_units_small leaves for the tile launch
    bool zero_copy_queries, block_ok, small_units, fuse_prepare, small_first;
    // the tile pass (tiles)
    Descent descent = Descent::Octet;
    uint32_t multi_blocks = 0;  // blocks per query of k_descend_multi, when that is the descent
    bool own_units = false;     // every query's descent writes its own units ...
    uint32_t units_per_query = 0;  // ... query q's at [q * units_per_query, ...) (0: one query, or the units of all by leaf)
    bool single_fused = false;  // units and binary16 copies come out of the descent itself (SingleQueryOut)
    bool ids_by_tiles = false;
    UnitBuilder units = UnitBuilder::None;
    bool small_tiles = false;   // k_leaf_tiles16<true> is the tile launch
    TileLaunch tile_launch = TileLaunch::None;
    uint32_t tile_grid_x = 0, tile_grid_y = 0;
    bool fused_flag = false;
    uint64_t sel_lds = 0, fused_lds = 0;
    Flagger flagger = Flagger::None;
    uint32_t max_vis8 = 0;
};

// The descent runs one wave (or block) per query: AH_SEARCH_WAVE, a query leaf of at most 32 KiB (it is kept in LDS), and
// no filter that keeps under 5 % of the items (a query then pops more nodes than the queues of a wave hold).
inline bool wave_descent_wanted(const SearchKnobs &kn, size_t padded_row_bytes, bool filtered, double share) {
    return kn.wave && padded_row_bytes <= (32u << 10) && (!filtered || share >= 0.05);
}

// Step 3 of the sorted path; max_nn: the longest candidate list of the sub-batch (read back only when no bitmap fits).
inline SortedDedup sorted_dedup_kind(bool bitmap_fits, uint32_t max_nn) {
    return bitmap_fits ? SortedDedup::Bitmap : max_nn <= kSortLds ? SortedDedup::SortLds : SortedDedup::SortGlobal;
}

inline ChunkPlan plan_chunk(const ChunkShape &z, const SearchKnobs &kn) {
    ChunkPlan p{};
    const size_t nq = (size_t)z.nq, k = (size_t)z.count;
    p.max_tiles_bound = (uint32_t)(nq * ((size_t)z.nns_stride / z.tile_candidates + 1));
    // count <= 2048: the batched tournament top-k; beyond: the single-query kernels, one query after the other (the
    // reference accepts any count, `Reader::nns(count)`; large counts are rare and not a throughput path)
    p.big_k = !z.batch_count;
    p.kstride = p.big_k ? z.kstride_single : z.kstride_batch;
    p.heap_cap = z.n_nodes + z.n_trees + 2;
    // leaf-tile re-rank (see k_leaf_tiles): which submissions take it, and its scratch
    p.bitmap_words = (uint32_t)(((uint64_t)z.max_id / 32 + 1 + 1023) / 1024 * 1024);
    p.bitmap_fits = kn.bitmap && p.bitmap_words <= kBitmapMaxWords;
    // nns.dedup() of the tiles: the LDS bitmap, or a hash set of the candidates when the id space is too big for it
    p.hash_fits = z.nns_stride <= kHashMaxCandidates && z.max_id != 0xFFFFFFFFu;
    // (never in a mixed sub-batch: the tiles read the kept ids of a leaf from ONE of its visits for all of them, k_leaf_tiles;
    // without them no descent is a last pass, so k_descend_multi and the units of a single query are out as well)
    // (count <= kSelectCap: the selections behind the tiles hold kSelectCap keys and select at least min(count, distinct
    // candidates) of them, so a larger count could only do the whole tile pass, overflow and be redone — after an int8 pass and
    // its binary16 retry where that stage is on, each noted as a failure of the int8 stage in its window of 64 sub-batches.
    // Unless a query cannot have more than kSelectCap candidates at all: a count meant as "everything" under a small search_k)
    p.tiles = !z.mixed && kn.tiles && (p.bitmap_fits || p.hash_fits) && !p.big_k && (k <= kSelectCap || z.nns_stride <= kSelectCap) &&
              z.dims >= 32 && z.max_desc <= 65535u * kTileSlab &&
              (z.metric == AH_EUCLIDEAN || z.metric == AH_COSINE || z.metric == AH_DOT_PRODUCT);
    p.visit_cap = (uint32_t)std::min<uint64_t>((uint64_t)nq * z.nns_stride, 2u << 20);
    p.n_leaf_sums = (z.n_nodes + kLeafScanItems - 1) / kLeafScanItems;
    // certified top-k screen of the tile re-rank: the binary16 shadow of the rows must exist (ah_index_create makes it)
    p.screened = p.tiles && kn.screen && (z.metric == AH_COSINE || z.metric == AH_DOT_PRODUCT) && z.screen_ready;
    // ... and on the int8 copy before that (round 6): the submissions of at least AH_SEARCH_SCREEN8_MIN_QUERIES queries (65: past
    // the small ones' unit builder).  From 9 queries a call the leaf tiles are bound by the bytes of their rows (64 queries: 294 of
    // the call's 508 us) and the int8 rows do cut them to 249 — but the wider band of survivors costs the selection 65 -> 95 us
    // and the queries' digits a launch: 511 us against 502, measured, so the default leaves those calls on binary16; see ScreenSearch
    p.screened8 = p.screened && z.allow8 && kn.screen8 && !z.search8_off &&
                  (long long)nq > std::max(kn.small_tiles_max_queries, kn.screen8_min_queries - 1) && z.screen8_ready;
    // (a few queries a call: the list of (unit, slab) pairs k_units_small leaves for the tile launch)
    p.items_cap = p.tiles && (long long)nq <= kn.small_units_max_queries && kn.item_list
                      ? nq * ((size_t)z.nns_stride / kTileSmallSlab + 1) + kSmallVisits + 1
                      : 0;
    // (a small submission: the kernel that prepares the query leaves reads the pinned staging buffer itself — 6 KB over the link
    // cost less than the copy engine's launch)
    p.zero_copy_queries = z.by_vector && (long long)nq <= kn.small_units_max_queries;
    // The small-submission kernels have hard capacities and, on the leaf-tile path, nothing behind them: k_descend_block holds 32
    // leaves per octet (trees t = octet mod 32), k_units_small kSmallVisits visits per call; past either the whole chunk is
    // redone the long way — correct, and more than twice the latency (round-5 advice: 128-d data at search_k = 10 000 opens
    // ~100 leaves per query, a 3-tree index more than 32 per tree).  So: an estimate of the leaves one query opens — search_k
    // items at the index's mean leaf size (what a filter keeps of it), a quarter more for leaves smaller than the mean — decides
    // on the host whether a call starts there at all (at most 8 estimated leaves per octet, 0.8 x kSmallVisits visits per call).
    // AH_SEARCH_SMALL_GATE=0: as before (the overflow tests force the fall-backs with it).
    bool block_fits = true, small_units_fit = true;
    if (kn.small_gate && z.n_leaves) {
        const double mean_leaf = std::max(1.0, (double)z.desc_len / z.n_leaves * (z.filtered ? std::max(z.filter_share, 1e-3) : 1.0));
        const double est_leaves = 1.25 * (double)z.search_k / mean_leaf + 2.0;
        // (measured, round 6: 64 queries x ~18 estimated leaves per octet overflowed the block kernel — the best-first order does
        // not spread a query's leaves evenly over the trees; the benchmarked shapes sit near 1 per octet)
        block_fits = est_leaves / std::max(1u, std::min(z.n_trees, 32u)) <= 8.0;
        small_units_fit = (double)nq * est_leaves <= 0.8 * kSmallVisits;
    }
    p.block_ok = block_fits && (long long)nq <= kn.block_max_queries;
    // (a small submission on the leaf-tile path makes the binary16 copies of its queries in the launch that places its visits)
    p.small_units = p.tiles && small_units_fit && (long long)nq <= kn.small_units_max_queries;
    // a query pops about 1 / (kept share) as many nodes under a filter: start with the big queues (one query per CU
    // at a time) only then; otherwise they take what the small ones (four per CU) could not hold
    p.small_first = !z.filtered || z.filter_share >= 0.35;
    // (... and when the block descent is the first kernel to want the leaves, it prepares them itself)
    // (small_units: otherwise k_queries_h16 wants the leaves BEFORE the descent — until round 6 a call with the block
    // descent on and k_units_small off screened against copies of unprepared leaves and was saved by the fall-back only)
    p.fuse_prepare = p.zero_copy_queries && p.tiles && p.small_units && z.wave_descent && !(z.metric >= AH_BQ_EUCLIDEAN) && p.small_first &&
                     p.block_ok && kn.fused_prepare;
    if (!p.tiles) return p;

    // ---- the tile pass: descent with its visits recorded, no host round trip before the results
    // a small submission: slabs of 64 rows (a dozen leaves then fill 150 CUs instead of 50) and a grid that does not
    // dispatch 24 000 blocks to find 12 units
    const unsigned tile_slabs = std::max(1u, (z.max_desc + kTileSlab - 1) / kTileSlab);
    const unsigned small_slabs = std::max(1u, (z.max_desc + kTileSmallSlab - 1) / kTileSmallSlab);
    // (never with the int8 stage: that one starts past AH_SEARCH_SMALL_TILES_MAX_QUERIES queries)
    p.small_tiles = p.screened && !p.screened8 && (long long)nq <= kn.small_tiles_max_queries && small_slabs <= 65535u;
    if (!z.wave_descent)
        p.descent = Descent::Octet;
    else if (p.small_first && p.block_ok) {
        // On the leaf-tile path nothing runs behind the block kernel: what it cannot hold (rare: its capacities, equal keys
        // of two octets across the cut) raises bit 4 of *err and the submission is redone the long way, instead of every
        // small call paying two more launches for passes that find nothing to do.
        // A handful of queries, more trees than one wave has octets: the trees of a query dealt over G blocks of one descent wave
        // each (k_descend_multi) — one query on G compute units.  Only as the last pass (what it cannot hold takes the long way).
        const uint32_t per_block = (uint32_t)std::min<long long>(8, std::max<long long>(1, kn.multi_trees_per_block));
        const uint32_t multi_blocks = std::min<uint32_t>(kMultiMaxBlocks, (z.n_trees + per_block - 1) / per_block);
        const bool multi = kn.multi && multi_blocks >= 2 && (long long)nq <= std::min<long long>(kn.multi_max_queries, kMultiMaxQueries);
        p.descent = multi ? Descent::Multi : Descent::Block;
        p.multi_blocks = multi ? multi_blocks : 0;
        // ... and a few queries whose descents write their own units, query by query (the flat tile launch reads them with
        // blockIdx.y = query): no launch that sorts a hundred visits of all queries by leaf.  Queries that open the same leaf
        // read its rows once each.
        const uint32_t units_per_query = (uint32_t)(p.visit_cap / std::max<size_t>(nq, 1));
        p.own_units = multi && nq > 1 && p.small_tiles && units_per_query >= kMultiCap && kn.multi_own_units && kn.flat_tiles;
        // (one query: its units and its binary16 copy come out of the descent itself, see SingleQueryOut)
        p.single_fused = (nq == 1 || p.own_units) && p.small_units && kn.single_fused;
        if (p.single_fused) {
            p.units_per_query = nq == 1 ? 0u : units_per_query;
            p.ids_by_tiles = p.small_tiles && !z.uniform_filter && kn.multi_ids_by_tiles;
        }
    } else
        p.descent = p.small_first ? Descent::WaveSmallBig : Descent::WaveBig;
    p.units = p.single_fused ? UnitBuilder::Descent : p.small_units ? UnitBuilder::UnitsSmall : UnitBuilder::LeafScan;
    const bool items_made = p.units == UnitBuilder::UnitsSmall && p.items_cap != 0;
    if (p.screened8) {
        // the leaves few queries reached on the int8 copy (a quarter of the f32 bytes, a wider band of survivors), the leaves
        // many queries share on the binary16 copy as before; the selection takes every candidate's bound from its own stage
        p.tile_launch = TileLaunch::Tiles8And16, p.tile_grid_x = 2048, p.tile_grid_y = tile_slabs;
        p.max_vis8 = (uint32_t)std::max<long long>(1, kn.screen8_max_visits);
    } else if (!p.screened) {
        p.tile_launch = TileLaunch::F32, p.tile_grid_x = 2048, p.tile_grid_y = tile_slabs;
    } else if (p.small_tiles && p.single_fused && (nq == 1 || p.units_per_query) && p.visit_cap >= 128u && kn.flat_tiles) {
        // (queries whose units came out of their descent: a flat list of (leaf, slab) items, see the kernel)
        p.tile_launch = TileLaunch::Flat, p.tile_grid_x = z.nns_stride / kTileSmallSlab + 129u, p.tile_grid_y = (unsigned)nq;
    } else if (p.small_tiles && items_made) {  // one block per listed (unit, slab) pair (grid.y = 1: an overflowed list is walked)
        p.tile_launch = TileLaunch::ItemList, p.tile_grid_x = (unsigned)std::min<size_t>(p.items_cap, 2048), p.tile_grid_y = 1;
    } else if (p.small_tiles) {
        p.tile_launch = TileLaunch::Small2D, p.tile_grid_x = std::min<unsigned>(2048u, 32u * (unsigned)nq), p.tile_grid_y = small_slabs;
    } else {  // the candidates on the binary16 copies first: half the bytes (see k_search_select_screened)
        p.tile_launch = TileLaunch::Big2D, p.tile_grid_x = 2048, p.tile_grid_y = tile_slabs;
    }
    // a small submission: nns.dedup() inside the selection kernel (FLAG), when the bitmap fits beside its other LDS
    p.sel_lds = (size_t)z.pitch * 4;  // the query leaf in f32
    p.fused_lds = p.sel_lds + (size_t)p.bitmap_words * 4;
    p.fused_flag = p.small_units && p.screened && p.bitmap_fits && z.nns_stride <= 16384 && p.fused_lds + (26u << 10) <= (160u << 10) &&
                   kn.fused_flag;
    p.flagger = p.fused_flag ? Flagger::Fused : p.bitmap_fits ? Flagger::Bitmap : Flagger::Hash;
    return p;
}

// ---- the scratch of one sub-batch ----------------------------------------------------------------------------------------
// Bufs: SearchBufs (search.hip), or anything with members of those names and element sizes.  The order is the order in the
// block.  Two copies rely on it: d_oi, d_od, d_err, d_unique lie back to back, and so do their pinned mirrors h_oi, h_od,
// h_err, h_counts — the tile path reads all four back with ONE copy (a call of one query is a dozen launches and copies of
// ~5 us each); d_sks, d_cnt (and h_sks, h_cnt) lie back to back and are uploaded with one.
// What lies beyond the last array (kSearchDeviceSlack, kSearchPinnedSlack) is the sums' slack of 4096 bytes as they were
// before the layouts were written down once; the pinned sum never counted h_err, whose 256 bytes came out of that slack.
constexpr size_t kSearchDeviceSlack = 4096, kSearchPinnedSlack = 4096 - 256;

template <class Bufs>
void search_device_layout(Carver &c, const ChunkShape &z, const ChunkPlan &p, Bufs &b) {
    const size_t nq = (size_t)z.nq, k = (size_t)z.count, total = nq * (size_t)z.nns_stride;
    c.take(&b.d_qf32, nq * z.dims);
    c.take(&b.d_qrows, nq);
    c.take(&b.d_qvecs, nq * pad256(z.row_bytes));
    c.take(&b.d_qhdrs, nq * 2);
    c.take(&b.d_nns, total);
    c.take(&b.d_dist, total);
    c.take(&b.d_counts, nq);
    c.take(&b.d_overflow, nq);
    c.take(&b.d_list, nq);
    c.take(&b.d_segs, nq);
    c.take(&b.d_tiles, p.max_tiles_bound);
    c.take(&b.d_ka, nq * p.kstride);
    c.take(&b.d_kb, nq * p.kstride);
    c.take(&b.d_oi, nq * k);
    c.take(&b.d_od, nq * k);
    c.take(&b.d_err, kStatusWords);  // [error bits][SearchStatSlot counters]
    c.take(&b.d_unique, nq);
    c.take(&b.d_inv, z.inv_bytes / 4, z.inv_bytes != 0);
    c.take(&b.d_visits, p.visit_cap, p.tiles);
    c.take(&b.d_sorted, p.visit_cap, p.tiles);
    c.take(&b.d_units, p.visit_cap, p.tiles);
    c.take(&b.d_leaf_count, (size_t)z.n_nodes + 2, p.tiles);  // + the number of visits, + the number of units
    c.take(&b.d_cursor, z.n_nodes, p.tiles);
    c.take(&b.d_ustart, z.n_nodes, p.tiles);
    c.take(&b.d_leaf_sums, p.n_leaf_sums, p.tiles);
    c.take(&b.d_items, p.items_cap, p.tiles && p.items_cap != 0);
    c.take(&b.d_unit_counts, nq, p.tiles);
    c.take(&b.d_aux, total, p.screened && z.metric == AH_COSINE);
    c.take(&b.d_q16, nq * z.hpitch, p.screened);
    c.take(&b.d_qstats, nq, p.screened);
    c.take(&b.d_q8, nq * (size_t)z.pitch8 * 2, p.screened8);
    c.take(&b.d_q8stats, nq, p.screened8);
    c.take(&b.d_aux8, total, p.screened8);
    c.take(&b.d_slots, nq, z.mixed);
    c.take(&b.d_sks, nq, z.varied);
    c.take(&b.d_cnt, nq, z.varied);
    // (reserved and not handed out, as the sum always did: one more word per query with the tile arrays, and the norms'
    // array of a screened sub-batch of another metric than Cosine)
    if (p.tiles) c.take<uint32_t>(nq);
    if (p.screened && z.metric != AH_COSINE) c.take<float>(total);
}

// the pinned mirrors: what the host writes for the uploads, then what it reads back
template <class Bufs>
void search_pinned_layout(Carver &c, const ChunkShape &z, const ChunkPlan &p, Bufs &b) {
    const size_t nq = (size_t)z.nq, k = (size_t)z.count;
    c.take(&b.h_q, nq * z.dims);
    c.take(&b.h_qrows, nq);
    c.take(&b.h_overflow, nq);
    c.take(&b.h_list, nq);
    c.take(&b.h_segs, nq);
    c.take(&b.h_tiles, p.max_tiles_bound);
    c.take(&b.h_oi, nq * k);
    c.take(&b.h_od, nq * k);
    c.take(&b.h_err, kStatusWords);
    c.take(&b.h_counts, nq);
    c.take(&b.h_slots, nq, z.mixed);
    c.take(&b.h_sks, nq, z.varied);
    c.take(&b.h_cnt, nq, z.varied);
}

}  // namespace ah
