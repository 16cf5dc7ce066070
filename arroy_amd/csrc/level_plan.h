// level_plan.h — how one level of the forest build runs its first margin pass (BatchBuild in forest.hip): node-major,
// row-major with TC trees per group, row-major with a group's normals resident in LDS, or the dense MFMA product; the
// row-major launches the level is cut into; and whether the level is handed back so that the tail runs in groups of trees.
// One pure function of the level's shape and of the tunables: the build launches exactly what plan_level returns.  Plain C++
// with no device call and no tunable read, so that tests/level_plan_check.cpp can replay recorded levels on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/arroy_hip.h"  // ah_margin_mode, ah_metric

namespace ah {

// The tunables (common.h) a level's plan and its launches read, filled once per batch.
struct LevelKnobs {
    bool screen, screen_verify, rows_advance, rows_lds, retry_gate, exact_wide, node_prefetch;
    int rows_force, dense;
    uint32_t tile_blocks, node_blocks, split_blocks, row_blocks, rows_max_tc, dense_max_cols;
    double rows_cache_mb, dense_gmacs;
    long long mask_bits;
    uint32_t tail_groups;  // the tail in groups of trees (AH_BUILD_TAIL_GROUPS): most groups, where it is cut, least ids
    double tail_node_items;
    uint64_t tail_min_items;
    uint64_t lds_normals_bytes = 128u << 10;  // LDS given to the normals of one tree group (of 160 KiB per CU)
};

// One level as the plan sees it.
struct LevelShape {
    uint64_t N;  // rows of the dataset
    uint32_t n_trees, n_nodes;
    uint64_t pairs;  // (item, tree) pairs still under a node of the level
    uint32_t split_after;
    uint64_t rec_bytes, row_bytes;  // bytes of one normal as the margin pass streams it; of one row
    uint32_t hpitch;
    int metric;
    bool screen, screen8, rows8_lo;
    double screen8_quality;
    bool rows_allowed;      // full-dataset trees of an f32 metric, and the caller does not ask for node-major
    bool prev_rows;         // the previous level ran row-major
    bool grouped, fork_now;  // a tree group of the tail (node-major); the tail has been cut already
    bool subset;            // the trees cover id lists, not the dataset
    uint32_t mode_req;      // ah_margin_mode without AH_MARGIN_EXACT_ONLY
    bool dense_grid_legal;  // the dense product of the level fits one launch (dense_plan)
    const uint32_t *tree_first;  // [n_trees + 1]: first node of every tree, ~0 for a tree without one
};

struct RowsLaunch {  // `groups` groups of `tcv` trees from tree `t0` on, `np` trees in each
    uint32_t tcv, t0, groups, np;
};

struct LevelPlan {
    uint32_t row_tc = 0;  // >= 2: the level is row-major as far as node_of / side_bytes / the next level are concerned
    uint32_t lds_tc = 0, lds_worst = 0;  // LDS-resident groups of lds_tc trees; nodes of the largest group
    bool dense = false;
    bool fork = false;        // hand the level back unlaunched: the caller cuts it into groups of trees
    double best_cost = -1.0;  // AUTO: modelled cost in ns of the cheapest of node-major / row-major for this level
    std::vector<uint32_t> tree_first;  // the level's, with the gaps closed when the LDS variant was wanted
    std::vector<RowsLaunch> launches;  // the row-major launches of the level (none: dense or node-major)
};

// The last trees of a forest (`rem` of them, fewer than a group of `tc`) take the largest instantiation that they fill, or
// the next larger one when only a few of its slots would idle (13 trees: one 16-slot pass, measured 15 ms, instead of
// 8 + 4 + 1: 18-23 ms; spare slots repeat the last tree).
inline uint32_t tail_group_width(uint32_t tc, uint32_t rem) {
    uint32_t w = tc;
    while (w > 2 && w > rem) w >>= 1;
    for (uint32_t up = w << 1; up <= tc && w < rem; up <<= 1)
        if (up >= rem && up - rem <= (up >= 16 ? 3u : 1u)) w = up;
    return w;
}

// The launches of a row-major pass over n_trees trees in groups of tc: all full groups as one entry (the screened pass runs
// them chunk-major in ONE launch), then the groups tail_group_width forms for the last trees, a launch each.  LDS groups
// exist for 8 and 16 trees only: the last group keeps its width.
inline std::vector<RowsLaunch> rows_launch_list(uint32_t n_trees, uint32_t tc, bool lds) {
    std::vector<RowsLaunch> out;
    const uint32_t full = n_trees / tc;
    if (full) out.push_back(RowsLaunch{tc, 0, full, tc});
    for (uint32_t t0 = full * tc; t0 < n_trees;) {
        const uint32_t rem = n_trees - t0;
        const uint32_t tcv = lds ? tc : tail_group_width(tc, rem);
        const uint32_t np = std::min<uint32_t>(tcv, rem);
        out.push_back(RowsLaunch{tcv, t0, 1, np});
        t0 += np;
    }
    return out;
}

// Measured cost of one row-major pass in ns per row, as a function of the tree-group size and of the bytes of normals
// the group streams in the level (profiles/r02_*: 10M x 768 x 100 trees, every level forced to one group size), for
// the f32 kernels (rows of 3072 bytes) and for the screened kernels (binary16 rows of 1536 bytes).  While the normals fit
// the L2s a pass is bound by the vector-memory pipeline — one 16-byte load per 4 FMAs / 4 dot2c — and costs more as the
// octets of a wave stop sharing normals (deeper levels); beyond ~10 MB they come through the fabric and every group size
// converges to (1 + tc) rows' worth of traffic at ~8 TB/s.  Linear interpolation between the measured points.
struct CostPt {
    double mb, ns;
};
template <size_t N>
inline double interp(const CostPt (&t)[N], double mb) {
    if (mb <= t[0].mb) return t[0].ns;
    for (size_t i = 1; i < N; i++)
        if (mb <= t[i].mb) return t[i - 1].ns + (t[i].ns - t[i - 1].ns) * (mb - t[i - 1].mb) / (t[i].mb - t[i - 1].mb);
    return t[N - 1].ns;
}
inline double rows_pass_ns_per_row(uint32_t tc, double ws_mb, bool screened) {
    static const CostPt e16[] = {{0.4, 1.60}, {3.2, 1.83}, {6.3, 2.05}, {12.6, 2.33}, {25, 5.08}, {50, 6.05}, {100, 6.5}, {400, 6.8}};
    static const CostPt e8[] = {{0.2, 1.16}, {1.6, 1.22}, {3.2, 2.0}, {6.3, 2.5}, {12.6, 3.1}, {25, 3.5}, {100, 3.7}};
    static const CostPt e4[] = {{0.1, 0.73}, {0.8, 0.85}, {3.2, 0.88}, {6.3, 1.07}, {12.6, 1.45}, {25, 1.85}, {50, 2.05}, {100, 2.14}};
    static const CostPt e2[] = {{0.05, 0.49}, {0.8, 0.60}, {3.1, 0.62}, {6.3, 0.74}, {12.6, 0.99}, {25, 1.14}, {50, 1.21}};
    // screened kernels, chunk-major launches, epilogue on owner lanes (run r02w: 96 trees, every level forced)
    static const CostPt s16[] = {{0.025, 1.11}, {0.2, 1.13}, {0.4, 1.20}, {0.8, 1.25}, {1.6, 1.30}, {3.2, 1.45}, {6.4, 1.99},
                                 {12.7, 2.94}, {25, 3.57}, {51, 3.92}, {102, 4.10}, {203, 4.21}};
    static const CostPt s8[] = {{0.012, 0.58}, {0.1, 0.61}, {0.2, 0.67}, {0.4, 0.71}, {0.8, 0.74}, {1.6, 0.77}, {3.2, 0.85},
                                {6.4, 1.24}, {12.7, 1.66}, {25, 1.94}, {51, 2.09}, {102, 2.15}};
    static const CostPt s4[] = {{0.025, 0.325}, {0.05, 0.353}, {0.1, 0.415}, {0.2, 0.463}, {0.4, 0.493}, {0.8, 0.511},
                                {1.7, 0.45}, {3.4, 0.50}, {6.8, 0.69}, {13.6, 0.90}, {27, 1.03}, {54, 1.10}};  // one XCD per group, nt rows > 5 MB
    static const CostPt s2[] = {{0.003, 0.235}, {0.05, 0.243}, {0.1, 0.261}, {0.2, 0.274}, {0.4, 0.284}, {0.8, 0.292},
                                {1.6, 0.314}, {3.2, 0.389}, {6.4, 0.49}, {12.7, 0.56}, {25, 0.60}};
    if (screened) return tc >= 16 ? interp(s16, ws_mb) : tc == 8 ? interp(s8, ws_mb) : tc == 4 ? interp(s4, ws_mb) : interp(s2, ws_mb);
    return tc >= 16 ? interp(e16, ws_mb) : tc == 8 ? interp(e8, ws_mb) : tc == 4 ? interp(e4, ws_mb) : interp(e2, ws_mb);
}

inline LevelPlan plan_level(const LevelShape &sh, const LevelKnobs &k) {
    LevelPlan plan;
    const uint64_t N = sh.N, rec_bytes = sh.rec_bytes;
    const uint32_t n_trees = sh.n_trees, n_nodes = sh.n_nodes, mode_req = sh.mode_req;
    const bool screen = sh.screen, rows_allowed = sh.rows_allowed, grouped = sh.grouped;
    std::vector<uint32_t> &tree_first = plan.tree_first;
    tree_first.assign(sh.tree_first, sh.tree_first + n_trees + 1);

    // ---- margin mode of the first attempt ------------------------------------------------------------------------
    // Row-major streams all N rows once per group of row_tc trees; node-major reads only the still-active items, once
    // per tree.  A forced mode (ah_build_options.margin_mode) pins the kernel family wherever it is legal.
    const uint64_t nodes_per_tree = (n_nodes + n_trees - 1) / n_trees;
    uint32_t &row_tc = plan.row_tc, &lds_tc = plan.lds_tc, &lds_worst = plan.lds_worst;
    double &best_cost = plan.best_cost;
    if (grouped) {
        // a tree group of the tail: node-major (what the level it was cut from had chosen)
    } else if (rows_allowed && mode_req == AH_MARGIN_AUTO) {
        // Cost model in ns per row of 3072 bytes, fitted to per-level rocprofv3 traces of the 10M x 768 x 100-tree
        // build (profiles/): node-major = one HBM read of the row per (item, tree) pair; row-major = per pass and
        // row the HBM read of the row plus row_tc normals through the vector memory pipeline (L2 while the group's
        // normals of the level fit, the fabric beyond), scaled by the share of (row, tree) pairs still splitting,
        // plus the node_of / mask conversion of the level.
        // costs in ns, for rows of this dataset's size: node-major = one HBM read of the row per (item, tree) pair
        // (0.47 ns per 3072-byte row at 6.7 TB/s; the screen reads half the bytes)
        const double scale = screen ? (double)sh.hpitch * 2 / 1536.0 : (double)sh.row_bytes / 3072.0;
        // (with the int8 first stage: 768 bytes + ~10 % x 768 (second digit) per pair on data that quantises like the
        // benchmark's; worse data decide less there: scaled by the quality figure ensure_screen8 measured)
        // (measured, 10M x 768 x 100 trees: 0.130-0.142 ns per pair on uniform rows, quality 0.12, 0.140-0.151 on ~N(0,1)
        // rows, quality 0.18, with the rows' second digit as stage 1; 0.152-0.170 / 0.170-0.186 with the binary16 row)
        // (+0.02: the row-major entries of the tables below carry their mask conversion twice — level 9 of that build,
        // measured both ways, takes 130.7 ms row-major and 136.9 ms node-major, and this keeps it row-major)
        const double node8_ns = sh.rows8_lo ? std::min(0.24, 0.135 + 0.15 * sh.screen8_quality)
                                            : std::min(0.24, 0.155 + 0.125 * sh.screen8_quality);
        const double node_ns = screen ? (sh.screen8 && sh.metric != AH_DOT_PRODUCT ? node8_ns : 0.24) : 0.47;
        const double active = (double)sh.pairs / ((double)n_trees * (double)N);
        const double cost_node = (double)sh.pairs * node_ns * scale;
        const double convert = (double)n_trees * (double)N *
                               ((sh.prev_rows && k.rows_advance ? 0.007 : 0.01 + 0.03 * std::min(1.0, (double)nodes_per_tree / 256.0)) +
                                0.012 * std::min(1.0, (double)nodes_per_tree / 512.0));
        // A tc-slot schedule costs what its launches cost (rows_launch_list): the full groups in one chunk-major launch,
        // then the groups formed for the last trees (16 + ... + 4, or one more full group when only a few of its slots
        // would idle: idle slots cost what busy ones cost), each a launch of its own and priced as the pass of ITS size.
        // The table of pass costs was fitted on 96-tree builds, six or more groups in flight; a launch of one or two
        // 16-slot groups has the L2s to itself and behaves like one with half the normals (13-tree share, levels 6-9
        // forced both ways: 13.1 / 13.5 / 15.5 / 21.7 ms as one 16-slot pass — the table says 12.5 / 13.1 / 14.7 / 20.5
        // that way — and 16.9 / 17.2 / 17.8 / 20.7 as 8 + 4 + 1, which the table prices as it stands).
        // Counting 13 trees as 13/16 of a 16-slot pass and 13/8 of an 8-slot one kept level 5 of that share row-major
        // (13 ms; the dense product takes 11), level 8 on 8 + 4 + 1 and level 9 row-major (19.5; node-major 18.3).
        double best = 0.97 * cost_node;
        const double floor_ns = screen ? 0.15 : 0.45;  // the read of the row alone (screened: mostly Infinity Cache)
        auto launch_ns_per_row = [&](uint32_t tcv, uint32_t groups) {
            double ws_mb = (double)((uint64_t)tcv * nodes_per_tree * rec_bytes) / 1e6;
            if (groups <= 2 && tcv >= 16) ws_mb *= 0.5;
            return groups * (floor_ns + (rows_pass_ns_per_row(tcv, ws_mb, screen) - floor_ns) * std::min(1.0, active * 1.05));
        };
        for (uint32_t tc = std::min(16u, k.rows_max_tc); tc >= 2; tc >>= 1) {
            if (tc > 2 && tc / 2 >= n_trees) continue;  // do not instantiate more slots than trees
            const double ws_mb = (double)((uint64_t)tc * nodes_per_tree * rec_bytes) / 1e6;
            if (k.rows_cache_mb > 0 && ws_mb > k.rows_cache_mb) continue;
            double ns_per_row = 0.0;
            for (const RowsLaunch &l : rows_launch_list(n_trees, tc, false)) ns_per_row += launch_ns_per_row(l.tcv, l.groups);
            const double cost_rows = (double)N * ns_per_row * scale + convert;
            if (cost_rows < best || (k.rows_force == 1 && row_tc == 0)) {
                best = std::min(best, cost_rows);
                row_tc = tc;
            }
        }
        best_cost = best;
    } else if (rows_allowed && mode_req != AH_MARGIN_DENSE_MFMA) {
        row_tc = mode_req & 0xFFu;
    }
    // Dense screen of the level on the matrix units (dense_device.h): one product rows x normals^T instead of
    // n_trees / tc passes.  Cost: the rows leave HBM once (binary16), hpitch multiply-adds per (row, column) at the
    // sustained MFMA rate, an epilogue per (row, tree), and the reference arithmetic for the pairs left open.
    bool &dense = plan.dense;
    // (a launch carries at most 2^32 - 1 work-items: threads x row tiles x column tiles of the shape the level would take)
    const bool dense_legal = !grouped && rows_allowed && screen && k.dense != 0 && n_nodes <= k.dense_max_cols && sh.dense_grid_legal;
    if (dense_legal && mode_req == AH_MARGIN_DENSE_MFMA) {
        dense = true;
    } else if (dense_legal && mode_req == AH_MARGIN_AUTO) {
        // measured (10M x 768, 100 and 13 trees, profiles/r02_dense): the product itself 0.17 ns per row + 0.0023 ns per
        // (row, tree) of epilogue + hpitch multiply-adds per (row, padded column) at 495e3 MAC/ns (990 TF), never below
        // the 0.40 ns per row of the narrow kernel; 0.008 ns per pair for k_forest_exact_pairs
        const uint32_t bn = n_nodes > 128 ? 256u : 128u;
        const double cols = (double)(((uint64_t)n_nodes + bn - 1) / bn * bn);
        const double hscale = (double)sh.hpitch / 768.0;
        // (short rows: a tile's k-loop is a few latency-bound steps and the epilogue does not shrink with the row — never
        // below 0.25 ns per row; the exact pass scans a byte per pair whatever the row length)
        const double per_row = std::max(std::max(0.40 * hscale, 0.25), 0.17 * hscale + 0.0023 * n_trees + cols * (double)sh.hpitch / k.dense_gmacs);
        const double convert = (double)n_trees * (double)N * (sh.prev_rows && k.rows_advance ? 0.007 : 0.04);
        const double cost_dense = (double)N * per_row + (double)sh.pairs * (0.002 + 0.006 * (double)sh.row_bytes / 3072.0) + convert;
        dense = k.dense == 1 || best_cost < 0 || cost_dense < best_cost;
    }
    if (dense) row_tc = 16;  // the level is row-major as far as node_of / side_bytes / the next level are concerned
    // Top levels: all normals of a group of >= 8 trees fit in LDS -> the LDS-resident variant of the row-major pass.
    const bool want_lds = dense ? false : mode_req == AH_MARGIN_AUTO ? k.rows_lds && row_tc >= 2 : (mode_req & 0x100u) != 0;
    if (!grouped && rows_allowed && want_lds && (rec_bytes & 15) == 0) {
        tree_first[n_trees] = n_nodes;  // trees without a node in this level start where the next tree starts
        for (uint32_t t = n_trees; t-- > 0;) tree_first[t] = std::min(tree_first[t], tree_first[t + 1]);
        // measured per tree and row: screened 0.039 ns for 16-tree groups, 0.040 for 8-tree groups; f32 0.061 / 0.070
        const uint32_t tc_hi = mode_req == AH_MARGIN_AUTO ? std::min<uint32_t>(16, k.rows_max_tc) : (mode_req & 0xFFu);
        const uint32_t tc_lo = mode_req == AH_MARGIN_AUTO ? 8u : tc_hi;
        for (uint32_t tc = tc_hi; tc >= tc_lo && tc >= 8; tc >>= 1) {
            uint32_t worst = 0;
            for (uint32_t t0 = 0; t0 < n_trees; t0 += tc)
                worst = std::max(worst, tree_first[std::min(n_trees, t0 + tc)] - tree_first[t0]);
            if ((uint64_t)worst * rec_bytes <= k.lds_normals_bytes) {
                lds_tc = tc;
                lds_worst = worst;
                break;
            }
        }
        if (lds_tc) row_tc = lds_tc;
        else if (mode_req != AH_MARGIN_AUTO) row_tc = 0;  // a forced LDS mode that does not fit: node-major
    }

    // ---- the tail in groups? ---------------------------------------------------------------------------------------
    // This level would run node-major, most of its children will be Descendants nodes (fewer than 2 x split_after
    // items per node on average), every tree still has nodes in it, and the ids under them are worth the trouble:
    // hand the level back unlaunched; the caller cuts it into groups of trees.
    // (Skewed data — clusters of duplicates that keep a few nodes large for another thirty levels while most of the
    // forest is done — never meet the first condition and stay level by level: cut at the level where a tenth of the
    // ids is final, the 10M x 100-tree build on AH_SYNTH_CLUSTERED rows ran 29 levels five times over, 2.56 s against
    // 2.46: every level carries four attempts' launches whatever its size.)
    // (tree_first is read as the LDS test above left it: after a forced LDS mode that does not fit, with its gaps closed)
    if (!grouped && !sh.fork_now && k.tail_groups >= 2 && n_trees >= 2 && !sh.subset && row_tc < 2 && !dense &&
        sh.pairs >= k.tail_min_items && (double)sh.pairs <= k.tail_node_items * (double)sh.split_after * (double)n_nodes) {
        bool all = true;
        for (uint32_t t = 0; t < n_trees && all; t++)
            all = tree_first[t] != 0xFFFFFFFFu && (t == 0 ? tree_first[0] == 0 : tree_first[t] > tree_first[t - 1]);
        plan.fork = all;
    }
    if (!plan.fork && row_tc >= 2 && !dense) plan.launches = rows_launch_list(n_trees, row_tc, lds_tc != 0);
    return plan;
}

}  // namespace ah
