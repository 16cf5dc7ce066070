// plan_chunk's gate for mixed sub-batches on the leaf tiles (arroy_amd/csrc/search_plan.h: ChunkPlan::mixed_tiles,
// AH_SEARCH_MIXED_TILES) on the host, no device: every condition at its threshold, what a mixed tile plan must not name, and
// its scratch against the uniform tile plan's.  Built by tests/test_search_mixed_plan_cpu.py with ASan and UBSan.
#include "../arroy_amd/csrc/search_plan.h"

#include <cstdio>

using namespace ah;

static int failures = 0;
static void check(bool ok, const char *what) {
    if (!ok) fprintf(stderr, "FAILED: %s\n", what), failures++;
}

// every array of both layouts, one byte an element: the layouts are compared by which arrays they carve and how long
struct Bufs {
    char *d_qf32, *d_qrows, *d_qvecs, *d_qhdrs, *d_nns, *d_dist, *d_counts, *d_overflow, *d_list, *d_segs, *d_tiles, *d_ka, *d_kb, *d_oi, *d_od,
        *d_err, *d_unique, *d_inv, *d_visits, *d_sorted, *d_units, *d_leaf_count, *d_cursor, *d_ustart, *d_leaf_sums, *d_items, *d_unit_counts,
        *d_aux, *d_q16, *d_qstats, *d_q8, *d_q8stats, *d_aux8, *d_slots, *d_sks, *d_cnt;
    char *h_q, *h_qrows, *h_overflow, *h_list, *h_segs, *h_tiles, *h_oi, *h_od, *h_err, *h_counts, *h_slots, *h_sks, *h_cnt;
};
static void layouts(const ChunkShape &z, const ChunkPlan &p, size_t &dev, size_t &pin) {
    Bufs b{};
    Carver d(nullptr), h(nullptr);
    search_device_layout(d, z, p, b);
    search_pinned_layout(h, z, p, b);
    dev = d.off, pin = h.off;
}

int main() {
    SearchKnobs kn{};
    kn.wave = kn.bitmap = kn.tiles = kn.screen = kn.screen8 = kn.fused_flag = kn.item_list = kn.small_gate = kn.multi = kn.single_fused = true;
    kn.multi_own_units = kn.flat_tiles = kn.multi_ids_by_tiles = kn.mid_tiles = kn.fused_prepare = true;
    kn.small_units_max_queries = kn.block_max_queries = kn.mid_tiles_max_queries = 64, kn.small_tiles_max_queries = 8, kn.screen8_min_queries = 9;
    kn.multi_trees_per_block = 8, kn.multi_max_queries = 32, kn.screen8_max_visits = 4;
    kn.mixed_tiles = true;
    ChunkShape z{};  // 20 000 rows x 200 dimensions under 12 trees, leaves of ~130 rows, search_k of 15 of them
    z.nq = 16, z.count = 10, z.search_k = 2000, z.nns_stride = 2200, z.by_vector = z.allow8 = z.screen_ready = z.screen8_ready = z.batch_count = true;
    z.n_nodes = 3700, z.n_trees = 12, z.n_leaves = 1850, z.desc_len = 240000, z.max_desc = 200, z.metric = AH_COSINE, z.wave_descent = true;
    z.dims = 200, z.pitch = 208, z.hpitch = z.pitch8 = 256, z.row_bytes = 800, z.n = 20000, z.max_id = 19999, z.filter_share = 0.5;
    z.tile_candidates = 512, z.kstride_batch = 4096, z.kstride_single = 4100;
    z.filtered = z.mixed = true;
    auto plan = [&](uint64_t nq, int metric = AH_COSINE) {
        ChunkShape s = z;
        s.nq = nq, s.metric = metric;
        return plan_chunk(s, kn);
    };
    auto is_mixed = [](const ChunkPlan &p) { return p.tiles && p.mixed_tiles && p.tile_launch == TileLaunch::Mixed; };
    // what reads "the kept ids of the unit's first visit", or sizes anything by them
    auto names_nothing_per_first_visit = [](const ChunkPlan &p) {
        return !p.screened8 && !p.small_tiles && !p.mid_tiles && p.items_cap == 0 && !p.own_units && !p.single_fused && !p.ids_by_tiles &&
               p.descent != Descent::Multi && !p.tiles_bq && p.max_vis8 == 0;
    };
    for (uint64_t nq : {2, 8, 9, 16, 64, 65, 300}) {
        const ChunkPlan p = plan(nq);
        check(is_mixed(p) && p.screened && names_nothing_per_first_visit(p), "a mixed Cosine sub-batch takes the mixed tiles and nothing per first visit");
        check(p.tile_grid_x == std::min<uint64_t>(2048, 32 * nq) && p.tile_grid_y == 4, "blockIdx.x walks the units, blockIdx.y the slabs of the full leaf");
        check(p.units == (p.small_units ? UnitBuilder::UnitsSmall : UnitBuilder::LeafScan) && p.small_units == (nq <= 16), "units by node only: k_units_small or the leaf scan");
        check(p.descent == (nq <= 64 ? Descent::Block : Descent::WaveSmallBig), "the block descent as the last pass, the waves past it");
    }
    z.filter_share = 0.2;
    check(is_mixed(plan(16)) && plan(16).descent == Descent::WaveBig, "the big waves first under a small share");
    z.filter_share = 0.002, z.wave_descent = false;
    check(is_mixed(plan(16)) && plan(16).descent == Descent::Octet && names_nothing_per_first_visit(plan(16)), "octets without the wave descent");
    z.filter_share = 0.5, z.wave_descent = true;
    // the scratch: the arrays of the uniform tile plan of the same shape, plus d_slots / h_slots
    {
        ChunkShape u = z;
        u.mixed = false, u.uniform_filter = true;
        SearchKnobs plain = kn;  // (the uniform plan without what the mixed one must not name, so that the array lists compare)
        plain.item_list = plain.screen8 = false;
        size_t dev_m, pin_m, dev_u, pin_u;
        layouts(z, plan_chunk(z, kn), dev_m, pin_m);
        layouts(u, plan_chunk(u, plain), dev_u, pin_u);
        check(plan_chunk(u, plain).tiles && !plan_chunk(u, plain).mixed_tiles && plan_chunk(u, plain).tile_launch != TileLaunch::Mixed, "a uniform sub-batch is untouched");
        check(dev_m == dev_u + pad256(z.nq) && pin_m == pin_u + pad256(z.nq), "both layouts: the uniform tile plan's arrays plus the slots");
    }
    // each metric / screen combination
    check(is_mixed(plan(16, AH_DOT_PRODUCT)) && plan(16, AH_DOT_PRODUCT).screened, "DotProduct on the binary16 dot screen");
    check(is_mixed(plan(16, AH_EUCLIDEAN)) && !plan(16, AH_EUCLIDEAN).screened, "Euclidean on its f32 rows");
    check(!plan(16, AH_MANHATTAN).tiles, "Manhattan without the difference screen stays on the sorted path");
    for (int m : {AH_BQ_EUCLIDEAN, AH_BQ_COSINE, AH_BQ_MANHATTAN}) check(!plan(16, m).tiles, "the 1-bit metrics stay on the sorted path");
    kn.tiles_bq = true;
    for (int m : {AH_BQ_EUCLIDEAN, AH_BQ_COSINE, AH_BQ_MANHATTAN}) check(!plan(16, m).tiles && !plan(16, m).tiles_bq, "... under AH_SEARCH_TILES_BQ too");
    kn.tiles_bq = false, kn.screen_diff = true;
    check(is_mixed(plan(16, AH_MANHATTAN)) && plan(16, AH_MANHATTAN).screened && is_mixed(plan(16, AH_EUCLIDEAN)) && plan(16, AH_EUCLIDEAN).screened,
          "the difference screen");
    z.search_diff_off = true;
    check(!plan(16, AH_MANHATTAN).tiles && is_mixed(plan(16, AH_EUCLIDEAN)) && !plan(16, AH_EUCLIDEAN).screened, "the difference screen switched off");
    z.search_diff_off = false, kn.screen_diff = false, kn.screen = false;
    check(!plan(16).tiles && !plan(16, AH_DOT_PRODUCT).tiles && is_mixed(plan(16, AH_EUCLIDEAN)), "unscreened Cosine / DotProduct stay on the sorted path");
    kn.screen = true, z.screen_ready = false;
    check(!plan(16).tiles, "no binary16 copy, no screen");
    z.screen_ready = true;
    // the existing gates at their thresholds
    z.count = kSelectCap;
    check(is_mixed(plan(16)), "count = kSelectCap");
    z.count = kSelectCap + 1;
    check(!plan(16).tiles, "count = kSelectCap + 1");
    z.nns_stride = kSelectCap;
    check(is_mixed(plan(16)), "... unless the buffer is that short");
    z.count = 10, z.nns_stride = 2200, z.dims = 32;
    check(is_mixed(plan(16)), "dims 32");
    z.dims = 31;
    check(!plan(16).tiles, "dims 31");
    z.dims = 200, z.max_desc = 65535u * kTileSmallSlab;
    check(is_mixed(plan(16)) && plan(16).tile_grid_y == 65535u, "small_slabs 65535");
    z.max_desc = 65535u * kTileSmallSlab + 1;
    check(!plan(16).tiles, "small_slabs 65536");
    z.max_desc = 200, z.batch_count = false;
    check(!plan(16).tiles, "never big_k");
    z.batch_count = true, z.max_id = 0xFFFFFFFEu, z.nns_stride = kHashMaxCandidates + 1;
    check(!plan(16).tiles, "neither the bitmap nor the hash dedup");
    z.nns_stride = 2200;
    check(is_mixed(plan(16)) && plan(16).flagger == Flagger::Hash, "the hash dedup");
    z.max_id = 0xFFFFFFFFu;
    check(!plan(16).tiles, "id u32::MAX is the flaggers' mark of a duplicate: no dedup of the tiles holds it");
    z.max_id = 19999, kn.tiles = false;
    check(!plan(16).tiles, "AH_SEARCH_TILES=0");
    kn.tiles = true;
    // not mixed / switch off: the plan as before
    kn.mixed_tiles = false;
    const ChunkPlan off = plan(16);
    check(!off.tiles && !off.mixed_tiles && off.tile_launch == TileLaunch::None && !off.screened && off.items_cap == 0 && !off.small_units && !off.fuse_prepare,
          "switch off: a mixed sub-batch takes the sorted path");
    if (failures) return 1;
    printf("mixed sub-batches are planned where they should be\n");
    return 0;
}
