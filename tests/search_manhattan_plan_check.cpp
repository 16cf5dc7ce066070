// plan_chunk under AH_SEARCH_TILES_MANHATTAN (arroy_amd/csrc/search_plan.h) on the host: with the knob a uniform Manhattan sub-batch
// plans as the Euclidean one of its shape, field for field; without it as before; the difference screen, mixed sub-batches and the
// mid tiles are untouched.  Built by tests/test_search_manhattan_plan_cpu.py with ASan and UBSan.
#include "../arroy_amd/csrc/search_plan.h"

#include <cstdio>

using namespace ah;

static int failures = 0;
static void check(bool ok, const char *what) {
    if (!ok) fprintf(stderr, "FAILED: %s\n", what), failures++;
}
static bool same(const ChunkPlan &a, const ChunkPlan &b) {
    return a.big_k == b.big_k && a.kstride == b.kstride && a.max_tiles_bound == b.max_tiles_bound && a.heap_cap == b.heap_cap &&
           a.bitmap_words == b.bitmap_words && a.bitmap_fits == b.bitmap_fits && a.hash_fits == b.hash_fits && a.tiles == b.tiles &&
           a.visit_cap == b.visit_cap && a.n_leaf_sums == b.n_leaf_sums && a.screened == b.screened && a.screened8 == b.screened8 &&
           a.items_cap == b.items_cap && a.zero_copy_queries == b.zero_copy_queries && a.block_ok == b.block_ok && a.small_units == b.small_units &&
           a.fuse_prepare == b.fuse_prepare && a.small_first == b.small_first && a.descent == b.descent && a.multi_blocks == b.multi_blocks &&
           a.own_units == b.own_units && a.units_per_query == b.units_per_query && a.single_fused == b.single_fused && a.ids_by_tiles == b.ids_by_tiles &&
           a.units == b.units && a.small_tiles == b.small_tiles && a.tile_launch == b.tile_launch && a.tile_grid_x == b.tile_grid_x &&
           a.tile_grid_y == b.tile_grid_y && a.fused_flag == b.fused_flag && a.sel_lds == b.sel_lds && a.fused_lds == b.fused_lds && a.flagger == b.flagger &&
           a.max_vis8 == b.max_vis8 && a.tiles_bq == b.tiles_bq && a.mid_tiles == b.mid_tiles && a.mixed_tiles == b.mixed_tiles;
}

int main() {
    SearchKnobs kn{};
    kn.wave = kn.bitmap = kn.tiles = kn.screen = kn.screen8 = kn.fused_flag = kn.item_list = kn.small_gate = kn.multi = kn.single_fused = true;
    kn.multi_own_units = kn.flat_tiles = kn.multi_ids_by_tiles = kn.fused_prepare = true;
    kn.small_units_max_queries = kn.block_max_queries = kn.mid_tiles_max_queries = 64, kn.small_tiles_max_queries = 8, kn.screen8_min_queries = 65;
    kn.multi_trees_per_block = 8, kn.multi_max_queries = 32, kn.screen8_max_visits = 4;
    ChunkShape z{};  // 20 000 rows x 200 dimensions under 12 trees, leaves of ~130 rows, search_k of 15 of them
    z.count = 10, z.search_k = 2000, z.nns_stride = 2200, z.by_vector = z.allow8 = z.screen_ready = z.screen8_ready = z.batch_count = true;
    z.n_nodes = 3700, z.n_trees = 12, z.n_leaves = 1850, z.desc_len = 240000, z.max_desc = 200, z.wave_descent = true;
    z.dims = 200, z.pitch = 224, z.hpitch = z.pitch8 = 256, z.row_bytes = 896, z.n = 20000, z.max_id = 19999, z.filter_share = 1.0;
    z.tile_candidates = 512, z.kstride_batch = 4096, z.kstride_single = 4100;
    auto plan = [&](uint64_t nq, int metric, SearchKnobs k, bool l1, bool screen_diff = false, bool mixed_tiles = false, bool mid = false) {
        ChunkShape s = z;
        s.nq = nq, s.metric = metric;
        k.tiles_manhattan = l1, k.screen_diff = screen_diff, k.mixed_tiles = mixed_tiles, k.mid_tiles = mid;
        return plan_chunk(s, k);
    };
    const int E = AH_EUCLIDEAN, M = AH_MANHATTAN;
    for (int filtered = 0; filtered < 2; filtered++) {  // uniform sub-batches, unfiltered and under one filter
        z.filtered = z.uniform_filter = filtered != 0, z.filter_share = filtered ? 0.5 : 1.0;
        for (uint64_t nq : {1, 16, 200}) {
            const ChunkPlan e = plan(nq, E, kn, true), before = plan(nq, M, kn, false);
            check(e.tiles && e.tile_launch == TileLaunch::F32 && !e.screened && same(plan(nq, M, kn, true), e), "with the knob: Euclidean's f32 plan, field for field");
            check(!before.tiles && before.tile_launch == TileLaunch::None && before.units == UnitBuilder::None && !before.small_units && before.items_cap == 0,
                  "without the knob: the sorted path");
            check(same(e, plan(nq, E, kn, false)) && same(plan(nq, AH_COSINE, kn, true), plan(nq, AH_COSINE, kn, false)), "no other metric's plan changes");
            check(plan(nq, M, kn, true, true).screened && same(plan(nq, M, kn, true, true), plan(nq, M, kn, false, true)), "the difference screen serves as before");
        }
    }
    z.filtered = z.uniform_filter = false, z.filter_share = 1.0, z.dims = 31;
    check(!plan(16, M, kn, true).tiles, "dims 31: the gate of the f32 tiles");
    z.dims = 200, z.search_diff_off = true;
    check(!plan(16, M, kn, false, true).tiles && same(plan(16, M, kn, true, true), plan(16, E, kn, true, true)), "the screen switched off: the exact tiles under the knob");
    z.search_diff_off = false;
    check(plan(16, E, kn, true, false, false, true).mid_tiles && !plan(16, M, kn, true, false, false, true).mid_tiles &&
              same(plan(16, M, kn, true, false, false, true), plan(16, M, kn, true)),
          "the mid tiles: Euclidean's as before, never Manhattan's");
    z.filtered = z.mixed = true, z.filter_share = 0.5;
    check(!plan(16, M, kn, true, false, true).tiles && same(plan(16, M, kn, true, false, true), plan(16, M, kn, false, false, true)), "a mixed sub-batch keeps the sorted path");
    if (failures) return 1;
    printf("Manhattan sub-batches are planned where they should be\n");
    return 0;
}
