// plan_chunk's flag for the mid-size submissions' tiles (arroy_amd/csrc/search_plan.h: ChunkPlan::mid_tiles) on the host, no
// device: every condition at its threshold, and the plan with the switch off untouched.  Built by
// tests/test_search_mid_plan_cpu.py with ASan and UBSan.
#include "../arroy_amd/csrc/search_plan.h"

#include <cstdio>

using namespace ah;

static int failures = 0;
static void check(bool ok, const char *what) {
    if (!ok) fprintf(stderr, "FAILED: %s\n", what), failures++;
}

int main() {
    SearchKnobs kn{};
    kn.wave = kn.bitmap = kn.tiles = kn.screen = kn.screen8 = kn.fused_flag = kn.item_list = kn.small_gate = kn.multi = true;
    kn.small_units_max_queries = kn.block_max_queries = 64, kn.small_tiles_max_queries = 8, kn.screen8_min_queries = 65;
    kn.multi_trees_per_block = 8, kn.multi_max_queries = 32, kn.screen8_max_visits = 4;
    kn.mid_tiles = true, kn.mid_tiles_max_queries = 64;
    ChunkShape z{};  // 20 000 rows x 200 dimensions under 12 trees, leaves of ~130 rows, search_k of 15 of them
    z.nq = 16, z.count = 10, z.search_k = 2000, z.nns_stride = 2200, z.by_vector = z.allow8 = z.screen_ready = z.screen8_ready = z.batch_count = true;
    z.n_nodes = 3700, z.n_trees = 12, z.n_leaves = 1850, z.desc_len = 240000, z.max_desc = 200, z.metric = AH_COSINE, z.wave_descent = true;
    z.dims = 200, z.pitch = 208, z.hpitch = z.pitch8 = 256, z.row_bytes = 800, z.n = 20000, z.max_id = 19999, z.filter_share = 1.0;
    z.tile_candidates = 512, z.kstride_batch = 4096, z.kstride_single = 4100;
    auto plan = [&](uint64_t nq, int metric = AH_COSINE) {
        ChunkShape s = z;
        s.nq = nq, s.metric = metric;
        return plan_chunk(s, kn);
    };
    const ChunkPlan p = plan(16);
    check(p.mid_tiles && p.tile_launch == TileLaunch::Mid && p.units == UnitBuilder::UnitsSmall && !p.small_tiles && !p.screened8, "16 queries take the mid tiles");
    check(p.items_cap == 16 * (2200 / 64 + 1) + kSmallVisits + 1 && p.tile_grid_x == p.items_cap - 1 && p.tile_grid_y == 1, "one block per item the list can hold");
    check(!plan(8).mid_tiles && plan(8).small_tiles && plan(9).mid_tiles && plan(64).mid_tiles && !plan(65).mid_tiles, "the band is 9 .. 64 queries");
    check(plan(16, AH_DOT_PRODUCT).mid_tiles && plan(16, AH_EUCLIDEAN).mid_tiles && !plan(16, AH_EUCLIDEAN).screened, "DotProduct screened, Euclidean on its f32 rows");
    check(!plan(16, AH_MANHATTAN).mid_tiles && !plan(16, AH_BQ_COSINE).mid_tiles, "Manhattan without its screen and the 1-bit metrics stay out");
    kn.screen_diff = true;
    check(plan(16, AH_MANHATTAN).mid_tiles && plan(16, AH_EUCLIDEAN).mid_tiles && plan(16, AH_EUCLIDEAN).screened, "the difference screen");
    kn.screen = false;
    check(!plan(16).mid_tiles && plan(16, AH_EUCLIDEAN).mid_tiles, "unscreened Cosine keeps the f32 tiles with its epilogue");
    kn.screen = true, kn.screen8_min_queries = 9;
    check(plan(16).screened8 && !plan(16).mid_tiles, "never with the int8 stage");
    kn.screen8_min_queries = 65, kn.mid_tiles_max_queries = 12;
    check(plan(12).mid_tiles && !plan(13).mid_tiles, "AH_SEARCH_MID_TILES_MAX_QUERIES");
    kn.mid_tiles_max_queries = 64, kn.mid_items_cap = 4;
    check(plan(16).mid_tiles && plan(16).items_cap == 5 && plan(16).tile_grid_x == 4, "AH_SEARCH_MID_ITEMS_CAP");
    kn.mid_items_cap = 0, kn.item_list = false;
    check(!plan(16).mid_tiles, "no list, no mid tiles");
    kn.item_list = true;
    z.search_k = 20000, z.nns_stride = 20200;  // ~195 estimated leaves a query: k_units_small does not place these visits
    check(!plan(16).small_units && !plan(16).mid_tiles, "the small path's admission rule comes first");
    z.search_k = 2000, z.nns_stride = 2200, z.dims = 24;
    check(!plan(16).tiles && !plan(16).mid_tiles, "dims >= 32");
    z.dims = 200, kn.mid_tiles = false;
    const ChunkPlan off = plan(16);
    check(!off.mid_tiles && off.tile_launch == TileLaunch::Big2D && off.tile_grid_x == 2048 && off.items_cap == p.items_cap, "switch off: the plan as before");
    if (failures) return 1;
    printf("the mid tiles are planned where they should be\n");
    return 0;
}
