// plan_chunk under AH_SEARCH_FLAG_SLICED (arroy_amd/csrc/search_plan.h: ChunkPlan::flag_slices, Flagger::HashSliced) on the host, no
// device: every condition at its threshold, the switch at 0 the plan as before.  Built by tests/test_search_flag_sliced_plan_cpu.py.
#include "../arroy_amd/csrc/search_plan.h"

#include <cstdio>

using namespace ah;

static int failures = 0;
static void check(bool ok, const char *what) {
    if (!ok) fprintf(stderr, "FAILED: %s\n", what), failures++;
}
// field for field; flags = false: all but what names the duplicate flagger
static bool same(const ChunkPlan &a, const ChunkPlan &b, bool flags = true) {
#define F(x) &&a.x == b.x
    return true F(big_k) F(kstride) F(max_tiles_bound) F(heap_cap) F(tiles) F(visit_cap) F(n_leaf_sums) F(screened) F(screened8) F(items_cap)
        F(zero_copy_queries) F(block_ok) F(small_units) F(fuse_prepare) F(small_first) F(descent) F(multi_blocks) F(own_units) F(units_per_query)
        F(single_fused) F(ids_by_tiles) F(units) F(small_tiles) F(tile_launch) F(tile_grid_x) F(tile_grid_y) F(fused_flag) F(sel_lds) F(max_vis8)
        F(tiles_bq) F(mid_tiles) F(mixed_tiles) &&
        (!flags || (true F(bitmap_words) F(bitmap_fits) F(hash_fits) F(fused_lds) F(flagger) F(flag_slices)));
#undef F
}

int main() {
    SearchKnobs parent{};  // a library without the switch: both new knobs zero
    parent.wave = parent.bitmap = parent.tiles = parent.screen = parent.screen8 = parent.fused_flag = parent.item_list = parent.small_gate = parent.multi = true;
    parent.small_units_max_queries = parent.block_max_queries = 64, parent.small_tiles_max_queries = 8, parent.screen8_min_queries = 65;
    parent.multi_trees_per_block = 8, parent.multi_max_queries = 32, parent.screen8_max_visits = 4;
    SearchKnobs off = parent, on = parent;
    off.flag_slice_candidates = on.flag_slice_candidates = 16384, on.flag_sliced = true;
    ChunkShape z{};  // 5M rows x 768 dimensions under 100 trees, leaves of ~400 rows
    z.count = 100, z.by_vector = z.allow8 = z.screen_ready = z.screen8_ready = z.batch_count = z.wave_descent = true;
    z.n_nodes = 2500000, z.n_trees = 100, z.n_leaves = 1250000, z.desc_len = 500000000, z.max_desc = 768, z.metric = AH_COSINE;
    z.dims = z.pitch = z.hpitch = z.pitch8 = 768, z.row_bytes = 3072, z.n = 5000000, z.filter_share = 1.0, z.tile_candidates = 512;
    auto plan = [&](const SearchKnobs &kn, uint32_t stride, uint32_t max_id = 4999999, uint64_t nq = 200) {
        ChunkShape s = z;
        s.nq = nq, s.nns_stride = stride, s.search_k = stride - z.max_desc, s.max_id = max_id, s.kstride_batch = s.kstride_single = stride;
        return plan_chunk(s, kn);
    };
    const uint32_t H = kHashMaxCandidates, fit = kBitmapMaxWords * 32 - 1, cap = kFlagMaxSlices * 16384;  // fit: the bitmap's largest max_id
    for (uint64_t nq : {1, 16, 200})
        for (uint32_t stride : {2048u, H, H + 1, 32768u, cap, cap + 1})
            for (uint32_t max_id : {19999u, fit, fit + 1, 4999999u, 0xFFFFFFFFu})
                check(same(plan(off, stride, max_id, nq), plan(parent, stride, max_id, nq)) && plan(off, stride, max_id, nq).flagger != Flagger::HashSliced,
                      "switch 0: the parent's plan field for field");
    const ChunkPlan a = plan(on, H), b = plan(on, H + 1), c = plan(on, 32768, fit), d = plan(on, 32768, fit + 1);
    check(a.tiles && a.flagger == Flagger::Hash && a.flag_slices == 0 && same(a, plan(off, H)), "stride 24 576: one hash set, as before");
    check(b.tiles && !b.hash_fits && !b.bitmap_fits && b.flagger == Flagger::HashSliced && b.flag_slices == 2 && !b.fused_flag, "stride 24 577: two slices");
    check(!plan(off, H + 1).tiles && plan(off, H + 1).flagger == Flagger::None, "... and the sorted path without the switch");
    check(c.bitmap_words == kBitmapMaxWords && c.flagger == Flagger::Bitmap && same(c, plan(off, 32768, fit)), "max_id 1 277 951: the bitmap, as before");
    check(d.bitmap_words > kBitmapMaxWords && d.flagger == Flagger::HashSliced && same(d, c, false), "max_id 1 277 952: sliced, the bitmap's plan behind the flags");
    check(plan(on, cap).flag_slices == kFlagMaxSlices && plan(on, cap).tiles, "64 slices: the cap");
    check(plan(on, cap + 1).flag_slices == 0 && !plan(on, cap + 1).tiles && same(plan(on, cap + 1), plan(off, cap + 1)), "65 slices: the sorted path");
    check(plan(on, 32768, 0xFFFFFFFFu).flag_slices == 0 && !plan(on, 32768, 0xFFFFFFFFu).tiles, "max_id 0xFFFFFFFF is the empty slot");
    on.flag_slice_candidates = 4096;
    check(plan(on, 32768).flag_slices == 8 && !plan(on, 64 * 4096 + 1).tiles, "AH_SEARCH_FLAG_SLICE_CANDIDATES 4096");
    on.flag_slice_candidates = 1 << 20, on.bitmap = false;
    check(plan(on, 131072, 39999).flag_slices == 1 && plan(on, 131072, 39999).flagger == Flagger::HashSliced && plan(on, 16384, 3999).flagger == Flagger::Hash,
          "AH_SEARCH_BITMAP=0 takes the bitmap away; 1 048 576 a slice: one slice");
    if (failures) return 1;
    printf("the sliced flags are planned where they should be\n");
    return 0;
}
