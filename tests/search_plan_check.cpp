// The plan of one search sub-batch (arroy_amd/csrc/search_plan.h) on the host, no device: plan_chunk and the byte totals of the
// two scratch layouts against the sub-batches recorded from the search before the plan was one function
// (tests/golden/search_plan_cases.txt: tunables | shape | decisions | decisions of the tile pass | device and pinned bytes);
// both layouts walked over a fake block (alignment, order, no overlap, the adjacency the single copies rely on);
// wave_descent_wanted and sorted_dedup_kind at their thresholds.  Built by tests/test_search_plan_cpu.py with ASan and UBSan.
#include "../arroy_amd/csrc/search_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace ah;

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            fprintf(stderr, "FAILED: " __VA_ARGS__); \
            fprintf(stderr, "\n");                \
            failures++;                           \
        }                                         \
    } while (0)

// stand-ins with the element sizes of search.hip's types (the recorded byte totals hold them to those)
struct B16 { uint64_t a, b; };  // Visit, TileUnit, RerankSeg, float4
struct B8 { uint64_t a; };      // RerankTile, uint2
struct Bufs {
    float *d_qf32;
    uint32_t *d_qrows;
    uint8_t *d_qvecs;
    float *d_qhdrs;
    uint32_t *d_nns;
    float *d_dist;
    uint32_t *d_counts, *d_overflow, *d_list;
    B16 *d_segs;
    B8 *d_tiles;
    uint64_t *d_ka, *d_kb;
    uint32_t *d_oi;
    float *d_od;
    uint32_t *d_err, *d_unique, *d_inv;
    B16 *d_visits, *d_sorted, *d_units;
    uint32_t *d_leaf_count, *d_cursor, *d_ustart;
    B8 *d_leaf_sums;
    uint32_t *d_items, *d_unit_counts;
    float *d_aux;
    uint16_t *d_q16;
    B16 *d_qstats;
    int8_t *d_q8;
    B16 *d_q8stats;
    float *d_aux8;
    uint32_t *d_slots, *d_sks, *d_cnt;
    float *h_q;
    uint32_t *h_qrows, *h_overflow, *h_list;
    B16 *h_segs;
    B8 *h_tiles;
    uint32_t *h_oi;
    float *h_od;
    uint32_t *h_err, *h_counts, *h_slots, *h_sks, *h_cnt;
};

struct Case {
    SearchKnobs kn{};
    ChunkShape z{};
    std::vector<long long> p, t;  // the decisions as recorded
    size_t dev_bytes = 0, pin_bytes = 0;
};

static bool parse(const std::string &line, Case &c) {
    std::istringstream in(line);
    std::string tag;
    long long v[25];
    if (!(in >> tag) || tag != "kn") return false;
    for (auto &x : v)
        if (!(in >> x)) return false;
    SearchKnobs &k = c.kn;
    k.bitmap = v[0], k.tiles = v[1], k.screen = v[2], k.screen8 = v[3], k.item_list = v[4], k.small_gate = v[5], k.status_wipe = v[6];
    k.fused_prepare = v[7], k.multi = v[8], k.multi_own_units = v[9], k.flat_tiles = v[10], k.single_fused = v[11], k.multi_ids_by_tiles = v[12];
    k.multi_trace = v[13], k.fused_flag = v[14], k.spin_wait = v[15], k.wave = v[16], k.debug = v[17];
    k.small_tiles_max_queries = v[18], k.screen8_min_queries = v[19], k.small_units_max_queries = v[20], k.block_max_queries = v[21];
    k.multi_trees_per_block = v[22], k.multi_max_queries = v[23], k.screen8_max_visits = v[24];
    ChunkShape &z = c.z;
    int by_vector, filtered, mixed, varied, uniform, wave, allow8, r16, r8, off8, batch_count;
    unsigned long long share_bits;
    if (!(in >> tag) || tag != "|" || !(in >> tag) || tag != "z") return false;
    in >> z.nq >> z.count >> z.search_k >> z.nns_stride >> by_vector >> filtered >> mixed >> varied >> uniform >> std::hex >> share_bits >> std::dec >>
        wave >> allow8 >> z.n_nodes >> z.n_trees >> z.n_leaves >> z.desc_len >> z.max_desc >> z.metric >> z.dims >> z.pitch >> z.hpitch >> z.pitch8 >>
        z.row_bytes >> z.n >> z.max_id >> r16 >> r8 >> off8 >> z.tile_candidates >> z.inv_bytes >> batch_count >> z.kstride_batch >> z.kstride_single;
    z.by_vector = by_vector, z.filtered = filtered, z.mixed = mixed, z.varied = varied, z.uniform_filter = uniform, z.wave_descent = wave;
    z.allow8 = allow8, z.screen_ready = r16, z.screen8_ready = r8, z.search8_off = off8, z.batch_count = batch_count;
    static_assert(sizeof(double) == 8, "the share travels as its bits");
    memcpy(&z.filter_share, &share_bits, 8);
    if (!(in >> tag) || tag != "|" || !(in >> tag) || tag != "p") return false;
    c.p.resize(18), c.t.resize(16);
    for (auto &x : c.p) in >> x;
    if (!(in >> tag) || tag != "|" || !(in >> tag) || tag != "t") return false;
    for (auto &x : c.t) in >> x;
    if (!(in >> tag) || tag != "|" || !(in >> tag) || tag != "b") return false;
    in >> c.dev_bytes >> c.pin_bytes;
    return !in.fail();
}

static std::string join(const std::vector<long long> &v) {
    std::string out;
    for (long long x : v) out += (out.empty() ? "" : " ") + std::to_string(x);
    return out;
}

// every array lies in the block, 256-aligned, behind the END of the one before it; an array not wanted is null
struct Arr {
    const char *name;
    const void *p;
    size_t bytes;  // as the search asks for them (search.hip before the layouts were written down once)
};
static size_t walk(const std::vector<Arr> &arrays, const uint8_t *base, size_t bytes, size_t line) {
    const uint8_t *last_end = base;
    size_t n = 0;
    for (const Arr &a : arrays) {
        const uint8_t *p = static_cast<const uint8_t *>(a.p);
        if (!p) continue;
        n++;
        CHECK((size_t)(p - base) % 256 == 0, "case %zu: %s is not 256-aligned", line, a.name);
        CHECK(p >= last_end, "case %zu: %s overlaps the array before it", line, a.name);
        CHECK(a.bytes > 0 && p + a.bytes <= base + bytes, "case %zu: %s (%zu bytes) does not lie inside the block", line, a.name, a.bytes);
        last_end = p + a.bytes;
    }
    return n;
}

static void check_layouts(const Case &c, const ChunkPlan &p, size_t line) {
    Bufs count{};
    Carver dn(nullptr), pn(nullptr);
    search_device_layout(dn, c.z, p, count);
    search_pinned_layout(pn, c.z, p, count);
    CHECK(dn.off + kSearchDeviceSlack == c.dev_bytes, "case %zu: device bytes %zu, recorded %zu", line, dn.off + kSearchDeviceSlack, c.dev_bytes);
    CHECK(pn.off + kSearchPinnedSlack == c.pin_bytes, "case %zu: pinned bytes %zu, recorded %zu", line, pn.off + kSearchPinnedSlack, c.pin_bytes);
    CHECK(!count.d_qf32 && !count.h_q && !count.d_err, "case %zu: the counting walk handed out a pointer", line);
    // a fake block: only addresses are compared, nothing is read or written through them
    uint8_t *const dbase = reinterpret_cast<uint8_t *>(uintptr_t(1) << 40), *const pbase = reinterpret_cast<uint8_t *>(uintptr_t(1) << 41);
    Bufs b{};
    Carver dv(dbase), pv(pbase);
    search_device_layout(dv, c.z, p, b);
    search_pinned_layout(pv, c.z, p, b);
    CHECK(dv.off == dn.off && pv.off == pn.off, "case %zu: the two walks of a layout disagree", line);
    const ChunkShape &z = c.z;
    const size_t nq = (size_t)z.nq, words = nq * 4, total = nq * (size_t)z.nns_stride * 4, out = nq * (size_t)z.count * 4, keys = nq * (size_t)p.kstride * 8;
    const size_t qf = nq * (size_t)z.dims * 4, segs = nq * 16, tl = (size_t)p.max_tiles_bound * 8, vis = (size_t)p.visit_cap * 16, nodes = (size_t)z.n_nodes * 4;
    const size_t nd = walk({{"d_qf32", b.d_qf32, qf}, {"d_qrows", b.d_qrows, words}, {"d_qvecs", b.d_qvecs, nq * pad256(z.row_bytes)},
                            {"d_qhdrs", b.d_qhdrs, nq * 8}, {"d_nns", b.d_nns, total}, {"d_dist", b.d_dist, total}, {"d_counts", b.d_counts, words},
                            {"d_overflow", b.d_overflow, words}, {"d_list", b.d_list, words}, {"d_segs", b.d_segs, segs}, {"d_tiles", b.d_tiles, tl},
                            {"d_ka", b.d_ka, keys}, {"d_kb", b.d_kb, keys}, {"d_oi", b.d_oi, out}, {"d_od", b.d_od, out},
                            {"d_err", b.d_err, kStatusWords * 4}, {"d_unique", b.d_unique, words}, {"d_inv", b.d_inv, (size_t)z.inv_bytes},
                            {"d_visits", b.d_visits, vis}, {"d_sorted", b.d_sorted, vis}, {"d_units", b.d_units, vis},
                            {"d_leaf_count", b.d_leaf_count, nodes + 8}, {"d_cursor", b.d_cursor, nodes}, {"d_ustart", b.d_ustart, nodes},
                            {"d_leaf_sums", b.d_leaf_sums, (size_t)p.n_leaf_sums * 8}, {"d_items", b.d_items, (size_t)p.items_cap * 4},
                            {"d_unit_counts", b.d_unit_counts, words}, {"d_aux", b.d_aux, total}, {"d_q16", b.d_q16, nq * (size_t)z.hpitch * 2},
                            {"d_qstats", b.d_qstats, nq * 16}, {"d_q8", b.d_q8, nq * (size_t)z.pitch8 * 2}, {"d_q8stats", b.d_q8stats, nq * 16},
                            {"d_aux8", b.d_aux8, total}, {"d_slots", b.d_slots, words}, {"d_sks", b.d_sks, words}, {"d_cnt", b.d_cnt, words}},
                           dbase, dv.off, line);
    const size_t np = walk({{"h_q", b.h_q, qf}, {"h_qrows", b.h_qrows, words}, {"h_overflow", b.h_overflow, words}, {"h_list", b.h_list, words},
                            {"h_segs", b.h_segs, segs}, {"h_tiles", b.h_tiles, tl}, {"h_oi", b.h_oi, out}, {"h_od", b.h_od, out},
                            {"h_err", b.h_err, kStatusWords * 4}, {"h_counts", b.h_counts, words}, {"h_slots", b.h_slots, words},
                            {"h_sks", b.h_sks, words}, {"h_cnt", b.h_cnt, words}},
                           pbase, pv.off, line);
    const size_t tiles = p.tiles ? 8 + (p.items_cap != 0) : 0, screen = p.screened ? 2 + (c.z.metric == AH_COSINE) + 3 * p.screened8 : 0;
    CHECK(nd == 17 + (c.z.inv_bytes != 0) + tiles + screen + c.z.mixed + 2 * c.z.varied, "case %zu: %zu device arrays", line, nd);
    CHECK(np == 10 + (size_t)c.z.mixed + 2 * c.z.varied, "case %zu: %zu pinned arrays", line, np);
    const size_t out_pad = pad256(out);
    // the tile path reads ids, distances, status words and unique counts back with one copy of 2 out + 256 + nq * 4 bytes
    CHECK((uint8_t *)b.d_od == (uint8_t *)b.d_oi + out_pad, "case %zu: d_od is not right behind d_oi", line);
    CHECK((uint8_t *)b.d_err == (uint8_t *)b.d_od + out_pad, "case %zu: d_err is not right behind d_od", line);
    CHECK((uint8_t *)b.d_unique == (uint8_t *)b.d_err + pad256(kStatusWords * 4), "case %zu: d_unique is not right behind d_err", line);
    CHECK((uint8_t *)b.h_od == (uint8_t *)b.h_oi + out_pad, "case %zu: h_od is not right behind h_oi", line);
    CHECK((uint8_t *)b.h_err == (uint8_t *)b.h_od + out_pad, "case %zu: h_err is not right behind h_od", line);
    CHECK((uint8_t *)b.h_counts == (uint8_t *)b.h_err + pad256(kStatusWords * 4), "case %zu: h_counts is not right behind h_err", line);
    CHECK((size_t)((uint8_t *)b.h_counts + nq * 4 - pbase) <= c.pin_bytes, "case %zu: the read-back ends beyond the pinned block", line);
    if (c.z.varied) {  // search_k and count of every query go up with one copy of pad256(nq * 4) + nq * 4 bytes
        CHECK((uint8_t *)b.d_cnt == (uint8_t *)b.d_sks + pad256(nq * 4), "case %zu: d_cnt is not right behind d_sks", line);
        CHECK((uint8_t *)b.h_cnt == (uint8_t *)b.h_sks + pad256(nq * 4), "case %zu: h_cnt is not right behind h_sks", line);
    }
}

static size_t replay(const char *path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot open %s", path);
    std::string line;
    size_t n = 0, at = 0;
    while (std::getline(in, line)) {
        at++;
        if (line.empty() || line[0] == '#') continue;
        Case c;
        if (!parse(line, c)) {
            CHECK(false, "line %zu does not parse", at);
            continue;
        }
        n++;
        const ChunkPlan p = plan_chunk(c.z, c.kn);
        const std::vector<long long> gp = {p.big_k, (long long)p.kstride, p.max_tiles_bound, p.heap_cap, p.bitmap_words, p.bitmap_fits, p.hash_fits,
                                           p.tiles, p.visit_cap, p.n_leaf_sums, p.screened, p.screened8, (long long)p.items_cap, p.zero_copy_queries,
                                           p.block_ok, p.small_units, p.fuse_prepare, p.small_first};
        const std::vector<long long> gt = {(long long)p.descent, p.multi_blocks, p.own_units, p.units_per_query, p.single_fused, p.ids_by_tiles,
                                           (long long)p.units, p.small_tiles, (long long)p.tile_launch, p.tile_grid_x, p.tile_grid_y, p.fused_flag,
                                           (long long)p.sel_lds, (long long)p.fused_lds, (long long)p.flagger, p.max_vis8};
        CHECK(gp == c.p, "line %zu: planned [%s], recorded [%s]", at, join(gp).c_str(), join(c.p).c_str());
        CHECK(gt == c.t, "line %zu: tile pass planned [%s], recorded [%s]", at, join(gt).c_str(), join(c.t).c_str());
        check_layouts(c, p, at);
    }
    return n;
}

static void check_thresholds() {
    SearchKnobs kn{};
    kn.wave = true;
    const double below = 0.05 - 1e-12, above = 0.05;
    CHECK(wave_descent_wanted(kn, 32u << 10, false, 0.0), "no filter, a leaf of 32 KiB: the wave descent");
    CHECK(!wave_descent_wanted(kn, (32u << 10) + 256, false, 1.0), "a leaf of 32 KiB + 256 does not fit the wave descent's LDS");
    CHECK(wave_descent_wanted(kn, 1024, true, above) && !wave_descent_wanted(kn, 1024, true, below), "the 5 %% rule");
    CHECK(wave_descent_wanted(kn, 1024, false, below), "the share of no filter does not count");
    kn.wave = false;
    CHECK(!wave_descent_wanted(kn, 1024, false, 1.0), "AH_SEARCH_WAVE=0");
    CHECK(sorted_dedup_kind(true, kSortLds + 1) == SortedDedup::Bitmap, "a bitmap that fits comes first");
    CHECK(sorted_dedup_kind(false, kSortLds) == SortedDedup::SortLds, "kSortLds ids sort in LDS");
    CHECK(sorted_dedup_kind(false, kSortLds + 1) == SortedDedup::SortGlobal, "kSortLds + 1 ids sort in global memory");
    // a row pitch past 8192 floats (no recorded case has one): no wave descent, and the selection's query leaf alone is past
    // the 32 KiB of dynamic LDS it may ask for without the opt-in
    kn.wave = kn.bitmap = kn.tiles = kn.screen = kn.fused_flag = true;
    kn.small_units_max_queries = kn.block_max_queries = 64, kn.small_tiles_max_queries = 8;
    ChunkShape z{};
    z.nq = 1, z.count = 10, z.search_k = 400, z.nns_stride = 464, z.by_vector = z.allow8 = z.screen_ready = z.batch_count = true;
    z.n_nodes = 100, z.n_trees = 3, z.n_leaves = 50, z.desc_len = 6000, z.max_desc = 64, z.metric = AH_COSINE;
    z.dims = 8200, z.pitch = z.hpitch = z.pitch8 = 8256, z.row_bytes = 8256 * 4, z.n = 2000, z.max_id = 1999;
    z.tile_candidates = 512, z.kstride_batch = 4096, z.kstride_single = 4100;
    z.wave_descent = wave_descent_wanted(kn, pad256(z.row_bytes), false, 1.0);
    const ChunkPlan p = plan_chunk(z, kn);
    CHECK(!z.wave_descent && p.tiles && p.screened && p.descent == Descent::Octet && p.units == UnitBuilder::UnitsSmall, "the wide row's tile pass");
    CHECK(p.sel_lds == 8256 * 4 && p.sel_lds > (32u << 10) && p.fused_flag && p.fused_lds == p.sel_lds + 1024 * 4, "the wide row's selection");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s search_plan_cases.txt\n", argv[0]);
        return 2;
    }
    check_thresholds();
    const size_t n = replay(argv[1]);
    CHECK(n >= 250, "only %zu recorded sub-batches", n);
    if (failures) return 1;
    printf("every sub-batch planned as recorded (%zu)\n", n);
    return 0;
}
