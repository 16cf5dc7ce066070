// The per-level plan of the forest build (arroy_amd/csrc/level_plan.h) on the host, no device: the width rule of the last
// tree group against its table, plan_level against the levels recorded from the build before the plan was one function
// (tests/golden/level_plan_cases.txt: shape, tunables, first node of every tree -> decisions, best_cost as a hex float), and
// the uniform 10M x 768 x 100-tree ladder DESIGN.md names.  Built by tests/test_level_plan_cpu.py with ASan and UBSan.
#include "../arroy_amd/csrc/level_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

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

static std::string widths_of(const std::vector<RowsLaunch> &l) {
    std::string out;
    for (const RowsLaunch &e : l) out += (out.empty() ? "" : ",") + std::to_string(e.tcv) + "x" + std::to_string(e.groups) + "/" + std::to_string(e.np);
    return out;
}

// a. the rule of the last trees: widths for rem = 1 .. tc - 1
static void check_tail_widths() {
    const uint32_t w2[] = {2}, w4[] = {2, 2, 4}, w8[] = {2, 2, 4, 4, 4, 4, 8}, w16[] = {2, 2, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8, 16, 16, 16};
    const struct {
        uint32_t tc;
        const uint32_t *want;
    } tables[] = {{2, w2}, {4, w4}, {8, w8}, {16, w16}};
    for (const auto &t : tables)
        for (uint32_t rem = 1; rem < t.tc; rem++)
            CHECK(tail_group_width(t.tc, rem) == t.want[rem - 1], "tail_group_width(%u, %u) = %u, table says %u", t.tc, rem,
                  tail_group_width(t.tc, rem), t.want[rem - 1]);
    // launch lists at tc = 16: width x groups / trees in each
    const struct {
        uint32_t trees;
        const char *want;
    } lists[] = {{13, "16x1/13"}, {12, "8x1/8,4x1/4"}, {7, "8x1/7"}, {3, "4x1/3"}, {1, "2x1/1"}, {100, "16x6/16,4x1/4"}, {16, "16x1/16"}};
    for (const auto &l : lists) {
        const std::string got = widths_of(rows_launch_list(l.trees, 16, false));
        CHECK(got == l.want, "launch list of %u trees at tc 16: %s, expected %s", l.trees, got.c_str(), l.want);
    }
    // the trees of a list are consecutive and complete; LDS groups keep their width
    for (uint32_t tc = 2; tc <= 16; tc <<= 1)
        for (uint32_t trees = 1; trees <= 130; trees++)
            for (int lds = 0; lds < 2; lds++) {
                uint32_t at = 0;
                for (const RowsLaunch &e : rows_launch_list(trees, tc, lds != 0)) {
                    CHECK(e.t0 == at && e.np >= 1 && e.np <= e.tcv && e.tcv <= tc && (e.groups == 1 || e.np == e.tcv), "list of %u trees at tc %u", trees, tc);
                    CHECK(!lds || e.tcv == tc, "an LDS group of %u trees at tc %u changed its width", trees, tc);
                    at += (e.groups - 1) * e.tcv + e.np;
                }
                CHECK(at == trees, "list of %u trees at tc %u covers %u", trees, tc, at);
            }
}

// b. the recorded levels
static int check_recorded(const char *path) {
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", path);
        return -1;
    }
    int n = 0, autos = 0, forks = 0, lds = 0, dense = 0, unfit = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tag, tok;
        LevelShape sh{};
        LevelKnobs k{};
        unsigned long long N, pairs, rec_bytes, row_bytes, tail_min;
        int screen, screen8, lo, allowed, prev, grouped, fork_now, subset, legal, adv, rlds;
        auto hexf = [&ss]() {
            std::string t;
            ss >> t;
            return strtod(t.c_str(), nullptr);
        };
        ss >> tag >> N >> sh.n_trees >> sh.n_nodes >> pairs >> sh.split_after >> rec_bytes >> row_bytes >> sh.hpitch >> sh.metric >> screen >>
            screen8 >> lo;
        sh.screen8_quality = hexf();
        ss >> allowed >> prev >> grouped >> fork_now >> subset >> sh.mode_req >> legal;
        if (tag != "L" || !ss) {
            fprintf(stderr, "bad line %d\n", n + 1);
            return -1;
        }
        sh.N = N, sh.pairs = pairs, sh.rec_bytes = rec_bytes, sh.row_bytes = row_bytes;
        sh.screen = screen, sh.screen8 = screen8, sh.rows8_lo = lo, sh.rows_allowed = allowed, sh.prev_rows = prev, sh.grouped = grouped;
        sh.fork_now = fork_now, sh.subset = subset, sh.dense_grid_legal = legal;
        ss >> tag >> k.rows_force >> k.dense >> adv >> rlds >> k.rows_max_tc;
        k.rows_cache_mb = hexf();
        ss >> k.dense_max_cols;
        k.dense_gmacs = hexf();
        ss >> k.tail_groups;
        k.tail_node_items = hexf();
        ss >> tail_min >> tok;
        if (tag != "K" || tok != "T" || !ss) {
            fprintf(stderr, "bad line %d\n", n + 1);
            return -1;
        }
        k.rows_advance = adv, k.rows_lds = rlds, k.tail_min_items = tail_min;
        std::vector<uint32_t> tf(sh.n_trees + 1);
        for (uint32_t &v : tf) ss >> v;
        sh.tree_first = tf.data();
        uint32_t row_tc, lds_tc, lds_worst;
        int want_dense, want_fork;
        ss >> tag >> row_tc >> lds_tc >> lds_worst >> want_dense >> want_fork;
        const double best_cost = hexf();
        if (tag != "R" || !ss) {
            fprintf(stderr, "bad line %d\n", n + 1);
            return -1;
        }
        const LevelPlan p = plan_level(sh, k);
        n++;
        CHECK(p.row_tc == row_tc && p.lds_tc == lds_tc && p.lds_worst == lds_worst && (int)p.dense == want_dense && (int)p.fork == want_fork &&
                  memcmp(&p.best_cost, &best_cost, sizeof best_cost) == 0,
              "recorded level %d: row_tc %u lds_tc %u lds_worst %u dense %d fork %d best_cost %a, recorded %u %u %u %d %d %a", n, p.row_tc, p.lds_tc,
              p.lds_worst, (int)p.dense, (int)p.fork, p.best_cost, row_tc, lds_tc, lds_worst, want_dense, want_fork, best_cost);
        // the launches are those of the mode, over every tree once
        uint32_t trees = 0;
        for (const RowsLaunch &l : p.launches) trees += (l.groups - 1) * l.tcv + l.np;
        CHECK(p.launches.empty() == (p.fork || p.dense || p.row_tc < 2) && (p.launches.empty() || trees == sh.n_trees), "recorded level %d: launches", n);
        autos += best_cost >= 0, forks += want_fork, lds += lds_tc != 0, dense += want_dense;
        unfit += (sh.mode_req & 0x100u) && !grouped && allowed && (rec_bytes & 15) == 0 && lds_tc == 0;
    }
    printf("%d recorded levels reproduced (%d priced by the model, %d dense, %d LDS-resident, %d forced LDS that did not fit, %d handed back)\n", n,
           autos, dense, lds, unfit, forks);
    CHECK(n >= 500 && autos >= 50 && forks >= 1 && lds >= 50 && dense >= 50 && unfit >= 1, "the recorded cases no longer cover every decision");
    return 0;
}

// c. the uniform ladder of DESIGN.md ("Margin mode of a level"): 10M x 768, 100 trees, level L = 100 * 2^L nodes, 10^9 pairs,
// screened with the int8 stage and its second digit, quality 0.12 (uniform rows); the default tunables, as every recorded
// default build carries them.  Dense on levels 0-5, row-major with TC 16 / 16 / 8 / 4 on 6-9 (recorded by running the build's
// own decision code of commit 79a367e on these shapes), node-major from 10.
static void check_ladder() {
    LevelKnobs k{};
    k.rows_force = -1, k.dense = -1, k.rows_advance = true, k.rows_lds = true, k.rows_max_tc = 16, k.rows_cache_mb = -1.0;
    k.dense_max_cols = 16384, k.dense_gmacs = 495000.0, k.tail_groups = 0;
    const uint32_t want_tc[15] = {16, 16, 16, 16, 16, 16, 16, 16, 8, 4, 0, 0, 0, 0, 0};
    const char *want_list[15] = {"", "", "", "", "", "", "16x6/16,4x1/4", "16x6/16,4x1/4", "8x12/8,4x1/4", "4x25/4", "", "", "", "", ""};
    bool prev = false;
    for (uint32_t L = 0; L < 15; L++) {
        LevelShape sh{};
        sh.N = 10000000, sh.n_trees = 100, sh.n_nodes = 100u << L, sh.pairs = 1000000000ull;
        sh.rec_bytes = 1664, sh.row_bytes = 3072, sh.hpitch = 768, sh.metric = 2;
        sh.screen = sh.screen8 = sh.rows8_lo = true, sh.screen8_quality = 0.12;
        sh.rows_allowed = true, sh.prev_rows = prev, sh.dense_grid_legal = true;
        std::vector<uint32_t> tf(101);
        for (uint32_t t = 0; t <= 100; t++) tf[t] = t << L;
        sh.tree_first = tf.data();
        const LevelPlan p = plan_level(sh, k);
        CHECK(p.dense == (L <= 5) && p.row_tc == want_tc[L] && p.lds_tc == 0 && !p.fork && widths_of(p.launches) == want_list[L],
              "ladder level %u: dense %d row_tc %u launches %s", L, (int)p.dense, p.row_tc, widths_of(p.launches).c_str());
        prev = p.row_tc >= 2;
    }
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: level_plan_check <recorded cases>\n");
        return 2;
    }
    check_tail_widths();
    if (check_recorded(argv[1]) != 0) return 2;
    check_ladder();
    if (failures) return 1;
    printf("every level planned as recorded\n");
    return 0;
}
