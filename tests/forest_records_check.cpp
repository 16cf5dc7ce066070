// The host side of a forest-build batch (arroy_amd/csrc/forest_records.h) with no device: a small command interpreter that
// tests/test_forest_records_cpu.py drives with synthetic forests (random trees of counts, laid out level by level as
// k_next_emit writes them), ring traffic, group cuts and batch shapes, and whose printed output the test compares with its
// own restatement.  Built with ASan and UBSan.  Commands (one per line, whitespace-separated; results on stdout):
//   sizeof                                               sizes of the shared PODs
//   sizes N n_trees M split_after nstride hstride stride8 rows bits readback_mb
//   cuts n_trees groups ratio_percent
//   ring cap  |  alloc bytes  |  retire                   a TableRing: offsets, "noroom", the head after every step
//   forest n_trees first_tree split_after streaming id_base nstride node_base desc_base roots_base, then the tree bases
//          (n_trees + 1) and the tree seeds (n_trees) on the next two lines: the roots
//   table depth n_nodes chunk_off rec_full rec_off threads fork_parent dump, then n_nodes lines
//          "tree start count n_left attempt state": one digest
//   swapfull | wrap n_nodes | grow level_nodes k n_1 .. n_k | recs | emit tA tB threads | nodes | leaves tA tB threads
#include "../arroy_amd/csrc/forest_records.h"
#include "../include/arroy_hip.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

using namespace ah;

struct Forest {
    BatchRecords rec;
    std::vector<ah_node> nodes;
    std::vector<uint32_t> roots;
    size_t roots_base = 0;
    uint64_t desc_base = 0;
};

static void print_stream_node(const char *tag, const ah_stream_node &n) {
    printf("%s %u %u %u %u %u %u %u %u %" PRIu64 "\n", tag, n.id, n.tree, (unsigned)n.kind, (unsigned)n.has_normal, n.left, n.right, n.count,
           n.depth, (uint64_t)n.payload_offset);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::unique_ptr<Forest> f;
    TableRing ring;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string cmd;
        if (!(ls >> cmd)) continue;
        if (cmd == "sizeof") {
            printf("sizeof %zu %zu %zu %zu %zu\n", sizeof(FNode), sizeof(FTile), sizeof(NextCounts), sizeof(LevelInfo), sizeof(NormalStats8));
        } else if (cmd == "sizes") {
            uint64_t N, M, nstride, hstride, stride8;
            uint32_t n_trees, split_after;
            int rows, bits;
            long long mb;
            ls >> N >> n_trees >> M >> split_after >> nstride >> hstride >> stride8 >> rows >> bits >> mb;
            const BatchSizes z = batch_sizes(N, n_trees, M, split_after, nstride, hstride, stride8, rows != 0, bits != 0, mb);
            printf("sizes %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                   " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu %zu %zu %zu %zu %zu\n",
                   z.max_nodes, z.max_tiles, z.perm, z.nodes, z.tiles, z.masks, z.tile_left, z.child, z.block_sums, z.node_of, z.side_bytes,
                   z.side_bits, z.arena_block, z.shadow_block, z.shadow8_block, z.info_words, z.pin_info, z.pin_nodes, z.pin_head, z.bounce,
                   z.pinned_bytes());
        } else if (cmd == "cuts") {
            uint32_t n_trees, groups;
            long long ratio;
            ls >> n_trees >> groups >> ratio;
            printf("cuts");
            for (uint32_t c : tail_group_trees(n_trees, groups, ratio)) printf(" %u", c);
            printf("\n");
        } else if (cmd == "ring") {
            ring = TableRing{};
            ls >> ring.cap;
        } else if (cmd == "alloc") {
            size_t bytes, off = 0;
            ls >> bytes;
            const size_t head_before = ring.head, live_before = ring.tables.size();
            if (ring.alloc(bytes, &off)) {
                PendingTable e{};
                e.ring_off = off;
                e.n_nodes = (uint32_t)bytes;  // (the interpreter's own use: the bytes of the range)
                ring.tables.push_back(e);
                printf("off %zu head %zu\n", off, ring.head);
            } else {
                printf("noroom %s\n", ring.head == head_before && ring.tables.size() == live_before ? "unchanged" : "CHANGED");
            }
        } else if (cmd == "retire") {
            if (ring.tables.empty()) {
                printf("retire empty\n");
            } else {
                printf("retire %zu\n", ring.tables.front().ring_off);
                ring.tables.pop_front();
            }
        } else if (cmd == "forest") {
            uint32_t n_trees, first_tree, split_after, id_base;
            int streaming;
            uint64_t nstride, desc_base;
            size_t node_base, roots_base;
            ls >> n_trees >> first_tree >> split_after >> streaming >> id_base >> nstride >> node_base >> desc_base >> roots_base;
            std::vector<uint64_t> bases(n_trees + 1), seeds(n_trees);
            for (auto &b : bases) in >> b;
            for (auto &s : seeds) in >> s;
            f.reset(new Forest());
            f->roots_base = roots_base, f->desc_base = desc_base;
            f->nodes.resize(node_base);
            f->roots.resize(roots_base);
            f->rec.init(n_trees, first_tree, split_after, streaming != 0, id_base, nstride, node_base);
            f->rec.reserve(bases[n_trees] / (split_after + 1) + n_trees);
            std::vector<FNode> lv(n_trees);
            std::vector<uint32_t> tree_first(n_trees + 1, 0xFFFFFFFFu);
            LevelInfo info{};
            f->rec.seed_roots(bases.data(), seeds.data(), lv.data(), &info, tree_first.data());
            printf("info %u %u %u %llu\n", info.n_nodes, info.n_tiles, info.n_fix, info.pairs);
            for (uint32_t i = 0; i < info.n_nodes; i++)
                printf("root %u %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u %u %u\n", i, lv[i].key, lv[i].start, lv[i].tree, lv[i].count, lv[i].n_left,
                       lv[i].attempt, lv[i].state, lv[i].tile_begin, lv[i].n_tiles, lv[i].fix);
            printf("tree_first");
            for (uint32_t t : tree_first) printf(" %u", t);
            printf("\n");
        } else if (!f) {
            fprintf(stderr, "command %s before a forest\n", cmd.c_str());
            return 2;
        } else if (cmd == "table") {
            uint32_t depth, n_nodes, threads;
            uint64_t chunk_off;
            int rec_full, fork_parent, dump;
            size_t rec_off;
            ls >> depth >> n_nodes >> chunk_off >> rec_full >> rec_off >> threads >> fork_parent >> dump;
            std::vector<FNode> tbl(n_nodes);
            for (FNode &nd : tbl) {
                nd = FNode{};
                in >> nd.tree >> nd.start >> nd.count >> nd.n_left >> nd.attempt >> nd.state;
            }
            std::vector<ah_stream_node> sn(f->rec.streaming ? n_nodes : 0);
            const uint32_t *rec_of = rec_full ? f->rec.level_rec_full.data() + rec_off : f->rec.level_rec.data();
            const DigestResult r = f->rec.digest_level(depth, n_nodes, tbl.data(), chunk_off, rec_of, threads, f->rec.streaming ? sn.data() : nullptr);
            if (fork_parent) f->rec.level_rec_full.swap(f->rec.level_rec);
            printf("digest %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u n_recs %zu routed %" PRIu64 "\n", r.evals, r.retries, r.dummies, r.routed,
                   r.bad, f->rec.n_recs, f->rec.items_routed);
            if (r.bad == 0xFFFFFFFFu && dump) {
                for (const ah_stream_node &n : sn) print_stream_node("sn", n);
                printf("next");
                for (uint32_t v : (fork_parent ? f->rec.level_rec_full : f->rec.level_rec)) printf(" %u", v);
                printf("\n");
            }
        } else if (cmd == "swapfull") {
            f->rec.level_rec_full.swap(f->rec.level_rec);
        } else if (cmd == "wrap") {
            uint32_t n_nodes;
            ls >> n_nodes;
            printf("wrap %d\n", f->rec.stream_ids_wrap(n_nodes) ? 1 : 0);
        } else if (cmd == "grow") {
            uint32_t level_nodes, k;
            ls >> level_nodes >> k;
            std::deque<PendingTable> pending(k);
            for (PendingTable &e : pending) ls >> e.n_nodes;
            f->rec.grow_ahead(level_nodes, pending);
            printf("grow %zu n_recs %zu\n", f->rec.recs.size(), f->rec.n_recs);
        } else if (cmd == "recs") {
            for (size_t i = 0; i < f->rec.n_recs; i++) {
                const HostRec &r = f->rec.recs[i];
                printf("rec %zu %u %u %u %u %u %" PRIu64 " %u %u %" PRIu64 "\n", i, (unsigned)r.kind, (unsigned)r.has_normal, r.tree, r.left, r.right,
                       r.start, r.count, r.depth, r.normal_off);
            }
            printf("tree_count");
            for (uint64_t c : f->rec.tree_count) printf(" %" PRIu64, c);
            printf("\ntree_root");
            for (uint32_t c : f->rec.tree_root) printf(" %u", c);
            printf("\n");
        } else if (cmd == "emit") {
            uint32_t tA, tB;
            unsigned threads;
            ls >> tA >> tB >> threads;
            const bool ok = f->rec.emit_range(tA, tB, threads, f->nodes, f->roots, f->roots_base, f->desc_base);
            printf("emit %s cursor %zu tree %u\n", ok ? "ok" : "refused", f->rec.emit_cursor, f->rec.emit_tree);
        } else if (cmd == "nodes") {
            for (size_t i = f->rec.node_base; i < f->nodes.size(); i++) {
                const ah_node &n = f->nodes[i];
                printf("node %zu %u %u %u %u %u %" PRIu64 " %u %u\n", i, (unsigned)n.kind, (unsigned)n.has_normal, n.tree, n.left, n.right,
                       (uint64_t)n.offset, n.count, n.depth);
            }
            printf("roots");
            for (size_t i = f->roots_base; i < f->roots.size(); i++) printf(" %u", f->roots[i]);
            printf("\ncounts %" PRIu64 " %" PRIu64 "\n", f->rec.n_split, f->rec.n_desc);
        } else if (cmd == "leaves") {
            uint32_t tA, tB;
            unsigned threads;
            ls >> tA >> tB >> threads;
            std::vector<ah_stream_node> out;
            f->rec.leaves_of(tA, tB, threads, out);
            printf("leaves %zu\n", out.size());
            for (const ah_stream_node &n : out) print_stream_node("leaf", n);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    printf("done\n");
    return 0;
}
