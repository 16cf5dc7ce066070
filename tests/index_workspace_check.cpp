// The workspace layouts of the index maintenance calls (arroy_amd/csrc/index_workspace.h) on the host alone, no device call:
// for a few sizes, 0 and 1 included, every array of every layout lies inside its block, no two overlap, the arrays are carved
// in the order the kernels were written for, and the block and its zeroed part are as long as the formulas the calls used
// before the layouts were written down once.  Built with -fsanitize=address,undefined by test_index_workspace_cpu.py; the
// block is a real host allocation of bytes() bytes and every array is filled, so a layout that outgrows its block is a
// heap-buffer-overflow report as well.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../arroy_amd/csrc/index_workspace.h"

using namespace ah;

namespace {

constexpr uint32_t kScanTile = 256 * 16;  // scan_device.h
// words of the control blocks and records: the enums and structs of index_update.hip / index_audit.hip
constexpr size_t CTL_WORDS = 8, ICTL_WORDS = 7, GCTL_WORDS = 5, CCTL_WORDS = 4;
constexpr size_t kAuditClasses = 10;
constexpr size_t kAuditCtlBytes = 8 * kAuditClasses + 16 + 8 + 4 * kAuditClasses + 16, kTreeWordsBytes = 16;

// the argument structs of the kernels, reduced to what the layouts carve
struct DeleteArgs {
    uint32_t *order, *rep, *cnt, *flags, *own, *seg, *chg, *dseg, *cursor, *merged, *ctl;
};
struct InsertArgs {
    uint32_t *cnt, *seg, *cursor, *chg, *fresh, *nlen, *dlen, *touched, *landed, *ctl;
};
struct Node4 {
    uint32_t kind, a, b, c;
};
struct GraftArgs {
    uint32_t *named, *pos_of_rank, *new_of_old, *replaced, *fin, *len, *ctl;
};
struct CompactArgs {
    uint32_t *new_index, *new_row, *ctl;
};
struct AuditArgs {
    uint32_t *owner, *links, *order;
    unsigned char *tree;               // TreeWords
    unsigned long long *tree_items;
    unsigned char *ctl;                // AuditCtl
};

int failures = 0;

// an array as the caller sees it after carve(): where it starts, how many bytes the kernels may write
struct Span {
    const char *name;
    void *p;
    size_t bytes;
};

// the block of `ws` allocated, carved into `spans` by `get` (called after the carve), every span written, and checked
template <class Get>
void check(const char *what, const Workspace &ws, size_t want_bytes, size_t want_zeroed, Get get) {
    if (ws.bytes() != want_bytes || ws.zeroed_bytes() != want_zeroed) {
        fprintf(stderr, "%s: %zu bytes (%zu zeroed), the call's formula gives %zu (%zu)\n", what, ws.bytes(), ws.zeroed_bytes(), want_bytes, want_zeroed);
        failures++;
    }
    unsigned char *block = static_cast<unsigned char *>(malloc(std::max<size_t>(ws.bytes(), 1)));
    ws.carve(block, ws.bytes());
    const std::vector<Span> spans = get();
    const unsigned char *at = block;  // the arrays follow each other without a gap, in the order listed
    for (const Span &s : spans) {
        if (s.p != at) {
            fprintf(stderr, "%s: %s starts at byte %td, not at %td\n", what, s.name, static_cast<unsigned char *>(s.p) - block, at - block);
            failures++;
        }
        memset(s.p, 0xA5, s.bytes);
        at = static_cast<unsigned char *>(s.p) + s.bytes;
    }
    if (at != block + ws.bytes()) {
        fprintf(stderr, "%s: the arrays end at byte %td of %zu\n", what, at - block, ws.bytes());
        failures++;
    }
    free(block);
}

void one(uint32_t nn, uint32_t n_trees, size_t n, uint32_t n_view) {
    char what[128];
    const size_t per_node = (size_t)nn + 1;
    const size_t scan_tiles = (nn + kScanTile - 1) / kScanTile + 1;
    {
        snprintf(what, sizeof what, "delete(n_nodes %u)", nn);
        DeleteArgs a{};
        uint32_t *tiles = nullptr;
        const Workspace ws = delete_workspace(a, &tiles, nn, kScanTile, CTL_WORDS);
        const size_t work_words = 10 * per_node + scan_tiles + CTL_WORDS;  // delete_impl
        check(what, ws, work_words * 4, work_words * 4, [&] {
            return std::vector<Span>{{"order", a.order, per_node * 4}, {"rep", a.rep, per_node * 4}, {"cnt", a.cnt, per_node * 4},
                                     {"flags", a.flags, per_node * 4}, {"own", a.own, per_node * 4}, {"seg", a.seg, per_node * 4},
                                     {"chg", a.chg, per_node * 4}, {"dseg", a.dseg, per_node * 4}, {"cursor", a.cursor, per_node * 4},
                                     {"merged", a.merged, per_node * 4}, {"tile_sums", tiles, scan_tiles * 4}, {"ctl", a.ctl, CTL_WORDS * 4}};
        });
    }
    {
        snprintf(what, sizeof what, "insert(n_nodes %u, n_trees %u, n %zu)", nn, n_trees, n);
        InsertArgs a{};
        uint64_t *seeds = nullptr;
        uint32_t *tiles = nullptr, *ids = nullptr, *leaf = nullptr;
        const Workspace ws = insert_workspace(a, &seeds, &tiles, &ids, &leaf, nn, n_trees, n, kScanTile, ICTL_WORDS);
        const size_t pairs = n * n_trees, seed_words = 2 * (size_t)n_trees;
        const size_t work_words = 8 * per_node + scan_tiles + ICTL_WORDS + seed_words + n + 2 * pairs;  // insert_impl
        check(what, ws, work_words * 4, (8 * per_node + scan_tiles + ICTL_WORDS) * 4, [&] {
            return std::vector<Span>{{"seeds", seeds, (size_t)n_trees * 8}, {"cnt", a.cnt, per_node * 4}, {"seg", a.seg, per_node * 4},
                                     {"cursor", a.cursor, per_node * 4}, {"chg", a.chg, per_node * 4}, {"fresh", a.fresh, per_node * 4},
                                     {"nlen", a.nlen, per_node * 4}, {"dlen", a.dlen, per_node * 4}, {"touched", a.touched, per_node * 4},
                                     {"tile_sums", tiles, scan_tiles * 4}, {"ctl", a.ctl, ICTL_WORDS * 4}, {"ids", ids, n * 4},
                                     {"leaf", leaf, pairs * 4}, {"landed", a.landed, pairs * 4}};
        });
    }
    for (uint32_t n_repl : {0u, 1u}) {
        // a graft of a view of n_view nodes and n_trees trees: n_repl roots replace a node, the others are new roots
        if (n_repl > n_trees || n_repl > nn || (n_view == 0 && n_trees)) continue;
        const uint32_t n_old = nn, n_used = nn - nn / 3, n_added = n_trees - n_repl, n_new = n_used + n_view - n_repl;
        const uint64_t vdesc = 3 * (uint64_t)n_view + 1;
        snprintf(what, sizeof what, "graft(n_old %u, n_used %u, n_view %u, %u replacing + %u new roots)", n_old, n_used, n_view, n_repl, n_added);
        GraftArgs a{};
        uint32_t *tiles = nullptr;
        GraftUploads<Node4> u{};
        const Workspace ws = graft_workspace(a, &tiles, u, GraftSizes{n_old, n_used, n_view, n_new, n_repl, n_added, vdesc}, kScanTile, GCTL_WORDS);
        const size_t g_tiles = ((size_t)n_new + kScanTile - 1) / kScanTile + 1;  // graft_impl
        const size_t zeroed = 2 * ((size_t)n_new + 1) + n_used + 2 * (size_t)n_old + n_view + g_tiles + GCTL_WORDS;
        const size_t words = zeroed + 2 * (size_t)n_view + 2 * (size_t)n_repl + n_added + vdesc + 4 * (size_t)n_view;
        check(what, ws, words * 4, zeroed * 4, [&] {
            return std::vector<Span>{{"named", a.named, ((size_t)n_new + 1) * 4}, {"len", a.len, ((size_t)n_new + 1) * 4},
                                     {"pos_of_rank", a.pos_of_rank, (size_t)n_used * 4}, {"new_of_old", a.new_of_old, (size_t)n_old * 4},
                                     {"replaced", a.replaced, (size_t)n_old * 4}, {"fin", a.fin, (size_t)n_view * 4},
                                     {"tile_sums", tiles, g_tiles * 4}, {"ctl", a.ctl, GCTL_WORDS * 4}, {"vfin", u.vfin, (size_t)n_view * 4},
                                     {"vtgt", u.vtgt, (size_t)n_view * 4}, {"repl", u.repl, (size_t)n_repl * 4}, {"kinds", u.kinds, (size_t)n_repl * 4},
                                     {"added", u.added, (size_t)n_added * 4}, {"vdesc", u.vdesc, (size_t)vdesc * 4},
                                     {"vnodes", u.vnodes, (size_t)n_view * sizeof(Node4)}};
        });
    }
    for (size_t extra_words : {(size_t)0, (size_t)nn}) {
        snprintf(what, sizeof what, "compact(n_nodes %u, %zu extra words)", nn, extra_words);
        CompactArgs a{};
        uint32_t *tiles = nullptr, *extra = nullptr;
        const Workspace ws = compact_workspace(a, &tiles, &extra, nn, extra_words, kScanTile, CCTL_WORDS);
        const size_t bytes = (2 * per_node + scan_tiles + CCTL_WORDS + extra_words) * 4;  // compact_count
        check(what, ws, bytes, bytes, [&] {
            return std::vector<Span>{{"new_index", a.new_index, per_node * 4}, {"new_row", a.new_row, per_node * 4}, {"tile_sums", tiles, scan_tiles * 4},
                                     {"ctl", a.ctl, CCTL_WORDS * 4}, {"extra", extra, extra_words * 4}};
        });
    }
    {
        snprintf(what, sizeof what, "audit(n_nodes %u, n_trees %u)", nn, n_trees);
        AuditArgs a{};
        const Workspace ws = audit_workspace(a, nn, n_trees, kAuditCtlBytes / 4, kTreeWordsBytes / 4);
        const size_t tree_bytes = (size_t)n_trees * (kTreeWordsBytes + 8);  // audit_run
        const size_t work_bytes = kAuditCtlBytes + tree_bytes + 3 * (size_t)nn * 4;
        check(what, ws, work_bytes, work_bytes, [&] {
            return std::vector<Span>{{"ctl", a.ctl, kAuditCtlBytes}, {"tree_items", a.tree_items, (size_t)n_trees * 8},
                                     {"tree", a.tree, (size_t)n_trees * kTreeWordsBytes}, {"owner", a.owner, (size_t)nn * 4},
                                     {"links", a.links, (size_t)nn * 4}, {"order", a.order, (size_t)nn * 4}};
        });
        if (reinterpret_cast<uintptr_t>(a.tree_items) % 8 != 0) {
            fprintf(stderr, "%s: the 8-byte counters start on an odd word\n", what);
            failures++;
        }
    }
}

}  // namespace

int main() {
    // (n_nodes, n_trees, n, n_view): nothing at all, one of each, around one scan tile, several tiles
    const uint32_t nodes[] = {0, 1, 2, 4095, 4096, 4097, 20001};
    const uint32_t trees[] = {0, 1, 3};
    const size_t ids[] = {0, 1, 1000};
    const uint32_t views[] = {0, 1, 5, 5000};
    int cases = 0;
    for (uint32_t nn : nodes)
        for (uint32_t nt : trees)
            for (size_t n : ids)
                for (uint32_t nv : views) {
                    one(nn, nt, n, nv);
                    cases++;
                }
    if (failures) {
        fprintf(stderr, "%d layout check(s) failed\n", failures);
        return 1;
    }
    printf("index workspaces: %d size tuples, every layout inside its block\n", cases);
    return 0;
}
