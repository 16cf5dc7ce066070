// The workspace layout of ah_index_drop_trees (drop_workspace, arroy_amd/csrc/index_workspace.h) on the host alone, no device
// call: for node counts from 0 up across a scan-tile boundary and a few numbers of dropped roots, every array lies inside the
// block, no two overlap, they are carved in the order drop_impl (index_update.hip) expects, and the block and its zeroed part
// are as long as the call's arithmetic says.  Built with -fsanitize=address,undefined by test_index_drop_cpu.py; the block is a
// real host allocation of bytes() bytes and every array is filled, so a layout that outgrows its block is a
// heap-buffer-overflow report as well.  (The other five layouts: index_workspace_check.cpp.)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../arroy_amd/csrc/index_workspace.h"

using namespace ah;

namespace {

constexpr uint32_t kScanTile = 256 * 16;  // scan_device.h
constexpr size_t DCTL_WORDS = 6;          // enum DCtl of index_update.hip

// the argument struct of the kernels, reduced to what the layout carves
struct DropArgs {
    uint32_t *order, *dropped, *len, *rpos, *ctl;
};

struct Span {
    const char *name;
    uint32_t *p;
    size_t words;
};

int failures = 0;

void one(uint32_t nn, uint32_t n_drop) {
    const size_t per_node = (size_t)nn + 1;
    const size_t scan_tiles = ((size_t)nn + kScanTile - 1) / kScanTile + 1;
    const size_t zeroed_words = 4 * per_node + scan_tiles + DCTL_WORDS, words = zeroed_words + n_drop;  // drop_impl
    DropArgs a{};
    uint32_t *tiles = nullptr, *seed_roots = nullptr;
    const Workspace ws = drop_workspace(a, &tiles, &seed_roots, nn, n_drop, kScanTile, DCTL_WORDS);
    if (ws.bytes() != words * 4 || ws.zeroed_bytes() != zeroed_words * 4) {
        fprintf(stderr, "drop(n_nodes %u, n_drop %u): %zu bytes (%zu zeroed), the call's arithmetic gives %zu (%zu)\n", nn, n_drop, ws.bytes(),
                ws.zeroed_bytes(), words * 4, zeroed_words * 4);
        failures++;
    }
    uint32_t *block = static_cast<uint32_t *>(malloc(std::max<size_t>(ws.bytes(), 1)));
    ws.carve(block, ws.bytes());
    const std::vector<Span> spans = {{"order", a.order, per_node}, {"dropped", a.dropped, per_node}, {"len", a.len, per_node},
                                     {"rpos", a.rpos, per_node},   {"tile_sums", tiles, scan_tiles},  {"ctl", a.ctl, DCTL_WORDS},
                                     {"seed_roots", seed_roots, n_drop}};
    const uint32_t *at = block;  // the arrays follow each other without a gap, in the order listed
    uint32_t tag = 1;
    for (const Span &s : spans) {
        if (s.p != at) {
            fprintf(stderr, "drop(n_nodes %u, n_drop %u): %s starts at word %td, not at %td\n", nn, n_drop, s.name, s.p - block, at - block);
            failures++;
        }
        for (size_t i = 0; i < s.words; i++) s.p[i] = tag;
        at = s.p + s.words;
        tag++;
    }
    if (at != block + words) {
        fprintf(stderr, "drop(n_nodes %u, n_drop %u): the arrays end at word %td of %zu\n", nn, n_drop, at - block, words);
        failures++;
    }
    // what was written into one array is still there after the others were filled
    tag = 1;
    for (const Span &s : spans) {
        for (size_t i = 0; i < s.words; i++)
            if (s.p[i] != tag) {
                fprintf(stderr, "drop(n_nodes %u, n_drop %u): %s[%zu] was overwritten\n", nn, n_drop, s.name, i);
                failures++;
                break;
            }
        tag++;
    }
    free(block);
}

}  // namespace

int main() {
    int cases = 0;
    // every node count from 0 across the first scan-tile boundary, then around the second and well past it
    std::vector<uint32_t> nodes;
    for (uint32_t nn = 0; nn <= kScanTile + 2; nn++) nodes.push_back(nn);
    for (uint32_t nn : {2 * kScanTile - 1, 2 * kScanTile, 2 * kScanTile + 1, 20001u}) nodes.push_back(nn);
    for (uint32_t nn : nodes)
        for (uint32_t n_drop : {0u, 1u, 3u, 1000u}) {
            if (n_drop > nn) continue;  // (a dropped root is a node)
            one(nn, n_drop);
            cases++;
        }
    if (failures) {
        fprintf(stderr, "%d layout check(s) failed\n", failures);
        return 1;
    }
    printf("drop workspace: %d size pairs, every array inside its block\n", cases);
    return 0;
}
