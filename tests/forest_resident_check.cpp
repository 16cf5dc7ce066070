// The host side of a resident forest (arroy_amd/csrc/forest_resident.h) with no device: tests/test_forest_resident_cpu.py
// writes emitted node lists and the chunks of their levels, this program prints the plan resident_plan makes of them, and the
// test compares it with its own restatement.  Built once plainly and once with ASan and UBSan.  Input (whitespace-separated):
//   plan stride first_row desc_base M n_chunks n_nodes
//   n_chunks x "host_off n"            the levels' records, in launch order
//   n_nodes  x "kind has_normal offset count"
// Output per plan: "bad", or "row chunk index row" per plane in view order and "ids lo hi n_desc n_ids n_none"; "done" at the end.
#include "../arroy_amd/csrc/forest_resident.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>

using namespace ah;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string cmd;
    while (in >> cmd) {
        if (cmd != "plan") return 3;
        uint64_t stride, first_row, desc_base, M, n_chunks, n_nodes;
        in >> stride >> first_row >> desc_base >> M >> n_chunks >> n_nodes;
        std::vector<ResidentChunk> chunks(n_chunks);
        for (ResidentChunk &c : chunks) in >> c.host_off >> c.n;
        // (an array of exactly n_nodes: a read past the list is a read past the allocation)
        std::unique_ptr<ah_node[]> nodes(new ah_node[n_nodes ? n_nodes : 1]());
        for (uint64_t i = 0; i < n_nodes; i++) {
            unsigned kind, has_normal;
            uint64_t offset, count;
            in >> kind >> has_normal >> offset >> count;
            nodes[i].kind = (uint8_t)kind;
            nodes[i].has_normal = (uint8_t)has_normal;
            nodes[i].offset = offset;
            nodes[i].count = (uint32_t)count;
        }
        if (!in) return 4;
        ResidentPlan plan;
        if (!resident_plan(nodes.get(), (size_t)n_nodes, chunks, stride, (uint32_t)first_row, desc_base, M, &plan)) {
            printf("bad\n");
            continue;
        }
        for (const ResidentRow &r : plan.rows) printf("row %u %u %u\n", r.chunk, r.index, r.row);
        printf("ids %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", plan.ids_lo, plan.ids_hi, plan.n_desc, plan.n_ids, plan.n_none);
    }
    printf("done\n");
    return 0;
}
