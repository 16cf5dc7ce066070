// forest_resident.h — the host side of a resident forest (forest.hip, "the device copy"): from the node list a batch has
// emitted and the places its levels' normal records have on the device, which record becomes which row of the forest's device
// rows, and where the batch's item ids lie in the forest's device ids.  The rows are the ones ah_index_create_from_view would
// make of the forest's own view: row r belongs to the r-th split node with a plane in view order, the ids lie in view order at
// the view's offsets.  Plain C++ with no device call, so that tests/forest_resident_check.cpp can drive it on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/arroy_hip.h"

namespace ah {

// The normal records of one level (or of one level of a tail group) of the batch: `n` records of the build's record stride,
// which the view names by the byte offsets [host_off, host_off + n x stride).  Chunks are kept in launch order, which is
// ascending in host_off; `chunk` of a ResidentRow indexes this list (the caller keeps the device address next to it).
struct ResidentChunk {
    uint64_t host_off;
    uint64_t n;
};
// one row of the device copy: record `index` of chunk `chunk` becomes row `row`
struct ResidentRow {
    uint32_t chunk, index, row;
};
struct ResidentPlan {
    std::vector<ResidentRow> rows;  // in view order: rows[i].row = first_row + i
    uint64_t ids_lo = 0, ids_hi = 0;  // the Descendants nodes' ids cover [ids_lo, ids_hi) of the view's blob (0, 0: no node holds one)
    uint64_t n_desc = 0, n_ids = 0;   // Descendants nodes, and the ids they hold
    uint64_t n_none = 0;              // split nodes without a plane (`normal: None`): no row
};

// The plan of the nodes [0, n_nodes) of `nodes` — the part of the forest's node list one batch emitted.  first_row: rows the
// forest holds already.  [desc_base, desc_base + M): where the batch's permutation lies in the view's blob.  false (plan
// unspecified): a plane names no record of the chunks, an id list leaves the batch's range, or the rows pass 2^32 - 1 — the
// node list is not the one this batch emitted, and the caller gives up the device copy rather than write anywhere.
inline bool resident_plan(const ah_node *nodes, size_t n_nodes, const std::vector<ResidentChunk> &chunks, uint64_t stride,
                          uint32_t first_row, uint64_t desc_base, uint64_t M, ResidentPlan *out) {
    ResidentPlan p;
    if (stride == 0) return false;
    bool any = false;
    for (size_t i = 0; i < n_nodes; i++) {
        const ah_node &nd = nodes[i];
        if (nd.kind == AH_NODE_SPLIT) {
            if (!nd.has_normal) {
                p.n_none++;
                continue;
            }
            // the last chunk that starts at or below the record
            size_t lo = 0, hi = chunks.size();
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (chunks[mid].host_off <= nd.offset) lo = mid + 1;
                else hi = mid;
            }
            if (lo == 0) return false;
            const ResidentChunk &c = chunks[lo - 1];
            const uint64_t rel = nd.offset - c.host_off;
            if (rel % stride != 0 || rel / stride >= c.n) return false;
            if ((uint64_t)first_row + p.rows.size() >= 0xFFFFFFFFull) return false;
            p.rows.push_back(ResidentRow{(uint32_t)(lo - 1), (uint32_t)(rel / stride), first_row + (uint32_t)p.rows.size()});
        } else if (nd.kind == AH_NODE_DESCENDANTS) {
            if (nd.offset < desc_base || nd.offset + nd.count > desc_base + M) return false;
            p.n_desc++;
            p.n_ids += nd.count;
            if (nd.count) {
                p.ids_lo = any ? std::min<uint64_t>(p.ids_lo, nd.offset) : nd.offset;
                p.ids_hi = any ? std::max<uint64_t>(p.ids_hi, nd.offset + nd.count) : nd.offset + nd.count;
                any = true;
            }
        } else {
            return false;
        }
    }
    if (p.n_ids > M) return false;
    *out = std::move(p);
    return true;
}

}  // namespace ah
