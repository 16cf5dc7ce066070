// The host leg of scripts/measure_index_open.py: what a `Reader::open` does today before ah_index_create_from_view — every
// tree node decoded on ONE host thread with the serial functions of arroy_amd/csrc/node_decode.h, the children renumbered to
// ranks, the Descendants ids concatenated and the split planes copied into the arrays of an ah_forest_view.  Built by the
// script into a shared object of its own (no device call, no libarroy_hip.so).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../arroy_amd/csrc/node_decode.h"
#include "../include/arroy_hip.h"

namespace decode = ah::decode;

extern "C" {

struct HostView {
    ah_node *nodes;
    uint32_t *roots, *descendants;
    uint8_t *normals;
    uint64_t n_nodes, descendants_len, normals_len, normal_stride;
    uint32_t n_trees, bad_reason;
    uint64_t bad_position;
};

__attribute__((visibility("default"))) void host_view_free(HostView *v) {
    free(v->nodes), free(v->roots), free(v->descendants), free(v->normals);
    memset(v, 0, sizeof *v);
}

// 0, or 1 with bad_position / bad_reason (decode::Reason) set and nothing allocated
__attribute__((visibility("default"))) int host_view_decode(const uint32_t *node_ids, const uint8_t *const *values, const size_t *lens, size_t n,
                                                            const uint32_t *root_ids, uint32_t n_trees, uint64_t header_size, uint64_t vector_size,
                                                            HostView *out) {
    memset(out, 0, sizeof *out);
    auto fail = [&](uint64_t at, uint32_t reason) {
        host_view_free(out);
        out->bad_position = at, out->bad_reason = reason;
        return 1;
    };
    auto rank_of = [&](uint32_t id) -> uint32_t {
        const uint32_t *p = std::lower_bound(node_ids, node_ids + n, id);
        return p != node_ids + n && *p == id ? (uint32_t)(p - node_ids) : 0xFFFFFFFFu;
    };
    // pass 1: the sizes
    uint64_t ids = 0, normals = 0;
    for (size_t i = 0; i < n; i++) {
        const decode::Measured m = decode::measure_value(values[i], lens[i], header_size, vector_size);
        if (m.reason) return fail(i, m.reason);
        ids += m.ids, normals += m.has_normal;
    }
    out->n_nodes = n, out->n_trees = n_trees, out->descendants_len = ids;
    out->normal_stride = header_size + vector_size, out->normals_len = normals * out->normal_stride;
    out->nodes = (ah_node *)calloc(std::max<size_t>(1, n), sizeof(ah_node));
    out->roots = (uint32_t *)malloc(std::max<size_t>(1, n_trees) * 4);
    out->descendants = (uint32_t *)malloc(std::max<uint64_t>(1, ids) * 4);
    out->normals = (uint8_t *)malloc(std::max<uint64_t>(1, out->normals_len));
    if (!out->nodes || !out->roots || !out->descendants || !out->normals) return fail(0, 0);
    // pass 2: the arrays
    uint64_t at = 0, row = 0;
    for (size_t i = 0; i < n; i++) {
        const decode::Measured m = decode::measure_value(values[i], lens[i], header_size, vector_size);
        ah_node &nd = out->nodes[i];
        nd.kind = (uint8_t)m.kind;
        if (m.kind == ah::codec::kTagSplit) {
            nd.left = rank_of(m.left), nd.right = rank_of(m.right);
            if (nd.left == 0xFFFFFFFFu || nd.right == 0xFFFFFFFFu) return fail(i, decode::R_CHILD_ABSENT);
            if (m.has_normal) {
                nd.has_normal = 1;
                nd.offset = row * out->normal_stride;
                memcpy(out->normals + nd.offset, values[i] + ah::codec::kSplitHead, out->normal_stride);
                row++;
            }
        } else {
            nd.offset = at, nd.count = (uint32_t)m.ids;
            if (const uint32_t r = decode::decode_descendants(values[i], lens[i], out->descendants + at)) return fail(i, r);
            at += m.ids;
        }
    }
    for (uint32_t t = 0; t < n_trees; t++)
        if ((out->roots[t] = rank_of(root_ids[t])) == 0xFFFFFFFFu) return fail(t, decode::R_ROOT_ABSENT);
    return 0;
}

}  // extern "C"
