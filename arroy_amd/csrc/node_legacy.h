// The bytes arroy v0.4 - v0.6 stored for a tree node (`GenericReadNodeCodecFromV0_4_0`, src/node.rs:284-319), stated once for
// the host and the device, next to node_decode.h, which reads what has not changed: Descendants values are those of v0.7.
//
//   split node    [2][left NodeId][right NodeId][vector]: 11 + vector_size bytes, no header.  A NodeId is [mode u8][item u32 BE];
//                 a child is a tree node (mode Tree) or a stored item (mode Item).  The mode bytes are Tree = 2, Item = 3 in
//                 v0.5 and v0.6 (src/node_id.rs), Item = 0, Tree = 1 in v0.4 (src/upgrade.rs:32-38)
//   normal        never absent: `normal: None` was stored as a vector `is_zero` accepts — every f32 element == 0.0, so -0.0
//                 is zero and a NaN is not (src/unaligned_vector/f32.rs:54-56), or every byte of a binary-quantized vector 0
//                 (binary_quantized.rs:71-73).  A normal that is not zero gets `D::new_header(vector)` as its header
//
// The upgrade (`from_0_6_to_current`, src/upgrade.rs:183-270) visits the split values in key order, left child before right:
// every Item child becomes a new Descendants node of that one id, numbered behind the last tree node in that order.
//
// No HIP call, no allocation, no library state: tests/node_legacy_check.cpp includes this file in a plain host program.  Every
// byte is read byte-wise, so a value may start at any address.
#pragma once
#include "node_decode.h"

namespace ah {
namespace legacy {

enum Layout : int { L_V0_7 = 0, L_V0_5 = 1, L_V0_4 = 2, L_COUNT };  // = ah_node_layout (include/arroy_hip.h)

constexpr uint32_t kNodeIdBytes = 5;
constexpr uint32_t kSplitHead = 1 + 2 * kNodeIdBytes;  // tag + two NodeIds: the vector begins here

// the reasons a legacy value is refused for, behind those of node_decode.h
enum Reason : uint32_t {
    R_LEGACY_SPLIT_LEN = decode::R_COUNT,  // a split value that is not 11 + vector bytes long
    R_CHILD_MODE,                          // a child's mode byte is neither Tree nor Item under the layout
    R_COUNT
};
inline const char *reason_text(uint32_t r) {
    if (r == R_LEGACY_SPLIT_LEN) return "a split value of the v0.4 - v0.6 layouts is 11 + vector bytes long";
    if (r == R_CHILD_MODE) return "a child's mode byte is neither Tree nor Item under the layout";
    return decode::reason_text(r);
}

AH_CODEC_FN bool layout_valid(int layout) { return layout >= L_V0_7 && layout < L_COUNT; }
AH_CODEC_FN uint32_t mode_tree(int layout) { return layout == L_V0_4 ? 1u : 2u; }
AH_CODEC_FN uint32_t mode_item(int layout) { return layout == L_V0_4 ? 0u : 3u; }
AH_CODEC_FN uint64_t split_value_len(uint64_t vector_size) { return kSplitHead + vector_size; }

// `is_zero` of a stored vector: f32 elements with the sign bit masked, the bytes of a binary-quantized vector as they are
AH_CODEC_FN bool word_is_zero(uint32_t w, bool f32) { return (w & (f32 ? 0x7FFFFFFFu : 0xFFFFFFFFu)) == 0; }
AH_CODEC_FN bool vector_is_zero(const uint8_t *vec, uint64_t vector_size, bool f32) {
    for (uint64_t at = 0; at + 4 <= vector_size; at += 4)
        if (!word_is_zero(decode::get_le32(vec + at), f32)) return false;
    for (uint64_t at = vector_size & ~(uint64_t)3; at < vector_size; at++)
        if (vec[at]) return false;
    return true;
}

struct Measured {
    decode::Measured m;      // as node_decode.h fills it; a split's left / right are the ids as stored, has_normal is set by
                             // the caller that tests the vector (measure_value below does)
    uint32_t left_is_item, right_is_item;
};
// the head of a split value `bytes[0] == 2`: length, modes, ids.  has_normal is left 0
AH_CODEC_FN Measured measure_split_head(const uint8_t *bytes, uint64_t len, int layout, uint64_t vector_size) {
    Measured r{};
    r.m.kind = codec::kTagSplit;
    if (len != split_value_len(vector_size)) {
        r.m.reason = R_LEGACY_SPLIT_LEN;
        return r;
    }
    const uint32_t lm = bytes[1], rm = bytes[1 + kNodeIdBytes];
    if ((lm != mode_tree(layout) && lm != mode_item(layout)) || (rm != mode_tree(layout) && rm != mode_item(layout))) {
        r.m.reason = R_CHILD_MODE;
        return r;
    }
    r.left_is_item = lm == mode_item(layout);
    r.right_is_item = rm == mode_item(layout);
    r.m.left = decode::get_be32(bytes + 2);
    r.m.right = decode::get_be32(bytes + 2 + kNodeIdBytes);
    return r;
}
// One value of a legacy layout (L_V0_5 / L_V0_4): a split value by the rules above, everything else by node_decode.h
AH_CODEC_FN Measured measure_value(const uint8_t *bytes, uint64_t len, int layout, uint64_t vector_size, bool f32) {
    if (len >= 1 && bytes[0] == codec::kTagSplit) {
        Measured r = measure_split_head(bytes, len, layout, vector_size);
        if (r.m.reason == decode::R_OK) r.m.has_normal = !vector_is_zero(bytes + kSplitHead, vector_size, f32);
        return r;
    }
    Measured r{};
    r.m = decode::measure_value(bytes, len, 0, vector_size);
    return r;
}

}  // namespace legacy
}  // namespace ah
