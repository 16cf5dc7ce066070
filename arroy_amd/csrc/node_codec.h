// The bytes LMDB stores for a tree node (`NodeCodec`, src/node.rs:229-241), stated once for the host and the device.
//
//   split node    [2][left u32 BE][right u32 BE] and, when the node has a normal, [D::Header][vector bytes]
//   Descendants   [1] + the portable Roaring serialisation without run containers:
//                 u32 LE cookie 12346, u32 LE container count nc, nc x (u16 key = id >> 16, u16 cardinality - 1),
//                 nc x u32 byte offset of the container's body from the start of the serialisation, then per container in
//                 key order the sorted low 16 bits as u16 LE (cardinality <= 4096) or an 8192-byte bitmap (bit v & 7 of
//                 byte v >> 3).  An empty list is cookie + 0.
//
// No HIP call, no allocation, no library state: tests/node_codec_check.cpp includes this file in a plain host program.
// The serial functions here are the reference the kernels of encode.hip are tested against; the kernels share the
// constants, the size formulas and the byte helpers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AH_CODEC_FN __host__ __device__ inline
#else
#define AH_CODEC_FN inline
#endif

namespace ah {
namespace codec {

constexpr uint8_t kTagDescendants = 1, kTagSplit = 2;
constexpr uint32_t kRoaringCookie = 12346;  // SERIAL_COOKIE_NO_RUNCONTAINER
constexpr uint32_t kArrayMax = 4096;        // cardinality up to which a container is a sorted u16 array
constexpr uint32_t kBitmapBytes = 8192;
constexpr uint32_t kSplitHead = 9;          // tag + two child ids

AH_CODEC_FN void put_le16(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
AH_CODEC_FN void put_le32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}
AH_CODEC_FN void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// ---- sizes ---------------------------------------------------------------------------------------------------------
AH_CODEC_FN uint64_t split_value_len(bool has_normal, uint64_t header_size, uint64_t vector_size) {
    return kSplitHead + (has_normal ? header_size + vector_size : 0);
}
AH_CODEC_FN uint64_t container_body_len(uint64_t cardinality) {
    return cardinality <= kArrayMax ? 2 * cardinality : kBitmapBytes;
}
// tag + cookie + count + (key, cardinality) pairs + offsets + bodies
AH_CODEC_FN uint64_t descendants_value_len(uint64_t n_containers, uint64_t body_bytes) {
    return 1 + 8 + 8 * n_containers + body_bytes;
}
// what a list of `count` ids can need at most: every container costs 8 bytes of tables and at most 2 bytes per id (an
// array) or 8192 bytes for more than 4096 ids (a bitmap)
AH_CODEC_FN uint64_t descendants_value_bound(uint64_t count) { return 9 + 10 * count; }

// byte j of a split value whose normal record has its header at `hdr` and its vector at `vec` (j < split_value_len)
AH_CODEC_FN uint8_t split_value_byte(uint64_t j, uint32_t left, uint32_t right, const uint8_t *hdr, uint64_t header_size,
                                     const uint8_t *vec) {
    if (j == 0) return kTagSplit;
    if (j < 5) return (uint8_t)(left >> (8 * (4 - j)));
    if (j < 9) return (uint8_t)(right >> (8 * (8 - j)));
    j -= kSplitHead;
    return j < header_size ? hdr[j] : vec[j - header_size];
}

// ---- serial encoders (host reference; `out` has room for the length the matching size function returns) ---------------
// hdr == nullptr: `normal: None`
AH_CODEC_FN uint64_t encode_split(uint8_t *out, uint32_t left, uint32_t right, const uint8_t *hdr, uint64_t header_size,
                                  const uint8_t *vec, uint64_t vector_size) {
    const uint64_t len = split_value_len(hdr != nullptr, header_size, vector_size);
    for (uint64_t j = 0; j < len; j++) out[j] = split_value_byte(j, left, right, hdr, header_size, vec);
    return len;
}

// container count and value length of ids[0, n); false when the ids do not ascend strictly
AH_CODEC_FN bool measure_descendants(const uint32_t *ids, uint64_t n, uint32_t *out_containers, uint64_t *out_len) {
    uint64_t nc = 0, body = 0, first = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n; i++) {
        if (i && ids[i] <= ids[i - 1]) ok = false;
        if (i == 0 || (ids[i] >> 16) != (ids[i - 1] >> 16)) {
            if (i) body += container_body_len(i - first);
            first = i;
            nc++;
        }
    }
    if (n) body += container_body_len(n - first);
    *out_containers = (uint32_t)nc;
    *out_len = descendants_value_len(nc, body);
    return ok;
}

// ids ascend strictly; returns the bytes written (= measure_descendants' length)
AH_CODEC_FN uint64_t encode_descendants(uint8_t *out, const uint32_t *ids, uint64_t n) {
    uint32_t nc = 0;
    uint64_t len = 0;
    (void)measure_descendants(ids, n, &nc, &len);
    out[0] = kTagDescendants;
    uint8_t *v = out + 1;  // offsets count from here
    put_le32(v, kRoaringCookie);
    put_le32(v + 4, nc);
    uint64_t at = 8 + 8 * (uint64_t)nc, i = 0;
    for (uint32_t c = 0; i < n; c++) {
        uint64_t j = i;
        while (j < n && (ids[j] >> 16) == (ids[i] >> 16)) j++;
        const uint64_t card = j - i;
        put_le16(v + 8 + 4 * (uint64_t)c, ids[i] >> 16);
        put_le16(v + 8 + 4 * (uint64_t)c + 2, (uint32_t)(card - 1));
        put_le32(v + 8 + 4 * (uint64_t)nc + 4 * (uint64_t)c, (uint32_t)at);
        if (card <= kArrayMax) {
            for (uint64_t k = 0; k < card; k++) put_le16(v + at + 2 * k, ids[i + k] & 0xFFFFu);
        } else {
            for (uint32_t k = 0; k < kBitmapBytes; k++) v[at + k] = 0;
            for (uint64_t k = 0; k < card; k++) {
                const uint32_t low = ids[i + k] & 0xFFFFu;
                v[at + (low >> 3)] |= (uint8_t)(1u << (low & 7u));
            }
        }
        at += container_body_len(card);
        i = j;
    }
    return 1 + at;
}

}  // namespace codec
}  // namespace ah
