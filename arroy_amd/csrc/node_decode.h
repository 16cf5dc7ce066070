// The bytes LMDB stores for a tree node (`NodeCodec`, node_codec.h) read back: the inverse of the encoders there, stated once
// for the host and the device.
//
//   split node    9 bytes (`normal: None`) or 9 + header_size + vector_size: [2][left u32 BE][right u32 BE][D::Header][vector]
//   Descendants   [1] + what `RoaringBitmap::deserialize_from` accepts — the portable serialisation of roaring_parse.h in
//                 both cookie forms, run containers included (node_codec.h writes the 12346 form only)
//
// No HIP call, no allocation, no library state: tests/node_decode_check.cpp includes this file in a plain host program.
// Every byte is read byte-wise, so a value may start at any address.  The serial functions here are the reference the kernels
// of index_decode.hip are tested against; the kernels share the header reader, the container reader and the reason codes.
// The rules and their order are those of roaring::parse (roaring_parse.h), whose constants are used, not restated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "node_codec.h"
#include "roaring_parse.h"

namespace ah {
namespace decode {

// Why a value, or a forest of values, is refused.  The smallest (node position, reason) of a call is the one reported.
enum Reason : uint32_t {
    R_OK = 0,
    R_EMPTY,         // a value of no bytes
    R_TAG,           // neither a split node nor a Descendants node (an item's tag 0 included)
    R_SPLIT_LEN,     // a split value that is neither 9 bytes nor 9 + header + vector
    R_SHORT,         // shorter than the headers of its containers
    R_COOKIE,
    R_KEY_ORDER,
    R_PAST_END,      // a container that runs past the value
    R_OFFSET,        // an offset entry that disagrees with the sizes
    R_TRAILING,      // bytes behind the last container
    R_TOO_MANY_IDS,  // more ids than a 32-bit count holds
    // the content of the containers, in the order of RoaringReason (filter.hip)
    R_ARRAY_ORDER,
    R_BITMAP_CARDINALITY,
    R_RUN_ORDER,
    R_RUN_PAST_END,
    R_RUN_CARDINALITY,
    // the links between the values
    R_CHILD_ABSENT,
    R_ROOT_ABSENT,
    R_COUNT
};

inline const char *reason_text(uint32_t r) {
    static const char *const kWhy[R_COUNT] = {
        "",
        "the value is empty",
        "unknown node tag (1: Descendants, 2: split node)",
        "a split value is 9 bytes or 9 + header + vector bytes long",
        "the value is shorter than the headers of its containers",
        "unknown Roaring cookie (12346, or 12347 in the low 16 bits)",
        "the container keys must ascend strictly",
        "a container runs past the end of the value",
        "an offset entry disagrees with the container sizes",
        "bytes behind the last container",
        "more ids than a 32-bit count holds",
        "an array container does not ascend strictly",
        "a bitmap container's popcount is not its cardinality",
        "the runs of a container overlap or are out of order",
        "a run reaches past 65535",
        "the runs' total length is not the cardinality",
        "a child id is not among node_ids",
        "a root id is not among node_ids",
    };
    return r < R_COUNT ? kWhy[r] : "malformed";
}

AH_CODEC_FN uint32_t get_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
AH_CODEC_FN uint32_t get_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
AH_CODEC_FN uint32_t get_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

// ---- the headers of a serialisation `ser[0, slen)` (a Descendants value without its tag) ------------------------------------
struct Header {
    uint64_t nc;          // containers
    uint64_t pairs_at;    // nc x (u16 key, u16 cardinality - 1)
    uint64_t flags_at;    // the run flags; 0: the 12346 form, which has none
    uint64_t offsets_at;  // nc x u32; 0: the 12347 form below kNoOffsetThreshold containers, which has none
    uint64_t headers;     // where the first container begins
};
AH_CODEC_FN uint32_t read_header(const uint8_t *ser, uint64_t slen, Header *h) {
    if (slen < 4) return R_SHORT;
    const uint32_t cookie = get_le32(ser);
    uint64_t at;
    h->flags_at = 0;
    if (cookie == roaring::kCookieNoRuns) {
        if (slen < 8) return R_SHORT;
        h->nc = get_le32(ser + 4);
        at = 8;
    } else if ((cookie & 0xFFFFu) == roaring::kCookieRuns) {
        h->nc = (uint64_t)(cookie >> 16) + 1;
        h->flags_at = 4;
        at = 4 + (h->nc + 7) / 8;
    } else {
        return R_COOKIE;
    }
    const bool has_offsets = !h->flags_at || h->nc >= roaring::kNoOffsetThreshold;
    h->pairs_at = at;
    h->offsets_at = has_offsets ? at + 4 * h->nc : 0;
    h->headers = at + 4 * h->nc + (has_offsets ? 4 * h->nc : 0);
    return h->headers > slen ? (uint32_t)R_SHORT : (uint32_t)R_OK;  // (from here nc <= slen / 4)
}

struct ContainerAt {
    uint32_t key;          // id >> 16
    uint32_t kind;         // roaring::Kind
    uint32_t cardinality;  // 1 .. 65536, as the header states it
    uint32_t n_runs;       // KIND_RUN: the runs behind the payload's first u16, else 0
    uint64_t offset;       // of the payload in the serialisation; KIND_RUN: of its n_runs word
    uint64_t bytes;        // KIND_RUN: 2 + 4 n_runs
};
AH_CODEC_FN bool is_run(const uint8_t *ser, const Header &h, uint64_t c) { return h.flags_at && ((ser[h.flags_at + (c >> 3)] >> (c & 7)) & 1u); }
// container c < h.nc, which begins at byte `pos`: R_OK and *out, or R_PAST_END
AH_CODEC_FN uint32_t container_at(const uint8_t *ser, uint64_t slen, const Header &h, uint64_t c, uint64_t pos, ContainerAt *out) {
    out->key = get_le16(ser + h.pairs_at + 4 * c);
    out->cardinality = get_le16(ser + h.pairs_at + 4 * c + 2) + 1;
    out->offset = pos;
    out->n_runs = 0;
    out->bytes = 0;
    if (is_run(ser, h, c)) {
        out->kind = roaring::KIND_RUN;
        if (pos + 2 > slen) return R_PAST_END;
        out->n_runs = get_le16(ser + pos);
        out->bytes = 2 + 4 * (uint64_t)out->n_runs;
    } else if (out->cardinality <= roaring::kArrayMax) {
        out->kind = roaring::KIND_ARRAY;
        out->bytes = 2 * (uint64_t)out->cardinality;
    } else {
        out->kind = roaring::KIND_BITMAP;
        out->bytes = roaring::kBitmapBytes;
    }
    return pos + out->bytes > slen ? (uint32_t)R_PAST_END : (uint32_t)R_OK;
}
// Container c of a serialisation whose headers measure_value has accepted: through the offset header where there is one,
// through the (at most three) containers in front of it otherwise.
AH_CODEC_FN void locate_container(const uint8_t *ser, uint64_t slen, const Header &h, uint64_t c, ContainerAt *out) {
    uint64_t pos = h.headers;
    if (h.offsets_at) {
        pos = get_le32(ser + h.offsets_at + 4 * c);
    } else {
        for (uint64_t i = 0; i < c; i++) {
            (void)container_at(ser, slen, h, i, pos, out);
            pos += out->bytes;
        }
    }
    (void)container_at(ser, slen, h, c, pos, out);
}

// ---- one value ---------------------------------------------------------------------------------------------------------------
struct Measured {
    uint32_t kind;        // codec::kTagSplit | codec::kTagDescendants (= AH_NODE_*); 0 when refused before the tag was known
    uint32_t has_normal;  // split
    uint32_t left, right;  // split: the children's node ids
    uint64_t ids;          // Descendants: the sum of the header's cardinalities
    uint32_t containers;
    uint32_t arrays, bitmaps, runs;  // ... by kind
    uint32_t reason;                 // R_OK, or why the value is refused (the other members then mean nothing)
};
// The checks of a serialisation come in the order of roaring::parse: shorter than its headers, an unknown cookie, keys that
// do not ascend strictly, a container past the end, an offset entry that disagrees, bytes behind the last container.
AH_CODEC_FN Measured measure_value(const uint8_t *bytes, uint64_t len, uint64_t header_size, uint64_t vector_size) {
    Measured m{};
    auto refuse = [&](uint32_t r) {
        m.reason = r;
        return m;
    };
    if (len < 1) return refuse(R_EMPTY);
    if (bytes[0] == codec::kTagSplit) {
        m.kind = codec::kTagSplit;
        if (len != codec::split_value_len(false, header_size, vector_size) && len != codec::split_value_len(true, header_size, vector_size))
            return refuse(R_SPLIT_LEN);
        m.has_normal = len != codec::kSplitHead;
        m.left = get_be32(bytes + 1);
        m.right = get_be32(bytes + 5);
        return m;
    }
    if (bytes[0] != codec::kTagDescendants) return refuse(R_TAG);
    m.kind = codec::kTagDescendants;
    const uint8_t *ser = bytes + 1;
    const uint64_t slen = len - 1;
    Header h;
    if (const uint32_t r = read_header(ser, slen, &h)) return refuse(r);
    for (uint64_t c = 1; c < h.nc; c++)
        if (get_le16(ser + h.pairs_at + 4 * c) <= get_le16(ser + h.pairs_at + 4 * (c - 1))) return refuse(R_KEY_ORDER);
    uint64_t pos = h.headers;
    for (uint64_t c = 0; c < h.nc; c++) {
        ContainerAt k;
        if (const uint32_t r = container_at(ser, slen, h, c, pos, &k)) return refuse(r);
        (k.kind == roaring::KIND_ARRAY ? m.arrays : k.kind == roaring::KIND_BITMAP ? m.bitmaps : m.runs)++;
        m.ids += k.cardinality;
        pos += k.bytes;
    }
    if (h.offsets_at) {
        uint64_t at = h.headers;
        for (uint64_t c = 0; c < h.nc; c++) {
            ContainerAt k;
            (void)container_at(ser, slen, h, c, at, &k);
            if (get_le32(ser + h.offsets_at + 4 * c) != at) return refuse(R_OFFSET);
            at += k.bytes;
        }
    }
    if (pos != slen) return refuse(R_TRAILING);
    if (m.ids > 0xFFFFFFFFull) return refuse(R_TOO_MANY_IDS);
    m.containers = (uint32_t)h.nc;
    return m;
}

// The ids of a Descendants value measure_value has accepted, into out_ids[0, ids): R_OK, or the first content rule a
// container breaks.  Nothing is written past out_ids + ids, whatever the payloads hold.
AH_CODEC_FN uint32_t decode_descendants(const uint8_t *bytes, uint64_t len, uint32_t *out_ids) {
    const uint8_t *ser = bytes + 1;
    const uint64_t slen = len - 1;
    Header h;
    if (const uint32_t r = read_header(ser, slen, &h)) return r;
    uint64_t pos = h.headers, at = 0;
    for (uint64_t c = 0; c < h.nc; c++) {
        ContainerAt k;
        if (const uint32_t r = container_at(ser, slen, h, c, pos, &k)) return r;
        const uint8_t *p = ser + pos;
        const uint32_t high = k.key << 16;
        uint32_t n = 0;
        if (k.kind == roaring::KIND_ARRAY) {
            for (; n < k.cardinality; n++) {
                const uint32_t v = get_le16(p + 2 * (uint64_t)n);
                if (n && v <= get_le16(p + 2 * (uint64_t)(n - 1))) return R_ARRAY_ORDER;
                out_ids[at + n] = high | v;
            }
        } else if (k.kind == roaring::KIND_BITMAP) {
            for (uint32_t v = 0; v < 65536; v++)
                if ((p[v >> 3] >> (v & 7)) & 1u) {
                    if (n == k.cardinality) return R_BITMAP_CARDINALITY;
                    out_ids[at + n++] = high | v;
                }
            if (n != k.cardinality) return R_BITMAP_CARDINALITY;
        } else {
            uint32_t prev_end = 0;
            for (uint32_t r = 0; r < k.n_runs; r++) {
                const uint32_t start = get_le16(p + 2 + 4 * (uint64_t)r), end = start + get_le16(p + 4 + 4 * (uint64_t)r);  // inclusive
                if (end > 0xFFFFu) return R_RUN_PAST_END;
                if (r && start <= prev_end) return R_RUN_ORDER;
                for (uint32_t v = start; v <= end; v++) {
                    if (n == k.cardinality) return R_RUN_CARDINALITY;
                    out_ids[at + n++] = high | v;
                }
                prev_end = end;
            }
            if (n != k.cardinality) return R_RUN_CARDINALITY;
        }
        at += k.cardinality;
        pos += k.bytes;
    }
    return R_OK;
}

}  // namespace decode
}  // namespace ah
