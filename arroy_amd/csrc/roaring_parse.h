// The headers of one serialized RoaringBitmap (the portable serialisation, little-endian), read on the host: which containers
// the blob holds and where their payloads lie.  No HIP, no allocation beyond the descriptor vector, O(containers) — never a
// walk over ids.  Every byte is read through memcpy, so a blob may start at any address.  ah_filter_create_roaring_batch
// (filter.hip) parses with this and expands the payloads on the device (k_roaring_expand), which checks their content;
// tests/roaring_parse_check.cpp runs it under AddressSanitizer / UBSan over prefixes and mutations of a valid corpus.
//
//   u32 cookie   12346: no run containers; then u32 nc
//                low 16 bits 12347: nc = (cookie >> 16) + 1; then ceil(nc / 8) bytes of run flags (bit i & 7 of byte i >> 3)
//   nc x (u16 key, u16 cardinality - 1), keys strictly ascending
//   nc x u32 byte offset of the container from the start of the blob — always with 12346, with 12347 only when nc >= 4
//   the containers in key order, back to back:
//     run      u16 n_runs, n_runs x (u16 start, u16 length - 1)
//     array    cardinality <= 4096: `cardinality` ascending u16
//     bitmap   otherwise: 8192 bytes, bit v & 63 of 64-bit word v >> 6
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace ah {
namespace roaring {

constexpr uint32_t kCookieNoRuns = 12346, kCookieRuns = 12347;
constexpr uint32_t kNoOffsetThreshold = 4;  // with kCookieRuns the offset header exists from this many containers on
constexpr uint32_t kArrayMax = 4096, kBitmapBytes = 8192;

enum Kind : uint32_t { KIND_ARRAY = 0, KIND_BITMAP = 1, KIND_RUN = 2 };

struct Container {
    uint32_t key;          // id >> 16
    uint32_t kind;         // Kind
    uint32_t cardinality;  // 1 .. 65536, as the header states it (the device checks the payload against it)
    uint32_t n_runs;       // KIND_RUN: the runs of the payload (read from its first two bytes), else 0
    uint64_t offset;       // of the payload from the start of the blob; KIND_RUN: of its n_runs word
    uint64_t bytes;        // KIND_RUN: 2 + 4 n_runs, the n_runs word included
};

inline uint32_t load_u16(const uint8_t *p) {
    uint16_t v;
    memcpy(&v, p, 2);
    return v;  // (little-endian hosts only, like every other layout of the library)
}
inline uint32_t load_u32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// The containers of blob[0 .. len) into `out` (cleared first) and the bitmap's cardinality into *cardinality.  Returns true,
// or false with the reason in err (the container named where there is one); `out` is then meaningless.  The checks come in
// this order: a blob shorter than its headers, an unknown cookie, keys that do not ascend strictly, a container that runs
// past len, an offset entry that disagrees with the sizes, len that is not the end of the last container.
inline bool parse(const uint8_t *blob, size_t len, std::vector<Container> &out, uint64_t *cardinality, char *err, size_t err_cap) {
    out.clear();
    if (cardinality) *cardinality = 0;
    auto fail = [&](const char *fmt, auto... a) {
        if (err && err_cap) snprintf(err, err_cap, fmt, a...);
        return false;
    };
    if (len < 4) return fail("%zu bytes are shorter than a cookie", len);
    const uint32_t cookie = load_u32(blob);
    uint64_t nc, at;
    const uint8_t *flags = nullptr;
    if (cookie == kCookieNoRuns) {
        if (len < 8) return fail("%zu bytes are shorter than the headers (8 bytes)", len);
        nc = load_u32(blob + 4);
        at = 8;
    } else if ((cookie & 0xFFFFu) == kCookieRuns) {
        nc = (uint64_t)(cookie >> 16) + 1;
        flags = blob + 4;
        at = 4 + (nc + 7) / 8;
    } else {
        return fail("unknown cookie %u (12346, or 12347 in the low 16 bits)", cookie);
    }
    const bool has_offsets = !flags || nc >= kNoOffsetThreshold;
    const uint64_t pairs_at = at, offsets_at = at + 4 * nc, headers = offsets_at + (has_offsets ? 4 * nc : 0);
    if (headers > len) return fail("%zu bytes are shorter than the headers of %llu containers (%llu bytes)", len, (unsigned long long)nc, (unsigned long long)headers);
    // (from here nc <= len / 4)
    for (uint64_t i = 1; i < nc; i++) {
        const uint32_t prev = load_u16(blob + pairs_at + 4 * (i - 1)), key = load_u16(blob + pairs_at + 4 * i);
        if (key <= prev) return fail("container %llu: key %u after key %u: the keys must ascend strictly", (unsigned long long)i, key, prev);
    }
    out.reserve((size_t)nc);
    uint64_t pos = headers, total = 0;
    for (uint64_t i = 0; i < nc; i++) {
        Container c{};
        c.key = load_u16(blob + pairs_at + 4 * i);
        c.cardinality = load_u16(blob + pairs_at + 4 * i + 2) + 1;
        c.offset = pos;
        if (flags && ((flags[i >> 3] >> (i & 7)) & 1u)) {
            c.kind = KIND_RUN;
            if (pos + 2 > len) return fail("container %llu: its run count at byte %llu lies past the %zu bytes", (unsigned long long)i, (unsigned long long)pos, len);
            c.n_runs = load_u16(blob + pos);
            c.bytes = 2 + 4 * (uint64_t)c.n_runs;
        } else if (c.cardinality <= kArrayMax) {
            c.kind = KIND_ARRAY;
            c.bytes = 2 * (uint64_t)c.cardinality;
        } else {
            c.kind = KIND_BITMAP;
            c.bytes = kBitmapBytes;
        }
        if (pos + c.bytes > len)
            return fail("container %llu: bytes %llu .. %llu run past the %zu bytes", (unsigned long long)i, (unsigned long long)pos, (unsigned long long)(pos + c.bytes), len);
        pos += c.bytes;
        total += c.cardinality;
        out.push_back(c);
    }
    if (has_offsets)
        for (uint64_t i = 0; i < nc; i++) {
            const uint32_t stated = load_u32(blob + offsets_at + 4 * i);
            if (stated != out[(size_t)i].offset)
                return fail("container %llu: offset entry %u, but the sizes put it at byte %llu", (unsigned long long)i, stated, (unsigned long long)out[(size_t)i].offset);
        }
    if (pos != len) return fail("%zu bytes, but the containers end at byte %llu", len, (unsigned long long)pos);
    if (cardinality) *cardinality = total;
    return true;
}

}  // namespace roaring
}  // namespace ah
