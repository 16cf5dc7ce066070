// Host check of arroy_amd/csrc/node_decode.h (its own main, no device call; built with AddressSanitizer and UBSan by
// tests/test_node_decode_cpu.py).  Reads cases, one per line:
//   V <header bytes> <vector bytes> <hex>   a value as it is
//   I <n> <id> ... <id>                     an id set: encoded by node_codec.h (cookie 12346), and serialized again in the
//                                           12347 form, a container run-encoded where that is smaller
// and prints for every value (two for an I line: the 12346 form, then the 12347 form) one line
//   <reason> <kind> <has_normal> <left> <right> <ids> <containers> <arrays> <bitmaps> <runs> <content reason> <id> ... <id>
// Every value is then fed three ways, each input in a heap allocation of exactly its length at offsets 0 to 3 from the start
// of the block (a read past the length is a heap-buffer-overflow report, a misaligned typed load one of UBSan): whole, every
// prefix, and single-byte mutations.  Each input either decodes or is refused; where it decodes the ids ascend strictly, are
// as many as the headers state (they are written into a block of exactly that many), every container is found where the
// serial walk finds it, and a 12346 value re-encodes to the same bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../arroy_amd/csrc/node_decode.h"

namespace codec = ah::codec;
namespace decode = ah::decode;
namespace roaring = ah::roaring;

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            printf("FAILED %s: ", #cond);     \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            if (++failures > 20) exit(1);     \
        }                                     \
    } while (0)

void put16(std::vector<uint8_t> &b, uint32_t v) {
    b.push_back((uint8_t)v);
    b.push_back((uint8_t)(v >> 8));
}
void put32(std::vector<uint8_t> &b, uint32_t v) {
    put16(b, v & 0xFFFF);
    put16(b, v >> 16);
}

// [1] + the 12347 serialisation of ascending distinct ids, a container run-encoded where that is smaller
std::vector<uint8_t> serialize_runs(const std::vector<uint32_t> &ids) {
    struct Body {
        uint32_t key, card;
        bool run;
        std::vector<uint8_t> bytes;
    };
    std::vector<Body> bodies;
    for (size_t a = 0; a < ids.size();) {
        size_t b = a;
        while (b < ids.size() && (ids[b] >> 16) == (ids[a] >> 16)) b++;
        Body body{ids[a] >> 16, (uint32_t)(b - a), false, {}};
        std::vector<uint8_t> run;
        uint32_t n_runs = 0;
        put16(run, 0);
        for (size_t i = a; i < b;) {
            size_t j = i;
            while (j + 1 < b && ids[j + 1] == ids[j] + 1) j++;
            put16(run, ids[i] & 0xFFFF);
            put16(run, (uint32_t)(j - i));
            n_runs++;
            i = j + 1;
        }
        run[0] = (uint8_t)n_runs, run[1] = (uint8_t)(n_runs >> 8);
        if (body.card <= roaring::kArrayMax) {
            for (size_t i = a; i < b; i++) put16(body.bytes, ids[i] & 0xFFFF);
        } else {
            body.bytes.assign(roaring::kBitmapBytes, 0);
            for (size_t i = a; i < b; i++) body.bytes[(ids[i] & 0xFFFF) >> 3] |= (uint8_t)(1u << (ids[i] & 7));
        }
        if (run.size() < body.bytes.size()) body.run = true, body.bytes = run;
        bodies.push_back(body);
        a = b;
    }
    std::vector<uint8_t> w{codec::kTagDescendants};
    const size_t nc = bodies.size();
    if (nc == 0) {
        put32(w, roaring::kCookieNoRuns);
        put32(w, 0);
        return w;
    }
    put32(w, roaring::kCookieRuns | ((uint32_t)(nc - 1) << 16));
    std::vector<uint8_t> flags((nc + 7) / 8, 0);
    for (size_t i = 0; i < nc; i++)
        if (bodies[i].run) flags[i >> 3] |= (uint8_t)(1u << (i & 7));
    w.insert(w.end(), flags.begin(), flags.end());
    for (const Body &b : bodies) put16(w, b.key), put16(w, b.card - 1);
    if (nc >= roaring::kNoOffsetThreshold) {
        uint64_t at = w.size() - 1 + 4 * nc;
        for (const Body &b : bodies) {
            put32(w, (uint32_t)at);
            at += b.bytes.size();
        }
    }
    for (const Body &b : bodies) w.insert(w.end(), b.bytes.begin(), b.bytes.end());
    return w;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct Result {
    decode::Measured m;
    uint32_t content = 0;  // decode_descendants' answer for an accepted Descendants value
    std::vector<uint32_t> ids;
};

// `len` bytes in an allocation of exactly len + shift bytes, at `shift` from its start: measured, decoded, and held against
// every rule an accepted value must satisfy
Result feed(const uint8_t *bytes, size_t len, size_t shift, uint64_t hs, uint64_t vs, const char *what) {
    uint8_t *heap = (uint8_t *)malloc(len + shift ? len + shift : 1);
    if (len) memcpy(heap + shift, bytes, len);
    const uint8_t *v = heap + shift;
    Result r;
    r.m = decode::measure_value(v, len, hs, vs);
    if (r.m.reason == decode::R_OK && r.m.kind == codec::kTagSplit) {
        CHECK(len == 9 || len == 9 + hs + vs, "%s: a split value of %zu bytes accepted", what, len);
        CHECK(r.m.has_normal == (len != 9), "%s: has_normal", what);
    }
    if (r.m.reason == decode::R_OK && r.m.kind == codec::kTagDescendants) {
        // every container where the serial walk puts it, inside the value, back to back
        decode::Header h;
        CHECK(decode::read_header(v + 1, len - 1, &h) == decode::R_OK && h.nc == r.m.containers, "%s: headers", what);
        uint64_t pos = h.headers, total = 0;
        for (uint64_t c = 0; c < h.nc; c++) {
            decode::ContainerAt walk, found;
            CHECK(decode::container_at(v + 1, len - 1, h, c, pos, &walk) == decode::R_OK, "%s: container %llu", what, (unsigned long long)c);
            decode::locate_container(v + 1, len - 1, h, c, &found);
            CHECK(found.offset == walk.offset && found.bytes == walk.bytes && found.key == walk.key && found.kind == walk.kind &&
                      found.cardinality == walk.cardinality && found.n_runs == walk.n_runs,
                  "%s: container %llu is not where the walk finds it", what, (unsigned long long)c);
            CHECK(walk.offset + walk.bytes <= len - 1 && walk.cardinality >= 1 && walk.cardinality <= 65536, "%s: container %llu", what, (unsigned long long)c);
            pos += walk.bytes, total += walk.cardinality;
        }
        CHECK(pos == len - 1 && total == r.m.ids && r.m.arrays + r.m.bitmaps + r.m.runs == r.m.containers, "%s: the containers do not add up", what);
        // the ids into a block of exactly the stated count
        uint32_t *out = (uint32_t *)malloc(r.m.ids ? r.m.ids * 4 : 1);
        r.content = decode::decode_descendants(v, len, out);
        if (r.content == decode::R_OK) {
            r.ids.assign(out, out + r.m.ids);
            for (size_t i = 1; i < r.ids.size(); i++)
                if (r.ids[i] <= r.ids[i - 1]) {
                    CHECK(false, "%s: id %zu (%u) after %u", what, i, r.ids[i], r.ids[i - 1]);
                    break;
                }
            if (decode::get_le32(v + 1) == roaring::kCookieNoRuns) {
                uint32_t nc = 0;
                uint64_t enc_len = 0;
                CHECK(codec::measure_descendants(r.ids.data(), r.ids.size(), &nc, &enc_len) && enc_len == len && nc == r.m.containers,
                      "%s: re-encodes to %llu bytes, not %zu", what, (unsigned long long)enc_len, len);
                if (enc_len == len) {
                    std::vector<uint8_t> again(len);
                    codec::encode_descendants(again.data(), r.ids.data(), r.ids.size());
                    CHECK(memcmp(again.data(), v, len) == 0, "%s: re-encodes to other bytes", what);
                }
            }
        } else {
            CHECK(r.content >= decode::R_ARRAY_ORDER && r.content <= decode::R_RUN_CARDINALITY, "%s: content reason %u", what, r.content);
        }
        free(out);
    }
    free(heap);
    return r;
}

bool same(const Result &a, const Result &b) {
    return a.m.reason == b.m.reason && a.m.kind == b.m.kind && a.m.has_normal == b.m.has_normal && a.m.left == b.m.left && a.m.right == b.m.right &&
           a.m.ids == b.m.ids && a.m.containers == b.m.containers && a.content == b.content && a.ids == b.ids;
}

size_t n_values = 0, n_prefixes = 0, n_mutations = 0, n_mutations_decoded = 0;

void exercise(const std::vector<uint8_t> &value, uint64_t hs, uint64_t vs) {
    n_values++;
    const Result whole = feed(value.data(), value.size(), 0, hs, vs, "whole");
    for (size_t shift = 1; shift <= 3; shift++) CHECK(same(whole, feed(value.data(), value.size(), shift, hs, vs, "shifted")), "the answer depends on the address");
    std::cout << whole.m.reason << ' ' << whole.m.kind << ' ' << whole.m.has_normal << ' ' << whole.m.left << ' ' << whole.m.right << ' ' << whole.m.ids
              << ' ' << whole.m.containers << ' ' << whole.m.arrays << ' ' << whole.m.bitmaps << ' ' << whole.m.runs << ' ' << whole.content;
    for (uint32_t id : whole.ids) std::cout << ' ' << id;
    std::cout << "\n";
    // every prefix (the bodies of long values are stepped through coarsely behind the headers)
    for (size_t len = 0; len < value.size(); len += (len < 300 || value.size() - len < 40) ? 1 : 61) {
        const Result r = feed(value.data(), len, len & 3, hs, vs, "prefix");
        n_prefixes++;
        if (whole.m.reason == decode::R_OK && whole.m.kind == codec::kTagDescendants && whole.m.containers)
            CHECK(r.m.reason != decode::R_OK || r.m.containers < whole.m.containers, "prefix %zu of %zu accepted with every container", len, value.size());
    }
    // single-byte mutations, mostly in the headers (where the structure is)
    if (value.empty()) return;
    const size_t head = std::min<size_t>(value.size(), 9 + 9 * (size_t)whole.m.containers + 8);
    for (int m = 0; m < 40; m++) {
        std::vector<uint8_t> b = value;
        const size_t at = (m % 4 == 3 ? rnd() % b.size() : rnd() % head);
        b[at] = m % 3 == 0 ? (uint8_t)(b[at] ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
        const Result r = feed(b.data(), b.size(), m & 3, hs, vs, "mutation");
        n_mutations++;
        n_mutations_decoded += r.m.reason == decode::R_OK && r.content == decode::R_OK;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: node_decode_check CASES\n"), 2;
    std::ifstream in(argv[1]);
    if (!in) return fprintf(stderr, "cannot open the cases\n"), 2;
    std::string text;
    size_t line = 0;
    while (std::getline(in, text)) {
        line++;
        if (text.empty() || text[0] == '#') continue;
        std::istringstream ss(text);
        std::string kind;
        ss >> kind;
        if (kind == "V") {
            uint64_t hs = 0, vs = 0;
            std::string hex;
            ss >> hs >> vs >> hex;
            if (!ss) return fprintf(stderr, "case %zu: short value case\n", line), 2;
            std::vector<uint8_t> value;
            if (hex != "-")
                for (size_t i = 0; i + 1 < hex.size(); i += 2) value.push_back((uint8_t)std::strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            exercise(value, hs, vs);
        } else if (kind == "I") {
            uint64_t n = 0;
            ss >> n;
            std::vector<uint32_t> ids(n);
            for (uint64_t i = 0; i < n; i++) ss >> ids[i];
            if (!ss) return fprintf(stderr, "case %zu: short id list\n", line), 2;
            uint32_t nc = 0;
            uint64_t len = 0;
            if (!codec::measure_descendants(ids.data(), n, &nc, &len)) return fprintf(stderr, "case %zu: ids do not ascend\n", line), 2;
            std::vector<uint8_t> value(len);
            codec::encode_descendants(value.data(), ids.data(), n);
            exercise(value, 4, 120);
            exercise(serialize_runs(ids), 4, 120);
        } else {
            return fprintf(stderr, "case %zu: unknown case kind\n", line), 2;
        }
    }
    printf("# %zu values, %zu prefixes, %zu mutations (%zu still decode)\n", n_values, n_prefixes, n_mutations, n_mutations_decoded);
    if (failures) return 1;
    printf("# every accepted value decodes inside its bytes and its count\n");
    return 0;
}
