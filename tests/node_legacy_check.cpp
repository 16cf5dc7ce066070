// Host check of arroy_amd/csrc/node_legacy.h (its own main, no device call; built with AddressSanitizer and UBSan by
// tests/test_node_legacy_cpu.py).  Reads cases, one per line:
//   L <layout> <f32: 1 | 0> <vector bytes> <hex>   a value of a legacy layout (1: v0.5 / v0.6, 2: v0.4) as it is
//   Z <f32: 1 | 0> <hex>                           a stored vector alone
// and prints for an L line
//   <reason> <kind> <has_normal> <left> <right> <left is item> <right is item> <ids> <reason's text>
// and for a Z line `is_zero`, 1 or 0.  Every L value is then fed three ways, each input in a heap allocation of exactly its
// length at offsets 0 to 3 from the start of the block (a read past the length is a heap-buffer-overflow report, a misaligned
// typed load one of UBSan): whole, every prefix, and single-byte mutations.  An accepted split value has the one legal length,
// both mode bytes legal under the layout, and has_normal exactly when some element of the vector is not zero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../arroy_amd/csrc/node_legacy.h"

namespace codec = ah::codec;
namespace decode = ah::decode;
namespace legacy = ah::legacy;

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

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

std::vector<uint8_t> unhex(const std::string &hex) {
    std::vector<uint8_t> out;
    if (hex != "-")
        for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)std::strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

// is_zero, restated on typed values: an f32 element compares equal to 0.0, a byte is 0
bool plain_is_zero(const uint8_t *vec, size_t n, bool f32) {
    if (!f32) {
        for (size_t i = 0; i < n; i++)
            if (vec[i]) return false;
        return true;
    }
    for (size_t i = 0; i + 4 <= n; i += 4) {
        float x;
        memcpy(&x, vec + i, 4);
        if (!(x == 0.0f)) return false;
    }
    return true;
}

legacy::Measured feed(const uint8_t *bytes, size_t len, size_t shift, int layout, uint64_t vs, bool f32, const char *what) {
    uint8_t *heap = (uint8_t *)malloc(len + shift ? len + shift : 1);
    if (len) memcpy(heap + shift, bytes, len);
    const uint8_t *v = heap + shift;
    const legacy::Measured r = legacy::measure_value(v, len, layout, vs, f32);
    if (r.m.reason == decode::R_OK && r.m.kind == codec::kTagSplit) {
        CHECK(len == 11 + vs, "%s: a split value of %zu bytes accepted", what, len);
        const uint32_t tree = legacy::mode_tree(layout), item = legacy::mode_item(layout);
        CHECK((v[1] == tree || v[1] == item) && (v[6] == tree || v[6] == item), "%s: mode bytes %u %u accepted", what, v[1], v[6]);
        CHECK(r.left_is_item == (v[1] == item) && r.right_is_item == (v[6] == item), "%s: which child is an item", what);
        CHECK(r.m.left == decode::get_be32(v + 2) && r.m.right == decode::get_be32(v + 7), "%s: the ids", what);
        CHECK(r.m.has_normal == !plain_is_zero(v + 11, vs, f32), "%s: has_normal", what);
        CHECK(legacy::vector_is_zero(v + 11, vs, f32) == plain_is_zero(v + 11, vs, f32), "%s: is_zero", what);
    }
    if (len >= 1 && v[0] != codec::kTagSplit) {
        const decode::Measured d = decode::measure_value(v, len, 0, vs);
        CHECK(d.reason == r.m.reason && d.kind == r.m.kind && d.ids == r.m.ids, "%s: a value that is no split value is judged by node_decode.h", what);
    }
    CHECK(r.m.reason == decode::R_OK || (r.m.reason < legacy::R_COUNT && legacy::reason_text(r.m.reason)[0] != 0), "%s: reason %u", what, r.m.reason);
    free(heap);
    return r;
}

bool same(const legacy::Measured &a, const legacy::Measured &b) {
    return a.m.reason == b.m.reason && a.m.kind == b.m.kind && a.m.has_normal == b.m.has_normal && a.m.left == b.m.left && a.m.right == b.m.right &&
           a.left_is_item == b.left_is_item && a.right_is_item == b.right_is_item && a.m.ids == b.m.ids;
}

size_t n_values = 0, n_prefixes = 0, n_mutations = 0, n_mutations_accepted = 0;

void exercise(const std::vector<uint8_t> &value, int layout, uint64_t vs, bool f32) {
    n_values++;
    const legacy::Measured whole = feed(value.data(), value.size(), 0, layout, vs, f32, "whole");
    for (size_t shift = 1; shift <= 3; shift++)
        CHECK(same(whole, feed(value.data(), value.size(), shift, layout, vs, f32, "shifted")), "the answer depends on the address");
    std::cout << whole.m.reason << ' ' << whole.m.kind << ' ' << whole.m.has_normal << ' ' << whole.m.left << ' ' << whole.m.right << ' '
              << whole.left_is_item << ' ' << whole.right_is_item << ' ' << whole.m.ids << ' ' << legacy::reason_text(whole.m.reason) << "\n";
    for (size_t len = 0; len < value.size(); len++) {
        const legacy::Measured r = feed(value.data(), len, len & 3, layout, vs, f32, "prefix");
        n_prefixes++;
        if (whole.m.reason == decode::R_OK && whole.m.kind == codec::kTagSplit) CHECK(r.m.reason != decode::R_OK, "prefix %zu of a split value of %zu bytes accepted", len, value.size());
    }
    if (value.empty()) return;
    for (int m = 0; m < 60; m++) {
        std::vector<uint8_t> b = value;
        const size_t at = (m % 4 == 3 ? rnd() % b.size() : rnd() % (b.size() < 12 ? b.size() : 12));
        b[at] = m % 3 == 0 ? (uint8_t)(b[at] ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
        const legacy::Measured r = feed(b.data(), b.size(), m & 3, layout, vs, f32, "mutation");
        n_mutations++;
        n_mutations_accepted += r.m.reason == decode::R_OK;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: node_legacy_check CASES\n"), 2;
    std::ifstream in(argv[1]);
    if (!in) return fprintf(stderr, "cannot open the cases\n"), 2;
    CHECK(!legacy::layout_valid(-1) && legacy::layout_valid(0) && legacy::layout_valid(2) && !legacy::layout_valid(3), "layout_valid");
    std::string text;
    size_t line = 0;
    while (std::getline(in, text)) {
        line++;
        if (text.empty() || text[0] == '#') continue;
        std::istringstream ss(text);
        std::string kind, hex;
        ss >> kind;
        if (kind == "L") {
            int layout = 0, f32 = 0;
            uint64_t vs = 0;
            ss >> layout >> f32 >> vs >> hex;
            if (!ss || (layout != legacy::L_V0_5 && layout != legacy::L_V0_4)) return fprintf(stderr, "case %zu: bad value case\n", line), 2;
            exercise(unhex(hex), layout, vs, f32 != 0);
        } else if (kind == "Z") {
            int f32 = 0;
            ss >> f32 >> hex;
            if (!ss) return fprintf(stderr, "case %zu: bad vector case\n", line), 2;
            const std::vector<uint8_t> vec = unhex(hex);
            bool answer = false;
            for (size_t shift = 0; shift <= 3; shift++) {  // in an allocation of exactly its length, at every alignment
                uint8_t *heap = (uint8_t *)malloc(vec.size() + shift ? vec.size() + shift : 1);
                if (!vec.empty()) memcpy(heap + shift, vec.data(), vec.size());
                const bool z = legacy::vector_is_zero(heap + shift, vec.size(), f32 != 0);
                CHECK(z == plain_is_zero(heap + shift, vec.size(), f32 != 0), "case %zu: is_zero against the typed comparison", line);
                CHECK(shift == 0 || z == answer, "case %zu: is_zero depends on the address", line);
                answer = z;
                free(heap);
            }
            std::cout << (answer ? 1 : 0) << "\n";
        } else {
            return fprintf(stderr, "case %zu: unknown case kind\n", line), 2;
        }
    }
    printf("# %zu values, %zu prefixes, %zu mutations (%zu still accepted)\n", n_values, n_prefixes, n_mutations, n_mutations_accepted);
    if (failures) return 1;
    printf("# every accepted legacy value keeps the rules of its layout\n");
    return 0;
}
