// The host parser of serialized RoaringBitmaps (arroy_amd/csrc/roaring_parse.h) on its own, no device call: a valid corpus in
// both cookie forms, every prefix of every blob, a few thousand single-byte mutations, and every blob again at an odd address.
// Each input lies in a heap allocation of exactly its length, so a read past `len` is a heap-buffer-overflow report of
// AddressSanitizer, and a misaligned typed load one of UBSan (built with -fsanitize=address,undefined and run by
// tests/test_roaring_parse_cpu.py).  The parser must answer every input with either a
// refusal that says why, or a descriptor list whose payloads lie inside the blob, back to back, ending at its end; for the
// valid corpus the list must be the one the serializer here wrote.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../arroy_amd/csrc/roaring_parse.h"

using namespace ah::roaring;

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

struct Written {
    std::vector<uint8_t> bytes;
    std::vector<Container> containers;
    uint64_t cardinality = 0;
};

// The serialisation of ascending distinct ids; runs: cookie 12347, a container run-encoded where that is smaller.
Written serialize(const std::vector<uint32_t> &ids, bool runs) {
    struct Body {
        uint32_t key, kind, card, n_runs;
        std::vector<uint8_t> bytes;
    };
    std::vector<Body> bodies;
    for (size_t a = 0; a < ids.size();) {
        size_t b = a;
        while (b < ids.size() && (ids[b] >> 16) == (ids[a] >> 16)) b++;
        Body body{ids[a] >> 16, KIND_ARRAY, (uint32_t)(b - a), 0, {}};
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
        if (body.card <= kArrayMax) {
            for (size_t i = a; i < b; i++) put16(body.bytes, ids[i] & 0xFFFF);
        } else {
            body.kind = KIND_BITMAP;
            body.bytes.assign(kBitmapBytes, 0);
            for (size_t i = a; i < b; i++) body.bytes[(ids[i] & 0xFFFF) >> 3] |= (uint8_t)(1u << (ids[i] & 7));
        }
        if (runs && run.size() < body.bytes.size()) body.kind = KIND_RUN, body.n_runs = n_runs, body.bytes = run;
        bodies.push_back(body);
        a = b;
    }
    Written w;
    const size_t nc = bodies.size();
    bool offsets = true;
    if (!runs || nc == 0) {
        put32(w.bytes, kCookieNoRuns);
        put32(w.bytes, (uint32_t)nc);
    } else {
        put32(w.bytes, kCookieRuns | ((uint32_t)(nc - 1) << 16));
        std::vector<uint8_t> flags((nc + 7) / 8, 0);
        for (size_t i = 0; i < nc; i++)
            if (bodies[i].kind == KIND_RUN) flags[i >> 3] |= (uint8_t)(1u << (i & 7));
        w.bytes.insert(w.bytes.end(), flags.begin(), flags.end());
        offsets = nc >= kNoOffsetThreshold;
    }
    for (const Body &b : bodies) put16(w.bytes, b.key), put16(w.bytes, b.card - 1);
    uint64_t at = w.bytes.size() + (offsets ? 4 * nc : 0);
    for (const Body &b : bodies) {
        if (offsets) put32(w.bytes, (uint32_t)at);
        w.containers.push_back(Container{b.key, b.kind, b.card, b.n_runs, at, b.bytes.size()});
        w.cardinality += b.card;
        at += b.bytes.size();
    }
    for (const Body &b : bodies) w.bytes.insert(w.bytes.end(), b.bytes.begin(), b.bytes.end());
    return w;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

std::vector<std::vector<uint32_t>> corpus() {
    std::vector<std::vector<uint32_t>> sets;
    sets.push_back({});
    sets.push_back({5});
    sets.push_back({0, 31, 32, 65535});
    sets.push_back({1, 2, 3, 65541, 65542, 65543, 65544, 65545});  // the worked example of the header
    sets.push_back({70000, 0xFFFF0000u, 0xFFFFFFFFu});
    std::vector<uint32_t> s;
    for (uint32_t i = 0; i < 65536; i++) s.push_back(i);  // a full span: bitmap, or one run
    sets.push_back(s);
    s.clear();
    for (uint32_t i = 0; i < 65536; i += 2) s.push_back(65536 + i);  // 32768 runs of one: a bitmap in either form
    sets.push_back(s);
    s.clear();
    for (uint32_t i = 0; i < 4096; i++) s.push_back(3 * i);  // an array of exactly 4096
    for (uint32_t i = 0; i < 4097; i++) s.push_back(65536 + 5 * i);  // a bitmap of 4097
    sets.push_back(s);
    for (uint32_t nc : {3u, 4u, 8u, 9u, 17u}) {  // around the offset-header threshold and the flag bytes
        s.clear();
        for (uint32_t k = 0; k < nc; k++)
            for (uint32_t j = 0; j < 30 + k; j++) s.push_back((2 * k + 1) * 65536 + (k % 2 ? 7 * j : 100 + j));
        sets.push_back(s);
    }
    for (int r = 0; r < 6; r++) {  // random sets over a few spans
        s.clear();
        const uint32_t n = 1 + rnd() % 6000, range = 1u << (10 + rnd() % 10);
        for (uint32_t i = 0; i < n; i++) s.push_back(rnd() % range);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        sets.push_back(s);
    }
    return sets;
}

// parse() of `len` bytes copied into an allocation of exactly len + shift bytes, at `shift` from its start
bool parse_copy(const uint8_t *bytes, size_t len, size_t shift, std::vector<Container> &out, uint64_t *card, std::string &why) {
    uint8_t *heap = (uint8_t *)malloc(len + shift ? len + shift : 1);
    if (len) memcpy(heap + shift, bytes, len);
    char err[200] = "";
    const bool ok = parse(heap + shift, len, out, card, err, sizeof err);
    why = err;
    free(heap);
    return ok;
}

// what every accepted input must satisfy, whatever it is
void check_ranges(const std::vector<Container> &cs, size_t len, const char *what) {
    uint64_t at = 0, last_key = 0;
    for (size_t i = 0; i < cs.size(); i++) {
        const Container &c = cs[i];
        CHECK(c.offset + c.bytes <= len && c.bytes > 0, "%s: container %zu at %llu + %llu of %zu", what, i, (unsigned long long)c.offset, (unsigned long long)c.bytes, len);
        CHECK(i == 0 || (c.offset == at && c.key > last_key), "%s: container %zu is not behind its predecessor", what, i);
        CHECK(c.cardinality >= 1 && c.cardinality <= 65536 && c.key <= 0xFFFF && c.kind <= KIND_RUN, "%s: container %zu", what, i);
        CHECK(c.kind == KIND_RUN ? c.bytes == 2 + 4ull * c.n_runs : c.kind == KIND_ARRAY ? c.bytes == 2ull * c.cardinality && c.cardinality <= kArrayMax
                                                                                      : c.bytes == kBitmapBytes && c.cardinality > kArrayMax,
              "%s: container %zu has the wrong size for its kind", what, i);
        at = c.offset + c.bytes, last_key = c.key;
    }
    CHECK(cs.empty() || at == len, "%s: the containers end at %llu of %zu", what, (unsigned long long)at, len);
}

}  // namespace

int main() {
    size_t blobs = 0, prefixes = 0, mutations = 0, accepted_mutations = 0;
    for (const auto &ids : corpus())
        for (bool runs : {false, true}) {
            const Written w = serialize(ids, runs);
            blobs++;
            for (size_t shift : {0, 1, 3}) {  // the valid blob, at an even and at odd addresses
                std::vector<Container> got;
                uint64_t card = 0;
                std::string why;
                CHECK(parse_copy(w.bytes.data(), w.bytes.size(), shift, got, &card, why), "a valid blob of %zu ids was refused: %s", ids.size(), why.c_str());
                CHECK(card == ids.size() && card == w.cardinality, "cardinality %llu of %zu ids", (unsigned long long)card, ids.size());
                CHECK(got.size() == w.containers.size(), "%zu containers, wrote %zu", got.size(), w.containers.size());
                for (size_t i = 0; i < got.size() && i < w.containers.size(); i++) {
                    const Container &a = got[i], &b = w.containers[i];
                    CHECK(a.key == b.key && a.kind == b.kind && a.cardinality == b.cardinality && a.n_runs == b.n_runs && a.offset == b.offset && a.bytes == b.bytes,
                          "container %zu differs from what was written", i);
                }
                check_ranges(got, w.bytes.size(), "valid");
            }
            // every prefix: refused with a reason (a proper prefix never ends where its containers end) — the bitmap bodies are
            // stepped through coarsely behind the headers
            for (size_t len = 0; len < w.bytes.size(); len += (len < 200 || w.bytes.size() - len < 40) ? 1 : 37) {
                std::vector<Container> got;
                std::string why;
                const bool ok = parse_copy(w.bytes.data(), len, len & 1, got, nullptr, why);
                prefixes++;
                if (ok) check_ranges(got, len, "prefix");
                else CHECK(!why.empty(), "a refusal without a reason at prefix %zu", len);
                CHECK(!ok || got.size() < w.containers.size() || w.containers.empty(), "prefix %zu of %zu accepted with every container", len, w.bytes.size());
            }
            // single-byte mutations, mostly in the headers (where the structure is)
            const size_t head = std::min<size_t>(w.bytes.size(), 8 + 9 * w.containers.size() + 8);
            for (int m = 0; m < 120; m++) {
                std::vector<uint8_t> b = w.bytes;
                const size_t at = (m % 4 == 3 ? rnd() % b.size() : rnd() % head);
                const uint8_t old = b[at];
                b[at] = m % 3 == 0 ? (uint8_t)(old ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
                std::vector<Container> got;
                std::string why;
                const bool ok = parse_copy(b.data(), b.size(), m & 1, got, nullptr, why);
                mutations++;
                accepted_mutations += ok;
                if (ok) check_ranges(got, b.size(), "mutation");
                else CHECK(!why.empty(), "a refusal without a reason");
            }
        }
    printf("%zu blobs, %zu prefixes, %zu mutations (%zu still well-formed)\n", blobs, prefixes, mutations, accepted_mutations);
    if (failures) return 1;
    printf("every accepted blob has its containers inside it\n");
    return 0;
}
