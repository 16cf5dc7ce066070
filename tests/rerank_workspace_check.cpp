// The device and pinned layouts of a sub-batch of ah_rerank_batch (arroy_amd/csrc/rerank_workspace.h) on the host alone, no
// device call: for every combination of the stages and sizes from 0 to the limits of a sub-batch, the bytes a counting Carver
// reports are allocated exactly (a real heap block: a layout that outgrows it is a heap-buffer-overflow report as well), the
// same layout carves the block, the first and last byte of every array are written, and: every array starts on a 256-byte
// boundary, the arrays follow each other in the documented order without overlapping, an array the call does not use is
// null, and the bytes are no more than the sums rerank_batch_chunk kept by hand before the layouts were written down once —
// and no less than those minus the slack they carried.  Built with -fsanitize=address,undefined by
// test_rerank_workspace_cpu.py.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../arroy_amd/csrc/rerank_workspace.h"

using namespace ah;

namespace {

// the types of common.h, reduced to their sizes
struct Seg {
    uint64_t off;
    uint32_t n, k;
};
struct Tile {
    uint32_t query, first;
};
struct Float4 {
    float x, y, z, w;
};
struct Bufs {
    float *d_q_f32;
    uint8_t *d_qvecs;
    float *d_qhdrs;
    Seg *d_segs;
    Tile *d_tiles;
    uint32_t *d_ids;
    float *d_dist;
    uint64_t *d_keys_a, *d_keys_b;
    uint32_t *d_out_ids;
    float *d_out_dist;
    uint32_t *d_err, *d_inv_counters;
    uint16_t *d_q16;
    Float4 *d_qstats;
    float *d_aux;
    int8_t *d_q8;
    Float4 *d_q8stats;
    float *d_aux8;
};

// What the hand-kept sums allowed beyond the arrays, which the derived sizes drop: 4096 bytes "for drift" (the 16 status words
// lived in them), and at most one 256-byte padding for each of the seven optional arrays where it is absent.
constexpr size_t kDroppedSlack = 4096 + 7 * 256;
constexpr size_t kStatusBytes = 256;  // pad256(16 words)

// the sums of rerank_batch_chunk before this header (sizeof(HostSeg) = 16, sizeof(HostTile) = 8)
size_t old_dev_bytes(const RerankSizes &z) {
    const size_t qstride = pad256(z.row_bytes);
    const size_t screen_bytes = (z.screened ? pad256(z.nq * z.hpitch * 2) + pad256(z.nq * 16) + pad256(z.total * 4) : 0) +
                                (z.screened8 ? pad256(z.nq * z.pitch8 * 2) + pad256(z.nq * 16) + pad256(z.total * 4) : 0);
    return pad256(z.nq * z.dims * 4) + z.nq * qstride + pad256(z.nq * 8) + pad256(z.nq * 16) + pad256(z.n_tiles * 8) +
           pad256(z.total * 4) * 2 + 2 * pad256(z.nq * z.kstride * 8) + pad256(z.nq * z.k * 4) * 2 + pad256(z.inv_bytes) + screen_bytes + 4096;
}
size_t old_pin_bytes(const RerankSizes &z) {
    return pad256(z.nq * z.dims * 4) + pad256(z.nq * 16) + pad256(z.n_tiles * 8) + pad256(z.total * 4) + pad256(z.nq * z.k * 4) * 2 + 4096;
}

std::atomic<int> failures{0};
std::atomic<long> layouts{0};

struct Span {
    const char *name;
    void *p;
    size_t bytes;
    bool wanted;
};
#define SPAN(ptr, count, wanted) Span{#ptr, ptr, (size_t)(count) * sizeof(*(ptr)), wanted}

// `layout` counted, allocated exactly, carved; `spans` lists the arrays in the documented order
template <class Layout, class Spans>
void check(const char *what, const RerankSizes &z, size_t old_bytes, Layout layout, Spans spans) {
    Carver count(nullptr);
    layout(count);
    for (const Span &s : spans())
        if (s.p) fprintf(stderr, "%s: the counting pass handed out %s\n", what, s.name), failures++;
    const size_t bytes = count.off;
    if (bytes > old_bytes || bytes + kDroppedSlack < old_bytes || bytes != old_bytes - 4096 + kStatusBytes) {
        fprintf(stderr, "%s (nq %zu dims %zu k %zu total %zu tiles %zu inv %zu stages %d%d): %zu bytes, the hand-kept sum gave %zu\n", what, z.nq,
                z.dims, z.k, z.total, z.n_tiles, z.inv_bytes, z.screened, z.screened8, bytes, old_bytes);
        failures++;
    }
    unsigned char *block = static_cast<unsigned char *>(aligned_alloc(256, bytes));  // (bytes: a multiple of 256, never 0)
    Carver carve(block);
    layout(carve);
    if (carve.off != bytes) fprintf(stderr, "%s: carved %zu of %zu bytes\n", what, carve.off, bytes), failures++;
    const unsigned char *at = block;
    for (const Span &s : spans()) {
        if (!s.wanted) {
            if (s.p) fprintf(stderr, "%s: %s is not used and not null\n", what, s.name), failures++;
            continue;
        }
        unsigned char *p = static_cast<unsigned char *>(s.p);
        if (p != at || (p - block) % 256 != 0) {  // in order, without a gap beyond the padding: disjoint as well
            fprintf(stderr, "%s: %s starts at byte %td, not at %td\n", what, s.name, p - block, at - block);
            failures++;
            break;
        }
        if (s.bytes) p[0] = 1, p[s.bytes - 1] = 2;
        at = p + pad256(s.bytes);
    }
    if (at != block + bytes) fprintf(stderr, "%s: the arrays end at byte %td of %zu\n", what, at - block, bytes), failures++;
    free(block);
    layouts++;
}

void check_shape(const RerankSizes &z) {
    Bufs b{};
    check(
        "device", z, old_dev_bytes(z), [&](Carver &c) { rerank_device_layout(c, z, b); },
        [&] {
            return std::vector<Span>{SPAN(b.d_q_f32, z.nq * z.dims, true),
                                     SPAN(b.d_qvecs, z.nq * pad256(z.row_bytes), true),
                                     SPAN(b.d_qhdrs, z.nq * 2, true),
                                     SPAN(b.d_segs, z.nq, true),
                                     SPAN(b.d_tiles, z.n_tiles, true),
                                     SPAN(b.d_ids, z.total, true),
                                     SPAN(b.d_dist, z.total, true),
                                     SPAN(b.d_keys_a, z.nq * z.kstride, true),
                                     SPAN(b.d_keys_b, z.nq * z.kstride, true),
                                     SPAN(b.d_out_ids, z.nq * z.k, true),
                                     SPAN(b.d_out_dist, z.nq * z.k, true),
                                     SPAN(b.d_err, 16, true),
                                     SPAN(b.d_inv_counters, z.inv_bytes / 4, z.inv_bytes != 0),
                                     SPAN(b.d_q16, z.nq * z.hpitch, z.screened),
                                     SPAN(b.d_qstats, z.nq, z.screened),
                                     SPAN(b.d_aux, z.total, z.screened),
                                     SPAN(b.d_q8, z.nq * z.pitch8 * 2, z.screened8),
                                     SPAN(b.d_q8stats, z.nq, z.screened8),
                                     SPAN(b.d_aux8, z.total, z.screened8)};
        });
    RerankPinned<Seg, Tile> p{};
    check(
        "pinned", z, old_pin_bytes(z), [&](Carver &c) { rerank_pinned_layout(c, z, p); },
        [&] {
            return std::vector<Span>{SPAN(p.q, z.nq * z.dims, true),       SPAN(p.segs, z.nq, true),
                                     SPAN(p.tiles, z.n_tiles, true),       SPAN(p.ids, z.total, true),
                                     SPAN(p.out_ids, z.nq * z.k, true),    SPAN(p.out_dist, z.nq * z.k, true),
                                     SPAN(p.err, 16, true)};
        });
}

}  // namespace

int main() {
    static_assert(sizeof(Seg) == 16 && sizeof(Tile) == 8 && sizeof(Float4) == 16, "the sizes common.h asserts");
    constexpr size_t kTile = 512, kChunk = 4096;  // batch.hip: candidates of a tile, keys of a tournament chunk
    std::vector<RerankSizes> shapes;
    for (int stages = 0; stages < 4; stages++)
        for (size_t inv_bytes : {(size_t)0, (size_t)4 * 1000003})
            for (size_t nq : {1, 2, 1024})
                for (size_t dims : {1, 32, 1536})
                    for (size_t k : {1, 256, 2048})
                        for (size_t total : {(size_t)0, (size_t)1, nq, (size_t)64 << 20})
                            for (bool with_tiles : {false, true}) {
                                RerankSizes z{};
                                z.nq = nq, z.dims = dims, z.row_bytes = dims * 4, z.k = k, z.total = total;
                                z.n_tiles = with_tiles ? (total + kTile - 1) / kTile + nq : 0;  // (a partial tile per list at most)
                                // (keys: one chunk per list, or 16 for a few lists — not the 64 Mi keys a single list of
                                // that length has: the ids already make such a block gigabytes)
                                z.kstride = nq <= 2 ? 16 * kChunk : kChunk;
                                z.inv_bytes = inv_bytes;
                                z.hpitch = (dims + 31) / 32 * 32, z.pitch8 = (dims + 63) / 64 * 64;
                                z.screened = stages & 1, z.screened8 = stages & 2;
                                shapes.push_back(z);
                            }
    // (a block of 64 Mi candidates is gigabytes, and a sanitizer's bookkeeping for it a quarter of a second: a few threads)
    std::atomic<size_t> next{0};
    std::vector<std::thread> workers;
    for (unsigned t = 0; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++)
        workers.emplace_back([&] {
            for (size_t i = next++; i < shapes.size(); i = next++) check_shape(shapes[i]);
        });
    for (std::thread &w : workers) w.join();
    if (failures) {
        fprintf(stderr, "%d failures\n", failures.load());
        return 1;
    }
    printf("every layout inside its block (%zu shapes, %ld layouts)\n", shapes.size(), layouts.load());
    return 0;
}
